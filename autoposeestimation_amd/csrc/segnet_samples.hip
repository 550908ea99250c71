// Training samples of SegNet, built on the device from resident frames (reference DenseFusion/vanilla_segmentation/
// data_controller.py:43-93).  The reference does this in Pillow and numpy on the host, per sample: colour jitter of a real frame; for a
// `data_syn` frame brightness 1.5, a Gaussian blur, its jitter, float64 noise and a jittered real background added where its own label
// is 0; one of four flips; Normalize on the 0..255 scale.  Here a batch is two launches and no read-back (no draw depends on a pixel):
//   segnet_prepare_kernel  64 workgroups per job, each walking 32 x 32 tiles.  A `data_syn` job's tile is brightened into LDS with a halo
//                          of three pixels, goes through the six box passes between two ping-pong planes (a neighbour's index is clamped
//                          in IMAGE coordinates: the end pixel stands in for the missing one only at the ends of a line of the frame; what
//                          the clamp to the plane's own border spoils moves in one pixel per pass and never reaches the tile) and is
//                          written to the workspace.  Each workgroup also writes ONE partial of the integer L sum that the contrast op
//                          of each list needs -- of the blurred frame for a `data_syn` job, so the blur has to exist before the mean does
//                          -- with plain stores, combined in index order in the second launch: exact whatever the schedule.
//   segnet_samples_kernel  one thread per output pixel: flip, jitter, composite, float32, Normalize; planar f32 and i64 stores.
// The per-pixel arithmetic is segnet_px.h / aug_px.h (also compiled for the host, tools/check_segnet_px.py); batch, reduction and the
// checks of a jitter list are sample_batch.h, shared with the other sample builders.
#include "sample_batch.h"
#include "segnet_px.h"

namespace {

using namespace ape;

constexpr int kT = 256;
constexpr int kTile = 32;                    // side of a tile of the prepare launch
constexpr int kHalo = 3;                     // three passes of a three-tap box per direction
constexpr int kPlane = kTile + 2 * kHalo;
constexpr int kTileW = 32, kTileH = 8;       // output tile of the samples launch

using SegnetBatch = SampleBatch<ape_segnet_job, 3>;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// grid (kBlocks, nb)
__global__ __launch_bounds__(kT) void segnet_prepare_kernel(SegnetBatch bt, int job0, int H, int W, unsigned long long* luma, uint8_t* ws)
{
    __shared__ uchar4 s_plane[2][kPlane][kPlane];
    __shared__ unsigned long long red0[kT / 64], red1[kT / 64];
    const ape_segnet_job& j = bt.j[blockIdx.y];
    const bool syn = j.back_rgb != nullptr;                          // uniform per workgroup
    const int kc0 = aug_contrast_at(j.jit[0]), kc1 = syn ? aug_contrast_at(j.jit[1]) : -1;
    uint8_t* blurred = syn ? ws + j.blur_off : nullptr;
    const unsigned int ww = j.blur_ww, fw = j.blur_fw;
    const int tid = threadIdx.x;
    const int tiles_x = (W + kTile - 1) / kTile, tiles = tiles_x * ((H + kTile - 1) / kTile);
    unsigned long long s0 = 0, s1 = 0;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int x0 = (t % tiles_x) * kTile, y0 = (t / tiles_x) * kTile;
        const int ox = x0 - kHalo, oy = y0 - kHalo;                  // image coordinates of the plane's corner
        if (syn) {
            for (int i = tid; i < kPlane * kPlane; i += kT) {
                const int py = i / kPlane, px = i % kPlane, gx = ox + px, gy = oy + py;
                uchar4 v = make_uchar4(0, 0, 0, 0);
                if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                    const uint8_t* p = j.rgb + ((long)gy * W + gx) * 3;
                    v = make_uchar4((unsigned char)pil_blend(0, p[0], j.bright), (unsigned char)pil_blend(0, p[1], j.bright),
                                    (unsigned char)pil_blend(0, p[2], j.bright), 0);
                }
                s_plane[0][py][px] = v;
            }
            __syncthreads();
            // passes 0..2 along the rows, 3..5 along the columns; an even number of passes, so the result is back in plane 0.  Only
            // positions inside the image are written, and their neighbours are inside it too: nothing else is ever read.
            for (int pass = 0; pass < 6; ++pass) {
                const uchar4 (*src)[kPlane] = s_plane[pass & 1];
                uchar4 (*dst)[kPlane] = s_plane[(pass & 1) ^ 1];
                for (int i = tid; i < kPlane * kPlane; i += kT) {
                    const int py = i / kPlane, px = i % kPlane, gx = ox + px, gy = oy + py;
                    if (gx < 0 || gx >= W || gy < 0 || gy >= H) continue;
                    uchar4 l, r;
                    if (pass < 3) {
                        l = src[py][clampi(clampi(gx - 1, 0, W - 1) - ox, 0, kPlane - 1)];
                        r = src[py][clampi(clampi(gx + 1, 0, W - 1) - ox, 0, kPlane - 1)];
                    } else {
                        l = src[clampi(clampi(gy - 1, 0, H - 1) - oy, 0, kPlane - 1)][px];
                        r = src[clampi(clampi(gy + 1, 0, H - 1) - oy, 0, kPlane - 1)][px];
                    }
                    const uchar4 c = src[py][px];
                    dst[py][px] = make_uchar4((unsigned char)segnet_blur_tap(l.x, c.x, r.x, ww, fw), (unsigned char)segnet_blur_tap(l.y, c.y, r.y, ww, fw),
                                              (unsigned char)segnet_blur_tap(l.z, c.z, r.z, ww, fw), 0);
                }
                __syncthreads();
            }
        }
        for (int i = tid; i < kTile * kTile; i += kT) {
            const int ty = i / kTile, tx = i % kTile, gx = x0 + tx, gy = y0 + ty;
            if (gx >= W || gy >= H) continue;
            int r, g, b;
            if (syn) {
                const uchar4 v = s_plane[0][ty + kHalo][tx + kHalo];
                uint8_t* out = blurred + ((long)gy * W + gx) * 3;
                out[0] = v.x; out[1] = v.y; out[2] = v.z;
                if (kc0 >= 0) {
                    r = v.x; g = v.y; b = v.z;
                    aug_jitter(j.jit[0], kc0, 0, r, g, b);
                    s0 += (unsigned long long)pil_luma(r, g, b);
                }
            } else if (kc0 >= 0) {
                aug_jittered_rgb(j.rgb, j.jit[0], W, gx, gy, kc0, 0, r, g, b);
                s0 += (unsigned long long)pil_luma(r, g, b);
            }
            if (kc1 >= 0) {
                aug_jittered_rgb(j.back_rgb, j.jit[1], W, gx, gy, kc1, 0, r, g, b);
                s1 += (unsigned long long)pil_luma(r, g, b);
            }
        }
        if (syn) __syncthreads();                                    // plane 0 is read above and filled again by the next tile
    }
    park(part<Sum>(s0, red0), part<Sum>(s1, red1));
    __syncthreads();
    if (tid == 0) {
        const long p = (long)(job0 + blockIdx.y) * 2 * kBlocks + blockIdx.x;
        luma[p] = total<kT / 64, Sum>(red0);
        luma[p + kBlocks] = total<kT / 64, Sum>(red1);
    }
}

// grid (tiles_x, tiles_y, nb)
__global__ __launch_bounds__(kT) void segnet_samples_kernel(SegnetBatch bt, int job0, int H, int W, const unsigned long long* __restrict__ luma,
                                                            const uint8_t* __restrict__ ws, float* __restrict__ rgb, long long* __restrict__ target)
{
    __shared__ int s_mean[2];
    const ape_segnet_job& j = bt.j[blockIdx.z];
    const int s = job0 + blockIdx.z;
    if (threadIdx.x < 2) s_mean[threadIdx.x] = mean_from_partials(j.jit[threadIdx.x], luma + ((long)s * 2 + threadIdx.x) * kBlocks, H, W);
    __syncthreads();
    const int x = blockIdx.x * kTileW + threadIdx.x % kTileW, y = blockIdx.y * kTileH + threadIdx.x / kTileW;
    if (x >= W || y >= H) return;
    int xs, ys;
    segnet_src(j.flip, H, W, x, y, xs, ys);
    const bool syn = j.back_rgb != nullptr;
    const uint8_t* frame = syn ? ws + j.blur_off : j.rgb;
    const double* noise = syn ? (const double*)(ws + j.noise_off) + ((long)ys * W + xs) : nullptr;
    const int mean[2] = {s_mean[0], s_mean[1]};
    float v[3];
    const int lab = segnet_pixel(j, frame, H, W, xs, ys, mean, noise, v);
    const long plane = (long)H * W, o = (long)y * W + x;
    float* out = rgb + (long)s * 3 * plane + o;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c * plane] = segnet_normalised(v[c], bt.mean[c], bt.stdv[c]);
    target[(long)s * plane + o] = lab;
}

bool region_ok(long long off, int align, size_t bytes, size_t base, size_t ws_bytes)
{
    if (off < 0 || (off & (align - 1)) || (size_t)off < base || (size_t)off > ws_bytes) return false;
    return ws_bytes - (size_t)off >= bytes;
}

// what both launches refuse in a job; the noise is only looked at where it is read
bool job_ok(const ape_segnet_job& j, int H, int W, size_t base, size_t ws_bytes, bool with_noise)
{
    if (!j.rgb || !j.label || (j.back_rgb == nullptr) != (j.back_label == nullptr)) return false;
    if (!jitter_ok(j.jit[0]) || !jitter_ok(j.jit[1])) return false;
    if (!j.back_rgb) return true;
    if (!(j.bright == j.bright)) return false;
    if ((unsigned long long)j.blur_ww + 2ull * j.blur_fw > (1ull << 24)) return false;
    const size_t px = (size_t)H * W;
    if (!region_ok(j.blur_off, 16, px * 3, base, ws_bytes)) return false;
    return !with_noise || region_ok(j.noise_off, 8, px * 3 * sizeof(double), base, ws_bytes);
}

}  // namespace

extern "C" size_t ape_segnet_samples_frames_offset(int B) { return B < 1 ? 0 : (size_t)B * 2 * kBlocks * sizeof(unsigned long long); }

extern "C" int ape_segnet_samples_prepare(const ape_segnet_job* jobs, int B, int H, int W, void* ws, size_t ws_bytes, void* stream)
{
    if (!frame_ok(B, H, W)) return APE_EINVAL;
    if (B == 0) return APE_OK;
    if (!jobs || !ws || ((uintptr_t)ws & 15)) return APE_EINVAL;
    const size_t base = ape_segnet_samples_frames_offset(B);
    if (ws_bytes < base) return APE_EWORKSPACE;
    for (int i = 0; i < B; ++i)
        if (!job_ok(jobs[i], H, W, base, ws_bytes, false)) return APE_EINVAL;
    SegnetBatch bt = {};
    for_each_chunk(bt, jobs, B, [&](const SegnetBatch& b, int i0, int nb) {
        hipLaunchKernelGGL(segnet_prepare_kernel, dim3(kBlocks, nb), dim3(kT), 0, (hipStream_t)stream, b, i0, H, W, (unsigned long long*)ws,
                           (uint8_t*)ws);
    });
    return check_launch("ape_segnet_samples_prepare");
}

extern "C" int ape_segnet_samples(const ape_segnet_job* jobs, int B, int H, int W, const float* mean3_host, const float* std3_host, float* rgb,
                                  long long* target, void* ws, size_t ws_bytes, void* stream)
{
    SegnetBatch bt = {};
    if (!frame_ok(B, H, W) || !norm_ok(mean3_host, std3_host, bt)) return APE_EINVAL;
    if (B == 0) return APE_OK;
    if (!jobs || !rgb || !target || !ws || ((uintptr_t)rgb & 3) || ((uintptr_t)target & 7) || ((uintptr_t)ws & 15)) return APE_EINVAL;
    const size_t base = ape_segnet_samples_frames_offset(B);
    if (ws_bytes < base) return APE_EWORKSPACE;
    for (int i = 0; i < B; ++i)
        if (jobs[i].flip < 0 || jobs[i].flip > 3 || !job_ok(jobs[i], H, W, base, ws_bytes, true)) return APE_EINVAL;
    const dim3 tiles(ceil_div(W, kTileW), ceil_div(H, kTileH));
    for_each_chunk(bt, jobs, B, [&](const SegnetBatch& b, int i0, int nb) {
        hipLaunchKernelGGL(segnet_samples_kernel, dim3(tiles.x, tiles.y, nb), dim3(kT), 0, (hipStream_t)stream, b, i0, H, W,
                           (const unsigned long long*)ws, (const uint8_t*)ws, rgb, target);
    });
    return check_launch("ape_segnet_samples");
}
