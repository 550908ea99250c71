// Training samples of the segmentor, built on the device from resident frames (reference segmentation/dataset.py:88-112 with the
// transforms of segmentation/utils.py:25-66 and CropAndZoom :361-487).  The reference does this in Pillow on the host, per sample: colour
// jitter of the full frame, rotation of frame and label, a label-driven square crop and a resize to 480 x 480 (BICUBIC / NEAREST).  Here a
// batch is two launches with one small read-back between them:
//   seg_stats_kernel   over the full frames: the integer L sum that ImageEnhance.Contrast needs (the un-rotated frame as it is when the
//                      op runs) and the extents of the ROTATED label's pixels == 255; one partial of each per workgroup, plain stores,
//                      combined in index order (sums here in the second launch, extents on the host) -- exact whatever the schedule
//   seg_train_kernel   one workgroup per 32 x 32 tile of OUTPUT pixels, three phases through LDS: (1) the tile's source patch -- its
//                      footprint in the crop plus the filter's reach, at most 37 x 37 for an enlargement -- each pixel jittered, rotated
//                      and taken at the crop's origin, so the expensive colour arithmetic runs ~1.4 times per output pixel at scale 1 and
//                      less when the crop is enlarged, not five times per pass; (2) the horizontal pass into LDS as u8; (3) the vertical
//                      pass, ToTensor, Normalize and planar f32 stores: a row of the tile is one 128-byte line per channel.  The label is
//                      gathered through the NEAREST index tables.
// The host only draws: the crop box needs the extents (the upper bound of np.random.randint depends on them), hence the read-back; the
// resize tables (2 x S x 5 weights and starts, 2 x S nearest indices per sample) are built there in double, as Pillow builds them, and the
// kernels do integer work only.  The per-pixel arithmetic is seg_px.h / aug_px.h (also compiled for the host, tools/check_seg_px.py);
// batch, reduction and job checks are sample_batch.h, shared with the other two sample builders.
#include "sample_batch.h"
#include "seg_px.h"

namespace {

using namespace ape;

constexpr int kTileW = 32, kTileH = 8, kT = kTileW * kTileH;
constexpr int kOT = 32;              // output tile side of the second launch
constexpr int kPatch = 40;           // patch side in LDS: (kOT - 1) * scale + 1 starts and 5 taps <= 37 for scale <= 1
constexpr int kTabInts = 14;         // table ints per output pixel side: hmin 1, hk 5, vmin 1, vk 5, nx 1, ny 1

using SegBatch = SampleBatch<ape_seg_train_job, 3>;

// grid (kBlocks, nb)
__global__ __launch_bounds__(kT) void seg_stats_kernel(SegBatch bt, int job0, int H, int W, unsigned long long* __restrict__ luma,
                                                       int* __restrict__ ext)
{
    __shared__ unsigned long long red_s[kT / 64];
    __shared__ int red_e[kT / 64][4], red_c[kT / 64];
    const ape_seg_train_job& j = bt.j[blockIdx.y];
    const int kc = aug_contrast_at(j.jit);
    unsigned long long s = 0;
    Extent e;
    int cnt = 0;
    const int tiles_x = (W + kTileW - 1) / kTileW, tiles = tiles_x * ((H + kTileH - 1) / kTileH);
    const int tx = threadIdx.x % kTileW, ty = threadIdx.x / kTileW;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int x = (t % tiles_x) * kTileW + tx, y = (t / tiles_x) * kTileH + ty;
        if (x < W && y < H) {
            if (kc >= 0) {                           // uniform per workgroup
                int r, g, b;
                aug_jittered_rgb(j.rgb, j.jit, W, x, y, kc, 0, r, g, b);
                s += (unsigned long long)pil_luma(r, g, b);
            }
            int xs, ys;
            if (aug_rot_src(j.rot, H, W, x, y, false, xs, ys) && j.label[(long)ys * W + xs] == 255) {
                e.add(x, y);
                ++cnt;
            }
        }
    }
    park(part<Sum>(s, red_s), part(e, red_e), part<Sum>(cnt, red_c));
    __syncthreads();
    if (threadIdx.x == 0) {
        const long p = (long)(job0 + blockIdx.y) * kBlocks + blockIdx.x;
        luma[p] = total<kT / 64, Sum>(red_s);
        total<kT / 64>(red_e, ext + p * 5);
        ext[p * 5 + 4] = total<kT / 64, Sum>(red_c);
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// grid (tiles, tiles, nb).  Every LDS index is clamped and every frame read is bounds-checked on its coordinates: the tables come from the
// caller through device memory, where the entry point cannot look at them.
__global__ __launch_bounds__(kT) void seg_train_kernel(SegBatch bt, int job0, int H, int W, int S, const unsigned long long* __restrict__ luma,
                                                       const int* __restrict__ tables, float* __restrict__ img, long long* __restrict__ label)
{
    __shared__ int s_mean;
    __shared__ int s_min[2][kOT], s_k[2][kOT][5];                // [0] horizontal (per output column), [1] vertical (per output row)
    __shared__ uchar4 s_patch[kPatch][kPatch];
    __shared__ uchar4 s_h[kPatch][kOT];
    const ape_seg_train_job& j = bt.j[blockIdx.z];
    const int s = job0 + blockIdx.z;
    const int* tab = tables + (long)s * kTabInts * S;
    const int ox0 = blockIdx.x * kOT, oy0 = blockIdx.y * kOT;
    const int nw = S - ox0 < kOT ? S - ox0 : kOT, nh = S - oy0 < kOT ? S - oy0 : kOT;
    const int tid = threadIdx.x;
    if (tid < 2 * kOT) {
        const int ax = tid / kOT, t = tid % kOT;
        const int o = (ax ? oy0 : ox0) + t;
        const int oc = o < S ? o : S - 1;                        // past the edge: a copy of the last line, never stored
        const int* base = tab + ax * 6 * S;
        s_min[ax][t] = base[oc];
        for (int k = 0; k < 5; ++k) s_k[ax][t][k] = base[S + oc * 5 + k];
    } else if (tid == 2 * kOT) {
        s_mean = mean_from_partials(j.jit, luma + (long)s * kBlocks, H, W);
    }
    __syncthreads();
    const int px0 = s_min[0][0], py0 = s_min[1][0];
    const int pw = clampi(s_min[0][nw - 1] + 5 - px0, 0, kPatch), ph = clampi(s_min[1][nh - 1] + 5 - py0, 0, kPatch);
    const int side = j.crop_side, mean = s_mean;
    // 1. the source patch: jitter -> rotate -> crop, per pixel
    for (int i = tid; i < ph * pw; i += kT) {
        const int pr = i / pw, pc = i % pw;
        const unsigned r = (unsigned)py0 + (unsigned)pr, c = (unsigned)px0 + (unsigned)pc;
        int cr = 0, cg = 0, cb = 0;
        if (r < (unsigned)side && c < (unsigned)side) seg_crop_rgb(j, H, W, (int)r, (int)c, mean, cr, cg, cb);
        s_patch[pr][pc] = make_uchar4((unsigned char)cr, (unsigned char)cg, (unsigned char)cb, 0);
    }
    __syncthreads();
    // 2. horizontal pass
    for (int i = tid; i < ph * kOT; i += kT) {
        const int pr = i / kOT, t = i % kOT;
        const int base = s_min[0][t] - px0;
        int a0 = 1 << (kSegResampleBits - 1), a1 = a0, a2 = a0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uchar4 p = s_patch[pr][clampi(base + k, 0, kPatch - 1)];
            const int kk = s_k[0][t][k];
            a0 += p.x * kk; a1 += p.y * kk; a2 += p.z * kk;
        }
        s_h[pr][t] = make_uchar4((unsigned char)seg_resample_clip8(a0), (unsigned char)seg_resample_clip8(a1),
                                 (unsigned char)seg_resample_clip8(a2), 0);
    }
    __syncthreads();
    // 3. vertical pass, ToTensor, Normalize; the label through the nearest tables
    const int* nx = tab + 12 * S;
    const int* ny = tab + 13 * S;
    const long plane = (long)S * S;
    for (int i = tid; i < kOT * kOT; i += kT) {
        const int ty = i / kOT, tx = i % kOT;
        if (tx >= nw || ty >= nh) continue;
        const int base = s_min[1][ty] - py0;
        int a0 = 1 << (kSegResampleBits - 1), a1 = a0, a2 = a0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uchar4 p = s_h[clampi(base + k, 0, kPatch - 1)][tx];
            const int kk = s_k[1][ty][k];
            a0 += p.x * kk; a1 += p.y * kk; a2 += p.z * kk;
        }
        const int ox = ox0 + tx, oy = oy0 + ty;
        const long o = (long)oy * S + ox;
        float* out = img + (long)s * 3 * plane + o;
        out[0] = ((float)seg_resample_clip8(a0) / 255.f - bt.mean[0]) / bt.stdv[0];
        out[plane] = ((float)seg_resample_clip8(a1) / 255.f - bt.mean[1]) / bt.stdv[1];
        out[2 * plane] = ((float)seg_resample_clip8(a2) / 255.f - bt.mean[2]) / bt.stdv[2];
        const unsigned lr = (unsigned)ny[oy], lc = (unsigned)nx[ox];
        int lab = 0;
        if (lr < (unsigned)side && lc < (unsigned)side) lab = seg_crop_label(j, H, W, (int)lr, (int)lc);
        label[(long)s * plane + o] = lab ? j.class_id : 0;
    }
}

// grid (tiles_x, tiles_y, nb)
__global__ __launch_bounds__(kT) void seg_plain_kernel(SegBatch bt, int job0, int H, int W, float* __restrict__ img, long long* __restrict__ label)
{
    const ape_seg_train_job& j = bt.j[blockIdx.z];
    const int s = job0 + blockIdx.z;
    const int x = blockIdx.x * kTileW + threadIdx.x % kTileW, y = blockIdx.y * kTileH + threadIdx.x / kTileW;
    if (x >= W || y >= H) return;
    const long plane = (long)H * W, o = (long)y * W + x;
    const uint8_t* px = j.rgb + o * 3;
    float* out = img + (long)s * 3 * plane + o;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c * plane] = ((float)px[c] / 255.f - bt.mean[c]) / bt.stdv[c];
    label[(long)s * plane + o] = j.label[o] ? j.class_id : 0;
}

bool job_ok(const ape_seg_train_job& j, int H, int W) { return j.rgb && j.label && rotation_ok(j.rot, H, W) && jitter_ok(j.jit); }

}  // namespace

extern "C" size_t ape_seg_train_extents_offset(int B) { return B < 1 ? 0 : (size_t)B * kBlocks * sizeof(unsigned long long); }

extern "C" size_t ape_seg_train_tables_offset(int B)
{
    return B < 1 ? 0 : ape_seg_train_extents_offset(B) + (size_t)B * kBlocks * 5 * sizeof(int);          // a multiple of 16
}

extern "C" size_t ape_seg_train_workspace_bytes(int B, int S)
{
    return B < 1 || S < 1 ? 0 : ape_seg_train_tables_offset(B) + (size_t)B * kTabInts * S * sizeof(int);
}

extern "C" int ape_seg_train_stats(const ape_seg_train_job* jobs, int B, int H, int W, void* ws, size_t ws_bytes, void* stream)
{
    if (!frame_ok(B, H, W)) return APE_EINVAL;
    if (B == 0) return APE_OK;
    if (!jobs || !ws || ((uintptr_t)ws & 15)) return APE_EINVAL;
    if (ws_bytes < ape_seg_train_tables_offset(B)) return APE_EWORKSPACE;
    for (int i = 0; i < B; ++i)
        if (!job_ok(jobs[i], H, W)) return APE_EINVAL;
    SegBatch bt = {};
    for_each_chunk(bt, jobs, B, [&](const SegBatch& b, int i0, int nb) {
        hipLaunchKernelGGL(seg_stats_kernel, dim3(kBlocks, nb), dim3(kT), 0, (hipStream_t)stream, b, i0, H, W, (unsigned long long*)ws,
                           (int*)((char*)ws + ape_seg_train_extents_offset(B)));
    });
    return check_launch("ape_seg_train_stats");
}

extern "C" int ape_seg_train_samples(const ape_seg_train_job* jobs, int B, int H, int W, int S, const float* mean3_host, const float* std3_host,
                                     float* img, long long* label, void* ws, size_t ws_bytes, void* stream)
{
    SegBatch bt = {};
    if (!frame_ok(B, H, W) || S < 1 || S > 32767 || !norm_ok(mean3_host, std3_host, bt)) return APE_EINVAL;
    if (B == 0) return APE_OK;
    // (img: the stores are scalar f32, which 4 bytes would serve; 16 is asked, as of the other sample builder's output, so that a caller's
    // buffer can later be written in wider pieces without a change of contract)
    if (!jobs || !img || !label || !ws || ((uintptr_t)img & 15) || ((uintptr_t)label & 7) || ((uintptr_t)ws & 15)) return APE_EINVAL;
    if (ws_bytes < ape_seg_train_workspace_bytes(B, S)) return APE_EWORKSPACE;
    for (int i = 0; i < B; ++i) {
        const ape_seg_train_job& j = jobs[i];
        if (!job_ok(j, H, W)) return APE_EINVAL;
        if (j.crop_side < 1 || j.crop_side > S) return APE_EINVAL;                   // enlargement only
        if (j.crop_x < -32768 || j.crop_x > 32767 || j.crop_y < -32768 || j.crop_y > 32767) return APE_EINVAL;
        if (j.class_id < 0) return APE_EINVAL;
    }
    const int tiles = ceil_div(S, kOT);
    for_each_chunk(bt, jobs, B, [&](const SegBatch& b, int i0, int nb) {
        hipLaunchKernelGGL(seg_train_kernel, dim3(tiles, tiles, nb), dim3(kT), 0, (hipStream_t)stream, b, i0, H, W, S,
                           (const unsigned long long*)ws, (const int*)((const char*)ws + ape_seg_train_tables_offset(B)), img, label);
    });
    return check_launch("ape_seg_train_samples");
}

extern "C" int ape_seg_plain_samples(const ape_seg_train_job* jobs, int B, int H, int W, const float* mean3_host, const float* std3_host,
                                     float* img, long long* label, void* stream)
{
    SegBatch bt = {};
    if (!frame_ok(B, H, W) || !norm_ok(mean3_host, std3_host, bt)) return APE_EINVAL;
    if (B == 0) return APE_OK;
    if (!jobs || !img || !label || ((uintptr_t)img & 3) || ((uintptr_t)label & 7)) return APE_EINVAL;
    for (int i = 0; i < B; ++i)
        if (!jobs[i].rgb || !jobs[i].label || jobs[i].class_id < 0) return APE_EINVAL;
    const dim3 tiles(ceil_div(W, kTileW), ceil_div(H, kTileH));
    for_each_chunk(bt, jobs, B, [&](const SegBatch& b, int i0, int nb) {
        hipLaunchKernelGGL(seg_plain_kernel, dim3(tiles.x, tiles.y, nb), dim3(kT), 0, (hipStream_t)stream, b, i0, H, W, img, label);
    });
    return check_launch("ape_seg_plain_samples");
}
