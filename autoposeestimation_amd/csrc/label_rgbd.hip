// The classical RGB-D labeller (reference label_generator/utils.py:createLabel_RGBD, :45-364) on the device, a batch of frame pairs at a
// time, in float64 where the reference is.  Parity with OpenCV unpinned: the colour-space change, the morphology, the box filter and the
// component numbering follow OpenCV's documented semantics as tests/label_rgbd_reference.py restates them; the per-pixel arithmetic is
// label_px.h, which tools/check_label_px.py also compiles for the host.
//
// Whole-frame passes (HBM-bound, 8 B per pixel and image):
//   rgbd_gate          depth u16 -> float64 inside [measure_dist - 150, measure_dist + 150], else 0                      (:102-108)
//   rgbd_plane / box   the background's centre window: holes filled from the three-point plane, then the 5 x 5 box filter (:135-159)
//   rgbd_score         HSV / RGB differences, clip at 100, weights, channel sum (kept as the colour score), depth term, threshold
//   rgbd_morph1d       one axis of an erode (min) or dilate (max); min and max are exact, so rows then columns IS the k x k result.  A
//                      pass reads in-image pixels only and writes a whole image, so no out-of-image intermediate ever exists
//   rgbd_wrap          np.array(img, dtype=np.uint8): truncate, wrap modulo 256
//   ccl.h              run-based union-find, root = smallest pixel index = raster-order numbering
//   rgbd_stats         per component the pixel count and the sum of the image, as u64 fixed point in two limbs (2^-12 and 2^-52 units):
//                      integer atomics, so the sums do not depend on the arrival order and two runs give the same bits
//   rgbd_pick / apply  best component above min_size by int(mean) or by size, strict '>', first in raster order wins ties; without a
//                      winner the reference keeps `uni[0]`: the background region, or everything when there is no background pixel
//   rgbd_dev / cut     population std of the non-zero colour scores, pixels below mean - std zeroed                       (:311-315)
#include "common.h"
#include "label_px.h"
#include "ccl.h"

namespace {

using namespace ape;

constexpr int kT = 256;
constexpr int kGridCap = 16384;
typedef unsigned long long u64;

struct RgbdArgs {
    double w[6], wd, threshold;
    int mode;
};

// per-frame state of one component round
struct RgbdFrame {
    u64 best;            // (score << 32) | (0xffffffff - root index inside the frame); 0 = no winner
    u64 hi, lo;          // sum of the kept non-zero colour scores
    u64 hi2, lo2;        // sum of their squared deviations
    unsigned int n, pad;
};

// v in [0, 2^18) -> two integer limbs: hi counts 2^-12, lo counts 2^-52 (exact for every double >= 2^-1 in range, below 2^-53 off else)
__device__ __forceinline__ void fx_split(double v, u64& hi, u64& lo)
{
    v = v >= 0.0 ? v : 0.0;                      // (NaN too)
    v = v > 262143.0 ? 262143.0 : v;
    const double s = v * 4096.0, f = floor(s);
    hi = (u64)f;
    lo = (u64)rint((s - f) * 1099511627776.0);
}
__device__ __forceinline__ double fx_value(u64 hi, u64 lo) { return (double)hi * (1.0 / 4096.0) + (double)lo * (1.0 / 4503599627370496.0); }

__device__ __forceinline__ u64 wave_sum(u64 v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ void rgbd_gate_kernel(const uint16_t* __restrict__ depth, const double* __restrict__ md, double* __restrict__ out, int HW, long npix)
{
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x)
        out[p] = label_gate((double)depth[p], md[p / HW]);
}

// window pixel q of frame b = q / (wh * ww); frames without a non-zero window pixel (valid[b] == 0) are left alone (:117)
__global__ void rgbd_plane_kernel(const double* __restrict__ bd, const double* __restrict__ pts, const int* __restrict__ valid,
                                  double* __restrict__ tmp, int HW, int W, int r0, int c0, int wh, int ww, long nwin)
{
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < nwin; q += (long)gridDim.x * blockDim.x) {
        const int b = q / ((long)wh * ww);
        if (!valid[b]) continue;
        const int rem = q - (long)b * wh * ww;
        const int row = rem / ww, col = rem - row * ww;
        tmp[q] = label_plane_pixel(label_plane_of(pts + (long)b * 9), row, col, bd[(long)b * HW + (long)(r0 + row) * W + c0 + col]);
    }
}

__global__ void rgbd_box_kernel(const double* __restrict__ tmp, const int* __restrict__ valid, double* __restrict__ bd, int HW, int W, int r0,
                                int c0, int wh, int ww, int k, double tap, long nwin)
{
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < nwin; q += (long)gridDim.x * blockDim.x) {
        const int b = q / ((long)wh * ww);
        if (valid && !valid[b]) continue;
        const int rem = q - (long)b * wh * ww;
        const int row = rem / ww, col = rem - row * ww;
        const int lo = k / 2;
        const double* src = tmp + (long)b * wh * ww;
        double acc = 0.0;
        for (int dy = -lo; dy <= k - 1 - lo; ++dy) {
            const double* line = src + (long)label_reflect101(row + dy, wh) * ww;
            for (int dx = -lo; dx <= k - 1 - lo; ++dx) acc = acc + tap * line[label_reflect101(col + dx, ww)];
        }
        bd[(long)b * HW + (long)(r0 + row) * W + c0 + col] = acc;
    }
}

__global__ void rgbd_score_kernel(const uint8_t* __restrict__ f_rgb, const uint8_t* __restrict__ b_rgb, const uint16_t* __restrict__ f_depth,
                                  const double* __restrict__ bd, const double* __restrict__ md, RgbdArgs a, double* __restrict__ score,
                                  double* __restrict__ color, int HW, long npix)
{
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
        double fd = 0.0, bdv = 0.0, col;
        if (a.wd > 0.0) {
            fd = label_gate((double)f_depth[p], md[p / HW]);
            bdv = bd[p];
        }
        score[p] = label_score(f_rgb + p * 3, b_rgb + p * 3, fd, bdv, a.mode, a.w, a.wd, a.threshold, col);
        color[p] = col;
    }
}

// one axis of an erode / dilate with a k-wide all-ones footprint, offsets -(k / 2) .. k - 1 - (k / 2); out-of-image pixels do not take part
template <bool kMax>
__global__ void rgbd_morph1d_kernel(const double* __restrict__ src, double* __restrict__ dst, int H, int W, int k, int vertical, long npix)
{
    const int lo = k / 2;
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
        const int x = p % W, y = (p / W) % H;
        const int at = vertical ? y : x, n = vertical ? H : W;
        const long step = vertical ? W : 1;
        int o0 = -lo, o1 = k - 1 - lo;
        if (at + o0 < 0) o0 = -at;
        if (at + o1 > n - 1) o1 = n - 1 - at;
        double m = src[p + o0 * step];
        for (int o = o0 + 1; o <= o1; ++o) {
            const double v = src[p + o * step];
            m = kMax ? (v > m ? v : m) : (v < m ? v : m);
        }
        dst[p] = m;
    }
}

__global__ void rgbd_wrap_kernel(const double* __restrict__ img, uint8_t* __restrict__ out, long npix, int binary)
{
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
        const int v = label_wrap_u8(img[p]);
        out[p] = (uint8_t)(binary ? (v != 0) : v);
    }
}

__global__ void rgbd_frame_init_kernel(RgbdFrame* st, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) st[b] = RgbdFrame{0, 0, 0, 0, 0, 0, 0};
}

// ccl_compress_kernel with the two-limb accumulators: a root zeroes its own triple
__global__ void rgbd_compress_kernel(int* __restrict__ L, long npix, u64* __restrict__ hi, u64* __restrict__ lo, unsigned int* __restrict__ cnt)
{
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
        int a = L[p];
        if (a < 0) continue;
        while (true) {
            const int q = L[a];
            if (q == a) break;
            a = q;
        }
        L[p] = a;
        if (a == (int)p) { hi[p] = 0ull; lo[p] = 0ull; cnt[p] = 0u; }
    }
}

// per component: count and fixed-point sum of img at the root's index; a wave is 64 consecutive pixels, one atomic triple per distinct root in it
__global__ void rgbd_stats_kernel(const double* __restrict__ img, const int* __restrict__ L, u64* __restrict__ hi, u64* __restrict__ lo,
                                  unsigned int* __restrict__ cnt, long npix)
{
    const long nround = (npix + 63) & ~63L;
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < nround; p += (long)gridDim.x * blockDim.x) {
        int root = -1;
        u64 h = 0, l = 0;
        if (p < npix) {
            root = L[p];
            if (root >= 0) fx_split(img[p], h, l);
        }
        const int lane = threadIdx.x & 63;
        u64 todo = __ballot(root >= 0);
        for (int rounds = 0; todo && rounds < 6; ++rounds) {
            const int leader = __ffsll((long long)todo) - 1;
            const int r0 = __shfl(root, leader);
            const bool mine = root == r0;
            const u64 grp = __ballot(mine);
            const u64 hs = wave_sum(mine ? h : 0ull), ls = wave_sum(mine ? l : 0ull);
            if (lane == leader) {
                atomicAdd(&hi[r0], hs);
                atomicAdd(&lo[r0], ls);
                atomicAdd(&cnt[r0], (unsigned int)__popcll(grp));
            }
            todo &= ~grp;
        }
        if (root >= 0 && ((todo >> lane) & 1ull)) {
            atomicAdd(&hi[root], h);
            atomicAdd(&lo[root], l);
            atomicAdd(&cnt[root], 1u);
        }
    }
}

__global__ void rgbd_pick_kernel(const int* __restrict__ L, const u64* __restrict__ hi, const u64* __restrict__ lo,
                                 const unsigned int* __restrict__ cnt, RgbdFrame* __restrict__ st, int HW, int min_size, int by_size, long npix)
{
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
        if (L[p] != (int)p) continue;
        const unsigned int n = cnt[p];
        if ((long)n <= (long)min_size) continue;                      // counts[i + 1] > min_size
        const int b = p / HW;
        u64 s = n;
        if (!by_size) {
            const double mean = fx_value(hi[p], lo[p]) / (double)n;
            s = mean >= 1.0 ? (u64)mean : 0ull;                       // int(np.mean(...)); `> score` with score = 0 needs at least 1
        }
        if (s) atomicMax(&st[b].best, (s << 32) | (u64)(0xffffffffu - (unsigned int)(p - (long)b * HW)));
    }
}

__device__ __forceinline__ bool rgbd_kept(const int* L, const unsigned int* cnt, const RgbdFrame& f, int b, int HW, long p)
{
    const int root = L[p];
    if (f.best) return root == (int)((long)b * HW + (long)(0xffffffffu - (unsigned int)(f.best & 0xffffffffull)));
    return root < 0 || cnt[root] == (unsigned int)HW;          // uni[0]: the background, or label 1 when the frame has no background pixel
}

// color zeroed outside the chosen label (in place); with `sums` the kept non-zero values are summed per frame; with `out` the final mask
__global__ void rgbd_apply_kernel(const int* __restrict__ L, const unsigned int* __restrict__ cnt, RgbdFrame* __restrict__ st,
                                  double* __restrict__ color, uint8_t* __restrict__ out, int HW, int sums)
{
    const int b = blockIdx.y;
    const RgbdFrame f = st[b];
    u64 h = 0, l = 0, n = 0;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < HW; q += gridDim.x * blockDim.x) {
        const long p = (long)b * HW + q;
        double v = color[p];
        if (!rgbd_kept(L, cnt, f, b, HW, p)) v = 0.0;
        if (out) out[p] = v != 0.0 ? 255 : 0;
        else color[p] = v;
        if (sums && v != 0.0) {
            u64 a, c;
            fx_split(v, a, c);
            h += a; l += c; n += 1;
        }
    }
    if (sums) {
        h = wave_sum(h); l = wave_sum(l); n = wave_sum(n);
        if ((threadIdx.x & 63) == 0 && n) {
            atomicAdd(&st[b].hi, h);
            atomicAdd(&st[b].lo, l);
            atomicAdd(&st[b].n, (unsigned int)n);
        }
    }
}

__global__ void rgbd_dev_kernel(const double* __restrict__ color, RgbdFrame* __restrict__ st, int HW)
{
    const int b = blockIdx.y;
    const double mean = fx_value(st[b].hi, st[b].lo) / (double)st[b].n;
    u64 h = 0, l = 0;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < HW; q += gridDim.x * blockDim.x) {
        const double v = color[(long)b * HW + q];
        if (v != 0.0) {
            const double d = v - mean;
            u64 a, c;
            fx_split(d * d, a, c);
            h += a; l += c;
        }
    }
    h = wave_sum(h); l = wave_sum(l);
    if ((threadIdx.x & 63) == 0 && (h | l)) {
        atomicAdd(&st[b].hi2, h);
        atomicAdd(&st[b].lo2, l);
    }
}

__global__ void rgbd_cut_kernel(double* __restrict__ color, const RgbdFrame* __restrict__ st, double* __restrict__ mean_std, int HW)
{
    const int b = blockIdx.y;
    const double n = (double)st[b].n;
    const double mean = fx_value(st[b].hi, st[b].lo) / n;
    const double sd = sqrt(fx_value(st[b].hi2, st[b].lo2) / n);
    const double cut = mean - sd;
    if (mean_std && blockIdx.x == 0 && threadIdx.x == 0) { mean_std[b * 2] = mean; mean_std[b * 2 + 1] = sd; }
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < HW; q += gridDim.x * blockDim.x) {
        const long p = (long)b * HW + q;
        if (color[p] < cut) color[p] = 0.0;
    }
}

__global__ void rgbd_stats_out_kernel(const int* __restrict__ L, const u64* __restrict__ hi, const u64* __restrict__ lo,
                                      const unsigned int* __restrict__ cnt, int* __restrict__ root, unsigned int* __restrict__ count,
                                      double* __restrict__ sum, long npix)
{
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
        const bool is_root = L[p] == (int)p;
        root[p] = L[p];
        count[p] = is_root ? cnt[p] : 0u;
        sum[p] = is_root ? fx_value(hi[p], lo[p]) : 0.0;
    }
}

struct RgbdWs {
    uint8_t* fg;
    int* L;
    u64 *hi, *lo;
    unsigned int* cnt;
    RgbdFrame* st;
};

size_t rgbd_ws_bytes(int B, int H, int W)
{
    const size_t npix = (size_t)B * H * W;
    return align_up(npix) + align_up(npix * 4) * 2 + align_up(npix * 8) * 2 + align_up((size_t)B * sizeof(RgbdFrame));
}

RgbdWs rgbd_carve(void* workspace, int B, int H, int W)
{
    const size_t npix = (size_t)B * H * W;
    char* ws = (char*)workspace;
    RgbdWs r;
    r.hi = (u64*)ws;            ws += align_up(npix * 8);
    r.lo = (u64*)ws;            ws += align_up(npix * 8);
    r.L = (int*)ws;             ws += align_up(npix * 4);
    r.cnt = (unsigned int*)ws;  ws += align_up(npix * 4);
    r.st = (RgbdFrame*)ws;      ws += align_up((size_t)B * sizeof(RgbdFrame));
    r.fg = (uint8_t*)ws;
    return r;
}

bool rgbd_shape_ok(int B, int H, int W)
{
    return B >= 0 && B <= 65535 && H >= 1 && W >= 1 && (long)B * H * W < (1L << 31) - 64;
}

// wrap -> labelling -> per-component count and sum of img
void rgbd_label_and_stats(const double* img, const RgbdWs& r, int B, int H, int W, hipStream_t st)
{
    const long npix = (long)B * H * W;
    const int g = grid_for(npix, kT, kGridCap);
    hipLaunchKernelGGL(rgbd_frame_init_kernel, dim3(ceil_div(B, kT)), dim3(kT), 0, st, r.st, B);
    hipLaunchKernelGGL(rgbd_wrap_kernel, dim3(g), dim3(kT), 0, st, img, r.fg, npix, 1);
    hipLaunchKernelGGL(ccl_init_kernel, dim3(g), dim3(kT), 0, st, r.fg, r.L, W, npix);
    hipLaunchKernelGGL(ccl_merge_kernel, dim3(g), dim3(kT), 0, st, r.fg, r.L, H, W, npix);
    hipLaunchKernelGGL(rgbd_compress_kernel, dim3(g), dim3(kT), 0, st, r.L, npix, r.hi, r.lo, r.cnt);
    hipLaunchKernelGGL(rgbd_stats_kernel, dim3(g), dim3(kT), 0, st, img, r.L, r.hi, r.lo, r.cnt, npix);
}

}  // namespace

extern "C" size_t ape_rgbd_cca_workspace_bytes(int B, int H, int W)
{
    if (!rgbd_shape_ok(B, H, W)) return 0;
    return rgbd_ws_bytes(B, H, W);
}

extern "C" int ape_rgbd_gate_f64(const uint16_t* depth, const double* measure_dist, double* out, int B, int H, int W, void* stream)
{
    if (!depth || !measure_dist || !out || !rgbd_shape_ok(B, H, W)) return APE_EINVAL;
    const long npix = (long)B * H * W;
    if (npix == 0) return APE_OK;
    hipLaunchKernelGGL(rgbd_gate_kernel, dim3(grid_for(npix, kT, kGridCap)), dim3(kT), 0, (hipStream_t)stream, depth, measure_dist, out, H * W, npix);
    return check_launch("ape_rgbd_gate_f64");
}

extern "C" int ape_rgbd_plane_fill_f64(double* b_depth, const double* pts, const int* valid, double* tmp, int B, int H, int W, int r0, int r1,
                                       int c0, int c1, void* stream)
{
    if (!b_depth || !pts || !valid || !tmp || !rgbd_shape_ok(B, H, W) || r0 < 0 || r1 > H || r0 >= r1 || c0 < 0 || c1 > W || c0 >= c1)
        return APE_EINVAL;
    const int wh = r1 - r0, ww = c1 - c0;
    const long nwin = (long)B * wh * ww;
    if (nwin == 0) return APE_OK;
    const int g = grid_for(nwin, kT, kGridCap);
    const double tap = (double)(1.0f / 25.0f);               // np.ones((5, 5), np.float32) / 25
    hipLaunchKernelGGL(rgbd_plane_kernel, dim3(g), dim3(kT), 0, (hipStream_t)stream, b_depth, pts, valid, tmp, H * W, W, r0, c0, wh, ww, nwin);
    hipLaunchKernelGGL(rgbd_box_kernel, dim3(g), dim3(kT), 0, (hipStream_t)stream, tmp, valid, b_depth, H * W, W, r0, c0, wh, ww, 5, tap, nwin);
    return check_launch("ape_rgbd_plane_fill_f64");
}

extern "C" int ape_rgbd_box_f64(const double* src, double* dst, int B, int H, int W, int k, void* stream)
{
    if (!src || !dst || src == dst || !rgbd_shape_ok(B, H, W) || k < 1 || k > 255) return APE_EINVAL;
    const long npix = (long)B * H * W;
    if (npix == 0) return APE_OK;
    const double tap = (double)(1.0f / (float)(k * k));
    hipLaunchKernelGGL(rgbd_box_kernel, dim3(grid_for(npix, kT, kGridCap)), dim3(kT), 0, (hipStream_t)stream, src, (const int*)nullptr, dst, H * W, W,
                       0, 0, H, W, k, tap, npix);
    return check_launch("ape_rgbd_box_f64");
}

extern "C" int ape_rgbd_score_f64(const uint8_t* f_rgb, const uint8_t* b_rgb, const uint16_t* f_depth, const double* b_depth,
                                  const double* measure_dist, int mode, const double* weights7_host, double threshold, double* score,
                                  double* color, int B, int H, int W, void* stream)
{
    if (!f_rgb || !b_rgb || !weights7_host || !score || !color || !rgbd_shape_ok(B, H, W)) return APE_EINVAL;
    if (mode != APE_RGBD_MODE_RGB && mode != APE_RGBD_MODE_HSV && mode != APE_RGBD_MODE_BOTH) return APE_EINVAL;
    RgbdArgs a;
    for (int c = 0; c < 6; ++c) a.w[c] = weights7_host[c];
    a.wd = weights7_host[6];
    a.threshold = threshold;
    a.mode = mode;
    if (a.wd > 0.0 && (!f_depth || !b_depth || !measure_dist)) return APE_EINVAL;
    const long npix = (long)B * H * W;
    if (npix == 0) return APE_OK;
    hipLaunchKernelGGL(rgbd_score_kernel, dim3(grid_for(npix, kT, kGridCap)), dim3(kT), 0, (hipStream_t)stream, f_rgb, b_rgb, f_depth, b_depth,
                       measure_dist, a, score, color, H * W, npix);
    return check_launch("ape_rgbd_score_f64");
}

extern "C" int ape_rgbd_morph_f64(const double* src, double* dst, double* tmp, int B, int H, int W, int k, int dilate, void* stream)
{
    if (!src || !dst || !tmp || tmp == src || tmp == dst || !rgbd_shape_ok(B, H, W) || k < 1) return APE_EINVAL;
    const long npix = (long)B * H * W;
    if (npix == 0) return APE_OK;
    const int g = grid_for(npix, kT, kGridCap);
    hipStream_t st = (hipStream_t)stream;
    if (dilate) {
        hipLaunchKernelGGL(rgbd_morph1d_kernel<true>, dim3(g), dim3(kT), 0, st, src, tmp, H, W, k, 0, npix);
        hipLaunchKernelGGL(rgbd_morph1d_kernel<true>, dim3(g), dim3(kT), 0, st, (const double*)tmp, dst, H, W, k, 1, npix);
    } else {
        hipLaunchKernelGGL(rgbd_morph1d_kernel<false>, dim3(g), dim3(kT), 0, st, src, tmp, H, W, k, 0, npix);
        hipLaunchKernelGGL(rgbd_morph1d_kernel<false>, dim3(g), dim3(kT), 0, st, (const double*)tmp, dst, H, W, k, 1, npix);
    }
    return check_launch("ape_rgbd_morph_f64");
}

extern "C" int ape_rgbd_wrap_u8(const double* img, uint8_t* out, long npix, void* stream)
{
    if (!img || !out || npix < 0) return APE_EINVAL;
    if (npix == 0) return APE_OK;
    hipLaunchKernelGGL(rgbd_wrap_kernel, dim3(grid_for(npix, kT, kGridCap)), dim3(kT), 0, (hipStream_t)stream, img, out, npix, 0);
    return check_launch("ape_rgbd_wrap_u8");
}

extern "C" int ape_rgbd_component_stats(const double* img, int* root, unsigned int* count, double* sum, int B, int H, int W, void* workspace,
                                        size_t workspace_bytes, void* stream)
{
    if (!img || !root || !count || !sum || !workspace || !rgbd_shape_ok(B, H, W)) return APE_EINVAL;
    if (B == 0) return APE_OK;
    if (workspace_bytes < rgbd_ws_bytes(B, H, W)) return APE_EWORKSPACE;
    const RgbdWs r = rgbd_carve(workspace, B, H, W);
    const long npix = (long)B * H * W;
    rgbd_label_and_stats(img, r, B, H, W, (hipStream_t)stream);
    hipLaunchKernelGGL(rgbd_stats_out_kernel, dim3(grid_for(npix, kT, kGridCap)), dim3(kT), 0, (hipStream_t)stream, r.L, r.hi, r.lo, r.cnt, root,
                       count, sum, npix);
    return check_launch("ape_rgbd_component_stats");
}

extern "C" int ape_rgbd_cca_round(const double* img, double* color, uint8_t* out_or_null, double* mean_std_or_null, int B, int H, int W,
                                  int min_size, int by_size, int remove_one_std, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!img || !color || !workspace || !rgbd_shape_ok(B, H, W)) return APE_EINVAL;
    if (out_or_null && remove_one_std) return APE_EINVAL;            // the cut belongs to the first round, the mask to the second
    if (B == 0) return APE_OK;
    if (workspace_bytes < rgbd_ws_bytes(B, H, W)) return APE_EWORKSPACE;
    const RgbdWs r = rgbd_carve(workspace, B, H, W);
    hipStream_t st = (hipStream_t)stream;
    const long npix = (long)B * H * W;
    const int HW = H * W;
    rgbd_label_and_stats(img, r, B, H, W, st);
    hipLaunchKernelGGL(rgbd_pick_kernel, dim3(grid_for(npix, kT, kGridCap)), dim3(kT), 0, st, r.L, r.hi, r.lo, r.cnt, r.st, HW, min_size, by_size,
                       npix);
    int gx = ceil_div(HW, kT);
    gx = gx > 64 ? 64 : gx;
    hipLaunchKernelGGL(rgbd_apply_kernel, dim3(gx, B), dim3(kT), 0, st, r.L, r.cnt, r.st, color, out_or_null, HW, remove_one_std ? 1 : 0);
    if (remove_one_std) {
        hipLaunchKernelGGL(rgbd_dev_kernel, dim3(gx, B), dim3(kT), 0, st, (const double*)color, r.st, HW);
        hipLaunchKernelGGL(rgbd_cut_kernel, dim3(gx, B), dim3(kT), 0, st, color, (const RgbdFrame*)r.st, mean_std_or_null, HW);
    }
    return check_launch("ape_rgbd_cca_round");
}
