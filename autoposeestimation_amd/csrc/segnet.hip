// The glue of SegNet (DenseFusion/vanilla_segmentation/segnet.py:74-121, loss.py:11-21), NHWC fp32, one pass each:
//   max-pool 2x2 / stride 2 that records its winner     F.max_pool2d(kernel_size=2, stride=2, return_indices=True)
//   max-unpool 2x2                                      F.max_unpool2d(x, idx, 2, 2, output_size=(H, W))   (also the pool's backward)
//   gather at the recorded position                     the unpool's backward; a pool with forced indices
//   cross-entropy over the pixels of a logit map        nn.CrossEntropyLoss (mean) with its gradient
// The winner of a window is kept as code = 2 * dy + dx in one byte per element, not as torch's flat int64 index: the unpool of a window
// then needs nothing but its own code, so it is a plain write of the whole output (no memset, no scatter, no dependence on launch order).
// One thread per four channels: 16-byte loads and stores along the channel run, a uchar4 for the codes.
#include "common.h"

namespace {

constexpr int kT = 256;
constexpr int kGridCap = 8192;        // most workgroups of a grid-stride launch (ape::grid_for)

// torch's CPU rule (ATen max_pool2d_with_indices: `(val > maxval) || isnan(val)` from -inf, index of the window's first element): the
// first of equal maxima wins, 0.0 against -0.0 keeps the first, an all -inf window keeps position 0, the last NaN in scan order wins
__device__ __forceinline__ void take(float v, int k, float& best, unsigned& pos)
{
    if (v > best || v != v) { best = v; pos = k; }
}

__global__ __launch_bounds__(kT) void maxpool2x2_idx_kernel(const float4* __restrict__ x, float4* __restrict__ y, uchar4* __restrict__ code,
                                                            int B, int H, int W, int C4, int Ho, int Wo)
{
    const long total = (long)B * Ho * Wo * C4;
    const long row = (long)W * C4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = i % C4;
        long t = i / C4;
        const int ox = t % Wo; t /= Wo;
        const int oy = t % Ho;
        const int b = t / Ho;
        const float4* p = x + ((long)(b * H + 2 * oy) * W + 2 * ox) * C4 + c;
        const float4 v0 = p[0], v1 = p[C4], v2 = p[row], v3 = p[row + C4];
        const float ninf = -__builtin_inff();
        float4 m = make_float4(ninf, ninf, ninf, ninf);
        unsigned kx = 0, ky = 0, kz = 0, kw = 0;
        take(v0.x, 0, m.x, kx); take(v1.x, 1, m.x, kx); take(v2.x, 2, m.x, kx); take(v3.x, 3, m.x, kx);
        take(v0.y, 0, m.y, ky); take(v1.y, 1, m.y, ky); take(v2.y, 2, m.y, ky); take(v3.y, 3, m.y, ky);
        take(v0.z, 0, m.z, kz); take(v1.z, 1, m.z, kz); take(v2.z, 2, m.z, kz); take(v3.z, 3, m.z, kz);
        take(v0.w, 0, m.w, kw); take(v1.w, 1, m.w, kw); take(v2.w, 2, m.w, kw); take(v3.w, 3, m.w, kw);
        y[i] = m;
        code[i] = make_uchar4((unsigned char)kx, (unsigned char)ky, (unsigned char)kz, (unsigned char)kw);
    }
}

__device__ __forceinline__ float4 placed(float4 v, uchar4 k, unsigned at)
{
    return make_float4(k.x == at ? v.x : 0.f, k.y == at ? v.y : 0.f, k.z == at ? v.z : 0.f, k.w == at ? v.w : 0.f);
}

// One thread per CELL of the output and four channels: the 2x2 window of a pooled element, or what an odd last row / column leaves of one
// (then zeros).  The cells tile x, so every element is written exactly once.
__global__ __launch_bounds__(kT) void max_unpool2x2_kernel(const float4* __restrict__ y, const uchar4* __restrict__ code, float4* __restrict__ x,
                                                           int B, int H, int W, int C4, int Ho, int Wo, int Hc, int Wc)
{
    const long total = (long)B * Hc * Wc * C4;
    const long row = (long)W * C4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = i % C4;
        long t = i / C4;
        const int ox = t % Wc; t /= Wc;
        const int oy = t % Hc;
        const int b = t / Hc;
        float4* p = x + ((long)(b * H + 2 * oy) * W + 2 * ox) * C4 + c;
        if (oy < Ho && ox < Wo) {
            const long j = ((long)(b * Ho + oy) * Wo + ox) * C4 + c;
            const float4 v = y[j];
            const uchar4 k = code[j];
            p[0] = placed(v, k, 0);
            p[C4] = placed(v, k, 1);
            p[row] = placed(v, k, 2);
            p[row + C4] = placed(v, k, 3);
        } else {
            p[0] = zero;
            if (2 * ox + 1 < W) p[C4] = zero;
            if (2 * oy + 1 < H) p[row] = zero;          // (a cell with both neighbours in range is a whole window and took the branch above)
        }
    }
}

__device__ __forceinline__ float pick(float a, float b, float c, float d, unsigned k)
{
    const float lo = (k & 1u) ? b : a, hi = (k & 1u) ? d : c;
    return (k & 2u) ? hi : lo;
}

// The window's four 16-byte runs are loaded whole and the coded lane selected in registers: the four channels of a thread may name four
// different positions, and both rows of the window are fetched as cache lines either way.
__global__ __launch_bounds__(kT) void gather2x2_kernel(const float4* __restrict__ x, const uchar4* __restrict__ code, float4* __restrict__ y,
                                                       int B, int H, int W, int C4, int Ho, int Wo)
{
    const long total = (long)B * Ho * Wo * C4;
    const long row = (long)W * C4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = i % C4;
        long t = i / C4;
        const int ox = t % Wo; t /= Wo;
        const int oy = t % Ho;
        const int b = t / Ho;
        const float4* p = x + ((long)(b * H + 2 * oy) * W + 2 * ox) * C4 + c;
        const float4 v0 = p[0], v1 = p[C4], v2 = p[row], v3 = p[row + C4];
        const uchar4 k = code[i];
        y[i] = make_float4(pick(v0.x, v1.x, v2.x, v3.x, k.x), pick(v0.y, v1.y, v2.y, v3.y, k.y), pick(v0.z, v1.z, v2.z, v3.z, k.z),
                           pick(v0.w, v1.w, v2.w, v3.w, k.w));
    }
}

// ---- cross-entropy ------------------------------------------------------------------------------------------------------------------
constexpr int kCeMaxC = 64;
constexpr int kCeMaxBlocks = 1024;     // partials of the first stage; the pixel -> (block, thread) assignment depends on P alone

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// fixed-order sum of one double per thread over a 256-thread workgroup; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* lds)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return lds[0] + lds[1] + lds[2] + lds[3];
}

// One pixel per thread: the maximum, the sum of exponentials and the pixel's term  logsumexp(x) - x[label]  in fp32; the terms of a thread
// and then of the workgroup are summed in float64 in a fixed order.  With `dlogits`, the row softmax - onehot is written unscaled (the
// scale g / n_valid is known only after the count: ce_scale_kernel); a pixel whose label is >= C writes a zero row and adds to the count.
__global__ __launch_bounds__(kT) void ce_fwd_kernel(const float* __restrict__ logits, int ld, int C, const uint8_t* __restrict__ labels, long P,
                                                    float* __restrict__ dlogits, double* __restrict__ part)
{
    __shared__ double red[4];
    double sum = 0.0, bad = 0.0;
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < P; p += (long)gridDim.x * blockDim.x) {
        const float* l = logits + p * ld;
        const int lab = labels[p];
        float* d = dlogits ? dlogits + p * ld : nullptr;
        if (lab >= C) {
            bad += 1.0;
            if (d)
                for (int c = 0; c < ld; ++c) d[c] = 0.f;
            continue;
        }
        float m = l[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, l[c]);
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(l[c] - m);
        sum += (double)((m - l[lab]) + logf(s));
        if (d) {
            const float inv = 1.f / s;
            for (int c = 0; c < C; ++c) d[c] = expf(l[c] - m) * inv - (c == lab ? 1.f : 0.f);
            for (int c = C; c < ld; ++c) d[c] = 0.f;
        }
    }
    sum = block_sum(sum, red);
    bad = block_sum(bad, red);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = sum;
        part[2 * blockIdx.x + 1] = bad;
    }
}

__global__ __launch_bounds__(kT) void ce_finish_kernel(const double* __restrict__ part, int nblocks, long P, float g, double* __restrict__ out,
                                                       float* __restrict__ scale)
{
    __shared__ double red[4];
    double sum = 0.0, bad = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kT) {
        sum += part[2 * i];
        bad += part[2 * i + 1];
    }
    sum = block_sum(sum, red);
    bad = block_sum(bad, red);
    if (threadIdx.x == 0) {
        const double n = (double)P - bad;
        out[0] = sum / n;                      // no valid pixel: 0 / 0 = NaN, as torch's mean of nothing
        out[1] = bad;
        *scale = (float)((double)g / n);
    }
}

__global__ __launch_bounds__(kT) void ce_scale_kernel(float* __restrict__ d, long n4, long n, const float* __restrict__ scale)
{
    const float s = *scale;
    float4* d4 = (float4*)d;
    const long first = blockIdx.x * (long)blockDim.x + threadIdx.x, step = (long)gridDim.x * blockDim.x;
    for (long i = first; i < n4; i += step) {
        float4 v = d4[i];
        v.x *= s; v.y *= s; v.z *= s; v.w *= s;
        d4[i] = v;
    }
    for (long i = 4 * n4 + first; i < n; i += step) d[i] *= s;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// the checks the three window kernels share; `n` = elements of the full-resolution tensor
inline int window_check(int B, int H, int W, int C)
{
    if (B < 0 || H < 0 || W < 0 || C < 4 || C % 4) return APE_EINVAL;
    if ((long)B * H * W * C > (1L << 31)) return APE_EINVAL;
    return APE_OK;
}

}  // namespace

extern "C" int ape_maxpool2x2_idx_nhwc_f32(const float* x, float* y, uint8_t* code, int B, int H, int W, int C, void* stream)
{
    if (window_check(B, H, W, C) != APE_OK) return APE_EINVAL;
    const int Ho = H / 2, Wo = W / 2;
    const long total = (long)B * Ho * Wo * (C / 4);
    if (total == 0) return APE_OK;
    if (!x || !y || !code || !aligned16(x) || !aligned16(y) || ((uintptr_t)code & 3u)) return APE_EINVAL;
    hipLaunchKernelGGL(maxpool2x2_idx_kernel, dim3(ape::grid_for(total, kT, kGridCap)), dim3(kT), 0, (hipStream_t)stream, (const float4*)x, (float4*)y,
                       (uchar4*)code, B, H, W, C / 4, Ho, Wo);
    return ape::check_launch("ape_maxpool2x2_idx_nhwc_f32");
}

extern "C" int ape_max_unpool2x2_nhwc_f32(const float* y, const uint8_t* code, float* x, int B, int H, int W, int C, void* stream)
{
    if (window_check(B, H, W, C) != APE_OK) return APE_EINVAL;
    const int Ho = H / 2, Wo = W / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2;
    const long total = (long)B * Hc * Wc * (C / 4);
    if (total == 0) return APE_OK;
    if (!x || !aligned16(x)) return APE_EINVAL;
    if ((long)B * Ho * Wo > 0 && (!y || !code || !aligned16(y) || ((uintptr_t)code & 3u))) return APE_EINVAL;
    hipLaunchKernelGGL(max_unpool2x2_kernel, dim3(ape::grid_for(total, kT, kGridCap)), dim3(kT), 0, (hipStream_t)stream, (const float4*)y, (const uchar4*)code,
                       (float4*)x, B, H, W, C / 4, Ho, Wo, Hc, Wc);
    return ape::check_launch("ape_max_unpool2x2_nhwc_f32");
}

extern "C" int ape_gather2x2_nhwc_f32(const float* x, const uint8_t* code, float* y, int B, int H, int W, int C, void* stream)
{
    if (window_check(B, H, W, C) != APE_OK) return APE_EINVAL;
    const int Ho = H / 2, Wo = W / 2;
    const long total = (long)B * Ho * Wo * (C / 4);
    if (total == 0) return APE_OK;
    if (!x || !y || !code || !aligned16(x) || !aligned16(y) || ((uintptr_t)code & 3u)) return APE_EINVAL;
    hipLaunchKernelGGL(gather2x2_kernel, dim3(ape::grid_for(total, kT, kGridCap)), dim3(kT), 0, (hipStream_t)stream, (const float4*)x, (const uchar4*)code,
                       (float4*)y, B, H, W, C / 4, Ho, Wo);
    return ape::check_launch("ape_gather2x2_nhwc_f32");
}

static inline int ce_blocks(long P)
{
    const long g = (P + kT - 1) / kT;
    return (int)(g < 1 ? 1 : (g > kCeMaxBlocks ? kCeMaxBlocks : g));
}

extern "C" size_t ape_cross_entropy_workspace_bytes(long P)
{
    if (P < 0) return 0;
    return (size_t)ce_blocks(P) * 2 * sizeof(double) + 16;      // partials (sum, count) | the gradient's scale
}

extern "C" int ape_cross_entropy_f32(const float* logits, int ld, int C, const uint8_t* labels, long P, float g, double* out, float* dlogits,
                                     void* ws, size_t ws_bytes, void* stream)
{
    if (P < 0 || C < 1 || C > kCeMaxC || ld < C || !out || !ws || ((uintptr_t)ws & 7u) || ((uintptr_t)out & 7u)) return APE_EINVAL;
    if (P * (long)ld > (1L << 31)) return APE_EINVAL;
    if (P > 0 && (!logits || !labels)) return APE_EINVAL;
    if (ws_bytes < ape_cross_entropy_workspace_bytes(P)) return APE_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int nb = ce_blocks(P);
    double* part = (double*)ws;
    float* scale = (float*)(part + 2 * (size_t)nb);
    hipLaunchKernelGGL(ce_fwd_kernel, dim3(nb), dim3(kT), 0, st, logits, ld, C, labels, P, dlogits, part);
    hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(kT), 0, st, part, nb, P, g, out, scale);
    if (dlogits && P > 0) {
        const long n = P * (long)ld, n4 = aligned16(dlogits) ? n / 4 : 0;
        hipLaunchKernelGGL(ce_scale_kernel, dim3(ape::grid_for(n4 > 0 ? n4 : n, kT, kGridCap)), dim3(kT), 0, st, dlogits, n4, n, scale);
    }
    return ape::check_launch("ape_cross_entropy_f32");
}
