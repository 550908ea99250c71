// Kernels of the segmentor's training step (reference segmentation/__init__.py:134-156: model.train() -> smp Unet forward ->
// jaccard_loss -> IoU.add -> backward -> optimizer.step()).  What the DenseFusion tape (backward.hip) lacks for smp's Unet:
//
//   BatchNorm2d in train mode    batch statistics over B*H*W rows (fp64 partials around a per-channel shift, merged in a fixed order),
//                                running buffers updated on the device; fused apply  y = act(x_hat * gamma + beta [+ residual])
//   BatchNorm2d backward         ReLU mask from the saved output, sum(g) / sum(g * x_hat) per channel in one fixed-order reduction, dx
//   nearest x2 up-sample bwd     2x2 sums read from a channel slice (ld, offset) of the decoder's concatenation gradient
//   channel softmax fwd / bwd    smp's SegmentationHead activation (softmax over the NHWC channel axis)
//   Jaccard loss fwd / bwd       segmentation/utils.py:71-114 (softmax, or the swapped sigmoid pair for C == 1), on strided logits
//   confusion matrix             utils.py:139-196: arg-max (first maximum) + K x K histogram privatised in LDS, merged with u64 atomics
//   SGD, multi-tensor            torch.optim.SGD (momentum, dampening, weight decay, nesterov)
// Every float reduction that spans workgroups writes a partials slab reduced by a second pass in a fixed order (no float atomics), so
// two launches on the same inputs give the same bits.  Tensors are NHWC fp32 unless stated.
#include "common.h"

namespace {

constexpr int kT = 256;
constexpr int kGridCap = 65535;        // most workgroups of a grid-stride launch (ape::grid_for)
constexpr int kBnGroups = 1024;         // most row groups of the BN reductions (partials slab: kBnGroups x C x 2 doubles)

// ---- BatchNorm statistics -------------------------------------------------------------------------------------------------
// grid (C/64, groups); 4 row lanes x 64 channels.  Sums of d = x - shift (shift = x[0][c]) in fp64: a channel with mean 1e3 and std
// 1e-2 keeps its variance (sum(x^2) - n mean^2 would cancel it away).
__global__ __launch_bounds__(kT) void bn_stats_kernel(const float* __restrict__ x, double* __restrict__ part, long rows, int C,
                                                      long rows_per_group)
{
    __shared__ double red[2][4][64];
    const int cl = threadIdx.x & 63, g = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    const long r0 = (long)blockIdx.y * rows_per_group;
    long r1 = r0 + rows_per_group;
    r1 = r1 > rows ? rows : r1;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        const double sh = x[c];
        for (long r = r0 + g; r < r1; r += 4) {
            const double d = (double)x[r * C + c] - sh;
            s1 += d;
            s2 += d * d;
        }
    }
    red[0][g][cl] = s1;
    red[1][g][cl] = s2;
    __syncthreads();
    if (g == 0 && c < C) {
        double* o = part + ((long)blockIdx.y * C + c) * 2;
        o[0] = ((red[0][0][cl] + red[0][1][cl]) + red[0][2][cl]) + red[0][3][cl];
        o[1] = ((red[1][0][cl] + red[1][1][cl]) + red[1][2][cl]) + red[1][3][cl];
    }
}

// per channel: partials in group order -> mean, invstd (biased variance), running buffers (unbiased variance), num_batches_tracked
__global__ void bn_stats_finish_kernel(const float* __restrict__ x, const double* __restrict__ part, int groups, long rows, int C, float eps,
                                       float momentum, float* __restrict__ mean, float* __restrict__ invstd, float* __restrict__ run_mean,
                                       float* __restrict__ run_var, long long* __restrict__ nbt)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && nbt) nbt[0] += 1;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int g = 0; g < groups; ++g) {
        s1 += part[((long)g * C + c) * 2];
        s2 += part[((long)g * C + c) * 2 + 1];
    }
    const double n = (double)rows, md = s1 / n;
    double var = s2 / n - md * md;
    var = var < 0.0 ? 0.0 : var;
    const double mud = (double)x[c] + md;
    const float mu = (float)mud;
    mean[c] = mu;                       // mean as a float pair: x - hi - lo keeps x_hat exact for a large mean over a small spread
    mean[C + c] = (float)(mud - (double)mu);
    invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (run_mean) run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mu;
    if (run_var) run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)(var * n / (n - 1.0));
}

// y = act((x - mean) * invstd * gamma + beta [+ res])
__global__ void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ invstd,
                                const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ res,
                                float* __restrict__ y, long total, int C, int relu)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        float v = ((x[i] - mean[c]) - mean[C + c]) * invstd[c] * gamma[c] + beta[c];
        if (res) v += res[i];
        y[i] = relu ? (v > 0.f ? v : 0.f) : v;
    }
}

// ---- BatchNorm backward ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bn_g(const float* dy, const float* y, long i) { return (y && !(y[i] > 0.f)) ? 0.f : dy[i]; }

// part[g][c] = (sum g, sum g * x_hat) over the group's rows, g = dy masked by the saved output (y > 0) when y is given
__global__ __launch_bounds__(kT) void bn_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                           const float* __restrict__ x, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, double* __restrict__ part, long rows,
                                                           int C, long rows_per_group)
{
    __shared__ double red[2][4][64];
    const int cl = threadIdx.x & 63, g = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    const long r0 = (long)blockIdx.y * rows_per_group;
    long r1 = r0 + rows_per_group;
    r1 = r1 > rows ? rows : r1;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        const float mu = mean[c], mlo = mean[C + c], is = invstd[c];
        for (long r = r0 + g; r < r1; r += 4) {
            const long i = r * C + c;
            const float gv = bn_g(dy, y, i);
            s1 += gv;
            s2 += (double)gv * (double)(((x[i] - mu) - mlo) * is);
        }
    }
    red[0][g][cl] = s1;
    red[1][g][cl] = s2;
    __syncthreads();
    if (g == 0 && c < C) {
        double* o = part + ((long)blockIdx.y * C + c) * 2;
        o[0] = ((red[0][0][cl] + red[0][1][cl]) + red[0][2][cl]) + red[0][3][cl];
        o[1] = ((red[1][0][cl] + red[1][1][cl]) + red[1][2][cl]) + red[1][3][cl];
    }
}

// dbeta = sum g, dgamma = sum g x_hat; coef[c] = (sum g / n, sum g x_hat / n) for the dx pass
__global__ void bn_bwd_finish_kernel(const double* __restrict__ part, int groups, long rows, int C, float* __restrict__ dgamma,
                                     float* __restrict__ dbeta, float* __restrict__ coef)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int g = 0; g < groups; ++g) {
        s1 += part[((long)g * C + c) * 2];
        s2 += part[((long)g * C + c) * 2 + 1];
    }
    if (dbeta) dbeta[c] = (float)s1;
    if (dgamma) dgamma[c] = (float)s2;
    coef[2 * c] = (float)(s1 / (double)rows);
    coef[2 * c + 1] = (float)(s2 / (double)rows);
}

// dx = gamma * invstd * (g - mean(g) - x_hat * mean(g x_hat)); dres = g
__global__ void bn_bwd_dx_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x,
                                 const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
                                 const float* __restrict__ coef, float* __restrict__ dx, float* __restrict__ dres, long total, int C)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const float gv = bn_g(dy, y, i);
        if (dres) dres[i] = gv;
        if (dx) {
            const float xh = ((x[i] - mean[c]) - mean[C + c]) * invstd[c];
            dx[i] = gamma[c] * invstd[c] * ((gv - coef[2 * c]) - xh * coef[2 * c + 1]);
        }
    }
}

// ---- nearest x2 up-sample backward ----------------------------------------------------------------------------------------
// dx[b][h][w][c] = sum_{i,j < 2} dy[b][2h+i][2w+j][off + c]   (dy row pitch ld)
__global__ void upsample2x_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int B, int h, int w, int C, int ld, int off)
{
    const long total = (long)B * h * w * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long p = i / C;
        const int xw = (int)(p % w);
        p /= w;
        const int xh = (int)(p % h);
        const long b = p / h;
        const long W2 = 2L * w;
        const long r0 = ((b * 2 * h + 2 * xh) * W2 + 2 * xw) * ld + off + c;
        const long r1 = r0 + W2 * ld;
        dx[i] = (dy[r0] + dy[r0 + ld]) + (dy[r1] + dy[r1 + ld]);
    }
}

// ---- channel softmax (NHWC rows) ------------------------------------------------------------------------------------------
__global__ void softmax_rows_kernel(const float* __restrict__ x, float* __restrict__ y, long rows, int C)
{
    for (long r = blockIdx.x * (long)blockDim.x + threadIdx.x; r < rows; r += (long)gridDim.x * blockDim.x) {
        const float* xr = x + r * C;
        float m = xr[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, xr[c]);
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(xr[c] - m);
        const float inv = 1.f / s;
        for (int c = 0; c < C; ++c) y[r * C + c] = expf(xr[c] - m) * inv;
    }
}

// dx = y * (dy - sum(dy * y))
__global__ void softmax_rows_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dx, long rows, int C)
{
    for (long r = blockIdx.x * (long)blockDim.x + threadIdx.x; r < rows; r += (long)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += dy[r * C + c] * y[r * C + c];
        for (int c = 0; c < C; ++c) dx[r * C + c] = y[r * C + c] * (dy[r * C + c] - s);
    }
}

// ---- Jaccard loss ---------------------------------------------------------------------------------------------------------
// logits[b][c][h][w] at element strides st[0..3]; labels i64 [B*H*W].  K = loss channels (C, or 2 for C == 1: probas = [sigmoid,
// 1 - sigmoid], one-hot = [t == 1, t == 0], utils.py:87-94).  The reference sums over dims (0,) + range(2, true.ndim) (utils.py:100):
// over (B, H, W) for [B,1,H,W] labels, but over (B, H) only for [B,H,W] labels -- one intersection / cardinality per (class, column w),
// all of them averaged.  `ncol` = W in that case (slot = column), 1 otherwise; the loss restates both.
constexpr int kJacMax = 32;
struct Strides4 { long s[4]; };

__device__ __forceinline__ const float* jac_px(const float* logits, const Strides4& st, long p, int H, int W)
{
    const int w = (int)(p % W);
    const long q = p / W;
    const int h = (int)(q % H);
    const long b = q / H;
    return logits + b * st.s[0] + (long)h * st.s[2] + (long)w * st.s[3];
}

// probabilities of one pixel into pr[kJacMax] (softmax in fp32 as F.softmax, or the sigmoid pair)
__device__ __forceinline__ void jac_probs(const float* xp, long sc, int C, float* pr)
{
    if (C == 1) {
        const float s = 1.f / (1.f + expf(-xp[0]));
        pr[0] = s;
        pr[1] = 1.f - s;
        return;
    }
    float m = xp[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, xp[c * sc]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < kJacMax; ++c)
        if (c < C) { pr[c] = expf(xp[c * sc] - m); s += pr[c]; }
    const float inv = 1.f / s;
#pragma unroll
    for (int c = 0; c < kJacMax; ++c)
        if (c < C) pr[c] *= inv;
}

// the loss channel of label t (-1: out of range)
__device__ __forceinline__ int jac_cls(long long t, int C)
{
    if (C == 1) return t == 1 ? 0 : (t == 0 ? 1 : -1);
    return (t >= 0 && t < C) ? (int)t : -1;
}

// flat pixel index of the i-th pixel of slot s
__device__ __forceinline__ long jac_flat(long i, int s, int ncol) { return ncol == 1 ? i : i * ncol + s; }

// grid (groups, ncol): part[(s * groups + g) * K + k] = (sum p_k t_k, sum p_k, sum t_k) over the group's pixels of slot s;
// flags[0] |= presence bit of every label value, flags[1] |= 1 on an out-of-range label
__global__ __launch_bounds__(kT) void jaccard_fwd_kernel(const float* __restrict__ logits, Strides4 st, const long long* __restrict__ labels,
                                                         long per_slot, int ncol, int H, int W, int C, double* __restrict__ part,
                                                         unsigned* __restrict__ flags)
{
    __shared__ float red[3][kT / 64][kJacMax];
    const int K = C == 1 ? 2 : C, slot = blockIdx.y, groups = gridDim.x;
    float ai[kJacMax], ap[kJacMax], at[kJacMax], pr[kJacMax];
#pragma unroll
    for (int k = 0; k < kJacMax; ++k) { ai[k] = 0.f; ap[k] = 0.f; at[k] = 0.f; pr[k] = 0.f; }
    unsigned present = 0u, bad = 0u;
    for (long i = blockIdx.x * (long)kT + threadIdx.x; i < per_slot; i += (long)groups * kT) {
        const long p = jac_flat(i, slot, ncol);
        const long long t = labels[p];
        const int tc = jac_cls(t, C);
        if (t >= 0 && t < 32) present |= 1u << (int)t;
        if (tc < 0) { bad = 1u; continue; }
        jac_probs(jac_px(logits, st, p, H, W), st.s[1], C, pr);
#pragma unroll
        for (int k = 0; k < kJacMax; ++k)
            if (k < K) {
                ap[k] += pr[k];
                ai[k] += k == tc ? pr[k] : 0.f;
                at[k] += k == tc ? 1.f : 0.f;
            }
    }
    // presence / range flags: integer atomics (order-free)
    for (int o = 32; o > 0; o >>= 1) { present |= __shfl_xor(present, o); bad |= __shfl_xor(bad, o); }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        if (present) atomicOr(flags, present);
        if (bad) atomicOr(flags + 1, 1u);
    }
#pragma unroll
    for (int k = 0; k < kJacMax; ++k)
        if (k < K) {
            float a = ai[k], b = ap[k], c = at[k];
            for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); c += __shfl_xor(c, o); }
            if (lane == 0) { red[0][wave][k] = a; red[1][wave][k] = b; red[2][wave][k] = c; }
        }
    __syncthreads();
    if (threadIdx.x < K) {
        const int k = threadIdx.x;
        double* o = part + (((long)slot * groups + blockIdx.x) * K + k) * 3;
        for (int j = 0; j < 3; ++j) {
            double sum = 0.0;
            for (int wv = 0; wv < kT / 64; ++wv) sum += (double)red[j][wv][k];
            o[j] = sum;
        }
    }
}

// one workgroup: loss[0] = 1 - mean over (label values v present, slots s) of I / (S - I + eps)  (NaN with an out-of-range label);
// coef[(s * K + k) * 2 + {0, 1}] = (a, b) with dloss / dp_k(pixel of slot s) = t_k a + b
__global__ __launch_bounds__(kT) void jaccard_finish_kernel(const double* __restrict__ part, int groups, int ncol, int C, float eps,
                                                            const unsigned* __restrict__ flags, float* __restrict__ loss,
                                                            float* __restrict__ coef)
{
    __shared__ double red[kT];
    const int K = C == 1 ? 2 : C;
    const unsigned present = flags[0];
    int np = 0;
    for (int k = 0; k < K; ++k) np += (present >> k) & 1u;
    const double inv = -1.0 / ((double)np * (double)ncol);
    double jsum = 0.0;
    for (int e = threadIdx.x; e < K * ncol; e += kT) {
        const int sl = e / K, k = e % K;
        double si = 0.0, sp = 0.0, stt = 0.0;
        for (int g = 0; g < groups; ++g) {
            const double* q = part + (((long)sl * groups + g) * K + k) * 3;
            si += q[0];
            sp += q[1];
            stt += q[2];
        }
        const float I = (float)si, S = (float)(sp + stt);          // fp32 like the reference's sums
        const float U = S - I + eps;
        const bool on = (present >> k) & 1u;
        if (on) jsum += (double)(I / U);
        const double u = (double)U, f = on ? inv : 0.0;
        coef[2 * e] = (float)(f * (1.0 / u + (double)I / (u * u)));
        coef[2 * e + 1] = (float)(f * (-(double)I / (u * u)));
    }
    red[threadIdx.x] = jsum;
    __syncthreads();
    for (int o = kT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        loss[0] = flags[1] ? __int_as_float(0x7fc00000) : (float)(1.0 - red[0] / ((double)np * (double)ncol));
}

// dlogits through the softmax (sigmoid) Jacobian, written in the logits' own strides; gscale = upstream gradient (device scalar)
__global__ __launch_bounds__(kT) void jaccard_bwd_kernel(const float* __restrict__ logits, Strides4 st, const long long* __restrict__ labels,
                                                         long npix, int ncol, int H, int W, int C, const float* __restrict__ coef,
                                                         const unsigned* __restrict__ flags, const float* __restrict__ gscale,
                                                         float* __restrict__ dlogits, Strides4 dst)
{
    float pr[kJacMax];
#pragma unroll
    for (int k = 0; k < kJacMax; ++k) pr[k] = 0.f;
    const int K = C == 1 ? 2 : C;
    const float gs = gscale[0];
    const bool bad = flags[1] != 0u;
    for (long p = blockIdx.x * (long)kT + threadIdx.x; p < npix; p += (long)gridDim.x * kT) {
        const int tc = jac_cls(labels[p], C);
        float* dp = (float*)jac_px(dlogits, dst, p, H, W);
        if (tc < 0 || bad) {
            for (int c = 0; c < C; ++c) dp[c * dst.s[1]] = __int_as_float(0x7fc00000);
            continue;
        }
        const float* cf = coef + (ncol == 1 ? 0 : (long)(p % W) * K * 2);
        jac_probs(jac_px(logits, st, p, H, W), st.s[1], C, pr);
        if (C == 1) {
            const float q0 = (tc == 0 ? cf[0] : 0.f) + cf[1], q1 = (tc == 1 ? cf[2] : 0.f) + cf[3];
            dp[0] = gs * (pr[0] * pr[1] * (q0 - q1));
            continue;
        }
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < kJacMax; ++k)
            if (k < C) s += pr[k] * ((k == tc ? cf[2 * k] : 0.f) + cf[2 * k + 1]);
#pragma unroll
        for (int k = 0; k < kJacMax; ++k)
            if (k < C) dp[k * dst.s[1]] = gs * (pr[k] * (((k == tc ? cf[2 * k] : 0.f) + cf[2 * k + 1]) - s));
    }
}

// ---- confusion matrix ------------------------------------------------------------------------------------------------------
constexpr int kConfMax = 64;

// class of pixel p: scores (arg-max over K at strides st, first maximum; NaN counts as the maximum like numpy.argmax) or an i64 label
__device__ __forceinline__ long long conf_cls(const float* scores, const Strides4& st, const long long* labels, long p, int H, int W, int K)
{
    if (!scores) return labels[p];
    const float* xp = jac_px(scores, st, p, H, W);
    float best = xp[0];
    int bi = 0;
    for (int k = 1; k < K; ++k) {
        const float v = xp[k * st.s[1]];
        if (best != best) break;
        if (v > best || v != v) { best = v; bi = k; }
    }
    return bi;
}

__global__ __launch_bounds__(kT) void confusion_kernel(const float* __restrict__ pred_scores, Strides4 pst, const long long* __restrict__ pred_labels,
                                                       const float* __restrict__ tgt_scores, Strides4 tst, const long long* __restrict__ tgt_labels,
                                                       long npix, int H, int W, int K, unsigned long long* __restrict__ conf,
                                                       unsigned* __restrict__ bad)
{
    __shared__ unsigned hist[kConfMax * kConfMax];
    for (int i = threadIdx.x; i < K * K; i += kT) hist[i] = 0u;
    __syncthreads();
    unsigned nbad = 0u;
    for (long p = blockIdx.x * (long)kT + threadIdx.x; p < npix; p += (long)gridDim.x * kT) {
        const long long pc = conf_cls(pred_scores, pst, pred_labels, p, H, W, K);
        const long long tc = conf_cls(tgt_scores, tst, tgt_labels, p, H, W, K);
        if (pc < 0 || pc >= K || tc < 0 || tc >= K) { nbad = 1u; continue; }
        atomicAdd(&hist[tc * K + pc], 1u);          // rows = target, columns = prediction (utils.py:187-190)
    }
    if (nbad) atomicOr(bad, 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < K * K; i += kT)
        if (hist[i]) atomicAdd(conf + i, (unsigned long long)hist[i]);
}

// ---- SGD ------------------------------------------------------------------------------------------------------------------
constexpr int kSgdJobs = 64;
struct SgdBatch { ape_sgd_job j[kSgdJobs]; };
__global__ void sgd_multi_kernel(const SgdBatch b, float lr, float momentum, float dampening, float wd, int nesterov)
{
    const ape_sgd_job& a = b.j[blockIdx.y];
    float* __restrict__ p = a.param;
    const float* __restrict__ g = a.grad;
    float* __restrict__ buf = a.momentum_buffer;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < a.n; i += (long)gridDim.x * blockDim.x) {
        float d = g[i];
        if (wd != 0.f) d += wd * p[i];
        if (buf) {
            const float bv = a.first ? d : momentum * buf[i] + (1.f - dampening) * d;
            buf[i] = bv;
            d = nesterov ? d + momentum * bv : bv;
        }
        p[i] -= lr * d;
    }
}

// row groups: ~2048 workgroups over the channel tiles, >= 256 rows each; the group count depends on the shape only (deterministic)
static inline long rows_per(long rows, int C, int* groups)
{
    const int ct = ape::ceil_div(C, 64);
    long g = (rows + 255) / 256;
    const long want = 2048 / ct;
    g = g > want ? want : g;
    g = g > kBnGroups ? kBnGroups : (g < 1 ? 1 : g);
    *groups = (int)g;
    return (rows + g - 1) / g;
}

static inline Strides4 mk_strides(const long* s) { Strides4 r; for (int i = 0; i < 4; ++i) r.s[i] = s[i]; return r; }

}  // namespace

extern "C" size_t ape_bn_workspace_bytes(int C)
{
    return C < 1 ? 0 : (size_t)kBnGroups * C * 2 * sizeof(double);
}

extern "C" int ape_bn_train_fwd_f32(const float* x, const float* gamma, const float* beta, const float* residual, float* y, float* mean,
                                    float* invstd, float* running_mean, float* running_var, long long* num_batches_tracked, long rows,
                                    int C, float eps, float momentum, int act, void* ws, size_t ws_bytes, void* stream)
{
    if (!x || !gamma || !beta || !y || !mean || !invstd || !ws || C < 1 || rows < 2 || !(eps > 0.f) || (act != APE_ACT_NONE && act != APE_ACT_RELU))
        return APE_EINVAL;
    if (ws_bytes < ape_bn_workspace_bytes(C)) return APE_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int groups;
    const long rpg = rows_per(rows, C, &groups);
    double* part = (double*)ws;
    hipLaunchKernelGGL(bn_stats_kernel, dim3(ape::ceil_div(C, 64), groups), dim3(kT), 0, st, x, part, rows, C, rpg);
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3(ape::ceil_div(C, 64)), dim3(64), 0, st, x, part, groups, rows, C, eps, momentum, mean,
                       invstd, running_mean, running_var, num_batches_tracked);
    const long total = rows * C;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(ape::grid_for(total, kT, kGridCap)), dim3(kT), 0, st, x, mean, invstd, gamma, beta, residual, y, total, C,
                       act == APE_ACT_RELU ? 1 : 0);
    return ape::check_launch("ape_bn_train_fwd_f32");
}

extern "C" int ape_bn_train_bwd_f32(const float* dy, const float* y, const float* x, const float* mean, const float* invstd, const float* gamma,
                                    float* dx, float* dgamma, float* dbeta, float* dres, long rows, int C, void* ws, size_t ws_bytes, void* stream)
{
    if (!dy || !x || !mean || !invstd || !gamma || !ws || C < 1 || rows < 1) return APE_EINVAL;
    if (ws_bytes < ape_bn_workspace_bytes(C) + (size_t)C * 2 * sizeof(float)) return APE_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int groups;
    const long rpg = rows_per(rows, C, &groups);
    double* part = (double*)ws;
    float* coef = (float*)((char*)ws + ape_bn_workspace_bytes(C));
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(ape::ceil_div(C, 64), groups), dim3(kT), 0, st, dy, y, x, mean, invstd, part, rows, C, rpg);
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3(ape::ceil_div(C, 64)), dim3(64), 0, st, part, groups, rows, C, dgamma, dbeta, coef);
    if (dx || dres) {
        const long total = rows * C;
        hipLaunchKernelGGL(bn_bwd_dx_kernel, dim3(ape::grid_for(total, kT, kGridCap)), dim3(kT), 0, st, dy, y, x, mean, invstd, gamma, coef, dx, dres, total, C);
    }
    return ape::check_launch("ape_bn_train_bwd_f32");
}

extern "C" int ape_upsample_nearest2x_bwd_f32(const float* dy, int ld, int off, float* dx, int B, int h, int w, int C, void* stream)
{
    if (!dy || !dx || B < 0 || h < 1 || w < 1 || C < 1 || off < 0 || off + C > ld) return APE_EINVAL;
    const long total = (long)B * h * w * C;
    if (total == 0) return APE_OK;
    hipLaunchKernelGGL(upsample2x_bwd_kernel, dim3(ape::grid_for(total, kT, kGridCap)), dim3(kT), 0, (hipStream_t)stream, dy, dx, B, h, w, C, ld, off);
    return ape::check_launch("ape_upsample_nearest2x_bwd_f32");
}

extern "C" int ape_softmax_rows_f32(const float* x, float* y, long rows, int C, void* stream)
{
    if (!x || !y || rows < 0 || C < 1) return APE_EINVAL;
    if (rows == 0) return APE_OK;
    hipLaunchKernelGGL(softmax_rows_kernel, dim3(ape::grid_for(rows, kT, kGridCap)), dim3(kT), 0, (hipStream_t)stream, x, y, rows, C);
    return ape::check_launch("ape_softmax_rows_f32");
}

extern "C" int ape_softmax_rows_bwd_f32(const float* dy, const float* y, float* dx, long rows, int C, void* stream)
{
    if (!dy || !y || !dx || rows < 0 || C < 1) return APE_EINVAL;
    if (rows == 0) return APE_OK;
    hipLaunchKernelGGL(softmax_rows_bwd_kernel, dim3(ape::grid_for(rows, kT, kGridCap)), dim3(kT), 0, (hipStream_t)stream, dy, y, dx, rows, C);
    return ape::check_launch("ape_softmax_rows_bwd_f32");
}

// row groups per slot of the Jaccard partials: about 256 workgroups in all (a shape-only choice: deterministic)
static inline int jac_groups(long per_slot, int ncol)
{
    long g = (per_slot + kT - 1) / kT, want = 256 / ncol;
    g = g > want ? want : g;
    return (int)(g < 1 ? 1 : g);
}

extern "C" size_t ape_jaccard_workspace_bytes(int C, int ncol)
{
    if (C < 1 || ncol < 1) return 0;
    const int K = C == 1 ? 2 : C;
    const size_t blocks = ncol > 256 ? (size_t)ncol : 256;          // slots x groups <= max(ncol, 256)
    return blocks * K * 3 * sizeof(double) + (size_t)2 * K * ncol * sizeof(float) + 2 * sizeof(unsigned);
}

static int jac_check(const float* logits, const long* st, const long long* labels, int B, int C, int H, int W, int ncol, void* ws)
{
    if (!logits || !st || !labels || !ws || B < 1 || H < 1 || W < 1 || C < 1 || C > kJacMax || (ncol != 1 && ncol != W)) return APE_EINVAL;
    for (int i = 0; i < 4; ++i)
        if (st[i] < 0) return APE_EINVAL;
    return APE_OK;
}

extern "C" int ape_jaccard_fwd_f32(const float* logits, const long* strides_host, const long long* labels, int B, int C, int H, int W,
                                   int ncol, float eps, float* loss, void* ws, size_t ws_bytes, void* stream)
{
    if (jac_check(logits, strides_host, labels, B, C, H, W, ncol, ws) || !loss) return APE_EINVAL;
    if (ws_bytes < ape_jaccard_workspace_bytes(C, ncol)) return APE_EWORKSPACE;
    const int K = C == 1 ? 2 : C;
    hipStream_t st = (hipStream_t)stream;
    const size_t blocks = ncol > 256 ? (size_t)ncol : 256;
    double* part = (double*)ws;
    float* coef = (float*)(part + blocks * K * 3);
    unsigned* flags = (unsigned*)(coef + (size_t)2 * K * ncol);
    if (hipMemsetAsync(flags, 0, 2 * sizeof(unsigned), st) != hipSuccess) { ape::set_last_error("hipMemsetAsync"); return APE_ELAUNCH; }
    const long per_slot = (long)B * H * W / ncol;
    const int groups = jac_groups(per_slot, ncol);
    hipLaunchKernelGGL(jaccard_fwd_kernel, dim3(groups, ncol), dim3(kT), 0, st, logits, mk_strides(strides_host), labels, per_slot, ncol, H, W,
                       C, part, flags);
    hipLaunchKernelGGL(jaccard_finish_kernel, dim3(1), dim3(kT), 0, st, part, groups, ncol, C, eps, flags, loss, coef);
    return ape::check_launch("ape_jaccard_fwd_f32");
}

extern "C" int ape_jaccard_bwd_f32(const float* logits, const long* strides_host, const long long* labels, int B, int C, int H, int W,
                                   int ncol, const float* gscale, float* dlogits, const long* dstrides_host, const void* ws, size_t ws_bytes,
                                   void* stream)
{
    if (jac_check(logits, strides_host, labels, B, C, H, W, ncol, (void*)ws) || !gscale || !dlogits || !dstrides_host) return APE_EINVAL;
    if (ws_bytes < ape_jaccard_workspace_bytes(C, ncol)) return APE_EWORKSPACE;
    const int K = C == 1 ? 2 : C;
    const size_t blocks = ncol > 256 ? (size_t)ncol : 256;
    const float* coef = (const float*)((const double*)ws + blocks * K * 3);
    const unsigned* flags = (const unsigned*)(coef + (size_t)2 * K * ncol);
    const long npix = (long)B * H * W;
    int groups = ape::grid_for(npix, kT, kGridCap);
    groups = groups > 4096 ? 4096 : groups;
    hipLaunchKernelGGL(jaccard_bwd_kernel, dim3(groups), dim3(kT), 0, (hipStream_t)stream, logits, mk_strides(strides_host), labels, npix, ncol,
                       H, W, C, coef, flags, gscale, dlogits, mk_strides(dstrides_host));
    return ape::check_launch("ape_jaccard_bwd_f32");
}

extern "C" int ape_confusion_add(const float* pred_scores, const long* pred_strides_host, const long long* pred_labels, const float* tgt_scores,
                                 const long* tgt_strides_host, const long long* tgt_labels, int B, int H, int W, int K,
                                 unsigned long long* conf, unsigned* bad_flag, void* stream)
{
    if ((!pred_scores == !pred_labels) || (!tgt_scores == !tgt_labels) || (pred_scores && !pred_strides_host) || (tgt_scores && !tgt_strides_host)
        || !conf || !bad_flag || B < 0 || H < 1 || W < 1 || K < 1 || K > kConfMax)
        return APE_EINVAL;
    const long npix = (long)B * H * W;
    if (npix == 0) return APE_OK;
    const long zero[4] = {0, 0, 0, 0};
    int groups = ape::grid_for(npix, kT, kGridCap);
    groups = groups > 1024 ? 1024 : groups;
    hipLaunchKernelGGL(confusion_kernel, dim3(groups), dim3(kT), 0, (hipStream_t)stream, pred_scores,
                       mk_strides(pred_scores ? pred_strides_host : zero), pred_labels, tgt_scores, mk_strides(tgt_scores ? tgt_strides_host : zero),
                       tgt_labels, npix, H, W, K, conf, bad_flag);
    return ape::check_launch("ape_confusion_add");
}

extern "C" int ape_sgd_step_multi_f32(int n, const ape_sgd_job* jobs, float lr, float momentum, float dampening, float weight_decay,
                                      int nesterov, void* stream)
{
    if (n < 0 || (n && !jobs) || !(lr >= 0.f) || !(momentum >= 0.f) || (nesterov && (momentum <= 0.f || dampening != 0.f))) return APE_EINVAL;
    for (int i = 0; i < n; ++i)
        if (!jobs[i].param || !jobs[i].grad || jobs[i].n < 0 || (momentum != 0.f && !jobs[i].momentum_buffer)) return APE_EINVAL;
    for (int i0 = 0; i0 < n; i0 += kSgdJobs) {
        SgdBatch b{};
        const int nb = n - i0 < kSgdJobs ? n - i0 : kSgdJobs;
        long nmax = 1;
        for (int i = 0; i < nb; ++i) {
            b.j[i] = jobs[i0 + i];
            if (momentum == 0.f) b.j[i].momentum_buffer = nullptr;
            nmax = jobs[i0 + i].n > nmax ? jobs[i0 + i].n : nmax;
        }
        int gx = ape::grid_for(nmax, kT, kGridCap);
        gx = gx > 256 ? 256 : gx;
        hipLaunchKernelGGL(sgd_multi_kernel, dim3(gx, nb), dim3(kT), 0, (hipStream_t)stream, b, lr, momentum, dampening, weight_decay, nesterov);
    }
    return ape::check_launch("ape_sgd_step_multi_f32");
}
