// The four pose errors of the YCB-Video toolbox, for every (ground-truth object, pose source) of a benchmark run in one call.
//   DenseFusion/replace_ycb_toolbox/evaluate_poses_keyframe.m:148-217 (transform_pts_Rt, add, adi, re, te)
//
// The toolbox builds a KD-tree over the estimated-posed model per object and source and asks it for the nearest neighbour of every
// ground-truth-posed model point (adi), in float64; YCB's models have ~2.6 k points each and are not of one length.  Here the search is the
// exhaustive one, in float64 throughout ((dx dx + dy dy) + dz dz, no FMA: the library is built with -ffp-contract=off), so the minimum
// is the minimum of the same numbers whatever the order they are visited in:
//
//   pose_points_kernel<S>   one workgroup per (instance-source pair, tile of 2 * 256 / S queries).  The estimated cloud R_est p + t_est is
//                           produced once per workgroup, chunk by chunk (kChunk points) into LDS as three float64 arrays (SoA: the S lanes of
//                           a query read S consecutive doubles -- 8-byte reads of consecutive addresses touch every bank once; at S = 1 the
//                           whole wave reads one address, a broadcast), so M has no upper limit.  A thread owns TWO queries: every reference
//                           point read from LDS (three ds_read_b64) feeds 2 x 9 float64 VALU operations.  S lanes share a query's references
//                           (r = s, s + S, ...) and merge their minima by wave shuffles; S grows while the call would leave the chip idle
//                           (the rule of ape_adds_dis_batched_f32 / ape_knn_f32).  The work index (pair, tile) is ONE 64-bit number walked by
//                           a grid-stride loop over blockIdx.x: no grid dimension limited to 65 535 carries it.
//   pose_finish_kernel      one workgroup per pair: the two means, re and te.
//
// Determinism, and the same bits for every S: the per-point distances do not depend on S (a minimum), and they are added in ONE order:
// per block of 512 consecutive model points thread t adds d[2 t] + d[2 t + 1], a wave adds by shfl_down 32..1, the four waves' sums are added
// in order; the blocks' sums are added in order.  At S = 1 a workgroup's tile IS such a block and it writes the block's two sums (16 bytes
// per 512 points of workspace); at S > 1 -- small calls only -- the per-point distances go to the workspace and pose_finish_kernel runs the
// same block sum over them.
//
// Work: sum over pairs of M^2 pair evaluations of 9 float64 operations; bytes: 24 M per workgroup from L2, 32 out per pair => float64 VALU bound.
#include "common.h"

namespace {

constexpr int kT = 256;
constexpr int kChunk = 1024;      // reference points per LDS chunk: 24 KB per workgroup, six workgroups (24 waves) per CU
constexpr int kQ = 2 * kT;        // queries per workgroup at one lane per query (kQ / S at S lanes); the block of the summation order

__device__ __forceinline__ void load_pose(const double* __restrict__ p, double R[9], double t[3])
{   // row-major 3 x 4
    R[0] = p[0]; R[1] = p[1]; R[2] = p[2]; t[0] = p[3];
    R[3] = p[4]; R[4] = p[5]; R[5] = p[6]; t[1] = p[7];
    R[6] = p[8]; R[7] = p[9]; R[8] = p[10]; t[2] = p[11];
}

// RT * [p; 1]: one spelling for both poses and for both uses of the estimated one, so that est == gt gives distances of exactly 0
__device__ __forceinline__ void apply(const double R[9], const double t[3], double x, double y, double z, double& ox, double& oy, double& oz)
{
    ox = ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
    oy = ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
    oz = ((R[6] * x + R[7] * y) + R[8] * z) + t[2];
}

// the class's rows of `models`, or false when the class or the table is not what the call declared (nothing is read or written then)
__device__ __forceinline__ bool model_span(const int* __restrict__ offsets, int n_models, long n_points, int c, int m_max, int& off, int& M)
{
    if (c < 0 || c >= n_models) return false;
    const int a = offsets[c], b = offsets[c + 1];
    if (a < 0 || b < a || (long)b > n_points || b - a > m_max) return false;
    off = a;
    M = b - a;
    return true;
}

// the block sum of the summation order, for two quantities at once; every thread gets both sums
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*red)[4])
{
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off);
        b += __shfl_down(b, off);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
}

template <int S>
__global__ __launch_bounds__(kT) void pose_points_kernel(const double* __restrict__ models, const int* __restrict__ offsets, int n_models,
                                                         long n_points, const int* __restrict__ cls, const double* __restrict__ rt_gt,
                                                         const double* __restrict__ rt_est, const unsigned char* __restrict__ valid, int n_src,
                                                         int m_max, int tiles_max, long total, double* __restrict__ ws)
{
    __shared__ double sx[kChunk], sy[kChunk], sz[kChunk];
    __shared__ double red[2][4];
    constexpr int G = kT / S;       // groups of S lanes; group g owns queries 2 g and 2 g + 1 of the tile
    const int s = threadIdx.x % S, g = threadIdx.x / S;
    for (long w = blockIdx.x; w < total; w += gridDim.x) {     // (everything up to the chunk loop is uniform over the workgroup)
        const long pair = w / tiles_max;
        const int tile = (int)(w - pair * tiles_max);
        if (!valid[pair]) continue;
        int off, M;
        if (!model_span(offsets, n_models, n_points, cls[pair / n_src], m_max, off, M)) continue;
        const int q0 = tile * (2 * G);
        if (q0 >= M) continue;
        double Rg[9], tg[3], Re[9], te[3];
        load_pose(rt_gt + (pair / n_src) * 12, Rg, tg);
        load_pose(rt_est + pair * 12, Re, te);
        const double* __restrict__ P = models + (long)off * 3;
        const int qa = q0 + 2 * g, qb = qa + 1;              // (neighbours: the waves past the model's end hold no query at all)
        const int ca = qa < M ? qa : M - 1, cb = qb < M ? qb : M - 1;
        const double pax = P[ca * 3], pay = P[ca * 3 + 1], paz = P[ca * 3 + 2];
        const double pbx = P[cb * 3], pby = P[cb * 3 + 1], pbz = P[cb * 3 + 2];
        double gax, gay, gaz, gbx, gby, gbz;
        apply(Rg, tg, pax, pay, paz, gax, gay, gaz);
        apply(Rg, tg, pbx, pby, pbz, gbx, gby, gbz);
        double besta = __builtin_inf(), bestb = __builtin_inf();
        for (int c0 = 0; c0 < M; c0 += kChunk) {
            const int n = M - c0 < kChunk ? M - c0 : kChunk;
            __syncthreads();                                   // the previous chunk (or work item) has been read
            for (int j = threadIdx.x; j < n; j += kT) {
                const double* p = P + (long)(c0 + j) * 3;
                apply(Re, te, p[0], p[1], p[2], sx[j], sy[j], sz[j]);
            }
            __syncthreads();
            if (qa < M) {                                      // a wave without a query skips the scan (the last tile of a model)
#pragma unroll 4
                for (int r = s; r < n; r += S) {
                    const double x = sx[r], y = sy[r], z = sz[r];
                    const double ax = x - gax, ay = y - gay, az = z - gaz;
                    const double bx = x - gbx, by = y - gby, bz = z - gbz;
                    const double da = (ax * ax + ay * ay) + az * az;
                    const double db = (bx * bx + by * by) + bz * bz;
                    besta = fmin(da, besta);                   // one v_min_f64 (a compare and two selects otherwise)
                    bestb = fmin(db, bestb);
                }
            }
        }
#pragma unroll
        for (int o = S / 2; o > 0; o >>= 1) {
            besta = fmin(__shfl_xor(besta, o), besta);
            bestb = fmin(__shfl_xor(bestb, o), bestb);
        }
        double eax, eay, eaz, ebx, eby, ebz;
        apply(Re, te, pax, pay, paz, eax, eay, eaz);
        apply(Re, te, pbx, pby, pbz, ebx, eby, ebz);
        const double ax = eax - gax, ay = eay - gay, az = eaz - gaz;
        const double bx = ebx - gbx, by = eby - gby, bz = ebz - gbz;
        const double adda = sqrt((ax * ax + ay * ay) + az * az), addb = sqrt((bx * bx + by * by) + bz * bz);
        const double adia = sqrt(besta), adib = sqrt(bestb);
        if (S == 1) {
            double vi = (qa < M ? adia : 0.0) + (qb < M ? adib : 0.0);
            double vd = (qa < M ? adda : 0.0) + (qb < M ? addb : 0.0);
            block_sum2(vi, vd, red);
            if (threadIdx.x == 0) {
                ws[w * 2] = vi;
                ws[w * 2 + 1] = vd;
            }
        } else if (s == 0) {
            double* d = ws + pair * m_max * 2;
            if (qa < M) { d[qa * 2] = adia; d[qa * 2 + 1] = adda; }
            if (qb < M) { d[qb * 2] = adib; d[qb * 2 + 1] = addb; }
        }
    }
}

// evaluate_poses_keyframe.m:195-207 with the general inverse (adjugate over determinant).  0.5 (trace(Re inv(Rg)) - 1) loses its digits to
// the subtraction near 0 degrees; there the same quantity is 1 + 0.5 trace((Re - Rg) inv(Rg)), whose only rounding sits in the small term:
// that spelling is taken on the near side (cosine above 0), the toolbox's on the far side, where it is the well-conditioned one.
__device__ __forceinline__ double rotation_error(const double Re[9], const double Rg[9])
{
    double A[9];
    A[0] = Rg[4] * Rg[8] - Rg[5] * Rg[7]; A[1] = Rg[2] * Rg[7] - Rg[1] * Rg[8]; A[2] = Rg[1] * Rg[5] - Rg[2] * Rg[4];
    A[3] = Rg[5] * Rg[6] - Rg[3] * Rg[8]; A[4] = Rg[0] * Rg[8] - Rg[2] * Rg[6]; A[5] = Rg[2] * Rg[3] - Rg[0] * Rg[5];
    A[6] = Rg[3] * Rg[7] - Rg[4] * Rg[6]; A[7] = Rg[1] * Rg[6] - Rg[0] * Rg[7]; A[8] = Rg[0] * Rg[4] - Rg[1] * Rg[3];
    const double det = (Rg[0] * A[0] + Rg[1] * A[3]) + Rg[2] * A[6];
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = A[i] / det;
    const double m00 = (Re[0] * A[0] + Re[1] * A[3]) + Re[2] * A[6];
    const double m11 = (Re[3] * A[1] + Re[4] * A[4]) + Re[5] * A[7];
    const double m22 = (Re[6] * A[2] + Re[7] * A[5]) + Re[8] * A[8];
    double c = 0.5 * (((m00 + m11) + m22) - 1.0);
    if (c > 0.0) {
        double D[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) D[i] = Re[i] - Rg[i];
        const double d00 = (D[0] * A[0] + D[1] * A[3]) + D[2] * A[6];
        const double d11 = (D[3] * A[1] + D[4] * A[4]) + D[5] * A[7];
        const double d22 = (D[6] * A[2] + D[7] * A[5]) + D[8] * A[8];
        c = 1.0 + 0.5 * ((d00 + d11) + d22);
    }
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);      // (a NaN stays a NaN)
    return 180.0 * acos(c) / 3.141592653589793;
}

__global__ __launch_bounds__(kT) void pose_finish_kernel(const int* __restrict__ offsets, int n_models, long n_points, const int* __restrict__ cls,
                                                         const double* __restrict__ rt_gt, const double* __restrict__ rt_est,
                                                         const unsigned char* __restrict__ valid, long n_pairs, int n_src, int m_max,
                                                         int tiles_max, int per_query, const double* __restrict__ ws, double* __restrict__ out)
{
    __shared__ double red[2][4];
    for (long pair = blockIdx.x; pair < n_pairs; pair += gridDim.x) {
        double* o = out + pair * 4;
        if (!valid[pair]) {
            if (threadIdx.x < 4) o[threadIdx.x] = __builtin_inf();
            continue;
        }
        int off, M;
        if (!model_span(offsets, n_models, n_points, cls[pair / n_src], m_max, off, M)) {
            if (threadIdx.x < 4) o[threadIdx.x] = __builtin_nan("");
            continue;
        }
        const int nb = (M + kQ - 1) / kQ;
        double si = 0.0, sd = 0.0;
        for (int b = 0; b < nb; ++b) {
            double vi, vd;
            if (per_query) {
                const double* d = ws + pair * m_max * 2;
                const int qa = b * kQ + 2 * threadIdx.x, qb = qa + 1;
                vi = (qa < M ? d[qa * 2] : 0.0) + (qb < M ? d[qb * 2] : 0.0);
                vd = (qa < M ? d[qa * 2 + 1] : 0.0) + (qb < M ? d[qb * 2 + 1] : 0.0);
                block_sum2(vi, vd, red);
            } else {
                vi = ws[(pair * tiles_max + b) * 2];
                vd = ws[(pair * tiles_max + b) * 2 + 1];
            }
            si += vi;
            sd += vd;
        }
        if (threadIdx.x == 0) {
            double Rg[9], tg[3], Re[9], te[3];
            load_pose(rt_gt + (pair / n_src) * 12, Rg, tg);
            load_pose(rt_est + pair * 12, Re, te);
            const double dx = tg[0] - te[0], dy = tg[1] - te[1], dz = tg[2] - te[2];
            o[0] = si / (double)M;                  // (M == 0: the mean of nothing, NaN)
            o[1] = sd / (double)M;
            o[2] = rotation_error(Re, Rg);
            o[3] = sqrt((dx * dx + dy * dy) + dz * dz);
        }
    }
}

constexpr long kFill = 256L * 8 * 64;      // lanes that fill 256 CUs (as ape_knn_f32 and ape_adds_dis_batched_f32 count them)
constexpr long kGridCap = 1L << 20;        // workgroups of a launch; the grid-stride loops take the rest

inline int choose_lanes(long n_pairs, int m_max)
{
    int S = 1;
    while (S < 64 && n_pairs * m_max * S < kFill && S * 4 <= m_max) S *= 4;
    return S;
}

inline int tiles_of(int m_max, int S) { return ape::ceil_div(m_max, kQ / S); }

}  // namespace

extern "C" int ape_pose_errors_chunk(void) { return kChunk; }
extern "C" int ape_pose_errors_queries(void) { return kQ; }

extern "C" int ape_pose_errors_lanes(long n_pairs, int m_max)
{
    if (n_pairs < 0 || m_max < 1) return APE_EINVAL;
    return choose_lanes(n_pairs, m_max);
}

extern "C" size_t ape_pose_errors_workspace_bytes(long n_pairs, int m_max)
{
    if (n_pairs <= 0 || m_max < 1) return 0;
    const int S = choose_lanes(n_pairs, m_max);
    const size_t rows = S == 1 ? (size_t)n_pairs * tiles_of(m_max, 1) : (size_t)n_pairs * m_max;
    return rows * 2 * sizeof(double);
}

extern "C" int ape_pose_errors_f64(const double* models, const int* offsets, int n_models, long n_points, const int* cls, const double* rt_gt,
                                   const double* rt_est, const unsigned char* valid, long n_inst, int n_src, int m_max, double* out,
                                   void* workspace, size_t workspace_bytes, void* stream)
{
    if (n_inst < 0 || n_src < 1 || n_models < 1 || n_points < 0 || m_max < 1 || n_inst > (1L << 40) / n_src) return APE_EINVAL;
    if (n_inst == 0) return APE_OK;
    if (!models || !offsets || !cls || !rt_gt || !rt_est || !valid || !out || !workspace || ((uintptr_t)workspace & 7)) return APE_EINVAL;
    const long n_pairs = n_inst * n_src;
    if (workspace_bytes < ape_pose_errors_workspace_bytes(n_pairs, m_max)) return APE_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int S = choose_lanes(n_pairs, m_max);
    const int tiles_max = tiles_of(m_max, S);
    const long total = n_pairs * tiles_max;
    const dim3 grid((unsigned)(total < kGridCap ? total : kGridCap));
    double* ws = (double*)workspace;
#define APE_POSE_POINTS(S_)                                                                                                                   \
    hipLaunchKernelGGL(pose_points_kernel<S_>, grid, dim3(kT), 0, st, models, offsets, n_models, n_points, cls, rt_gt, rt_est, valid, n_src, \
                       m_max, tiles_max, total, ws)
    switch (S) {
        case 1: APE_POSE_POINTS(1); break;
        case 4: APE_POSE_POINTS(4); break;
        case 16: APE_POSE_POINTS(16); break;
        default: APE_POSE_POINTS(64); break;
    }
#undef APE_POSE_POINTS
    hipLaunchKernelGGL(pose_finish_kernel, dim3((unsigned)(n_pairs < kGridCap ? n_pairs : kGridCap)), dim3(kT), 0, st, offsets, n_models,
                       n_points, cls, rt_gt, rt_est, valid, n_pairs, n_src, m_max, tiles_max, S == 1 ? 0 : 1, ws, out);
    return ape::check_launch("ape_pose_errors_f64");
}
