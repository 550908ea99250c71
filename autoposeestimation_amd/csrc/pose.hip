// Pose extraction / re-centring / refinement composition on the device (no host round trips):
//   pose_select   DenseFusion/tools/utils.py:7-18 (my_estimator_prediction) + :43-86 (get_new_points):
//                 which = argmax_n c (first maximum), q = r[which]/|r[which]|, t = points[which] + t[which],
//                 new_points = (points - t) . R(q)   with R's nine terms exactly as written at utils.py:46-67
//   pose_compose  tools/utils.py:20-40 (my_refined_prediction) with lib/transformations.py:1254-1278
//                 (quaternion_matrix) and :1320-1341,1361-1363 (quaternion_from_matrix, isprecise=True): float64
//   pose_recentre DenseFusion/tools/eval_ycb.py:205-210 (iterative refinement: cloud re-centred with the CURRENT pose,
//                 R and T rounded to float32 as `.astype(np.float32)` does there)
// The reference pulls 7 floats to the host after the estimator and after the refiner (two device syncs per object);
// here the pose stays in HBM as [B][7] float64 (w,x,y,z, tx,ty,tz) until the caller asks for it.
#include "common.h"
#include "pose_quat.h"

namespace {

// nine terms of the rotation "base" exactly as the reference spells them (float32)
__device__ __forceinline__ void quat_base(float w, float x, float y, float z, float R[9])
{
    R[0] = 1.0f - 2.0f * (y * y + z * z);
    R[1] = 2.0f * x * y - 2.0f * w * z;
    R[2] = 2.0f * w * y + 2.0f * x * z;
    R[3] = 2.0f * x * y + 2.0f * z * w;
    R[4] = 1.0f - 2.0f * (x * x + z * z);
    R[5] = -2.0f * w * x + 2.0f * y * z;
    R[6] = -2.0f * w * y + 2.0f * x * z;
    R[7] = 2.0f * w * x + 2.0f * y * z;
    R[8] = 1.0f - 2.0f * (x * x + y * y);
}

constexpr int kSelThreads = 256;     // workgroup of the per-crop kernels below; the arg-max's candidate order is tied to it
constexpr int kNoIndex = 0x7fffffff;

// one thread's running (maximum, index) over ITS rows, visited in ascending order: the first maximum is kept; a NaN is kept only as the
// thread's first value (nothing compares greater than it afterwards)
__device__ __forceinline__ void argmax_take(float c, int i, float& best, int& bi)
{
    if (c > best || bi == kNoIndex) { best = c; bi = i; }
}

// the workgroup's first maximum from the kSelThreads per-thread candidates (value in sc[], index in si[]): returns the index to every
// thread, its value stays in sc[0]
__device__ __forceinline__ int argmax_reduce(float best, int bi, float* sc, int* si)
{
    sc[threadIdx.x] = best;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int off = kSelThreads / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            const float oc = sc[threadIdx.x + off];
            const int oi = si[threadIdx.x + off];
            if (oi != kNoIndex && (si[threadIdx.x] == kNoIndex || oc > sc[threadIdx.x] || (oc == sc[threadIdx.x] && oi < si[threadIdx.x]))) {
                sc[threadIdx.x] = oc;
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    return si[0];
}

// everything after the arg-max: h = the selected row's (r0..r3, t0..t2), w its index.  Thread 0 normalises the quaternion, places the
// translation and writes the pose; then the whole workgroup re-centres the crop's cloud (when new_points is asked for).
// points / new_points: this crop's n rows.
__device__ __forceinline__ void pose_from_heads(const float* h, int w, const float4* __restrict__ points, double* __restrict__ po,
                                                float4* __restrict__ new_points, int n, float* sR, float* st)
{
    if (threadIdx.x == 0) {
        const float nrm = sqrtf(((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]) + h[3] * h[3]);
        const float q0 = h[0] / nrm, q1 = h[1] / nrm, q2 = h[2] / nrm, q3 = h[3] / nrm;
        const float4 p = points[w];
        st[0] = p.x + h[4]; st[1] = p.y + h[5]; st[2] = p.z + h[6];   // (points + pred_t)[which]
        quat_base(q0, q1, q2, q3, sR);
        po[0] = q0; po[1] = q1; po[2] = q2; po[3] = q3;
        po[4] = st[0]; po[5] = st[1]; po[6] = st[2];
    }
    __syncthreads();
    if (new_points) {
        const float tx = st[0], ty = st[1], tz = st[2];
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const float4 p = points[i];
            const float dx = p.x - tx, dy = p.y - ty, dz = p.z - tz;
            float4 o;
            o.x = (dx * sR[0] + dy * sR[3]) + dz * sR[6];
            o.y = (dx * sR[1] + dy * sR[4]) + dz * sR[7];
            o.z = (dx * sR[2] + dy * sR[5]) + dz * sR[8];
            o.w = 0.f;
            new_points[i] = o;
        }
    }
}

// one workgroup per crop.  heads[b][n][8] = (r0..r3, t0..t2, c); points[b][n][4] (xyz,-)
__global__ __launch_bounds__(kSelThreads) void pose_select_kernel(const float* __restrict__ heads, const float4* __restrict__ points,
                                                                  double* __restrict__ pose, int* __restrict__ which_out,
                                                                  float4* __restrict__ new_points, int n)
{
    __shared__ float sc[kSelThreads];
    __shared__ int si[kSelThreads];
    __shared__ float sR[9];
    __shared__ float st[3];
    const int b = blockIdx.x;
    heads += (size_t)b * n * 8;
    points += (size_t)b * n;
    float best = -__builtin_inff();
    int bi = kNoIndex;
    for (int i = threadIdx.x; i < n; i += blockDim.x) argmax_take(heads[(size_t)i * 8 + 7], i, best, bi);
    const int w = argmax_reduce(best, bi, sc, si);
    if (threadIdx.x == 0 && which_out) which_out[b] = w;
    pose_from_heads(heads + (size_t)w * 8, w, points, pose + (size_t)b * 7, new_points ? new_points + (size_t)b * n : nullptr, n, sR, st);
}

// The estimator's heads when only the pose is wanted (PoseNet.forward_pose): my_estimator_prediction reads r and t at the arg-max of the
// confidence alone, so the confidence head runs on every point and the r / t heads on that one row per crop.
//
// head_conf_argmax: one workgroup per crop.  Row i's confidence is head_select_kernel's j == 7 value (the same fmaf chain over ascending k,
// + bias, 1 / (1 + expf(-s))); the arg-max over the SIGMOID values is pose_select_kernel's (argmax_take / argmax_reduce: thread t sees rows
// t, t + 256, ..).  A thread owns a row, so a plain load would have 64 lanes walk 64 different 512-byte rows; instead the workgroup stages
// 256 rows x 32 k through LDS with row-contiguous 16-byte loads (the next chunk's loads are in flight while this one is summed) and each
// thread sums its own row's 32 values in k order from LDS (row stride 33 words: no bank conflicts).  Then the crop's selected row of the
// point features is copied out for the r / t chain.
constexpr int kConfKC = 32;                   // k per staged chunk
constexpr int kConfQ = kConfKC / 4;           // float4 per row and chunk
constexpr int kConfLd = kConfKC + 1;

__global__ __launch_bounds__(kSelThreads) void head_conf_argmax_kernel(const float* __restrict__ h, int ldh, int off_c,
                                                                       const float* __restrict__ wc, const float* __restrict__ bc,
                                                                       const int64_t* __restrict__ obj, int* __restrict__ which_out,
                                                                       float* __restrict__ conf_out, const float* __restrict__ pf, int ld_pf,
                                                                       float* __restrict__ pf_row_out, int n, int K)
{
    __shared__ float tile[kSelThreads * kConfLd];
    __shared__ float sc[kSelThreads];
    __shared__ int si[kSelThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int o = (int)obj[b];
    const float* w = wc + (size_t)o * K;           // (uniform: read through the scalar cache)
    const float bias = bc[o];
    h += (size_t)b * n * ldh + off_c;
    const int kch = (K + kConfKC - 1) / kConfKC;
    const int stages = ((n + kSelThreads - 1) / kSelThreads) * kch;
    float4 nxt[kConfQ];
    // chunk `stage` = rows (stage / kch) * 256 .. + 255, k (stage % kch) * 32 .. + 31: float4 number j * 256 + tid of it
    auto fetch = [&](int stage) {
        const int r0 = (stage / kch) * kSelThreads, k0 = (stage % kch) * kConfKC;
#pragma unroll
        for (int j = 0; j < kConfQ; ++j) {
            const int idx = j * kSelThreads + tid;
            const int r = r0 + idx / kConfQ, k = k0 + (idx % kConfQ) * 4;
            nxt[j] = (r < n && k < K) ? *reinterpret_cast<const float4*>(h + (size_t)r * ldh + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    fetch(0);
    float best = -__builtin_inff(), s = 0.f;
    int bi = kNoIndex;
    for (int stage = 0; stage < stages; ++stage) {
        __syncthreads();                           // the previous chunk has been summed
#pragma unroll
        for (int j = 0; j < kConfQ; ++j) {
            const int idx = j * kSelThreads + tid;
            float* t = tile + (idx / kConfQ) * kConfLd + (idx % kConfQ) * 4;
            t[0] = nxt[j].x; t[1] = nxt[j].y; t[2] = nxt[j].z; t[3] = nxt[j].w;
        }
        __syncthreads();
        if (stage + 1 < stages) fetch(stage + 1);
        const int blk = stage / kch, ch = stage - blk * kch;
        const int k0 = ch * kConfKC, kn = K - k0 < kConfKC ? K - k0 : kConfKC;
        const float* t = tile + tid * kConfLd;
        if (ch == 0) s = 0.f;
#pragma unroll 8
        for (int k = 0; k < kn; ++k) s = fmaf(t[k], w[k0 + k], s);
        const int i = blk * kSelThreads + tid;
        if (ch == kch - 1 && i < n) {
            s += bias;
            argmax_take(1.f / (1.f + expf(-s)), i, best, bi);
        }
    }
    const int sel = argmax_reduce(best, bi, sc, si);
    if (tid == 0) {
        which_out[b] = sel;
        conf_out[b] = sc[0];
    }
    if (pf) {
        const float* src = pf + ((size_t)b * n + sel) * ld_pf;
        for (int c = tid; c < ld_pf; c += kSelThreads) pf_row_out[(size_t)b * ld_pf + c] = src[c];
    }
}

// pose_from_row: one workgroup per crop.  h[b][ldh] holds the r and t layer-3 activations of the crop's SELECTED row at off_r / off_t;
// threads 0..6 evaluate the object's 4 + 3 last-layer rows on it (head_select_kernel's j < 7), then pose_select_kernel's tail.
__global__ __launch_bounds__(kSelThreads) void pose_from_row_kernel(const float* __restrict__ h, int ldh, int off_r, int off_t,
                                                                    const float* __restrict__ wr, const float* __restrict__ br,
                                                                    const float* __restrict__ wt, const float* __restrict__ bt,
                                                                    const int64_t* __restrict__ obj, const int* __restrict__ which,
                                                                    const float4* __restrict__ points, double* __restrict__ pose,
                                                                    float4* __restrict__ new_points, int n, int K)
{
    __shared__ float sh[8];
    __shared__ float sR[9];
    __shared__ float st[3];
    const int b = blockIdx.x;
    if (threadIdx.x < 7) {
        const int j = threadIdx.x, o = (int)obj[b];
        const float* hp = h + (size_t)b * ldh + (j < 4 ? off_r : off_t);
        const float* w = j < 4 ? wr + (size_t)(o * 4 + j) * K : wt + (size_t)(o * 3 + j - 4) * K;
        float s = 0.f;
        for (int k = 0; k < K; ++k) s = fmaf(hp[k], w[k], s);
        sh[j] = s + (j < 4 ? br[o * 4 + j] : bt[o * 3 + j - 4]);
    }
    __syncthreads();
    int w = which[b];
    w = w < 0 ? 0 : w >= n ? n - 1 : w;            // (an index from elsewhere than head_conf_argmax must not leave the crop's cloud)
    pose_from_heads(sh, w, points + (size_t)b * n, pose + (size_t)b * 7, new_points ? new_points + (size_t)b * n : nullptr, n, sR, st);
}

__global__ void pose_compose_kernel(double* __restrict__ pose, const float* __restrict__ ref_r, int ldr,
                                    const float* __restrict__ ref_t, int ldt, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double* po = pose + (size_t)b * 7;
    Mat4 A = quaternion_matrix(po);
    A.m[0][3] = po[4]; A.m[1][3] = po[5]; A.m[2][3] = po[6];
    const float* r = ref_r + (size_t)b * ldr;
    const float* t = ref_t + (size_t)b * ldt;
    const float nrm = sqrtf(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]);  // torch.norm in float32
    const double q2[4] = {(double)(r[0] / nrm), (double)(r[1] / nrm), (double)(r[2] / nrm), (double)(r[3] / nrm)};
    Mat4 Bm = quaternion_matrix(q2);
    Bm.m[0][3] = (double)t[0]; Bm.m[1][3] = (double)t[1]; Bm.m[2][3] = (double)t[2];
    Mat4 C;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += A.m[i][k] * Bm.m[k][j];
            C.m[i][j] = s;
        }
    const double tx = C.m[0][3], ty = C.m[1][3], tz = C.m[2][3];
    C.m[0][3] = C.m[1][3] = C.m[2][3] = 0.0;
    double q[4];
    quaternion_from_matrix_precise(C, q);
    po[0] = q[0]; po[1] = q[1]; po[2] = q[2]; po[3] = q[3];
    po[4] = tx; po[5] = ty; po[6] = tz;
}

__global__ void pose_recentre_kernel(const float4* __restrict__ points, const double* __restrict__ pose,
                                     float4* __restrict__ new_points, int n)
{
    const int b = blockIdx.y;
    const double* po = pose + (size_t)b * 7;
    const Mat4 M = quaternion_matrix(po);
    float R[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = (float)M.m[i][j];
    const float tx = (float)po[4], ty = (float)po[5], tz = (float)po[6];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 p = points[(size_t)b * n + i];
        const float dx = p.x - tx, dy = p.y - ty, dz = p.z - tz;
        float4 o;
        o.x = (dx * R[0] + dy * R[3]) + dz * R[6];
        o.y = (dx * R[1] + dy * R[4]) + dz * R[7];
        o.z = (dx * R[2] + dy * R[5]) + dz * R[8];
        o.w = 0.f;
        new_points[(size_t)b * n + i] = o;
    }
}

}  // namespace

extern "C" int ape_pose_select_f32(const float* heads, const float* points4, double* pose, int* which, float* new_points4,
                                   int B, int n, void* stream)
{
    if (!heads || !points4 || !pose || B < 0 || n < 1) return APE_EINVAL;
    if (B == 0) return APE_OK;
    hipLaunchKernelGGL(pose_select_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, heads, (const float4*)points4, pose,
                       which, (float4*)new_points4, n);
    return ape::check_launch("ape_pose_select_f32");
}

extern "C" int ape_head_conf_argmax_f32(const float* h3c, int ldh, int off_c, const float* wc, const float* bc, const int64_t* obj,
                                        int* which_out, float* conf_out, const float* pf, int ld_pf, float* pf_row_out, int B, int n,
                                        int K, void* stream)
{
    if (!h3c || !wc || !bc || !obj || !which_out || !conf_out || B < 0 || n < 1 || K < 4 || K > 1024 || off_c < 0 || ldh < off_c + K)
        return APE_EINVAL;
    if (((uintptr_t)h3c & 15) || (ldh & 3) || (off_c & 3) || (K & 3)) return APE_EINVAL;      // rows are read 16 bytes at a time
    if (pf && (!pf_row_out || ld_pf < 1)) return APE_EINVAL;
    if (B == 0) return APE_OK;
    hipLaunchKernelGGL(head_conf_argmax_kernel, dim3(B), dim3(kSelThreads), 0, (hipStream_t)stream, h3c, ldh, off_c, wc, bc, obj,
                       which_out, conf_out, pf, ld_pf, pf_row_out, n, K);
    return ape::check_launch("ape_head_conf_argmax_f32");
}

extern "C" int ape_pose_from_row_f32(const float* h3rt_row, int ldh, int off_r, int off_t, const float* wr, const float* br,
                                     const float* wt, const float* bt, const int64_t* obj, const int* which, const float* points4,
                                     double* pose, float* new_points4, int B, int n, int K, void* stream)
{
    if (!h3rt_row || !wr || !br || !wt || !bt || !obj || !which || !points4 || !pose || B < 0 || n < 1 || K < 1 || K > 1024 ||
        off_r < 0 || off_t < 0 || ldh < off_r + K || ldh < off_t + K)
        return APE_EINVAL;
    if (B == 0) return APE_OK;
    hipLaunchKernelGGL(pose_from_row_kernel, dim3(B), dim3(kSelThreads), 0, (hipStream_t)stream, h3rt_row, ldh, off_r, off_t, wr, br,
                       wt, bt, obj, which, (const float4*)points4, pose, (float4*)new_points4, n, K);
    return ape::check_launch("ape_pose_from_row_f32");
}

extern "C" int ape_pose_compose_f64(double* pose, const float* ref_r, int ldr, const float* ref_t, int ldt, int B, void* stream)
{
    if (!pose || !ref_r || !ref_t || B < 0 || ldr < 4 || ldt < 3) return APE_EINVAL;
    if (B == 0) return APE_OK;
    hipLaunchKernelGGL(pose_compose_kernel, dim3(ape::ceil_div(B, 64)), dim3(64), 0, (hipStream_t)stream, pose, ref_r, ldr,
                       ref_t, ldt, B);
    return ape::check_launch("ape_pose_compose_f64");
}

extern "C" int ape_pose_recentre_f32(const float* points4, const double* pose, float* new_points4, int B, int n, void* stream)
{
    if (!points4 || !pose || !new_points4 || B < 0 || n < 1) return APE_EINVAL;
    if (B == 0) return APE_OK;
    dim3 grid(ape::ceil_div(n, 256), B);
    hipLaunchKernelGGL(pose_recentre_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const float4*)points4, pose,
                       (float4*)new_points4, n);
    return ape::check_launch("ape_pose_recentre_f32");
}
