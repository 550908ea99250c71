// What the sample builders (bgsub_train.hip, seg_train.hip, pose_train.hip, linemod.hip, ycb.hip) share around their kernels: the batch of
// jobs that travels as kernel arguments and the loop that launches it in chunks, the workgroup reduction of their statistics passes, the
// mean that ImageEnhance.Contrast needs from the partial sums, and the host checks of what a job's rotation and jitter list may hold.  For
// the three DenseFusion builders (the last three) also the host checks of a job's crop and output slot and the layout of their workspace;
// what their samples kernels share on the device is sample_points.h.
#pragma once
#include <limits.h>

#include "common.h"
#include "aug_px.h"

namespace ape {

constexpr int kJobs = 16;            // jobs per launch: at most 16 * 232 B of kernel arguments (limit 4 KB)
constexpr int kBlocks = 64;          // partials per sample (and image) of a statistics pass: one per workgroup

template <class Job, int C>
struct SampleBatch {
    Job j[kJobs];
    float mean[C], stdv[C];
};

// the jobs of a batch in chunks of kJobs: launch(bt, first job of the chunk, jobs in it)
template <class Batch, class Job, class Launch>
void for_each_chunk(Batch& bt, const Job* jobs, int B, Launch launch)
{
    static_assert(sizeof(Batch) <= 3900, "kernel arguments");
    for (int i0 = 0; i0 < B; i0 += kJobs) {
        const int nb = B - i0 < kJobs ? B - i0 : kJobs;
        for (int i = 0; i < nb; ++i) bt.j[i] = jobs[i0 + i];
        launch(bt, i0, nb);
    }
}

// ---- wave -> LDS -> thread 0, of the quantities a caller names -------------------------------------------------------------------------
// `park(part...)` (every thread): each part reduced over the wave -- one shuffle loop for all of them, so their latencies overlap -- and
// lane 0 stores it to the part's LDS slot of its wave.  After the caller's __syncthreads, `total` (thread 0) folds the slots in wave
// order.  Integers only, so the result does not depend on the order.  A kernel pays for the parts it lists and for nothing else.
struct Sum { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };
struct Min { __device__ int operator()(int a, int b) const { return b < a ? b : a; } };
struct Max { __device__ int operator()(int a, int b) const { return b > a ? b : a; } };

template <class T, class Op>
struct Part {                            // a scalar: this thread's value and slot[waves]
    T v;
    T* slot;
    __device__ void step(int o) { v = Op()(v, __shfl_down(v, o, 64)); }
    __device__ void store(int w) const { slot[w] = v; }
};
template <class Op, class T>
__device__ __forceinline__ Part<T, Op> part(T v, T* slot) { return {v, slot}; }

// (min row, max row, min column, max column) of the pixels a thread saw; INT_MAX, -1, INT_MAX, -1 when it saw none
struct Extent {
    int rmin = INT_MAX, rmax = -1, cmin = INT_MAX, cmax = -1;
    __device__ void add(int x, int y) { merge(y, y, x, x); }
    __device__ void merge(int r0, int r1, int c0, int c1)
    {
        rmin = Min()(rmin, r0); rmax = Max()(rmax, r1); cmin = Min()(cmin, c0); cmax = Max()(cmax, c1);
    }
};
struct ExtentPart {                      // an Extent and slot[waves][4]
    Extent e;
    int (*slot)[4];
    __device__ void step(int o) { e.merge(__shfl_down(e.rmin, o, 64), __shfl_down(e.rmax, o, 64), __shfl_down(e.cmin, o, 64), __shfl_down(e.cmax, o, 64)); }
    __device__ void store(int w) const { slot[w][0] = e.rmin; slot[w][1] = e.rmax; slot[w][2] = e.cmin; slot[w][3] = e.cmax; }
};
__device__ __forceinline__ ExtentPart part(const Extent& e, int (*slot)[4]) { return {e, slot}; }

template <class... P>
__device__ __forceinline__ void park(P... p)
{
    for (int o = 32; o > 0; o >>= 1) (p.step(o), ...);
    if ((threadIdx.x & 63) == 0) (p.store(threadIdx.x >> 6), ...);
}

template <int kWaves, class Op, class T>
__device__ __forceinline__ T total(const T* slot)
{
    T t = slot[0];
    for (int w = 1; w < kWaves; ++w) t = Op()(t, slot[w]);
    return t;
}

template <int kWaves>
__device__ __forceinline__ void total(const int (*slot)[4], int* out4)
{
    Extent e;
    for (int w = 0; w < kWaves; ++w) e.merge(slot[w][0], slot[w][1], slot[w][2], slot[w][3]);
    out4[0] = e.rmin; out4[1] = e.rmax; out4[2] = e.cmin; out4[3] = e.cmax;
}

// the mean ImageEnhance.Contrast blends towards, from the kBlocks partial L sums of the image (added in index order); 0 without a contrast
__device__ __forceinline__ int mean_from_partials(const ape_aug_jitter& jit, const unsigned long long* partial, int H, int W)
{
    if (aug_contrast_at(jit) < 0) return 0;
    unsigned long long tot = 0;
    for (int i = 0; i < kBlocks; ++i) tot += partial[i];
    return aug_mean_of_sum(tot, H, W);
}

// ---- what an entry point refuses before it launches ---------------------------------------------------------------------------------------
inline bool frame_ok(int B, int H, int W) { return B >= 0 && H >= 1 && W >= 1 && H <= 32767 && W <= 32767; }

inline bool rotation_ok(const ape_aug_rotation& rot, int H, int W)
{
    if (rot.mode < APE_ROT_NONE || rot.mode > APE_ROT_270) return false;
    return (rot.mode != APE_ROT_90 && rot.mode != APE_ROT_270) || H == W;
}

inline bool jitter_ok(const ape_aug_jitter& jit)
{
    if (jit.n_ops < 0 || jit.n_ops > 4) return false;
    int contrasts = 0;
    for (int k = 0; k < jit.n_ops; ++k) {
        const int c = jit.code[k];
        if (c < APE_JIT_BRIGHTNESS || c > APE_JIT_HUE) return false;
        if (c == APE_JIT_HUE && (jit.shift[k] < 0 || jit.shift[k] > 255)) return false;
        if (c != APE_JIT_HUE && !(jit.factor[k] == jit.factor[k])) return false;         // NaN
        contrasts += c == APE_JIT_CONTRAST;
    }
    return contrasts <= 1;               // a second one would need the sum of an image that depends on the first sum
}

// Normalize's mean / std (HOST pointers) into the batch: a zero std and a NaN mean are refused
template <int C, class Job>
bool norm_ok(const float* mean, const float* stdv, SampleBatch<Job, C>& bt)
{
    if (!mean || !stdv) return false;
    for (int c = 0; c < C; ++c) {
        if (!(stdv[c] != 0.f) || !(mean[c] == mean[c])) return false;
        bt.mean[c] = mean[c];
        bt.stdv[c] = stdv[c];
    }
    return true;
}

// ---- the DenseFusion builders: crop, output slot, workspace ------------------------------------------------------------------------------
inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// get_bbox's crops: sides from border_list inside a 480 x 640 frame
template <class Job>
bool crop_ok(const Job& j, int H, int W)
{
    const int hc = j.rmax - j.rmin, wc = j.cmax - j.cmin;
    if (j.rmin < 0 || j.cmin < 0 || j.rmax > H || j.cmax > W || j.rmax <= j.rmin || j.cmax <= j.cmin) return false;
    return hc >= 40 && hc <= 480 && wc >= 40 && wc <= 640 && hc % 40 == 0 && wc % 40 == 0;
}

// the job's sample (choose | points | crop, ape_pose_train_sample_bytes) lies 16-byte aligned inside the packed block
template <class Job>
bool slot_ok(const Job& j, int N, size_t out_bytes)
{
    if (j.out_off < 0 || (j.out_off & 15)) return false;
    const size_t need = ape_pose_train_sample_bytes(N, j.rmax - j.rmin, j.cmax - j.cmin);
    return (size_t)j.out_off <= out_bytes && out_bytes - (size_t)j.out_off >= need;
}

// workspace of a builder: partials[B] (part_bytes each, a multiple of 16) | rows i32[B][H][row_ints] | prefix i32[B][H] | sel i32[B][N] | end
struct SampleLayout {
    size_t part_bytes;
    int row_ints;
    size_t rows(int B) const { return B < 1 ? 0 : (size_t)B * part_bytes; }
    size_t tables(int B, int H) const { return B < 1 || H < 1 ? 0 : rows(B) + up16((size_t)B * H * row_ints * sizeof(int)); }
    size_t sel(int B, int H) const { return B < 1 || H < 1 ? 0 : tables(B, H) + (size_t)B * H * sizeof(int); }
    size_t end(int B, int H, int N) const { return B < 1 || H < 1 || N < 1 ? 0 : up16(sel(B, H) + (size_t)B * N * sizeof(int)); }
};

}  // namespace ape
