// 8-connected component labelling of a batch of byte images on the device, shared by the segmentation post-processing (segpost.hip) and
// the largest-contour box of the LineMOD samples (linemod.hip).  Every including file gets its own copy of the kernels (internal linkage).
#pragma once
#include <stdint.h>

#include "common.h"

namespace {

// union-find on the pixel grid; every access to L during the merge is an agent-scope atomic (coherent across XCDs)
__device__ __forceinline__ int ld_relaxed(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ int uf_find(const int* L, int a)
{
    int p = ld_relaxed(&L[a]);
    while (p != a) { a = p; p = ld_relaxed(&L[a]); }
    return a;
}

__device__ void uf_union(int* L, int a, int b)
{
    bool done = false;
    while (!done) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a < b) {
            const int old = atomicMin(&L[b], a);
            done = old == b;
            b = old;
        } else if (b < a) {
            const int old = atomicMin(&L[a], b);
            done = old == a;
            a = old;
        } else {
            done = true;
        }
    }
}

// Run-based labelling: a wave covers 64 consecutive pixels; inside it every pixel is pointed at the first pixel of its
// horizontal run straight away (ballot of the run boundaries, no atomics), so the union-find only has to join RUNS:
//   * a run that continues across the wave's left edge joins the previous wave's run (one union per wave at most);
//   * a run joins the row above once per overlap with a run there (at the first pixel of the overlap), plus the two diagonal
//     contacts that no vertical contact implies.
// A 126 x 126 object costs ~130 unions instead of ~16 000 per-pixel unions all chasing the same root.  Unions link the larger
// root under the smaller, so the final root of a component is its smallest pixel index whatever the order: identical labels.
__global__ void ccl_init_kernel(const uint8_t* __restrict__ label, int* __restrict__ L, int W, long npix)
{
    const long nround = (npix + 63) & ~63L;          // whole waves stay converged for the ballot
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < nround; p += (long)gridDim.x * blockDim.x) {
        const int lane = threadIdx.x & 63;
        const bool in = p < npix;
        const int c = in ? label[p] : 0;
        const int x = in ? (int)(p % W) : 0;
        const int cl = __shfl_up(c, 1);
        const bool cont = in && lane > 0 && x > 0 && cl == c;          // continues the run of the lane to the left
        const unsigned long long starts = __ballot(!cont);
        if (in) {
            const unsigned long long below = starts & ((2ULL << lane) - 1ULL);      // lane 63: 2<<63 wraps to 0, -1 = all ones
            const int start = 63 - __clzll(below);
            L[p] = c ? (int)(p - (lane - start)) : -1;
        }
    }
}

// L indices are global over the batch (frame b occupies [b*H*W, (b+1)*H*W)), so roots are unique batch-wide.
__global__ void ccl_merge_kernel(const uint8_t* __restrict__ label, int* __restrict__ L, int H, int W, long npix)
{
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
        const uint8_t c = label[p];
        if (!c) continue;
        const int x = p % W;
        const int y = (p / W) % H;
        const bool left = x > 0 && label[p - 1] == c;
        if (left && (threadIdx.x & 63) == 0) uf_union(L, (int)p, (int)p - 1);   // in-wave run links were made by ccl_init_kernel
        if (y > 0) {
            const bool nw = x > 0 && label[p - W - 1] == c;
            if (label[p - W] == c) {
                // N present (NW and NE hang on N's run): one union per overlap of this run with a run above, at its first pixel
                if (!left || !nw) uf_union(L, (int)p, (int)(p - W));
            } else {
                if (nw && !left) uf_union(L, (int)p, (int)(p - W - 1));        // with a left neighbour, ITS N is this NW
                if (x < W - 1 && label[p - W + 1] == c && label[p + 1] != c)     // with a right neighbour, ITS N is this NE
                    uf_union(L, (int)p, (int)(p - W + 1));
            }
        }
    }
}
// sum / cnt (may be null): the per-component score accumulators live at the ROOT pixel's index; a root zeroes its own pair here instead of a
// pass that zeroed all npix pairs (236 MB per 64 frames) before the labelling
__global__ void ccl_compress_kernel(int* __restrict__ L, long npix, unsigned long long* __restrict__ sum, unsigned int* __restrict__ cnt)
{
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
        int a = L[p];
        if (a < 0) continue;
        while (true) {
            const int q = L[a];   // parents only ever point to smaller indices: chains end at the root
            if (q == a) break;
            a = q;
        }
        L[p] = a;   // benign race: other lanes may read either the old parent or the root, both lead to the root
        if (sum && a == (int)p) { sum[p] = 0ull; cnt[p] = 0u; }
    }
}

}  // namespace
