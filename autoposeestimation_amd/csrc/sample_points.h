// What the samples kernels of the three DenseFusion sample builders (pose_train.hip, linemod.hip, ycb.hip) share on the device: the
// planar writer of the normalised crop and the walk that turns one kept rank into `choose` and the three floats of its point.  Device
// only: pose_px.h / ycb_px.h stay plain C++ for tools/check_pose_px.py and tools/check_ycb_px.py.
#pragma once
#include "sample_batch.h"
#include "pose_px.h"

namespace ape {

constexpr int kImgBlocks = 96;       // workgroups per sample that write the crop (at most 480 * 640 pixels: <= 12.5 per thread)

// The normalised crop of job j, planar, by workgroups 0..kImgBlocks-1 of kT threads; rgb(x, y, r, g, b): the uint8 colour at frame (x, y).
template <int kT, class Batch, class Job, class Rgb>
__device__ __forceinline__ void write_crop(const Batch& bt, const Job& j, float* img, Rgb rgb)
{
    const int Wc = j.cmax - j.cmin;
    const long plane = (long)(j.rmax - j.rmin) * Wc;
    for (long i = (long)blockIdx.x * kT + threadIdx.x; i < plane; i += (long)kImgBlocks * kT) {
        const int r = (int)(i / Wc), c = (int)(i % Wc);
        int cr, cg, cb;
        rgb(j.cmin + c, j.rmin + r, cr, cg, cb);
        img[i] = ((float)cr - bt.mean[0]) / bt.stdv[0];
        img[plane + i] = ((float)cg - bt.mean[1]) / bt.stdv[1];
        img[2 * plane + i] = ((float)cb - bt.mean[2]) / bt.stdv[2];
    }
}

struct Window {                          // rows [r0, r1), columns [c0, c1)
    int r0, r1, c0, c1;
};
template <class Job>
__device__ __forceinline__ Window crop_window(const Job& j) { return {j.rmin, j.rmax, j.cmin, j.cmax}; }

// One chosen point per wave (every lane of the wave calls this with the same arguments): point `pt` < N of the sample whose slot starts at
// `base` (choose i64[N] | points f32[N][3]) is the valid pixel of rank `rank`, counted in row-major order over the builder's window.  The
// row comes from a binary search of the sample's exclusive row prefix pf[0..H), the column from a ballot / popcount walk of that one row,
// 64 columns at a time.  The policy P names what differs between the builders:
//   P::window(j, H, W)           the Window that was counted (it contains the crop's valid pixels);
//   P::valid(j, H, W, x, y)      the pixel is a valid one;
//   P::point(j, H, W, x, y, q)   q[0..3) = its back-projection.
// `pf` and `rank` come from the caller through device memory, where the entry point cannot look at them: the row found is always inside
// the frame, a row or a column outside the window is never read, every store goes to the slot of the point, and a rank without a pixel
// (a prefix or a rank the caller got wrong) writes zeros.  Control flow is wave-uniform up to the one storing lane.
template <class P, class Job>
__device__ __forceinline__ void sample_point(const Job& j, int H, int W, int pt, int N, const int* pf, int rank, unsigned char* base)
{
    const int lane = threadIdx.x & 63;
    const Window w = P::window(j, H, W);
    long long* choose = (long long*)base + pt;
    float* p = (float*)(base + 8L * N) + 3L * pt;
    const int y = pose_row_of_rank(pf, H, rank);
    int rem = rank - pf[y];                          // the pixel's rank inside its row
    bool found = false;
    const bool row_in = y >= w.r0 && y < w.r1;
    for (int x0 = w.c0; x0 < w.c1 && !found && row_in; x0 += 64) {
        const int x = x0 + lane;
        const bool v = x < w.c1 && P::valid(j, H, W, x, y);
        const unsigned long long m = __ballot(v);
        const int c = __popcll(m);
        if (rem >= 0 && rem < c) {
            found = true;
            if (v && __popcll(m & ((1ull << lane) - 1ull)) == rem) {       // exactly one lane
                float q[3];
                P::point(j, H, W, x, y, q);
                *choose = (long long)(y - j.rmin) * (j.cmax - j.cmin) + (x - j.cmin);
                p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
            }
        }
        rem -= c;
    }
    if (!found && lane == 0) {
        *choose = 0;
        p[0] = p[1] = p[2] = 0.f;
    }
}

}  // namespace ape
