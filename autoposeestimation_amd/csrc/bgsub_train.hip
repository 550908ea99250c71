// Training samples of the background-subtraction segmentor, built on the device from resident raw frames (reference
// background_subtraction/utils.py:414-646 `load_subtraction` + `augment`, dataset.py:60-86).  The reference does this in Pillow on the host,
// five PNG decodes and up to five rotations, two colour jitters and two HSV conversions per sample, behind four loader processes; here the
// decoded frames stay in HBM and a batch is two launches:
//   bgsub_luma_sum_kernel   ImageEnhance.Contrast blends towards the mean of L over the WHOLE image as it is when the op runs (after the
//                           rotation's black corners and the colour ops before it): replay those per pixel and sum L in integers
//   bgsub_train_kernel      rotate -> jitter -> flips -> HSV -> differences -> normalise, one thread per output pixel
// The per-pixel arithmetic is bgsub_px.h on aug_px.h (Pillow's own C restated; also compiled for the host and checked against the
// installed Pillow there); batch, reduction and job checks are sample_batch.h, shared with the other two sample builders.
// Bandwidth- and latency-bound: ~3.4 MB gathered twice and ~12 MB written per 480 x 640 sample.
//
// Thread map: a workgroup is a 32 x 8 tile of OUTPUT pixels, x fastest.  Stores are then full lines (a wave covers two rows of 32 pixels:
// 2 x 1 KB of x8 as float4 pairs, 2 x 256 B of labels), and the rotated gathers of a tile stay inside a compact patch of the source
// (at most ~34 x 34 pixels at 45 degrees) instead of a 256-pixel slanted line that touches a new cache line every few pixels.
//
// Sums: each workgroup of the first pass writes ONE partial sum of its own (plain store, fixed grid-stride order inside), the second
// pass adds the kBlocks partials of its sample in index order: integer, so exact and bit-reproducible whatever the schedule, and the
// workspace never needs zeroing -- the batch is two launches with nothing between them.
#include "sample_batch.h"
#include "bgsub_px.h"

namespace {

using namespace ape;

constexpr int kTileW = 32, kTileH = 8, kT = kTileW * kTileH;
using TrainBatch = SampleBatch<ape_bgsub_train_job, 7>;

// grid (kBlocks, 2 * nb): image = blockIdx.y & 1 of job blockIdx.y >> 1; partial[(job0 + job) * 2 + image][kBlocks]
__global__ __launch_bounds__(kT) void bgsub_luma_sum_kernel(TrainBatch bt, int job0, int H, int W, unsigned long long* __restrict__ partial)
{
    __shared__ unsigned long long red[kT / 64];
    const ape_bgsub_train_job& j = bt.j[blockIdx.y >> 1];
    const int im = blockIdx.y & 1;
    const int kc = aug_contrast_at(j.jit[im]);
    unsigned long long s = 0;
    if (kc >= 0) {                                   // uniform per workgroup
        const int tiles_x = (W + kTileW - 1) / kTileW, tiles = tiles_x * ((H + kTileH - 1) / kTileH);
        const int tx = threadIdx.x % kTileW, ty = threadIdx.x / kTileW;
        for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
            const int x = (t % tiles_x) * kTileW + tx, y = (t / tiles_x) * kTileH + ty;
            if (x < W && y < H) {
                int r, g, b;
                bgsub_jittered_rgb(j, im, H, W, x, y, kc, 0, r, g, b);
                s += (unsigned long long)pil_luma(r, g, b);
            }
        }
    }
    park(part<Sum>(s, red));
    __syncthreads();
    if (threadIdx.x == 0) partial[((long)(job0 + (blockIdx.y >> 1)) * 2 + im) * kBlocks + blockIdx.x] = total<kT / 64, Sum>(red);
}

// grid (tiles_x, tiles_y, nb)
__global__ __launch_bounds__(kT) void bgsub_train_kernel(TrainBatch bt, int job0, int H, int W, const unsigned long long* __restrict__ partial,
                                                         float4* __restrict__ x8, long long* __restrict__ label, uint8_t* __restrict__ u8)
{
    __shared__ int means[2];
    const ape_bgsub_train_job& j = bt.j[blockIdx.z];
    const int s = job0 + blockIdx.z;
    if (threadIdx.x < 2) means[threadIdx.x] = mean_from_partials(j.jit[threadIdx.x], partial + ((long)s * 2 + threadIdx.x) * kBlocks, H, W);
    __syncthreads();
    const int xo = blockIdx.x * kTileW + threadIdx.x % kTileW, yo = blockIdx.y * kTileH + threadIdx.x / kTileW;
    if (xo >= W || yo >= H) return;
    int ch[7];
    const int lab = bgsub_train_pixel(j, H, W, xo, yo, means[0], means[1], ch);
    const long p = ((long)s * H + yo) * W + xo;
    float v[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) v[c] = ((float)ch[c] / 255.f - bt.mean[c]) / bt.stdv[c];      // ToTensor, Normalize
    x8[p * 2] = make_float4(v[0], v[1], v[2], v[3]);
    x8[p * 2 + 1] = make_float4(v[4], v[5], v[6], 0.f);
    label[p] = lab;
    if (u8) {
#pragma unroll
        for (int c = 0; c < 7; ++c) u8[p * 7 + c] = (uint8_t)ch[c];
    }
}

bool job_ok(const ape_bgsub_train_job& j, int H, int W)
{
    if (!j.f_rgb || !j.b_rgb || !j.f_depth || !j.b_depth || !j.label) return false;
    return rotation_ok(j.rot, H, W) && jitter_ok(j.jit[0]) && jitter_ok(j.jit[1]);
}

}  // namespace

extern "C" size_t ape_bgsub_train_workspace_bytes(int B)
{
    return B < 1 ? 0 : (size_t)B * 2 * kBlocks * sizeof(unsigned long long);
}

extern "C" int ape_bgsub_train_samples(const ape_bgsub_train_job* jobs, int B, int H, int W, const float* mean7_host, const float* std7_host,
                                       float* x8, long long* label, uint8_t* u8_or_null, void* ws, size_t ws_bytes, void* stream)
{
    if (!frame_ok(B, H, W) || !mean7_host || !std7_host) return APE_EINVAL;
    if (B == 0) return APE_OK;
    if (!jobs || !x8 || !label || !ws || ((uintptr_t)x8 & 15) || ((uintptr_t)ws & 15)) return APE_EINVAL;
    if (ws_bytes < ape_bgsub_train_workspace_bytes(B)) return APE_EWORKSPACE;
    TrainBatch bt;
    if (!norm_ok(mean7_host, std7_host, bt)) return APE_EINVAL;
    bool any_contrast = false;
    for (int i = 0; i < B; ++i) {
        if (!job_ok(jobs[i], H, W)) return APE_EINVAL;
        any_contrast = any_contrast || aug_contrast_at(jobs[i].jit[0]) >= 0 || aug_contrast_at(jobs[i].jit[1]) >= 0;
    }
    const dim3 tiles(ceil_div(W, kTileW), ceil_div(H, kTileH));
    const hipStream_t st = (hipStream_t)stream;
    // the first pass of every chunk, then the second: two launches for B <= kJobs
    if (any_contrast)
        for_each_chunk(bt, jobs, B, [&](const TrainBatch& b, int i0, int nb) {
            hipLaunchKernelGGL(bgsub_luma_sum_kernel, dim3(kBlocks, 2 * nb), dim3(kT), 0, st, b, i0, H, W, (unsigned long long*)ws);
        });
    for_each_chunk(bt, jobs, B, [&](const TrainBatch& b, int i0, int nb) {
        hipLaunchKernelGGL(bgsub_train_kernel, dim3(tiles.x, tiles.y, nb), dim3(kT), 0, st, b, i0, H, W, (const unsigned long long*)ws,
                           (float4*)x8, label, u8_or_null);
    });
    return check_launch("ape_bgsub_train_samples");
}
