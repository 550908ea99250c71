// Training samples of DenseFusion, built on the device from resident frames (reference DenseFusion/datasets/myDatasetAugmented/
// dataset.py:158-326).  The reference does this in Pillow and numpy on the host, per sample: colour jitter of the full frame, Image.rotate
// of colour, label and depth, get_bbox of the label, the `choose` compaction of the valid pixels inside the box with a drawn subset, the
// back-projection of the chosen pixels and the normalised crop.  Here a batch is two launches with one small read-back between them:
//   pose_stats_kernel    over the full frames, one wave per row: the integer L sum that ImageEnhance.Contrast needs, the extents of the
//                        ROTATED label's pixels == 255 (one partial of each per workgroup) and, per row, the number of valid pixels
//                        (rotated label == 255 and rotated depth != 0), written by the wave that walked the row.  Plain stores, combined in
//                        index order: exact whatever the schedule.
//   pose_samples_kernel  workgroups 0..kImgBlocks-1 of a sample write the normalised crop, the others one chosen point per wave
//                        (sample_points.h, over whole rows).
// Whole-row counts are in-crop counts: every labelled pixel lies inside get_bbox's crop.  With the tight extents [r0, r1) the rounded side
// s' is an even number >= s = r1 - r0 (a multiple of 40), the centre is c = floor((r0 + r1) / 2) >= (r0 + r1 - 1) / 2, so
// c - s'/2 <= (r0 + r1)/2 - s/2 = r0 and c + s'/2 >= r1 - 1/2, an integer, hence >= r1; a shift back inside the frame moves the box over
// [0, s') or (480 - s', 480], which still covers [r0, r1) because s' <= 480 (640 for the columns) -- tests/test_pose_samples_host.py
// checks this over random extents.
// The host only draws and does get_bbox's arithmetic; `target` / `model_points` depend on no pixel and stay with numpy's float64 there.
// The per-pixel arithmetic is pose_px.h / aug_px.h (also compiled for the host, tools/check_pose_px.py); batch, reduction and job checks
// and workspace layout are sample_batch.h, the crop writer and the chosen-point walk sample_points.h.
#include "sample_points.h"

namespace {

using namespace ape;

constexpr int kT = 256, kWaves = kT / 64;

using PoseBatch = SampleBatch<ape_pose_train_job, 3>;

// workspace: luma u64[B][kBlocks] | ext i32[B][kBlocks][4] | rows i32[B][H] | prefix | sel
constexpr SampleLayout kLayout = {kBlocks * (sizeof(unsigned long long) + 4 * sizeof(int)), 1};

// whole rows: every labelled pixel lies inside the crop (above)
struct PosePoints {
    static __device__ Window window(const ape_pose_train_job&, int H, int W) { return {0, H, 0, W}; }
    static __device__ bool valid(const ape_pose_train_job& j, int H, int W, int x, int y) { return pose_valid(j, H, W, x, y); }
    static __device__ void point(const ape_pose_train_job& j, int H, int W, int x, int y, float* q)
    {
        pose_point(j, x, y, pose_depth_at(j, H, W, x, y), q);
    }
};

// grid (kBlocks, nb)
__global__ __launch_bounds__(kT) void pose_stats_kernel(PoseBatch bt, int job0, int H, int W, unsigned long long* __restrict__ luma,
                                                        int* __restrict__ ext, int* __restrict__ rows)
{
    __shared__ unsigned long long red_s[kWaves];
    __shared__ int red_e[kWaves][4];
    const ape_pose_train_job& j = bt.j[blockIdx.y];
    const int kc = aug_contrast_at(j.jit);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long s = 0;
    Extent e;
    int* row_out = rows + (long)(job0 + blockIdx.y) * H;
    for (int y = blockIdx.x * kWaves + wave; y < H; y += gridDim.x * kWaves) {          // a row belongs to one wave
        int cnt = 0;
        for (int x = lane; x < W; x += 64) {
            if (kc >= 0) {                           // uniform per workgroup
                int r, g, b;
                aug_jittered_rgb(j.rgb, j.jit, W, x, y, kc, 0, r, g, b);
                s += (unsigned long long)pil_luma(r, g, b);
            }
            if (pose_label_at(j, H, W, x, y) == 255) {
                e.add(x, y);
                cnt += pose_depth_at(j, H, W, x, y) != 0;
            }
        }
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
        if (lane == 0) row_out[y] = cnt;
    }
    park(part<Sum>(s, red_s), part(e, red_e));
    __syncthreads();
    if (threadIdx.x == 0) {
        const long p = (long)(job0 + blockIdx.y) * kBlocks + blockIdx.x;
        luma[p] = total<kWaves, Sum>(red_s);
        total<kWaves>(red_e, ext + p * 4);
    }
}

// grid (kImgBlocks + ceil(N / kWaves), nb).  `prefix` and `sel` come from the caller through device memory, where the entry point cannot
// look at them: see sample_point; every frame read is bounds-checked on its coordinates (pose_px.h).
__global__ __launch_bounds__(kT) void pose_samples_kernel(PoseBatch bt, int job0, int H, int W, int N, const unsigned long long* __restrict__ luma,
                                                          const int* __restrict__ prefix, const int* __restrict__ sel, unsigned char* __restrict__ out,
                                                          long img_off)
{
    __shared__ int s_mean;
    const ape_pose_train_job& j = bt.j[blockIdx.y];
    const int s = job0 + blockIdx.y;
    unsigned char* base = out + j.out_off;
    if (blockIdx.x < kImgBlocks) {                   // the normalised crop (:307-313), planar
        if (threadIdx.x == 0) s_mean = mean_from_partials(j.jit, luma + (long)s * kBlocks, H, W);
        __syncthreads();
        const int mean = s_mean;
        write_crop<kT>(bt, j, (float*)(base + img_off), [&](int x, int y, int& r, int& g, int& b) { pose_rgb_at(j, H, W, x, y, mean, r, g, b); });
        return;
    }
    const int pt = (blockIdx.x - kImgBlocks) * kWaves + (threadIdx.x >> 6);
    if (pt < N) sample_point<PosePoints>(j, H, W, pt, N, prefix + (long)s * H, sel[(long)s * N + pt], base);
}

bool job_ok(const ape_pose_train_job& j, int H, int W)
{
    if (!j.rgb || !j.depth || !j.label) return false;
    if (j.rot.mode == APE_ROT_AFFINE)
        for (int i = 0; i < 6; ++i)
            if (!(j.rot.a[i] == j.rot.a[i])) return false;                                // NaN: the depth's walk casts it to int
    return rotation_ok(j.rot, H, W) && jitter_ok(j.jit);
}

}  // namespace

extern "C" size_t ape_pose_train_extents_offset(int B) { return B < 1 ? 0 : (size_t)B * kBlocks * sizeof(unsigned long long); }

extern "C" size_t ape_pose_train_rows_offset(int B) { return kLayout.rows(B); }
extern "C" size_t ape_pose_train_tables_offset(int B, int H) { return kLayout.tables(B, H); }
extern "C" size_t ape_pose_train_sel_offset(int B, int H) { return kLayout.sel(B, H); }
extern "C" size_t ape_pose_train_workspace_bytes(int B, int H, int N) { return kLayout.end(B, H, N); }

extern "C" size_t ape_pose_train_image_offset(int N) { return N < 1 ? 0 : up16((size_t)N * 20); }

extern "C" size_t ape_pose_train_sample_bytes(int N, int Hc, int Wc)
{
    return N < 1 || Hc < 1 || Wc < 1 ? 0 : up16(ape_pose_train_image_offset(N) + (size_t)3 * Hc * Wc * sizeof(float));
}

extern "C" int ape_pose_train_stats(const ape_pose_train_job* jobs, int B, int H, int W, void* ws, size_t ws_bytes, void* stream)
{
    if (!frame_ok(B, H, W)) return APE_EINVAL;
    if (B == 0) return APE_OK;
    if (!jobs || !ws || ((uintptr_t)ws & 15)) return APE_EINVAL;
    if (ws_bytes < ape_pose_train_tables_offset(B, H)) return APE_EWORKSPACE;
    for (int i = 0; i < B; ++i)
        if (!job_ok(jobs[i], H, W)) return APE_EINVAL;
    PoseBatch bt = {};
    for_each_chunk(bt, jobs, B, [&](const PoseBatch& b, int i0, int nb) {
        hipLaunchKernelGGL(pose_stats_kernel, dim3(kBlocks, nb), dim3(kT), 0, (hipStream_t)stream, b, i0, H, W, (unsigned long long*)ws,
                           (int*)((char*)ws + ape_pose_train_extents_offset(B)), (int*)((char*)ws + ape_pose_train_rows_offset(B)));
    });
    return check_launch("ape_pose_train_stats");
}

extern "C" int ape_pose_train_samples(const ape_pose_train_job* jobs, int B, int H, int W, int N, const float* mean3_host, const float* std3_host,
                                      void* out, size_t out_bytes, void* ws, size_t ws_bytes, void* stream)
{
    PoseBatch bt = {};
    if (!frame_ok(B, H, W) || N < 1 || N > (1 << 24) || !norm_ok(mean3_host, std3_host, bt)) return APE_EINVAL;
    if (B == 0) return APE_OK;
    if (!jobs || !out || !ws || ((uintptr_t)out & 15) || ((uintptr_t)ws & 15)) return APE_EINVAL;
    if (ws_bytes < ape_pose_train_workspace_bytes(B, H, N)) return APE_EWORKSPACE;
    for (int i = 0; i < B; ++i) {
        const ape_pose_train_job& j = jobs[i];
        if (!job_ok(j, H, W) || !crop_ok(j, H, W) || !slot_ok(j, N, out_bytes)) return APE_EINVAL;
    }
    const int blocks = kImgBlocks + ceil_div(N, kWaves);
    const char* w = (const char*)ws;
    for_each_chunk(bt, jobs, B, [&](const PoseBatch& b, int i0, int nb) {
        hipLaunchKernelGGL(pose_samples_kernel, dim3(blocks, nb), dim3(kT), 0, (hipStream_t)stream, b, i0, H, W, N, (const unsigned long long*)ws,
                           (const int*)(w + ape_pose_train_tables_offset(B, H)), (const int*)(w + ape_pose_train_sel_offset(B, H)),
                           (unsigned char*)out, (long)ape_pose_train_image_offset(N));
    });
    return check_launch("ape_pose_train_samples");
}
