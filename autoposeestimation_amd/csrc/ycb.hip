// Samples of the YCB-Video data set, built on the device from resident frames (reference DenseFusion/datasets/ycb/dataset.py:97-232 and
// the per-roi samples of tools/eval_ycb.py:136-190).  The reference does this in Pillow and numpy on the host, per sample: up to five
// synthetic "front" frames tried as occluders of the multi-class label, an object drawn among those that keep more than 50 valid pixels,
// colour jitter, the get_bbox crop over the occluded label mask, a wrapping uint8 composite onto a real background (synthetic frames) and
// with the front, float64 pixel noise, `choose`, the float32 cloud and the normalised crop.  A batch is
//   ycb_overlap_kernel   per (label, front label, depth) triple the joint histogram [22][22][2] of (class, front class, depth != 0): LDS
//                        bins per workgroup (a wave adds each distinct key of its 64 pixels once), then one global integer add per
//                        non-zero bin.  The host reads from it which front candidate leaves more than 1000 labelled pixels and how many
//                        valid pixels every object keeps;
//   ycb_rows_kernel      one wave per row: the valid pixels of the row inside a window, the first and last member column, and the integer
//                        L sums that ImageEnhance.Contrast needs for the frame, the background and the front;
//   ycb_samples_kernel   workgroups 0..kImgBlocks-1 of a sample write the normalised crop, the others one chosen point per wave
//                        (sample_points.h, over the crop).
// The host only draws and does get_bbox's integer arithmetic between the launches.  Everything relies on -ffp-contract=off.
#include "sample_points.h"
#include "ycb_px.h"

namespace {

using namespace ape;

constexpr int kT = 256, kWaves = kT / 64;
constexpr int kClasses = 22;         // 0 (background) .. 21
constexpr int kBins = kClasses * kClasses * 2;
constexpr int kSrc = 3;              // jittered source images of a job: frame, background, front

using YcbBatch = SampleBatch<ape_ycb_job, 3>;
struct PairBatch {
    ape_ycb_pair j[kJobs];
};

// workspace: luma u64[B][kSrc][kBlocks] | rows i32[B][H][3] | prefix | sel | noise
constexpr SampleLayout kLayout = {kSrc * kBlocks * sizeof(unsigned long long), 3};

struct YcbPoints {
    static __device__ Window window(const ape_ycb_job& j, int, int) { return crop_window(j); }
    static __device__ bool valid(const ape_ycb_job& j, int, int W, int x, int y) { return ycb_valid(j, (long)y * W + x); }
    static __device__ void point(const ape_ycb_job& j, int, int W, int x, int y, float* q) { ycb_point(j, x, y, j.depth[(long)y * W + x], q); }
};

// grid (kBlocks, nb)
__global__ __launch_bounds__(kT) void ycb_overlap_kernel(PairBatch bt, int pair0, int HW, unsigned int* __restrict__ table)
{
    __shared__ unsigned int bins[kBins];
    const ape_ycb_pair& j = bt.j[blockIdx.y];
    for (int i = threadIdx.x; i < kBins; i += kT) bins[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int rounds = (HW + gridDim.x * kT - 1) / (gridDim.x * kT);        // the same for every lane: the ballots below stay whole
    for (int it = 0; it < rounds; ++it) {
        const int p = (it * gridDim.x + blockIdx.x) * kT + threadIdx.x;
        int key = -1;
        if (p < HW) {
            const int a = j.label[p], f = j.front_label ? j.front_label[p] : 0;
            if (a < kClasses && f < kClasses) key = (a * kClasses + f) * 2 + (j.depth[p] != 0);
        }
        unsigned long long todo = __ballot(key >= 0);
        while (todo) {                               // every distinct key of the wave once: a frame is mostly background
            const int lead = __ffsll((long long)todo) - 1;
            const int k = __shfl(key, lead, 64);
            const unsigned long long same = __ballot(key == k);
            if (lane == lead) atomicAdd(&bins[k], (unsigned int)__popcll(same));
            todo &= ~same;
        }
    }
    __syncthreads();
    unsigned int* out = table + (long)(pair0 + blockIdx.y) * kBins;
    for (int i = threadIdx.x; i < kBins; i += kT)
        if (bins[i]) atomicAdd(&out[i], bins[i]);
}

// grid (kBlocks, nb)
__global__ __launch_bounds__(kT) void ycb_rows_kernel(YcbBatch bt, int job0, int H, int W, unsigned long long* __restrict__ luma, int* __restrict__ rows)
{
    __shared__ unsigned long long red_s[kSrc][kWaves];
    const ape_ycb_job& j = bt.j[blockIdx.y];
    const uint8_t* src[kSrc] = {j.rgb, j.back_rgb, j.front_rgb};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long s[kSrc] = {0, 0, 0};
    int* row_out = rows + (long)(job0 + blockIdx.y) * H * 3;
    for (int y = blockIdx.x * kWaves + wave; y < H; y += gridDim.x * kWaves) {          // a row belongs to one wave
        for (int k = 0; k < kSrc; ++k) {
            if (!src[k]) continue;
            const ape_aug_jitter jit = ycb_jitter(j.jit[k]);
            const int kc = aug_contrast_at(jit);
            if (kc < 0) continue;                    // uniform per workgroup: the mean is over the whole image
            for (int x = lane; x < W; x += 64) {
                int r, g, b;
                aug_jittered_rgb(src[k], jit, W, x, y, kc, 0, r, g, b);
                s[k] += (unsigned long long)pil_luma(r, g, b);
            }
        }
        int cnt = 0, first = W, last = -1;
        const bool in_rows = y >= j.win_r0 && y < j.win_r1;
        for (int x = lane; x < W; x += 64) {
            const long p = (long)y * W + x;
            if (!ycb_member(j, p)) continue;
            first = Min()(first, x);
            last = Max()(last, x);
            cnt += in_rows && x >= j.win_c0 && x < j.win_c1 && j.depth[p] != 0;
        }
        for (int o = 32; o > 0; o >>= 1) {
            cnt += __shfl_down(cnt, o, 64);
            first = Min()(first, __shfl_down(first, o, 64));
            last = Max()(last, __shfl_down(last, o, 64));
        }
        if (lane == 0) { row_out[3 * y] = cnt; row_out[3 * y + 1] = first; row_out[3 * y + 2] = last; }
    }
    park(part<Sum>(s[0], red_s[0]), part<Sum>(s[1], red_s[1]), part<Sum>(s[2], red_s[2]));
    __syncthreads();
    if (threadIdx.x < kSrc)
        luma[((long)(job0 + blockIdx.y) * kSrc + threadIdx.x) * kBlocks + blockIdx.x] = total<kWaves, Sum>(red_s[threadIdx.x]);
}

// grid (kImgBlocks + ceil(N / kWaves), nb).  `prefix` and `sel` come from the caller through device memory, where the entry point cannot
// look at them: see sample_point; the rows and columns walked are those of the (checked) crop.
__global__ __launch_bounds__(kT) void ycb_samples_kernel(YcbBatch bt, int job0, int H, int W, int N, const unsigned long long* __restrict__ luma,
                                                         const int* __restrict__ prefix, const int* __restrict__ sel, const char* __restrict__ ws,
                                                         unsigned char* __restrict__ out, long img_off)
{
    __shared__ int s_mean[kSrc];
    const ape_ycb_job& j = bt.j[blockIdx.y];
    if (j.skip) return;
    const int s = job0 + blockIdx.y;
    unsigned char* base = out + j.out_off;
    if (blockIdx.x < kImgBlocks) {                   // the normalised crop (:150-167, :229), planar
        if (threadIdx.x < kSrc) {
            const uint8_t* src = threadIdx.x == 0 ? j.rgb : (threadIdx.x == 1 ? j.back_rgb : j.front_rgb);
            s_mean[threadIdx.x] = src ? mean_from_partials(ycb_jitter(j.jit[threadIdx.x]), luma + ((long)s * kSrc + threadIdx.x) * kBlocks, H, W) : 0;
        }
        __syncthreads();
        const int mean[kSrc] = {s_mean[0], s_mean[1], s_mean[2]};
        const int Wc = j.cmax - j.cmin;
        const long plane = (long)(j.rmax - j.rmin) * Wc;
        const double* noise = j.noise_off >= 0 ? (const double*)(ws + j.noise_off) : nullptr;
        float* img = (float*)(base + img_off);
        for (long i = (long)blockIdx.x * kT + threadIdx.x; i < plane; i += (long)kImgBlocks * kT) {
            const int r = (int)(i / Wc), c = (int)(i % Wc);
            int v[3];
            ycb_pixel(j, W, j.cmin + c, j.rmin + r, mean, v);
            for (int k = 0; k < 3; ++k) img[k * plane + i] = ycb_normalised(v[k], noise ? noise + k * plane + i : nullptr, bt.mean[k], bt.stdv[k]);
        }
        return;
    }
    const int pt = (blockIdx.x - kImgBlocks) * kWaves + (threadIdx.x >> 6);
    if (pt < N) sample_point<YcbPoints>(j, H, W, pt, N, prefix + (long)s * H, sel[(long)s * N + pt], base);
}

bool list_ok(const ape_ycb_jitter& c) { return jitter_ok(ycb_jitter(c)); }

// what both launches need of a job
bool job_ok(const ape_ycb_job& j, int H, int W)
{
    if (!j.rgb || !j.depth || !j.label || ((uintptr_t)j.depth & 1)) return false;
    if (!j.front_rgb != !j.front_label) return false;
    if (j.obj < 1 || j.obj >= kClasses) return false;
    const int lo = j.front_label ? 1 : 0;
    if (j.front_a < lo || j.front_a >= kClasses || j.front_b < lo || j.front_b >= kClasses) return false;
    if (j.win_r0 < 0 || j.win_r1 > H || j.win_r0 > j.win_r1 || j.win_c0 < 0 || j.win_c1 > W || j.win_c0 > j.win_c1) return false;
    if (!(j.cam_fx != 0.f) || !(j.cam_fy != 0.f) || !(j.cam_scale != 0.f)) return false;             // zero or NaN
    return list_ok(j.jit[0]) && list_ok(j.jit[1]) && list_ok(j.jit[2]);
}

}  // namespace

extern "C" int ape_ycb_overlap(const ape_ycb_pair* pairs, int P, int H, int W, uint32_t* table, void* stream)
{
    if (!frame_ok(P, H, W)) return APE_EINVAL;
    if (P == 0) return APE_OK;
    if (!pairs || !table || ((uintptr_t)table & 3)) return APE_EINVAL;
    for (int i = 0; i < P; ++i)
        if (!pairs[i].label || !pairs[i].depth || ((uintptr_t)pairs[i].depth & 1)) return APE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(table, 0, (size_t)P * kBins * sizeof(uint32_t), st) != hipSuccess) return check_launch("ape_ycb_overlap");
    PairBatch bt = {};
    for_each_chunk(bt, pairs, P, [&](const PairBatch& b, int i0, int nb) {
        hipLaunchKernelGGL(ycb_overlap_kernel, dim3(kBlocks, nb), dim3(kT), 0, st, b, i0, H * W, (unsigned int*)table);
    });
    return check_launch("ape_ycb_overlap");
}

extern "C" size_t ape_ycb_rows_offset(int B) { return kLayout.rows(B); }
extern "C" size_t ape_ycb_tables_offset(int B, int H) { return kLayout.tables(B, H); }
extern "C" size_t ape_ycb_sel_offset(int B, int H) { return kLayout.sel(B, H); }
extern "C" size_t ape_ycb_noise_offset(int B, int H, int N) { return kLayout.end(B, H, N); }

extern "C" int ape_ycb_rows(const ape_ycb_job* jobs, int B, int H, int W, void* ws, size_t ws_bytes, void* stream)
{
    if (!frame_ok(B, H, W)) return APE_EINVAL;
    if (B == 0) return APE_OK;
    if (!jobs || !ws || ((uintptr_t)ws & 15)) return APE_EINVAL;
    if (ws_bytes < ape_ycb_tables_offset(B, H)) return APE_EINVAL;     // (a size like the others: refused)
    for (int i = 0; i < B; ++i)
        if (!job_ok(jobs[i], H, W)) return APE_EINVAL;
    YcbBatch bt = {};
    for_each_chunk(bt, jobs, B, [&](const YcbBatch& b, int i0, int nb) {
        hipLaunchKernelGGL(ycb_rows_kernel, dim3(kBlocks, nb), dim3(kT), 0, (hipStream_t)stream, b, i0, H, W, (unsigned long long*)ws,
                           (int*)((char*)ws + ape_ycb_rows_offset(B)));
    });
    return check_launch("ape_ycb_rows");
}

extern "C" int ape_ycb_samples(const ape_ycb_job* jobs, int B, int H, int W, int N, const float* mean3_host, const float* std3_host, void* out,
                               size_t out_bytes, void* ws, size_t ws_bytes, void* stream)
{
    YcbBatch bt = {};
    if (!frame_ok(B, H, W) || N < 1 || N > (1 << 24) || !norm_ok(mean3_host, std3_host, bt)) return APE_EINVAL;
    if (B == 0) return APE_OK;
    if (!jobs || !out || !ws || ((uintptr_t)out & 15) || ((uintptr_t)ws & 15)) return APE_EINVAL;
    if (ws_bytes < ape_ycb_noise_offset(B, H, N)) return APE_EINVAL;     // (a size like the others: refused)
    for (int i = 0; i < B; ++i) {
        const ape_ycb_job& j = jobs[i];
        if (!job_ok(j, H, W)) return APE_EINVAL;
        if (j.skip) continue;
        if (!crop_ok(j, H, W) || !slot_ok(j, N, out_bytes)) return APE_EINVAL;
        if (j.noise_off >= 0) {
            const size_t nb = (size_t)24 * (j.rmax - j.rmin) * (j.cmax - j.cmin);
            if ((j.noise_off & 7) || (size_t)j.noise_off < ape_ycb_noise_offset(B, H, N) || (size_t)j.noise_off > ws_bytes
                || ws_bytes - (size_t)j.noise_off < nb)
                return APE_EINVAL;
        }
    }
    const int blocks = kImgBlocks + ceil_div(N, kWaves);
    const char* w = (const char*)ws;
    for_each_chunk(bt, jobs, B, [&](const YcbBatch& b, int i0, int nb) {
        hipLaunchKernelGGL(ycb_samples_kernel, dim3(blocks, nb), dim3(kT), 0, (hipStream_t)stream, b, i0, H, W, N, (const unsigned long long*)ws,
                           (const int*)(w + ape_ycb_tables_offset(B, H)), (const int*)(w + ape_ycb_sel_offset(B, H)), w, (unsigned char*)out,
                           (long)ape_pose_train_image_offset(N));
    });
    return check_launch("ape_ycb_samples");
}
