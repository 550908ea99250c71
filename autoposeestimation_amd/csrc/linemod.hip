// Samples of the LineMOD data set, built on the device from resident frames (reference DenseFusion/datasets/linemod/dataset.py:90-195).
// The reference does this in Pillow, numpy and OpenCV on the host, per sample: colour jitter of the full frame, the crop of get_bbox over
// the ground-truth `obj_bb` (or, in 'eval', over the bounding box of the largest contour of a segmentation result), the `choose` compaction
// of the valid pixels inside the crop with a drawn subset, the back-projection of the chosen pixels and the normalised crop.  Unlike the
// builder of pose_train.hip the crop does NOT come from the extents of the label, so label pixels lie outside it as a matter of course:
// counts and ranks are over the pixels inside the crop only.  A batch is
//   ape_linemod_boxes ('eval' only)  lm_mask_kernel (label == 255 of every frame into one byte image), the union-find labelling of ccl.h,
//                        lm_roots_kernel / lm_extent_kernel (per component the four extents, at its root: integer atomicMin / atomicMax),
//                        lm_pick_kernel (per frame one 64-bit atomicMax of (w * h, first pixel earliest)), lm_box_kernel -> [B][4];
//   lm_rows_kernel       one wave per row: the valid pixels of the row inside the crop, written by the wave that walked it, and the integer
//                        L sum that ImageEnhance.Contrast needs (one partial per workgroup, added in index order);
//   lm_samples_kernel    workgroups 0..kImgBlocks-1 of a sample write the normalised crop, the others one chosen point per wave
//                        (sample_points.h, over the crop).
// The host only draws and does get_bbox's integer arithmetic between the launches.  Everything relies on -ffp-contract=off.
#include "sample_points.h"
#include "ccl.h"

namespace {

using namespace ape;

constexpr int kT = 256, kWaves = kT / 64;

using LmBatch = SampleBatch<ape_linemod_job, 3>;

// workspace: luma u64[B][kBlocks] | rows i32[B][H] | prefix | sel
constexpr SampleLayout kLayout = {kBlocks * sizeof(unsigned long long), 1};

struct LabelTable {
    const uint8_t* p[kJobs];
};

constexpr int kGridCap = 16384;        // most workgroups of a grid-stride launch (ape::grid_for)

// ---- largest-contour box -------------------------------------------------------------------------------------------------------------
// grid (gx, nb): mask[f0 + y][q] = label == 255
__global__ __launch_bounds__(kT) void lm_mask_kernel(LabelTable tb, int f0, int HW, uint8_t* __restrict__ mask)
{
    const uint8_t* lab = tb.p[blockIdx.y];
    uint8_t* out = mask + (long)(f0 + blockIdx.y) * HW;
    for (int q = blockIdx.x * kT + threadIdx.x; q < HW; q += gridDim.x * kT) out[q] = lab[q] == 255 ? 1 : 0;
}

// a root owns the extents of its component: (min row, max row, min column, max column) at ext[4 * root]
__global__ __launch_bounds__(kT) void lm_roots_kernel(const int* __restrict__ L, int* __restrict__ ext, unsigned long long* __restrict__ best,
                                                      int B, long npix)
{
    for (long p = blockIdx.x * (long)kT + threadIdx.x; p < npix; p += (long)gridDim.x * kT) {
        if (p < B) best[p] = 0ull;
        if (L[p] != (int)p) continue;
        int* e = ext + p * 4;
        e[0] = INT_MAX; e[1] = -1; e[2] = INT_MAX; e[3] = -1;
    }
}

// only the ends of a component's row runs can move its extents
__global__ __launch_bounds__(kT) void lm_extent_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ L, int* __restrict__ ext,
                                                       int H, int W, long npix)
{
    for (long p = blockIdx.x * (long)kT + threadIdx.x; p < npix; p += (long)gridDim.x * kT) {
        const int root = L[p];
        if (root < 0) continue;
        const int x = (int)(p % W), y = (int)((p / W) % H);
        int* e = ext + (long)root * 4;
        if (x == 0 || !mask[p - 1]) { atomicMin(&e[0], y); atomicMax(&e[1], y); atomicMin(&e[2], x); }
        if (x == W - 1 || !mask[p + 1]) atomicMax(&e[3], x);
    }
}

// per frame the largest w * h; among equals the smallest root = the component whose first pixel comes first in raster order
__global__ __launch_bounds__(kT) void lm_pick_kernel(const int* __restrict__ L, const int* __restrict__ ext, unsigned long long* __restrict__ best,
                                                     int HW, long npix)
{
    for (long p = blockIdx.x * (long)kT + threadIdx.x; p < npix; p += (long)gridDim.x * kT) {
        if (L[p] != (int)p) continue;
        const int* e = ext + p * 4;
        const int b = (int)(p / HW);
        const unsigned long long area = (unsigned long long)(e[3] - e[2] + 1) * (unsigned long long)(e[1] - e[0] + 1);
        const unsigned int first = 0x7fffffffu - (unsigned int)(p - (long)b * HW);
        atomicMax(&best[b], (area << 32) | (unsigned long long)first);
    }
}

__global__ void lm_box_kernel(const int* __restrict__ ext, const unsigned long long* __restrict__ best, int* __restrict__ boxes, int B, int HW)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int* o = boxes + b * 4;
    const unsigned long long key = best[b];
    if (!key) { o[0] = o[1] = o[2] = o[3] = 0; return; }
    const long root = (long)b * HW + (long)(0x7fffffffu - (unsigned int)(key & 0xffffffffull));
    const int* e = ext + root * 4;
    o[0] = e[2]; o[1] = e[0]; o[2] = e[3] - e[2] + 1; o[3] = e[1] - e[0] + 1;      // cv2.boundingRect: x, y, w, h
}

// ---- samples ---------------------------------------------------------------------------------------------------------------------------
// `mask_label * mask_depth` (dataset.py:106-112): band 0 of the label == 255 and depth != 0
__device__ __forceinline__ bool lm_valid(const ape_linemod_job& j, int W, int x, int y)
{
    const long p = (long)y * W + x;
    return j.label[p * j.label_bands] == 255 && j.depth[p] != 0;
}

// dataset.py:147-160 as numpy computes it in float32: `depth / cam_scale`, `(col - cx) * z / fx`, `(row - cy) * z / fy`, the whole cloud
// `/ 1000.0`; the translation noise is added in float64 (numpy promotes the float32 cloud) and `astype(float32)` rounds once
__device__ __forceinline__ void lm_point(const ape_linemod_job& j, int x, int y, int d, float* p)
{
    const float pt2 = (float)d / j.cam_scale;
    const float pt0 = ((float)x - j.cam_cx) * pt2 / j.cam_fx;
    const float pt1 = ((float)y - j.cam_cy) * pt2 / j.cam_fy;
    p[0] = pt0 / 1000.0f; p[1] = pt1 / 1000.0f; p[2] = pt2 / 1000.0f;
    if (j.add_noise)
        for (int k = 0; k < 3; ++k) p[k] = (float)((double)p[k] + j.add_t[k]);
}

struct LmPoints {
    static __device__ Window window(const ape_linemod_job& j, int, int) { return crop_window(j); }
    static __device__ bool valid(const ape_linemod_job& j, int, int W, int x, int y) { return lm_valid(j, W, x, y); }
    static __device__ void point(const ape_linemod_job& j, int, int W, int x, int y, float* q) { lm_point(j, x, y, j.depth[(long)y * W + x], q); }
};

// grid (kBlocks, nb)
__global__ __launch_bounds__(kT) void lm_rows_kernel(LmBatch bt, int job0, int H, int W, unsigned long long* __restrict__ luma, int* __restrict__ rows)
{
    __shared__ unsigned long long red_s[kWaves];
    const ape_linemod_job& j = bt.j[blockIdx.y];
    const int kc = aug_contrast_at(j.jit);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long s = 0;
    int* row_out = rows + (long)(job0 + blockIdx.y) * H;
    for (int y = blockIdx.x * kWaves + wave; y < H; y += gridDim.x * kWaves) {          // a row belongs to one wave
        if (kc >= 0) {                               // uniform per workgroup: the mean is over the whole frame
            for (int x = lane; x < W; x += 64) {
                int r, g, b;
                aug_jittered_rgb(j.rgb, j.jit, W, x, y, kc, 0, r, g, b);
                s += (unsigned long long)pil_luma(r, g, b);
            }
        }
        int cnt = 0;
        if (y >= j.rmin && y < j.rmax)
            for (int x = j.cmin + lane; x < j.cmax; x += 64) cnt += lm_valid(j, W, x, y);
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
        if (lane == 0) row_out[y] = cnt;
    }
    park(part<Sum>(s, red_s));
    __syncthreads();
    if (threadIdx.x == 0) luma[(long)(job0 + blockIdx.y) * kBlocks + blockIdx.x] = total<kWaves, Sum>(red_s);
}

// grid (kImgBlocks + ceil(N / kWaves), nb).  `prefix` and `sel` come from the caller through device memory, where the entry point cannot
// look at them: see sample_point; the rows and columns walked are those of the (checked) crop.
__global__ __launch_bounds__(kT) void lm_samples_kernel(LmBatch bt, int job0, int H, int W, int N, const unsigned long long* __restrict__ luma,
                                                        const int* __restrict__ prefix, const int* __restrict__ sel, unsigned char* __restrict__ out,
                                                        long img_off)
{
    __shared__ int s_mean;
    const ape_linemod_job& j = bt.j[blockIdx.y];
    if (j.skip) return;
    const int s = job0 + blockIdx.y;
    unsigned char* base = out + j.out_off;
    if (blockIdx.x < kImgBlocks) {                   // the normalised crop (:117-126, :192), planar
        if (threadIdx.x == 0) s_mean = j.add_noise ? mean_from_partials(j.jit, luma + (long)s * kBlocks, H, W) : 0;
        __syncthreads();
        const int mean = s_mean;
        const int n_ops = j.add_noise ? j.jit.n_ops : 0;
        write_crop<kT>(bt, j, (float*)(base + img_off),
                       [&](int x, int y, int& r, int& g, int& b) { aug_jittered_rgb(j.rgb, j.jit, W, x, y, n_ops, mean, r, g, b); });
        return;
    }
    const int pt = (blockIdx.x - kImgBlocks) * kWaves + (threadIdx.x >> 6);
    if (pt < N) sample_point<LmPoints>(j, H, W, pt, N, prefix + (long)s * H, sel[(long)s * N + pt], base);
}

bool job_ok(const ape_linemod_job& j, int H, int W)
{
    if (!j.rgb || !j.depth || !j.label || j.label_bands < 1 || j.label_bands > 4) return false;
    if (!(j.cam_fx != 0.f) || !(j.cam_fy != 0.f) || !(j.cam_scale != 0.f)) return false;             // zero or NaN
    return jitter_ok(j.jit) && crop_ok(j, H, W);
}

}  // namespace

extern "C" size_t ape_linemod_box_workspace_bytes(int B, int H, int W)
{
    if (B < 1 || H < 1 || W < 1) return 0;
    const size_t npix = (size_t)B * H * W;
    // L i32[npix] | ext i32[npix][4] | best u64[B] | mask u8[npix]
    return up16(npix * 20) + up16((size_t)B * 8) + up16(npix);
}

extern "C" int ape_linemod_boxes(const void* const* labels_host, int B, int H, int W, int* boxes, void* ws, size_t ws_bytes, void* stream)
{
    if (!frame_ok(B, H, W)) return APE_EINVAL;
    if (B == 0) return APE_OK;
    if (!labels_host || !boxes || !ws || ((uintptr_t)ws & 15) || ((uintptr_t)boxes & 3)) return APE_EINVAL;
    const long npix = (long)B * H * W;
    if (npix >= (1L << 31) - 1) return APE_EINVAL;
    for (int i = 0; i < B; ++i)
        if (!labels_host[i]) return APE_EINVAL;
    if (ws_bytes < ape_linemod_box_workspace_bytes(B, H, W)) return APE_EINVAL;     // (a size like the others: refused)
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    int* L = (int*)w;
    int* ext = (int*)(w + npix * 4);
    unsigned long long* best = (unsigned long long*)(w + up16((size_t)npix * 20));
    uint8_t* mask = (uint8_t*)(w + up16((size_t)npix * 20) + up16((size_t)B * 8));
    const int HW = H * W;
    int gx = ceil_div(HW, kT);
    gx = gx > 256 ? 256 : gx;
    for (int f0 = 0; f0 < B; f0 += kJobs) {
        const int nb = B - f0 < kJobs ? B - f0 : kJobs;
        LabelTable tb = {};
        for (int i = 0; i < nb; ++i) tb.p[i] = (const uint8_t*)labels_host[f0 + i];
        hipLaunchKernelGGL(lm_mask_kernel, dim3(gx, nb), dim3(kT), 0, st, tb, f0, HW, mask);
    }
    const int g = ape::grid_for(npix, kT, kGridCap);
    hipLaunchKernelGGL(ccl_init_kernel, dim3(g), dim3(kT), 0, st, mask, L, W, npix);
    hipLaunchKernelGGL(ccl_merge_kernel, dim3(g), dim3(kT), 0, st, mask, L, H, W, npix);
    hipLaunchKernelGGL(ccl_compress_kernel, dim3(g), dim3(kT), 0, st, L, npix, (unsigned long long*)nullptr, (unsigned int*)nullptr);
    hipLaunchKernelGGL(lm_roots_kernel, dim3(g), dim3(kT), 0, st, L, ext, best, B, npix);
    hipLaunchKernelGGL(lm_extent_kernel, dim3(g), dim3(kT), 0, st, mask, L, ext, H, W, npix);
    hipLaunchKernelGGL(lm_pick_kernel, dim3(g), dim3(kT), 0, st, L, ext, best, HW, npix);
    hipLaunchKernelGGL(lm_box_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, st, ext, best, boxes, B, HW);
    return check_launch("ape_linemod_boxes");
}

extern "C" size_t ape_linemod_rows_offset(int B) { return kLayout.rows(B); }
extern "C" size_t ape_linemod_tables_offset(int B, int H) { return kLayout.tables(B, H); }
extern "C" size_t ape_linemod_sel_offset(int B, int H) { return kLayout.sel(B, H); }
extern "C" size_t ape_linemod_workspace_bytes(int B, int H, int N) { return kLayout.end(B, H, N); }

extern "C" int ape_linemod_rows(const ape_linemod_job* jobs, int B, int H, int W, void* ws, size_t ws_bytes, void* stream)
{
    if (!frame_ok(B, H, W)) return APE_EINVAL;
    if (B == 0) return APE_OK;
    if (!jobs || !ws || ((uintptr_t)ws & 15)) return APE_EINVAL;
    if (ws_bytes < ape_linemod_tables_offset(B, H)) return APE_EINVAL;     // (a size like the others: refused)
    for (int i = 0; i < B; ++i)
        if (!job_ok(jobs[i], H, W)) return APE_EINVAL;
    LmBatch bt = {};
    for_each_chunk(bt, jobs, B, [&](const LmBatch& b, int i0, int nb) {
        hipLaunchKernelGGL(lm_rows_kernel, dim3(kBlocks, nb), dim3(kT), 0, (hipStream_t)stream, b, i0, H, W, (unsigned long long*)ws,
                           (int*)((char*)ws + ape_linemod_rows_offset(B)));
    });
    return check_launch("ape_linemod_rows");
}

extern "C" int ape_linemod_samples(const ape_linemod_job* jobs, int B, int H, int W, int N, const float* mean3_host, const float* std3_host,
                                   void* out, size_t out_bytes, void* ws, size_t ws_bytes, void* stream)
{
    LmBatch bt = {};
    if (!frame_ok(B, H, W) || N < 1 || N > (1 << 24) || !norm_ok(mean3_host, std3_host, bt)) return APE_EINVAL;
    if (B == 0) return APE_OK;
    if (!jobs || !out || !ws || ((uintptr_t)out & 15) || ((uintptr_t)ws & 15)) return APE_EINVAL;
    if (ws_bytes < ape_linemod_workspace_bytes(B, H, N)) return APE_EINVAL;     // (a size like the others: refused)
    for (int i = 0; i < B; ++i) {
        const ape_linemod_job& j = jobs[i];
        if (!job_ok(j, H, W)) return APE_EINVAL;
        if (!j.skip && !slot_ok(j, N, out_bytes)) return APE_EINVAL;
    }
    const int blocks = kImgBlocks + ceil_div(N, kWaves);
    const char* w = (const char*)ws;
    for_each_chunk(bt, jobs, B, [&](const LmBatch& b, int i0, int nb) {
        hipLaunchKernelGGL(lm_samples_kernel, dim3(blocks, nb), dim3(kT), 0, (hipStream_t)stream, b, i0, H, W, N, (const unsigned long long*)ws,
                           (const int*)(w + ape_linemod_tables_offset(B, H)), (const int*)(w + ape_linemod_sel_offset(B, H)),
                           (unsigned char*)out, (long)ape_pose_train_image_offset(N));
    });
    return check_launch("ape_linemod_samples");
}
