// The live view's two overlay images on the device (pipeline/utils.py:471-476,510-513,576-585 with
// pc_reconstruction/open3d_utils.py:233-270), and the arithmetic of the two label-review screens (pipeline/utils.py:280-286,362):
//   stamp_counts  per object: R.p + t of every model point in float64 (one rounding per multiply and add), the pin-hole projection with
//                 int() truncation (points2pixel), and one integer atomic per stamp CENTRE whose whole point_size x point_size stamp
//                 lies inside the image (pointcloud2image skips the others) into the object's count plane
//   blend         per pixel: the class tint `v*0.7 + colour*0.3` of the segmentation image; and for the frame's objects in list order
//                 k = the object's centre counts summed over the point_size x point_size neighbourhood = the number of stamps that cover
//                 the pixel, then `v = mark*0.3 + v*0.7` k times (all stamps of an object carry one colour, so their order is immaterial)
// Count planes: planes[J][B][H][W] u32, plane j of frame b = the j-th object of that frame.  The stamp call clears them first
// (hipMemsetAsync on the caller's stream), so a workspace may hold anything.  Integer atomics only: the images are a function of the
// inputs, bit for bit, whatever order the adds arrive in.
#include "common.h"
#include <stdio.h>

namespace {

constexpr int OBJ_CHUNK = 64;       // objects per stamp launch: their table travels in the kernel arguments (1 KB)
struct ObjChunk { int32_t v[OBJ_CHUNK][4]; };   // (frame, first cloud row, cloud rows, plane)

constexpr double EPS4 = 2.220446049250313e-16 * 4.0;   // transformations._EPS

// lib/transformations.py:1254-1278 (quaternion_matrix): nq = q.q, identity below _EPS, q *= sqrt(2 / nq), the nine terms
__device__ __forceinline__ void quaternion_rows(const double* __restrict__ q7, double R[9])
{
    double w = q7[0], x = q7[1], y = q7[2], z = q7[3];
    const double nq = ((w * w + x * x) + y * y) + z * z;
    if (nq < EPS4) {
        R[0] = 1.0; R[1] = 0.0; R[2] = 0.0; R[3] = 0.0; R[4] = 1.0; R[5] = 0.0; R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
        return;
    }
    const double s = sqrt(2.0 / nq);
    w *= s; x *= s; y *= s; z *= s;
    R[0] = (1.0 - y * y) - z * z; R[1] = x * y - z * w;         R[2] = x * z + y * w;
    R[3] = x * y + z * w;         R[4] = (1.0 - x * x) - z * z; R[5] = y * z - x * w;
    R[6] = x * z - y * w;         R[7] = y * z + x * w;         R[8] = (1.0 - x * x) - y * y;
}

// a projected coordinate that int() can take and an int32 can hold (the reference raises on the others)
__device__ __forceinline__ bool pixel_ok(double u) { return u > -2147483649.0 && u < 2147483648.0; }

__global__ void __launch_bounds__(256)
overlay_stamp_counts_kernel(ObjChunk chunk, int first_obj, const double* __restrict__ clouds, const double* __restrict__ pose,
                            int pose_form, const int32_t* __restrict__ n_cand, double fx, double fy, double ppx, double ppy, int step,
                            unsigned* __restrict__ planes, int B, int H, int W)
{
    const int oc = blockIdx.y;
    const int frame = chunk.v[oc][0], off = chunk.v[oc][1], len = chunk.v[oc][2], plane = chunk.v[oc][3];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const int o = first_obj + oc;
    if (n_cand && n_cand[o] <= 0) return;
    double R[9], t[3];
    if (pose_form == 0) {
        const double* q7 = pose + (size_t)o * 7;
        quaternion_rows(q7, R);
        t[0] = q7[4]; t[1] = q7[5]; t[2] = q7[6];
    } else {
        const double* m = pose + (size_t)o * 12;
        R[0] = m[0]; R[1] = m[1]; R[2] = m[2];  t[0] = m[3];
        R[3] = m[4]; R[4] = m[5]; R[5] = m[6];  t[1] = m[7];
        R[6] = m[8]; R[7] = m[9]; R[8] = m[10]; t[2] = m[11];
    }
    const double* p = clouds + ((size_t)off + i) * 3;
    const double p0 = p[0], p1 = p[1], p2 = p[2];
    const double x = ((p0 * R[0] + p1 * R[1]) + p2 * R[2]) + t[0];
    const double y = ((p0 * R[3] + p1 * R[4]) + p2 * R[5]) + t[1];
    const double z = ((p0 * R[6] + p1 * R[7]) + p2 * R[8]) + t[2];
    if (z == 0.0) return;
    const double u = x / (z / fx) + ppx;
    const double v = y / (z / fy) + ppy;
    if (!pixel_ok(u) || !pixel_ok(v)) return;       // (NaN fails both comparisons)
    const long long col = (long long)u, row = (long long)v;
    if (row - step < 0 || col - step < 0 || row + step + 1 > H || col + step + 1 > W) return;
    atomicAdd(planes + (((size_t)plane * B + frame) * H + (size_t)row) * W + (size_t)col, 1u);
}

__device__ __forceinline__ uint8_t clip_u8(double v) { return (uint8_t)(int)(v < 0.0 ? 0.0 : v > 255.0 ? 255.0 : v); }

// `v = mark*0.3 + v*0.7`, k times, on one channel.  The loop leaves early only at a true fixed point (the application returned its
// input bit for bit: every later one would too).
__device__ __forceinline__ double blend_f64(double v, double m03, unsigned k)
{
    for (unsigned i = 0; i < k; ++i) {
        const double nv = m03 + v * 0.7;
        if (nv == v) break;
        v = nv;
    }
    return v;
}
__device__ __forceinline__ uint8_t blend_u8(uint8_t v, double m03, unsigned k)
{
    for (unsigned i = 0; i < k; ++i) {
        const uint8_t nv = (uint8_t)(int)(m03 + (double)v * 0.7);       // numpy's float64 -> uint8 assignment of a value in 0..255
        if (nv == v) break;
        v = nv;
    }
    return v;
}

struct BlendArgs {
    const uint8_t* rgb; const uint8_t* objmap; const int32_t* slot_obj; const int32_t* obj_cls; const double* seg_colour;
    const double* mark; const int32_t* n_cand; const unsigned* planes; uint8_t* seg_out; uint8_t* pose_out;
    int n, J, B, H, W, step, mode;
};

// one pixel: in[3] -> seg[3], pos[3]
__device__ __forceinline__ void blend_pixel(const BlendArgs& a, long px, const uint8_t in[3], uint8_t seg[3], uint8_t pos[3])
{
    const int hw = a.H * a.W;
    const int b = (int)(px / hw);
    const int r = (int)(px - (long)b * hw);
    const int y = r / a.W, x = r - y * a.W;
    const int cls = a.objmap ? (int)a.objmap[px] : 0;
    seg[0] = in[0]; seg[1] = in[1]; seg[2] = in[2];
    double vf[3] = {(double)in[0], (double)in[1], (double)in[2]};
    uint8_t vu[3] = {in[0], in[1], in[2]};
    bool tinted = false;
    for (int j = 0; j < a.J; ++j) {
        const int o = a.slot_obj[b * a.J + j];
        if (o < 0 || o >= a.n) continue;
        if (a.n_cand && a.n_cand[o] <= 0) continue;
        if (!tinted && cls > 0 && a.obj_cls[o] == cls) {
            tinted = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double col = a.seg_colour ? a.seg_colour[(size_t)o * 3 + c] : (c == 0 ? 255.0 : 0.0);
                const double f = (double)in[c] * 0.7 + col * 0.3;
                seg[c] = a.mode == 0 ? clip_u8(f) : (uint8_t)(int)f;
            }
        }
        const unsigned* pl = a.planes + ((size_t)j * a.B + b) * hw;
        unsigned k = 0;
        const int y0 = max(y - a.step, 0), y1 = min(y + a.step, a.H - 1), x0 = max(x - a.step, 0), x1 = min(x + a.step, a.W - 1);
        for (int yy = y0; yy <= y1; ++yy)
            for (int xx = x0; xx <= x1; ++xx) k += pl[yy * a.W + xx];
        if (k == 0) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double m03 = (a.mark ? a.mark[(size_t)o * 3 + c] : (c == 0 ? 255.0 : 0.0)) * 0.3;
            if (a.mode == 0) vf[c] = blend_f64(vf[c], m03, k);
            else vu[c] = blend_u8(vu[c], m03, k);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[c] = a.mode == 0 ? clip_u8(vf[c]) : vu[c];
}

// four pixels = three dwords per thread and image; the pixels past the last full group by the last threads, byte by byte
__global__ void __launch_bounds__(256)
overlay_blend_kernel(BlendArgs a, long n_pixels)
{
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long groups = n_pixels / 4;
    if (g < groups) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.rgb) + g * 3;
        uint32_t w[3] = {src[0], src[1], src[2]}, so[3] = {0, 0, 0}, po[3] = {0, 0, 0};
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            uint8_t in[3], seg[3], pos[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) in[c] = (uint8_t)(w[(p * 3 + c) >> 2] >> (8 * ((p * 3 + c) & 3)));
            blend_pixel(a, g * 4 + p, in, seg, pos);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                so[(p * 3 + c) >> 2] |= (uint32_t)seg[c] << (8 * ((p * 3 + c) & 3));
                po[(p * 3 + c) >> 2] |= (uint32_t)pos[c] << (8 * ((p * 3 + c) & 3));
            }
        }
        uint32_t* sd = reinterpret_cast<uint32_t*>(a.seg_out) + g * 3;
        uint32_t* pd = reinterpret_cast<uint32_t*>(a.pose_out) + g * 3;
        sd[0] = so[0]; sd[1] = so[1]; sd[2] = so[2];
        pd[0] = po[0]; pd[1] = po[1]; pd[2] = po[2];
    } else {
        const long px = groups * 4 + (g - groups);
        if (px >= n_pixels) return;
        uint8_t in[3] = {a.rgb[px * 3], a.rgb[px * 3 + 1], a.rgb[px * 3 + 2]}, seg[3], pos[3];
        blend_pixel(a, px, in, seg, pos);
        for (int c = 0; c < 3; ++c) {
            a.seg_out[px * 3 + c] = seg[c];
            a.pose_out[px * 3 + c] = pos[c];
        }
    }
}

int refuse(const char* fn, const char* why)
{
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: %s", fn, why);
    ape::set_last_error(msg);
    return APE_EINVAL;
}

// (pixel indices inside one plane set are ints; the plane index times B*H*W is a size_t)
bool planes_fit(int J, int B, int H, int W) { return J <= 4096 && (double)B * H * W < 2147483648.0; }

}  // namespace

extern "C" int ape_overlay_stamp_counts_f64(const int32_t* objs_host, int n, const double* clouds, long total_points, const double* pose,
                                            int pose_form, const int32_t* n_cand, double fx, double fy, double ppx, double ppy,
                                            int point_size, uint32_t* planes, int J, int B, int H, int W, void* stream)
{
    static const char* fn = "ape_overlay_stamp_counts_f64";
    if (!planes) return refuse(fn, "planes is null");
    if (B <= 0 || H <= 0 || W <= 0 || J <= 0 || !planes_fit(J, B, H, W)) return refuse(fn, "B, H, W and J must be positive (and the planes addressable)");
    if (point_size < 1 || !(point_size & 1)) return refuse(fn, "point_size must be odd and >= 1");
    if (n < 0 || total_points < 0 || (pose_form != 0 && pose_form != 1)) return refuse(fn, "negative count or unknown pose form");
    if (n > 0 && (!objs_host || !clouds || !pose)) return refuse(fn, "objs_host, clouds or pose is null");
    if (((uintptr_t)planes & 3) || ((uintptr_t)clouds & 7) || ((uintptr_t)pose & 7) || ((uintptr_t)n_cand & 3)) return refuse(fn, "misaligned pointer");
    int max_len = 0;
    for (int i = 0; i < n; ++i) {
        const int32_t* o = objs_host + (size_t)i * 4;
        if (o[0] < 0 || o[0] >= B) return refuse(fn, "an object's frame index is outside 0..B-1");
        if (o[1] < 0 || o[2] < 0 || (long)o[1] + (long)o[2] > total_points) return refuse(fn, "an object's cloud rows leave the cloud array");
        if (o[3] < 0 || o[3] >= J) return refuse(fn, "an object's plane is outside 0..J-1");
        if (o[2] > max_len) max_len = o[2];
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(planes, 0, (size_t)J * B * H * W * sizeof(uint32_t), st) != hipSuccess) {
        ape::set_last_error("ape_overlay_stamp_counts_f64: hipMemsetAsync of the count planes");
        return APE_ELAUNCH;
    }
    if (max_len == 0) return APE_OK;
    for (int first = 0; first < n; first += OBJ_CHUNK) {
        const int m = n - first < OBJ_CHUNK ? n - first : OBJ_CHUNK;
        ObjChunk chunk;
        int len = 0;
        for (int i = 0; i < OBJ_CHUNK; ++i)
            for (int k = 0; k < 4; ++k) chunk.v[i][k] = i < m ? objs_host[(size_t)(first + i) * 4 + k] : 0;
        for (int i = 0; i < m; ++i) len = chunk.v[i][2] > len ? chunk.v[i][2] : len;
        if (len == 0) continue;
        hipLaunchKernelGGL(overlay_stamp_counts_kernel, dim3(ape::ceil_div(len, 256), m), dim3(256), 0, st, chunk, first, clouds, pose,
                           pose_form, n_cand, fx, fy, ppx, ppy, (point_size - 1) / 2, planes, B, H, W);
        const int rc = ape::check_launch(fn);
        if (rc != APE_OK) return rc;
    }
    return APE_OK;
}

extern "C" int ape_overlay_blend_u8(const uint8_t* rgb, const uint8_t* objmap, const int32_t* slot_obj, const int32_t* obj_cls,
                                    const double* seg_colour, const double* mark, const int32_t* n_cand, int n, const uint32_t* planes,
                                    int J, int B, int H, int W, int point_size, int mode, uint8_t* seg_out, uint8_t* pose_out, void* stream)
{
    static const char* fn = "ape_overlay_blend_u8";
    if (!rgb || !slot_obj || !planes || !seg_out || !pose_out) return refuse(fn, "rgb, slot_obj, planes, seg_out or pose_out is null");
    if (B <= 0 || H <= 0 || W <= 0 || J <= 0 || !planes_fit(J, B, H, W)) return refuse(fn, "B, H, W and J must be positive (and the planes addressable)");
    if (point_size < 1 || !(point_size & 1)) return refuse(fn, "point_size must be odd and >= 1");
    if (n < 0 || (mode != 0 && mode != 1)) return refuse(fn, "negative object count or unknown mode");
    if (n > 0 && !obj_cls) return refuse(fn, "obj_cls is null");
    if (((uintptr_t)rgb & 3) || ((uintptr_t)seg_out & 3) || ((uintptr_t)pose_out & 3) || ((uintptr_t)planes & 3) || ((uintptr_t)slot_obj & 3) ||
        ((uintptr_t)obj_cls & 3) || ((uintptr_t)n_cand & 3) || ((uintptr_t)seg_colour & 7) || ((uintptr_t)mark & 7))
        return refuse(fn, "misaligned pointer");
    if (rgb == seg_out || rgb == pose_out || seg_out == pose_out) return refuse(fn, "the images must be three buffers");
    BlendArgs a = {rgb, objmap, slot_obj, obj_cls, seg_colour, mark, n_cand, planes, seg_out, pose_out, n, J, B, H, W, (point_size - 1) / 2, mode};
    const long n_pixels = (long)B * H * W;
    const long threads = n_pixels / 4 + n_pixels % 4;
    hipLaunchKernelGGL(overlay_blend_kernel, dim3(ape::ceil_div(threads, 256)), dim3(256), 0, (hipStream_t)stream, a, n_pixels);
    return ape::check_launch(fn);
}
