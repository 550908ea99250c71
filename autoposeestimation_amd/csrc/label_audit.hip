// Label-quality audit on the device (experiments/gt_test.py of the reference):
//   pair_counts  compute_IoU's four pixel counts (:160-194) for every sample of a batch and every pair of its label planes, in one pass
//                over the planes: 16 pixels per lane and step, every plane read once with one 16-byte load, its non-zero bytes folded
//                into bit p of a per-pixel byte; a pair (a, b) is then two shifts, three ANDs and three population counts per dword.
//                Lane counters are registers, waves reduce by shuffles, the workgroup in LDS, and one 64-bit integer atomic per
//                counter and workgroup reaches memory.  Integer sums: the result does not depend on the order of arrival.
//   pair_blend   the comparison image of :105-120 (dead code upstream behind plot_labels = False): two label planes tinted into two
//                channels of the colour frame, float64, product and sum as separate roundings, the second step reading the first's.
// Plane p of sample b starts at byte (b L + p) HW: any alignment.  The 16-byte loads are therefore issued at byte granularity
// (global loads on gfx950 take any address); the last partial group of a plane is read byte by byte, never past the plane's end.
#include "common.h"
#include <stdio.h>
#include <string.h>

namespace {

constexpr int MAX_L = 8, MAX_P = 16;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int PX_PER_STEP = THREADS * 16;      // pixels a workgroup takes per step
constexpr int STEPS = 2;                       // steps per workgroup: 8192 pixels of one sample

struct PairTable { uint8_t a[MAX_P], b[MAX_P]; };

// 0x01 in every byte of x that is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x)
{
    return ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u) >> 7;
}

__device__ __forceinline__ uint4 load16(const uint8_t* __restrict__ p)
{
    uint4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

__global__ void __launch_bounds__(THREADS)
label_pair_counts_kernel(const uint8_t* __restrict__ labels, int L, int HW, int blocks_per_sample, PairTable pairs, int P,
                         unsigned long long* __restrict__ counts)
{
    __shared__ uint32_t part[WAVES][MAX_P][3];
    const int b = blockIdx.x / blocks_per_sample;
    const long first = (long)(blockIdx.x - b * blocks_per_sample) * (PX_PER_STEP * STEPS);
    const long last = min((long)HW, first + PX_PER_STEP * STEPS);       // this workgroup's pixels of sample b: first .. last-1
    const uint8_t* __restrict__ base = labels + (size_t)b * L * HW;
    uint32_t n_a[MAX_P], n_b[MAX_P], n_ab[MAX_P];
#pragma unroll
    for (int j = 0; j < MAX_P; ++j) n_a[j] = n_b[j] = n_ab[j] = 0;

    for (long px = first + (long)threadIdx.x * 16; px < last; px += PX_PER_STEP) {
        uint32_t w[4] = {0, 0, 0, 0};                                   // byte i: bit p = plane p is foreground at pixel px + i
        if (px + 16 <= last) {
#pragma unroll
            for (int p = 0; p < MAX_L; ++p) {
                if (p < L) {
                    const uint4 v = load16(base + (size_t)p * HW + px);
                    w[0] |= nonzero_bytes(v.x) << p;
                    w[1] |= nonzero_bytes(v.y) << p;
                    w[2] |= nonzero_bytes(v.z) << p;
                    w[3] |= nonzero_bytes(v.w) << p;
                }
            }
        } else {
            for (int p = 0; p < L; ++p) {
                const uint8_t* __restrict__ src = base + (size_t)p * HW;
                for (int i = 0; px + i < last; ++i)
                    if (src[px + i]) w[i >> 2] |= 1u << (8 * (i & 3) + p);
            }
        }
#pragma unroll
        for (int j = 0; j < MAX_P; ++j) {
            if (j < P) {
                const int sa = pairs.a[j], sb = pairs.b[j];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t fa = (w[k] >> sa) & 0x01010101u, fb = (w[k] >> sb) & 0x01010101u;
                    n_a[j] += __popc(fa);
                    n_b[j] += __popc(fb);
                    n_ab[j] += __popc(fa & fb);
                }
            }
        }
    }

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < MAX_P; ++j) {
        if (j < P) {
            uint32_t va = n_a[j], vb = n_b[j], vab = n_ab[j];
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                va += __shfl_down(va, s, 64);
                vb += __shfl_down(vb, s, 64);
                vab += __shfl_down(vab, s, 64);
            }
            if (lane == 0) {
                part[wave][j][0] = va;
                part[wave][j][1] = vb;
                part[wave][j][2] = vab;
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 4 * P) {
        const int j = threadIdx.x >> 2, c = threadIdx.x & 3;
        unsigned long long fa = 0, fb = 0, both = 0;
        for (int v = 0; v < WAVES; ++v) {
            fa += part[v][j][0];
            fb += part[v][j][1];
            both += part[v][j][2];
        }
        const unsigned long long n = (unsigned long long)(last - first);
        const unsigned long long val = c == 0 ? both : c == 1 ? fa - both : c == 2 ? fb - both : n - fa - fb + both;
        if (val) atomicAdd(counts + ((size_t)b * P + j) * 4 + c, val);
    }
}

__device__ __forceinline__ uint8_t tint(uint8_t v, uint8_t label, double c0, double c1)
{
    const double x = (double)v * c0;
    const double y = (double)label * c1;
    return (uint8_t)(long long)(x + y);         // numpy's float64 -> uint8 store: toward zero (a value outside 0..255 wraps)
}

__global__ void __launch_bounds__(256)
label_pair_blend_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ labels, int L, int HW, int plane_a, int ch_a,
                        int plane_b, int ch_b, double c0, double c1, uint8_t* __restrict__ out, long n_pixels)
{
    const long px = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (px >= n_pixels) return;
    const long b = px / HW, r = px - b * HW;
    uint8_t v[3] = {rgb[px * 3], rgb[px * 3 + 1], rgb[px * 3 + 2]};
    const uint8_t la = labels[(b * L + plane_a) * HW + r], lb = labels[(b * L + plane_b) * HW + r];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (la && c == ch_a) v[c] = tint(v[c], la, c0, c1);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (lb && c == ch_b) v[c] = tint(v[c], lb, c0, c1);
    out[px * 3] = v[0];
    out[px * 3 + 1] = v[1];
    out[px * 3 + 2] = v[2];
}

int refuse(const char* fn, const char* why)
{
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: %s", fn, why);
    ape::set_last_error(msg);
    return APE_EINVAL;
}

bool planes_fit(int B, int L, long HW) { return (double)B * (double)L * (double)HW < 2147483648.0; }

}  // namespace

extern "C" int ape_label_pair_counts_u8(const uint8_t* labels, int B, int L, int HW, const int32_t* pairs_host, int P, uint64_t* counts,
                                        void* stream)
{
    static const char* fn = "ape_label_pair_counts_u8";
    if (!labels || !pairs_host || !counts) return refuse(fn, "labels, pairs_host or counts is null");
    if (B <= 0 || HW <= 0) return refuse(fn, "B and HW must be positive");
    if (L < 1 || L > MAX_L) return refuse(fn, "L must be 1..8");
    if (P < 1 || P > MAX_P) return refuse(fn, "P must be 1..16");
    if (!planes_fit(B, L, HW)) return refuse(fn, "B L HW must stay below 2^31");
    if ((uintptr_t)counts & 7) return refuse(fn, "counts must be 8-byte aligned");
    PairTable table;
    memset(&table, 0, sizeof(table));
    for (int j = 0; j < P; ++j) {
        const int32_t a = pairs_host[2 * j], b = pairs_host[2 * j + 1];
        if (a < 0 || a >= L || b < 0 || b >= L) return refuse(fn, "a pair names a plane outside 0..L-1");
        table.a[j] = (uint8_t)a;
        table.b[j] = (uint8_t)b;
    }
    const int blocks_per_sample = ape::ceil_div(HW, PX_PER_STEP * STEPS);
    if ((double)blocks_per_sample * B >= 2147483648.0) return refuse(fn, "too many samples for one launch");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)B * P * 4 * sizeof(uint64_t), st) != hipSuccess) {
        ape::set_last_error("ape_label_pair_counts_u8: hipMemsetAsync of the counts");
        return APE_ELAUNCH;
    }
    hipLaunchKernelGGL(label_pair_counts_kernel, dim3(blocks_per_sample * B), dim3(THREADS), 0, st, labels, L, HW, blocks_per_sample, table,
                       P, reinterpret_cast<unsigned long long*>(counts));
    return ape::check_launch(fn);
}

extern "C" int ape_label_pair_blend_u8(const uint8_t* rgb, const uint8_t* labels, int B, int L, int H, int W, int plane_a, int ch_a,
                                       int plane_b, int ch_b, double c0, double c1, uint8_t* out, void* stream)
{
    static const char* fn = "ape_label_pair_blend_u8";
    if (!rgb || !labels || !out) return refuse(fn, "rgb, labels or out is null");
    if (B <= 0 || L <= 0 || H <= 0 || W <= 0) return refuse(fn, "B, L, H and W must be positive");
    if (!planes_fit(B, L, (long)H * W) || !planes_fit(B, 3, (long)H * W)) return refuse(fn, "B L H W and 3 B H W must stay below 2^31");
    if (ch_a < 0 || ch_a > 2 || ch_b < 0 || ch_b > 2) return refuse(fn, "a channel is outside 0..2");
    if (plane_a < 0 || plane_a >= L || plane_b < 0 || plane_b >= L) return refuse(fn, "a plane is outside 0..L-1");
    const size_t bytes = (size_t)B * H * W * 3;
    if (out < rgb + bytes && rgb < out + bytes) return refuse(fn, "out must not overlap rgb");
    const long n_pixels = (long)B * H * W;
    hipLaunchKernelGGL(label_pair_blend_kernel, dim3(ape::ceil_div(n_pixels, 256)), dim3(256), 0, (hipStream_t)stream, rgb, labels, L, H * W,
                       plane_a, ch_a, plane_b, ch_b, c0, c1, out, n_pixels);
    return ape::check_launch(fn);
}
