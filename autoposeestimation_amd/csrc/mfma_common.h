// Device helpers shared by the matrix (MFMA) kernels: vector types, the activation epilogue, the bf16 hi/lo operand split, the LDS
// swizzle, the hand-written LDS / wait statements of the LDS-DMA kernels and the halo ring geometry.  Everything here is inlined into
// kernels whose gfx950 assembly is pinned: change it only with tools/isa_identical.py beside you.
#pragma once
#include "common.h"

// timing-only ablation switches (results wrong when set): compiled IN only by `make ablations` (-DAPE_ABLATIONS -> ../libape_hip_abl.so, what
// tools/mb_*_abl.py load) and, for upconv_fused.hip, by `make stamps` (-DAPE_UPFUSE_ABLATIONS); `a` is the kernel's argument struct.  In
// the product build they cost: the run-time tests around the MFMA rows, waits and DMA statements of halo_s32 were 1 ms of the 33 ms step
// (same-box A/B).
#if defined(APE_ABLATIONS) || defined(APE_UPFUSE_ABLATIONS)
#define ABL(bit) (a.dbg & (bit))
#else
#define ABL(bit) 0
#endif

// one 16-byte LDS read whose address, offset and destination registers the kernel chooses itself
// (the host pass of hipcc instantiates kernel bodies too and silently drops a kernel whose body holds an asm it cannot check
// against the HOST target -- the library then lacks the kernel's stub -- so the statement exists in the device pass only)
#if defined(__HIP_DEVICE_COMPILE__)
#define APE_DS_READ(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off) : "memory")
#else
#define APE_DS_READ(dst, addr, off) (void)(addr)
#endif

namespace ape {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;

// word 3 of a buffer resource: DATA_FORMAT = 32 bit, nothing else set -- a raw buffer whose byte offsets are checked against num_records
// (the LDS-DMA kernels rely on that check: what lies past the range arrives as zeros)
constexpr int BUF_RSRC_FLAGS = 0x00020000;

// NONE / RELU / PRELU as selects on loop-invariant scalars (a `switch` per element compiled to a cascade of scalar compares and branches
// per element: ~1.8 k scalar instructions in a 256-element epilogue); same values bit for bit (1 * v == v, also for -0 and NaN)
__device__ __forceinline__ float activate(float v, int act, float alpha)
{
    if (act == APE_ACT_SIGMOID) return 1.f / (1.f + __expf(-v));
    const float neg = act == APE_ACT_RELU ? 0.f : (act == APE_ACT_PRELU ? alpha : 1.f) * v;
    return v > 0.f ? v : neg;
}

// ---- THE OPERAND SPLIT ("bf16x3", the S32 layout): v ~ hi + lo with hi = bf16(v) and lo = bf16(v - float(hi)), both conversions round to
// nearest even, the subtraction exact in fp32.  Every kernel that splits an operand or stores an S32 tensor computes these two values
// bit for bit (the cross-kernel bitwise tests rely on it); tests/conv_products_reference.py and tests/test_split_format_emulation.py
// restate them on the host.  Kernels that split in their own loops (another element order, a conditional lo plane) still take lo from
// split_lo; DESIGN.md 6w lists every site.
__device__ __forceinline__ __bf16 split_lo(float v, __bf16 hi) { return (__bf16)(v - (float)hi); }

__device__ __forceinline__ void split4(const float4 v, bf16x4& hi, bf16x4& lo)
{
    hi[0] = (__bf16)v.x; hi[1] = (__bf16)v.y; hi[2] = (__bf16)v.z; hi[3] = (__bf16)v.w;
    lo[0] = split_lo(v.x, hi[0]); lo[1] = split_lo(v.y, hi[1]);
    lo[2] = split_lo(v.z, hi[2]); lo[3] = split_lo(v.w, hi[3]);
}
__device__ __forceinline__ void split8(const f32x4 v0, const f32x4 v1, bf16x8& hi, bf16x8& lo)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        hi[e] = (__bf16)v0[e];
        lo[e] = split_lo(v0[e], hi[e]);
        hi[4 + e] = (__bf16)v1[e];
        lo[4 + e] = split_lo(v1[e], hi[4 + e]);
    }
}
__device__ __forceinline__ void split8(const float4 v0, const float4 v1, bf16x8& hi, bf16x8& lo)
{
    const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        hi[e] = (__bf16)v[e];
        lo[e] = split_lo(v[e], hi[e]);
    }
}

// element offset of 16-B chunk c of tile row `row`, rows of 32 bf16 (64 B, unpadded)
// (16x16x32 fragments: lane l reads chunk l >> 4 of row l & 15; ds_read_b128 services the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31},
// ...: the permutation that keeps the 16 lanes of a group on 16 distinct 16-B bank slots is chunk ^ (-(row >> 2) & 3))
__device__ __forceinline__ int swz(int row, int c) { return row * 32 + ((c ^ ((0 - (row >> 2)) & 3)) << 3); }

// source coordinate of a bilinear resize (ATen area_pixel_compute_source_index)
__device__ __forceinline__ float src_index(int dst, float scale, bool align_corners)
{
    if (align_corners) return scale * (float)dst;
    const float s = scale * ((float)dst + 0.5f) - 0.5f;
    return s < 0.f ? 0.f : s;
}

// keeps asm-read destinations allocated up to this point (a free function: asm operands cannot name variables captured by a generic
// lambda; device pass only: the host pass cannot check a "v" constraint)
__device__ __forceinline__ void keep_regs(const u32x4& a, const u32x4& b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" :: "v"(a), "v"(b));
#endif
}

// s_waitcnt vmcnt(n) for a wave-uniform run-time n (the immediate must be a literal)
__device__ __forceinline__ void wait_vmcnt(int n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
#endif
}

// LDS geometry of the 3x3 halo kernels on LDS-DMA operands (conv3x3_halo_s32.hip, conv3x3_halo_mx.hip): a ring of pixel rows and a ring
// of per-tap weight tiles, 128-byte lines.  In a namespace of its own: other kernels have a TS of their own.
namespace halo_ring {
constexpr int TS = 16;                  // output tile edge
constexpr int HWP = 24;                 // pixels per ring row (3 DMA pieces); the halo needs 16 + 2 d <= 24 of them
constexpr int ROW_B = HWP * 128;        // 3072 B
constexpr int RING_ROWS = 32;
constexpr int A_BYTES = RING_ROWS * ROW_B;          // 96 KB
constexpr int B_TILE = 128 * 128;                   // one tap's weights: 128 rows x (hi 64 B | lo 64 B)
constexpr int B_RING = 4;
constexpr int LDS_BYTES = A_BYTES + B_RING * B_TILE;   // 160 KB
}  // namespace halo_ring

}  // namespace ape
