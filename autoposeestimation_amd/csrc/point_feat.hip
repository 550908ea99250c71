// The point-feature front of PoseNetFeat / PoseRefineNetFeat (DenseFusion/lib/network.py:39-68, 136-168) in ONE launch:
//   pf[m] = [conv1(x4[m]) 64 | e_conv1(emb[m]) 64 | conv2(.) 128 | e_conv2(.) 128], every layer with bias and ReLU,
// written as fp32 rows, as S32 lines (s32.h), or both.  It replaces five launches -- conv_bf16_kernel (conv1, K = 4), three
// conv_gemm_kernel / conv_rows_kernel launches and f32_to_s32_kernel -- that wrote pf, re-read a third of it and then re-read and
// re-wrote all of it; here a row's 144 input bytes are read once and its output bytes written once.
//
// CONTRACT: bit for bit what those five launches give.  An output element depends on its own row, its own weight row and the K order
// only, so each layer restates the arithmetic of the kernel it replaces:
//   conv1                    conv_bf16_kernel's !tap_uniform path: v_mfma_f32_32x32x16_bf16, ACTIVATIONS as the first operand, per 16-deep
//                            step mfma(x_lo, w_hi), mfma(x_hi, w_lo), mfma(x_hi, w_hi); two steps, of which only k = 0..3 of the first holds
//                            data (everything else is the +0 the staging pass wrote); split4; bias, then activate()
//   e_conv1, conv2, e_conv2  conv_gemm_body: v_mfma_f32_16x16x32_bf16, WEIGHTS as the first operand, accumulator from 0, k-tiles ascending,
//                            per k-tile mfma(w_hi, x_lo), mfma(w_lo, x_hi), mfma(w_hi, x_hi); split8; bias after the k-loop, then act_fast()
//   conv2 / e_conv2          read the post-ReLU fp32 values of conv1 / e_conv1 and split them again with split8 (what re-reading pf did)
//   S32 bytes                split4 of the fp32 values (f32_to_s32_kernel)
//
// Shape: a workgroup of 8 waves owns 256 rows, a wave 32 of them (the row count of conv1's 32x32 accumulator, two 16-row blocks of the
// gemm layers).  The weight planes of the three gemm layers (72 KB) are copied once per workgroup into LDS in conv_gemm's swizzled 64-byte
// rows; conv1's 2 KB stay in registers.  Each wave has a private 32 x 64 fp32 staging tile in LDS: a layer writes 64 output columns into it
// from its accumulator layout, then the tile is (a) streamed out row-major -- 256 contiguous fp32 bytes and two whole 128-byte S32 lines per
// row, 16 bytes per lane -- and (b) for the first layers read back in fragment order as the next layer's operand.  The tile is wave-private, so
// the only workgroup barrier is the one behind the weight copy.  No host tables, no synchronisation: the launch is capturable.
#include "s32.h"

namespace {

using namespace ape;

constexpr int PF_C = 384;                   // columns of pf
constexpr int NWAVE = 8;
constexpr int NT = NWAVE * 64;
constexpr int WROWS = 32;                   // rows per wave
constexpr int PF_ROWS = NWAVE * WROWS;      // rows per workgroup (256)
constexpr int LDF = 68;                     // floats per staged row (64 + 4: 16-byte aligned rows, row starts 4 banks apart)

// LDS, in bf16 elements: per layer [plane][k-tile][Cout rows of 32 bf16, chunks swizzled by swz()]
constexpr int W_E1 = 0;
constexpr int W_C2 = W_E1 + 2 * 1 * 64 * 32;
constexpr int W_E2 = W_C2 + 2 * 2 * 128 * 32;
constexpr int W_ELEMS = W_E2 + 2 * 2 * 128 * 32;                       // 36864 bf16 = 72 KB
constexpr int LDS_BYTES = W_ELEMS * 2 + NWAVE * WROWS * LDF * 4;       // + 68 KB of staging tiles = 140 KB

struct PointFeatArgs {
    const float* x4;       // [M][4]
    const float* emb;      // [M][32]
    const __bf16 *w1, *we1, *w2, *we2;      // packed planes (ape_pack_weights_bf16): hi [Cout][Kp] then lo [Cout][Kp]
    const float *b1, *be1, *b2, *be2;
    float* pf;             // [M][384] fp32 or NULL
    char* pfs;             // the same rows as S32 lines or NULL
    long M;
    int parts;             // APE_POINT_FEAT_X | APE_POINT_FEAT_EMB
};

// orders this wave's LDS accesses for the compiler (the hardware executes one wave's LDS instructions in issue order)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// packed planes of a Cin = 32 * NKT layer -> LDS, all threads of the workgroup
template <int COUT, int NKT>
__device__ __forceinline__ void stage_weights(__bf16* dst, const __bf16* src, int tid)
{
    constexpr int CHUNKS = 2 * COUT * NKT * 4;          // 16-byte chunks, contiguous in src: ((plane * COUT + n) * NKT + kt) * 4 + c
    for (int i = tid; i < CHUNKS; i += NT) {
        const int c = i & 3, kt = (i >> 2) % NKT, n = (i / (4 * NKT)) % COUT, pl = i / (4 * NKT * COUT);
        *reinterpret_cast<u32x4*>(dst + (pl * NKT + kt) * COUT * 32 + swz(n, c)) = *reinterpret_cast<const u32x4*>(src + (size_t)i * 8);
    }
}

template <int COUT, int NKT>
__device__ __forceinline__ bf16x8 w_frag(const __bf16* w, int pl, int kt, int row, int fc)
{
    return *reinterpret_cast<const bf16x8*>(w + (pl * NKT + kt) * COUT * 32 + swz(row, fc));
}

// the wave's staged 32 x 64 tile -> columns [coff, coff + 64) of its rows: a pass is 4 rows x 16 float4
__device__ __forceinline__ void flush64(const float* T, const PointFeatArgs& a, long r0, int coff, int lane)
{
    const int c4 = lane & 15, rr = lane >> 4;
#pragma unroll
    for (int ps = 0; ps < WROWS / 4; ++ps) {
        const int row = ps * 4 + rr;
        const long m = r0 + row;
        const float4 v = *reinterpret_cast<const float4*>(T + row * LDF + c4 * 4);
        if (m < a.M) {          // (the same for both lanes of a pair of s32_store4_pair: they share the row)
            if (a.pf) *reinterpret_cast<float4*>(a.pf + m * PF_C + coff + c4 * 4) = v;
            if (a.pfs) s32_store4_pair(a.pfs, m, PF_C / 4, coff / 4 + c4, v);
        }
    }
}

// conv2 / e_conv2 (64 -> 128): operand = the staged tile of the first layer, output columns [coff, coff + 128) through the same tile
__device__ __forceinline__ void layer2(const __bf16* w, const float* bias, float* T, const PointFeatArgs& a, long r0, int coff, int lane)
{
    const int frow = lane & 15, fc = lane >> 4;
    bf16x8 xh[2][2], xl[2][2];          // [16-row block][k-tile]
#pragma unroll
    for (int pb = 0; pb < 2; ++pb)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            const float* s = T + (pb * 16 + frow) * LDF + kt * 32 + fc * 8;
            split8(*reinterpret_cast<const f32x4*>(s), *reinterpret_cast<const f32x4*>(s + 4), xh[pb][kt], xl[pb][kt]);
        }
    wave_sync();                        // the tile is overwritten below
    const ActFast af = act_fast_make(APE_ACT_RELU, 0.f);
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = h * 4 + jj;
            f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                const bf16x8 wh = w_frag<128, 2>(w, 0, kt, j * 16 + frow, fc), wl = w_frag<128, 2>(w, 1, kt, j * 16 + frow, fc);
#pragma unroll
                for (int pb = 0; pb < 2; ++pb) {
                    acc[pb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xl[pb][kt], acc[pb], 0, 0, 0);
                    acc[pb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, xh[pb][kt], acc[pb], 0, 0, 0);
                    acc[pb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xh[pb][kt], acc[pb], 0, 0, 0);
                }
            }
            // lane (frow, fc) holds channels 16 j + 4 fc .. + 3 of row 16 pb + frow
            const float4 b4 = *reinterpret_cast<const float4*>(bias + j * 16 + fc * 4);
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                float vv[4] = {acc[pb][0], acc[pb][1], acc[pb][2], acc[pb][3]};
                vv[0] += b4.x; vv[1] += b4.y; vv[2] += b4.z; vv[3] += b4.w;
                *reinterpret_cast<float4*>(T + (pb * 16 + frow) * LDF + jj * 16 + fc * 4) =
                    make_float4(act_fast(vv[0], af), act_fast(vv[1], af), act_fast(vv[2], af), act_fast(vv[3], af));
            }
        }
        wave_sync();
        flush64(T, a, r0, coff + h * 64, lane);
        wave_sync();
    }
}

__global__ __launch_bounds__(NT) void point_feat_kernel(const PointFeatArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __bf16* const W = reinterpret_cast<__bf16*>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* const T = reinterpret_cast<float*>(smem_raw + W_ELEMS * 2) + wave * (WROWS * LDF);

    if (a.parts & APE_POINT_FEAT_X) stage_weights<128, 2>(W + W_C2, a.w2, tid);
    if (a.parts & APE_POINT_FEAT_EMB) {
        stage_weights<64, 1>(W + W_E1, a.we1, tid);
        stage_weights<128, 2>(W + W_E2, a.we2, tid);
    }
    __syncthreads();

    const long r0 = (long)blockIdx.x * PF_ROWS + wave * WROWS;
    if (r0 >= a.M) return;
    const long last = a.M - 1;          // rows >= M are computed on row M - 1 and dropped by flush64

    if (a.parts & APE_POINT_FEAT_X) {
        // ---- conv1: 32 rows x 64 channels as two 32x32x16 accumulators; lane l holds row l & 31, k = 8 (l >> 5) .. + 7 of the 16-deep step
        const int l31 = lane & 31;
        const bool k0 = lane < 32;                                   // the lanes of k = 0..7: x in k = 0..3, zeros behind (Kp = 8, K = 4)
        const long m = r0 + l31 < last ? r0 + l31 : last;
        const float4 xv = *reinterpret_cast<const float4*>(a.x4 + m * 4);
        bf16x4 h4, l4;
        split4(k0 ? xv : make_float4(0.f, 0.f, 0.f, 0.f), h4, l4);
        const bf16x4 z4 = {(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
        const bf16x8 ah = __builtin_shufflevector(h4, z4, 0, 1, 2, 3, 4, 5, 6, 7), al = __builtin_shufflevector(l4, z4, 0, 1, 2, 3, 4, 5, 6, 7);
        const bf16x8 z8 = __builtin_shufflevector(z4, z4, 0, 1, 2, 3, 4, 5, 6, 7);
        const u32x4 zu = {0u, 0u, 0u, 0u};
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const u32x4 uh = *reinterpret_cast<const u32x4*>(a.w1 + (j * 32 + l31) * 8);
            const u32x4 ul = *reinterpret_cast<const u32x4*>(a.w1 + 64 * 8 + (j * 32 + l31) * 8);
            const bf16x8 bh = __builtin_bit_cast(bf16x8, k0 ? uh : zu), bl = __builtin_bit_cast(bf16x8, k0 ? ul : zu);
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[j], 0, 0, 0);
            // the second 16-deep step of conv_bf16_kernel's 32-deep k-tile: all operands are the zeros of its staging pass
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z8, z8, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z8, z8, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z8, z8, acc[j], 0, 0, 0);
        }
        const int fh = lane >> 5;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float b = a.b1[j * 32 + l31];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = (e & 3) + 8 * (e >> 2) + 4 * fh;      // accumulator element e of lane (l31, fh): row `row`, channel 32 j + l31
                float t = acc[j][e];
                t += b;
                T[row * LDF + j * 32 + l31] = activate(t, APE_ACT_RELU, 0.f);
            }
        }
        wave_sync();
        flush64(T, a, r0, 0, lane);
        layer2(W + W_C2, a.b2, T, a, r0, 128, lane);
    }

    if (a.parts & APE_POINT_FEAT_EMB) {
        // ---- e_conv1 (32 -> 64, one k-tile): lane (frow, fc) holds k = 8 fc .. + 7 of row 16 pb + frow, loaded straight from global memory
        const int frow = lane & 15, fc = lane >> 4;
        bf16x8 eh[2], el[2];
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            const long m = r0 + pb * 16 + frow < last ? r0 + pb * 16 + frow : last;
            const float* s = a.emb + m * 32 + fc * 8;
            split8(*reinterpret_cast<const f32x4*>(s), *reinterpret_cast<const f32x4*>(s + 4), eh[pb], el[pb]);
        }
        const ActFast af = act_fast_make(APE_ACT_RELU, 0.f);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            const bf16x8 wh = w_frag<64, 1>(W + W_E1, 0, 0, j * 16 + frow, fc), wl = w_frag<64, 1>(W + W_E1, 1, 0, j * 16 + frow, fc);
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                acc[pb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, el[pb], acc[pb], 0, 0, 0);
                acc[pb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, eh[pb], acc[pb], 0, 0, 0);
                acc[pb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, eh[pb], acc[pb], 0, 0, 0);
            }
            const float4 b4 = *reinterpret_cast<const float4*>(a.be1 + j * 16 + fc * 4);
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                float vv[4] = {acc[pb][0], acc[pb][1], acc[pb][2], acc[pb][3]};
                vv[0] += b4.x; vv[1] += b4.y; vv[2] += b4.z; vv[3] += b4.w;
                *reinterpret_cast<float4*>(T + (pb * 16 + frow) * LDF + j * 16 + fc * 4) =
                    make_float4(act_fast(vv[0], af), act_fast(vv[1], af), act_fast(vv[2], af), act_fast(vv[3], af));
            }
        }
        wave_sync();
        flush64(T, a, r0, 64, lane);
        layer2(W + W_E2, a.be2, T, a, r0, 256, lane);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

/* see include/ape_hip.h */
extern "C" int ape_point_feat_bf16(const float* x4, const float* emb, const void* w_conv1, const float* b_conv1, const void* w_e_conv1,
                                   const float* b_e_conv1, const void* w_conv2, const float* b_conv2, const void* w_e_conv2,
                                   const float* b_e_conv2, float* pf, void* pf_s32, long M, int parts, int nsplit, void* stream)
{
    if (nsplit != 3) return APE_EINVAL;                                                      // split-bf16 only
    if (parts < 1 || parts > (APE_POINT_FEAT_X | APE_POINT_FEAT_EMB)) return APE_EINVAL;     // at least one half, no unknown bits
    if (!pf && !pf_s32) return APE_EINVAL;                                                   // at least one output
    if (M < 0 || M > (1L << 31) - PF_ROWS) return APE_EINVAL;                                // (the grid is M / 256 workgroups)
    if ((parts & APE_POINT_FEAT_X) && (!x4 || !w_conv1 || !b_conv1 || !w_conv2 || !b_conv2)) return APE_EINVAL;
    if ((parts & APE_POINT_FEAT_EMB) && (!emb || !w_e_conv1 || !b_e_conv1 || !w_e_conv2 || !b_e_conv2)) return APE_EINVAL;
    // 16-byte loads and stores (unselected halves are never touched, so their pointers are not looked at)
    if (!aligned16(pf) || !aligned16(pf_s32)) return APE_EINVAL;
    if ((parts & APE_POINT_FEAT_X) && !(aligned16(x4) && aligned16(w_conv1) && aligned16(b_conv2) && aligned16(w_conv2))) return APE_EINVAL;
    if ((parts & APE_POINT_FEAT_EMB) && !(aligned16(emb) && aligned16(w_e_conv1) && aligned16(b_e_conv1) && aligned16(w_e_conv2) && aligned16(b_e_conv2)))
        return APE_EINVAL;
    if (M == 0) return APE_OK;
    static ape::DeviceOnce once;
    const int rc = ape::device_once(once, reinterpret_cast<const void*>(point_feat_kernel), LDS_BYTES, nullptr);
    if (rc != APE_OK) return rc;
    PointFeatArgs a;
    a.x4 = x4; a.emb = emb;
    a.w1 = (const __bf16*)w_conv1; a.we1 = (const __bf16*)w_e_conv1; a.w2 = (const __bf16*)w_conv2; a.we2 = (const __bf16*)w_e_conv2;
    a.b1 = b_conv1; a.be1 = b_e_conv1; a.b2 = b_conv2; a.be2 = b_e_conv2;
    a.pf = pf; a.pfs = (char*)pf_s32; a.M = M; a.parts = parts;
    hipLaunchKernelGGL(point_feat_kernel, dim3(ape::ceil_div(M, PF_ROWS)), dim3(NT), LDS_BYTES, (hipStream_t)stream, a);
    return ape::check_launch("ape_point_feat_bf16");
}
