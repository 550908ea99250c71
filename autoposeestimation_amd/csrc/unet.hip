// 3x3 / stride 1 / pad 1 convolution of the smp Unet decoder (DecoderBlock.conv1 / conv2 and the segmentation head) over the VIRTUAL
// input  cat([nearest_up2(A), B], dim=channels):  input channel c of output pixel (y, x) is
//     A[(y >> 1, x >> 1), c]        for c < C1        (UPS = true; UPS = false reads A at full resolution: the head, conv2)
//     B[(y, x), c - C1]             for C1 <= c < C1 + C2 (the skip; C2 may be 0)
// so neither the up-sampled tensor nor the concatenation is ever written.  Implicit GEMM on v_mfma_f32_16x16x32_bf16 with the WEIGHTS
// as the row operand (D[row = output channel 4 kq + r][col = pixel lane & 15], a lane ends up with four consecutive output channels of
// one pixel, as in conv3x3_halo.hip); K = 9 (C1 + C2) in [tap][C1 | C2] order, the packed planes of ape_pack_weights_bf16.
//
// Layout: one workgroup = 4 waves along the flattened pixel axis (b, y, x) x 16 NC output channels; one wave = NP groups of 16
// pixels x NC groups of 16 channels.  Each lane fetches, per 32-deep k-step, the eight channels 8 kq .. 8 kq + 7 of its pixel at the
// tap straight from HBM / L2 (two 16-B loads, split to bf16 hi / lo in registers) and the eight matching weights of each channel group
// (16 B per plane): no LDS.  The narrow layers of the decoder's full-resolution end (Cout 32 / 16 / classes) take NC = 2 / 1 with
// 128-pixel waves, the wide ones NC = 4 with 64-pixel waves.  Channel counts are multiples of 16, so a k-step may be half empty
// (C1 + C2 = 16 or 48, ...): the lanes beyond the tap's channels contribute zeros.
//
// Epilogues: (1) folded-BN bias + ReLU, fp32 NHWC store into y[.., yoff + co] (ldy); (2) HEAD, classes <= 16 (NC = 1): bias, then
// csrc/seg_head.h's softmax (+ softmax) / arg-max / tie rule, label u8 + score f32 per pixel -- the logits are never stored.
// Pixel and element offsets are 64-bit: at B = 64 the 240 x 320 x 128 virtual input of decoder block 3 is 629 M elements.
#include "mfma_common.h"
#include "seg_head.h"

namespace {

using namespace ape;

constexpr int UNET_WAVES = 4;

struct UnetArgs {
    const float* a;          // [B][H >> UPS][W >> UPS][lda], channels 0..C1-1 read
    const float* b;          // [B][H][W][ldb], channels 0..C2-1 read (unused when C2 == 0)
    const __bf16* w;         // hi plane [Cout][K], lo plane at w + plane_stride
    const float* bias;       // [Cout] or null
    float* y;                // [B][H][W][ldy], channels yoff .. yoff + Cout - 1 written (epilogue 1)
    uint8_t* label;          // [B][H][W] (epilogue 2)
    float* score;            // [B][H][W] (epilogue 2)
    long M;                  // B * H * W output pixels
    long plane_stride;
    int lda, C1, ldb, C2, Ctot, K, H, W, Cout, ldy, yoff, head_dsm;
};

template <int NSPLIT, bool UPS, int NC, int NP, bool HEAD>
__global__ __launch_bounds__(64 * UNET_WAVES) void unet_conv3x3_kernel(const UnetArgs g)
{
    static_assert(!HEAD || NC == 1, "the head epilogue takes one 16-class group");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const long m_wave = ((long)blockIdx.x * UNET_WAVES + wave) * (16 * NP);
    const int co0 = blockIdx.y * (16 * NC);
    const int H = g.H, W = g.W;
    const int Ha = UPS ? H >> 1 : H, Wa = UPS ? W >> 1 : W;

    // this lane's pixel of each 16-pixel group; y = -4 marks a pixel beyond M (every tap then falls outside the image)
    int pb[NP], py[NP], px[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const long m = m_wave + 16 * p + r16;
        if (m < g.M) {
            const long hw = (long)H * W;
            const long bi = m / hw, rem = m - bi * hw;
            pb[p] = (int)bi;
            py[p] = (int)(rem / W);
            px[p] = (int)(rem - (long)py[p] * W);
        } else {
            pb[p] = 0; py[p] = -4; px[p] = 0;
        }
    }
    // weight rows of this lane (output channel co0 + 16 j + r16); rows past Cout (the head's classes) read as zero
    bool wok[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) wok[j] = co0 + 16 * j + r16 < g.Cout;

    f32x4 acc[NP][NC];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int j = 0; j < NC; ++j) acc[p][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        long offa[NP], offb[NP];            // element offset of the tap's source pixel in A / B, -1 outside the image (zero padding)
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int yy = py[p] + dy, xx = px[p] + dx;
            const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
            const int ya = UPS ? yy >> 1 : yy, xa = UPS ? xx >> 1 : xx;
            offa[p] = ok ? (((long)pb[p] * Ha + ya) * Wa + xa) * g.lda : -1L;
            offb[p] = ok ? (((long)pb[p] * H + yy) * W + xx) * g.ldb : -1L;
        }
        const long ktap = (long)tap * g.Ctot;
        for (int c0 = 0; c0 < g.Ctot; c0 += 32) {
            const int c = c0 + 8 * kq;
            const bool cok = c < g.Ctot;
            const bool from_a = c < g.C1;
            bf16x8 wh[NC], wl[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                if (cok && wok[j]) {
                    const __bf16* wp = g.w + (long)(co0 + 16 * j + r16) * g.K + ktap + c;
                    wh[j] = *reinterpret_cast<const bf16x8*>(wp);
                    if (NSPLIT == 3) wl[j] = *reinterpret_cast<const bf16x8*>(wp + g.plane_stride);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { wh[j][e] = (__bf16)0.f; wl[j][e] = (__bf16)0.f; }
                }
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                if (m_wave + 16 * p >= g.M) continue;              // (wave-uniform) a group wholly past the last pixel
                const long off = from_a ? offa[p] : offb[p];
                float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
                if (cok && off >= 0) {
                    const float* src = from_a ? g.a + off + c : g.b + off + (c - g.C1);
                    v0 = reinterpret_cast<const float4*>(src)[0];
                    v1 = reinterpret_cast<const float4*>(src)[1];
                }
                bf16x8 ah, al;
                split8(v0, v1, ah, al);
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    // the two cross terms first, then hi . hi (conv3x3_halo.hip's order)
                    if (NSPLIT == 3) {
                        acc[p][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], al, acc[p][j], 0, 0, 0);
                        acc[p][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[j], ah, acc[p][j], 0, 0, 0);
                    }
                    acc[p][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], ah, acc[p][j], 0, 0, 0);
                }
            }
        }
    }

    if (HEAD) {
        const int C = g.Cout;
        f32x4 breg;
#pragma unroll
        for (int r = 0; r < 4; ++r) breg[r] = (4 * kq + r < C && g.bias) ? g.bias[4 * kq + r] : 0.f;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (m_wave + 16 * p >= g.M) continue;
            const f32x4 logits = acc[p][0] + breg;
            int am;
            float pm;
            ape_seg::seg_head_finish(logits, C, lane, g.head_dsm, am, pm);
            const long m = m_wave + 16 * p + r16;
            if (kq == 0 && m < g.M) {
                g.label[m] = (uint8_t)am;
                g.score[m] = pm;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int co = co0 + 16 * j + 4 * kq;
            if (co0 + 16 * j >= g.Cout) continue;                  // (wave-uniform: Cout % 16 == 0)
            float bv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) bv[r] = g.bias ? g.bias[co + r] : 0.f;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const long m = m_wave + 16 * p + r16;
                if (m >= g.M) continue;
                float o[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[p][j][r] + bv[r];
                    o[r] = v > 0.f ? v : 0.f;
                }
                *reinterpret_cast<float4*>(g.y + m * g.ldy + g.yoff + co) = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
    }
}

template <int NSPLIT, bool UPS, int NC, int NP, bool HEAD>
int launch_unet(const UnetArgs& a, hipStream_t st)
{
    const long px_per_wg = 16L * NP * UNET_WAVES;
    const long gx = (a.M + px_per_wg - 1) / px_per_wg;
    const int gy = ape::ceil_div(a.Cout, 16 * NC);
    if (gx > 0x7fffffffL) return APE_EINVAL;
    hipLaunchKernelGGL((unet_conv3x3_kernel<NSPLIT, UPS, NC, NP, HEAD>), dim3((unsigned)gx, gy), dim3(64 * UNET_WAVES), 0, st, a);
    return ape::check_launch("ape_unet_conv3x3");
}

// output-channel tile of a layer: 64 per wave for Cout >= 64 (64-pixel waves), 32 / 16 for the narrow full-resolution layers
// (128-pixel waves)
template <int NSPLIT, bool UPS>
int launch_relu(const UnetArgs& a, hipStream_t st)
{
    if (a.Cout >= 64) return launch_unet<NSPLIT, UPS, 4, 4, false>(a, st);
    if (a.Cout == 32 || a.Cout == 48) return launch_unet<NSPLIT, UPS, 2, 8, false>(a, st);
    return launch_unet<NSPLIT, UPS, 1, 8, false>(a, st);
}

// the argument checks shared by both entries (output geometry B x H x W, Cout output channels / classes)
bool args_ok(const float* a, int lda, int C1, const float* b, int ldb, int C2, const void* w, int B, int H, int W, int ups, int nsplit)
{
    if (!a || !w || (nsplit != 1 && nsplit != 3) || (ups != 0 && ups != 1)) return false;
    if (B < 0 || H < 1 || W < 1 || C1 < 16 || C1 % 16 || C2 < 0 || C2 % 16 || lda < C1 || lda % 4) return false;
    if (C2 && (!b || ldb < C2 || ldb % 4)) return false;
    if (ups && ((H & 1) || (W & 1))) return false;
    if (9L * (C1 + C2) >= (1L << 30)) return false;
    return true;
}

UnetArgs make_args(const float* a, int lda, int C1, const float* b, int ldb, int C2, const void* w, const float* bias, int B, int H, int W,
                   int Cout)
{
    UnetArgs g;
    g.a = a; g.b = b; g.w = (const __bf16*)w; g.bias = bias;
    g.y = nullptr; g.label = nullptr; g.score = nullptr;
    g.M = (long)B * H * W;
    g.lda = lda; g.C1 = C1; g.ldb = C2 ? ldb : 0; g.C2 = C2; g.Ctot = C1 + C2; g.K = 9 * (C1 + C2);
    g.plane_stride = (long)Cout * g.K;
    g.H = H; g.W = W; g.Cout = Cout; g.ldy = 0; g.yoff = 0; g.head_dsm = 0;
    return g;
}

// one thread per output pixel and channel quad (S = 2: nearest x2; S = 1: a copy into the channel window)
template <int S>
__global__ __launch_bounds__(256) void nearest_up_kernel(const float4* __restrict__ x, float* __restrict__ y, long n, int h, int w, int cq,
                                                         int ldy, int yoff)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int q = (int)(i % cq);
    const long pix = i / cq;                        // output pixel (b, Y, X) of [B][S h][S w]
    const int X = (int)(pix % (S * w));
    const long r = pix / (S * w);
    const int Y = (int)(r % (S * h));
    const long bi = r / (S * h);
    const float4 v = x[((bi * h + Y / S) * w + X / S) * cq + q];
    *reinterpret_cast<float4*>(y + pix * ldy + yoff + 4 * q) = v;
}

}  // namespace

extern "C" int ape_nearest_upsample_nhwc_f32(const float* x, float* y, int B, int h, int w, int C, int scale, int ldy, int yoff, void* stream)
{
    if (!x || !y || B < 0 || h < 1 || w < 1 || C < 4 || C % 4 || (scale != 1 && scale != 2) || ldy % 4 || yoff % 4 || yoff < 0 ||
        yoff + C > ldy)
        return APE_EINVAL;
    const long n = (long)B * scale * scale * h * w * (C / 4);
    if (n == 0) return APE_OK;
    if ((n + 255) / 256 > 0x7fffffffL) return APE_EINVAL;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (scale == 2)
        hipLaunchKernelGGL(nearest_up_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, (const float4*)x, y, n, h, w, C / 4, ldy, yoff);
    else
        hipLaunchKernelGGL(nearest_up_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (const float4*)x, y, n, h, w, C / 4, ldy, yoff);
    return ape::check_launch("ape_nearest_upsample_nhwc_f32");
}

extern "C" int ape_unet_conv3x3_supported(int C1, int C2, int Cout, int ups)
{
    return C1 >= 16 && C1 % 16 == 0 && C2 >= 0 && C2 % 16 == 0 && Cout >= 16 && Cout % 16 == 0 && (ups == 0 || ups == 1) &&
           9L * (C1 + C2) < (1L << 30);
}

extern "C" int ape_unet_conv3x3_bf16(const float* a, int lda, int C1, const float* b, int ldb, int C2, const void* w_packed,
                                     const float* bias, float* y, int ldy, int yoff, int B, int H, int W, int Cout, int ups, int nsplit,
                                     void* stream)
{
    if (!args_ok(a, lda, C1, b, ldb, C2, w_packed, B, H, W, ups, nsplit) || !y) return APE_EINVAL;
    if (!ape_unet_conv3x3_supported(C1, C2, Cout, ups) || ldy % 4 || yoff % 4 || yoff < 0 || yoff + Cout > ldy) return APE_EINVAL;
    if (B == 0) return APE_OK;
    UnetArgs g = make_args(a, lda, C1, b, ldb, C2, w_packed, bias, B, H, W, Cout);
    g.y = y; g.ldy = ldy; g.yoff = yoff;
    hipStream_t st = (hipStream_t)stream;
    if (nsplit == 3) return ups ? launch_relu<3, true>(g, st) : launch_relu<3, false>(g, st);
    return ups ? launch_relu<1, true>(g, st) : launch_relu<1, false>(g, st);
}

extern "C" int ape_unet_conv3x3_seghead_bf16(const float* a, int lda, int C1, const float* b, int ldb, int C2, const void* w_packed,
                                             const float* bias, int C, uint8_t* label, float* score, int B, int H, int W, int ups,
                                             int nsplit, int double_softmax, void* stream)
{
    if (!args_ok(a, lda, C1, b, ldb, C2, w_packed, B, H, W, ups, nsplit) || !label || !score || C < 1 || C > 16) return APE_EINVAL;
    if (B == 0) return APE_OK;
    UnetArgs g = make_args(a, lda, C1, b, ldb, C2, w_packed, bias, B, H, W, C);
    g.label = label; g.score = score; g.head_dsm = double_softmax ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    if (nsplit == 3) return ups ? launch_unet<3, true, 1, 8, true>(g, st) : launch_unet<3, false, 1, 8, true>(g, st);
    return ups ? launch_unet<1, true, 1, 8, true>(g, st) : launch_unet<1, false, 1, 8, true>(g, st);
}
