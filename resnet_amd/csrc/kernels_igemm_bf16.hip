// kernels_igemm_bf16.hip -- the bf16-activation path (BASELINE configs[4]): convolutions as an im2col-free implicit
// GEMM on v_mfma_f32_32x32x16_bf16, fp32 accumulate.  Activations and activation gradients are stored as bf16 in the same
// NCHW tensors; parameters, parameter gradients, Adam state and BN statistics stay fp32 (the policy of
// resnet_cudnn_nchw.cu:1196-1211, TENSOR_OP_MATH_ALLOW_CONVERSION, with the storage made explicit).
//
//   forward  Y = W * im2col(X)      M = K, columns (n,ho,wo), reduction (tap, c); A = weights rounded to bf16 and re-laid
//                                   as k-step tiles [t][c/64][K][64] (one tile = one contiguous run of 16-byte loads)
//   dgrad    dX = W^T * dY          M = C, reduction (tap, k); S=2: four parity classes (blockIdx.y); A = [t][k/64][C][64]
//   wgrad    dW = dY * im2col(X)^T  M = K, columns (tap, 64-channel block) in pairs, reduction (n,ho,wo) split over
//                                   blockIdx.y; fp32 partials [split][t][k][c] reduced in a fixed order
//
// The MFMA operands want the REDUCTION index contiguous per lane (8 bf16 = one ds_read_b128): LDS images are
// [row or column][64 reduction elements], pitch 144 bytes (conflict-free ds_read_b128: 16 lanes x 36 dwords cover all 64
// banks).  In NCHW the channel -- the reduction index of forward and dgrad -- is the STRIDED dimension, so the gathered
// operand is transposed on the way into LDS: a thread gathers 32 channels of ONE pixel (2-byte loads, coalesced along the
// pixels of a wave), packs them in registers and writes four 16-byte pieces of the pixel's row.  wgrad reduces over pixels (contiguous),
// so both its operands are gathered along the reduction and go to LDS element-wise.
// Epilogue of forward / dgrad: accumulators are transposed through LDS so that a lane owns one output channel and 32
// consecutive pixels -> 16-byte (8 x bf16) stores, and the forward pass leaves per-tile batch-norm statistics (count, mean,
// M2, computed from the fp32 accumulators before rounding) exactly as the fp32 kernel does.
#include <stdlib.h>
#include "mi_common.hpp"
#include <type_traits>
#include "mi_device.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float pf4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16;

enum { BG_FWD = 0, BG_DGRAD = 1, BG_WGRAD = 2 };
enum { BGOP_FWD = 0, BGOP_DGRAD = 1, BGOP_WGRAD = 2 };
#define BG_BK 64
#ifndef BG_ABLATE
#define BG_ABLATE 0 /* experiments only (tools/variant.sh): 1 = no B loads in the loop, 2 = no loads, 3 = no loads + no LDS stores, 4 = no MFMA */
#endif
#define BG_LDB 144 /* bytes per LDS row: 64 bf16 + 16 bytes of padding (36 dwords: 16 lanes of a ds_read_b128 cover all 64 banks) */
#define BG_BIAS 256 /* = MI_GUARD (mi_host.h): slack bytes in front of / behind every tensor these kernels read; a tap shift of
                       up to (W + 1) elements must fit: W <= 120 (mi_bgemm_supported) */

struct BgArgs {
    int N, C, K, H, W, Ho, Wo; // KS x KS, stride S, pad KS/2
    int HW, P;
    int ncols;                 // fwd/dgrad: N*Pc columns
    int Pc;                    // fwd/dgrad: columns per image: P, or P rounded up to 8 for the 16-byte staging (columns >= P of an image: masked)
    FastDiv fdPc;
    int mtiles, tiles;
    int nhalf, cb64;           // wgrad: 64-column halves = T * C/64; C/64
    int klen;                  // wgrad: reduction length per split (multiple of 32)
    FastDiv fdP, fdWo, fdM, fdCb;
    float *bn_part;            // forward: statistics partials, three planes [bn_np][K]
    int bn_np;
    int vw;                    // fwd / dgrad-s1 epilogue: pixels per store (8, 4 or 1)
    // dgrad (pixel-major epilogue) that also does the REDUCTION pass of the batch-norm backward its output feeds: the stored
    // gradient is gated by bnb_mask > 0, and per (column tile, channel) the sums of g and g (x - mean) go to bnb_part
    const u16 *bnb_x, *bnb_mask;
    const float *bnb_mean;
    float *bnb_part;           // two planes [bnb_np][C]
    int bnb_np;
};

__device__ __forceinline__ float bg_bf2f(u16 v) { return __uint_as_float((uint32_t)v << 16); }
__device__ __forceinline__ uint32_t bg_pack2(float a, float b) { // round to nearest even, NaN stays NaN (v_cvt_pk_bf16_f32)
    f32x2 v = {a, b};
    bf16x2 r = __builtin_convertvector(v, bf16x2);
    return *(uint32_t *)&r;
}
__device__ __forceinline__ u16 bg_f2bf(float a) { return (u16)(bg_pack2(a, 0.f) & 0xffffu); }

// 16-bit lane masks of one dword from two validity bits
__device__ __forceinline__ uint32_t bg_lane_mask(uint32_t two_bits) {
    return ((two_bits & 1u) ? 0x0000ffffu : 0u) | ((two_bits & 2u) ? 0xffff0000u : 0u);
}
template <int VW> struct BgVec;
template <> struct BgVec<8> { typedef u32x4 T; };
template <> struct BgVec<4> { typedef u32x2 T; };
template <> struct BgVec<1> { typedef u32x2 T; }; // unused placeholder
// loads of VW bf16 whose address is only 2-byte aligned (a tap shifts the pixel index by one): gfx950 under ROCm serves them
// at the streaming rate (tools/ubench/unaligned_load.hip: 5.9 TB/s at every element shift)
typedef u32x4 __attribute__((aligned(2))) u32x4_u;
typedef u32x2 __attribute__((aligned(2))) u32x2_u;
template <int VW> __device__ __forceinline__ typename BgVec<VW>::T bg_ldv(const char *p) {
    if constexpr (VW == 8) return *(const u32x4_u *)p;
    else return *(const u32x2_u *)p;
}

// VW (wgrad only) = pixels per operand load: 1 = element-wise gathers (any plane size); 8 / 4 = 16- / 8-byte loads along the
// pixels (plane size a multiple of VW; stride 2: output ROW length a multiple of VW).  Forward and dgrad always gather
// element-wise along the pixels of a wave (see bgemm_stage_vw for what was measured).
// SWP (forward / dgrad with 16-byte staging, planes a multiple of 4 pixels, not the strided stride-2 dgrad scatter): the
// product is taken the other way round (pixels = accumulator rows, channels = columns), so a lane ends up with 4 CONSECUTIVE
// pixels of ONE output channel per accumulator quad: 8- / 16-byte stores and lane-local BN statistics, no LDS round trip.
// SBUF (SWP only): ONE operand buffer, two barriers per k-step, the next k-step's loads held in registers across the multiply:
// half the LDS, so THREE workgroups per CU.  Wins where the tile count fills 768 slots about as well as 512 (bgemm_single_buffer).
template <int MODE, int KS, int S, int WMW, int VW, int SWP, int SBUF>
__global__ void __launch_bounds__(256)
bgemm_kernel(const u16 *__restrict__ Aop, const u16 *__restrict__ Bop, void *__restrict__ OutV, const u16 *__restrict__ addend,
             const BgArgs g) {
    constexpr int BM = 64 * WMW;
    constexpr int TN = WMW == 2 ? 2 : 1;
    constexpr int WNC = 32 * TN;
    constexpr int T = KS * KS, PAD = KS / 2;
    constexpr int NA = BM / 32;              // fwd/dgrad: 16-byte loads of A per thread and tile (BM x 64 bf16)
    constexpr int NAS = BM / 4;              // wgrad, VW == 1: 2-byte loads of A per thread and tile
    constexpr bool VEC = MODE == BG_WGRAD && VW > 1;
    // forward / dgrad with 16-byte operand loads (VW == 8; the source pixels of 8 consecutive columns are consecutive in memory:
    // stride-1 forward, every dgrad): a thread loads 8 pixels of 4 ADJACENT channels -- 16 lanes cover 128 pixels of one
    // channel plane, 256 contiguous bytes -- transposes them in registers (v_perm) and writes 8 bytes (4 channels) per pixel.
    // Its LDS image has pitch 160 bytes with the 16-byte chunks of a row rotated by (row >> 4): ds_read_b128 stays
    // conflict-free, the transposing ds_write_b64 are 2-way (tools: the search in DESIGN.md section 7).
    constexpr bool VB = MODE != BG_WGRAD && VW == 8;
    constexpr int LDBB = VB ? 160 : BG_LDB;   // pitch of the B image
    constexpr bool SB = SWP && SBUF;
    typedef typename BgVec<VW>::T LT;
    constexpr int LW = VW / 2;               // dwords per vector load
    // wgrad vector staging: a unit = VW pixels of one row; BG_BK / VW units per 64-pixel row
    constexpr int NPU = VEC ? BG_BK / VW : 1;
    constexpr int RPT = 256 / NPU;           // rows one pass of the 256 threads covers
    constexpr int NAU = VEC ? BM / RPT : 1, NBU = VEC ? 128 / RPT : 1;
    constexpr bool S2W = false; // (stride-2 weight gradients read the parity planes of x: unit stride, one load)
    extern __shared__ __attribute__((aligned(16))) unsigned char bg_smem[];
    unsigned char *As = bg_smem;                         // [2][BM][BG_LDB]
    unsigned char *Bs = bg_smem + 2 * BM * BG_LDB;       // [2][128][LDBB]  (SWP with a one-k-step reduction: [1][..] each)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = WMW == 2 ? wave >> 1 : 0, wn = WMW == 2 ? wave & 1 : wave;

    // ---- block -> tile (XCD-contiguous, M-tiles fastest: the blocks that share a gathered pixel tile share an L2) ----
    auto map_tile = [&](uint32_t L, uint32_t &ct_, int &m0_, int &n0_) {
        const uint32_t per = (uint32_t)g.tiles >> 3;
        if (L < per * 8) L = (L & 7) * per + (L >> 3);
        ct_ = fd_div(L, g.fdM);
        m0_ = (int)(L - ct_ * g.mtiles) * BM;
        n0_ = (int)ct_ * 128;
    };
    uint32_t ct;
    int m0, n0;
    // wgrad: (tile, split) from a SPLIT-major list cut into eight contiguous pieces, one per XCD (workgroups go to the XCDs round-robin by
    // linear id): all the tiles that reduce over one stretch of pixels run on one XCD at about the same time, so each operand byte is
    // fetched from HBM by one L2 (tile-major placement had every XCD's L2 fetch the whole reduction range for its tiles): 3x3 on 128
    // channels at 28x28 0.190 -> 0.118 ms, 1x1 1024 -> 256 at 14x14 0.083 -> 0.064 ms
    uint32_t wg_split = blockIdx.y;
    if (MODE == BG_WGRAD && gridDim.y >= 8) { // (fewer splits than XCDs: the tile-major pieces of map_tile, which split the OPERANDS over the XCDs)
        const uint32_t T_ = gridDim.x, tot = T_ * gridDim.y, per = tot >> 3;
        uint32_t V = blockIdx.y * T_ + blockIdx.x;
        if (V < per * 8) V = (V & 7) * per + (V >> 3);
        wg_split = V / T_;
        const uint32_t tl = V - wg_split * T_;
        ct = fd_div(tl, g.fdM);
        m0 = (int)(tl - ct * g.mtiles) * BM;
        n0 = (int)ct * 128;
    } else map_tile(blockIdx.x, ct, m0, n0);

    f32x16 acc[2][TN];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    // ---- per-thread staging state (byte offsets; every tensor is < 2^32 bytes: mi_bgemm_supported) ----
    uint32_t b_lane = 0;
    uint32_t mask = 0;
    int ph = 0, pw = 0, ntaps = 1;
    int ntiles = 0, kend = 0;
    int hf_r[2] = {0, 0}, hf_s[2] = {0, 0}, hf_ok[2] = {0, 0};
    uint32_t hf_c[2] = {0, 0};
    uint32_t vb_lane = 0;       // VB: byte offset (+ BG_BIAS) of (image, centre pixel of the thread's first column, its first channel)
    uint64_t vm_lo = 0;         // VB: validity of the thread's 8 pixels, 8 bits per tap, taps 0..7
    uint32_t vm_hi = 0;         //     tap 8
    if (MODE == BG_FWD || MODE == BG_DGRAD) {
        if (MODE == BG_FWD) { ntaps = T; ntiles = T * (g.C / BG_BK); }
        else if (S == 1) { ntaps = T; ntiles = T * (g.K / BG_BK); }
        else {
            const int cls = 3 - (int)blockIdx.y; // heaviest class (4 taps) first
            ph = cls >> 1; pw = cls & 1;
            ntaps = (ph ? 2 : 1) * (pw ? 2 : 1);
            ntiles = ntaps * (g.K / BG_BK);
        }
    }
    if (SWP && (ntiles == 1 || SB)) Bs = bg_smem + BM * BG_LDB;
    // forward / dgrad: the staging state of the tile at column n0 (per thread: source offsets and tap masks of its columns)
    auto tile_state = [&]() {
        // validity of column j's tap t (bit t), and the byte offset of its centre pixel in channel 0 of its image
        auto column = [&](int j, uint32_t &centre) -> uint32_t {
            const uint32_t jc = j < g.ncols ? (uint32_t)j : (uint32_t)g.ncols - 1;
            const uint32_t n = fd_div(jc, g.fdPc);
            const uint32_t q = jc - n * g.Pc;
            const bool jin = j < g.ncols && q < (uint32_t)g.P; // (padding columns of an image: no output pixel)
            const uint32_t p = min(q, (uint32_t)g.P - 1);
            const uint32_t ho = fd_div(p, g.fdWo), wo = p - ho * g.Wo;
            uint32_t m = 0;
            if (MODE == BG_FWD && S == 2 && VB) {
                // x comes as four parity planes per channel (bg_s2d_kernel): [n][c][ph][pw][Ho][Wo].  Tap (r, s) reads plane
                // ((r + 1) & 1, (s + 1) & 1) at (ho - (r == 0), wo - (s == 0)): unit stride along the output pixels
                centre = (uint32_t)(n * g.C * g.HW + p) * 2u;
#pragma unroll
                for (int t = 0; t < T; t++)
                    if (jin && (int)ho - (t / KS == 0) >= 0 && (int)wo - (t % KS == 0) >= 0) m |= 1u << t;
            } else if (MODE == BG_FWD) {
                centre = (uint32_t)(n * g.C * g.HW + (S * ho) * g.W + S * wo) * 2u;
#pragma unroll
                for (int t = 0; t < T; t++) {
                    const int hi = S * (int)ho - PAD + t / KS, wi = S * (int)wo - PAD + t % KS;
                    if (jin && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W) m |= 1u << t;
                }
            } else if (S == 1) {
                centre = (uint32_t)(n * g.K * g.P + p) * 2u;
#pragma unroll
                for (int t = 0; t < T; t++) {
                    const int hs = (int)ho + PAD - t / KS, ws = (int)wo + PAD - t % KS;
                    if (jin && hs >= 0 && hs < g.Ho && ws >= 0 && ws < g.Wo) m |= 1u << t;
                }
            } else {
                centre = (uint32_t)(n * g.K * g.P + p) * 2u; // (a, b) itself is always a valid source pixel
                const int ntw = pw ? 2 : 1;
                for (int tt = 0; tt < ntaps; tt++) {
                    const int th = tt / ntw, tw = tt - th * ntw;
                    const int dh = (ph && th == 0) ? 1 : 0, dw = (pw && tw == 0) ? 1 : 0;
                    if (jin && (int)ho + dh < g.Ho && (int)wo + dw < g.Wo) m |= 1u << tt;
                }
            }
            return m;
        };
        const uint32_t plane = (uint32_t)(MODE == BG_FWD ? g.HW : g.P);
        if (!VB) {
            uint32_t centre;
            mask = column(n0 + (tid & 127), centre);
            b_lane = centre + (uint32_t)(32 * (tid >> 7)) * plane * 2u; // + the first reduction channel of this thread within a tile
        } else {
            const int col0 = n0 + (tid & 15) * 8;
            uint32_t c0 = 0;
            vm_lo = 0; vm_hi = 0;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                uint32_t ce;
                const uint32_t m = column(col0 + e, ce);
                if (e == 0) c0 = ce;
#pragma unroll
                for (int t = 0; t < 8; t++) vm_lo |= (uint64_t)((m >> t) & 1u) << (8 * t + e);
                vm_hi |= ((m >> 8) & 1u) << e;
            }
            // (a group past the last column decodes to the last column for every pixel: mask 0, loads in bounds)
            // + BG_BIAS: the unsigned offset stays non-negative when a tap points a few pixels in front of the tensor; the base
            // pointer is lowered to match
            vb_lane = c0 + (uint32_t)(4 * (tid >> 4)) * plane * 2u + BG_BIAS;
        }
    };
    if (MODE == BG_FWD || MODE == BG_DGRAD) {
        tile_state();
    } else {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t u = 2u * ct + h;
            const uint32_t tp = fd_div(u, g.fdCb);
            hf_ok[h] = u < (uint32_t)g.nhalf;
            const int tap = hf_ok[h] ? (int)tp : 0;
            hf_r[h] = tap / KS; hf_s[h] = tap - KS * hf_r[h];
            hf_c[h] = hf_ok[h] ? (u - tp * g.cb64) * 64u : 0u;
        }
        const int kbeg = (int)wg_split * g.klen;
        kend = min(g.N * g.Pc, kbeg + g.klen);
        ntiles = (kend - kbeg + BG_BK - 1) / BG_BK;
    }

    // registers of the tile in flight
    // SWP 3x3: TWO k-steps of loads in flight (two register sets: +3-6 % on the 3x3 layers; the 1x1 layers gained nothing and a
    // one-k-step launch lost its third resident workgroup to the registers)
    constexpr int NSET = (SWP && KS == 3 && !SB) ? 2 : 1;
    u32x4 ra4[NSET][NA];
    u16 ra[NAS], rb[32];
    u32x4 vb[NSET][4];                      // VB: 8 pixels of 4 adjacent channels
    uint32_t vmask[NSET] = {};
    LT wa[NAU], wb[NBU][S2W ? 2 : 1];       // VEC wgrad
    uint32_t wmask[NBU], wamask = 0;
    int sel_a = 1, sel_b = 1;
    int ld_t = 0, ld_c0 = 0;
    int ld_k0 = (MODE == BG_WGRAD) ? (int)wg_split * g.klen : 0;
    auto ldg16 = [](const char *ubase, uint32_t lane_off) -> u16 { return *(const u16 *)(ubase + lane_off); };

    bool abl_started = false;
    constexpr std::integral_constant<int, 0> I0{};
    constexpr std::integral_constant<int, NSET - 1> I1{};
    auto fetch = [&](auto set_tag) {
        constexpr int SET = decltype(set_tag)::value;
        if (MODE == BG_FWD || MODE == BG_DGRAD) {
            const int t = min(ld_t, ntaps - 1); // the two drain iterations re-read the last tap
            sel_b = (mask >> t) & 1;
            const char *fa, *fb;
            int shift;        // element offset of tap t's source pixel from the centre pixel
            size_t bstride;
            if (MODE == BG_FWD) {
                const int r = KS == 3 ? (t * 11) >> 5 : 0, s = t - KS * r;
                fa = (const char *)(Aop + ((size_t)(t * (g.C / BG_BK) + ld_c0 / BG_BK) * g.K + m0) * BG_BK);
                fb = (const char *)(Bop + (size_t)ld_c0 * g.HW);
                if (S == 2 && VB) shift = (2 * ((r + 1) & 1) + ((s + 1) & 1)) * g.P - (r == 0) * g.Wo - (s == 0); // parity layout
                else shift = (r - PAD) * g.W + (s - PAD);
                bstride = (size_t)g.HW * 2;
                ld_c0 += BG_BK;
                if (ld_c0 == g.C) { ld_c0 = 0; ld_t++; }
            } else {
                int wt;
                if (S == 1) {
                    const int r = KS == 3 ? (t * 11) >> 5 : 0, s = t - KS * r;
                    wt = t;
                    shift = (PAD - r) * g.Wo + (PAD - s);
                } else {
                    const int th = pw ? t >> 1 : t, tw = pw ? t & 1 : 0;
                    const int r = ph ? 2 * th : 1, s = pw ? 2 * tw : 1;
                    wt = 3 * r + s;
                    shift = (ph & (th ^ 1)) * g.Wo + (pw & (tw ^ 1));
                }
                fa = (const char *)(Aop + ((size_t)(wt * (g.K / BG_BK) + ld_c0 / BG_BK) * g.C + m0) * BG_BK);
                fb = (const char *)(Bop + (size_t)ld_c0 * g.P);
                bstride = (size_t)g.P * 2;
                ld_c0 += BG_BK;
                if (ld_c0 == g.K) { ld_c0 = 0; ld_t++; }
            }
            if (BG_ABLATE >= 1 && BG_ABLATE <= 3 && abl_started) { /* keep the registers of the first tiles */ }
            else if (!VB) {
                const uint32_t fb_lane = b_lane + (uint32_t)(sel_b * shift * 2); // outside: centre pixel, stored as 0
#pragma unroll
                for (int q = 0; q < 32; q++) rb[q] = ldg16(fb + (size_t)q * bstride, fb_lane);
            } else {
                vmask[SET] = t < 8 ? (uint32_t)(vm_lo >> (8 * t)) & 0xffu : vm_hi;
                const uint32_t off = vb_lane + (uint32_t)((vmask[SET] ? shift : 0) * 2); // no valid pixel at all: stay on the centre
                // two passes of 4 channels: this thread's channels 4 cq .. 4 cq + 3 and + 64 would be the next tile, so the
                // 64-channel tile is covered by cq = 0..15 with 4 channels each
#pragma unroll
                for (int c = 0; c < 4; c++) vb[SET][c] = bg_ldv<8>(fb - BG_BIAS + (size_t)c * bstride + off);
            }
            if (!(BG_ABLATE >= 2 && BG_ABLATE <= 3 && abl_started)) {
#pragma unroll
                for (int q = 0; q < NA; q++) ra4[SET][q] = *(const u32x4 *)(fa + (size_t)(tid + 256 * q) * 16);
            }
        } else if (!VEC) {
            const int kk = ld_k0 + (tid & 63);
            sel_a = kk < kend;
            const uint32_t kc = sel_a ? (uint32_t)kk : (uint32_t)kend - 1;
            const uint32_t n = fd_div_ge2(kc, g.fdP);
            const uint32_t pp = kc - n * g.P;
            const uint32_t ho = fd_div_ge2(pp, g.fdWo), wo = pp - ho * g.Wo;
            const uint32_t row = (uint32_t)tid >> 6;
            const char *fa = (const char *)(Aop + (size_t)m0 * g.P);
            const uint32_t fa_lane = (n * (uint32_t)(g.K * g.P) + pp + row * g.P) * 2u;
#pragma unroll
            for (int q = 0; q < NAS; q++) ra[q] = ldg16(fa + (size_t)(4 * q) * g.P * 2, fa_lane);
            sel_b = 0;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int hi = S * (int)ho - PAD + hf_r[h], wi = S * (int)wo - PAD + hf_s[h];
                const int inb = (int)((uint32_t)hi < (uint32_t)g.H) & (int)((uint32_t)wi < (uint32_t)g.W);
                const uint32_t pix = inb ? (uint32_t)(hi * g.W + wi) : (S * ho) * g.W + S * wo;
                const uint32_t fb_lane = (n * (uint32_t)(g.C * g.HW) + pix + (row + hf_c[h]) * g.HW) * 2u;
                sel_b |= (sel_a & inb & hf_ok[h]) << h;
#pragma unroll
                for (int q = 0; q < 16; q++) rb[16 * h + q] = ldg16((const char *)Bop + (size_t)(4 * q) * g.HW * 2, fb_lane);
            }
            ld_k0 += BG_BK;
        } else {
            // VW consecutive pixels of one image per load: dY rows as they lie, x rows shifted by the tap.  The reduction index
            // runs over (image, q) with q < Pc = P rounded up to VW: pixels q >= P of an image are masked in BOTH operands.
            // Stride 2: x comes as four parity planes per channel (bg_s2d_kernel), so every tap is a unit-stride read as well.
            constexpr uint32_t ones = (1u << VW) - 1u;
            const int part = tid % NPU, row0 = tid / NPU;
            const int kk = ld_k0 + part * VW;
            sel_a = kk < kend;
            const uint32_t kc = sel_a ? (uint32_t)kk : (uint32_t)(kend - VW);
            const uint32_t n = fd_div_ge2(kc, g.fdPc);
            const uint32_t pp = kc - n * g.Pc;                       // < P: a group never starts in the padding
            const uint32_t ho0 = fd_div_ge2(pp, g.fdWo), wo0 = pp - ho0 * g.Wo;
            const int cntv = min(VW, g.P - (int)pp);
            const uint32_t inimg = sel_a ? (cntv >= VW ? ones : ((1u << cntv) - 1u)) : 0u;
            const char *fa = (const char *)(Aop + (size_t)m0 * g.P);
            const uint32_t fa_lane = (n * (uint32_t)(g.K * g.P) + pp + (uint32_t)row0 * g.P) * 2u;
#pragma unroll
            for (int q = 0; q < NAU; q++) wa[q] = bg_ldv<VW>(fa + (size_t)(RPT * q) * g.P * 2 + fa_lane);
            wamask = inimg;
            // the VW pixels may run over the end of an output row once (VW <= Wo: bgemm_stage_vw)
            const int ew = g.Wo - (int)wo0;
            const uint32_t lo = ew >= VW ? ones : ((1u << ew) - 1u), hi = ones & ~lo;
#pragma unroll
            for (int q = 0; q < NBU; q++) {
                const int col = row0 + RPT * q;
                const int h = (RPT * q) >> 6;          // compile-time
                const int r = h ? hf_r[1] : hf_r[0], s = h ? hf_s[1] : hf_s[0];
                const uint32_t cbase = (h ? hf_c[1] : hf_c[0]) + (uint32_t)(col & 63);
                // taps that look one row up / one column left, one row down / one column right (stride 2: never down / right)
                const bool up = S == 1 ? r < PAD : r == 0, down = S == 1 && r > PAD;
                const bool left = S == 1 ? s < PAD : s == 0, right = S == 1 && s > PAD;
                const uint32_t rm = up ? (((int)ho0 >= 1 ? lo : 0u) | hi)
                                       : down ? (((int)ho0 <= g.Ho - 2 ? lo : 0u) | ((int)ho0 + 1 <= g.Ho - 2 ? hi : 0u)) : ones;
                const uint32_t cm = left ? ones & ~((wo0 == 0 ? 1u : 0u) | (ew < VW ? (1u << ew) : 0u))
                                         : right ? ones & ~((ew - 1 < VW) ? (1u << (ew - 1)) : 0u) : ones;
                uint32_t m = (KS == 1 ? ones : rm & cm) & inimg;
                int pix;
                if (S == 1) pix = (int)pp + (r - PAD) * g.W + (s - PAD);
                else pix = (2 * ((r + 1) & 1) + ((s + 1) & 1)) * g.P + (int)pp - (r == 0) * g.Wo - (s == 0); // parity plane + offset
                if (m == 0) pix = (int)pp; // nothing valid: stay on a pixel that exists
                // + BG_BIAS: the unsigned offset stays non-negative when a tap points a few pixels in front of the tensor (masked
                // lanes inside the allocation's guard bytes); the base pointer is lowered to match
                const uint32_t off = (n * (uint32_t)(g.C * g.HW) + cbase * (uint32_t)g.HW + (uint32_t)(pix + BG_BIAS / 2)) * 2u;
                wb[q][0] = bg_ldv<VW>((const char *)Bop - BG_BIAS + off);
                wmask[q] = (h ? hf_ok[1] : hf_ok[0]) ? m : 0u;
            }
            ld_k0 += BG_BK;
        }
    };
    // every other 16-bit element of two consecutive vectors (a stride-2 span) packed into one
    auto evens = [](const LT a, const LT b) -> LT {
        LT o;
        if constexpr (VW == 8) {
            o[0] = __builtin_amdgcn_perm(a[1], a[0], 0x05040100u); o[1] = __builtin_amdgcn_perm(a[3], a[2], 0x05040100u);
            o[2] = __builtin_amdgcn_perm(b[1], b[0], 0x05040100u); o[3] = __builtin_amdgcn_perm(b[3], b[2], 0x05040100u);
        } else {
            o[0] = __builtin_amdgcn_perm(a[1], a[0], 0x05040100u); o[1] = __builtin_amdgcn_perm(b[1], b[0], 0x05040100u);
        }
        return o;
    };
    auto stash = [&](auto set_tag, const int buf) {
        constexpr int SET = decltype(set_tag)::value;
        unsigned char *as = As + buf * (BM * BG_LDB), *bs = Bs + buf * (128 * LDBB);
        if (MODE == BG_WGRAD) {
            if (!VEC) {
                const int kx = tid & 63, row = tid >> 6;
#pragma unroll
                for (int q = 0; q < NAS; q++) *(u16 *)(as + (row + 4 * q) * BG_LDB + kx * 2) = sel_a ? ra[q] : (u16)0;
#pragma unroll
                for (int q = 0; q < 32; q++)
                    *(u16 *)(bs + (row + 4 * q) * BG_LDB + kx * 2) = ((sel_b >> (q >> 4)) & 1) ? rb[q] : (u16)0;
            } else {
                const int part = tid % NPU, row0 = tid / NPU;
#pragma unroll
                for (int q = 0; q < NAU; q++) {
                    LT v = wa[q];
#pragma unroll
                    for (int j = 0; j < LW; j++) v[j] &= bg_lane_mask(wamask >> (2 * j));
                    *(LT *)(as + (row0 + RPT * q) * BG_LDB + part * (VW * 2)) = v;
                }
#pragma unroll
                for (int q = 0; q < NBU; q++) {
                    LT v;
                    if constexpr (S2W) v = evens(wb[q][0], wb[q][1]); else v = wb[q][0];
#pragma unroll
                    for (int j = 0; j < LW; j++) v[j] &= bg_lane_mask(wmask[q] >> (2 * j));
                    *(LT *)(bs + (row0 + RPT * q) * BG_LDB + part * (VW * 2)) = v;
                }
            }
        } else {
            if (!VB) {
                // transposed on the way in: 32 channels of ONE pixel -> 64 contiguous bytes of the pixel's LDS row
                const int bj = tid & 127, kh = tid >> 7;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    u32x4 v;
#pragma unroll
                    for (int q = 0; q < 4; q++) v[q] = sel_b ? ((uint32_t)rb[8 * i + 2 * q] | ((uint32_t)rb[8 * i + 2 * q + 1] << 16)) : 0u;
                    *(u32x4 *)(bs + bj * LDBB + kh * 64 + 16 * i) = v;
                }
            } else {
                // 4 channels x 8 pixels in registers -> per pixel one 8-byte piece (channels 4 cq .. 4 cq + 3) of its LDS row
                const int g8 = tid & 15, cq = tid >> 4;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    u32x2 e0 = {__builtin_amdgcn_perm(vb[SET][1][j], vb[SET][0][j], 0x05040100u), __builtin_amdgcn_perm(vb[SET][3][j], vb[SET][2][j], 0x05040100u)};
                    u32x2 e1 = {__builtin_amdgcn_perm(vb[SET][1][j], vb[SET][0][j], 0x07060302u), __builtin_amdgcn_perm(vb[SET][3][j], vb[SET][2][j], 0x07060302u)};
                    if (!((vmask[SET] >> (2 * j)) & 1u)) { e0[0] = 0u; e0[1] = 0u; }
                    if (!((vmask[SET] >> (2 * j + 1)) & 1u)) { e1[0] = 0u; e1[1] = 0u; }
                    const int r0 = 8 * g8 + 2 * j, r1 = r0 + 1; // r0 >> 4 == r1 >> 4 == g8 >> 1
                    const int chunk = ((cq >> 1) + (g8 >> 1)) & 7;
                    *(u32x2 *)(bs + r0 * LDBB + chunk * 16 + (cq & 1) * 8) = e0;
                    *(u32x2 *)(bs + r1 * LDBB + chunk * 16 + (cq & 1) * 8) = e1;
                }
            }
#pragma unroll
            for (int q = 0; q < NA; q++) {
                const int u = tid + 256 * q;
                if (!(BG_ABLATE == 8)) *(u32x4 *)(as + (u >> 3) * BG_LDB + (u & 7) * 16) = ra4[SET][q];
            }
        }
    };

    const int fr = lane & 31, fk = lane >> 5;
    auto compute = [&](const int buf) {
        const unsigned char *as = As + buf * (BM * BG_LDB) + (wm * 64 + fr) * BG_LDB + fk * 16;
        const unsigned char *bs = Bs + buf * (128 * LDBB) + (wn * WNC + fr) * LDBB + (VB ? 0 : fk * 16);
#pragma unroll
        for (int s = 0; s < BG_BK / 16; s++) {
            bf16x8 av[2], bv[TN];
#pragma unroll
            for (int i = 0; i < 2; i++) {
                if (BG_ABLATE == 8 && MODE != BG_WGRAD) { u32x4 t = ra4[0][(2 * i + s) % NA]; av[i] = *(bf16x8 *)&t; } /* experiment: A operand without LDS */
                else av[i] = *(const bf16x8 *)(as + i * 32 * BG_LDB + s * 32);
            }
#pragma unroll
            for (int j = 0; j < TN; j++) {
                if (VB) { // chunk (2 s + fk) of the row, rotated by (row >> 4)
                    const int rot = (wn * WNC + j * 32 + fr) >> 4;
                    bv[j] = *(const bf16x8 *)(bs + j * 32 * LDBB + ((2 * s + fk + rot) & 7) * 16);
                } else bv[j] = *(const bf16x8 *)(bs + j * 32 * LDBB + s * 32);
            }
            if (BG_ABLATE == 4) { // keep the fragment reads alive without the matrix pipe
#pragma unroll
                for (int i = 0; i < 2; i++) asm volatile("" ::"v"(av[i]));
#pragma unroll
                for (int j = 0; j < TN; j++) asm volatile("" ::"v"(bv[j]));
            } else {
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int j = 0; j < TN; j++) {
                        if constexpr (SWP) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bv[j], av[i], acc[i][j], 0, 0, 0);
                        else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
                    }
            }
        }
    };
    u16 *Out = (u16 *)OutV;
    const int Mdim = MODE == BG_FWD ? g.K : g.C;
    const int Pout = MODE == BG_FWD ? g.P : g.HW;
    const bool stats = MODE == BG_FWD && g.bn_part != nullptr && BG_ABLATE != 7;
    auto epi_swp = [&]() {
        // accumulator (i, j): rows = the 32 pixels of column tile j, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5); column = channel
        // m0 + wm 64 + i 32 + (lane & 31).  A quad r = 4 q .. 4 q + 3 is 4 consecutive pixels: whole or padding (plane % 4 == 0).
        const int l31 = lane & 31, hh = lane >> 5;
        uint32_t okm = 0;   // bit j * 4 + q: the quad holds real pixels
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int col = n0 + wn * WNC + j * 32 + 8 * q + 4 * hh;
                const uint32_t cc = (uint32_t)min(col, g.ncols - 1);
                const uint32_t n = fd_div(cc, g.fdPc), pp = cc - n * g.Pc;
                if (col < g.ncols && pp < (uint32_t)g.P) { okm |= 1u << (j * 4 + q); cnt += 4; }
            }
        // lane-local BN statistics of the wave's 64 channels x WNC pixels (a lane holds TN * 16 pixels of ONE channel)
#pragma unroll
        for (int i = 0; i < 2; i++) {
            if (!stats) break;
            const int m = m0 + wm * 64 + i * 32 + l31;
            const float s0 = __shfl(acc[i][0][0], l31, 64); // the wave's first pixel (always a real one if any is)
            float sd = 0.f, sq = 0.f;
#pragma unroll
            for (int j = 0; j < TN; j++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const bool ok = (okm >> (j * 4 + q)) & 1u;
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const float d = ok ? acc[i][j][4 * q + e] - s0 : 0.f;
                        sd += d;
                        sq = fmaf(d, d, sq);
                    }
                }
            sd += __shfl_xor(sd, 32, 64);
            sq += __shfl_xor(sq, 32, 64);
            const int nvw = cnt + __shfl_xor(cnt, 32, 64);
            if (hh == 0) {
                constexpr int PPT = 4 / WMW;
                const float inv = nvw > 0 ? 1.0f / (float)nvw : 0.f;
                const size_t plane = (size_t)g.bn_np * g.K;
                const size_t o = (size_t)(ct * PPT + wn) * g.K + m;
                g.bn_part[o] = (float)nvw;
                g.bn_part[plane + o] = nvw > 0 ? s0 + sd * inv : 0.f;
                g.bn_part[2 * plane + o] = fmaxf(sq - sd * sd * inv, 0.f);
            }
        }
        // Stores.  Straight from the accumulators a wave instruction would touch 32 channel rows with 16-32 bytes each, and the
        // L2 takes one request per piece (measured: the stores alone were 40 % of a short-reduction layer).  So the wave's tile
        // goes through a wave-private LDS image [64 channels][WNC pixels] (the operand tiles are dead after the loop's last
        // barrier) and is read back with lanes running ALONG a channel row: a wave instruction then writes whole 128-byte lines.
        // dgrad keeps fp32 in the image so that the shortcut addend is added before the one rounding to bf16.
        constexpr bool F32I = MODE == BG_DGRAD;
        constexpr int ESZ = F32I ? 4 : 2;
        constexpr int PITCH = WNC * ESZ + 16;
        constexpr int IROWS = F32I ? 32 : 64;  // channel rows per image: the fp32 image takes the wave's two 32-row halves in turn
        unsigned char *img = bg_smem + wave * (IROWS * PITCH);
        auto fill = [&](const int i) {         // accumulators (i, *) -> image rows (F32I ? 0 : 32 i) + lane & 31
#pragma unroll
            for (int j = 0; j < TN; j++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    unsigned char *d = img + ((F32I ? 0 : i * 32) + l31) * PITCH + (j * 32 + 8 * q + 4 * hh) * ESZ;
                    if constexpr (F32I) {
                        pf4 v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                        *(pf4 *)d = v;
                    } else {
                        u32x2 v = {bg_pack2(acc[i][j][4 * q], acc[i][j][4 * q + 1]), bg_pack2(acc[i][j][4 * q + 2], acc[i][j][4 * q + 3])};
                        *(u32x2 *)d = v;
                    }
                }
        };
        auto drain = [&](auto cpx_tag, const int ch0) { // image rows -> channels m0 + wm 64 + ch0 + row
            constexpr int CPX = decltype(cpx_tag)::value; // pixels per lane and store: 8 (16 bytes) or 4
            constexpr int CPR = WNC / CPX;                 // lanes along one channel row
            constexpr int RPP = 64 / CPR;                  // channel rows per wave instruction
            const int c = lane % CPR, r0 = lane / CPR;
            const int col = n0 + wn * WNC + c * CPX;
            const uint32_t cc = (uint32_t)min(col, g.ncols - 1);
            const uint32_t n = fd_div(cc, g.fdPc), pp = cc - n * g.Pc;
            const bool ok = col < g.ncols && pp < (uint32_t)g.P; // (a group of CPX pixels is whole or padding)
            const uint32_t obase = n * (uint32_t)(Mdim * Pout) + pp;
#pragma unroll
            for (int ps = 0; ps < IROWS / RPP; ps++) {
                const int row = ps * RPP + r0;
                const size_t o = (size_t)(obase + (uint32_t)(m0 + wm * 64 + ch0 + row) * (uint32_t)Pout);
                const unsigned char *sp = img + row * PITCH + c * CPX * ESZ;
                uint32_t pk[CPX / 2];
                if constexpr (F32I) {
                    float w[CPX];
#pragma unroll
                    for (int e = 0; e < CPX / 4; e++) {
                        const pf4 v = *(const pf4 *)(sp + 16 * e);
                        w[4 * e] = v[0]; w[4 * e + 1] = v[1]; w[4 * e + 2] = v[2]; w[4 * e + 3] = v[3];
                    }
                    if (addend && ok) {
                        uint32_t ad[CPX / 2];
                        if constexpr (CPX == 8) { const u32x4 a4 = *(const u32x4 *)(addend + o); ad[0] = a4[0]; ad[1] = a4[1]; ad[2] = a4[2]; ad[3] = a4[3]; }
                        else { const u32x2 a2 = *(const u32x2 *)(addend + o); ad[0] = a2[0]; ad[1] = a2[1]; }
#pragma unroll
                        for (int e = 0; e < CPX / 2; e++) {
                            w[2 * e] += __uint_as_float(ad[e] << 16);
                            w[2 * e + 1] += __uint_as_float(ad[e] & 0xffff0000u);
                        }
                    }
#pragma unroll
                    for (int e = 0; e < CPX / 2; e++) pk[e] = bg_pack2(w[2 * e], w[2 * e + 1]);
                    if (g.bnb_part) { // (uniform) the BN' reduction over this wave's WNC pixels of channel `row`
                        const int ch = m0 + wm * 64 + ch0 + row;
                        const float mean = g.bnb_mean[ch];
                        float s1 = 0.f, s2 = 0.f;
                        if (ok) {
                            uint32_t xv[CPX / 2], mv[CPX / 2];
                            if constexpr (CPX == 8) {
                                const u32x4 x4 = *(const u32x4 *)(g.bnb_x + o), m4 = *(const u32x4 *)(g.bnb_mask + o);
#pragma unroll
                                for (int e = 0; e < 4; e++) { xv[e] = x4[e]; mv[e] = m4[e]; }
                            } else {
                                const u32x2 x2 = *(const u32x2 *)(g.bnb_x + o), m2 = *(const u32x2 *)(g.bnb_mask + o);
#pragma unroll
                                for (int e = 0; e < 2; e++) { xv[e] = x2[e]; mv[e] = m2[e]; }
                            }
#pragma unroll
                            for (int e = 0; e < CPX / 2; e++) {
                                // the gradient as it is STORED (rounded), gated by the sign of the activation; bf16 > 0 <=> its 16 bits
                                // as a signed integer > 0 (NaN aside)
                                const bool on0 = (int16_t)(mv[e] & 0xffffu) > 0, on1 = (int32_t)mv[e] > 0xffff;
                                const float g0 = on0 ? __uint_as_float(pk[e] << 16) : 0.f, g1 = on1 ? __uint_as_float(pk[e] & 0xffff0000u) : 0.f;
                                pk[e] = (on0 ? pk[e] & 0xffffu : 0u) | (on1 ? pk[e] & 0xffff0000u : 0u);
                                s1 += g0 + g1;
                                s2 = fmaf(g0, __uint_as_float(xv[e] << 16) - mean, s2);
                                s2 = fmaf(g1, __uint_as_float(xv[e] & 0xffff0000u) - mean, s2);
                            }
                        }
#pragma unroll
                        for (int m = 1; m < CPR; m <<= 1) { s1 += __shfl_xor(s1, m, 64); s2 += __shfl_xor(s2, m, 64); }
                        if (c == 0) {
                            constexpr int PPT = 4 / WMW;
                            const size_t po = (size_t)(ct * PPT + wn) * Mdim + ch;
                            g.bnb_part[po] = s1;
                            g.bnb_part[(size_t)g.bnb_np * Mdim + po] = s2;
                        }
                    }
                } else {
                    if constexpr (CPX == 8) { const u32x4 v = *(const u32x4 *)sp; pk[0] = v[0]; pk[1] = v[1]; pk[2] = v[2]; pk[3] = v[3]; }
                    else { const u32x2 v = *(const u32x2 *)sp; pk[0] = v[0]; pk[1] = v[1]; }
                }
                if (ok) {
                    if constexpr (CPX == 8) { u32x4 st = {pk[0], pk[1], pk[2], pk[3]}; *(u32x4 *)(Out + o) = st; }
                    else { u32x2 st = {pk[0], pk[1]}; *(u32x2 *)(Out + o) = st; }
                }
            }
        };
        auto drain_vw = [&](const int ch0) {
            if (g.vw == 8) drain(std::integral_constant<int, 8>{}, ch0);
            else drain(std::integral_constant<int, 4>{}, ch0);
        };
        if constexpr (F32I) {
            fill(0); drain_vw(0);
            fill(1); drain_vw(32);
        } else {
            fill(0); fill(1); drain_vw(0);
        }
    };
    if constexpr (SWP) {
        // No loads past the reduction's end (a short reduction -- 1 to 4 k-steps for the 1x1 expansions -- would otherwise wait for loads it never
        // uses); a one-k-step launch gets by with a single operand buffer (the host then allocates one: 3 workgroups per CU)
        if constexpr (SB) {
            fetch(I0);
            stash(I0, 0);
            if (ntiles > 1) fetch(I0);
            __syncthreads();
            int it = 0;
            for (; it + 2 < ntiles; it++) {
                compute(0);
                __syncthreads();
                stash(I0, 0);
                fetch(I0);
                __syncthreads();
            }
            if (it + 1 < ntiles) {
                compute(0);
                __syncthreads();
                stash(I0, 0);
                __syncthreads();
            }
            compute(0);
        } else if constexpr (NSET == 2) {
            fetch(I0);                  // k-step 0
            if (ntiles > 1) fetch(I1);  // k-step 1
            stash(I0, 0);
            if (ntiles > 2) fetch(I0);  // k-step 2
            __syncthreads();
            int it = 0;
            for (; it + 4 < ntiles; it += 2) { // k-step it from LDS, it + 1 -> LDS, it + 2 in flight, it + 3 issued
                stash(I1, 1); fetch(I1); compute(0); __syncthreads();
                stash(I0, 0); fetch(I0); compute(1); __syncthreads();
            }
            for (; it < ntiles; it++) {
                const int buf = it & 1;
                if (it + 1 < ntiles) { if (buf) stash(I0, 0); else stash(I1, 1); }
                if (it + 3 < ntiles) { if (buf) fetch(I0); else fetch(I1); }
                compute(buf);
                if (it + 1 < ntiles) __syncthreads();
            }
        } else {
            fetch(I0);
            stash(I0, 0);
            if (ntiles > 1) fetch(I0);
            __syncthreads();
            int it = 0;
            for (; it + 2 < ntiles; it++) {
                const int buf = it & 1;
                stash(I0, buf ^ 1);
                fetch(I0);
                compute(buf);
                __syncthreads();
            }
            if (it + 1 < ntiles) {
                stash(I0, (it & 1) ^ 1);
                compute(it & 1);
                __syncthreads();
                it++;
            }
            compute(it & 1);
        }
        __syncthreads(); // the epilogue re-uses the operand buffers
        if (BG_ABLATE != 6) epi_swp();
        return;
    }
    fetch(I0);
    stash(I0, 0);
    fetch(I0);
    abl_started = true;
    __syncthreads();
    for (int it = 0; it < ntiles; it++) {
        const int buf = it & 1;
        if (!(BG_ABLATE == 3)) stash(I0, buf ^ 1); // tile it+1 (held in registers) -> the other buffer; then the registers take tile it+2
        fetch(I0);
        compute(buf);
        __syncthreads();
    }

    // ---- epilogue: accumulator layout col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) ----
    if (MODE == BG_WGRAD) {
        float *Out = (float *)OutV;
#pragma unroll
        for (int j = 0; j < TN; j++) {
            const int lc = wn * WNC + j * 32 + (lane & 31);
            const int h = lc >> 6; // wave-uniform; selects (no runtime-indexed arrays: they would live in scratch)
            if (!(h ? hf_ok[1] : hf_ok[0])) continue;
            const int tap = h ? hf_r[1] * KS + hf_s[1] : hf_r[0] * KS + hf_s[0];
            const size_t coff = ((size_t)((size_t)wg_split * T + tap) * g.K) * g.C + (h ? hf_c[1] : hf_c[0]) + (lc & 63);
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int row = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    Out[coff + (size_t)row * g.C] = acc[i][j][r];
                }
        }
        return;
    }
    if (BG_ABLATE == 6) { /* experiment: no epilogue at all */
        float sacc = 0.f;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < TN; j++)
#pragma unroll
                for (int r = 0; r < 16; r++) sacc += acc[i][j][r];
        if (sacc == 1.2345678f) Out[0] = 1;
        return;
    }

    const bool wide = g.vw > 1 && !(MODE == BG_DGRAD && S == 2);
    if (wide || stats) {
        // each wave transposes 64 rows x 32 columns at a time through its own 8 KB of LDS (the tiles are dead after the
        // loop's last barrier): lane = row then owns 32 consecutive columns
        float *tw = (float *)bg_smem + wave * (32 * 64);
        const int l31 = lane & 31, row = lane;
        const int rowg = m0 + wm * 64 + row;
        int nvw = 0;              // valid columns of this wave (padding columns of an image and columns past the end excluded)
        float s0 = 0.f, sd = 0.f, sq = 0.f;
#pragma unroll
        for (int j = 0; j < TN; j++) {
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int rg = 0; rg < 4; rg++) {
                    const int row4 = i * 8 + rg * 2 + (lane >> 5);
                    pf4 q4 = {acc[i][j][rg * 4 + 0], acc[i][j][rg * 4 + 1], acc[i][j][rg * 4 + 2], acc[i][j][rg * 4 + 3]};
                    *(pf4 *)(tw + l31 * 64 + ((row4 ^ (l31 & 15)) << 2)) = q4;
                }
            float v[32];
#pragma unroll
            for (int c = 0; c < 32; c++) v[c] = tw[c * 64 + ((((row >> 2) ^ (c & 15))) << 2) + (row & 3)];
            if (stats) {
                if (j == 0) s0 = v[0];
#pragma unroll
                for (int gq = 0; gq < 4; gq++) { // the valid columns of an 8-column group are a prefix of it
                    const int col = n0 + wn * WNC + j * 32 + 8 * gq;
                    int cnt = 0;
                    if (col < g.ncols) {
                        const uint32_t nn = fd_div((uint32_t)col, g.fdPc);
                        cnt = min(8, max(0, g.P - (int)((uint32_t)col - nn * g.Pc)));
                    }
                    nvw += cnt;
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const float d = e < cnt ? v[8 * gq + e] - s0 : 0.f;
                        sd += d;
                        sq = fmaf(d, d, sq);
                    }
                }
            }
            if (wide) {
                const int colb = n0 + wn * WNC + j * 32;
                if (g.vw == 8) {
#pragma unroll
                    for (int gq = 0; gq < 4; gq++) {
                        const int col = colb + 8 * gq;
                        if (col < g.ncols) { // vw == 8: the plane is a multiple of 8, no padding columns
                            const uint32_t n = fd_div((uint32_t)col, g.fdPc);
                            const uint32_t p = (uint32_t)col - n * g.Pc;
                            const size_t o = ((size_t)n * Mdim + rowg) * Pout + p;
                            float w8[8];
#pragma unroll
                            for (int e = 0; e < 8; e++) w8[e] = v[8 * gq + e];
                            if (MODE == BG_DGRAD && addend) {
                                const u32x4 ad = *(const u32x4 *)(addend + o);
#pragma unroll
                                for (int e = 0; e < 4; e++) {
                                    w8[2 * e] += __uint_as_float(ad[e] << 16);
                                    w8[2 * e + 1] += __uint_as_float(ad[e] & 0xffff0000u);
                                }
                            }
                            u32x4 pk;
#pragma unroll
                            for (int e = 0; e < 4; e++) pk[e] = bg_pack2(w8[2 * e], w8[2 * e + 1]);
                            if (BG_ABLATE == 5) { if (pk[0] == 0x12345678u) *(u32x4 *)(Out + o) = pk; } /* experiment: no output stores */
                            else *(u32x4 *)(Out + o) = pk;
                        }
                    }
                } else { // 4 pixels per store
#pragma unroll
                    for (int gq = 0; gq < 8; gq++) {
                        const int col = colb + 4 * gq;
                        const uint32_t n = fd_div((uint32_t)min(col, g.ncols - 1), g.fdPc);
                        const uint32_t p = (uint32_t)min(col, g.ncols - 1) - n * g.Pc;
                        if (col < g.ncols && p < (uint32_t)g.P) { // groups of 4 are whole: the plane is a multiple of 4
                            const size_t o = ((size_t)n * Mdim + rowg) * Pout + p;
                            float w4[4];
#pragma unroll
                            for (int e = 0; e < 4; e++) w4[e] = v[4 * gq + e];
                            if (MODE == BG_DGRAD && addend) {
                                const u32x2 ad = *(const u32x2 *)(addend + o);
#pragma unroll
                                for (int e = 0; e < 2; e++) {
                                    w4[2 * e] += __uint_as_float(ad[e] << 16);
                                    w4[2 * e + 1] += __uint_as_float(ad[e] & 0xffff0000u);
                                }
                            }
                            u32x2 pk = {bg_pack2(w4[0], w4[1]), bg_pack2(w4[2], w4[3])};
                            *(u32x2 *)(Out + o) = pk;
                        }
                    }
                }
            }
        }
        if (stats) {
            constexpr int PPT = 4 / WMW;
            const float inv = nvw > 0 ? 1.0f / (float)nvw : 0.f;
            const size_t plane = (size_t)g.bn_np * g.K;
            const size_t o = (size_t)(ct * PPT + wn) * g.K + rowg;
            g.bn_part[o] = (float)nvw;
            g.bn_part[plane + o] = nvw > 0 ? s0 + sd * inv : 0.f;
            g.bn_part[2 * plane + o] = fmaxf(sq - sd * sd * inv, 0.f);
        }
    }
    if (!wide) {
        // 2-byte stores straight from the accumulators (planes whose size is not a multiple of 4, stride-2 dgrad)
#pragma unroll
        for (int j = 0; j < TN; j++) {
            const int col = n0 + wn * WNC + j * 32 + (lane & 31);
            if (col >= g.ncols) continue;
            const uint32_t n = fd_div((uint32_t)col, g.fdPc);
            const uint32_t p = (uint32_t)col - n * g.Pc;
            if (p >= (uint32_t)g.P) continue; // padding column
            size_t coff;
            if (MODE == BG_FWD) coff = (size_t)n * g.K * g.P + p;
            else if (S == 1) coff = (size_t)n * g.C * g.HW + p;
            else {
                const uint32_t a = fd_div(p, g.fdWo), b = p - a * g.Wo;
                coff = (size_t)n * g.C * g.HW + (size_t)(2 * a + ph) * g.W + 2 * b + pw;
            }
#pragma unroll
            for (int i = 0; i < 2; i++) {
                float ad[16];
                if (MODE == BG_DGRAD && addend) {
#pragma unroll
                    for (int r = 0; r < 16; r++)
                        ad[r] = bg_bf2f(addend[coff + (size_t)(m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * Pout]);
                }
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int row = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    float v = acc[i][j][r];
                    if (MODE == BG_DGRAD && addend) v += ad[r];
                    Out[coff + (size_t)row * Pout] = bg_f2bf(v);
                }
            }
        }
    }
}

// weights KCRS fp32 -> bf16 k-step tiles.  fwd: [t][c/32][K][32] (inner = c); dgrad: [t][k/32][C][32] (inner = k).
// One launch for MANY layers (table in device memory, as igemm_wt_all_kernel): block = one 32 x 32 (k, c) tile of one layer.
__global__ void __launch_bounds__(256)
bg_wt_all_kernel(const mid_wt_entry *__restrict__ entries, const int *__restrict__ tile_entry) {
    __shared__ float tile[32][9 * 32 + 1];
    const mid_wt_entry E = entries[tile_entry[blockIdx.x]];
    const int tl = (int)blockIdx.x - E.tile0, ctiles = E.C / 32, T = E.T;
    const int c0 = (tl % ctiles) * 32, k0 = (tl / ctiles) * 32, row = T * 32;
    for (int e = threadIdx.x; e < 32 * row; e += 256) {
        const int kr = e / row, x = e - kr * row;
        tile[kr][x] = E.w[((size_t)(k0 + kr) * E.C + c0) * T + x];
    }
    __syncthreads();
    u16 *fw = (u16 *)E.fwd, *dg = (u16 *)E.dgrad;
    for (int e = threadIdx.x; e < T * 1024; e += 256) {
        const int t = e >> 10, u = (e >> 5) & 31, v = e & 31; // v fastest = contiguous output dim
        if (fw) fw[((size_t)(t * (E.C / BG_BK) + c0 / BG_BK) * E.K + k0 + u) * BG_BK + (c0 % BG_BK) + v] = bg_f2bf(tile[u][v * T + t]);
        if (dg) dg[((size_t)(t * (E.K / BG_BK) + k0 / BG_BK) * E.C + c0 + u) * BG_BK + (k0 % BG_BK) + v] = bg_f2bf(tile[v][u * T + t]);
    }
}
// the same for one layer (operator layer / no table): grid (C/32, K/32)
template <int T>
__global__ void __launch_bounds__(256)
bg_wt_kernel(const float *__restrict__ w, u16 *__restrict__ fw, u16 *__restrict__ dg, int K, int C) {
    __shared__ float tile[32][T * 32 + 1];
    const int k0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int e = threadIdx.x; e < 32 * T * 32; e += 256) {
        const int kr = e / (T * 32), x = e - kr * (T * 32);
        tile[kr][x] = w[((size_t)(k0 + kr) * C + c0) * T + x];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < T * 1024; e += 256) {
        const int t = e >> 10, u = (e >> 5) & 31, v = e & 31;
        if (fw) fw[((size_t)(t * (C / BG_BK) + c0 / BG_BK) * K + k0 + u) * BG_BK + (c0 % BG_BK) + v] = bg_f2bf(tile[u][v * T + t]);
        if (dg) dg[((size_t)(t * (K / BG_BK) + k0 / BG_BK) * C + c0 + u) * BG_BK + (k0 % BG_BK) + v] = bg_f2bf(tile[v][u * T + t]);
    }
}

// x [NC][H][W] -> four parity planes [NC][ph][pw][H/2][W/2] (bf16; H, W even): what the stride-2 forward convolution and its
// weight gradient read with unit stride.  One thread: two input rows x 16 columns (two 16-byte loads each, any 2-byte
// alignment) -> 8 output pixels (one 16-byte store) in each of the 4 planes.
__global__ void __launch_bounds__(256)
bg_s2d_kernel(const u16 *__restrict__ x, u16 *__restrict__ out, uint32_t units, int H, int W, FastDiv fdUW, FastDiv fdHo) {
    const int Ho = H / 2, Wo = W / 2, UW = (W + 15) / 16; // units per row pair
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
        const uint32_t t = fd_div(u, fdUW);
        const int ux = (int)(u - t * UW);
        const uint32_t nc = fd_div(t, fdHo);
        const int a = (int)(t - nc * Ho);
        const u16 *src = x + (size_t)nc * H * W + (size_t)(2 * a) * W + 16 * ux;
        u16 *dst = out + (size_t)nc * H * W + (size_t)a * Wo + 8 * ux;
        const int nv = min(16, W - 16 * ux); // valid columns of this unit (W need not be a multiple of 16)
#pragma unroll
        for (int ph = 0; ph < 2; ph++) {
            if (nv == 16) {
                const u32x4 v0 = *(const u32x4_u *)(src + (size_t)ph * W), v1 = *(const u32x4_u *)(src + (size_t)ph * W + 8);
                u32x4 ev = {__builtin_amdgcn_perm(v0[1], v0[0], 0x05040100u), __builtin_amdgcn_perm(v0[3], v0[2], 0x05040100u),
                            __builtin_amdgcn_perm(v1[1], v1[0], 0x05040100u), __builtin_amdgcn_perm(v1[3], v1[2], 0x05040100u)};
                u32x4 od = {__builtin_amdgcn_perm(v0[1], v0[0], 0x07060302u), __builtin_amdgcn_perm(v0[3], v0[2], 0x07060302u),
                            __builtin_amdgcn_perm(v1[1], v1[0], 0x07060302u), __builtin_amdgcn_perm(v1[3], v1[2], 0x07060302u)};
                *(u32x4_u *)(dst + (size_t)(2 * ph) * Ho * Wo) = ev;
                *(u32x4_u *)(dst + (size_t)(2 * ph + 1) * Ho * Wo) = od;
            } else {
                int e0 = 0;
                if (nv >= 8) { // the first 8 columns as one 16-byte load, two 8-byte stores
                    const u32x4 v = *(const u32x4_u *)(src + (size_t)ph * W);
                    u32x2 ev = {__builtin_amdgcn_perm(v[1], v[0], 0x05040100u), __builtin_amdgcn_perm(v[3], v[2], 0x05040100u)};
                    u32x2 od = {__builtin_amdgcn_perm(v[1], v[0], 0x07060302u), __builtin_amdgcn_perm(v[3], v[2], 0x07060302u)};
                    *(u32x2_u *)(dst + (size_t)(2 * ph) * Ho * Wo) = ev;
                    *(u32x2_u *)(dst + (size_t)(2 * ph + 1) * Ho * Wo) = od;
                    e0 = 8;
                }
                for (int e = e0; e < nv; e++) dst[(size_t)(2 * ph + (e & 1)) * Ho * Wo + (e >> 1)] = src[(size_t)ph * W + e];
            }
        }
    }
}
static int bg_s2d(hipStream_t st, const u16 *x, u16 *out, long NC, int H, int W) {
    const int UW = (W + 15) / 16, Ho = H / 2;
    const long units = NC * Ho * UW;
    if (units >= 2147483648L) { mi_record_error("bg_s2d", "tensor too large"); return -2; }
    long blocks = (units + 255) / 256;
    if (blocks > 65536 * 8) blocks = 65536 * 8;
    mi_prof_begin(st, MI_FAM_PCONV, 0.0, 4.0 * (double)NC * H * W); /* part of the stride-2 layers' cost: counted in the 3x3 family's time */
    hipLaunchKernelGGL(bg_s2d_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, out, (uint32_t)units, H, W, make_fastdiv(UW), make_fastdiv(Ho));
    mi_prof_end(st);
    MI_LAUNCH_CHECK("bg_s2d_kernel");
    return 0;
}

// fp32 <-> bf16 tensors (operator layer, tests)
__global__ void __launch_bounds__(256) bg_f2b_kernel(const float *__restrict__ in, u16 *__restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = bg_f2bf(in[i]);
}
__global__ void __launch_bounds__(256) bg_b2f_kernel(const u16 *__restrict__ in, float *__restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = bg_bf2f(in[i]);
}

// ------------------------------------------------------------------------------------------------------------
int mi_bgemm_supported(int op, int N, int C, int H, int K, int k, int stride) {
    if (!((k == 1 && stride == 1) || (k == 3 && (stride == 1 || stride == 2)))) return 0;
    if (H % stride || H / stride < 2 || H > 120) return 0;
    if ((double)N * C * H * H >= 2147480000.0 || (double)N * K * (H / stride) * (H / stride) >= 2147480000.0) return 0; /* 32-bit byte offsets (+ BG_BIAS) */
    return C % 64 == 0 && K % 64 == 0; /* tiles: 64 rows, 64 reduction elements */
}
#define BG_SLOTS 512 /* 256 CUs x 2 resident workgroups (72 KB of LDS) */
static int bgemm_wgrad_splits_p(long kd, int C, int K, int k);
static int bgemm_wgrad_splits(int N, int C, int H, int K, int k, int stride) {
    const int bm = K % 128 == 0 ? 128 : 64;
    const long nhalf = (long)k * k * (C / 64);
    const long tiles = ((nhalf + 1) / 2) * (K / bm);
    const long ksteps = ((long)N * (H / stride) * (H / stride) + BG_BK - 1) / BG_BK;
    int best = 1;
    double best_eff = 0;
    for (int s = 1; s <= 512; s++) {
        if (s > 1 && ksteps / s < 32) break;
        const double waves = (double)tiles * s / BG_SLOTS;
        const double eff = waves / (double)((long)((tiles * s + BG_SLOTS - 1) / BG_SLOTS));
        if (eff > best_eff + 0.02) { best_eff = eff; best = s; }
    }
    return best;
}
extern "C" size_t mi_bgemm_part_floats(int N, int C, int H, int K, int k, int stride) {
    const int P = (H / stride) * (H / stride);
    int mx = 1;
    for (int vw = 1; vw <= 8; vw *= 2) { // the launch picks its split count on the padded reduction length: take the largest
        const int s = bgemm_wgrad_splits_p((long)N * ((P + vw - 1) / vw * vw), C, K, k);
        if (s > mx) mx = s;
    }
    return (size_t)mx * k * k * K * C;
}

static void bgemm_geometry(BgArgs &g, int N, int C, int H, int K, int stride) {
    g.N = N; g.C = C; g.K = K; g.H = H; g.W = H; g.Ho = H / stride; g.Wo = H / stride;
    g.HW = H * H; g.P = g.Ho * g.Wo;
    g.Pc = g.P; g.ncols = N * g.P;
    g.fdP = make_fastdiv(g.P); g.fdWo = make_fastdiv(g.Wo); g.fdPc = g.fdP;
    g.fdCb = make_fastdiv(1);
}
// the launch-trace name of the last bgemm_kernel launch: op, taps, stride, rows per tile, pixels per staged load, pixel-major product, one buffer
static thread_local const char *bg_variant = "bgemm_kernel";
template <int MODE, int KS, int S, int WMW, int VW, int SWP = 0, int SBUF = 0>
static int bgemm_launch_t(hipStream_t st, dim3 grid, const u16 *A, const u16 *B, void *out, const u16 *addend, const BgArgs &g) {
    constexpr int BM = 64 * WMW;
    constexpr size_t ldbb = (MODE != BG_WGRAD && VW == 8) ? 160 : BG_LDB;
    constexpr size_t tiles_b = (size_t)2 * (BM * BG_LDB + 128 * ldbb), ep_b = (size_t)4 * 32 * 64 * 4;
    size_t lds = tiles_b > ep_b ? tiles_b : ep_b;
    if (SWP) { // its epilogue image (<= 36 KB) fits one operand buffer; a one-k-step reduction uses one buffer only
        const int ksteps = (MODE == BG_FWD ? g.C : g.K) / BG_BK * KS * KS;
        lds = (ksteps == 1 || SBUF) ? tiles_b / 2 : tiles_b;
    }
    // raised once per instantiation to the largest value any launch of it can ask for (`lds` varies at run time for the SWP forms:
    // a one-k-step launch followed by a multi-k-step one of the same instantiation must not find the limit at the smaller value)
    static int attr_set = 0;
    if (!attr_set) {
        constexpr size_t lds_max = tiles_b > ep_b ? tiles_b : ep_b;
        if (lds_max > 64 * 1024 &&
            hipFuncSetAttribute((const void *)bgemm_kernel<MODE, KS, S, WMW, VW, SWP, SBUF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max) != hipSuccess) {
            mi_record_error("bgemm_kernel", "cannot raise the dynamic LDS limit");
            return -1;
        }
        attr_set = 1;
    }
    hipLaunchKernelGGL((bgemm_kernel<MODE, KS, S, WMW, VW, SWP, SBUF>), grid, dim3(256), lds, st, A, B, out, addend, g);
    bg_variant = mi_trace_name("bgemm_kernel<%s,k%d,s%d,bm%d,vw%d%s%s>", MODE == BG_FWD ? "fwd" : MODE == BG_DGRAD ? "dgrad" : "wgrad", KS, S, BM, VW,
                               SWP ? ",swp" : "", SBUF ? ",sbuf" : "");
    return 0;
}
// One operand buffer and three resident workgroups per CU (768 slots), or two buffers and two (512)?  Measured per layer at
// N = 256 (tools/bench_ops.py --bf16): with every slot busy three workgroups deliver about 1.1x (3x3: the two-buffer form also
// keeps two k-steps of loads in flight) to 1.2x (1x1) the throughput of two, so the choice is the one whose LAST ROUND of
// workgroups is fuller: 3x3 @56 (6272 tiles) 0.167 -> 0.138 ms, the 256->512 / 512->1024 projections 0.71 -> 0.66-0.68, but
// 256 ch @14 (800 tiles: 1.04 rounds of 768) 0.114 -> 0.120.  RESNET_MI_BF16_SBUF=0|1 forces it.
static int bgemm_single_buffer(int tiles, int ks) {
    static int force = -1;
    if (force < 0) { const char *e = getenv("RESNET_MI_BF16_SBUF"); force = e ? atoi(e) : 2; }
    if (force == 0 || force == 1) return force;
    const double gain = ks == 1 ? 1.2 : 1.1;
    const double t2 = (double)((tiles + BG_SLOTS - 1) / BG_SLOTS) * 2.0;
    const double t3 = (double)((tiles + 767) / 768) * 3.0 / gain;
    return t3 < t2;
}
static int bgemm_swp_enabled(void) {
    static int swp_on = -1;
    if (swp_on < 0) { const char *e = getenv("RESNET_MI_BF16_SWP"); swp_on = e ? atoi(e) : 1; }
    return swp_on;
}
template <int MODE, int KS, int S>
static int bgemm_launch_v(hipStream_t st, dim3 grid, const u16 *A, const u16 *B, void *out, const u16 *addend, const BgArgs &g, int bm, int vw) {
    // the pixel-major product (SWP): 16-byte staging, planes a multiple of 4 pixels, contiguous output pixels
    const int swp_on = bgemm_swp_enabled();
    if constexpr (MODE != BG_WGRAD && !(MODE == BG_DGRAD && S == 2)) {
        if (vw == 8 && g.vw > 1 && swp_on) {
            if (bgemm_single_buffer(g.tiles, KS)) {
                if (bm == 128) return bgemm_launch_t<MODE, KS, S, 2, 8, 1, 1>(st, grid, A, B, out, addend, g);
                return bgemm_launch_t<MODE, KS, S, 1, 8, 1, 1>(st, grid, A, B, out, addend, g);
            }
            if (bm == 128) return bgemm_launch_t<MODE, KS, S, 2, 8, 1>(st, grid, A, B, out, addend, g);
            return bgemm_launch_t<MODE, KS, S, 1, 8, 1>(st, grid, A, B, out, addend, g);
        }
    }
    if (bm == 128) {
        if (vw == 8) return bgemm_launch_t<MODE, KS, S, 2, 8>(st, grid, A, B, out, addend, g);
        if (vw == 4) return bgemm_launch_t<MODE, KS, S, 2, 4>(st, grid, A, B, out, addend, g);
        return bgemm_launch_t<MODE, KS, S, 2, 1>(st, grid, A, B, out, addend, g);
    }
    if (vw == 8) return bgemm_launch_t<MODE, KS, S, 1, 8>(st, grid, A, B, out, addend, g);
    if (vw == 4) return bgemm_launch_t<MODE, KS, S, 1, 4>(st, grid, A, B, out, addend, g);
    return bgemm_launch_t<MODE, KS, S, 1, 1>(st, grid, A, B, out, addend, g);
}
// vw: pixels per operand load of the STAGING (1 = element-wise); see bgemm_stage_vw
template <int MODE>
static int bgemm_launch(hipStream_t st, dim3 grid, const u16 *A, const u16 *B, void *out, const u16 *addend, const BgArgs &g, int k,
                        int stride, int bm, int vw) {
    if (k == 1 && stride == 1) return bgemm_launch_v<MODE, 1, 1>(st, grid, A, B, out, addend, g, bm, vw);
    if (k == 3 && stride == 1) return bgemm_launch_v<MODE, 3, 1>(st, grid, A, B, out, addend, g, bm, vw);
    if (k == 3 && stride == 2) return bgemm_launch_v<MODE, 3, 2>(st, grid, A, B, out, addend, g, bm, vw);
    return -2;
}
// Pixels per operand load of a forward's or dgrad's staging: the 16-byte form (8), whose source pixels must be consecutive in memory --
// every dgrad, forward with stride 1, and forward with stride 2 once x has been re-laid as parity planes (the caller checks it has the
// buffer) -- at any plane size (the column space is padded to groups of 8 per image); RESNET_MI_BF16_VW below 8: element-wise gathers
// (1, the first correct form).  The weight gradient's width is bgemm_wgrad_vw's.
static int bgemm_stage_vw(void) {
    static int cap = -1;
    if (cap < 0) { const char *e = getenv("RESNET_MI_BF16_VW"); cap = e ? atoi(e) : 8; }
    return cap >= 8 ? 8 : 1;
}
static int bgemm_fam(int k) { return k == 1 ? MI_FAM_GEMM : MI_FAM_PCONV; }
static int bgemm_pick_bm(int M, long coltiles) {
    if (M % 128) return 64;
    static int force = -1;
    if (force < 0) { const char *e = getenv("RESNET_MI_BF16_BM"); force = e ? atoi(e) : 0; }
    if (force == 64 || force == 128) return force;
    // 64-row tiles where 128-row ones would leave most of the chip empty (fewer than one workgroup per CU)
    return (long)(M / 128) * coltiles < 256 ? 64 : 128;
}
static int bgemm_vw(int P) { return P % 8 == 0 ? 8 : P % 4 == 0 ? 4 : 1; }
// output tiling of a forward (M = K) or dgrad (M = C) once the staging width svw is known (8: the column space padded to groups of 8
// pixels per image); returns the rows per tile
static int bgemm_plan_tiles(BgArgs &g, int M, int svw) {
    if (svw == 8) { g.Pc = (g.P + 7) / 8 * 8; g.ncols = g.N * g.Pc; g.fdPc = make_fastdiv(g.Pc); }
    const int ctl = mi_cdiv(g.ncols, 128);
    const int bm = bgemm_pick_bm(M, ctl);
    g.mtiles = M / bm;
    g.tiles = g.mtiles * ctl;
    g.fdM = make_fastdiv(g.mtiles);
    return bm;
}

static int bg_prelayout_one(hipStream_t st, const float *w, u16 *fw, u16 *dg, int K, int C, int k) {
    if (k == 1) hipLaunchKernelGGL(bg_wt_kernel<1>, dim3(C / 32, K / 32), dim3(256), 0, st, w, fw, dg, K, C);
    else hipLaunchKernelGGL(bg_wt_kernel<9>, dim3(C / 32, K / 32), dim3(256), 0, st, w, fw, dg, K, C);
    MI_LAUNCH_CHECK("bg_wt_kernel");
    return 0;
}

int mi_bgemm_fwd(hipStream_t st, mid_workspace *ws, const u16 *x, const float *w, u16 *y, int N, int C, int H, int K, int k, int stride,
                 mid_bn_parts *parts) {
    const int T = k * k;
    const u16 *A = (const u16 *)ws->pre_fwd;
    if (!A) {
        if (!ws->wt || ws->wt_floats * 2 < (size_t)T * C * K) { mi_record_error("mi_bgemm_fwd", "workspace too small"); return -3; }
        if (bg_prelayout_one(st, w, (u16 *)ws->wt, nullptr, K, C, k)) return -1;
        A = (const u16 *)ws->wt;
    }
    BgArgs g = {};
    bgemm_geometry(g, N, C, H, K, stride);
    int svw = bgemm_stage_vw();
    ws->s2d_valid = 0; // on return: 1 = this launch left x as parity planes in ws->s2d (the layer's weight gradient may reuse them)
    if (stride == 2 && svw == 8) { // the 16-byte staging reads x as parity planes: one pass over x first
        if (ws->s2d && ws->s2d_bytes >= (size_t)N * C * g.HW * 2) {
            if (bg_s2d(st, x, (u16 *)ws->s2d, (long)N * C, H, H)) return -1;
            x = (const u16 *)ws->s2d;
            ws->s2d_valid = 1;
        } else svw = 1;
    }
    const int bm = bgemm_plan_tiles(g, K, svw);
    const int ctl = mi_cdiv(g.ncols, 128);
    g.vw = bgemm_vw(g.P);
    if (parts) {
        parts->nparts = 0;
        const int np = ctl * (bm == 128 ? 2 : 4);
        if (parts->buf && parts->floats >= (size_t)3 * np * K) { g.bn_part = parts->buf; g.bn_np = np; parts->nparts = np; }
    }
    mi_prof_begin(st, bgemm_fam(k), 2.0 * T * (double)N * g.P * C * K, 2.0 * ((double)N * C * g.HW + (double)N * g.P * K) + 4.0 * T * C * K);
    const int rc = bgemm_launch<BG_FWD>(st, dim3(g.tiles), A, x, y, nullptr, g, k, stride, bm, svw);
    mi_prof_end(st);
    if (rc) return rc;
    MI_LAUNCH_CHECK(bg_variant);
    return 0;
}

// fz (optional): the reduction pass of the batch-norm backward that consumes dx, fused into this kernel's epilogue where the
// launch takes the pixel-major form; fz->nparts > 0 on return says it did (dx then holds the GATED gradient)
int mi_bgemm_dgrad(hipStream_t st, mid_workspace *ws, const float *w, const u16 *dy, u16 *dx, const u16 *addend, int N, int C, int H,
                   int K, int k, int stride, mid_bn_bwd_parts *fz) {
    if (fz) fz->nparts = 0;
    const int T = k * k;
    const u16 *A = (const u16 *)ws->pre_dgrad;
    if (!A) {
        if (!ws->wt || ws->wt_floats * 2 < (size_t)T * C * K) { mi_record_error("mi_bgemm_dgrad", "workspace too small"); return -3; }
        if (bg_prelayout_one(st, w, nullptr, (u16 *)ws->wt, K, C, k)) return -1;
        A = (const u16 *)ws->wt;
    }
    BgArgs g = {};
    bgemm_geometry(g, N, C, H, K, stride);
    const int svw = bgemm_stage_vw();
    const int bm = bgemm_plan_tiles(g, C, svw);
    const int ctl = mi_cdiv(g.ncols, 128);
    g.vw = bgemm_vw(g.HW);
    if (fz && fz->buf && stride == 1 && svw == 8 && g.vw > 1 && bgemm_swp_enabled()) {
        const int np = ctl * (bm == 128 ? 2 : 4);
        if (fz->floats >= (size_t)2 * np * C) {
            g.bnb_x = (const u16 *)fz->x; g.bnb_mask = (const u16 *)fz->mask; g.bnb_mean = fz->means;
            g.bnb_part = fz->buf; g.bnb_np = np; fz->nparts = np;
        }
    }
    mi_prof_begin(st, bgemm_fam(k), 2.0 * T * (double)N * g.P * C * K,
                  2.0 * ((double)N * g.P * K + (double)N * C * g.HW * ((addend ? 2 : 1) + (g.bnb_part ? 2 : 0))) + 4.0 * T * C * K);
    const int rc = bgemm_launch<BG_DGRAD>(st, dim3(g.tiles, stride == 2 ? 4 : 1), A, dy, dx, addend, g, k, stride, bm, svw);
    mi_prof_end(st);
    if (rc) return rc;
    MI_LAUNCH_CHECK(bg_variant);
    return 0;
}

int mi_igemm_wgrad_reduce(hipStream_t st, const float *part, float *dw, int K, int C, int k, int splits); // kernels_igemm.hip

static int bgemm_wgrad_vw(int Wo, int stride, bool have_parity) {
    static int cap = -1;
    if (cap < 0) { const char *e = getenv("RESNET_MI_BF16_VW"); cap = e ? atoi(e) : 8; }
    if (stride == 2 && !have_parity) return 1;
    // a span of VW output pixels may leave its output row once: VW <= Wo
    int vw = Wo >= 8 ? 8 : Wo >= 4 ? 4 : 1;
    if (vw > cap) vw = cap >= 4 && Wo >= 4 ? 4 : 1;
    return vw;
}
static int bgemm_wgrad_splits_p(long kd, int C, int K, int k) {
    const int bm = K % 128 == 0 ? 128 : 64;
    const long nhalf = (long)k * k * (C / 64);
    const long tiles = ((nhalf + 1) / 2) * (K / bm);
    const long ksteps = (kd + BG_BK - 1) / BG_BK;
    int best = 1;
    double best_eff = 0;
    for (int s = 1; s <= 512; s++) {
        if (s > 1 && ksteps / s < 32) break;
        const double waves = (double)tiles * s / BG_SLOTS;
        const double eff = waves / (double)((long)((tiles * s + BG_SLOTS - 1) / BG_SLOTS));
        if (eff > best_eff + 0.02) { best_eff = eff; best = s; }
    }
    return best;
}
// geometry, tiling and reduction split of a weight gradient (parity_ok: x may be read as parity planes); returns the rows per tile,
// *vw = pixels per staged load, *splits = what the split heuristic asked for, *used = the splits launched (grid.y)
static int bgemm_plan_wgrad(BgArgs &g, int N, int C, int H, int K, int k, int stride, bool parity_ok, int *vw, int *splits, int *used) {
    const int T = k * k;
    bgemm_geometry(g, N, C, H, K, stride);
    *vw = bgemm_wgrad_vw(g.Wo, stride, parity_ok);
    if (*vw > 1) { g.Pc = (g.P + *vw - 1) / *vw * *vw; g.fdPc = make_fastdiv(g.Pc); }
    const long kd = (long)N * g.Pc;
    *splits = bgemm_wgrad_splits_p(kd, C, K, k);
    const int bm = K % 128 == 0 ? 128 : 64;
    g.mtiles = K / bm;
    g.cb64 = C / 64;
    g.nhalf = T * g.cb64;
    g.fdCb = make_fastdiv(g.cb64);
    g.tiles = g.mtiles * ((g.nhalf + 1) / 2);
    g.fdM = make_fastdiv(g.mtiles);
    g.klen = mi_cdiv(mi_cdiv(kd, *splits), BG_BK) * BG_BK;
    *used = mi_cdiv(kd, g.klen);
    return bm;
}
extern "C" int mi_bgemm_wgrad(mid_stream s, mid_workspace *ws, const void *xv, const void *dyv, float *dw, int N, int C, int H, int K, int k, int stride) {
    hipStream_t st = (hipStream_t)s;
    const u16 *x = (const u16 *)xv, *dy = (const u16 *)dyv;
    const int T = k * k;
    if (!mi_bgemm_supported(BGOP_WGRAD, N, C, H, K, k, stride)) { mi_record_error("mi_bgemm_wgrad", "shape not supported by the bf16 kernels"); return -2; }
    BgArgs g = {};
    const bool parity_ok = stride == 2 && ws && ws->s2d && ws->s2d_bytes >= (size_t)N * C * H * H * 2;
    int vw, splits, used;
    const int bm = bgemm_plan_wgrad(g, N, C, H, K, k, stride, parity_ok, &vw, &splits, &used);
    if (!ws || ws->part_floats < (size_t)splits * T * K * C) { mi_record_error("mi_bgemm_wgrad", "workspace too small"); return -3; }
    if (stride == 2 && vw > 1) { // x as parity planes: every tap becomes a unit-stride read
        if (!ws->s2d_valid && bg_s2d(st, x, (u16 *)ws->s2d, (long)N * C, H, H)) return -1;
        x = (const u16 *)ws->s2d;
    }
    mi_prof_begin(st, bgemm_fam(k), 2.0 * T * (double)N * g.P * C * K, 2.0 * ((double)N * C * g.HW + (double)N * g.P * K) + 4.0 * T * C * K);
    const int rc = bgemm_launch<BG_WGRAD>(st, dim3(g.tiles, used), dy, x, ws->part, nullptr, g, k, stride, bm, vw);
    if (rc) { mi_prof_end(st); return rc; }
    const int rr = mi_igemm_wgrad_reduce(st, ws->part, dw, K, C, k, used);
    mi_prof_end(st);
    if (rr) return rr;
    MI_LAUNCH_CHECK(bg_variant);
    return 0;
}

extern "C" {
int mid_bf16_supported(int op, int N, int C, int H, int K, int k, int stride) { return mi_bgemm_supported(op, N, C, H, K, k, stride); }
/* one layer's weights KCRS fp32 -> the bf16 k-step tiles of the forward pass [t][c/64][K][64] (what mid_conv_prelayout_all_bf16 makes for a table) */
int mid_bf16_prelayout_fwd(mid_stream s, const float *w, void *out, int K, int C, int k) { return bg_prelayout_one((hipStream_t)s, w, (u16 *)out, nullptr, K, C, k); }
/* ... and of the dgrad [t][k/64][C][64] */
int mid_bf16_prelayout_dgrad(mid_stream s, const float *w, void *out, int K, int C, int k) { return bg_prelayout_one((hipStream_t)s, w, nullptr, (u16 *)out, K, C, k); }
int mid_conv_prelayout_all_bf16(mid_stream s, const mid_wt_entry *entries_dev, const int *tile_entry_dev, int ntiles) {
    if (ntiles <= 0) return 0;
    hipLaunchKernelGGL(bg_wt_all_kernel, dim3(ntiles), dim3(256), 0, (hipStream_t)s, entries_dev, tile_entry_dev);
    MI_LAUNCH_CHECK("bg_wt_all_kernel");
    return 0;
}
int mid_conv_fwd_bf16(mid_stream s, mid_workspace *ws, const void *x, const float *w, void *y, int N, int C, int H, int K, int k,
                      int stride, mid_bn_parts *parts) {
    if (parts) parts->nparts = 0;
    if (!mi_bgemm_supported(BGOP_FWD, N, C, H, K, k, stride)) { mi_record_error("mid_conv_fwd_bf16", "shape not supported by the bf16 kernels"); return -2; }
    return mi_bgemm_fwd((hipStream_t)s, ws, (const u16 *)x, w, (u16 *)y, N, C, H, K, k, stride, parts);
}
int mid_conv_dgrad_bf16(mid_stream s, mid_workspace *ws, const float *w, const void *dy, void *dx, const void *addend, int N, int C,
                        int H, int K, int k, int stride) {
    if (!mi_bgemm_supported(BGOP_DGRAD, N, C, H, K, k, stride)) { mi_record_error("mid_conv_dgrad_bf16", "shape not supported by the bf16 kernels"); return -2; }
    return mi_bgemm_dgrad((hipStream_t)s, ws, w, (const u16 *)dy, (u16 *)dx, (const u16 *)addend, N, C, H, K, k, stride, nullptr);
}
int mid_conv_dgrad_bn_bf16(mid_stream s, mid_workspace *ws, const float *w, const void *dy, void *dx, const void *addend, int N, int C,
                           int H, int K, int k, int stride, mid_bn_bwd_parts *fz) {
    if (!mi_bgemm_supported(BGOP_DGRAD, N, C, H, K, k, stride)) { mi_record_error("mid_conv_dgrad_bn_bf16", "shape not supported by the bf16 kernels"); return -2; }
    return mi_bgemm_dgrad((hipStream_t)s, ws, w, (const u16 *)dy, (u16 *)dx, (const u16 *)addend, N, C, H, K, k, stride, fz);
}
/* mi_conv_plan for the NCHW route (resnet_mi.h): the planners of mi_bgemm_fwd / _dgrad / _wgrad with the operator's workspace (parity
 * planes for a stride-2 input).  0 where the route refuses the shape */
int mid_bf16_conv_plan(int op, int N, int C, int H, int K, int k, int stride, int out[7]) {
    if (!mi_bgemm_supported(op, N, C, H, K, k, stride)) return 0;
    BgArgs g = {};
    if (op == BGOP_WGRAD) {
        int vw, splits, used;
        out[0] = bgemm_plan_wgrad(g, N, C, H, K, k, stride, stride == 2, &vw, &splits, &used);
        out[1] = 128; out[2] = g.tiles; out[3] = g.tiles; out[4] = 1; out[5] = used; out[6] = mid_wgrad_reduce_grouped(K, C, used);
        return 1;
    }
    bgemm_geometry(g, N, C, H, K, stride);
    out[0] = bgemm_plan_tiles(g, op == BGOP_FWD ? K : C, bgemm_stage_vw());
    out[1] = 128; out[2] = g.tiles; out[3] = g.tiles; out[4] = 1; out[5] = 1; out[6] = 0;
    return 1;
}
int mid_f32_to_bf16(mid_stream s, const float *in, void *out, size_t n) {
    size_t b = (n + 255) / 256; if (b > 65536) b = 65536; if (b < 1) b = 1;
    hipLaunchKernelGGL(bg_f2b_kernel, dim3((unsigned)b), dim3(256), 0, (hipStream_t)s, in, (u16 *)out, n);
    MI_LAUNCH_CHECK("bg_f2b_kernel");
    return 0;
}
int mid_bf16_to_f32(mid_stream s, const void *in, float *out, size_t n) {
    size_t b = (n + 255) / 256; if (b > 65536) b = 65536; if (b < 1) b = 1;
    hipLaunchKernelGGL(bg_b2f_kernel, dim3((unsigned)b), dim3(256), 0, (hipStream_t)s, (const u16 *)in, out, n);
    MI_LAUNCH_CHECK("bg_b2f_kernel");
    return 0;
}
}
