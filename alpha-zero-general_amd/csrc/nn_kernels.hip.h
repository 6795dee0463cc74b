// nn_kernels.hip.h -- the shared device helpers of the policy/value net kernels for gfx950, and the one-launch V80 forward on f32 /
// bf16 x 3 operands.
//
// The reference evaluates the net with ONNX Runtime / torch on the CPU, one leaf at a time or 8 at a time
// (GenericNNetWrapper.py:94-157).  Here one lock-step round evaluates T leaves at once, every net in one launch: the kernels of the other
// nn_*.hip.h headers include this one for
//   nn_tid, the bf16 x 3 split helpers and the plane layout (split3*, store_split4 / load_split4), nn_wave_max / nn_wave_sum,
//   act_apply / act_apply2 / hardsigmoid and the f32 MFMA fragment order (FRAG).
// The V80 network (splendor/SplendorNNet.py:262-283,397-440) is a chain of *skinny* GEMMs (M = 7*T rows, K,N in {56,168,392,81}) plus
// per-(sample,channel) glue; v80_block_body runs one InvertedResidual1d block of it on a 16-sample tile held in LDS, and
//   k_v80_net      first layer + trunk block + both head blocks and tails, MFMA v_mfma_f32_16x16x4_f32 throughout (exact f32)
//   k_v80_net_spx  the same with the tile the blocks read kept as three bf16 planes and the expand GEMMs on bf16 x 3 operands
// are the full-range forms of the forward (include/azg.h, "Activation range"); the default f16 x 2 form is nn_v80_h2.hip.h.
#pragma once
// the non-template kernels of this header get internal linkage in a translation unit that only wants its device helpers (azg_async.hip)
#ifndef AZG_NN_KERNEL
#define AZG_NN_KERNEL
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

// The net has a tolerance contract (|pi|,|v| within 1e-5 of the reference's fp32 outputs), not a bit-exact one: FMA
// contraction is allowed in this header (the MCTS / env code keeps -ffp-contract=off).
#pragma clang fp contract(fast)

namespace azg {

// The thread index as the net kernels' helper functions see it.  In the translation unit of the pipeline's PERSISTENT net kernel
// (azg_async.hip defines AZG_NN_OPAQUE_TID) it is laundered through an empty asm at every use: the forward runs inside one long loop there,
// everything derived from the raw threadIdx.x is loop-invariant, and the compiler hoisted ~50 per-lane operand addresses of the Santorini
// forward to the kernel's entry and SPILLED them (k_async_net<NetC5>: 196 B of scratch, one scratch reload per basic block of the
// forward, each waiting with vmcnt(0) behind the weight prefetch; the stand-alone kernel has no scratch).  Opaque, they are recomputed
// where they are used -- a handful of VALU instructions per helper call.
__device__ __forceinline__ int nn_tid() {
#ifdef AZG_NN_OPAQUE_TID
    int t = (int)threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
#else
    return (int)threadIdx.x;
#endif
}


typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));     // v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 operands

// wave-wide f32 max / sum through DPP butterflies (rows of 16) + four readlanes; every lane gets the result
// ---- split-precision operand helpers (bf16 x 3, see nn_conv5x5.hip.h) ----
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ uint32_t bf16_rn(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ void split3(float x, uint32_t& h, uint32_t& m, uint32_t& l) {
    h = bf16_rn(x);
    float r = x - __uint_as_float(h << 16);
    m = bf16_rn(r);
    r = r - __uint_as_float(m << 16);
    l = bf16_rn(r);
}
// two values at once on the hardware converter (v_cvt_pk_bf16_f32, round to nearest even like bf16_rn): word = bf16(a) | bf16(b) << 16
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t bf16_pk(float a, float b) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2_t));
}
__device__ __forceinline__ void split3x2(float a, float b, uint32_t& h, uint32_t& m, uint32_t& l) {
    h = bf16_pk(a, b);
    a -= __uint_as_float(h << 16); b -= __uint_as_float(h & 0xFFFF0000u);
    m = bf16_pk(a, b);
    a -= __uint_as_float(m << 16); b -= __uint_as_float(m & 0xFFFF0000u);
    l = bf16_pk(a, b);
}
// byte offset of (row, 16-byte chunk q) inside one plane
__device__ __forceinline__ int pl_off(int row, int q) { return row * 128 + ((q ^ (row & 7)) << 4); }
// four consecutive channels (ch0 % 4 == 0) of one cell -> the three planes
__device__ __forceinline__ void store_split4(uint8_t* planes, int plane_bytes, int row, int ch0, float4 o) {
    uint32_t h[2], m[2], l[2];
    split3x2(o.x, o.y, h[0], m[0], l[0]); split3x2(o.z, o.w, h[1], m[1], l[1]);
    uint8_t* dst = planes + pl_off(row, ch0 >> 3) + ((ch0 & 4) << 1);
    *(uint2*)dst = make_uint2(h[0], h[1]);
    *(uint2*)(dst + plane_bytes) = make_uint2(m[0], m[1]);
    *(uint2*)(dst + 2 * plane_bytes) = make_uint2(l[0], l[1]);
}
__device__ __forceinline__ float bf16_lo_f32(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi_f32(uint32_t w) { return __uint_as_float(w & 0xFFFF0000u); }
__device__ __forceinline__ float4 load_split4(const uint8_t* planes, int plane_bytes, int row, int ch0) {
    const uint8_t* src = planes + pl_off(row, ch0 >> 3) + ((ch0 & 4) << 1);
    const uint2 h = *(const uint2*)src, m = *(const uint2*)(src + plane_bytes), l = *(const uint2*)(src + 2 * plane_bytes);
    return make_float4((bf16_lo_f32(h.x) + bf16_lo_f32(m.x)) + bf16_lo_f32(l.x), (bf16_hi_f32(h.x) + bf16_hi_f32(m.x)) + bf16_hi_f32(l.x),
                       (bf16_lo_f32(h.y) + bf16_lo_f32(m.y)) + bf16_lo_f32(l.y), (bf16_hi_f32(h.y) + bf16_hi_f32(m.y)) + bf16_hi_f32(l.y));
}


__device__ __forceinline__ float nn_wave_max(float x) {
    x = fmaxf(x, __uint_as_float(dpp_u32<0xB1>(__float_as_uint(x)))); x = fmaxf(x, __uint_as_float(dpp_u32<0x4E>(__float_as_uint(x))));
    x = fmaxf(x, __uint_as_float(dpp_u32<0x141>(__float_as_uint(x)))); x = fmaxf(x, __uint_as_float(dpp_u32<0x140>(__float_as_uint(x))));
    const float a = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), 0)), b = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), 16));
    const float c = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), 32)), d = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), 48));
    return fmaxf(fmaxf(a, b), fmaxf(c, d));
}
__device__ __forceinline__ float nn_wave_sum(float x) {
    x += __uint_as_float(dpp_u32<0xB1>(__float_as_uint(x))); x += __uint_as_float(dpp_u32<0x4E>(__float_as_uint(x)));
    x += __uint_as_float(dpp_u32<0x141>(__float_as_uint(x))); x += __uint_as_float(dpp_u32<0x140>(__float_as_uint(x)));
    const float a = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), 0)), b = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), 16));
    const float c = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), 32)), d = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), 48));
    return (a + b) + (c + d);
}

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_HSWISH = 2, ACT_HSIGMOID = 3 };

__device__ __forceinline__ float act_apply(float x, int act) {
    if (act == ACT_RELU) return x > 0.f ? x : 0.f;
    if (act == ACT_HSWISH) { float t = fminf(fmaxf(x + 3.f, 0.f), 6.f); return x * t * (1.f / 6.f); }
    if (act == ACT_HSIGMOID) return fminf(fmaxf(x + 3.f, 0.f), 6.f) * (1.f / 6.f);
    return x;
}
// activation of two packed values
__device__ __forceinline__ f32x2 act_apply2(f32x2 x, int act) {
    if (act == ACT_RELU) return f32x2{fmaxf(x.x, 0.f), fmaxf(x.y, 0.f)};
    if (act == ACT_HSWISH || act == ACT_HSIGMOID) {
        // relu6(x + 3) / 6 == clamp(x / 6 + 1 / 2, 0, 1): ONE packed FMA with the CLAMP output modifier (round 4; was a packed add, a
        // v_med3_f32 per component and a packed multiply by 1 / 6).  The compiler does not fold a clamp into v_pk_fma_f32: inline asm.
        f32x2 t;
        const f32x2 k = f32x2{1.f / 6.f, 1.f / 6.f};
        asm("v_pk_fma_f32 %0, %1, %2, 0.5 op_sel_hi:[1,0,0] clamp" : "=v"(t) : "v"(x), "s"(k));
        return act == ACT_HSWISH ? x * t : t;
    }
    return x;
}
__device__ __forceinline__ float hardsigmoid(float x) { return fminf(fmaxf(x + 3.f, 0.f), 6.f) * (1.f / 6.f); }

// ---------------------------------------------------------------------------------------------------------------------
// Fused InvertedResidual1d block (SplendorNNet.py:189-202 with :148-187), one workgroup = 16 samples = 112 token rows:
//   x[112][C=56] --expand GEMM+BN+act--> h[112][E=168] --depthwise Linear(7->7)+BN+act, SE squeeze--> pooled[16][E]
//   --SE fc1+ReLU--> [16][Q=40] --SE fc2+Hardsigmoid--> sc[16][E];   out = (h * sc) @ Wp + BN + x      (project + residual)
// The expanded activations (19 MB per block at T = 4096) never leave the CU: they live in LDS between the phases, and so do
// the block's input and output tiles (a launch per layer would move ~115 MB of HBM traffic per block).
// All four GEMMs use MFMA f32 16x16x4 with the WEIGHTS as the A operand held in registers (prefetched from L2 at kernel
// start, overlapping the x load) and the activations as the B operand read as float4 from LDS; 12 waves per workgroup:
//   expand   11 column tiles x 7 row tiles      wave w < 11 owns column tile w
//   SE fc1   3 column tiles x 1 row tile         waves 0..2
//   SE fc2   11 column tiles x 1 row tile        waves 0..10
//   project  4 column tiles x 7 row tiles        wave w owns column tile w&3 and row tiles {w>>2, (w>>2)+3, (w>>2)+6}
// Hard-wired to the V80 geometry C = 56, E = 168, Q = 40; the zero-padded weights We[64][176], W1[176][48], W2[48][176],
// Wp[176][64] are passed in MFMA fragment order (FRAG above).
struct V80BlockW {
    const float *We, *be, *Wd, *sd, *bd, *W1, *b1, *W2, *b2, *Wp, *bp;     // be/b1/b2/bp zero-padded to the padded widths
};
// What the whole-net fusion hangs onto the three blocks (v80_block_body MODE 1..3):
//   MODE 1 (trunk):       boards int8 [B][56][7] -> f32 tile (layout change in LDS) -> first_layer Linear(56,56)+BN
//                         (SplendorNNet.py:397-401) -> block -> output tile in LDS
//   MODE 2 (policy head): block -> Flatten -> Linear(392,81)+ReLU -> Linear(81,81) -> masked softmax -> pi in HBM
//   MODE 3 (value head):  block -> Flatten -> Linear(392,P)+ReLU -> Linear(P,P) -> tanh -> v in HBM   (:414-440)
// The block output tile stays in LDS (in place of x, row stride 60), so the flatten index of the head weights is
// k = l*60 + c (rows with c >= 56 are zero): Wh1 is [432][96] (policy) / [432][16] (value), zero padded.
struct V80NetW {
    const float *W0, *b0;                  // first layer [64][64], [64]
    const float *Wh1, *bh1, *Wh2, *bh2;    // policy: [432][96], [96], [96][96], [96];  value: [432][16], [16], [P][P], [P]
                                           // (W0, Wh1 and the policy Wh2 in fragment order; the value Wh2 is plain)
};

// weight operands are stored in MFMA fragment order: frag[tile nt][K chunk c][lane][j] = W[16c + 4*(lane>>4) + j][16nt + (lane&15)],
// so a wave fetches one chunk of one column tile as a single 1 KiB global_load_dwordx4.  Where K = 8 mod 16 (56, 168) the
// last chunk is stored "half": frag[nt][c_last][lane][j] = W[16c + 2*(lane>>4) + j] for j < 2 (j >= 2 unused), so that
// chunk costs two MFMAs instead of four
#define FRAG(ptr, NCH, nt, c) (*(const float4*)((ptr) + ((((size_t)(nt) * (NCH) + (c)) * 64 + lane) << 2)))

#ifdef AZG_NN_PHASE_TIMES
static __device__ long long g_v80_phase[4][16];
#define AZG_PH(k) do { if (blockIdx.x == 7 && threadIdx.x == 0) g_v80_phase[MODE][k] = clock64(); } while (0)
#else
#define AZG_PH(k)
#endif

// The block (+ optional first layer in front, + optional head tail behind) on one 16-sample tile.  X = the tile's [112][60]
// f32 buffer in LDS, H = the rest of the workgroup's LDS ([112][172] + 2 x [16][172] + [16][52] + 64 floats).
//   INLDS:  the input tile is already in X (the head MODEs; MODE 1 builds it from the boards)
//   OUTLDS: the block output replaces X in place (MODE 1 sets it, the head MODEs always do: nothing but boards, valid, pi and v
//           crosses HBM); SAVE: and is copied to xsave
//   SPX:    the input tile lives in LDS as three bf16 planes [112][64] (hi + mid + lo, the layout of nn_conv5x5.hip.h) instead of
//           the f32 [112][60] tile, written split once by the producing epilogue, and the expand GEMM runs on bf16 x 3 operands (six
//           v_mfma_f32_16x16x32_bf16 per product; W.We = [11 tiles][2 K chunks of 32][3 planes][64 lanes][8] bf16).  The trunk block
//           rewrites the planes in place; the head blocks leave them alone (the value head reuses the trunk output) and put their
//           f32 output O [112][60] over the dead pooled / SE-hidden buffers for the head tail.
template <int ACT, int POOLMAX, int MODE, bool INLDS, bool OUTLDS, bool SAVE, bool SPX = false>
__device__ __forceinline__ void v80_block_body(float* X, float* H, float* xsave, const V80BlockW& W, int B,
                                               const int8_t* __restrict__ boards, const V80NetW& N,
                                               const uint8_t* __restrict__ valid, float* __restrict__ pi_out,
                                               float* __restrict__ v_out, int P) {
    constexpr int C = 56, E = 168, NS = 16, ROWS = NS * 7, XS = 60, HS = 172, QS = 52, FK = 7 * XS /* 420 */, A = 81;
    static_assert(MODE == 1 ? !INLDS && OUTLDS : (MODE == 2 || MODE == 3) && INLDS, "the tile stays in LDS from the boards to pi / v");
    static_assert(!SPX || !SAVE, "SPX: one copy of the trunk output serves both heads");
    // (SPX: SC first, so that pooled + SE hidden + depthwise weights + 12 KB behind them form the 26.9 KB of the head blocks' output tile)
    float* SC = SPX ? H + ROWS * HS : H + ROWS * HS + NS * HS;          // scales [NS][HS]
    float* PL = SPX ? SC + NS * HS : H + ROWS * HS;                     // pooled [NS][HS]
    float* SH = SPX ? PL + NS * HS : SC + NS * HS;                      // SE hidden [NS][QS]
    float* WD = SH + NS * QS;           // [49]
    float* OT = PL;                     // SPX, head blocks: the block output O [ROWS][XS] f32 (PL, SH, WD are dead by the project phase)
    uint8_t* XPL = (uint8_t*)X;         // SPX: the three planes
    constexpr int PB = ROWS * 128;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, r16 = lane & 15;
    const int b0 = blockIdx.x * NS;
    const int nt_p = wave & 3;
    AZG_PH(0);

    float4 we[4], w2r[3], w1r[11], wpr[11];
    uint4 weS[6];                       // SPX: [K chunk][plane] fragments of the wave's expand tile
    const int nt_e = wave < 11 ? wave : 0, nt_1 = wave < 3 ? wave : 0;
    auto load_we = [&]() {
        if (SPX) {
#pragma unroll
            for (int k = 0; k < 6; k++) weS[k] = ((const uint4*)W.We)[((size_t)nt_e * 6 + k) * 64 + lane];
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++) we[c] = FRAG(W.We, 4, nt_e, c);
        }
    };
    auto load_w2_wp = [&]() {
#pragma unroll
        for (int c = 0; c < 3; c++) w2r[c] = FRAG(W.W2, 3, nt_e, c);
#pragma unroll
        for (int c = 0; c < 11; c++) wpr[c] = FRAG(W.Wp, 11, nt_p, c);
    };
    if (MODE == 1) {
        // ---- P0': board tile (int8, [s][c][l]) -> X0[s*7+l][c] f32 (aliases H), then first layer -> X ----
        float* X0 = H;
        const int nb = min(NS, B - b0);
        const uint32_t* bsrc = (const uint32_t*)(boards + (size_t)b0 * (7 * C));
        uint32_t bv[3];                                   // the board tile is requested before any weight
#pragma unroll
        for (int k = 0; k < 3; k++) { const int i = tid + 768 * k; bv[k] = (i < NS * (7 * C / 4) && i / (7 * C / 4) < nb) ? bsrc[i] : 0u; }
        float4 w0r[4];
#pragma unroll
        for (int c = 0; c < 4; c++) w0r[c] = FRAG(N.W0, 4, nt_p, c);
        const float4 b04 = *(const float4*)(N.b0 + nt_p * 16 + 4 * g);
        load_we();                                        // block weights stream in behind the first layer
        load_w2_wp();
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int i = tid + 768 * k;
            if (i < NS * (7 * C / 4)) {
                const int s = i / (7 * C / 4), d = i - s * (7 * C / 4);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int idx = 4 * d + q, c = idx / 7, l = idx - c * 7;
                    X0[(s * 7 + l) * XS + c] = (float)(int8_t)(bv[k] >> (8 * q));
                }
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int rt = wave >> 2; rt < 7; rt += 3) {
            const float* xr = X0 + (rt * 16 + r16) * XS + 4 * g;
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float4 a = *(const float4*)(xr + 16 * c);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w0r[c].x, a.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w0r[c].y, a.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w0r[c].z, a.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w0r[c].w, a.w, acc, 0, 0, 0);
            }
            {   // half chunk k = 48..55 (FRAG_HALF order: lane group g holds k = 48 + 2g + {0,1})
                const f32x2 a = *(const f32x2*)(xr + 48 - 2 * g);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w0r[3].x, a.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w0r[3].y, a.y, acc, 0, 0, 0);
            }
            const int col0 = nt_p * 16 + 4 * g;
            if (SPX)                  // all 64 columns of the planes (56..63 get 0: zero-padded W0 / b0)
                store_split4(XPL, PB, rt * 16 + r16, col0, make_float4(acc[0] + b04.x, acc[1] + b04.y, acc[2] + b04.z, acc[3] + b04.w));
            else if (col0 < XS)       // columns 56..59 get 0 (zero-padded W0 / b0)
                *(float4*)(X + (rt * 16 + r16) * XS + col0) =
                    make_float4(acc[0] + b04.x, acc[1] + b04.y, acc[2] + b04.z, acc[3] + b04.w);
        }
        __syncthreads();
    }

    AZG_PH(1);
    // ---- the weight fragments (L2) are requested in the order the phases need them: the vmcnt counter retires in order,
    //      so P1 only waits for what it uses while the rest keeps streaming in ----
    if (MODE != 1) load_we();
    const float4 be4 = *(const float4*)(W.be + nt_e * 16 + 4 * g);
    const float wd_stage = tid < 49 ? W.Wd[tid] : 0.f;       // requested now, parked in LDS after the expand phase (used by P2)
    if (MODE != 1) load_w2_wp();
    const float4 b14 = *(const float4*)(W.b1 + nt_1 * 16 + 4 * g);
    const float4 b24 = *(const float4*)(W.b2 + nt_e * 16 + 4 * g);
    const float4 bp4 = *(const float4*)(W.bp + nt_p * 16 + 4 * g);
    __syncthreads();
    AZG_PH(2);

    // ---- P1: expand + BN + act -> H ----
    if (wave < 11) {
#pragma unroll 1
        for (int rt = 0; rt < 7; rt++) {
            const float* xr = X + (rt * 16 + r16) * XS + 4 * g;
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            if (SPX) {
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    const uint8_t* src = XPL + pl_off(rt * 16 + r16, 4 * c + g);
                    const bf16x8 ah = __builtin_bit_cast(bf16x8, *(const uint4*)src), am = __builtin_bit_cast(bf16x8, *(const uint4*)(src + PB)),
                                 al = __builtin_bit_cast(bf16x8, *(const uint4*)(src + 2 * PB));
                    const bf16x8 wh = __builtin_bit_cast(bf16x8, weS[3 * c]), wm = __builtin_bit_cast(bf16x8, weS[3 * c + 1]),
                                 wl = __builtin_bit_cast(bf16x8, weS[3 * c + 2]);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, ah, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, al, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wm, am, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wm, ah, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, am, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, ah, acc, 0, 0, 0);
                }
            } else {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float4 a = *(const float4*)(xr + 16 * c);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(we[c].x, a.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(we[c].y, a.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(we[c].z, a.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(we[c].w, a.w, acc, 0, 0, 0);
            }
            {   // half chunk k = 48..55
                const f32x2 a = *(const f32x2*)(xr + 48 - 2 * g);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(we[3].x, a.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(we[3].y, a.y, acc, 0, 0, 0);
            }
            }
            const int col0 = nt_e * 16 + 4 * g;
            if (col0 < E) {
                const f32x2 lo = act_apply2(f32x2{acc[0] + be4.x, acc[1] + be4.y}, ACT);
                const f32x2 hi = act_apply2(f32x2{acc[2] + be4.z, acc[3] + be4.w}, ACT);
                *(float4*)(H + (rt * 16 + r16) * HS + col0) = make_float4(lo.x, lo.y, hi.x, hi.y);
            }
        }
    }
    if (tid < 49) WD[tid] = wd_stage;
    __syncthreads();
    AZG_PH(3);
    if (wave < 3) {                    // SE fc1 weights: requested now (the expand fragments are dead), they land during P2
#pragma unroll
        for (int c = 0; c < 11; c++) w1r[c] = FRAG(W.W1, 11, nt_1, c);
    }

    // ---- P2: depthwise Linear(7->7) over the token axis + BN + act (in place) + SE squeeze ----
    float wd[49];                      // wave-uniform 7x7 weights -> SGPRs (one LDS broadcast read each, once per wave)
#pragma unroll
    for (int k = 0; k < 49; k++) wd[k] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, WD[k])));
    // two adjacent channels per thread as one f32x2: the 49 multiply-adds of the token mix run as v_pk_fma_f32
    for (int i = tid; i < NS * (E / 2); i += 768) {
        const int s = i / (E / 2), c = 2 * (i - s * (E / 2));
        float* base = H + (s * 7) * HS + c;
        f32x2 in[7];
#pragma unroll
        for (int l = 0; l < 7; l++) in[l] = *(const f32x2*)(base + l * HS);
        const f32x2 scl = *(const f32x2*)(W.sd + c), bb = *(const f32x2*)(W.bd + c);
        f32x2 pool = POOLMAX ? f32x2{-INFINITY, -INFINITY} : f32x2{0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 7; m++) {
            f32x2 a = f32x2{0.f, 0.f};
#pragma unroll
            for (int l = 0; l < 7; l++) a += wd[m * 7 + l] * in[l];
            a = act_apply2(a * scl + bb, ACT);
            *(f32x2*)(base + m * HS) = a;
            if (POOLMAX) { pool.x = fmaxf(pool.x, a.x); pool.y = fmaxf(pool.y, a.y); } else pool += a;
        }
        if (!POOLMAX) pool = pool * (1.f / 7.f);
        *(f32x2*)(PL + s * HS + c) = pool;
    }
    __syncthreads();
    AZG_PH(4);

    // ---- P3: SE fc1 + ReLU : SH[16][48] = relu(PL[16][168] @ W1 + b1) ----
    if (wave < 3) {
        const float* pr = PL + r16 * HS + 4 * g;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 10; c++) {
            const float4 a = *(const float4*)(pr + 16 * c);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1r[c].x, a.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1r[c].y, a.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1r[c].z, a.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1r[c].w, a.w, acc, 0, 0, 0);
        }
        {   // half chunk k = 160..167
            const f32x2 a = *(const f32x2*)(pr + 160 - 2 * g);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1r[10].x, a.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1r[10].y, a.y, acc, 0, 0, 0);
        }
        float4 v;
        v.x = fmaxf(acc[0] + b14.x, 0.f); v.y = fmaxf(acc[1] + b14.y, 0.f);
        v.z = fmaxf(acc[2] + b14.z, 0.f); v.w = fmaxf(acc[3] + b14.w, 0.f);
        *(float4*)(SH + r16 * QS + nt_1 * 16 + 4 * g) = v;
    }
    __syncthreads();
    AZG_PH(5);

    // ---- P4: SE fc2 + Hardsigmoid : SC[16][168] ----
    if (wave < 11) {
        const float* hr = SH + r16 * QS + 4 * g;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float4 a = *(const float4*)(hr + 16 * c);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w2r[c].x, a.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w2r[c].y, a.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w2r[c].z, a.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w2r[c].w, a.w, acc, 0, 0, 0);
        }
        const int col0 = nt_e * 16 + 4 * g;
        if (col0 < E) {
            float4 v;
            v.x = hardsigmoid(acc[0] + b24.x); v.y = hardsigmoid(acc[1] + b24.y);
            v.z = hardsigmoid(acc[2] + b24.z); v.w = hardsigmoid(acc[3] + b24.w);
            *(float4*)(SC + r16 * HS + col0) = v;
        }
    }
    __syncthreads();
    AZG_PH(6);

    // policy head: the first Linear's weight fragments stream in from L2 while P5 runs (we / w1r / w2r are dead by now)
    float4 wr[14], w2h[6];
    const int ht_nt = wave % 6, ht_half = wave / 6;
    const int ht_beg = ht_half * 14, ht_n = ht_half ? 13 : 14;          // 27 K chunks of 16 (432 >= 420)
    if (MODE == 2) {
#pragma unroll
        for (int cc = 0; cc < 14; cc++) wr[cc] = cc < ht_n ? FRAG(N.Wh1, 27, ht_nt, ht_beg + cc) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (wave < 6) {
#pragma unroll
            for (int c = 0; c < 6; c++) w2h[c] = FRAG(N.Wh2, 6, wave, c);
        }
    }

    // ---- P5: project (SE-scaled operand) + BN + residual -> in place of x in LDS ----
#pragma unroll 1
    for (int rt = wave >> 2; rt < 7; rt += 3) {
        const int row = rt * 16 + r16;
        const float* hr = H + row * HS + 4 * g;
        const float* sr = SC + (row / 7) * HS + 4 * g;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 10; c++) {
            float4 a = *(const float4*)(hr + 16 * c);
            const float4 s4 = *(const float4*)(sr + 16 * c);
            a.x *= s4.x; a.y *= s4.y; a.z *= s4.z; a.w *= s4.w;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wpr[c].x, a.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wpr[c].y, a.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wpr[c].z, a.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wpr[c].w, a.w, acc, 0, 0, 0);
        }
        {   // half chunk k = 160..167
            const f32x2 a = *(const f32x2*)(hr + 160 - 2 * g) * *(const f32x2*)(sr + 160 - 2 * g);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wpr[10].x, a.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wpr[10].y, a.y, acc, 0, 0, 0);
        }
        const int col0 = nt_p * 16 + 4 * g;
        if (SPX) {
            const float4 xr = load_split4(XPL, PB, row, col0);       // (columns 56..63 of the planes are zero)
            const float4 o4 = make_float4(acc[0] + bp4.x + xr.x, acc[1] + bp4.y + xr.y, acc[2] + bp4.z + xr.z, acc[3] + bp4.w + xr.w);
            if (MODE == 1) store_split4(XPL, PB, row, col0, o4);     // trunk: in place, a lane rewrites the elements it read
            else if (col0 < XS) *(float4*)(OT + row * XS + col0) = o4;
        } else {
            if (col0 < XS) {          // each element is read (residual) and overwritten by the same lane
                float* xp = X + row * XS + col0;
                const float4 xr = *(const float4*)xp;
                const float4 o4 = make_float4(acc[0] + bp4.x + xr.x, acc[1] + bp4.y + xr.y, acc[2] + bp4.z + xr.z,
                                              acc[3] + bp4.w + xr.w);
                *(float4*)xp = o4;
                if (SAVE) *(float4*)(xsave + row * XS + col0) = o4;
            }
        }
    }

    AZG_PH(7);
    if (MODE == 2) {
        // ---- policy head tail on the block output O = X viewed as [16][420] ----
        constexpr int LS = 100;
        float* RED = H;                      // [2][16][LS]   K-halves of the first Linear
        float* HID = RED + 2 * 16 * LS;      // [16][LS]
        float* LG = HID + 16 * LS;           // [16][LS]
        const int nt = ht_nt, half = ht_half, c_beg = ht_beg, n_c = ht_n;
        __syncthreads();                     // O complete, H free
        AZG_PH(8);
        {
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int cc = 0; cc < 14; cc++) {
                const int k0 = 16 * (c_beg + cc) + 4 * g;
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                if (cc < n_c && k0 < FK) a = *(const float4*)((SPX ? OT : X) + r16 * FK + k0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[cc].x, a.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[cc].y, a.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[cc].z, a.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[cc].w, a.w, acc, 0, 0, 0);
            }
            *(float4*)(RED + (half * 16 + r16) * LS + nt * 16 + 4 * g) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        }
        __syncthreads();
        if (tid < 16 * 24) {
            const int s = tid / 24, col = 4 * (tid - s * 24);
            const float4 p0 = *(const float4*)(RED + s * LS + col), p1 = *(const float4*)(RED + (16 + s) * LS + col);
            const float4 bb = *(const float4*)(N.bh1 + col);
            *(float4*)(HID + s * LS + col) = make_float4(fmaxf(p0.x + p1.x + bb.x, 0.f), fmaxf(p0.y + p1.y + bb.y, 0.f),
                                                         fmaxf(p0.z + p1.z + bb.z, 0.f), fmaxf(p0.w + p1.w + bb.w, 0.f));
        }
        __syncthreads();
        if (wave < 6) {
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 6; c++) {
                const float4 a = *(const float4*)(HID + r16 * LS + 16 * c + 4 * g);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w2h[c].x, a.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w2h[c].y, a.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w2h[c].z, a.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w2h[c].w, a.w, acc, 0, 0, 0);
            }
            const float4 bb = *(const float4*)(N.bh2 + wave * 16 + 4 * g);
            *(float4*)(LG + r16 * LS + wave * 16 + 4 * g) =
                make_float4(acc[0] + bb.x, acc[1] + bb.y, acc[2] + bb.z, acc[3] + bb.w);
        }
        __syncthreads();
        AZG_PH(9);
        // masked softmax == exp(log_softmax(where(valid, logits, -1e8))) (GenericNNetWrapper.py:105-107), one wave per sample
        for (int s = wave; s < NS; s += 12) {
            const int b = b0 + s;
            if (b >= B) continue;
            const int a1 = lane + 64;
            float x0 = valid[(size_t)b * A + lane] ? LG[s * LS + lane] : -1e8f;
            float x1 = a1 < A ? (valid[(size_t)b * A + a1] ? LG[s * LS + a1] : -1e8f) : -INFINITY;
            const float mx = nn_wave_max(fmaxf(x0, x1));
            x0 = expf(x0 - mx);
            x1 = a1 < A ? expf(x1 - mx) : 0.f;
            const float sum = nn_wave_sum(x0 + x1);
            pi_out[(size_t)b * A + lane] = x0 / sum;
            if (a1 < A) pi_out[(size_t)b * A + a1] = x1 / sum;
        }
        AZG_PH(10);
    }

    if (MODE == 3) {
        // ---- value head tail: Linear(392,P) -> ReLU -> Linear(P,P) -> tanh ----
        float* RED = H;                      // [12][16][16]
        __syncthreads();
        {
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int cc = 0; cc < 3; cc++) {
                const int c = wave + 12 * cc;
                const int k0 = 16 * c + 4 * g;
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c < 27) {
                    w4 = FRAG(N.Wh1, 27, 0, c);
                    if (k0 < FK) a = *(const float4*)((SPX ? OT : X) + r16 * FK + k0);
                }
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.x, a.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.y, a.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.z, a.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.w, a.w, acc, 0, 0, 0);
            }
            *(float4*)(RED + (wave * 16 + r16) * 16 + 4 * g) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        }
        __syncthreads();
        if (tid < NS * P) {
            const int s = tid / P, p = tid - s * P, b = b0 + s;
            if (b < B) {
                float a = N.bh2[p];
                for (int j = 0; j < P; j++) {
                    float h = N.bh1[j];
                    for (int w = 0; w < 12; w++) h += RED[(w * 16 + s) * 16 + j];
                    a += fmaxf(h, 0.f) * N.Wh2[j * P + p];
                }
                v_out[(size_t)b * P + p] = tanhf(a);
            }
        }
    }
}

// dynamic LDS of the two kernels below (bytes).  V80_LDS = X [112][60] + H of v80_block_body; k_v80_net = + a second [112][60] tile;
// k_v80_net_spx = three bf16 planes [112][64] instead of X, + 12 KB behind H (the head blocks' output tile)
constexpr size_t V80_LDS = (size_t)(112 * 60 + 112 * 172 + 2 * 16 * 172 + 16 * 52 + 64) * sizeof(float);
constexpr size_t V80_NET_LDS = V80_LDS + (size_t)112 * 60 * sizeof(float);
constexpr size_t V80_SPX_LDS = (size_t)3 * 112 * 128 + (V80_LDS - (size_t)112 * 60 * sizeof(float)) + 12288;
static_assert(V80_LDS <= 160 * 1024 && V80_NET_LDS <= 160 * 1024 && V80_SPX_LDS <= 160 * 1024, "k_v80_*: LDS");

// The whole V80 forward of one 16-sample tile in ONE workgroup pass: first layer + trunk block (its output stays in LDS and
// is copied to a second tile buffer), policy head block + tail on the first copy, value head block + tail on the second.
// Nothing but the int8 boards, the valid masks and pi / v crosses HBM; LDS = 2 x [112][60] + the block's 129.5 KB = 156.4 KB.
AZG_NN_KERNEL __global__ __launch_bounds__(768) void k_v80_net(V80BlockW Wt, V80BlockW Wp, V80BlockW Wv, V80NetW N0, V80NetW Np, V80NetW Nv,
                                                 const int8_t* __restrict__ boards, const uint8_t* __restrict__ valid, int B,
                                                 int P, float* __restrict__ pi_out, float* __restrict__ v_out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* X = smem;
    float* XT = X + 112 * 60;
    float* H = XT + 112 * 60;
    v80_block_body<1, 0, 1, false, true, true>(X, H, XT, Wt, B, boards, N0, nullptr, nullptr, nullptr, P);
    __syncthreads();
    v80_block_body<2, 1, 2, true, false, false>(X, H, nullptr, Wp, B, nullptr, Np, valid, pi_out, nullptr, P);
    __syncthreads();
    v80_block_body<2, 1, 3, true, false, false>(XT, H, nullptr, Wv, B, nullptr, Nv, nullptr, nullptr, v_out, P);
}

// The same forward with the tile the three blocks read kept as bf16 planes and the expand GEMMs on bf16 x 3 operands (SPX above):
// LDS = 3 x [112][64] bf16 + the block's buffers + 12 KB = 154.3 KB; one copy of the trunk output serves both heads.
AZG_NN_KERNEL __global__ __launch_bounds__(768) void k_v80_net_spx(V80BlockW Wt, V80BlockW Wp, V80BlockW Wv, V80NetW N0, V80NetW Np, V80NetW Nv,
                                                     const int8_t* __restrict__ boards, const uint8_t* __restrict__ valid, int B,
                                                     int P, float* __restrict__ pi_out, float* __restrict__ v_out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* X = smem;                                  // three bf16 planes [112][64]
    float* H = X + 3 * 112 * 128 / 4;
    v80_block_body<1, 0, 1, false, true, false, true>(X, H, nullptr, Wt, B, boards, N0, nullptr, nullptr, nullptr, P);
    __syncthreads();
    v80_block_body<2, 1, 2, true, false, false, true>(X, H, nullptr, Wp, B, nullptr, Np, valid, pi_out, nullptr, P);
    __syncthreads();
    v80_block_body<2, 1, 3, true, false, false, true>(X, H, nullptr, Wv, B, nullptr, Nv, nullptr, nullptr, v_out, P);
}

}  // namespace azg

#pragma clang fp contract(off)
