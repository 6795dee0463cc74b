// nn_smallworld.hip.h -- the Smallworld transformer (smallworld/SmallworldNNet.py nn_version 62, :246-254, stem :86-137, heads :139-180,
// forward :268-294: InputStem over the (N, 8) int8 tokens -> 48, three post-norm nn.TransformerEncoderLayer (d_model 48, 3 heads of 16,
// feed-forward 192, ReLU, LayerNorm eps 1e-5, no mask), ActionSlicerHead (local 48 -> 5 on the nA area tokens, mean of the other tokens
// -> global 48 -> 16 and value 48 -> P), masked softmax over A = 5 nA + 16 actions, tanh) as ONE launch per leaf batch.
//
// Geometry (template on the player count P): N = 40 / 52 / 66 tokens, each sample's tokens padded to NT = 48 / 64 / 80 rows (3 / 4 / 5 MFMA
// row tiles, so a tile never straddles two samples); a workgroup owns NS = 4 / 3 / 2 samples = RT = 12 / 12 / 10 row tiles, sample-major
// (row = s * NT + token).  Twelve waves (768 threads), one workgroup per CU.
// Every per-token GEMM is out^T = W^T x act^T on v_mfma_f32_16x16x4_f32: the weights are the A operand (fragments streamed from global
// memory, L2-resident), the activations the B operand.  All GEMMs share ONE k order: in MFMA m of a chain the lane (i = lane & 15,
// g = lane >> 4) supplies k = 16 (m >> 2) + 4 g + (m & 3), which is exactly where the MFMA result puts output channel 16 t + 4 g + j
// (t = m >> 2, j = m & 3).  So an output held in VGPRs is the next GEMM's B operand without a trip through LDS, and a row read from LDS
// is three float4 per lane.
//   stem     (VALU) out_proj folded at pack time into three lookup tables and one 21 -> 48 projection: per token three gathers, 21 FMAs
//            per channel, LayerNorm (the row's 48 channels live in the four lanes i, i + 16, i + 32, i + 48: two xor shuffles)
//   pass 1   QKV = X W_in^T + b_in (the 1/4 attention scale folded into the Q rows, exact): items (row tile, Q|K|V), 3 x 12 MFMAs each
//   pass 2   one query tile per wave, fused end to end in VGPRs: per head S^T = K Q^T (4 MFMAs per 16-key tile), softmax over the keys on
//            the VALU (padding keys -inf), O^T = V^T P^T (the lane's probabilities are the B operand as they are, V read from LDS by
//            scalar reads), then out_proj (12 MFMAs per column tile) + bias + residual, LN1, the feed-forward in four chunks of 48
//            hidden channels (linear1 + ReLU: 3 x 12 MFMAs into VGPRs, then their 12 k-steps of linear2: 3 x 12 MFMAs), + bias +
//            residual, LN2, written back over the tile's X rows.  Pass 2
//            reads only the QKV buffer and its own rows of X, so the in-place write is safe.
//   heads    (VALU) local head per area token, mean of the non-area tokens, global + value heads, logits in the QKV buffer, masked
//            softmax one wave per sample
// LDS (static): X [RT * 16][52] f32 (the residual stream) + QKV [RT * 16][148] f32 + the pooled vectors [NS][48]: 150.8 / 150.6 / 125.4
// KB.  Two barriers per layer.
//
// Operand precision: f32 MFMA (exact products, f32 accumulation), not the f16 x 2 split operands of the Santorini / Splendor kernels.
// The per-token GEMMs have K = 48 (and 192 for linear2), the attention products K = 16 per head: the split form pads K to chunks of
// 32 and needs three MFMAs per product and a second operand format for every activation, the attention scores and probabilities
// included, for a bounded range.  f32 keeps the full range of the softmax inputs and the same 1e-5 contract as the torch net; the
// cost is a 4x higher MFMA floor.
#pragma once
#include "nn_kernels.hip.h"

namespace azg {

struct Sw62NetW {
    const float *Tppl, *Tpwr, *Tpl;   // folded stem tables [31][48], [41][48], [6][48] (embedding @ out_proj slice^T)
    const float *Wst, *bst;           // folded stem projection [21][48] (x0, x3..x6 / 10, then bits 0..7 of x3 and of x4), bias [48]
    const float *lnsw, *lnsb;         // stem LayerNorm [48], [48]
    const float *Wqkv, *bqkv;         // per layer [9 ct][12 m][64] fragments of in_proj^T (Q rows * 1/4), bias [L][144] (Q part * 1/4)
    const float *Wo, *bo;             // per layer [3][12][64] fragments of out_proj^T, bias [L][48]
    const float *ln1w, *ln1b;         // [L][48]
    const float *W1, *b1;             // per layer [12][12][64] fragments of linear1^T, bias [L][192]
    const float *W2, *b2;             // per layer [3][48][64] fragments of linear2^T, bias [L][48]
    const float *ln2w, *ln2b;         // [L][48]
    const float *Wl, *bl;             // local head [48][5], [5]
    const float *Wg, *bg;             // global head [48][16], [16]
    const float *Wv, *bv;             // value head [48][P], [P]
};
constexpr int SW_NW = 25;

constexpr int SW_D = 48, SW_LAYERS = 3, SW_XS = 52, SW_QS = 148, SW_THREADS = 768, SW_WAVES = SW_THREADS / 64;

template <int P> struct Sw62Geo;
template <> struct Sw62Geo<2> { static constexpr int N = 40, NA = 23, NS = 4; };
template <> struct Sw62Geo<3> { static constexpr int N = 52, NA = 30, NS = 3; };
template <> struct Sw62Geo<4> { static constexpr int N = 66, NA = 39, NS = 2; };

template <int P> struct Sw62 {
    static constexpr int N = Sw62Geo<P>::N, NA = Sw62Geo<P>::NA, NS = Sw62Geo<P>::NS, A = 5 * NA + 16;
    static constexpr int TPS = (N + 15) / 16, NT = TPS * 16, RT = NS * TPS, ROWS = RT * 16;
    static constexpr int LDS_FLOATS = ROWS * (SW_XS + SW_QS) + NS * SW_D;
    static_assert(LDS_FLOATS * sizeof(float) <= 160 * 1024, "k_sw62_net: LDS");
    static_assert(RT <= SW_WAVES, "k_sw62_net: one query tile per wave");
    static_assert(NS <= SW_WAVES && NS * A <= ROWS * SW_QS, "k_sw62_net: heads");
};

__device__ __forceinline__ f32x4 sw_mfma(float a, float b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0); }

// sum / max over the four lanes that hold one row (i, i + 16, i + 32, i + 48); every one of them gets the same bits
__device__ __forceinline__ float sw_row_sum(float x) {
    x += __shfl_xor(x, 16);
    return x + __shfl_xor(x, 32);
}
__device__ __forceinline__ float sw_row_max(float x) {
    x = fmaxf(x, __shfl_xor(x, 16));
    return fmaxf(x, __shfl_xor(x, 32));
}

// LayerNorm(48) of the row whose channels 16 t + 4 g + j the lane holds in x[4 t + j]
__device__ __forceinline__ void sw_layernorm(float (&x)[12], const float* __restrict__ w, const float* __restrict__ b, int g) {
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < 12; m++) s += x[m];
    const float mean = sw_row_sum(s) * (1.f / SW_D);
    float q = 0.f;
#pragma unroll
    for (int m = 0; m < 12; m++) q = fmaf(x[m] - mean, x[m] - mean, q);
    const float rs = 1.f / sqrtf(sw_row_sum(q) * (1.f / SW_D) + 1e-5f);
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const float4 ww = *(const float4*)(w + 16 * t + 4 * g), bb = *(const float4*)(b + 16 * t + 4 * g);
        x[4 * t + 0] = fmaf((x[4 * t + 0] - mean) * rs, ww.x, bb.x);
        x[4 * t + 1] = fmaf((x[4 * t + 1] - mean) * rs, ww.y, bb.y);
        x[4 * t + 2] = fmaf((x[4 * t + 2] - mean) * rs, ww.z, bb.z);
        x[4 * t + 3] = fmaf((x[4 * t + 3] - mean) * rs, ww.w, bb.w);
    }
}

// one output column tile: acc = sum over the KM MFMAs of fragment m (global, [KM][64]) x b[m]
template <int KM>
__device__ __forceinline__ f32x4 sw_gemm_tile(const float* __restrict__ wf, const float (&b)[KM], int lane,
                                              f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f}) {
#pragma unroll
    for (int m = 0; m < KM; m++) acc = sw_mfma(wf[m * 64 + lane], b[m], acc);
    return acc;
}

__device__ __forceinline__ void sw_load_row(const float* __restrict__ r, int g, float (&a)[12]) {   // channels 16 t + 4 g + j of an LDS row
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const float4 q = *(const float4*)(r + 16 * t + 4 * g);
        a[4 * t] = q.x, a[4 * t + 1] = q.y, a[4 * t + 2] = q.z, a[4 * t + 3] = q.w;
    }
}
__device__ __forceinline__ void sw_store_row(float* __restrict__ r, int g, const float (&a)[12]) {
#pragma unroll
    for (int t = 0; t < 3; t++) *(float4*)(r + 16 * t + 4 * g) = make_float4(a[4 * t], a[4 * t + 1], a[4 * t + 2], a[4 * t + 3]);
}

// The forward of one workgroup (samples NS * wg ..) as a device function: the body of k_sw62_net and -- ASYNC -- of the asynchronous
// pipeline's net kernel (azg_async.hip.h NetSw62): sample s of the workgroup is then tree sidx[s] (LDS; < 0 = no sample, computed on zero
// tokens like a padding sample and not written), `boards` / `valid` are both the pipeline's leaf-record array (kernels.hip.h AsyncLeaf<G>:
// int8 state [SP] = the [N][8] tokens + valid bit mask u64[AW] at AL_MASK, stride AL_STRIDE), read past the L1; the samples' masks are
// fetched into `smask` (LDS u64 [NS][AW]); pi / v rows are written WRITE-THROUGH at the tree's index.  The weight table is read through
// the CONSTANT address space (the kernel's own argument segment / the pipeline's argument block).
typedef const Sw62NetW __attribute__((address_space(4))) * Sw62NetWC;
#define W (*Wp)
template <int P, bool ASYNC, int AL_STRIDE = 0, int AL_MASK = 0>
__device__ __forceinline__ void sw62_net_body(float* lds, const Sw62NetWC Wp, const int8_t* __restrict__ boards, const uint8_t* __restrict__ valid,
                                              int B, float* __restrict__ pi, float* __restrict__ v, const int wg, const int* sidx = nullptr,
                                              unsigned long long* smask = nullptr) {
    using C = Sw62<P>;
    constexpr int AW = (C::A + 63) / 64;
    float* X = lds;                          // [ROWS][52]
    float* Q = X + C::ROWS * SW_XS;          // [ROWS][148]: q 0..47, k 48..95, v 96..143
    float* G = Q + C::ROWS * SW_QS;          // [NS][48]
    int tid_ = threadIdx.x;
    if (ASYNC) asm volatile("" : "+v"(tid_));            // (opaque inside the pipeline's persistent loop)
    const int tid = tid_, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
    const int s0 = wg * C::NS, ns = ASYNC ? C::NS : min(C::NS, B - s0);
    if constexpr (ASYNC) {
        if (tid < C::NS * AW) {
            const int b = sidx[tid / AW];
            smask[tid] = b >= 0 ? __hip_atomic_load((const unsigned long long*)(valid + (size_t)b * AL_STRIDE + AL_MASK) + tid % AW, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT)
                                : 0ull;
        }
    }

    // ---- stem: wave w < RT owns row tile w.  Padding rows and samples past B are computed on zero tokens (finite), stored as zero ----
    if (wave < C::RT) {
        const int row = wave * 16 + i16, s = row / C::NT, t = row - s * C::NT;
        int c[8];
        if constexpr (ASYNC) {               // (the token's 8 bytes in one agent-scope load: written write-through by a descent wave on another CU)
            const int b = s < C::NS ? sidx[s] : -1;
            const unsigned long long tok = b >= 0 && t < C::N ? __hip_atomic_load((const unsigned long long*)(boards + (size_t)b * AL_STRIDE) + t,
                                                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                                              : 0ull;
#pragma unroll
            for (int k = 0; k < 8; k++) c[k] = (int)(int8_t)(tok >> (8 * k));
        } else {
            const bool live = s < ns && t < C::N;
#pragma unroll
            for (int k = 0; k < 8; k++) c[k] = live ? (int)boards[((size_t)(s0 + s) * C::N + t) * 8 + k] : 0;
        }
        float f[21];
        f[0] = (float)c[0] / 10.f, f[1] = (float)c[3] / 10.f, f[2] = (float)c[4] / 10.f, f[3] = (float)c[5] / 10.f, f[4] = (float)c[6] / 10.f;
#pragma unroll
        for (int k = 0; k < 8; k++) {        // floor((x) / 2^k) mod 2 of the reference == bit k of the int8 two's-complement pattern
            f[5 + k] = (float)((c[3] >> k) & 1);
            f[13 + k] = (float)((c[4] >> k) & 1);
        }
        const int e1 = min(max(c[1] + 15, 0), 30), e2 = min(max(c[2] + 20, 0), 40), e7 = min(max(c[7] + 1, 0), 5);
        float* xr = X + row * SW_XS;
#pragma unroll 1
        for (int q = 0; q < 3; q++) {        // (not unrolled: 63 float4 weight reads per pass, the unrolled loop spills)
            const int col = 16 * q + 4 * g;
            const float4 b = *(const float4*)(W.bst + col), t1 = *(const float4*)(W.Tppl + e1 * SW_D + col);
            const float4 t2 = *(const float4*)(W.Tpwr + e2 * SW_D + col), t3 = *(const float4*)(W.Tpl + e7 * SW_D + col);
            float4 a = make_float4(b.x + t1.x + t2.x + t3.x, b.y + t1.y + t2.y + t3.y, b.z + t1.z + t2.z + t3.z, b.w + t1.w + t2.w + t3.w);
#pragma unroll
            for (int k = 0; k < 21; k++) {
                const float4 w = *(const float4*)(W.Wst + k * SW_D + col);
                a.x = fmaf(f[k], w.x, a.x), a.y = fmaf(f[k], w.y, a.y), a.z = fmaf(f[k], w.z, a.z), a.w = fmaf(f[k], w.w, a.w);
            }
            *(float4*)(xr + col) = a;
        }
        float x[12];
        sw_load_row(xr, g, x);
        sw_layernorm(x, W.lnsw, W.lnsb, g);
        if (t >= C::N) {
#pragma unroll
            for (int m = 0; m < 12; m++) x[m] = 0.f;
        }
        sw_store_row(xr, g, x);
    }
    __syncthreads();

    for (int l = 0; l < SW_LAYERS; l++) {
        // ---- pass 1: QKV = X W_in^T + b_in; item = (row tile, part) ----
        for (int it = wave; it < C::RT * 3; it += SW_WAVES) {
            const int rt = it / 3, part = it - 3 * rt, row = rt * 16 + i16;
            float a[12];
            sw_load_row(X + row * SW_XS, g, a);
#pragma unroll
            for (int u = 0; u < 3; u++) {
                const int ct = 3 * part + u;
                const f32x4 acc = sw_gemm_tile<12>(W.Wqkv + (size_t)((l * 9 + ct) * 12) * 64, a, lane);
                const float4 bb = *(const float4*)(W.bqkv + l * 144 + 16 * ct + 4 * g);
                *(float4*)(Q + row * SW_QS + 16 * ct + 4 * g) = make_float4(acc[0] + bb.x, acc[1] + bb.y, acc[2] + bb.z, acc[3] + bb.w);
            }
        }
        __syncthreads();

        // ---- pass 2: attention + out_proj + LN1 + feed-forward + LN2 of query tile `wave` ----
        if (wave < C::RT) {
            const int row = wave * 16 + i16, s = wave / C::TPS, kb = s * C::NT, t = row - kb;
            float o[12];
#pragma unroll
            for (int h = 0; h < 3; h++) {
                const float4 qv = *(const float4*)(Q + row * SW_QS + 16 * h + 4 * g);
                float sc[C::TPS][4];
                float mx = -INFINITY;
#pragma unroll
                for (int kt = 0; kt < C::TPS; kt++) {
                    const float4 kv = *(const float4*)(Q + (kb + 16 * kt + i16) * SW_QS + 48 + 16 * h + 4 * g);
                    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
                    acc = sw_mfma(kv.x, qv.x, acc);
                    acc = sw_mfma(kv.y, qv.y, acc);
                    acc = sw_mfma(kv.z, qv.z, acc);
                    acc = sw_mfma(kv.w, qv.w, acc);
#pragma unroll
                    for (int j = 0; j < 4; j++) {    // score of key 16 kt + 4 g + j for query i16
                        sc[kt][j] = 16 * kt + 4 * g + j < C::N ? acc[j] : -INFINITY;
                        mx = fmaxf(mx, sc[kt][j]);
                    }
                }
                mx = sw_row_max(mx);
                float sum = 0.f;
#pragma unroll
                for (int kt = 0; kt < C::TPS; kt++)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        sc[kt][j] = expf(sc[kt][j] - mx);
                        sum += sc[kt][j];
                    }
                sum = sw_row_sum(sum);
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kt = 0; kt < C::TPS; kt++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc = sw_mfma(Q[(kb + 16 * kt + 4 * g + j) * SW_QS + 96 + 16 * h + i16], sc[kt][j], acc);
#pragma unroll
                for (int j = 0; j < 4; j++) o[4 * h + j] = acc[j] / sum;
            }
            float x1[12];
            sw_load_row(X + row * SW_XS, g, x1);
#pragma unroll
            for (int ct = 0; ct < 3; ct++) {
                const f32x4 acc = sw_gemm_tile<12>(W.Wo + (size_t)((l * 3 + ct) * 12) * 64, o, lane);
                const float4 bb = *(const float4*)(W.bo + l * SW_D + 16 * ct + 4 * g);
                x1[4 * ct] += acc[0] + bb.x, x1[4 * ct + 1] += acc[1] + bb.y, x1[4 * ct + 2] += acc[2] + bb.z, x1[4 * ct + 3] += acc[3] + bb.w;
            }
            sw_layernorm(x1, W.ln1w + l * SW_D, W.ln1b + l * SW_D, g);
            // feed-forward in four chunks of 48 hidden channels (hidden chunk -> VGPRs -> its 12 k-steps of linear2): the 192 hidden
            // values never live at once
            f32x4 y[3] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll 1
            for (int c = 0; c < 4; c++) {
                float hc[12];
#pragma unroll
                for (int u = 0; u < 3; u++) {
                    const int ct = 3 * c + u;
                    const f32x4 acc = sw_gemm_tile<12>(W.W1 + (size_t)((l * 12 + ct) * 12) * 64, x1, lane);
                    const float4 bb = *(const float4*)(W.b1 + l * 192 + 16 * ct + 4 * g);
                    hc[4 * u] = fmaxf(acc[0] + bb.x, 0.f), hc[4 * u + 1] = fmaxf(acc[1] + bb.y, 0.f);
                    hc[4 * u + 2] = fmaxf(acc[2] + bb.z, 0.f), hc[4 * u + 3] = fmaxf(acc[3] + bb.w, 0.f);
                }
#pragma unroll
                for (int ct = 0; ct < 3; ct++) y[ct] = sw_gemm_tile<12>(W.W2 + (size_t)((l * 3 + ct) * 48 + 12 * c) * 64, hc, lane, y[ct]);
            }
#pragma unroll
            for (int ct = 0; ct < 3; ct++) {
                const float4 bb = *(const float4*)(W.b2 + l * SW_D + 16 * ct + 4 * g);
                x1[4 * ct] += y[ct][0] + bb.x, x1[4 * ct + 1] += y[ct][1] + bb.y, x1[4 * ct + 2] += y[ct][2] + bb.z, x1[4 * ct + 3] += y[ct][3] + bb.w;
            }
            sw_layernorm(x1, W.ln2w + l * SW_D, W.ln2b + l * SW_D, g);
            if (t < C::N) sw_store_row(X + row * SW_XS, g, x1);
        }
        __syncthreads();
    }

    // ---- heads: logits L [NS][A] over the QKV buffer in the policy layout [l0 | l1 | l2 | l3 | g0..7 | l4 | g8..15] ----
    float* L = Q;
    for (int e = tid; e < C::NS * C::NA * 5; e += SW_THREADS) {      // local head of area token t, column c
        const int s = e / (C::NA * 5), r = e - s * (C::NA * 5), t = r / 5, c = r - 5 * t;
        const float* xr = X + (s * C::NT + t) * SW_XS;
        float a = W.bl[c];
#pragma unroll 8
        for (int d = 0; d < SW_D; d++) a = fmaf(xr[d], W.Wl[d * 5 + c], a);
        L[s * C::A + (c < 4 ? c * C::NA + t : 4 * C::NA + 8 + t)] = a;
    }
    for (int e = tid; e < C::NS * SW_D; e += SW_THREADS) {           // mean of the non-area tokens
        const int s = e / SW_D, d = e - s * SW_D;
        float sum = 0.f;
        for (int t = C::NA; t < C::N; t++) sum += X[(s * C::NT + t) * SW_XS + d];
        G[e] = sum / (float)(C::N - C::NA);
    }
    __syncthreads();
    for (int e = tid; e < C::NS * (16 + P); e += SW_THREADS) {       // global head (g0..15) and value head
        const int s = e / (16 + P), c = e - s * (16 + P);
        const float* gs = G + s * SW_D;
        if (c < 16) {
            float a = W.bg[c];
            for (int d = 0; d < SW_D; d++) a = fmaf(gs[d], W.Wg[d * 16 + c], a);
            L[s * C::A + (c < 8 ? 4 * C::NA + c : 5 * C::NA + c)] = a;
        } else if (ASYNC ? sidx[s] >= 0 : s < ns) {
            float a = W.bv[c - 16];
            for (int d = 0; d < SW_D; d++) a = fmaf(gs[d], W.Wv[d * P + c - 16], a);
            if constexpr (ASYNC) __hip_atomic_store((uint32_t*)v + (size_t)sidx[s] * P + c - 16, __float_as_uint(tanhf(a)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else v[(size_t)(s0 + s) * P + c - 16] = tanhf(a);
        }
    }
    __syncthreads();
    if (wave < ns && (!ASYNC || sidx[wave] >= 0)) {          // masked softmax of sample `wave` (invalid -> -1e8, as the reference)
        const int b = ASYNC ? sidx[wave] : s0 + wave;
        float* lg = L + wave * C::A;
        const uint8_t* va = valid + (size_t)b * C::A;
        float mx = -3.0e38f;
        for (int a = lane; a < C::A; a += 64) {
            bool ok;
            if constexpr (ASYNC) ok = (smask[wave * AW + (a >> 6)] >> lane) & 1ull;
            else ok = va[a];
            const float x = ok ? lg[a] : -1e8f;
            lg[a] = x;
            mx = fmaxf(mx, x);
        }
        mx = nn_wave_max(mx);
        float sum = 0.f;
        for (int a = lane; a < C::A; a += 64) {
            const float e = expf(lg[a] - mx);
            lg[a] = e;
            sum += e;
        }
        sum = nn_wave_sum(sum);
        float* po = pi + (size_t)b * C::A;
        for (int a = lane; a < C::A; a += 64) {
            if constexpr (ASYNC) __hip_atomic_store((uint32_t*)po + a, __float_as_uint(lg[a] / sum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else po[a] = lg[a] / sum;
        }
    }
}
#undef W

template <int P>
__global__ __launch_bounds__(SW_THREADS) void k_sw62_net(Sw62NetW W /* first argument: offset 0 of the kernel argument segment, read through it */,
                                                       const int8_t* __restrict__ boards, const uint8_t* __restrict__ valid, int B,
                                                       float* __restrict__ pi, float* __restrict__ v) {
    __shared__ __attribute__((aligned(16))) float lds[Sw62<P>::LDS_FLOATS];
    (void)W;
    sw62_net_body<P, false>(lds, (Sw62NetWC)__builtin_amdgcn_kernarg_segment_ptr(), boards, valid, B, pi, v, (int)blockIdx.x);
}

}  // namespace azg
