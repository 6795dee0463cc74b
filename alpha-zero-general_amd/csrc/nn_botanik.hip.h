// nn_botanik.hip.h -- the Botanik nets (botanik/BotanikNNet.py nn_version 10 :105-160 and 11 :162-237, forward :251-292) as ONE launch
// per leaf batch: the 1-d branch, one (V10) or two (V11) machine branches, the summed branch outputs through final_layers_PI / _V, the
// masked softmax and the tanh.
//
// The net.  Board int8 (66, 5, 7); the forward reads rows 0..25.
//   1-d branch: rows 0..5 as (C = 7, L = 30), token t = r*5 + k, channel c = byte t*7 + c.  first_layer_1d (Linear 7 -> 7 + BN), trunk_1d
//     = InvertedResidual1d(7, 21, 7, 30, ReLU, SE avg: the reference passes "RE" as use_se, which is truthy), then per head
//     InvertedResidual1d(7, 21, 7, 30, Hardswish, SE max) + Flatten (c*30 + t) + Linear(210, 428 | 2).  The "depthwise" layer of these
//     blocks is a dense 30 x 30 token-mixing Linear shared by the 21 channels, then a per-channel BN.
//   machine branch m (mach0: bytes 210.., mach1: 560..): the first 343 bytes as (H, W, C) = (7, 7, 7), conv3x3 7 -> 16 (no bias, no BN),
//     one torchvision InvertedResidual 16 -> 32 -> 16 (ReLU, no SE), then per head three InvertedResidual 16 -> 48 -> 16 (Hardswish,
//     SE avg 48 -> 16 -> 48) + Flatten (c*49 + cell) + Linear(784, 428 | 2).
//   final: policy = Linear(428,428)(ReLU(Linear(428,428)(sum of the branch policies))), masked (-1e8) softmax; value likewise 2 -> 2 -> 2, tanh.
//
// Geometry.  A workgroup owns NS = 8 samples and has eight waves.  The machine activations are CELL-major, row = cell * 8 + sample
// (49 cells -> 392 rows, padded to 25 MFMA row tiles = 400 rows).  Every 1x1 convolution is out^T = W^T x act^T on v_mfma_f32_16x16x4_f32
// with the weights as the A operand (fragments in global memory, kept in VGPRs for a pass) and the activations as the B operand; lane
// (i = lane & 15, g = lane >> 4) ends with output channels 16 t + 4 g .. + 3 of row i (as nn_abalone.hip.h).
//   first conv   K = 63 (tap * 7 + c, padded to 64: MFMA m reads k = 16 g + m) straight from the int8 boards in global memory
//   expand       K = 16 (k = 4 g + m: one float4 LDS read per row), 2 or 3 column tiles
//   depthwise    3x3 on the vector ALUs, fused into the project GEMM as its B operand (times the SE scale of the sample); its weights are
//                tap-major [9][E] and read per tap (float4 per four channels: held in VGPRs for a pass they would take 108 registers and
//                spill); the SE's avg pool is a separate pass, thread (sample, channel), which computes the same depthwise outputs once more
//   project      K = 32 / 48 (k = G g + m), 1 column tile; bias + residual added in place (the lane that reads an element writes it)
// The branch policy Linears are one GEMM over the concatenated features [feat_1d | feat_m0 (| feat_m1)] (K = 994 / 1778, the biases
// summed at pack time), rows = the 8 samples (MFMA rows 8..15 are zero), 27 column tiles (428 -> 432), k = 4 j + g: the accumulators stay
// in VGPRs (wave w owns column tiles w, w + 8, w + 16, w + 24) while the branches are computed one after the other, each branch adding
// its K slice once its head features are in LDS.  final_layers_PI are two more such GEMMs (K = 432).  The weights of these GEMMs are
// streamed from global memory (L2) once per workgroup.  The value Linears (N = 2) are wave dot products, wave = sample.
// The 1-d branch (84 k MACs per sample, K = 7 / 21 / 30) runs on the vector ALUs, one thread per output element.
// LDS (150.8 KB, one workgroup per CU): X [400][20] (the branch's trunk stream), Y [400][20] (the head stream), H [400][52] (the expanded
// tile; also the 1-d branch, the head features and the final-layer vectors in turn), 3.6 KB of SE and value vectors.
// NS: 8 is the largest sample count whose expanded tile fits in LDS next to X and Y (not timed against others; 4 would halve the MFMA
// rows that are real samples in the FC GEMMs and double the weight stream per sample).  Measured at 4096 leaves: 760 us (V10) and
// 1285 us (V11), 11 % of the f32-MFMA floor; batching the FC weight loads (BOT_FCU) took it from 996 / 1980 us.  DESIGN.md §3.11, §9.
//
// Operand precision: f32 MFMA (exact products, f32 accumulation) and f32 VALU, the same 1e-5 contract as the torch net.
#pragma once
#include "nn_kernels.hip.h"

namespace azg {

struct BotNetW {
    const float* W1d;   // 1-d branch blob (BOT1_*): first layer W [7][7] (out, in), b [7]; then trunk, PI head, V head blocks of BOT1_BLK floats
    const float* Wm;    // machine branch blobs, BOT_MBLOB floats per branch (BOTM_*)
    const float* Wpi;   // policy FC fragments: [27 ct][53 j][64] (1-d, K 210 padded to 212), then per branch [27][196][64]; element W[4 j + g][16 ct + i]
    const float* bpi;   // [432] the branch policy biases summed (428..431 zero)
    const float* Wv;    // value FC rows: 1-d [2][210], then per branch [2][784]
    const float *Wf1, *bf1, *Wf2, *bf2;   // final_layers_PI.0 / .2 as [27][108][64] fragments (K, N 428 -> 432, zero padded), biases [432]
    const float* tail;  // [14]: summed value biases [2], final_layers_V.0 W [2][2] (out, in), b [2], final_layers_V.2 W [2][2], b [2]
};

constexpr int BOT_NS = 8, BOT_THREADS = 512, BOT_WAVES = BOT_THREADS / 64;
constexpr int BOT_BOARD = 2310, BOT_A = 428, BOT_CT = 27, BOT_CELLS = 49, BOT_RT = 25, BOT_ROWS = BOT_RT * 16, BOT_XS = 20, BOT_HS = 52;
constexpr int BOT_F1 = 212, BOT_FM = 784, BOT_FMLD = 788, BOT_ZLD = 436, BOT_E1 = 630;
// 1-d blob: offsets inside one block of BOT1_BLK floats
constexpr int BOT1_BLK0 = 56, BOT1_BLK = 1629;
constexpr int BOT1_WE = 0, BOT1_BE = 147, BOT1_WT = 168, BOT1_SD = 1068, BOT1_BD = 1089, BOT1_W1 = 1110, BOT1_B1 = 1278, BOT1_W2 = 1286,
              BOT1_B2 = 1454, BOT1_WP = 1475, BOT1_BP = 1622;
// machine blob: conv fragments [16][64]; trunk block at BOTM_T; six SE blocks (PI 0..2, V 3..5) of BOTM_HB floats at BOTM_H
constexpr int BOTM_T = 1024, BOTM_T_BE = 512, BOTM_T_WD = 544, BOTM_T_BD = 832, BOTM_T_WP = 864, BOTM_T_BP = 1376;
constexpr int BOTM_H = 2416, BOTM_HB = 3680, BOTM_BE = 768, BOTM_WD = 816, BOTM_BD = 1248, BOTM_W1 = 1296, BOTM_B1 = 2064, BOTM_W2 = 2080,
              BOTM_B2 = 2848, BOTM_WP = 2896, BOTM_BP = 3664;
constexpr int BOT_MBLOB = BOTM_H + 6 * BOTM_HB;
constexpr int BOT_KQ1 = 53, BOT_KQM = 196, BOT_KQF = 108, BOT_FCU = 8;   // FC K steps (4 each); BOT_FCU steps per batch of loads
constexpr size_t BOT_LDS = (size_t)(2 * BOT_ROWS * BOT_XS + BOT_ROWS * BOT_HS + BOT_NS * (48 + 16 + 48 + 2)) * sizeof(float);
static_assert(BOT_LDS <= 160 * 1024, "k_bot_net: LDS");
static_assert(BOT_NS == BOT_WAVES, "k_bot_net: one wave per sample in the value dots and the softmax");
static_assert(BOT_NS * 16 == 128 && BOT_RT * 16 >= BOT_CELLS * BOT_NS, "k_bot_net: row = cell * 8 + sample");
static_assert(2 * BOT_NS * BOT_F1 + 2 * BOT_NS * BOT_E1 <= BOT_ROWS * BOT_HS, "k_bot_net: 1-d branch in H");
static_assert(BOT_NS * BOT_FMLD <= BOT_ROWS * BOT_HS && 2 * BOT_NS * BOT_ZLD <= BOT_ROWS * BOT_HS, "k_bot_net: features in H");
static_assert(4 * BOT_KQ1 >= 210 && 4 * BOT_KQM == BOT_FM && 4 * BOT_KQF == 16 * BOT_CT && 16 * BOT_CT + 4 <= BOT_ZLD, "k_bot_net: FC K");

template <int ACT>
__device__ __forceinline__ float bot_act(float x) {   // 0: ReLU, 1: Hardswish
    return ACT ? x * (fminf(fmaxf(x + 3.f, 0.f), 6.f) / 6.f) : fmaxf(x, 0.f);
}
__device__ __forceinline__ float bot_hsig(float x) { return fminf(fmaxf(x + 3.f, 0.f), 6.f) / 6.f; }

__device__ __forceinline__ void bot_opaque(int& x) { asm volatile("" : "+v"(x)); }   // keeps per-lane address arithmetic inside the pass

__device__ __forceinline__ bool bot_on(int cell, int tap, int& ncell) {   // tap (ky * 3 + kx) of a cell stays on the 7 x 7 square
    const int y = cell / 7, x = cell - 7 * y, yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
    ncell = yy * 7 + xx;
    return cell < BOT_CELLS && yy >= 0 && yy < 7 && xx >= 0 && xx < 7;
}

// acc[q] += W^T x F^T for the column tiles ct = wave + 8 q of a [27][KQ][64] fragment array; F [8 samples][ldf] in LDS (k < 4 KQ)
template <int KQ>
__device__ __forceinline__ void bot_fc(const float* __restrict__ W, const float* F, int ldf, f32x4 (&acc)[4], int wave, int lane) {
    bot_opaque(lane);
    const int i16 = lane & 15, g = lane >> 4;
    const bool real = i16 < BOT_NS, four = wave + 3 * BOT_WAVES < BOT_CT;   // waves 0..2 own four column tiles, the others three
    const float* f = F + (real ? i16 : 0) * ldf + g;
    // four running pointers (column tiles wave + 8 q).  The weights are loaded BOT_FCU steps at a time before the MFMAs that use them: one
    // load per MFMA with its own wait leaves the pass bound by L2 latency
    const float* w0 = W + (size_t)wave * KQ * 64 + lane;
    const float* w1 = w0 + (size_t)BOT_WAVES * KQ * 64;
    const float* w2 = w1 + (size_t)BOT_WAVES * KQ * 64;
    const float* w3 = w2 + (size_t)BOT_WAVES * KQ * 64;
    int j = 0;
#pragma unroll 1
    for (; j + BOT_FCU <= KQ; j += BOT_FCU) {
        float a[4][BOT_FCU], b[BOT_FCU];
#pragma unroll
        for (int u = 0; u < BOT_FCU; u++) {
            a[0][u] = w0[u * 64];
            a[1][u] = w1[u * 64];
            a[2][u] = w2[u * 64];
            a[3][u] = four ? w3[u * 64] : 0.f;
            b[u] = real ? f[4 * (j + u)] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < BOT_FCU; u++) {
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][u], b[u], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1][u], b[u], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2][u], b[u], acc[2], 0, 0, 0);
            if (four) acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3][u], b[u], acc[3], 0, 0, 0);
        }
        w0 += BOT_FCU * 64;
        w1 += BOT_FCU * 64;
        w2 += BOT_FCU * 64;
        w3 += BOT_FCU * 64;
    }
#pragma unroll 1
    for (; j < KQ; j++) {
        const float b = real ? f[4 * j] : 0.f;
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(*w0, b, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(*w1, b, acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(*w2, b, acc[2], 0, 0, 0);
        if (four) acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(*w3, b, acc[3], 0, 0, 0);
        w0 += 64;
        w1 += 64;
        w2 += 64;
        w3 += 64;
    }
}

// Z[s][16 ct + 4 g + r] = act(acc + bias) for the 8 sample rows
template <bool RELU>
__device__ __forceinline__ void bot_fc_store(const f32x4 (&acc)[4], const float* __restrict__ bias, float* Z, int wave, int lane) {
    const int i16 = lane & 15, g = lane >> 4;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int ct = wave + BOT_WAVES * q, col = 16 * ct + 4 * g;
        if (ct < BOT_CT && i16 < BOT_NS) {
            const float4 b = *(const float4*)(bias + col);
            float4 o = make_float4(acc[q][0] + b.x, acc[q][1] + b.y, acc[q][2] + b.z, acc[q][3] + b.w);
            if (RELU) o = make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
            *(float4*)(Z + i16 * BOT_ZLD + col) = o;
        }
    }
}

// VA[s][o] += Wv[o][:K] . F[s][:K], wave = sample
__device__ __forceinline__ void bot_vdot(const float* __restrict__ Wv, int K, const float* F, int ldf, float* VA, int wave, int lane) {
    bot_opaque(lane);
    const float* f = F + wave * ldf;
    float a0 = 0.f, a1 = 0.f;
    for (int k = lane; k < K; k += 64) {
        a0 = fmaf(Wv[k], f[k], a0);
        a1 = fmaf(Wv[K + k], f[k], a1);
    }
    a0 = nn_wave_sum(a0);
    a1 = nn_wave_sum(a1);
    if (lane == 0) {
        VA[wave * 2] += a0;
        VA[wave * 2 + 1] += a1;
    }
}

// one InvertedResidual1d (7 -> 21 -> 7 over 30 tokens, SE, residual) in place on Xio [8][212]; E, D [8][630]; every thread calls it
template <int ACT, bool MAXPOOL>
__device__ void bot_block1d(const float* __restrict__ w, float* Xio, float* E, float* D, float* SP, float* SH, float* SS, int tid) {
    bot_opaque(tid);
    for (int e = tid; e < BOT_NS * BOT_E1; e += BOT_THREADS) {      // expand 7 -> 21 (+ BN, act)
        const int s = e / BOT_E1, q = e - s * BOT_E1, ch = q / 30, t = q - 30 * ch;
        float o = w[BOT1_BE + ch];
#pragma unroll
        for (int c = 0; c < 7; c++) o = fmaf(w[BOT1_WE + ch * 7 + c], Xio[s * BOT_F1 + c * 30 + t], o);
        E[e] = bot_act<ACT>(o);
    }
    __syncthreads();
    for (int e = tid; e < BOT_NS * BOT_E1; e += BOT_THREADS) {      // token mix 30 -> 30, per-channel BN, act
        const int s = e / BOT_E1, q = e - s * BOT_E1, ch = q / 30, t = q - 30 * ch;
        const float* er = E + s * BOT_E1 + ch * 30;
        const float* wt = w + BOT1_WT + t * 30;
        float o = 0.f;
#pragma unroll 10
        for (int u = 0; u < 30; u++) o = fmaf(wt[u], er[u], o);
        D[e] = bot_act<ACT>(fmaf(o, w[BOT1_SD + ch], w[BOT1_BD + ch]));
    }
    __syncthreads();
    if (tid < BOT_NS * 21) {                                         // SE squeeze over the tokens
        const int s = tid / 21, ch = tid - 21 * s;
        const float* d = D + s * BOT_E1 + ch * 30;
        float p = d[0];
        for (int t = 1; t < 30; t++) p = MAXPOOL ? fmaxf(p, d[t]) : p + d[t];
        SP[tid] = MAXPOOL ? p : p / 30.f;
    }
    __syncthreads();
    if (tid < BOT_NS * 8) {                                          // fc1 21 -> 8 + ReLU
        const int s = tid >> 3, o = tid & 7;
        float h = w[BOT1_B1 + o];
        for (int ch = 0; ch < 21; ch++) h = fmaf(w[BOT1_W1 + o * 21 + ch], SP[s * 21 + ch], h);
        SH[tid] = fmaxf(h, 0.f);
    }
    __syncthreads();
    if (tid < BOT_NS * 21) {                                         // fc2 8 -> 21 + Hardsigmoid
        const int s = tid / 21, ch = tid - 21 * s;
        float x = w[BOT1_B2 + ch];
#pragma unroll
        for (int o = 0; o < 8; o++) x = fmaf(w[BOT1_W2 + ch * 8 + o], SH[s * 8 + o], x);
        SS[tid] = bot_hsig(x);
    }
    __syncthreads();
    for (int e = tid; e < BOT_NS * 210; e += BOT_THREADS) {         // project 21 -> 7 (+ BN) of the scaled tile, residual
        const int s = e / 210, q = e - s * 210, c = q / 30, t = q - 30 * c;
        float o = w[BOT1_BP + c];
        for (int ch = 0; ch < 21; ch++) o = fmaf(w[BOT1_WP + c * 21 + ch], D[s * BOT_E1 + ch * 30 + t] * SS[s * 21 + ch], o);
        Xio[s * BOT_F1 + q] += o;
    }
    __syncthreads();
}

// 1x1 expand 16 -> 16 NCT (+ BN, act): S [400][20] -> H [400][52]
template <int NCT, int ACT>
__device__ __forceinline__ void bot_expand(const float* __restrict__ We, const float* __restrict__ be, const float* S, float* H, int wave, int lane) {
    bot_opaque(lane);
    const int i16 = lane & 15, g = lane >> 4;
    float w[NCT][4];
    float4 b[NCT];
#pragma unroll
    for (int t = 0; t < NCT; t++) {
#pragma unroll
        for (int m = 0; m < 4; m++) w[t][m] = We[(t * 4 + m) * 64 + lane];
        b[t] = *(const float4*)(be + 16 * t + 4 * g);
    }
#pragma unroll 1
    for (int rt = wave; rt < BOT_RT; rt += BOT_WAVES) {
        const int row = rt * 16 + i16;
        const float4 a4 = *(const float4*)(S + row * BOT_XS + 4 * g);
        const float a[4] = {a4.x, a4.y, a4.z, a4.w};
        f32x4 acc[NCT];
#pragma unroll
        for (int t = 0; t < NCT; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 4; m++)
#pragma unroll
            for (int t = 0; t < NCT; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][m], a[m], acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NCT; t++)
            *(float4*)(H + row * BOT_HS + 16 * t + 4 * g) = make_float4(bot_act<ACT>(acc[t][0] + b[t].x), bot_act<ACT>(acc[t][1] + b[t].y),
                                                                        bot_act<ACT>(acc[t][2] + b[t].z), bot_act<ACT>(acc[t][3] + b[t].w));
    }
}

// SE of a 48-channel block: avg pool of the depthwise outputs (thread = sample, channel), fc1 48 -> 16 + ReLU, fc2 16 -> 48 + Hardsigmoid
__device__ void bot_se2d(const float* __restrict__ blk, const float* H, float* SP, float* SH, float* SS, int tid) {
    bot_opaque(tid);
    if (tid < BOT_NS * 48) {
        const int s = tid / 48, ch = tid - 48 * s;
        float w9[9];
#pragma unroll
        for (int t = 0; t < 9; t++) w9[t] = blk[BOTM_WD + t * 48 + ch];
        const float bb = blk[BOTM_BD + ch];
        float p = 0.f;
        for (int cell = 0; cell < BOT_CELLS; cell++) {
            float d = bb;
#pragma unroll
            for (int tap = 0; tap < 9; tap++) {
                int nc;
                if (bot_on(cell, tap, nc)) d = fmaf(w9[tap], H[(nc * BOT_NS + s) * BOT_HS + ch], d);
            }
            p += bot_act<1>(d);
        }
        SP[tid] = p / 49.f;
    }
    __syncthreads();
    if (tid < BOT_NS * 16) {
        const int s = tid >> 4, o = tid & 15;
        float h = blk[BOTM_B1 + o];
        for (int ch = 0; ch < 48; ch++) h = fmaf(blk[BOTM_W1 + o * 48 + ch], SP[s * 48 + ch], h);
        SH[tid] = fmaxf(h, 0.f);
    }
    __syncthreads();
    if (tid < BOT_NS * 48) {
        const int s = tid / 48, ch = tid - 48 * s;
        float x = blk[BOTM_B2 + ch];
#pragma unroll
        for (int o = 0; o < 16; o++) x = fmaf(blk[BOTM_W2 + ch * 16 + o], SH[s * 16 + o], x);
        SS[tid] = bot_hsig(x);
    }
}

// depthwise 3x3 (+ BN, act, SE scale) of H as the B operand of the project NE -> 16 (+ BN) + residual into Xio
template <int NE, bool SE, int ACT>
__device__ __forceinline__ void bot_project(const float* __restrict__ Wd, const float* __restrict__ bdw, const float* __restrict__ Wp,
                                            const float* __restrict__ bp, const float* H, const float* SS, float* Xio, int wave, int lane) {
    bot_opaque(lane);
    constexpr int G = NE / 4;
    const int i16 = lane & 15, g = lane >> 4;
    float bb[G], wp[G];
#pragma unroll
    for (int m = 0; m < G; m++) {
        bb[m] = bdw[G * g + m];
        wp[m] = Wp[m * 64 + lane];
    }
    const float4 bq = *(const float4*)(bp + 4 * g);
#pragma unroll 1
    for (int rt = wave; rt < BOT_RT; rt += BOT_WAVES) {
        const int row = rt * 16 + i16, cell = row >> 3, s = row & 7;
        float d[G];
#pragma unroll
        for (int m = 0; m < G; m++) d[m] = bb[m];
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            int nc;
            if (bot_on(cell, tap, nc)) {
                const float4* hp = (const float4*)(H + (nc * BOT_NS + s) * BOT_HS + G * g);
                const float4* wq = (const float4*)(Wd + tap * NE + G * g);   // tap-major weights: one float4 per four channels
#pragma unroll
                for (int q = 0; q < G / 4; q++) {
                    const float4 h = hp[q], w = wq[q];
                    d[4 * q] = fmaf(w.x, h.x, d[4 * q]);
                    d[4 * q + 1] = fmaf(w.y, h.y, d[4 * q + 1]);
                    d[4 * q + 2] = fmaf(w.z, h.z, d[4 * q + 2]);
                    d[4 * q + 3] = fmaf(w.w, h.w, d[4 * q + 3]);
                }
            }
        }
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < G; m++) {
            float dm = bot_act<ACT>(d[m]);
            if (SE) dm *= SS[s * 48 + G * g + m];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[m], dm, acc, 0, 0, 0);
        }
        if (cell < BOT_CELLS) {
            float4* xp = (float4*)(Xio + row * BOT_XS + 4 * g);
            const float4 r = *xp;
            *xp = make_float4((acc[0] + bq.x) + r.x, (acc[1] + bq.y) + r.y, (acc[2] + bq.z) + r.z, (acc[3] + bq.w) + r.w);
        }
    }
}

template <int NM>
__global__ __launch_bounds__(BOT_THREADS) void k_bot_net(BotNetW N, const int8_t* __restrict__ boards, const uint8_t* __restrict__ valid,
                                                         int B, float* __restrict__ pi, float* __restrict__ v) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    float* X = (float*)lds;                   // [400][20]
    float* Y = X + BOT_ROWS * BOT_XS;         // [400][20]
    float* H = Y + BOT_ROWS * BOT_XS;         // [400][52]
    float* SP = H + BOT_ROWS * BOT_HS;        // [8][48]
    float* SH = SP + BOT_NS * 48;             // [8][16]
    float* SS = SH + BOT_NS * 16;             // [8][48]
    float* VA = SS + BOT_NS * 48;             // [8][2] summed value outputs of the branches
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
    const int s0 = blockIdx.x * BOT_NS, ns = min(BOT_NS, B - s0);
    const int8_t* bd = boards + (size_t)s0 * BOT_BOARD;   // samples past B read as empty boards; their outputs are not written

    f32x4 acc[4] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    if (tid < BOT_NS * 2) VA[tid] = N.tail[tid & 1];

    // ---- 1-d branch (vector ALUs) in H: X1, Y1 [8][212] (columns 210, 211 zero: the K padding of the policy GEMM), E, D [8][630] ----
    {
        float* X1 = H;
        float* Y1 = X1 + BOT_NS * BOT_F1;
        float* E = Y1 + BOT_NS * BOT_F1;
        float* D = E + BOT_NS * BOT_E1;
        for (int e = tid; e < BOT_NS * BOT_F1; e += BOT_THREADS) {   // first_layer_1d 7 -> 7 (+ BN)
            const int s = e / BOT_F1, q = e - s * BOT_F1, c = q / 30, t = q - 30 * c;
            float o = 0.f;
            if (q < 210) {
                o = N.W1d[49 + c];
#pragma unroll
                for (int cc = 0; cc < 7; cc++) o = fmaf(N.W1d[c * 7 + cc], s < ns ? (float)bd[s * BOT_BOARD + t * 7 + cc] : 0.f, o);
            }
            X1[e] = o;
        }
        __syncthreads();
        bot_block1d<0, false>(N.W1d + BOT1_BLK0, X1, E, D, SP, SH, SS, tid);
#pragma unroll 1
        for (int h = 0; h < 2; h++) {
            for (int e = tid; e < BOT_NS * BOT_F1; e += BOT_THREADS) Y1[e] = X1[e];
            __syncthreads();
            bot_block1d<1, true>(N.W1d + BOT1_BLK0 + (1 + h) * BOT1_BLK, Y1, E, D, SP, SH, SS, tid);
            if (h == 0) bot_fc<BOT_KQ1>(N.Wpi, Y1, BOT_F1, acc, wave, lane);
            else bot_vdot(N.Wv, 210, Y1, BOT_F1, VA, wave, lane);
            __syncthreads();
        }
    }

    // ---- machine branches ----
#pragma unroll 1
    for (int m = 0; m < NM; m++) {
        const float* wm = N.Wm + (size_t)m * BOT_MBLOB;
        const int off = 210 + 350 * m;
        {   // conv3x3 7 -> 16 from the int8 boards: X; the padding rows (cell 49) are zero
            float wc[16];
#pragma unroll
            for (int k = 0; k < 16; k++) wc[k] = wm[k * 64 + lane];
#pragma unroll 1
            for (int rt = wave; rt < BOT_RT; rt += BOT_WAVES) {
                const int row = rt * 16 + i16, cell = row >> 3, s = row & 7;
                f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int mm = 0; mm < 16; mm++) {
                    const int k = 16 * g + mm, tap = k / 7, c = k - 7 * tap;
                    int nc;
                    const float b = (k < 63 && s < ns && bot_on(cell, tap, nc)) ? (float)bd[s * BOT_BOARD + off + nc * 7 + c] : 0.f;
                    a = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[mm], b, a, 0, 0, 0);
                }
                *(float4*)(X + row * BOT_XS + 4 * g) = cell < BOT_CELLS ? make_float4(a[0], a[1], a[2], a[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        __syncthreads();
        {   // trunk: InvertedResidual 16 -> 32 -> 16, ReLU, no SE
            const float* t = wm + BOTM_T;
            bot_expand<2, 0>(t, t + BOTM_T_BE, X, H, wave, lane);
            __syncthreads();
            bot_project<32, false, 0>(t + BOTM_T_WD, t + BOTM_T_BD, t + BOTM_T_WP, t + BOTM_T_BP, H, SS, X, wave, lane);
            __syncthreads();
        }
#pragma unroll 1
        for (int h = 0; h < 2; h++) {   // head h (0 policy, 1 value): three InvertedResidual 16 -> 48 -> 16, Hardswish, SE; on Y
            for (int e = tid; e < BOT_ROWS * BOT_XS; e += BOT_THREADS) Y[e] = X[e];
            __syncthreads();
#pragma unroll 1
            for (int b = 0; b < 3; b++) {
                const float* blk = wm + BOTM_H + (3 * h + b) * BOTM_HB;
                bot_expand<3, 1>(blk, blk + BOTM_BE, Y, H, wave, lane);
                __syncthreads();
                bot_se2d(blk, H, SP, SH, SS, tid);
                __syncthreads();
                bot_project<48, true, 1>(blk + BOTM_WD, blk + BOTM_BD, blk + BOTM_WP, blk + BOTM_BP, H, SS, Y, wave, lane);
                __syncthreads();
            }
            float* F = H;   // head features [8][788], channel-major c * 49 + cell
            for (int e = tid; e < BOT_NS * BOT_FM; e += BOT_THREADS) {
                const int s = e / BOT_FM, q = e - s * BOT_FM, c = q / BOT_CELLS, cell = q - BOT_CELLS * c;
                F[s * BOT_FMLD + q] = Y[(cell * BOT_NS + s) * BOT_XS + c];
            }
            __syncthreads();
            if (h == 0) bot_fc<BOT_KQM>(N.Wpi + (size_t)BOT_CT * BOT_KQ1 * 64 + (size_t)m * BOT_CT * BOT_KQM * 64, F, BOT_FMLD, acc, wave, lane);
            else bot_vdot(N.Wv + 420 + m * 2 * BOT_FM, BOT_FM, F, BOT_FMLD, VA, wave, lane);
            __syncthreads();
        }
    }

    // ---- final_layers_PI: Z = sum + bias, Z2 = ReLU(Linear(Z)), Z = Linear(Z2); masked softmax; value MLP + tanh ----
    float* Z = H;
    float* Z2 = H + BOT_NS * BOT_ZLD;
    bot_fc_store<false>(acc, N.bpi, Z, wave, lane);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    bot_fc<BOT_KQF>(N.Wf1, Z, BOT_ZLD, acc, wave, lane);
    bot_fc_store<true>(acc, N.bf1, Z2, wave, lane);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    bot_fc<BOT_KQF>(N.Wf2, Z2, BOT_ZLD, acc, wave, lane);
    bot_fc_store<false>(acc, N.bf2, Z, wave, lane);
    __syncthreads();

    const int s = wave;
    if (s < ns) {   // masked softmax of sample `wave` (invalid -> -1e8, as the reference)
        float* l = Z + s * BOT_ZLD;
        const uint8_t* va = valid + (size_t)(s0 + s) * BOT_A;
        float mx = -3.0e38f;
        for (int a = lane; a < BOT_A; a += 64) {
            const float x = va[a] ? l[a] : -1e8f;
            l[a] = x;
            mx = fmaxf(mx, x);
        }
        mx = nn_wave_max(mx);
        float sum = 0.f;
        for (int a = lane; a < BOT_A; a += 64) {
            const float e = expf(l[a] - mx);
            l[a] = e;
            sum += e;
        }
        sum = nn_wave_sum(sum);
        float* po = pi + (size_t)(s0 + s) * BOT_A;
        for (int a = lane; a < BOT_A; a += 64) po[a] = l[a] / sum;
        if (lane < 2) {   // final_layers_V: 2 -> 2 + ReLU -> 2, tanh
            const float* T = N.tail;
            const float x0 = VA[s * 2], x1 = VA[s * 2 + 1];
            const float h0 = fmaxf(fmaf(T[3], x1, fmaf(T[2], x0, T[6])), 0.f);
            const float h1 = fmaxf(fmaf(T[5], x1, fmaf(T[4], x0, T[7])), 0.f);
            v[(size_t)(s0 + s) * 2 + lane] = tanhf(fmaf(T[9 + 2 * lane], h1, fmaf(T[8 + 2 * lane], h0, T[12 + lane])));
        }
    }
}

}  // namespace azg
