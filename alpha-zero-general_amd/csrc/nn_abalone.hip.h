// nn_abalone.hip.h -- the Abalone MobileNet (abalone/AbaloneNNet.py nn_version 21, forward :173-201: conv3x3 3 -> 24 + BN + ReLU,
// four torchvision InvertedResidual blocks 24 -> 48 -> 24 (1x1 expand + BN + ReLU, depthwise 3x3 + BN + ReLU, 1x1 project + BN,
// residual), policy 1x1 conv 24 -> 42 + BN laid out [9][9][42] + masked softmax over 3402 actions, value 1x1 conv 24 -> 4 + BN + ReLU
// (channel-major) ++ Linear(6, 16) + ReLU of the metadata -> 64 -> P, tanh) as ONE launch per leaf batch.
//
// Geometry.  A workgroup owns NS = 4 samples; its activation tiles are CELL-major, row = cell * 4 + sample (81 cells -> 324 rows, padded
// to 21 MFMA row tiles = 336 rows: a 16-row tile is four neighbouring cells x the four samples).  Every GEMM is out^T = W^T x act^T on
// v_mfma_f32_16x16x4_f32 with the weights as the A operand (fragments in global memory, kept in VGPRs for a whole pass) and the
// activations as the B operand; lane (i = lane & 15, g = lane >> 4) ends with the four output channels 16 t + 4 g .. + 3 of row i.
//   first conv   K = 27 (tap * 3 + c, padded to 32: MFMA m reads k = 8 g + m), 2 column tiles (24 -> 32); the 0/1 inputs are read
//                straight from the staged int8 boards, a tap that leaves the 9 x 9 square is a zero (per lane: a tile spans 4 cells)
//   expand       K = 24 (MFMA m reads k = 6 g + m: three float2 LDS reads per row), 3 column tiles (48)
//   depthwise    on the vector ALUs, fused into the project GEMM: the lane computes the 12 depthwise outputs of channels 12 g .. + 11
//                of its row (nine taps x three float4 reads of the expanded tile, weights in VGPRs) and feeds them as the B operand
//   project      K = 48 (MFMA m reads k = 12 g + m), 2 column tiles (24 -> 32); bias + residual added in place into X (the lane that
//                reads an element writes it; the depthwise pass reads H only)
//   heads        one GEMM K = 24, 3 column tiles: columns 0..41 the policy conv, 42..45 the value conv, 46..47 zero
// LDS (108.8 KB, one workgroup per CU): X [336][28] f32 (the 24-channel residual stream), H [336][52] f32 (the 48-channel expanded
// tile; row strides 28 / 52: multiples of 4, so the float4 accesses stay aligned), 1.25 KB of head vectors.
// The whole expanded tile of the four samples fits next to the residual stream, so no band schedule is needed: each block is two passes
// (expand; depthwise + project) with one barrier after each.  The int8 boards are staged in H before block 0, the logits [4][3402]
// and value features [4][340] in H after block 3.  Eight waves walk the 21 row tiles of a pass (3 3 3 3 3 2 2 2).
//
// Operand precision: f32 MFMA (exact products, f32 accumulation), not the f16 x 2 split operands of the Santorini / Splendor kernels.
// The net is 1.05 M MACs per sample of which 0.9 M are GEMMs with K = 24 / 48 and N = 24 / 48: at these widths the padding of the
// f16 x 2 path (K chunks of 32, three MFMAs per product) leaves a small gain over the f32 instruction, for a second operand format of
// every activation tile and a bounded activation range.  f32 keeps the full range and the same 1e-5 contract as the torch net.
// Roofline (4096 leaves): 4.45 G MFMA MACs with the padding (57 us at the f32-MFMA peak) + 0.57 G depthwise FMAs on the
// VALU (15 us) + 71 MB of pi / masks / boards (11 us); measured 270 us.
#pragma once
#include "nn_kernels.hip.h"

namespace azg {

struct Aba21NetW {
    const float *W0, *b0;     // first conv: [2 ct][8 m][64 lanes] element W0[k = 8 g + m][16 ct + (lane & 15)], k = tap * 3 + c (< 27); bias [24]
    const float *We, *be;     // expand: per block [3 ct][6 m][64] element We[k = 6 g + m][16 ct + i]; bias [NB][48]
    const float *Wd, *bd;     // depthwise: [NB][48][9] (BN folded); bias [NB][48]
    const float *Wp, *bp;     // project: per block [2 ct][12 m][64] element Wp[k = 12 g + m][16 ct + i] (columns 24..31 zero); bias [NB][24]
    const float *Wh, *bh;     // heads 1x1: [3 ct][6 m][64] element Wh[k = 6 g + m][col] (policy 0..41, value 42..45, zero 46..47); bias [48]
    const float *Wm, *bm;     // meta fc [6][16], bias [16]
    const float *Wf1, *bf1;   // value fc1 [340][64] (row = c * 81 + cell, then the 16 meta features), bias [64]
    const float *Wf2, *bf2;   // value fc2 [64][P], bias [P]
};

constexpr int ABA_NS = 4, ABA_CELLS = 81, ABA_BOARD = 324, ABA_RT = 21, ABA_ROWS = ABA_RT * 16, ABA_XS = 28, ABA_HS = 52;
constexpr int ABA_A = 3402, ABA_FEAT = 340, ABA_THREADS = 512;
constexpr size_t ABA_LDS = (size_t)(ABA_ROWS * ABA_XS + ABA_ROWS * ABA_HS + ABA_NS * 16 + ABA_NS * 64) * sizeof(float);
static_assert(ABA_LDS <= 160 * 1024, "k_aba21_net: LDS");
static_assert(ABA_NS * (ABA_A + ABA_FEAT) <= ABA_ROWS * ABA_HS, "k_aba21_net: head buffers in H");

__device__ __forceinline__ bool aba_on(int cell, int tap, int& ncell) {   // tap (ky * 3 + kx) of a cell stays on the 9 x 9 square
    const int y = cell / 9, x = cell - 9 * y, yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
    ncell = yy * 9 + xx;
    return cell < ABA_CELLS && yy >= 0 && yy < 9 && xx >= 0 && xx < 9;
}

template <int NB, int P>
__global__ __launch_bounds__(ABA_THREADS) void k_aba21_net(Aba21NetW N, const int8_t* __restrict__ boards, const uint8_t* __restrict__ valid,
                                                          int B, float* __restrict__ pi, float* __restrict__ v) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    float* X = (float*)lds;                      // [336][28]
    float* H = X + ABA_ROWS * ABA_XS;            // [336][52]
    float* M = H + ABA_ROWS * ABA_HS;            // meta [4][16], value fc1 [4][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
    const int s0 = blockIdx.x * ABA_NS, ns = min(ABA_NS, B - s0);

    // ---- boards -> LDS (int8, behind H's first bytes); samples past B are empty boards whose outputs are not written ----
    int8_t* Bd = (int8_t*)H;
    for (int e = tid; e < ABA_NS * ABA_BOARD; e += ABA_THREADS) {
        const int s = e / ABA_BOARD;
        Bd[e] = s < ns ? boards[(size_t)(s0 + s) * ABA_BOARD + (e - s * ABA_BOARD)] : (int8_t)0;
    }
    __syncthreads();
    if (tid < ABA_NS * 16) {                     // meta_fc: board[0][0..5][3] -> 16, ReLU
        const int s = tid >> 4, o = tid & 15;
        float m = N.bm[o];
#pragma unroll
        for (int q = 0; q < 6; q++) m = fmaf((float)Bd[s * ABA_BOARD + q * 4 + 3], N.Wm[q * 16 + o], m);
        M[tid] = fmaxf(m, 0.f);
    }

    // ---- first conv 3 -> 24 (+ folded BN, ReLU); rows of the padding cells 81..83 are zero ----
    {
        float w0[2][8];
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int m = 0; m < 8; m++) w0[t][m] = N.W0[(t * 8 + m) * 64 + lane];
        for (int rt = wave; rt < ABA_RT; rt += ABA_THREADS / 64) {
            const int row = rt * 16 + i16, cell = row >> 2, s = row & 3;
            f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const int k = 8 * g + m, tap = k / 3, c = k - 3 * tap;
                int nc;
                const float b = (k < 27 && aba_on(cell, tap, nc)) ? (float)Bd[s * ABA_BOARD + nc * 4 + c] : 0.f;
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[0][m], b, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[1][m], b, acc[1], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int co = 16 * t + 4 * g;
                if (co < 24) {
                    const float4 bb = *(const float4*)(N.b0 + co);
                    float4 o = make_float4(fmaxf(acc[t][0] + bb.x, 0.f), fmaxf(acc[t][1] + bb.y, 0.f), fmaxf(acc[t][2] + bb.z, 0.f),
                                           fmaxf(acc[t][3] + bb.w, 0.f));
                    if (cell >= ABA_CELLS) o = make_float4(0.f, 0.f, 0.f, 0.f);
                    *(float4*)(X + row * ABA_XS + co) = o;
                }
            }
        }
    }
    __syncthreads();

    // ---- the inverted residual blocks ----
    for (int b = 0; b < NB; b++) {
        {   // expand 24 -> 48 (+ BN, ReLU): X -> H
            float we[3][6];
#pragma unroll
            for (int t = 0; t < 3; t++)
#pragma unroll
                for (int m = 0; m < 6; m++) we[t][m] = N.We[((b * 3 + t) * 6 + m) * 64 + lane];
            float4 be[3];
#pragma unroll
            for (int t = 0; t < 3; t++) be[t] = *(const float4*)(N.be + b * 48 + 16 * t + 4 * g);
            for (int rt = wave; rt < ABA_RT; rt += ABA_THREADS / 64) {
                const int row = rt * 16 + i16;
                const float2* xr = (const float2*)(X + row * ABA_XS + 6 * g);
                const float2 a0 = xr[0], a1 = xr[1], a2 = xr[2];
                const float a[6] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y};
                f32x4 acc[3] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int m = 0; m < 6; m++)
#pragma unroll
                    for (int t = 0; t < 3; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(we[t][m], a[m], acc[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 3; t++)
                    *(float4*)(H + row * ABA_HS + 16 * t + 4 * g) = make_float4(fmaxf(acc[t][0] + be[t].x, 0.f), fmaxf(acc[t][1] + be[t].y, 0.f),
                                                                                fmaxf(acc[t][2] + be[t].z, 0.f), fmaxf(acc[t][3] + be[t].w, 0.f));
            }
        }
        __syncthreads();
        {   // depthwise 3x3 (+ BN, ReLU) on the fly as the B operand of the project 48 -> 24 (+ BN) + residual: H -> X
            float wd[12][9], bd[12], wp[2][12];
#pragma unroll
            for (int m = 0; m < 12; m++) {
                bd[m] = N.bd[b * 48 + 12 * g + m];
#pragma unroll
                for (int t = 0; t < 9; t++) wd[m][t] = N.Wd[(b * 48 + 12 * g + m) * 9 + t];
            }
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int m = 0; m < 12; m++) wp[t][m] = N.Wp[((b * 2 + t) * 12 + m) * 64 + lane];
            const float4 bp0 = *(const float4*)(N.bp + b * 24 + 4 * g);
            const float4 bp1 = g < 2 ? *(const float4*)(N.bp + b * 24 + 16 + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
            for (int rt = wave; rt < ABA_RT; rt += ABA_THREADS / 64) {
                const int row = rt * 16 + i16, cell = row >> 2, s = row & 3;
                float d[12];
#pragma unroll
                for (int m = 0; m < 12; m++) d[m] = bd[m];
#pragma unroll
                for (int tap = 0; tap < 9; tap++) {
                    int nc;
                    if (aba_on(cell, tap, nc)) {
                        const float4* hp = (const float4*)(H + (nc * 4 + s) * ABA_HS + 12 * g);
                        const float4 h0 = hp[0], h1 = hp[1], h2 = hp[2];
                        const float h[12] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w, h2.x, h2.y, h2.z, h2.w};
#pragma unroll
                        for (int m = 0; m < 12; m++) d[m] = fmaf(wd[m][tap], h[m], d[m]);
                    }
                }
                f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int m = 0; m < 12; m++) {
                    const float dm = fmaxf(d[m], 0.f);
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[0][m], dm, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[1][m], dm, acc[1], 0, 0, 0);
                }
                if (cell < ABA_CELLS) {
                    float4* x0 = (float4*)(X + row * ABA_XS + 4 * g);
                    const float4 r0 = *x0;
                    *x0 = make_float4((acc[0][0] + bp0.x) + r0.x, (acc[0][1] + bp0.y) + r0.y, (acc[0][2] + bp0.z) + r0.z, (acc[0][3] + bp0.w) + r0.w);
                    if (g < 2) {
                        float4* x1 = (float4*)(X + row * ABA_XS + 16 + 4 * g);
                        const float4 r1 = *x1;
                        *x1 = make_float4((acc[1][0] + bp1.x) + r1.x, (acc[1][1] + bp1.y) + r1.y, (acc[1][2] + bp1.z) + r1.z, (acc[1][3] + bp1.w) + r1.w);
                    }
                }
            }
        }
        __syncthreads();
    }

    // ---- heads: one 1x1 GEMM 24 -> 48 columns (policy 0..41, value 42..45): logits L [4][3402] (cell * 42 + plane), value features
    // F [4][340] (c * 81 + cell, then the 16 meta features) ----
    float* L = H;
    float* F = H + ABA_NS * ABA_A;
    {
        float wh[3][6];
#pragma unroll
        for (int t = 0; t < 3; t++)
#pragma unroll
            for (int m = 0; m < 6; m++) wh[t][m] = N.Wh[(t * 6 + m) * 64 + lane];
        for (int rt = wave; rt < ABA_RT; rt += ABA_THREADS / 64) {
            const int row = rt * 16 + i16, cell = row >> 2, s = row & 3;
            const float2* xr = (const float2*)(X + row * ABA_XS + 6 * g);
            const float2 a0 = xr[0], a1 = xr[1], a2 = xr[2];
            const float a[6] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y};
            f32x4 acc[3] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int m = 0; m < 6; m++)
#pragma unroll
                for (int t = 0; t < 3; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wh[t][m], a[m], acc[t], 0, 0, 0);
            if (cell < ABA_CELLS) {
#pragma unroll
                for (int t = 0; t < 3; t++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int col = 16 * t + 4 * g + r;
                        const float o = acc[t][r] + N.bh[col];
                        if (col < 42) L[s * ABA_A + cell * 42 + col] = o;
                        else if (col < 46) F[s * ABA_FEAT + (col - 42) * ABA_CELLS + cell] = fmaxf(o, 0.f);
                    }
            }
        }
        if (tid < ABA_NS * 16) F[(tid >> 4) * ABA_FEAT + 324 + (tid & 15)] = M[tid];
    }
    __syncthreads();

    if (wave < ABA_NS) {   // masked softmax of sample `wave` (invalid -> -1e8, as the reference; rows of samples past B are skipped)
        const int s = wave;
        if (s < ns) {
            float* l = L + s * ABA_A;
            const uint8_t* va = valid + (size_t)(s0 + s) * ABA_A;
            float mx = -3.0e38f;
            for (int a = lane; a < ABA_A; a += 64) {
                const float x = va[a] ? l[a] : -1e8f;
                l[a] = x;
                mx = fmaxf(mx, x);
            }
            mx = nn_wave_max(mx);
            float sum = 0.f;
            for (int a = lane; a < ABA_A; a += 64) {
                const float e = expf(l[a] - mx);
                l[a] = e;
                sum += e;
            }
            sum = nn_wave_sum(sum);
            float* po = pi + (size_t)(s0 + s) * ABA_A;
            for (int a = lane; a < ABA_A; a += 64) po[a] = l[a] / sum;
        }
    } else {               // value fc1 340 -> 64 + ReLU: thread (s, o)
        const int t2 = tid - ABA_NS * 64, s = t2 >> 6, o = t2 & 63;
        float h = N.bf1[o];
        const float* f = F + s * ABA_FEAT;
        for (int k = 0; k < ABA_FEAT; k++) h = fmaf(f[k], N.Wf1[k * 64 + o], h);
        M[ABA_NS * 16 + t2] = fmaxf(h, 0.f);
    }
    __syncthreads();
    if (tid < ABA_NS * P) {
        const int s = tid / P, o = tid - s * P;
        if (s < ns) {
            float x = N.bf2[o];
            for (int k = 0; k < 64; k++) x = fmaf(M[ABA_NS * 16 + s * 64 + k], N.Wf2[k * P + o], x);
            v[(size_t)(s0 + s) * P + o] = tanhf(x);
        }
    }
}

}  // namespace azg
