// nn_akropolis.hip.h -- the Akropolis net (akropolis/AkropolisNNet.py nn_version 31: constructor :91-146, input slicing :377-388,
// forward :573-622) as ONE launch per leaf batch: the board convolutions of every player, the kernel-1 InvertedResidual `proj_p` with
// its squeeze-excitation, the construction-site context, the bilinear policy per site tile, the value head and the masked softmax over
// A = 1014 CS actions (CS = P + 2 site tiles).
//
// Geometry (template on the player count P): board int8 [13][13][C], C = 3P + 2 (descr 0..P-1, height P..2P-1, tileID 2P..3P-1,
// scores plane 3P, globals plane 3P + 1).  One workgroup of three waves per sample; lane `tid` owns board cell `tid` (169 of the 192
// lanes; the other 23 skip the per-cell work and add nothing to the reductions).
//   context  (few lanes) s1 = scores Ws + bs, g1 = Hardswish(globals Wg + bg) (BN folded), t[c] = Hardswish(conv1d over the three
//            site codes through the per-position code tables Tc [3][12][32]); f3[c] = [t, s1, g1].  Then per tile a = Hardswish(f3 Wi
//            + bi) (b1n folded into proj_i), h = f3 Wo + bo, and W_c[o][r] = a[r] h[16 o + r]; proj_p's per-sample constant c0 = [s1, g1]
//            Wec + be; the value head on flatten(f3) -> v = tanh(...).
//   boards   per player: conv1 (5 -> 8, BN folded) from the per-tap code tables T1 [9][12][8] (the embedding folded in; copied to
//            LDS) plus the height and tileID columns, Hardswish, into a zero-bordered 15 x 15 LDS image (two planes of four channels:
//            consecutive cells read consecutive float4); conv2 (8 -> 8, BN folded) reads the 3 x 3 neighbourhood from it, Hardswish,
//            and the lane folds its 8 outputs straight into proj_p's first 1x1 (e[32] += out We[8 i .. 8 i + 7], in VGPRs).
//   proj_p   d = Hardswish(dws Hardswish(e + c0) + dwb); SE mean over the 169 cells (a reduce-scatter butterfly of the 32 channels
//            across the wave, then three partial rows in LDS), 32 -> 8 ReLU -> 32 Hardsigmoid; p = (d * se) Wp + bp, 16 per cell in VGPRs.
//   policy   logit[c][cell][o] = p[cell] . W_c[o] (16 FMAs each, W_c read from LDS as broadcast float4), invalid -> -1e8 as the
//            reference (the dot products accumulate in f64); the 6 CS logits of the lane stay in VGPRs through the workgroup max, the sum
//            of exps and the store.
// Uniform weights (conv1's height / tileID columns, conv2, We, Wp, ...) are read through the scalar cache, one tap / one input channel
// at a time (unrolling further runs out of SGPRs).  LDS (static): the board bytes, the conv1 image [2][225][4], T1, f3, W_c and a few
// vectors: 15.3 / 16.4 / 17.5 KB for P = 2 / 3 / 4.  94 / 100 / 106 VGPRs, no spills, no scratch: 5 / 4 / 4 waves per SIMD, i.e. 6 / 5 / 5
// workgroups per CU.
//
// Why the vector ALUs and not MFMA: every contraction here has K = 8..72 and per-sample shapes of 169 rows (the policy: 169 x 16 x
// 6 CS); the f32 MFMA has the same peak as the f32 VALU on gfx950 (157 TF), and a lane-per-cell layout keeps every intermediate of a
// cell in its own VGPRs from conv2 to the softmax, with no LDS round trip or tile padding.  Operands are f32 with f32 accumulation,
// except the policy's 16-term dot products, which accumulate in f64 (see there).
#pragma once
#include "nn_kernels.hip.h"

namespace azg {

// The weights come in three packed f32 blocks (AkropolisV31Hip.pack, include/azg.h), offsets in floats:
//   w[0] context  Ws [15P][16], bs [16] (dense_scores); Wg [2][8], bg [8] (dense_globs, BN folded); Tc [3][12][32], bc [32]
//                 (conv1d_constr per-position code tables); Wi [56][16], bi [16] (proj_i, b1n folded); Wo [56][96], bo [96] (proj_o,
//                 h[o][r] = column 16 o + r); Wec [24][32], be [32] (proj_p's first 1x1 on the s1 | g1 channels, BN folded); value head
//                 Wv1 [56 CS][16], bv1 [16] (BN folded), Wv2 [16][16], bv2 [16], Wv3 [16][P], bv3 [P]
//   w[1] boards   T1 [9 taps][12 codes][8] (conv1 on the embedded descr, BN folded), W1x [9][2][8] (its height / tileID columns), b1 [8],
//                 W2 [9 taps][8 in][8 out], b2 [8] (conv2, BN folded), We [8P][32] (proj_p's first 1x1 on the board channels, BN folded)
//   w[2] proj_p   dws, dwb [32] (depthwise 1x1 + BN), fc1 [32][8], fc1b [8], fc2 [8][32], fc2b [32] (SE), Wp [32][16], bp [16] (project, BN
//                 folded)
// Three pointers instead of one per tensor: the offsets are compile-time constants, so the kernel holds 6 SGPRs of weight addresses
// and the wave-uniform weight reads of the hot loops go through the scalar cache.
constexpr int AKR_NW = 3, AKR_THREADS = 192, AKR_CELLS = 169, AKR_IMG = 225;

template <int P> struct Akr31 {
    static constexpr int C = 3 * P + 2, CS = P + 2, S = 169 * C, A = 1014 * CS, NL = 6 * CS;
    static constexpr int SB = (S + 15) / 16 * 16;      // board bytes, padded to 16
    // w[0]
    static constexpr int WS = 0, BS = WS + 240 * P, WG = BS + 16, BG = WG + 16, TC = BG + 8, BC = TC + 1152, WI = BC + 32, BI = WI + 896,
                         WO = BI + 16, BO = WO + 5376, WEC = BO + 96, BE = WEC + 768, WV1 = BE + 32, BV1 = WV1 + 896 * CS, WV2 = BV1 + 16,
                         BV2 = WV2 + 256, WV3 = BV2 + 16, BV3 = WV3 + 16 * P, N_CTX = BV3 + P;
    // w[1]
    static constexpr int T1 = 0, W1X = 864, B1 = W1X + 144, W2 = B1 + 8, B2 = W2 + 576, WE = B2 + 8, N_BOARDS = WE + 256 * P;
    // w[2]
    static constexpr int DWS = 0, DWB = 32, FC1 = 64, FC1B = FC1 + 256, FC2 = FC1B + 8, FC2B = FC2 + 256, WP = FC2B + 32, BP = WP + 512,
                         N_PROJ = BP + 16;
};

__device__ __forceinline__ float akr_hs(float x) { return x * fminf(fmaxf(x + 3.f, 0.f), 6.f) * (1.f / 6.f); }   // Hardswish
__device__ __forceinline__ int akr_code(int8_t c) { return min(max((int)c, 0), 11); }                   // clamp(0, 11) of the reference

template <int P>
__global__ __launch_bounds__(AKR_THREADS) void k_akr31_net(const float* __restrict__ wx, const float* __restrict__ wb, const float* __restrict__ wp,
                                                         const int8_t* __restrict__ boards, const uint8_t* __restrict__ valid,
                                                         float* __restrict__ pi, float* __restrict__ v) {
    using K = Akr31<P>;
    constexpr int C = K::C, CS = K::CS;
    __shared__ __attribute__((aligned(16))) float img[2 * AKR_IMG * 4];   // conv1 output, zero border: [quad][15 * 15][4]
    __shared__ __attribute__((aligned(16))) float t1[9 * 12 * 8];
    __shared__ __attribute__((aligned(16))) float f3[CS * 56];
    __shared__ __attribute__((aligned(16))) float wc[CS * 96];            // W_c [c][o][r]
    __shared__ float c0[32], v1[16], v2[16], red[3][32], z[8], se[32], rmax[3], rsum[3];
    __shared__ __attribute__((aligned(16))) int8_t bd[K::SB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t s = blockIdx.x;
    const int8_t* board = boards + s * K::S;
    for (int i = tid; i < K::S; i += AKR_THREADS) bd[i] = board[i];
    for (int i = tid; i < 9 * 12 * 2; i += AKR_THREADS) ((float4*)t1)[i] = ((const float4*)(wb + K::T1))[i];
    for (int i = tid; i < 2 * AKR_IMG; i += AKR_THREADS) ((float4*)img)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();

    // ---- context: t (conv1d of the site codes), s1, g1 -> f3 ----
    for (int e = tid; e < CS * 32 + 24; e += AKR_THREADS) {
        if (e < CS * 32) {
            const int c = e >> 5, o = e & 31;
            float a = wx[K::BC + o];
#pragma unroll
            for (int k = 0; k < 3; k++) a += wx[K::TC + (k * 12 + akr_code(bd[(c * 13 + k) * C + 3 * P + 1])) * 32 + o];
            f3[c * 56 + o] = akr_hs(a);
        } else if (e < CS * 32 + 16) {
            const int j = e - CS * 32;
            float a = wx[K::BS + j];
            for (int q = 0; q < 15 * P; q++) a = fmaf((float)bd[((q / 5) * 13 + q % 5) * C + 3 * P], wx[K::WS + q * 16 + j], a);
            for (int c = 0; c < CS; c++) f3[c * 56 + 32 + j] = a;
        } else {
            const int j = e - CS * 32 - 16;
            const float g0 = (float)bd[((CS + 1) * 13) * C + 3 * P + 1], g1 = (float)bd[((CS + 1) * 13 + 1) * C + 3 * P + 1];
            const float a = akr_hs(fmaf(g1, wx[K::WG + 8 + j], fmaf(g0, wx[K::WG + j], wx[K::BG + j])));
            for (int c = 0; c < CS; c++) f3[c * 56 + 48 + j] = a;
        }
    }
    __syncthreads();

    // ---- W_c = a * h per site tile, proj_p's per-sample constant c0, value layer 1 ----
    for (int e = tid; e < CS * 96 + 48; e += AKR_THREADS) {
        if (e < CS * 96) {
            const int c = e / 96, j = e - 96 * c, r = j & 15;
            const float* f = f3 + c * 56;
            float a = wx[K::BI + r], h = wx[K::BO + j];
#pragma unroll 8
            for (int k = 0; k < 56; k++) {
                a = fmaf(f[k], wx[K::WI + k * 16 + r], a);
                h = fmaf(f[k], wx[K::WO + k * 96 + j], h);
            }
            wc[e] = akr_hs(a) * h;
        } else if (e < CS * 96 + 32) {
            const int o = e - CS * 96;
            float a = wx[K::BE + o];
            for (int k = 0; k < 24; k++) a = fmaf(f3[32 + k], wx[K::WEC + k * 32 + o], a);
            c0[o] = a;
        } else {
            const int j = e - CS * 96 - 32;
            float a = wx[K::BV1 + j];
            for (int k = 0; k < CS * 56; k++) a = fmaf(f3[k], wx[K::WV1 + k * 16 + j], a);
            v1[j] = akr_hs(a);
        }
    }
    __syncthreads();
    if (tid < 16) {
        float a = wx[K::BV2 + tid];
#pragma unroll
        for (int k = 0; k < 16; k++) a = fmaf(v1[k], wx[K::WV2 + k * 16 + tid], a);
        v2[tid] = akr_hs(a);
    }
    __syncthreads();

    // ---- the P boards: conv1 -> LDS image -> conv2 -> proj_p's first 1x1, accumulated in VGPRs ----
    const bool live = tid < AKR_CELLS;
    const int cell = live ? tid : 0, y = cell / 13, x = cell - 13 * y;      // (lanes past the board address cell 0 and store nothing)
    float e[32];
#pragma unroll
    for (int o = 0; o < 32; o++) e[o] = 0.f;
#pragma unroll 1
    for (int i = 0; i < P; i++) {
        if (live) {
            float acc[8];
#pragma unroll
            for (int o = 0; o < 8; o++) acc[o] = wb[K::B1 + o];
#pragma unroll 1
            for (int t = 0; t < 9; t++) {
                    const int ky = t / 3, kx = t - 3 * ky, yy = y + ky - 1, xx = x + kx - 1;
                    if (yy >= 0 && yy < 13 && xx >= 0 && xx < 13) {   // the conv pads its (embedded) input with zeros
                        const int8_t* cp = bd + (yy * 13 + xx) * C;
                        const float hgt = (float)cp[P + i], tile = (float)cp[2 * P + i];
                        const float4* tb = (const float4*)(t1 + (t * 12 + akr_code(cp[i])) * 8);
                        const float4 ta = tb[0], tc = tb[1];
                        const float tv[8] = {ta.x, ta.y, ta.z, ta.w, tc.x, tc.y, tc.z, tc.w};
#pragma unroll
                        for (int o = 0; o < 8; o++) acc[o] += fmaf(tile, wb[K::W1X + t * 16 + 8 + o], fmaf(hgt, wb[K::W1X + t * 16 + o], tv[o]));
                    }
                }
            const int q = (y + 1) * 15 + x + 1;
            ((float4*)img)[q] = make_float4(akr_hs(acc[0]), akr_hs(acc[1]), akr_hs(acc[2]), akr_hs(acc[3]));
            ((float4*)img)[AKR_IMG + q] = make_float4(akr_hs(acc[4]), akr_hs(acc[5]), akr_hs(acc[6]), akr_hs(acc[7]));
        }
        __syncthreads();
        if (live) {
            float acc[8];
#pragma unroll
            for (int o = 0; o < 8; o++) acc[o] = wb[K::B2 + o];
#pragma unroll 1
            for (int t = 0; t < 9; t++) {      // (one tap at a time: its 64 weights in SGPRs)
                    const int ky = t / 3, kx = t - 3 * ky, q = (y + ky) * 15 + x + kx;
                    const float4 u0 = ((const float4*)img)[q], u1 = ((const float4*)img)[AKR_IMG + q];
                    const float in[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
#pragma unroll
                    for (int k = 0; k < 8; k++)
#pragma unroll
                        for (int o = 0; o < 8; o++) acc[o] = fmaf(in[k], wb[K::W2 + (t * 8 + k) * 8 + o], acc[o]);
                }
#pragma unroll 1
            for (int k = 0; k < 8; k++) {
                const float b = akr_hs(acc[k]);
#pragma unroll
                for (int o = 0; o < 32; o++) e[o] = fmaf(b, wb[K::WE + (8 * i + k) * 32 + o], e[o]);
            }
        }
        __syncthreads();       // the next player's conv1 overwrites the image
    }

    // ---- proj_p: +c0, Hardswish, depthwise scale + BN, Hardswish; SE over the cells ----
#pragma unroll
    for (int o = 0; o < 32; o++) e[o] = live ? akr_hs(fmaf(akr_hs(e[o] + c0[o]), wp[K::DWS + o], wp[K::DWB + o])) : 0.f;
    {
        // reduce-scatter butterfly: after the xor-32 .. xor-2 steps lane l holds channel 16 b5 + 8 b4 + 4 b3 + 2 b2 + b1 (b = bits of
        // l) summed over the lanes that share those bits; the xor-1 step completes the wave's sum
        float r[32];
#pragma unroll
        for (int o = 0; o < 32; o++) r[o] = e[o];
#pragma unroll
        for (int w = 16; w >= 1; w >>= 1) {
            const bool hi = lane & (2 * w);
#pragma unroll
            for (int j = 0; j < w; j++) {
                const float send = hi ? r[j] : r[j + w], keep = hi ? r[j + w] : r[j];
                r[j] = keep + __shfl_xor(send, 2 * w);
            }
        }
        r[0] += __shfl_xor(r[0], 1);
        if (!(lane & 1))
            red[wave][((lane >> 5) & 1) * 16 + ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1)] = r[0];
    }
    __syncthreads();
    if (tid < 8) {
        float a = wp[K::FC1B + tid];
        for (int k = 0; k < 32; k++) a = fmaf((red[0][k] + red[1][k] + red[2][k]) / (float)AKR_CELLS, wp[K::FC1 + k * 8 + tid], a);
        z[tid] = fmaxf(a, 0.f);
    }
    __syncthreads();
    if (tid < 32) {
        float a = wp[K::FC2B + tid];
#pragma unroll
        for (int k = 0; k < 8; k++) a = fmaf(z[k], wp[K::FC2 + k * 32 + tid], a);
        se[tid] = fminf(fmaxf(a + 3.f, 0.f), 6.f) * (1.f / 6.f);   // Hardsigmoid
    }
    __syncthreads();

    // ---- project (p = (d * se) Wp + bp), then the policy logits of the lane's cell ----
    float p[16];
#pragma unroll
    for (int r = 0; r < 16; r++) p[r] = wp[K::BP + r];
#pragma unroll 4
    for (int k = 0; k < 32; k++) {
        const float dk = e[k] * se[k];
#pragma unroll
        for (int r = 0; r < 16; r++) p[r] = fmaf(dk, wp[K::WP + k * 16 + r], p[r]);
    }
    // the 16-term dot products accumulate in f64 (products of f32 operands, exact in f64): on boards with large heights or scores the
    // logits reach the thousands, and an f32 sum alone puts pi ~3e-5 from the f64 forward
    double pd[16];
#pragma unroll
    for (int r = 0; r < 16; r++) pd[r] = (double)p[r];
    float lg[K::NL];
    float mx = -3.0e38f;
    const uint8_t* va = valid + s * K::A + cell * 6;
#pragma unroll
    for (int c = 0; c < CS; c++)
#pragma unroll
        for (int o = 0; o < 6; o++) {
            const float4* w4 = (const float4*)(wc + c * 96 + o * 16);
            double a = 0.0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float4 w = w4[q];
                a = fma(pd[4 * q], (double)w.x, a), a = fma(pd[4 * q + 1], (double)w.y, a);
                a = fma(pd[4 * q + 2], (double)w.z, a), a = fma(pd[4 * q + 3], (double)w.w, a);
            }
            lg[c * 6 + o] = live ? (va[c * 1014 + o] ? (float)a : -1e8f) : -3.0e38f;
            mx = fmaxf(mx, lg[c * 6 + o]);
        }

    // ---- masked softmax over the workgroup ----
    mx = nn_wave_max(mx);
    if (lane == 0) rmax[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(rmax[0], rmax[1]), rmax[2]);
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < K::NL; j++) {
        lg[j] = live ? expf(lg[j] - mx) : 0.f;
        sum += lg[j];
    }
    sum = nn_wave_sum(sum);
    if (lane == 0) rsum[wave] = sum;
    __syncthreads();
    sum = rsum[0] + rsum[1] + rsum[2];
    // (the kernel's global stores come last: no store precedes a weight load, so the wave-uniform ones go through the scalar cache)
    if (tid < P) {
        float a = wx[K::BV3 + tid];
#pragma unroll
        for (int k = 0; k < 16; k++) a = fmaf(v2[k], wx[K::WV3 + k * P + tid], a);
        v[s * P + tid] = tanhf(a);
    }
    if (live) {
        float* po = pi + s * K::A + tid * 6;
#pragma unroll
        for (int c = 0; c < CS; c++)
#pragma unroll
            for (int o = 0; o < 6; o += 2) *(float2*)(po + c * 1014 + o) = make_float2(lg[c * 6 + o] / sum, lg[c * 6 + o + 1] / sum);
    }
}

}  // namespace azg
