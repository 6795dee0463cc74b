// azg_nn.hip -- C-ABI (include/azg.h) of the policy/value net kernels: host-side launch code (NeuralNet.predict for a whole
// leaf batch).  Second translation unit of libazg_hip.so; compiled with the default flags (the forest unit, azg.hip, forbids
// scalarised global loads, see build.py).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

// this unit also holds the per-CU round kernel (azg_fused.hip.h, included at the end): its workgroups run 16 independent tree waves, so
// wave_sync() must be a wavefront fence here (the net kernels synchronise with __syncthreads() directly and are not affected)
#define AZG_WAVE_LOCAL_SYNC 1
#include "../../include/azg.h"
#include "azg_host.h"
#include "azg_common.hip.h"
#include "nn_kernels.hip.h"
#include "nn_v80_h2.hip.h"
#include "nn_mb1d.hip.h"
#include "nn_conv5x5.hip.h"
#include "nn_abalone.hip.h"
#include "nn_smallworld.hip.h"
#include "nn_akropolis.hip.h"
#include "nn_botanik.hip.h"

using namespace azg;

// ---- the V80 forward on f32 / bf16 x 3 operands, one launch (nn_kernels.hip.h; NeuralNet.predict, GenericNNetWrapper.py:94-120; V80: SplendorNNet.py:262-283) ----
static int v80_forward(const int8_t* boards, const uint8_t* valid, const float* const* w /* 43 */, int B,
                       int P, float* pi, float* v, void* stream, bool split) {
    if (!boards || !valid || !w || !pi || !v || B <= 0) return fail("azg_nn_v80_forward: null/empty argument");
    if (P < 2 || P > 4) return fail("azg_nn_v80_forward: 2 <= P <= 4");
    V80BlockW Wt{w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12]};
    V80BlockW Wp{w[13], w[14], w[15], w[16], w[17], w[18], w[19], w[20], w[21], w[22], w[23]};
    V80BlockW Wv{w[24], w[25], w[26], w[27], w[28], w[29], w[30], w[31], w[32], w[33], w[34]};
    V80NetW N0{w[0], w[1], nullptr, nullptr, nullptr, nullptr};
    V80NetW Np{nullptr, nullptr, w[35], w[36], w[37], w[38]};
    V80NetW Nv{nullptr, nullptr, w[39], w[40], w[41], w[42]};
    hipStream_t s = (hipStream_t)stream;
    // V80 geometry (SplendorNNet.py:262-283): trunk ReLU + mean-SE, both heads Hardswish + max-SE
    if (split) return launch_lds<k_v80_net_spx>(dim3((B + 15) / 16), dim3(768), V80_SPX_LDS, s, Wt, Wp, Wv, N0, Np, Nv, boards, valid, B, P, pi, v);
    return launch_lds<k_v80_net>(dim3((B + 15) / 16), dim3(768), V80_NET_LDS, s, Wt, Wp, Wv, N0, Np, Nv, boards, valid, B, P, pi, v);
}


extern "C" int azg_nn_v80_forward(const int8_t* boards, const uint8_t* valid, const float* const* w /* 43 */, int B,
                                  int P, float* pi, float* v, void* stream) {
    return v80_forward(boards, valid, w, B, P, pi, v, stream, false);
}

extern "C" int azg_nn_v80_forward_split(const int8_t* boards, const uint8_t* valid, const float* const* w /* 43 */, int B,
                                        int P, float* pi, float* v, void* stream) {
    return v80_forward(boards, valid, w, B, P, pi, v, stream, true);
}

// The V80 forward on fp16 hi+lo split operands with token-major tiles (nn_v80_h2.hip.h): one launch, one workgroup per 16 samples
extern "C" int azg_nn_v80_forward_h2(const int8_t* boards, const uint8_t* valid, const void* const* w /* 43 */,
                                     const float* descale /* 16, host */, int B, int P, float* pi, float* v, void* stream) {
    if (!boards || !valid || !w || !descale || !pi || !v || B <= 0) return fail("azg_nn_v80_forward_h2: null/empty argument");
    if (P < 2 || P > 4) return fail("azg_nn_v80_forward_h2: 2 <= P <= 4");
    const H2Weights HW = h2_weights(w, descale);
    hipStream_t s = (hipStream_t)stream;
    // AZG_V80_WAVES=16: the 16-wave / 128-VGPR variant (the form the fused round kernel uses); default 12
    static const int waves_h2 = (getenv("AZG_V80_WAVES") && atoi(getenv("AZG_V80_WAVES")) == 16) ? 16 : 12;
    if (waves_h2 == 16) return launch_lds<k_v80_net_h2<16>>(dim3((B + 15) / 16), dim3(1024), H2_LDS, s, HW, boards, valid, B, P, pi, v);
    return launch_lds<k_v80_net_h2<12>>(dim3((B + 15) / 16), dim3(768), H2_LDS, s, HW, boards, valid, B, P, pi, v);
}

#ifdef AZG_NN_PHASE_TIMES
extern "C" int azg_nn_debug_phase_times(long long* out /* [4][16] */) {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_v80_phase), sizeof(long long) * 64));
    return 0;
}
extern "C" int azg_nn_debug_phase_times_c5(long long* out /* [32] */) {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_c5_phase), sizeof(long long) * 32));
    HIPCHK(hipMemcpyFromSymbol(out + 28, HIP_SYMBOL(g_c5_first), sizeof(long long) * 3));      // stamps inside the first convolution
    return 0;
}
extern "C" int azg_nn_debug_phase_times_h2(long long* out /* [4][16] */) {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_h2_phase), sizeof(long long) * 64));
    return 0;
}
#endif

// ---- whole MobileNet-1d forward, any supported geometry, one launch (nn_mb1d.hip.h) ----
// (the geometries CfgSplendor2 / 3 / 4, CfgAzul, CfgMinivilles2 / 3 / 4, CfgTLP3 / 4 / 5: nn_mb1d.hip.h)

template <class CF, bool H2>
static int launch_mb1d(const Mb1dNetW& N, const int8_t* boards, const uint8_t* valid, int B, float* pi, float* v, hipStream_t s) {
    constexpr size_t lds = (size_t)CF::LDS_FLOATS * sizeof(float);
    static_assert(lds <= 160 * 1024, "geometry does not fit the LDS of a CU");
    return launch_lds<k_mb1d_net<CF, H2>>(dim3((B + CF::NS - 1) / CF::NS), dim3(768), lds, s, N, boards, valid, B, pi, v);
}

template <bool H2>
static int mb1d_forward(int geometry, const int8_t* boards, const uint8_t* valid, const float* const* w, const float* descale,
                        int B, float* pi, float* v, void* stream) {
    if (!boards || !valid || !w || !pi || !v || B <= 0 || (H2 && !descale)) return fail("azg_nn_mb1d_forward: null/empty argument");
    Mb1dNetW N;
    for (int i = 0; i < 16; i++) N.ds[i] = H2 ? descale[i] : 1.f;
    N.W0 = w[0]; N.b0 = w[1];
    for (int b = 0; b < 3; b++) {
        const float* const* q = w + 2 + 11 * b;
        N.blk[b] = Mb1dBlockW{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10]};
    }
    const float* const* h = w + 35;
    N.Wpi1 = h[0]; N.bpi1 = h[1]; N.Wpi2 = h[2]; N.bpi2 = h[3]; N.Wv1 = h[4]; N.bv1 = h[5]; N.Wv2 = h[6]; N.bv2 = h[7];
    hipStream_t s = (hipStream_t)stream;
    switch (geometry) {
        case AZG_NET_SPLENDOR2: return launch_mb1d<CfgSplendor2, H2>(N, boards, valid, B, pi, v, s);
        case AZG_NET_SPLENDOR3: return launch_mb1d<CfgSplendor3, H2>(N, boards, valid, B, pi, v, s);
        case AZG_NET_SPLENDOR4: return launch_mb1d<CfgSplendor4, H2>(N, boards, valid, B, pi, v, s);
        case AZG_NET_AZUL: return launch_mb1d<CfgAzul, H2>(N, boards, valid, B, pi, v, s);
        case AZG_NET_MINIVILLES2: return launch_mb1d<CfgMinivilles2, H2>(N, boards, valid, B, pi, v, s);
        case AZG_NET_TLP3: return launch_mb1d<CfgTLP3, H2>(N, boards, valid, B, pi, v, s);
        case AZG_NET_MINIVILLES3: return launch_mb1d<CfgMinivilles3, H2>(N, boards, valid, B, pi, v, s);
        case AZG_NET_MINIVILLES4: return launch_mb1d<CfgMinivilles4, H2>(N, boards, valid, B, pi, v, s);
        case AZG_NET_TLP4: return launch_mb1d<CfgTLP4, H2>(N, boards, valid, B, pi, v, s);
        case AZG_NET_TLP5: return launch_mb1d<CfgTLP5, H2>(N, boards, valid, B, pi, v, s);
        default: return fail("azg_nn_mb1d_forward: unknown geometry");
    }
}

extern "C" int azg_nn_mb1d_forward(int geometry, const int8_t* boards, const uint8_t* valid, const float* const* w, int B,
                                   float* pi, float* v, void* stream) {
    return mb1d_forward<false>(geometry, boards, valid, w, nullptr, B, pi, v, stream);
}

// the same forward with the GEMM phases on f16 x 2 split-precision operands: matrices as h2 fragments, descale[16] on the host
extern "C" int azg_nn_mb1d_forward_h2(int geometry, const int8_t* boards, const uint8_t* valid, const void* const* w,
                                      const float* descale, int B, float* pi, float* v, void* stream) {
    return mb1d_forward<true>(geometry, boards, valid, (const float* const*)w, descale, B, pi, v, stream);
}

// ---- Santorini ResNet V88/V89 (no-gods geometry: A = 162, P = 2, 5 residual blocks), one launch (nn_conv5x5.hip.h) ----
static int conv5_launch(const int8_t* boards, const uint8_t* valid, const float* const* w, int n_blocks, int A, int P, int B,
                        float* pi, float* v, void* stream, int split /* 0 f32, 3 bf16 x 3, 2 f16 x 2 */, float descale = 1.f) {
    if (!boards || !valid || !w || !pi || !v || B <= 0) return fail("azg_nn_conv5_forward: null/empty argument");
    if (n_blocks != 5 || A != 162 || P != 2) return fail("azg_nn_conv5_forward: built for 5 residual blocks, A = 162, P = 2");
    Conv5NetW N{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12], w[13]};
    const dim3 grid((B + 7) / 8), block(768);
    hipStream_t s = (hipStream_t)stream;
    if (split == 2) return launch_lds<k_conv5_net<5, 162, 2, 2>>(grid, block, C5_LDS_H2, s, N, boards, valid, B, pi, v, descale);
    if (split) return launch_lds<k_conv5_net<5, 162, 2, 3>>(grid, block, C5_LDS_BF16X3, s, N, boards, valid, B, pi, v, 1.f);
    return launch_lds<k_conv5_net<5, 162, 2, 0>>(grid, block, C5_LDS_F32, s, N, boards, valid, B, pi, v, 1.f);
}

extern "C" int azg_nn_conv5_forward(const int8_t* boards, const uint8_t* valid, const float* const* w, int n_blocks, int A,
                                    int P, int B, float* pi, float* v, void* stream) {
    return conv5_launch(boards, valid, w, n_blocks, A, P, B, pi, v, stream, 0);
}

extern "C" int azg_nn_conv5_forward_split(const int8_t* boards, const uint8_t* valid, const float* const* w, int n_blocks, int A,
                                          int P, int B, float* pi, float* v, void* stream) {
    return conv5_launch(boards, valid, w, n_blocks, A, P, B, pi, v, stream, 3);
}

extern "C" int azg_nn_conv5_forward_h2(const int8_t* boards, const uint8_t* valid, const float* const* w, float descale, int n_blocks,
                                       int A, int P, int B, float* pi, float* v, void* stream) {
    return conv5_launch(boards, valid, w, n_blocks, A, P, B, pi, v, stream, 2, descale);
}

// ---- Santorini-with-gods net V78 (10 InvertedResidual blocks, A = 1782, P = 2): trunk + value head, then the policy FC (nn_conv5x5.hip.h) ----
static int s78_launch(const int8_t* boards, const uint8_t* valid, const float* const* w, int n_blocks, int A, int P, int B, float* pi,
                      float* v, void* stream, int split /* 0 f32, 3 bf16 x 3, 2 f16 x 2 */, float ds_e = 1.f, float ds_p = 1.f,
                      float* logits_ws = nullptr /* f16 x 2: non-null = the two-launch policy FC */) {
    if (!boards || !valid || !w || !pi || !v || B <= 0) return fail("azg_nn_s78_forward: null/empty argument");
    if (n_blocks != 10 || A != 1782 || P != 2) return fail("azg_nn_s78_forward: built for 10 blocks, A = 1782, P = 2");
    S78NetW N{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12], w[13], w[14], w[15], w[16], w[17], w[18]};
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(768), grid16((B + 15) / 16);
    if (split == 2) {
        if (launch_lds<k_s78_net_split<10, 1782, 2, 2>>(dim3((B + 7) / 8), block, S78_LDS_H2, s, N, boards, valid, B, pi, v, ds_e, ds_p)) return -1;
    } else if (split) {
        if (launch_lds<k_s78_net_split<10, 1782, 2, 3>>(dim3((B + 7) / 8), block, S78_LDS_BF16X3, s, N, boards, valid, B, pi, v, 1.f, 1.f)) return -1;
    } else {
        if (launch_lds<k_s78_net<10, 1782, 2>>(dim3((B + 3) / 4), block, S78_LDS_F32, s, N, boards, valid, B, pi, v)) return -1;
    }
    if (split != 2) return launch_lds<k_s78_policy<1782, 132>>(grid16, block, S78_POLICY_LDS, s, N.Wfp, N.bfp, valid, B, pi);
    // the policy FC on f16 x 2 operands as well (w[11] then holds its hi / lo fragments + the descale): in one launch, or -- with the caller's
    // workspace for the raw logits [B][1792] (the pi rows hold the policy features until every column quarter has read them) -- in two: 64
    // samples x a quarter of the columns per workgroup, then the softmax
    if (!logits_ws) return launch_lds<k_s78_policy_h2<1782, 132>>(grid16, block, S78_POLICY_H2_LDS, s, (const uint4*)N.Wfp, N.bfp, valid, B, pi);
    if (launch_lds<k_s78_policy_gemm_h2<1782, 132>>(dim3((B + 63) / 64, 4), block, S78_POLICY_GEMM_LDS, s, (const uint4*)N.Wfp, N.bfp, B, pi, logits_ws)) return -1;
    return launch_lds<k_s78_policy_softmax<1782>>(dim3((B + 3) / 4), dim3(256), 0, s, logits_ws, valid, B, pi);
}

extern "C" int azg_nn_s78_forward(const int8_t* boards, const uint8_t* valid, const float* const* w, int n_blocks, int A, int P,
                                  int B, float* pi, float* v, void* stream) {
    return s78_launch(boards, valid, w, n_blocks, A, P, B, pi, v, stream, 0);
}

extern "C" int azg_nn_s78_forward_split(const int8_t* boards, const uint8_t* valid, const float* const* w, int n_blocks, int A, int P,
                                        int B, float* pi, float* v, void* stream) {
    return s78_launch(boards, valid, w, n_blocks, A, P, B, pi, v, stream, 3);
}

extern "C" int azg_nn_s78_forward_h2(const int8_t* boards, const uint8_t* valid, const float* const* w, float ds_e, float ds_p, int n_blocks,
                                     int A, int P, int B, float* pi, float* v, float* logits_ws, void* stream) {
    return s78_launch(boards, valid, w, n_blocks, A, P, B, pi, v, stream, 2, ds_e, ds_p, logits_ws);
}

// ---- Abalone net V21 (4 InvertedResidual blocks on the 9 x 9 grid, A = 3402, P = 2): one launch, 4 samples per workgroup (nn_abalone.hip.h) ----
extern "C" int azg_nn_aba21_forward(const int8_t* boards, const uint8_t* valid, const float* const* w, int n_blocks, int A, int P, int B,
                                    float* pi, float* v, void* stream) {
    if (!boards || !valid || !w || !pi || !v || B <= 0) return fail("azg_nn_aba21_forward: null/empty argument");
    if (n_blocks != 4 || A != ABA_A || P != 2) return fail("azg_nn_aba21_forward: built for 4 blocks, A = 3402, P = 2");
    for (int i = 0; i < 16; i++)
        if (!w[i]) return fail("azg_nn_aba21_forward: null weight pointer");
    Aba21NetW N{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12], w[13], w[14], w[15]};
    return launch_lds<k_aba21_net<4, 2>>(dim3((B + ABA_NS - 1) / ABA_NS), dim3(ABA_THREADS), ABA_LDS, (hipStream_t)stream, N, boards, valid, B, pi, v);
}

// ---- Smallworld net V62 (3-layer transformer encoder over the N tokens, P = 2 / 3 / 4): one launch, 4 / 3 / 2 samples per workgroup
// (nn_smallworld.hip.h) ----
extern "C" int azg_nn_sw62_forward(const int8_t* boards, const uint8_t* valid, const float* const* w, int n_layers, int A, int P, int B,
                                   float* pi, float* v, void* stream) {
    if (!boards || !valid || !w || !pi || !v || B <= 0) return fail("azg_nn_sw62_forward: null/empty argument");
    if (n_layers != SW_LAYERS || !((P == 2 && A == Sw62<2>::A) || (P == 3 && A == Sw62<3>::A) || (P == 4 && A == Sw62<4>::A)))
        return fail("azg_nn_sw62_forward: built for 3 layers and (P, A) = (2, 131), (3, 166) or (4, 211)");
    for (int i = 0; i < SW_NW; i++)
        if (!w[i]) return fail("azg_nn_sw62_forward: null weight pointer");
    Sw62NetW N{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12], w[13], w[14], w[15], w[16], w[17], w[18],
               w[19], w[20], w[21], w[22], w[23], w[24]};
    hipStream_t st = (hipStream_t)stream;
    if (P == 2) k_sw62_net<2><<<dim3((B + Sw62<2>::NS - 1) / Sw62<2>::NS), dim3(SW_THREADS), 0, st>>>(N, boards, valid, B, pi, v);
    else if (P == 3) k_sw62_net<3><<<dim3((B + Sw62<3>::NS - 1) / Sw62<3>::NS), dim3(SW_THREADS), 0, st>>>(N, boards, valid, B, pi, v);
    else k_sw62_net<4><<<dim3((B + Sw62<4>::NS - 1) / Sw62<4>::NS), dim3(SW_THREADS), 0, st>>>(N, boards, valid, B, pi, v);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- Akropolis net V31 (board convolutions per player + kernel-1 InvertedResidual + bilinear policy per site tile, P = 2 / 3 / 4): one
// launch, one sample per workgroup (nn_akropolis.hip.h) ----
extern "C" int azg_nn_akr31_forward(const int8_t* boards, const uint8_t* valid, const float* const* w, int P, int A, int B, float* pi,
                                    float* v, void* stream) {
    if (!boards || !valid || !w || !pi || !v || B <= 0) return fail("azg_nn_akr31_forward: null/empty argument");
    if (!((P == 2 && A == Akr31<2>::A) || (P == 3 && A == Akr31<3>::A) || (P == 4 && A == Akr31<4>::A)))
        return fail("azg_nn_akr31_forward: built for (P, A) = (2, 4056), (3, 5070) or (4, 6084)");
    for (int i = 0; i < AKR_NW; i++)
        if (!w[i]) return fail("azg_nn_akr31_forward: null weight pointer");
    hipStream_t st = (hipStream_t)stream;
    if (P == 2) k_akr31_net<2><<<dim3(B), dim3(AKR_THREADS), 0, st>>>(w[0], w[1], w[2], boards, valid, pi, v);
    else if (P == 3) k_akr31_net<3><<<dim3(B), dim3(AKR_THREADS), 0, st>>>(w[0], w[1], w[2], boards, valid, pi, v);
    else k_akr31_net<4><<<dim3(B), dim3(AKR_THREADS), 0, st>>>(w[0], w[1], w[2], boards, valid, pi, v);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- Botanik nets V10 / V11 (1-d branch + 1 or 2 machine branches, A = 428, P = 2): one launch, 8 samples per workgroup (nn_botanik.hip.h) ----
template <int NM>
static int bot_launch(const BotNetW& N, const int8_t* boards, const uint8_t* valid, int B, float* pi, float* v, hipStream_t s) {
    return launch_lds<k_bot_net<NM>>(dim3((B + BOT_NS - 1) / BOT_NS), dim3(BOT_THREADS), BOT_LDS, s, N, boards, valid, B, pi, v);
}

extern "C" int azg_nn_bot_forward(const int8_t* boards, const uint8_t* valid, const float* const* w, int n_mach, int P, int A, int B,
                                  float* pi, float* v, void* stream) {
    if (!boards || !valid || !w || !pi || !v || B <= 0) return fail("azg_nn_bot_forward: null/empty argument");
    if ((n_mach != 1 && n_mach != 2) || P != 2 || A != BOT_A)
        return fail("azg_nn_bot_forward: built for n_mach 1 (nn_version 10) or 2 (nn_version 11), P = 2, A = 428");
    for (int i = 0; i < 10; i++)
        if (!w[i]) return fail("azg_nn_bot_forward: null weight pointer");
    BotNetW N{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9]};
    return n_mach == 1 ? bot_launch<1>(N, boards, valid, B, pi, v, (hipStream_t)stream) : bot_launch<2>(N, boards, valid, B, pi, v, (hipStream_t)stream);
}

#include "azg_fused.hip.h"
