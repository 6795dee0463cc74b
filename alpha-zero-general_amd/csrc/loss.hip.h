// loss.hip.h -- the validation losses of GenericNNetWrapper.evaluate (:159-177, loss_pi / loss_v :179-190) on the outputs of an engine
// net: the nets return PROBABILITIES where the torch losses want log-probabilities, and a validation set is tens of thousands of rows.
// k_eval_losses: one 64-lane wave per example row, A and P run-time arguments, lane l takes actions l, l + 64, ... (one coalesced
// request per 64 entries), no LDS.  Logs and sums are f64; every lane sums its own entries in index order and the lanes are combined in
// one fixed xor tree, so a row's numbers are the same bits in every call and for every B.  k_eval_totals: ONE wave that sums the rows
// (lane l takes rows l, l + 64, ... in order, then the same tree) -- no ticket, no atomics: the totals are as reproducible as the rows.
#pragma once
#include <float.h>

#include "azg_common.hip.h"

namespace azg {

// sum of an f64 over the wave, the same bits in every lane (an f64 add commutes, so both sides of every xor step compute the same sum)
__device__ __forceinline__ double wave_tree_sum_f64(double x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += shfl_xor_f64(x, m);
    return x;
}

// first index of the maximum over the wave of the lanes' (value, index) candidates; idx < 0 = the lane has none
__device__ __forceinline__ int wave_first_argmax_f32(float best, int idx) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ob = __shfl_xor(best, m, 64);
        const int oi = __shfl_xor(idx, m, 64);
        const bool take = oi >= 0 && (idx < 0 || ob > best || (ob == best && oi < idx));
        best = take ? ob : best;
        idx = take ? oi : idx;
    }
    return uni_i32(idx);
}

// rows[b] = { sum_a t (log t - log max(pi, FLT_MIN)) over the actions with t > 0 (F.kl_div's xlogy convention: t == 0 adds exactly 0,
//             whatever pi is),  sum_p ((z + q_weight q) / (1 + q_weight) - v)^2 }
// flags[b] = { first-index argmax of target_pi == first-index argmax of pi (np.argmax; a NaN never wins),
//              the number of actions with t > 0 and pi < FLT_MIN: where the floor was applied }
// a row with active == 0 writes zeros.  P <= 8 (checked by the caller): lane p holds player p's squared error.
__global__ __launch_bounds__(64) void k_eval_losses(const float* __restrict__ pi, const float* __restrict__ v,
                                                    const float* __restrict__ target_pi, const float* __restrict__ z,
                                                    const float* __restrict__ q, const uint8_t* __restrict__ active, int B, int A, int P,
                                                    float q_weight, double* __restrict__ rows, int32_t* __restrict__ flags) {
    const int b = blockIdx.x, l = lane_id();
    if (b >= B) return;
    if (active && !uni_i32((int)active[b])) {
        if (l == 0) { rows[2 * (size_t)b] = 0.0; rows[2 * (size_t)b + 1] = 0.0; flags[2 * (size_t)b] = 0; flags[2 * (size_t)b + 1] = 0; }
        return;
    }
    const float* p = pi + (size_t)b * A;
    const float* t = target_pi + (size_t)b * A;
    double kl = 0.0;
    int floored = 0, ti = -1, pj = -1;
    float tbest = 0.f, pbest = 0.f;
    for (int a = l; a < A; a += 64) {
        const float ta = t[a], pa = p[a];
        if (ta == ta && (ti < 0 || ta > tbest)) { tbest = ta; ti = a; }
        if (pa == pa && (pj < 0 || pa > pbest)) { pbest = pa; pj = a; }
        if (ta > 0.f) {
            const bool low = pa < FLT_MIN;
            floored += low ? 1 : 0;
            kl += (double)ta * (log((double)ta) - log((double)(low ? FLT_MIN : pa)));
        }
    }
    kl = wave_tree_sum_f64(kl);
    floored = wave_sum_i32(floored);
    const int top1 = wave_first_argmax_f32(tbest, ti) == wave_first_argmax_f32(pbest, pj) ? 1 : 0;
    double se = 0.0;
    if (l < P) {
        const size_t i = (size_t)b * P + l;
        const double d = ((double)z[i] + (double)q_weight * (double)q[i]) / (1.0 + (double)q_weight) - (double)v[i];
        se = d * d;
    }
    se = wave_tree_sum_f64(se);
    if (l == 0) { rows[2 * (size_t)b] = kl; rows[2 * (size_t)b + 1] = se; flags[2 * (size_t)b] = top1; flags[2 * (size_t)b + 1] = floored; }
}

// totals[0..3] (+)= the sums over the B rows of rows[:, 0], rows[:, 1], flags[:, 0], flags[:, 1] (the counts are exact in f64 below
// 2^53).  One wave; inactive rows hold zeros.  B == 0 writes (or keeps) the totals alone.
__global__ __launch_bounds__(64) void k_eval_totals(const double* __restrict__ rows, const int32_t* __restrict__ flags, int B, int accumulate,
                                                    double* __restrict__ totals) {
    const int l = lane_id();
    double s0 = 0.0, s1 = 0.0, c0 = 0.0, c1 = 0.0;
#pragma unroll 4
    for (int b = l; b < B; b += 64) {
        s0 += rows[2 * (size_t)b];
        s1 += rows[2 * (size_t)b + 1];
        c0 += (double)flags[2 * (size_t)b];
        c1 += (double)flags[2 * (size_t)b + 1];
    }
    s0 = wave_tree_sum_f64(s0);
    s1 = wave_tree_sum_f64(s1);
    c0 = wave_tree_sum_f64(c0);
    c1 = wave_tree_sum_f64(c1);
    if (l < 4) {
        const double s = l == 0 ? s0 : l == 1 ? s1 : l == 2 ? c0 : c1;
        totals[l] = accumulate ? totals[l] + s : s;
    }
}

}  // namespace azg
