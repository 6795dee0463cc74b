// pick.hip.h -- one move per game from a row of A entries, without a search: the baseline contestants of arena.py (the reference's
// <G>Players.RandomPlayer.play and pit.py's raw-policy players) and the argmax that ends an Arena ply (Arena.py:79, np.argmax).
// One 64-lane wave per game, no LDS.  A is a run-time argument: one kernel per mode serves every game.  Rows are read lane-strided
// (lane l reads entries l, l + 64, ...: one coalesced request per 64 entries); "index order" over such a row is chunk by chunk of 64,
// a ballot or a wave scan inside the chunk.
#pragma once
#include "forest.hip.h"

namespace azg {

#define AZG_PICK_UNIFORM 0   /* uniform among the valid actions */
#define AZG_PICK_ARGMAX 1    /* first index of the maximum of probs over the valid actions */
#define AZG_PICK_SAMPLE 2    /* proportionally to probs over the valid actions */

// sum of an f64 over the wave, wave-uniform (the DPP butterfly of wave_sum_u64 with an f64 add)
__device__ __forceinline__ double wave_sum_f64(double x) {
    uint64_t v = (uint64_t)__double_as_longlong(x);
#define AZG_OP_FADD(a, b) ((uint64_t)__double_as_longlong(__longlong_as_double((long long)(a)) + __longlong_as_double((long long)(b))))
    AZG_DPP_REDUCE_U64(v, AZG_OP_FADD);
#undef AZG_OP_FADD
    const double a = __longlong_as_double((long long)readlane_u64(v, 0)), b = __longlong_as_double((long long)readlane_u64(v, 16));
    const double c = __longlong_as_double((long long)readlane_u64(v, 32)), d = __longlong_as_double((long long)readlane_u64(v, 48));
    return (a + b) + (c + d);
}
// inclusive prefix sum of an f64 over the lanes of the wave, in lane order
__device__ __forceinline__ double wave_scan_f64(double x) {
    const int l = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t u = (uint64_t)__double_as_longlong(x);
        const uint32_t lo = __shfl_up((uint32_t)u, d, 64), hi = __shfl_up((uint32_t)(u >> 32), d, 64);
        const double o = __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
        x = l >= d ? x + o : x;
    }
    return x;
}
// the lane whose set bit of `ballot` has rank k (k < popcount(ballot)), wave-uniform
__device__ __forceinline__ int ballot_select(uint64_t ballot, int k) {
    const int l = lane_id();
    const int below = __popcll(ballot & ((1ull << l) - 1ull));
    return first_lane(__ballot(((ballot >> l) & 1ull) && below == k));
}

// weight of entry a in the sampling mode: its probability when the action is valid and the probability is positive, else nothing (a NaN too)
__device__ __forceinline__ double pick_weight(const float* p, const uint8_t* va, int a, int A) {
    if (a >= A || (va && !va[a])) return 0.0;
    const float x = p[a];
    return x > 0.f ? (double)x : 0.0;
}

template <int MODE>
__global__ __launch_bounds__(64) void k_pick_actions(const float* __restrict__ probs, const uint8_t* __restrict__ valid, int T, int A,
                                                     const uint8_t* __restrict__ active, uint64_t rng_seed, uint64_t stream0,
                                                     uint64_t* counters, int32_t* __restrict__ actions_out) {
    const int t = blockIdx.x, l = lane_id();
    if (t >= T) return;
    if (active && !uni_i32((int)active[t])) return;
    const uint8_t* va = valid ? valid + (size_t)t * A : nullptr;
    const float* p = probs ? probs + (size_t)t * A : nullptr;
    int pick = 0;
    if constexpr (MODE == AZG_PICK_ARGMAX) {
        // np.argmax over the valid entries: every lane keeps the first maximum of its own entries (ascending, strict '>': a NaN is
        // never greater), the wave the maximum with the lowest index; no candidate at all (all-NaN, all-invalid) -> 0
        float best = 0.f;
        int idx = -1;
        for (int a = l; a < A; a += 64) {
            const float x = p[a];
            const bool ok = (!va || va[a]) && x == x;
            if (ok && (idx < 0 || x > best)) { best = x; idx = a; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ob = __shfl_xor(best, m, 64);
            const int oi = __shfl_xor(idx, m, 64);
            const bool take = oi >= 0 && (idx < 0 || ob > best || (ob == best && oi < idx));
            best = take ? ob : best;
            idx = take ? oi : idx;
        }
        pick = uni_i32(idx) < 0 ? 0 : uni_i32(idx);
    } else {
        const uint64_t c0 = counters ? ld_agent_u64(counters + t) : 0ull;
        Rng rng{rng_seed, stream0 + (uint64_t)t, c0};
        const double u = rng.u01();                                    // exactly one draw per picked move, valid actions or not
        if (l == 0 && counters) counters[t] = c0 + 1ull;
        if constexpr (MODE == AZG_PICK_UNIFORM) {
            int cnt = 0;
            for (int a = l; a < A; a += 64) cnt += (!va || va[a]) ? 1 : 0;
            const int nv = wave_sum_i32(cnt);
            if (nv > 0) {
                int k = (int)(u * (double)nv);                         // the k-th valid action in index order
                k = k > nv - 1 ? nv - 1 : k;
                for (int base = 0; base < A; base += 64) {
                    const int a = base + l;
                    const uint64_t b = __ballot(a < A && (!va || va[a]));
                    const int c = __popcll(b);
                    if (k < c) { pick = base + ballot_select(b, k); break; }
                    k -= c;
                }
            }
        } else {
            // np.random.choice(A, p=pi): the first index whose cumulative weight (f64, index order) exceeds u * total.  The total is the wave
            // sum of the lanes' partial sums; the walk adds whole chunks of 64 until the target falls into one and scans that chunk.  The two
            // sums round differently, so a target in the last ulps of the total can fall off the end: then the last valid index
            double part = 0.0;
            int last = -1;
            for (int a = l; a < A; a += 64) {
                part += pick_weight(p, va, a, A);
                if (!va || va[a]) last = a;
            }
            const double target = u * wave_sum_f64(part);
            last = wave_max_i32(last);
            pick = last < 0 ? 0 : last;
            if (last >= 0) {
                double carry = 0.0;
                for (int base = 0; base <= last; base += 64) {
                    const double w = pick_weight(p, va, base + l, A);
                    const double tot = wave_sum_f64(w);
                    if (carry + tot > target) {
                        const double cum = carry + wave_scan_f64(w);             // (every lane takes part in the scan: not behind the &&)
                        const uint64_t b = __ballot(w > 0.0 && cum > target);
                        if (b) { pick = base + first_lane(b); break; }
                    }
                    carry += tot;
                }
            }
        }
    }
    if (l == 0) actions_out[t] = pick;
}

}  // namespace azg
