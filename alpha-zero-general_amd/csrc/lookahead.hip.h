// lookahead.hip.h -- every successor of n positions in ONE launch (azg_env_lookahead), and the greedy players' candidate rule on top of
// it (azg_greedy_candidates): <G>Players.GreedyPlayer.play is "for every valid move: getNextState, getScore", a one-ply lookahead.
// One workgroup = one 64-lane wave.  Wave (t, w) of the grid (n, waves_per_state) holds state t and its valid mask in LDS, walks the
// valid actions in index order and takes those whose rank among the valid ones is w modulo waves_per_state: base state -> work buffer
// (LDS to LDS), G::wave_make_move on a fresh Rng, G::game_ended and G::get_score on the work buffer, one output row.  Every candidate
// of a state starts from the same counter of the same stream: the launch is a peek, nothing is advanced or written back.
// LDS: two states (the second with the game's MoveScratch behind it), two masks (game_ended uses the one it is given as scratch).
#pragma once
#include "../../include/azg.h"
#include "game_azul.hip.h"
#include "playout.hip.h"

namespace azg {

template <class G>
__global__ __launch_bounds__(64) void k_env_lookahead(const int8_t* __restrict__ states, const int32_t* __restrict__ players,
                                                      const uint8_t* __restrict__ active, int n, int W, uint64_t rng_seed, uint64_t stream0,
                                                      const uint64_t* __restrict__ counters, uint8_t* __restrict__ out_valid,
                                                      int32_t* __restrict__ out_scores, float* __restrict__ out_ended,
                                                      int32_t* __restrict__ out_next, int8_t* __restrict__ out_states) {
    __shared__ __attribute__((aligned(16))) int8_t base0[G::SP];
    __shared__ __attribute__((aligned(16))) int8_t work0[G::SP + MoveScratch<G>::value];
    __shared__ __attribute__((aligned(16))) uint64_t vmask[G::AW];      // the valid moves of the base state, kept for the whole walk
    __shared__ __attribute__((aligned(16))) uint64_t smask[G::AW];      // game_ended's scratch
    const int t = blockIdx.x, w = blockIdx.y, l = lane_id();            // grid (n, W)
    if (t >= n || w >= W) return;
    if (active && !uni_i32((int)active[t])) return;
    uint32_t off0 = 0;
    asm volatile("" : "+s"(off0));
    int8_t* base = base0 + off0;
    Forest<G>::load_state_unpadded(base, states + (size_t)t * G::S);
    const int cur = players ? ld_agent_i32(players + t) : 0;
    const uint64_t c0 = counters ? ld_agent_u64(counters + t) : 0ull;
    G::valid_mask(base, cur, vmask);
    wave_sync();
    if (w == 0)
        for (int a = l; a < G::A; a += 64) out_valid[(size_t)t * G::A + a] = (uint8_t)((vmask[a >> 6] >> (a & 63)) & 1);
    int rank = 0;                                                       // valid actions in the words walked so far
    for (int wi = 0; wi < G::AW; wi++) {
        const uint64_t mv = playout_mask_word<G>(vmask, wi);
        const uint64_t m = ((uint64_t)uni_u32((uint32_t)(mv >> 32)) << 32) | uni_u32((uint32_t)mv);
        const int c = __popcll(m);
        // the set bits of this word have ranks rank .. rank + c - 1: this wave takes the k-th of them for k = k0, k0 + W, ...
        for (int k = (w + W - rank % W) % W; k < c; k += W) {
            const int a = wi * 64 + ballot_select(m, k);
            // the work buffer's LDS address goes through an empty asm once per candidate, as the state's does once per ply in
            // k_env_playouts (playout.hip.h): nothing derived from it is hoisted out of the walk
            uint32_t off = 0;
            asm volatile("" : "+s"(off));
            int8_t* st = work0 + off;
            wave_sync();                                                // (the previous candidate's reads of the work buffer are done)
            for (int i = l; i < G::SP / 4; i += 64) ((uint32_t*)st)[i] = ((const uint32_t*)base)[i];
            wave_sync();
            Rng rng{rng_seed, stream0 + (uint64_t)t, c0};
            const int np = uni_i32(G::wave_make_move(st, a, cur, 0ll, rng));
            wave_sync();
            const size_t row = (size_t)t * G::A + (size_t)a;
            if (out_states) Forest<G>::store_state_unpadded(out_states + row * G::S, st);
            float es[G::P];
            G::game_ended(st, np, es, smask);
            if (l == 0) {
#pragma unroll
                for (int p = 0; p < G::P; p++) {
                    out_ended[row * G::P + p] = es[p];
                    out_scores[row * G::P + p] = G::get_score(st, p);
                }
                out_next[row] = np;
            }
        }
        rank += c;
    }
}

// ---- the greedy players' candidate sets ---------------------------------------------------------------------------------------
// One wave per canonical position (the mover is seat 0); out[t][a] = 1 where a is a candidate, a position without a valid move gives
// an all-zero row.  The move itself is azg_pick_actions(mode 0, valid = candidates).

// candidates = the valid a of maximal key[a]; KEY(a) is evaluated for valid a only
template <class KEY>
__device__ __forceinline__ void greedy_argmax_rows(const uint8_t* va, int A, uint8_t* out, KEY key) {
    const int l = lane_id();
    long long best = INT64_MIN;
    for (int a = l; a < A; a += 64)
        if (va[a]) { const long long x = key(a); best = x > best ? x : best; }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {                                  // (keys are differences of two i32: 33 bits)
        const long long o = (long long)shfl_xor_u64((uint64_t)best, m);
        best = o > best ? o : best;
    }
    for (int a = l; a < A; a += 64) out[a] = (uint8_t)((va[a] && key(a) == best) ? 1 : 0);
}

// rule AZG_GREEDY_LEAD, any game: key = score[0] - max over p >= 1 of score[p] after the move
__global__ __launch_bounds__(64) void k_greedy_lead(const uint8_t* __restrict__ valid, const int32_t* __restrict__ scores, int n, int A, int P,
                                                    const uint8_t* __restrict__ active, uint8_t* __restrict__ out) {
    const int t = blockIdx.x;
    if (t >= n) return;
    if (active && !uni_i32((int)active[t])) return;
    const int32_t* sc = scores + (size_t)t * A * P;
    greedy_argmax_rows(valid + (size_t)t * A, A, out + (size_t)t * A, [&](int a) {
        long long other = INT64_MIN;
        for (int p = 1; p < P; p++) other = sc[(size_t)a * P + p] > other ? (long long)sc[(size_t)a * P + p] : other;
        return (long long)sc[(size_t)a * P] - (P > 1 ? other : 0ll);
    });
}

// rule AZG_GREEDY_REFERENCE, Abalone (abalone/AbalonePlayers.py:182-206): key = score[1] - score[0] of the un-renumbered successor
__global__ __launch_bounds__(64) void k_greedy_ref_abalone(const uint8_t* __restrict__ valid, const int32_t* __restrict__ scores, int n, int A,
                                                           const uint8_t* __restrict__ active, uint8_t* __restrict__ out) {
    const int t = blockIdx.x;
    if (t >= n) return;
    if (active && !uni_i32((int)active[t])) return;
    const int32_t* sc = scores + (size_t)t * A * 2;
    greedy_argmax_rows(valid + (size_t)t * A, A, out + (size_t)t * A,
                       [&](int a) { return (long long)sc[(size_t)a * 2 + 1] - (long long)sc[(size_t)a * 2]; });
}

// rule AZG_GREEDY_REFERENCE, Splendor (splendor/SplendorPlayers.py:68-90): M = max over the valid moves of seat 1's score after the
// move, init = seat 0's score before it.  M != init: the valid moves that reach M.  Otherwise the valid ids in [0, 12) (buy a visible
// card), else those in [30, 60) (take gems), else every valid id.
template <class G>
__global__ __launch_bounds__(64) void k_greedy_ref_splendor(const int8_t* __restrict__ states, const uint8_t* __restrict__ valid,
                                                            const int32_t* __restrict__ scores, int n, const uint8_t* __restrict__ active,
                                                            uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) int8_t st[G::SP];
    const int t = blockIdx.x, l = lane_id();
    if (t >= n) return;
    if (active && !uni_i32((int)active[t])) return;
    Forest<G>::load_state_unpadded(st, states + (size_t)t * G::S);
    const int init = uni_i32(G::get_score(st, 0));
    const uint8_t* va = valid + (size_t)t * G::A;
    const int32_t* sc = scores + (size_t)t * G::A * G::P;
    uint8_t* o = out + (size_t)t * G::A;
    int best = INT32_MIN, any = 0;
    for (int a = l; a < G::A; a += 64)
        if (va[a]) { const int s = sc[(size_t)a * G::P + 1]; best = s > best ? s : best; any = 1; }
    const int M = wave_max_i32(best);
    if (!wave_max_i32(any)) {
        for (int a = l; a < G::A; a += 64) o[a] = 0;
        return;
    }
    if (M != init) {
        for (int a = l; a < G::A; a += 64) o[a] = (uint8_t)((va[a] && sc[(size_t)a * G::P + 1] == M) ? 1 : 0);
        return;
    }
    int buy = 0, gem = 0;
    for (int a = l; a < G::A; a += 64) {
        buy |= (va[a] && a < 12) ? 1 : 0;
        gem |= (va[a] && a >= 30 && a < 60) ? 1 : 0;
    }
    buy = wave_max_i32(buy);
    gem = wave_max_i32(gem);
    const int lo = buy ? 0 : gem ? 30 : 0, hi = buy ? 12 : gem ? 60 : G::A;
    for (int a = l; a < G::A; a += 64) o[a] = (uint8_t)((va[a] && a >= lo && a < hi) ? 1 : 0);
}

// rule AZG_GREEDY_REFERENCE, Azul (azul/AzulPlayers.py:36-70): no env step, a closed form on the canonical board.  The reference
// scans the valid moves in index order and keeps the first one with the greatest (to_line, -to_floor) -- except that its test
// `if not best_move` is true for best_move == 0 as well as None: a kept move 0 is replaced by the NEXT valid move whatever its key.
// So: the first-index maximum of (to_line, -to_floor) over the valid moves other than 0, and move 0 only when no other move is valid.
__global__ __launch_bounds__(64) void k_greedy_ref_azul(const int8_t* __restrict__ states, const uint8_t* __restrict__ valid, int n,
                                                        const uint8_t* __restrict__ active, uint8_t* __restrict__ out) {
    constexpr int S = AzulDev::S, A = AzulDev::A, COLS = AzulDev::COLS;
    static_assert(AzulDev::R_CENTRE == 3 && AzulDev::R_PROW == 11, "board[3 + move // 30] and board[11][line] of the reference");
    const int t = blockIdx.x, l = lane_id();
    if (t >= n) return;
    if (active && !uni_i32((int)active[t])) return;
    const int8_t* st = states + (size_t)t * S;
    const uint8_t* va = valid + (size_t)t * A;
    int best = INT32_MIN;                                             // (to_line, -to_floor, -index) packed: one integer maximum
    for (int a = l; a < A; a += 64) {
        if (a == 0 || !va[a]) continue;
        const int colour = (a % 30) / 6, line = a % 6;
        const int num_tiles = st[(3 + a / 30) * COLS + colour];
        int to_line = 0, to_floor = num_tiles;
        if (line != 5) {
            const int room = line + 1 - st[11 * COLS + line];
            to_line = room < num_tiles ? room : num_tiles;
            to_floor = num_tiles - to_line;
        }
        const int key = ((to_line + 256) << 20) | ((511 - (to_floor + 256)) << 8) | (255 - a);      // int8 inputs: every field in range
        best = key > best ? key : best;
    }
    best = wave_max_i32(best);
    const int pick = best != INT32_MIN ? 255 - (best & 255) : (va[0] ? 0 : -1);
    for (int a = l; a < A; a += 64) out[(size_t)t * A + a] = (uint8_t)(a == pick ? 1 : 0);
}

}  // namespace azg
