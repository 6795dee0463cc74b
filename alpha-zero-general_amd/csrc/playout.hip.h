// playout.hip.h -- random playouts to the end of the game in ONE launch (azg_env_playouts): <G>Players.RandomPlayer.play looped by
// Arena.playGame (Arena.py:67-84), launcher.py's random play, and the leaf value of a search without a net (nnet.RolloutEvaluator).
// One workgroup = one 64-lane wave = one playout; the state and the valid mask stay in LDS from the first ply to the last, exactly as
// k_env_next_state and k_env_valid_moves hold them, and the only global traffic inside the ply loop is the optional action trace.
// Row r = t * k + j is playout j of input state t and draws from the counter stream (rng_seed, stream0 + r): the move pick takes one
// uniform, the env step (dice, refills, card draws) continues on the same stream.  A ply is game_ended -> cap -> valid_mask -> pick ->
// wave_make_move, which is what the ply-by-ply loop over azg_env_game_ended / azg_env_valid_moves / azg_pick_actions(mode 0) /
// azg_env_next_state computes when its pick and its env step share (stream0, counters).
#pragma once
#include "pick.hip.h"

namespace azg {

#define AZG_PLAYOUT_ENDED 0     /* the game ended: out_ended holds getGameEnded(final board, final player) */
#define AZG_PLAYOUT_CAP 1       /* max_plies moves were played and the game goes on: out_ended is all zeros */
#define AZG_PLAYOUT_STUCK 2     /* the player to move has no valid action in a game that has not ended: out_ended is all zeros */

// inclusive prefix sum of an i32 over the lanes of the wave, in lane order
__device__ __forceinline__ int wave_scan_i32(int x) {
    const int l = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(x, d, 64);
        x = l >= d ? x + o : x;
    }
    return x;
}

// word w of the LDS valid mask with the bits from A on cleared
template <class G>
__device__ __forceinline__ uint64_t playout_mask_word(const uint64_t* mask, int w) {
    const uint64_t m = mask[w];
    if ((G::A & 63) != 0 && w == G::AW - 1) return m & ((1ull << (G::A & 63)) - 1ull);
    return m;
}

template <class G>
__global__ __launch_bounds__(64) void k_env_playouts(const int8_t* __restrict__ states, const int32_t* __restrict__ players,
                                                     const uint8_t* __restrict__ active, int n, int k, int max_plies, uint64_t rng_seed,
                                                     uint64_t stream0, uint64_t* counters, float* __restrict__ out_ended,
                                                     int32_t* __restrict__ out_plies, uint8_t* __restrict__ out_status,
                                                     int8_t* __restrict__ out_states, int32_t* __restrict__ out_players,
                                                     int32_t* __restrict__ out_actions) {
    __shared__ __attribute__((aligned(16))) int8_t st0[G::SP + MoveScratch<G>::value];
    __shared__ __attribute__((aligned(16))) uint64_t mask[G::AW];
    const size_t r = blockIdx.x;
    const int t = (int)(r / (size_t)k), l = lane_id();
    if (t >= n) return;
    if (active && !uni_i32((int)active[t])) return;
    Forest<G>::load_state_unpadded(st0, states + (size_t)t * G::S);
    int cur = players ? ld_agent_i32(players + t) : 0;
    Rng rng{rng_seed, stream0 + (uint64_t)r, counters ? ld_agent_u64(counters + r) : 0ull};
    float es[G::P];
    int plies = 0, status = AZG_PLAYOUT_ENDED;
    for (;;) {
        // The state's LDS address goes through an empty asm once per ply (an offset of zero the compiler cannot see through): it stays an LDS
        // address, but nothing derived from it is hoisted out of the ply loop.  Without this hipcc fails on SmallworldDev<3> and <4> with
        // "Illegal instruction detected: V_CMP_NE_U32_e32 0, $src_shared_base" -- the null test of a pointer into the state
        // (ppl_owner_of) on the loop-invariant generic form of the address.  The single-ply env kernels never hit it.
        uint32_t off = 0;
        asm volatile("" : "+s"(off));
        int8_t* st = st0 + off;
        G::game_ended(st, cur, es, mask);
        int over = 0;
#pragma unroll
        for (int p = 0; p < G::P; p++) over |= es[p] != 0.f ? 1 : 0;
        if (uni_i32(over)) break;
        if (plies >= max_plies) { status = AZG_PLAYOUT_CAP; break; }
        wave_sync();                                                   // (game_ended may have used the mask as its scratch)
        G::valid_mask(st, cur, mask);
        wave_sync();
        // lane l counts the words l, l + 64, ... of the mask; the pick walks the words in index order, 64 at a time
        int cnt = 0;
        for (int w = l; w < G::AW; w += 64) cnt += __popcll(playout_mask_word<G>(mask, w));
        const int nv = wave_sum_i32(cnt);
        if (nv == 0) { status = AZG_PLAYOUT_STUCK; break; }
        const double u = rng.u01();                                    // exactly one draw per picked move
        int kth = (int)(u * (double)nv);                               // the kth valid action in index order (k_pick_actions, mode 0)
        kth = kth > nv - 1 ? nv - 1 : kth;
        int action = 0;
        for (int base = 0; base < G::AW; base += 64) {
            const int w = base + l;
            const int c = w < G::AW ? __popcll(playout_mask_word<G>(mask, w)) : 0;
            const int incl = wave_scan_i32(c);
            const int tot = __shfl(incl, 63, 64);
            if (kth < tot) {
                const int src = first_lane(__ballot(incl > kth));      // the word that holds the kth set bit
                const int rank = kth - (__shfl(incl, src, 64) - __shfl(c, src, 64));
                action = (base + src) * 64 + ballot_select(playout_mask_word<G>(mask, base + src), rank);
                break;
            }
            kth -= tot;
        }
        action = uni_i32(action);
        if (out_actions && l == 0) out_actions[r * (size_t)max_plies + (size_t)plies] = action;
        wave_sync();                                                   // (every lane has read the mask before the step may reuse LDS)
        cur = uni_i32(G::wave_make_move(st, action, cur, 0ll, rng));
        rng.counter = ((uint64_t)uni_u32((uint32_t)(rng.counter >> 32)) << 32) | uni_u32((uint32_t)rng.counter);
        plies++;
    }
    if (l == 0) {
        if (counters) counters[r] = rng.counter;
#pragma unroll
        for (int p = 0; p < G::P; p++) out_ended[r * G::P + p] = status == AZG_PLAYOUT_ENDED ? es[p] : 0.f;
        out_plies[r] = plies;
        out_status[r] = (uint8_t)status;
        if (out_players) out_players[r] = cur;
    }
    if (out_states) Forest<G>::store_state_unpadded(out_states + r * G::S, st0);
}

}  // namespace azg
