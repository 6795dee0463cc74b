// azg_lookahead.hip -- the one-ply lookahead kernel and the greedy players' candidate kernels (lookahead.hip.h) with their C-ABI,
// azg_env_lookahead and azg_greedy_candidates.  A translation unit of its own for the reason given at the top of azg_playout.hip: one
// k_env_lookahead per game calls that game's valid_mask, wave_make_move, game_ended and get_score, and extra callers of the game plugins
// must not change what the compiler inlines into the kernels of the other units.
#include <hip/hip_runtime.h>
#include <string>
#include <type_traits>

#include "azg_dispatch.h"
#include "lookahead.hip.h"

using namespace azg;

extern "C" int azg_env_lookahead(int game, int variant, const int8_t* states, const int32_t* players, const uint8_t* active, int n,
                                 int waves_per_state, uint64_t rng_seed, uint64_t stream0, const uint64_t* counters, uint8_t* out_valid,
                                 int32_t* out_scores, float* out_ended, int32_t* out_next_player, int8_t* out_states, void* stream) {
    if (waves_per_state < 1 || waves_per_state > 64) return fail("azg_env_lookahead: waves_per_state must be in 1 .. 64");
    variant = norm_variant(game, variant);
    if (azg_game_info(game, variant, nullptr, nullptr, nullptr, nullptr, nullptr) != 0) return -1;
    if (n == 0) return 0;
    if (n < 0 || !states || !out_valid || !out_scores || !out_ended || !out_next_player) return fail("azg_env_lookahead: null / negative argument");
    AZG_DISPATCH(game, variant,
                 k_env_lookahead<G><<<dim3((unsigned)n, (unsigned)waves_per_state), dim3(64), 0, (hipStream_t)stream>>>(
                     states, players, active, n, waves_per_state, rng_seed, stream0, counters, out_valid, out_scores, out_ended, out_next_player, out_states));
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int azg_greedy_candidates(int game, int variant, int rule, const int8_t* states, const uint8_t* valid, const int32_t* scores, int n,
                                     const uint8_t* active, uint8_t* out_candidates, void* stream) {
    if (rule != AZG_GREEDY_REFERENCE && rule != AZG_GREEDY_LEAD) return fail("azg_greedy_candidates: rule must be 0 (reference) or 1 (lead)");
    variant = norm_variant(game, variant);
    int A = 0, P = 0;
    if (azg_game_info(game, variant, nullptr, &A, &P, nullptr, nullptr) != 0) return -1;
    if (rule == AZG_GREEDY_REFERENCE && game != AZG_SPLENDOR && game != AZG_AZUL && game != AZG_ABALONE)
        return fail("azg_greedy_candidates: the reference defines no greedy player for this game");
    if (n == 0) return 0;
    const bool board_only = rule == AZG_GREEDY_REFERENCE && game == AZG_AZUL;
    if (n < 0 || !valid || !out_candidates || (!board_only && !scores) ||
        (rule == AZG_GREEDY_REFERENCE && game != AZG_ABALONE && !states))
        return fail("azg_greedy_candidates: null / negative argument");
    const dim3 grid((unsigned)n), block(64);
    hipStream_t s = (hipStream_t)stream;
    if (rule == AZG_GREEDY_LEAD)
        k_greedy_lead<<<grid, block, 0, s>>>(valid, scores, n, A, P, active, out_candidates);
    else if (game == AZG_ABALONE)
        k_greedy_ref_abalone<<<grid, block, 0, s>>>(valid, scores, n, A, active, out_candidates);
    else if (game == AZG_AZUL)
        k_greedy_ref_azul<<<grid, block, 0, s>>>(states, valid, n, active, out_candidates);
    else if (variant == 2)
        k_greedy_ref_splendor<SplendorDev<2>><<<grid, block, 0, s>>>(states, valid, scores, n, active, out_candidates);
    else if (variant == 3)
        k_greedy_ref_splendor<SplendorDev<3>><<<grid, block, 0, s>>>(states, valid, scores, n, active, out_candidates);
    else
        k_greedy_ref_splendor<SplendorDev<4>><<<grid, block, 0, s>>>(states, valid, scores, n, active, out_candidates);
    HIPCHK(hipGetLastError());
    return 0;
}
