// azg_playout.hip -- the random-playout kernels (playout.hip.h) and their C-ABI, azg_env_playouts.  A translation unit of its own: one
// k_env_playouts per game calls that game's game_ended, valid_mask and wave_make_move, and inside azg.hip those extra callers changed
// what the compiler inlines into kernels that were there before (k_env_valid_moves<SantoriniDev<11>> turned into a call with a stack;
// k_select, k_selfplay_advance and k_env_canonical of SmallworldDev<4> came out differently).  Here they share nothing with them.
#include <hip/hip_runtime.h>
#include <string>
#include <type_traits>

#include "azg_dispatch.h"
#include "playout.hip.h"

using namespace azg;

// ---- random playouts to the end of the game (playout.hip.h) --------------------------------------------------------------
extern "C" int azg_env_playouts(int game, int variant, const int8_t* states, const int32_t* players, const uint8_t* active, int n, int k,
                                int max_plies, uint64_t rng_seed, uint64_t stream0, uint64_t* counters, float* out_ended, int32_t* out_plies,
                                uint8_t* out_status, int8_t* out_states, int32_t* out_players, int32_t* out_actions, void* stream) {
    if (k < 1) return fail("azg_env_playouts: k must be at least 1");
    if (max_plies < 1 || max_plies > 65535) return fail("azg_env_playouts: max_plies must be in 1 .. 65535");
    variant = norm_variant(game, variant);
    if (azg_game_info(game, variant, nullptr, nullptr, nullptr, nullptr, nullptr) != 0) return -1;
    if (n == 0) return 0;
    if (n < 0 || !states || !out_ended || !out_plies || !out_status) return fail("azg_env_playouts: null / negative argument");
    if ((long long)n * (long long)k > 0x7FFFFFFFll) return fail("azg_env_playouts: n * k exceeds 2^31 - 1 playouts");
    AZG_DISPATCH(game, variant,
                 k_env_playouts<G><<<dim3((unsigned)(n * k)), dim3(64), 0, (hipStream_t)stream>>>(states, players, active, n, k, max_plies,
                                     rng_seed, stream0, counters, out_ended, out_plies, out_status, out_states, out_players, out_actions));
    HIPCHK(hipGetLastError());
    return 0;
}
