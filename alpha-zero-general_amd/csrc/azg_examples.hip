// azg_examples.hip -- the example-expansion kernels (examples.hip.h) and their C-ABI, azg_examples_expand.  A translation unit of its
// own for the reason azg_playout.hip gives: a second caller of every game's symmetry functions inside azg.hip would change what the
// compiler inlines into the kernels that are there.
#include <hip/hip_runtime.h>
#include <string>
#include <type_traits>

#include "azg_dispatch.h"
#include "examples.hip.h"

using namespace azg;

extern "C" int azg_examples_expand(int game, int variant, const int8_t* states, const float* pi, const float* z, const uint8_t* valids,
                                   const float* q, int n, const int32_t* order, const int64_t* first_row, int64_t row_begin, int64_t row_end,
                                   int8_t* out_states, float* out_pi, float* out_z, uint8_t* out_valids, float* out_q, int32_t* out_count,
                                   uint64_t rng_seed, uint64_t stream0, void* stream) {
    variant = norm_variant(game, variant);
    if (azg_game_info(game, variant, nullptr, nullptr, nullptr, nullptr, nullptr) != 0) return -1;
    if (row_end < row_begin) return fail("azg_examples_expand: row_end < row_begin");
    if (n == 0) return 0;
    if (n < 0 || !states || !pi || !z || !valids || !q || !out_count) return fail("azg_examples_expand: null / negative argument");
    if (first_row && row_end > row_begin && (!out_states || !out_pi || !out_z || !out_valids || !out_q))
        return fail("azg_examples_expand: null output column");
    const ExamplesOut o{out_states, out_pi, out_z, out_valids, out_q, row_begin, row_end, ((uintptr_t)out_states & 3) == 0 ? 1 : 0};
    AZG_DISPATCH(game, variant, {
        if constexpr (G::RANDOM_SYM)
            k_examples_expand_built<G><<<dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream>>>(states, pi, z, valids, q, n, order, first_row, o,
                                                                                             out_count, rng_seed, stream0);
        else
            k_examples_expand<G><<<dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream>>>(states, pi, z, valids, q, n, order, first_row, o,
                                                                                       out_count);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int azg_train_gather_forms(int game, int variant, const int8_t* states, const float* pi, const float* z, const uint8_t* valids,
                                      const float* q, const int64_t* first_row, const int64_t* row_end, const uint64_t* streams, int n,
                                      const int32_t* ids, int B, int8_t* out_boards, float* out_pi, float* out_z, uint8_t* out_valids,
                                      float* out_q, uint64_t rng_seed, void* stream) {
    variant = norm_variant(game, variant);
    if (azg_game_info(game, variant, nullptr, nullptr, nullptr, nullptr, nullptr) != 0) return -1;
    if (B < 0) return fail("azg_train_gather_forms: B >= 0 is required");
    if (B == 0) return 0;
    if (n < 1) return fail("azg_train_gather_forms: n >= 1 is required");
    if (!states || !pi || !z || !valids || !q || !first_row || !row_end || !ids || !out_boards || !out_pi || !out_z || !out_valids || !out_q)
        return fail("azg_train_gather_forms: a required pointer is NULL");
    const FormsIn in{states, pi, z, valids, q, first_row, row_end, streams, n};
    const FormsOut o{out_boards, out_pi, out_z, out_valids, out_q, ((uintptr_t)out_boards & 3) == 0 ? 1 : 0};
    AZG_DISPATCH(game, variant, {
        if constexpr (G::RANDOM_SYM)
            k_gather_forms_built<G><<<dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream>>>(in, ids, B, o, rng_seed);
        else
            k_gather_forms<G><<<dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream>>>(in, ids, B, o);
    });
    HIPCHK(hipGetLastError());
    return 0;
}
