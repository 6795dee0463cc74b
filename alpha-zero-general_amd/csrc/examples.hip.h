// examples.hip.h -- one iteration's drained records -> the dense rows of the five example columns in ONE launch (azg_examples_expand):
// Coach.executeEpisode's `for sym in getSymmetries(...)` (Coach.py:66-69) for n records at once, written where the trainer reads them.
// One workgroup = one 64-lane wave = one group (record), exactly as k_env_symmetries / k_env_symmetries_built (kernels.hip.h) hold it: the
// state in LDS, the forms through the same G::sym_exists / sym_state_byte / sym_action_src and G::sym_build (+ SYM_DEDUP) interfaces, in
// the same order and with the same draws.  What differs is where a form goes: form k of group g is ROW first_row[g] + k of the outputs
// (no [n][K][.] intermediate, no mask pass), z and q of the source record are replicated into the row, and only rows inside
// [row_begin, row_end) are written -- a form outside the window is still built, counted and, where the game draws, paid for in draws.
// first_row == NULL is the count pass: the same loop without a store.
// States are stored as dwords (4 bytes per lane, 256 B per wave instruction) where S is a multiple of 4 and the buffer is 4-byte aligned
// -- every row then starts on a dword --, as single bytes otherwise; the bytes are the same either way.
#pragma once
#include "forest.hip.h"

namespace azg {

struct ExamplesOut {
    int8_t* states; float* pi; float* z; uint8_t* valids; float* q;      // row-major [rows][S | A | P | A | P]
    int64_t row_begin, row_end;                                           // the only rows that may be written
    int wide;                                                             // states 4-byte aligned: dword stores where S % 4 == 0
};

// 4 consecutive bytes of form c, as the byte stores would leave them in memory (little endian)
template <class G>
__device__ __forceinline__ uint32_t examples_state_dword(const int8_t* st, int c, int i) {
    return (uint32_t)(uint8_t)G::sym_state_byte(st, c, i) | ((uint32_t)(uint8_t)G::sym_state_byte(st, c, i + 1) << 8) |
           ((uint32_t)(uint8_t)G::sym_state_byte(st, c, i + 2) << 16) | ((uint32_t)(uint8_t)G::sym_state_byte(st, c, i + 3) << 24);
}

// z and q of the source record into row `row`
template <class G>
__device__ __forceinline__ void examples_store_zq(const ExamplesOut& o, int64_t row, const float* zin, const float* qin) {
    if (lane_id() < G::P) {
        o.z[row * G::P + lane_id()] = zin[lane_id()];
        o.q[row * G::P + lane_id()] = qin[lane_id()];
    }
}

// Games whose forms are byte and action maps of the state (k_env_symmetries).
template <class G>
__global__ __launch_bounds__(64) void k_examples_expand(const int8_t* states, const float* pi, const float* z, const uint8_t* valids,
                                                         const float* q, int n, const int32_t* order, const int64_t* first_row,
                                                         ExamplesOut o, int32_t* out_count) {
    __shared__ __attribute__((aligned(16))) int8_t st[G::SP];
    const int g = blockIdx.x;
    if (g >= n) return;
    const int src_rec = order ? order[g] : g;
    if ((unsigned)src_rec >= (unsigned)n) {                  // an order entry outside [0, n): no form, nothing read
        if (lane_id() == 0) out_count[g] = 0;
        return;
    }
    Forest<G>::load_state_unpadded(st, states + (size_t)src_rec * G::S);
    const float* pin = pi + (size_t)src_rec * G::A;
    const uint8_t* vin = valids + (size_t)src_rec * G::A;
    const bool write = first_row != nullptr;
    const int64_t row0 = write ? first_row[g] : 0;
    int k = 0;
    for (int c = 0; c < G::NSYM_CAND; c++) {
        if (!G::sym_exists(st, c)) continue;
        const int64_t row = row0 + k;
        if (write && row >= o.row_begin && row < o.row_end) {
            if (G::S % 4 == 0 && o.wide) {
                uint32_t* dst = (uint32_t*)(o.states + row * G::S);
                for (int i = lane_id(); i < G::S / 4; i += 64) dst[i] = examples_state_dword<G>(st, c, 4 * i);
            } else {
                for (int i = lane_id(); i < G::S; i += 64) o.states[row * G::S + i] = G::sym_state_byte(st, c, i);
            }
            for (int a = lane_id(); a < G::A; a += 64) {
                const int src = G::sym_action_src(st, c, a);          // < 0: no action maps onto a (Abalone groups off the grid)
                o.pi[row * G::A + a] = src >= 0 ? pin[src] : 0.f;
                o.valids[row * G::A + a] = src >= 0 ? vin[src] : (uint8_t)0;
            }
            examples_store_zq<G>(o, row, z + (size_t)src_rec * G::P, q + (size_t)src_rec * G::P);
        }
        k++;
    }
    if (lane_id() == 0) out_count[g] = k;
}

// Games whose forms are BUILT by lane 0 (G::RANDOM_SYM, k_env_symmetries_built): group g draws from the counter stream
// (rng_seed, stream0 + g) -- the GROUP index, whatever source record `order` names.
template <class G>
__global__ __launch_bounds__(64) void k_examples_expand_built(const int8_t* states, const float* pi, const float* z, const uint8_t* valids,
                                                               const float* q, int n, const int32_t* order, const int64_t* first_row,
                                                               ExamplesOut o, int32_t* out_count, uint64_t rng_seed, uint64_t stream0) {
    constexpr int NKEEP = G::SYM_DEDUP ? G::NSYM_CAND : 1;
    __shared__ __attribute__((aligned(16))) int8_t st[G::SP];
    __shared__ __attribute__((aligned(16))) int8_t kept[NKEEP][G::SP];
    __shared__ int16_t act_src[G::A];
    __shared__ int exists_s;
    const int g = blockIdx.x;
    if (g >= n) return;
    const int src_rec = order ? order[g] : g;
    if ((unsigned)src_rec >= (unsigned)n) {
        if (lane_id() == 0) out_count[g] = 0;
        return;
    }
    Forest<G>::load_state_unpadded(st, states + (size_t)src_rec * G::S);
    const float* pin = pi + (size_t)src_rec * G::A;
    const uint8_t* vin = valids + (size_t)src_rec * G::A;
    const bool write = first_row != nullptr;
    const int64_t row0 = write ? first_row[g] : 0;
    Rng rng{rng_seed, stream0 + (uint64_t)g, 0};
    int k = 0;
    for (int c = 0; c < G::NSYM_CAND; c++) {
        int8_t* cand = kept[G::SYM_DEDUP ? (k < NKEEP ? k : NKEEP - 1) : 0];
        for (int i = lane_id(); i < G::S; i += 64) cand[i] = st[i];
        __syncthreads();
        if (lane_id() == 0) exists_s = G::sym_build(st, c, cand, act_src, rng, vin) ? 1 : 0;     // (draws even when the form is dropped below)
        __syncthreads();
        bool keep = exists_s != 0;
        if (keep && G::SYM_DEDUP) {
            for (int e = 0; e < k && keep; e++) {
                bool diff = false;
                for (int i = lane_id(); i < G::S; i += 64) diff |= kept[e][i] != cand[i];
                keep = __ballot(diff) != 0;
            }
        }
        if (keep) {
            const int64_t row = row0 + k;
            if (write && row >= o.row_begin && row < o.row_end) {
                if (G::S % 4 == 0 && o.wide) {                       // (cand is 16-byte aligned: G::SP is a multiple of 16)
                    uint32_t* dst = (uint32_t*)(o.states + row * G::S);
                    const uint32_t* cw = (const uint32_t*)cand;
                    for (int i = lane_id(); i < G::S / 4; i += 64) dst[i] = cw[i];
                } else {
                    for (int i = lane_id(); i < G::S; i += 64) o.states[row * G::S + i] = cand[i];
                }
                for (int a = lane_id(); a < G::A; a += 64) {
                    const int src = act_src[a];                      // < 0: nothing maps onto a
                    o.pi[row * G::A + a] = src >= 0 ? pin[src] : 0.f;
                    o.valids[row * G::A + a] = src >= 0 ? vin[src] : (uint8_t)0;
                }
                examples_store_zq<G>(o, row, z + (size_t)src_rec * G::P, q + (size_t)src_rec * G::P);
            }
            k++;
        }
        __syncthreads();
    }
    if (lane_id() == 0) out_count[g] = k;
}

// ---- the other half: a training batch straight from the RECORDS (azg_train_gather_forms) -----------------------------------------------
// Nothing forces the rows above to be stored: row r of the expanded history is a function of (record, form index) -- and of the record's
// stream where the game draws.  One wave per BATCH row b: r = ids[b]; the record is the lowest g with row_end[g] > r (row_end is
// non-decreasing: a wave-uniform binary search over read-only memory), the form is k = r - first_row[g], and row b of the outputs gets
// the bytes k_examples_expand* writes to row first_row[g] + k -- the same candidates in the same order through the same interfaces.
// An id that no record owns, or a k outside [0, NSYM_CAND), returns before anything but the index columns is read.
struct FormsIn {
    const int8_t* states; const float* pi; const float* z; const uint8_t* valids; const float* q;     // records [n][S | A | P | A | P]
    const int64_t* first_row; const int64_t* row_end; const uint64_t* streams; int n;
};
struct FormsOut {
    int8_t* boards; float* pi; float* z; uint8_t* valids; float* q;      // row-major [B][S | A | P | A | P]
    int wide;                                                             // boards 4-byte aligned: dword stores where S % 4 == 0
};

// -> the record that owns virtual row ids[b] and (k) its form index; -1 when there is none
__device__ __forceinline__ int forms_locate(const FormsIn& in, const int32_t* ids, int b, int ncand, int& k) {
    const int64_t r = ids[b];
    if (r < 0) return -1;
    int lo = 0, hi = in.n;                                               // lowest g with row_end[g] > r
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (in.row_end[mid] > r) hi = mid; else lo = mid + 1;
    }
    if (lo >= in.n) return -1;
    const int64_t kk = r - in.first_row[lo];
    if (kk < 0 || kk >= ncand) return -1;
    k = (int)kk;
    return lo;
}

// pi / valids of batch row b through the action map `src_of`, and the record's z / q
template <class G, class F>
__device__ __forceinline__ void forms_store_tail(const FormsIn& in, const FormsOut& o, int g, int b, F src_of) {
    const float* pin = in.pi + (size_t)g * G::A;
    const uint8_t* vin = in.valids + (size_t)g * G::A;
    for (int a = lane_id(); a < G::A; a += 64) {
        const int src = src_of(a);                                       // < 0: no action maps onto a
        o.pi[(size_t)b * G::A + a] = src >= 0 ? pin[src] : 0.f;
        o.valids[(size_t)b * G::A + a] = src >= 0 ? (uint8_t)(vin[src] != 0) : (uint8_t)0;
    }
    if (lane_id() < G::P) {
        o.z[(size_t)b * G::P + lane_id()] = in.z[(size_t)g * G::P + lane_id()];
        o.q[(size_t)b * G::P + lane_id()] = in.q[(size_t)g * G::P + lane_id()];
    }
}

// Map games: form k is the k-th candidate with sym_exists; the candidates are counted 64 at a time, one per lane (Azul has 120).
template <class G>
__global__ __launch_bounds__(64) void k_gather_forms(FormsIn in, const int32_t* ids, int B, FormsOut o) {
    __shared__ __attribute__((aligned(16))) int8_t st[G::SP];
    const int b = blockIdx.x;
    if (b >= B) return;
    int k = 0;
    const int g = forms_locate(in, ids, b, G::NSYM_CAND, k);
    if (g < 0) return;
    Forest<G>::load_state_unpadded(st, in.states + (size_t)g * G::S);
    int c = -1;
    for (int c0 = 0; c0 < G::NSYM_CAND; c0 += 64) {
        const int mine = c0 + lane_id();
        const bool e = mine < G::NSYM_CAND && G::sym_exists(st, mine);
        const uint64_t m = __ballot(e);
        const int cnt = __popcll(m);
        if (k < cnt) {                                                   // the lane whose candidate has k existing ones in front of it
            const uint64_t hit = __ballot(e && __popcll(m & ((1ull << lane_id()) - 1ull)) == k);
            c = c0 + (__ffsll((unsigned long long)hit) - 1);
            break;
        }
        k -= cnt;
    }
    if (c < 0) return;                                                   // the record has fewer than k + 1 forms
    if (G::S % 4 == 0 && o.wide) {
        uint32_t* dst = (uint32_t*)(o.boards + (size_t)b * G::S);
        for (int i = lane_id(); i < G::S / 4; i += 64) dst[i] = examples_state_dword<G>(st, c, 4 * i);
    } else {
        for (int i = lane_id(); i < G::S; i += 64) o.boards[(size_t)b * G::S + i] = G::sym_state_byte(st, c, i);
    }
    forms_store_tail<G>(in, o, g, b, [&](int a) { return G::sym_action_src(st, c, a); });
}

// Built games: the wave rebuilds candidates 0, 1, ... on the record's stream (rng_seed, streams[g]), counter from 0, exactly as
// k_examples_expand_built does -- the draws of a dropped candidate included -- and stops at the k-th kept form.
template <class G>
__global__ __launch_bounds__(64) void k_gather_forms_built(FormsIn in, const int32_t* ids, int B, FormsOut o, uint64_t rng_seed) {
    constexpr int NKEEP = G::SYM_DEDUP ? G::NSYM_CAND : 1;
    __shared__ __attribute__((aligned(16))) int8_t st[G::SP];
    __shared__ __attribute__((aligned(16))) int8_t kept[NKEEP][G::SP];
    __shared__ int16_t act_src[G::A];
    __shared__ int exists_s;
    const int b = blockIdx.x;
    if (b >= B) return;
    int want = 0;
    const int g = forms_locate(in, ids, b, G::NSYM_CAND, want);
    if (g < 0) return;
    Forest<G>::load_state_unpadded(st, in.states + (size_t)g * G::S);
    const uint8_t* vin = in.valids + (size_t)g * G::A;
    Rng rng{rng_seed, in.streams ? in.streams[g] : (uint64_t)g, 0};
    int k = 0;
    for (int c = 0; c < G::NSYM_CAND; c++) {
        int8_t* cand = kept[G::SYM_DEDUP ? (k < NKEEP ? k : NKEEP - 1) : 0];
        for (int i = lane_id(); i < G::S; i += 64) cand[i] = st[i];
        __syncthreads();
        if (lane_id() == 0) exists_s = G::sym_build(st, c, cand, act_src, rng, vin) ? 1 : 0;
        __syncthreads();
        bool keep = exists_s != 0;
        if (keep && G::SYM_DEDUP) {
            for (int e = 0; e < k && keep; e++) {
                bool diff = false;
                for (int i = lane_id(); i < G::S; i += 64) diff |= kept[e][i] != cand[i];
                keep = __ballot(diff) != 0;
            }
        }
        if (keep) {
            if (k == want) {
                if (G::S % 4 == 0 && o.wide) {                           // (cand is 16-byte aligned: G::SP is a multiple of 16)
                    uint32_t* dst = (uint32_t*)(o.boards + (size_t)b * G::S);
                    const uint32_t* cw = (const uint32_t*)cand;
                    for (int i = lane_id(); i < G::S / 4; i += 64) dst[i] = cw[i];
                } else {
                    for (int i = lane_id(); i < G::S; i += 64) o.boards[(size_t)b * G::S + i] = cand[i];
                }
                forms_store_tail<G>(in, o, g, b, [&](int a) { return (int)act_src[a]; });
                return;
            }
            k++;
        }
        __syncthreads();
    }
}

}  // namespace azg
