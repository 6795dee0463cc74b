// train.hip.h -- the training step's batch side (GenericNNetWrapper.train :44-92): which examples a step takes, their five columns, and the
// two losses with their gradients with respect to the net's outputs.  Nothing here is read back by the host.
// k_train_sample_ids: np.random.choice(n, batch, replace=False) (:57) for MANY steps in one launch, one wave per step: a Fisher-Yates shuffle
//   over a virtual identity on the RNG contract of include/azg.h.  The 64 lanes compute 64 uniforms at a time (three mix64 each), lane 0 runs
//   the chain against an open-addressing map in LDS that holds only the displaced entries of the permutation (at most `batch`).
// k_train_gather: one wave per batch row copies the row's five columns; rows start at any byte offset, so the byte columns move as bytes.
// k_train_loss_rows / k_train_loss_totals: one wave per row / ONE wave for the totals, as loss.hip.h -- sums in f64, lanes in index order
//   and one fixed xor tree, so the numbers are the same bits in every call; the gradients in f32, operation for operation what autograd
//   computes for train.loss_pi + v_coeff * train.loss_v.
// k_adamw_onecycle / k_adamw_step_advance: the optimiser step of :81-82 (AdamW + OneCycleLR) for ALL parameters in one launch, with the
//   step's scalars taken from a table row that a counter in device memory picks; then the counter's increment.  No atomics, no LDS.
#pragma once
#include "azg_common.hip.h"

namespace azg {

constexpr int TRAIN_MAX_BATCH = 8192;
constexpr int TRAIN_MAP_SLOTS = 2 * TRAIN_MAX_BATCH;        // load factor <= 1/2: a step adds at most one entry
constexpr uint32_t TRAIN_MAP_EMPTY = 0xFFFFFFFFu;            // (keys are indices below 2^31)

// sum of an f64 over the wave, the same bits in every lane (loss.hip.h's helper: that header's kernels may be defined in one unit only)
__device__ __forceinline__ double train_wave_tree_sum_f64(double x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += shfl_xor_f64(x, m);
    return x;
}

// slot of `key`, or of the first empty slot of its probe sequence; at most `slots` probes (the map is never more than half full, so an
// empty slot always ends the walk earlier: the bound only keeps the loop finite whatever the LDS holds)
__device__ __forceinline__ uint32_t train_map_find(const uint32_t* keys, uint32_t key, int log2_slots) {
    const uint32_t mask = (1u << log2_slots) - 1u;
    uint32_t s = (key * 0x9E3779B1u) >> (32 - log2_slots);
    for (uint32_t probes = 0; probes <= mask; probes++) {
        const uint32_t k = keys[s];
        if (k == key || k == TRAIN_MAP_EMPTY) break;
        s = (s + 1u) & mask;
    }
    return s;
}

// ids[s][0 .. batch) for step s = blockIdx.x, on the stream (rng_seed, stream0 + s), counters 0 .. batch - 1:
//   p = identity on [0, n);  for i = 0 .. batch - 1:  m = n - i, j = i + min(floor(u01(i) m), m - 1), ids[i] = p[j], p[j] = p[i].
// log2_slots: the map uses the first 2^log2_slots (>= 2 batch, >= 64, <= TRAIN_MAP_SLOTS) slots -- checked by the caller.
__global__ __launch_bounds__(64) void k_train_sample_ids(uint32_t n, int batch, uint64_t rng_seed, uint64_t stream0, int log2_slots,
                                                         int32_t* __restrict__ ids) {
    __shared__ uint32_t keys[TRAIN_MAP_SLOTS];
    __shared__ uint32_t vals[TRAIN_MAP_SLOTS];
    __shared__ uint32_t jbuf[64];
    const int l = lane_id();
    const int slots = 1 << log2_slots;
    for (int k = l; k < slots; k += 64) keys[k] = TRAIN_MAP_EMPTY;
    const uint64_t base = mix64(mix64(rng_seed ^ 0x9E3779B97F4A7C15ULL) + (stream0 + (uint64_t)blockIdx.x));
    int32_t* out = ids + (size_t)blockIdx.x * (size_t)batch;
    for (int i0 = 0; i0 < batch; i0 += 64) {
        const int cnt = batch - i0 < 64 ? batch - i0 : 64;
        if (l < cnt) {
            const uint32_t i = (uint32_t)(i0 + l), m = n - i;
            const double u = (double)(mix64(base + (uint64_t)i) >> 11) * (1.0 / 9007199254740992.0);
            uint32_t r = (uint32_t)(u * (double)m);                       // floor: the product is >= 0 and below 2^31
            r = r < m - 1u ? r : m - 1u;
            jbuf[l] = i + r;
        }
        wave_sync();                                                      // (the first round: the cleared keys too)
        if (l == 0) {
            for (int k = 0; k < cnt; k++) {
                const uint32_t i = (uint32_t)(i0 + k), j = jbuf[k];
                const uint32_t sj = train_map_find(keys, j, log2_slots);
                const uint32_t pj = keys[sj] == j ? vals[sj] : j;
                out[i] = (int32_t)pj;
                if (j != i) {                                             // p[j] = p[i]; index i itself is never looked at again
                    const uint32_t si = train_map_find(keys, i, log2_slots);
                    const uint32_t pi = keys[si] == i ? vals[si] : i;
                    if (keys[sj] == j || keys[sj] == TRAIN_MAP_EMPTY) { keys[sj] = j; vals[sj] = pi; }
                }
            }
        }
        wave_sync();
    }
}

// out_*[b] = column[ids[b]] for the five example columns, row b = 4 blockIdx.x + the wave's index; valids as 0 / 1 bytes.  An id outside
// [0, n) is the caller's error: the row then holds example 0 (no address outside the columns is formed).
__global__ __launch_bounds__(256) void k_train_gather(const int8_t* __restrict__ boards, const float* __restrict__ pi, const float* __restrict__ z,
                                                      const uint8_t* __restrict__ valids, const float* __restrict__ q,
                                                      const int32_t* __restrict__ ids, int n, int B, int S, int A, int P,
                                                      int8_t* __restrict__ out_boards, float* __restrict__ out_pi, float* __restrict__ out_z,
                                                      uint8_t* __restrict__ out_valids, float* __restrict__ out_q) {
    const int l = lane_id();
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    int id = uni_i32(ids[b]);
    if ((uint32_t)id >= (uint32_t)n) id = 0;
    const size_t src = (size_t)id, dst = (size_t)b;
    {
        const float* s = pi + src * A;
        float* d = out_pi + dst * A;
#pragma unroll 4
        for (int a = l; a < A; a += 64) d[a] = s[a];
    }
    {
        const uint8_t* s = valids + src * A;
        uint8_t* d = out_valids + dst * A;
#pragma unroll 4
        for (int a = l; a < A; a += 64) d[a] = s[a] != 0 ? 1 : 0;
    }
    {
        const int8_t* s = boards + src * S;
        int8_t* d = out_boards + dst * S;
#pragma unroll 4
        for (int a = l; a < S; a += 64) d[a] = s[a];
    }
    if (l < P) {
        out_z[dst * P + l] = z[src * P + l];
        out_q[dst * P + l] = q[src * P + l];
    }
}

// rows[b] = { sum over the actions with t > 0 of t (log t - log_pi)  (F.kl_div's xlogy convention: t == 0 adds exactly 0 and gets the
//             gradient 0, whatever log_pi holds -- masked actions carry -1e8),  sum_p (t_v - v)^2 }, both in f64 from the f32 inputs;
// grad_log_pi[b][a] = -(t inv_b), grad_v[b][p] = -(g_v (2 (t_v - v))) in f32 with t_v = (z + q_weight q) inv_1q: every factor is passed in as
// the f32 the host computed (inv_b = 1 / B, g_v = v_coeff * (1 / (B P)), inv_1q = 1 / (1 + q_weight)) -- the products autograd forms.
__global__ __launch_bounds__(64) void k_train_loss_rows(const float* __restrict__ log_pi, const float* __restrict__ v,
                                                        const float* __restrict__ target_pi, const float* __restrict__ z,
                                                        const float* __restrict__ q, int B, int A, int P, float q_weight, float inv_1q,
                                                        float inv_b, float g_v, float* __restrict__ grad_log_pi, float* __restrict__ grad_v,
                                                        double* __restrict__ rows) {
    const int b = blockIdx.x, l = lane_id();
    if (b >= B) return;
    const float* lp = log_pi + (size_t)b * A;
    const float* t = target_pi + (size_t)b * A;
    float* g = grad_log_pi + (size_t)b * A;
    double kl = 0.0;
    for (int a = l; a < A; a += 64) {
        const float ta = t[a];
        float ga = 0.f;
        if (ta > 0.f) {
            kl += (double)ta * (log((double)ta) - (double)lp[a]);
            ga = -(ta * inv_b);
        }
        g[a] = ga;
    }
    kl = train_wave_tree_sum_f64(kl);
    double se = 0.0;
    if (l < P) {
        const size_t i = (size_t)b * P + l;
        const float zi = z[i], qi = q[i], vi = v[i];
        const double d = ((double)zi + (double)q_weight * (double)qi) / (1.0 + (double)q_weight) - (double)vi;
        se = d * d;
        const float tv = (zi + q_weight * qi) * inv_1q;
        grad_v[i] = -(g_v * (2.f * (tv - vi)));
    }
    se = train_wave_tree_sum_f64(se);
    if (l == 0) { rows[2 * (size_t)b] = kl; rows[2 * (size_t)b + 1] = se; }
}

// out = { sum_b rows[b][0] / B, sum_b rows[b][1] / (B P) }: one wave, lane l takes rows l, l + 64, ... in order, then the fixed tree
__global__ __launch_bounds__(64) void k_train_loss_totals(const double* __restrict__ rows, int B, int P, double* __restrict__ out) {
    const int l = lane_id();
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
    for (int b = l; b < B; b += 64) {
        s0 += rows[2 * (size_t)b];
        s1 += rows[2 * (size_t)b + 1];
    }
    s0 = train_wave_tree_sum_f64(s0);
    s1 = train_wave_tree_sum_f64(s1);
    if (l == 0) out[0] = s0 / (double)B;
    if (l == 1) out[1] = s1 / ((double)B * (double)P);
}

// ---- the optimiser: torch.optim.AdamW under OneCycleLR in ONE launch, the step number read from device memory ---------------------------
// (the two kernels below are named k_adamw_*, not k_train_*: tests/test_train_batches_surface.py counts the k_train_ kernels of this unit)
constexpr int TRAIN_ADAMW_CHUNK = 2048;                    // elements per workgroup: 256 lanes x two float4
struct TrainAdamwSeg { float* p; const float* g; float* m; float* v; long long numel; };     // azg_adamw_seg of include/azg.h
struct TrainAdamwChunk { int seg, first; };                                                 // azg_adamw_chunk

// one element of torch's foreach AdamW (_multi_tensor_adamw, not capturable, no amsgrad), every operation rounded on its own:
//   p *= r0;  m += r1 (g - m);  v *= r2;  v += (g g) r3;  p -= r4 (m / (sqrt(v) / r5 + r6))
__device__ __forceinline__ void train_adamw_elem(float& p, float g, float& m, float& v, float r0, float r1, float r2, float r3, float r4,
                                                 float r5, float r6) {
    p = __fmul_rn(p, r0);
    m = __fadd_rn(m, __fmul_rn(r1, __fsub_rn(g, m)));
    v = __fmul_rn(v, r2);
    v = __fadd_rn(v, __fmul_rn(__fmul_rn(g, g), r3));
    const float d = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), r5), r6);
    p = __fsub_rn(p, __fmul_rn(r4, __fdiv_rn(m, d)));
}

// workgroup c updates elements [first, first + 2048) (or up to numel) of segment chunks[c].seg with row clamp(*step, 0, total_steps - 1) of
// the table.  Everything but the elements is wave-uniform: the step, the table row, the chunk and its segment arrive in scalar registers.
// 16-byte accesses when the chunk is whole and the segment's four pointers are 16-byte aligned (`first` is a multiple of 2048), else one
// element per lane and trip.  A chunk that names no segment, or starts outside its segment, touches nothing.
__global__ __launch_bounds__(256) void k_adamw_onecycle(const TrainAdamwSeg* __restrict__ segs, int n_segs,
                                                        const TrainAdamwChunk* __restrict__ chunks, const float* __restrict__ table,
                                                        int total_steps, const long long* __restrict__ step) {
    long long s = *step;
    s = s < 0 ? 0 : (s > (long long)total_steps - 1 ? (long long)total_steps - 1 : s);
    const float* r = table + 8 * s;
    const float r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4], r5 = r[5], r6 = r[6];
    const TrainAdamwChunk c = chunks[blockIdx.x];
    if ((unsigned)c.seg >= (unsigned)n_segs) return;
    const TrainAdamwSeg sg = segs[c.seg];
    if (c.first < 0 || (long long)c.first >= sg.numel) return;
    const long long left = sg.numel - (long long)c.first;
    // (the pointers come out of a table: without the address space the compiler can only use flat accesses)
    typedef __attribute__((address_space(1))) float gf32;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) f32x4 gf32x4;
    gf32* p = (gf32*)sg.p + c.first;
    const gf32* g = (const gf32*)sg.g + c.first;
    gf32* m = (gf32*)sg.m + c.first;
    gf32* v = (gf32*)sg.v + c.first;
    const bool aligned = ((((uintptr_t)sg.p) | ((uintptr_t)sg.g) | ((uintptr_t)sg.m) | ((uintptr_t)sg.v)) & 15) == 0 && (c.first & 3) == 0;
    if (aligned && left >= TRAIN_ADAMW_CHUNK) {
        f32x4 p4[2], g4[2], m4[2], v4[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {                                   // all eight loads first: the kernel is bound by memory
            const int i = (int)threadIdx.x + 256 * k;
            p4[k] = ((const gf32x4*)p)[i];
            g4[k] = ((const gf32x4*)g)[i];
            m4[k] = ((const gf32x4*)m)[i];
            v4[k] = ((const gf32x4*)v)[i];
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int i = (int)threadIdx.x + 256 * k;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                float pe = p4[k][e], me = m4[k][e], ve = v4[k][e];
                train_adamw_elem(pe, g4[k][e], me, ve, r0, r1, r2, r3, r4, r5, r6);
                p4[k][e] = pe;
                m4[k][e] = me;
                v4[k][e] = ve;
            }
            ((gf32x4*)p)[i] = p4[k];
            ((gf32x4*)m)[i] = m4[k];
            ((gf32x4*)v)[i] = v4[k];
        }
    } else {
        const int cnt = left < TRAIN_ADAMW_CHUNK ? (int)left : TRAIN_ADAMW_CHUNK;
        for (int i = (int)threadIdx.x; i < cnt; i += 256) {
            float pi = p[i], mi = m[i], vi = v[i];
            train_adamw_elem(pi, g[i], mi, vi, r0, r1, r2, r3, r4, r5, r6);
            p[i] = pi;
            m[i] = mi;
            v[i] = vi;
        }
    }
}

// *step += 1 -- a launch of its own behind k_adamw_onecycle on the same stream: no workgroup of the update can see the new value
__global__ __launch_bounds__(64) void k_adamw_step_advance(long long* __restrict__ step) {
    if (threadIdx.x == 0) *step = *step + 1;
}

}  // namespace azg
