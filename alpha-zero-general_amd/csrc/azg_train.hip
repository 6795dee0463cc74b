// azg_train.hip -- the training step's batch kernels (train.hip.h) and their C-ABI: azg_train_sample_ids, azg_train_gather,
// azg_train_losses; the optimiser's: azg_train_adamw, azg_train_step_advance.  A translation unit of its own, like azg_loss.hip: nothing here can change what the compiler makes of a kernel that
// was there before.
#include <hip/hip_runtime.h>
#include <string>

#include "../../include/azg.h"
#include "azg_host.h"
#include "train.hip.h"

using namespace azg;

extern "C" int azg_train_sample_ids(int64_t n, int batch, int n_steps, uint64_t rng_seed, uint64_t stream0, int32_t* ids_out, void* stream) {
    if (batch < 1 || batch > TRAIN_MAX_BATCH) return fail("azg_train_sample_ids: 1 <= batch <= 8192 is required");
    if (n < batch || n > 0x7FFFFFFFLL) return fail("azg_train_sample_ids: batch <= n < 2^31 is required");
    if (n_steps < 0) return fail("azg_train_sample_ids: n_steps >= 0 is required");
    if (n_steps == 0) return 0;
    if (!ids_out) return fail("azg_train_sample_ids: ids_out is NULL");
    int log2_slots = 6;                                                  // the map: >= 2 batch slots, a power of two
    while ((1 << log2_slots) < 2 * batch) log2_slots++;
    if ((1 << log2_slots) > TRAIN_MAP_SLOTS) return fail("azg_train_sample_ids: internal: map larger than its LDS");
    k_train_sample_ids<<<dim3((unsigned)n_steps), dim3(64), 0, (hipStream_t)stream>>>((uint32_t)n, batch, rng_seed, stream0, log2_slots, ids_out);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int azg_train_gather(const int8_t* boards, const float* pi, const float* z, const uint8_t* valids, const float* q, const int32_t* ids,
                                int n, int B, int S, int A, int P, int8_t* out_boards, float* out_pi, float* out_z, uint8_t* out_valids,
                                float* out_q, void* stream) {
    if (n < 1 || B < 0 || S < 1 || A < 1 || P < 1 || P > 8) return fail("azg_train_gather: n >= 1, B >= 0, S >= 1, A >= 1 and 1 <= P <= 8 are required");
    if (B > 0x7FFFFFFF - 64) return fail("azg_train_gather: B must be below 2^31 - 64");
    if (B == 0) return 0;
    if (!boards || !pi || !z || !valids || !q || !ids || !out_boards || !out_pi || !out_z || !out_valids || !out_q)
        return fail("azg_train_gather: a required pointer is NULL");
    k_train_gather<<<dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(boards, pi, z, valids, q, ids, n, B, S, A, P, out_boards,
                                                                                     out_pi, out_z, out_valids, out_q);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int azg_train_losses(const float* log_pi, const float* v, const float* target_pi, const float* z, const float* q, int B, int A, int P,
                                float q_weight, float v_coeff, float* grad_log_pi, float* grad_v, double* rows, double* out, void* stream) {
    if (B < 1 || A < 1 || P < 1 || P > 8) return fail("azg_train_losses: B >= 1, A >= 1 and 1 <= P <= 8 are required");
    if (B > 0x7FFFFFFF - 64 || A > 0x7FFFFFFF - 64) return fail("azg_train_losses: B and A must be below 2^31 - 64");
    if (!(q_weight > -1.f)) return fail("azg_train_losses: q_weight must be above -1");
    if (!log_pi || !v || !target_pi || !z || !q || !grad_log_pi || !grad_v || !rows || !out) return fail("azg_train_losses: a required pointer is NULL");
    // the scale factors as autograd forms them: a division of a tensor by a host scalar is a product with the scalar's f32 reciprocal
    const float inv_1q = 1.f / (1.f + q_weight);
    const float inv_b = 1.f / (float)B;
    const float g_v = v_coeff * (1.f / (float)((double)B * (double)P));
    k_train_loss_rows<<<dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream>>>(log_pi, v, target_pi, z, q, B, A, P, q_weight, inv_1q, inv_b, g_v,
                                                                             grad_log_pi, grad_v, rows);
    k_train_loss_totals<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(rows, B, P, out);
    HIPCHK(hipGetLastError());
    return 0;
}

static_assert(sizeof(TrainAdamwSeg) == sizeof(azg_adamw_seg) && sizeof(TrainAdamwChunk) == sizeof(azg_adamw_chunk), "include/azg.h and train.hip.h disagree");

extern "C" int azg_train_adamw(const azg_adamw_seg* segs, int n_segs, const azg_adamw_chunk* chunks, int n_chunks, const float* table,
                               int total_steps, const int64_t* step, void* stream) {
    if (!segs || !chunks || !table || !step) return fail("azg_train_adamw: a required pointer is NULL");
    if (n_segs < 1) return fail("azg_train_adamw: n_segs >= 1 is required");
    if (n_chunks < 1) return fail("azg_train_adamw: n_chunks >= 1 is required");
    if (total_steps < 1) return fail("azg_train_adamw: total_steps >= 1 is required");
    k_adamw_onecycle<<<dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream>>>((const TrainAdamwSeg*)segs, n_segs, (const TrainAdamwChunk*)chunks,
                                                                                   table, total_steps, (const long long*)step);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int azg_train_step_advance(int64_t* step, void* stream) {
    if (!step) return fail("azg_train_step_advance: step is NULL");
    k_adamw_step_advance<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>((long long*)step);
    HIPCHK(hipGetLastError());
    return 0;
}
