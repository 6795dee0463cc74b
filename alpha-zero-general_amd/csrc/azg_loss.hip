// azg_loss.hip -- the validation-loss kernels (loss.hip.h) and their C-ABI, azg_eval_losses.  A translation unit of its own, like
// azg_playout.hip: nothing here can change what the compiler makes of a kernel that was there before.
#include <hip/hip_runtime.h>
#include <string>

#include "../../include/azg.h"
#include "azg_host.h"
#include "loss.hip.h"

using namespace azg;

extern "C" int azg_eval_losses(const float* pi, const float* v, const float* target_pi, const float* z, const float* q, const uint8_t* active,
                               int B, int A, int P, float q_weight, double* rows, int32_t* flags, double* totals, int accumulate,
                               void* stream) {
    if (B < 0 || A < 1 || P < 1 || P > 8) return fail("azg_eval_losses: B >= 0, A >= 1 and 1 <= P <= 8 are required");
    if (B > 0x7FFFFFFF - 64 || A > 0x7FFFFFFF - 64) return fail("azg_eval_losses: B and A must be below 2^31 - 64");
    if (!(q_weight > -1.f)) return fail("azg_eval_losses: q_weight must be above -1");
    if (!totals) return fail("azg_eval_losses: totals is NULL");
    if (B > 0 && (!pi || !v || !target_pi || !z || !q || !rows || !flags)) return fail("azg_eval_losses: a required pointer is NULL");
    if (B > 0) k_eval_losses<<<dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream>>>(pi, v, target_pi, z, q, active, B, A, P, q_weight, rows, flags);
    k_eval_totals<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(rows, flags, B, accumulate, totals);
    HIPCHK(hipGetLastError());
    return 0;
}
