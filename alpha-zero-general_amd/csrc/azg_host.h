// host-side helpers shared by the translation units of libazg_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <string>

int azg_fail(const std::string& m);               // records the message for azg_last_error(), returns -1
static inline int fail(const std::string& m) { return azg_fail(m); }
#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(_e)); } while (0)

// Launch kernel K with `lds` bytes of dynamic LDS and check the launch.  More than 64 KiB needs the kernel's limit raised first: once per
// kernel instantiation AND per device (a function attribute belongs to the device that was current when it was set).  The limit is always
// all of the CU's 160 KiB that the kernel's static LDS leaves, never `lds`: one kernel may be launched with several sizes.  (Two threads
// that both find the flag clear both set the attribute: harmless.)
constexpr size_t AZG_LDS_MAX = 160 * 1024;
template <auto K, class... A>
static int launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, A... args) {
    if (lds > AZG_LDS_MAX) return fail("launch_lds: more dynamic LDS than the 160 KiB of a CU");
    if (lds > 64 * 1024) {
        static std::atomic<bool> raised[64];
        int device = 0;
        HIPCHK(hipGetDevice(&device));
        if (device < 0 || device >= 64) return fail("launch_lds: device index out of range");
        if (!raised[device].load(std::memory_order_acquire)) {
            hipFuncAttributes fa;                   // (the runtime refuses a limit that exceeds 160 KiB together with the kernel's static LDS)
            HIPCHK(hipFuncGetAttributes(&fa, (const void*)K));
            HIPCHK(hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(AZG_LDS_MAX - fa.sharedSizeBytes)));
            raised[device].store(true, std::memory_order_release);
        }
    }
    K<<<grid, block, lds, s>>>(args...);
    HIPCHK(hipGetLastError());
    return 0;
}

// internal (not part of include/azg.h): what azg_fused.hip needs from a forest handle owned by azg.hip
struct azg_forest;
namespace azg { struct ForestDev; }
const azg::ForestDev* azg_forest_dev_internal(azg_forest* f, int* game, int* variant, double* dirichlet_alpha);

// objects another translation unit hangs on a forest handle (the argument blocks / queues of the round kernels in azg_nn.hip): owned by
// the forest, released by azg_forest_destroy through `deleter` -- nothing is keyed by a forest's address, which a later forest can inherit
void azg_forest_attach(azg_forest* f, const char* key, void* obj, void (*deleter)(void*));
void* azg_forest_attached(azg_forest* f, const char* key);
