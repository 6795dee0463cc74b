// azg_async_preamble.h -- what the two translation units of the asynchronous tree pipeline (azg_async.hip: the net kernel and the C-ABI;
// azg_async_sel.hip: the descent kernel) share in front of azg_async.hip.h.  The units differ in AZG_NN_OPAQUE_TID, in the AZG_ASYNC_PART_*
// they ask for, and in their code-generation flags (build.py).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

// every workgroup of k_async_select runs 16 independent tree waves: wave_sync() must be a wavefront fence (azg_common.hip.h)
#define AZG_WAVE_LOCAL_SYNC 1
#define AZG_FUSED_DEVICE_ONLY 1
#define AZG_NN_KERNEL static
#include "../../include/azg.h"
#include "../../include/azg_testaids.h"
#include "azg_host.h"
#include "azg_common.hip.h"
#include "nn_kernels.hip.h"
#include "nn_v80_h2.hip.h"
#include "nn_conv5x5.hip.h"
#include "nn_mb1d.hip.h"
#include "nn_smallworld.hip.h"
#include "game_santorini.hip.h"
#include "game_azul.hip.h"
#include "game_smallworld.hip.h"
#include "game_minivilles.hip.h"
#include "game_tlp.hip.h"

using namespace azg;
