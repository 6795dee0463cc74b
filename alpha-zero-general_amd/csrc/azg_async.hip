// azg_async.hip -- third translation unit of libazg_hip.so: the asynchronous tree pipeline (azg_async.hip.h: persistent descent workgroups +
// persistent net workgroups, device-side queues): its NET kernel and its C-ABI.  The descent kernel is azg_async_sel.hip: the two
// kernels want different code generation (build.py: machine LICM off takes the forward from 32.3 to 26.6 us and the descent from 23.2 to
// 30.6 us).
#define AZG_NN_OPAQUE_TID 1        /* nn_kernels.hip.h nn_tid(): nothing thread-derived is hoisted out of the persistent net kernel's loop */
#include "azg_async_preamble.h"

#define AZG_ASYNC_PART_NET 1
#include "azg_async.hip.h"
