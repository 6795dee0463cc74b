// azg_async_sel.hip -- fourth translation unit: the DESCENT kernel of the asynchronous tree pipeline and its launcher (the net kernel and the
// C-ABI are azg_async.hip, which says why they are two units).
#include "azg_async_preamble.h"

#define AZG_ASYNC_PART_SELECT 1
#include "azg_async.hip.h"
