// tv_fused_cpacc.hip -- fp32 instantiations of the one-sweep ACCELERATED Chambolle-Pock iteration (tv_fused.h, ALG_CPACC): the sweep and
// its two-array fix-up.  The entry points tv_cp_accel_sweep / tv_cp_accel_fixup live in tv_fused.hip.
#include "tv_fused_launch.h"

TV_FUSED_INSTANTIATE(float, ALG_CPACC)
