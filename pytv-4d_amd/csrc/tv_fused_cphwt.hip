// tv_fused_cphwt.hip -- fp32 instantiations of the one-sweep ADAPTIVE Huber-TV Chambolle-Pock iteration (tv_fused.h, ALG_CPHWT): the sweep only --
// its fix-up is the ALG_CPACC one (tv_fused_cpacc.hip).  The entry point tv_cp_hwtv_sweep lives in tv_fused.hip.
#include "tv_fused_launch.h"

TV_FUSED_INSTANTIATE(float, ALG_CPHWT)
