// tv_fused_cpacc_f64.hip -- fp64 instantiations of the one-sweep accelerated Chambolle-Pock iteration (tv_fused.h, ALG_CPACC; 2 columns
// per 16-byte lane).
#include "tv_fused_launch.h"

TV_FUSED_INSTANTIATE(double, ALG_CPACC)
