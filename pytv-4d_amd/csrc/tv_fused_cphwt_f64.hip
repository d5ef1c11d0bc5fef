// tv_fused_cphwt_f64.hip -- fp64 instantiations of the one-sweep adaptive Huber-TV Chambolle-Pock iteration (tv_fused.h, ALG_CPHWT; 2 columns
// per 16-byte lane): the sweep only, its fix-up is the ALG_CPACC one.
#include "tv_fused_launch.h"

TV_FUSED_INSTANTIATE(double, ALG_CPHWT)
