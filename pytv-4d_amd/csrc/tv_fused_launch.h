// tv_fused_launch.h -- launch templates of the one-sweep kernels (tv_fused.h).  One (dtype, ALG) pair per translation unit
// (tv_fused.hip: float CP, tv_fused_f64.hip: double CP, tv_fused_admm.hip / tv_fused_admm_f64.hip: ADMM, tv_fused_cpop*.hip: the
// operator sweep, tv_fused_cpacc*.hip: the accelerated iteration, tv_fused_cphub*.hip: the Huber-TV iteration, tv_fused_cphwt*.hip: the adaptive
// Huber-TV iteration) so that the
// sets of instantiations compile next to each other; the extern "C" entry points and the launch geometry live in tv_fused.hip.
#pragma once
#include "tv_host.h"
#include "tv_stencil.h"
#include "tv_fused.h"

// launch geometry of the fix-up classes (tv_fused.h, k_cp_fixup)
struct FixPlan {
    dim3 g0, g1, g2, g3;
    long long n0, n1, n2, n3;
    int chunk_lo, zc, zb, zn;
    bool xw;
};

inline constexpr const char* kNoFusedSM = "unsupported (scheme, M) for the one-sweep path";

// the sweep: every M <= 8 has its own instantiation, more frames run as time windows of CP_TWN = 8 frames (M == 0 below).
// ADMM is built with the in-block column hand-off only (XW; TV_FUSED_XW=0 is a debugging switch of the CP sweep).
template <typename T, int ALG>
static int fused_sweep_launch(const tv_geom* g, const DG& d, const LC& lc, hipStream_t st, const FusedArgsT<T>& a, int zc, int chunk0, bool xw,
                              bool force_win) {
    if (ALG != ALG_CP && !xw) return fail(TV_E_ARG, "the ADMM / operator / accelerated sweeps are built with TV_FUSED_XW=1 only");
    const bool win = d.m > CP_TWN || force_win || cphwt_windowed(ALG, g->scheme, d.m, (int)sizeof(T));
    return dispatch_scheme_m(WindowedMs{}, g->scheme, win ? 0 : d.m, kNoFusedSM, [&]<int S, int M>() -> int {
        if constexpr (cphwt_windowed(ALG, S, M, (int)sizeof(T))) {
            return fail(TV_E_ARG, kNoFusedSM);          // (not reached: `win` sends these to M == 0)
        } else if constexpr (M == 0) {          // M > 8: windows of 8 frames, or one ragged window (force_win, cphwt_windowed)
            if (xw) hipLaunchKernelGGL((k_cp_fused<S, CP_TWN, true, true, T, ALG>), lc.grid, lc.block, 0, st, d, make_w<T>(g), a, zc, chunk0);
            else if constexpr (ALG == ALG_CP)
                hipLaunchKernelGGL((k_cp_fused<S, CP_TWN, false, true, T, ALG>), lc.grid, lc.block, 0, st, d, make_w<T>(g), a, zc, chunk0);
        } else if (xw) hipLaunchKernelGGL((k_cp_fused<S, M, true, false, T, ALG>), lc.grid, lc.block, 0, st, d, make_w<T>(g), a, zc, chunk0);
        else if constexpr (ALG == ALG_CP)
            hipLaunchKernelGGL((k_cp_fused<S, M, false, false, T, ALG>), lc.grid, lc.block, 0, st, d, make_w<T>(g), a, zc, chunk0);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

template <typename T, int ALG>
static int fused_fixup_launch(const tv_geom* g, const DG& d, hipStream_t st, const FixupArgsT<T>& a, const FixPlan& p, double* w0) {
    if (ALG != ALG_CP && !p.xw) return fail(TV_E_ARG, "the ADMM / operator / accelerated sweeps are built with TV_FUSED_XW=1 only");
    // the Huber-TV sweeps have no fix-up kernel of their own (no k_cp_fixup instantiation): tv_cp_accel_fixup, ALG_CPACC, serves them unchanged
    if (alg_borrows_fixup(ALG)) return fail(TV_E_ARG, "internal: the fix-up of the Huber-TV sweeps is the ALG_CPACC one");
    const dim3 blk(64, 4, 1);
    return dispatch_scheme(g->scheme, [&]<int S>() -> int {
        auto launch = [&]<bool XW>() -> int {
            if constexpr ((ALG == ALG_CP || XW) && !alg_borrows_fixup(ALG)) {
                hipLaunchKernelGGL((k_cp_fixup<S, 0, XW, T, ALG>), p.g0, blk, 0, st, d, make_w<T>(g), a, p.zc, p.zb, p.zn, w0);
                if (d.za) hipLaunchKernelGGL((k_cp_fixup<S, 1, XW, T, ALG>), p.g1, blk, 0, st, d, make_w<T>(g), a, p.zc, p.zb, p.zn, w0 + p.n0);
                hipLaunchKernelGGL((k_cp_fixup<S, 2, XW, T, ALG>), p.g2, blk, 0, st, d, make_w<T>(g), a, p.zc, p.zb, p.zn, w0 + p.n0 + p.n1);
                if (p.n3 > 0)
                    hipLaunchKernelGGL((k_cp_fixup<S, 3, XW, T, ALG>), p.g3, blk, 0, st, d, make_w<T>(g), a, p.zc, p.zb, p.zn, w0 + p.n0 + p.n1 + p.n2);
                HIP_TRY(hipGetLastError());
            }
            return 0;
        };
        return p.xw ? launch.template operator()<true>() : launch.template operator()<false>();
    });
}

// one definition per (dtype, ALG), each in its own translation unit
namespace tvm {
template <typename T, int ALG>
int fused_sweep(const tv_geom* g, const DG& d, const LC& lc, hipStream_t st, const FusedArgsT<T>& a, int zc, int chunk0, bool xw, bool force_win);
template <typename T, int ALG> int fused_fixup(const tv_geom* g, const DG& d, hipStream_t st, const FixupArgsT<T>& a, const FixPlan& p, double* w0);
}  // namespace tvm

#define TV_FUSED_INSTANTIATE(T, ALG)                                                                                                       \
    namespace tvm {                                                                                                                        \
    template <>                                                                                                                            \
    int fused_sweep<T, ALG>(const tv_geom* g, const DG& d, const LC& lc, hipStream_t st, const FusedArgsT<T>& a, int zc, int chunk0, bool xw, \
                            bool force_win) {                                                                                              \
        return fused_sweep_launch<T, ALG>(g, d, lc, st, a, zc, chunk0, xw, force_win);                                                     \
    }                                                                                                                                      \
    template <> int fused_fixup<T, ALG>(const tv_geom* g, const DG& d, hipStream_t st, const FixupArgsT<T>& a, const FixPlan& p, double* w0) { \
        return fused_fixup_launch<T, ALG>(g, d, st, a, p, w0);                                                                             \
    }                                                                                                                                      \
    }
