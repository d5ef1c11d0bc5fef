// tv_march_D.hip -- instantiations + launchers of the plane-marching FORWARD kernels (tv_march.h).
#include "tv_host.h"
#include "tv_stencil.h"
#include "tv_march.h"

// SKIP: the (scheme, M) to leave out -- wide16() or wtv_spill16() of tv_host.h; the caller keeps those geometries on the one-site kernel
constexpr bool skip_none(int, int) { return false; }
template <template <int, typename, int> class EpiT, bool (*SKIP)(int, int) = skip_none, typename Args>
static int launch_D_march(Call& c, const Args& args) {
    const int zc = march_zchunk(c.d);
    const LC lc = march_cfg(c.d, zc);
    c.nblocks = lc.nblocks;
    return dispatch_scheme_m(MarchMs{}, c.g->scheme, c.d.m, kNoMarchSM, [&]<int S, int M>() -> int {
        if constexpr (SKIP(S, M)) {
            return fail(TV_E_ARG, kNoMarchSM);
        } else {
            EpiT<S, float, 4> epi{args};
            hipLaunchKernelGGL((k_D_march<S, M, EpiT<S, float, 4>>), lc.grid, lc.block, 0, c.st, c.d, make_w<float>(c.g), (const float*)c.c,
                               (const float*)c.prev, (const float*)c.next, zc, epi);
            HIP_TRY(hipGetLastError());
            return 0;
        }
    });
}

namespace tvm {
int D_march(Call& c, const StoreDArgs<float>& a) { return launch_D_march<StoreD>(c, a); }
int D_march(Call& c, const CpDualArgs<float>& a) { return launch_D_march<CpDual>(c, a); }
int D_march(Call& c, const CpDualHuberArgs<float>& a) { return launch_D_march<CpDualHuber, wide16>(c, a); }
int D_march(Call& c, const CpDualWtvArgs<float>& a) { return launch_D_march<CpDualWtv, wtv_spill16>(c, a); }
// CpDualHwtv is NOT instantiated in k_D_march: CpDualWtv already leaves (central, 8) one wave per SIMD and spills with 16 frames, and this
// epilogue carries more per site.  tv_cp_dual_hwtv never asks for the marching form; the one-site kernel runs on every geometry.
int D_march(Call&, const CpDualHwtvArgs<float>&) { return fail(TV_E_ARG, kNoMarchSM); }
int D_march(Call& c, const AdmmZUArgs<float>& a) { return launch_D_march<AdmmZU>(c, a); }
int D_march(Call& c, const GapDArgs<float>& a) { return launch_D_march<GapD>(c, a); }
int D_norms(const tv_geom* g, const DG& d, const void* x, const void* xp, const void* xn, hipStream_t st, long long* nb,
            float* norms_ext, double* partials, int ghost_lo, int ghost_hi) {
    const int zc = march_zchunk(d);
    LC lc = march_cfg(d, zc);
    const int planes = d.nz + ghost_lo + ghost_hi;
    lc.grid.y = (unsigned)((planes + zc - 1) / zc);
    lc.nblocks = (long long)lc.grid.x * lc.grid.y;
    *nb = lc.nblocks;
    return dispatch_scheme_m(MarchMs{}, g->scheme, d.m, kNoMarchSM, [&]<int S, int M>() -> int {
        NormEpi<S, float, 4> epi{norms_ext, partials};
        // low-traffic epilogue: M = 8 requests the whole next plane and the halo rows at the top of the z step
        // (PF = 2, 2 waves/SIMD); smaller M take the LIGHT variant (3 waves/SIMD, single-buffered tile), 15-20 %
        // faster than the default one here (measured); M = 16 fits neither
        if constexpr (M == 8)
            hipLaunchKernelGGL((k_D_march<S, M, NormEpi<S, float, 4>, false, 2>), lc.grid, lc.block, 0, st, d, make_w<float>(g),
                               (const float*)x, (const float*)xp, (const float*)xn, zc, epi, 2, -ghost_lo, d.nz + ghost_hi);
        else if constexpr (M < 8)
            hipLaunchKernelGGL((k_D_march<S, M, NormEpi<S, float, 4>, true>), lc.grid, lc.block, 0, st, d, make_w<float>(g),
                               (const float*)x, (const float*)xp, (const float*)xn, zc, epi, 2, -ghost_lo, d.nz + ghost_hi);
        else
            hipLaunchKernelGGL((k_D_march<S, M, NormEpi<S, float, 4>>), lc.grid, lc.block, 0, st, d, make_w<float>(g), (const float*)x,
                               (const float*)xp, (const float*)xn, zc, epi, 2, -ghost_lo, d.nz + ghost_hi);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}
int D_normal_op(const tv_geom* g, const DG& d, const void* x, const void* xp, const void* xn, hipStream_t st, long long* nb,
                float* out, float rho, double* partials) {
    const int zc = march_zchunk(d);
    const LC lc = march_cfg(d, zc);
    *nb = lc.nblocks;
    const WT<float> w = make_w<float>(g);
    NormalEpi<HYBRID, float, 4> epi{out, rho, w.wz, w.wt, w.sf, d.mask, partials};
    return dispatch_m(MarchMs{}, d.m, kNoMarchSM, [&]<int M>() -> int {
        if constexpr (M == 8) {
            // whole next plane + halo rows requested at the top of the z step: 1.61 -> 1.28 ms on 64x8x1024x1024
            hipLaunchKernelGGL((k_D_march<HYBRID, M, NormalEpi<HYBRID, float, 4>, false, 2>), lc.grid, lc.block, 0, st, d, w,
                               (const float*)x, (const float*)xp, (const float*)xn, zc, epi, 2, 0, -1);
            HIP_TRY(hipGetLastError());
            return 0;
        }
        if constexpr (M <= 8) {          // (M == 8 returned above; its instantiation of this form stays part of the library)
            hipLaunchKernelGGL((k_D_march<HYBRID, M, NormalEpi<HYBRID, float, 4>, true>), lc.grid, lc.block, 0, st, d, w,
                               (const float*)x, (const float*)xp, (const float*)xn, zc, epi, 2, 0, -1);
            HIP_TRY(hipGetLastError());
            return 0;
        }
        return fail(TV_E_ARG, "marching normal operator: M > 8");
    });
}
}  // namespace tvm
