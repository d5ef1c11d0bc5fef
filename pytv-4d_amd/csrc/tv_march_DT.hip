// tv_march_DT.hip -- instantiations + launchers of the plane-marching TRANSPOSED kernels (tv_march.h).
#include "tv_host.h"
#include "tv_stencil.h"
#include "tv_march.h"

template <template <typename, int> class EpiT, template <typename> class Args, typename T>
static int launch_DT_march(Call& c, const Args<T>& args) {
    constexpr int V = 16 / (int)sizeof(T);
    const int zc = march_zchunk(c.d);
    const LC lc = march_cfg(c.d, zc);
    c.nblocks = lc.nblocks;
    return dispatch_scheme_m(MarchMs{}, c.g->scheme, c.d.m, kNoMarchSM, [&]<int S, int M>() -> int {
        EpiT<T, V> epi{args};
        hipLaunchKernelGGL((k_DT_march<S, M, EpiT<T, V>, T>), lc.grid, lc.block, 0, c.st, c.d, make_w<T>(c.g), (const T*)c.c,
                           (const T*)c.prev, (const T*)c.next, zc, epi);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

namespace tvm {
int DT_march(Call& c, const StoreDTArgs<float>& a) { return launch_DT_march<StoreDT>(c, a); }
int DT_march(Call& c, const StoreDTArgs<double>& a) {
    // as AxpyDT with no base and alpha = 1 (tv_march.h: the StoreDT instantiation for double takes 256 VGPRs or spills)
    return launch_DT_march<AxpyDT>(c, AxpyDTArgs<double>{a.out, nullptr, 1.0, nullptr, nullptr, 0.0});
}
int DT_march(Call& c, const AxpyDTArgs<float>& a) { return launch_DT_march<AxpyDT>(c, a); }
int DT_march(Call& c, const AxpyDTArgs<double>& a) { return launch_DT_march<AxpyDT>(c, a); }
int DT_march(Call& c, const CpPrimalArgs<float>& a) { return launch_DT_march<CpPrimal>(c, a); }
int DT_march(Call& c, const CpPrimalAccelArgs<float>& a) { return launch_DT_march<CpPrimalAccel>(c, a); }
int DT_march(Call& c, const CpPrimalProxArgs<float>& a, bool store) {
    return pick_store<CpPrimalProx, CpPrimalProxRes>(store, [&]<template <typename, int> class E>() { return launch_DT_march<E>(c, a); });
}
int DT_march(Call& c, const CpPrimalKLArgs<float>& a, bool store) {
    return pick_store<CpPrimalKL, CpPrimalKLRes>(store, [&]<template <typename, int> class E>() { return launch_DT_march<E>(c, a); });
}
int DT_march(Call& c, const CpPrimalWLSArgs<float>& a, bool store) {
    return pick_store<CpPrimalWLS, CpPrimalWLSRes>(store, [&]<template <typename, int> class E>() { return launch_DT_march<E>(c, a); });
}
int DT_march(Call& c, const GapDTArgs<float>& a) { return launch_DT_march<GapDT>(c, a); }
}  // namespace tvm
