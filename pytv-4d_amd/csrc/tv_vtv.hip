// tv_vtv.hip -- channel-coupled (vectorial / joint) TV: the M frames of a volume are channels of ONE object, and the l2 norm of the
// regulariser is taken per SPATIAL site s = (z, y, x) over all gradient channels AND all frames (include/pytv4d.h):
//   P(x) = 1/2 |x - x0|^2 + lambda sum_s |D x|_{F,s},   |D x|_{F,s} = ( sum_{m, c} (D x)[z, c, m, y, x]^2 )^(1/2)
// Neither k_D<Epilogue> nor k_gap* can form that norm: their threads own one site of ONE frame.  Here a thread owns one spatial site (z, y,
// one 16-byte x-lane or one scalar x) and walks its M frames, N*N (pitched: frame_pitch) apart; the gradient of a site of a frame is
// d_site (tv_site.h), the code every one-site kernel uses -- the four schemes, mask_static / time_factor / time_weight_vol, reg_z_over_reg,
// the volume edges and the z-halo planes come from that one place.
//
//   k_dual_vtv<S, T, V, M> : q <- (q + sigma D x) * wtv_scale(|q + sigma D x|_{F,s}, lambda), ONE factor per spatial site  (tv_cp_dual_vtv)
//        M > 0   REGISTER form: v of all M frames stays in registers; x and q are read once, q is written once (2 Nd + 1 words per voxel)
//        M == 0  GENERIC form, any frame count: pass 1 accumulates |v|^2 over the frames, pass 2 recomputes v and stores v * scale; no v is
//                kept and none is written unscaled (3 Nd + 2 words per voxel if pass 2 misses every cache)
//   k_gap_vtv<S, T, V>     : the three sums of the duality-gap certificate, reduce-only  (tv_dual_gap_vtv)
#include <hip/hip_runtime.h>

#include "tv_host.h"
#include "tv_stencil.h"
#include "tv_site.h"

namespace tv {

// The square root of a site's norms, CORRECTLY ROUNDED in both dtypes.  tv_device.h's tsqrt is, for fp32, the toolchain's native square root: good
// to one ulp, and lowered to the bare v_sqrt_f32 in some instantiations and to the corrected sequence in others -- which made the register
// form and the generic form disagree by one ulp of a site's factor.  The plain builtin under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt is the IEEE result everywhere, so the two forms give the same q bit for bit.
__device__ __forceinline__ float  vtv_sqrt(float v)  { return __builtin_sqrtf(v); }
__device__ __forceinline__ double vtv_sqrt(double v) { return __builtin_sqrt(v); }
// s += a^2 with ONE rounding per term, spelled out: both forms accumulate a site's norms in the same order with the same roundings, whatever
// the compiler would contract
template <typename T, int V> __device__ __forceinline__ void vtv_add_sq(Vec<T, V>& s, const Vec<T, V>& a) {
#pragma unroll
    for (int i = 0; i < V; ++i) s.v[i] = tfma(a.v[i], a.v[i], s.v[i]);
}
// v = q + sigma D x of one frame of the site, slot by slot, as ONE fused multiply-add per element -- what the compiler makes of
// cp_dual_wtv_site's expression, so a site inside its ball ends with the q that tv_cp_dual_wtv leaves there (tests/test_gpu_cp_vtv.py), and
// spelled out so that pass 1 and pass 2 of the generic form cannot round v differently.  NT: the loads are the last use of q.
template <int S, typename T, int V, bool NT>
__device__ __forceinline__ void vtv_v(const DG& g, const T* base, const Vec<T, V> (&o)[8], T sigma, Vec<T, V> (&v)[8], Vec<T, V>& vs) {
    for_each_channel<S>(g, [&](auto slot, int ch) {
        constexpr int k = decltype(slot)::value;
        const T* p = base + (long long)ch * g.s_z;
        const Vec<T, V> qv = NT ? vload_s<T, V, S == CENTRAL>(p) : vload<T, V>(p);
#pragma unroll
        for (int i = 0; i < V; ++i) v[k].v[i] = tfma(sigma, o[k].v[i], qv.v[i]);
        vtv_add_sq<T, V>(vs, v[k]);
    });
}
template <int S, typename T, int V>
__device__ __forceinline__ void vtv_store(const DG& g, T* base, const Vec<T, V> (&v)[8], const Vec<T, V>& scale) {
    for_each_channel<S>(g, [&](auto slot, int ch) {
        constexpr int k = decltype(slot)::value;
        vstore_s<T, V, S == CENTRAL>(base + (long long)ch * g.s_z, v[k] * scale);
    });
}
template <typename T> __device__ __forceinline__ long long vtv_q_offset(const DG& g, const Coord& c) {
    return (long long)c.zl * g.s_dz + (long long)c.t * g.s_t + (long long)c.y * g.rp + c.col0;
}

// the epilogues d_site hands one frame's gradient slots to; vs / ds: the thread's running |v|^2 and |D x|^2 of the spatial site
template <int S, typename T, int V, bool KEEP> struct VtvAccumulate {      // KEEP: v stays with the caller (register form)
    static constexpr bool REDUCES = true;
    const T* q;
    T sigma;
    Vec<T, V> (*v)[8];
    Vec<T, V>* vs;
    Vec<T, V>* ds;
    __device__ __forceinline__ double operator()(const DG& g, const Coord& c, const Vec<T, V> (&o)[8]) const {
        if constexpr (KEEP) {
            vtv_v<S, T, V, true>(g, q + vtv_q_offset<T>(g, c), o, sigma, *v, *vs);
        } else {
            Vec<T, V> tmp[8];
            vtv_v<S, T, V, false>(g, q + vtv_q_offset<T>(g, c), o, sigma, tmp, *vs);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) vtv_add_sq<T, V>(*ds, o[k]);            // inactive slots are exactly zero
        return 0.0;
    }
};
template <int S, typename T, int V> struct VtvStore {                      // pass 2 of the generic form: v again, stored times the site's factor
    static constexpr bool REDUCES = true;
    T* q;
    T sigma;
    Vec<T, V> scale;
    __device__ __forceinline__ double operator()(const DG& g, const Coord& c, const Vec<T, V> (&o)[8]) const {
        T* base = q + vtv_q_offset<T>(g, c);
        Vec<T, V> v[8];
        Vec<T, V> unused = vsplat<T, V>(T(0));
        vtv_v<S, T, V, true>(g, base, o, sigma, v, unused);
        vtv_store<S, T, V>(g, base, v, scale);
        return 0.0;
    }
};

// grid = launch_cfg(d, V, nz) with ONE frame: blockIdx.y == 0, the thread's frame index is set here
template <int S, typename T, int V, int M>
__global__ __launch_bounds__(256) void k_dual_vtv(DG g, WT<T> w, const T* x, const T* xp, const T* xn, T* q, T sigma, T lambda, double* partials) {
    __shared__ double sm[16];
    Coord c = thread_coord<V>(g, 0);
    double acc = 0.0;
    if (c.ok) {
        Vec<T, V> vs = vsplat<T, V>(T(0)), ds = vs, scale;
        auto finish = [&]() {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                acc += (double)vtv_sqrt(ds.v[i]);
                scale.v[i] = wtv_scale(vtv_sqrt(vs.v[i]), lambda);
            }
        };
        if constexpr (M > 0) {
            Vec<T, V> v[M][8];
#pragma unroll
            for (int t = 0; t < M; ++t) {
                c.t = t;
                d_site<S, T, V>(g, w, x, xp, xn, 1, c, VtvAccumulate<S, T, V, true>{q, sigma, &v[t], &vs, &ds}, PlainMem());
            }
            finish();
#pragma unroll
            for (int t = 0; t < M; ++t) {
                c.t = t;
                vtv_store<S, T, V>(g, q + vtv_q_offset<T>(g, c), v[t], scale);
            }
        } else {
            for (int t = 0; t < g.m; ++t) {
                c.t = t;
                d_site<S, T, V>(g, w, x, xp, xn, 1, c, VtvAccumulate<S, T, V, false>{q, sigma, nullptr, &vs, &ds}, PlainMem());
            }
            finish();
            for (int t = 0; t < g.m; ++t) {
                c.t = t;
                d_site<S, T, V>(g, w, x, xp, xn, 1, c, VtvStore<S, T, V>{q, sigma, scale}, PlainMem());
            }
        }
    }
    acc = block_sum(acc, sm);
    if (threadIdx.x == 0 && threadIdx.y == 0) partials[linear_block_id()] = acc;
}

// one frame of the site for the certificate: D x (slots o) and D^T q at the same voxels, as GapSiteWtv; the frame's |D x|^2 and <q, D x>
// are added per column in fp64 to the site's sums, the fidelity terms go straight to the thread's totals
template <int S, typename T, int V> struct GapSiteVtv {
    static constexpr bool REDUCES = true;
    WT<T> w;
    SrcScaled<T, V> src;     // (scale 1, as in GapSiteHuber)
    const T* x;
    const T* x0;
    double* dsq;             // [V] sum over the frames of |D x|^2
    double* dot;             // [V] sum over the frames of <q, D x>
    double* acc3;            // the calling thread's three sums
    __device__ __forceinline__ double operator()(const DG& g, const Coord& c, const Vec<T, V> (&o)[8]) const {
        long long inpl;
        const Vec<T, V> gd = dt_site<S, T, V>(g, w, src, c, inpl);
        const long long offd = (long long)c.zl * g.s_dz + inpl, off = (long long)c.zl * g.s_z + inpl;
        Vec<T, V> qo = vsplat<T, V>(T(0));
        for_each_channel<S>(g, [&](auto slot, int ch) { qo = qo + src.ld(offd + (long long)ch * g.s_z) * o[decltype(slot)::value]; });
        const Vec<T, V> ds = sumsq_slots<T, V>(o), xv = vload<T, V>(x + off), x0v = vload<T, V>(x0 + off);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const double e = (double)xv.v[i] - (double)x0v.v[i];
            const double r = e + (double)gd.v[i];
            dsq[i] += (double)ds.v[i];
            dot[i] += (double)qo.v[i];
            acc3[1] += 0.5 * e * e;
            acc3[2] += 0.5 * r * r;
        }
        return 0.0;
    }
};
template <int S, typename T, int V>
__global__ __launch_bounds__(256) void k_gap_vtv(DG g, WT<T> w, const T* x, const T* xp, const T* xn, SrcScaled<T, V> src, const T* x0,
                                                  double lambda, double* p_vtv, double* p_fid, double* p_gap) {
    __shared__ double sm[16];
    Coord c = thread_coord<V>(g, 0);
    double a[3] = {0.0, 0.0, 0.0};
    if (c.ok) {
        double dsq[V], dot[V];
#pragma unroll
        for (int i = 0; i < V; ++i) dsq[i] = dot[i] = 0.0;
        for (int t = 0; t < g.m; ++t) {
            c.t = t;
            d_site<S, T, V>(g, w, x, xp, xn, 1, c, GapSiteVtv<S, T, V>{w, src, x, x0, dsq, dot, a}, PlainMem());
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const double n = sqrt(dsq[i]);
            a[0] += n;
            a[2] += lambda * n - dot[i];            // >= 0 for |q_s|_F <= lambda (Cauchy-Schwarz over the joint vector)
        }
    }
    const long long b = linear_block_id();
    const bool first = (threadIdx.x == 0 && threadIdx.y == 0);
    const double vtv = block_sum(a[0], sm);
    if (first) p_vtv[b] = vtv;
    const double fid = block_sum(a[1], sm);
    if (first) p_fid[b] = fid;
    const double gap = block_sum(a[2], sm);
    if (first) p_gap[b] = gap;
}

}  // namespace tv

// the launch geometry of both kernels: launch_cfg's tiles of one plane, one grid row (the frames are walked, not launched)
static LC vtv_cfg(const DG& d, int V) {
    DG one = d;
    one.m = 1;
    return launch_cfg(one, V, d.nz);
}

// ---- which (scheme, M) run the register form ------------------------------------------------------------------------------------------
// v costs 4 Nd VGPRs per frame and 16-byte lane in either dtype: up to 8 frames with the four-channel schemes, up to 4 with hybrid's eight.
// Every instantiation is free of scratch (profiles/vectorial_tv_regs.txt) and the register form is the faster one wherever both were timed
// (profiles/vectorial_tv_bench.txt); every other (scheme, M) runs the generic form.  tv_cp_dual_vtv's dispatch and its instantiations share
// this ONE rule.
using VtvRegMs = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8>;
constexpr bool vtv_reg_form(int scheme, int m) { return m >= 1 && m <= (scheme == HYBRID ? 4 : 8); }

template <int S, typename T, int V, int M>
static void vtv_launch(const LC& lc, hipStream_t st, const tv_geom* g, const DG& d, const void* x, const void* xp, const void* xn, void* q,
                       double sigma, double lambda, double* partials) {
    hipLaunchKernelGGL((k_dual_vtv<S, T, V, M>), lc.grid, lc.block, 0, st, d, make_w<T>(g), (const T*)x, (const T*)xp, (const T*)xn, (T*)q,
                       (T)sigma, (T)lambda, partials);
}

extern "C" {

// Dual step of the channel-coupled model (include/pytv4d.h).  Every argument check precedes the first device access.
// TV_VTV_FORM: 2 = the generic form for every M; any other value (0, unset) = the default rule, the register form where it is instantiated.
int tv_cp_dual_vtv(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, void* q, double sigma_D, double lambda,
                   double* vtv, void* ws, void* stream) {
    DG d;
    if (int rc = make_dg(g, d, true)) return rc;
    if (int rc = wtv_null({{"x", x}, {"q", q}, {"vtv", vtv}, {"ws", ws}})) return rc;
    if (!finite_pos(lambda)) return fail(TV_E_ARG, "lambda must be a finite number > 0");
    if (!finite_pos(sigma_D)) return fail(TV_E_ARG, "sigma_D must be a finite number > 0");
    if (int rc = wtv_halo(check_x_halos(g, d, x_prev, x_next), "x_prev", "x_next")) return rc;
    const bool vec = rows_vectorisable(g, d) && aligned16({x, x_prev, x_next, q, d.wv});
    hipStream_t st = (hipStream_t)stream;
    const Partials P(ws, d);
    const bool generic = env_int("TV_VTV_FORM", 0) == 2;
    long long nblocks = 0;
    int rc = dispatch(g->scheme, g->dtype, vec, [&]<int S, typename T, int V>() -> int {
        const LC lc = vtv_cfg(d, V);
        nblocks = lc.nblocks;
        if (!generic && vtv_reg_form(S, d.m)) {
            if (int rc = dispatch_m(VtvRegMs{}, d.m, "internal: no register form of tv_cp_dual_vtv for this frame count", [&]<int M>() -> int {
                    vtv_launch<S, T, V, vtv_reg_form(S, M) ? M : 0>(lc, st, g, d, x, x_prev, x_next, q, sigma_D, lambda, P.slot(0));
                    return 0;
                }))
                return rc;
        } else {
            vtv_launch<S, T, V, 0>(lc, st, g, d, x, x_prev, x_next, q, sigma_D, lambda, P.slot(0));
        }
        HIP_TRY(hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    return P.reduce(0, nblocks, vtv, st);
}

// P(x) - Dual(q) of the channel-coupled model with its two by-products; reduce-only (include/pytv4d.h).  One kernel form, every geometry:
// the call is made once per convergence check.  Every argument check precedes the first device access.
int tv_dual_gap_vtv(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, const void* q, const void* q_prev,
                    const void* q_next, const void* x0, double lambda, double* out, void* ws, void* stream) {
    DG d;
    if (int rc = make_dg(g, d, true)) return rc;
    if (int rc = wtv_null({{"x", x}, {"q", q}, {"x0", x0}, {"out", out}, {"ws", ws}})) return rc;
    if (!finite_pos(lambda)) return fail(TV_E_ARG, "lambda must be a finite number > 0");
    if (int rc = wtv_halo(check_x_halos(g, d, x_prev, x_next), "x_prev", "x_next")) return rc;
    if (int rc = wtv_halo(check_y_halos(g, d, q_prev, q_next), "q_prev", "q_next")) return rc;
    const bool vec = rows_vectorisable(g, d) && aligned16({x, x_prev, x_next, q, q_prev, q_next, x0, d.wv});
    hipStream_t st = (hipStream_t)stream;
    const Partials P(ws, d);                              // slot 0: sum_s |D x|_F, slot 1: 1/2 |x - x0|^2, slot 2: the gap
    return dispatch(g->scheme, g->dtype, vec, [&]<int S, typename T, int V>() -> int {
        const LC lc = vtv_cfg(d, V);
        SrcScaled<T, V> src{(const T*)q, (const T*)q_prev, (const T*)q_next, T(1)};
        hipLaunchKernelGGL((k_gap_vtv<S, T, V>), lc.grid, lc.block, 0, st, d, make_w<T>(g), (const T*)x, (const T*)x_prev, (const T*)x_next,
                           src, (const T*)x0, lambda, P.slot(0), P.slot(1), P.slot(2));
        HIP_TRY(hipGetLastError());
        return P.reduce_n(3, lc.nblocks, out, st);
    });
}

}  // extern "C"
