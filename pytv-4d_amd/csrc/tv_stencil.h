// tv_stencil.h -- per-site stencil arithmetic shared by the one-site-per-thread kernels
// (tv_kernels.hip) and the plane-marching kernels (tv_march.h): the neighbourhood struct, the
// gradient channels of one site for the four schemes, and the fused epilogues.
//
// Per-voxel definitions follow SURVEY 8a-1 / 8a-2, i.e. pytv/tv_operators_CPU.py:117-154,198-218,
// 264-284,330-358 (D) and :398-448,487-516,554-583,622-658 (D^T).
#pragma once
#include <cmath>
#include <type_traits>

#include "tv_device.h"

namespace tv {

// =============================================================================================
// neighbourhood of x around one voxel-vector
// =============================================================================================
template <typename T, int V> struct XN {
    Vec<T, V> c;                 // centre
    Vec<T, V> nr, pr;            // next / previous row
    Vec<T, V> nc, pc;            // next / previous column (shifted vectors)
    Vec<T, V> nz, pz;            // next / previous plane
    Vec<T, V> nt, pt;            // next / previous frame
    bool h_nr, h_pr, h_nz, h_pz, h_nt, h_pt;
    int col0;
};

// How a kernel reaches an array.  PlainMem: ordinary loads / stores (every kernel whose inputs were complete before it started).
// CohMem (tv_small.hip, the persistent small-volume kernels): the array is written by OTHER blocks of the SAME launch -- blocks that may sit
// on another XCD with its own L2 -- so every access is an agent-coherent (sc1) raw-buffer access relative to the array's base
// (profiles/r6_coherence_probe.txt: sc1 store + sc1 load is never stale, plain loads are; repeated sc1 loads of a line hit the L2).
struct PlainMem {
    template <typename T, int V> __device__ __forceinline__ Vec<T, V> ld(const T* p) const { return vload<T, V>(p); }
    template <typename T> __device__ __forceinline__ T ld1(const T* p) const { return *p; }
    template <typename T, int V> __device__ __forceinline__ void st(T* p, const Vec<T, V>& v) const { vstore<T, V>(p, v); }
};
struct CohMem {
    __amdgpu_buffer_rsrc_t r;
    const char* base;
    static constexpr int AUX = 16;                   // sc1 on gfx942 / gfx950
    template <typename T> __device__ __forceinline__ static CohMem make(const T* b, long long nbytes) {
        CohMem m;
        m.r = __builtin_amdgcn_make_buffer_rsrc((void*)b, 0, (int)(nbytes > 0x7fffffffll ? 0x7fffffffll : nbytes), 0x00020000);
        m.base = reinterpret_cast<const char*>(b);
        return m;
    }
    template <typename T> __device__ __forceinline__ int off(const T* p) const { return (int)(reinterpret_cast<const char*>(p) - base); }
    template <typename T> __device__ __forceinline__ T ld1(const T* p) const {
        if constexpr (sizeof(T) == 4) {
            return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(r, off(p), 0, AUX));
        } else {
            typedef int v2i __attribute__((ext_vector_type(2)));
            return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(r, off(p), 0, AUX));
        }
    }
    template <typename T, int V> __device__ __forceinline__ Vec<T, V> ld(const T* p) const {
        if constexpr (V == 1) {
            Vec<T, V> o; o.v[0] = ld1<T>(p); return o;
        } else {
            static_assert(sizeof(Vec<T, V>) == 16, "16-byte lanes");
            typedef int v4i __attribute__((ext_vector_type(4)));
            return __builtin_bit_cast(Vec<T, V>, __builtin_amdgcn_raw_buffer_load_b128(r, off(p), 0, AUX));
        }
    }
    template <typename T, int V> __device__ __forceinline__ void st(T* p, const Vec<T, V>& v) const {
        if constexpr (V == 1 && sizeof(T) == 4) {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v.v[0]), r, off(p), 0, AUX);
        } else if constexpr (V == 1) {
            typedef int v2i __attribute__((ext_vector_type(2)));
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2i, v.v[0]), r, off(p), 0, AUX);
        } else {
            typedef int v4i __attribute__((ext_vector_type(4)));
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i, v), r, off(p), 0, AUX);
        }
    }
};

template <typename T, int V, bool NEXT, bool PREV, typename MP = PlainMem>
__device__ __forceinline__ void load_xn(const DG& g, const T* plane_c, const T* plane_p, const T* plane_n,
                                        const Coord& c, XN<T, V>& o, const MP& mp = MP()) {
    const long long off = (long long)c.t * g.s_t + (long long)c.y * g.rp + c.col0;
    const T* p = plane_c + off;
    o.c = mp.template ld<T, V>(p);
    o.col0 = c.col0;
    const Vec<T, V> zero = vsplat<T, V>(T(0));
    o.nr = o.pr = o.nc = o.pc = o.nz = o.pz = o.nt = o.pt = zero;
    o.h_nr = o.h_pr = o.h_nz = o.h_pz = o.h_nt = o.h_pt = false;
    if (NEXT) {
        o.h_nr = (c.y + 1 < g.ny);
        if (o.h_nr) o.nr = mp.template ld<T, V>(p + g.rp);
        const T tail = (c.col0 + V < g.nx) ? mp.template ld1<T>(p + V) : T(0);
        o.nc = shift_left<T, V>(o.c, tail);
        if (g.za) {
            o.h_nz = (plane_n != nullptr);
            if (o.h_nz) o.nz = mp.template ld<T, V>(plane_n + off);
        }
        if (g.ta) {
            o.h_nt = (c.t + 1 < g.m);
            if (o.h_nt) o.nt = mp.template ld<T, V>(p + g.s_t);
        }
    }
    if (PREV) {
        o.h_pr = (c.y > 0);
        if (o.h_pr) o.pr = mp.template ld<T, V>(p - g.rp);
        const T head = (c.col0 > 0) ? mp.template ld1<T>(p - 1) : T(0);
        o.pc = shift_right<T, V>(o.c, head);
        if (g.za) {
            o.h_pz = (plane_p != nullptr);
            if (o.h_pz) o.pz = mp.template ld<T, V>(plane_p + off);
        }
        if (g.ta) {
            o.h_pt = (c.t > 0);
            if (o.h_pt) o.pt = mp.template ld<T, V>(p - g.s_t);
        }
    }
}

// =============================================================================================
// gradient channels of one voxel-vector, in SLOT order
//   non-hybrid: 0 rows, 1 cols, 2 z, 3 t
//   hybrid    : 0 row-up, 1 col-up, 2 row-down, 3 col-down, 4 z-up, 5 z-down, 6 t-up, 7 t-down
// =============================================================================================
template <int S, typename T, int V>
__device__ __forceinline__ void d_slots(const DG& g, const WT<T>& w, const XN<T, V>& n, const Vec<T, V>& mf,
                                        Vec<T, V> (&o)[8]) {
    const Vec<T, V> zero = vsplat<T, V>(T(0));
    Vec<T, V> f_r = zero, f_c = zero, f_z = zero, f_t = zero;   // forward
    Vec<T, V> b_r = zero, b_c = zero, b_z = zero, b_t = zero;   // backward
    Vec<T, V> c_r = zero, c_c = zero, c_z = zero, c_t = zero;   // central
    constexpr bool FW = (S == UPWIND || S == HYBRID || S == CENTRAL);   // central needs fwd for 2-point axes
    constexpr bool BW = (S == DOWNWIND || S == HYBRID);
    if (FW) {
        if (n.h_nr) f_r = n.nr - n.c;
#pragma unroll
        for (int i = 0; i < V; ++i) f_c.v[i] = (n.col0 + i < g.nx - 1) ? n.nc.v[i] - n.c.v[i] : T(0);
        if (n.h_nz) f_z = w.wz * (n.nz - n.c);
        if (n.h_nt) f_t = (w.wt * (n.nt - n.c)) * mf;
    }
    if (BW) {
        if (n.h_pr) b_r = n.c - n.pr;
#pragma unroll
        for (int i = 0; i < V; ++i) b_c.v[i] = ((unsigned)(n.col0 + i - 1) < (unsigned)(g.nx - 1)) ? n.c.v[i] - n.pc.v[i] : T(0);   // 1 <= col <= nx - 1 (pad columns of a pitched row: 0)
        if (n.h_pz) b_z = w.wz * (n.c - n.pz);
        if (n.h_pt) b_t = (w.wt * (n.c - n.pt)) * mf;
    }
    if (S == CENTRAL) {
        if (n.h_nr && n.h_pr) c_r = n.nr - n.pr;
#pragma unroll
        for (int i = 0; i < V; ++i)
            c_c.v[i] = (n.col0 + i > 0 && n.col0 + i < g.nx - 1) ? n.nc.v[i] - n.pc.v[i] : T(0);
        if (g.z_two) c_z = f_z;
        else if (n.h_nz && n.h_pz) c_z = w.wz * (n.nz - n.pz);
        if (g.t_two) c_t = f_t;
        else if (n.h_nt && n.h_pt) c_t = (w.wt * (n.nt - n.pt)) * mf;
    }
    if (S == UPWIND) { o[0] = f_r; o[1] = f_c; o[2] = f_z; o[3] = f_t; }
    if (S == DOWNWIND) { o[0] = b_r; o[1] = b_c; o[2] = b_z; o[3] = b_t; }
    if (S == CENTRAL) {
        const T h = T(0.5);
        o[0] = h * c_r; o[1] = h * c_c; o[2] = h * c_z; o[3] = h * c_t;
    }
    if (S == HYBRID) {
        const T s = Consts<T>::inv_sqrt2();
        o[0] = s * f_r; o[1] = s * f_c; o[2] = s * b_r; o[3] = s * b_c;
        o[4] = s * f_z; o[5] = s * b_z; o[6] = s * f_t; o[7] = s * b_t;
    }
    if (S != HYBRID) { o[4] = o[5] = o[6] = o[7] = zero; }
}

template <int I> using IC = std::integral_constant<int, I>;

// f(slot, channel) for every ACTIVE channel; slot is a compile-time constant
template <int S, typename F> __device__ __forceinline__ void for_each_channel(const DG& g, F&& f) {
    f(IC<0>{}, 0);
    f(IC<1>{}, 1);
    if (S == HYBRID) {
        f(IC<2>{}, 2);
        f(IC<3>{}, 3);
        if (g.za) { f(IC<4>{}, g.ch_z); f(IC<5>{}, g.ch_z + 1); }
        if (g.ta) { f(IC<6>{}, g.ch_t); f(IC<7>{}, g.ch_t + 1); }
    } else {
        if (g.za) f(IC<2>{}, g.ch_z);
        if (g.ta) f(IC<3>{}, g.ch_t);
    }
}

template <typename T, int V> __device__ __forceinline__ Vec<T, V> sumsq_slots(const Vec<T, V> (&o)[8]) {
    Vec<T, V> s = vsplat<T, V>(T(0));
#pragma unroll
    for (int k = 0; k < 8; ++k) s = s + o[k] * o[k];   // inactive slots are exactly zero
    return s;
}

// =============================================================================================
// epilogues of the forward kernel
// An epilogue that is launched from both kernel forms (one site per thread: k_D / k_DT; plane-marching: k_D_march / k_DT_march) keeps its
// data members in a plain struct XArgs<T> and derives from it: the host names the fields ONCE, where it builds that struct (the entry point
// in tv_kernels.hip), and both launchers take it whole (run_D / run_DT there, tvm::D_march / tvm::DT_march in tv_march_D/DT.hip).
// =============================================================================================
template <typename T> struct StoreDArgs { T* d; double* partials; };
template <int S, typename T, int V> struct StoreD : StoreDArgs<T> {
    static constexpr bool REDUCES = false;
    __device__ __forceinline__ double operator()(const DG& g, const Coord& c, const Vec<T, V> (&o)[8]) const {
        T* base = this->d + (long long)c.zl * g.s_dz + (long long)c.t * g.s_t + (long long)c.y * g.rp + c.col0;
        for_each_channel<S>(g, [&](auto slot, int ch) { vstore<T, V>(base + (long long)ch * g.s_z, o[decltype(slot)::value]); });
        return 0.0;
    }
};

// 1/|Dx| per voxel into an array with one extra plane in front; 0 where |Dx| == 0 (the reference sets
// |Dx| := +inf there so that the site contributes nothing, pytv/tv_GPU.py:88 -- same effect), and also where
// |Dx| is so small that its reciprocal would overflow.  Storing the reciprocal makes pass 2 division-free.
// ONE rule for "the gradient is zero" in every sub-gradient kernel (two-pass NormEpi, one-pass inv_norm, marching
// D_norms): |Dx|^2 below the smallest normal number of the type
template <typename T> __device__ __forceinline__ T tiny_sumsq();
template <> __device__ __forceinline__ float tiny_sumsq<float>() { return 0x1p-126f; }
template <> __device__ __forceinline__ double tiny_sumsq<double>() { return 0x1p-1022; }
template <int S, typename T, int V> struct NormEpi {
    static constexpr bool REDUCES = true;
    T* norms_ext;
    double* partials;
    __device__ __forceinline__ double operator()(const DG& g, const Coord& c, const Vec<T, V> (&o)[8]) const {
        const Vec<T, V> s = sumsq_slots<T, V>(o);
        Vec<T, V> n;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const T r = tsqrt(s.v[i]);
            acc += (double)r;
            n.v[i] = (s.v[i] >= tiny_sumsq<T>()) ? T(1) / r : T(0);
        }
        vstore<T, V>(norms_ext + (long long)(c.zl + 1) * g.s_z + (long long)c.t * g.s_t + (long long)c.y * g.rp + c.col0, n);
        return (c.zl >= 0 && c.zl < g.nz) ? acc : 0.0;
    }
};

// Chambolle-Pock dual update, README.md:149-151 (with keepdims over the channel axis)
// The arithmetic of one site: v = q + sigma D x per channel (q read at `base`), scale = 1 / max(1, |v|_2 / lambda) per column -- the new
// q is v * scale; returns |D x|_2 summed over the columns.  ONE body for the update (CpDual) and for the reduce-only pass that measures
// what the update would change (tv_cp_dual_residual, tv_kernels.hip: CpDualRes).
template <int S, typename T, int V>
__device__ __forceinline__ double cp_dual_site(const DG& g, const T* base, const Vec<T, V> (&o)[8], T sigma, T inv_lambda,
                                               Vec<T, V> (&v)[8], Vec<T, V>& scale) {
    Vec<T, V> vs = vsplat<T, V>(T(0));
    for_each_channel<S>(g, [&](auto slot, int ch) {
        constexpr int k = decltype(slot)::value;
        v[k] = vload_s<T, V, S == CENTRAL>(base + (long long)ch * g.s_z) + sigma * o[k];
        vs = vs + v[k] * v[k];
    });
    const Vec<T, V> ds = sumsq_slots<T, V>(o);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        acc += (double)tsqrt(ds.v[i]);
        scale.v[i] = T(1) / tmax(T(1), tsqrt(vs.v[i]) * inv_lambda);
    }
    return acc;
}
template <typename T> struct CpDualArgs { T* q; T sigma, inv_lambda; double* partials; };
template <int S, typename T, int V> struct CpDual : CpDualArgs<T> {
    static constexpr bool REDUCES = true;
    __device__ __forceinline__ double operator()(const DG& g, const Coord& c, const Vec<T, V> (&o)[8]) const {
        T* base = this->q + (long long)c.zl * g.s_dz + (long long)c.t * g.s_t + (long long)c.y * g.rp + c.col0;
        Vec<T, V> v[8];
        Vec<T, V> scale;
        const double acc = cp_dual_site<S, T, V>(g, base, o, this->sigma, this->inv_lambda, v, scale);
        for_each_channel<S>(g, [&](auto slot, int ch) {
            constexpr int k = decltype(slot)::value;
            vstore_s<T, V, S == CENTRAL>(base + (long long)ch * g.s_z, v[k] * scale);
        });
        return acc;
    }
};

// Chambolle-Pock dual update for the HUBER-TV regulariser lambda sum h_alpha(|D x|_2), h_alpha(t) = t^2 / (2 alpha) for t <= alpha and
// t - alpha / 2 beyond (Chambolle & Pock 2011, section 6.2.1): the conjugate gains (alpha / 2 lambda) |q|^2, so its prox shrinks before it
// projects.  The arithmetic of one site: v = (q + sigma D x) * shrink per channel with shrink = 1 / (1 + sigma alpha / lambda) (formed in
// double by the host), scale = 1 / max(1, |v|_2 / lambda) per column -- the new q is v * scale; returns sum over the columns of
// h_alpha(n), n = |D x|_2, as (n - a) + a^2 / (2 alpha) with a = min(n, alpha): no branch, fp64.  cp_dual_site's sibling: ONE body for the
// update (CpDualHuber), whatever kernel form calls it.
template <int S, typename T, int V>
__device__ __forceinline__ double cp_dual_huber_site(const DG& g, const T* base, const Vec<T, V> (&o)[8], T sigma, T shrink, T inv_lambda,
                                                     double alpha, double half_inv_alpha, Vec<T, V> (&v)[8], Vec<T, V>& scale) {
    Vec<T, V> vs = vsplat<T, V>(T(0));
    for_each_channel<S>(g, [&](auto slot, int ch) {
        constexpr int k = decltype(slot)::value;
        v[k] = shrink * (vload_s<T, V, S == CENTRAL>(base + (long long)ch * g.s_z) + sigma * o[k]);
        vs = vs + v[k] * v[k];
    });
    const Vec<T, V> ds = sumsq_slots<T, V>(o);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const double n = (double)tsqrt(ds.v[i]);
        const double a = fmin(n, alpha);
        acc += (n - a) + (a * a) * half_inv_alpha;
        scale.v[i] = T(1) / tmax(T(1), tsqrt(vs.v[i]) * inv_lambda);
    }
    return acc;
}
template <typename T> struct CpDualHuberArgs { T* q; T sigma, shrink, inv_lambda; double alpha, half_inv_alpha; double* partials; };
template <int S, typename T, int V> struct CpDualHuber : CpDualHuberArgs<T> {
    static constexpr bool REDUCES = true;
    __device__ __forceinline__ double operator()(const DG& g, const Coord& c, const Vec<T, V> (&o)[8]) const {
        T* base = this->q + (long long)c.zl * g.s_dz + (long long)c.t * g.s_t + (long long)c.y * g.rp + c.col0;
        Vec<T, V> v[8];
        Vec<T, V> scale;
        const double acc = cp_dual_huber_site<S, T, V>(g, base, o, this->sigma, this->shrink, this->inv_lambda, this->alpha,
                                                       this->half_inv_alpha, v, scale);
        for_each_channel<S>(g, [&](auto slot, int ch) {
            constexpr int k = decltype(slot)::value;
            vstore_s<T, V, S == CENTRAL>(base + (long long)ch * g.s_z, v[k] * scale);
        });
        return acc;
    }
};

// Chambolle-Pock dual update for the SPATIALLY ADAPTIVE regulariser lambda sum g_i |D x|_{2,i}, g_i >= 0 per voxel (tv_cp_dual_wtv): the
// conjugate differs from plain TV's only in the radius of the ball a site's dual vector is projected onto, r = lambda g_i.  The arithmetic
// of one site: v = q + sigma D x per channel, n = |v|_2, r per column; the new q is v * scale with scale SELECTED per column:
//   r = 0 (g_i = 0)  ->  the constant 0: q = +-0 in every channel, also where n rounds to 0
//   n <= r           ->  the constant 1: v * 1 is v bit for bit (IEEE), never v times a COMPUTED factor that may round off 1
//   n > r            ->  r / n, evaluated for the result only here, where n > r > 0: no 0 / 0 or x / 0 reaches q
// Returns sum over the columns of g_i |D x|_2 in fp64.  gw is the weight at the site (read once: non-temporal).  cp_dual_site's sibling.
// wtv_scale: that selected factor for one column, n = |v|_2 and r = lambda g_i (also the one-sweep kernel's, tv_fused.h ALG_CPHWT).
template <typename T> __device__ __forceinline__ T wtv_scale(T n, T r) { return (r > T(0)) ? ((n > r) ? r / n : T(1)) : T(0); }
template <int S, typename T, int V>
__device__ __forceinline__ double cp_dual_wtv_site(const DG& g, const T* base, const Vec<T, V> (&o)[8], const Vec<T, V>& gw, T sigma, T lambda,
                                                   Vec<T, V> (&v)[8], Vec<T, V>& scale) {
    Vec<T, V> vs = vsplat<T, V>(T(0));
    for_each_channel<S>(g, [&](auto slot, int ch) {
        constexpr int k = decltype(slot)::value;
        v[k] = vload_s<T, V, S == CENTRAL>(base + (long long)ch * g.s_z) + sigma * o[k];
        vs = vs + v[k] * v[k];
    });
    const Vec<T, V> ds = sumsq_slots<T, V>(o);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const T n = tsqrt(vs.v[i]), r = lambda * gw.v[i];
        acc += (double)gw.v[i] * (double)tsqrt(ds.v[i]);
        scale.v[i] = wtv_scale<T>(n, r);
    }
    return acc;
}
template <typename T> struct CpDualWtvArgs { T* q; const T* gw; T sigma, lambda; double* partials; };
template <int S, typename T, int V> struct CpDualWtv : CpDualWtvArgs<T> {
    static constexpr bool REDUCES = true;
    __device__ __forceinline__ double operator()(const DG& g, const Coord& c, const Vec<T, V> (&o)[8]) const {
        const long long inpl = (long long)c.t * g.s_t + (long long)c.y * g.rp + c.col0;
        T* base = this->q + (long long)c.zl * g.s_dz + inpl;
        const Vec<T, V> gv = vload_s<T, V>(this->gw + (long long)c.zl * g.s_z + inpl);
        Vec<T, V> v[8];
        Vec<T, V> scale;
        const double acc = cp_dual_wtv_site<S, T, V>(g, base, o, gv, this->sigma, this->lambda, v, scale);
        for_each_channel<S>(g, [&](auto slot, int ch) {
            constexpr int k = decltype(slot)::value;
            vstore_s<T, V, S == CENTRAL>(base + (long long)ch * g.s_z, v[k] * scale);
        });
        return acc;
    }
};

// Chambolle-Pock dual update for the ADAPTIVE HUBER-TV regulariser lambda sum g_i h_alpha(|D x|_{2,i}), g_i >= 0 per voxel (tv_cp_dual_hwtv):
// the two above combined.  With r = lambda g_i the conjugate of a site's term is alpha |q|^2 / (2 r) + indicator(|q|_2 <= r) (g_i = 0: the
// indicator of q = 0), so its prox shrinks by the site's OWN factor and projects onto the site's own ball.  The arithmetic of one site:
//   shrink = r / (r + sigma alpha) per column, the constant 0 where r = 0 (sigma alpha > 0 is formed in double by the host: no x / 0)
//   v      = shrink (q + sigma D x) per channel,  n = |v|_2
//   q     <- v * wtv_scale(n, r): the select of cp_dual_wtv_site -- inside its ball a site keeps v bit for bit, g_i = 0 keeps q = +-0
// Returns sum over the columns of g_i h_alpha(|D x|_2) in fp64, h_alpha in the branch-free form of cp_dual_huber_site.
template <typename T, int V> __device__ __forceinline__ Vec<T, V> hwtv_shrink(const Vec<T, V>& gw, T lambda, T sigma_alpha) {
    Vec<T, V> sh;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const T r = lambda * gw.v[i];
        sh.v[i] = (r > T(0)) ? r / (r + sigma_alpha) : T(0);
    }
    return sh;
}
template <int S, typename T, int V>
__device__ __forceinline__ double cp_dual_hwtv_site(const DG& g, const T* base, const Vec<T, V> (&o)[8], const Vec<T, V>& gw, T sigma, T lambda,
                                                    T sigma_alpha, double alpha, double half_inv_alpha, Vec<T, V> (&v)[8], Vec<T, V>& scale) {
    const Vec<T, V> shrink = hwtv_shrink<T, V>(gw, lambda, sigma_alpha);
    Vec<T, V> vs = vsplat<T, V>(T(0));
    for_each_channel<S>(g, [&](auto slot, int ch) {
        constexpr int k = decltype(slot)::value;
        v[k] = shrink * (vload_s<T, V, S == CENTRAL>(base + (long long)ch * g.s_z) + sigma * o[k]);
        vs = vs + v[k] * v[k];
    });
    const Vec<T, V> ds = sumsq_slots<T, V>(o);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const double n = (double)tsqrt(ds.v[i]);
        const double a = fmin(n, alpha);
        acc += (double)gw.v[i] * ((n - a) + (a * a) * half_inv_alpha);
        scale.v[i] = wtv_scale<T>(tsqrt(vs.v[i]), lambda * gw.v[i]);
    }
    return acc;
}
template <typename T> struct CpDualHwtvArgs { T* q; const T* gw; T sigma, lambda, sigma_alpha; double alpha, half_inv_alpha; double* partials; };
template <int S, typename T, int V> struct CpDualHwtv : CpDualHwtvArgs<T> {
    static constexpr bool REDUCES = true;
    __device__ __forceinline__ double operator()(const DG& g, const Coord& c, const Vec<T, V> (&o)[8]) const {
        const long long inpl = (long long)c.t * g.s_t + (long long)c.y * g.rp + c.col0;
        T* base = this->q + (long long)c.zl * g.s_dz + inpl;
        const Vec<T, V> gv = vload_s<T, V>(this->gw + (long long)c.zl * g.s_z + inpl);
        Vec<T, V> v[8];
        Vec<T, V> scale;
        const double acc = cp_dual_hwtv_site<S, T, V>(g, base, o, gv, this->sigma, this->lambda, this->sigma_alpha, this->alpha,
                                                      this->half_inv_alpha, v, scale);
        for_each_channel<S>(g, [&](auto slot, int ch) {
            constexpr int k = decltype(slot)::value;
            vstore_s<T, V, S == CENTRAL>(base + (long long)ch * g.s_z, v[k] * scale);
        });
        return acc;
    }
};

// ADMM: v = Dx + u;  z = v * max(0, 1 - thresh/|v|);  u = v - z.   tform: the first array receives t = z - u_new
// (= 2 z - v) instead of z: the next right-hand side x0 + rho D^T (z - u) then reads ONE gradient array
template <typename T> struct AdmmZUArgs { T* z; T* u; T thresh; double* partials; int tform = 0; };
template <int S, typename T, int V> struct AdmmZU : AdmmZUArgs<T> {
    static constexpr bool REDUCES = true;
    __device__ __forceinline__ double operator()(const DG& g, const Coord& c, const Vec<T, V> (&o)[8]) const {
        const long long off = (long long)c.zl * g.s_dz + (long long)c.t * g.s_t + (long long)c.y * g.rp + c.col0;
        Vec<T, V> v[8];
        Vec<T, V> vs = vsplat<T, V>(T(0));
        for_each_channel<S>(g, [&](auto slot, int ch) {
            constexpr int k = decltype(slot)::value;
            v[k] = o[k] + vload<T, V>(this->u + off + (long long)ch * g.s_z);
            vs = vs + v[k] * v[k];
        });
        const Vec<T, V> ds = sumsq_slots<T, V>(o);
        Vec<T, V> scale;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            acc += (double)tsqrt(ds.v[i]);
            const T nv = tsqrt(vs.v[i]);
            scale.v[i] = (nv > T(0)) ? tmax(T(0), T(1) - this->thresh / nv) : T(0);
        }
        for_each_channel<S>(g, [&](auto slot, int ch) {
            constexpr int k = decltype(slot)::value;
            const Vec<T, V> zz = v[k] * scale;
            const Vec<T, V> un = v[k] - zz;
            vstore<T, V>(this->z + off + (long long)ch * g.s_z, this->tform ? zz - un : zz);
            vstore<T, V>(this->u + off + (long long)ch * g.s_z, un);
        });
        return acc;
    }
};

// out = x + rho * D^T D x from the HYBRID channel slots (D^T D is the same operator for upwind, downwind and
// hybrid: sum_a w_a^2 (bwd_a - fwd_a)); the slots hold s*w*fwd / s*w*bwd with s = 1/sqrt(2).  Marching path only.
template <int S, typename T, int V> struct NormalEpi {
    static constexpr bool REDUCES = true;
    static_assert(S == HYBRID, "evaluated with the hybrid channel slots");
    T* out;
    T rho, wz, wt, sf;
    const uint8_t* mask;
    double* partials;
    __device__ __forceinline__ double operator()(const DG& g, const Coord& c, const Vec<T, V> (&o)[8], const Vec<T, V>& xc) const {
        const T inv_s = T(1.4142135623730950488);
        Vec<T, V> r = (o[2] - o[0]) + (o[3] - o[1]);
        if (g.za) r = r + wz * (o[5] - o[4]);
        if (g.ta) {
            Vec<T, V> rt = wt * (o[7] - o[6]);                     // the slots already carry one mask factor
            if (mask != nullptr || g.tf != nullptr) rt = rt * mask_factor<T, V>(g, sf, c.y, c.col0);
            r = r + rt;
        }
        Vec<T, V> ov;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            ov.v[i] = xc.v[i] + rho * (inv_s * r.v[i]);
            acc += (double)xc.v[i] * (double)ov.v[i];
        }
        vstore<T, V>(out + (long long)c.zl * g.s_z + (long long)c.t * g.s_t + (long long)c.y * g.rp + c.col0, ov);
        return acc;
    }
};

// =============================================================================================
// sub-gradient of one site (radius-1 schemes):  with f = forward, b = backward difference at the site,
//   D up-channel at p-e equals (w b)(p), D down-channel at p+e equals (w f)(p), so
//   G(p) = s * sum_a [ up: d_b/n(p-e) - d_f/n(p) ] + [ down: d_b/n(p) - d_f/n(p+e) ],  d = ((w diff) mf) s as in D;
//   1/n comes precomputed from pass 1 (NormEpi), so this is multiplications only
// =============================================================================================
template <typename T, int V>
__device__ __forceinline__ Vec<T, V> div_where(const Vec<T, V>& d, const Vec<T, V>& inv_n, bool valid) {
    Vec<T, V> r = vsplat<T, V>(T(0));
    if (valid) r = d * inv_n;                                         // inv_n == 0 where |Dx| == 0
    return r;
}

// sub-gradient of one site-vector from the radius-1 neighbourhoods of x (xs) and of 1/|Dx| (ns)
// mf_prev / mf_next (weight volume only): the time-channel factor of the voxel one frame back / ahead -- D_up(p - e_t)
// carries the factor of frame t-1 and D_down(p + e_t) that of frame t+1; nullptr: the factor does not depend on t
template <int S, typename T, int V>
__device__ __forceinline__ Vec<T, V> subgrad_site(const DG& g, const WT<T>& w, const XN<T, V>& xs, const XN<T, V>& ns,
                                                  const Vec<T, V>& mf, const Vec<T, V>* mf_prev = nullptr,
                                                  const Vec<T, V>* mf_next = nullptr) {
    static_assert(S != CENTRAL, "radius-2 scheme");
    constexpr bool UP = (S == UPWIND || S == HYBRID), DN = (S == DOWNWIND || S == HYBRID);
    const T s = (S == HYBRID) ? Consts<T>::inv_sqrt2() : T(1);
    const Vec<T, V> zero = vsplat<T, V>(T(0));
    Vec<T, V> r = zero;
    auto axis = [&](const Vec<T, V>& nxt, const Vec<T, V>& prv, bool hn, bool hp, const Vec<T, V>& n_nxt, const Vec<T, V>& n_prv,
                    T wa, bool weighted, bool timeax) {
        Vec<T, V> f = hn ? nxt - xs.c : zero, b = hp ? xs.c - prv : zero;
        if (weighted) { f = wa * f; b = wa * b; }
        if (timeax) { f = f * mf; b = b * mf; }
        if (S == HYBRID) { f = s * f; b = s * b; }
        if (UP) r = r + (div_where<T, V>(b, n_prv, hp) - div_where<T, V>(f, ns.c, hn));
        if (DN) r = r + (div_where<T, V>(b, ns.c, hp) - div_where<T, V>(f, n_nxt, hn));
    };
    axis(xs.nr, xs.pr, xs.h_nr, xs.h_pr, ns.nr, ns.pr, T(1), false, false);
#pragma unroll
    for (int i = 0; i < V; ++i) {      // columns: validity per element
        const int col = xs.col0 + i;
        const bool hn = col < g.nx - 1, hp = col > 0;
        T fi = hn ? xs.nc.v[i] - xs.c.v[i] : T(0), bi = hp ? xs.c.v[i] - xs.pc.v[i] : T(0);
        if (S == HYBRID) { fi *= s; bi *= s; }
        T acc = T(0);
        if (UP) acc += (hp ? bi * ns.pc.v[i] : T(0)) - (hn ? fi * ns.c.v[i] : T(0));
        if (DN) acc += (hp ? bi * ns.c.v[i] : T(0)) - (hn ? fi * ns.nc.v[i] : T(0));
        r.v[i] += acc;
    }
    if (g.za) axis(xs.nz, xs.pz, xs.h_nz, xs.h_pz, ns.nz, ns.pz, w.wz, true, false);
    if (g.ta && mf_prev == nullptr) axis(xs.nt, xs.pt, xs.h_nt, xs.h_pt, ns.nt, ns.pt, w.wt, true, true);
    if (g.ta && mf_prev != nullptr) {
        Vec<T, V> f = xs.h_nt ? xs.nt - xs.c : zero, b = xs.h_pt ? xs.c - xs.pt : zero;
        f = w.wt * f; b = w.wt * b;
        Vec<T, V> f_c = f * mf, b_c = b * mf, b_p = b * (*mf_prev), f_n = f * (*mf_next);
        if (S == HYBRID) { f_c = s * f_c; b_c = s * b_c; b_p = s * b_p; f_n = s * f_n; }
        if (UP) r = r + (div_where<T, V>(b_p, ns.pt, xs.h_pt) - div_where<T, V>(f_c, ns.c, xs.h_nt));
        if (DN) r = r + (div_where<T, V>(b_c, ns.c, xs.h_pt) - div_where<T, V>(f_n, ns.nt, xs.h_nt));
    }
    if (S == HYBRID) r = s * r;
    return r;
}

// =============================================================================================
// transposed operator: sources and epilogues
// =============================================================================================
template <typename T, int V> struct SrcPlain {
    const T* y;
    const T* yp;     // halo plane z0-1 of the backward-looking z channel
    const T* yn;     // halo plane z0+nz of the forward-looking z channel
    __device__ __forceinline__ Vec<T, V> ld(long long off) const { return vload<T, V>(y + off); }
    __device__ __forceinline__ T lds(long long off) const { return y[off]; }
    __device__ __forceinline__ Vec<T, V> ldp(long long off) const { return vload<T, V>(yp + off); }
    __device__ __forceinline__ Vec<T, V> ldn(long long off) const { return vload<T, V>(yn + off); }
};
template <typename T, int V> struct SrcDiff {    // a - b, halos already differenced
    const T* a;
    const T* b;
    const T* yp;
    const T* yn;
    __device__ __forceinline__ Vec<T, V> ld(long long off) const { return vload<T, V>(a + off) - vload<T, V>(b + off); }
    __device__ __forceinline__ T lds(long long off) const { return a[off] - b[off]; }
    __device__ __forceinline__ Vec<T, V> ldp(long long off) const { return vload<T, V>(yp + off); }
    __device__ __forceinline__ Vec<T, V> ldn(long long off) const { return vload<T, V>(yn + off); }
};

template <typename T> struct StoreDTArgs { T* out; double* partials; };
template <typename T, int V> struct StoreDT : StoreDTArgs<T> {
    static constexpr bool REDUCES = false;
    __device__ __forceinline__ double operator()(long long off, const Vec<T, V>& r) const {
        vstore<T, V>(this->out + off, r);
        return 0.0;
    }
};
template <typename T> struct AxpyDTArgs {
    T* out;
    const T* base;
    T alpha;
    double* partials;
    const T* base2 = nullptr;       // tv_DT_axpy2: the primal step of Chambolle-Pock with a data-fidelity operator,
    T beta = T(0);                  // x - tau A^T p - tau D^T q in one pass (base = x, base2 = A^T p, beta = alpha = -tau)
};
template <typename T, int V> struct AxpyDT : AxpyDTArgs<T> {     // out = base + beta * base2 + alpha * r
    static constexpr bool REDUCES = false;
    __device__ __forceinline__ double operator()(long long off, const Vec<T, V>& r) const {
        Vec<T, V> b = (this->base != nullptr) ? vload_s<T, V>(this->base + off) : vsplat<T, V>(T(0));
        if (this->base2 != nullptr) b = b + this->beta * vload_s<T, V>(this->base2 + off);
        vstore_s<T, V>(this->out + off, b + this->alpha * r);
        return 0.0;
    }
};
// Chambolle-Pock primal step with the fidelity-dual update folded in, README.md:148,154,157
template <typename T> struct CpPrimalArgs { T* x; const T* x0; T* p; T tau, sigma_a, inv_1p_sigma_a; double* partials; };
template <typename T, int V> struct CpPrimal : CpPrimalArgs<T> {
    static constexpr bool REDUCES = true;
    __device__ __forceinline__ double operator()(long long off, const Vec<T, V>& r) const {
        const Vec<T, V> xv = vload_s<T, V>(this->x + off), x0v = vload_s<T, V>(this->x0 + off), pv = vload_s<T, V>(this->p + off);
        Vec<T, V> pn, xn;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            pn.v[i] = (pv.v[i] + this->sigma_a * (xv.v[i] - x0v.v[i])) * this->inv_1p_sigma_a;
            xn.v[i] = (xv.v[i] - this->tau * pn.v[i]) - this->tau * r.v[i];
            const double e = (double)xn.v[i] - (double)x0v.v[i];
            acc += 0.5 * e * e;
        }
        vstore_s<T, V>(this->p + off, pn);
        vstore_s<T, V>(this->x + off, xn);
        return acc;
    }
};

// Accelerated Chambolle-Pock primal step (Chambolle & Pock 2011, Algorithm 2, for the 1-strongly convex fidelity 1/2 |x - x0|^2):
//   x_new = (x - tau D^T q + tau x0) / (1 + tau);  x_bar = x_new + theta (x_new - x);  x = x_new          (tv_cp_primal_accel)
// inv_1p_tau = 1 / (1 + tau) is formed by the host in double.  x and x_bar are different arrays; pads stay zero (r, x, x0 are zero there).
template <typename T> struct CpPrimalAccelArgs { T* x; T* x_bar; const T* x0; T tau, inv_1p_tau, theta; double* partials; };
template <typename T, int V> struct CpPrimalAccel : CpPrimalAccelArgs<T> {
    static constexpr bool REDUCES = true;
    __device__ __forceinline__ double operator()(long long off, const Vec<T, V>& r) const {
        const Vec<T, V> xv = vload_s<T, V>(this->x + off), x0v = vload_s<T, V>(this->x0 + off);
        Vec<T, V> xn, xb;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            xn.v[i] = ((xv.v[i] - this->tau * r.v[i]) + this->tau * x0v.v[i]) * this->inv_1p_tau;
            xb.v[i] = xn.v[i] + this->theta * (xn.v[i] - xv.v[i]);
            const double e = (double)xn.v[i] - (double)x0v.v[i];
            acc += 0.5 * e * e;
        }
        vstore_s<T, V>(this->x + off, xn);
        vstore_s<T, V>(this->x_bar + off, xb);
        return acc;
    }
};

// Chambolle-Pock primal step with a POINTWISE PROX of the fidelity F(x - x0) (Chambolle & Pock 2011, Algorithm 1 / section 6.2.2: TV-L1;
// tv_cp_primal_prox).  With e = (x - tau D^T q) - x0 every fidelity here has  prox_{tau F}(e) = e - clamp(c e, -t, t):
//   L1     c = 1                    t = tau      the soft threshold; inside the dead zone c e == e, so e - e == 0 and x_new == x0 bit for bit
//   Huber  c = tau / (delta + tau)  t = tau
//   L2     c = tau / (1 + tau)      t = +inf
// c and t are formed by the host in double.  One multiply, one three-way median, one subtract per element; no branch.
//   STORE:  x_new = x0 + prox(e);  x_bar = x_new + theta (x_new - x);  x = x_new;  sum F(x_new - x0)          Nd + 4 words per voxel
//   !STORE: reduce-only -- sum ((x - x_new) / tau)^2, the fixed-point residual of the fidelity block; x, x0 read, nothing written
// F in fp64 from a = min(|e|, cap):  (|e| - a) + a^2 half_inv   (L1: cap = 0, half_inv = 0; Huber: cap = delta, half_inv = 1 / (2 delta);
// L2: cap = +inf, half_inv = 1/2).  Pads stay zero (r, x, x0 are zero there: e = 0, prox(0) = 0).
__device__ __forceinline__ float  tclamp(float v, float t)   { return __builtin_amdgcn_fmed3f(v, -t, t); }
__device__ __forceinline__ double tclamp(double v, double t) { return fmin(fmax(v, -t), t); }
template <typename T> struct CpPrimalProxArgs { T* x; T* x_bar; const T* x0; T tau, theta, c, t; double cap, half_inv, inv_tau; double* partials; };
template <typename T, int V, bool STORE> struct CpPrimalProxT : CpPrimalProxArgs<T> {
    static constexpr bool REDUCES = true;
    __device__ __forceinline__ double operator()(long long off, const Vec<T, V>& r) const {
        const Vec<T, V> xv = vload_s<T, V>(this->x + off), x0v = vload_s<T, V>(this->x0 + off);
        Vec<T, V> xn, xb;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const T e = (xv.v[i] - this->tau * r.v[i]) - x0v.v[i];
            xn.v[i] = x0v.v[i] + (e - tclamp(this->c * e, this->t));
            if (STORE) {
                xb.v[i] = xn.v[i] + this->theta * (xn.v[i] - xv.v[i]);
                const double ae = fabs((double)xn.v[i] - (double)x0v.v[i]);
                const double a = fmin(ae, this->cap);
                acc += (ae - a) + a * a * this->half_inv;
            } else {
                const double d = ((double)xv.v[i] - (double)xn.v[i]) * this->inv_tau;
                acc += d * d;
            }
        }
        if (STORE) {
            vstore_s<T, V>(this->x + off, xn);
            vstore_s<T, V>(this->x_bar + off, xb);
        }
        return acc;
    }
};
template <typename T, int V> using CpPrimalProx = CpPrimalProxT<T, V, true>;       // the <typename, int> forms the launchers take: pick_store
template <typename T, int V> using CpPrimalProxRes = CpPrimalProxT<T, V, false>;

// Chambolle-Pock primal step for the POISSON data term, the generalised Kullback-Leibler divergence F(x) = sum (x - x0 + x0 log(x0 / x)) over
// x >= 0 with counts x0 >= 0 (0 log 0 = 0; tv_cp_primal_kl).  With v = x - tau D^T q and b = v - tau the prox is the positive root of
// x^2 - b x - tau x0:  prox_{tau F}(v) = (b + s) / 2,  s = sqrt(b^2 + 4 tau x0).  For b << 0 that sum cancels to nothing, so the root is taken
// in the form that adds magnitudes on either side of b = 0 (the two are the same number: (b + s)(s - b) = 4 tau x0):
//   x_new = b >= 0 ? (b + s) / 2 : 2 tau x0 / (s - b)                         a select; both arms are evaluated
// two_tau and four_tau are formed by the host in double.  Exact by construction: x0 = 0 with b < 0 gives 0 / (2 |b|) = 0 (x0 = 0 with b >= 0
// gives b), and a pad element (r = x = x0 = 0, so b = -tau) stays 0 however the square root rounds.  x0 >= 0 is the caller's contract.
//   STORE:  x_bar = x_new + theta (x_new - x);  x = x_new;  sum F(x_new) in fp64                              Nd + 4 words per voxel
//   !STORE: reduce-only -- sum ((x - x_new) / tau)^2, the fixed-point residual of the fidelity block; x, x0 read, nothing written.  Exactly
//           0 at a site that is a fixed point in exact arithmetic with representable data (see below), which x - x_new need not be.
__device__ __forceinline__ float  tlog1p(float v)  { return log1pf(v); }
__device__ __forceinline__ double tlog1p(double v) { return log1p(v); }
// one site of F: x - x0 + x0 log(x0 / x) = x0 (u - log1p(u)) with u = (x - x0) / x0, evaluated in T (>= 0 term by term: u >= log1p(u)) and
// accumulated in fp64 by the caller; x where x0 == 0.  (A double-precision log per voxel showed through the memory traffic: DESIGN.md 3.6.)
template <typename T> __device__ __forceinline__ double kl_term(T xn, T x0) {
    const T u = (xn - x0) / x0;
    return (double)(x0 > T(0) ? x0 * (u - tlog1p(u)) : xn);
}
template <typename T> struct CpPrimalKLArgs { T* x; T* x_bar; const T* x0; T tau, theta, two_tau, four_tau; double inv_tau; double* partials; };
template <typename T, int V, bool STORE> struct CpPrimalKLT : CpPrimalKLArgs<T> {
    static constexpr bool REDUCES = true;
    __device__ __forceinline__ double operator()(long long off, const Vec<T, V>& r) const {
        const Vec<T, V> xv = vload_s<T, V>(this->x + off), x0v = vload_s<T, V>(this->x0 + off);
        Vec<T, V> xn, xb;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const T b = (xv.v[i] - this->tau * r.v[i]) - this->tau;
            const T s = tsqrt(tfma(b, b, this->four_tau * x0v.v[i]));
            const T hi = T(0.5) * (b + s), lo = (this->two_tau * x0v.v[i]) / (s - b);
            xn.v[i] = b >= T(0) ? hi : lo;
            if (STORE) {
                xb.v[i] = xn.v[i] + this->theta * (xn.v[i] - xv.v[i]);
                acc += kl_term(xn.v[i], x0v.v[i]);
            } else {
                // x_new - x = (s - c) / 2 with c = 2 x - b = x + tau (1 + r), and s^2 - c^2 = 4 tau (x0 - x (1 + r)): for c >= 0 the
                // displacement is taken from that numerator, which is an exact 0 at a fixed point (x = x0, r = 0: a constant image).
                // The numerator is rounded in T: near a fixed point that is not exactly one it cancels, and (x_new - x) / tau carries
                // about 2 eps (x0 + |x| |1 + r|) / (s + c) per site -- bounded by the eps |x| / tau that x - x_new carries, so the sum
                // equals sum ((x - x_new) / tau)^2 to rounding, not bit for bit.
                const T c = (xv.v[i] + this->tau * r.v[i]) + this->tau;
                const double den = (double)s + (double)c;
                const double moved = 2.0 * (double)(x0v.v[i] - xv.v[i] * (T(1) + r.v[i])) / den;
                const double d = (c >= T(0) && den > 0.0) ? moved : ((double)xn.v[i] - (double)xv.v[i]) * this->inv_tau;
                acc += d * d;
            }
        }
        if (STORE) {
            vstore_s<T, V>(this->x + off, xn);
            vstore_s<T, V>(this->x_bar + off, xb);
        }
        return acc;
    }
};
template <typename T, int V> using CpPrimalKL = CpPrimalKLT<T, V, true>;
template <typename T, int V> using CpPrimalKLRes = CpPrimalKLT<T, V, false>;

// Chambolle-Pock primal step for a WEIGHTED quadratic data term with a BOX: F(x) = 1/2 sum w (x - x0)^2 + indicator(lo <= x <= hi), with a
// per-voxel weight w >= 0 (tv_cp_primal_wls; w = 0: the voxel is unknown and TV fills it in -- inpainting, Chambolle & Pock 2011, section
// 6.3; w = 1 / sigma^2: heteroscedastic least squares).  F is separable, so the prox of tau F is the clamp of the quadratic's prox.  With
// v = x - tau D^T q and c = tau w / (1 + tau w):
//   x_new = clamp(v - c (v - x0), lo, hi)
// -- this form, not (v + tau w x0) / (1 + tau w), for what it makes exact: w == 0 gives c == 0 and x_new = clamp(v) bit for bit; v == x0 gives
// x0 bit for bit, so a constant image inside the box with q = 0 is left where it is and its residual is exactly 0.  One divide, one fused
// multiply-add, one three-way median per element; no branch.  lo / hi may be -inf / +inf.
//   STORE:  x_bar = x_new + theta (x_new - x);  x = x_new;  sum 1/2 w (x_new - x0)^2 in fp64                  Nd + 5 words per voxel
//   !STORE: reduce-only -- sum ((x - x_new) / tau)^2, the fixed-point residual of the fidelity block; x, x0, w read, nothing written (Nd + 3)
// Pads stay zero: r, x, x0 and w are zero there, so x_new = clamp(0), and the entry point takes boxes with lo <= 0 <= hi only.
// The caller's contract: w finite and >= 0, tau w finite.
__device__ __forceinline__ float  tclamp3(float v, float lo, float hi)    { return __builtin_amdgcn_fmed3f(v, lo, hi); }
__device__ __forceinline__ double tclamp3(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }
template <typename T> struct CpPrimalWLSArgs { T* x; T* x_bar; const T* x0; const T* w; T tau, theta, lo, hi; double inv_tau; double* partials; };
template <typename T, int V, bool STORE> struct CpPrimalWLST : CpPrimalWLSArgs<T> {
    static constexpr bool REDUCES = true;
    __device__ __forceinline__ double operator()(long long off, const Vec<T, V>& r) const {
        const Vec<T, V> xv = vload_s<T, V>(this->x + off), x0v = vload_s<T, V>(this->x0 + off), wv = vload_s<T, V>(this->w + off);
        Vec<T, V> xn, xb;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const T v = xv.v[i] - this->tau * r.v[i];
            const T tw = this->tau * wv.v[i];
            const T c = tw / (T(1) + tw);
            xn.v[i] = tclamp3(v - c * (v - x0v.v[i]), this->lo, this->hi);
            if (STORE) {
                xb.v[i] = xn.v[i] + this->theta * (xn.v[i] - xv.v[i]);
                const double e = (double)xn.v[i] - (double)x0v.v[i];
                acc += 0.5 * (double)wv.v[i] * e * e;
            } else {
                const double d = ((double)xv.v[i] - (double)xn.v[i]) * this->inv_tau;
                acc += d * d;
            }
        }
        if (STORE) {
            vstore_s<T, V>(this->x + off, xn);
            vstore_s<T, V>(this->x_bar + off, xb);
        }
        return acc;
    }
};
template <typename T, int V> using CpPrimalWLS = CpPrimalWLST<T, V, true>;
template <typename T, int V> using CpPrimalWLSRes = CpPrimalWLST<T, V, false>;

// =============================================================================================
// duality gap of 1/2 |x - x0|^2 + lambda |D x|_{2,1} at (x, qs = qscale q), reduce-only (tv_dual_gap): with gd = D^T qs
//   gap = sum_sites [ 1/2 (x - x0 + gd)^2 + lambda |D x|_2 - <qs, D x> ]      both parts >= 0 site by site for |qs|_2 <= lambda
// Each site's term is formed from the T-valued stencil results and accumulated in fp64; nothing is stored.
// =============================================================================================
// the dual variable as the gather sees it: q scaled by a constant (ADMM: q = u, qscale = rho; Chambolle-Pock: 1)
template <typename T, int V> struct SrcScaled {
    const T* y;
    const T* yp;
    const T* yn;
    T s;
    __device__ __forceinline__ Vec<T, V> ld(long long off) const { return s * vload<T, V>(y + off); }
    __device__ __forceinline__ T lds(long long off) const { return s * y[off]; }
    __device__ __forceinline__ Vec<T, V> ldp(long long off) const { return s * vload<T, V>(yp + off); }
    __device__ __forceinline__ Vec<T, V> ldn(long long off) const { return s * vload<T, V>(yn + off); }
};
// the three per-site terms from D x (slots o), the site's own samples of qs (slots qv), x, x0 and gd; sums over the V columns
template <typename T, int V>
__device__ __forceinline__ void gap_terms(const Vec<T, V> (&o)[8], const Vec<T, V> (&qv)[8], const Vec<T, V>& xv, const Vec<T, V>& x0v,
                                          const Vec<T, V>* gd, double lambda, double& a_tv, double& a_fid, double& a_gap) {
    const Vec<T, V> ds = sumsq_slots<T, V>(o);
    Vec<T, V> dot = vsplat<T, V>(T(0));
#pragma unroll
    for (int k = 0; k < 8; ++k) dot = dot + qv[k] * o[k];              // inactive slots are exactly zero in o
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const T nrm = tsqrt(ds.v[i]);
        const double e = (double)xv.v[i] - (double)x0v.v[i];
        a_tv += (double)nrm;
        a_fid += 0.5 * e * e;
        a_gap += lambda * (double)nrm - (double)dot.v[i];
        if (gd != nullptr) {
            const double r = e + (double)gd->v[i];
            a_gap += 0.5 * r * r;
        }
    }
}
// The same three terms for the Huber-TV model 1/2 |x - x0|^2 + lambda sum h_alpha(|D x|_2) at (x, q), |q|_2 <= lambda (tv_dual_gap_huber):
//   gap = sum_sites [ 1/2 (x - x0 + gd)^2 + lambda h_alpha(|D x|_2) - <q, D x> + (alpha / 2 lambda) |q|^2 ]
// The regulariser part is >= 0 site by site (Fenchel-Young).  Where |D x|_2 <= alpha it IS the square (lambda / 2 alpha) |D x - (alpha /
// lambda) q|^2 and is summed as that square; beyond alpha it is lambda (n - alpha / 2) - <q, D x> + (alpha / 2 lambda) |q|^2.  a_hub
// receives h_alpha(|D x|_2) in cp_dual_huber_site's form.  The constants are host doubles; fp64 throughout, from the T-valued stencil results.
struct HuberGapConsts {
    double lambda, alpha, half_inv_alpha;      // 1 / (2 alpha)
    double a_over_l, l_over_2a, a_over_2l;     // alpha / lambda, lambda / (2 alpha), alpha / (2 lambda)
};
template <typename T, int V>
__device__ __forceinline__ void gap_terms_huber(const Vec<T, V> (&o)[8], const Vec<T, V> (&qv)[8], const Vec<T, V>& xv, const Vec<T, V>& x0v,
                                                const Vec<T, V>& gd, const HuberGapConsts& k, double& a_hub, double& a_fid, double& a_gap) {
    const Vec<T, V> ds = sumsq_slots<T, V>(o);
    // one column at a time, its index a compile-time constant: the nested channel loop keeps the compiler from unrolling a run-time
    // column loop, and a run-time index into the lanes puts them into scratch
    auto column = [&]<int I>(IC<I>) {
        const double n = (double)tsqrt(ds.v[I]);
        const double a = fmin(n, k.alpha);
        double sq = 0.0, dot = 0.0, qq = 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {                                  // inactive slots are exactly zero in o and in qv
            const double d = (double)o[c].v[I], qc = (double)qv[c].v[I];
            const double e = d - k.a_over_l * qc;
            sq += e * e;
            dot += qc * d;
            qq += qc * qc;
        }
        const double e = (double)xv.v[I] - (double)x0v.v[I];
        const double r = e + (double)gd.v[I];
        a_hub += (n - a) + (a * a) * k.half_inv_alpha;
        a_fid += 0.5 * e * e;
        a_gap += 0.5 * r * r + (n <= k.alpha ? k.l_over_2a * sq : k.lambda * (n - 0.5 * k.alpha) - dot + k.a_over_2l * qq);
    };
    [&]<int... I>(std::integer_sequence<int, I...>) { (column(IC<I>{}), ...); }(std::make_integer_sequence<int, V>{});
}
// gap_terms for the spatially adaptive model 1/2 |x - x0|^2 + lambda sum g_i |D x|_{2,i} at (x, q), |q|_2 <= lambda g_i per site
// (tv_dual_gap_wtv): the radius lambda g_i of the site in place of lambda.  a_wtv receives g_i |D x|_2; the site's gap term is
// 1/2 (x - x0 + gd)^2 + (lambda g_i |D x|_2 - <q, D x>), both parts >= 0 for a feasible q (Cauchy-Schwarz), never formed as P - Dual.
template <typename T, int V>
__device__ __forceinline__ void gap_terms_wtv(const Vec<T, V> (&o)[8], const Vec<T, V> (&qv)[8], const Vec<T, V>& xv, const Vec<T, V>& x0v,
                                              const Vec<T, V>& gv, const Vec<T, V>& gd, double lambda, double& a_wtv, double& a_fid, double& a_gap) {
    const Vec<T, V> ds = sumsq_slots<T, V>(o);
    Vec<T, V> dot = vsplat<T, V>(T(0));
#pragma unroll
    for (int k = 0; k < 8; ++k) dot = dot + qv[k] * o[k];              // inactive slots are exactly zero in o
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const double gn = (double)gv.v[i] * (double)tsqrt(ds.v[i]);
        const double e = (double)xv.v[i] - (double)x0v.v[i];
        const double r = e + (double)gd.v[i];
        a_wtv += gn;
        a_fid += 0.5 * e * e;
        a_gap += 0.5 * r * r + (lambda * gn - (double)dot.v[i]);
    }
}
// The same three terms for the adaptive Huber-TV model 1/2 |x - x0|^2 + lambda sum g_i h_alpha(|D x|_{2,i}) at (x, q), |q|_2 <= r_i = lambda g_i per
// site and q = 0 where g_i = 0 (tv_dual_gap_hwtv).  a_hwtv receives g_i h_alpha(|D x|_2); the site's gap term is
//   1/2 (x - x0 + gd)^2  +  ( r_i h_alpha(n) + [r_i > 0] alpha |q|^2 / (2 r_i) - <q, D x> ),    n = |D x|_2,
// both parts >= 0 (Fenchel-Young).  As in gap_terms_huber the second part is summed as the perfect square (r_i / 2 alpha) |D x - (alpha / r_i) q|^2
// where n <= alpha and r_i > 0; where r_i = 0 it is - <q, D x>, which is 0 for the q = 0 the dual kernel leaves.  fp64 throughout; the
// per-site constants alpha / r_i ... are formed from g_i here (one division per column; the call runs once per convergence check).
template <typename T, int V>
__device__ __forceinline__ void gap_terms_hwtv(const Vec<T, V> (&o)[8], const Vec<T, V> (&qv)[8], const Vec<T, V>& xv, const Vec<T, V>& x0v,
                                               const Vec<T, V>& gv, const Vec<T, V>& gd, double lambda, double alpha, double half_inv_alpha,
                                               double& a_hwtv, double& a_fid, double& a_gap) {
    const Vec<T, V> ds = sumsq_slots<T, V>(o);
    auto column = [&]<int I>(IC<I>) {          // one column at a time, its index a compile-time constant (gap_terms_huber)
        const double n = (double)tsqrt(ds.v[I]);
        const double a = fmin(n, alpha);
        const double h = (n - a) + (a * a) * half_inv_alpha;
        const double r = lambda * (double)gv.v[I];
        const double a_over_r = (r > 0.0) ? alpha / r : 0.0;
        double sq = 0.0, dot = 0.0, qq = 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {                                  // inactive slots are exactly zero in o and in qv
            const double d = (double)o[c].v[I], qc = (double)qv[c].v[I];
            const double e = d - a_over_r * qc;
            sq += e * e;
            dot += qc * d;
            qq += qc * qc;
        }
        const double e = (double)xv.v[I] - (double)x0v.v[I];
        const double rr = e + (double)gd.v[I];
        a_hwtv += (double)gv.v[I] * h;
        a_fid += 0.5 * e * e;
        a_gap += 0.5 * rr * rr + ((r > 0.0 && n <= alpha) ? r * half_inv_alpha * sq : r * h - dot + 0.5 * a_over_r * qq);
    };
    [&]<int... I>(std::integer_sequence<int, I...>) { (column(IC<I>{}), ...); }(std::make_integer_sequence<int, V>{});
}
// D-side pass of the plane-marching form (k_D_march): |D x|_{2,1}, 1/2 |x - x0|^2 and sum (lambda |D x|_2 - <qs, D x>); reads x0 and q once.
// The D^T-side pass (GapDT) ran BEFORE it on the same grid and left its per-block sums in `partials`: finish() adds to them.
template <typename T> struct GapDArgs {
    const T* q;
    const T* x0;
    T qscale;
    double lambda;
    double* p_tv;
    double* p_fid;
    double* partials;     // the gap sums (the name k_D_march expects of an epilogue)
};
template <int S, typename T, int V> struct GapD : GapDArgs<T> {
    static constexpr bool REDUCES = false;       // three sums, written by finish()
    double a_tv = 0.0, a_fid = 0.0, a_gap = 0.0;
    __device__ __forceinline__ double operator()(const DG& g, const Coord& c, const Vec<T, V> (&o)[8], const Vec<T, V>& xc) {
        const long long inpl = (long long)c.t * g.s_t + (long long)c.y * g.rp + c.col0;
        const T* base = this->q + (long long)c.zl * g.s_dz + inpl;
        Vec<T, V> qv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) qv[k] = vsplat<T, V>(T(0));
        for_each_channel<S>(g, [&](auto slot, int ch) {
            qv[decltype(slot)::value] = this->qscale * vload_s<T, V>(base + (long long)ch * g.s_z);
        });
        const Vec<T, V> x0v = vload_s<T, V>(this->x0 + (long long)c.zl * g.s_z + inpl);
        gap_terms<T, V>(o, qv, xc, x0v, nullptr, this->lambda, a_tv, a_fid, a_gap);
        return 0.0;
    }
    __device__ __forceinline__ void finish(double* sm) {
        const long long b = linear_block_id();
        const bool first = (threadIdx.x == 0 && threadIdx.y == 0);
        const double tv = block_sum(a_tv, sm);
        if (first) this->p_tv[b] = tv;
        const double fid = block_sum(a_fid, sm);
        if (first) this->p_fid[b] = fid;
        const double gap = block_sum(a_gap, sm);
        if (first) this->partials[b] = this->partials[b] + gap;
    }
};
// D^T-side pass of the plane-marching form (k_DT_march): sum 1/2 (x - x0 + qscale D^T q)^2; reads x and x0 once
template <typename T> struct GapDTArgs { const T* x; const T* x0; T qscale; double* partials; };
template <typename T, int V> struct GapDT : GapDTArgs<T> {
    static constexpr bool REDUCES = true;
    __device__ __forceinline__ double operator()(long long off, const Vec<T, V>& r) const {
        const Vec<T, V> xv = vload_s<T, V>(this->x + off), x0v = vload_s<T, V>(this->x0 + off);
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const double e = ((double)xv.v[i] - (double)x0v.v[i]) + (double)(this->qscale * r.v[i]);
            acc += 0.5 * e * e;
        }
        return acc;
    }
};

// One axis of the gather.  MODE 0: y^(p-e) - y^(p)   (adjoint of a forward difference)
//                          MODE 1: y^(p) - y^(p+e)   (adjoint of a backward difference)
//                          MODE 2: y^(p-e) - y^(p+e) (adjoint of a central difference)
// y^ = y with the samples the forward operator never writes forced to zero.
// lo/hi are the loaded neighbour vectors; pos/n the coordinate along the axis and its extent.
template <int MODE, typename T, int V>
__device__ __forceinline__ Vec<T, V> adj_axis(int pos, int n, const Vec<T, V>& lo, const Vec<T, V>& ce, const Vec<T, V>& hi) {
    const Vec<T, V> zero = vsplat<T, V>(T(0));
    if (MODE == 0) return ((pos >= 1) ? lo : zero) - ((pos <= n - 2) ? ce : zero);
    if (MODE == 1) return ((pos >= 1) ? ce : zero) - ((pos <= n - 2) ? hi : zero);
    return ((pos >= 2) ? lo : zero) - ((pos <= n - 3) ? hi : zero);
}


}  // namespace tv
