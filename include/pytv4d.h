/* pytv4d.h -- C-ABI of the MI355X-native PyTV-4D hot path (libpytv4d_hip.so).
 *
 * Drop-in boundary: these entry points are what a binding of the reference's L2/L3 Python API
 * (pytv/tv_operators_GPU.py, pytv/tv_GPU.py) calls instead of torch.nn.functional.conv3d +
 * slice-assign.  Plain pointers and sizes only; every pointer is a DEVICE pointer unless the
 * comment says otherwise; every function enqueues on the caller's hipStream_t (passed as
 * void*, NULL = default stream) and returns without synchronising.
 *
 * Return value: 0 = ok, <0 = argument error (TV_E_*), >0 = hipError_t of a failed HIP call.
 * tv_last_error() gives a human readable message for the calling thread.
 *
 * Layouts (C-contiguous, cols fastest; pytv/tv_operators_CPU.py:82-83,96-97):
 *   image     x : (nz, m, ny, nx)
 *   gradient  d : (nz, nd, m, ny, nx)      channel axis between z and time
 * Channel order: rows, cols, [z], [t]; hybrid: row-up, col-up, row-down, col-down,
 * [z-up, z-down], [t-up, t-down]  (pytv/tv_operators_CPU.py:117-152).
 *
 * z-slab sharding: a rank holds planes [z0, z0+nz) of a volume of nz_global planes.  Halo
 * arguments point to the neighbouring ranks' boundary planes (m*ny*nx elements each); they may be
 * NULL when the corresponding global plane does not exist or is not needed by the scheme.
 */
#ifndef PYTV4D_H
#define PYTV4D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TV_UPWIND   0
#define TV_DOWNWIND 1
#define TV_CENTRAL  2
#define TV_HYBRID   3

#define TV_F32 0
#define TV_F64 1

#define TV_E_ARG      (-1)   /* NULL / negative size / unknown enum            */
#define TV_E_HALO     (-2)   /* a halo plane the scheme needs was not supplied */
#define TV_E_CHANNELS (-3)   /* nd does not match scheme and active axes       */

/* Geometry and weights of one z-slab.  Mirrors the keyword arguments every reference operator
 * takes: reg_z_over_reg, reg_time, mask_static, factor_reg_static
 * (pytv/tv_operators_GPU.py:134,253,362,471,583,719,828,938; pytv/tv_GPU.py:47,142,217,290). */
/* Version of the binary interface declared in this header: bumped whenever tv_geom, the workspace layout or the
 * meaning of an entry point's arguments changes incompatibly (round 1: 1; round 2 added the three weight-volume
 * pointers and a second partial-sum array in the workspace: 2; round 3 added the two leading fields below: 3;
 * round 4 added row_pitch / frame_pitch at the end: 4; round 5 grew the workspace to THREE partial-sum arrays
 * (TV_CP_FID_BOTH, tv_cheb_step(dots = NULL)), gave tv_cp_sweep its flags and changed tv_cheb_step's NULL-dots contract -- stamped as 5
 * in round 6, together with the persistent small-volume entry points tv_small_*).
 * Every entry point that takes a tv_geom rejects a struct whose struct_size / abi_version are not the library's own
 * with TV_E_ARG -- a host built against an older header fails loudly instead of having its trailing fields read as
 * garbage.  tv_geom_init() fills the two fields in. */
#define TV_ABI_VERSION 5

typedef struct tv_geom {
    uint32_t struct_size;       /* sizeof(tv_geom) of the header the HOST was compiled against   */
    uint32_t abi_version;       /* TV_ABI_VERSION of that header                                  */
    int64_t nz;                 /* planes held by this rank                                  */
    int64_t m, ny, nx;          /* time frames, rows, cols                                   */
    int64_t nz_global;          /* planes of the whole volume (== nz when not sharded)       */
    int64_t z0;                 /* global index of local plane 0                             */
    int32_t scheme;             /* TV_UPWIND .. TV_HYBRID                                    */
    int32_t dtype;              /* TV_F32 / TV_F64                                           */
    double  reg_z_over_reg;     /* z weight; z axis active iff nz_global > 1 and this > 0    */
    double  reg_time;           /* time weight; time axis active iff m > 1 and this > 0      */
    double  factor_reg_static;  /* time channels scaled by sqrt(this) where mask_static != 0 */
    const uint8_t* mask_static; /* device, ny*nx bytes, or NULL (the reference's `False`)    */
    const void* time_factor;    /* device, ny*nx elements of `dtype`, or NULL: per-pixel multiplier f(y,x) of the
                                 * time channels, i.e. f^2 is a per-pixel weight on reg_time.  Generalises
                                 * (mask_static, factor_reg_static), which is f = mask ? sqrt(factor) : 1 -- the
                                 * "weight matrix" of the reference's to-do list (README.md:258); both may be set,
                                 * the factors multiply */
    const void* time_weight_vol;/* device, nz*m*ny*nx elements of `dtype`, or NULL: per-VOXEL multiplier f(z,t,y,x) of the
                                 * time channels (f^2 = weight on reg_time at that voxel): the reference's to-do "weight matrix
                                 * of size Nz x M x N x N" (README.md:258), local planes of the slab.  Multiplies with the two
                                 * per-pixel forms above.  D scales the time channel of a voxel by f at THAT voxel; D^T is the
                                 * exact adjoint (every sample is scaled by its own voxel's f before the difference), which for
                                 * a weight that does not vary along t is the reference's "scale the time part at the output
                                 * voxel" (pytv/tv_operators_CPU.py:442-446); the sub-gradient keeps its unit-weight adjoint
                                 * (the weight enters through D only, pytv/tv_GPU.py:104-122).  The plane-marching, one-sweep and
                                 * one-pass fast paths do not take a weight volume (tv_cp_fused_supported /
                                 * tv_subgrad_fused_supported answer 0): the one-site-per-thread kernels do the work */
    const void* time_weight_prev;/* plane z0-1 / z0+nz of the same volume (m*ny*nx elements each) or NULL: only the          */
    const void* time_weight_next;/* ghost-plane norms of tv_subgrad on a slab read them                                       */
    /* PITCHED arrays (round 4; 0 = dense, the reference's layout).  Every image-like array of a call (x, x0, p, G, norms, halo
     * planes, a weight volume) and every gradient-like array (d, q, z, u: one image per channel) shares them:
     *   row_pitch   : elements from one row of a frame to the next  (>= nx; a multiple of 16 bytes)
     *   frame_pitch : elements from one frame to the next           (>= ny * row_pitch; a multiple of 16 bytes)
     * element (z, [c,] t, y, x) lives at ((z [* nd + c]) * m + t) * frame_pitch + y * row_pitch + x.  mask_static / time_factor stay
     * dense (ny * nx).  Why: (i) frames whose rows are not multiples of 128 bytes -- the reference's own shapes, pytv/tests.py:48
     * N = 100, README.md:76-79 rand(20, 4, 100, 100) -- straddle cache lines and write sectors (1000-column frames ran at 0.55 x the
     * rate of 1024-column ones in round 3); (ii) the one-sweep kernels read ~20 streams per block that are congruent modulo the
     * frame size: a frame pitch that is not a power of two spreads them over the HBM channels.
     * The PAD elements (columns >= nx of a row, the tail of a frame) belong to the library's caller but must hold ZEROS on entry
     * wherever an array is read; every pitch-aware entry point leaves them zero (or untouched).  An entry point that does not
     * take pitched arrays refuses them with TV_E_ARG (tv_last_error names it) -- nothing reads a pitched array as a dense one.
     * nx need not be a multiple of the 16-byte lane (4 floats / 2 doubles) when row_pitch is: the vector kernels then own the pad
     * columns of the last lane (this is how 1001-column frames leave the scalar kernels). */
    int64_t row_pitch;
    int64_t frame_pitch;
} tv_geom;

/* zero a tv_geom and stamp it with the header's struct size and interface version */
static inline void tv_geom_init(tv_geom* g) {
    unsigned char* b = (unsigned char*)g;
    for (size_t i = 0; i < sizeof(tv_geom); ++i) b[i] = 0;
    g->struct_size = (uint32_t)sizeof(tv_geom);
    g->abi_version = TV_ABI_VERSION;
}

/* ---- housekeeping ------------------------------------------------------------------------ */
const char* tv_last_error(void);
int         tv_version(void);                         /* 10000*major + 100*minor + patch     */
int         tv_abi_version(void);                     /* TV_ABI_VERSION the library was built with */
/* Tuning / debugging options (TV_ZCHUNK, TV_NO_FUSED, ...: DESIGN.md section 7).  The table is process-wide and explicit:
 * every entry is initialised ONCE from the environment variable of the same name when the library first consults it,
 * and afterwards changes only through these calls -- no entry point reads the environment per call.
 *   tv_set_option   : 0, or TV_E_ARG for an unknown name
 *   tv_unset_option : back to "not set" (every call site then uses its built-in default)
 *   tv_get_option   : the value, or dflt when the option is not set                                            */
int         tv_set_option(const char* name, int value);
int         tv_unset_option(const char* name);
int         tv_get_option(const char* name, int dflt);
/* Number of gradient channels nd for this geometry (pytv/tv_operators_GPU.py:170-174,
 * 290-294,399-403,507-511), or TV_E_ARG. */
int         tv_num_channels(const tv_geom* g);
/* Bytes of device scratch the reducing entry points need in `ws` for this geometry. */
size_t      tv_workspace_bytes(const tv_geom* g);

/* ---- operators: replace pytv.tv_operators_GPU.D_* / D_T_* / compute_L21_norm ---------------- */
/* d = D x.  x_prev / x_next: the plane z0-1 / z0+nz of the image (or NULL).
 * Replaces D_hybrid/D_downwind/D_upwind/D_central (pytv/tv_operators_GPU.py:134-581). */
int tv_D(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, void* d, void* stream);

/* out = D^T y.  y_prev: plane z0-1 of the z channel whose adjoint looks backwards (upwind /
 * central z channel; hybrid: z-up channel); y_next: plane z0+nz of the channel whose adjoint
 * looks forwards (downwind / central z channel; hybrid: z-down channel).
 * Replaces D_T_hybrid/D_T_downwind/D_T_upwind/D_T_central (pytv/tv_operators_GPU.py:583-1052). */
int tv_DT(const tv_geom* g, const void* y, const void* y_prev, const void* y_next, void* out, void* stream);

/* *result (device, fp64) = sum_p sqrt(sum_c d[p,c]^2); norms (nz,m,ny,nx) optional (NULL = skip).
 * Replaces compute_L21_norm (pytv/tv_operators_GPU.py:46-90). */
int tv_l21(const tv_geom* g, const void* d, int32_t nd, void* norms, double* result, void* ws, void* stream);

/* ---- direct TV API: replaces pytv.tv_GPU.tv_* ------------------------------------------------ */
/* *tv (device fp64) = TV of the local planes; G = the reference's sub-gradient
 * (pytv/tv_GPU.py:47-375).  norms_ext: REQUIRED scratch/output of (nz + 2) planes; on return
 * plane k+1 holds 1 / |D x| of local plane k, 0 where |D x| == 0 -- the reciprocal of the
 * reference's grad_norms (which has those zeros replaced by +inf, pytv/tv_GPU.py:88).  "== 0" means here, and in every
 * other sub-gradient entry point: |D x|^2 below the smallest NORMAL number of the dtype (fp32: |D x| < 1.1e-19), where a
 * square carries no information any more; the reference zeroes only at exactly 0.
 * x_prev / x_next: TWO planes each (z0-2, z0-1) / (z0+nz, z0+nz+1) when sharded, else NULL. */
int tv_subgrad(const tv_geom* g, const void* x, const void* x_prev, const void* x_next,
               void* G, void* norms_ext, double* tv, void* ws, void* stream);

/* The same TV value and sub-gradient in ONE pass over x (1/|Dx| never leaves the chip): all four schemes (central:
 * not with a two-point z or time axis), fp32, Nx % 4 == 0, any M (more than 8 frames: overlapping time windows), 16-byte aligned arrays
 * (tv_subgrad_fused_supported).  Use it when the per-voxel norms are not wanted (return_grad_norms=False,
 * pytv/tv_GPU.py:47).  Halos as for tv_subgrad.  A |Dx|^2 below the smallest normal fp32 number counts as 0. */
int tv_subgrad_fused_supported(const tv_geom* g);
int tv_subgrad_fused(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, void* G, double* tv,
                     void* ws, void* stream);
/* The same with the per-voxel norms as a by-product: norms (nz,m,ny,nx) = |D x| with zeros replaced by +inf -- the
 * reference's grad_norms (return_grad_norms=True, pytv/tv_GPU.py:47,88,135-139).  Three words per voxel. */
int tv_subgrad_fused_norms(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, void* G, void* norms,
                           double* tv, void* ws, void* stream);
/* One iteration of the README's sub-gradient loop (README.md:118-124) in the same single pass, G never stored:
 *   x_out = x - step * ((x - x0) + lambda * G(x));  *tv = TV(x);  *fid = 1/2 |x_out - x0|^2   (local planes).
 * x and x_out must be different buffers (ping-pong).  Same geometries as tv_subgrad_fused. */
int tv_subgrad_step_fused(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, const void* x0,
                          void* x_out, double step, double lambda, double* tv, double* fid, void* ws, void* stream);

/* ---- fused Chambolle-Pock inner loop (README.md:141-157) ----------------------------------- */
/* q <- proj_{|.|_2 <= lambda}(q + sigma_D * D x); *tv (device fp64) = |D x|_{2,1} of local planes. */
int tv_cp_dual(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, void* q,
               double sigma_D, double lambda, double* tv, void* ws, void* stream);
/* p <- (p + sigma_A (x - x0)) / (1 + sigma_A);  x <- x - tau p - tau D^T q;
 * *fid (device fp64) = 1/2 |x_new - x0|^2 of local planes.  q_prev/q_next as y_prev/y_next in tv_DT. */
int tv_cp_primal(const tv_geom* g, const void* q, const void* q_prev, const void* q_next, void* x,
                 const void* x0, void* p, double tau, double sigma_A, double* fid, void* ws, void* stream);

/* Primal step of the ACCELERATED Chambolle-Pock iteration (Chambolle & Pock 2011, Algorithm 2; the fidelity 1/2 |x - x0|^2 is 1-strongly
 * convex, so its prox is closed-form and no fidelity dual p exists), with the extrapolation folded into the same pass:
 *   x_new = (x - tau D^T q + tau x0) / (1 + tau);  x_bar = x_new + theta (x_new - x);  x = x_new;
 *   *fid (device fp64) = 1/2 |x_new - x0|^2 of the local planes.  q_prev / q_next as y_prev / y_next in tv_DT.
 * The dual step of the iteration is tv_cp_dual called on x_bar with that iteration's sigma; tau, sigma and theta of iteration k are host
 * doubles (pytv.solvers.accel_schedule).  1 / (1 + tau) is formed once in double.  Every geometry tv_cp_primal takes (four schemes, fp32 /
 * fp64, 16-byte lanes or scalar rows, pitched arrays -- pads stay zero --, mask_static / time_factor / time_weight_vol, z-slabs); fp32
 * planes of >= 4 MiB take the plane-marching kernel: Nd + 4 words per voxel.
 * x and x_bar must be different arrays, tau finite and > 0, theta finite and in [0, 1], else TV_E_ARG; a missing halo plane is TV_E_HALO;
 * all checks precede any device access. */
int tv_cp_primal_accel(const tv_geom* g, const void* q, const void* q_prev, const void* q_next, void* x, void* x_bar,
                       const void* x0, double tau, double theta, double* fid, void* ws, void* stream);

/* Primal step of Chambolle-Pock (Chambolle & Pock 2011, Algorithm 1; section 6.2.2 for TV-L1) for a fidelity F(x - x0) whose prox is
 * POINTWISE, with the extrapolation folded into the same pass.  F by `fidelity`: */
#define TV_FID_L2    0   /* 1/2 |x - x0|^2                                   */
#define TV_FID_L1    1   /* |x - x0|_1                                       */
#define TV_FID_HUBER 2   /* sum h_delta(x - x0): e^2/(2 delta) for |e| <= delta, |e| - delta/2 beyond */
#define TV_CPP_RESIDUAL 1 /* flag: reduce-only */
/* STEP mode (flags == 0), one pass of Nd + 4 words per voxel like tv_cp_primal_accel:
 *   e = (x - tau D^T q) - x0;  x_new = x0 + prox_{tau F}(e);  x_bar = x_new + theta (x_new - x);  x = x_new;
 *   *out (device fp64) = F(x_new - x0) over the local planes, accumulated in fp64.
 * prox_{tau F}(e) is  e / (1 + tau)  (L2),  the soft threshold sign(e) max(|e| - tau, 0)  (L1),  e delta / (delta + tau) where
 * |e| <= delta + tau and e - tau sign(e) beyond  (Huber).  All three are evaluated as  e - clamp(c e, -t, t)  with c = tau / (1 + tau),
 * t = +inf (L2); c = 1, t = tau (L1); c = tau / (delta + tau), t = tau (Huber) -- constants formed once in double, no branch.  An L1 site
 * inside the dead zone |e| <= tau therefore returns x0 BIT FOR BIT (x0 + (e - e)).  `delta` is read for Huber only.
 * RESIDUAL mode (flags == TV_CPP_RESIDUAL): REDUCE-ONLY, nothing is written except out and ws; x_bar may be NULL and theta is ignored.
 *   *out = sum_sites ((x - x_new) / tau)^2, accumulated site by site in fp64 -- the fixed-point residual of the fidelity block: zero iff
 *   -D^T q is in the subdifferential of F at x - x0.  Together with tv_cp_dual_residual (zero iff q is in the subdifferential of
 *   lambda |.|_2 at D x) it is an optimality certificate of the pair (x, q).  (A duality gap does not exist for L1 / Huber without a
 *   feasibility projection of D^T q.)
 * q_prev / q_next as y_prev / y_next in tv_DT; slab partials add up to the unsharded scalars.  Every geometry tv_cp_primal_accel takes, with
 * its dispatch (four schemes, fp32 / fp64, 16-byte lanes or scalar rows, pitched arrays -- pads stay zero --, mask_static / time_factor /
 * time_weight_vol, z-slabs; fp32 planes of >= 4 MiB take the plane-marching kernel, both modes).
 * TV_E_ARG: an unknown fidelity or flag bit, a NULL array (x_bar in step mode), x == x_bar, tau not finite and > 0, delta not finite and
 * > 0 (Huber), theta not finite or outside [0, 1] (step mode); a missing halo plane is TV_E_HALO; all checks precede any device access. */
int tv_cp_primal_prox(const tv_geom* g, const void* q, const void* q_prev, const void* q_next, void* x, void* x_bar, const void* x0,
                      int32_t fidelity, double delta, double tau, double theta, int32_t flags, double* out, void* ws, void* stream);

/* Primal step of Chambolle-Pock (Chambolle & Pock 2011, Algorithm 1) for the POISSON data term: the generalised Kullback-Leibler divergence
 *   F(x) = sum_sites ( x - x0 + x0 log(x0 / x) )  over x >= 0, for counts x0 >= 0  (0 log 0 = 0; +inf where x = 0 < x0),
 * with the extrapolation folded into the same pass.  flags: 0 or TV_CPP_RESIDUAL.
 * STEP mode (flags == 0), one pass of Nd + 4 words per voxel like tv_cp_primal_prox:
 *   v = x - tau D^T q;  b = v - tau;  s = sqrt(b^2 + 4 tau x0);
 *   x_new = prox_{tau F}(v) = (b + s) / 2, evaluated as  b >= 0 ? (b + s) / 2 : 2 tau x0 / (s - b)  -- the same root without the
 *   cancellation of b + s for b << 0;  x_bar = x_new + theta (x_new - x);  x = x_new;
 *   *out (device fp64) = F(x_new) over the local planes, accumulated in fp64.
 * A site with x0 == 0 returns exactly 0 for b < 0 and b otherwise; x_new >= 0 everywhere.  x0 >= 0 is the caller's contract: the kernel does
 * not clamp it (a negative x0 can give NaN).
 * RESIDUAL mode (flags == TV_CPP_RESIDUAL): REDUCE-ONLY, nothing is written except out and ws; x_bar may be NULL and theta is ignored.
 *   *out = sum_sites ((x - x_new) / tau)^2 in fp64 -- zero iff -D^T q is in the subdifferential of F at x; with tv_cp_dual_residual an
 *   optimality certificate of the pair (x, q).
 *   Where x + tau (1 + D^T q) >= 0 the displacement is evaluated as 2 (x0 - x (1 + D^T q)) / (s + x + tau (1 + D^T q)), the same number in
 *   exact arithmetic: an exact 0 at x = x0, D^T q = 0 (a constant image), and equal to (x - x_new) / tau to rounding elsewhere.
 * q_prev / q_next, geometries and dispatch as tv_cp_primal_prox (four schemes, fp32 / fp64, 16-byte lanes or scalar rows, pitched arrays --
 * pads stay zero --, mask_static / time_factor / time_weight_vol, z-slabs; fp32 planes of >= 4 MiB take the plane-marching kernel, both
 * modes); slab partials add up to the unsharded scalars.
 * TV_E_ARG: an unknown flag bit, a NULL array (x_bar in step mode), x == x_bar, tau not finite and > 0, theta not finite or outside [0, 1]
 * (step mode); a missing halo plane is TV_E_HALO; all checks precede any device access. */
int tv_cp_primal_kl(const tv_geom* g, const void* q, const void* q_prev, const void* q_next, void* x, void* x_bar,
                    const void* x0, double tau, double theta, int32_t flags, double* out, void* ws, void* stream);

/* Primal step of Chambolle-Pock (Chambolle & Pock 2011, Algorithm 1) for a WEIGHTED quadratic data term with a BOX constraint,
 *   F(x) = 1/2 sum_sites w (x - x0)^2  over lo <= x <= hi,  w >= 0 per voxel (an array like x0),
 * with the extrapolation folded into the same pass.  w = 0 marks a voxel as unknown -- a dead detector module, a masked frame, a metal
 * trace: TV fills it in (the inpainting model of section 6.3 of the paper); w = 1 / sigma^2 is heteroscedastic least squares.
 * flags: 0 or TV_CPP_RESIDUAL.
 * STEP mode (flags == 0), one pass of Nd + 5 words per voxel (tv_cp_primal_prox's Nd + 4 and w):
 *   v = x - tau D^T q;  c = tau w / (1 + tau w);  x_new = clamp(v - c (v - x0), lo, hi)  -- the prox of a separable term is the clamp of
 *   the quadratic's prox;  x_bar = x_new + theta (x_new - x);  x = x_new;
 *   *out (device fp64) = 1/2 sum w (x_new - x0)^2 over the local planes, accumulated in fp64.
 * Exact by construction: a site with w == 0 returns clamp(v) BIT FOR BIT, a site with v == x0 returns x0 bit for bit (a constant image
 * inside the box with q = 0 does not move), every x_new lies in [lo, hi].  lo / hi may be -inf / +inf (no bound on that side).
 * THE BOX MUST CONTAIN 0 (lo <= 0 <= hi, else TV_E_ARG): the pad elements of pitched arrays are computed like voxels -- x, x0, w and
 * D^T q are 0 there, so they come out as clamp(0) -- and they have to stay 0.  TV and the data term do not change when x, x0 and the box
 * are shifted by one constant, so a caller with another box shifts the problem (pytv.solvers.WeightedChambollePock does).
 * The caller's contract: w finite and >= 0 and tau w finite; the kernel does not check it (a negative or infinite w can give NaN).
 * RESIDUAL mode (flags == TV_CPP_RESIDUAL): REDUCE-ONLY, nothing is written except out and ws; x_bar may be NULL and theta is ignored.
 *   *out = sum_sites ((x - x_new) / tau)^2 in fp64 -- zero iff -D^T q is in the subdifferential of F at x; with tv_cp_dual_residual an
 *   optimality certificate of the pair (x, q).  Nd + 3 words per voxel.
 * q_prev / q_next, geometries and dispatch as tv_cp_primal_kl (four schemes, fp32 / fp64, 16-byte lanes -- w aligned like the others -- or
 * scalar rows, pitched arrays, mask_static / time_factor / time_weight_vol, z-slabs; fp32 planes of >= 4 MiB take the plane-marching
 * kernel, both modes); slab partials add up to the unsharded scalars.
 * TV_E_ARG: an unknown flag bit, a NULL array (x_bar in step mode), x == x_bar, lo or hi NaN, a box that does not contain 0, tau not finite
 * and > 0, theta not finite or outside [0, 1] (step mode); a missing halo plane is TV_E_HALO; all checks precede any device access. */
int tv_cp_primal_wls(const tv_geom* g, const void* q, const void* q_prev, const void* q_next, void* x, void* x_bar,
                     const void* x0, const void* w, double lo, double hi, double tau, double theta, int32_t flags,
                     double* out, void* ws, void* stream);

/* Duality-gap certificate of the model every solver here minimises, P(x) = 1/2 |x - x0|^2 + lambda |D x|_{2,1}, for an iterate x and a dual
 * variable qs = qscale * q with |qs|_2 <= lambda per site (Chambolle-Pock: its q, qscale = 1; scaled-form ADMM: q = u, qscale = rho; both are
 * projections).  Over the local planes, with gd = D^T qs:
 *   out[0] = |D x|_{2,1}
 *   out[1] = 1/2 |x - x0|^2
 *   out[2] = sum_sites [ 1/2 (x - x0 + gd)^2 + lambda |D x|_2 - <qs, D x> ]  =  P(x) - Dual(qs),  Dual(qs) = <gd, x0> - 1/2 |gd|^2
 * out[2] is accumulated site by site in that cancellation-free form (both parts are >= 0 at every site of a feasible qs), never as P - Dual;
 * it is not clamped: in fp32 a converged pair can come out slightly negative (absolute error of order eps * P).  The caller has
 * P = out[1] + lambda * out[0], Dual = P - out[2], and by strong convexity 1/2 |x - x*|^2 <= out[2].
 * REDUCE-ONLY: nothing is written except out (three device fp64 words) and ws.  x_prev / x_next as in tv_cp_dual, q_prev / q_next as in
 * tv_DT (unscaled, like q); slab partials add up to the unsharded scalars.  lambda > 0 and a finite qscale != 0, else TV_E_ARG.
 * Every geometry of tv_cp_dual / tv_cp_primal (four schemes, fp32 / fp64, pitched arrays, weight maps / volumes): one launch, Nd + 2 words per
 * voxel; fp32 planes of >= 4 MiB (the plane-marching kernels' domain): a D^T-side and a D-side pass, 2 Nd + 5 words. */
int tv_dual_gap(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, const void* q, const void* q_prev,
                const void* q_next, const void* x0, double lambda, double qscale, double* out, void* ws, void* stream);

/* Optimality residual of the TV block of the saddle problem Chambolle-Pock iterates on, for solvers whose fidelity term has no cheap dual
 * objective (a general operator A: pytv.solvers.ChambollePockOperator).  (x, q) is stationary for that block iff q = proj(q + s D x) for one
 * (equivalently every) s > 0; over the local planes
 *   out[0] = |D x|_{2,1}
 *   out[1] = sum_sites |q - proj_{|.|_2 <= lambda}(q + sigma_D D x)|_2^2 / sigma_D^2
 * out[1] is accumulated site by site in that form, in fp64, never as a difference of two sums.  The update and the projection are the very
 * arithmetic of tv_cp_dual (one shared device function, IEEE sqrt / divide): q - proj(..) is bit for bit what the next tv_cp_dual with the
 * same sigma_D would change, and out[1] == 0 exactly where it would change nothing.
 * REDUCE-ONLY: nothing is written except out (two device fp64 words) and ws.  x_prev / x_next as in tv_cp_dual; slab partials add up to the
 * unsharded scalars.  lambda > 0 and a finite sigma_D > 0, else TV_E_ARG; a missing halo plane is TV_E_HALO; all checks precede any device
 * access.  Every geometry tv_cp_dual takes (four schemes, fp32 / fp64, 16-byte lanes or scalar rows, pitched arrays, weight maps / volumes,
 * z-slabs): one launch of the one-site-per-thread kernel, Nd + 1 words per voxel.  Large planes stay on that kernel as well -- the call
 * is made once per convergence check, not once per iteration. */
int tv_cp_dual_residual(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, const void* q, double sigma_D,
                        double lambda, double* out, void* ws, void* stream);

/* Dual step of Chambolle-Pock for the HUBER-TV regulariser (Chambolle & Pock 2011, section 6.2.1: the Huber-ROF model against staircasing)
 *   P(x) = 1/2 |x - x0|^2 + lambda sum_sites h_alpha(|D x|_2),   h_alpha(t) = t^2 / (2 alpha) for t <= alpha, t - alpha / 2 beyond:
 * quadratic below a gradient magnitude alpha, TV above it.  The conjugate of the regulariser gains (alpha / 2 lambda) |q|^2, so
 *   v = (q + sigma_D D x) / (1 + sigma_D alpha / lambda);   q <- v / max(1, |v|_2 / lambda)      (shrink, then project)
 *   *hub (device fp64) = sum_sites h_alpha(|D x|_2) of the local planes, each site as (n - a) + a^2 / (2 alpha), a = min(n, alpha), in fp64.
 * 1 / (1 + sigma_D alpha / lambda) is formed once in double.  The primal half of the iteration is tv_cp_primal_accel with constant tau and
 * theta (Algorithm 3 of the paper: both halves of the saddle problem are strongly convex; pytv.solvers.cp_linear_steps).
 * 2 Nd + 1 words per voxel; q is written in place, nothing else but hub and ws.  x_prev / x_next, alignment and dispatch as tv_cp_dual: four
 * schemes, fp32 / fp64, 16-byte lanes or scalar rows, pitched arrays -- pads stay zero --, mask_static / time_factor / time_weight_vol,
 * z-slabs; fp32 planes of >= 4 MiB take the plane-marching kernel (not central / hybrid with 16 frames: those instantiations would spill to
 * scratch and do not exist; the one-site kernel runs there).
 * TV_E_ARG: a NULL array, lambda, alpha or sigma_D not finite and > 0 (alpha = 0 is tv_cp_dual's model and is refused), a tv_geom of
 * another interface version; a missing halo plane is TV_E_HALO as in tv_cp_dual; all checks precede any device access. */
int tv_cp_dual_huber(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, void* q,
                     double sigma_D, double lambda, double alpha, double* hubout, void* ws, void* stream);

/* Duality-gap certificate of the Huber-TV model above for an iterate x and a dual variable q with |q|_2 <= lambda per site (what
 * tv_cp_dual_huber leaves).  Dual(q) = <gd, x0> - 1/2 |gd|^2 - (alpha / 2 lambda) |q|^2 with gd = D^T q.  Over the local planes
 *   out[0] = sum_sites h_alpha(|D x|_2)
 *   out[1] = 1/2 |x - x0|^2
 *   out[2] = sum_sites [ 1/2 (x - x0 + gd)^2 + lambda h_alpha(|D x|_2) - <q, D x> + (alpha / 2 lambda) |q|^2 ]  =  P(x) - Dual(q)
 * Both parts of a site's term are >= 0 (Fenchel-Young).  Where |D x|_2 <= alpha the second part is summed as the perfect square
 * (lambda / 2 alpha) |D x - (alpha / lambda) q|^2, exactly >= 0; beyond alpha as lambda (|D x|_2 - alpha / 2) - <q, D x> + (alpha / 2 lambda) |q|^2.
 * Accumulated in fp64 from the stencil results of the array dtype, never as P - Dual, not clamped.  The caller has
 * P = out[1] + lambda * out[0], Dual = P - out[2], and 1/2 |x - x*|^2 <= out[2].
 * REDUCE-ONLY: nothing is written except out (three device fp64 words) and ws.  x_prev / x_next as in tv_cp_dual, q_prev / q_next as in
 * tv_DT; slab partials add up to the unsharded scalars.  Every geometry of tv_dual_gap: one launch of the one-site-per-thread kernel,
 * Nd + 2 words per voxel, large planes too (the call is made once per convergence check; there is no plane-marching form).
 * TV_E_ARG: a NULL array, lambda or alpha not finite and > 0, a tv_geom of another interface version; a missing halo plane is
 * TV_E_HALO; all checks precede any device access. */
int tv_dual_gap_huber(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, const void* q, const void* q_prev,
                      const void* q_next, const void* x0, double lambda, double alpha, double* out, void* ws, void* stream);

/* Dual step of Chambolle-Pock for the SPATIALLY ADAPTIVE regulariser: a per-voxel weight g_i >= 0 on the TV term,
 *   P(x) = 1/2 |x - x0|^2 + lambda sum_i g_i |D x|_{2,i}
 * (noise-adaptive lambda, edge-stopping weights g = 1 / (1 + (|D x0| / kappa)^2), protected regions g = 0).  The conjugate differs from
 * plain TV's only in the radius of the ball a site's dual vector is projected onto: r_i = lambda g_i instead of lambda.  At each site
 *   v = q + sigma_D D x per channel,  n = |v|_2;   q <- v where n <= r_i,  v * (r_i / n) beyond        (a select, not a multiply by 1)
 *   *wtv (device fp64) = sum_i g_i |D x|_{2,i} of the local planes, accumulated in fp64: the loss is fid + lambda * *wtv.
 * For finite inputs with g >= 0: a site inside its ball keeps q = v bit for bit; a site with g_i = 0 ends with q = +-0 in every channel;
 * the result is never NaN or Inf (n = 0 with r = 0 included: r / n is used only where n > r); |q|_2 <= r_i up to rounding afterwards.
 * gw is an image-like array of the geometry's dtype stored exactly like x0: the local planes of the slab, pitched with the others (pads
 * zero), NO halo plane (the projection is local), part of the 16-byte alignment test.  g FINITE AND >= 0 IS THE CALLER'S CONTRACT: the
 * kernel does not check it (pytv.solvers.AdaptiveTVChambollePock does, once, at construction).
 * 2 Nd + 2 words per voxel; q is written in place, nothing else but wtv and ws.  x_prev / x_next, alignment and dispatch as tv_cp_dual:
 * four schemes, fp32 / fp64, 16-byte lanes or scalar rows, pitched arrays, mask_static / time_factor / time_weight_vol, z-slabs; fp32
 * planes of >= 4 MiB take the plane-marching kernel (NOT downwind / central / hybrid WITH 16 FRAMES: those instantiations would spill to
 * scratch and do not exist; the one-site kernel runs there).  The primal half of the iteration is tv_cp_primal_accel.
 * TV_E_ARG: a NULL array ("<name> is NULL", gw included), lambda or sigma_D not finite and > 0, a tv_geom of another interface version;
 * a missing halo plane is TV_E_HALO ("x_prev: ..." / "x_next: ..."); all checks precede any device access. */
int tv_cp_dual_wtv(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, void* q, const void* gw,
                   double sigma_D, double lambda, double* wtv, void* ws, void* stream);

/* Duality-gap certificate of the spatially adaptive model above for an iterate x and a dual variable q with |q|_2 <= lambda g_i per site
 * (what tv_cp_dual_wtv leaves).  Dual(q) = <gd, x0> - 1/2 |gd|^2 with gd = D^T q.  Over the local planes
 *   out[0] = sum_i g_i |D x|_{2,i}
 *   out[1] = 1/2 |x - x0|^2
 *   out[2] = sum_sites [ 1/2 (x - x0 + gd)^2  +  (lambda g_i |D x|_2 - <q, D x>) ]  =  P(x) - Dual(q)
 * Both parts of a site's term are >= 0 for a feasible q.  Accumulated site by site in that form in fp64, never as P - Dual, not clamped.
 * The caller has P = out[1] + lambda * out[0], Dual = P - out[2], and 1/2 |x - x*|^2 <= out[2].
 * REDUCE-ONLY: nothing is written except out (three device fp64 words) and ws.  x_prev / x_next as in tv_cp_dual, q_prev / q_next as in
 * tv_dual_gap; gw as in tv_cp_dual_wtv (no halo plane; finite and >= 0 is the caller's contract, not checked); slab partials add up to
 * the unsharded scalars.  Every geometry of tv_dual_gap: one launch of the one-site-per-thread kernel, Nd + 3 words per voxel, large
 * planes too (the call is made once per convergence check; there is no plane-marching form).
 * TV_E_ARG: a NULL array ("<name> is NULL", gw included), lambda not finite and > 0, a tv_geom of another interface version; a missing
 * halo plane is TV_E_HALO ("x_prev: ..." / "x_next: ..." / "q_prev: ..." / "q_next: ..."); all checks precede any device access. */
int tv_dual_gap_wtv(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, const void* q, const void* q_prev,
                    const void* q_next, const void* x0, const void* gw, double lambda, double* out, void* ws, void* stream);

/* Dual step of Chambolle-Pock for the ADAPTIVE HUBER-TV regulariser: the per-voxel weight g_i >= 0 of tv_cp_dual_wtv on the Huber function of
 * tv_cp_dual_huber,
 *   P(x) = 1/2 |x - x0|^2 + lambda sum_i g_i h_alpha(|D x|_{2,i}).
 * With r_i = lambda g_i the conjugate of a site's term is alpha |q_i|^2 / (2 r_i) + indicator(|q_i|_2 <= r_i); for g_i = 0 it is the indicator of
 * q_i = 0.  At each site
 *   shrink_i = r_i / (r_i + sigma_D alpha)               (the constant 0 where r_i = 0; sigma_D alpha > 0, formed once in double: no division by zero)
 *   v = shrink_i (q + sigma_D D x) per channel,  n = |v|_2;   q <- v where n <= r_i,  v * (r_i / n) beyond,  0 where r_i = 0    (tv_cp_dual_wtv's select)
 *   *hwtv (device fp64) = sum_i g_i h_alpha(|D x|_{2,i}) of the local planes, h_alpha as (n - a) + a^2 / (2 alpha), a = min(n, alpha), in fp64.
 * For finite inputs with g >= 0: a site inside its ball keeps q = v bit for bit; a site with g_i = 0 ends with q = +-0 in every channel; the
 * result is never NaN or Inf; |q|_2 <= r_i up to rounding afterwards.  gw as in tv_cp_dual_wtv: stored like x0, NO halo plane, part of the
 * 16-byte alignment test, finite and >= 0 by the caller's contract (pytv.solvers.AdaptiveHuberChambollePock checks it once).
 * 2 Nd + 2 words per voxel; q is written in place, nothing else but hwtv and ws.  x_prev / x_next, alignment and dispatch as tv_cp_dual: four
 * schemes, fp32 / fp64, 16-byte lanes or scalar rows, pitched arrays, mask_static / time_factor / time_weight_vol, z-slabs.  ALWAYS the
 * one-site-per-thread kernel: there is NO plane-marching form of this epilogue, fp32 planes of >= 4 MiB run the one-site kernel too (on
 * unsharded volumes tv_cp_hwtv_sweep serves the large planes).  The primal half of the iteration is tv_cp_primal_accel.
 * TV_E_ARG: a NULL array ("<name> is NULL", gw included), lambda, alpha or sigma_D not finite and > 0 (alpha = 0 is tv_cp_dual_wtv's model and is
 * refused), a tv_geom of another interface version; a missing halo plane is TV_E_HALO ("x_prev: ..." / "x_next: ..."); all checks precede any
 * device access. */
int tv_cp_dual_hwtv(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, void* q, const void* gw,
                    double sigma_D, double lambda, double alpha, double* hwtv, void* ws, void* stream);

/* Duality-gap certificate of the adaptive Huber-TV model above for an iterate x and a dual variable q with |q|_2 <= lambda g_i per site (what
 * tv_cp_dual_hwtv leaves).  Dual(q) = <gd, x0> - 1/2 |gd|^2 - sum_{r_i > 0} alpha |q_i|^2 / (2 r_i) with gd = D^T q, r_i = lambda g_i.  Over the
 * local planes
 *   out[0] = sum_i g_i h_alpha(|D x|_{2,i})
 *   out[1] = 1/2 |x - x0|^2
 *   out[2] = sum_sites [ 1/2 (x - x0 + gd)^2  +  ( r_i h_alpha(|D x|_2) + [r_i > 0] alpha |q|^2 / (2 r_i) - <q, D x> ) ]  =  P(x) - Dual(q)
 * Both parts of a site's term are >= 0 (Fenchel-Young).  Where |D x|_2 <= alpha and r_i > 0 the second part is summed as the perfect square
 * (r_i / 2 alpha) |D x - (alpha / r_i) q|^2.  Accumulated site by site in fp64, never as P - Dual, not clamped.  The caller has
 * P = out[1] + lambda * out[0], Dual = P - out[2], and 1/2 |x - x*|^2 <= out[2].
 * REDUCE-ONLY: nothing is written except out (three device fp64 words) and ws.  Halos, gw and geometries as tv_dual_gap_wtv: one launch of the
 * one-site-per-thread kernel, Nd + 3 words per voxel, large planes too (there is no plane-marching form); slab partials add up to the
 * unsharded scalars.
 * TV_E_ARG: a NULL array ("<name> is NULL", gw included), lambda or alpha not finite and > 0, a tv_geom of another interface version; a
 * missing halo plane is TV_E_HALO ("x_prev: ..." / "x_next: ..." / "q_prev: ..." / "q_next: ..."); all checks precede any device access. */
int tv_dual_gap_hwtv(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, const void* q, const void* q_prev,
                     const void* q_next, const void* x0, const void* gw, double lambda, double alpha, double* out, void* ws, void* stream);

/* Dual step of Chambolle-Pock for the CHANNEL-COUPLED (vectorial / joint / collaborative) TV regulariser: the M frames of the volume are
 * channels of ONE object (dual- and multi-energy CT, multi-contrast or multi-echo series, colour stacks, gated frames with shared anatomy)
 * and one Frobenius norm is taken per SPATIAL site s = (z, y, x) over all Nd gradient channels c and all M frames m,
 *   P(x) = 1/2 |x - x0|^2 + lambda sum_s |D x|_{F,s},    |D x|_{F,s} = ( sum_{m,c} (D x)[z, c, m, y, x]^2 )^(1/2).
 * With reg_time = 0 this is the pure spatial joint TV; with reg_time > 0 the weighted time differences join the same norm; M = 1 is plain
 * TV.  The conjugate is the indicator of one ball of radius lambda per spatial site bounding the M Nd-vector.  At each site
 *   v = q + sigma_D D x for every frame and channel,  n = |v|_{F,s};   q <- v where n <= lambda,  v * (lambda / n) beyond
 * with ONE FACTOR PER SITE, selected (the constant 1, or lambda / n) and applied to every frame and channel of the site.
 *   *vtv (device fp64) = sum_s |D x|_{F,s} of the local planes, accumulated in fp64: the loss is fid + lambda * *vtv.
 * EXACT, for finite inputs: a site inside its ball keeps q = v bit for bit (v times the constant 1; v is formed as tv_cp_dual_wtv forms
 * it); lambda / n is evaluated only where n > lambda > 0, so the result is never NaN or Inf; |q_s|_F <= lambda up to rounding afterwards.
 * A thread owns one spatial site and walks its frames.  Two kernel forms, chosen by (scheme, M):
 *   register form  M <= 8 (hybrid: M <= 4): v of all frames stays in registers, x and q are read once and q is written once: 2 Nd + 1 words per voxel
 *   generic form   any M:  pass 1 accumulates n^2 over the frames, pass 2 recomputes v and stores v * factor: 3 Nd + 2 words per voxel if
 *                  pass 2 is served by HBM alone, less where L2 / MALL hold the site's frames.  v is never written unscaled.
 * (option TV_VTV_FORM = 2: the generic form for every M; the two forms give the same q bit for bit.)  q is written in place, nothing else but vtv and ws.  x_prev / x_next,
 * alignment and geometries as tv_cp_dual: four schemes, fp32 / fp64, 16-byte lanes or scalar rows, pitched arrays, mask_static /
 * time_factor / time_weight_vol, z-slabs (a z-cut never separates the frames of a site).  There is no plane-marching form.  The primal half
 * of the iteration is tv_cp_primal_accel.
 * TV_E_ARG: a NULL array ("<name> is NULL"), lambda or sigma_D not finite and > 0, a tv_geom of another interface version; a missing halo
 * plane is TV_E_HALO ("x_prev: ..." / "x_next: ..."); all checks precede any device access. */
int tv_cp_dual_vtv(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, void* q,
                   double sigma_D, double lambda, double* vtv, void* ws, void* stream);

/* Duality-gap certificate of the channel-coupled model above for an iterate x and a dual variable q with |q_s|_F <= lambda per spatial
 * site (what tv_cp_dual_vtv leaves).  Dual(q) = <gd, x0> - 1/2 |gd|^2 with gd = D^T q.  Over the local planes
 *   out[0] = sum_s |D x|_{F,s}
 *   out[1] = 1/2 |x - x0|^2
 *   out[2] = sum_voxels 1/2 (x - x0 + gd)^2  +  sum_s ( lambda |D x|_{F,s} - sum_{m,c} q D x )  =  P(x) - Dual(q)
 * EXACT for any feasible q.  Both parts are >= 0 site by site (Cauchy-Schwarz over the joint vector); they are accumulated in that form in
 * fp64 (a site's |D x|^2 and <q, D x> are summed over its frames in fp64 from the stencil's results), never as P - Dual, not clamped.
 * The caller has P = out[1] + lambda * out[0], Dual = P - out[2], and 1/2 |x - x*|^2 <= out[2].
 * REDUCE-ONLY: nothing is written except out (three device fp64 words) and ws.  x_prev / x_next as in tv_cp_dual, q_prev / q_next as in
 * tv_dual_gap; slab partials add up to the unsharded scalars.  One kernel form for every geometry of tv_cp_dual_vtv (a thread owns a spatial
 * site and walks its frames; Nd + 2 words per voxel): the call is made once per convergence check.
 * TV_E_ARG: a NULL array ("<name> is NULL"), lambda not finite and > 0, a tv_geom of another interface version; a missing halo plane is
 * TV_E_HALO ("x_prev: ..." / "x_next: ..." / "q_prev: ..." / "q_next: ..."); all checks precede any device access. */
int tv_dual_gap_vtv(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, const void* q, const void* q_prev,
                    const void* q_next, const void* x0, double lambda, double* out, void* ws, void* stream);

/* One-sweep form of the same iteration (all four schemes; fp32, nx % 4 == 0, nx >= 64,
 * any m: more than 8 frames are processed as time windows of 8): q is read and written ONCE per
 * iteration.  x is ping-ponged.
 *   tv_cp_fused_supported : 1 if this geometry can take the one-sweep path, else 0
 *   tv_cp_fused           : q <- proj(q + sigma_D D x_in); p <- (p + sigma_A (x_in - x0)) / (1 + sigma_A);
 *                           x_out <- x_in - tau p - tau D^T q   EXCEPT the adjoint terms that cross a
 *                           wave tile (8 rows x 32 cols; columns: only the 256-col block tile), a z-chunk, a time window or the slab; *tv = |D x_in|_{2,1},
 *                           *fid = 1/2 |x_out - x0|^2 over the sites that are already complete
 *   tv_cp_fixup           : adds the missing terms to x_out (q_prev / q_next as in tv_DT) and returns
 *                           the fidelity of those sites in *fid; total fidelity = sum of the two.
 * Both can be restricted to a range so that halo exchanges hide behind the interior work: the sweep to
 * z-chunks [chunk_begin, chunk_begin + chunk_count) (tv_cp_zchunk() planes each, chunk_count < 0 = all),
 * the fix-up to local planes [z_begin, z_begin + z_count) (z_count < 0 = all).  Only the first chunk reads
 * x_prev, only the last x_next; only plane 0 reads q_prev, only plane nz-1 q_next.
 * Ranges are exact: whichever way the chunks and planes are split over calls, every array comes out bit-identical to the whole
 * call, and the partial *tv / *fid add up to its scalars (to the last digits of an fp64 sum).  Seams are not: x_out (r of the ADMM
 * form) of a site next to a chunk or slab seam is rounded once by the sweep and once more by the fix-up, a site inside a chunk once
 * only -- slabs reproduce the unsharded x_out bit for bit when their cuts are multiples of the unsharded tv_cp_zchunk(), and to
 * the rounding of the dtype otherwise; q, u and every stored sample of t' never depend on the seams (tests/test_gpu_sweep_ranges.py). */
int tv_cp_fused_supported(const tv_geom* g);
int tv_cp_zchunk(const tv_geom* g);
int tv_cp_fused(const tv_geom* g, const void* x_in, const void* x_prev, const void* x_next, void* q, const void* x0,
                void* p, void* x_out, double sigma_D, double lambda, double tau, double sigma_A, int64_t chunk_begin,
                int64_t chunk_count, double* tv, double* fid, void* ws, void* stream);
int tv_cp_fixup(const tv_geom* g, const void* q, const void* q_prev, const void* q_next, void* x_out, const void* x0,
                double tau, int64_t z_begin, int64_t z_count, double* fid, void* ws, void* stream);
/* tv_cp_fused with flags (round 4).  TV_CP_FID_OF_INPUT: *fid = 1/2 |x_in - x0|^2 over ALL local sites (the sweep has x_in
 * and x0 in registers) instead of 1/2 |x_out - x0|^2 over the sites that are already complete; tv_cp_fixup then needs no x0
 * (pass x0 = NULL: it adds the missing terms only, *fid = 0) and moves one word less per site it visits.  A loop takes the
 * fidelity of iterate k+1 from sweep k+1 (the README's loss line, README.md:157, pairs 1/2 |x_{k+1} - x0|^2 with the TV of x_k)
 * and needs one plain reduction for the last iterate.
 * q_in / q_out: the dual variable is read from q_in and written to q_out.  q_in == q_out is the in-place update of tv_cp_fused;
 * two arrays (ping-pong, the caller swaps them after every iteration) cost a second q but run ~9 % faster: HBM serves "read one
 * array, write another" better than a read-modify-write of the same lines (tools/archive/bwtest4: 5.98 against 5.50 TB/s for this
 * kernel's memory shape).  tv_cp_fixup takes q_out. */
#define TV_CP_FID_OF_INPUT 1
/* TV_CP_FID_BOTH (round 5; only together with TV_CP_FID_OF_INPUT): `fid` points to TWO doubles -- fid[0] as above, fid[1] = 1/2 |x_out - x0|^2 over
 * the sites that are already complete (what the flag-less tv_cp_fused returns); the tv_cp_fixup that follows is then called WITH x0 and
 * returns the rest.  The LAST sweep of a lagged loop uses it: the fidelity of the final iterate needs no separate reduction pass. */
#define TV_CP_FID_BOTH 2
int tv_cp_sweep(const tv_geom* g, const void* x_in, const void* x_prev, const void* x_next, const void* q_in, void* q_out, const void* x0,
                void* p, void* x_out, double sigma_D, double lambda, double tau, double sigma_A, int32_t flags, int64_t chunk_begin,
                int64_t chunk_count, double* tv, double* fid, void* ws, void* stream);
/* One-sweep form of the ACCELERATED iteration (tv_cp_dual on x_bar + tv_cp_primal_accel; same geometries as tv_cp_fused:
 * tv_cp_fused_supported), in the memory shape of tv_cp_sweep -- x_bar is the stencil input and is ping-ponged, the iterate x is the
 * per-site array that is read and written in place, there is no fidelity dual p:
 *   tv_cp_accel_sweep : q_out <- proj(q_in + sigma_D D xbar_in);  x_new = (x - tau D^T q_out + tau x0) / (1 + tau);
 *                       xbar_out <- x_new + theta (x_new - x);  x <- x_new
 *                       EXCEPT the adjoint terms tv_cp_fused leaves out;  *tv = |D xbar_in|_{2,1};  *fid = 1/2 |x_new - x0|^2 over the sites that
 *                       are already complete; TV_CP_FID_OF_INPUT: *fid = 1/2 |x - x0|^2 of the x the call STARTED from, over all local sites;
 *                       TV_CP_FID_BOTH: fid[0] that, fid[1] the flag-less partial (`fid` points to two doubles)
 *   tv_cp_accel_fixup : adds the missing terms m to BOTH arrays (x_new and x_bar are affine in D^T q): x <- x - c m, xbar_out <- xbar_out - (1 + theta) c m
 *                       with c = tau / (1 + tau), both coefficients formed in double; *fid = 1/2 |x - x0|^2 of the sites it visited, or 0 with
 *                       x0 = NULL (a loop that takes the fidelity from the next sweep).  It takes q_out; q_prev / q_next as in tv_DT.
 * q_in == q_out is the in-place update.  tau, theta (and sigma_D) are those of ONE iteration (pytv.solvers.accel_schedule); 1 / (1 + tau) is
 * formed once in double.  2 Nd + 5 words per voxel where the kernel pair moves 3 Nd + 5.  Chunk / plane ranges, halos and flags as in
 * tv_cp_sweep / tv_cp_fixup: q_out, x and xbar_out come out bit-identical however the chunks and planes are split over calls, and slabs
 * cut at multiples of the unsharded tv_cp_zchunk() reproduce the unsharded x and xbar_out bit for bit (other cuts: to the rounding of the
 * dtype; q_out always).  TV_E_ARG, each with its own message, before any device access: a NULL array (x0 may be NULL in the fix-up only),
 * xbar_in == xbar_out, x aliasing xbar_in / xbar_out / x0, lambda not > 0, tau not finite or not > 0, theta not finite or outside [0, 1],
 * unknown flags or TV_CP_FID_BOTH without TV_CP_FID_OF_INPUT, a geometry tv_cp_fused_supported refuses, arrays not 16-byte aligned.  A
 * missing halo plane is TV_E_HALO. */
int tv_cp_accel_sweep(const tv_geom* g, const void* xbar_in, const void* xbar_prev, const void* xbar_next, const void* q_in, void* q_out,
                      const void* x0, void* x, void* xbar_out, double sigma_D, double lambda, double tau, double theta, int32_t flags,
                      int64_t chunk_begin, int64_t chunk_count, double* tv, double* fid, void* ws, void* stream);
int tv_cp_accel_fixup(const tv_geom* g, const void* q, const void* q_prev, const void* q_next, void* x, void* xbar_out, const void* x0,
                      double tau, double theta, int64_t z_begin, int64_t z_count, double* fid, void* ws, void* stream);
/* One-sweep form of the HUBER-TV iteration (tv_cp_dual_huber on x_bar + tv_cp_primal_accel with constant tau and theta; same geometries as
 * tv_cp_fused: tv_cp_fused_supported).  tv_cp_accel_sweep with the Huber dual update -- per channel one more multiply, then the same projection:
 *   tv_cp_huber_sweep : v = (q_in + sigma_D D xbar_in) / (1 + sigma_D alpha / lambda);  q_out <- v / max(1, |v|_2 / lambda);
 *                       x_new, xbar_out, x exactly as tv_cp_accel_sweep, EXCEPT the adjoint terms tv_cp_fused leaves out;
 *                       *hub = sum_sites h_alpha(|D xbar_in|_2) over the local planes, each site as (n - a) + a^2 / (2 alpha), a = min(n, alpha), in
 *                       fp64 (tv_cp_dual_huber's sum);  *fid and the flags TV_CP_FID_OF_INPUT / TV_CP_FID_BOTH as tv_cp_accel_sweep
 * 1 / (1 + sigma_D alpha / lambda) and 1 / (2 alpha) are formed once in double.  2 Nd + 5 words per voxel where the pair tv_cp_dual_huber +
 * tv_cp_primal_accel moves 3 Nd + 5.
 * THE FIX-UP OF THIS SWEEP IS tv_cp_accel_fixup, called with the same tau and theta (and q_out): it only gathers D^T q terms from the stored
 * dual variable, whatever update produced it.  There is no fix-up symbol of its own.
 * Flags, chunk ranges, halos, aliasing rules, the 16-byte alignment test and the bit-for-bit statements about ranges and slabs are those of
 * tv_cp_accel_sweep.  TV_E_ARG, each with its own message, before any device access: every case tv_cp_accel_sweep refuses, and alpha not finite
 * or not > 0 (alpha = 0 is plain TV: tv_cp_accel_sweep).  A missing halo plane is TV_E_HALO. */
int tv_cp_huber_sweep(const tv_geom* g, const void* xbar_in, const void* xbar_prev, const void* xbar_next, const void* q_in, void* q_out,
                      const void* x0, void* x, void* xbar_out, double sigma_D, double lambda, double alpha, double tau, double theta,
                      int32_t flags, int64_t chunk_begin, int64_t chunk_count, double* hub, double* fid, void* ws, void* stream);
/* One-sweep form of the ADAPTIVE HUBER-TV iteration (tv_cp_dual_hwtv on x_bar + tv_cp_primal_accel with constant tau and theta; same
 * geometries as tv_cp_fused: tv_cp_fused_supported).  tv_cp_huber_sweep with the per-site shrink factor and radius of tv_cp_dual_hwtv:
 *   tv_cp_hwtv_sweep : q_out <- the dual update of tv_cp_dual_hwtv on (q_in, xbar_in, gw);  x_new, xbar_out, x exactly as tv_cp_accel_sweep,
 *                      EXCEPT the adjoint terms tv_cp_fused leaves out;  *hwtv = sum_i g_i h_alpha(|D xbar_in|_{2,i}) over the local planes in
 *                      fp64;  *fid and the flags TV_CP_FID_OF_INPUT / TV_CP_FID_BOTH as tv_cp_accel_sweep
 * gw of a site is one more streamed 16-byte load per frame: stored like x0, the local planes only, NO halo plane (the projection is local),
 * part of the 16-byte alignment test.  2 Nd + 6 words per voxel where the pair tv_cp_dual_hwtv + tv_cp_primal_accel moves 3 Nd + 6.
 * THE FIX-UP OF THIS SWEEP IS tv_cp_accel_fixup, called with the same tau and theta (and q_out).  There is no fix-up symbol of its own.
 * Flags, chunk ranges, halos, aliasing rules and the bit-for-bit statements about ranges and slabs are those of tv_cp_accel_sweep.  TV_E_ARG,
 * each with its own message, before any device access: every case tv_cp_accel_sweep refuses, "gw is NULL", and lambda, alpha or sigma_D not
 * finite and > 0.  A missing halo plane is TV_E_HALO. */
int tv_cp_hwtv_sweep(const tv_geom* g, const void* xbar_in, const void* xbar_prev, const void* xbar_next, const void* q_in, void* q_out,
                     const void* x0, void* x, void* xbar_out, const void* gw, double sigma_D, double lambda, double alpha, double tau,
                     double theta, int32_t flags, int64_t chunk_begin, int64_t chunk_count, double* hwtv, double* fid, void* ws, void* stream);

/* ---- fused ADMM updates (not in the reference; README.md:26,135 mention only) --------------- */
/* v = D x + u; z = v * max(0, 1 - thresh/|v|_2); u = v - z; *tv (device fp64) = |D x|_{2,1}. */
int tv_admm_zu(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, void* z, void* u,
               double thresh, double* tv, void* ws, void* stream);
/* One-sweep form of the outer iteration's dual side (round 3; same geometries as tv_cp_fused: tv_cp_fused_supported):
 * the z / u update AND the residual the next x-solve starts from, from one pass over u --
 *   v = D x + u;  z = v * max(0, 1 - thresh/|v|_2);  u <- v - z (in place);  t' = (z - u) - D x;
 *   r <- (x0 - x) + rho D^T t'  =  [x0 + rho D^T (z - u)] - (I + rho D^T D) x
 *   *tv = |D x|_{2,1};  *rr = <r, r> over the sites that are already complete (device fp64, local planes)
 * EXCEPT, exactly as in tv_cp_fused, the adjoint terms that cross a wave tile, a z-chunk, a time window or the slab:
 * tv_admm_fixup adds those to r (t_prev / t_next: halo planes of t' as y_prev / y_next in tv_DT) and returns <r, r> of
 * the sites it completed; total = sum of the two.  t (same shape as u) receives t': every sample if bit 0 of full_store is set
 * (then z = t' + u + D x), otherwise only the samples the fix-up and the neighbouring ranks read (the rest of the array is
 * left untouched).  Bit 1 of full_store: *rr = |x - x0|^2 over ALL local sites instead (a solver that needs no <r, r> -- the Chebyshev
 * x-solve -- gets the fidelity of the iterate for free; tv_admm_fixup's *rr is then meaningless).
 * 2 Nd + 3 words per voxel where tv_admm_tu + tv_DT_axpy + tv_normal_op2(b) move 4 Nd + 6.
 * Chunk / plane ranges as in tv_cp_fused / tv_cp_fixup.  Replaces: nothing in the reference (README.md:26,135 name ADMM only). */
int tv_admm_fused(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, void* u, void* t, const void* x0, void* r,
                  double thresh, double rho, int32_t full_store, int64_t chunk_begin, int64_t chunk_count, double* tv, double* rr,
                  void* ws, void* stream);
/* tv_admm_fused with separate arrays for the dual variable (round 5): u_in is read, u_out written (equal: tv_admm_fused).  A caller that
 * keeps both and swaps them after every outer iteration can rebuild the split variable z = shrink(D x + u_in, thresh) whenever it is
 * asked for (tv_admm_zu on a copy of u_in), so the sweep need not store every sample of t' (full_store bit 0 clear): Nd words per voxel
 * and outer iteration less than the z-preserving form of tv_admm_fused.  Replaces: nothing in the reference (README.md:26,135). */
int tv_admm_sweep(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, const void* u_in, void* u_out, void* t,
                  const void* x0, void* r, double thresh, double rho, int32_t full_store, int64_t chunk_begin, int64_t chunk_count,
                  double* tv, double* rr, void* ws, void* stream);
int tv_admm_fixup(const tv_geom* g, const void* t, const void* t_prev, const void* t_next, void* r, double rho, int64_t z_begin,
                  int64_t z_count, double* rr, void* ws, void* stream);
/* One-sweep form of Chambolle-Pock with a data-fidelity operator A (README.md:2,148 with A != I; same geometries as tv_cp_fused):
 *   tv_cpop_fused : q <- proj(q + sigma_D D x_in);  x_out <- x_in - tau atp - tau D^T q   (atp = A^T p, an image, read only)
 *                   EXCEPT the adjoint terms tv_cp_fused leaves out;  *tv = |D x_in|_{2,1}
 *   tv_cpop_fixup : adds those terms to x_out (q_prev / q_next as in tv_DT)
 * 2 Nd + 4 words per voxel where tv_cp_dual + tv_DT_axpy2 move 3 Nd + 4.  Chunk / plane ranges as in tv_cp_fused / tv_cp_fixup. */
int tv_cpop_fused(const tv_geom* g, const void* x_in, const void* x_prev, const void* x_next, void* q, const void* atp, void* x_out,
                  double sigma_D, double lambda, double tau, int64_t chunk_begin, int64_t chunk_count, double* tv, void* ws, void* stream);
int tv_cpop_fixup(const tv_geom* g, const void* q, const void* q_prev, const void* q_next, void* x_out, double tau, int64_t z_begin,
                  int64_t z_count, void* ws, void* stream);
/* out = base + alpha * D^T (a - b)   (b and/or base may be NULL).  ab_prev / ab_next: halo planes
 * of (a - b) for the channels named in tv_DT. */
int tv_DT_axpy2(const tv_geom* g, const void* a, const void* b, const void* ab_prev, const void* ab_next,
                const void* base, const void* base2, double beta, double alpha, void* out, void* stream);
/* ^ out = base + beta * base2 + alpha * D^T (a - b): the primal step of Chambolle-Pock with a data-fidelity operator A
 *   (the CT use case, README.md:2,148), x - tau A^T p - tau D^T q in ONE pass: base = x, base2 = A^T p, beta = alpha = -tau.
 * The two data-space updates of that iteration (vectors of ANY length n, the user's A decides):
 *   tv_cpop_p        : p <- (p + sigma_A r) / (1 + sigma_A),  r = A x - b carried over from the previous iteration
 *   tv_cpop_residual : r <- ax - b;  *fid (device fp64) = 1/2 |r|^2;  ws: >= 2048 doubles of device scratch */
int tv_cpop_p(int32_t dtype, int64_t n, void* p, const void* r, double sigma_A, void* stream);
int tv_cpop_residual(int32_t dtype, int64_t n, const void* ax, const void* b, void* r, double* fid, void* ws, void* stream);
int tv_DT_axpy(const tv_geom* g, const void* a, const void* b, const void* ab_prev, const void* ab_next,
               const void* base, double alpha, void* out, void* stream);
/* out = x + rho * D^T D x, computed from x alone (radius-2 stencil); *dot (device fp64) = <x, out>
 * over local planes.  x_prev / x_next: TWO planes each as in tv_subgrad. */
int tv_normal_op(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, double rho,
                 void* out, double* dot, void* ws, void* stream);
/* The same operator with two dot products and an optional right-hand side, for conjugate gradients:
 *   b == NULL : out = A x,      dots[0] = <x, A x>,   dots[1] = <x, x>
 *   b != NULL : out = b - A x,  dots[0] = <out, out>, dots[1] = <x, x>;  out2 (or NULL) receives a second copy of out
 * A = I + rho D^T D; dots: two device fp64 words (local planes). */
int tv_normal_op2(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, double rho, const void* b, void* out,
                  void* out2, double* dots, void* ws, void* stream);
/* One step of the Chebyshev iteration on (I + rho D^T D) e = b (round 3: an x-solve whose scalars do not depend on the vectors --
 * no dot product, hence no all-reduce on a sharded volume, and 4 words per voxel and step where a CG step moves 11):
 *   out = [add +] x + alpha (b - A x) + beta (x - y)          y NULL: y = yscale * b (0: no y); add, ref may be NULL
 *   (x may be b itself: with e_1 = a_0 b never stored, the first two steps are  e_2 = b + a' (b - A b) + b' b  and a step with
 *   y = a_0 b -- 2 + 3 words instead of 2 + 3 + 4)
 *   dots[0] = |b - A x|^2,  dots[1] = |out - ref|^2 if ref is given, else |x|^2      (device fp64, local planes)
 *   dots may be NULL (round 5): no dot products -- the streaming kernel drops their fp64 arithmetic and the two reduction launches
 *   (the ADMM x-solve needs none of them unless it is asked for the fidelity of its last step); ref needs dots.
 * out must not alias an input.  x_prev / x_next: TWO halo planes each, as in tv_normal_op.  The coefficients of step k follow from
 * the spectral interval [1, 1 + rho L] alone (pytv/solvers.py::chebyshev_coefficients restates the recurrence).
 * tv_axpby: out = a x + b y (y NULL: a x); *dist2 (or NULL, then ref and ws may be NULL too) = |out - ref|^2; out NULL (with ref):
 * the distance alone, nothing is stored (round 4: the fidelity of the last iterate of a lagged Chambolle-Pock block).
 * Replaces: nothing in the reference (its README names ADMM only, README.md:26,135). */
int tv_cheb_step(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, double rho, const void* b, const void* y,
                 double yscale, const void* add, const void* ref, double alpha, double beta, void* out, double* dots, void* ws, void* stream);
int tv_axpby(const tv_geom* g, double a, const void* x, double b, const void* y, const void* ref, void* out, double* dist2, void* ws,
             void* stream);
/* One step of the SINGLE-REDUCTION conjugate gradient (Chronopoulos-Gear form; one all-reduce of two scalars per step on
 * a sharded volume instead of two all-reduces).  sc: four device fp64 words
 *     sc[0] = gamma = <r, r>,  sc[1] = delta = <r, w> with w = A r   (already summed over the ranks)
 *     sc[2] = gamma of the previous step,  sc[3] = alpha of the previous step; sc[3] == 0 marks the FIRST step of a solve
 *   beta = first ? 0 : gamma / gamma_old;   alpha = gamma / (first ? delta : delta - beta gamma / alpha_old)
 *   d = r + beta d;  s = w + beta s (= A d);  x += alpha d;  r -= alpha s;   then sc[2] = gamma, sc[3] = alpha
 * Breakdown: gamma_old <= 0 gives beta = 0, and a denominator <= 0 gives alpha = 0 -- d and s still advance, x and r are left as they
 * are, and sc[3] is stored as 1e-300 instead of 0, so that the next step of the solve is not taken for a first step.
 * x0 != NULL: *fid = 1/2 |x_new - x0|^2 (the ADMM loss after the last step, for one extra read). */
int tv_cg_update(const tv_geom* g, void* x, void* r, void* d, void* s, const void* w, double* sc, const void* x0, double* fid,
                 void* ws, void* stream);
/* The z / u update of tv_admm_zu storing t = z - u_new in place of z: the next right-hand side x0 + rho D^T (z - u) is
 * then tv_DT_axpy(t, NULL, ..) over ONE gradient array; z = t + u whenever it is wanted. */
int tv_admm_tu(const tv_geom* g, const void* x, const void* x_prev, const void* x_next, void* t, void* u,
               double thresh, double* tv, void* ws, void* stream);
/* Conjugate-gradient vector updates with device-resident scalars (no host round trip):
 *   tv_cg_step1: alpha = rs/dAd;  x += alpha d;  r -= alpha Ad;  *rs_new = <r, r>
 *   tv_cg_step2: beta = rs_new/rs; d = r + beta d
 * Breakdown: tv_cg_step1 with dAd <= 0 takes alpha = 0 -- x and r are left as they are and *rs_new = <r, r> of the unchanged r.
 * tv_cg_step2 with rs <= 0 takes beta = 0 -- d becomes r, a restart from the steepest-descent direction. */
int tv_cg_step1(const tv_geom* g, void* x, void* r, const void* d, const void* Ad, const double* rs,
                const double* dAd, double* rs_new, void* ws, void* stream);
int tv_cg_step2(const tv_geom* g, void* d, const void* r, const double* rs_new, const double* rs, void* stream);

/* ---- small vector helpers on (nz,m,ny,nx) arrays -------------------------------------------- */
/* out = a - b (used for ADMM halos and residuals) */
int tv_sub(int32_t dtype, int64_t n, const void* a, const void* b, void* out, void* stream);
/* *result (device fp64) = <a, b> */
int tv_dot(const tv_geom* g, const void* a, const void* b, double* result, void* ws, void* stream);
/* x <- x - step * ((x - x0) + lambda * G); *fid = 1/2 |x_new - x0|^2  (README.md:122-123) */
int tv_subgrad_step(const tv_geom* g, void* x, const void* x0, const void* G, double step, double lambda,
                    double* fid, void* ws, void* stream);

/* ---- persistent small-volume loops (round 6, interface version 5) ------------------------------------------------------------------
 * The reference's user loops (README.md:107-124 sub-gradient descent, :141-157 Chambolle-Pock) on volumes that fit the caches
 * (its own shapes: README.md:76-79 rand(20,4,100,100), 256 x 256 / 512 x 512 images, pytv/tests.py:48 N = 100): n_iter iterations in
 * ONE cooperative launch -- every block keeps its sites for the whole loop and waits only for the blocks that own neighbouring sites
 * between the two phases of an iteration; arrays that neighbours read are accessed agent-coherently (csrc/tv_small.hip).
 * Unsharded volumes only (g->nz == g->nz_global, no halos); any scheme, fp32 / fp64, any nx (16-byte lanes when nx and the pointers
 * allow), pitched arrays, weight maps / volumes.  The stream must not run other kernels of the caller concurrently with these
 * launches in a way that could starve them of compute units (the blocks of a launch wait for each other).
 *   tv_small_supported       : 1 if the geometry fits (<= TV_SMALL_MAX_KVOXELS thousand voxels, default 4096; arrays below 2^31 bytes)
 *   tv_small_workspace_bytes : bytes of the scratch buffer `ws` for n_iter iterations per launch (block flags + per-block partials).
 *                              `ws` must be ZERO-FILLED once before its first use (hipMemset); the calls keep it consistent afterwards
 *                              (the blocks' phase counters continue from call to call: no reset per launch).  One `ws` per stream.
 *                              Safety net: should the blocks of a launch not all become resident (they wait for each other), the launch
 *                              abandons itself after ~2 s of polling instead of hanging: every hist entry of the call is NaN, the state
 *                              arrays are undefined and `ws` must be zero-filled again.  The verdict is the ABORT word, 32-bit word
 *                              8192 * 32 + 1 of `ws` (non-zero after an abandoned call), not the history: a diverging iteration or a
 *                              NaN in the input gives non-finite history entries from a launch that completed.
 *   tv_small_cp              : n_iter iterations of  p <- (p + sigma_A (x - x0)) / (1 + sigma_A);  q <- proj(q + sigma_D D x);
 *                              x <- x - tau p - tau D^T q  exactly as tv_cp_dual + tv_cp_primal compute them, x / p / q updated in
 *                              place.  hist (device fp64): hist[k * hist_stride] = |D x_k|_{2,1} (the iterate the dual update of
 *                              iteration k saw), hist[k * hist_stride + hist_fid_offset] = 1/2 |x_{k+1} - x0|^2
 *                              (a dense (n_iter, 2) array: stride 2, offset 1; 0 < hist_fid_offset < hist_stride)
 *   tv_small_subgrad_descent : n_iter iterations of  x <- x - step ((x - x0) + lambda G(x))  (tv_subgrad + tv_subgrad_step's
 *                              arithmetic); the iterate is ping-ponged between x and x_alt: after an ODD n_iter the result is in
 *                              x_alt, after an even one in x; norms_ext: (nz + 2) planes of scratch (1 / |D x|);
 *                              hist as above: TV(x_k) and 1/2 |x_{k+1} - x0|^2
 *   tv_small_admm            : n_outer outer iterations of scaled-form ADMM whose x-solve is n_cheb (1 .. 32) Chebyshev steps -- what
 *                              tv_DT_axpy + tv_normal_op2 + tv_cheb_step + tv_admm_tu compute per outer iteration:
 *                                r = x0 - x + rho D^T (t - D x);  e_{k+1} = e_k + alpha_k (r - (I + rho D^T D) e_k) + beta_k (e_k - e_{k-1}),
 *                                e_0 = e_{-1} = 0, k = 0 .. n_cheb-1;  x <- x + e_{n_cheb};
 *                                z = shrink(D x + u, thresh);  u <- u + D x - z;  t <- z - u
 *                              alpha / beta: HOST arrays of n_cheb coefficients (they follow from the spectral interval [1, 1 + rho L] alone).
 *                              STATE, updated in place: x, t (= z - u, a gradient array) and u (a gradient array), as the ordinary
 *                              single-reduction path keeps them -- calls can be mixed with tv_admm_tu based iterations.  SCRATCH, contents
 *                              undefined on entry and exit: r, e_a, e_b (images) and grad (a gradient array); all eight arrays differ.
 *                              hist[k * hist_stride] = |D x_{k+1}|_{2,1}, hist[k * hist_stride + hist_fid_offset] = |x_{k+1} - x0|^2
 *                              (NOT halved: the two scalars tv_admm_tu and the last tv_cheb_step deliver) of the x outer iteration k formed.
 *                              2 n_cheb phases per outer iteration; tv_small_workspace_bytes(g, n_outer) sizes `ws` for it as well, and one
 *                              `ws` may serve the three loops in any order. */
int    tv_small_supported(const tv_geom* g);
size_t tv_small_workspace_bytes(const tv_geom* g, int64_t n_iter);
int    tv_small_cp(const tv_geom* g, void* x, const void* x0, void* p, void* q, double sigma_D, double lambda, double tau,
                   double sigma_A, int64_t n_iter, double* hist, int64_t hist_stride, int64_t hist_fid_offset, void* ws, void* stream);
int    tv_small_subgrad_descent(const tv_geom* g, void* x, void* x_alt, const void* x0, void* norms_ext, double step, double lambda,
                                int64_t n_iter, double* hist, int64_t hist_stride, int64_t hist_fid_offset, void* ws, void* stream);
int    tv_small_admm(const tv_geom* g, void* x, const void* x0, void* t, void* u, void* r, void* e_a, void* e_b, void* grad, double rho,
                     double thresh, const double* alpha, const double* beta, int64_t n_cheb, int64_t n_outer, double* hist,
                     int64_t hist_stride, int64_t hist_fid_offset, void* ws, void* stream);

/* ---- multi-GPU: z-slab neighbours over RCCL, one process per GPU ------------------------------ */
/* The reference is single-GPU (its README only remarks that the (Nz, M, N, N) layout "can be decomposed easily along z",
 * README.md:235).  Rank r holds the planes [z0, z0 + nz) (tv_geom::z0 / nz_global) and, per operator apply, trades the
 * boundary plane(s) named by the halo arguments above with ranks r-1 / r+1: a chain, not a ring.
 *   tv_ctx_unique_id : rank 0 fills 128 bytes; the host program hands them to every rank by its own means
 *   tv_ctx_create    : collective over the nranks processes (ncclCommInitRank); `device` = HIP device of this process
 *   tv_halo_exchange : ONE grouped exchange on `stream`, in stream order, no host synchronisation: `count` elements of
 *                      `dtype` to / from prev_rank and next_rank (-1 = no such neighbour; NULL buffer = nothing that way).
 *                      Matching is per peer in posting order: a rank's send_next meets its next rank's recv_prev.
 *   tv_allreduce_f64 : in-place sum / max of n fp64 device words over all ranks, on `stream`
 * RCCL is bound at run time (dlopen): hosts that never create a context never load it.
 * Errors: 0 ok, < 0 argument, 1..999 hipError_t, 1000 + ncclResult_t. */
#define TV_UNIQUE_ID_BYTES 128
#define TV_SUM 0
#define TV_MAX 1
typedef struct tv_ctx tv_ctx;
int tv_ctx_unique_id(void* id_out);
int tv_ctx_create(tv_ctx** ctx, int rank, int nranks, const void* unique_id, int device);
int tv_ctx_destroy(tv_ctx* ctx);
int tv_ctx_rank(const tv_ctx* ctx);
int tv_ctx_size(const tv_ctx* ctx);
int tv_halo_exchange(tv_ctx* ctx, int32_t dtype, int64_t count, int prev_rank, int next_rank, const void* send_prev,
                     const void* send_next, void* recv_prev, void* recv_next, void* stream);
int tv_allreduce_f64(tv_ctx* ctx, double* buf, int64_t n, int32_t op, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PYTV4D_H */
