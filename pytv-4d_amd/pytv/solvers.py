"""Device-resident drivers of the reference's user-level loops.

The reference ships its solvers as README snippets that round-trip numpy <-> GPU four times per
iteration (README.md:118-124 sub-gradient descent, :141-157 Chambolle-Pock; ADMM is only mentioned,
:26,135).  Here the state lives on the GPU(s) for the whole run and every iteration is a handful of
fused HIP kernels (include/pytv4d.h):

    ChambollePock       tv_cp_fused + tv_cp_fixup (one sweep: q read and written once)  (5+2Nd) words/voxel + fix-up
                        or the pair tv_cp_dual (D + sigma-step + projection, TV partial) (1+2Nd)
                        + tv_cp_primal (fidelity dual + D^T + primal step, loss partial)  (Nd+5)
    AcceleratedChambollePock  tv_cp_dual on the extrapolated point + tv_cp_primal_accel (D^T, closed-form fidelity prox, extrapolation)  (Nd+4)
                        or tv_cp_accel_sweep + tv_cp_accel_fixup (one sweep, 5+2Nd words/voxel + fix-up)
                        with the step schedule of Chambolle & Pock 2011, Algorithm 2: O(1/k^2) instead of O(1/k)
    RobustChambollePock tv_cp_dual on the extrapolated point + tv_cp_primal_prox (D^T, pointwise prox of an L1 / Huber / L2 fidelity,
                        extrapolation)  (Nd+4): TV-L1 and TV-Huber for impulse noise (Chambolle & Pock 2011, section 6.2.2)
    PoissonChambollePock tv_cp_dual on the extrapolated point + tv_cp_primal_kl (D^T, cancellation-free prox of the Kullback-Leibler
                        fidelity, extrapolation)  (Nd+4): TV-KL for photon-counting data
    WeightedChambollePock tv_cp_dual on the extrapolated point + tv_cp_primal_wls (D^T, prox of a per-voxel weighted quadratic fidelity
                        clamped to a box, extrapolation)  (Nd+5): inpainting of unknown voxels, heteroscedastic data, bounds on the iterate
    HuberChambollePock  tv_cp_dual_huber on the extrapolated point (shrink + projection, Huber partial) + tv_cp_primal_accel with fixed steps
                        (or tv_cp_huber_sweep + tv_cp_accel_fixup: one sweep, 5+2Nd words/voxel + fix-up):
                        the Huber-TV regulariser against staircasing, linearly convergent (Chambolle & Pock 2011, Algorithm 3)
    AdaptiveTVChambollePock  tv_cp_dual_wtv on the extrapolated point (projection onto a per-voxel radius reg * g_i, weighted TV partial)
                        (2Nd+2) + tv_cp_primal_accel with the accelerated schedule: spatially adaptive TV (noise-adaptive lambda,
                        edge-stopping weights, protected regions)
    AdaptiveHuberChambollePock  tv_cp_dual_hwtv on the extrapolated point (per-voxel shrink and radius, weighted Huber partial) (2Nd+2) +
                        tv_cp_primal_accel with fixed steps (or tv_cp_hwtv_sweep + tv_cp_accel_fixup: one sweep, 6+2Nd words/voxel +
                        fix-up): the Huber-TV regulariser under a per-voxel weight, linearly convergent
    VectorialTVChambollePock  tv_cp_dual_vtv on the extrapolated point (ONE projection per spatial site over all frames and channels: a
                        thread walks the frames of its site) (2Nd+1 up to 8 frames, hybrid 4; at most 3Nd+2 beyond) + tv_cp_primal_accel with the
                        accelerated schedule: channel-coupled (vectorial / joint) TV of multi-energy, multi-contrast and colour stacks
    ChambollePockOperator  the same with a user data-fidelity operator A / A^T on device tensors (tv_cp_dual + tv_cpop_*)
    ADMM                tv_admm_tu / tv_admm_zu, tv_DT_axpy, tv_normal_op2 (I + rho D^T D from x alone, two dot products) +
                        tv_cg_update (single-reduction CG; textbook tv_cg_step1/2 kept)
    SubgradientDescent  tv_subgrad_step_fused (TV, G and the descent step in ONE pass over x) or tv_subgrad + tv_subgrad_step

With a ``Slab`` (one process per GPU) each rank holds a contiguous z-slab; one boundary plane per
neighbour is exchanged per operator apply (two for the radius-2 kernels) and, for Chambolle-Pock,
hidden behind the interior planes' kernel.  Scalars (TV, fidelity, CG dots) stay on the device as
fp64 and are all-reduced there; nothing synchronises with the host inside the loop.
"""

import math
import types

import torch

from . import _native as _nv
from .slab import HaloPlan, Slab

__all__ = ["ChambollePock", "AcceleratedChambollePock", "RobustChambollePock", "PoissonChambollePock", "WeightedChambollePock", "HuberChambollePock", "AdaptiveTVChambollePock", "AdaptiveHuberChambollePock", "VectorialTVChambollePock", "ChambollePockOperator", "ADMM", "SubgradientDescent", "cp_step_size", "cp_step_pair",
           "accel_schedule", "cp_linear_steps", "auto_pitch", "operator_norm_sq"]


def cp_step_size(nz_global, m, reg_z_over_reg, reg_time, time_weight_max=1.0):
    """tau = 1 / (1 + L^2) with L^2 = 4 (2 + reg_z [z active] + reg_time * time_weight_max [t active]) >= |D|^2.
    time_weight_max: the largest per-pixel weight on the time regularisation (``factor_reg_static`` where
    ``mask_static`` is set, the maximum of a weight map; ``Geometry.time_weight_max``) -- the time channels are scaled
    by its square root, so it belongs in the bound.  Reduces to the reference's 1/(8+1) in 2-D (README.md:143)."""
    z = nz_global > 1 and reg_z_over_reg > 0
    t = m > 1 and reg_time > 0
    return 1.0 / (1.0 + 4.0 * (2.0 + (reg_z_over_reg if z else 0.0) + (reg_time * time_weight_max if t else 0.0)))


def normal_spectral_bound(scheme, nz_global, m, reg_z_over_reg, reg_time, time_weight_max=1.0):
    """L >= lambda_max(D^T D): 4 per one-sided difference axis (1 per halved central one) times the square of the axis weight;
    hybrid is the mean of the two one-sided operators.  1 / (1 + L) is cp_step_size for the one-sided schemes."""
    z = nz_global > 1 and reg_z_over_reg > 0
    t = m > 1 and reg_time > 0
    s = 2.0 + (reg_z_over_reg if z else 0.0) + (reg_time * time_weight_max if t else 0.0)
    return (1.0 if scheme == "central" else 4.0) * s


def cp_step_pair(L2, tau=None, sigma=None, names=("tau", "sigma")):
    """(tau, sigma) of a primal-dual iteration whose convergence wants tau sigma L^2 <= 1 (``L2`` = ``normal_spectral_bound``) as Python
    floats.  Both None: 1 / sqrt(L^2) each; one given: the other is 1 / (L^2 times it).  ValueError unless both are finite and > 0 and
    tau sigma L^2 <= 1 + 1e-12; ``names``: what the caller's parameters are called, for the messages."""
    if tau is None and sigma is None:
        tau = sigma = 1.0 / math.sqrt(L2)
    elif tau is None:
        tau = 1.0 / (L2 * float(sigma)) if float(sigma) != 0.0 else 0.0      # (0 is refused below, not by the division)
    elif sigma is None:
        sigma = 1.0 / (L2 * float(tau)) if float(tau) != 0.0 else 0.0
    tau, sigma = float(tau), float(sigma)
    if not (tau > 0.0 and sigma > 0.0 and math.isfinite(tau + sigma)):
        raise ValueError("%s and %s must be finite and > 0" % tuple(names))
    if tau * sigma * L2 > 1.0 + 1e-12:
        raise ValueError("%s * %s * L^2 = %.6g > 1 (L^2 = %g: normal_spectral_bound): the iteration need not converge"
                         % (names[0], names[1], tau * sigma * L2, L2))
    return tau, sigma


def accel_schedule(tau0, sigma0, gamma, n, start=0):
    """Step sizes of iterations start .. start + n - 1 of the accelerated Chambolle-Pock iteration (Chambolle & Pock 2011, Algorithm 2)
    for a gamma-strongly convex primal term: three fp64 numpy arrays (tau, sigma, theta) of length n with
        theta_k = 1 / sqrt(1 + 2 gamma tau_k),  tau_{k+1} = theta_k tau_k,  sigma_{k+1} = sigma_k / theta_k.
    A pure function of its arguments (the schedule does not depend on the data), computed on the host in fp64 from k = 0 whatever
    ``start`` is: ``start=k`` continues the arrays of ``start=0`` bit for bit.  sigma_k is formed as sigma0 (tau0 / tau_k), not by its
    own recurrence, so tau_k sigma_k = tau0 sigma0 holds to a few roundings for every k (the product is what the convergence proof
    bounds by 1 / L^2).  gamma = 0: theta = 1 and constant steps, Algorithm 1.  tau_k gamma k -> 1 as k grows."""
    import numpy as np
    tau0, sigma0, gamma, n, start = float(tau0), float(sigma0), float(gamma), int(n), int(start)
    if not (tau0 > 0.0 and sigma0 > 0.0 and gamma >= 0.0) or not all(np.isfinite((tau0, sigma0, gamma))):
        raise ValueError("accel_schedule: tau0 and sigma0 must be finite and > 0, gamma finite and >= 0")
    if n < 0 or start < 0:
        raise ValueError("accel_schedule: n and start must be >= 0")
    tau, theta = np.empty(start + n), np.empty(start + n)
    t = tau0
    for k in range(start + n):
        th = 1.0 / np.sqrt(1.0 + 2.0 * gamma * t)
        tau[k], theta[k] = t, th
        t = th * t
    sigma = sigma0 * (tau0 / tau)
    return tau[start:].copy(), sigma[start:].copy(), theta[start:].copy()


def cp_linear_steps(L2, gamma, delta):
    """(tau, sigma, theta, mu) of the LINEARLY convergent Chambolle-Pock iteration (Chambolle & Pock 2011, Algorithm 3) for a saddle problem
    whose primal term is gamma-strongly convex and whose dual term is delta-strongly convex, |K|^2 <= ``L2``, as Python floats:
        mu = 2 sqrt(gamma delta) / sqrt(L2),  tau = mu / (2 gamma),  sigma = mu / (2 delta),  theta = 1 / (1 + mu)
    so that tau sigma L2 = 1; the iterates converge as O(omega^k) with omega = (1 + theta) / (2 + mu) < 1.  sigma is formed as
    1 / (L2 tau) -- the same number, and the product then equals 1 to three roundings whatever the arguments.  ValueError unless the
    three arguments are finite and > 0."""
    L2, gamma, delta = float(L2), float(gamma), float(delta)
    if not all(math.isfinite(v) and v > 0.0 for v in (L2, gamma, delta)):
        raise ValueError("cp_linear_steps: L2, gamma and delta must be finite and > 0")
    mu = 2.0 * math.sqrt(gamma * delta) / math.sqrt(L2)
    tau = mu / (2.0 * gamma)
    return tau, 1.0 / (L2 * tau), 1.0 / (1.0 + mu), mu


def operator_norm_sq(A, AT, like, n_iter=20, seed=0, slab=None):
    """Upper estimate of |A|^2 = lambda_max(A^T A) for a pair of callables on device tensors (``ChambollePockOperator``'s ``A`` / ``AT``):
    ``n_iter`` steps of the power iteration v <- A^T A v / |A^T A v| from a seeded random image shaped like ``like``, the last |A^T A v|
    (|v| = 1) times a safety factor of 1.05 -- the power iteration approaches lambda_max from below.  Returns a Python float.
    ``n_iter`` calls of each operator, every scalar stays on the device: ONE host synchronisation per call, not one per iteration
    (a sharded ``slab`` adds its all-reduce of one scalar per iteration; every rank gets the same number)."""
    n_iter = int(n_iter)
    if n_iter < 1:
        raise ValueError("operator_norm_sq: n_iter must be >= 1")
    gen = torch.Generator(device=like.device)
    gen.manual_seed(int(seed) + (slab.rank if slab is not None else 0))
    v = torch.randn(like.shape, dtype=like.dtype, device=like.device, generator=gen)

    def norm(t):
        s = torch.sum(torch.linalg.vector_norm(t, dtype=torch.float64) ** 2).reshape(1)
        if slab is not None:
            slab.allreduce_sum_(s)
        return torch.sqrt(s)

    v = v / norm(v).to(v.dtype)
    lam = None
    for _ in range(n_iter):
        w = AT(A(v))
        lam = norm(w)
        v = w / torch.clamp_min(lam, torch.finfo(torch.float64).tiny).to(w.dtype)
    return 1.05 * float(lam.item())


def chebyshev_coefficients(lmax, n):
    """(alpha_k, beta_k), k = 0 .. n-1, of e_{k+1} = e_k + alpha_k (b - A e_k) + beta_k (e_k - e_{k-1}), e_0 = e_{-1} = 0, for a
    symmetric A with spectrum in [1, lmax] (Saad, Iterative Methods for Sparse Linear Systems, alg. 12.1 as a three-term
    recurrence).  The scalars depend on the interval only: no dot product, no all-reduce."""
    theta, delta = 0.5 * (lmax + 1.0), 0.5 * (lmax - 1.0)
    if delta <= 1e-14 * theta:
        return [(1.0 / theta, 0.0)] * n
    sigma = theta / delta
    out, rho_prev = [(1.0 / theta, 0.0)], 1.0 / sigma
    for _ in range(1, n):
        rho_k = 1.0 / (2.0 * sigma - rho_prev)
        out.append((2.0 * rho_k / delta, rho_k * rho_prev))
        rho_prev = rho_k
    return out[:n]


def auto_pitch(ny, nx, dtype, frame_pad_bytes=0):
    """(row_pitch, frame_pitch) in elements for a solver's private state, or None when dense storage is as good.
    Rows are rounded up to 128 bytes when that costs at most 8 % (a frame whose rows are not whole cache lines has every row
    segment straddle lines and 64-byte write sectors: 64 x 8 x 1000 x 1000 runs the one-sweep Chambolle-Pock iteration in 9.2 ms
    padded against 18.1 ms dense, profiles/r4_pitch_bench.txt); otherwise -- short rows, where 128-byte rounding would add up to
    a quarter more bytes and measured SLOWER (256 x 4 x 100 x 100: 0.33 against 0.27 ms) -- only ragged rows (Nx not a multiple
    of the 16-byte lane) are rounded up to the lane, which takes them off the scalar-lane kernels.
    frame_pad_bytes: extra bytes between frames (round 4 measured that de-aliasing the frame pitch does NOT move the one-sweep
    kernel: tools/archive/bwtest4, tools/archive/alias_probe.py, profiles/r4_alias_probe.txt, profiles/r4_bwtest4_frame_pitch.txt; kept as an argument for experiments)."""
    es = 4 if dtype == torch.float32 else 8
    lane = 16 // es
    nx, ny = int(nx), int(ny)
    rp128 = ((nx * es + 127) // 128 * 128) // es
    if rp128 != nx and (rp128 - nx) <= 0.08 * nx:
        rp = rp128
    elif nx % lane != 0:
        rp = (nx + lane - 1) // lane * lane
    else:
        rp = nx
    pad = int(frame_pad_bytes) // es
    if rp == nx and pad == 0:
        return None
    return rp, ny * rp + pad


def _plane0(halo):
    """plane 0 of an optional halo buffer"""
    return halo[0] if halo is not None else None


def _redoc(fn, head=None, tail=""):
    """The method ``fn`` again -- the same code object, signature and defaults, no call in between -- under the docstring ``head``
    (None: its own) + ``tail``.  How a class states its own text (its model's ``_GAP_DOC`` / ``_RES_DOC``, what its scalars mean) for a
    method whose one body lives in a base class."""
    f = types.FunctionType(fn.__code__, fn.__globals__, fn.__name__, fn.__defaults__, fn.__closure__)
    f.__qualname__, f.__doc__ = fn.__qualname__, (fn.__doc__ if head is None else head) + tail
    return f


class _SlabProblem:
    """Common state: local slab geometry (and sub-slab geometries for interior / edge launches)."""

    def __init__(self, x0, scheme, reg_z_over_reg, reg_time, mask_static, factor_reg_static, slab, pitch=None):
        """pitch: "auto" (the solvers' default) = ``auto_pitch`` decides: dense for frames whose rows are whole cache lines (every
        BASELINE configuration), padded rows otherwise; None / "dense" = the state is dense like the caller's x0;
        (row_pitch, frame_pitch) in elements = every array of the solver's state (x0 is COPIED into such storage) is pitched
        (include/pytv4d.h, tv_geom::row_pitch / frame_pitch).  With padded state ``result()`` / ``x`` are (Nz, M, Ny, Nx) VIEWS of
        padded storage (``.contiguous()`` gives a dense copy)."""
        if slab is not None:
            self._refuse_thin_slabs(slab, reg_z_over_reg)     # first: the one refusal that every rank of a job must raise alike
        if not isinstance(x0, torch.Tensor) or not x0.is_cuda:
            raise ValueError("x0 must be a device tensor (this rank's z-slab of the volume)")
        if x0.dim() != 4:
            raise ValueError("x0 must be 4-D (Nz_local, M, N, N)")
        if isinstance(pitch, str):
            if pitch not in ("auto", "dense"):
                raise ValueError("pitch must be 'auto', 'dense' (or None) or (row_pitch, frame_pitch)")
            pitch = auto_pitch(x0.shape[2], x0.shape[3], x0.dtype) if pitch == "auto" else None
        self.pitch = (0, 0) if pitch is None else (int(pitch[0]), int(pitch[1]))
        self.x0 = x0.contiguous() if self.pitch == (0, 0) else x0
        self.device = x0.device
        self.dtype = x0.dtype
        self.scheme = scheme
        self.slab = slab if slab is not None else Slab(x0.shape[0], rank=0, world=1)
        if self.slab.nz != x0.shape[0]:
            raise ValueError("x0 has %d planes but this rank's slab has %d" % (x0.shape[0], self.slab.nz))
        self.kw = dict(reg_z_over_reg=reg_z_over_reg, reg_time=reg_time, mask_static=mask_static,
                       factor_reg_static=factor_reg_static)
        self._geoms = {}
        self.lib = _nv.lib()
        nz, m, ny, nx = self.x0.shape
        self._pkw = dict(row_pitch=self.pitch[0], frame_pitch=self.pitch[1])
        geo = _nv.Geometry((nz, m, ny, nx), scheme, self.dtype, self.device, nz_global=self.slab.nz_global, z0=self.slab.z0,
                           **self.kw, **self._pkw)
        if geo.pitched:
            x0p = geo.new_image()
            x0p.copy_(x0)
            self.x0 = x0p
        self._wvol = None
        if geo.weight_vol is not None:
            # per-voxel weights on the time regularisation (mask_static = float array of this rank's slab shape): the
            # neighbours' boundary planes of the weight are fetched ONCE (the sub-gradient's ghost-plane norms read them)
            wv = geo.weight_vol[0]
            gp = geo.new_image(1) if self.slab.prev is not None else None
            gn = geo.new_image(1) if self.slab.next is not None else None
            self.slab.wait(self.slab.exchange(send_prev=wv[0:1] if self.slab.prev is not None else None,
                                              send_next=wv[nz - 1:nz] if self.slab.next is not None else None,
                                              recv_prev=gp, recv_next=gn))
            self._wvol = (wv, gp, gn)
            twm = torch.tensor([geo.time_weight_max], dtype=torch.float64, device=self.device)
            if self.slab.sharded:
                self.slab.allreduce_max_(twm)
            self._twmax = float(twm.item())
            geo = None
        self.geo = geo if geo is not None else self.geom(0, nz)
        self._geoms[(0, nz)] = self.geo

    HALO_PLANES = 1     # planes of x a kernel reads beyond this rank's slab, per neighbour (``SubgradientDescent``, ``ADMM``: 2)

    def _refuse_thin_slabs(self, s, reg_z_over_reg):
        """A solver with ``HALO_PLANES`` = 2 cannot serve a rank that holds one plane: that rank would send one plane where its neighbour
        receives two (``HaloPlan.exchange_image2``), and its plane z0 - 2 belongs to the rank two away.  Decided from ``slab.parts``,
        which every rank holds identically, and before anything of the constructor communicates (the ghost planes and the maximum
        of a per-voxel time weight): every rank raises the same error, none is left waiting in a collective.  A volume whose z axis
        is not regularised (reg_z_over_reg = 0, or one plane in all) exchanges nothing and is served at any partition."""
        need = self.HALO_PLANES
        sizes = [n for _, n in s.parts]
        if need > 1 and s.sharded and s.nz_global > 1 and float(reg_z_over_reg) > 0 and min(sizes) < need:
            raise ValueError("%s reads %d halo planes from each z-neighbour, so every rank must hold >= %d planes: %d planes over %d ranks "
                             "are split as %s" % (type(self).__name__, need, need, s.nz_global, s.world, sizes))

    def _one_sweep_default(self, sharded_ok):
        """The default-path rule of the Chambolle-Pock solvers: the one-sweep kernel where tv_cp_fused_supported accepts the geometry --
        except on volumes too small to fill the GPU with its blocks (8 rows x 256 columns x >= 8 planes x all frames each: a block holds
        >= 16 k x M voxels and a CU takes 8 / M of them, so 256 CUs want >= 33 Mvoxel for one full round; tools/archive/fused_vs_pair.py:
        0.5 - 0.7 x of the kernel pair at 6 - 8 Mvoxel with few planes, break-even at 8 - 13 Mvoxel, 1.15 - 1.25 x faster from 16 Mvoxel on
        whatever the plane size -- 256x1x512x512 runs 990 - 1040 it/s against 870).  Option TV_FUSED_MIN_KVOXELS (thousands of voxels of
        this rank's slab) moves the switch.  sharded_ok: False = never on a sharded slab (the solvers whose one-sweep path has no
        sweep / exchange / fix-up schedule)."""
        if self.slab.sharded and not sharded_ok:
            return False
        return bool(self.lib.tv_cp_fused_supported(self.geo.ref)) and self.x0.numel() >= 1024 * _nv.get_option("TV_FUSED_MIN_KVOXELS", 16384)

    # ---- persistent small-volume loops (round 6; csrc/tv_small.hip) ------------------------------------------------------------------
    SMALL_MAX_VOXELS = 4 << 20      # the automatic rule: volumes of at most 4 Mvoxel take it (the reference's own shapes hold 0.07 - 1; measured against
                                    # the kernel pair / one-pass kernel from hipGraphs: x 2.5 - 3.7 up to 1 Mvoxel, x 1.5 - 2.2 at 4, x 1.0 - 1.1 at 9: profiles/r6_small_volume_larger.txt)
    SMALL_BLOCK = 128               # iterations per cooperative launch

    def _small_ok(self, persistent):
        """persistent: None = automatic (unsharded, <= SMALL_MAX_VOXELS, geometry supported), True = required, False = off"""
        if persistent is False:
            return False
        ok = (not self.slab.sharded) and bool(self.lib.tv_small_supported(self.geo.ref))
        if persistent is True:
            if not ok:
                raise ValueError("persistent=True: the persistent small-volume kernels take unsharded volumes that tv_small_supported accepts")
            return True
        return ok and self.x0.numel() <= self.SMALL_MAX_VOXELS

    def _small_ws(self):
        """scratch of the persistent kernels: block flags (zero-filled ONCE: their phase counters continue from launch to launch) + partials"""
        if getattr(self, "_small_ws_buf", None) is None:
            nbytes = self.lib.tv_small_workspace_bytes(self.geo.ref, self.SMALL_BLOCK)
            self._small_ws_buf = torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=self.device)
        return self._small_ws_buf

    def _small_blocks(self, rows, launch):
        """``len(rows)`` iterations in blocks of ``SMALL_BLOCK`` per cooperative launch: ``launch(k, row_ptr)`` enqueues k of them, the reduction
        that closes the launch writing their scalars into the rows from ``row_ptr`` on (stride ``rows.stride(0)``)."""
        if rows.stride(1) != 1:
            raise ValueError("rows must be a (n, %d) fp64 tensor with contiguous rows" % rows.shape[1])
        n, done = rows.shape[0], 0
        while done < n:
            k = min(self.SMALL_BLOCK, n - done)
            launch(k, rows[done].data_ptr())
            done += k

    # 32-bit word of the workspace that a launch raises when it abandons itself (csrc/tv_small.hip: small_abort_word, kMaxSmallBlocks * kFlagStride + 1)
    SMALL_ABORT_WORD = 8192 * 32 + 1

    def _small_check(self):
        """the persistent kernels abandon a launch whose blocks cannot all run at once instead of hanging (csrc/tv_small.hip, small_sync): they
        raise the workspace's abort word.  That word is the verdict, not the loss: a diverging iteration or a NaN in the input gives a non-finite
        loss on every path and is returned as it is.  An abandoned workspace is dropped (the next launch gets a zero-filled one)."""
        ws = getattr(self, "_small_ws_buf", None)
        if ws is None:
            return
        if int(ws.view(torch.int32)[self.SMALL_ABORT_WORD].item()) != 0:        # one 4-byte device-to-host copy (waits for the launches)
            self._small_ws_buf = None
            raise RuntimeError("the persistent small-volume kernel abandoned its launch (its blocks were not resident together); the state is "
                               "undefined: construct the solver with persistent=False or lower TV_SMALL_BLOCKS_PER_CU")

    def geom(self, a, b):
        """Geometry of local planes [a, b) seen as a slab of the global volume."""
        key = (a, b)
        if key not in self._geoms:
            nz, m, ny, nx = self.x0.shape
            if self._wvol is None:
                self._geoms[key] = _nv.Geometry((b - a, m, ny, nx), self.scheme, self.dtype, self.device,
                                                nz_global=self.slab.nz_global, z0=self.slab.z0 + a, **self.kw, **self._pkw)
            else:
                wv, gp, gn = self._wvol
                kw = dict(self.kw, mask_static=False, factor_reg_static=0)
                dev = (wv[a:b], wv[a - 1] if a > 0 else (gp[0] if gp is not None else None),
                       wv[b] if b < nz else (gn[0] if gn is not None else None))
                g = _nv.Geometry((b - a, m, ny, nx), self.scheme, self.dtype, self.device, nz_global=self.slab.nz_global,
                                 z0=self.slab.z0 + a, weight_dev=dev, **kw, **self._pkw)
                g.time_weight_max = self._twmax
                self._geoms[key] = g
        return self._geoms[key]

    @property
    def stream(self):
        return _nv.current_stream(self.device)

    def new_plane(self, n=1):
        """n image planes (halo buffers) with the state's pitches"""
        _, m, ny, nx = self.x0.shape
        if self.pitch != (0, 0):
            return self.geo.new_image(n)
        return torch.empty((n, m, ny, nx), dtype=self.dtype, device=self.device)

    # ---- buffers of the Chambolle-Pock loops: one boundary plane of x and of q per neighbour that the scheme reads -----------------------
    def _halo_set(self):
        """A set of halo planes of its own: dict(xp, xn, qp, qn), None where ``plan`` needs no plane (the loop's set is bound by
        ``_bind_loop_buffers``; a check that must leave those alone takes a second one)."""
        pl = self.plan
        return dict(xp=self.new_plane() if pl.x_need_prev else None, xn=self.new_plane() if pl.x_need_next else None,
                    qp=self.new_plane() if pl.g_need_prev else None, qn=self.new_plane() if pl.g_need_next else None)

    def _bind_loop_buffers(self):
        """``ws`` (the kernels' workspace), ``plan`` (which planes travel) and the loop's halo planes ``xh_prev / xh_next / qh_prev / qh_next``"""
        self.ws = self.geo.workspace()
        self.plan = HaloPlan(self.slab, self.scheme, self.geo.z_active)
        h = self._halo_set()
        self.xh_prev, self.xh_next, self.qh_prev, self.qh_next = h["xp"], h["xn"], h["qp"], h["qn"]

    # ---- the arena (round 5, OPT-IN): ONE allocation for the arrays an iteration streams through ---------------------------------------
    # The time of the streaming kernels depends on where their arrays sit in physical memory (EXPERIMENTS.md section 3, round 4: the
    # "placement lottery" -- separate allocations land anywhere: 31.3 - 34.2 ms per north-star sweep from one construction to the next).
    # Carved out of ONE allocation with 24 - 48 MiB between consecutive arrays the sweep takes the SAME time construction after
    # construction (spread 0.4 - 0.5 % against 6 - 9 %: profiles/r5_slab_placement_probe{,2,3,4}.txt, tools/archive/slab_placement_probe.py) --
    # but WHICH time is decided by where the one big allocation lands: 31.1 ms on one box, 33.1 - 33.4 on three others, alternating
    # 31.05 / 32.1 from construction to construction on a fifth; a second arena measured beside the first (``_tune_arena``) does not
    # help where both land on the slow level (profiles/r5_bench_northstar_arena_first_command.json: 33.2 ms, 35.5 ms per iteration
    # against 33.8 with the per-array tuner).  Deterministic, not fast: it is therefore an OPTION (``arena=True``) for callers who
    # want run-to-run reproducible timing; the default stays separate allocations + the measuring tuner.
    ARENA_GAP_BYTES = 32 << 20
    _arena = None
    _arena_closed = False

    def _image_elems(self):
        nz, m, ny, nx = self.x0.shape
        return nz * m * (self.pitch[1] if self.pitch != (0, 0) else ny * nx)

    def _arena_open(self, n_images, n_grads, enable=None):
        """enable: None / False = off (the default), True = on; returns whether an arena is open"""
        img = self._image_elems()
        es = self.x0.element_size()
        if enable is None:
            enable = False
        if not enable or self.device.type != "cuda":
            return False
        gap = self.ARENA_GAP_BYTES // es
        al = 256 // es                            # every carve starts on a 256-byte boundary (round-5 advice: the C entry points want 16)
        rnd = lambda n: -(-n // al) * al
        total = n_images * (rnd(img) + gap) + n_grads * (rnd(img * self.geo.nd) + gap)
        try:
            self._arena = torch.empty(total, dtype=self.dtype, device=self.device)
        except RuntimeError:                      # no single block of that size: separate allocations (and the placement tuner)
            self._arena = None
            torch.cuda.empty_cache()
            return False
        self._arena_off, self._arena_gap, self._arena_align, self._arena_closed = 0, gap, al, False
        return True

    def _arena_close(self):
        """the state is carved: later new_image() / new_grad() calls allocate on their own"""
        self._arena_closed = True

    def _arena_take(self, elems):
        a = self._arena
        if a is None or self._arena_closed or self._arena_off + elems > a.numel():
            return None
        v = a[self._arena_off:self._arena_off + elems]
        self._arena_off += -(-elems // self._arena_align) * self._arena_align + self._arena_gap
        return v

    def new_image(self, zero=True):
        """an array like x0 (this rank's planes) with the state's pitches; pads always zero"""
        buf = self._arena_take(self._image_elems())
        if buf is not None:
            nz, m, ny, nx = self.x0.shape
            if self.pitch != (0, 0):
                buf.zero_()
                return buf.as_strided((nz, m, ny, nx), self.geo.image_strides())
            if zero:
                buf.zero_()
            return buf.view(nz, m, ny, nx)
        if self.pitch != (0, 0):
            return self.geo.new_image()
        return torch.zeros_like(self.x0) if zero else torch.empty_like(self.x0)

    def new_grad(self):
        """a zeroed gradient-like array (nz, Nd, M, Ny, Nx) with the state's pitches"""
        buf = self._arena_take(self._image_elems() * self.geo.nd)
        if buf is not None:
            nz, m, ny, nx = self.x0.shape
            nd = self.geo.nd
            buf.zero_()
            if self.pitch != (0, 0):
                fp, rp = self.geo.frame_pitch, self.geo.row_pitch
                return buf.as_strided((nz, nd, m, ny, nx), (nd * m * fp, m * fp, fp, rp, 1))
            return buf.view(nz, nd, m, ny, nx)
        return self.geo.new_grad()

    def image_copy(self, src):
        out = self.new_image(zero=False)
        out.copy_(src)
        return out

    def result(self):
        """The iterate as a DENSE (Nz, M, Ny, Nx) tensor: with padded state (``pitch``) a contiguous copy -- callers that ``.view(-1)``
        it, take its ``data_ptr()`` or hand it to the dense ``tv_*`` entry points must not see pad columns (round-4 advice); ``.x``
        stays the raw (possibly strided) view of the solver's storage."""
        return self.x.contiguous() if self.pitch != (0, 0) else self.x

    # ---- hipGraph replay of the loop -------------------------------------------------------------------------------------------------
    _ROLES = ()     # the attributes whose bindings a step() may rotate at Python level (buffer ping-pongs, counters)

    def _run_graphed_head(self, hist, use_graph):
        """Two eager iterations (also the warm-up of the capture), then graph replays over the rows of ``hist``; returns the row at which
        the caller's eager tail starts (0: nothing ran)."""
        n = hist.shape[0]
        if not (use_graph and not self.slab.sharded and n >= 2 + 2 * self.GRAPH_BLOCK):
            return 0
        self.step(hist[0])
        self.step(hist[1])
        return 2 + self._run_graphed_from(hist, 2, n)

    def _run_graphed_from(self, hist, first, n_iter):
        """Capture GRAPH_BLOCK iterations (not executed during capture) and replay them over hist[first:]; returns how many iterations ran."""
        K = self.GRAPH_BLOCK
        nrep = (n_iter - first) // K
        if nrep < 1:
            return 0
        # the steps REBIND buffers at Python level (x / x_alt, q / q_alt, u / u_alt; the Chebyshev x-solve writes the new image next to
        # the old one and swaps x / d / Ad / b): a capture that fails part-way must not leave them pointing at buffers whose kernels
        # never ran (round-3 advice)
        saved = {k: getattr(self, k) for k in self._ROLES if hasattr(self, k)}
        try:
            buf = torch.zeros((K, hist.shape[1]), dtype=torch.float64, device=self.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for k in range(K):
                    self.step(buf[k])
            # a block that does not return the buffers to their roles (odd number of role swaps) would not be the same iteration when
            # it is replayed -- cannot happen with GRAPH_BLOCK even, checked all the same
            ok = all(getattr(self, k) is v for k, v in saved.items() if isinstance(v, torch.Tensor))
        except Exception:
            ok = False
        for k, v in saved.items():               # nothing ran: undo the bookkeeping (the counters too)
            setattr(self, k, v)
        if not ok:
            return 0                             # stay eager
        done = 0
        for r in range(nrep):
            graph.replay()
            hist[first + done:first + done + K].copy_(buf)
            done += K
        return done

    # ---- placement of an x -> x_alt ping-pong by measurement (ChambollePock._tune_x_placement, SubgradientDescent._tune_placement) ------
    # ``launch()`` enqueues one x -> x_alt step of the solver's real kernel with whatever is bound NOW (x, x_alt, x0, p, q).
    def _pp_one(self, launch, i_buf, o_buf):
        """one timed step i_buf -> o_buf; returns its event pair"""
        self.x, self.x_alt = i_buf, o_buf
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        return a, b

    def _pp_round_trip(self, launch, u, v, reps, skip=0):
        """ms of u -> v plus v -> u (best of ``reps``, after ``skip`` repetitions that are not counted); leaves x = u, x_alt = v bound"""
        evs = [(self._pp_one(launch, u, v), self._pp_one(launch, v, u)) for _ in range(skip + reps)][skip:]
        torch.cuda.synchronize(self.device)
        self.x, self.x_alt = u, v
        return min(e[0][0].elapsed_time(e[0][1]) for e in evs) + min(e[1][0].elapsed_time(e[1][1]) for e in evs)

    def _pp_pairs(self, launch, cands, reps):
        """Every ordered pair of the candidates timed (best of ``reps``): (ms[i][j] of i -> j rounded, None on the diagonal; the best unordered
        pair [i, j]; its two directions in ms; those of the first pair)."""
        n = len(cands)
        ev = [[[] for _ in range(n)] for _ in range(n)]
        for r in range(reps):
            for i in range(n):
                for j in range(n):
                    if i != j:
                        ev[i][j].append(self._pp_one(launch, cands[i], cands[j]))
        torch.cuda.synchronize(self.device)
        t = [[(min(a.elapsed_time(b) for a, b in ev[i][j]) if i != j else float("inf")) for j in range(n)] for i in range(n)]
        _, bi, bj = min(((t[i][j] + t[j][i], i, j) for i in range(n) for j in range(i + 1, n)))
        return ([[None if i == j else round(t[i][j], 3) for j in range(n)] for i in range(n)], [bi, bj],
                [round(t[bi][bj], 3), round(t[bj][bi], 3)], [round(t[0][1], 3), round(t[1][0], 3)])

    def _pp_x0(self, launch, u, v, spare, reps):
        """x0 (read once per step): the caller's array against a copy in ``spare``, a buffer that is left; returns the two round trips in ms
        and keeps the copy only if it is strictly faster."""
        x0_orig = self.x0
        spare.copy_(x0_orig)
        t0 = self._pp_round_trip(launch, u, v, reps)
        self.x0 = spare
        t1 = self._pp_round_trip(launch, u, v, reps)
        if t0 <= t1:
            self.x0 = x0_orig
        return [round(t0, 3), round(t1, 3)]

    # ---- duality-gap certificate (tv_dual_gap; ChambollePock / ADMM: the solvers that carry a dual variable) ----------------------------------
    _GAP_DOC = """For P(x) = 1/2 |x - x0|^2 + reg |D x|_{2,1} and any dual variable q with |q|_2 <= reg per site,
        Dual(q) = <D^T q, x0> - 1/2 |D^T q|^2 <= P(x*) <= P(x), and by strong convexity 1/2 |x - x*|^2 <= P(x) - Dual(q): the gap bounds the
        distance to the minimiser, not the progress of the loop.  The kernel (tv_dual_gap) sums it site by site in its cancellation-free form
        1/2 (x - x0 + D^T q)^2 + (reg |D x|_2 - <q, D x>), both parts >= 0, and writes nothing but three scalars.
        fp32 FLOOR: the cancellation inside reg |D x|_2 - <q, D x> leaves an absolute error of order eps_fp32 * P, so relative gaps below
        about 1e-6 are not resolvable in fp32; the gap may then come out slightly negative (it is not clamped) and ``run_until`` ends on
        its iteration limit with ``converged=False``."""

    def _gap_certificate(self, x, q, qscale):
        """(primal, dual, gap) of the iterate x and the dual variable qscale * q as Python floats, global over all ranks: one exchange of the
        boundary planes of x and q (buffers of its own: the loop's halo planes, slots and lagged-fidelity block are not touched), one
        tv_dual_gap on this rank's planes, one all-reduce of the three scalars."""
        pl, s = self.plan, self.slab
        b = getattr(self, "_gap_buf", None)
        if b is None:
            b = self._gap_buf = dict(out=torch.zeros(3, dtype=torch.float64, device=self.device), **self._halo_set())
        s.wait(pl.exchange_image(x, b["xp"], b["xn"]))
        s.wait(pl.exchange_grad(q, _plane0(b["qp"]), _plane0(b["qn"])))
        out = b["out"]
        self._gap_kernel(x, q, qscale, b, out)
        s.allreduce_sum_(out)
        tv, fid, gap = (float(v) for v in out.cpu().tolist())
        primal = fid + self.reg * tv
        return primal, primal - gap, gap

    def _gap_kernel(self, x, q, qscale, b, out):
        """the reduce-only entry point of ``_gap_certificate``: tv_dual_gap; out[0] is the regulariser's sum (``HuberChambollePock``: the
        Huber sum, from tv_dual_gap_huber)"""
        _nv.check(self.lib.tv_dual_gap(self.geo.ref, _nv.ptr(x), _nv.ptr(b["xp"]), _nv.ptr(b["xn"]), _nv.ptr(q), _nv.ptr(b["qp"]), _nv.ptr(b["qn"]),
                                       _nv.ptr(self.x0), self.reg, float(qscale), out.data_ptr(), _nv.ptr(self.ws), self.stream))

    def _run_until_gap(self, rel_gap, max_n, check_every):
        """``run`` in blocks of ``check_every`` until gap <= rel_gap * max(|primal|, tiny) at a check or ``max_n`` iterations are done."""
        import numpy as np
        rel_gap, max_n, check_every = float(rel_gap), int(max_n), int(check_every)
        if check_every < 1 or max_n < 0:
            raise ValueError("run_until: check_every must be >= 1 and the iteration limit >= 0")
        tiny = float(np.finfo(np.float64).tiny)
        losses, done = [], 0
        while True:
            n = min(check_every, max_n - done)
            if n > 0:
                losses.append(np.asarray(self.run(n), dtype=np.float64))
                done += n
            primal, dual, gap = self.duality_gap()
            converged = gap <= rel_gap * max(abs(primal), tiny)
            if converged or done >= max_n:
                break
        info = dict(iterations=done, primal=primal, dual=dual, gap=gap, converged=bool(converged), error_bound=float(np.sqrt(2.0 * max(gap, 0.0))))
        return (np.concatenate(losses) if losses else np.zeros(0)), info

    def _run_until_residual(self, rel_res, max_iter, check_every):
        """``run`` in blocks of ``check_every`` until ``residuals()["total"]`` <= rel_res**2 * ``initial_residual()`` at a check or ``max_iter``
        iterations are done (the solvers without a duality gap: ``ChambollePockOperator``, ``RobustChambollePock``,
        ``PoissonChambollePock``, ``WeightedChambollePock``)."""
        import numpy as np
        rel_res, max_iter, check_every = float(rel_res), int(max_iter), int(check_every)
        if check_every < 1 or max_iter < 0:
            raise ValueError("run_until: check_every must be >= 1 and the iteration limit >= 0")
        r0 = self.initial_residual()
        losses, done = [], 0
        if r0 == 0.0:
            res, converged = self.residuals(), True
        else:
            while True:
                n = min(check_every, max_iter - done)
                if n > 0:
                    losses.append(np.asarray(self.run(n), dtype=np.float64))
                    done += n
                res = self.residuals()
                converged = res["total"] <= rel_res * rel_res * r0
                if converged or done >= max_iter:
                    break
        info = dict(iterations=done, converged=bool(converged), residuals=res, initial=r0,
                    relative=float(np.sqrt(res["total"] / r0)) if r0 > 0.0 else 0.0)
        return (np.concatenate(losses) if losses else np.zeros(0)), info

    def _reset_state(self):
        """Back to the state of a fresh solver in the arrays that are bound now."""
        self.x.copy_(self.x0)

    def _pp_tune(self, tune_placement, allowed, keep, tune):
        """Constructor side of the tuners.  tune_placement None = the automatic rule: images of >= 4 GiB with room for three more and 8 GiB to
        spare, where the solver allows it (``allowed``).  Sharded slabs too: the tuner launches local kernels only, no rank waits for another;
        every rank of a weak-scaling run holds a slab of the single-GPU size and plays the same placement lottery.
        The tuner is an optimisation, never a failure (out of memory while holding the candidates, ...): the bindings named in ``keep`` are
        put back and the state is re-initialised."""
        if tune_placement is None:
            img_bytes = self.x.numel() * self.x.element_size()
            free, _total = torch.cuda.mem_get_info(self.device)
            tune_placement = allowed and img_bytes >= (4 << 30) and free >= 3 * img_bytes + (8 << 30)
        if not tune_placement:
            return
        kept = [(k, getattr(self, k)) for k in keep]
        try:
            tune()
        except RuntimeError as exc:
            for k, v in kept:
                setattr(self, k, v)
            self._reset_state()
            torch.cuda.empty_cache()
            self.placement = {"error": str(exc)[:200]}


class _GapStopping:
    """``duality_gap`` / ``run_until`` of the solvers whose state (x, q) carries an exact duality gap (``ChambollePock``,
    ``AcceleratedChambollePock``, ``HuberChambollePock``, ``AdaptiveTVChambollePock``, ``VectorialTVChambollePock``), over ``_gap_certificate`` / ``_run_until_gap`` of
    ``_SlabProblem``.  A class binds the two under its own text with ``_redoc``: the ``_GAP_DOC`` of its model as the tail (a head of its
    own where it says more) and supplies ``_gap_kernel`` where its gap is not plain TV's."""

    def duality_gap(self):
        """(primal, dual, gap) of the current iterate and dual variable (x, q) as Python floats, between ``run`` / ``run_steps`` / ``step``
        calls; the state of the loop is not touched.  Sharded: collective, every rank calls it and gets the same numbers.
        """
        return self._gap_certificate(self.x, self.q, 1.0)

    def run_until(self, rel_gap, max_iter, check_every=10):
        """Iterate until the answer is certified: ``run`` in blocks of ``check_every`` iterations, stopping at the first check where
        gap <= rel_gap * max(|primal|, tiny), or after ``max_iter`` iterations.  Returns (loss_history, info); info: ``iterations``, ``primal``,
        ``dual``, ``gap``, ``converged`` and ``error_bound`` = sqrt(2 max(gap, 0)), the bound on |x - x*|_2.
        """
        return self._run_until_gap(rel_gap, max_iter, check_every)


# =================================================================================================
class ChambollePock(_GapStopping, _SlabProblem):
    """min_x 1/2 |x - x0|^2 + regularization * TV(x), README.md:141-157 with the state on the GPU.

    Per-step scalars: ``SLOTS`` fp64 device words, TV parts in [0:7], fidelity parts in [7:14] (one slot per
    launch; they are summed, over launches and over ranks, only when the loss is asked for).

    x0 : this rank's slab (device tensor).  ``step()`` enqueues one iteration; ``run(n)`` enqueues n
    and returns the loss history (one host synchronisation at the end)."""

    SLOTS = 14
    F = 7               # first fidelity slot

    @classmethod
    def loss_from_slots(cls, h, regularization):
        """README.md:157 loss from an (n, SLOTS) array of (already rank-summed) per-step scalars."""
        return h[:, cls.F:cls.SLOTS].sum(axis=1) + regularization * h[:, 0:cls.F].sum(axis=1)

    def __init__(self, x0, regularization, scheme="hybrid", reg_z_over_reg=1.0, reg_time=0.0, mask_static=False,
                 factor_reg_static=0, sigma_D=0.5, sigma_A=1.0, tau=None, slab=None, overlap=True, fused=None, pitch="auto",
                 q_pingpong=False, tune_placement=None, arena=None, persistent=None):
        """persistent (round 6): None = volumes of at most ``SMALL_MAX_VOXELS`` on one GPU run ``run`` / ``run_steps`` as ONE launch per
        ``SMALL_BLOCK`` iterations (tv_small_cp: the kernel pair's arithmetic inside a persistent kernel); False = never; True = required.
        fused: None = use the one-sweep kernel (tv_cp_fused + tv_cp_fixup: q read and written once per
        iteration) whenever the geometry supports it, False = always the dual + primal kernel pair.
        pitch: see ``_SlabProblem`` ("auto", the default: padded rows where that pays; None / "dense"; (row_pitch, frame_pitch)).
        q_pingpong (one-sweep path; default off): read the dual variable from one array and write it to a second one, swapping them
        every iteration, instead of updating it in place.  An arithmetic-free kernel with the sweep's memory shape gains 9 % from
        it (tools/archive/bwtest4, profiles/r4_bwtest4_q_pingpong.txt); the real sweep does not (tools/archive/pp_probe.py: 33.3 against 33.4 ms in
        one pool, and one of the two directions can be 3 ms slower than the other when the arrays are separate allocations) --
        kept as an option of tv_cp_sweep, not used by default.
        arena (round 5, default off): True = x, x_alt, p, a private copy of x0 and q are carved out of ONE allocation with 32 MiB
        between them (``_SlabProblem._arena_open``): the sweep then takes the same time in every construction (spread 0.5 % instead
        of 6 - 9 %) -- on whatever level that allocation landed, which is the slow one more often than not; see the comment there.
        tune_placement: None = on for volumes (slabs) of >= 4 GiB per image with memory to spare and no arena (see
        ``_tune_x_placement``)."""
        super().__init__(x0, scheme, reg_z_over_reg, reg_time, mask_static, factor_reg_static, slab, pitch=pitch)
        self.reg = float(regularization)
        self.sigma_D, self.sigma_A = float(sigma_D), float(sigma_A)
        self.tau = float(tau) if tau is not None else cp_step_size(self.slab.nz_global, x0.shape[1], reg_z_over_reg, reg_time,
                                                                    self.geo.time_weight_max)
        fused_given = fused is not None
        if fused is None and persistent is True:
            fused = False                                 # the persistent loop was asked for: it replaces the kernel pair, not the one-sweep kernel
        if fused is None:
            fused = self._one_sweep_default(sharded_ok=True)      # (this solver has the slab schedule of the one-sweep path)
        # (an explicit fused=False asks for the kernel pair: the persistent loop replaces it only when it is asked for as well)
        if bool(fused) and persistent is True:
            raise ValueError("fused=True and persistent=True are two different kernels: ask for one")
        self.small = (not bool(fused)) and self._small_ok(False if (fused_given and persistent is None) else persistent)
        self.fused = bool(fused)
        if self.fused and not self.lib.tv_cp_fused_supported(self.geo.ref):
            raise ValueError("the one-sweep Chambolle-Pock kernel does not support this geometry (tv_cp_fused_supported: "
                             "fp32, Nx % 4 == 0, Nx >= 64, Ny * Nx <= 2^30; any number of frames)")
        # the arrays of the iteration, in the order the arena was measured with: x, x_alt, p, x0 (the solver's own copy), q
        self._x0_src, self._q_pingpong, self._arena_want = self.x0, bool(q_pingpong), arena
        self.arena = False
        self._alloc_state()
        self._bind_loop_buffers()
        pl = self.plan
        sh = pl.on
        self.ch_back, self.ch_fwd = pl.ch_back, pl.ch_fwd
        self.overlap = bool(overlap) and sh and self.slab.nz >= 3 and not self.fused
        self.hist = None
        self.it = 0
        self.timing = None      # set to a list to collect (start, after kernel 1, after kernel 2) HIP events per step
        self.phase_timing = None  # set to a list to collect one (name, event) list per step: every phase boundary of the schedule
        self._scratch = torch.zeros(self.SLOTS, dtype=torch.float64, device=self.device)
        self._lag = None                 # None: every step returns its own fidelity; else: lagged-fidelity block (see run_steps)
        self._final = False              # the block's last iteration: its sweep returns BOTH fidelities (TV_CP_FID_BOTH), its fix-up reads x0
        self._lag_void = torch.zeros(1, dtype=torch.float64, device=self.device)
        self._both = torch.zeros((self.SLOTS, 2), dtype=torch.float64, device=self.device)     # [slot][input, output] of the final sweeps
        self._cur_out = self._scratch
        if self.fused:
            self.zchunk = int(self.lib.tv_cp_zchunk(self.geo.ref))
            self.nchunks = (self.slab.nz + self.zchunk - 1) // self.zchunk
            # interior-first scheduling of the one-sweep path needs an interior: >= 3 chunks and >= 3 planes
            self.overlap_fused = bool(overlap) and sh and self.nchunks >= 3 and self.slab.nz >= 3
        self.placement = None
        if self.fused and self.arena and tune_placement is None:
            # an arena of >= 4 GiB images with room for a second one: measure two, keep the faster (never on a sharded slab's behalf of others:
            # local sweeps only)
            img_bytes = self.x.numel() * self.x.element_size()
            free, _total = torch.cuda.mem_get_info(self.device)
            if img_bytes >= (4 << 30) and free >= self._arena.numel() * self._arena.element_size() + (8 << 30):
                self._tune_arena()
        if self.fused:
            # (q is NOT kept: the tuner keeps exactly one q bound at any time -- the best so far -- and at most one
            # candidate beside it, so that a winning candidate frees the original before the next one is allocated; round-4 advice)
            self._pp_tune(tune_placement, not self.arena, ("x", "x_alt", "p", "x0"), self._tune_x_placement)

    def _reset_state(self):
        """Back to the initial state: x = x0, p = q = q_alt = 0, no lagged-fidelity block open."""
        self._lag = None
        self.x.copy_(self.x0)
        self.p.zero_()
        self.q.zero_()
        if self.q_alt is not None:
            self.q_alt.zero_()

    def _alloc_state(self):
        """(Re)allocate x, x_alt, p, the private copy of x0, q [, q_alt] -- out of a fresh arena when one can be had -- and put them
        into the initial state (x = x0, p = q = 0)."""
        self._arena = None
        want = self._arena_want
        self.arena = self._arena_open(4 if self.fused else 3, 2 if (self.fused and self._q_pingpong) else 1, want) if (self.fused or want) else False
        self.x0 = self._x0_src
        self.x = self.image_copy(self.x0)
        self.x_alt = self.new_image() if self.fused else None      # ping-pong partner of x
        self.p = self.new_image()
        if self.arena:
            self.x0 = self.image_copy(self._x0_src)
        self.q = self.new_grad()
        self.q_alt = self.new_grad() if (self.fused and self._q_pingpong) else None
        if self.arena:
            self._arena_close()

    def _tune_arena(self, reps=2):
        """Two arenas, measured with the real sweep, the faster one kept (round 5).  WHERE one big allocation lands decides the level
        of every sweep that runs on it -- 31.0 or 32.1 ms on one box, 31.2 or 33.1 on others, the same for every construction that gets
        the same region and independent of the gap between the arrays (profiles/r5_slab_placement_probe{3,4}.txt) -- and two
        allocations made one after the other land in different regions.  Costs one more arena for a moment and ~8 sweeps; the state
        is re-initialised afterwards, results do not depend on it."""
        import time as _time
        t_begin = _time.perf_counter()
        out = torch.zeros(self.SLOTS, dtype=torch.float64, device=self.device)

        def round_trip():                        # the first of reps + 1 repetitions is the warm-up
            hp = self.x[0:1] if self.plan.x_need_prev else None
            hn = self.x[0:1] if self.plan.x_need_next else None
            return self._pp_round_trip(lambda: self._sweep(0, -1, hp, hn, out[0:1], out[self.F:self.F + 1]), self.x, self.x_alt, reps, skip=1)

        names = ("_arena", "_arena_off", "_arena_gap", "x", "x_alt", "p", "x0", "q", "q_alt")
        t0 = round_trip()
        first = {k: getattr(self, k) for k in names}
        info = {"round_trip_ms": [round(t0, 3)]}
        try:
            self._alloc_state()
            if not self.arena:
                raise RuntimeError("no second arena")
            t1 = round_trip()
            info["round_trip_ms"].append(round(t1, 3))
            if t0 <= t1:                         # keep the first: the second loses its last references here
                for k, v in first.items():
                    setattr(self, k, v)
        except RuntimeError as exc:              # out of memory for a second arena, ...: an optimisation, never a failure
            for k, v in first.items():
                setattr(self, k, v)
            self.arena = True
            info["error"] = str(exc)[:160]
        del first
        torch.cuda.empty_cache()
        self._reset_state()
        torch.cuda.synchronize(self.device)
        info["chosen"] = int(len(info["round_trip_ms"]) == 2 and info["round_trip_ms"][1] < info["round_trip_ms"][0])
        info["seconds"] = round(_time.perf_counter() - t_begin, 3)
        self.placement = {"arena": info}

    # ---- one phase on local planes [a, b) -----------------------------------------------------
    def _dual(self, a, b, xp, xn, out):
        g = self.geom(a, b)
        _nv.check(self.lib.tv_cp_dual(g.ref, _nv.ptr(self.x[a:b]), _nv.ptr(xp), _nv.ptr(xn), _nv.ptr(self.q[a:b]),
                                      self.sigma_D, self.reg, out.data_ptr(), _nv.ptr(self.ws), self.stream))

    def _primal(self, a, b, qp, qn, out):
        g = self.geom(a, b)
        _nv.check(self.lib.tv_cp_primal(g.ref, _nv.ptr(self.q[a:b]), _nv.ptr(qp), _nv.ptr(qn), _nv.ptr(self.x[a:b]),
                                        _nv.ptr(self.x0[a:b]), _nv.ptr(self.p[a:b]), self.tau, self.sigma_A,
                                        out.data_ptr(), _nv.ptr(self.ws), self.stream))

    def _tune_x_placement(self, n_extra=2, reps=2):
        """Pick WHERE the arrays of the iteration live by MEASUREMENT: the dual variable q (one alternative allocation, when the
        memory is there), the two image buffers the iterate ping-pongs between (``n_extra`` more candidates, every ordered pair
        timed), and the fidelity dual p (the candidates that are left).

        Why: on MI355X the time of the one-sweep kernel depends on where its arrays landed in
        physical memory -- the same binary on the same data runs the north-star sweep in 31.2 or in 34 ms, the level is fixed for
        the life of an allocation, and it differs between the two directions of the x ping-pong (sweeps alternate 34.5 / 32.5 ms):
        the memory side answers the reads of one placement ~4 % later than those of another (TCC_EA0_RDREQ_LEVEL / TCC_EA0_RDREQ,
        evenly over all 128 L2 channels: profiles/r4_channel_counters.txt; the rate of a plain copy depends on the distance
        between source and destination in the same way: profiles/r4_deltatest.txt).  Nothing a process can ask the allocator for
        controls it (page size, alignment, one pool or many, a pitch: profiles/r4_vmtest.txt, r4_bwtest4_frame_pitch.txt,
        r3_placement_experiments.txt), but it can be MEASURED.  Costs ~40 sweeps once per solver (~1.3 s for the north star:
        same-box A/B 33.8 / 34.3 / 34.8 ms per iteration with it, 35.2 / 35.4 / 35.2 without, profiles/r4_placement_tuner_ab.txt);
        the state is re-initialised afterwards, results do not depend on it."""
        import time as _time
        t_begin = _time.perf_counter()
        out = torch.zeros(self.SLOTS, dtype=torch.float64, device=self.device)
        hp = self.x[0:1] if self.plan.x_need_prev else None           # timing only: any plane of the right layout serves as a halo
        hn = self.x[0:1] if self.plan.x_need_next else None
        info = {}

        def launch():
            self._sweep(0, -1, hp, hn, out[0:1], out[self.F:self.F + 1])

        def round_trip(u, v):
            return self._pp_round_trip(launch, u, v, reps)

        x_a, x_b = self.x, self.x_alt
        for _ in range(2):                                                   # warm-up (code load, clocks)
            self._pp_one(launch, x_a, x_b)
        # ---- the dual variable: one alternative allocation, if it fits with room to spare ---------------------------------------
        q_bytes = self.q.numel() * self.q.element_size()
        img_bytes = x_a.numel() * x_a.element_size()
        free, _total = torch.cuda.mem_get_info(self.device)
        if self.q_alt is None and free >= q_bytes + (n_extra + 1) * img_bytes + (8 << 30):
            # up to two alternatives, one at a time (never more than two q arrays alive): a slow q allocation costs up to 2 ms per
            # sweep (profiles/r4_bench_northstar_first_command_e.json: round trips 67.3 vs 63.5 ms)
            best_q, best_t = self.q, round_trip(x_a, x_b)
            info["q_round_trip_ms"] = [round(best_t, 3)]
            try:
                for _ in range(2):
                    cand = self.new_grad()
                    self.q = cand
                    t2 = round_trip(x_a, x_b)
                    info["q_round_trip_ms"].append(round(t2, 3))
                    if t2 < best_t:
                        best_q, best_t = cand, t2
                    self.q = best_q                  # the loser (the original included) loses its last reference here
                    del cand
                    torch.cuda.empty_cache()
            except RuntimeError as exc:              # no room for another candidate: keep the best q measured so far, go on with the images
                self.q = best_q
                torch.cuda.empty_cache()
                info["q_error"] = str(exc)[:160]
            del best_q
        # ---- the image pair: every ordered pair of the candidates ------------------------------------------------------------------
        cands = [x_a, x_b] + [self.new_image() for _ in range(n_extra)]
        ms, (bi, bj), chosen_ms, first_ms = self._pp_pairs(launch, cands, reps)
        info.update({"candidates": len(cands), "sweep_ms": ms, "chosen": [bi, bj], "chosen_ms": chosen_ms, "first_pair_ms": first_ms})
        x_a, x_b = cands[bi], cands[bj]
        # ---- the fidelity dual p: the candidates that are left, against the allocation it has ------------------------------------------
        rest = [c for k, c in enumerate(cands) if k not in (bi, bj)]
        del cands
        p_cands = [self.p] + rest
        tp = []
        for c in p_cands:
            self.p = c
            tp.append(round_trip(x_a, x_b))
        kp = min(range(len(tp)), key=lambda k: tp[k])
        self.p = p_cands[kp]
        info["p_round_trip_ms"] = [round(v, 3) for v in tp]
        info["p_chosen"] = kp
        # ---- x0 (read once per sweep): the caller's array against a copy in one of the buffers that are left ------------------------
        spare = [c for k, c in enumerate(p_cands) if k != kp]
        del p_cands, rest
        if spare:
            info["x0_round_trip_ms"] = self._pp_x0(launch, x_a, x_b, spare[0], reps)
        del spare
        self.x, self.x_alt = x_a, x_b
        self._reset_state()                          # the timed sweeps wrote into x, p and q
        torch.cuda.synchronize(self.device)
        torch.cuda.empty_cache()
        info["seconds"] = round(_time.perf_counter() - t_begin, 3)
        self.placement = info

    def _sweep(self, c0, cn, xp, xn, tv_slot, fid_slot):
        """One sweep launch.  In a lagged-fidelity block (``_lag``, see ``_run_eager``) the sweep returns 1/2 |x_in - x0|^2 over all
        sites -- the fidelity of the iterate the PREVIOUS step produced -- into the previous step's slot, and the fix-up reads no x0."""
        g = self.geo
        flags = 0
        own_slot, both = fid_slot, None
        if self._lag is not None:
            flags = 1                                    # TV_CP_FID_OF_INPUT
            i = fid_slot.storage_offset() - self._cur_out.storage_offset()
            if self._lag is False:
                fid_slot = self._lag_void                # first sweep of a block: nobody waits for its input's fidelity
            else:                                        # the same slot index, one row back
                fid_slot = self._lag[i:i + 1]
            if self._final:
                # last iteration of the block (round 5): the sweep returns the fidelity of its input AND of its output (complete sites), the
                # fix-up -- called with x0 -- the rest: no reduction pass over x and x0 closes the block any more
                flags = 3                                # TV_CP_FID_OF_INPUT | TV_CP_FID_BOTH
                both, prev_slot = self._both[i], fid_slot
                fid_slot = both
        _nv.check(self.lib.tv_cp_sweep(g.ref, _nv.ptr(self.x), _nv.ptr(xp), _nv.ptr(xn), _nv.ptr(self.q),
                                       _nv.ptr(self.q_alt if self.q_alt is not None else self.q), _nv.ptr(self.x0),
                                       _nv.ptr(self.p), _nv.ptr(self.x_alt), self.sigma_D, self.reg, self.tau, self.sigma_A, flags,
                                       c0, cn, tv_slot.data_ptr(), fid_slot.data_ptr(), _nv.ptr(self.ws), self.stream))
        if both is not None:
            prev_slot.copy_(both[0:1])
            own_slot.copy_(both[1:2])

    def _fixup(self, z0, zn, qp, qn, fid_slot):
        g = self.geo
        lag = self._lag is not None and not self._final
        _nv.check(self.lib.tv_cp_fixup(g.ref, _nv.ptr(self.q_alt if self.q_alt is not None else self.q), _nv.ptr(qp), _nv.ptr(qn), _nv.ptr(self.x_alt),
                                       None if lag else _nv.ptr(self.x0), self.tau, z0, zn,
                                       (self._lag_void if lag else fid_slot).data_ptr(), _nv.ptr(self.ws), self.stream))

    def _step_fused(self, out):
        """One-sweep iteration: x halos -> sweep (x -> x_alt) -> q' halos -> fix-up -> swap.  With a sharded
        slab the interior chunks / planes run while the halo planes are in flight: the first half of the interior chunks
        hides the x exchange, then the two edge chunks run, and the SECOND half of the interior chunks (with the interior
        fix-up behind it) hides the q' exchange -- the interior fix-up alone is too short for that on a 32-plane slab.
        ``phase_timing`` (a list): one event per phase boundary on the launch stream, so that a scaling run can say where an
        iteration's time went -- in particular how long the stream sat in ``s.wait(h)`` with nothing left to overlap."""
        s, nz, F = self.slab, self.slab.nz, self.F
        self._cur_out = out
        ev = self._events()
        mark = self._phase_marker()
        qhp, qhn = _plane0(self.qh_prev), _plane0(self.qh_next)
        mark("start")
        h = self.plan.exchange_image(self.x, self.xh_prev, self.xh_next)
        if ev:
            ev[0].record()
        if self.overlap_fused:
            nch = self.nchunks
            na = (nch - 2 + 1) // 2                      # interior chunks before the edge chunks, nb after them
            nb = nch - 2 - na
            self._sweep(1, na, None, None, out[0:1], out[F:F + 1])
            mark("sweep_interior_a")
            s.wait(h)
            mark("x_halo_wait_exposed")
            self._sweep(0, 1, self.xh_prev, None, out[1:2], out[F + 1:F + 2])
            self._sweep(nch - 1, 1, None, self.xh_next, out[2:3], out[F + 2:F + 3])
            mark("sweep_edges")
            h = self.plan.exchange_grad(self.q_alt if self.q_alt is not None else self.q, qhp, qhn)
            if nb > 0:
                self._sweep(1 + na, nb, None, None, out[3:4], out[F + 3:F + 4])
            mark("sweep_interior_b")
            if ev:
                ev[1].record()
        else:
            s.wait(h)
            mark("x_halo_wait_exposed")
            self._sweep(0, -1, self.xh_prev, self.xh_next, out[0:1], out[F:F + 1])
            mark("sweep")
            if ev:
                ev[1].record()
            h = self.plan.exchange_grad(self.q_alt if self.q_alt is not None else self.q, qhp, qhn)
        if self.overlap_fused:
            self._fixup(1, nz - 2, None, None, out[F + 4:F + 5])
            mark("fixup_interior")
            s.wait(h)
            mark("q_halo_wait_exposed")
            self._fixup(0, 1, self.qh_prev, None, out[F + 5:F + 6])
            self._fixup(nz - 1, 1, None, self.qh_next, out[F + 6:F + 7])
            mark("fixup_edges")
        else:
            s.wait(h)
            mark("q_halo_wait_exposed")
            self._fixup(0, -1, self.qh_prev, self.qh_next, out[F + 4:F + 5])
            mark("fixup")
        if ev:
            ev[2].record()
        self.x, self.x_alt = self.x_alt, self.x
        if self.q_alt is not None:
            self.q, self.q_alt = self.q_alt, self.q          # self.q is always the current dual variable
        self.it += 1
        if self._lag is not None:
            self._lag = out                      # the next sweep delivers THIS step's fidelity into these slots

    def _phase_marker(self):
        """mark(name): record an event on the launch stream that closes phase `name` (no-op unless ``phase_timing`` is a list)"""
        if self.phase_timing is None:
            return lambda name: None
        rec = []
        self.phase_timing.append(rec)

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            rec.append((name, e))
        return mark

    @staticmethod
    def phase_means_ms(phase_timing):
        """{phase: mean milliseconds per step} from the event lists collected in ``phase_timing`` (synchronise first)"""
        acc, order = {}, []
        for rec in phase_timing:
            for (_, a), (name, b) in zip(rec[:-1], rec[1:]):
                if name not in acc:
                    acc[name] = []
                    order.append(name)
                acc[name].append(a.elapsed_time(b))
        return {k: float(sum(acc[k]) / len(acc[k])) for k in order}

    def _events(self):
        if self.timing is None:
            return None
        ev = tuple(torch.cuda.Event(enable_timing=True) for _ in range(3))
        self.timing.append(ev)
        return ev

    def step(self, out=None):
        """Enqueue one iteration.  out: fp64 device tensor of SLOTS words receiving this rank's TV parts
        [0:7] and fidelity parts [7:14] (summed later); defaults to an internal scratch."""
        out = self._scratch if out is None else out
        if self.fused:
            return self._step_fused(out)
        nz, s, F = self.slab.nz, self.slab, self.F
        x, q = self.x, self.q
        ev = self._events()
        mark = self._phase_marker()
        mark("start")
        # ---------------- dual: q <- proj(q + sigma D x) -----------------------------------------
        h = self.plan.exchange_image(x, self.xh_prev, self.xh_next)
        if ev:
            ev[0].record()
        if self.overlap:
            self._dual(1, nz - 1, x[0:1], x[nz - 1:nz], out[0:1])
            mark("dual_interior")
            s.wait(h)
            mark("x_halo_wait_exposed")
            self._dual(0, 1, self.xh_prev, x[1:2], out[1:2])
            self._dual(nz - 1, nz, x[nz - 2:nz - 1], self.xh_next, out[2:3])
            mark("dual_edges")
        else:
            s.wait(h)
            mark("x_halo_wait_exposed")
            self._dual(0, nz, self.xh_prev, self.xh_next, out[0:1])
            mark("dual")
        if ev:
            ev[1].record()
        # ---------------- primal: x <- x - tau p - tau D^T q ---------------------------------------
        h = self.plan.exchange_grad(q, _plane0(self.qh_prev), _plane0(self.qh_next))
        if self.overlap:
            self._primal(1, nz - 1, q[0, self.ch_back], q[nz - 1, self.ch_fwd], out[F:F + 1])
            mark("primal_interior")
            s.wait(h)
            mark("q_halo_wait_exposed")
            self._primal(0, 1, self.qh_prev, q[1, self.ch_fwd], out[F + 1:F + 2])
            self._primal(nz - 1, nz, q[nz - 2, self.ch_back], self.qh_next, out[F + 2:F + 3])
            mark("primal_edges")
        else:
            s.wait(h)
            mark("q_halo_wait_exposed")
            self._primal(0, nz, self.qh_prev, self.qh_next, out[F:F + 1])
            mark("primal")
        if ev:
            ev[2].record()
        self.it += 1

    GRAPH_BLOCK = 10            # iterations captured per hipGraph (even: the x ping-pong returns to its start)
    GRAPH_MAX_VOXELS = 1 << 23  # below this an iteration is launch-bound (tens of microseconds of kernels)

    def run(self, n_iter, record_loss=True, graph=None):
        """n_iter iterations; returns the README's loss history (README.md:157) as a numpy array
        (global over all ranks), or None.  graph: None = capture the loop in a hipGraph when the problem is
        small enough to be launch-bound and not sharded; True / False force it."""
        hist = torch.zeros((n_iter, self.SLOTS), dtype=torch.float64, device=self.device)
        use_graph = (self.x0.numel() <= self.GRAPH_MAX_VOXELS and not self.slab.sharded and self.timing is None and self.phase_timing is None) if graph is None else bool(graph)
        small = self._small_now()
        if small and graph is None:
            use_graph = False                     # the persistent kernel IS the loop: nothing left to capture
        start = self._run_graphed_head(hist, use_graph)
        self.run_steps(hist[start:n_iter])
        if small:
            self._small_check()
        if not record_loss:
            return None
        self.slab.allreduce_sum_(hist)
        return self.loss_from_slots(hist.cpu().numpy(), self.reg)

    def run_steps(self, rows):
        """Enqueue ``len(rows)`` iterations, row k of the (n, SLOTS) fp64 device tensor ``rows`` receiving the scalars of iteration k.
        One-sweep path (round 4): the fidelity 1/2 |x_{k+1} - x0|^2 of row k is delivered by the sweep of iteration k+1 (it has
        x_{k+1} and x0 in registers: tv_cp_sweep, TV_CP_FID_OF_INPUT), so the fix-up reads no x0; the LAST iteration's sweep returns the
        fidelity of its output as well (TV_CP_FID_BOTH, round 5: over the complete sites; its fix-up, called with x0, adds the rest).
        The rows must be zero on entry (slots are written once each)."""
        n = rows.shape[0]
        if n == 0:
            return
        if self._small_now():
            return self._run_small(rows)
        if not self.fused:
            for k in range(n):
                self.step(rows[k])
            return
        self._lag = False                # first sweep of the block: its input's fidelity belongs to nobody
        try:
            for k in range(n):
                self._final = (k == n - 1)       # the last sweep returns both fidelities (round 4: one more pass over x and x0 closed the block)
                self.step(rows[k])
        finally:
            self._lag = None
            self._final = False

    def _small_now(self):
        """the persistent path runs the loop unless somebody asked for per-step events (bench.py: ``timing`` / ``phase_timing``)"""
        return self.small and self.timing is None and self.phase_timing is None

    def _run_small(self, rows):
        """``len(rows)`` iterations in blocks of ``SMALL_BLOCK`` per cooperative launch (tv_small_cp): x, p, q updated in place; TV of the
        iterate each dual update saw -> slot 0, 1/2 |x_new - x0|^2 -> slot F (the slots the kernel pair fills)."""
        ws = self._small_ws()

        def launch(k, row_ptr):
            # the reduction that closes the launch writes TV -> slot 0 and the fidelity -> slot F of the rows themselves
            _nv.check(self.lib.tv_small_cp(self.geo.ref, _nv.ptr(self.x), _nv.ptr(self.x0), _nv.ptr(self.p), _nv.ptr(self.q), self.sigma_D, self.reg,
                                           self.tau, self.sigma_A, k, row_ptr, rows.stride(0), self.F, _nv.ptr(ws), self.stream))
            self.it += k

        self._small_blocks(rows, launch)

    duality_gap = _redoc(_GapStopping.duality_gap, """(primal, dual, gap) of the current iterate and dual variable (x, q) as Python floats -- on every path (kernel pair, one-sweep,
        persistent), between ``run`` / ``run_steps`` calls; the state of the loop is not touched.  Sharded: collective, every rank calls it
        and gets the same numbers.
        """, _SlabProblem._GAP_DOC)
    run_until = _redoc(_GapStopping.run_until, tail=_SlabProblem._GAP_DOC)

    _ROLES = ("it", "x", "x_alt", "q", "q_alt")

    def _run_graphed_from(self, hist, first, n_iter):
        done = super()._run_graphed_from(hist, first, n_iter)
        self.it += done                  # (the capture left the counter where it was)
        return done


# =================================================================================================
class _ExtrapolatedCP(_SlabProblem):
    """What the Chambolle-Pock solvers with the state (x, x_bar, q) share (``AcceleratedChambollePock``, ``HuberChambollePock``,
    ``AdaptiveTVChambollePock``, ``RobustChambollePock``, ``PoissonChambollePock``, ``WeightedChambollePock``): the state and its halo
    planes, the iteration -- ``step``: a dual kernel on the extrapolated point x_bar, then a primal kernel that extrapolates -- and the
    loop around it.  A subclass validates its steps (``cp_step_pair`` / ``cp_linear_steps`` on ``L2``), calls ``_alloc_state`` and says
    what differs through three hooks:

        _steps(k)                           (tau, sigma, theta) of iteration k as Python floats.  Here: the constants ``self.tau``,
                                            ``self.sigma``, ``self.theta`` (Algorithm 1: theta = 1; Algorithm 3: ``cp_linear_steps``);
                                            ``AcceleratedChambollePock``: the schedule of Algorithm 2
        _dual_kernel(sigma, out_ptr)        here tv_cp_dual (plain TV); tv_cp_dual_huber, tv_cp_dual_wtv, tv_cp_dual_vtv
        _primal_kernel(tau, theta, out_ptr) here tv_cp_primal_accel (quadratic fidelity); ``_FixedPointResiduals``: the class's ``_prox``

    and keeps ``step`` / ``run`` under docstrings of its own (what its scalars mean).  The one-sweep form of the iteration is
    ``_OneSweepCP``.  Per-step scalars: the slots of ``ChambollePock``."""

    SLOTS, F = ChambollePock.SLOTS, ChambollePock.F
    loss_from_slots = ChambollePock.loss_from_slots
    _fused = False          # the kernel pair; ``_OneSweepCP`` makes it a choice

    def __init__(self, x0, regularization, scheme, reg_z_over_reg, reg_time, mask_static, factor_reg_static, slab, pitch):
        super().__init__(x0, scheme, reg_z_over_reg, reg_time, mask_static, factor_reg_static, slab, pitch=pitch)
        self.reg = float(regularization)
        self.L2 = normal_spectral_bound(scheme, self.slab.nz_global, x0.shape[1], reg_z_over_reg, reg_time, self.geo.time_weight_max)

    def _alloc_state(self):
        """x = x_bar = x0, q = 0, the loop's buffers, iteration 0.  (The order of the allocations is kept as it was measured: where
        separate allocations land moves the streaming kernels' time, see the arena comment in ``_SlabProblem``.)"""
        self.x = self.image_copy(self.x0)
        self.x_bar = self.image_copy(self.x0)
        self.q = self.new_grad()
        self._bind_loop_buffers()
        self.it = 0
        self._scratch = torch.zeros(self.SLOTS, dtype=torch.float64, device=self.device)

    def reset(self):
        """Back to the state of a fresh solver: x = x_bar = x0, q = 0, iteration 0 (where the steps follow a schedule, it starts again).
        Choices made after construction (``AcceleratedChambollePock.set_fused``) stay."""
        self.x.copy_(self.x0)
        self.x_bar.copy_(self.x0)
        self.q.zero_()
        self.it = 0

    def step(self, out=None):
        """Enqueue one iteration with the steps of iteration ``self.it``.  out: fp64 device tensor of SLOTS words (zero on entry) receiving
        this rank's regulariser of x_bar in slot 0 and its fidelity of x_new in slot F; defaults to an internal scratch."""
        out = self._scratch if out is None else out
        tau, sigma, theta = self._steps(self.it)
        if self._fused:
            self._one_sweep(tau, sigma, theta, out)
        else:
            F = self.F
            self._dual_half(sigma, out)
            self._primal_kernel(tau, theta, out[F:F + 1].data_ptr())
        self.it += 1

    def _steps(self, k):
        """(tau_k, sigma_k, theta_k) as Python floats: constant steps"""
        return self.tau, self.sigma, self.theta

    def _dual_half(self, sigma, out):
        """q <- proj_{|.|_2 <= reg}(q + sigma D x_bar), this rank's |D x_bar|_{2,1} into out[0]; sharded: the boundary planes of x_bar travel
        before the kernel and those of the new q after it (into ``qh_prev`` / ``qh_next``, for the primal kernel), both waits exposed."""
        s, pl = self.slab, self.plan
        if pl.on:           # (no plane travels otherwise: at launch-bound sizes the two empty exchanges are host time worth skipping)
            s.wait(pl.exchange_image(self.x_bar, self.xh_prev, self.xh_next))
        self._dual_kernel(sigma, out[0:1].data_ptr())
        if pl.on:
            s.wait(pl.exchange_grad(self.q, _plane0(self.qh_prev), _plane0(self.qh_next)))

    def _dual_kernel(self, sigma, out_ptr):
        """the dual entry point of ``_dual_half``: tv_cp_dual (plain TV); ``HuberChambollePock`` and ``AdaptiveTVChambollePock`` have their own"""
        _nv.check(self.lib.tv_cp_dual(self.geo.ref, _nv.ptr(self.x_bar), _nv.ptr(self.xh_prev), _nv.ptr(self.xh_next), _nv.ptr(self.q),
                                      sigma, self.reg, out_ptr, _nv.ptr(self.ws), self.stream))

    def _primal_kernel(self, tau, theta, out_ptr):
        """the primal entry point of ``step``: tv_cp_primal_accel (D^T, the closed-form prox of the quadratic fidelity, extrapolation by theta)"""
        _nv.check(self.lib.tv_cp_primal_accel(self.geo.ref, _nv.ptr(self.q), _nv.ptr(self.qh_prev), _nv.ptr(self.qh_next), _nv.ptr(self.x),
                                              _nv.ptr(self.x_bar), _nv.ptr(self.x0), tau, theta, out_ptr, _nv.ptr(self.ws), self.stream))

    def run_steps(self, rows):
        """Enqueue ``len(rows)`` iterations, row k of the (n, SLOTS) fp64 device tensor ``rows`` (zero on entry) receiving the scalars of
        iteration k."""
        for k in range(rows.shape[0]):
            self.step(rows[k])

    def _run(self, n_iter, record_loss):
        """``run`` of the subclasses (each documents what its loss history means)"""
        hist = torch.zeros((int(n_iter), self.SLOTS), dtype=torch.float64, device=self.device)
        self.run_steps(hist)
        if not record_loss:
            return None
        self.slab.allreduce_sum_(hist)
        return self.loss_from_slots(hist.cpu().numpy(), self.reg)


class _OneSweepCP(_ExtrapolatedCP):
    """The one-sweep path of an ``_ExtrapolatedCP`` solver with the quadratic fidelity (``AcceleratedChambollePock``, ``HuberChambollePock``):
    a sweep kernel -- x_bar is its stencil input and is ping-ponged with a second buffer, x and q are updated in place -- followed by
    tv_cp_accel_fixup.  The state (x, x_bar, q) is that of the kernel pair.  A class supplies ``_sweep_kernel(tau, sigma, theta, tv_ptr,
    fid_ptr, g, ws, st)`` (one launch over all chunks, x_bar -> x_bar_alt; g, ws, st: the geometry reference, workspace pointer and stream
    that the two launches of an iteration share), ends its constructor with ``_init_path()`` and binds ``fused`` / ``step`` under its
    own text."""

    def _init_path(self):
        """the end of construction: no partner of x_bar yet, the default path"""
        self.x_bar_alt = None            # ping-pong partner of x_bar on the one-sweep path, allocated on first use
        self.set_fused(None)

    @property
    def fused(self):
        """True: iterations run as the sweep kernel + tv_cp_accel_fixup; False: as the kernel pair (``set_fused``)"""
        return self._fused

    def set_fused(self, fused):
        """Choose the path of the iterations that follow.  True = the one-sweep kernel (ValueError where tv_cp_fused_supported refuses the
        geometry, and on a sharded slab: the sweep / exchange / fix-up schedule of slabs is not built for this solver), False = the kernel
        pair, None = the construction default (class docstring).  The state is untouched; ``reset()`` keeps the choice."""
        if fused is None:
            fused = self._one_sweep_default(sharded_ok=False)        # ``ChambollePock``'s rule, unsharded volumes only
        elif fused:
            if not self.lib.tv_cp_fused_supported(self.geo.ref):
                raise ValueError("the one-sweep kernel does not support this geometry (tv_cp_fused_supported: whole 16-byte lanes or pitched "
                                 "rows, Nx >= 64, frames below 2^31 bytes)")
            if self.slab.sharded:
                raise ValueError("set_fused(True): the one-sweep path of %s takes unsharded volumes only" % type(self).__name__)
        self._fused = bool(fused)

    def _one_sweep(self, tau, sigma, theta, out):
        """the iteration as one sweep over all chunks (x_bar -> x_bar_alt, x and q in place) and one fix-up over all planes; both return a
        part of the fidelity (slots F, F + 1)"""
        if self.x_bar_alt is None:
            # (lazy, and so AFTER the state arrays: where separate allocations land moves the streaming kernels' time, ``_alloc_state``)
            self.x_bar_alt = self.new_image()
        F = self.F
        # (fetched once for both launches: fetching them again for the fix-up measured 1 - 2 us on a 30 us launch-bound iteration)
        g, ws, st = self.geo.ref, _nv.ptr(self.ws), self.stream
        self._sweep_kernel(tau, sigma, theta, out[0:1].data_ptr(), out[F:F + 1].data_ptr(), g, ws, st)
        _nv.check(self.lib.tv_cp_accel_fixup(g, _nv.ptr(self.q), None, None, _nv.ptr(self.x), _nv.ptr(self.x_bar_alt), _nv.ptr(self.x0),
                                             tau, theta, 0, -1, out[F + 1:F + 2].data_ptr(), ws, st))
        self.x_bar, self.x_bar_alt = self.x_bar_alt, self.x_bar


# =================================================================================================
class AcceleratedChambollePock(_GapStopping, _OneSweepCP):
    """min_x 1/2 |x - x0|^2 + regularization * TV(x) with the ACCELERATED primal-dual iteration (Chambolle & Pock 2011, Algorithm 2).
    The fidelity is 1-strongly convex: with theta_k = 1 / sqrt(1 + 2 gamma tau_k), tau_{k+1} = theta_k tau_k, sigma_{k+1} = sigma_k / theta_k
    (``accel_schedule``; gamma <= 1) the iterates converge as O(1/k^2) where ``ChambollePock`` -- the reference's README loop, fixed steps,
    no extrapolation -- converges as O(1/k).  State: x, x_bar (images), q (gradient); x = x_bar = x0, q = 0 at the start.  Iteration k:

        q     <- proj_{|.|_2 <= reg}(q + sigma_k D x_bar)                           tv_cp_dual on x_bar          (2 Nd + 1 words per voxel)
        x_new <- (x - tau_k D^T q + tau_k x0) / (1 + tau_k)
        x_bar <- x_new + theta_k (x_new - x);  x <- x_new                           tv_cp_primal_accel, one pass (Nd + 4)

    That kernel pair moves 3 Nd + 5 words per voxel.  The ONE-SWEEP path (``set_fused``, ``fused``) runs the same iteration as
    tv_cp_accel_sweep + tv_cp_accel_fixup -- ``ChambollePock``'s one-sweep kernel with another epilogue: x_bar is the stencil input and is
    ping-ponged with a second buffer, x is updated in place, q is read and written once: 2 Nd + 5 words.  The state (x, x_bar, q) is the same
    on both paths, so ``set_fused`` may be called between iterations at any time.  DEFAULT: ``ChambollePock``'s rule -- the sweep where
    tv_cp_fused_supported accepts the geometry, the volume is not sharded and holds at least 1024 * TV_FUSED_MIN_KVOXELS (16 Mi) voxels, the
    pair otherwise.  Measured on 64x8x1024x1024 fp32 (profiles/cp_accel_sweep_bench.txt): the sweep path takes 0.65 -
    0.81 of the pair's time per iteration in all four schemes and 1.00 - 1.05 of ``ChambollePock``'s one-sweep iteration.

    The scalars of iteration k are host doubles passed to the launches.  Not built: hipGraph capture, a device-resident step table, the
    placement tuner / arena of ``ChambollePock``, a persistent small-volume form, and the sweep / exchange / fix-up schedule of a sharded slab
    (slabs run the kernel pair) -- at the reference's small shapes the solver pays a launch per kernel against the persistent loop of
    ``ChambollePock``.  The Huber-TV regulariser (quadratic below a gradient magnitude alpha, against staircasing;
    linearly convergent) is ``HuberChambollePock``; a per-voxel weight on the TV term (spatially adaptive TV, this schedule) is
    ``AdaptiveTVChambollePock``; one norm per spatial site over all frames (channel-coupled TV, this schedule) is
    ``VectorialTVChambollePock``.

    gamma = 0 gives theta = 1 and constant steps (Algorithm 1 with extrapolation).  The step schedule continues across ``run`` /
    ``run_steps`` / ``step`` calls (``self.it`` counts the iterations done); ``reset()`` starts it again.
    Sharded (``slab``): the boundary plane(s) of x_bar travel before the dual kernel and those of q before the primal kernel, both waits
    exposed (no interior / edge overlap).

    Per-step scalars: the slots of ``ChambollePock`` -- TV in slot 0, fidelity in slot ``F`` (one-sweep path: the sweep's part in slot ``F``,
    the fix-up's in ``F + 1``; they are summed when the loss is asked for)."""

    def __init__(self, x0, regularization, scheme="hybrid", reg_z_over_reg=1.0, reg_time=0.0, mask_static=False,
                 factor_reg_static=0, tau0=None, sigma0=None, gamma=1.0, slab=None, pitch="auto"):
        """tau0, sigma0: the steps of iteration 0; they must satisfy tau0 sigma0 L^2 <= 1 with L^2 = ``normal_spectral_bound`` of the geometry
        (the time axis weighted by the largest per-pixel weight, as in ``cp_step_size``), else ValueError.  Default: both 1 / sqrt(L^2); one
        given: the other is 1 / (L^2 times it).  gamma: the strong-convexity constant the schedule uses, 1.0 = that of the fidelity term
        (0 <= gamma <= 1 keeps the O(1/k^2) proof; 0 = constant steps).  pitch: see ``_SlabProblem``."""
        super().__init__(x0, regularization, scheme, reg_z_over_reg, reg_time, mask_static, factor_reg_static, slab, pitch)
        self.gamma = float(gamma)
        if not (self.gamma >= 0.0 and math.isfinite(self.gamma)):
            raise ValueError("tau0 and sigma0 must be finite and > 0, gamma finite and >= 0")
        self.tau0, self.sigma0 = cp_step_pair(self.L2, tau0, sigma0, names=("tau0", "sigma0"))
        self._alloc_state()
        self._sched = None
        self._init_path()

    fused = property(_OneSweepCP.fused.fget, doc="True: iterations run as tv_cp_accel_sweep + tv_cp_accel_fixup; False: as tv_cp_dual + "
                                                 "tv_cp_primal_accel (``set_fused``)")

    def _steps(self, k):
        """(tau_k, sigma_k, theta_k) as Python floats, from a cached ``accel_schedule`` that grows by doubling"""
        key = (self.tau0, self.sigma0, self.gamma)
        if self._sched is None or self._sched[0] != key or k >= len(self._sched[1][0]):
            self._sched = (key, accel_schedule(*key, max(256, 2 * (k + 1))))
        tau, sigma, theta = self._sched[1]
        return float(tau[k]), float(sigma[k]), float(theta[k])

    def _sweep_kernel(self, tau, sigma, theta, tv_ptr, fid_ptr, g, ws, st):
        _nv.check(self.lib.tv_cp_accel_sweep(g, _nv.ptr(self.x_bar), None, None, _nv.ptr(self.q), _nv.ptr(self.q), _nv.ptr(self.x0),
                                             _nv.ptr(self.x), _nv.ptr(self.x_bar_alt), sigma, self.reg, tau, theta, 0, 0, -1, tv_ptr, fid_ptr,
                                             ws, st))

    step = _redoc(_ExtrapolatedCP.step, """Enqueue one iteration with the steps of iteration ``self.it``.  out: fp64 device tensor of SLOTS words (zero on entry) receiving this
        rank's |D x_bar|_{2,1} in slot 0 and 1/2 |x_new - x0|^2 in slot F; defaults to an internal scratch.""")

    def run(self, n_iter, record_loss=True):
        """n_iter iterations (one host synchronisation at the end); returns the loss history as a numpy array (global over all ranks), or
        None.  Row k is 1/2 |x_{k+1} - x0|^2 + reg |D x_bar_k|_{2,1}: the TV term is that of the EXTRAPOLATED point the dual step saw, not
        of an iterate -- a progress indicator in the slots of ``ChambollePock``'s history, not the objective of x_{k+1}.  The exact primal
        value of the current iterate is ``duality_gap()[0]``.  A diverging run (steps forced past the bound) returns its numbers, non-finite
        ones included; it never raises."""
        return self._run(n_iter, record_loss)

    duality_gap = _redoc(_GapStopping.duality_gap, tail=_SlabProblem._GAP_DOC)
    run_until = _redoc(_GapStopping.run_until, tail=_SlabProblem._GAP_DOC)


# =================================================================================================
class HuberChambollePock(_GapStopping, _OneSweepCP):
    """min_x 1/2 |x - x0|^2 + regularization * sum_sites h_alpha(|D x|_2) -- the HUBER-TV (Huber-ROF) model of Chambolle & Pock 2011, section
    6.2.1, the standard remedy for the staircasing of plain TV (smooth ramps coming back as terraces):

        h_alpha(t) = t^2 / (2 alpha)  for t <= alpha,     t - alpha / 2  beyond

    ``alpha`` is the gradient magnitude below which the model smooths instead of preserving an edge, in grey levels per weighted difference
    (the differences D takes: per pixel, times sqrt(reg_z_over_reg) / sqrt(reg_time) along z / t).  It scales with the data's grey levels.

    The quadratic part makes the conjugate of the regulariser (alpha / regularization)-strongly convex; the fidelity is 1-strongly convex.
    Both halves of the saddle problem being strongly convex, Algorithm 3 of the paper applies: FIXED steps from ``cp_linear_steps(L2, gamma,
    alpha / regularization)``, theta < 1, linear convergence O(omega^k).  State: x, x_bar (images), q (gradient); x = x_bar = x0, q = 0 at
    the start.  One iteration:

        v      = (q + sigma D x_bar) / (1 + sigma alpha / reg)
        q     <- v / max(1, |v|_2 / reg)                                            tv_cp_dual_huber on x_bar  (2 Nd + 1 words per voxel)
        x_new <- (x - tau D^T q + tau x0) / (1 + tau)
        x_bar <- x_new + theta (x_new - x);  x <- x_new                             tv_cp_primal_accel, one pass (Nd + 4)

    -- the kernel pair of ``AcceleratedChambollePock`` with another dual epilogue: 3 Nd + 5 words per voxel.  Sharded (``slab``): the boundary
    plane(s) of x_bar travel before the dual kernel and those of q before the primal kernel, both waits exposed.

    The ONE-SWEEP path (``set_fused``, ``fused``) runs the same iteration as tv_cp_huber_sweep +
    tv_cp_accel_fixup -- the one-sweep kernel of ``AcceleratedChambollePock`` with one more multiply per channel in its dual update and the
    Huber sum as its first partial; the fix-up is that solver's, unchanged.  x_bar is ping-ponged with a second buffer, x is updated in
    place, q is read and written once: 2 Nd + 5 words per voxel.  The state (x, x_bar, q) is the same on both paths, so ``set_fused`` may be
    called between iterations at any time.  DEFAULT: ``ChambollePock``'s rule -- the sweep where tv_cp_fused_supported accepts the geometry,
    the volume is not sharded and holds at least 1024 * TV_FUSED_MIN_KVOXELS (16 Mi) voxels, the pair otherwise.  Measured on
    64x8x1024x1024 fp32 (profiles/huber_cp_sweep_bench.txt): the sweep path takes 0.66 - 0.83 of the pair's time per
    iteration in all four schemes and 1.00 - 1.03 of ``AcceleratedChambollePock``'s one-sweep iteration, so the rule holds for every scheme.

    The model has an EXACT duality gap (``duality_gap``, ``run_until``), as the plain-TV solvers have.

    alpha -> 0 makes mu -> 0 (tau -> 0, sigma -> inf): the linear rate degenerates, and ``AcceleratedChambollePock`` -- plain TV, O(1/k^2)
    -- is then the solver to use.  alpha = 0 is refused.

    Not built (out of scope here): the sweep / exchange / fix-up schedule of a sharded slab on the one-sweep path (slabs run the kernel
    pair), a persistent small-volume form, hipGraph capture, the placement tuner / arena of ``ChambollePock``, a plane-marching form of the
    gap kernel, and Huber-TV under the L1 / Huber / KL data terms of ``RobustChambollePock`` / ``PoissonChambollePock``.  A per-voxel
    weight on the (plain) TV term is ``AdaptiveTVChambollePock``.  A per-voxel weight on THIS regulariser is ``AdaptiveHuberChambollePock``.

    Per-step scalars: the slots of ``ChambollePock`` -- sum h_alpha(|D x_bar|_2) in slot 0, 1/2 |x_new - x0|^2 in slot ``F`` (one-sweep
    path: the sweep's part in slot ``F``, the fix-up's in ``F + 1``; they are summed when the loss is asked for)."""

    def __init__(self, x0, regularization, alpha, scheme="hybrid", reg_z_over_reg=1.0, reg_time=0.0, mask_static=False,
                 factor_reg_static=0, gamma=1.0, slab=None, pitch="auto"):
        """alpha: see the class docstring; finite and > 0, as is ``regularization``.  gamma: the strong-convexity constant of the fidelity the
        steps are computed for, 0 < gamma <= 1 (1.0 = its true value; smaller = more conservative steps).  ValueError otherwise.  pitch: see
        ``_SlabProblem``.  The path of the iterations starts at the default rule of the class docstring; ``set_fused`` changes it."""
        alpha, gamma = float(alpha), float(gamma)
        if not (math.isfinite(alpha) and alpha > 0.0):
            raise ValueError("HuberChambollePock: alpha must be finite and > 0 (alpha = 0 is plain TV: AcceleratedChambollePock)")
        if not (0.0 < gamma <= 1.0):
            raise ValueError("HuberChambollePock: gamma must be in (0, 1]")
        if not (math.isfinite(float(regularization)) and float(regularization) > 0.0):
            raise ValueError("HuberChambollePock: regularization must be finite and > 0")
        super().__init__(x0, regularization, scheme, reg_z_over_reg, reg_time, mask_static, factor_reg_static, slab, pitch)
        self.alpha, self.gamma = alpha, gamma
        self.tau, self.sigma, self.theta, self.mu = cp_linear_steps(self.L2, gamma, alpha / self.reg)
        self._alloc_state()
        self._init_path()

    fused = property(_OneSweepCP.fused.fget, doc="True: iterations run as tv_cp_huber_sweep + tv_cp_accel_fixup; False: as tv_cp_dual_huber + "
                                                 "tv_cp_primal_accel (``set_fused``)")

    def _dual_kernel(self, sigma, out_ptr):
        _nv.check(self.lib.tv_cp_dual_huber(self.geo.ref, _nv.ptr(self.x_bar), _nv.ptr(self.xh_prev), _nv.ptr(self.xh_next), _nv.ptr(self.q),
                                            sigma, self.reg, self.alpha, out_ptr, _nv.ptr(self.ws), self.stream))

    def _sweep_kernel(self, tau, sigma, theta, tv_ptr, fid_ptr, g, ws, st):
        _nv.check(self.lib.tv_cp_huber_sweep(g, _nv.ptr(self.x_bar), None, None, _nv.ptr(self.q), _nv.ptr(self.q), _nv.ptr(self.x0),
                                             _nv.ptr(self.x), _nv.ptr(self.x_bar_alt), sigma, self.reg, self.alpha, tau, theta, 0, 0, -1,
                                             tv_ptr, fid_ptr, ws, st))

    step = _redoc(_ExtrapolatedCP.step, """Enqueue one iteration.  out: fp64 device tensor of SLOTS words (zero on entry) receiving this rank's sum h_alpha(|D x_bar|_2) in
        slot 0 and 1/2 |x_new - x0|^2 in slot F; defaults to an internal scratch.""")

    def run(self, n_iter, record_loss=True):
        """n_iter iterations (one host synchronisation at the end); returns the loss history as a numpy array (global over all ranks), or
        None.  Row k is 1/2 |x_{k+1} - x0|^2 + reg * sum h_alpha(|D x_bar_k|_2): the regulariser is that of the EXTRAPOLATED point the dual
        step saw -- a progress indicator in the slots of ``ChambollePock``'s history.  The exact primal value of the current iterate is
        ``duality_gap()[0]``."""
        return self._run(n_iter, record_loss)

    _GAP_DOC = """For P(x) = 1/2 |x - x0|^2 + reg sum h_alpha(|D x|_2) and any dual variable q with |q|_2 <= reg per site,
        Dual(q) = <D^T q, x0> - 1/2 |D^T q|^2 - (alpha / 2 reg) |q|^2 <= P(x*) <= P(x), and by strong convexity 1/2 |x - x*|^2 <= P(x) - Dual(q).
        The kernel (tv_dual_gap_huber) sums the gap site by site as 1/2 (x - x0 + D^T q)^2 + [reg h_alpha(|D x|_2) - <q, D x> + (alpha / 2 reg)
        |q|^2], both parts >= 0 (the second as a perfect square where |D x|_2 <= alpha), and writes nothing but three scalars.
        fp32 FLOOR: beyond alpha the second part cancels, leaving an absolute error of order eps_fp32 * P, so relative gaps below about 1e-6
        are not resolvable in fp32; the gap may then come out slightly negative (it is not clamped) and ``run_until`` ends on its iteration
        limit with ``converged=False``."""

    def _gap_kernel(self, x, q, qscale, b, out):
        _nv.check(self.lib.tv_dual_gap_huber(self.geo.ref, _nv.ptr(x), _nv.ptr(b["xp"]), _nv.ptr(b["xn"]), _nv.ptr(q), _nv.ptr(b["qp"]),
                                             _nv.ptr(b["qn"]), _nv.ptr(self.x0), self.reg, self.alpha, out.data_ptr(), _nv.ptr(self.ws),
                                             self.stream))

    duality_gap = _redoc(_GapStopping.duality_gap, """(primal, dual, gap) of the current iterate and dual variable (x, q) as Python floats, between ``run`` / ``run_steps`` / ``step``
        calls; the state of the loop is not touched (halo buffers of its own, one all-reduce of three scalars).  primal = 1/2 |x - x0|^2 +
        reg * sum h_alpha(|D x|_2).  Sharded: collective, every rank calls it and gets the same numbers.
        """, _GAP_DOC)
    run_until = _redoc(_GapStopping.run_until, tail=_GAP_DOC)


# =================================================================================================
class AdaptiveTVChambollePock(AcceleratedChambollePock):
    """min_x 1/2 |x - x0|^2 + regularization * sum_i g_i |D x|_{2,i} with a PER-VOXEL REGULARISATION WEIGHT g_i >= 0 (``reg_weights``, an
    array like x0) -- spatially adaptive TV, with the accelerated iteration of ``AcceleratedChambollePock`` (Chambolle & Pock 2011,
    Algorithm 2: the fidelity is still 1-strongly convex).  What g is for:

        noise-adaptive lambda     CT slices and frames whose noise level varies with dose or path length: g_i follows the local noise
        edge-stopping weights     g = 1 / (1 + (|D x0|_2 / kappa)^2), the weighted TV of the segmentation and edge-preserving denoising
                                  literature (``pytv.edge_stopping_weights``)
        protected regions         g = 0 inside a region of interest: it is left alone while the background is smoothed

    The conjugate of the regulariser differs from plain TV's only in the radius of the ball each site's dual vector is projected onto:
    regularization * g_i instead of regularization.  D, D^T, the step bound and the schedule are those of plain TV.  Iteration k:

        v      = q + sigma_k D x_bar;  r_i = reg g_i
        q     <- v where |v|_2 <= r_i, v r_i / |v|_2 beyond                          tv_cp_dual_wtv on x_bar      (2 Nd + 2 words per voxel)
        x_new <- (x - tau_k D^T q + tau_k x0) / (1 + tau_k)
        x_bar <- x_new + theta_k (x_new - x);  x <- x_new                           tv_cp_primal_accel, one pass (Nd + 4)

    -- the kernel pair of ``AcceleratedChambollePock`` with another dual epilogue that reads one more array (g): 3 Nd + 6 words per voxel.
    A site inside its ball keeps v bit for bit and a site with g_i = 0 keeps q = 0 exactly, so a protected voxel whose neighbouring sites
    are protected too never moves.  All-zero g is allowed: the solver then returns x0.  g is stored like x0 (this
    rank's planes, pitched with it) and needs no halo plane.  Sharded (``slab``): as ``AcceleratedChambollePock``.

    The model has an EXACT duality gap (tv_dual_gap_wtv), so ``duality_gap`` / ``run_until`` certify the iterate as they do for plain TV.

    Not built (out of scope here): the one-sweep / fix-up form of the iteration (``set_fused(True)`` raises, ``fused`` is always False), a
    persistent small-volume form, hipGraph capture, the placement tuner / arena of ``ChambollePock``, a plane-marching form of the gap
    kernel, g under the L1 / Huber / KL / weighted data terms of ``RobustChambollePock`` / ``PoissonChambollePock`` /
    ``WeightedChambollePock`` or with the Huber-TV regulariser of ``HuberChambollePock``, and g in ``ADMM`` / ``SubgradientDescent``.
    g with the Huber-TV regulariser, one-sweep path included, is the sibling class ``AdaptiveHuberChambollePock``.

    Per-step scalars: the slots of ``ChambollePock`` -- sum g_i |D x_bar|_2 in slot 0, 1/2 |x_new - x0|^2 in slot ``F``."""

    def __init__(self, x0, regularization, reg_weights, scheme="hybrid", reg_z_over_reg=1.0, reg_time=0.0, mask_static=False,
                 factor_reg_static=0, tau0=None, sigma0=None, gamma=1.0, slab=None, pitch="auto"):
        """reg_weights: g, a floating-point (or bool) array of x0's shape (this rank's slab), finite and >= 0; kept in the layout of x0.
        regularization: finite and > 0.  ValueError otherwise; sharded: the check of g is collective, every rank raises.  tau0, sigma0,
        gamma, pitch: see ``AcceleratedChambollePock``."""
        if not (math.isfinite(float(regularization)) and float(regularization) > 0.0):
            raise ValueError("AdaptiveTVChambollePock: regularization must be finite and > 0")
        # g is checked BEFORE the state is allocated (an x0 that is no device tensor is left to the base's own refusal)
        g = self._checked_weights(x0, reg_weights, slab) if isinstance(x0, torch.Tensor) and x0.is_cuda else None
        super().__init__(x0, regularization, scheme, reg_z_over_reg, reg_time, mask_static, factor_reg_static, tau0, sigma0, gamma, slab, pitch)
        self.g = self.image_copy(g)

    @staticmethod
    def _checked_weights(x0, reg_weights, slab):
        """``reg_weights`` as a device tensor of x0's dtype, or ValueError; ``slab`` (or None) carries the one all-reduce that makes the
        refusal collective"""
        g = torch.as_tensor(reg_weights, device=x0.device)
        shape_ok = tuple(g.shape) == tuple(x0.shape) and (g.dtype == torch.bool or g.dtype.is_floating_point)
        if shape_ok:
            g = g.to(x0.dtype)
            glo, ghi = torch.aminmax(g)                                     # NaN propagates through both
            bad = (~((glo >= 0) & torch.isfinite(ghi))).to(torch.float64).reshape(1)
        else:
            bad = torch.ones(1, dtype=torch.float64, device=x0.device)
        if slab is not None:
            slab.allreduce_sum_(bad)
        if not shape_ok:
            raise ValueError("AdaptiveTVChambollePock: reg_weights must be a bool or floating-point array of x0's shape, %r (got %r, %s)"
                             % (tuple(x0.shape), tuple(g.shape), g.dtype))
        if float(bad.item()) != 0.0:
            raise ValueError("AdaptiveTVChambollePock: reg_weights must be finite and >= 0 everywhere")
        return g

    def set_fused(self, fused):
        """The one-sweep kernels do not know about g: True raises ValueError; False and None (the construction default) keep the kernel
        pair.  ``fused`` is always False."""
        if fused:
            raise ValueError("set_fused(True): AdaptiveTVChambollePock has no one-sweep path (the one-sweep kernels take a scalar lambda)")
        self._fused = False

    def _dual_kernel(self, sigma, out_ptr):
        _nv.check(self.lib.tv_cp_dual_wtv(self.geo.ref, _nv.ptr(self.x_bar), _nv.ptr(self.xh_prev), _nv.ptr(self.xh_next), _nv.ptr(self.q),
                                          _nv.ptr(self.g), sigma, self.reg, out_ptr, _nv.ptr(self.ws), self.stream))

    _GAP_DOC = """For P(x) = 1/2 |x - x0|^2 + reg sum g_i |D x|_{2,i} and any dual variable q with |q|_2 <= reg g_i per site,
        Dual(q) = <D^T q, x0> - 1/2 |D^T q|^2 <= P(x*) <= P(x), and by strong convexity 1/2 |x - x*|^2 <= P(x) - Dual(q).  The kernel
        (tv_dual_gap_wtv) sums the gap site by site as 1/2 (x - x0 + D^T q)^2 + (reg g_i |D x|_2 - <q, D x>), both parts >= 0, and writes
        nothing but three scalars.
        fp32 FLOOR: the cancellation inside the second part leaves an absolute error of order eps_fp32 * P, so relative gaps below about
        1e-6 are not resolvable in fp32; the gap may then come out slightly negative (it is not clamped) and ``run_until`` ends on its
        iteration limit with ``converged=False``."""

    def _gap_kernel(self, x, q, qscale, b, out):
        _nv.check(self.lib.tv_dual_gap_wtv(self.geo.ref, _nv.ptr(x), _nv.ptr(b["xp"]), _nv.ptr(b["xn"]), _nv.ptr(q), _nv.ptr(b["qp"]),
                                           _nv.ptr(b["qn"]), _nv.ptr(self.x0), _nv.ptr(self.g), self.reg, out.data_ptr(), _nv.ptr(self.ws),
                                           self.stream))

    duality_gap = _redoc(_GapStopping.duality_gap, """(primal, dual, gap) of the current iterate and dual variable (x, q) as Python floats, between ``run`` / ``run_steps`` / ``step``
        calls; the state of the loop is not touched.  primal = 1/2 |x - x0|^2 + reg * sum g_i |D x|_2.  Sharded: collective, every rank
        calls it and gets the same numbers.
        """, _GAP_DOC)
    run_until = _redoc(_GapStopping.run_until, tail=_GAP_DOC)


# =================================================================================================
class VectorialTVChambollePock(AcceleratedChambollePock):
    """min_x 1/2 |x - x0|^2 + regularization * sum_s |D x|_{F,s} -- CHANNEL-COUPLED (vectorial / joint / collaborative) TV: the M frames of
    the (Nz, M, N, N) volume are channels of ONE object, and one Frobenius norm is taken per SPATIAL site s = (z, y, x) over all gradient
    channels c and all frames m,

        |D x|_{F,s} = ( sum_{m,c} (D x)[z, c, m, y, x]^2 )^(1/2)

    (Blomgren & Chan 1998; Bresson & Chan 2008).  Every other solver here regularises the frames independently -- their edges move
    independently and detail is lost in the weak channels; the coupled norm puts the edges of all channels in the same places: dual- and
    multi-energy CT, multi-contrast or multi-echo series, colour stacks, gated frames with shared anatomy.  With ``reg_time`` = 0 this is
    the pure spatial joint TV; with ``reg_time`` > 0 the weighted time differences join the same norm; M = 1 is plain TV.

    The fidelity is still 1-strongly convex and |D|^2 is unchanged, so the iteration is that of ``AcceleratedChambollePock`` (Chambolle &
    Pock 2011, Algorithm 2, ``accel_schedule``); only the ball of the dual projection changes -- ONE ball of radius reg per spatial site
    bounding the M Nd-vector, so ONE factor per site, applied to every frame and channel.  Iteration k:

        v      = q + sigma_k D x_bar  (all m, c of site s);  n_s = |v_s|_F
        q     <- v where n_s <= reg, v reg / n_s beyond                             tv_cp_dual_vtv on x_bar
        x_new <- (x - tau_k D^T q + tau_k x0) / (1 + tau_k)
        x_bar <- x_new + theta_k (x_new - x);  x <- x_new                           tv_cp_primal_accel, one pass (Nd + 4)

    tv_cp_dual_vtv: a thread owns a spatial site and walks its frames.  Up to 8 frames (hybrid: 4) v stays in registers -- 2 Nd + 1 words
    per voxel, the pair moves the 3 Nd + 5 words of ``AcceleratedChambollePock``'s; more frames take two passes over the site's frames (n_s,
    then v again times the factor): at most 3 Nd + 2, so 4 Nd + 6 words for the pair, less where the caches hold a site's frames (DESIGN.md
    section 3.11).  A site inside its ball keeps v bit for bit; nothing is NaN or Inf for finite input.  Sharded (``slab``): as
    ``AcceleratedChambollePock`` -- a z-cut never separates the frames of a site, so the same kernel pair runs with the same exchanges.

    The model has an EXACT duality gap (tv_dual_gap_vtv), so ``duality_gap`` / ``run_until`` certify the iterate as they do for plain TV.

    Not built (out of scope here): a one-sweep / fix-up, plane-marching, persistent or hipGraph form of the iteration (``set_fused(True)``
    raises, ``fused`` is always False), a per-voxel weight or the Huber function on the coupled norm (``AdaptiveTVChambollePock`` /
    ``HuberChambollePock`` have them per frame), and the coupled norm in ``ADMM`` / ``SubgradientDescent``.

    Per-step scalars: the slots of ``ChambollePock`` -- sum_s |D x_bar|_{F,s} in slot 0, 1/2 |x_new - x0|^2 in slot ``F``."""

    def __init__(self, x0, regularization, scheme="hybrid", reg_z_over_reg=1.0, reg_time=0.0, mask_static=False, factor_reg_static=0,
                 tau0=None, sigma0=None, gamma=1.0, slab=None, pitch="auto"):
        """regularization: finite and > 0 (ValueError otherwise).  tau0, sigma0, gamma, pitch: see ``AcceleratedChambollePock``."""
        if not (math.isfinite(float(regularization)) and float(regularization) > 0.0):
            raise ValueError("VectorialTVChambollePock: regularization must be finite and > 0")
        super().__init__(x0, regularization, scheme, reg_z_over_reg, reg_time, mask_static, factor_reg_static, tau0, sigma0, gamma, slab, pitch)

    def set_fused(self, fused):
        """The one-sweep kernels project frame by frame: True raises ValueError; False and None (the construction default) keep the kernel
        pair.  ``fused`` is always False."""
        if fused:
            raise ValueError("set_fused(True): VectorialTVChambollePock has no one-sweep path (the one-sweep kernels project each frame's "
                             "dual vector on its own)")
        self._fused = False

    def _dual_kernel(self, sigma, out_ptr):
        _nv.check(self.lib.tv_cp_dual_vtv(self.geo.ref, _nv.ptr(self.x_bar), _nv.ptr(self.xh_prev), _nv.ptr(self.xh_next), _nv.ptr(self.q),
                                          sigma, self.reg, out_ptr, _nv.ptr(self.ws), self.stream))

    _GAP_DOC = """For P(x) = 1/2 |x - x0|^2 + reg sum_s |D x|_{F,s} and any dual variable q with |q_s|_F <= reg per spatial site,
        Dual(q) = <D^T q, x0> - 1/2 |D^T q|^2 <= P(x*) <= P(x), and by strong convexity 1/2 |x - x*|^2 <= P(x) - Dual(q).  The kernel
        (tv_dual_gap_vtv) sums the gap as 1/2 (x - x0 + D^T q)^2 per voxel + (reg |D x|_{F,s} - <q, D x>_s) per spatial site, both parts
        >= 0 (Cauchy-Schwarz over the joint vector), and writes nothing but three scalars.
        fp32 FLOOR: the cancellation inside the second part leaves an absolute error of order eps_fp32 * P, so relative gaps below about
        1e-6 are not resolvable in fp32; the gap may then come out slightly negative (it is not clamped) and ``run_until`` ends on its
        iteration limit with ``converged=False``."""

    def _gap_kernel(self, x, q, qscale, b, out):
        _nv.check(self.lib.tv_dual_gap_vtv(self.geo.ref, _nv.ptr(x), _nv.ptr(b["xp"]), _nv.ptr(b["xn"]), _nv.ptr(q), _nv.ptr(b["qp"]),
                                           _nv.ptr(b["qn"]), _nv.ptr(self.x0), self.reg, out.data_ptr(), _nv.ptr(self.ws), self.stream))

    duality_gap = _redoc(_GapStopping.duality_gap, """(primal, dual, gap) of the current iterate and dual variable (x, q) as Python floats, between ``run`` / ``run_steps`` / ``step``
        calls; the state of the loop is not touched.  primal = 1/2 |x - x0|^2 + reg * sum_s |D x|_{F,s}.  Sharded: collective, every rank
        calls it and gets the same numbers.
        """, _GAP_DOC)
    run_until = _redoc(_GapStopping.run_until, tail=_GAP_DOC)


# =================================================================================================
class AdaptiveHuberChambollePock(_GapStopping, _OneSweepCP):
    """min_x 1/2 |x - x0|^2 + regularization * sum_i g_i h_alpha(|D x|_{2,i}) -- the HUBER-TV regulariser of ``HuberChambollePock`` under the
    PER-VOXEL WEIGHT g_i >= 0 of ``AdaptiveTVChambollePock`` (``reg_weights``, an array like x0).  Edge-stopping weights and noise-adaptive
    lambda smooth hardest on the flat and gently ramped regions, exactly where plain TV leaves terraces; h_alpha is quadratic below the
    gradient magnitude ``alpha`` and removes them (see the two sibling classes for what g and alpha mean).

    With r_i = reg g_i the conjugate of a site's term is alpha |q_i|^2 / (2 r_i) + indicator(|q_i|_2 <= r_i) (g_i = 0: the indicator of
    q_i = 0); it is (alpha / (reg g_max))-strongly convex, the fidelity is 1-strongly convex, so Algorithm 3 of Chambolle & Pock 2011
    applies: FIXED steps from ``cp_linear_steps(L2, gamma, alpha / (reg g_max))``, linear convergence.  g_max is the maximum of g over ALL
    ranks, so every rank takes the same steps; an all-zero g is allowed (g_max = 1 for the steps) and the solver then returns x0.  State:
    x, x_bar (images), q (gradient); x = x_bar = x0, q = 0 at the start.  One iteration:

        shrink_i = r_i / (r_i + sigma alpha)                                        (0 where r_i = 0)
        v      = shrink_i (q + sigma D x_bar)
        q     <- v where |v|_2 <= r_i, v r_i / |v|_2 beyond, 0 where r_i = 0        tv_cp_dual_hwtv on x_bar   (2 Nd + 2 words per voxel)
        x_new <- (x - tau D^T q + tau x0) / (1 + tau)
        x_bar <- x_new + theta (x_new - x);  x <- x_new                             tv_cp_primal_accel, one pass (Nd + 4)

    -- 3 Nd + 6 words per voxel as that kernel pair.  A site inside its ball keeps v bit for bit and a site with g_i = 0 keeps q = 0
    exactly, so a protected voxel whose neighbouring sites are protected too never moves.  g is stored like x0 (this rank's planes, pitched
    with it) and needs no halo plane.  Sharded (``slab``): the kernel pair, the boundary plane(s) of x_bar travel before the dual kernel and
    those of q before the primal kernel, both waits exposed.

    The ONE-SWEEP path (``set_fused``, ``fused``) runs the same iteration as tv_cp_hwtv_sweep + tv_cp_accel_fixup -- the one-sweep kernel of
    ``HuberChambollePock`` with g of the site as one more streamed load per frame; the fix-up is ``AcceleratedChambollePock``'s, unchanged:
    2 Nd + 6 words per voxel.  The state (x, x_bar, q) is the same on both paths, so ``set_fused`` may be called between iterations at any
    time.  DEFAULT: ``ChambollePock``'s rule -- the sweep where tv_cp_fused_supported accepts the geometry, the volume is not sharded and
    holds at least 1024 * TV_FUSED_MIN_KVOXELS (16 Mi) voxels -- but only for the schemes in ``SWEEP_DEFAULT_SCHEMES``, those whose sweep
    iteration measured faster than the pair's by more than the pair's run-to-run spread on 64x8x1024x1024 fp32
    (profiles/adaptive_huber_bench.txt); the pair otherwise.

    The model has an EXACT duality gap (tv_dual_gap_hwtv), so ``duality_gap`` / ``run_until`` certify the iterate.

    Not built (out of scope here): a plane-marching form of the dual kernel (large-plane SLABS run the one-site kernel; unsharded large
    planes have the sweep) and of the gap kernel, the sweep / exchange / fix-up schedule of a sharded slab, a persistent small-volume form,
    hipGraph capture, and a per-voxel alpha.

    Per-step scalars: the slots of ``ChambollePock`` -- sum g_i h_alpha(|D x_bar|_2) in slot 0, 1/2 |x_new - x0|^2 in slot ``F`` (one-sweep
    path: the sweep's part in slot ``F``, the fix-up's in ``F + 1``; they are summed when the loss is asked for)."""

    SWEEP_DEFAULT_SCHEMES = ("upwind", "downwind", "hybrid")      # not central: its sweep took 1.08 of the pair's time (it runs without the dual prefetch)

    def _one_sweep_default(self, sharded_ok):
        """``_SlabProblem``'s rule, for the schemes in ``SWEEP_DEFAULT_SCHEMES`` only (class docstring)"""
        return self.scheme in self.SWEEP_DEFAULT_SCHEMES and super()._one_sweep_default(sharded_ok)

    def __init__(self, x0, regularization, reg_weights, alpha, scheme="hybrid", reg_z_over_reg=1.0, reg_time=0.0, mask_static=False,
                 factor_reg_static=0, gamma=1.0, slab=None, pitch="auto"):
        """reg_weights: g, a floating-point (or bool) array of x0's shape (this rank's slab), finite and >= 0; kept in the layout of x0.
        alpha, regularization: finite and > 0.  gamma: as in ``HuberChambollePock``, 0 < gamma <= 1.  ValueError otherwise; sharded: the
        check of g is collective, every rank raises.  pitch: see ``_SlabProblem``.  The path of the iterations starts at the default rule
        of the class docstring; ``set_fused`` changes it."""
        alpha, gamma = float(alpha), float(gamma)
        if not (math.isfinite(alpha) and alpha > 0.0):
            raise ValueError("AdaptiveHuberChambollePock: alpha must be finite and > 0 (alpha = 0 is plain adaptive TV: AdaptiveTVChambollePock)")
        if not (0.0 < gamma <= 1.0):
            raise ValueError("AdaptiveHuberChambollePock: gamma must be in (0, 1]")
        if not (math.isfinite(float(regularization)) and float(regularization) > 0.0):
            raise ValueError("AdaptiveHuberChambollePock: regularization must be finite and > 0")
        # g is checked BEFORE the state is allocated (an x0 that is no device tensor is left to the base's own refusal)
        g = None
        if isinstance(x0, torch.Tensor) and x0.is_cuda:
            try:
                g = AdaptiveTVChambollePock._checked_weights(x0, reg_weights, slab)
            except ValueError as exc:            # the sibling's check (collective on slabs), under this class's name
                raise ValueError(str(exc).replace("AdaptiveTVChambollePock", "AdaptiveHuberChambollePock", 1)) from None
        super().__init__(x0, regularization, scheme, reg_z_over_reg, reg_time, mask_static, factor_reg_static, slab, pitch)
        gmax = g.max().to(torch.float64).reshape(1)
        self.slab.allreduce_max_(gmax)                    # over ALL ranks: the steps must be the same everywhere
        self.g_max = float(gmax.item())
        self.alpha, self.gamma = alpha, gamma
        self.tau, self.sigma, self.theta, self.mu = cp_linear_steps(self.L2, gamma, alpha / (self.reg * (self.g_max if self.g_max > 0.0 else 1.0)))
        self._alloc_state()
        self.g = self.image_copy(g)
        self._init_path()

    fused = property(_OneSweepCP.fused.fget, doc="True: iterations run as tv_cp_hwtv_sweep + tv_cp_accel_fixup; False: as tv_cp_dual_hwtv + "
                                                 "tv_cp_primal_accel (``set_fused``)")

    def _dual_kernel(self, sigma, out_ptr):
        _nv.check(self.lib.tv_cp_dual_hwtv(self.geo.ref, _nv.ptr(self.x_bar), _nv.ptr(self.xh_prev), _nv.ptr(self.xh_next), _nv.ptr(self.q),
                                           _nv.ptr(self.g), sigma, self.reg, self.alpha, out_ptr, _nv.ptr(self.ws), self.stream))

    def _sweep_kernel(self, tau, sigma, theta, tv_ptr, fid_ptr, g, ws, st):
        _nv.check(self.lib.tv_cp_hwtv_sweep(g, _nv.ptr(self.x_bar), None, None, _nv.ptr(self.q), _nv.ptr(self.q), _nv.ptr(self.x0),
                                            _nv.ptr(self.x), _nv.ptr(self.x_bar_alt), _nv.ptr(self.g), sigma, self.reg, self.alpha, tau,
                                            theta, 0, 0, -1, tv_ptr, fid_ptr, ws, st))

    step = _redoc(_ExtrapolatedCP.step, """Enqueue one iteration.  out: fp64 device tensor of SLOTS words (zero on entry) receiving this rank's sum g_i h_alpha(|D x_bar|_2)
        in slot 0 and 1/2 |x_new - x0|^2 in slot F; defaults to an internal scratch.""")

    def run(self, n_iter, record_loss=True):
        """n_iter iterations (one host synchronisation at the end); returns the loss history as a numpy array (global over all ranks), or
        None.  Row k is 1/2 |x_{k+1} - x0|^2 + reg * sum g_i h_alpha(|D x_bar_k|_2): the regulariser is that of the EXTRAPOLATED point the
        dual step saw -- a progress indicator in the slots of ``ChambollePock``'s history.  The exact primal value of the current iterate
        is ``duality_gap()[0]``."""
        return self._run(n_iter, record_loss)

    _GAP_DOC = """For P(x) = 1/2 |x - x0|^2 + reg sum g_i h_alpha(|D x|_{2,i}) and any dual variable q with |q|_2 <= r_i = reg g_i per site,
        Dual(q) = <D^T q, x0> - 1/2 |D^T q|^2 - sum_{r_i > 0} alpha |q_i|^2 / (2 r_i) <= P(x*) <= P(x), and by strong convexity
        1/2 |x - x*|^2 <= P(x) - Dual(q).  The kernel (tv_dual_gap_hwtv) sums the gap site by site as 1/2 (x - x0 + D^T q)^2 +
        [r_i h_alpha(|D x|_2) + alpha |q|^2 / (2 r_i) - <q, D x>], both parts >= 0 (the second as a perfect square where |D x|_2 <= alpha),
        and writes nothing but three scalars.
        fp32 FLOOR: beyond alpha the second part cancels, leaving an absolute error of order eps_fp32 * P, so relative gaps below about 1e-6
        are not resolvable in fp32; the gap may then come out slightly negative (it is not clamped) and ``run_until`` ends on its iteration
        limit with ``converged=False``."""

    def _gap_kernel(self, x, q, qscale, b, out):
        _nv.check(self.lib.tv_dual_gap_hwtv(self.geo.ref, _nv.ptr(x), _nv.ptr(b["xp"]), _nv.ptr(b["xn"]), _nv.ptr(q), _nv.ptr(b["qp"]),
                                            _nv.ptr(b["qn"]), _nv.ptr(self.x0), _nv.ptr(self.g), self.reg, self.alpha, out.data_ptr(),
                                            _nv.ptr(self.ws), self.stream))

    duality_gap = _redoc(_GapStopping.duality_gap, """(primal, dual, gap) of the current iterate and dual variable (x, q) as Python floats, between ``run`` / ``run_steps`` / ``step``
        calls; the state of the loop is not touched.  primal = 1/2 |x - x0|^2 + reg * sum g_i h_alpha(|D x|_2).  Sharded: collective, every
        rank calls it and gets the same numbers.
        """, _GAP_DOC)
    run_until = _redoc(_GapStopping.run_until, tail=_GAP_DOC)


# =================================================================================================
class _FixedPointResiduals:
    """The optimality residual of the solvers whose fidelity has a pointwise prox but no cheap duality gap (``RobustChambollePock``,
    ``PoissonChambollePock``, ``WeightedChambollePock``): tv_cp_dual_residual for the dual block, the class's primal kernel in residual mode for the fidelity block.
    The class supplies ``_prox(q, qp, qn, x, x_bar, theta, flags, out_ptr)`` (its primal entry point: the loop's ``_primal_kernel`` and,
    in residual mode, R_x) and ``_fidelity_value()``, takes its steps with ``_fixed_steps`` (Algorithm 1), calls ``_init_residuals`` at the
    end of its constructor, and binds ``residuals`` / ``run_until`` under its own text with ``_redoc`` (its ``_RES_DOC`` as the tail)."""

    def _fixed_steps(self, tau, sigma):
        """the constant steps of Algorithm 1: (tau, sigma) validated by ``cp_step_pair`` on ``L2``, theta = 1"""
        self.tau, self.sigma = cp_step_pair(self.L2, tau, sigma)
        self.theta = 1.0

    def _primal_kernel(self, tau, theta, out_ptr):
        self._prox(self.q, self.qh_prev, self.qh_next, self.x, self.x_bar, theta, 0, out_ptr)

    def residuals(self):
        """{"x": R_x, "q": R_q, "total": R_x + R_q, "tv": |D x|_{2,1}, "fid": F(x - x0)} of the current pair (x, q) as Python floats, between
        ``step`` / ``run`` calls; x, x_bar, q and the loop's halo planes are left as they are.  One all-reduce of the scalars, one host
        synchronisation.  Sharded: collective, every rank calls it and gets the same numbers.
        """
        return self._residual_dict(self._residual_scalars())

    def run_until(self, rel_res, max_iter, check_every=10):
        """Iterate until the residual has dropped by the factor asked for: ``run`` in blocks of ``check_every`` iterations, stopping at the
        first check where R_k <= rel_res**2 * R_0, or after ``max_iter`` iterations.  R_0 is the residual of the pair the constructor left
        (x0, q = 0); R_0 == 0 (a constant image: a saddle point already) returns at once with ``converged=True``.
        Returns (loss_history, info); info: ``iterations``, ``converged``, ``residuals`` (the last ``residuals()`` dict), ``initial`` = R_0 and
        ``relative`` = sqrt(R_k / R_0).  A check costs one Nd + 1-word pass, one Nd + 2-word pass and the fidelity reduction.
        """
        return self._run_until_residual(rel_res, max_iter, check_every)

    def _init_residuals(self):
        """halo buffers of ``residuals`` (its own: the loop's are not touched), and R_0 of the starting pair, enqueued here and read back
        (one synchronisation) only when somebody asks"""
        self._res_buf = self._halo_set()
        self._res0 = self._residual_scalars()
        self._R0 = None

    def _residual_scalars(self):
        """fp64 device words [|D x|_{2,1}, R_q, R_x, fidelity] of the current pair on this rank; kernels and reductions are enqueued,
        nothing waits for them.  Touches ``_res_buf`` and the workspace, never x, x_bar, q or the loop's halo planes."""
        out = torch.zeros(4, dtype=torch.float64, device=self.device)
        s, pl, b = self.slab, self.plan, self._res_buf
        s.wait(pl.exchange_image(self.x, b["xp"], b["xn"]))
        _nv.check(self.lib.tv_cp_dual_residual(self.geo.ref, _nv.ptr(self.x), _nv.ptr(b["xp"]), _nv.ptr(b["xn"]), _nv.ptr(self.q), self.sigma,
                                               self.reg, out[0:2].data_ptr(), _nv.ptr(self.ws), self.stream))
        s.wait(pl.exchange_grad(self.q, _plane0(b["qp"]), _plane0(b["qn"])))
        self._prox(self.q, b["qp"], b["qn"], self.x, None, 0.0, _nv.TV_CPP_RESIDUAL, out[2:3].data_ptr())
        out[3] = self._fidelity_value()
        return out

    def _residual_dict(self, out):
        self.slab.allreduce_sum_(out)                    # the four scalars in one call
        tv, rq, rx, fid = (float(v) for v in out.cpu().tolist())
        return {"x": rx, "q": rq, "total": rx + rq, "tv": tv, "fid": fid}

    def initial_residual(self):
        """R_0: ``residuals()["total"]`` of the pair the constructor left (x0, q = 0; enqueued there, read back on the first call)."""
        if self._R0 is None:
            self._R0 = self._residual_dict(self._res0)
        return self._R0["total"]


# =================================================================================================
class RobustChambollePock(_FixedPointResiduals, _ExtrapolatedCP):
    """min_x F(x - x0) + regularization * TV(x) for a ROBUST data term F (Chambolle & Pock 2011, section 6.2.2: TV-L1), with Algorithm 1
    of that paper (theta = 1, fixed steps).  ``fidelity``:

        "l1"     |x - x0|_1                       impulse noise: dead / hot detector pixels, zingers, salt and pepper
        "huber"  sum h_delta(x - x0)              e^2 / (2 delta) for |e| <= delta, |e| - delta / 2 beyond (``delta`` required, > 0)
        "l2"     1/2 |x - x0|^2                   the model of the other solvers, for comparison

    L1 and Huber are not strongly convex, so there is no accelerated schedule (``AcceleratedChambollePock`` is for the quadratic term only).
    State: x, x_bar (images), q (gradient); x = x_bar = x0, q = 0 at the start.  One iteration:

        q     <- proj_{|.|_2 <= reg}(q + sigma D x_bar)                             tv_cp_dual on x_bar        (2 Nd + 1 words per voxel)
        x_new <- x0 + prox_{tau F}((x - tau D^T q) - x0)
        x_bar <- 2 x_new - x;  x <- x_new                                           tv_cp_primal_prox, one pass (Nd + 4)

    -- the kernel-pair branch of ``AcceleratedChambollePock.step`` with another pointwise prox: 3 Nd + 5 words per voxel.  Sharded
    (``slab``): the boundary plane(s) of x_bar travel before the dual kernel and those of q before the primal kernel, both waits exposed.

    STEPS.  tau sigma L^2 <= 1 with L^2 = ``normal_spectral_bound``; both default to 1 / sqrt(L^2), one given: the other is 1 / (L^2 times
    it).  For L1 / Huber the balanced default is SLOW: the prox moves a voxel by at most tau per iteration, so an outlier of 255 grey
    levels needs hundreds of iterations at tau = 0.35.  A ``tau`` of a few grey levels of the data converges far faster -- on 0..255 data
    (NumPy restatement, 400 iterations) the relative residual is 2e-2 to 1e-1 with the default against about 7e-4 or better with tau = 5.

    How good is the iterate?  These models have no duality gap without a feasibility projection of D^T q; ``residuals()`` gives the
    fixed-point (KKT) residual of the saddle problem, ``run_until`` stops on it.

    Not built (out of scope here): a one-sweep / fix-up form of the iteration, hipGraph capture, a persistent small-volume form, the placement
    tuner / arena of ``ChambollePock``.  The Poisson / Kullback-Leibler fidelity (a pointwise prox with a square root and positivity
    handling of its own) is ``PoissonChambollePock``; the Huber-TV REGULARISER (with the quadratic data term) is ``HuberChambollePock``.

    Per-step scalars: the slots of ``ChambollePock`` -- |D x_bar|_{2,1} in slot 0, F(x_new - x0) in slot ``F``."""

    def __init__(self, x0, regularization, fidelity="l1", delta=None, scheme="hybrid", reg_z_over_reg=1.0, reg_time=0.0, mask_static=False,
                 factor_reg_static=0, tau=None, sigma=None, slab=None, pitch="auto"):
        """fidelity: "l1", "huber" or "l2"; delta: the Huber width in grey levels (required for "huber", ignored otherwise).  tau, sigma: see
        the class docstring -- tau * sigma * L^2 > 1 + 1e-12 raises ValueError.  pitch: see ``_SlabProblem``."""
        if fidelity not in _nv.FIDELITIES:
            raise ValueError("fidelity must be one of %s, got %r" % (sorted(_nv.FIDELITIES), fidelity))
        if fidelity == "huber":
            if delta is None or not (float(delta) > 0.0 and math.isfinite(float(delta))):
                raise ValueError("fidelity='huber' needs a finite delta > 0")
        super().__init__(x0, regularization, scheme, reg_z_over_reg, reg_time, mask_static, factor_reg_static, slab, pitch)
        self.fidelity, self.fid_code = fidelity, _nv.FIDELITIES[fidelity]
        self.delta = float(delta) if fidelity == "huber" else 0.0
        self._fixed_steps(tau, sigma)
        self._alloc_state()
        self._init_residuals()

    def _prox(self, q, qp, qn, x, x_bar, theta, flags, out_ptr):
        _nv.check(self.lib.tv_cp_primal_prox(self.geo.ref, _nv.ptr(q), _nv.ptr(qp), _nv.ptr(qn), _nv.ptr(x), _nv.ptr(x_bar), _nv.ptr(self.x0),
                                             self.fid_code, self.delta, self.tau, theta, flags, out_ptr, _nv.ptr(self.ws), self.stream))

    step = _redoc(_ExtrapolatedCP.step, """Enqueue one iteration.  out: fp64 device tensor of SLOTS words (zero on entry) receiving this rank's |D x_bar|_{2,1} in slot 0 and
        F(x_new - x0) in slot F; defaults to an internal scratch.""")

    def run(self, n_iter, record_loss=True):
        """n_iter iterations (one host synchronisation at the end); returns the loss history as a numpy array (global over all ranks), or
        None.  Row k is F(x_{k+1} - x0) + reg |D x_bar_k|_{2,1}: the TV term is that of the extrapolated point the dual step saw -- a
        progress indicator in the slots of ``ChambollePock``'s history; the objective of the current iterate is
        ``residuals()["fid"] + reg * residuals()["tv"]``."""
        return self._run(n_iter, record_loss)

    # ---- optimality residual of the saddle problem (tv_cp_dual_residual + tv_cp_primal_prox in residual mode) ----------------------------
    _RES_DOC = """(x, q) is a saddle point of  min_x max_{|q|_2 <= reg}  F(x - x0) + <D x, q>  (whose x solves the problem) iff it is a fixed point
        of both updates of the iteration.  The residual R = R_x + R_q:
            R_x = |x - x0 - prox_{tau F}(x - tau D^T q - x0)|^2 / tau^2      zero iff -D^T q is in the subdifferential of F at x - x0:
                                                                             tv_cp_primal_prox in residual mode, Nd + 2 words per voxel
            R_q = |q - proj(q + sigma D x)|^2 / sigma^2                      zero iff q is in the subdifferential of reg |.|_2 at D x:
                                                                             tv_cp_dual_residual, Nd + 1 words per voxel
        both summed site by site in fp64 by reduce-only kernels.  fp32: R_x is resolved down to about (eps_fp32 |x| / tau)^2 per voxel."""

    def _fidelity_value(self):
        """F(x - x0) of this rank as a 0-d fp64 device tensor: element-wise torch arithmetic in the image dtype, summed in fp64.  Called once
        per check, never inside the loop (the loop's own fidelity scalar comes out of tv_cp_primal_prox)."""
        e = torch.sub(self.x, self.x0).abs_()
        if self.fidelity == "l1":
            return e.sum(dtype=torch.float64)
        if self.fidelity == "l2":
            return 0.5 * torch.linalg.vector_norm(e, dtype=torch.float64) ** 2
        a = e.clamp(max=self.delta)
        return (e - a).sum(dtype=torch.float64) + torch.linalg.vector_norm(a, dtype=torch.float64) ** 2 / (2.0 * self.delta)

    residuals = _redoc(_FixedPointResiduals.residuals, tail=_RES_DOC)
    run_until = _redoc(_FixedPointResiduals.run_until, tail=_RES_DOC)


# =================================================================================================
class PoissonChambollePock(_FixedPointResiduals, _ExtrapolatedCP):
    """min_{x >= 0} F(x) + regularization * TV(x) for POISSON (photon-counting) data x0 >= 0 -- CT projections, low-dose frames,
    fluorescence stacks --, where the maximum-likelihood data term is the generalised Kullback-Leibler divergence

        F(x) = sum_i ( x_i - x0_i + x0_i log(x0_i / x_i) )        >= 0, zero at x = x0; 0 log 0 = 0; +inf where x_i = 0 < x0_i

    with Algorithm 1 of Chambolle & Pock 2011 (theta = 1, fixed steps; F is not strongly convex on x >= 0, so there is no accelerated
    schedule).  State: x, x_bar (images), q (gradient); x = x_bar = x0, q = 0 at the start.  One iteration:

        q     <- proj_{|.|_2 <= reg}(q + sigma D x_bar)                             tv_cp_dual on x_bar        (2 Nd + 1 words per voxel)
        v      = x - tau D^T q;  b = v - tau
        x_new <- prox_{tau F}(v) = (b + sqrt(b^2 + 4 tau x0)) / 2
        x_bar <- 2 x_new - x;  x <- x_new                                           tv_cp_primal_kl, one pass  (Nd + 4)

    -- 3 Nd + 5 words per voxel, the loop of ``RobustChambollePock`` with another pointwise prox.  The kernel takes the root in a form
    without cancellation (2 tau x0 / (sqrt(..) - b) where b < 0), so the iterate is >= 0 everywhere, a site with x0 = 0 goes to exactly 0
    once b < 0, and the loss stays finite.  Sharded (``slab``): as ``RobustChambollePock``.

    STEPS.  tau sigma L^2 <= 1 with L^2 = ``normal_spectral_bound``; both default to 1 / sqrt(L^2), one given: the other is 1 / (L^2 times
    it).  ``residuals()`` gives the fixed-point (KKT) residual of the saddle problem, ``run_until`` stops on it.  (A duality gap would need
    1 + D^T q > 0 at every site, which the iterates do not guarantee.)

    Not built: a one-sweep / fix-up form of the iteration, hipGraph capture, a persistent small-volume form, the placement tuner / arena
    of ``ChambollePock``, and a background term.  The Huber-TV regulariser exists for the quadratic data term only (``HuberChambollePock``).

    Per-step scalars: the slots of ``ChambollePock`` -- |D x_bar|_{2,1} in slot 0, F(x_new) in slot ``F``."""

    def __init__(self, x0, regularization, scheme="hybrid", reg_z_over_reg=1.0, reg_time=0.0, mask_static=False,
                 factor_reg_static=0, tau=None, sigma=None, slab=None, pitch="auto"):
        """x0: the counts, >= 0 and finite (ValueError otherwise: one min / max reduction; sharded: collective, every rank raises).  tau,
        sigma: see the class docstring -- tau * sigma * L^2 > 1 + 1e-12 raises ValueError.  pitch: see ``_SlabProblem``."""
        super().__init__(x0, regularization, scheme, reg_z_over_reg, reg_time, mask_static, factor_reg_static, slab, pitch)
        self._fixed_steps(tau, sigma)
        lo, hi = torch.aminmax(x0)                       # NaN propagates through both
        bad = (~((lo >= 0) & torch.isfinite(hi))).to(torch.float64).reshape(1)
        self.slab.allreduce_sum_(bad)
        if float(bad.item()) != 0.0:
            raise ValueError("PoissonChambollePock: x0 must be counts -- finite and >= 0 everywhere")
        self._alloc_state()
        self._init_residuals()

    def _prox(self, q, qp, qn, x, x_bar, theta, flags, out_ptr):
        _nv.check(self.lib.tv_cp_primal_kl(self.geo.ref, _nv.ptr(q), _nv.ptr(qp), _nv.ptr(qn), _nv.ptr(x), _nv.ptr(x_bar), _nv.ptr(self.x0),
                                           self.tau, theta, flags, out_ptr, _nv.ptr(self.ws), self.stream))

    step = _redoc(_ExtrapolatedCP.step, """Enqueue one iteration.  out: fp64 device tensor of SLOTS words (zero on entry) receiving this rank's |D x_bar|_{2,1} in slot 0 and
        F(x_new) in slot F; defaults to an internal scratch.""")

    def run(self, n_iter, record_loss=True):
        """n_iter iterations (one host synchronisation at the end); returns the loss history as a numpy array (global over all ranks), or
        None.  Row k is F(x_{k+1}) + reg |D x_bar_k|_{2,1}: the TV term is that of the extrapolated point the dual step saw -- a progress
        indicator in the slots of ``ChambollePock``'s history; the objective of the current iterate is
        ``residuals()["fid"] + reg * residuals()["tv"]``."""
        return self._run(n_iter, record_loss)

    _RES_DOC = """(x, q) is a saddle point of  min_{x >= 0} max_{|q|_2 <= reg}  F(x) + <D x, q>  (whose x solves the problem) iff it is a fixed point
        of both updates of the iteration.  The residual R = R_x + R_q:
            R_x = |x - prox_{tau F}(x - tau D^T q)|^2 / tau^2                zero iff -D^T q is in the subdifferential of F at x:
                                                                             tv_cp_primal_kl in residual mode, Nd + 2 words per voxel
            R_q = |q - proj(q + sigma D x)|^2 / sigma^2                      zero iff q is in the subdifferential of reg |.|_2 at D x:
                                                                             tv_cp_dual_residual, Nd + 1 words per voxel
        both summed site by site in fp64 by reduce-only kernels.  fp32: R_x is resolved down to about (eps_fp32 |x| / tau)^2 per voxel."""

    _FID_CHUNK = 1 << 24          # elements per fp64 temporary of ``_fidelity_value``

    def _fidelity_value(self):
        """F(x) of this rank as a 0-d fp64 device tensor: torch arithmetic in fp64 (0 log 0 = 0; +inf where x = 0 < x0), a few planes at
        a time so that the fp64 temporaries stay small.  Called once per check, never inside the loop (the loop's own fidelity scalar
        comes out of tv_cp_primal_kl)."""
        nz = self.x.shape[0]
        planes = max(1, self._FID_CHUNK // max(1, self.x[0].numel()))
        total = torch.zeros((), dtype=torch.float64, device=self.device)
        for a in range(0, nz, planes):
            x, c = self.x[a:a + planes].double(), self.x0[a:a + planes].double()
            ratio = torch.where(c > 0, c / x, torch.ones_like(c))
            total += (x - c).sum() + torch.xlogy(c, ratio).sum()
        return total

    residuals = _redoc(_FixedPointResiduals.residuals, """{"x": R_x, "q": R_q, "total": R_x + R_q, "tv": |D x|_{2,1}, "fid": F(x)} of the current pair (x, q) as Python floats, between
        ``step`` / ``run`` calls; x, x_bar, q and the loop's halo planes are left as they are.  One all-reduce of the scalars, one host
        synchronisation.  Sharded: collective, every rank calls it and gets the same numbers.
        """, _RES_DOC)
    run_until = _redoc(_FixedPointResiduals.run_until, tail=_RES_DOC)


# =================================================================================================
class WeightedChambollePock(_FixedPointResiduals, _ExtrapolatedCP):
    """min_{lower <= x <= upper} 1/2 sum_i w_i (x_i - x0_i)^2 + regularization * TV(x) with a PER-VOXEL DATA WEIGHT w >= 0 and an optional
    BOX on the iterate, with Algorithm 1 of Chambolle & Pock 2011 (theta = 1, fixed steps).

        w_i = 0          the voxel is UNKNOWN -- a dead detector module, a masked frame, a metal trace, a missing projection -- and TV fills
                         it in from its neighbours: the inpainting model of section 6.3 of the paper (x0 there is never looked at)
        w_i = 1 / s_i^2  heteroscedastic least squares: every voxel is trusted according to its own noise level
        lower, upper     bounds that hold EXACTLY on every iterate: non-negative attenuation, a normalised range [0, 1]

    State: x, x_bar (images), q (gradient); x = x_bar = clamp(x0), q = 0 at the start.  One iteration:

        q     <- proj_{|.|_2 <= reg}(q + sigma D x_bar)                             tv_cp_dual on x_bar         (2 Nd + 1 words per voxel)
        v      = x - tau D^T q;  c = tau w / (1 + tau w)
        x_new <- clamp(v - c (v - x0), lower, upper)                                the prox of a separable term: the quadratic's, clamped
        x_bar <- 2 x_new - x;  x <- x_new                                           tv_cp_primal_wls, one pass  (Nd + 5)

    -- 3 Nd + 6 words per voxel, the loop of ``RobustChambollePock`` with one more array read (w).  The prox is taken in the form above
    rather than (v + tau w x0) / (1 + tau w): a voxel with w = 0 is clamp(v) bit for bit, and a constant image inside the box is a fixed
    point bit for bit.  Sharded (``slab``): as ``RobustChambollePock``; w needs no halo plane.

    THE SHIFT.  The kernel takes boxes that contain 0 (the pad elements of pitched arrays must stay 0).  TV and the data term do not change
    when x, x0 and the box are shifted by one constant, so for another box the solver works on x0 - shift with the box
    [lower - shift, upper - shift], ``shift`` = min(max(0, lower), upper) -- the point of the box nearest to 0; 0 for every box that
    contains 0.  ``self.shift`` holds it, ``result()`` adds it back; ``self.x`` / ``self.x0`` / ``self.lower`` / ``self.upper`` are the
    SHIFTED state the kernels see.  (fp32: x0 - shift is rounded once, at construction.)

    STEPS.  tau sigma L^2 <= 1 with L^2 = ``normal_spectral_bound``; both default to 1 / sqrt(L^2), one given: the other is 1 / (L^2 times
    it).  ``residuals()`` gives the fixed-point (KKT) residual of the saddle problem, ``run_until`` stops on it.

    Not built (out of scope here): an ACCELERATED or linear-rate schedule -- the data term is min(w)-strongly convex only where every
    w > 0, and with gamma = min w the schedule of Algorithm 2 did not beat the fixed steps reliably in a NumPy restatement, so this solver
    runs Algorithm 1 only --, a one-sweep / fix-up form of the iteration, hipGraph capture, a persistent small-volume form, the placement
    tuner / arena of ``ChambollePock``, an ``x_init`` argument, and per-voxel weights on the TV term (``mask_static`` weights its time
    component only) under this data term: ``AdaptiveTVChambollePock`` has them for the plain quadratic data term.

    Per-step scalars: the slots of ``ChambollePock`` -- |D x_bar|_{2,1} in slot 0, 1/2 sum w (x_new - x0)^2 in slot ``F``."""

    def __init__(self, x0, regularization, weights, lower=None, upper=None, scheme="hybrid", reg_z_over_reg=1.0, reg_time=0.0,
                 mask_static=False, factor_reg_static=0, tau=None, sigma=None, slab=None, pitch="auto"):
        """x0: the data, finite.  weights: a bool array (True = known: stored as 1, False = unknown: 0) or a floating-point array, finite
        and >= 0, of x0's shape (this rank's slab); kept in the layout of x0.  lower, upper: the box, None = no bound on that side.
        ValueError: a wrong shape, weights that are negative or not finite, x0 not finite, lower > upper or a NaN bound, weights that are
        zero everywhere (on every rank: nothing ties the solution down), tau * max(w) not finite in the dtype of x0.  Sharded: the checks
        of the arrays are collective, every rank raises.  tau, sigma: see the class docstring -- tau * sigma * L^2 > 1 + 1e-12 raises
        ValueError.  pitch: see ``_SlabProblem``."""
        lo = -math.inf if lower is None else float(lower)
        hi = math.inf if upper is None else float(upper)
        if math.isnan(lo) or math.isnan(hi) or lo > hi:
            raise ValueError("WeightedChambollePock: lower <= upper is required (got lower=%r, upper=%r)" % (lower, upper))
        self.shift = min(max(0.0, lo), hi)
        if self.shift != 0.0 and isinstance(x0, torch.Tensor):
            x0 = x0 - self.shift
        super().__init__(x0, regularization, scheme, reg_z_over_reg, reg_time, mask_static, factor_reg_static, slab, pitch)
        self.lower, self.upper = lo - self.shift, hi - self.shift
        self._fixed_steps(tau, sigma)
        w = torch.as_tensor(weights, device=self.device)
        if tuple(w.shape) != tuple(x0.shape):
            raise ValueError("WeightedChambollePock: weights must have the shape of x0, %r (got %r)" % (tuple(x0.shape), tuple(w.shape)))
        if not (w.dtype == torch.bool or w.dtype.is_floating_point):
            raise ValueError("WeightedChambollePock: weights must be bool or floating point (got %s)" % w.dtype)
        w = w.to(self.dtype)
        wlo, whi = torch.aminmax(w)                      # NaN propagates through both
        xlo, xhi = torch.aminmax(x0)
        flags = torch.stack([~((wlo >= 0) & torch.isfinite(whi)), ~(torch.isfinite(xlo) & torch.isfinite(xhi))]).to(torch.float64)
        wmax = whi.to(torch.float64).nan_to_num(nan=0.0).reshape(1)
        self.slab.allreduce_sum_(flags)
        self.slab.allreduce_max_(wmax)
        bad_w, bad_x0 = (float(v) != 0.0 for v in flags.cpu().tolist())
        if bad_w:
            raise ValueError("WeightedChambollePock: weights must be finite and >= 0 everywhere")
        if bad_x0:
            raise ValueError("WeightedChambollePock: x0 must be finite everywhere (mark unknown voxels with a weight of 0 and any finite value)")
        wmax = float(wmax.item())
        if wmax == 0.0:
            raise ValueError("WeightedChambollePock: the weights are zero everywhere -- no voxel is known")
        if not self.tau * wmax <= torch.finfo(self.dtype).max:
            raise ValueError("WeightedChambollePock: tau * max(weights) = %g is not finite in %s" % (self.tau * wmax, self.dtype))
        self.w = self.image_copy(w)
        self._alloc_state()
        self._clamp_start()
        self._init_residuals()

    def _clamp_start(self):
        """x = x_bar = clamp(x0) (the pads of pitched arrays stay 0: the shifted box contains 0)"""
        self.x.clamp_(self.lower, self.upper)
        self.x_bar.copy_(self.x)

    def reset(self):
        """Back to the state of a fresh solver: x = x_bar = clamp(x0), q = 0, iteration 0."""
        super().reset()
        self._clamp_start()

    def result(self):
        """The iterate of the ORIGINAL problem (``shift`` added back) as a dense (Nz, M, Ny, Nx) tensor; with ``shift`` = 0 and dense state
        it is ``self.x`` itself, otherwise a copy."""
        out = super().result()
        return out + self.shift if self.shift != 0.0 else out

    def _prox(self, q, qp, qn, x, x_bar, theta, flags, out_ptr):
        _nv.check(self.lib.tv_cp_primal_wls(self.geo.ref, _nv.ptr(q), _nv.ptr(qp), _nv.ptr(qn), _nv.ptr(x), _nv.ptr(x_bar), _nv.ptr(self.x0),
                                            _nv.ptr(self.w), self.lower, self.upper, self.tau, theta, flags, out_ptr, _nv.ptr(self.ws),
                                            self.stream))

    step = _redoc(_ExtrapolatedCP.step, """Enqueue one iteration.  out: fp64 device tensor of SLOTS words (zero on entry) receiving this rank's |D x_bar|_{2,1} in slot 0 and
        1/2 sum w (x_new - x0)^2 in slot F; defaults to an internal scratch.""")

    def run(self, n_iter, record_loss=True):
        """n_iter iterations (one host synchronisation at the end); returns the loss history as a numpy array (global over all ranks), or
        None.  Row k is 1/2 sum w (x_{k+1} - x0)^2 + reg |D x_bar_k|_{2,1}: the TV term is that of the extrapolated point the dual step
        saw -- a progress indicator in the slots of ``ChambollePock``'s history; the objective of the current iterate is
        ``residuals()["fid"] + reg * residuals()["tv"]``."""
        return self._run(n_iter, record_loss)

    _RES_DOC = """(x, q) is a saddle point of  min_{lower <= x <= upper} max_{|q|_2 <= reg}  F(x) + <D x, q>,  F(x) = 1/2 sum w (x - x0)^2  (whose x
        solves the problem) iff it is a fixed point of both updates of the iteration.  The residual R = R_x + R_q:
            R_x = |x - prox_{tau F}(x - tau D^T q)|^2 / tau^2                zero iff -D^T q is in the subdifferential of F + box at x:
                                                                             tv_cp_primal_wls in residual mode, Nd + 3 words per voxel
            R_q = |q - proj(q + sigma D x)|^2 / sigma^2                      zero iff q is in the subdifferential of reg |.|_2 at D x:
                                                                             tv_cp_dual_residual, Nd + 1 words per voxel
        both summed site by site in fp64 by reduce-only kernels.  fp32: R_x is resolved down to about (eps_fp32 |x| / tau)^2 per voxel."""

    def _fidelity_value(self):
        """1/2 sum w (x - x0)^2 of this rank as a 0-d fp64 device tensor: element-wise torch arithmetic in the image dtype, summed in fp64.
        Called once per check, never inside the loop (the loop's own fidelity scalar comes out of tv_cp_primal_wls)."""
        e = torch.sub(self.x, self.x0)
        return 0.5 * e.mul_(e).mul_(self.w).sum(dtype=torch.float64)

    residuals = _redoc(_FixedPointResiduals.residuals, """{"x": R_x, "q": R_q, "total": R_x + R_q, "tv": |D x|_{2,1}, "fid": 1/2 sum w (x - x0)^2} of the current pair (x, q) as Python
        floats, between ``step`` / ``run`` calls; x, x_bar, q and the loop's halo planes are left as they are.  One all-reduce of the
        scalars, one host synchronisation.  Sharded: collective, every rank calls it and gets the same numbers.
        """, _RES_DOC)
    run_until = _redoc(_FixedPointResiduals.run_until, """Iterate until the residual has dropped by the factor asked for: ``run`` in blocks of ``check_every`` iterations, stopping at the
        first check where R_k <= rel_res**2 * R_0, or after ``max_iter`` iterations.  R_0 is the residual of the pair the constructor left
        (clamp(x0), q = 0); R_0 == 0 (a constant image: a saddle point already) returns at once with ``converged=True``.
        Returns (loss_history, info); info: ``iterations``, ``converged``, ``residuals`` (the last ``residuals()`` dict), ``initial`` = R_0 and
        ``relative`` = sqrt(R_k / R_0).  A check costs one Nd + 1-word pass, one Nd + 3-word pass and the fidelity reduction.
        """, _RES_DOC)


# =================================================================================================
class ChambollePockOperator(_SlabProblem):
    """min_x 1/2 |A x - b|^2 + regularization * TV(x) for a user-supplied linear operator A (the CT use case the
    reference is written for: README.md:2; its CP snippet is the special case A = I, README.md:148 ``sigma_A``).

        p <- (p + sigma_A (A x - b)) / (1 + sigma_A)
        q <- proj_{|.|_2 <= reg}(q + sigma_D D x)                       HIP: ONE sweep over q for both lines (tv_cpop_fused +
        x <- x - tau A^T p - tau D^T q                                   tv_cpop_fixup, round 3) or tv_cp_dual + tv_DT_axpy2

    ``A`` and ``AT`` are callables taking and returning DEVICE tensors (``A``: image (Nz, M, Ny, Nx) -> data of any
    shape, ``AT``: data -> image); they stay the user's code, the TV part runs in the HIP kernels.  ``A`` is applied ONCE by the
    constructor (the residual A x_init - b is carried from iteration to iteration); ``b`` must live on x_init's GPU.  ``tau`` must
    satisfy tau (sigma_A |A|^2 + sigma_D |D|^2) <= 1; the default assumes |A| <= 1.
    ``norm_A``: |A| as a number, or ``"estimate"`` (``operator_norm_sq``: 20 power iterations on A^T A from a seeded random image, times
    1.05); with ``tau=None`` the step is then tau = 1 / (sigma_A |A|^2 + sigma_D L), L = ``normal_spectral_bound`` >= |D|^2 -- the safe
    choice for a projector whose norm is in the tens or hundreds, where the default step diverges.  ``norm_A=None`` (the default) leaves
    tau exactly as it was; an explicit ``tau`` always wins.

    How good is the iterate?  A duality gap is out of reach here (with a general A the dual objective needs (A^T A)^-1); ``residuals()``
    gives the optimality (KKT) residual of the saddle problem the loop iterates on, ``run_until`` stops on it.

    With a ``slab`` (one process per GPU) ``x_init`` / ``b`` are this rank's z-slab of the image and its share of the data,
    ``A`` / ``AT`` act on the slab (operators that couple the slabs -- a cone-beam projector, say -- do their own
    communication inside the callables); the TV part trades the image / gradient halo planes like ``ChambollePock``."""

    NORM_ITER = 20          # power iterations of norm_A="estimate"

    def __init__(self, A, AT, b, x_init, regularization, scheme="hybrid", reg_z_over_reg=1.0, reg_time=0.0,
                 mask_static=False, factor_reg_static=0, sigma_D=0.5, sigma_A=1.0, tau=None, slab=None, fused=None, norm_A=None):
        super().__init__(x_init, scheme, reg_z_over_reg, reg_time, mask_static, factor_reg_static, slab)
        if not isinstance(b, torch.Tensor) or not b.is_cuda or b.device != self.device:
            # b's raw pointer goes to HIP kernels (tv_cpop_residual, tv_cpop_p): a host tensor or one on another GPU would be a
            # memory fault there, not the device-mismatch error torch used to raise (round-3 advice)
            raise ValueError("b must be a device tensor on the same GPU as x_init (%s), got %s"
                             % (self.device, b.device if isinstance(b, torch.Tensor) else type(b).__name__))
        self.A, self.AT = A, AT
        # fused (round 3): the TV part as ONE sweep over q (tv_cpop_fused + tv_cpop_fixup: the one-sweep Chambolle-Pock kernel with
        # A^T p in the place of the fidelity dual) instead of tv_cp_dual + tv_DT_axpy2 -- 2 Nd + 4 words per voxel instead of 3 Nd + 4
        can_fuse = bool(self.lib.tv_cp_fused_supported(self.geo.ref))
        if fused and not can_fuse:
            raise ValueError("fused=True needs a geometry tv_cp_fused_supported() accepts")
        self.fused = can_fuse if fused is None else bool(fused)
        self.reg = float(regularization)
        self.sigma_D, self.sigma_A = float(sigma_D), float(sigma_A)
        self.tau = float(tau) if tau is not None else cp_step_size(self.slab.nz_global, x_init.shape[1], reg_z_over_reg, reg_time,
                                                                    self.geo.time_weight_max)
        self.x = self.x0.clone()
        self.b = b.to(self.dtype).contiguous()
        self.p = torch.zeros_like(self.b)
        self.q = torch.zeros(self.geo.grad_shape, dtype=self.dtype, device=self.device)
        self.ws = self.geo.workspace()              # allocated before x_new, as it always was (``_bind_loop_buffers`` binds the same one)
        self.x_new = torch.empty_like(self.x)
        self._bind_loop_buffers()
        # the residual r = A x - b is CARRIED from one iteration to the next (round 2 applied A twice per iteration: once
        # for the dual update, once more for the loss of the new iterate -- the next iteration's first residual)
        self.r = torch.empty_like(self.b)
        self.n_A = self.n_AT = 0          # calls of the user's operators (tests assert one of each per iteration)
        if isinstance(norm_A, str) and norm_A != "estimate":
            raise ValueError("norm_A must be None, a number (|A|) or 'estimate'")
        self.norm_A_sq = None
        if norm_A is not None:
            if isinstance(norm_A, str):
                self.norm_A_sq = operator_norm_sq(self._count_A, self._count_AT, self.x, n_iter=self.NORM_ITER, slab=self.slab)
            else:
                self.norm_A_sq = float(norm_A) ** 2
            if not (self.norm_A_sq >= 0.0) or self.norm_A_sq == float("inf"):
                raise ValueError("norm_A must be a finite number >= 0 (estimate: A^T A v came out non-finite)")
            if tau is None:
                L = normal_spectral_bound(scheme, self.slab.nz_global, x_init.shape[1], reg_z_over_reg, reg_time, self.geo.time_weight_max)
                self.tau = 1.0 / (self.sigma_A * self.norm_A_sq + self.sigma_D * L)
        self._fid0 = torch.zeros((), dtype=torch.float64, device=self.device)
        self._residual(self.x, self._fid0)
        # calls the constructor made (the starting residual, the power iteration): n_A - n_A_setup == n_AT - n_AT_setup == iterations done
        self.n_A_setup, self.n_AT_setup = self.n_A, self.n_AT
        # optimality residual (``residuals``): the TV block of the starting triple is enqueued here, so that R_0 is that of the initial
        # triple whenever ``run_until`` is called; read back (one synchronisation) only when somebody asks
        self._steps = 0                   # step() calls: afterwards x_new holds the iterate the last step started from
        self._res_scr = None              # data-space scratch of ``residuals``
        self._res0 = self._residual_scalars(dual_zero=True)
        self._R0 = None

    def _count_A(self, v):
        self.n_A += 1
        return self._apply(self.A, v, self.b.shape, "A(x)")

    def _count_AT(self, v):
        self.n_AT += 1
        return self._apply(self.AT, v, self.x.shape, "AT(p)")

    def _apply(self, op, v, shape, what):
        out = op(v)
        if tuple(out.shape) != tuple(shape) or out.dtype != self.dtype or not out.is_cuda:
            raise ValueError("%s must return a device tensor of shape %s and dtype %s, got %s %s on %s"
                             % (what, tuple(shape), self.dtype, tuple(out.shape), out.dtype, out.device))
        return out if out.is_contiguous() else out.contiguous()

    def _residual(self, x, fid_slot):
        """r <- A x - b, fid_slot <- 1/2 |r|^2 (this rank's share): one call of A, one HIP kernel."""
        ax = self._apply(self.A, x, self.b.shape, "A(x)")
        self.n_A += 1
        _nv.check(self.lib.tv_cpop_residual(_nv.dtype_code(self.dtype), self.b.numel(), _nv.ptr(ax), _nv.ptr(self.b), _nv.ptr(self.r),
                                            fid_slot.data_ptr(), _nv.ptr(self.ws), self.stream))

    def step(self, out):
        """out: fp64 device tensor [tv, fid] of this rank: tv = |D x|_{2,1} of the iterate the step started from, fid =
        1/2 |A x_new - b|^2 of the one it produced (the mix the reference's loss line uses, README.md:157).
        One call of A and one of A^T per iteration; every update of ours is a HIP kernel on preallocated buffers:
            tv_cpop_p        p <- (p + sigma_A r) / (1 + sigma_A)
            tv_cp_dual       q <- proj(q + sigma_D D x), TV
            tv_DT_axpy2      x_new <- x - tau A^T p - tau D^T q          (one pass: q, x and A^T p read once)
            tv_cpop_residual r <- A x_new - b, fidelity"""
        g, s = self.geo, self.slab
        h = self.plan.exchange_image(self.x, self.xh_prev, self.xh_next)      # in flight while the data-space update runs
        _nv.check(self.lib.tv_cpop_p(_nv.dtype_code(self.dtype), self.p.numel(), _nv.ptr(self.p), _nv.ptr(self.r), self.sigma_A, self.stream))
        if self.fused:
            # one sweep: A^T p first (the user's operator runs while the x halos travel), then dual + primal update in one pass
            # over q, the q' halos, the fix-up
            atp = self._apply(self.AT, self.p, self.x.shape, "AT(p)")
            self.n_AT += 1
            s.wait(h)
            _nv.check(self.lib.tv_cpop_fused(g.ref, _nv.ptr(self.x), _nv.ptr(self.xh_prev), _nv.ptr(self.xh_next), _nv.ptr(self.q),
                                             _nv.ptr(atp), _nv.ptr(self.x_new), self.sigma_D, self.reg, self.tau, 0, -1,
                                             out[0:1].data_ptr(), _nv.ptr(self.ws), self.stream))
            h = self.plan.exchange_grad(self.q, _plane0(self.qh_prev), _plane0(self.qh_next))
            s.wait(h)
            _nv.check(self.lib.tv_cpop_fixup(g.ref, _nv.ptr(self.q), _nv.ptr(self.qh_prev), _nv.ptr(self.qh_next), _nv.ptr(self.x_new),
                                             self.tau, 0, -1, _nv.ptr(self.ws), self.stream))
            self.x, self.x_new = self.x_new, self.x
            self._residual(self.x, out[1:2])
            self._steps += 1
            return
        s.wait(h)
        _nv.check(self.lib.tv_cp_dual(g.ref, _nv.ptr(self.x), _nv.ptr(self.xh_prev), _nv.ptr(self.xh_next), _nv.ptr(self.q),
                                      self.sigma_D, self.reg, out[0:1].data_ptr(), _nv.ptr(self.ws), self.stream))
        h = self.plan.exchange_grad(self.q, _plane0(self.qh_prev), _plane0(self.qh_next))
        atp = self._apply(self.AT, self.p, self.x.shape, "AT(p)")             # the user's operator runs while the q halos travel
        self.n_AT += 1
        s.wait(h)
        _nv.check(self.lib.tv_DT_axpy2(g.ref, _nv.ptr(self.q), None, _nv.ptr(self.qh_prev), _nv.ptr(self.qh_next), _nv.ptr(self.x),
                                       _nv.ptr(atp), -self.tau, -self.tau, _nv.ptr(self.x_new), self.stream))
        self.x, self.x_new = self.x_new, self.x
        self._residual(self.x, out[1:2])
        self._steps += 1

    def run(self, n_iter):
        hist = torch.zeros((int(n_iter), 2), dtype=torch.float64, device=self.device)
        for it in range(hist.shape[0]):
            self.step(hist[it])
        self.slab.allreduce_sum_(hist)
        h = hist.cpu().numpy()
        return h[:, 1] + self.reg * h[:, 0]

    # ---- optimality residual of the saddle problem (tv_cp_dual_residual) ---------------------------------------------------------------
    _RES_DOC = """One ``step`` takes the triple (x, p, q) to
            p+ = (p + sigma_A (A x - b)) / (1 + sigma_A),   q+ = proj_{|.|_2 <= reg}(q + sigma_D D x),   x+ = x - tau (A^T p+ + D^T q+)
        and a triple is a saddle point of  min_x max_{p, |q| <= reg}  <A x - b, p> - 1/2 |p|^2 + <D x, q>  (whose x solves the problem) iff
        A^T p + D^T q = 0, p = A x - b and q = proj(q + s D x) for one (equivalently every) s > 0.  The residual R = R_x + R_p + R_q:
            R_x = |A^T p + D^T q|^2                              after a step: |x_before - x|^2 / tau^2 (one 2-word distance pass, no D^T)
            R_p = |p - (A x - b)|^2                              two data-space vectors the solver carries
            R_q = |q - proj(q + sigma_D D x)|^2 / sigma_D^2      the prox-gradient residual of the TV block: tv_cp_dual_residual, Nd + 1
                                                                 words per voxel, what the next dual update would change, summed per site
        R = 0 exactly at a saddle point, and nothing in it calls A or A^T.  fp32: R_x is a difference of iterates, resolved down to about
        (eps_fp32 |x| / tau)^2 per voxel."""

    def _residual_scalars(self, dual_zero=False):
        """fp64 device words [|D x|_{2,1}, R_q, |x_before - x|^2 (or R_x itself before any step), R_p, 1/2 |A x - b|^2] of the current
        triple on this rank; kernels and reductions are enqueued, nothing waits for them.  Touches the halo buffers (refilled by every
        step before it reads them), the workspace and -- before the first step only -- x_new, never x, p, q or r.
        dual_zero: the caller knows p = q = 0 (the constructor)."""
        out = torch.zeros(5, dtype=torch.float64, device=self.device)
        g, s, pl = self.geo, self.slab, self.plan
        s.wait(pl.exchange_image(self.x, self.xh_prev, self.xh_next))
        _nv.check(self.lib.tv_cp_dual_residual(g.ref, _nv.ptr(self.x), _nv.ptr(self.xh_prev), _nv.ptr(self.xh_next), _nv.ptr(self.q), self.sigma_D,
                                               self.reg, out[0:2].data_ptr(), _nv.ptr(self.ws), self.stream))
        if self._steps > 0:
            # x_new holds the iterate the last step started from: the distance alone (out = NULL: nothing is stored)
            _nv.check(self.lib.tv_axpby(g.ref, 1.0, _nv.ptr(self.x), 0.0, None, _nv.ptr(self.x_new), None, out[2:3].data_ptr(), _nv.ptr(self.ws),
                                        self.stream))
            p_zero = False
        else:
            # no previous x: p = q = 0 (what the constructor leaves) gives R_x = 0 without a call; a caller who has put a dual
            # start into p / q pays one A^T and one D^T here (x_new is free before the first step)
            p_zero = dual_zero or not bool(self.p.any())
            if not (dual_zero or (p_zero and not bool(self.q.any()))):
                atp = self._count_AT(self.p)
                self.n_AT_setup += 1
                s.wait(pl.exchange_grad(self.q, _plane0(self.qh_prev), _plane0(self.qh_next)))
                _nv.check(self.lib.tv_DT_axpy(g.ref, _nv.ptr(self.q), None, _nv.ptr(self.qh_prev), _nv.ptr(self.qh_next), _nv.ptr(atp), 1.0,
                                              _nv.ptr(self.x_new), self.stream))
                out[2] = torch.linalg.vector_norm(self.x_new, dtype=torch.float64) ** 2
        if p_zero:
            out[3] = torch.linalg.vector_norm(self.r, dtype=torch.float64) ** 2
        else:
            if self._res_scr is None:
                self._res_scr = torch.empty_like(self.r)
            torch.sub(self.p, self.r, out=self._res_scr)
            out[3] = torch.linalg.vector_norm(self._res_scr, dtype=torch.float64) ** 2
        out[4] = 0.5 * torch.linalg.vector_norm(self.r, dtype=torch.float64) ** 2
        return out

    def _residual_dict(self, out, stepped):
        self.slab.allreduce_sum_(out)                    # the five scalars in one call
        tv, rq, dx, rp, fid = (float(v) for v in out.cpu().tolist())
        rx = dx / (self.tau * self.tau) if stepped else dx
        return {"x": rx, "p": rp, "q": rq, "total": rx + rp + rq, "tv": tv, "fid": fid}

    def residuals(self):
        """{"x": R_x, "p": R_p, "q": R_q, "total": R, "tv": |D x|_{2,1}, "fid": 1/2 |A x - b|^2} of the current triple as Python floats,
        between ``step`` / ``run`` calls.  Leaves x, p, q, r and the counters n_A / n_AT as they are (the one exception: asked before
        the first step with a p or q the caller has made non-zero, R_x costs one A^T).  One host synchronisation.  Sharded: collective,
        every rank calls it and gets the same numbers.
        """
        return self._residual_dict(self._residual_scalars(), self._steps > 0)
    residuals.__doc__ += _RES_DOC

    def initial_residual(self):
        """R_0: ``residuals()["total"]`` of the triple the constructor left (enqueued there, read back on the first call)."""
        if self._R0 is None:
            self._R0 = self._residual_dict(self._res0, False)
        return self._R0["total"]

    def run_until(self, rel_res, max_iter, check_every=10):
        """Iterate until the residual has dropped by the factor asked for: ``run`` in blocks of ``check_every`` iterations, stopping at the
        first check where R_k <= rel_res**2 * R_0, or after ``max_iter`` iterations.  R_0 is the residual of the triple the constructor
        left (x_init, p = q = 0); R_0 == 0 (a saddle point already) returns at once with ``converged=True``.
        ``rel_res`` is RELATIVE TO THE STARTING POINT: the same number means a different accuracy from a different ``x_init`` -- a good
        start has a small R_0 and is asked for more.  Compare ``residuals()["total"]`` itself across runs.
        Returns (loss_history, info); info: ``iterations``, ``converged``, ``residuals`` (the last ``residuals()`` dict), ``initial`` = R_0 and
        ``relative`` = sqrt(R_k / R_0).  A check costs one Nd + 1-word pass, one 2-word distance pass and three data-space reductions: no
        call of A / A^T, and no host synchronisation between checks.  Both paths (``fused=True`` / ``False``).
        """
        return self._run_until_residual(rel_res, max_iter, check_every)
    run_until.__doc__ += _RES_DOC


# =================================================================================================
class SubgradientDescent(_SlabProblem):
    """README.md:118-124 with the state on the GPU: x <- x - step ((x - x0) + reg * G(x)).

    Per-step scalars: ``SLOTS`` fp64 device words, TV parts in [0:3], fidelity parts in [3:6] (one slot per launch:
    interior planes, first two planes, last two planes when the halo exchange is overlapped)."""

    SLOTS = 6
    HALO_PLANES = 2     # the sub-gradient of a site reads x two planes away

    @classmethod
    def loss_from_slots(cls, h, regularization):
        return h[:, 3:6].sum(axis=1) + regularization * h[:, 0:3].sum(axis=1)

    def __init__(self, x0, regularization, step_size, scheme="hybrid", reg_z_over_reg=1.0, reg_time=0.0,
                 mask_static=False, factor_reg_static=0, slab=None, one_pass=None, overlap=True, pitch="auto", tune_placement=None,
                 persistent=None):
        """tune_placement: None = on for one-pass problems (slabs) of >= 4 GiB per image with memory to spare (``_tune_placement``).
        persistent (round 6): None = volumes of at most ``SMALL_MAX_VOXELS`` on one GPU run ``run`` as ONE launch per ``SMALL_BLOCK``
        iterations (tv_small_subgrad_descent: tv_subgrad + tv_subgrad_step's arithmetic inside a persistent kernel); False / True."""
        super().__init__(x0, scheme, reg_z_over_reg, reg_time, mask_static, factor_reg_static, slab, pitch=pitch)
        self.reg, self.step_size = float(regularization), float(step_size)
        # (an explicit one_pass=True / False asks for that kernel family: the persistent loop replaces it only when it is asked for as well)
        self.small = self._small_ok(False if (one_pass is not None and persistent is None) else persistent)
        self.x = self.image_copy(self.x0)
        nz, m, ny, nx = self.x0.shape
        self.G = self.new_image()
        if one_pass is None:      # TV + G + step in one pass over x wherever the geometry allows (tv_subgrad_step_fused)
            one_pass = bool(self.lib.tv_subgrad_fused_supported(self.geo.ref))
            # the one-pass kernel folds the step into its store (it divides by step * reg): a vanishing product takes the two-pass path
            # (until round 5 the round-1 kernel took that corner for fp32; it lives in csrc/variants/ now)
            if self.step_size * self.reg < 1e-6:
                one_pass = False
        self.one_pass = bool(one_pass)
        # one pass: TV, G and the descent step in a single kernel, x ping-ponged (G is never stored); else the
        # two-pass tv_subgrad + tv_subgrad_step
        self.norms_ext = None if (self.one_pass and not self.small) else self.geo.new_image(nz + 2)
        if self.one_pass:
            self.x_alt = self.G
            self.G = None
        elif self.small:
            self.x_alt = self.new_image()           # the persistent loop ping-pongs the iterate
        self.ws = self.geo.workspace()
        self.plan = HaloPlan(self.slab, scheme, self.geo.z_active)
        sh = self.plan.on           # (with two halo planes per neighbour every rank holds >= 2 planes: ``_refuse_thin_slabs``)
        self.xh_prev = self.new_plane(2) if sh and self.slab.prev is not None else None
        self.xh_next = self.new_plane(2) if sh and self.slab.next is not None else None
        self.sh = sh
        # interior-first schedule (one-pass kernel: x is ping-ponged, so the planes being sent are never written while
        # the exchange is in flight): planes [2, nz - 2) need no halo and hide the two-plane exchange
        self.overlap = bool(overlap) and sh and self.one_pass and nz >= 5
        self._scratch = torch.zeros(self.SLOTS, dtype=torch.float64, device=self.device)
        self.placement = None
        if self.one_pass:
            self._pp_tune(tune_placement, True, ("x", "x_alt", "x0"), self._tune_placement)

    def _tune_placement(self, n_extra=2, reps=2):
        """Pick where the two image buffers of the x ping-pong (and x0) live by MEASUREMENT, as ``ChambollePock._tune_x_placement``
        does and for the same reason (the time of a streaming kernel depends on where its arrays landed
        in physical memory, per allocation and per direction of the ping-pong; the descent loop on the north-star volume runs at
        128 - 149 it/s from process to process with the same binary).  Every ordered pair of 2 + ``n_extra`` candidates is timed with
        the real kernel; then the caller's x0 against a copy in a buffer that is left.  ~30 steps once per solver; the iterate is
        re-initialised afterwards, results do not depend on it."""
        import time as _time
        t_begin = _time.perf_counter()
        nz = self.slab.nz
        out = torch.zeros(self.SLOTS, dtype=torch.float64, device=self.device)

        def launch():
            self._one_pass_range(0, nz, self.xh_prev, self.xh_next, out[0:1], out[3:4])

        x_a, x_b = self.x, self.x_alt
        for _ in range(2):                                                   # warm-up (code load, clocks)
            self._pp_one(launch, x_a, x_b)
        cands = [x_a, x_b] + [self.new_image() for _ in range(n_extra)]
        for c in cands[1:]:
            c.copy_(self.x0)                                                 # every candidate holds data of the problem's kind (no denormals, no NaN)
        ms, (bi, bj), chosen_ms, first_ms = self._pp_pairs(launch, cands, reps)
        info = {"candidates": len(cands), "step_ms": ms, "chosen": [bi, bj], "chosen_ms": chosen_ms, "first_pair_ms": first_ms}
        x_a, x_b = cands[bi], cands[bj]
        spare = [c for k, c in enumerate(cands) if k not in (bi, bj)]
        del cands
        if spare:
            info["x0_round_trip_ms"] = self._pp_x0(launch, x_a, x_b, spare[0], reps)
        del spare
        self.x, self.x_alt = x_a, x_b
        self._reset_state()
        torch.cuda.synchronize(self.device)
        torch.cuda.empty_cache()
        info["seconds"] = round(_time.perf_counter() - t_begin, 3)
        self.placement = info

    def _one_pass_range(self, a, b, hp, hn, tv_slot, fid_slot):
        g, x = self.geom(a, b), self.x
        _nv.check(self.lib.tv_subgrad_step_fused(g.ref, _nv.ptr(x[a:b]), _nv.ptr(hp), _nv.ptr(hn), _nv.ptr(self.x0[a:b]),
                                                 _nv.ptr(self.x_alt[a:b]), self.step_size, self.reg, tv_slot.data_ptr(),
                                                 fid_slot.data_ptr(), _nv.ptr(self.ws), self.stream))

    def step(self, out=None):
        """Enqueue one iteration; out: fp64 device tensor of SLOTS words (TV parts [0:3], fidelity parts [3:6])."""
        out = self._scratch if out is None else out
        nz, s, x = self.slab.nz, self.slab, self.x
        h = self.plan.exchange_image2(x, self.xh_prev, self.xh_next)
        if self.one_pass:
            if self.overlap:
                self._one_pass_range(2, nz - 2, x[0:2], x[nz - 2:nz], out[0:1], out[3:4])
                s.wait(h)
                self._one_pass_range(0, 2, self.xh_prev, x[2:4], out[1:2], out[4:5])
                self._one_pass_range(nz - 2, nz, x[nz - 4:nz - 2], self.xh_next, out[2:3], out[5:6])
            else:
                s.wait(h)
                self._one_pass_range(0, nz, self.xh_prev, self.xh_next, out[0:1], out[3:4])
            self.x, self.x_alt = self.x_alt, self.x
            return
        s.wait(h)
        g = self.geo
        _nv.check(self.lib.tv_subgrad(g.ref, _nv.ptr(x), _nv.ptr(self.xh_prev), _nv.ptr(self.xh_next), _nv.ptr(self.G),
                                      _nv.ptr(self.norms_ext), out[0:1].data_ptr(), _nv.ptr(self.ws), self.stream))
        _nv.check(self.lib.tv_subgrad_step(g.ref, _nv.ptr(x), _nv.ptr(self.x0), _nv.ptr(self.G), self.step_size, self.reg,
                                           out[3:4].data_ptr(), _nv.ptr(self.ws), self.stream))

    GRAPH_BLOCK = 10            # iterations captured per hipGraph (even: the x ping-pong returns to its start)
    GRAPH_MAX_VOXELS = 1 << 23  # below this an iteration is launch-bound (a few tens of microseconds of kernels)

    def run(self, n_iter, graph=None):
        """n_iter iterations; returns the README's loss history (README.md:124).  graph: None = replay blocks of
        GRAPH_BLOCK iterations from a hipGraph when the problem is small enough to be launch-bound and not sharded
        (the README's own 2-D example is), True / False force it."""
        hist = torch.zeros((n_iter, self.SLOTS), dtype=torch.float64, device=self.device)
        if self.small and graph is None:
            self._run_small(hist)
            self._small_check()
            return self.loss_from_slots(hist.cpu().numpy(), self.reg)
        use_graph = (self.x0.numel() <= self.GRAPH_MAX_VOXELS) if graph is None else bool(graph)
        for it in range(self._run_graphed_head(hist, use_graph), n_iter):
            self.step(hist[it])
        self.slab.allreduce_sum_(hist)
        return self.loss_from_slots(hist.cpu().numpy(), self.reg)

    def _run_small(self, rows):
        """``len(rows)`` descent steps in blocks of ``SMALL_BLOCK`` per cooperative launch (tv_small_subgrad_descent); TV(x_k) -> slot 0,
        1/2 |x_{k+1} - x0|^2 -> slot 3.  The iterate is ping-ponged: after an odd block x and x_alt trade places."""
        ws = self._small_ws()

        def launch(k, row_ptr):
            _nv.check(self.lib.tv_small_subgrad_descent(self.geo.ref, _nv.ptr(self.x), _nv.ptr(self.x_alt), _nv.ptr(self.x0), _nv.ptr(self.norms_ext),
                                                        self.step_size, self.reg, k, row_ptr, rows.stride(0), 3, _nv.ptr(ws), self.stream))
            if k & 1:
                self.x, self.x_alt = self.x_alt, self.x

        self._small_blocks(rows, launch)

    _ROLES = ("x", "x_alt")         # (x_alt: the one-pass kernel and the persistent loop only)


# =================================================================================================
class ADMM(_SlabProblem):
    """Scaled-form ADMM for min 1/2|x-x0|^2 + reg |z|_{2,1} s.t. Dx = z  (the
    reference names ADMM, README.md:26,135, but ships no code -- parity is pinned against
    oracle/tv_oracle.py::admm and, op by op, against the reference's D / D^T).

      x-step : (I + rho D^T D) x = x0 + rho D^T (z - u)   n_cg CG steps, warm start
      z-step : z = shrink(Dx + u, reg/rho);  u-step: u += Dx - z          (one fused kernel)

    single_reduction (default): the CG recurrence in its Chronopoulos-Gear form -- w = A r, gamma = <r,r> and
    delta = <r,w> come out of ONE kernel and are all-reduced together (one collective of two scalars per CG step instead
    of two collectives), the four vector updates are one kernel, the residual of the warm start and the loss of the
    outer iteration are fused into the kernels that read those vectors anyway, and the dual pair is kept as
    (t = z - u, u) so that the right-hand side reads one gradient array: 4 Nd + 11 n_cg + 5 words per voxel and outer
    iteration instead of 5 Nd + 11 n_cg + 17 (76 instead of 92 for Nd = 4, n_cg = 5).  ``single_reduction=False`` is the
    textbook recurrence of round 1 (tv_cg_step1 / tv_cg_step2).  Both are the same iteration in exact arithmetic;
    oracle.admm restates both.

    DEFAULTS THAT CHANGED IN ROUND 4 (existing callers get different -- equally valid -- iterates): ``x_solver=None`` runs the x-solve
    as ``n_cg`` Chebyshev steps instead of CG (same objective to 6 - 7 digits at every outer iteration, profiles/
    r4_admm_xsolve_study_f32.txt; ``x_solver="cg"`` is the old behaviour), ``keep_z=True`` stores every sample of t' so that ``.z`` works on
    the one-sweep path (``keep_z=False`` moves Nd fewer words per voxel), and ``pitch="auto"`` pads ragged rows: ``.x`` is then a strided
    view of padded storage, ``result()`` a dense copy."""

    HALO_PLANES = 2     # the normal operator D^T D of a site reads x two planes away

    def __init__(self, x0, regularization, rho, n_cg=10, scheme="hybrid", reg_z_over_reg=1.0, reg_time=0.0,
                 mask_static=False, factor_reg_static=0, slab=None, single_reduction=True, fused=None, keep_z=True, x_solver=None,
                 pitch="auto", tune_placement=None, persistent=False):
        """tune_placement: None = on for unsharded problems whose state is >= 16 GiB with room for a second copy (``_tune_placement``).
        persistent (round 7): True = ``run`` goes through ``SMALL_BLOCK`` outer iterations per cooperative launch (tv_small_admm: the
        Chebyshev x-solve and the z / u update inside a persistent kernel, csrc/tv_small.hip) -- for unsharded volumes tv_small_supported
        accepts, single_reduction, the Chebyshev x-solve, n_cg in 1 .. 32; it selects the non-fused state convention (x, t = z - u, u), so
        ``step`` / ``.x`` / ``.u`` / ``.z`` / ``result()`` work as on the ordinary non-fused path and can be mixed with ``run``.
        False (the default) = the ordinary kernels; there is no automatic rule."""
        super().__init__(x0, scheme, reg_z_over_reg, reg_time, mask_static, factor_reg_static, slab, pitch=pitch)
        self.reg, self.rho, self.n_cg = float(regularization), float(rho), int(n_cg)
        self.single = bool(single_reduction)
        # x_solver="chebyshev" (round 3): n_cg steps of the Chebyshev iteration on (I + rho D^T D) e = b - A x instead of CG.  Its
        # scalars follow from the spectral interval [1, 1 + rho L] alone, so a step is ONE streaming kernel (tv_cheb_step: e_k with
        # its stencil, r0 and e_{k-1} read, e_{k+1} written -- 4 words per voxel where a CG step moves 11) and a sharded solve
        # exchanges halo planes only: no all-reduce.  Same convergence as CG on this operator within the digits the loss is
        # reported to (the spectrum of D^T D fills its interval); oracle.admm(x_solver="chebyshev") restates it.
        # DEFAULT since round 4 (x_solver=None): Chebyshev wherever it applies (single_reduction, n_cg > 0), CG otherwise.  Measured on
        # the configs[4] per-GPU slab, 50 outer iterations, four schemes, rho in {0.02, 0.05, 0.2}, fp32 and fp64
        # (tools/archive/admm_xsolve_study.py, profiles/r4_admm_xsolve_study_*.txt): with the same number of steps the two reach the same
        # objective to 6 - 7 digits at EVERY outer iteration, and a Chebyshev outer iteration takes 12.8 - 16.3 ms where CG takes
        # 27 - 33 (fp64: 15 - 21 against 29 - 37): 2.1 - 2.4 x less wall time to any objective level, no all-reduce in the solve.
        # ``n_cg`` keeps its meaning: steps of the x-solve per outer iteration.  x_solver="cg" is the round-1..3 behaviour.
        x_solver_asked = x_solver
        if x_solver is None:
            x_solver = "chebyshev" if (self.single and self.n_cg > 0) else "cg"
        if x_solver not in ("cg", "chebyshev"):
            raise ValueError("x_solver must be None (the default since round 4: 'chebyshev' wherever it applies, i.e. single_reduction and "
                             "n_cg > 0), 'cg' (the behaviour of rounds 1 - 3) or 'chebyshev'")
        self.cheb = (x_solver == "chebyshev")
        if self.cheb and not (self.single and self.n_cg > 0):
            raise ValueError("x_solver='chebyshev' needs single_reduction=True (the default) and n_cg > 0")
        L = normal_spectral_bound(scheme, self.slab.nz_global, x0.shape[1], reg_z_over_reg, reg_time, self.geo.time_weight_max)
        self._cheb_coef = chebyshev_coefficients(1.0 + self.rho * L, self.n_cg) if self.cheb else None
        # one-sweep dual side (round 3): z / u update + the residual of the next x-solve in one pass over u
        # (tv_admm_sweep + tv_admm_fixup: 2 Nd + 3 words per voxel instead of the 4 Nd + 6 of tv_admm_tu + tv_DT_axpy +
        # tv_normal_op2).  keep_z=True (default since round 4: ``.z`` keeps working as it did before the one-sweep path existed): round 5
        # keeps a SECOND u array instead of every sample of t' -- u is ping-ponged and z = shrink(D x + u_old) is rebuilt when ``.z`` is
        # asked for, so the sweep moves the same 2 Nd + 3 words as with keep_z=False (round 4: 3 Nd + 3); keep_z=False saves the memory
        # of that array -- the split variable z is then not recoverable and ``.z`` raises, naming this flag.
        can_fuse = self.single and self.n_cg > 0 and bool(self.lib.tv_cp_fused_supported(self.geo.ref))
        if fused and not can_fuse:
            raise ValueError("fused=True needs single_reduction, n_cg > 0 and a geometry tv_cp_fused_supported() accepts")
        self.fused = can_fuse if fused is None else bool(fused)
        self.small = False
        if persistent:
            if x_solver_asked == "cg" or not self.cheb:
                raise ValueError("persistent=True runs the Chebyshev x-solve (x_solver=None or 'chebyshev', single_reduction=True, n_cg >= 1): "
                                 "CG needs a grid-wide dot product per step")
            if fused:
                raise ValueError("persistent=True keeps the non-fused state convention (x, t, u): fused=True cannot be combined with it")
            if self.n_cg > self.SMALL_MAX_CHEB:
                raise ValueError("persistent=True: at most %d Chebyshev steps per outer iteration (n_cg)" % self.SMALL_MAX_CHEB)
            self.small = self._small_ok(True)       # raises for a sharded slab / a volume outside tv_small_supported
            self.fused = False
        self._small_grad = None
        self.keep_z = bool(keep_z)
        self._have_r = False
        self.x = self.image_copy(self.x0)
        self._zt = self.new_grad()                   # z, or t = z - u (single_reduction)
        self.u = self.new_grad()
        # round 5: on the one-sweep path keep_z costs MEMORY, not traffic -- u is ping-ponged (tv_admm_sweep reads u, writes u_alt, the roles
        # swap), so z = shrink(D x + u_old) can be rebuilt whenever ``.z`` is asked for and the sweep stores t' sparsely as with
        # keep_z=False: 2 Nd + 3 words per voxel instead of 3 Nd + 3 (round 4 stored every sample of t' = z - u - D x)
        self.u_alt = self.new_grad() if (self.fused and self.keep_z) else None
        self.b = self.new_image()
        self.r = self.new_image()
        self.d = self.new_image()
        self.Ad = self.new_image()                   # A d (textbook) / s = A d (single reduction)
        self.ws = self.geo.workspace()
        self.plan = HaloPlan(self.slab, scheme, self.geo.z_active)
        pl, s_ = self.plan, self.slab
        sh = pl.on                  # (with two halo planes per neighbour every rank holds >= 2 planes: ``_refuse_thin_slabs``)
        self.sh = sh
        self.h2_prev = self.new_plane(2) if sh and s_.prev is not None else None
        self.h2_next = self.new_plane(2) if sh and s_.next is not None else None
        self.ch_back, self.ch_fwd = pl.ch_back, pl.ch_fwd
        self.wh_prev = self.new_plane() if pl.g_need_prev else None
        self.wh_next = self.new_plane() if pl.g_need_next else None
        self.ws_prev = self.new_plane() if pl.g_send_prev else None
        self.ws_next = self.new_plane() if pl.g_send_next else None
        self.sc = torch.zeros(4, dtype=torch.float64, device=self.device)   # rs, dAd, rs_new, spare / gamma, delta, gamma_old, alpha_old
        self.dots3 = torch.zeros((3, 2), dtype=torch.float64, device=self.device)
        self.dots = torch.zeros(2, dtype=torch.float64, device=self.device)
        self.rr = torch.zeros(2, dtype=torch.float64, device=self.device)     # <r, r> of the sweep / of the fix-up
        self.timing = None      # set to a list to collect one list of (name, HIP event) per outer iteration (bench.py --solver admm)
        self._marks = None
        self.placement = None
        # (u_alt is a candidate of the tuner too: count it, or `free >= set_bytes + 8 GiB` under-estimates by Nd words -- round-5 advice)
        set_bytes = (sum(getattr(self, k).numel() for k in self._STATE) + (self.u_alt.numel() if self.u_alt is not None else 0)) * self.x.element_size()
        if tune_placement is None:
            free, _total = torch.cuda.mem_get_info(self.device) if self.device.type == "cuda" else (0, 0)
            tune_placement = (not self.slab.sharded) and set_bytes >= (16 << 30) and free >= set_bytes + (8 << 30)
        if tune_placement:
            self._tune_placement()

    _STATE = ("x", "_zt", "u", "b", "r", "d", "Ad")      # the arrays an outer iteration streams through
    _ROLES = ("x", "d", "Ad", "b", "r", "_have_r", "u", "u_alt")

    # ---- what the x-solve of one outer iteration moves (bench.py's roofline_xsolve) ----------------------------------------------
    @property
    def xsolve_words(self):
        """Algorithmic words per voxel of the x-solve of ONE outer iteration (every array a launch touches counted once).
        Chebyshev, K = n_cg steps: e_1 = a0 r is never stored -- e_2 from r alone (2), a step with y = a0 r formed on the fly (3),
        K - 4 plain steps (e_k with its stencil, r, e_{k-1} read; e_{k+1} written: 4) and a last step that adds x (5): 4 K - 6.
        CG (single reduction): normal operator on r (2) + the fused update of four vectors (9) per step."""
        K = self.n_cg
        if self.cheb:
            return 3 if K == 1 else 4 * K - 6
        return 11 * K if self.single else 11 * K + 4

    @property
    def xsolve_launches(self):
        K = self.n_cg
        if self.cheb:
            return 1 if K == 1 else K - 1
        return 2 * K

    @property
    def xsolve_desc(self):
        if self.cheb:
            return ("tv_cheb_step: k_normal_stream<M,TWIN,T,CHEB> (%d launches: e_{k+1} = e_k + alpha (r - (I + rho D^T D) e_k) + beta (e_k - e_{k-1}), "
                    "one streaming pass each)" % self.xsolve_launches)
        return "tv_normal_op2 + tv_cg_update (%d launches)" % self.xsolve_launches

    def _reset_state(self):
        """Back to the state of a fresh solver (x = x0, everything else zero) in the arrays that are bound now."""
        self.x.copy_(self.x0)
        for k in self._STATE[1:]:
            getattr(self, k).zero_()
        if self.u_alt is not None:
            self.u_alt.zero_()
        for t in (self.sc, self.dots3, self.dots, self.rr):
            t.zero_()
        self._have_r = False

    def _tune_placement(self, n_sets=4, n_steps=2):
        """Pick WHERE the state lives by measurement, as ``ChambollePock._tune_x_placement`` does: the same
        outer iteration on the same data takes 17.5 or 19.5 ms on the configs[4] slab depending on where u, t and the image buffers
        landed (tools/archive/admm_placement_probe.py).  ``n_sets`` complete sets of state arrays are allocated one after the other (never
        more than two alive), ``n_steps`` outer iterations are timed on each after one to warm up, the fastest set is kept and put
        back into the initial state.  Unsharded problems only (an outer iteration of a slab waits for its neighbours)."""
        import time as _time
        t_begin = _time.perf_counter()
        out = torch.zeros((n_steps + 1, 2), dtype=torch.float64, device=self.device)

        def timed():
            self._reset_state()
            self.step(out[0])
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(n_steps):
                self.step(out[1 + k])
            b.record()
            torch.cuda.synchronize(self.device)
            return a.elapsed_time(b) / n_steps

        names = self._STATE + (("u_alt",) if self.u_alt is not None else ())

        def bound():                                 # the buffer roles rotate inside a step: take what is bound NOW
            return {k: getattr(self, k) for k in names}

        # the WHOLE tuner is an optimisation, never a failure (round-4 advice: the baseline measurement used to sit outside the try --
        # an out-of-memory error in a halo or Chebyshev temporary there failed the constructor)
        best, best_t, times, info = bound(), float("inf"), [], {}
        try:
            best_t = timed()
            best = bound()
            times.append(round(best_t, 3))
            for _ in range(n_sets - 1):
                cand = dict(x=self.new_image(), _zt=self.new_grad(), u=self.new_grad(), b=self.new_image(), r=self.new_image(),
                            d=self.new_image(), Ad=self.new_image())
                if self.u_alt is not None:
                    cand["u_alt"] = self.new_grad()
                for k, v in cand.items():
                    setattr(self, k, v)
                t = timed()
                times.append(round(t, 3))
                cand = bound()
                if t < best_t:
                    best_t, best = t, cand
                del cand
                for k, v in best.items():            # the loser loses its last reference here
                    setattr(self, k, v)
                torch.cuda.empty_cache()
        except RuntimeError as exc:                  # out of memory while a second set was alive, ...: an optimisation, never a failure
            for k, v in best.items():
                setattr(self, k, v)
            torch.cuda.empty_cache()
            info["error"] = str(exc)[:200]
        self._reset_state()
        torch.cuda.synchronize(self.device)
        info.update({"outer_ms": times, "chosen": times.index(min(times)) if times else None, "seconds": round(_time.perf_counter() - t_begin, 3)})
        self.placement = info

    @property
    def z(self):
        """The split variable z (single_reduction keeps t = z - u: z = t + u; the one-sweep path keeps t' = t - D x and recomputes
        D x -- on a sharded slab that is a halo exchange, so every rank has to ask for z, not just one).
        MEMORY: on the one-sweep path each access allocates two transient gradient-sized arrays (2 Nd words per voxel: z itself and a
        scratch copy of the dual variable) -- 32 GiB at the config4 hybrid slab; they are released when the caller drops z."""
        if self.fused and self._have_r:
            if not self.keep_z:
                raise RuntimeError("ADMM(..., keep_z=False) stores only the samples of z - u - D x its fix-up reads: z is not available; "
                                   "construct the solver with keep_z=True (the default)")
            # rebuilt on demand from x and the dual variable the last sweep READ (u_alt after the swap): z = shrink(D x + u_old)
            z = self.new_grad()
            u_old = self.new_grad()                  # (not .clone(): a clone of a pitched view is dense)
            u_old.copy_(self.u_alt)
            tv_ = torch.zeros(1, dtype=torch.float64, device=self.device)
            hp, hn = self._halo2(self.x)
            _nv.check(self.lib.tv_admm_zu(self.geo.ref, _nv.ptr(self.x), _nv.ptr(hp[1:2] if hp is not None else None),
                                          _nv.ptr(hn[0:1] if hn is not None else None), _nv.ptr(z), _nv.ptr(u_old), self.reg / self.rho,
                                          tv_.data_ptr(), _nv.ptr(self.ws), self.stream))
            return z
        return self._zt + self.u if self.single else self._zt

    def _halo2(self, v):
        self.slab.wait(self.plan.exchange_image2(v, self.h2_prev, self.h2_next))
        return self.h2_prev, self.h2_next

    def _normal_range(self, v, out, a, b, hp, hn, dots, rhs=None, out2=None):
        """out[a:b] = (I + rho D^T D) v (or rhs - that, with a copy in out2) on local planes [a, b); hp / hn: two-plane
        halos of that range; dots: two device words."""
        g = self.geom(a, b)
        _nv.check(self.lib.tv_normal_op2(g.ref, _nv.ptr(v[a:b]), _nv.ptr(hp), _nv.ptr(hn), self.rho,
                                         _nv.ptr(rhs[a:b]) if rhs is not None else None, _nv.ptr(out[a:b]),
                                         _nv.ptr(out2[a:b]) if out2 is not None else None, dots.data_ptr(), _nv.ptr(self.ws),
                                         self.stream))

    def _normal(self, v, out, dots, rhs=None, out2=None, reduce=True):
        """Two-plane halo exchange hidden behind the interior planes, then the operator; dots (2 device words) summed
        over the launches and, with ``reduce``, over the ranks."""
        nz = self.slab.nz
        if self.sh and nz >= 5:
            h = self.plan.exchange_image2(v, self.h2_prev, self.h2_next)
            self._normal_range(v, out, 2, nz - 2, v[0:2], v[nz - 2:nz], self.dots3[0], rhs, out2)
            self.slab.wait(h)
            self._normal_range(v, out, 0, 2, self.h2_prev, v[2:4], self.dots3[1], rhs, out2)
            self._normal_range(v, out, nz - 2, nz, v[nz - 4:nz - 2], self.h2_next, self.dots3[2], rhs, out2)
            torch.sum(self.dots3, dim=0, out=dots)
        else:
            hp, hn = self._halo2(v)
            self._normal_range(v, out, 0, nz, hp, hn, dots, rhs, out2)
        if reduce:
            self.slab.allreduce_sum_(dots)

    def _cheb_range(self, v, y, yscale, add, ref, out, alpha, beta, a, b, hp, hn, dots):
        g = self.geom(a, b)
        sl = lambda t_: _nv.ptr(t_[a:b]) if t_ is not None else None      # noqa: E731
        _nv.check(self.lib.tv_cheb_step(g.ref, _nv.ptr(v[a:b]), _nv.ptr(hp), _nv.ptr(hn), self.rho, _nv.ptr(self.r[a:b]), sl(y), yscale,
                                        sl(add), sl(ref), alpha, beta, _nv.ptr(out[a:b]), dots.data_ptr() if dots is not None else None,
                                        _nv.ptr(self.ws), self.stream))

    def _cheb_step(self, v, y, yscale, add, ref, out, alpha, beta, dots):
        """out = [add +] v + alpha (r - A v) + beta (v - y) on the slab (y None: y = yscale r); the two-plane halo exchange of v hides
        behind the interior planes exactly as in _normal; dots (or None: not wanted) <- [|r - A v|^2, |out - ref|^2 or |v|^2] summed over the
        launches."""
        nz = self.slab.nz
        args = (y, yscale, add, ref, out, alpha, beta)
        if self.sh and nz >= 5:
            h = self.plan.exchange_image2(v, self.h2_prev, self.h2_next)
            d3 = self.dots3 if dots is not None else (None, None, None)
            self._cheb_range(v, *args, 2, nz - 2, v[0:2], v[nz - 2:nz], d3[0])
            self.slab.wait(h)
            self._cheb_range(v, *args, 0, 2, self.h2_prev, v[2:4], d3[1])
            self._cheb_range(v, *args, nz - 2, nz, v[nz - 4:nz - 2], self.h2_next, d3[2])
            if dots is not None:
                torch.sum(self.dots3, dim=0, out=dots)
        else:
            hp, hn = self._halo2(v)
            self._cheb_range(v, *args, 0, nz, hp, hn, dots)

    def _solve_cheb(self, fid_slot):
        """x <- x + e_K, e_K = K Chebyshev steps on A e = r (self.r = b - A x); fid_slot <- |x - x0|^2 (local), or None if the caller
        takes the fidelity from the sweep that follows."""
        g, lib, K, coef = self.geo, self.lib, self.n_cg, self._cheb_coef
        bufs = [self.d, self.Ad, self.b]                  # all free between two solves
        a0 = coef[0][0]
        ref = self.x0 if fid_slot is not None else None
        if K == 1:
            _nv.check(lib.tv_axpby(g.ref, a0, _nv.ptr(self.r), 1.0, _nv.ptr(self.x), _nv.ptr(ref), _nv.ptr(bufs[0]),
                                   fid_slot.data_ptr() if fid_slot is not None else None, _nv.ptr(self.ws) if fid_slot is not None else None,
                                   self.stream))
            last = 0
        else:
            # e_1 = a0 r is never stored: the first kernel forms e_2 = e_1 + alpha_1 (r - A e_1) + beta_1 e_1 from r alone (x = b = r:
            # e_2 = r + a' (r - A r) + b' r), the second one takes y = a0 r on the fly -- 2 + 3 words instead of 2 + 3 + 4
            al1, be1 = coef[1]
            ap = al1 * a0
            bp = a0 + al1 + be1 * a0 - 1.0 - ap
            fin = (K == 2)
            # the dot products of a step (|r - A e_k|^2, |out - x0|^2) are asked for where they are used: by the last step, for the fidelity
            want = lambda fin_: self.dots if (fin_ and ref is not None) else None      # noqa: E731
            self._cheb_step(self.r, None, 0.0, self.x if fin else None, ref if fin else None, bufs[0], ap, bp, want(fin))
            for k in range(2, K):         # e_k lives in bufs[(k - 2) % 3]
                fin = (k + 1 == K)
                alpha, beta = coef[k]
                self._cheb_step(bufs[(k - 2) % 3], bufs[(k - 3) % 3] if k >= 3 else None, a0 if k == 2 else 0.0,
                                self.x if fin else None, ref if fin else None, bufs[(k - 1) % 3], alpha, beta, want(fin))
            if fid_slot is not None:
                fid_slot.copy_(self.dots[1:2])
            last = (K - 2) % 3
        # the new image was written next to the old one: swap the roles (the old x becomes a scratch vector)
        self.x, bufs[last] = bufs[last], self.x
        self.d, self.Ad, self.b = bufs

    def _rhs(self):
        """b = x0 + rho D^T (z - u); the boundary planes of (z - u) travel to the neighbours first."""
        g, lib, s, nz = self.geo, self.lib, self.slab, self.slab.nz
        code, plane = _nv.dtype_code(self.dtype), g.plane
        if self.single:          # the first array IS t = z - u
            h = s.exchange(send_prev=self._zt[0, self.ch_fwd] if self.plan.g_send_prev else None,
                           send_next=self._zt[nz - 1, self.ch_back] if self.plan.g_send_next else None,
                           recv_prev=_plane0(self.wh_prev), recv_next=_plane0(self.wh_next))
            s.wait(h)
            _nv.check(lib.tv_DT_axpy(g.ref, _nv.ptr(self._zt), None, _nv.ptr(self.wh_prev), _nv.ptr(self.wh_next),
                                     _nv.ptr(self.x0), self.rho, _nv.ptr(self.b), self.stream))
            return
        if self.plan.g_send_next:
            _nv.check(lib.tv_sub(code, plane, _nv.ptr(self._zt[nz - 1, self.ch_back]), _nv.ptr(self.u[nz - 1, self.ch_back]),
                                 _nv.ptr(self.ws_next), self.stream))
        if self.plan.g_send_prev:
            _nv.check(lib.tv_sub(code, plane, _nv.ptr(self._zt[0, self.ch_fwd]), _nv.ptr(self.u[0, self.ch_fwd]),
                                 _nv.ptr(self.ws_prev), self.stream))
        s.wait(s.exchange(send_prev=self.ws_prev, send_next=self.ws_next, recv_prev=self.wh_prev, recv_next=self.wh_next))
        _nv.check(lib.tv_DT_axpy(g.ref, _nv.ptr(self._zt), _nv.ptr(self.u), _nv.ptr(self.wh_prev), _nv.ptr(self.wh_next),
                                 _nv.ptr(self.x0), self.rho, _nv.ptr(self.b), self.stream))

    def _zu(self, out_tv):
        """z / u update (needs one x halo plane per side: the two-plane exchange is reused)."""
        g, lib = self.geo, self.lib
        hp, hn = self._halo2(self.x)
        xp = hp[1:2] if hp is not None else None      # plane z0-1
        xn = hn[0:1] if hn is not None else None      # plane z0+nz
        fn = lib.tv_admm_tu if self.single else lib.tv_admm_zu
        _nv.check(fn(g.ref, _nv.ptr(self.x), _nv.ptr(xp), _nv.ptr(xn), _nv.ptr(self._zt), _nv.ptr(self.u),
                     self.reg / self.rho, out_tv.data_ptr(), _nv.ptr(self.ws), self.stream))

    def step(self, out):
        """One outer iteration; out: fp64 device tensor [tv, |x - x0|^2] of this rank."""
        if self.single:
            return self._step_single(out)
        g, lib, s = self.geo, self.lib, self.slab
        code = _nv.dtype_code(self.dtype)
        self._rhs()
        # ---- CG on (I + rho D^T D) x = b, textbook recurrence -----------------------------------------
        rs, dAd, rs_new = self.sc[0:1], self.sc[1:2], self.sc[2:3]
        self._normal(self.x, self.r, self.dots, rhs=self.b, out2=self.d)      # r = d = b - A x, dots[0] = <r, r>
        rs.copy_(self.dots[0:1])
        for _ in range(self.n_cg):
            self._normal(self.d, self.Ad, self.dots)
            dAd.copy_(self.dots[0:1])
            _nv.check(lib.tv_cg_step1(g.ref, _nv.ptr(self.x), _nv.ptr(self.r), _nv.ptr(self.d), _nv.ptr(self.Ad),
                                      rs.data_ptr(), dAd.data_ptr(), rs_new.data_ptr(), _nv.ptr(self.ws), self.stream))
            s.allreduce_sum_(rs_new)
            _nv.check(lib.tv_cg_step2(g.ref, _nv.ptr(self.d), _nv.ptr(self.r), rs_new.data_ptr(), rs.data_ptr(), self.stream))
            rs.copy_(rs_new)
        self._zu(out[0:1])
        # fidelity 1/2 |x - x0|^2 = 1/2 <x-x0, x-x0>: r is free now
        _nv.check(lib.tv_sub(code, g.image_elems, _nv.ptr(self.x), _nv.ptr(self.x0), _nv.ptr(self.r), self.stream))
        _nv.check(lib.tv_dot(g.ref, _nv.ptr(self.r), _nv.ptr(self.r), out[1:2].data_ptr(), _nv.ptr(self.ws), self.stream))

    def _zu_fused(self, out_tv, out_fid=None):
        """z / u update and r = b - A x of the next solve in one sweep + fix-up; gamma = <r, r> (local) into sc[0] -- or, with the
        Chebyshev x-solve (which needs no gamma), |x - x0|^2 of the iterate into out_fid."""
        g, lib, s, nz = self.geo, self.lib, self.slab, self.slab.nz
        hp, hn = self._halo2(self.x)
        xp = hp[1:2] if hp is not None else None      # plane z0-1
        xn = hn[0:1] if hn is not None else None      # plane z0+nz
        u_out = self.u_alt if self.u_alt is not None else self.u          # keep_z: ping-pong (z is rebuilt from the array that was READ)
        _nv.check(lib.tv_admm_sweep(g.ref, _nv.ptr(self.x), _nv.ptr(xp), _nv.ptr(xn), _nv.ptr(self.u), _nv.ptr(u_out), _nv.ptr(self._zt),
                                    _nv.ptr(self.x0), _nv.ptr(self.r), self.reg / self.rho, self.rho,
                                    (2 if out_fid is not None else 0),
                                    0, -1, out_tv.data_ptr(), (out_fid if out_fid is not None else self.rr[0:1]).data_ptr(),
                                    _nv.ptr(self.ws), self.stream))
        if self.u_alt is not None:
            self.u, self.u_alt = self.u_alt, self.u
        self._mark("sweep")
        # the boundary planes of t' travel to the neighbours (as those of t = z - u do in _rhs)
        h = s.exchange(send_prev=self._zt[0, self.ch_fwd] if self.plan.g_send_prev else None,
                       send_next=self._zt[nz - 1, self.ch_back] if self.plan.g_send_next else None,
                       recv_prev=_plane0(self.wh_prev), recv_next=_plane0(self.wh_next))
        s.wait(h)
        _nv.check(lib.tv_admm_fixup(g.ref, _nv.ptr(self._zt), _nv.ptr(self.wh_prev), _nv.ptr(self.wh_next), _nv.ptr(self.r), self.rho,
                                    0, -1, self.rr[1:2].data_ptr(), _nv.ptr(self.ws), self.stream))
        if out_fid is None:
            torch.sum(self.rr, dim=0, keepdim=True, out=self.sc[0:1])
        self._have_r = True

    def _mark(self, name):
        """A HIP event on the launch stream (torch's current stream == the stream the C-ABI enqueues on), only while ``timing`` is a list."""
        if self._marks is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self._marks.append((name, e))

    def _step_single(self, out):
        if self.timing is None:
            return self._step_single_body(out)
        self._marks = []
        self._mark("start")
        self._step_single_body(out)
        self._mark("end")
        self.timing.append(self._marks)
        self._marks = None

    def _step_single_body(self, out):
        g, lib, s = self.geo, self.lib, self.slab
        sc, w, sv = self.sc, self.b, self.Ad          # w = A r lives in b (free once r is formed), s = A d in Ad
        if not (self.fused and self._have_r):
            self._rhs()
            # r = b - A x with gamma = <r, r> (local); then w = A r with delta = <r, w>: ONE all-reduce for the pair
            self._normal(self.x, self.r, self.dots, rhs=self.b, reduce=False)
            sc[0:1].copy_(self.dots[0:1])
        # (one-sweep path: r and gamma were left by the sweep that closed the previous outer iteration)
        if self.cheb:
            if self.fused:      # the sweep that follows reads x and x0 anyway: it returns |x - x0|^2, the solve's last step skips x0
                self._solve_cheb(None)
                self._mark("xsolve")
                self._zu_fused(out[0:1], out[1:2])
            else:
                self._solve_cheb(out[1:2])
                self._zu(out[0:1])
            return
        sc, w, sv = self.sc, self.b, self.Ad          # (b may have been rebound by an earlier Chebyshev solve: take it again)
        self._normal(self.r, w, self.dots, reduce=False)
        sc[1:2].copy_(self.dots[0:1])
        sc[2:4].zero_()                               # alpha_old = 0: first step of this solve
        s.allreduce_sum_(sc[0:2])
        for c in range(self.n_cg):
            last = (c + 1 == self.n_cg)
            _nv.check(lib.tv_cg_update(g.ref, _nv.ptr(self.x), _nv.ptr(self.r), _nv.ptr(self.d), _nv.ptr(sv), _nv.ptr(w),
                                       sc.data_ptr(), _nv.ptr(self.x0) if last else None, out[1:2].data_ptr() if last else None,
                                       _nv.ptr(self.ws), self.stream))
            if last:
                break
            self._normal(self.r, w, self.dots, reduce=False)          # dots = {<r, w>, <r, r>}
            sc[0:1].copy_(self.dots[1:2])
            sc[1:2].copy_(self.dots[0:1])
            s.allreduce_sum_(sc[0:2])
        if self.n_cg == 0:
            out[1:2] = torch.sum((self.x.double() - self.x0.double()) ** 2)     # the slot holds |x - x0|^2: run() halves it
        else:
            out[1:2].mul_(2.0)                        # run() halves: the slot holds |x - x0|^2 like the textbook path
        if self.fused:
            self._zu_fused(out[0:1])
        else:
            self._zu(out[0:1])

    GRAPH_BLOCK = 4             # outer iterations captured per hipGraph
    GRAPH_MAX_VOXELS = 1 << 23  # below this an outer iteration (~10 + 2 n_cg launches) is launch-bound
    SMALL_MAX_CHEB = 32         # Chebyshev steps per outer iteration the persistent kernel takes (csrc/tv_small.hip: kSmallMaxCheb)

    def _small_now(self):
        """the persistent path runs the loop unless somebody asked for per-step events (``timing``)"""
        return self.small and self.timing is None

    def _run_small(self, rows):
        """``len(rows)`` outer iterations in blocks of ``SMALL_BLOCK`` per cooperative launch (tv_small_admm): x, t, u updated in place;
        |D x|_{2,1} -> slot 0, |x - x0|^2 -> slot 1 of every row (the slots ``step`` fills).  r, d, Ad and a gradient array are scratch."""
        import ctypes
        ws = self._small_ws()
        if self._small_grad is None:
            self._small_grad = self.new_grad()
        K = self.n_cg
        alpha = (ctypes.c_double * K)(*[c[0] for c in self._cheb_coef])
        beta = (ctypes.c_double * K)(*[c[1] for c in self._cheb_coef])

        def launch(k, row_ptr):
            _nv.check(self.lib.tv_small_admm(self.geo.ref, _nv.ptr(self.x), _nv.ptr(self.x0), _nv.ptr(self._zt), _nv.ptr(self.u), _nv.ptr(self.r),
                                             _nv.ptr(self.d), _nv.ptr(self.Ad), _nv.ptr(self._small_grad), self.rho, self.reg / self.rho, alpha, beta,
                                             K, k, row_ptr, rows.stride(0), 1, _nv.ptr(ws), self.stream))

        self._small_blocks(rows, launch)

    def run(self, n_outer, graph=None):
        """n_outer outer iterations; returns the loss history.  graph: None = replay blocks of GRAPH_BLOCK outer iterations
        from a hipGraph when the problem is small enough to be launch-bound and not sharded (every scalar of the CG recurrence
        lives on the device, so an outer iteration has no host round trip to break the capture); True / False force it.
        ``persistent=True`` (and no ``timing``): the persistent kernel IS the loop, ``graph`` is not consulted."""
        hist = torch.zeros((n_outer, 2), dtype=torch.float64, device=self.device)
        if self._small_now():
            if n_outer > 0:
                self._run_small(hist)
            self._small_check()
            h = hist.cpu().numpy()
            return 0.5 * h[:, 1] + self.reg * h[:, 0]
        use_graph = (self.x0.numel() <= self.GRAPH_MAX_VOXELS) if graph is None else bool(graph)
        for k in range(self._run_graphed_head(hist, use_graph), n_outer):
            self.step(hist[k])
        self.slab.allreduce_sum_(hist)
        h = hist.cpu().numpy()
        return 0.5 * h[:, 1] + self.reg * h[:, 0]

    def duality_gap(self):
        """(primal, dual, gap) of the current iterate x and the dual variable rho * u as Python floats (u = v - shrink(v, reg / rho) is the
        projection of v onto the ball of radius reg / rho: rho * u is feasible by construction), between ``run`` / ``step`` calls, on every
        path; the state of the loop is not touched.  Sharded: collective, every rank calls it and gets the same numbers.
        """
        return self._gap_certificate(self.x, self.u, self.rho)
    duality_gap.__doc__ += _SlabProblem._GAP_DOC

    def run_until(self, rel_gap, max_outer, check_every=5):
        """Iterate until the answer is certified: ``run`` in blocks of ``check_every`` outer iterations, stopping at the first check where
        gap <= rel_gap * max(|primal|, tiny), or after ``max_outer`` outer iterations.  Returns (loss_history, info); info: ``iterations``,
        ``primal``, ``dual``, ``gap``, ``converged`` and ``error_bound`` = sqrt(2 max(gap, 0)), the bound on |x - x*|_2.
        """
        return self._run_until_gap(rel_gap, max_outer, check_every)
    run_until.__doc__ += _SlabProblem._GAP_DOC
