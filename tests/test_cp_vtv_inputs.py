"""Channel-coupled (vectorial) TV: the float64 NumPy reference of the model -- the joint dual projection, the duality-gap certificate and the
accelerated loop, built on ``oracle.tv_oracle.D`` / ``D_T`` -- and the SHARE CONDITIONS of the inputs that tests/test_gpu_cp_vtv.py hands to
the kernels, checked on that reference alone.  No GPU.

A spatial site s = (z, y, x) carries the M Nd-vector v_s = (q + sigma D x_bar)[z, :, :, y, x]; n_s = |v_s|_F.  The kernel's cases are
    inside      n_s <= lambda                                   v is kept
    outside     n_s >  lambda                                   v is scaled by lambda / n_s
    coupled     n_s >  lambda while at least one frame's own norm |v_s[:, m]|_2 is <= lambda
The third class is the discriminating one: a per-frame projection (tv_cp_dual) leaves such a frame alone, the joint one scales it.  LAM, SIGMA,
XBAR_SPREAD and the radius of q were chosen here, on the reference, so that every class holds at least 2 % of the sites for every (shape,
weighting, scheme) the GPU tests use."""
import functools

import numpy as np
import pytest

from conftest import SCHEMES
from oracle import tv_oracle as orc

LAM = 5.0                      # the radius of the ball
SIGMA = 0.1
XBAR_SPREAD = 10.0             # x_bar uniform in [0, 10): a component of sigma D x_bar has a standard deviation of about 0.4, the joint vector's
                               # norm grows like sqrt(M Nd) -- 0.6 (M = 1, two channels) to 3.3 (M = 16, hybrid) -- against LAM = 5
Q_RADIUS = 1.3                 # |q_s|_F uniform in [0, 1.3 LAM): three quarters of the sites start inside the ball
MIN_SHARE = 0.02

# lanes, M = 2 | scalar rows, M = 3 | one plane, M = 5: register form except hybrid | many frames: generic form | M = 1 | M = 4: the last
# register form of hybrid | M = 8 and 9: the last register form of the other schemes and the first generic one
SHAPES = [(3, 2, 16, 20), (2, 3, 9, 13), (1, 5, 8, 64), (2, 16, 6, 8), (1, 1, 32, 40), (1, 4, 8, 12), (1, 8, 6, 8), (2, 9, 5, 8)]
WEIGHTINGS = ("plain", "mask", "time_factor", "weight_vol", "no_time")
# the volumes that tests/test_gpu_cp_vtv.py cuts into z-ranges (register form, generic form) and the weightings it cuts them under: a
# per-pixel mask that every range shares, and a per-voxel time weight that the ranges cut by planes
Z_SHAPES = [(5, 2, 16, 20), (5, 9, 6, 8)]
Z_WEIGHTINGS = ("plain", "weight_vol", "mask")


def case_kw(name, shape):
    """the four weightings of tests/test_gpu_dual_gap.py (reg_z_over_reg 0.7, reg_time 0.25) and the time channel switched off"""
    rng = np.random.default_rng(17)
    if name == "mask":
        return dict(reg_z_over_reg=0.7, reg_time=0.25, mask_static=rng.random((1, 1) + shape[2:]) < 0.4, factor_reg_static=3.0)
    if name == "time_factor":
        return dict(reg_z_over_reg=0.7, reg_time=0.25, mask_static=(0.25 + 2.0 * rng.random((1, 1) + shape[2:])))
    if name == "weight_vol":
        return dict(reg_z_over_reg=0.7, reg_time=0.25, mask_static=(0.25 + 2.0 * rng.random(shape)))
    if name == "no_time":
        return dict(reg_z_over_reg=0.7, reg_time=0.0)
    return dict(reg_z_over_reg=0.7, reg_time=0.25)


# ------------------------------------------------------------------------------------------------
# the model in fp64
# ------------------------------------------------------------------------------------------------
def site_norm(v):
    """|v_s|_F of a gradient-like array (Nz, Nd, M, Ny, Nx): the norm over channels AND frames, shape (Nz, Ny, Nx)"""
    return np.sqrt(np.sum(v * v, axis=(1, 2)))


def frame_norm(v):
    """|v[:, :, m]|_2 per site of a frame, shape (Nz, M, Ny, Nx): the norm every other solver takes"""
    return np.sqrt(np.sum(v * v, axis=1))


def np_project_joint(v, lam):
    """v where |v_s|_F <= lam, v lam / |v_s|_F beyond: one factor per spatial site"""
    n = site_norm(v)
    return v * np.where(n > lam, lam / np.where(n > 0.0, n, 1.0), 1.0)[:, None, None]


def ref_dual(x, q, sigma, lam, scheme, kw):
    """(q_new, sum_s |D x|_F, v, n_s) in fp64"""
    Dx = orc.D(np.asarray(x, dtype=np.float64), scheme, **kw)
    v = np.asarray(q, dtype=np.float64) + sigma * Dx
    return np_project_joint(v, lam), float(np.sum(site_norm(Dx))), v, site_norm(v)


def ref_gap_parts(x, q, x0, lam, scheme, kw):
    """(|D x|_F per site, 1/2 (x - x0 + D^T q)^2 per voxel, lam |D x|_F - <q, D x> per site, |<q, D x>| per site)"""
    x, q, x0 = (np.asarray(a, dtype=np.float64) for a in (x, q, x0))
    Dx = orc.D(x, scheme, **kw)
    r = x - x0 + orc.D_T(q, scheme, **kw)
    n = site_norm(Dx)
    dot = np.sum(q * Dx, axis=(1, 2))
    return n, 0.5 * r * r, lam * n - dot, np.abs(dot)


def ref_gap(x, q, x0, lam, scheme, kw):
    """(sum_s |D x|_F, 1/2 |x - x0|^2, gap, sum |terms of the gap|) in fp64"""
    n, sq, reg_part, adot = ref_gap_parts(x, q, x0, lam, scheme, kw)
    e = np.asarray(x, dtype=np.float64) - np.asarray(x0, dtype=np.float64)
    return float(np.sum(n)), float(0.5 * np.sum(e * e)), float(np.sum(sq) + np.sum(reg_part)), float(np.sum(sq) + np.sum(lam * n + adot))


def np_vectorial(x0, n_iter, lam, scheme, kw, gamma=1.0, state=None):
    """n_iter iterations of Algorithm 2 (Chambolle & Pock 2011) with the joint projection from ``state`` = (x, x_bar, q, tau, sigma)
    (default: the start); returns (x, loss, state)"""
    x0 = np.asarray(x0, dtype=np.float64)
    if state is None:
        L2 = orc.normal_spectral_bound(scheme, x0.shape, **kw)
        state = (x0.copy(), x0.copy(), np.zeros_like(orc.D(x0, scheme, **kw)), 1.0 / np.sqrt(L2), 1.0 / np.sqrt(L2))
    x, xb, q, tau, sigma = state
    loss = np.zeros(n_iter)
    for k in range(n_iter):
        Dxb = orc.D(xb, scheme, **kw)
        q = np_project_joint(q + sigma * Dxb, lam)
        xn = (x - tau * orc.D_T(q, scheme, **kw) + tau * x0) / (1.0 + tau)
        theta = 1.0 / np.sqrt(1.0 + 2.0 * gamma * tau)
        xb = xn + theta * (xn - x)
        x = xn
        loss[k] = 0.5 * np.sum((x - x0) ** 2) + lam * np.sum(site_norm(Dxb))
        tau, sigma = theta * tau, sigma / theta
    return x, loss, (x, xb, q, tau, sigma)


# ------------------------------------------------------------------------------------------------
# the inputs of the kernel tests
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kernel_inputs(shape, scheme, dtype, weighting):
    """(x_bar, q, x0, kw): x_bar uniform in [0, XBAR_SPREAD), q a random direction per spatial site with |q_s|_F uniform in [0, Q_RADIUS LAM),
    x0 = x_bar + N(0, 1); rounded to the dtype, read-only"""
    kw = case_kw(weighting, shape)
    rng = np.random.default_rng(5)
    x = (XBAR_SPREAD * rng.random(shape)).astype(dtype)
    nd = orc.D(np.zeros(shape), scheme, **kw).shape[1]
    q = rng.standard_normal((shape[0], nd) + tuple(shape[1:]))
    q = (q / site_norm(q)[:, None, None] * (LAM * Q_RADIUS * rng.random((shape[0],) + tuple(shape[2:])))[:, None, None]).astype(dtype)
    x0 = (x.astype(np.float64) + rng.standard_normal(shape)).astype(dtype)
    for a in (x, q, x0):
        a.setflags(write=False)
    return x, q, x0, kw


def shares(v, lam):
    """the shares of the three classes among the spatial sites, and the mask of the third"""
    n, nf = site_norm(v), frame_norm(v)
    coupled = (n > lam) & np.any(nf <= lam, axis=1)
    return float(np.mean(n <= lam)), float(np.mean(n > lam)), float(np.mean(coupled)), coupled


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_class_of_sites_is_populated(shape, scheme):
    for weighting in WEIGHTINGS:
        for dtype in (np.float64, np.float32):
            x, q, _, kw = kernel_inputs(shape, scheme, dtype, weighting)
            _, _, v, _ = ref_dual(x, q, SIGMA, LAM, scheme, kw)
            inside, outside, coupled, _ = shares(v, LAM)
            print("%s %s %s %s: inside %.3f outside %.3f coupled %.3f" % (shape, scheme, weighting, np.dtype(dtype).name, inside, outside, coupled))
            assert inside >= MIN_SHARE and outside >= MIN_SHARE, (weighting, inside, outside)
            if shape[1] >= 2:
                assert coupled >= MIN_SHARE, (weighting, coupled)
            else:
                assert coupled == 0.0                                   # one frame: its own norm IS the site's


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", Z_SHAPES)
def test_every_class_of_sites_is_populated_in_every_plane_of_the_z_range_volumes(shape, scheme):
    """``Z_SHAPES`` are not in ``SHAPES``: the same three shares for the (shape, weighting) pairs of the z-range tests, over the volume AND in
    each of its 5 planes -- a range of one plane must not be all-inside (nothing projected) or all-outside"""
    for weighting in Z_WEIGHTINGS:
        for dtype in (np.float64, np.float32):
            x, q, _, kw = kernel_inputs(shape, scheme, dtype, weighting)
            _, _, v, _ = ref_dual(x, q, SIGMA, LAM, scheme, kw)
            what = (shape, scheme, weighting, np.dtype(dtype).name)
            inside, outside, coupled, _ = shares(v, LAM)
            assert min(inside, outside, coupled) >= MIN_SHARE, (what, inside, outside, coupled)
            for z in range(shape[0]):
                inside, outside, coupled, _ = shares(v[z:z + 1], LAM)
                print("%s %s %s %s plane %d: inside %.3f outside %.3f coupled %.3f" % (what + (z, inside, outside, coupled)))
                assert min(inside, outside, coupled) >= MIN_SHARE, (what, z, inside, outside, coupled)


def test_joint_projection_is_feasible_and_differs_from_the_per_frame_one():
    """the reference itself: |q_s|_F <= LAM afterwards, inside sites untouched, and at coupled sites the per-frame projection gives another q"""
    shape, scheme = (3, 2, 16, 20), "hybrid"
    x, q, _, kw = kernel_inputs(shape, scheme, np.float64, "plain")
    wq, _, v, n = ref_dual(x, q, SIGMA, LAM, scheme, kw)
    assert float(np.max(site_norm(wq))) <= LAM * (1.0 + 1e-14)
    inside = np.broadcast_to((n <= LAM)[:, None, None], v.shape)
    np.testing.assert_array_equal(wq[inside], v[inside])
    nf = frame_norm(v)
    per_frame = v * np.where(nf > LAM, LAM / np.where(nf > 0.0, nf, 1.0), 1.0)[:, None]
    coupled = shares(v, LAM)[3]
    assert bool(np.all(np.any(per_frame != wq, axis=(1, 2))[coupled]))


def test_identical_frames_are_single_frame_tv_at_weight_over_sqrt_m():
    """M identical frames, reg_time = 0: |.|_F = sqrt(M) |.|_2, so the joint model at weight lam is plain TV of one frame at lam / sqrt(M) --
    the known answer of the solver test, in the reference"""
    rng = np.random.default_rng(3)
    frame = 20.0 * rng.random((1, 1, 12, 16))
    x0 = np.repeat(frame, 4, axis=1)
    kw = dict(reg_z_over_reg=1.0, reg_time=0.0)
    joint = np_vectorial(x0, 25, 6.0, "upwind", kw)[0]
    single = np_vectorial(frame, 25, 3.0, "upwind", kw)[0]
    wrong = np_vectorial(frame, 25, 6.0, "upwind", kw)[0]
    for m in range(4):
        assert float(np.max(np.abs(joint[:, m] - single[:, 0]))) <= 1e-12 * 20.0
    assert float(np.max(np.abs(joint[:, 0] - wrong[:, 0]))) > 1e-3
