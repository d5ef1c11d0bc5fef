"""Validate the oracle against the REAL reference, through the outputs its CPU twin returned (tests/golden/make_golden.py
--only-sweep imports the reference and writes them): a sweep of degenerate geometries for D, D^T, TV and its sub-gradient
(reference_sweep.npz.xz), and BASELINE configs[0] on the reference's cameraman image (cameraman.npz)."""
import io
import lzma
import os

import numpy as np

from conftest import GOLDEN, SCHEMES
from oracle import tv_oracle as orc

GEOMS = [(1, 1, 9, 9), (4, 1, 8, 8), (3, 1, 7, 7), (5, 1, 6, 6), (1, 3, 7, 7), (4, 2, 6, 6), (3, 3, 6, 6), (5, 4, 7, 7), (6, 8, 5, 5),
         (3, 1, 2, 2), (4, 3, 2, 2), (1, 1, 3, 3), (3, 3, 4, 4)]      # tiny frames: central has no interior row / column at N = 2


def _sweep():
    with open(os.path.join(GOLDEN, "reference_sweep.npz.xz"), "rb") as f:
        return np.load(io.BytesIO(lzma.decompress(f.read())))


def test_oracle_equals_imported_reference():
    z = _sweep()
    refD, refDT, refG, reftv, Dshape = z["D"], z["DT"], z["G"], z["tv"], z["D_shape"]
    ninf = np.unpackbits(z["norms_inf"]).astype(bool)
    rng = np.random.default_rng(11)         # the generator's draws, in its order: mask, x, y
    worst = 0.0
    od = ov = 0                             # offsets into the concatenated D and per-voxel arrays
    cases = ((s, g, lz, mu, m) for s in SCHEMES for g in GEOMS for lz, mu in ((1.0, 0.0), (0.0, 0.0), (2.5, 1.0), (1.0, 2 ** -5), (0.0, 0.7))
             for m in (False, True) if not m or (mu > 0 and g[1] > 1))
    for k, (scheme, shape, lz, mu, use_mask) in enumerate(cases):
        mask = (rng.random((1, 1) + shape[2:]) > 0.4) if use_mask else False
        kw = dict(reg_z_over_reg=lz, reg_time=mu, mask_static=mask, factor_reg_static=3.0 if use_mask else 0)
        x = rng.integers(0, 2, shape).astype(np.float64)
        x[..., :2, :2] = 0.25
        Do = orc.D(x, scheme, **kw)
        assert tuple(Dshape[k]) == Do.shape, (scheme, shape, lz, mu)
        assert orc.num_channels(scheme, shape[0], shape[1], lz, mu) == Do.shape[1]
        nD, nV = Do.size, x.size
        worst = max(worst, np.abs(refD[od:od + nD] - Do.ravel()).max())
        y = rng.integers(-1, 2, Do.shape).astype(np.float64)
        worst = max(worst, np.abs(refDT[ov:ov + nV] - orc.D_T(y, scheme, **kw).ravel()).max())
        to, Go, no = orc.tv(x, scheme, return_grad_norms=True, **kw)
        tr = float(reftv[k])
        worst = max(worst, abs(tr - to) / max(1.0, abs(tr)), np.abs(refG[ov:ov + nV] - Go.ravel()).max())
        assert np.array_equal(ninf[ov:ov + nV], np.isinf(no).ravel())
        od, ov = od + nD, ov + nV
    assert k + 1 == len(reftv) == 344 and od == refD.size and ov == refG.size == refDT.size
    assert worst < 1e-12, worst


# BASELINE configs[0] on its REAL workload (SURVEY section 8d / BASELINE.md section 2): the README's sub-gradient loop
# (README.md:107-124) on the reference's cameraman image, native 256 x 256 and the 2 x 2 Kronecker 512 x 512 variant,
# hybrid, 300 iterations, np.random.seed(0); the image and the reference's own loss trajectory are stored in cameraman.npz.
WANT = {256: (97202967.0339645, 39074939.77692743), 512: (373250884.84215766, 139106604.86969954)}


def test_config0_cameraman_losses_match_baseline():
    z = np.load(os.path.join(GOLDEN, "cameraman.npz"))
    cam = z["image"].astype(np.int64)
    assert cam.shape == (256, 256) and cam.min() == 7 and cam.max() == 253
    losses = {}
    for n, img in ((256, cam), (512, np.kron(cam, np.ones((2, 2), dtype=cam.dtype)))):
        np.random.seed(0)
        truth = np.reshape(img, (1, 1) + img.shape)
        noisy = truth + 100 * np.random.rand(*truth.shape)
        x, loss = orc.subgradient_descent(noisy, 300, 25, 5e-3, scheme="hybrid")
        # the first value to the last digit; the last one to 1e-5: the oracle follows the reference to 1e-15 for the first ~100
        # iterations, then the trajectories part ways (a sub-gradient flips sign at |Dx| ~ 1e-14 under a different summation
        # order: 9e-8 at iteration 200, 1.3e-6 at 299 on the 256 image)
        assert abs(loss[0] - WANT[n][0]) <= 1e-12 * WANT[n][0], (n, loss[0])
        assert abs(loss[299] - WANT[n][1]) <= 1e-5 * WANT[n][1], (n, loss[299])
        assert np.all(np.diff(loss) < 0)
        losses[n] = loss
    # and the reference itself said the same on the native image (the numbers above are its outputs):
    # its own loop, iteration by iteration
    ref = z["gd_loss_hybrid_256"]
    assert ref.shape == (300,)
    for it in range(101):
        assert abs(ref[it] - losses[256][it]) <= 1e-12 * ref[it], (it, ref[it], losses[256][it])
    assert abs(ref[0] - WANT[256][0]) <= 1e-12 * ref[0] and abs(ref[-1] - WANT[256][1]) <= 1e-12 * ref[-1], (ref[0], ref[-1])
