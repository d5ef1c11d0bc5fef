#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by IMPORTING the reference (PyTV-4D v1.1.2).

Runs only in the authoring container, where the reference is mounted read-only:

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=/root/reference \
        python3 /root/repo/tests/golden/make_golden.py

Nothing but DATA is written: seeded inputs and the outputs the reference's CPU twin
(pytv.tv_operators_CPU / pytv.tv_CPU) returns for them.  The loops at the bottom are the
README's user-level driver snippets (README.md:107-124 sub-gradient descent, :141-157
Chambolle-Pock) calling the reference's operators.
"""
import json
import os
import sys

import numpy as np

import pytv  # the reference, from PYTHONPATH=/root/reference

assert "/root/reference" in os.path.abspath(pytv.__file__), pytv.__file__
OUT = os.path.dirname(os.path.abspath(__file__))
SCHEMES = ("upwind", "downwind", "central", "hybrid")
ops = pytv.tv_operators_CPU
tvc = pytv.tv_CPU

# name, shape (Nz, M, N, N), reg_z_over_reg, reg_time, mask?, factor, dtype
CASES = [
    ("2d",        (1, 1, 7, 7), 1.0, 0.0,    False, 0, "f8"),
    ("3d",        (5, 1, 6, 6), 1.0, 0.0,    False, 0, "f8"),
    ("3d_noz",    (5, 1, 6, 6), 0.0, 0.0,    False, 0, "f8"),
    ("3d_lz2p5",  (4, 1, 6, 6), 2.5, 0.0,    False, 0, "f8"),
    ("3d_nz6",    (6, 1, 5, 5), 1.0, 0.0,    False, 0, "f8"),
    ("3d_nz3",    (3, 1, 5, 5), 0.3, 0.0,    False, 0, "f8"),
    ("2dt_m4",    (1, 4, 6, 6), 1.0, 1.0,    False, 0, "f8"),
    ("4d_m2",     (3, 2, 6, 6), 1.0, 1.0,    False, 0, "f8"),
    ("4d_m3",     (3, 3, 5, 5), 1.0, 1.0,    False, 0, "f8"),
    ("4d_m4",     (4, 4, 5, 5), 1.0, 1.0,    False, 0, "f8"),
    ("4d_m8",     (3, 8, 5, 5), 1.0, 1.0,    False, 0, "f8"),
    ("4d_mu2m5",  (4, 3, 6, 6), 1.0, 2**-5,  False, 0, "f8"),
    ("4d_noz",    (4, 3, 6, 6), 0.0, 1.0,    False, 0, "f8"),
    ("4d_mask",   (3, 3, 6, 6), 2.5, 0.7,    True,  4, "f8"),
    ("4d_mask_m2", (4, 2, 5, 5), 1.0, 1.5,   True,  0.25, "f8"),
    ("4d_f32",    (3, 4, 8, 8), 1.0, 1.0,    False, 0, "f4"),
    ("4d_f32_mask", (5, 3, 8, 8), 0.5, 2.0,  True,  4, "f4"),
    # round 6: a boolean mask_static with the reference's DEFAULT factor_reg_static=0 (pytv/tv_operators_GPU.py:134): the time
    # differences vanish on the masked pixels (appended: the seeds 1000 + index of the cases above do not move)
    ("4d_mask_f0", (4, 3, 6, 6), 1.0, 1.0,   True,  0, "f8"),
    ("4d_f32_mask_f0", (3, 4, 8, 8), 2.0, 0.5, True, 0, "f4"),
]


def gen_ops():
    for scheme in SCHEMES:
        D = getattr(ops, "D_" + scheme)
        DT = getattr(ops, "D_T_" + scheme)
        tv = getattr(tvc, "tv_" + scheme)
        blob = {}
        names = []
        for ic, (name, shape, lz, mu, use_mask, factor, dt) in enumerate(CASES):
            rng = np.random.default_rng(1000 + ic)
            x = rng.standard_normal(shape).astype(dt)
            # a flat patch so that some gradient norms are exactly zero (sub-gradient guard)
            x[..., :2, :3] = x.dtype.type(0.5)
            mask = (rng.random((1, 1) + shape[2:]) > 0.5) if use_mask else False
            kw = dict(reg_z_over_reg=lz, reg_time=mu, mask_static=mask, factor_reg_static=factor)
            Dx = D(x.copy(), **kw)
            y = rng.standard_normal(Dx.shape).astype(dt)
            DTy = DT(y.copy(), **kw)
            DTDx = DT(Dx.copy(), **kw)
            l21, norms = ops.compute_L21_norm(Dx, return_array=True)
            tvv, G, gn = tv(x.copy(), return_grad_norms=True, **kw)
            names.append(name)
            pre = name + "/"
            blob[pre + "x"] = x
            blob[pre + "y"] = y
            blob[pre + "params"] = np.array([lz, mu, float(factor)], dtype=np.float64)
            blob[pre + "mask"] = np.asarray(mask)
            blob[pre + "D"] = Dx
            blob[pre + "DT"] = DTy
            blob[pre + "DTD"] = DTDx
            blob[pre + "l21"] = np.float64(l21)
            blob[pre + "norms"] = norms
            blob[pre + "tv"] = np.float64(tvv)
            blob[pre + "G"] = G
            blob[pre + "grad_norms"] = gn
        blob["case_names"] = np.array(names)
        np.savez_compressed(os.path.join(OUT, "ops_%s.npz" % scheme), **blob)
        print("wrote ops_%s.npz" % scheme)


def gen_known_answers():
    """README.md:76-93 known answer and its siblings; 5x5 impulse of the maths notebook."""
    ka = {}
    np.random.seed(0)
    x = np.random.rand(20, 4, 100, 100)
    for scheme in SCHEMES:
        tv = getattr(tvc, "tv_" + scheme)
        for tag, mu in (("mu0", 0.0), ("mu2m5", 2**-5)):
            tvv, G = tv(x.copy(), reg_time=mu)
            ka["readme_%s_%s" % (scheme, tag)] = {
                "tv": float(tvv), "G_sum": float(G.sum()), "G_abs_sum": float(np.abs(G).sum()),
                "G_sq_sum": float((G * G).sum()),
                "G_probe": [float(v) for v in G[[0, 7, 19, 3], [0, 1, 3, 2], [0, 50, 99, 17], [0, 31, 99, 64]]],
            }
    A = np.zeros((1, 1, 5, 5))
    A[0, 0, 2, 2] = 1.0
    for scheme in SCHEMES:
        tvv, G = getattr(tvc, "tv_" + scheme)(A.copy())
        ka["impulse5_" + scheme] = {"tv": float(tvv), "G": [[float(v) for v in row] for row in G[0, 0]]}
    with open(os.path.join(OUT, "known_answers.json"), "w") as f:
        json.dump(ka, f, indent=1, sort_keys=True)
    print("wrote known_answers.json")


def phantom2d(n, seed):
    rng = np.random.RandomState(seed)
    img = np.zeros((n, n))
    for _ in range(12):
        r0, c0 = rng.randint(0, n - 8, size=2)
        h, w = rng.randint(6, n // 2, size=2)
        img[r0:r0 + h, c0:c0 + w] += rng.rand() * 255.0 / 3.0
    return img


def gen_trajectories():
    """README driver loops on a seeded synthetic 2-D phantom (the reference's cameraman image is
    package data and is not copied)."""
    noise_level, nb_it, regularization, step_size = 100, 300, 25, 5e-3
    truth = phantom2d(64, 7).reshape(1, 1, 64, 64)
    np.random.seed(0)
    noisy = truth + noise_level * np.random.rand(*truth.shape)
    blob = {"truth": truth, "noisy": noisy,
            "params": np.array([noise_level, nb_it, regularization, step_size], dtype=np.float64)}

    for scheme in SCHEMES:
        tv = getattr(tvc, "tv_" + scheme)
        D = getattr(ops, "D_" + scheme)
        DT = getattr(ops, "D_T_" + scheme)

        # README.md:118-124
        est = np.copy(noisy)
        loss_gd = np.zeros([nb_it, ])
        for it in range(nb_it):
            tvv, G = tv(est)
            est += - step_size * ((est - noisy) + regularization * G)
            loss_gd[it] = 0.5 * np.sum(np.square(est - noisy)) + regularization * tvv
        blob["gd_loss_" + scheme] = loss_gd
        blob["gd_final_" + scheme] = est

        # README.md:141-157
        sigma_D, sigma_A, tau = 0.5, 1.0, 1 / (8 + 1)
        est = np.copy(noisy)
        dual_fid = np.zeros_like(est)
        dual_tv = np.zeros_like(D(est))
        loss_cp = np.zeros([nb_it, ])
        for it in range(nb_it):
            dual_fid = (dual_fid + sigma_A * (est - noisy)) / (1.0 + sigma_A)
            D_x = D(est)
            prox_argument = dual_tv + sigma_D * D_x
            dual_tv = prox_argument / np.maximum(1.0, np.sqrt(np.sum(prox_argument**2, axis=1)) / regularization)
            est = est - tau * dual_fid - tau * DT(dual_tv)
            loss_cp[it] = 0.5 * np.sum(np.square(est - noisy)) + regularization * ops.compute_L21_norm(D_x)
        blob["cp_loss_" + scheme] = loss_cp
        blob["cp_final_" + scheme] = est
    np.savez_compressed(os.path.join(OUT, "trajectories_2d.npz"), **blob)
    print("wrote trajectories_2d.npz")


def gen_trajectory_512():
    """BASELINE configs[0] at its SIZE (512 x 512, hybrid sub-gradient loop, 300 iterations, README.md:107-124) on a
    synthetic phantom -- the cameraman image itself is stored on its own (gen_cameraman: cameraman.npz, which
    tests/test_oracle_vs_reference.py pins the oracle on).  Only the phantom (it
    compresses), the seed and the outputs are stored: the noise is np.random.RandomState(0).rand, which NumPy keeps
    bit-stable across versions."""
    noise_level, nb_it, regularization, step_size = 100, 300, 25, 5e-3
    truth = phantom2d(512, 11).reshape(1, 1, 512, 512)
    np.random.seed(0)
    noisy = truth + noise_level * np.random.rand(*truth.shape)
    assert np.array_equal(noisy, truth + noise_level * np.random.RandomState(0).rand(*truth.shape))
    est = np.copy(noisy)
    loss = np.zeros([nb_it, ])
    for it in range(nb_it):
        tvv, G = tvc.tv_hybrid(est)
        est += - step_size * ((est - noisy) + regularization * G)
        loss[it] = 0.5 * np.sum(np.square(est - noisy)) + regularization * tvv
    np.savez_compressed(os.path.join(OUT, "trajectory_512.npz"), truth=truth,
                        params=np.array([noise_level, nb_it, regularization, step_size, 0], dtype=np.float64),
                        gd_loss_hybrid=loss, gd_final_mean=np.array(est.mean()), gd_final_row=est[0, 0, 200].copy(),
                        noisy_checksum=np.array(noisy.sum()))
    print("wrote trajectory_512.npz")


# the degenerate geometries of the oracle sweep (tests/test_oracle_vs_reference.py): tiny frames, central has no interior row /
# column at N = 2.  The inputs are drawn from np.random.default_rng(11) in exactly this order (mask, x, y), so that the test
# regenerates them; only the reference's outputs are stored.  x is a binary image (0 / 1, with a flat 0.25 patch in the first
# 2 x 2 corner of every frame) and y takes the values -1, 0, 1: differences of every sign, ties and zero gradients everywhere, and
# outputs that compress (the sub-gradient still divides by irrational norms).
SWEEP_GEOMS = [(1, 1, 9, 9), (4, 1, 8, 8), (3, 1, 7, 7), (5, 1, 6, 6), (1, 3, 7, 7), (4, 2, 6, 6), (3, 3, 6, 6), (5, 4, 7, 7), (6, 8, 5, 5),
               (3, 1, 2, 2), (4, 3, 2, 2), (1, 1, 3, 3), (3, 3, 4, 4)]
SWEEP_PARAMS = ((1.0, 0.0), (0.0, 0.0), (2.5, 1.0), (1.0, 2 ** -5), (0.0, 0.7))


def sweep_cases():
    """(scheme, shape, reg_z_over_reg, reg_time, use_mask) in the order of the sweep"""
    for scheme in SCHEMES:
        for shape in SWEEP_GEOMS:
            for lz, mu in SWEEP_PARAMS:
                for use_mask in (False, True):
                    if use_mask and not (mu > 0 and shape[1] > 1):
                        continue
                    yield scheme, shape, lz, mu, use_mask


def gen_reference_sweep():
    """D, D^T, TV, G and the infinite-norm pattern of the reference's CPU twin over the sweep (float64), every case's arrays
    flattened and concatenated in the sweep's order; an .npz, xz-compressed."""
    import io
    import lzma
    rng = np.random.default_rng(11)
    D, DT, G, tv, ninf, dshape = [], [], [], [], [], []
    for scheme, shape, lz, mu, use_mask in sweep_cases():
        mask = (rng.random((1, 1) + shape[2:]) > 0.4) if use_mask else False
        kw = dict(reg_z_over_reg=lz, reg_time=mu, mask_static=mask, factor_reg_static=3.0 if use_mask else 0)
        x = rng.integers(0, 2, shape).astype(np.float64)
        x[..., :2, :2] = 0.25
        Dr = getattr(ops, "D_" + scheme)(x.copy(), **kw)
        y = rng.integers(-1, 2, Dr.shape).astype(np.float64)
        tr, Gr, nr = getattr(tvc, "tv_" + scheme)(x.copy(), return_grad_norms=True, **kw)
        D.append(Dr.ravel())
        DT.append(getattr(ops, "D_T_" + scheme)(y.copy(), **kw).ravel())
        G.append(Gr.ravel())
        tv.append(tr)
        ninf.append(np.isinf(nr).ravel())
        dshape.append(Dr.shape)
    buf = io.BytesIO()
    np.savez(buf, D=np.concatenate(D), DT=np.concatenate(DT), G=np.concatenate(G), tv=np.array(tv, dtype=np.float64),
             norms_inf=np.packbits(np.concatenate(ninf)), D_shape=np.array(dshape, dtype=np.int32))
    with open(os.path.join(OUT, "reference_sweep.npz.xz"), "wb") as f:
        f.write(lzma.compress(buf.getvalue(), preset=9 | lzma.PRESET_EXTREME))
    print("wrote reference_sweep.npz.xz (%d cases)" % len(tv))


def gen_cameraman():
    """BASELINE configs[0] on its real image: the reference's cameraman (256 x 256, values 7 .. 253, stored as uint8) and the
    reference's own README sub-gradient loop on it (hybrid, 300 iterations, np.random.seed(0) noise): the loss of every iteration."""
    cam = np.asarray(pytv.utils.cameraman())
    assert cam.shape == (256, 256) and cam.min() == 7 and cam.max() == 253 and np.array_equal(cam, cam.astype(np.uint8))
    np.random.seed(0)
    truth = np.reshape(cam, (1, 1, 256, 256))
    noisy = truth + 100 * np.random.rand(*truth.shape)
    est = np.copy(noisy)
    loss = np.zeros(300)
    for it in range(300):
        tvv, G = tvc.tv_hybrid(est)
        est += -5e-3 * ((est - noisy) + 25 * G)
        loss[it] = 0.5 * np.sum(np.square(est - noisy)) + 25 * tvv
    np.savez_compressed(os.path.join(OUT, "cameraman.npz"), image=cam.astype(np.uint8), gd_loss_hybrid_256=loss)
    print("wrote cameraman.npz")


if __name__ == "__main__":
    if "--only-sweep" in sys.argv:            # the two fixtures of tests/test_oracle_vs_reference.py alone
        gen_reference_sweep()
        gen_cameraman()
        sys.exit(0)
    if "--only-512" not in sys.argv:
        gen_ops()
        gen_known_answers()
        gen_trajectories()
    gen_trajectory_512()
    gen_reference_sweep()
    gen_cameraman()
    sys.exit(0)
