"""The INTERIOR (FAST, ``run<0>``) and COLUMN-BORDER (``run<1>``) bodies of the one-pass sub-gradient kernel ``k_subgrad_col``
(csrc/tv_subgrad2.h, launched by ``sg2_launch`` of csrc/tv_subgrad_host.h) against the fp64 NumPy oracle, voxel by voxel.

A block runs the FAST body only when its tile, ring included, lies strictly inside the frame, and the column-border body only in
the tile rows of that interior rectangle: frames below ~30 x 250 (fp32) have no such tile, so the small shapes of
test_gpu_subgrad_onepass.py run the generic body ``run<2>`` alone.  The frames here are the smallest ones with >= 2 interior tile
rows, >= 2 interior block columns and a ragged remainder both ways; ``interior_rect`` restates the dispatch rule and every case
asserts what it says about its shape, so the shapes cannot silently stop reaching the code.

Bars: the project's (fp32 ``rtol = atol = 1e-5`` against the fp64 oracle on the up-cast input, fp64 ``1e-11``; TV ``1e-6`` /
``1e-11`` relative).  Every test prints the figures it observed before it asserts (``pytest -s``)."""
import collections
import functools

import numpy as np
import pytest

from oracle import tv_oracle as orc

F32, F64 = np.float32, np.float64
PAD = 4100                      # guard band, elements
STEP, LAM = 0.05, 2.0


# =====================================================================================================================
# 0. the dispatch rule of sg2_launch, restated (pure Python: the CPU-only test below pins it)
# =====================================================================================================================
def _cdiv(a, b):
    """integer division of C (truncates towards zero)"""
    q = abs(a) // b
    return q if a >= 0 else -q


def _tiling(shape, scheme, dtype, mode, aligned_opt=1, has_weights=False):
    """csrc/tv_subgrad_host.h, sg2_launch, line by line (product build: TV_SG2_R32 = 4, TV_SG2_NW32 = 4, TV_SG2_NWX = 2,
    TV_SG2_AL = 1, SG2_TWN = 8).  has_weights: False, True (a static mask or a per-pixel time factor) or "volume" (a per-voxel
    weight volume, which also switches the aligned tiles off)."""
    nz, m, ny, nx = (int(v) for v in shape)
    f64 = np.dtype(dtype) == np.dtype(np.float64)
    itemsize = 8 if f64 else 4
    R = 2 if f64 else 4
    halo = scheme in ("hybrid", "central")
    al_scheme = (aligned_opt != 0) if scheme in ("upwind", "downwind") else False        # TV_SG2_AL == 1: one-sided schemes only
    al = bool(al_scheme and m <= 8 and has_weights != "volume" and ny * nx * itemsize * m < (1 << 31) and (not f64 or mode != 0))
    NW = 8 if al else 4
    NWX = 1 if (f64 or al) else 2
    UR, UC = R * NW - 2, (64 if al else (60 if halo else 62))
    tx, ty = (nx + UC - 1) // UC, (ny + UR - 1) // UR
    RING, RB = (2 if halo else 1), R * NW
    txb = (tx + NWX - 1) // NWX
    ix0, iy0 = 1, 1
    ix1, iy1 = _cdiv(nx - 2 - 63 + RING, UC), _cdiv(ny - RB, UR)
    if al:
        ix1 = (nx - 1) // 64 - 1
    if nx < 66 or ny < RB + 2 or has_weights or ix1 < ix0 or iy1 < iy0:
        ix0, iy0, ix1, iy1 = 1, 1, 0, 0
    if ix1 >= ix0:              # wave-tile columns -> block-tile columns whose NWX wave tiles all lie inside
        b0, b1 = (ix0 + NWX - 1) // NWX, (ix1 + 1) // NWX - 1
        ix0, ix1 = b0, b1
        if ix1 < ix0:
            ix0, iy0, ix1, iy1 = 1, 1, 0, 0
    if f64:
        form = "E" if al else "D"
    else:
        form = "B" if al else ("A" if halo else "C")
    return dict(form=form, txb=txb, ty=ty, ix0=ix0, ix1=ix1, iy0=iy0, iy1=iy1, UR=UR, BW=UC * NWX)


def interior_rect(shape, scheme, dtype, mode, aligned_opt=1, has_weights=False):
    """(form, tx_blocks, ty, ix0, ix1, iy0, iy1): the kernel form (A - E, see FORMS) and the rectangle of block tiles that run
    the FAST body (empty when ix1 < ix0), as sg2_launch of csrc/tv_subgrad_host.h computes them.  mode: 0 tv_subgrad_fused,
    1 tv_subgrad_step_fused, 2 tv_subgrad_fused_norms.  aligned_opt: the TV_SG_ALIGNED option."""
    t = _tiling(shape, scheme, dtype, mode, aligned_opt, has_weights)
    return t["form"], t["txb"], t["ty"], t["ix0"], t["ix1"], t["iy0"], t["iy1"]


def _nonempty(rect):
    return rect[4] >= rect[3] and rect[6] >= rect[5]


# form: dtype, (scheme, mode, TV_SG_ALIGNED, M) settings that reach it, smallest frame with one interior tile, main frame
Form = collections.namedtuple("Form", "dtype minima main")
FORMS = {
    "A": Form(F32, {"hybrid": (30, 243), "central": (30, 243)}, (47, 370)),
    "B": Form(F32, {"upwind": (62, 129), "downwind": (62, 129)}, (95, 200)),
    "C": Form(F32, {"upwind": (30, 250), "downwind": (30, 250)}, (47, 380)),
    "D": Form(F64, {"hybrid": (14, 123), "central": (14, 123), "upwind": (14, 126), "downwind": (14, 126)}, (23, 190)),
    "E": Form(F64, {"upwind": (30, 129), "downwind": (30, 129)}, (47, 200)),
}


def _reach(form, scheme):
    """(aligned_opt, modes) under which (form, scheme) is what the launcher picks for M <= 8"""
    if form == "C":
        return 0, (0, 2, 1)
    if form == "D" and scheme in ("upwind", "downwind"):
        return 0, (0, 2, 1)              # (MODE 0 is form D with any TV_SG_ALIGNED)
    if form == "E":
        return 1, (2, 1)
    return 1, (0, 2, 1)


def test_interior_rect_minima():
    """CPU only: the helper on the table of smallest frames -- one interior tile there, none with one row or one column less."""
    for form, f in FORMS.items():
        for scheme, (ny, nx) in f.minima.items():
            al, modes = _reach(form, scheme)
            for mode in modes:
                for m in (1, 3, 8):
                    r = interior_rect((3, m, ny, nx), scheme, f.dtype, mode, al)
                    assert r[0] == form and r[3:] == (1, 1, 1, 1), (form, scheme, mode, m, r)
                    for shp in ((ny - 1, nx), (ny, nx - 1)):
                        r = interior_rect((3, m) + shp, scheme, f.dtype, mode, al)
                        assert r[0] == form and not _nonempty(r), (form, scheme, mode, shp, r)
                    r = interior_rect((3, m, ny + 1, nx + 1), scheme, f.dtype, mode, al)
                    assert _nonempty(r)
                    assert not _nonempty(interior_rect((3, m, ny, nx), scheme, f.dtype, mode, al, has_weights=True))
    # more than 8 frames (time windows): the one-sided fp32 schemes leave the aligned tiles (form C); fp64 stays / becomes form D
    assert interior_rect((3, 9, 30, 250), "upwind", F32, 0)[0] == "C" and _nonempty(interior_rect((3, 9, 30, 250), "upwind", F32, 0))
    assert interior_rect((3, 9, 47, 200), "downwind", F64, 1)[0] == "D"
    assert interior_rect((3, 8, 47, 200), "downwind", F64, 1)[0] == "E" and interior_rect((3, 8, 47, 200), "downwind", F64, 0)[0] == "D"
    # MODE 0 of fp64 is never aligned; a weight volume switches the aligned tiles off as well
    assert interior_rect((3, 3, 95, 200), "upwind", F32, 0, has_weights="volume")[0] == "C"
    # the main frames: >= 2 interior tile rows, >= 2 interior block columns, outline on every side, ragged both ways
    for form, f in FORMS.items():
        for scheme in f.minima:
            al, modes = _reach(form, scheme)
            t = _tiling((5, 3) + f.main, scheme, f.dtype, modes[-1], al)
            assert t["form"] == form and t["ix1"] - t["ix0"] >= 1 and t["iy1"] - t["iy0"] >= 1, (form, scheme, t)
            assert t["ix0"] == 1 and t["iy0"] == 1 and t["ix1"] < t["txb"] - 1 and t["iy1"] < t["ty"] - 1
            assert f.main[0] % t["UR"] and f.main[1] % t["BW"]


# =====================================================================================================================
# inputs, references (computed once per case, shared, read-only) and the three entry points
# =====================================================================================================================
@pytest.fixture(scope="module")
def nv():
    from pytv import _native
    _native.lib()
    return _native


def _input(shape, dtype, til, seed=0):
    """standard_normal * 10 with two flat patches (|Dx| == 0: the 0 -> +inf rule): one INSIDE the last interior tile, one across
    the corner where the first interior tile meets the outline tiles above and left of it"""
    rng = np.random.default_rng(1000 * seed + shape[1] + shape[3])
    img = (rng.standard_normal(shape) * 10).astype(dtype)
    ny, nx = shape[2:]
    ur, bw = til["UR"], til["BW"]
    bx, by = max(til["ix1"], 1), max(til["iy1"], 1)
    y0, x0 = by * ur + 3, bx * bw + 5
    img[:, :, y0:min(y0 + 3, ny), x0:min(x0 + 21, nx)] = 3.0
    img[:, :, ur - 2:min(ur + 2, ny), bw - 8:min(bw + 9, nx)] = -7.0
    return img


@functools.lru_cache(maxsize=3)
def _reference(shape, dtype, scheme, lz, mu, masked, aligned, mode):
    """(x, x0, mask, TV, G, norms) of the oracle, fp64, on the up-cast input; arrays are shared between tests: read-only"""
    til = _tiling(shape, scheme, dtype, mode, aligned)
    x = _input(shape, dtype, til)
    x0 = (np.random.default_rng(77).standard_normal(shape) * 10).astype(dtype)
    mask = (np.random.default_rng(5).random(shape[2:]) < 0.4) if masked else False
    tv, G, n = orc.tv(x.astype(np.float64), scheme, reg_z_over_reg=lz, reg_time=mu, mask_static=mask,
                      factor_reg_static=2.3 if masked else 0, return_grad_norms=True)
    for a in (x, x0, G, n):
        a.setflags(write=False)
    return x, x0, mask, float(tv), G, n


def _tdt(dtype):
    import torch
    return torch.float64 if np.dtype(dtype) == np.dtype(np.float64) else torch.float32


def _bars(dtype):
    f64 = np.dtype(dtype) == np.dtype(np.float64)
    return dict(g=1e-11 if f64 else 1e-5, tv=1e-11 if f64 else 1e-6, norms=1e-11 if f64 else 2e-6, eps=float(np.finfo(dtype).eps))


def _call(nv, mode, geo, x, x0=None, xp=None, xn=None, out=None, norms=None):
    """one entry point of the C-ABI; outputs pre-filled with NaN unless the caller brings its own"""
    import torch
    lib, st = nv.lib(), nv.current_stream(x.device)
    if out is None:
        out = torch.full_like(x, float("nan"))
    tv, fid = geo.scalar(), geo.scalar()
    ws = geo.workspace()
    if mode == 0:
        nv.check(lib.tv_subgrad_fused(geo.ref, nv.ptr(x), nv.ptr(xp), nv.ptr(xn), nv.ptr(out), nv.ptr(tv), nv.ptr(ws), st))
    elif mode == 2:
        if norms is None:
            norms = torch.full_like(x, float("nan"))
        nv.check(lib.tv_subgrad_fused_norms(geo.ref, nv.ptr(x), nv.ptr(xp), nv.ptr(xn), nv.ptr(out), nv.ptr(norms), nv.ptr(tv),
                                            nv.ptr(ws), st))
    else:
        nv.check(lib.tv_subgrad_step_fused(geo.ref, nv.ptr(x), nv.ptr(xp), nv.ptr(xn), nv.ptr(x0), nv.ptr(out), STEP, LAM, nv.ptr(tv),
                                           nv.ptr(fid), nv.ptr(ws), st))
    torch.cuda.synchronize()
    return out, float(tv), float(fid), norms


def _worst(got, ref, rtol, atol):
    """(largest |got - ref|, largest |got - ref| / (atol + rtol |ref|)): the second is what assert_allclose bounds by 1"""
    err = np.abs(got.astype(np.float64) - ref)
    return float(err.max()), float((err / (atol + rtol * np.abs(ref))).max())


def _check_against_oracle(nv, tag, shape, dtype, scheme, lz, mu, modes, aligned=1, masked=False, expect_interior=None, patch_aligned=None):
    """Run ``modes`` on the shared input and compare each with the oracle.  Returns {mode: (out, tv, fid, norms)} (host arrays).
    patch_aligned: the TV_SG_ALIGNED setting whose tiles place the flat patches of the input (default: ``aligned``)."""
    import torch
    x, x0, mask, tv_ref, G_ref, n_ref = _reference(shape, np.dtype(dtype).name, scheme, lz, mu, masked,
                                                   aligned if patch_aligned is None else patch_aligned, modes[-1])
    b = _bars(dtype)
    geo = nv.Geometry(shape, scheme, _tdt(dtype), torch.device("cuda", 0), reg_z_over_reg=lz, reg_time=mu, mask_static=mask,
                      factor_reg_static=2.3 if masked else 0)
    assert nv.lib().tv_subgrad_fused_supported(geo.ref) == 1
    xd, x0d = torch.tensor(x).cuda(), torch.tensor(x0).cuda()            # (copies: the shared arrays are read-only)
    res = {}
    for mode in modes:
        if expect_interior is not None:
            r = interior_rect(shape, scheme, dtype, mode, aligned, masked)
            assert _nonempty(r) == expect_interior[mode], (tag, mode, r)
        out, tv, fid, norms = _call(nv, mode, geo, xd, x0d)
        out = out.cpu().numpy()
        assert not np.isnan(out).any(), (tag, mode, int(np.isnan(out).sum()))
        tv_err = abs(tv - tv_ref) / abs(tv_ref)
        if mode == 1:
            # x_out = x - step ((x - x0) + lambda G): the G bar scaled by step * lambda, plus the rounding of the x-sized terms
            want = x.astype(np.float64) - STEP * ((x.astype(np.float64) - x0.astype(np.float64)) + LAM * G_ref)
            bound = STEP * LAM * (b["g"] + b["g"] * np.abs(G_ref)) + 4 * b["eps"] * float(np.abs(x).max())
            err = np.abs(out.astype(np.float64) - want)
            fid_ref = 0.5 * float(((out.astype(np.float64) - x0.astype(np.float64)) ** 2).sum())
            fid_err = abs(fid - fid_ref) / fid_ref
            print("OBS %s mode=1 x_out max_err=%.3e of bound %.3e (ratio %.3f) tv_rel=%.2e fid_rel=%.2e"
                  % (tag, err.max(), bound.min(), (err / bound).max(), tv_err, fid_err))
            assert (err <= bound).all(), (tag, float((err / bound).max()))
            assert fid_err <= b["tv"], (tag, fid, fid_ref)
        else:
            ga, gr = _worst(out, G_ref, b["g"], b["g"])
            print("OBS %s mode=%d G max_abs_err=%.3e (ratio to bar %.3f) tv_rel=%.2e" % (tag, mode, ga, gr, tv_err))
            np.testing.assert_allclose(out, G_ref, rtol=b["g"], atol=b["g"], err_msg="%s mode %d" % (tag, mode))
        assert tv_err <= b["tv"], (tag, mode, tv, tv_ref)
        if mode == 2:
            n1 = norms.cpu().numpy()
            assert np.array_equal(np.isinf(n1), np.isinf(n_ref)) and np.isinf(n1).sum() > 0, tag
            fin = np.isfinite(n_ref)
            print("OBS %s mode=2 norms max_rel_err=%.3e" % (tag, float((np.abs(n1[fin] - n_ref[fin]) / n_ref[fin]).max())))
            np.testing.assert_allclose(n1[fin], n_ref[fin], rtol=b["norms"], err_msg=tag)
            norms = n1
        res[mode] = (out, tv, fid, norms)
    return res


# =====================================================================================================================
# 1. every voxel against the fp64 oracle
# =====================================================================================================================
Case = collections.namedtuple("Case", "form scheme m aligned modes lz mu")
ALL, LZ, MU = (0, 2, 1), 1.7, 0.6


def _cases():
    c = []
    # A: fp32 hybrid / central (4 x 2 waves, 14 x 120 stored per block)
    for s in ("hybrid", "central"):
        c += [Case("A", s, 1, 1, ALL, LZ, MU), Case("A", s, 8, 1, ALL, LZ, MU)]
    c += [Case("A", "hybrid", 2, 1, ALL, LZ, MU), Case("A", "central", 3, 1, ALL, LZ, 0.0),           # (z only)
          Case("A", "hybrid", 5, 1, ALL, LZ, MU), Case("A", "central", 9, 1, ALL, LZ, MU), Case("A", "hybrid", 16, 1, ALL, LZ, MU),
          Case("A", "central", 19, 1, ALL, LZ, MU)]
    # B: fp32 upwind / downwind, aligned tiles (8 stacked waves, 30 x 64 stored); no time windows
    for s in ("upwind", "downwind"):
        c += [Case("B", s, 1, 1, ALL, LZ, MU), Case("B", s, 8, 1, ALL, LZ, MU)]
    c += [Case("B", "downwind", 2, 1, ALL, LZ, MU), Case("B", "upwind", 3, 1, ALL, LZ, MU), Case("B", "downwind", 5, 1, ALL, 0.0, 0.8)]   # (time only)
    # C: fp32 upwind / downwind on the non-aligned tiles: TV_SG_ALIGNED=0, and M > 8 (time windows)
    for s in ("upwind", "downwind"):
        c += [Case("C", s, 1, 0, ALL, LZ, MU), Case("C", s, 8, 0, ALL, LZ, MU)]
    c += [Case("C", "upwind", 9, 1, ALL, LZ, MU), Case("C", "downwind", 16, 1, ALL, LZ, MU), Case("C", "upwind", 19, 1, ALL, LZ, MU)]
    # D: fp64, 4 waves of 2-row strips (6 x 60 / 62 stored): hybrid / central in every mode ...
    for s in ("hybrid", "central"):
        c += [Case("D", s, 1, 1, ALL, LZ, MU), Case("D", s, 8, 1, ALL, LZ, MU)]
    c += [Case("D", "hybrid", 2, 1, ALL, LZ, MU), Case("D", "central", 3, 1, ALL, LZ, MU), Case("D", "hybrid", 5, 1, ALL, LZ, MU),
          Case("D", "central", 9, 1, ALL, LZ, MU), Case("D", "hybrid", 16, 1, ALL, LZ, MU), Case("D", "central", 19, 1, ALL, LZ, MU)]
    # ... upwind / downwind through MODE 0, through TV_SG_ALIGNED=0 in MODE 1 / 2, and through a time window
    for s in ("upwind", "downwind"):
        c += [Case("D", s, 1, 1, (0,), LZ, MU), Case("D", s, 8, 1, (0,), LZ, MU), Case("D", s, 1, 0, ALL, LZ, MU),
              Case("D", s, 8, 0, ALL, LZ, MU)]
    c += [Case("D", "upwind", 9, 1, ALL, LZ, MU)]
    # E: fp64 upwind / downwind, aligned tiles (14 x 64 stored), MODE 1 / 2 only
    for s in ("upwind", "downwind"):
        c += [Case("E", s, 1, 1, (2, 1), LZ, MU), Case("E", s, 8, 1, (2, 1), LZ, MU)]
    c += [Case("E", "upwind", 2, 1, (2, 1), LZ, MU), Case("E", "downwind", 3, 1, (2, 1), 0.0, 0.8), Case("E", "upwind", 5, 1, (2, 1), LZ, 0.0)]
    return c


def _case_id(c):
    return "%s-%s-M%d-al%d-modes%s%s" % (c.form, c.scheme, c.m, c.aligned, "".join(str(k) for k in c.modes),
                                         "" if (c.lz, c.mu) == (LZ, MU) else "-lz%g-mu%g" % (c.lz, c.mu))


@pytest.mark.gpu
@pytest.mark.parametrize("zchunk", [0, 2])
@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_every_voxel_against_the_oracle(nv, case, zchunk, tvopt):
    f = FORMS[case.form]
    shape = (5, case.m) + f.main
    tvopt("TV_ZCHUNK", zchunk)
    if case.aligned == 0:
        tvopt("TV_SG_ALIGNED", 0)
    for mode in case.modes:
        r = interior_rect(shape, case.scheme, f.dtype, mode, case.aligned)
        assert r[0] == case.form and _nonempty(r), (mode, r)
    tag = "%s zc=%d %s" % (_case_id(case), zchunk, "x".join(str(v) for v in shape))
    res = _check_against_oracle(nv, tag, shape, f.dtype, case.scheme, case.lz, case.mu, case.modes, case.aligned,
                                expect_interior={k: True for k in case.modes})
    # wherever MODE 0 and MODE 2 resolve to the same form they share a tile shape (the fp32 forms, fp64 hybrid / central, fp64
    # upwind / downwind in a time window or with TV_SG_ALIGNED=0): the same G, bit for bit
    if 0 in res and 2 in res and (interior_rect(shape, case.scheme, f.dtype, 0, case.aligned)
                                  == interior_rect(shape, case.scheme, f.dtype, 2, case.aligned)):
        assert np.array_equal(res[0][0], res[2][0])


# =====================================================================================================================
# 2. the rectangle's edges: the smallest frame with an interior tile, one row / one column less, one of each more
# =====================================================================================================================
def _edge_cases():
    out = []
    for form, f in FORMS.items():
        for scheme, (ny, nx) in f.minima.items():
            for dy, dx, interior in ((0, 0, True), (-1, 0, False), (0, -1, False), (1, 1, True)):
                out.append(pytest.param(form, scheme, (ny + dy, nx + dx), interior, id="%s-%s-%dx%d" % (form, scheme, ny + dy, nx + dx)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form,scheme,frame,interior", _edge_cases())
def test_edges_of_the_interior_rectangle(nv, form, scheme, frame, interior, tvopt):
    f = FORMS[form]
    al, modes = _reach(form, scheme)
    if al == 0:
        tvopt("TV_SG_ALIGNED", 0)
    shape = (3, 3) + frame
    # the modes in which this (scheme, option) IS the form (MODE 0 of form E's settings is form D: checked against the oracle all the same)
    own = {k: interior for k in (0, 1) if k in modes}
    for k in own:
        assert interior_rect(shape, scheme, f.dtype, k, al)[0] == form
    if 0 not in own:
        own[0] = _nonempty(interior_rect(shape, scheme, f.dtype, 0, al))
    _check_against_oracle(nv, "edge %s %s %dx%d" % (form, scheme, frame[0], frame[1]), shape, f.dtype, scheme, 1.3, 0.7, (0, 1), al,
                          expect_interior=own)


# =====================================================================================================================
# 3. the forms against each other on the same input
# =====================================================================================================================
BETWEEN = dict(rtol=2e-6, atol=2e-5)       # the suite's bars between two instantiations of this kernel


def _form_schemes():
    return [pytest.param(form, s, id="%s-%s" % (form, s)) for form, f in FORMS.items() for s in f.minima]


@pytest.mark.gpu
@pytest.mark.parametrize("form,scheme", _form_schemes())
def test_interior_dispatch_against_all_generic(nv, form, scheme, tvopt):
    """default dispatch (FAST / column-border / generic bodies) vs TV_SPARE=7 (every block generic): both within the oracle bars,
    and within the instantiation-to-instantiation bars of each other"""
    f = FORMS[form]
    al, modes = _reach(form, scheme)
    if al == 0:
        tvopt("TV_SG_ALIGNED", 0)
    shape = (3, 4) + f.main
    tag = "spare %s %s" % (form, scheme)
    a = _check_against_oracle(nv, tag + " default", shape, f.dtype, scheme, LZ, MU, modes, al, expect_interior={k: True for k in modes})
    tvopt("TV_SPARE", 7)
    b = _check_against_oracle(nv, tag + " TV_SPARE=7", shape, f.dtype, scheme, LZ, MU, modes, al)
    for k in modes:
        print("OBS %s mode=%d %s bit-equal to the all-generic launch: %s, TV rel diff %.2e"
              % (tag, k, "x_out" if k == 1 else "G", np.array_equal(a[k][0], b[k][0]), abs(a[k][1] - b[k][1]) / abs(a[k][1])))
        np.testing.assert_allclose(a[k][0], b[k][0], **BETWEEN)
        assert abs(a[k][1] - b[k][1]) <= 1e-9 * abs(a[k][1])


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["upwind", "downwind"])
@pytest.mark.parametrize("dtype,frame,forms", [(F32, (95, 380), ("B", "C")), (F64, (47, 200), ("E", "D"))], ids=["f32", "f64"])
def test_aligned_against_non_aligned_tiles(nv, scheme, dtype, frame, forms, tvopt):
    """the descent step (MODE 1) of the one-sided schemes with TV_SG_ALIGNED 1 and 0: both forms have interior tiles on this frame
    (95 x 380 in fp32: form B needs 62 rows, form C 250 columns)"""
    shape = (3, 4) + frame
    res = []
    for al, form in zip((1, 0), forms):
        r = interior_rect(shape, scheme, dtype, 1, al)
        assert r[0] == form and _nonempty(r), r
        if al == 0:
            tvopt("TV_SG_ALIGNED", 0)
        res.append(_check_against_oracle(nv, "aligned=%d %s %s" % (al, form, scheme), shape, dtype, scheme, LZ, MU, (1,), al,
                                         expect_interior={1: True}, patch_aligned=1)[1])       # the SAME input for both
    print("OBS aligned 1 vs 0 %s %s: x_out bit-equal %s, TV rel diff %.2e"
          % (np.dtype(dtype).name, scheme, np.array_equal(res[0][0], res[1][0]), abs(res[0][1] - res[1][1]) / abs(res[0][1])))
    np.testing.assert_allclose(res[0][0], res[1][0], **BETWEEN)
    assert abs(res[0][1] - res[1][1]) <= 1e-9 * abs(res[0][1])


@pytest.mark.gpu
@pytest.mark.parametrize("form,scheme", _form_schemes())
def test_static_mask_empties_the_rectangle(nv, form, scheme, tvopt):
    """a static mask on a frame that would otherwise have interior tiles: every block generic, oracle bars"""
    f = FORMS[form]
    al, modes = _reach(form, scheme)
    if al == 0:
        tvopt("TV_SG_ALIGNED", 0)
    shape = (3, 4) + f.main
    for k in modes:
        assert _nonempty(interior_rect(shape, scheme, f.dtype, k, al)) and not _nonempty(interior_rect(shape, scheme, f.dtype, k, al, True))
    _check_against_oracle(nv, "mask %s %s" % (form, scheme), shape, f.dtype, scheme, LZ, MU, modes, al, masked=True,
                          expect_interior={k: False for k in modes})


# =====================================================================================================================
# 4. slabs through interior tiles
# =====================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("zchunk", [16, 2])
@pytest.mark.parametrize("cuts", [(0, 3, 7), (0, 1, 2, 3, 4, 5, 6, 7)], ids=["cuts037", "cuts01234567"])
@pytest.mark.parametrize("form,scheme", [p for p in _form_schemes() if p.values[0] in "ABD"])
def test_slab_calls_through_interior_tiles_equal_unsharded(nv, form, scheme, cuts, zchunk, tvopt):
    """what test_one_pass_slab_calls_equal_unsharded asserts on 17 x 132, on frames with interior tiles and in fp64 as well: G and
    the descent step of every slab bit-equal to the unsharded call, TV and fidelity summing to it"""
    import torch
    f = FORMS[form]
    al, _ = _reach(form, scheme)             # fp64 upwind / downwind: TV_SG_ALIGNED=0 keeps the descent step on form D as well
    tvopt("TV_ZCHUNK", zchunk)
    if al == 0:
        tvopt("TV_SG_ALIGNED", 0)
    shape = (7, 3) + f.main
    for mode in (0, 1):
        r = interior_rect(shape, scheme, f.dtype, mode, al)
        assert r[0] == form and _nonempty(r), (mode, r)
    kw = dict(reg_z_over_reg=LZ, reg_time=MU)
    rng = np.random.default_rng(5)
    x = torch.as_tensor(rng.standard_normal(shape).astype(f.dtype)).cuda()
    x0 = torch.as_tensor(rng.standard_normal(shape).astype(f.dtype)).cuda()
    dev = torch.device("cuda", 0)
    gfull = nv.Geometry(shape, scheme, x.dtype, dev, **kw)
    G_full, tv_full, _, _ = _call(nv, 0, gfull, x)
    xo_full, tvf, fidf, _ = _call(nv, 1, gfull, x, x0)
    assert bool(torch.isfinite(G_full).all()) and bool(torch.isfinite(xo_full).all())
    nzg, tv_sum, tv1_sum, fid_sum = shape[0], 0.0, 0.0, 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        g = nv.Geometry((b - a,) + shape[1:], scheme, x.dtype, dev, nz_global=nzg, z0=a, **kw)

        def two(lo):     # two-plane halo, NaN where the global plane does not exist (must never be read)
            buf = torch.full((2,) + shape[1:], float("nan"), dtype=x.dtype, device=x.device)
            for k in range(2):
                if 0 <= lo + k < nzg:
                    buf[k] = x[lo + k]
            return buf
        xp2 = two(a - 2) if a > 0 else None
        xn2 = two(b) if b < nzg else None
        xs = x[a:b].contiguous()
        G, tvs, _, _ = _call(nv, 0, g, xs, xp=xp2, xn=xn2)
        assert torch.equal(G, G_full[a:b]), (scheme, a, b)
        xo, tv1, fids, _ = _call(nv, 1, g, xs, x0[a:b].contiguous(), xp=xp2, xn=xn2)
        assert torch.equal(xo, xo_full[a:b]), (scheme, a, b)
        tv_sum, tv1_sum, fid_sum = tv_sum + tvs, tv1_sum + tv1, fid_sum + fids
    assert abs(tv_sum - tv_full) <= 1e-12 * abs(tv_full)
    assert abs(tv1_sum - tvf) <= 1e-12 * abs(tvf)
    assert abs(fid_sum - fidf) <= 1e-12 * fidf


# =====================================================================================================================
# 5. pitch and bounds
# =====================================================================================================================
def _pads_zero(t):
    """every storage element of the strided view t that is NOT one of its elements is zero"""
    import torch
    n = 1 + sum((int(s) - 1) * int(st) for s, st in zip(t.shape, t.stride()))
    flat = t.as_strided((n,), (1,))
    return int(torch.count_nonzero(flat)) == int(torch.count_nonzero(t))      # (a NaN counts as non-zero on both sides)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,frame,rp,scheme,al", [
    (F32, (65, 250), 256, "hybrid", 1), (F32, (65, 250), 256, "central", 1),          # form A
    (F32, (65, 250), 256, "upwind", 1), (F32, (65, 250), 256, "downwind", 1),         # form B: the last aligned tile ends in the pad columns
    (F32, (65, 250), 256, "upwind", 0), (F32, (65, 250), 256, "downwind", 0),         # form C at its smallest width
    (F64, (33, 190), 192, "hybrid", 1), (F64, (33, 190), 192, "central", 1),          # form D
    (F64, (33, 190), 192, "upwind", 1), (F64, (33, 190), 192, "downwind", 1),         # form D (MODE 0) / E (MODE 1)
], ids=lambda v: v if isinstance(v, str) else (np.dtype(v).name if isinstance(v, type) else str(v).replace(" ", "")))
def test_pitched_rows_through_interior_tiles(nv, dtype, frame, rp, scheme, al, tvopt):
    """rows of 250 / 190 elements on a pitch of 256 / 192, frames with slack: bit-equal to the dense call, pads left zero"""
    import torch
    if al == 0:
        tvopt("TV_SG_ALIGNED", 0)
    shape = (3, 3) + frame
    fp = frame[0] * rp + 64
    for mode in (0, 1):
        assert _nonempty(interior_rect(shape, scheme, dtype, mode, al)), mode
    rng = np.random.default_rng(8)
    xh = (rng.standard_normal(shape) * 10).astype(dtype)
    x0h = (rng.standard_normal(shape) * 10).astype(dtype)
    dev = torch.device("cuda", 0)
    kw = dict(reg_z_over_reg=LZ, reg_time=MU)
    gd = nv.Geometry(shape, scheme, _tdt(dtype), dev, **kw)
    gp = nv.Geometry(shape, scheme, _tdt(dtype), dev, row_pitch=rp, frame_pitch=fp, **kw)
    assert gp.pitched
    xd, x0d = torch.as_tensor(xh).cuda(), torch.as_tensor(x0h).cuda()
    xp, x0p = gp.new_image(), gp.new_image()
    xp.copy_(xd)
    x0p.copy_(x0d)
    assert xp.stride()[-2] == rp and xp.stride()[-3] == fp
    for mode in (0, 1):
        dense, tvd, fidd, _ = _call(nv, mode, gd, xd, x0d)
        out = gp.new_image()
        out[...] = float("nan")                       # the elements only: the pads stay zero
        out, tvp, fidp, _ = _call(nv, mode, gp, xp, x0p, out=out)
        assert torch.equal(out, dense), (scheme, mode)
        assert bool(torch.isfinite(dense).all())
        assert _pads_zero(out) and _pads_zero(xp) and _pads_zero(x0p)
        assert abs(tvp - tvd) <= 1e-12 * abs(tvd) and abs(fidp - fidd) <= 1e-12 * max(abs(fidd), 1e-300)


@pytest.mark.gpu
@pytest.mark.parametrize("form,scheme", [p for p in _form_schemes() if p.values[0] in "ABDE"])
def test_nothing_outside_the_arrays_is_written(nv, form, scheme, tvopt):
    """x, x0, G / x_out and norms between NaN bands of 4100 elements on the frames with interior tiles: the bands survive, everything
    inside is finite"""
    import torch
    f = FORMS[form]
    al, modes = _reach(form, scheme)
    if al == 0:
        tvopt("TV_SG_ALIGNED", 0)
    shape = (4, 8) + f.main
    n = int(np.prod(shape))
    rng = np.random.default_rng(3)
    dt = _tdt(f.dtype)
    bufs = {k: torch.full((n + 2 * PAD,), float("nan"), dtype=dt, device="cuda") for k in ("x", "x0", "out", "norms")}
    v = {k: b[PAD:PAD + n].view(shape) for k, b in bufs.items()}
    v["x"].copy_(torch.as_tensor((rng.standard_normal(shape) * 10).astype(f.dtype)).cuda())
    v["x0"].copy_(torch.as_tensor((rng.standard_normal(shape) * 10).astype(f.dtype)).cuda())
    g = nv.Geometry(shape, scheme, dt, torch.device("cuda", 0), reg_z_over_reg=1.2, reg_time=0.8)
    for mode in modes:
        assert _nonempty(interior_rect(shape, scheme, f.dtype, mode, al))
        v["out"].fill_(float("nan"))
        v["norms"].fill_(float("nan"))
        _, tv, fid, _ = _call(nv, mode, g, v["x"], v["x0"], out=v["out"], norms=v["norms"])
        for k, b in bufs.items():
            assert bool(torch.isnan(b[:PAD]).all() and torch.isnan(b[-PAD:]).all()), (mode, k)
        assert bool(torch.isfinite(v["out"]).all()) and np.isfinite(tv) and np.isfinite(fid), mode
        assert bool(torch.isfinite(v["x"]).all()) and bool(torch.isfinite(v["x0"]).all())
        if mode == 2:
            # written everywhere and positive; +inf (the reference's convention for |Dx| == 0) exactly at the voxels that have no
            # difference at all on random data: the last corner of the volume for the forward differences of upwind, the first one
            # for downwind, all 16 corners for central, none for hybrid
            assert not bool(torch.isnan(v["norms"]).any()) and bool((v["norms"] > 0).all())
            ends = {"upwind": (-1,), "downwind": (0,), "central": (0, -1), "hybrid": ()}[scheme]
            want_inf = torch.zeros(shape, dtype=torch.bool, device="cuda")
            for iz in ends:
                for it in ends:
                    for iy in ends:
                        for ix in ends:
                            want_inf[iz, it, iy, ix] = True
            assert torch.equal(torch.isinf(v["norms"]), want_inf)
        else:
            assert bool(torch.isnan(v["norms"]).all())          # not an argument of this entry point: untouched


# =====================================================================================================================
# 6. the solver on a frame with interior tiles
# =====================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("form,scheme", [p for p in _form_schemes() if p.values[0] in "AB"])
def test_subgradient_descent_on_an_interior_frame(form, scheme, dtype):
    """SubgradientDescent(one_pass=True), 5 iterations, against the oracle's loop; the bars of test_subgradient_descent_pitched.
    In fp64 the same frames run forms D (hybrid / central) and E (upwind / downwind: the step is MODE 1)."""
    import torch
    import pytv
    shape = (5, 3) + FORMS[form].main
    assert _nonempty(interior_rect(shape, scheme, dtype, 1))
    rng = np.random.default_rng(3)
    x0 = (orc.phantom(shape, dtype=np.float64) + 100 * rng.random(shape)).astype(dtype)
    kw = dict(scheme=scheme, reg_z_over_reg=0.7, reg_time=1.3)
    sg = pytv.solvers.SubgradientDescent(torch.as_tensor(x0).cuda(), 2.0, 0.05, one_pass=True, **kw)
    assert sg.one_pass and not sg.small
    loss = sg.run(5)
    wx, wloss = orc.subgradient_descent(x0.astype(np.float64), 5, 2.0, 0.05, **kw)
    got = sg.result().cpu().numpy()
    f32 = dtype == F32
    print("OBS solver %s %s %s loss max_rel=%.2e x max_abs=%.2e" % (form, scheme, np.dtype(dtype).name,
                                                                   float(np.abs(loss / wloss - 1).max()), float(np.abs(got - wx).max())))
    np.testing.assert_allclose(loss, wloss, rtol=2e-5 if f32 else 1e-10)
    np.testing.assert_allclose(got, wx, rtol=1e-4 if f32 else 1e-9, atol=1e-3 if f32 else 1e-9)
