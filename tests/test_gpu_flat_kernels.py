"""The flat grid-stride kernels of csrc/tv_kernels.hip (TV_FLAT_LAUNCH: k_sub, k_dot, k_cg1, k_cg2, k_cgcg + k_cgcg_advance, k_axpby,
k_cpop_p, k_cpop_res, k_sgstep) called directly through their nine C entry points, at the places where such kernels go wrong:
lengths that are no multiple of the 16-byte lane, pointers that are not 16-byte aligned (all of them, or one only), a second trip of
the grid-stride loop, pitched storage (the pads are part of the vector and must stay zero), the documented minimum workspace, and
the breakdown guards of the conjugate-gradient scalars.

Reference: the operation as include/pytv4d.h states it, in NumPy fp64, from exactly the device's inputs (random normal x 10, cast to
the dtype under test, then widened).

Element-wise bound: |got_i - ref_i| <= (k + 1) eps_T M_i, where M_i is the expression with every term replaced by its absolute
value and k counts its floating-point operations plus the casts of its coefficients to T (written next to each operation below).
Each rounding contributes at most u = eps_T / 2 relative to M_i, so the kernel is within k u (1 + O(u)) <= (k + 1) u; the other half
of (k + 1) eps_T covers the fp64 reference's own k roundings when T is fp64.  FMA contraction removes roundings and only tightens
this.  The V = 1 and V > 1 instantiations are never compared bit for bit: their contraction may differ.

Reduced scalars (fp64 sums formed from what the kernel stored) are recomputed on the host from the device's own output array and must
agree to 1e-12 (the project's figure for fp64 sums, test_gpu_admm_ops.py): a wrong factor or a missed block then fails at 1e-12
instead of hiding inside an fp32 tolerance.

Every array handed to an entry point is a view into a larger buffer with GUARD sentinel elements on both sides; after the call the
sentinels, and every read-only input, must be bit-unchanged."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64                      # sentinel elements before and after every array (64 elements keep the 16-byte alignment in both dtypes)
SENT = -7777.25                 # the sentinel: finite, non-zero, exact in fp32
BLOCKS = 2048                   # kFlatBlocks of csrc/tv_host.h
S1 = BLOCKS * 256               # elements of one trip of the scalar (V = 1) instantiation
DTYPES = [np.float32, np.float64]
NAN = float("nan")
POOL_N = 2 * 2 * 513 * 1024 + 16 * 1009 + 64


@pytest.fixture(scope="module")
def nv():
    import pytv  # noqa: F401
    from pytv import _native
    return _native


def _lanes(dtype):
    return 16 // np.dtype(dtype).itemsize


_POOL = {}


def _vals(dtype, n, k):
    """operand k of a case: n values (random normal x 10 cast to dtype) from one pool per dtype that is drawn once and never written"""
    key = np.dtype(dtype).name
    if key not in _POOL:
        p = (np.random.default_rng(20241019).standard_normal(POOL_N) * 10).astype(dtype)
        p.setflags(write=False)
        _POOL[key] = p
    assert k < 16 and k * 1009 + n <= POOL_N
    return _POOL[key][k * 1009:k * 1009 + n]


def _same_bits(a, b):
    u = "u%d" % a.dtype.itemsize
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(u), b.view(u)))


def _f64(a):
    return np.asarray(a, dtype=np.float64)


class Buf:
    """`values` on the device between two guard bands; `off` elements of extra sentinel in front move the view off the 16-byte
    alignment of the allocation"""

    def __init__(self, values, off=0):
        import torch
        values = np.ascontiguousarray(values).reshape(-1)
        self.n, self.lo = values.size, GUARD + off
        self.host = np.full(self.lo + self.n + GUARD, SENT, dtype=values.dtype)
        self.host[self.lo:self.lo + self.n] = values
        self.dev = torch.as_tensor(self.host).cuda()
        assert self.dev.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.lo * self.host.itemsize

    def read(self):
        """the array as it is on the device now; the guard bands must be bit-unchanged"""
        now = self.dev.cpu().numpy()
        hi = self.lo + self.n
        assert _same_bits(now[:self.lo], self.host[:self.lo]), "guard band in front of the array was written"
        assert _same_bits(now[hi:], self.host[hi:]), "guard band behind the array was written"
        return now[self.lo:hi]

    def assert_unchanged(self):
        assert _same_bits(self.dev.cpu().numpy(), self.host), "a read-only input (or its guard band) was written"


def _scalar(v=SENT):
    return Buf(np.array([v], dtype=np.float64))


def _elementwise(got, ref, M, k, dtype, what):
    """|got - ref| <= (k + 1) eps_T M, element by element (a NaN anywhere fails)"""
    bound = (k + 1) * float(np.finfo(dtype).eps) * M
    err = np.abs(_f64(got) - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: %d of %d elements beyond (k + 1) eps M with k = %d; first at %d: got %r, reference %r, bound %.3g"
                             % (what, int(bad.sum()), bad.size, k, i, got[i], ref[i], bound[i]))


def _sum_close(got, want, what):
    assert abs(got - want) <= 1e-12 * abs(want), "%s: got %.17g, from the stored array %.17g" % (what, got, want)


def _code(nv, dtype):
    return nv.TV_F32 if dtype == np.float32 else nv.TV_F64


def _stream(nv):
    import torch
    return nv.current_stream(torch.device("cuda"))


# =====================================================================================================================================
# raw-length entry points: tv_sub, tv_cpop_p, tv_cpop_residual
# =====================================================================================================================================
def _lengths(dtype):
    V = _lanes(dtype)
    T1 = BLOCKS * 256 * V          # exactly one trip of the 16-byte-lane instantiation
    return [0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, T1, T1 + V, S1 + 1]      # S1 + 1 is odd: two trips on the scalar path


def _placements(dtype, operands):
    """element offsets of the operands from a 16-byte boundary: all aligned; all off by one; fp32 also all off by two (8-byte aligned
    only); exactly one operand off by one, each in turn (the call must still be right, on the scalar path)"""
    yield (0,) * operands
    yield (1,) * operands
    if dtype == np.float32:
        yield (2,) * operands
    for j in range(operands):
        yield tuple(1 if i == j else 0 for i in range(operands))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sub(nv, dtype):
    lib, st = nv.lib(), _stream(nv)
    for n in _lengths(dtype):
        a, b = _vals(dtype, n, 0), _vals(dtype, n, 1)
        ref, M = _f64(a) - _f64(b), np.abs(_f64(a)) + np.abs(_f64(b))
        for offs in _placements(dtype, 3):
            A, B, O = Buf(a, offs[0]), Buf(b, offs[1]), Buf(np.full(n, NAN, dtype), offs[2])
            assert lib.tv_sub(_code(nv, dtype), n, A.ptr, B.ptr, O.ptr, st) == 0
            out = O.read()                                             # n == 0: nothing but guard band, which must be unchanged
            A.assert_unchanged(), B.assert_unchanged()
            _elementwise(out, ref, M, 1, dtype, "tv_sub n=%d offsets %s" % (n, offs))        # out = a - b: k = 1 (sub)


def _check_cpop_p(nv, dtype, n, offs, sigma):
    lib, st = nv.lib(), _stream(nv)
    p, r = _vals(dtype, n, 2), _vals(dtype, n, 3)
    Pb, R = Buf(p, offs[0]), Buf(r, offs[1])
    assert lib.tv_cpop_p(_code(nv, dtype), n, Pb.ptr, R.ptr, sigma, st) == 0
    out = Pb.read()
    R.assert_unchanged()
    # p <- inv * (p + sigma * r), inv = (T)(1 / (1 + sigma_A)), sigma = (T)sigma_A: k = 5 (two casts, mul, add, mul)
    ref = (_f64(p) + sigma * _f64(r)) / (1.0 + sigma)
    M = (np.abs(_f64(p)) + sigma * np.abs(_f64(r))) / (1.0 + sigma)
    _elementwise(out, ref, M, 5, dtype, "tv_cpop_p n=%d offsets %s sigma_A=%g" % (n, offs, sigma))
    return p, out


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpop_p(nv, dtype):
    for n in _lengths(dtype):
        for offs in _placements(dtype, 2):
            _check_cpop_p(nv, dtype, n, offs, 0.7)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpop_p_step_sizes(nv, dtype):
    """sigma_A = 0 is the identity on p, bit for bit (inv = 1, p + 0 r = p); sigma_A = 1e6 stays within the same bound"""
    for n in _lengths(dtype):
        for offs in ((0, 0), (1, 1)):
            p, out = _check_cpop_p(nv, dtype, n, offs, 0.0)
            assert _same_bits(out, np.ascontiguousarray(p)), (n, offs)
            _check_cpop_p(nv, dtype, n, offs, 1e6)


def _check_cpop_residual(nv, dtype, n, offs):
    lib, st = nv.lib(), _stream(nv)
    ax, b = _vals(dtype, n, 4), _vals(dtype, n, 5)
    AX, B, R = Buf(ax, offs[0]), Buf(b, offs[1]), Buf(np.full(n, NAN, dtype), offs[2])
    # the documented minimum, "ws: >= 2048 doubles", between guard bands; NaN inside: a block that wrote no partial sum shows in *fid
    WS, FID = Buf(np.full(BLOCKS, NAN, np.float64)), _scalar()
    assert lib.tv_cpop_residual(_code(nv, dtype), n, AX.ptr, B.ptr, R.ptr, FID.ptr, WS.ptr, st) == 0
    r, fid = R.read(), FID.read()[0]
    WS.read()
    AX.assert_unchanged(), B.assert_unchanged()
    what = "tv_cpop_residual n=%d offsets %s" % (n, offs)
    _elementwise(r, _f64(ax) - _f64(b), np.abs(_f64(ax)) + np.abs(_f64(b)), 1, dtype, what)      # r = ax - b: k = 1 (sub)
    if n == 0:
        assert fid == 0.0 and not np.signbit(fid), what                 # *fid is cleared, nothing else is written
        WS.assert_unchanged()
    else:
        _sum_close(fid, 0.5 * float(np.sum(_f64(r) ** 2)), what + ": *fid = 1/2 |r|^2")


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpop_residual(nv, dtype):
    for n in _lengths(dtype):
        for offs in _placements(dtype, 3):
            _check_cpop_residual(nv, dtype, n, offs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpop_residual_needs_no_more_than_2048_doubles_of_workspace(nv, dtype):
    """every call of _check_cpop_residual passes exactly 2048 doubles between sentinels; here at the lengths where every one of the
    2048 blocks has work and where the last block's share is ragged"""
    V = _lanes(dtype)
    for n in (S1 - 1, S1, S1 * V - V, S1 * V + V * 255):
        for offs in ((0, 0, 0), (1, 1, 1)):
            _check_cpop_residual(nv, dtype, n, offs)


# =====================================================================================================================================
# geometry entry points: tv_dot, tv_cg_step1, tv_cg_step2, tv_cg_update, tv_axpby, tv_subgrad_step
# =====================================================================================================================================
DENSE = [(1, 1, 1, 1),            # one element
         (1, 1, 3, 5),            # odd: scalar path
         (2, 3, 5, 8),            # 16-byte-lane path
         (1, 1, 723, 727),        # 525 621 elements, odd: a second trip on the scalar path
         (2, 2, 513, 1024)]       # 2 101 248 elements: a second trip on the 16-byte-lane path in both dtypes
PITCHED = ((2, 3, 5, 6), 8, 48)   # shape, row_pitch, frame_pitch: two pad columns per row and one pad row per frame


def _torch_dtype(dtype):
    import torch
    return torch.float32 if dtype == np.float32 else torch.float64


def _dense_layouts(nv, dtype, shapes=DENSE):
    """(geometry, elements, offset) for every dense shape, as an aligned view and as a view one element off the alignment"""
    for shape in shapes:
        g = nv.Geometry(shape, "upwind", _torch_dtype(dtype), "cuda")
        for off in (0, 1):
            yield g, int(np.prod(shape)), off


def _ws(nv, g):
    """the geometry's workspace, NaN-filled: a block that wrote no partial sum shows in the reduced scalar"""
    ws = g.workspace()
    ws.fill_(NAN)
    return nv.ptr(ws)


# ---- tv_dot -------------------------------------------------------------------------------------------------------------------------
def _run_dot(nv, g, a, b, off):
    """b is None: the same array twice"""
    A = Buf(a, off)
    B = A if b is None else Buf(b, off)
    RES = _scalar()
    nv.check(nv.lib().tv_dot(g.ref, A.ptr, B.ptr, RES.ptr, _ws(nv, g), _stream(nv)))
    got = RES.read()[0]
    A.assert_unchanged(), B.assert_unchanged()
    _sum_close(got, float(np.sum(_f64(a) * _f64(a if b is None else b))), "tv_dot %s off %d" % (g.shape, off))
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_dot(nv, dtype):
    for g, n, off in _dense_layouts(nv, dtype):
        _run_dot(nv, g, _vals(dtype, n, 0), None, off)
        _run_dot(nv, g, _vals(dtype, n, 0), _vals(dtype, n, 1), off)


# ---- tv_cg_step1 --------------------------------------------------------------------------------------------------------------------
def _run_cg1(nv, g, dtype, x, r, d, Ad, rs, dAd, off):
    X, R, D, AD = Buf(x, off), Buf(r, off), Buf(d, off), Buf(Ad, off)
    RS, DAD, NEW = _scalar(rs), _scalar(dAd), _scalar()
    nv.check(nv.lib().tv_cg_step1(g.ref, X.ptr, R.ptr, D.ptr, AD.ptr, RS.ptr, DAD.ptr, NEW.ptr, _ws(nv, g), _stream(nv)))
    xn, rn, rs_new = X.read(), R.read(), NEW.read()[0]
    for b in (D, AD, RS, DAD):
        b.assert_unchanged()
    what = "tv_cg_step1 %s off %d dAd=%g" % (g.shape, off, dAd)
    if dAd > 0.0:
        al = rs / dAd
        # x + alpha d and r - alpha Ad with alpha = (T)(rs / dAd): k = 3 each (cast, mul, add)
        _elementwise(xn, _f64(x) + al * _f64(d), np.abs(_f64(x)) + abs(al) * np.abs(_f64(d)), 3, dtype, what + ": x")
        _elementwise(rn, _f64(r) - al * _f64(Ad), np.abs(_f64(r)) + abs(al) * np.abs(_f64(Ad)), 3, dtype, what + ": r")
    else:
        # breakdown (include/pytv4d.h): alpha = 0, nothing moves
        assert _same_bits(xn, np.ascontiguousarray(x)) and _same_bits(rn, np.ascontiguousarray(r)), what
    _sum_close(rs_new, float(np.sum(_f64(rn) ** 2)), what + ": *rs_new = <r, r>")
    return xn, rn, rs_new


@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_step1(nv, dtype):
    for g, n, off in _dense_layouts(nv, dtype):
        _run_cg1(nv, g, dtype, *(_vals(dtype, n, k) for k in range(4)), 3.7, 5.3, off)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_step1_breakdown_leaves_x_and_r_alone(nv, dtype):
    """dAd <= 0: alpha = 0, x and r bit-unchanged, *rs_new = <r, r>"""
    for g, n, off in _dense_layouts(nv, dtype):
        for dAd in (0.0, -5.3):
            _run_cg1(nv, g, dtype, *(_vals(dtype, n, k) for k in range(4)), 3.7, dAd, off)


# ---- tv_cg_step2 --------------------------------------------------------------------------------------------------------------------
def _run_cg2(nv, g, dtype, d, r, rs_new, rs, off):
    D, R, NEW, RS = Buf(d, off), Buf(r, off), _scalar(rs_new), _scalar(rs)
    nv.check(nv.lib().tv_cg_step2(g.ref, D.ptr, R.ptr, NEW.ptr, RS.ptr, _stream(nv)))
    dn = D.read()
    for b in (R, NEW, RS):
        b.assert_unchanged()
    what = "tv_cg_step2 %s off %d rs=%g" % (g.shape, off, rs)
    if rs > 0.0:
        be = rs_new / rs
        # r + beta d with beta = (T)(rs_new / rs): k = 3 (cast, mul, add)
        _elementwise(dn, _f64(r) + be * _f64(d), np.abs(_f64(r)) + abs(be) * np.abs(_f64(d)), 3, dtype, what)
    else:
        assert _same_bits(dn, np.ascontiguousarray(r)), what           # breakdown: beta = 0, d becomes r exactly
    return dn


@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_step2(nv, dtype):
    for g, n, off in _dense_layouts(nv, dtype):
        _run_cg2(nv, g, dtype, _vals(dtype, n, 0), _vals(dtype, n, 1), 2.9, 3.7, off)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_step2_restarts_when_rs_is_zero(nv, dtype):
    for g, n, off in _dense_layouts(nv, dtype):
        _run_cg2(nv, g, dtype, _vals(dtype, n, 0), _vals(dtype, n, 1), 2.9, 0.0, off)


# ---- tv_cg_update -------------------------------------------------------------------------------------------------------------------
def _cgcg_scalars(sc):
    """the recurrence of include/pytv4d.h with its breakdown guards, in the order csrc/tv_kernels.hip evaluates it"""
    gamma, delta, gamma_old, alpha_old = (float(v) for v in sc)
    first = alpha_old == 0.0
    beta = gamma / gamma_old if (not first and gamma_old > 0.0) else 0.0
    den = delta if first else delta - beta * gamma / alpha_old
    alpha = gamma / den if den > 0.0 else 0.0
    return alpha, beta, first


def _run_cg_update(nv, g, dtype, v, sc, x0, off):
    """one tv_cg_update on v = {x, r, d, s, w} with the scalars sc; returns the new vectors, the advanced sc and *fid (or None)"""
    B = {k: Buf(v[k], off) for k in "xrdsw"}
    SC = Buf(np.asarray(sc, dtype=np.float64))
    X0 = None if x0 is None else Buf(x0, off)
    FID = None if x0 is None else _scalar()
    nv.check(nv.lib().tv_cg_update(g.ref, B["x"].ptr, B["r"].ptr, B["d"].ptr, B["s"].ptr, B["w"].ptr, SC.ptr,
                                   None if x0 is None else X0.ptr, None if x0 is None else FID.ptr, _ws(nv, g), _stream(nv)))
    new = {k: B[k].read() for k in "xrds"}
    B["w"].assert_unchanged()
    sc_new = SC.read()
    al, be, first = _cgcg_scalars(sc)
    what = "tv_cg_update %s off %d sc=%s" % (g.shape, off, list(sc))
    x, r, d, s, w = (_f64(v[k]) for k in "xrdsw")
    if first:
        # d = r, s = w: copies; what d and s held before (NaN in these tests) must not leak in
        assert _same_bits(new["d"], np.ascontiguousarray(v["r"])) and _same_bits(new["s"], np.ascontiguousarray(v["w"])), what
        dn, sn, Md, Ms, kd = r, w, np.abs(r), np.abs(w), 0
    else:
        # d = r + beta d and s = w + beta s with beta = (T)beta: k = 3 each (cast, mul, add)
        dn, sn, Md, Ms, kd = r + be * d, w + be * s, np.abs(r) + abs(be) * np.abs(d), np.abs(w) + abs(be) * np.abs(s), 3
        _elementwise(new["d"], dn, Md, 3, dtype, what + ": d")
        _elementwise(new["s"], sn, Ms, 3, dtype, what + ": s")
    if al != 0.0:
        # x + alpha d_new and r - alpha s_new with alpha = (T)alpha: k = 3 (cast, mul, add) on top of the kd operations of d_new / s_new
        _elementwise(new["x"], x + al * dn, np.abs(x) + abs(al) * Md, 3 + kd, dtype, what + ": x")
        _elementwise(new["r"], r - al * sn, np.abs(r) + abs(al) * Ms, 3 + kd, dtype, what + ": r")
    else:
        # breakdown (den <= 0): alpha = 0, x and r bit-unchanged
        assert _same_bits(new["x"], np.ascontiguousarray(v["x"])) and _same_bits(new["r"], np.ascontiguousarray(v["r"])), what
    # sc[0], sc[1] are the caller's; sc[2] = gamma; sc[3] = alpha, or 1e-300 in place of 0 ("0 means first step" stays true)
    assert sc_new[0] == sc[0] and sc_new[1] == sc[1] and sc_new[2] == sc[0], what
    if al != 0.0:
        assert abs(sc_new[3] - al) <= 1e-12 * abs(al), what
    else:
        assert sc_new[3] == 1e-300, what
    fid = None
    if x0 is not None:
        X0.assert_unchanged()
        fid = FID.read()[0]
        _sum_close(fid, 0.5 * float(np.sum((_f64(new["x"]) - _f64(x0)) ** 2)), what + ": *fid = 1/2 |x_new - x0|^2")
    return new, sc_new, fid


def _cg_vectors(dtype, n, make=None):
    """x, r, w random; d, s NaN (the first step must not read them)"""
    make = make or (lambda a: a)
    v = {k: make(_vals(dtype, n, i)) for i, k in enumerate("xrw")}
    v["d"], v["s"] = make(np.full(n, NAN, dtype)), make(np.full(n, NAN, dtype))
    return v


def _two_cg_steps(nv, g, dtype, n, off, x0_first, make=None):
    """a first step (sc[3] == 0) and a second one fed from the advanced sc, one with x0 / fid and one without; returns the two fids"""
    make = make or (lambda a: a)
    v = _cg_vectors(dtype, n, make)
    x0 = make(_vals(dtype, n, 5))
    v1, sc1, fid1 = _run_cg_update(nv, g, dtype, v, [3.7, 5.3, 0.0, 0.0], x0 if x0_first else None, off)
    assert sc1[2] == 3.7 and sc1[3] != 0.0
    v1["w"] = make(_vals(dtype, n, 6))
    # beta = 2.9 / 3.7, den = 4.1 - beta 2.9 / (3.7 / 5.3) = 0.84: an ordinary second step
    _, sc2, fid2 = _run_cg_update(nv, g, dtype, v1, [2.9, 4.1, sc1[2], sc1[3]], None if x0_first else x0, off)
    assert sc2[2] == 2.9 and sc2[3] > 0.0
    return fid1, fid2


@pytest.mark.parametrize("x0_first", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_update_first_and_second_step(nv, dtype, x0_first):
    for g, n, off in _dense_layouts(nv, dtype):
        _two_cg_steps(nv, g, dtype, n, off, x0_first)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_update_breakdown(nv, dtype):
    """den <= 0: alpha = 0, so x and r stay bit-unchanged while d = r + beta d and s = w + beta s still advance; sc[2] = sc[0] and
    sc[3] = 1e-300, never 0 -- the step after a broken-down FIRST step is therefore not taken for a first step again"""
    for g, n, off in _dense_layouts(nv, dtype):
        v = _cg_vectors(dtype, n)
        v["d"], v["s"] = _vals(dtype, n, 7), _vals(dtype, n, 8)
        # mid-solve: beta = 2/3, den = 1 - (2/3) 2 / 0.6 < 0
        _run_cg_update(nv, g, dtype, v, [2.0, 1.0, 3.0, 0.6], _vals(dtype, n, 5), off)
        for delta in (0.0, -5.3):
            v = _cg_vectors(dtype, n)
            v1, sc1, _ = _run_cg_update(nv, g, dtype, v, [3.7, delta, 0.0, 0.0], None, off)
            assert sc1[3] == 1e-300
            v1["w"] = _vals(dtype, n, 6)
            _, be, first = _cgcg_scalars([2.9, 4.1, sc1[2], sc1[3]])
            assert not first and be == 2.9 / 3.7
            _run_cg_update(nv, g, dtype, v1, [2.9, 4.1, sc1[2], sc1[3]], None, off)


# ---- tv_axpby -----------------------------------------------------------------------------------------------------------------------
def _run_axpby(nv, g, dtype, a, x, b, y, ref, out, off, stored=None):
    """out: "new" (a NaN-filled array), "x" (in place) or None (the distance alone: `stored` is the array an earlier storing call of
    the same operation left, from which the distance is recomputed)"""
    X = Buf(x, off)
    Y = None if y is None else Buf(y, off)
    REF = None if ref is None else Buf(ref, off)
    OUT = {"new": Buf(np.full(x.size, NAN, dtype), off), "x": X, None: None}[out]
    DIST = None if ref is None else _scalar()
    nv.check(nv.lib().tv_axpby(g.ref, a, X.ptr, b, None if Y is None else Y.ptr, None if REF is None else REF.ptr,
                               None if OUT is None else OUT.ptr, None if DIST is None else DIST.ptr,
                               None if ref is None else _ws(nv, g), _stream(nv)))
    what = "tv_axpby %s off %d y %s ref %s out %s" % (g.shape, off, y is not None, ref is not None, out)
    for buf in (Y, REF) + (() if out == "x" else (X,)):
        if buf is not None:
            buf.assert_unchanged()
    if OUT is not None:
        stored = OUT.read()
        if y is None:
            # (T)a * x: k = 2 (cast, mul)
            _elementwise(stored, a * _f64(x), abs(a) * np.abs(_f64(x)), 2, dtype, what)
        else:
            # (T)a * x + (T)b * y: k = 5 (two casts, two muls, add)
            _elementwise(stored, a * _f64(x) + b * _f64(y), abs(a) * np.abs(_f64(x)) + abs(b) * np.abs(_f64(y)), 5, dtype, what)
    dist = None
    if ref is not None:
        dist = DIST.read()[0]
        _sum_close(dist, float(np.sum((_f64(stored) - _f64(ref)) ** 2)), what + ": *dist2 = |out - ref|^2")
    return stored, dist


def _axpby_forms(nv, g, dtype, n, off, make=None):
    """the four forms of include/pytv4d.h -- y given or NULL, out given or NULL, with and without ref -- and out aliasing x; returns
    the distances"""
    make = make or (lambda a: a)
    x, y, ref = (make(_vals(dtype, n, k)) for k in range(3))
    a, b = 1.7, -0.45
    dists = []
    for yy in (y, None):
        _run_axpby(nv, g, dtype, a, x, b, yy, None, "new", off)                        # out = a x [+ b y]
        _run_axpby(nv, g, dtype, a, x, b, yy, None, "x", off)                          # ... in place
        stored, d1 = _run_axpby(nv, g, dtype, a, x, b, yy, ref, "new", off)            # ... and |out - ref|^2
        _, d2 = _run_axpby(nv, g, dtype, a, x, b, yy, ref, None, off, stored=stored)   # the distance alone, nothing stored
        _, d3 = _run_axpby(nv, g, dtype, a, x, b, yy, ref, "x", off)                   # in place with the distance
        dists += [d1, d2, d3]
    return dists


@pytest.mark.parametrize("dtype", DTYPES)
def test_axpby_forms_and_aliasing(nv, dtype):
    for g, n, off in _dense_layouts(nv, dtype):
        _axpby_forms(nv, g, dtype, n, off)


# ---- tv_subgrad_step ----------------------------------------------------------------------------------------------------------------
def _run_subgrad_step(nv, g, dtype, x, x0, G, step, lam, off):
    X, X0, GG, FID = Buf(x, off), Buf(x0, off), Buf(G, off), _scalar()
    nv.check(nv.lib().tv_subgrad_step(g.ref, X.ptr, X0.ptr, GG.ptr, step, lam, FID.ptr, _ws(nv, g), _stream(nv)))
    xn, fid = X.read(), FID.read()[0]
    X0.assert_unchanged(), GG.assert_unchanged()
    what = "tv_subgrad_step %s off %d" % (g.shape, off)
    # x - step * ((x - x0) + lambda * G) with step = (T)step, lambda = (T)lambda: k = 7 (two casts, sub, mul, add, mul, sub)
    ref = _f64(x) - step * ((_f64(x) - _f64(x0)) + lam * _f64(G))
    M = np.abs(_f64(x)) + abs(step) * ((np.abs(_f64(x)) + np.abs(_f64(x0))) + abs(lam) * np.abs(_f64(G)))
    _elementwise(xn, ref, M, 7, dtype, what)
    # the fidelity of the NEW x
    _sum_close(fid, 0.5 * float(np.sum((_f64(xn) - _f64(x0)) ** 2)), what + ": *fid = 1/2 |x_new - x0|^2")
    return xn, fid


@pytest.mark.parametrize("dtype", DTYPES)
def test_subgrad_step(nv, dtype):
    for g, n, off in _dense_layouts(nv, dtype):
        _run_subgrad_step(nv, g, dtype, *(_vals(dtype, n, k) for k in range(3)), 0.05, 2.5, off)


# =====================================================================================================================================
# pitched storage: the flat kernels run over s_z * nz storage elements, pads included ("pads stay zero", include/pytv4d.h)
# =====================================================================================================================================
class Pitched:
    """the pitched geometry of PITCHED, the dense geometry of the same shape, and `store`: logical values -> the flat storage that
    Geometry.new_image lays out (zeros in the pads)"""

    def __init__(self, nv, dtype):
        shape, rp, fp = PITCHED
        self.shape, self.n = shape, int(np.prod(shape))
        self.g = nv.Geometry(shape, "upwind", _torch_dtype(dtype), "cuda", row_pitch=rp, frame_pitch=fp)
        self.dense = nv.Geometry(shape, "upwind", _torch_dtype(dtype), "cuda")
        assert self.g.pitched and self.g.image_elems == shape[0] * shape[1] * fp == 288
        ones = self.store(np.ones(self.n, dtype))
        self.pad = ones == 0
        assert int(self.pad.sum()) == 288 - self.n

    def store(self, values):
        import torch
        img = self.g.new_image()
        img.copy_(torch.as_tensor(np.array(values).reshape(self.shape)))
        assert tuple(img.stride()) == (144, 48, 8, 1) and img.storage_offset() == 0
        return img.as_strided((self.g.image_elems,), (1,)).cpu().numpy()

    def pads_zero(self, *arrays):
        for a in arrays:
            assert a.shape == self.pad.shape and not np.any(a[self.pad] != 0), "a pad element is no longer zero"


def _scalars_agree(pitched, dense):
    for p, d in zip(pitched, dense):
        assert (p is None) == (d is None)
        if p is not None:
            assert abs(p - d) <= 1e-12 * abs(d), (p, d)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pitched_dot(nv, dtype):
    P = Pitched(nv, dtype)
    a, b = _vals(dtype, P.n, 0), _vals(dtype, P.n, 1)
    for off in (0, 1):
        got = [_run_dot(nv, P.g, P.store(a), None, off), _run_dot(nv, P.g, P.store(a), P.store(b), off)]
        _scalars_agree(got, [_run_dot(nv, P.dense, a, None, off), _run_dot(nv, P.dense, a, b, off)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_pitched_cg_step1(nv, dtype):
    P = Pitched(nv, dtype)
    v = [_vals(dtype, P.n, k) for k in range(4)]
    for off in (0, 1):
        for dAd in (5.3, 0.0):
            xp, rp, sp = _run_cg1(nv, P.g, dtype, *(P.store(a) for a in v), 3.7, dAd, off)
            P.pads_zero(xp, rp)
            _, _, sd = _run_cg1(nv, P.dense, dtype, *v, 3.7, dAd, off)
            _scalars_agree([sp], [sd])


@pytest.mark.parametrize("dtype", DTYPES)
def test_pitched_cg_step2(nv, dtype):
    P = Pitched(nv, dtype)
    d, r = _vals(dtype, P.n, 0), _vals(dtype, P.n, 1)
    for off in (0, 1):
        for rs in (3.7, 0.0):
            P.pads_zero(_run_cg2(nv, P.g, dtype, P.store(d), P.store(r), 2.9, rs, off))


@pytest.mark.parametrize("dtype", DTYPES)
def test_pitched_cg_update(nv, dtype):
    P = Pitched(nv, dtype)
    for off in (0, 1):
        for x0_first in (True, False):
            got = _two_cg_steps(nv, P.g, dtype, P.n, off, x0_first, make=P.store)
            _scalars_agree(got, _two_cg_steps(nv, P.dense, dtype, P.n, off, x0_first))
        # the written arrays of a first and a second step: pads zero (d and s enter the first step with NaN in every element proper)
        v = _cg_vectors(dtype, P.n, P.store)
        v1, sc1, _ = _run_cg_update(nv, P.g, dtype, v, [3.7, 5.3, 0.0, 0.0], None, off)
        P.pads_zero(*(v1[k] for k in "xrds"))
        v1["w"] = P.store(_vals(dtype, P.n, 6))
        v2, _, _ = _run_cg_update(nv, P.g, dtype, v1, [2.9, 4.1, sc1[2], sc1[3]], P.store(_vals(dtype, P.n, 5)), off)
        P.pads_zero(*(v2[k] for k in "xrds"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_pitched_axpby(nv, dtype):
    P = Pitched(nv, dtype)
    x, y = _vals(dtype, P.n, 0), _vals(dtype, P.n, 1)
    for off in (0, 1):
        _scalars_agree(_axpby_forms(nv, P.g, dtype, P.n, off, make=P.store), _axpby_forms(nv, P.dense, dtype, P.n, off))
        for yy in (y, None):
            for out in ("new", "x"):
                stored, _ = _run_axpby(nv, P.g, dtype, 1.7, P.store(x), -0.45, None if yy is None else P.store(yy), None, out, off)
                P.pads_zero(stored)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pitched_subgrad_step(nv, dtype):
    P = Pitched(nv, dtype)
    v = [_vals(dtype, P.n, k) for k in range(3)]
    for off in (0, 1):
        xp, fp = _run_subgrad_step(nv, P.g, dtype, *(P.store(a) for a in v), 0.05, 2.5, off)
        P.pads_zero(xp)
        _, fd = _run_subgrad_step(nv, P.dense, dtype, *v, 0.05, 2.5, off)
        _scalars_agree([fp], [fd])
