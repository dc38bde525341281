"""GPU tests (pytest -m gpu) of PRE set propagation, cp_pre_amd/csrc/set_prop.hip, at its seams: ``setprop_kernel<TK, MODE>``
called through the C ABI (``_lib.load_setprop().pre_setprop_*``) at row lengths on both sides of every tile width, batches
on both sides of every row group, chunk remainders 0 / 1 / 31, tables shorter than the staged window, non-finite rows next to
finite ones in one workgroup, a centre that overflows in some columns, every layout the header allows, and the recipe's
edges (no interior, every tap wrapping, q-hat steps that leave the field) - and, last, through ``set_prop.propagate`` and
``set_pre_bounds``.  Integer rows, taps and tables are compared bit for bit with the loops of tests/setprop_helpers.py
(checked on the CPU by tests/test_setprop_ref_cpu.py), random floats element by element within the bound
tests/test_gpu_set_prop.py uses.  Outputs lie inside larger allocations filled with NaN that must be unchanged around them;
strided inputs and the tables carry NaN wherever no element lies.  tests/ODE_TESTS.md says which branch each shape reaches."""
import ctypes

import numpy as np
import pytest
import torch

import setprop_helpers as sh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PRE_E_SHAPE, PRE_E_UNSUPPORTED = -2, -3
F64, CORRELATION = 1, 2
KINDS = ("dense", "transposed", "comp20", "negBT", "pitch3", "negB", "comp31", "negT")
SHO_K = np.array([1., -2., 1.]) + (10 / 99) ** 2 * np.array([0., 1., 0.])
K5 = np.array([-1 / 12, 4 / 3, -5 / 2, 4 / 3, -1 / 12])
K7 = np.array([1 / 90, -3 / 20, 3 / 2, -49 / 18, 3 / 2, -3 / 20, 1 / 90])


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    from cp_pre_amd import _lib
    _lib.load_setprop()
    return torch.device(DEV)


def _L():
    from cp_pre_amd import _lib
    return _lib, _lib.load_setprop()


def source(data, kind="dense", dtype=np.float32):
    return sh.Source(data, kind, device=DEV, dtype=dtype, lead=int(kind[5]) if kind.startswith("comp") else 0)


class Table:
    """N doubles on the device with four NaN on either side: a table read one entry off its end meets one"""

    def __init__(self, values):
        buf = np.full(len(values) + 8, np.nan)
        buf[4:-4] = values
        self.dev = torch.from_numpy(buf).to(DEV)
        self.ptr = ctypes.c_void_p(self.dev.data_ptr() + 32)


def P(x):
    return ctypes.c_void_p(x.ptr) if x is not None else ctypes.c_void_p(0)


def bounds(cs, rs, B, N, g, a, f64, off=0, times=1, expect=0):
    """pre_setprop_bounds_f64 into framed lower / upper [B, N]; returns [(lo, hi)] after each call"""
    _lib, lib = _L()
    lo = sh.Framed(np.arange(B * N), torch.float64, off, DEV)
    hi = sh.Framed(np.arange(B * N), torch.float64, 1 - off, DEV)
    tg, ta = Table(g), Table(a)
    out = []
    for _ in range(times):
        rc = lib.pre_setprop_bounds_f64(P(cs), _lib.iarr64(cs.strides), P(rs), _lib.iarr64(rs.strides), B, N, tg.ptr, ta.ptr,
                                        P(lo), P(hi), F64 if f64 else 0, _lib.stream())
        torch.cuda.synchronize()
        assert rc == expect and lo.untouched() and hi.untouched(), (B, N, rc)
        out.append((lo.get().reshape(B, N), hi.get().reshape(B, N)))
    return out


def check_bounds_exact(c, r, g, a, f64, c_kind="dense", r_kind="dense", off=0):
    B, N = c.shape
    dt = np.float64 if f64 else np.float32
    cs, rs = source(c, c_kind, dt), source(r, r_kind, dt)
    sh.assert_exact_f64(sh.bounds_magnitude(cs.data, rs.data, g, a), cs.data, rs.data, g, a)
    (lo, hi), (lo2, hi2) = bounds(cs, rs, B, N, g, a, f64, off, times=2)
    want_lo, want_hi = sh.bounds_ref(cs.data, rs.data, g, a)
    sh.same_f64(lo, want_lo)
    sh.same_f64(hi, want_hi)
    assert np.array_equal(lo.view(np.int64), lo2.view(np.int64)) and np.array_equal(hi.view(np.int64), hi2.view(np.int64))
    return lo, hi


# ================================================================================================ pre_setprop_bounds_f64
@pytest.mark.parametrize("N", sh.NS)
def test_bounds_shapes_by_branch(gpu, N):
    """every N of the table at B = 1, RB - 1, RB, RB + 1, fp32 and fp64 rows: integer rows and integer tables, bit for bit"""
    rng = np.random.default_rng(N)
    g, a = sh.int_tables(rng, N)
    for n, B in enumerate(sh.batches(N)):
        sh.assert_plan(B, N)
        c, r = sh.ints(rng, -3, 3, B, N), sh.ints(rng, 0, 3, B, N)
        for f64 in (False, True):
            m = 2 * n + f64
            check_bounds_exact(c, r, g, a, f64, KINDS[m % 8], KINDS[(m + 3) % 8], off=m % 2)


@pytest.mark.parametrize("hull", ("interval_fft", "exact"))
@pytest.mark.parametrize("N", (1, 3, 33, 65, 129, 257, 513))
def test_bounds_random_floats_within_the_bound(gpu, N, hull):
    from cp_pre_amd import set_prop as sp
    rng = np.random.default_rng(N)
    g, a = sp.tables(sh.H_of(N, N), hull)
    B = sh.plan(1, N).RB + 1
    worst = 0.0
    for f64 in (False, True):
        dt = np.float64 if f64 else np.float32
        c, r = rng.standard_normal((B, N)).astype(dt), rng.random((B, N)).astype(dt)
        (lo, hi), = bounds(source(c, "comp20", dt), source(r, "transposed", dt), B, N, g, a, f64)
        want_lo, want_hi = sh.bounds_ref(c, r, g, a)
        t = sh.tol(N, sh.bounds_magnitude(c, r, g, a))
        worst = max(worst, sh.within(lo, want_lo, t), sh.within(hi, want_hi, t))
        host_lo, host_hi = sp._bounds_host(c.astype(np.float64), r.astype(np.float64), g, a)
        sh.within(lo, host_lo, t)
        sh.within(hi, host_hi, t)
    print(f"FRACTION setprop_bounds N={N} {hull} {worst:.4f}")


@pytest.mark.parametrize("N", (33, 65, 257))
@pytest.mark.parametrize("f64", (False, True))
def test_bounds_nonfinite_rows_and_their_neighbours(gpu, N, f64):
    """a NaN in c (row 0), an inf in r (row RB - 1) and both (row RB, the first of the next workgroup) in one launch: exactly
    those rows are NaN, every other row is the exact integer result"""
    rng = np.random.default_rng(N)
    RB = sh.plan(1, N).RB
    B = RB + 2
    g, a = sh.int_tables(rng, N)
    c, r = sh.ints(rng, -3, 3, B, N), sh.ints(rng, 0, 3, B, N)
    c[0, N - 1] = np.nan
    r[RB - 1, 0] = np.inf
    c[RB, N // 2], r[RB, N - 1] = -np.inf, np.inf
    lo, hi = check_bounds_exact(c, r, g, a, f64, "pitch3", "comp20")
    nan_rows = np.isnan(lo).all(axis=1)
    assert np.flatnonzero(nan_rows).tolist() == [0, RB - 1, RB] and np.isfinite(lo[~nan_rows]).all()
    assert np.array_equal(np.isnan(hi), np.isnan(lo))


@pytest.mark.parametrize("N", (33, 257))
def test_bounds_centre_that_overflows_in_some_columns(gpu, N):
    from cp_pre_amd import set_prop as sp
    rng = np.random.default_rng(N)
    B = 3
    g = (np.arange(N) % 3 != 0).astype(np.float64)         # 0, 1, 1, 0, 1, 1, ...: g[k] + g[k - 1] is 1 or 2
    a = sh.int_tables(rng, N)[1]
    c, r = sh.ints(rng, -3, 3, B, N), sh.ints(rng, 0, 3, B, N)
    c[1] = 0.0
    c[1, 0] = c[1, 1] = 1e308                               # centre_k = 1e308 (g[k] + g[k - 1])
    (lo, hi), = bounds(source(c, "dense", np.float64), source(r, "negBT", np.float64), B, N, g, a, True)
    host_lo, host_hi = sp._bounds_host(c, r, g, a)
    over = np.isnan(host_lo[1])
    assert over.any() and not over.all() and not np.isnan(host_lo[[0, 2]]).any()
    assert np.array_equal(over, (g + np.roll(g, 1)) == 2)
    sh.same_f64(lo, host_lo)
    sh.same_f64(hi, host_hi)
    want_lo, want_hi = sh.bounds_ref(c, r, g, a)
    sh.same_f64(lo, want_lo)
    sh.same_f64(hi, want_hi)


@pytest.mark.parametrize("c_kind", KINDS + ("zeroB",))
def test_bounds_layouts(gpu, c_kind):
    """(17, 65) and (9, 257): each layout of the centre rows against each of the radius rows, fp32 and fp64"""
    rng = np.random.default_rng(len(c_kind))
    for B, N in ((17, 65), (9, 257)):
        g, a = sh.int_tables(rng, N)
        c, r = sh.ints(rng, -3, 3, B, N), sh.ints(rng, 0, 3, B, N)
        for n, r_kind in enumerate(KINDS + ("zeroB",)):
            check_bounds_exact(c, r, g, a, bool(n % 2), c_kind, r_kind, off=n % 2)


def test_bounds_refusals_and_the_empty_batch(gpu):
    _lib, lib = _L()
    s = source(np.ones((2, 4), np.float32))
    g = np.ones(4)
    bounds(s, s, 0, 4, g, g, False)                        # B = 0: 0, nothing written (the frames are the whole allocation)
    lo = sh.Framed(np.arange(8), torch.float64, 1, DEV)
    t = Table(g)
    rc = lib.pre_setprop_bounds_f64(P(s), _lib.iarr64(s.strides), P(s), _lib.iarr64(s.strides), 2, 0, t.ptr, t.ptr, P(lo), P(lo), 0,
                                    _lib.stream())
    torch.cuda.synchronize()
    assert rc == PRE_E_SHAPE and lo.all_nan_bits()


# ================================================================================================ pre_setprop_recipe_f32
def recipe(fs, B, nt, taps, correlation, q, g, a, off=0, times=1):
    """pre_setprop_recipe_f32 into framed lower / upper [B, Nt + 1]; ``q``: None or (an object with .ptr, strides).  Returns
    the return code and [(lo, hi)] after each call."""
    _lib, lib = _L()
    N = nt + 1
    lo = sh.Framed(np.arange(B * N), torch.float64, off, DEV)
    hi = sh.Framed(np.arange(B * N), torch.float64, 1 - off, DEV)
    tg, ta = Table(g), Table(a)
    tp = (ctypes.c_double * len(taps))(*[float(w) for w in taps])
    out = []
    for _ in range(times):
        rc = lib.pre_setprop_recipe_f32(P(fs), _lib.iarr64(fs.strides), B, nt, tp, len(taps), P(q[0]) if q else None,
                                        _lib.iarr64(q[1]) if q else None, tg.ptr, ta.ptr, P(lo), P(hi),
                                        CORRELATION if correlation else 0, _lib.stream())
        torch.cuda.synchronize()
        assert lo.untouched() and hi.untouched(), (B, nt, rc)
        if rc != 0:
            assert lo.all_nan_bits() and hi.all_nan_bits()
            return rc, out
        out.append((lo.get().reshape(B, N), hi.get().reshape(B, N)))
    return 0, out


def qhat_forms(rng, B, nt, integer=True):
    """q-hat as the header allows it: none, a scalar, a [Nt] row, a strided [B, Nt] (a component view: NaN between its
    elements).  Yields (name, host value broadcastable to [B, Nt], (device operand, strides))."""
    draw = (lambda *s: rng.integers(1, 9, s).astype(np.float32)) if integer else (lambda *s: rng.random(s).astype(np.float32))
    yield "none", None, None
    v = draw(1, 1)
    yield "scalar", v, (source(v), (0, 0))
    v = draw(1, nt)
    yield "row", v, (source(v), (0, 1))
    v = draw(B, nt)
    s = source(v, "comp20")
    yield "strided", v, (s, s.strides)


def symmetric(t):
    k = len(t)
    return np.r_[t[:k // 2 + 1], t[:k // 2][::-1]] if k % 2 else t


def check_recipe_exact(x, taps, correlation, qv, q, g, a, kind="dense", off=0):
    B, nt = x.shape
    fs = source(x, kind)
    sh.assert_exact_f64(sh.recipe_magnitude(x, taps, correlation, qv, g, a), x, taps, g, a, *(() if qv is None else (qv,)))
    rc, ((lo, hi), (lo2, hi2)) = recipe(fs, B, nt, taps, correlation, q, g, a, off, times=2)
    assert rc == 0
    want_lo, want_hi = sh.recipe_ref(x, taps, correlation, qv, g, a)
    sh.same_f64(lo, want_lo)
    sh.same_f64(hi, want_hi)
    assert np.array_equal(lo.view(np.int64), lo2.view(np.int64)) and np.array_equal(hi.view(np.int64), hi2.view(np.int64))
    return lo, hi


@pytest.mark.parametrize("nt", (3, 4, 5) + tuple(N - 1 for N in sh.NS if N >= 31))
def test_recipe_shapes_by_branch(gpu, nt):
    """Nt = 3 (no interior radius), 4 (one), 5, then Nt = N - 1 for every N of the table; k = 1 .. 7 as far as Nt + 2 (every
    tap wraps), correlation on and off, every q-hat form; B on either side of a row group.  Integer taps, fields, q-hat
    and tables: bit for bit."""
    N = nt + 1
    rng = np.random.default_rng(nt)
    g, a = sh.int_tables(rng, N)
    RB = sh.plan(1, N).RB
    ks = [k for k in (1, 3, 5, 7) if k <= nt + 2]
    if nt in (3, 5):
        assert ks[-1] == nt + 2
    m = 0
    for k in ks:
        for correlation in (False, True):
            B = (RB - 1, RB + 1)[m % 2]
            if N in sh.TABLE:
                sh.assert_plan(B, N)
            x = sh.ints(rng, -4, 4, B, nt).astype(np.float32)
            taps = rng.integers(1, 4, k).astype(np.float64) * rng.choice([-1.0, 1.0], k)
            if not correlation:
                taps = symmetric(taps)
            if correlation and k >= 3 and nt >= 4:
                assert sh.steps_outside(nt, k, True)       # the last interior n keep |conv[n]|: q-hat has no such step
            for name, qv, q in qhat_forms(rng, B, nt):
                check_recipe_exact(x, taps, correlation, qv, q, g, a, KINDS[m % 8], off=m % 2)
                m += 1
    # kernels q-hat is not derived for, without it: an asymmetric one without correlation, even ones (k = Nt + 2 at Nt = 4)
    for taps, correlation in (([1.0, -2.0, 3.0], False), ([2.0, 1.0], False), ([1.0, 2.0, -1.0, 3.0], True),
                              ([1.0, 2.0, 3.0, -1.0, 2.0, 1.0], False)):
        if len(taps) <= nt + 2:
            check_recipe_exact(sh.ints(rng, -4, 4, RB + 1, nt).astype(np.float32), np.array(taps), correlation, None, None, g, a,
                               "pitch3")


@pytest.mark.parametrize("nt", (5, 64, 256, 512))
@pytest.mark.parametrize("hull", ("interval_fft", "exact"))
def test_recipe_random_floats_within_the_bound(gpu, nt, hull):
    from cp_pre_amd import set_prop as sp
    rng = np.random.default_rng(nt)
    B = sh.plan(1, nt + 1).RB + 1
    worst = 0.0
    for kernel, correlation in ((SHO_K, False), (K5, True), (K7, False), (K7, True)):
        g, a = sp.tables(sp.recipe_key(kernel, nt, 1e-6, correlation), hull)
        x = rng.standard_normal((B, nt)).astype(np.float32)
        for name, qv, q in qhat_forms(rng, B, nt, integer=False):
            rc, ((lo, hi),) = recipe(source(x, "comp31"), B, nt, kernel, correlation, q, g, a)
            assert rc == 0
            want_lo, want_hi = sh.recipe_ref(x, kernel, correlation, qv, g, a)
            t = sh.tol(nt + 1 + len(kernel), sh.recipe_magnitude(x, kernel, correlation, qv, g, a))
            worst = max(worst, sh.within(lo, want_lo, t), sh.within(hi, want_hi, t))
    print(f"FRACTION setprop_recipe Nt={nt} {hull} {worst:.4f}")


@pytest.mark.parametrize("nt", (31, 100, 300))
@pytest.mark.parametrize("correlation", (False, True))
def test_recipe_nonfinite_field_values(gpu, nt, correlation):
    """a NaN at a field's first step (row RB - 1) and an inf at its last (row RB, the next workgroup): those rows are NaN,
    with and without q-hat - q-hat replaces the radii the value reaches, the row is NaN all the same"""
    rng = np.random.default_rng(nt)
    N = nt + 1
    RB = sh.plan(1, N).RB
    B = RB + 2
    g, a = sh.int_tables(rng, N)
    x = sh.ints(rng, -4, 4, B, nt).astype(np.float32)
    x[RB - 1, 0] = np.nan
    x[RB, nt - 1] = np.inf
    taps = np.array([1.0, -2.0, 1.0])
    for name, qv, q in qhat_forms(rng, B, nt):
        lo, hi = check_recipe_exact(x, taps, correlation, qv, q, g, a, "pitch3")
        nan_rows = np.isnan(lo).all(axis=1)
        assert np.flatnonzero(nan_rows).tolist() == [RB - 1, RB] and np.isfinite(lo[~nan_rows]).all(), name
        assert np.array_equal(np.isnan(hi), np.isnan(lo))


def test_recipe_refusals_leave_the_outputs_untouched(gpu):
    rng = np.random.default_rng(1)
    ones = np.ones(8)
    q_of = {nt: (source(np.ones((1, nt), np.float32)), (0, 1)) for nt in (2, 3, 4, 7)}

    def call(nt, taps, correlation, with_q):
        x = sh.ints(rng, -4, 4, 2, nt).astype(np.float32)
        return recipe(source(x), 2, nt, np.array(taps, np.float64), correlation, q_of[nt] if with_q else None, ones[:nt + 1],
                      ones[:nt + 1])[0]

    assert call(3, [1.0] * 6, False, False) == PRE_E_UNSUPPORTED            # k = Nt + 3
    assert call(4, [1.0] * 7, True, False) == PRE_E_UNSUPPORTED             # k = Nt + 3
    assert call(3, [1.0] * 7, False, False) == PRE_E_UNSUPPORTED
    assert call(2, [1.0], False, False) == PRE_E_SHAPE                      # Nt < 3
    assert call(7, [1.0, -2.0, 0.5], False, True) == PRE_E_UNSUPPORTED      # asymmetric, no correlation, q-hat
    assert call(7, [1.0, 2.0, 2.0, 1.0], False, True) == PRE_E_UNSUPPORTED  # even, q-hat
    assert call(7, [1.0, 2.0], True, True) == PRE_E_UNSUPPORTED
    assert call(7, [1.0, -2.0, 0.5], True, True) == 0                       # the same kernels where they are served
    assert call(7, [1.0, -2.0, 0.5], False, False) == 0
    assert call(7, [1.0, 2.0, 2.0, 1.0], False, False) == 0
    assert call(4, [1.0] * 6, False, False) == 0                            # k = Nt + 2
    assert call(3, [1.0] * 5, True, True) == 0


# ================================================================================================ through the package
def test_propagate_on_operands_whose_layouts_and_types_disagree(gpu):
    from cp_pre_amd import set_prop as sp
    for B, N in ((17, 65), (9, 257), (33, 64)):
        rng = np.random.default_rng(N)
        c = rng.standard_normal((B, N)).astype(np.float32)
        r = rng.random((B, N))
        cs, rs = source(c, "comp31", np.float32), source(r, "transposed", np.float64)
        cv = cs.dev.as_strided((B, N), cs.strides, cs.origin)
        rv = rs.dev.as_strided((B, N), rs.strides, rs.origin)
        H = sh.H_of(N, N + 1)
        for hull in sp.HULLS:
            lo, hi = sp.propagate(cv, rv, H, hull=hull)
            g, a = sp.tables(H, hull)
            want_lo, want_hi = sh.bounds_ref(c, r, g, a)
            t = sh.tol(N, sh.bounds_magnitude(c, r, g, a))
            sh.within(lo.cpu().numpy(), want_lo, t)
            sh.within(hi.cpu().numpy(), want_hi, t)


def test_set_pre_bounds_on_a_component_view_with_strided_qhat(gpu):
    from cp_pre_amd import set_prop as sp
    for B, nt, kernel, correlation in ((17, 127, K5, False), (9, 256, K7, True), (33, 5, K7, False)):
        rng = np.random.default_rng(nt)
        x = rng.standard_normal((B, nt)).astype(np.float32)
        qv = rng.random((B, nt)).astype(np.float32)
        xs, qs = source(x, "comp20"), source(qv, "transposed")
        xv = xs.dev.as_strided((B, nt), xs.strides, xs.origin)
        qt = qs.dev.as_strided((B, nt), qs.strides, qs.origin)
        for radius, qhost in ((None, None), (qt, qv), (qt[0], qv[:1])):
            lo, hi = sp.set_pre_bounds(xv, kernel, correlation=correlation, radius=radius)
            g, a = sp.tables(sp.recipe_key(kernel, nt, 1e-6, correlation))
            want_lo, want_hi = sh.recipe_ref(x, kernel, correlation, qhost, g, a)
            t = sh.tol(nt + 1 + len(kernel), sh.recipe_magnitude(x, kernel, correlation, qhost, g, a))
            sh.within(lo.cpu().numpy(), want_lo, t)
            sh.within(hi.cpu().numpy(), want_hi, t)
