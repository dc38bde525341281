"""GPU tests (pytest -m gpu) of the ODE kernels of cp_pre_amd/csrc/ode_march.hip at their seams: ``ode_residual_kernel<K>`` and
the two wgrad kernels called through the C ABI (``_lib.load_ode().pre_ode_*``) at shapes picked by the branch they reach -
runs of 4 outputs that cross a row at every v, rows shorter than the window, the block edge at 1024 outputs, mixed tap
widths under non-finite data, shared and unshared sources, per-step coefficients, every layout the header allows, the block
ranges of the kernel gradient - and, last, through ``convops_0d.stencil`` and ``ode.ODEResidual.residual(out=...)``.
Small-integer data are compared bit for bit with integer numpy, random floats element by element against float64 within
the derived bounds of tests/ode_helpers.py (checked on the CPU by tests/test_ode_ref_cpu.py).  Every output lies inside a
larger allocation of the test's filled with NaN, which must be unchanged around it after each call; strided inputs carry NaN
wherever no element lies.  tests/ODE_TESTS.md says which branch each shape reaches."""
import ctypes

import numpy as np
import pytest
import torch

import ode_helpers as oh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PRE_E_SHAPE, PRE_E_UNSUPPORTED = -2, -3
ABS = 1
KS = (1, 3, 5, 7)
IN_KINDS = ("dense", "comp31", "transposed", "negB", "negT", "negBT", "zeroB", "pitch3")
OUT_KINDS = ("dense", "padded", "transposed", "negB", "negT", "negBT")


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    from cp_pre_amd import _lib
    _lib.load_ode()
    return torch.device(DEV)


def _L():
    from cp_pre_amd import _lib
    return _lib, _lib.load_ode()


def source(data, kind="dense"):
    return oh.Source(data, kind, device=DEV, lead=int(kind[5]) if kind.startswith("comp") else 0)


class Alias:
    """a [BS, Nt] view at ``offset`` elements into a device tensor another view also reads"""

    def __init__(self, dev, offset, strides, data):
        self.dev, self.ptr, self.strides, self.data = dev, dev.data_ptr() + 4 * offset, strides, np.asarray(data, np.float32)


def host_terms(terms):
    return [(s.data, taps, c) for s, taps, c in terms]


def launch_residual(terms, bs, nt, out, strides, flags=0):
    """pre_ode_residual_f32 on ``terms`` = [(source, taps, c or None)] into the framed ``out``; returns the return code"""
    _lib, lib = _L()
    arr = (_lib.PreOdeTerm * max(1, len(terms)))()
    keep = []
    for i, (s, taps, c) in enumerate(terms[:len(arr)]):
        arr[i].x, arr[i].sB, arr[i].sT = s.ptr, s.strides[0], s.strides[1]
        arr[i].k = len(taps)
        for j, w in enumerate(taps[:oh.MAX_TAPS]):
            arr[i].taps[j] = float(w)
        if c is not None:
            assert len(c) == nt
            keep.append(torch.from_numpy(np.asarray(c, np.float32)).to(DEV))
            arr[i].c = keep[-1].data_ptr()
    rc = lib.pre_ode_residual_f32(arr, len(terms), ctypes.c_void_p(out.ptr), _lib.iarr64(strides), bs, nt, flags, _lib.stream())
    torch.cuda.synchronize()
    return rc


def residual(terms, bs, nt, flags=0, out_kind="dense", off=0):
    """the residual of ``terms`` into a framed output laid out as ``out_kind``, ``off`` elements past a 256-byte boundary;
    the frame must hold what it held.  Returns the [BS, Nt] result."""
    strides = oh.layout(out_kind, bs, nt)
    out = oh.Framed(oh.offsets(bs, nt, *strides), offset=off, device=DEV)
    assert launch_residual(terms, bs, nt, out, strides, flags) == 0
    assert out.untouched(), (bs, nt, out_kind, off)
    return out.get().reshape(bs, nt)


def stencil(src, taps, bs, nt, flags=0, out_kind="dense", off=0):
    _lib, lib = _L()
    strides = oh.layout(out_kind, bs, nt)
    out = oh.Framed(oh.offsets(bs, nt, *strides), offset=off, device=DEV)
    t = np.ascontiguousarray(taps, np.float32)
    rc = lib.pre_ode_stencil_f32(ctypes.c_void_p(src.ptr), _lib.iarr64(src.strides), ctypes.c_void_p(out.ptr), _lib.iarr64(strides),
                                 bs, nt, t.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(t), flags, _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and out.untouched(), (bs, nt, out_kind, off)
    return out.get().reshape(bs, nt)


def check_exact(terms, bs, nt, **kw):
    oh.assert_exact_f32(host_terms(terms))
    got = residual(terms, bs, nt, **kw)
    oh.same_f32(got, oh.residual_ref(host_terms(terms), np.int64))
    return got


# ================================================================================================ ode_residual_kernel<K>
@pytest.mark.parametrize("bs,nt", sorted(oh.TABLE))
def test_residual_shapes_by_branch(gpu, bs, nt):
    """every row of the table at K = 1, 3, 5, 7: a K-wide term with a coefficient that differs at every t, a K-wide term on a
    second view with NaN between its rows, and (K > 1) a narrower term that shares the first view's window; integer data,
    compared bit for bit.  The stencil entry runs the same shape alone."""
    oh.assert_plan(bs, nt)
    rng = np.random.default_rng(bs * 4099 + nt)
    for n, K in enumerate(KS):
        a = source(oh.ints(rng, -8, 8, bs, nt), IN_KINDS[(bs + nt + n) % 6])
        b = source(oh.ints(rng, -8, 8, bs, nt), "pitch3")
        terms = [(a, oh.int_taps(rng, K), oh.coeff_row(nt)), (b, oh.int_taps(rng, K), None)]
        if K > 1:
            terms.append((a, oh.int_taps(rng, K - 2), oh.coeff_row(nt, 3)))
        check_exact(terms, bs, nt, out_kind=OUT_KINDS[(bs + n) % len(OUT_KINDS)], off=n % 2)
        taps = oh.int_taps(rng, K)
        oh.same_f32(stencil(b, taps, bs, nt, out_kind=OUT_KINDS[(nt + n) % len(OUT_KINDS)], off=(n + 1) % 2),
                    oh.conv_ref(b.data, taps, np.int64))


@pytest.mark.parametrize("bs,nt", [(5, 7), (341, 3), (2, 1023), (1025, 1), (147, 7)])
def test_residual_random_floats_within_the_derived_bound(gpu, bs, nt):
    """six terms of mixed widths and coefficients on random floats: |got - ref| <= (k_max + nterms + 2) 2^-24 S[b, t]"""
    rng = np.random.default_rng(bs + nt)
    worst = 0.0
    for K in KS:
        srcs = [source(rng.standard_normal((bs, nt)).astype(np.float32), kind) for kind in ("dense", "comp20", "pitch3")]
        terms = []
        for i in range(6):
            k = K if i == 0 else int(rng.choice([w for w in KS if w <= K]))
            c = rng.standard_normal(nt).astype(np.float32) if i % 2 == 0 else None
            terms.append((srcs[i % 3], rng.standard_normal(k).astype(np.float32), c))
        got = residual(terms, bs, nt, off=1)
        worst = max(worst, oh.within(got, oh.residual_ref(host_terms(terms)), oh.residual_tol(host_terms(terms))))
    print(f"FRACTION ode_residual ({bs},{nt}) {worst:.3f}")


def _planted(rng, bs, nt):
    """four fields of integers with NaN / +inf / -inf at a row start, a row end and mid-row, a field per tap width"""
    x = {k: oh.ints(rng, -8, 8, bs, nt) for k in KS}
    mid = nt // 2
    x[3][0, 0], x[3][1, nt - 1], x[3][2, mid] = np.nan, np.inf, -np.inf
    x[5][3, 0], x[5][4, nt - 1], x[5][5, mid] = np.nan, np.inf, -np.inf
    x[1][6, 0], x[1][6, nt - 1] = np.nan, -np.inf
    x[7][0, nt - 1], x[7][6, mid] = np.nan, np.inf
    return x


TAPS_WITH_ZEROS = {1: [2.0], 3: [0.0, 2.0, -1.0], 5: [1.0, 0.0, -2.0, 0.0, 3.0], 7: [-1.0, 0.0, 0.0, 2.0, 0.0, 1.0, 0.0]}


@pytest.mark.parametrize("nt", (2, 3, 9, 13))
def test_mixed_widths_nonfinite_footprint(gpu, nt):
    """one residual with terms of k = 1, 3, 5, 7, each on a view of its own: a NaN or inf reaches exactly the outputs whose
    TERM window covers it - not the K = 7 window the kernel slides - zero taps included (0 * NaN spreads)"""
    bs = 7
    rng = np.random.default_rng(nt)
    x = _planted(rng, bs, nt)
    kinds = {1: "dense", 3: "pitch3", 5: "comp20", 7: "negT"}
    for order in (KS, KS[::-1]):                           # the widest term first or last: K is found either way
        terms = [(source(x[k], kinds[k]), np.array(TAPS_WITH_ZEROS[k], np.float32), oh.coeff_row(nt) if k in (5, 7) else None)
                 for k in order]
        oh.assert_exact_f32(host_terms(terms))
        ref = oh.residual_ref(host_terms(terms))
        got = residual(terms, bs, nt, off=1)
        assert np.array_equal(oh.footprint(got), oh.footprint(ref))
        oh.same_f32(got, ref)
    if nt == 13:                                           # the k = 3 term, taps (0, 2, -1), -inf at t = 6 of row 2
        assert oh.footprint(ref[2]).tolist() == [0] * 5 + [2, 3, 1] + [0] * 5
        assert oh.footprint(ref[1]).tolist() == [0] * 11 + [3, 2]             # +inf at the row end: t = 11 (-1 tap), 12
        assert oh.footprint(ref[3]).tolist() == [1, 1, 1] + [0] * 10          # the k = 5 term's NaN at the row start


@pytest.mark.parametrize("nt", (3, 9, 13))
def test_mixed_widths_on_one_view(gpu, nt):
    """the same widths on ONE view (one shared window), one non-finite value at a time: the footprint is the union of the
    terms' own, and each narrow term's taps sit at their slots of the shared window"""
    bs = 5
    rng = np.random.default_rng(nt)
    base = oh.ints(rng, -8, 8, bs, nt)
    for k_wide in (3, 5, 7):
        for (b, t, v) in ((0, 0, np.nan), (1, nt - 1, np.inf), (2, nt // 2, -np.inf), (4, nt - 1, np.nan)):
            x = base.copy()
            x[b, t] = v
            s = source(x, "pitch3")
            terms = [(s, np.array(TAPS_WITH_ZEROS[k], np.float32), oh.coeff_row(nt, k) if k == 3 else None)
                     for k in KS if k <= k_wide]
            ref = oh.residual_ref(host_terms(terms))
            got = residual(terms, bs, nt)
            assert np.array_equal(oh.footprint(got), oh.footprint(ref)), (k_wide, b, t)
            oh.same_f32(got, ref)
            hit = np.flatnonzero(oh.footprint(ref[b]))
            assert hit.min() == max(0, t - k_wide // 2) and hit.max() == min(nt - 1, t + k_wide // 2)
            assert not oh.footprint(np.delete(ref, b, 0)).any()


@pytest.mark.parametrize("variant", ("one_view", "six_views", "same_pointer_two_strides", "state2", "state3"))
@pytest.mark.parametrize("bs,nt", [(37, 29), (5, 7)])
def test_sources(gpu, variant, bs, nt):
    rng = np.random.default_rng(bs + len(variant))
    widths = (7, 1, 5, 3, 3, 7)
    coef = [oh.coeff_row(nt, i) if i % 2 else None for i in range(6)]
    if variant == "one_view":
        s = source(oh.ints(rng, -8, 8, bs, nt), "pitch3")
        srcs = [s] * 6
    elif variant == "six_views":
        srcs = [source(oh.ints(rng, -8, 8, bs, nt), IN_KINDS[i]) for i in range(6)]
    elif variant == "same_pointer_two_strides":            # [BS, Nt] and the [Nt, BS] reading of the same words: two sources
        data = oh.ints(rng, -8, 8, bs, nt)
        s = source(data, "dense")
        t = Alias(s.dev, 0, (1, bs), data.reshape(-1)[np.arange(bs)[:, None] + np.arange(nt)[None, :] * bs])
        srcs = [s, t, s, t, t, s]
    else:
        S = int(variant[-1])
        st = oh.ints(rng, -8, 8, bs, nt, S)
        dev = torch.from_numpy(st).to(DEV)
        comps = [Alias(dev, c, (nt * S, S), st[..., c]) for c in range(S)]
        srcs = [comps[i % S] for i in range(6)]
    terms = [(srcs[i], oh.int_taps(rng, widths[i]), coef[i]) for i in range(6)]
    check_exact(terms, bs, nt, off=1)
    check_exact(terms[:2], bs, nt, out_kind="padded")


def test_coefficient_is_indexed_by_the_outputs_step(gpu):
    """c[t] differs at every t and the taps are (0, 1, 0): out[b, t] = c[t] x[b, t], at shapes that cross a row at every v"""
    for bs, nt in ((5, 7), (205, 5), (171, 6), (341, 3), (2, 1023)):
        x = np.ones((bs, nt), np.float32)
        c = oh.coeff_row(nt)
        got = residual([(source(x), [0.0, 1.0, 0.0], c), (source(x, "pitch3"), [1.0], None)], bs, nt)
        oh.same_f32(got, np.repeat(c[None] + 1.0, bs, 0))


@pytest.mark.parametrize("bs,nt", [(5, 7), (341, 3), (1, 1025)])
def test_absolute_flag(gpu, bs, nt):
    """|out| is the unflagged result with the sign bit cleared, bit for bit: a negative zero comes back +0.0, NaN stays NaN"""
    rng = np.random.default_rng(nt)
    x = rng.standard_normal((bs, nt)).astype(np.float32)
    x[0, 0] = np.nan
    x[:, nt // 2] = 0.0
    y = oh.ints(rng, -1, 1, bs, nt)                        # many exact zeros and cancellations
    terms = [(source(x, "comp20"), np.array([0.5, -1.0, 0.25], np.float32), oh.coeff_row(nt)),
             (source(y, "pitch3"), np.array([-1.0, 0.0, -1.0, 0.0, -1.0], np.float32), None)]
    plain = residual(terms, bs, nt, out_kind="padded")
    flagged = residual(terms, bs, nt, flags=ABS, out_kind="padded", off=1)
    nan = np.isnan(plain)
    assert nan.any() and (plain < 0).any()
    assert np.array_equal(np.isnan(flagged), nan)
    assert np.array_equal(flagged.view(np.int32)[~nan], plain.view(np.int32)[~nan] & 0x7FFFFFFF)
    ints_only = [(source(y), np.array([-1.0], np.float32), None)]
    flagged = residual(ints_only, bs, nt, flags=ABS)
    assert not (flagged.view(np.int32) < 0).any() and np.array_equal(flagged, np.abs(y))
    oh.same_f32(stencil(source(y), [-1.0], bs, nt, flags=ABS), np.abs(y))


@pytest.mark.parametrize("in_kind", IN_KINDS)
def test_layouts(gpu, in_kind):
    """every input layout against every output layout, (37, 29): 1073 outputs, two blocks, rows that cross at every v"""
    bs, nt = 37, 29
    rng = np.random.default_rng(len(in_kind))
    terms = [(source(oh.ints(rng, -8, 8, bs, nt), in_kind), oh.int_taps(rng, 5), None),
             (source(oh.ints(rng, -8, 8, bs, nt), "pitch3"), oh.int_taps(rng, 3), oh.coeff_row(nt))]
    for n, out_kind in enumerate(OUT_KINDS):
        check_exact(terms, bs, nt, out_kind=out_kind, off=n % 2)
    oh.same_f32(stencil(terms[0][0], terms[0][1], bs, nt, out_kind="padded", off=1), oh.conv_ref(terms[0][0].data, terms[0][1]))


def test_refusals_and_empty_fields_leave_the_output_untouched(gpu):
    _lib, lib = _L()
    bs, nt = 4, 16
    rng = np.random.default_rng(0)
    s = source(oh.ints(rng, -8, 8, bs, nt))
    good = (s, oh.int_taps(rng, 3), None)
    dense = oh.layout("dense", bs, nt)

    def fresh():
        return oh.Framed(np.arange(bs * nt), device=DEV)

    for strides in ((0, 1), (8, 1), (16, 0), (1, 2)):      # a broadcast row, interleaved rows, a broadcast step, interleaved steps
        out = fresh()
        assert launch_residual([good], bs, nt, out, strides) == PRE_E_SHAPE and out.all_nan_bits(), strides
    for k in (2, 4, 6, 9):
        out = fresh()
        assert launch_residual([(s, np.ones(k, np.float32), None)], bs, nt, out, dense) == PRE_E_UNSUPPORTED and out.all_nan_bits()
        t = np.ones(k, np.float32)
        rc = lib.pre_ode_stencil_f32(ctypes.c_void_p(s.ptr), _lib.iarr64(s.strides), ctypes.c_void_p(out.ptr), _lib.iarr64(dense), bs,
                                     nt, t.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), k, 0, _lib.stream())
        torch.cuda.synchronize()
        assert rc == PRE_E_UNSUPPORTED and out.all_nan_bits(), k
    out = fresh()
    arr = (_lib.PreOdeTerm * 7)()
    for i in range(7):
        arr[i].x, arr[i].sB, arr[i].sT, arr[i].k = s.ptr, nt, 1, 1
        arr[i].taps[0] = 1.0
    rc = lib.pre_ode_residual_f32(arr, 7, ctypes.c_void_p(out.ptr), _lib.iarr64(dense), bs, nt, 0, _lib.stream())
    torch.cuda.synchronize()
    assert rc == PRE_E_UNSUPPORTED and out.all_nan_bits()
    for b, t in ((0, nt), (bs, 0), (0, 0)):
        out = fresh()
        assert launch_residual([good], b, t, out, dense) == 0 and out.all_nan_bits(), (b, t)
    out = fresh()                                          # the same call with nothing wrong
    assert launch_residual([good], bs, nt, out, dense) == 0 and out.untouched()
    oh.same_f32(out.get().reshape(bs, nt), oh.conv_ref(s.data, good[1], np.int64))


# ================================================================================================ pre_ode_wgrad_f32
def wgrad(xs, gs, bs, nt, k, off=0, times=1):
    """pre_ode_wgrad_f32 with ``work`` framed at exactly PRE_ODE_WGRAD_BLOCKS * k doubles and filled with NaN (no stale
    partial may survive into dK), ``dk`` framed; ``times`` calls.  Returns dK after each call."""
    _lib, lib = _L()
    work = oh.Framed(np.arange(oh.WGRAD_BLOCKS * k), torch.float64, 0, DEV)
    dk = oh.Framed(np.arange(k), torch.float32, off, DEV)
    out = []
    for _ in range(times):
        rc = lib.pre_ode_wgrad_f32(ctypes.c_void_p(xs.ptr), _lib.iarr64(xs.strides), ctypes.c_void_p(gs.ptr), _lib.iarr64(gs.strides),
                                   bs, nt, k, ctypes.c_void_p(work.ptr), ctypes.c_void_p(dk.ptr), _lib.stream())
        torch.cuda.synchronize()
        assert rc == 0 and work.untouched() and dk.untouched(), (bs, nt, k)
        out.append(dk.get())
    return out, work.get()


WG_KINDS = ("dense", "comp20", "negBT", "negB", "comp31", "negT")


@pytest.mark.parametrize("bs,nt", sorted(oh.WGRAD_TABLE))
def test_wgrad_block_ranges_exact(gpu, bs, nt):
    """integer x and g (|.| <= 4): dK is the exact integer at every table row, k = 1, 3, 5, 7, twice with the same bits"""
    p = oh.assert_wgrad_plan(bs, nt)
    rng = np.random.default_rng(bs + nt)
    x, g = oh.ints(rng, -4, 4, bs, nt), oh.ints(rng, -4, 4, bs, nt)
    for n, k in enumerate(KS):
        oh.assert_exact_wgrad(x, g, k)
        xs, gs = source(x, WG_KINDS[(n + bs) % 6]), source(g, WG_KINDS[(n + nt + 3) % 6])
        (a, b), work = wgrad(xs, gs, bs, nt, k, off=n % 2, times=2)
        want = oh.wgrad_ref(x, g, k, np.int64)
        assert np.array_equal(a.astype(np.int64), want), (k, a.tolist(), want.tolist())
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
        work = work.reshape(oh.WGRAD_BLOCKS, k)
        assert np.all(work[p.nonempty:] == 0) and np.array_equal(work.sum(0), want)      # empty blocks write zeros


@pytest.mark.parametrize("bs,nt", [(1, 1), (147, 7), (2, 1023), (2405, 109)])
def test_wgrad_random_floats_within_the_derived_bound(gpu, bs, nt):
    rng = np.random.default_rng(bs)
    x, g = rng.standard_normal((bs, nt)).astype(np.float32), rng.standard_normal((bs, nt)).astype(np.float32)
    worst = 0.0
    for n, k in enumerate(KS):
        (a, b), _ = wgrad(source(x, WG_KINDS[n]), source(g, WG_KINDS[n + 2]), bs, nt, k, off=1, times=2)
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
        worst = max(worst, oh.within(a, oh.wgrad_ref(x, g, k), oh.wgrad_tol(x, g, k)))
    print(f"FRACTION ode_wgrad ({bs},{nt}) {worst:.3f}")


def test_wgrad_of_an_empty_field_is_zero(gpu):
    s = source(np.ones((1, 4), np.float32))
    for bs, nt in ((0, 4), (3, 0), (0, 0)):
        for k in KS:
            (a,), work = wgrad(s, s, bs, nt, k)
            assert np.array_equal(a.view(np.int32), np.zeros(k, np.int32)) and np.all(work == 0)


# ================================================================================================ through the package
def _torch_view(kind, bs, nt, off):
    strides = oh.layout(kind, bs, nt)
    f = oh.Framed(oh.offsets(bs, nt, *strides), offset=off, device=DEV)
    return f, f.alloc.as_strided((bs, nt), strides, f.origin)


def test_stencil_on_operands_whose_layouts_disagree(gpu):
    from cp_pre_amd.convops_0d import stencil as pkg_stencil
    bs, nt = 37, 29
    rng = np.random.default_rng(8)
    for n, (in_kind, out_kind) in enumerate((("transposed", "padded"), ("comp31", "transposed"), ("pitch3", "dense"),
                                             ("dense", "transposed"))):
        s = source(oh.ints(rng, -8, 8, bs, nt), in_kind)
        field = s.dev.as_strided((bs, nt), s.strides, s.origin)
        taps = oh.int_taps(rng, KS[n])
        f, out = _torch_view(out_kind, bs, nt, n % 2)
        got = pkg_stencil(field, taps, out=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and f.untouched()
        oh.same_f32(f.get().reshape(bs, nt), oh.conv_ref(s.data, taps, np.int64))


def test_residual_out_on_operands_whose_layouts_disagree(gpu):
    from cp_pre_amd import ode
    bs, nt = 37, 29
    rng = np.random.default_rng(9)
    st = oh.ints(rng, -8, 8, bs, nt, 3)
    state = torch.from_numpy(st).to(DEV)
    fields = [source(st[..., c], kind) for c, kind in enumerate(("transposed", "pitch3", "dense"))]
    views = [s.dev.as_strided((bs, nt), s.strides, s.origin) for s in fields]
    spec = [(0, oh.int_taps(rng, 7), oh.coeff_row(nt)), (1, oh.int_taps(rng, 1), None), (2, oh.int_taps(rng, 5), oh.coeff_row(nt, 2)),
            (0, oh.int_taps(rng, 3), None)]
    op = ode.ODEResidual(spec)
    host = [(st[..., c], taps, cf) for c, taps, cf in spec]
    oh.assert_exact_f32(host)
    want = oh.residual_ref(host, np.int64)
    for n, out_kind in enumerate(("transposed", "padded")):
        for operand in (state, views):
            f, out = _torch_view(out_kind, bs, nt, n)
            op.residual(operand, out=out)
            torch.cuda.synchronize()
            assert f.untouched()
            oh.same_f32(f.get().reshape(bs, nt), want)
        f, out = _torch_view(out_kind, bs, nt, 1 - n)
        op.residual(views, absolute=True, out=out)
        torch.cuda.synchronize()
        assert f.untouched()
        oh.same_f32(f.get().reshape(bs, nt), np.abs(want))
