"""GPU tests (pytest -m gpu) of the joint-CP calibration kernels of cp_pre_amd/csrc/calib.hip at their seams, called through
the C ABI on operands the pipeline never builds - bases 4 bytes off a 16-byte boundary, sizes on both sides of every
quad, block, launch and slice limit, tied and special values - against the plain numpy references of
tests/calib_helpers.py (checked on the CPU by tests/test_calib_ref_cpu.py).  Every output lies inside a larger allocation
of the test's filled with NaN or a bit pattern, which must be unchanged after each call; results are compared bit for
bit unless a test says otherwise.  tests/CALIB_TESTS.md says which branch each shape reaches."""
import ctypes

import numpy as np
import pytest
import torch

import calib_helpers as ch
from oracle import conformal as oc

pytestmark = pytest.mark.gpu

NAN, INF = np.float32(np.nan), np.float32(np.inf)
PRE_E_NULL, PRE_E_RANGE = -1, -4


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    from cp_pre_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _L():
    from cp_pre_amd import _lib
    return _lib, _lib.load()


def E(x, off=0, gpu="cuda:0", fill=None):
    """numpy array (or tensor) -> Embedded on the GPU, ``off`` elements past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return ch.embed(t, off, 64, fill, device=gpu)


def P(e):
    # (from the allocation: torch gives an EMPTY view a null data_ptr, and n == 0 is a case here)
    return ctypes.c_void_p(e.alloc.data_ptr() + e.lo * e.alloc.element_size()) if e is not None else ctypes.c_void_p(0)


def host(e):
    torch.cuda.synchronize()
    return e.view.cpu().numpy()


def same_bits(got, ref):
    got, ref = ch.bits32(got), ch.bits32(ref)
    bad = np.flatnonzero(got.reshape(-1) != ref.reshape(-1))
    assert bad.size == 0, (bad[:8].tolist(), got.reshape(-1)[bad[:8]].view(np.float32).tolist(),
                           ref.reshape(-1)[bad[:8]].view(np.float32).tolist())


# ================================================================================================ pre_kth_f32
def _kth(s_e, N, ks):
    _lib, lib = _L()
    out = E(np.full(len(ks), 123.0, np.float32))
    rc = lib.pre_kth_f32(P(s_e), N, _lib.iarr64(ks), len(ks), P(out), _lib.stream())
    got = host(out)
    assert out.untouched() and s_e.untouched()
    return rc, got


def _ranks(N):
    ks = {0, 1, N // 2, N - 2, N - 1}
    for a in oc.ALPHA_LEVELS:
        try:
            ks.add(oc.kth_index(N, a))
        except ValueError:
            pass
    return sorted(k for k in ks if 0 <= k < N)


KTH_N = [1, 2, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 65537]


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off4"])
@pytest.mark.parametrize("N", KTH_N)
def test_kth_sizes_and_bases(gpu, N, off):
    """float4 loop over N/8*8 elements on an aligned base, the scalar tail, the all-scalar form on a base 4 bytes off; the
    guard around the scores is NaN: an element read beyond N would make every answer NaN."""
    s = np.random.default_rng(N).standard_normal(N).astype(np.float32)
    ks = _ranks(N)
    rc, got = _kth(E(s, off), N, ks)
    assert rc == 0
    same_bits(got, ch.kth_ref(s, ks))


@pytest.mark.parametrize("nk", [1, 16, 17, 33])
def test_kth_rank_lists_cross_the_launch_of_16(gpu, nk):
    """unsorted ranks with duplicates, straight to the C entry point, 16 per launch"""
    N = 1025
    rng = np.random.default_rng(nk)
    s = rng.standard_normal(N).astype(np.float32)
    ks = rng.integers(0, N, nk).tolist()
    if nk > 2:
        ks[-1], ks[nk // 2] = ks[0], N - 1
    assert nk < 3 or (ks != sorted(ks) and len(set(ks)) < nk)
    for off in (0, 1):
        rc, got = _kth(E(s, off), N, ks)
        assert rc == 0
        same_bits(got, ch.kth_ref(s, ks))


def _families(N, rng):
    i = np.arange(N)
    r = rng.standard_normal(N)
    mixed = r.copy()
    mixed[::3], mixed[1::3] = -0.0, 0.0
    infs = r.copy()
    infs[[0, N // 2]], infs[[1, N - 1]] = np.inf, -np.inf
    return {"all_equal": np.full(N, 2.5), "two_values": np.where(rng.random(N) < 0.3, -1.5, 4.0),
            "shared_three_bytes": 1.0 + (i % 256) * 2.0 ** -23, "mixed_sign_zeros": mixed, "infs": infs,
            "subnormals": (rng.integers(-2000, 2000, N) * 2.0 ** -149), "quantised": np.round(r * 8) / 8, "randn": r}


@pytest.mark.parametrize("family", ["all_equal", "two_values", "shared_three_bytes", "mixed_sign_zeros", "infs", "subnormals",
                                    "quantised", "randn"])
def test_kth_data_families(gpu, family):
    """tied data (one lane adds the whole wave's count in every pass), spread data (never), and the orders in between"""
    for N in (65, 1025, 8193):
        s = _families(N, np.random.default_rng(N + 1))[family].astype(np.float32)
        ks = _ranks(N)
        for off in (0, 1):
            rc, got = _kth(E(s, off), N, ks)
            assert rc == 0
            same_bits(got, ch.kth_ref(s, ks))


def test_kth_nan_of_either_sign_in_loop_and_tail_but_not_beyond(gpu):
    N = 1027                                                       # N % 8 == 3: the scalar tail reads the last three
    s = np.random.default_rng(0).standard_normal(N).astype(np.float32)
    ks = _ranks(N)
    for off in (0, 1):
        rc, got = _kth(E(s, off), N, ks)                           # NaN in the guard only: not seen
        assert rc == 0 and not np.isnan(got).any()
        for pos in (5, N - 1, N - 3):
            for nanbits in (0x7FC00000, 0xFFC00000):
                t = s.copy()
                t.view(np.uint32)[pos] = nanbits
                rc, got = _kth(E(t, off), N, ks)
                assert rc == 0 and np.isnan(got).all(), (off, pos, hex(nanbits))
                same_bits(got, ch.kth_ref(t, ks))


def test_kth_error_returns(gpu):
    s = np.arange(16, dtype=np.float32)
    for ks, N, want in (([-1], 16, PRE_E_RANGE), ([16], 16, PRE_E_RANGE), ([3, 16], 16, PRE_E_RANGE), ([0], 0, PRE_E_NULL)):
        rc, got = _kth(E(s), N, ks)
        assert rc == want and (got == 123.0).all()


# ================================================================================================ pre_absdiff_f32
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 4095, 4096, 4097, 4 * 1024 * 3 + 1])
def test_absdiff_sizes_bases_and_special_values(gpu, n):
    _lib, lib = _L()
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    sp_a = np.array([-0.0, 0.0, INF, -INF, NAN, 1.0, INF, -1.5, NAN], np.float32)
    sp_b = np.array([0.0, -0.0, 1.0, 1.0, 1.0, NAN, INF, 2.0, -INF], np.float32)
    sp_a.view(np.uint32)[8] = 0xFFC00000                          # a NaN with the sign bit set
    k = min(n, 9)
    a[n - k:], b[n - k:] = sp_a[:k], sp_b[:k]                      # (at the end: the scalar tail sees some of them)
    a[:k // 2], b[:k // 2] = sp_a[:k // 2], sp_b[:k // 2]
    for with_b in (False, True):
        for mis in (None, "a", "b", "out"):
            if mis == "b" and not with_b:
                continue
            ea, eb = E(a, mis == "a"), (E(b, mis == "b") if with_b else None)
            out = E(np.full(n, -7.0, np.float32), mis == "out")
            rc = lib.pre_absdiff_f32(P(ea), P(eb), P(out), n, _lib.stream())
            got = host(out)
            assert rc == 0 and out.untouched() and ea.untouched() and (eb is None or eb.untouched())
            same_bits(got, ch.absdiff_ref(a, b if with_b else None))
            assert (got.view(np.uint32) >> 31 == 0).all(), "an output with its sign bit set"


# ================================================================================================ pre_std_axis0_f32
def _std(a, b, eps, off=0):
    _lib, lib = _L()
    n, M = a.shape
    ea, eb = E(a, off), (E(b, off) if b is not None else None)
    out = E(np.full(M, -7.0, np.float32), off)
    rc = lib.pre_std_axis0_f32(P(ea), P(eb), n, M, eps, P(out), _lib.stream())
    got = host(out)
    assert rc == 0 and out.untouched()
    return got


@pytest.mark.parametrize("n,M", [(17, 1), (17, 63), (17, 64), (17, 65), (17, 257), (3, 2 ** 19 - 1), (3, 2 ** 19), (3, 2 ** 19 + 1),
                                 (1, 65), (2, 65), (15, 65), (16, 65), (100, 65)])
def test_std_axis0_is_the_sequential_fp32_recipe(gpu, n, M):
    """blocks of 64 and (from 2^19 cells) 256 threads, partial last blocks, the 16-fold unrolled row loop and its remainder"""
    rng = np.random.default_rng(n * 7 + M)
    a = (rng.standard_normal((n, M)) * 3 + 1).astype(np.float32)
    b = rng.standard_normal((n, M)).astype(np.float32)
    for bb in (None, b):
        for eps in (0.0, 1e-6):
            same_bits(_std(a, bb, eps, off=int(M % 2)), ch.std_seq_ref(a, bb, eps))


def test_std_axis0_nan_and_inf_columns(gpu):
    rng = np.random.default_rng(9)
    a = rng.standard_normal((16, 257)).astype(np.float32)
    a[3, 5], a[15, 256], a[0, 64], a[7, 65] = NAN, INF, -INF, NAN
    a.view(np.uint32)[7, 65] = 0xFFC00000
    got = _std(a, None, 1e-6)
    assert np.isnan(got[[5, 256, 64, 65]]).all() and np.isnan(got).sum() == 4
    same_bits(got, ch.std_seq_ref(a, None, 1e-6))


# ================================================================================================ moments, std from moments
def _moments(x, b, M, stride, sums=None):
    """pre_moments_axis0_f64 on rows ``stride`` floats apart (the pad between rows is NaN); adds into ``sums``."""
    _lib, lib = _L()
    n = x.shape[0]

    def rows(v):
        r = np.full((n, stride), np.nan, np.float32)
        r[:, :M] = v
        return E(r)
    ea, eb = rows(x), (rows(b) if b is not None else None)
    if sums is None:
        sums = E(np.zeros(M, np.float64)), E(np.zeros(M, np.float64))
    rc = lib.pre_moments_axis0_f64(P(ea), P(eb), n, M, stride, P(sums[0]), P(sums[1]), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and sums[0].untouched() and sums[1].untouched()
    return sums


@pytest.mark.parametrize("n,M", [(20, 70), (33, 70), (64, 70), (65, 300), (1000, 8), (7, 300000)])
def test_moments_axis0_one_split_and_several(gpu, n, M):
    """one split adds with +=, several with atomics ((33, 70) upward, but not (7, 300000)); two calls add into the same sums"""
    rng = np.random.default_rng(n + M)
    # every value of x and of x - b is positive (4 +- 0.25 against +-0.1): no column sum cancels, so rtol 1e-12 is a bound an
    # fp64 summation of at most 2000 terms meets in any order (2000 * 2^-53 = 2.2e-13 of the sum)
    x1, x2 = ((rng.standard_normal((n, M)) * 0.25 + 4.0).astype(np.float32) for _ in range(2))
    b1, b2 = ((rng.standard_normal((n, M)) * 0.1).astype(np.float32) for _ in range(2))
    assert min(x1.min(), x2.min(), (x1 - b1).min(), (x2 - b2).min()) > 1.0
    for pad in (0, 3, 64):
        for with_b in (False, True):
            sums = _moments(x1, b1 if with_b else None, M, M + pad)
            s1, q1 = ch.moments_ref(x1, b1 if with_b else None)
            assert np.allclose(host(sums[0]), s1, rtol=1e-12, atol=0.0) and np.allclose(host(sums[1]), q1, rtol=1e-12, atol=0.0)
            sums = _moments(x2, b2 if with_b else None, M, M + pad, sums)
            s2, q2 = ch.moments_ref(np.concatenate([x1, x2]), np.concatenate([b1, b2]) if with_b else None)
            assert np.allclose(host(sums[0]), s2, rtol=1e-12, atol=0.0) and np.allclose(host(sums[1]), q2, rtol=1e-12, atol=0.0)


def _std_from_moments(s, q, n, eps):
    _lib, lib = _L()
    M = len(s)
    es, eq = E(np.asarray(s, np.float64)), E(np.asarray(q, np.float64))
    out = E(np.full(M, -7.0, np.float32), 1)
    rc = lib.pre_std_from_moments_f32(P(es), P(eq), n, M, eps, P(out), _lib.stream())
    got = host(out)
    assert rc == 0 and out.untouched()
    return got


@pytest.mark.parametrize("n", [64, 1000])
def test_std_from_moments_within_the_derived_bound(gpu, n, capsys):
    """mean / std in {0, 1, 1e3, 1e6}^2 and exactly constant columns: |var_got - var_ref| <= (n + 8) 2^-53 E[x^2]
    (tests/CALIB_TESTS.md), asserted on got^2 after allowing one fp32 rounding of the result (2^-23 relative on the std)."""
    x = ch.moments_columns(n)
    M = x.shape[1]
    assert ch.sum_is_exact(x).all()                                # the condition the bound is derived under
    sums = _moments(x, None, M, M + 3)
    s, q = host(sums[0]), host(sums[1])
    got = _std_from_moments(s, q, n, 0.0).astype(np.float64)
    ref_var = ch.std64_ref(x) ** 2
    ex2 = (x.astype(np.float64) ** 2).mean(0)
    bound = ch.moments_std_bound(n, ex2)
    lo, hi = (got * (1 - 2.0 ** -23)) ** 2 - 2.0 ** -298, (got * (1 + 2.0 ** -23)) ** 2 + 2.0 ** -298
    frac = np.maximum(np.maximum(lo - ref_var, ref_var - hi), 0) / np.where(bound > 0, bound, 1.0)
    with capsys.disabled():
        print(f"\n[std_from_moments n={n}] largest fraction of the bound per column: " + " ".join(f"{f:.3f}" for f in frac))
    assert (lo <= ref_var + bound).all() and (hi >= ref_var - bound).all(), frac
    # eps is one more fp32 addition on the same rounded std
    same_bits(_std_from_moments(s, q, n, 1e-6), got.astype(np.float32) + np.float32(1e-6))


def test_std_from_moments_clamps_and_keeps_nan(gpu):
    got = _std_from_moments([10.0, np.nan, 1.0, 0.0, 30.0], [9.0, 1.0, np.nan, 40.0, 90.0], 10, 0.0)
    same_bits(got, [0.0, NAN, NAN, 2.0, 0.0])
    same_bits(got, ch.std_from_moments_ref([10.0, np.nan, 1.0, 0.0, 30.0], [9.0, 1.0, np.nan, 40.0, 90.0], 10))


# ================================================================================================ joint score
def _score(a, b, mod, crop, init, offs=(0, 0, 0), flags=None):
    """pre_joint_score_f32 (or _flagged_f32) on a [n,T,X,Y]; ``offs``: a, b, mod 4 bytes off alignment."""
    _lib, lib = _L()
    n, T, X, Y = a.shape
    ea, eb, em = E(a, offs[0]), (E(b, offs[1]) if b is not None else None), E(mod, offs[2])
    sc = E(np.asarray(init, np.float32))
    if flags is None:
        rc = lib.pre_joint_score_f32(P(ea), P(eb), P(em), n, T, X, Y, *crop, P(sc), _lib.stream())
    else:
        ef = E(np.asarray(flags, np.int32))
        rc = lib.pre_joint_score_flagged_f32(P(ea), P(eb), P(em), n, T, X, Y, *crop, P(ef), P(sc), _lib.stream())
    got = host(sc)
    assert rc == 0 and sc.untouched()
    return got


def _score_data(shape, seed=0, with_b=True):
    rng = np.random.default_rng(seed + sum(shape))
    n = shape[0]
    a = rng.standard_normal(shape, dtype=np.float32)
    b = (rng.standard_normal(shape, dtype=np.float32) * np.float32(0.1)) if with_b else None
    mod = (rng.random(shape[1:], dtype=np.float32) + np.float32(0.5))
    init = np.full(n, 0.125, np.float32)
    init[0] = 1e6
    if n > 2:
        init[1] = NAN
    return a, b, mod, init


CROPS = [(0, 0, 0), (1, 1, 1), (0, 1, 0), (2, 0, 1)]
SMALL_SHAPES = [(5, 6, 9, 10), (5, 3, 7, 10), (5, 6, 9, 64), (3, 5, 33, 128), (3, 5, 33, 130), (2, 2, 3, 1028), (2, 1, 2, 2052)]


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_joint_score_forms_crops_and_bases(gpu, shape):
    """the flat form, the row form with a float4 and with a scalar walk, a partial last span, rows longer than the block;
    every crop, a crop that removes every cell, b null and non-null, then a, b, mod in turn 4 bytes off alignment"""
    a, b, mod, init = _score_data(shape)
    for crop in CROPS + [(shape[1], 0, 0)]:
        for bb in (None, b):
            same_bits(_score(a, bb, mod, crop, init), ch.joint_score_ref(a, bb, mod, crop, init))
    same_bits(_score(a, None, mod, (shape[1], 0, 0), init), init)
    for offs in ((1, 0, 0), (0, 0, 1), (0, 1, 0)):
        for crop in ((0, 0, 0), (1, 1, 1)):
            bb = b if offs[1] else None
            same_bits(_score(a, bb, mod, crop, init, offs), ch.joint_score_ref(a, bb, mod, crop, init))
            same_bits(_score(a, b, mod, crop, init, offs), ch.joint_score_ref(a, b, mod, crop, init))


@pytest.mark.parametrize("shape", [(70, 40, 64, 64), (65537, 1, 1, 64), (65538, 1, 2, 10)], ids=lambda s: "x".join(map(str, s)))
def test_joint_score_many_spans_and_the_batch_slice(gpu, shape):
    """groups > 1 spans per block; the batch slice of the row form at 65 535 samples; a flat form with many samples"""
    a, _, mod, init = _score_data(shape, with_b=False)
    for crop in ((0, 0, 0), (0, 0, 1)):
        same_bits(_score(a, None, mod, crop, init), ch.joint_score_ref(a, None, mod, crop, init))
    n = shape[0]
    flags = (np.arange(n) % 3 == 0).astype(np.int32)
    flags[-2:] = (1, 0)
    ref = ch.joint_score_ref(a, None, mod, (0, 0, 0), init)
    same_bits(_score(a, None, mod, (0, 0, 0), init, flags=flags), np.where(flags != 0, ref, init))


FORM_SHAPES = {"flat": (16, 6, 9, 10), "row_scalar": (16, 3, 7, 10), "row_float4": (16, 6, 9, 64)}


@pytest.mark.parametrize("form", list(FORM_SHAPES))
def test_joint_score_special_cells_kept_and_cropped(gpu, form):
    """NaN / +-inf residuals and NaN / zero / negative / subnormal modulations, each once in a kept cell and once in a
    cropped cell, where it must have no effect; the flagged form changes only the flagged samples"""
    shape = FORM_SHAPES[form]
    n, T, X, Y = shape
    a0, b0, mod0, init = _score_data(shape, seed=3)
    neg_nan = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
    for cell, crop, kept in (((T // 2, X // 2, Y // 2), (0, 0, 0), True), ((T // 2, X // 2, Y // 2), (1, 1, 1), True),
                             ((0, 0, 0), (0, 0, 0), True), ((0, 0, 0), (1, 1, 1), False), ((T // 2, 0, Y - 1), (0, 1, 0), False),
                             ((T // 2, X // 2, Y - 1), (0, 0, 1), False)):
        clean = ch.joint_score_ref(a0, None, mod0, crop, init)
        # residual cells, one kind per sample
        a = a0.copy()
        for i, v in enumerate((NAN, neg_nan, INF, -INF, 0.0, -0.0), start=2):
            a[i][cell] = v
        ref = ch.joint_score_ref(a, None, mod0, crop, init)
        same_bits(_score(a, None, mod0, crop, init), ref)
        if kept:
            assert np.isnan(ref[2]) and np.isnan(ref[3]) and ref[4] == INF and ref[5] == INF
        else:
            same_bits(ref, clean)
        # modulation cells, one kind per launch; sample 2 has residual 0 there, sample 3 a residual of -3, sample 4 +inf
        for mv in (NAN, np.float32(0.0), np.float32(-0.0), np.float32(-0.25), np.float32(1e-40), INF):
            mod, a = mod0.copy(), a0.copy()
            mod[cell], a[2][cell], a[3][cell], a[4][cell] = mv, 0.0, -3.0, INF       # (sample 4: inf / inf is NaN)
            ref = ch.joint_score_ref(a, None, mod, crop, init)
            assert not (kept and mv == INF) or np.isnan(ref[4])
            same_bits(_score(a, None, mod, crop, init), ref)
            same_bits(_score(a, np.zeros_like(a), mod, crop, init), ref)
            if not kept:
                same_bits(ref[4:], clean[4:])
            elif mv == 0 and not np.signbit(mv):
                assert np.isnan(ref[2]) and ref[3] == INF           # 0/0 and x/0
            elif mv == 0:
                assert np.isnan(ref[2]) and np.isfinite(ref[3])     # 0/-0 is NaN, x/-0 is -inf: never raises
            elif mv < 0:                                           # never raises the maximum: as if the cell were not there
                a[3][cell] = 0.0
                same_bits(ref[3:4], ch.joint_score_ref(a[3:4], None, np.abs(mod), crop, init[3:4]))
    flags = np.array([1, 0] * (n // 2), np.int32)
    flags[1] = 1
    ref = ch.joint_score_ref(a0, b0, mod0, (1, 1, 1), init)
    got = _score(a0, b0, mod0, (1, 1, 1), init, flags=flags)
    same_bits(got, np.where(flags != 0, ref, init))


def _planted(form_shape, scalar_walk):
    """One sample per planted pair (calib_helpers.planted_cells): zero residual over modulation 1 everywhere but the two
    cells, which ONE lane sees in memory order - neighbours of a quad in the float4 forms, 256 cells apart in the scalar walk."""
    cells = ch.planted_cells()
    T, X, Y = form_shape
    n = len(cells)
    a, mod = np.zeros((n, T, X, Y), np.float32), np.ones((T, X, Y), np.float32)
    af, mf = a.reshape(n, -1), mod.reshape(-1)
    for i, (_, (av1, sv1), (av2, sv2)) in enumerate(cells):
        c1, c2 = (i, i + 256) if scalar_walk else (4 * i, 4 * i + 1)
        assert c2 < mf.size
        af[i, c1], mf[c1], af[i, c2], mf[c2] = av1, sv1, av2, sv2
    return cells, a, mod


@pytest.mark.parametrize("form,shape,scalar", [("flat", (6, 9, 10), False), ("row_scalar", (2, 3, 130), True), ("row_float4", (6, 9, 64), False)])
def test_joint_score_guarded_divide_planted_cells(gpu, form, shape, scalar):
    """the counterexamples of the guard before guarded_divide.h (m subnormal; thr * sv subnormal with m and sv normal), the
    candidate after and before the cell that sets m, av at thr * sv and 1, 2 ulp below: equal to dividing every cell.
    (Before guarded_divide.h the *_after samples came out as m: the candidate was skipped.)"""
    cells, a, mod = _planted(shape, scalar)
    init = np.zeros(len(cells), np.float32)
    ref = ch.joint_score_ref(a, None, mod, (0, 0, 0), init)
    model, _, _ = ch.guarded_max_model(np.array([[c[1][0], c[2][0]] for c in cells]), np.array([[c[1][1], c[2][1]] for c in cells]))
    same_bits(model, ref)
    got = _score(a, None, mod, (0, 0, 0), init)
    bad = [cells[i][0] for i in np.flatnonzero(ch.bits32(got) != ch.bits32(ref))]
    assert not bad, (form, bad)


# ================================================================================================ segmin, pruned route
@pytest.mark.parametrize("shape", [(5, 8, 36), (17, 13, 20), (33, 10, 64)], ids=lambda s: "x".join(map(str, s)))
def test_segmin_mod(gpu, shape):
    _lib, lib = _L()
    T, X, Y = shape
    rng = np.random.default_rng(sum(shape))
    NS, TC = (X * Y + 63) // 64, (T + 15) // 16
    for cx, cy in ((0, 0), (1, 1)):
        for bad in (None, NAN, 0.0, -1.0):
            mod = (rng.random(shape, dtype=np.float32) + np.float32(0.1))
            if bad is not None:
                mod[T // 2, X // 2, Y // 2], mod[T - 1, 0, 0] = bad, bad          # one kept, one in the rim (kept without a crop)
            em, out = E(mod, 0), E(np.full((TC, NS), -7.0, np.float32), 1)
            rc = lib.pre_segmin_mod_f32(P(em), T, X, Y, cx, cy, P(out), _lib.stream())
            got = host(out)
            assert rc == 0 and out.untouched()
            ref = ch.segmin_ref(mod, cx, cy)
            same_bits(got, ref)
            if bad is not None:
                assert (ref == 0).sum() == (1 if cx else 2)


def _pruned_route(res, mod, cx, cy, scores_e, with_flags, stats_e):
    """moments + segment maxima, segment minima, the pruned pass, then (with flags) the full pass over the flagged samples"""
    _lib, lib = _L()
    n, T, X, Y = res.shape
    vol, NS, TC = T * X * Y, (X * Y + 63) // 64, (T + 15) // 16
    er, em = E(res), E(mod)
    mom = torch.zeros(2, vol, dtype=torch.float64, device="cuda:0")
    segmax = E(np.full((n, TC, NS), -1, np.int32))
    segmin = E(np.full((TC, NS), -7.0, np.float32))
    flags = E(np.full(n, 77, np.int32)) if with_flags else None
    st = _lib.stream()
    assert lib.pre_moments_segmax_f64(P(er), vol, n, T, X, Y, cx, cy, _lib.ptr(mom[0]), _lib.ptr(mom[1]), P(segmax), st) == 0
    assert lib.pre_segmin_mod_f32(P(em), T, X, Y, cx, cy, P(segmin), st) == 0
    assert lib.pre_joint_score_pruned_f32(P(er), vol, P(em), P(segmax), P(segmin), n, T, X, Y, cx, cy, P(scores_e), P(flags),
                                          P(stats_e), st) == 0
    nflag = 0
    if with_flags:
        assert lib.pre_joint_score_flagged_f32(P(er), None, P(em), n, T, X, Y, 0, cx, cy, P(flags), P(scores_e), st) == 0
        f = host(flags)
        assert set(np.unique(f).tolist()) <= {0, 1} and flags.untouched()
        nflag = int(f.sum())
    torch.cuda.synchronize()
    assert segmax.untouched() and segmin.untouched() and scores_e.untouched() and stats_e.untouched()
    return nflag, er, em


PRUNED_CASES = [(4096, 1, 2, 64), (4097, 1, 2, 64), (4099, 1, 2, 64), (4096, 3, 4, 64), (4097, 3, 4, 64), (4099, 3, 4, 64),
                (600, 20, 8, 64), (2100, 20, 8, 64), (9, 40, 12, 64)]


@pytest.mark.parametrize("shape", PRUNED_CASES, ids=lambda s: "x".join(map(str, s)))
def test_pruned_route_equals_the_full_pass(gpu, shape):
    """the wave-per-sample form with 1 to 3 samples in its last block, blocks of 512, 256 and 1024 threads; two slabs, the
    second inheriting the first one's scores; flags null and non-null; a modulation that jumps between neighbouring cells,
    so that the samples without a spike are flagged; the planted guarded-divide cells in the first samples"""
    _lib, lib = _L()
    n, T, X, Y = shape
    vol, total = T * X * Y, ((T + 15) // 16) * ((X * Y + 63) // 64)
    rng = np.random.default_rng(sum(shape))
    cells = ch.planted_cells()[:n // 2]
    slabs = []
    for slab in range(2):
        res = rng.standard_normal(shape, dtype=np.float32)
        mod = ((rng.random((T, X, Y), dtype=np.float32) + np.float32(0.5)) *
               np.where(rng.random((T, X, Y)) < 0.05, np.float32(0.2), np.float32(1.0))).astype(np.float32)
        spike = (T // 2, X // 2, 20)
        mod[spike] = 1.0
        res[len(cells)::3][(slice(None),) + spike] = 200.0 + slab                    # these samples prune, the others do not
        if slab == 0:
            # planted pairs: the two middle cells of a quad, 16 quads per row, from row x = 1 on where the plane has interior
            # rows (X >= 4) - kept under the crop (1, 1) as well, so that they are live with flags null and non-null
            rf, mf = res.reshape(n, -1), mod.reshape(-1)
            rf[:len(cells)] = 0.0
            for i, (_, (av1, sv1), (av2, sv2)) in enumerate(cells):
                c = ((1 if X >= 4 else 0) + i // 16) * Y + 4 * (i % 16) + 1
                assert c + 1 < X * Y and (X < 4 or c // Y < X - 1)
                mf[c], mf[c + 1] = sv1, sv2
                rf[len(cells):, c:c + 2] = 0.0                                       # (no other sample scores on these modulations)
                rf[i, c], rf[i, c + 1] = av1, av2
        slabs.append((res, mod))
    # (the large cases: one crop per flag setting, so that a case stays within a few seconds)
    combos = [(False, (0, 0)), (True, (1, 1))] if n * vol > 4_000_000 else [(f, c) for f in (False, True) for c in ((0, 0), (1, 1))]
    for with_flags, (cx, cy) in combos:
        full = E(np.zeros(n, np.float32))
        pruned = E(np.zeros(n, np.float32))
        stats = E(np.zeros(3, np.int64))
        flagged, prev = [], None
        for slab, (res, mod) in enumerate(slabs):
            nflag, er, em = _pruned_route(res, mod, cx, cy, pruned, with_flags, stats)
            flagged.append(nflag)
            assert lib.pre_joint_score_f32(P(er), None, P(em), n, T, X, Y, 0, cx, cy, P(full), _lib.stream()) == 0
            got, want = host(pruned), host(full)
            same_bits(want, ch.joint_score_ref(res, None, mod, (0, cx, cy), prev))
            same_bits(got, want)
            assert slab or (X < 4 and cx) or (want[:len(cells)] > 0).all()           # the planted cells are live in this run
            prev = want.copy()
            s = host(stats)
            assert s[1] == (slab + 1) * n * total and s[0] <= s[1], s
        if with_flags and total >= 8:
            assert 0 < flagged[0] < n, flagged                                       # some samples flagged, some not


# ================================================================================================ coverage
def _cov_data(n, M, per_sample, seed):
    rng = np.random.default_rng(seed + n * 31 + M)
    y = rng.standard_normal((n, M), dtype=np.float32)
    shp = (n, M) if per_sample else (M,)
    lo = -np.abs(rng.standard_normal(shp, dtype=np.float32)) - np.float32(0.1)
    hi = np.abs(rng.standard_normal(shp, dtype=np.float32)) + np.float32(0.1)
    y[0] = lo[0] if per_sample else lo                              # a sample exactly on its lower bounds
    if n > 1:
        y[n - 1] = hi[n - 1] if per_sample else hi                  # and one on its upper bounds
    if n > 3:
        y[2, M // 2] = NAN
        if per_sample:
            lo[3, 0] = NAN
    return y, lo, hi


def _cov_all(y, lo, hi, per_sample, offs=(0, 0, 0)):
    """the three coverage entry points on the same operands; returns what each added to / cleared in its output"""
    _lib, lib = _L()
    n, M = y.shape
    ey, el, eh = E(y, offs[0]), E(lo, offs[1]), E(hi, offs[2])
    st = _lib.stream()
    count = E(np.array([1000], np.int64))
    assert lib.pre_cov_count_f32(P(ey), P(el), P(eh), n, M, per_sample, P(count), st) == 0
    assert int(host(count)[0]) - 1000 == ch.cov_count_ref(y, lo, hi, per_sample) and count.untouched()
    for outside in (0, 1):
        counts = E(np.full(n, 5, np.int32))
        assert lib.pre_cov_rowcount_f32(P(ey), P(el), P(eh), n, M, per_sample, outside, P(counts), st) == 0
        assert np.array_equal(host(counts).astype(np.int64) - 5, ch.cov_rowcount_ref(y, lo, hi, per_sample, outside)), outside
        assert counts.untouched()
    start = np.ones(n, np.uint8)
    start[n // 2] = 0                                               # `inside` is only ever cleared
    inside = E(start)
    assert lib.pre_cov_joint_f32(P(ey), P(el), P(eh), n, M, per_sample, P(inside), st) == 0
    assert np.array_equal(host(inside) != 0, ch.cov_joint_ref(y, lo, hi, per_sample) & (start != 0)) and inside.untouched()


COV_CASES = [(1, 4), (7, 8), (8, 8), (9, 8), (100, 8), (53, 96), (5, 1028), (50, 42), (3, 7)]


@pytest.mark.parametrize("n,M", COV_CASES)
def test_coverage_forms_and_bases(gpu, n, M):
    """float4 forms with sample groups of whole eights and a ragged last one, the scalar forms (M % 4 != 0, or any operand
    4 bytes off), per-cell and per-sample bounds"""
    for per_sample in (0, 1):
        y, lo, hi = _cov_data(n, M, per_sample, 1)
        for offs in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            _cov_all(y, lo, hi, per_sample, offs)


def test_coverage_across_the_batch_slice(gpu):
    n, M = 65536 + 3, 4
    y, lo, hi = _cov_data(n, M, 1, 2)
    y[65535:, :] = np.array([[0.0, 0.0, 0.0, 0.0], [9.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, -9.0], [0.0, 0.0, 0.0, 0.0]], np.float32)
    lo[65535:], hi[65535:] = -1.0, 1.0
    _cov_all(y, lo, hi, 1)
    _cov_all(y, lo, hi, 1, (1, 0, 0))


@pytest.mark.parametrize("M", [8, 7])
def test_coverage_special_values(gpu, M):
    """y on a bound (inside, and outside too in rowcount's outside mode), NaN in y or in a bound (neither), lo > hi, infinite
    bounds, -0.0 against +0.0"""
    y, lo, hi = ch.cov_special_rows(M)
    _cov_all(y, lo, hi, 1)
    _cov_all(y, lo, hi, 1, (0, 0, 1))
    for i in range(y.shape[0]):                                     # each special row as the per-cell bounds of all samples
        _cov_all(np.concatenate([y, y[::-1]]), lo[i], hi[i], 0)
