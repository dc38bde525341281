"""The numpy references of tests/calib_helpers.py on the CPU: against oracle.conformal and the committed goldens where the
oracle covers a case, against hand-written expectations (what numpy itself returns) at the special values, and the guarded
divide of cp_pre_amd/csrc/guarded_divide.h run on the host against straight division.  The GPU tests of
tests/test_gpu_calib_seams.py rest on references that were checked here."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import calib_helpers as ch
from conftest import load_golden
from oracle import conformal as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cp_pre_amd", "csrc")
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _eqbits(a, b):
    return np.array_equal(ch.bits32(a), ch.bits32(b))


# ------------------------------------------------------------------------------------------------ goldens / oracle
@pytest.mark.parametrize("n", [7, 100, 256])
def test_references_reproduce_the_committed_goldens(n):
    g = load_golden("conformal.npz")
    s, r = g[f"scores|{n}"], g[f"res|{n}"]
    zero = np.zeros_like(r)
    mod = ch.std_seq_ref(r, zero).reshape(r.shape[1:])
    assert _eqbits(mod, g[f"mod|{n}"]) and _eqbits(ch.std_seq_ref(r).reshape(r.shape[1:]), g[f"mod|{n}"])
    r4 = r.reshape(n, 1, *r.shape[1:]) if r.ndim == 3 else r.reshape(n, 1, 1, -1)
    js = ch.joint_score_ref(r4, None, mod.reshape(r4.shape[1:]))
    assert _eqbits(js, g[f"jscore|{n}"]) and _eqbits(js, oc.ncf_metric_joint(r, zero, mod))
    assert _eqbits(ch.absdiff_ref(r, zero), np.abs(r))
    for i, a in enumerate(oc.ALPHA_LEVELS):
        k = int(g[f"k|{n}|{i}"])
        if k < 0:
            continue
        if s.ndim == 1:
            assert _eqbits(ch.kth_ref(s, [k]), [g[f"qhat|{n}|{i}"]])
        q = ch.kth_ref(js, [k])[0]
        assert _eqbits([q], [oc.calibrate(js, n, a)])
        lo, hi = (-q * mod).reshape(-1), (q * mod).reshape(-1)
        y = r.reshape(n, -1)
        inside = ch.cov_joint_ref(y, lo, hi, False)
        assert np.array_equal(inside, oc.filter_sims_joint([-q * mod, q * mod], r))
        assert ch.cov_count_ref(y, lo, hi, False) == int(((r >= -q * mod) & (r <= q * mod)).sum())
        for thr in (0.5, 0.9):
            for within in (False, True):
                cnt = ch.cov_rowcount_ref(y, lo, hi, False, 0 if within else 1)
                assert np.array_equal(cnt / y.shape[1] >= thr, oc.filter_sims_within_bounds(-q * mod, q * mod, r, thr, within))


def test_joint_reference_on_the_reference_executed_vectors():
    g = load_golden("conformal_ref.npz")
    for n in (7, 100, 256):
        cal = g[f"cal|{n}"][:, 1:-1, 1:-1]
        mod = ch.std_seq_ref(cal).reshape(cal.shape[1:])
        assert _eqbits(mod, g[f"mod|{n}"])
        full = g[f"cal|{n}"]
        modf = np.ones(full.shape[1:], np.float32)
        modf[1:-1, 1:-1] = mod
        js = ch.joint_score_ref(full[:, None], None, modf[None], crop=(0, 1, 1))        # the crop instead of the slice
        assert _eqbits(js, g[f"jscore|{n}"])


# ------------------------------------------------------------------------------------------------ select
def test_kth_ref_is_np_sort_and_np_quantile():
    rng = np.random.default_rng(1)
    for N in (1, 2, 65, 1025):
        for s in (rng.standard_normal(N), np.round(rng.standard_normal(N) * 8) / 8, np.full(N, 2.5),
                  np.where(np.arange(N) % 2 == 0, -0.0, 0.0), rng.standard_normal(N) * 1e-42):
            s = s.astype(np.float32)
            ks = np.unique(np.clip([0, 1, N // 2, N - 2, N - 1], 0, N - 1))
            got = ch.kth_ref(s, ks)
            assert got.dtype == np.float32 and np.array_equal(got, np.sort(s)[ks])        # (values: -0.0 == +0.0)
            for k, v in zip(ks, got):
                assert v == np.quantile(s, k / max(N - 1, 1), method="higher") or N == 1
    # the total order decides what np.sort leaves open: all -0.0 come before all +0.0
    s = np.array([0.0, -0.0, 0.0, -0.0, -1.0, 1.0], np.float32)
    assert ch.bits32(ch.kth_ref(s, [0, 1, 2, 3, 4, 5])).tolist() == ch.bits32([-1.0, -0.0, -0.0, 0.0, 0.0, 1.0]).tolist()
    # inf sorts at the ends
    assert _eqbits(ch.kth_ref(np.array([INF, 1, -INF, 2], np.float32), [0, 3]), [-INF, INF])


def test_kth_ref_nan_of_either_sign_makes_every_rank_nan():
    s = np.arange(9, dtype=np.float32)
    for nanbits in (0x7FC00000, 0xFFC00000, 0x7F800001):
        t = s.copy()
        t.view(np.uint32)[5] = nanbits
        assert np.isnan(ch.kth_ref(t, [0, 4, 8])).all()
        assert np.isnan(np.quantile(t, 0.5, method="higher"))                            # what numpy itself returns


# ------------------------------------------------------------------------------------------------ |a-b|, std, moments
def test_absdiff_ref_special_values():
    a = np.array([-0.0, 0.0, INF, -INF, NAN, 1.0, INF, -1.5], np.float32)
    b = np.array([0.0, -0.0, 1.0, 1.0, 1.0, NAN, INF, 2.0], np.float32)
    got = ch.absdiff_ref(a, b)
    assert _eqbits(got, [0.0, 0.0, INF, INF, NAN, NAN, NAN, 3.5])
    neg = a.copy()
    neg.view(np.uint32)[4] = 0xFFC00000
    assert (ch.absdiff_ref(neg).view(np.uint32) >> 31 == 0).all() and (got.view(np.uint32)[:4] >> 31 == 0).all()


def test_std_seq_ref_is_the_stated_recipe_and_np_std_on_rows():
    rng = np.random.default_rng(2)
    for n, M in ((1, 5), (2, 7), (17, 65), (100, 3)):
        a = (rng.standard_normal((n, M)) * 3 + 1).astype(np.float32)
        b = rng.standard_normal((n, M)).astype(np.float32)
        assert _eqbits(ch.std_seq_ref(a, b), np.std(a - b, axis=0))                     # numpy reduces axis 0 row by row
        assert _eqbits(ch.std_seq_ref(a, None, 1e-6), np.std(a, axis=0) + np.float32(1e-6))
        # by hand, one column, python floats rounded after every operation
        x = a[:, 0]
        s = np.float32(0)
        for v in x:
            s = np.float32(s + v)
        mean = np.float32(s / np.float32(n))
        acc = np.float32(0)
        for v in x:
            d = np.float32(v - mean)
            acc = np.float32(acc + np.float32(d * d))
        assert ch.std_seq_ref(a)[0] == np.float32(np.sqrt(np.float32(acc / np.float32(n))))
    a = np.ones((4, 3), np.float32)
    a[1, 0], a[2, 1] = NAN, INF
    got = ch.std_seq_ref(a)
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == 0.0                      # inf: inf - inf in the second pass


def test_moments_and_std_from_moments_refs_and_the_bound():
    for n in (64, 1000):
        x = ch.moments_columns(n)
        assert x.shape == (n, 21) and ch.sum_is_exact(x).all()         # the condition CALIB_TESTS.md derives the bound under
        assert not ch.sum_is_exact(np.array([[1.0], [2.0 ** -60], [-1.0]], np.float32))[0]
        s, q = ch.moments_ref(x)
        assert s.dtype == np.float64 and np.array_equal(s, x.astype(np.float64).sum(0))
        got = ch.std_from_moments_ref(s, q, n).astype(np.float64)
        ref_var = ch.std64_ref(x) ** 2
        assert (ref_var[3::4][:4] > 0).all() and (ref_var[0:16:4] == 0).all() and (ref_var[16:] == 0).all()
        bound = ch.moments_std_bound(n, (x.astype(np.float64) ** 2).mean(0))
        # one fp32 rounding of the result: 2^-23 relative on the std, as the GPU test allows
        lo, hi = (got * (1 - 2.0 ** -23)) ** 2 - 2.0 ** -298, (got * (1 + 2.0 ** -23)) ** 2 + 2.0 ** -298
        assert (lo <= ref_var + bound).all() and (hi >= ref_var - bound).all(), n
    assert ch.std_from_moments_ref([10.0], [9.0], 10)[0] == 0.0                          # negative variance clamps
    assert np.isnan(ch.std_from_moments_ref([NAN, 1.0], [1.0, NAN], 10)).all()
    assert ch.std_from_moments_ref([0.0], [40.0], 10, 1e-6)[0] == np.float32(2.0) + np.float32(1e-6)


# ------------------------------------------------------------------------------------------------ joint score
def test_joint_score_ref_special_cells():
    T, X, Y = 3, 4, 5
    a = np.full((12, T, X, Y), 0.5, np.float32)
    mod = np.full((T, X, Y), 2.0, np.float32)
    cell = (1, 2, 2)
    exp = [0.25] * 12
    a[1][cell] = NAN; exp[1] = NAN
    a[2][cell] = INF; exp[2] = INF
    a[3][cell] = -INF; exp[3] = INF
    a[4][cell] = -8.0; exp[4] = 4.0
    init = np.full(12, 0.125, np.float32)
    init[5] = 7.0; exp[5] = 7.0
    init[6] = NAN; exp[6] = NAN
    assert _eqbits(ch.joint_score_ref(a, None, mod, (0, 0, 0), init), exp)
    assert _eqbits(ch.joint_score_ref(a, np.zeros_like(a), mod, (1, 1, 1), init), exp)     # the cell is kept by the crop
    # the same cells cropped away: no effect
    cropped = (0, 0, 0)
    a2 = np.full_like(a, 0.5)
    for i, v in ((1, NAN), (2, INF), (3, -INF), (4, -8.0)):
        a2[i][cropped] = v
    exp2 = [0.25] * 12
    exp2[5], exp2[6] = 7.0, NAN
    assert _eqbits(ch.joint_score_ref(a2, None, mod, (1, 1, 1), init), exp2)
    # modulation cells: NaN, 0 over residual 0 (NaN) and != 0 (inf), negative (never raises), subnormal
    one = np.full((1, T, X, Y), 0.5, np.float32)
    for mv, av, want in ((NAN, 0.5, NAN), (0.0, 0.0, NAN), (0.0, 0.5, INF), (-1e-3, 0.5, 0.25), (-0.0, 0.5, 0.25),
                         (np.float32(1e-40), 0.5, INF), (np.float32(1e-40), 1e-5, np.float32(1e-5) / np.float32(1e-40))):
        m2, o2 = mod.copy(), one.copy()
        m2[cell], o2[0][cell] = mv, av
        assert _eqbits(ch.joint_score_ref(o2, None, m2), [want]), (mv, av)
        with np.errstate(all="ignore"):                                  # (what numpy's own max of quotients returns)
            assert mv <= 0 or _eqbits(ch.joint_score_ref(o2, None, m2), np.max(np.abs(o2) / m2, axis=(1, 2, 3)))
    # every cell cropped: the incoming scores, NaN included
    assert _eqbits(ch.joint_score_ref(a, None, mod, (2, 0, 0), init), init)


def test_segmin_ref_by_loops():
    rng = np.random.default_rng(4)
    for (T, X, Y), (cx, cy) in (((5, 8, 36), (1, 1)), ((17, 13, 20), (0, 0)), ((33, 3, 5), (1, 0)), ((2, 2, 70), (1, 1))):
        mod = (rng.random((T, X, Y)) + 0.1).astype(np.float32)
        mod[T // 2, X // 2, Y // 2] = NAN
        mod[0, X - 1, Y - 1] = -1.0
        mod[T - 1, 0, 0] = 0.0
        NS, TC = (X * Y + 63) // 64, (T + 15) // 16
        exp = np.full((TC, NS), INF, np.float32)
        bad = np.zeros((TC, NS), bool)
        for t in range(T):
            for x in range(cx, X - cx):
                for y in range(cy, Y - cy):
                    v, j = mod[t, x, y], (t // 16, (x * Y + y) // 64)
                    bad[j] |= not (v > 0)
                    exp[j] = min(exp[j], v) if not np.isnan(v) else exp[j]
        exp[bad] = 0.0
        assert _eqbits(ch.segmin_ref(mod, cx, cy), exp)


# ------------------------------------------------------------------------------------------------ coverage
def test_coverage_refs_special_values():
    y, lo, hi = ch.cov_special_rows(8)
    inside_special = [1, 1, 0, 0, 0, 0, 1, 1, 0, 1, 1, 1]            # the special cell of each row: inside?
    outside_special = [1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1]           # y <= lo or y >= hi (a cell ON a bound: both)
    assert ch.cov_rowcount_ref(y, lo, hi, True, 0).tolist() == [7 + v for v in inside_special]
    assert ch.cov_rowcount_ref(y, lo, hi, True, 1).tolist() == outside_special
    assert ch.cov_joint_ref(y, lo, hi, True).tolist() == [bool(v) for v in inside_special]
    assert ch.cov_count_ref(y, lo, hi, True) == 7 * 12 + sum(inside_special)
    # per-cell bounds: one row of bounds for all samples
    assert ch.cov_count_ref(y, lo[0], hi[0], False) == int(((y >= lo[:1]) & (y <= hi[:1])).sum())
    assert ch.cov_joint_ref(y, lo[0], hi[0], False).tolist() == oc.filter_sims_joint([lo[0], hi[0]], y).tolist()


# ------------------------------------------------------------------------------------------------ memory
def test_embed_places_the_operand_and_watches_the_frame():
    t = torch.arange(10, dtype=torch.float32).reshape(2, 5)
    for off in (0, 1):
        e = ch.embed(t, off, 8)
        assert e.view.data_ptr() % 16 == (4 * off) and torch.equal(e.view, t) and e.untouched()
        assert torch.isnan(e.alloc[:e.lo]).all() and torch.isnan(e.alloc[e.hi:]).all() and e.alloc.numel() - e.hi >= 8
        e.view.fill_(3.0)
        assert e.untouched()
        e.alloc[e.hi] = 1.0
        assert not e.untouched()
    for dt in (torch.int32, torch.int64, torch.uint8, torch.float64):
        e = ch.embed(torch.zeros(5, dtype=dt), 0, 4)
        assert e.untouched()
        e.alloc[e.lo - 1] = 1
        assert not e.untouched()


# ------------------------------------------------------------------------------------------------ the guarded divide
def test_guarded_model_counterexamples_bite_on_the_parent_form_only():
    for m, sv, av in ch.COUNTEREXAMPLES:
        with np.errstate(all="ignore"):
            assert np.float32(av / sv) > m                               # the cell does raise the maximum
        for cells in (([m, av], [1.0, sv]), ([av, m], [sv, 1.0])):
            want, _ = ch.plain_max(*cells)
            got, nan, div = ch.guarded_max_model(*cells)
            assert _eqbits(got, want) and not nan.any()
        want, _ = ch.plain_max([m, av], [1.0, sv])
        old, _, div = ch.guarded_max_model([m, av], [1.0, sv], parent=True)
        assert old[0] == m and want[0] > m and not div[0, 1]           # the parent's form skips it
    # inf / inf over an infinite modulation, once the maximum is positive: NaN by division, skipped by the parent's form
    _, nan, _ = ch.guarded_max_model([1.0, INF], [1.0, INF])
    _, nan_old, _ = ch.guarded_max_model([1.0, INF], [1.0, INF], parent=True)
    assert nan[0] and ch.plain_max([1.0, INF], [1.0, INF])[1][0] and not nan_old[0]


def test_guarded_model_equals_plain_division_on_planted_cells_and_random_lanes():
    cells = ch.planted_cells()
    assert len(cells) >= 2 * (2 + 3 + 6) - 2
    av = np.array([[c[1][0], c[2][0]] for c in cells], np.float32)
    sv = np.array([[c[1][1], c[2][1]] for c in cells], np.float32)
    want, wnan = ch.plain_max(av, sv)
    got, nan, div = ch.guarded_max_model(av, sv)
    assert _eqbits(got, want) and np.array_equal(nan, wnan)
    old, _, _ = ch.guarded_max_model(av, sv, parent=True)
    assert (ch.bits32(old) != ch.bits32(want)).sum() >= 4               # the planted cells bite on the parent's form
    rng = np.random.default_rng(5)
    L, K = 4096, 64
    sv = np.exp2(rng.uniform(-4, 4, (L, K))).astype(np.float32)
    av = (np.abs(rng.standard_normal((L, K))) * sv).astype(np.float32)
    av[::7, 3], sv[::11, 5], sv[::13, 9], sv[::17, 2] = NAN, 0.0, -1.0, 1e-40
    want, wnan = ch.plain_max(av, sv)
    got, nan, div = ch.guarded_max_model(av, sv)
    assert _eqbits(np.where(wnan, NAN, want), np.where(nan, NAN, got)) and np.array_equal(nan, wnan)
    assert 0.02 < div.mean() < 0.5                                       # most cells skip, the candidates divide


def test_guarded_divide_host_program(tmp_path):
    """tests/c_abi/guarded_divide_main.cpp runs the kernels' own function (guarded_divide.h) on the host against straight
    division: no mismatch, and in every regime both routes - the skip and the divide - were taken."""
    exe = tmp_path / "guarded_divide"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "c_abi", "guarded_divide_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "guarded divide ok" in r.stdout, r.stdout + r.stderr
    rows = re.findall(r"^(\w+)\s+skipped (\d+) divided (\d+) mismatches (\d+)$", r.stdout, flags=re.M)
    assert [x[0] for x in rows] == ["grid", "edge", "random", "special"]
    for name, skipped, divided, bad in rows:
        assert int(skipped) > 0 and int(divided) > 0 and int(bad) == 0, (name, skipped, divided, bad)
    assert int(rows[2][1]) + int(rows[2][2]) >= 2_000_000


def test_the_guarded_divide_is_stated_once():
    """calib.hip and screen_plane.h include guarded_divide.h, and the Makefile rebuilds their objects when it changes (what the
    function computes is checked by the host program above and by the planted cells of the GPU tests)."""
    for f in ("calib.hip", "screen_plane.h"):
        assert '#include "guarded_divide.h"' in open(os.path.join(CSRC, f)).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SHARED_HDRS := .*\bguarded_divide\.h\b", mk, flags=re.M)
    assert re.search(r"^SHARED_OBJS := .*\bcalib\.o\b", mk, flags=re.M)
