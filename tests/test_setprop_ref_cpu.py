"""CPU tests of tests/setprop_helpers.py, before anything of it judges a kernel: the loops written out from the header against
set_prop._bounds_host / recipe_sets_host and against the literal zonotope pipeline of tests/test_set_prop_cpu.py, the exactness
condition, and the launch plan of tests/ODE_TESTS.md row by row."""
import numpy as np
import pytest

import setprop_helpers as sh
from cp_pre_amd import set_prop as sp
from test_set_prop_cpu import K5, K7, SHO_K, literal_propagate, literal_set_PRE, noisy_cosine


@pytest.mark.parametrize("N", (1, 2, 3, 31, 33, 65))
def test_bounds_ref_is_the_hosts_closed_form(N):
    rng = np.random.default_rng(N)
    c, r = rng.standard_normal((5, N)), rng.random((5, N))
    c[1, N // 2] = np.nan
    r[3, 0] = np.inf
    for hull in sp.HULLS:
        g, a = sp.tables(sh.H_of(N, N), hull)
        lo, hi = sh.bounds_ref(c, r, g, a)
        want_lo, want_hi = sp._bounds_host(c, r, g, a)
        assert np.isnan(lo[[1, 3]]).all() and np.array_equal(np.isnan(lo), np.isnan(want_lo))
        t = sh.tol(N, sh.bounds_magnitude(c, r, g, a))
        ok = ~np.isnan(lo)
        sh.within(lo[ok], want_lo[ok], t[ok])
        sh.within(hi[ok], want_hi[ok], t[ok])
    ci, ri = sh.ints(rng, -3, 3, 4, N), sh.ints(rng, 0, 3, 4, N)
    gi, ai = sh.int_tables(rng, N)
    sh.assert_exact_f64(sh.bounds_magnitude(ci, ri, gi, ai), ci, ri, gi, ai)
    want = sp._bounds_host(ci, ri, gi, ai)
    got = sh.bounds_ref(ci, ri, gi, ai)
    sh.same_f64(got[0], want[0])
    sh.same_f64(got[1], want[1])


@pytest.mark.parametrize("n", (5, 8, 13))
def test_bounds_ref_against_the_literal_pipeline(n):
    rng = np.random.default_rng(n)
    c, r = rng.standard_normal(n), rng.random(n)
    H = sh.H_of(n, n)
    want = literal_propagate(c - r, c + r, H)
    g, a = sp.tables(H)
    lo, hi = sh.bounds_ref(c[None], r[None], g, a)
    t = 1e-12 * sh.bounds_magnitude(c[None], r[None], g, a)[0]
    assert np.all(np.abs(lo[0] - want[:, 0]) <= t) and np.all(np.abs(hi[0] - want[:, 1]) <= t)


@pytest.mark.parametrize("kernel,correlation", [(SHO_K, False), (SHO_K, True), (K5, False), (K7, True)])
def test_recipe_ref_against_the_literal_set_PRE(kernel, correlation):
    nt = 12
    x = noisy_cosine(nt, 7)
    want = literal_set_PRE(x, kernel, correlation)
    g, a = sp.tables(sp.recipe_key(kernel, nt, 1e-6, correlation))
    lo, hi = sh.recipe_ref(x[None], kernel, correlation, None, g, a)
    t = 1e-12 * sh.recipe_magnitude(x[None], kernel, correlation, None, g, a)[0]
    assert np.all(np.abs(lo[0] - want[:, 0]) <= t) and np.all(np.abs(hi[0] - want[:, 1]) <= t)


@pytest.mark.parametrize("nt", (3, 4, 5, 9, 32))
@pytest.mark.parametrize("correlation", (False, True))
def test_recipe_sets_are_the_hosts(nt, correlation):
    rng = np.random.default_rng(nt)
    x = rng.integers(-4, 5, (3, nt)).astype(np.float32)
    q_rows = rng.integers(1, 9, (3, nt)).astype(np.float32)
    for k in (1, 2, 3, 4, 5, 6, 7):
        if k > nt + 2:
            continue
        taps = rng.integers(1, 4, k).astype(np.float64)
        if k % 2 and not correlation:
            taps = np.r_[taps[:k // 2 + 1], taps[:k // 2][::-1]]           # symmetric: q-hat is defined
        qs = (None, 2.0, q_rows[0], q_rows) if k % 2 else (None,)
        for q in qs:
            c, r, bad = sh.recipe_sets(x, taps, correlation, q)
            wc, wr, wbad = sp.recipe_sets_host(x, taps, correlation, q)
            assert np.array_equal(c, wc) and np.array_equal(r, wr) and np.array_equal(bad, wbad), (k, q is None)
        assert k % 2 == 0 or sh.qhat_shift(k, correlation) == sp.qhat_shift(k, correlation)      # (derived for odd k only)
    xb = x.copy()
    xb[1, 0], xb[2, nt - 1] = np.nan, np.inf
    taps = np.array([1.0, 2.0, 1.0])
    for q in (None, 2.0):
        c, r, bad = sh.recipe_sets(xb, taps, correlation, q)
        assert bad.tolist() == [False, True, True] and np.array_equal(bad, sp.recipe_sets_host(xb, taps, correlation, q)[2])


def test_steps_that_leave_the_field_keep_the_convolved_radius():
    # with correlation the last (k - 1) / 2 + 1 interior n step past the field's end; without it none does
    assert sh.steps_outside(9, 3, True) == [9] and sh.steps_outside(9, 5, True) == [8, 9]
    assert sh.steps_outside(9, 7, True) == [7, 8, 9] and sh.steps_outside(5, 7, True) == [4, 5]
    assert all(sh.steps_outside(nt, k, False) == [] for nt in (3, 4, 5, 9, 64) for k in (1, 3, 5, 7))
    assert sh.steps_outside(9, 1, True) == [] and sh.steps_outside(3, 3, True) == []     # Nt = 3: no interior at all
    x = np.arange(1.0, 10.0)[None]
    c, r, _ = sh.recipe_sets(x, [1.0, 0.0, 2.0, 0.0, 1.0], True, np.full(9, 100.0))
    conv = sh.recipe_conv(x, [1.0, 0.0, 2.0, 0.0, 1.0], True)
    assert np.array_equal(r[0, [7, 8]], np.abs(conv[0, [8, 9]])) and np.all(r[0, 3:7] == 100.0)


def test_exactness_condition_holds_and_fails_where_it_should():
    rng = np.random.default_rng(5)
    N = 513
    c, r = sh.ints(rng, -3, 3, 9, N), sh.ints(rng, 0, 3, 9, N)
    g, a = sh.int_tables(rng, N)
    mag = sh.bounds_magnitude(c, r, g, a)
    sh.assert_exact_f64(mag, c, r, g, a)
    assert mag.max() <= N * 18
    with pytest.raises(AssertionError):
        sh.assert_exact_f64(sh.bounds_magnitude(c * 2.0 ** 45, r, g, a), c * 2.0 ** 45, r, g, a)
    with pytest.raises(AssertionError, match="integer"):
        sh.assert_exact_f64(mag, c + 0.5)


@pytest.mark.parametrize("N", sh.NS)
def test_plan_rows(N):
    for B in sh.batches(N):
        p = sh.assert_plan(B, N)
        assert p.window == p.TK + 31 and p.blocks == p.tiles * p.groups
        assert (p.chunks - 1) * 32 + p.jmax == N and 1 <= p.jmax <= 32
    assert sh.batches(N) == {64: (1, 31, 32, 33), 128: (1, 15, 16, 17), 256: (1, 7, 8, 9)}[sh.plan(1, N).TK]


def test_table_covers_what_the_issue_lists():
    assert {N % 32 for N in sh.NS} >= {0, 1, 31}
    assert {sh.plan(1, N).TK for N in sh.NS} == {64, 128, 256}
    for lo, hi in ((64, 65), (128, 129)):
        assert sh.plan(1, lo).TK != sh.plan(1, hi).TK
    assert sh.plan(1, 256).tiles == 1 and sh.plan(1, 257).tiles == 2
    assert all(sh.plan(1, N).wraps >= 2 for N in sh.NS if N < 32)
    assert sh.plan(0, 5).blocks == 0
