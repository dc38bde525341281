"""The numpy references, the plan restatement and the planted cells of tests/bounds_helpers.py on the CPU: against loops
written out by hand, against float64 arithmetic rounded once per operation, against exact rational arithmetic, and the plan
against the branch every row of the table in tests/BOUNDS_TESTS.md claims.  The GPU tests of
tests/test_gpu_bounds_seams.py rest on what is checked here."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import bounds_helpers as bh

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _eq(a, b):
    return np.array_equal(bh.bits32(a), bh.bits32(b))


# ------------------------------------------------------------------------------------------------ references
def _cellwise_loop(u, r, blo, bhi):
    """the per-cell loop of test_gpu_sample_bounds._cellwise_want, restated"""
    nk, M = blo.shape[0], u.shape[1]
    lo, hi = np.full((nk, M), np.inf, np.float32), np.full((nk, M), -np.inf, np.float32)
    cnt = np.zeros((nk, M), np.int32)
    for k in range(nk):
        ins = (r >= blo[k]) & (r <= bhi[k])
        for j in range(M):
            sel = u[:, j][ins[:, j]]
            cnt[k, j] = sel.size
            if sel.size:
                lo[k, j], hi[k, j] = sel.min(), sel.max()
    return lo, hi, cnt


def test_cellwise_ref_is_the_per_cell_loop_with_nan_in_u_and_r():
    rng = np.random.default_rng(0)
    u, r = rng.standard_normal((9, 7)).astype(np.float32), rng.standard_normal((9, 7)).astype(np.float32)
    u[2, 3], u[4, 0], r[5, 3], r[2, 1] = NAN, NAN, NAN, NAN
    r[4, 0] = 0.0                                                  # NaN in u inside at every level
    u[1, 6], u[3, 6] = INF, -INF
    blo, bhi = bh.sets_f32(np.array([0.0, 0.4, 1.0, 9.0], np.float32), None, (0.1 * rng.standard_normal(7)).astype(np.float32))
    blo[1, 5] = NAN                                                # a NaN bound: nothing inside
    got, want = bh.cellwise_ref(u, r, blo, bhi), _cellwise_loop(u, r, blo, bhi)
    assert _eq(got[0], want[0]) and _eq(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.isnan(got[0][3, 3]) and np.isnan(got[1][3, 0]) and got[2][3, 3] == 8 and got[2][1, 5] == 0
    assert got[0][1, 5] == INF and got[1][1, 5] == -INF and got[0][3, 6] == -INF and got[1][3, 6] == INF
    assert np.array_equal(bh.rowcount_ref(r, blo, bhi), np.stack([((r >= blo[k]) & (r <= bhi[k])).sum(1) for k in range(4)]))


def test_envelope_ref_is_the_hand_written_loop():
    rng = np.random.default_rng(1)
    u = rng.standard_normal((11, 5)).astype(np.float32)
    u[3, 2], u[7, 4] = NAN, NAN                                    # sample 3 accepted at level 0, sample 7 never
    acc = rng.random((4, 11)) < 0.5
    acc[0, 3], acc[:, 7], acc[2] = True, False, False
    lo, hi, cnt = bh.envelope_ref(u, acc)
    for k in range(4):
        for j in range(5):
            best_lo, best_hi, seen_nan = np.inf, -np.inf, False
            for s in range(11):
                if acc[k, s]:
                    v = u[s, j]
                    seen_nan |= bool(np.isnan(v))
                    best_lo, best_hi = min(best_lo, v), max(best_hi, v)
            if seen_nan:
                assert np.isnan(lo[k, j]) and np.isnan(hi[k, j])
            else:
                assert lo[k, j] == np.float32(best_lo) and hi[k, j] == np.float32(best_hi)
        assert cnt[k] == sum(acc[k])
    assert np.isnan(lo[0, 2]) and not np.isnan(lo[:, 4]).any() and (lo[2] == INF).all() and (hi[2] == -INF).all() and cnt[2] == 0


def test_merge_ref_and_the_comparison():
    prior = (np.array([1.0, -2.0, NAN, 0.0], np.float32), np.array([1.0, 5.0, 0.0, NAN], np.float32), np.array([3, 0, 1, 2], np.int32))
    new = (np.array([0.5, INF, 1.0, NAN], np.float32), np.array([NAN, -INF, 1.0, 2.0], np.float32), np.array([1, 0, 2, 5], np.int32))
    lo, hi, cnt = bh.merge_ref(new, prior)
    assert _eq(lo, [0.5, -2.0, NAN, NAN]) and _eq(hi, [NAN, 5.0, 1.0, NAN]) and cnt.tolist() == [4, 0, 3, 7] and cnt.dtype == np.int32
    sub = np.array([1e-45, -3e-45], np.float32)
    bh.same_bits(sub, sub.copy())
    bh.same_bits(np.array([0.0, NAN], np.float32), np.array([-0.0, -NAN], np.float32))          # a zero's sign, any NaN
    for a, b in (([1e-45], [0.0]), ([1e-45], [3e-45]), ([1.0], [np.nextafter(np.float32(1), np.float32(2))]), ([NAN], [INF])):
        with pytest.raises(AssertionError):
            bh.same_bits(np.array(a, np.float32), np.array(b, np.float32))
    with pytest.raises(AssertionError):
        bh.same_ints([1, 2], [1, 3])


def test_sets_f32_rounds_once_per_operation():
    rng = np.random.default_rng(2)
    q = (rng.random(6) * 3).astype(np.float32)
    qc = (rng.random((6, 40)) * 3).astype(np.float32)
    m = (0.5 + rng.random(40)).astype(np.float32)
    c = rng.standard_normal(40).astype(np.float32)
    cs = rng.standard_normal((5, 40)).astype(np.float32)
    d = np.float64
    for qq in (q, qc):
        q2 = (qq[:, None] if qq.ndim == 1 else qq).astype(d)
        for mm in (None, m):
            hw = (q2 * mm.astype(d)[None]).astype(np.float32).astype(d) if mm is not None else q2     # one rounding: the product
            lo, hi = bh.sets_f32(qq, mm, None)
            assert _eq(lo, np.broadcast_to((-hw).astype(np.float32), lo.shape)) and _eq(hi, np.broadcast_to(hw.astype(np.float32), hi.shape))
            lo, hi = bh.sets_f32(qq, mm, c)
            assert lo.shape == (6, 40)
            assert _eq(lo, (c.astype(d)[None] - hw).astype(np.float32)) and _eq(hi, (c.astype(d)[None] + hw).astype(np.float32))
            lo, hi = bh.sets_f32(qq, mm, cs)
            assert lo.shape == (6, 5, 40)
            assert _eq(lo, (cs.astype(d)[None] - hw[:, None]).astype(np.float32)) and _eq(hi, (cs.astype(d)[None] + hw[:, None]).astype(np.float32))
    # (fp64 sums of two fp32 numbers of this range round to fp32 as the exact sums do: 53 >= 2 * 24 + 2 bits)
    lo, hi = bh.sets_f32([INF, 0.0, -1.0, NAN], np.array([1.0, INF, 0.0], np.float32), np.array([INF, 0.0, 1.0], np.float32))
    assert np.isnan(lo[0, 0]) and hi[0, 0] == INF and np.isnan(lo[1, 1]) and lo[2, 2] == 1.0 and np.isnan(hi[3]).all()


# ------------------------------------------------------------------------------------------------ contraction cells
def _nearest_f32(x):
    """the fp32 number nearest to the Fraction x (ties to even), from exact comparisons"""
    g = np.float32(float(x))                                       # within an ulp or so: walk to the nearest from here
    while Fraction(float(g)) > x:
        g = np.nextafter(g, np.float32(-np.inf))
    while Fraction(float(np.nextafter(g, np.float32(np.inf)))) <= x:
        g = np.nextafter(g, np.float32(np.inf))
    up = np.nextafter(g, np.float32(np.inf))                       # g <= x < up
    dl, du = x - Fraction(float(g)), Fraction(float(up)) - x
    if dl != du:
        return g if dl < du else up
    return g if (g.view(np.int32) & 1) == 0 else up


def test_contraction_cells_differ_from_the_fused_result():
    cells = bh.contraction_cells()
    assert len(cells.plus) >= 8 and len(cells.minus) >= 8 and len(cells.product) >= 8
    for q, m, c in cells.plus:
        fused = _nearest_f32(Fraction(float(q)) * Fraction(float(m)) + Fraction(float(c)))
        assert fused == bh.fma_f32(q, m, c) and np.float32(c + np.float32(q * m)) != fused
    for q, m, c in cells.minus:
        fused = _nearest_f32(Fraction(float(c)) - Fraction(float(q)) * Fraction(float(m)))
        assert fused == bh.fma_f32(-q, m, c) and np.float32(c - np.float32(q * m)) != fused
    for q, m in cells.product:
        assert Fraction(float(np.float32(q * m))) != Fraction(float(q)) * Fraction(float(m))
    shared = bh.contraction_cells(q=np.float32(1.37))                                           # one q-hat for every cell
    assert all(len(part) >= 8 and (part[:, 0] == np.float32(1.37)).all() for part in shared)
    for q, m, c in shared.plus:
        assert np.float32(c + np.float32(q * m)) != _nearest_f32(Fraction(float(q)) * Fraction(float(m)) + Fraction(float(c)))
    for q, m, c in shared.minus:
        assert np.float32(c - np.float32(q * m)) != _nearest_f32(Fraction(float(c)) - Fraction(float(q)) * Fraction(float(m)))
    again = bh.contraction_cells()
    assert all(np.array_equal(a, b) for a, b in zip(cells, again))                             # seeded: the same cells every time


def test_fma_emulation_against_exact_arithmetic():
    rng = np.random.default_rng(3)
    q, m = (0.5 + 1.5 * rng.random(300)).astype(np.float32), (0.5 + 1.5 * rng.random(300)).astype(np.float32)
    c = (rng.standard_normal(300) * 4).astype(np.float32)
    got = bh.fma_f32(q, m, c)
    for i in range(300):
        assert got[i] == _nearest_f32(Fraction(float(q[i])) * Fraction(float(m[i])) + Fraction(float(c[i]))), i


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("shape", list(bh.TABLE) + list(bh.TABLE_MORE), ids=lambda s: f"{s[0]}x{s[1]}")
def test_plan_reaches_the_branch_its_row_claims(shape):
    p = bh.assert_plan(*shape)
    assert p.rows * p.W == 256 and (p.S - 1) * p.per + p.last == shape[0] and 0 < p.last <= p.per and p.P <= 4096


def test_rows_and_splits_without_a_sample_and_the_workspace_sizes():
    assert bh.plan(1, 1).rows == 4 and bh.plan(3, 64).rows == 4            # n < rows: rows 1..3 / row 3 stream nothing
    assert bh.plan(262145, 33).last < bh.plan(262145, 33).rows * 2         # 5 samples on 4 rows: one row with two, three with one
    assert bh.workspace_bytes(64, 129, 5, "cellwise") == 0                 # P == 1: none
    assert bh.workspace_bytes(64, 129, 5, "envelope") == 256               # the mask bits alone
    assert bh.workspace_bytes(4096, 64, 5, "envelope") == 16384 + 64 * 5 * 64 * 8
    assert bh.workspace_bytes(4097, 64, 5, "cellwise") == 68 * 5 * 64 * 12 + 2 * 5 * 64 * 12
    assert bh.workspace_bytes(300, 65, 33, "cellwise") == bh.workspace_bytes(300, 65, 16, "cellwise")
    assert bh.workspace_bytes(7, 3, 1, "envelope") == 256 + 256            # each part rounded up to 256 bytes


def test_mask_set_restates_the_kernel_s_classification():
    assert [bh.mask_set(m, 1) for m in (0, 1)] == [None, "A"]
    assert [bh.mask_set(m, 2) for m in (0, 1, 2, 3)] == [None, "D", "A", "A"]
    assert [bh.mask_set(m, 3) for m in range(8)] == [None, "D", "R", "D", "A", "R", "A", "A"]
    assert bh.mask_set(0xFFFF, 16) == "A" and bh.mask_set(0x7FFF, 16) == "D" and bh.mask_set(0x8001, 16) == "R"
    assert bh.mask_set(0x1FFFF, 16) == "A"                                 # (only the launch's 16 bits count)


# ------------------------------------------------------------------------------------------------ memory
def test_framed_and_cells():
    f = bh.framed(10, torch.float32, 1).set(np.arange(10, dtype=np.float32))
    assert f.untouched() and f.view.numel() == 10 and f.data_ptr() % 16 == 4 and torch.isnan(f.alloc[:f.lo]).all()
    f.alloc[f.hi] = 1.0
    assert not f.untouched()
    w = bh.framed(0, torch.uint8)
    assert w.untouched() and w.view.numel() == 0 and (w.data_ptr() - w.alloc.data_ptr()) % 256 == 0
    c = bh.framed(3, torch.int64, 2).set([1, 2, 3])
    c.view[1] = 7
    assert c.untouched() and c.data_ptr() % 8 == 0
    data = np.arange(2 * 24, dtype=np.float32).reshape(2, 24)
    cells = bh.Cells(data, **bh.split_of(24, 2))
    A, B, C = cells.ext
    sN, sA, sB = cells.strides
    assert A * B * C == 24 and min(A, B, C) > 1 and sB > C and sA > B * sB
    for j in range(24):
        a, b, x = j // (B * C), (j // C) % B, j % C
        assert cells.buf[1, a * sA + b * sB + x] == data[1, j]
    assert np.isnan(cells.buf).sum() == 2 * (sN - 24)
    assert bh.Cells(data, **bh.split_of(24, 1)).ext == (24, 1, 1) and bh.Cells(data, **bh.split_of(24, 0)).buf is data
    assert bh.factor3(257) is None and bh.factor3(65) == (1, 13, 5) and bh.split_of(257, 2) == dict(A=1, B=1, C=257)
