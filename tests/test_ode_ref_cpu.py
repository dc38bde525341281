"""CPU tests of tests/ode_helpers.py, before anything of it judges a kernel: the references against F.conv1d in float64,
against the reference-executed goldens and against integer loops written out by hand, the exactness conditions, the launch
plans of tests/ODE_TESTS.md row by row, and the memory helpers."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ode_helpers as oh
from cp_pre_amd import ode
from cp_pre_amd.convops_0d import ConvOperator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "convops_0d.npz"))


def conv1d64(x, taps):
    xd, k = torch.as_tensor(np.asarray(x, np.float64)), torch.as_tensor(np.asarray(taps, np.float64))
    return F.conv1d(xd[:, None], k[None, None], padding=len(taps) // 2)[:, 0].numpy()


@pytest.mark.parametrize("k", (1, 3, 5, 7))
@pytest.mark.parametrize("bs,nt", [(1, 1), (3, 2), (2, 3), (5, 7), (4, 33)])
def test_conv_ref_is_conv1d_in_float64(bs, nt, k):
    rng = np.random.default_rng(bs * 100 + nt * 10 + k)
    x, taps = rng.standard_normal((bs, nt)), rng.standard_normal(k)
    want = conv1d64(x, taps)
    got = oh.conv_ref(x, taps)
    mag = oh.conv_ref(np.abs(x), np.abs(taps))
    assert np.all(np.abs(got - want) <= 2 * k * oh.U53 * mag)
    xi, ti = oh.ints(rng, -8, 8, bs, nt), oh.int_taps(rng, k, nonzero=False)
    assert np.array_equal(oh.conv_ref(xi, ti, np.int64), conv1d64(xi, ti))       # integers: exact either way
    assert np.array_equal(oh.conv_ref(xi, ti, np.int64), oh.conv_ref(xi, ti))


def test_conv_ref_against_a_loop_written_out():
    rng = np.random.default_rng(1)
    for k in (1, 3, 5, 7):
        for nt in (1, 2, 3, 6):
            x, taps = rng.integers(-8, 9, (3, nt)), rng.integers(-3, 4, k)
            want = np.zeros((3, nt), np.int64)
            for b in range(3):
                for t in range(nt):
                    for j in range(k):
                        u = t + j - k // 2
                        if 0 <= u < nt:
                            want[b, t] += taps[j] * x[b, u]
            assert np.array_equal(oh.conv_ref(x, taps, np.int64), want), (k, nt)


def test_conv_ref_against_the_goldens():
    for nt in (1, 2, 3, 7, 100, 150):
        x = G[f"x_nt{nt}"]
        for k, (d, t) in {3: (2, 2), 5: (2, 4), 7: (2, 6)}.items():
            taps = ConvOperator(order=d, taylor_order=t, scale=0.7).kernel.numpy()
            assert taps.size == k
            term = [(x, taps, None)]
            oh.within(G[f"conv_nt{nt}_k{k}"], oh.residual_ref(term), oh.residual_tol(term))    # the golden ran in fp32


def test_residual_ref_against_the_golden_script_residual():
    sol = G["dho_sol"][None]                                   # [1, Nt, 2]
    m, c, k = (float(v) for v in G["dho_mck"])
    op = ode.DHO(m, c, k, float(G["dho_dt"]), split=True)
    terms = [(sol[..., comp], taps, None if cf is None else cf.numpy()) for comp, _, taps, cf in op.terms]
    oh.within(G["dho_split"], oh.residual_ref(terms), oh.residual_tol(terms))


def test_nonfinite_values_spread_as_in_conv1d():
    x = np.zeros((4, 9))
    x[0, 0], x[1, 8], x[2, 4], x[3, 3] = np.nan, np.inf, -np.inf, np.inf
    x[3, 5] = -np.inf
    for taps in ([0.0, 1.0, 0.0], [1.0, -2.0, 1.0], [2.0], [1.0, 0.0, -1.0, 0.0, 2.0]):
        with np.errstate(invalid="ignore"):
            want = conv1d64(x, taps)
        assert np.array_equal(oh.footprint(oh.conv_ref(x, taps)), oh.footprint(want)), taps
    assert oh.footprint(np.array([1.0, np.nan, np.inf, -np.inf])).tolist() == [0, 1, 2, 3]


def test_exactness_conditions_hold_and_fail_where_they_should():
    rng = np.random.default_rng(2)
    worst = [(np.full((2, 9), 8.0), np.full(7, 3.0), np.full(9, 4.0))] * 6
    oh.assert_exact_f32(worst)
    assert oh.magnitude(worst).max() == 6 * 4 * 7 * 3 * 8 == 4032
    with pytest.raises(AssertionError):
        oh.assert_exact_f32([(np.full((1, 3), 2.0 ** 22), np.full(3, 3.0), None)])
    with pytest.raises(AssertionError, match="integer"):
        oh.assert_exact_f32([(np.full((1, 3), 0.5), np.ones(3), None)])
    x, g = oh.ints(rng, -4, 4, 2405, 109), oh.ints(rng, -4, 4, 2405, 109)
    oh.assert_exact_wgrad(x, g, 7)
    assert 16 * oh.LARGEST < 2 ** 24
    with pytest.raises(AssertionError):
        oh.assert_exact_wgrad(np.full((1, 1 << 21), 4.0), np.full((1, 1 << 21), 4.0), 1)
    # integer data in fp32, summed in another order and with fma, give the same number: what "exact" buys
    terms = [(oh.ints(rng, -8, 8, 3, 11), oh.int_taps(rng, 7), oh.coeff_row(11)) for _ in range(6)]
    oh.assert_exact_f32(terms)
    # (the mirrored problem, terms last to first, in fp32: taps and steps are then summed in the opposite order)
    mirrored = oh.residual_ref([(x[:, ::-1], t[::-1], c[::-1]) for x, t, c in terms[::-1]], np.float32)
    assert mirrored.dtype == np.float32 and np.array_equal(mirrored[:, ::-1], oh.residual_ref(terms, np.int64))


def test_wgrad_ref_against_a_loop_and_autograd():
    rng = np.random.default_rng(3)
    for k in (1, 3, 5, 7):
        for bs, nt in ((1, 1), (3, 2), (2, 7), (4, 9)):
            x, g = rng.integers(-4, 5, (bs, nt)), rng.integers(-4, 5, (bs, nt))
            want = np.zeros(k, np.int64)
            for j in range(k):
                for b in range(bs):
                    for t in range(nt):
                        u = t + j - k // 2
                        if 0 <= u < nt:
                            want[j] += g[b, t] * x[b, u]
            assert np.array_equal(oh.wgrad_ref(x, g, k, np.int64), want), (k, bs, nt)
            kr = torch.zeros(k, dtype=torch.float64, requires_grad=True)
            F.conv1d(torch.as_tensor(x, dtype=torch.float64)[:, None], kr[None, None], padding=k // 2)[:, 0].backward(
                torch.as_tensor(g, dtype=torch.float64))
            assert np.array_equal(kr.grad.numpy(), want)


@pytest.mark.parametrize("shape", sorted(oh.TABLE))
def test_residual_plan_rows(shape):
    p = oh.assert_plan(*shape)
    assert p.total <= oh.LARGEST and p.threads == -(-p.total // 4) and 1 <= p.last_run <= 4


def test_residual_table_covers_what_the_issue_lists():
    plans = {s: oh.plan(*s) for s in oh.TABLE}
    totals = {p.total for p in plans.values()}
    assert {1, 3, 4, 5, 1023, 1024, 1025, 2049} <= totals
    assert {nt for _, nt in plans} >= {1, 2, 3, 4, 5, 6, 7, 8, 1023}
    assert {p.total % 4 for p in plans.values()} == {0, 1, 2, 3}
    for nt in (5, 6, 7):                                       # between them a crossing at each v
        assert any(s[1] == nt and p.cross_v for s, p in plans.items())
    assert {v for s, p in plans.items() if s[1] in (5, 6, 7) for v in p.cross_v} == {1, 2, 3}
    assert all(p.cross_v == () for s, p in plans.items() if s[1] in (4, 8))
    assert max(p.multi for s, p in plans.items() if s[1] in (1, 2, 3)) == 3


@pytest.mark.parametrize("shape", sorted(oh.WGRAD_TABLE))
def test_wgrad_plan_rows(shape):
    p = oh.assert_wgrad_plan(*shape)
    assert p.total <= oh.LARGEST
    assert p.nonempty <= oh.WGRAD_BLOCKS and (p.nonempty - 1) * p.per < p.total <= p.nonempty * p.per


def test_wgrad_plan_edges():
    assert oh.wgrad_plan(0, 5) == oh.WgPlan(0, 0, 0, False, False) and oh.wgrad_plan(5, 0).per == 0
    assert oh.wgrad_plan(1025, 1).nonempty == 513              # half the blocks are empty
    assert not oh.wgrad_plan(1024 * 256, 1).second and oh.wgrad_plan(1024 * 256 + 1, 1).second


def test_layouts_stay_inside_their_buffers_and_carry_nan_elsewhere():
    rng = np.random.default_rng(4)
    for kind in ("dense", "padded", "pitch3", "comp20", "comp31", "transposed", "negB", "negT", "negBT", "zeroB"):
        for bs, nt in ((1, 1), (3, 5), (4, 1), (1, 6)):
            data = oh.ints(rng, -8, 8, bs, nt)
            lead = int(kind[5]) if kind.startswith("comp") else 0
            s = oh.Source(data, kind, lead=lead)
            off = oh.offsets(bs, nt, *s.strides) + s.origin
            assert off.min() >= 0 and off.max() < s.host.size, kind
            assert np.array_equal(s.host[off], s.data), kind
            seen = np.zeros(s.host.size, bool)
            seen[off] = True
            assert np.isnan(s.host[~seen]).all() and not np.isnan(s.host[seen]).any(), kind
            if kind != "zeroB":
                assert np.unique(off).size == off.size, kind
                f = oh.Framed(oh.offsets(bs, nt, *s.strides), offset=1)
                assert f.untouched() and f.all_nan_bits()
                f.set(data)
                assert f.untouched() and not f.all_nan_bits() and np.array_equal(f.get().reshape(bs, nt), data)
                f.alloc[int(f.idx.min()) - 1 if kind in ("dense", "negB", "negT") else 0] = 1.0
                assert not f.untouched()
    with pytest.raises(AssertionError, match="overlaps"):
        oh.Framed(oh.offsets(4, 16, 8, 1))


def test_coefficient_rows_differ_within_any_run():
    c = oh.coeff_row(1023)
    assert np.all(c != 0) and np.abs(c).max() <= 4
    for d in (1, 2, 3):
        assert np.all(c[d:] != c[:-d])
