"""CPU tests of the references and checks of tests/dist_helpers.py (the histogram-exchange sweeps of
cp_pre_amd/csrc/dist_select.hip; tests/DIST_TESTS.md): the numpy references against the torch double ``DistOps`` and the
key functions of ``pipeline``, the properties of ``pipeline._dist_params`` / ``_dist_unpack``, the four sweeps together
(``simulate`` with ``DistOps``) against np.sort, and - sensitivity - one planted mistake per subclass of ``DistOps``, each
failing the check meant for it.  tests/test_gpu_dist_seams.py runs the same checks on the kernels."""
import os
import sys

import numpy as np
import pytest
import torch

from cp_pre_amd import pipeline

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dist_helpers as dh  # noqa: E402
from test_dist_histogram_cpu import DistOps  # noqa: E402

SIZES = (37, 300, 1800)
GRID = [(1, 37), (2, 150), (3, 129), (3, 600), (5, 409)]
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, 2.0 ** -149, -2.0 ** -149, 2.0 ** -127, 1.17549435e-38, -1.17549435e-38,
                    3.4028235e38, -3.4028235e38, 1.0, -1.0], np.float32)


def _params(win):
    return pipeline._dist_params(torch.from_numpy(np.ascontiguousarray(win)))


@pytest.fixture(scope="module", params=SIZES)
def fam(request):
    """(data [N, 20], its own window [3, 24] with four pads, params, nan, const, vconst)"""
    data = dh.family_columns(1, request.param, n0=request.param // 2)
    win = dh.window_ref(data, 24)
    return (data, win) + tuple(t.numpy() for t in _params(win))


# ================================================================================================ the references, pinned
def test_keys_equal_the_pipelines_and_invert(fam):
    x = np.concatenate([fam[0].reshape(-1), SPECIAL])
    x = x[~np.isnan(x)]
    k = dh.keys(x)
    assert k.dtype == np.int64 and k.min() >= 0 and k.max() < 1 << 32
    assert np.array_equal(k, pipeline._f2key(torch.from_numpy(x)).numpy())
    assert np.array_equal(dh.key2f(k).view(np.int32), x.view(np.int32))
    assert np.array_equal(pipeline._key2f(torch.from_numpy(k)).numpy().view(np.int32), x.view(np.int32))
    o = np.argsort(k, kind="stable")
    assert (x[o][1:] >= x[o][:-1]).all()                                  # ascending keys are ascending floats
    assert int(dh.keys(np.float32(-0.0))[0]) + 1 == int(dh.keys(np.float32(0.0))[0])     # two keys, one value


def test_window_ref_equals_the_double(fam):
    data, win = fam[0], fam[1]
    for kw, c0, C, W, Co in ((dict(), 0, 20, 1, 24), (dict(row_pad=3), 3, 17, 3, 7), (dict(planes=4, plane_pad=5), 2, 16, 2, 8),
                             (dict(), 0, 0, 2, 3)):
        S = dh.Source(data, **kw)
        got = dh.check_window(DistOps, S, c0, C, W, Co)
        if (c0, C, W * Co) == (0, 20, 24):
            assert np.array_equal(got, win)
    # the encodings themselves: MIN identities for the all-NaN column, the constant 0.0 for pads, the NaN flag
    i = dh.FAMILIES.index("all_nan")
    assert win[0, i] == np.int32(0x7FFFFFFF) and win[1, i] == np.int32(0x7FFFFFFF) and win[2, i] == 0
    assert (win[0, 20:] == 0).all() and (win[1, 20:] == -1).all() and (win[2, 20:] == 1).all()
    assert win[2, dh.FAMILIES.index("one_nan")] == 0 and win[2].sum() == 22
    lo = win[0].astype(np.int64) + (1 << 31)
    hi = 0xFFFFFFFF - (win[1].astype(np.int64) + (1 << 31))
    ok = ~np.isnan(data).all(0)
    assert np.array_equal(dh.key2f(lo[:20][ok]), np.nanmin(data[:, ok], 0))
    assert np.array_equal(dh.key2f(hi[:20][ok]), np.nanmax(data[:, ok], 0))


def test_bucket_ref_equals_the_doubles_map(fam):
    data, _, params = fam[0], fam[1], fam[2]
    b, part = dh.bucket_ref(data, params)
    bd, pd = DistOps._map(torch.from_numpy(data), torch.from_numpy(params), 0, 20)
    assert np.array_equal(part, pd.numpy())
    assert np.array_equal(b[:, part], bd.numpy()[:, part])


# ================================================================================================ pipeline._dist_params
def test_dist_params_properties(fam):
    data, win, params, nan, const, vconst = fam
    names = dh.FAMILIES
    lo = win[0].astype(np.int64) + (1 << 31)
    hi = 0xFFFFFFFF - (win[1].astype(np.int64) + (1 << 31))
    # NaN, constant and pad cells take no part
    excluded = {"constant", "one_nan", "all_nan"}
    for c in range(24):
        out = c >= 20 or names[c] in excluded
        assert (params[2, c] == -1) == out, c
        assert (params[2, c] >= 0) == (not out), c
    assert np.array_equal(np.flatnonzero(nan), [names.index("one_nan"), names.index("all_nan")])
    assert np.array_equal(np.flatnonzero(const), [names.index("constant")] + list(range(20, 24)))
    assert vconst[names.index("constant")] == np.float32(2.5) and (vconst[20:] == 0).all()
    # the map kind: value-linear exactly when window and scale are finite and positive (fp32, one operation each)
    part = np.flatnonzero(params[2, :20] >= 0)
    vlo, vhi = dh.key2f(lo[part]), dh.key2f(hi[part])
    with np.errstate(all="ignore"):
        span = vhi - vlo
        sf = np.float32(dh.NB) / span
    assert span.dtype == np.float32 and sf.dtype == np.float32
    lin = np.isfinite(vlo) & np.isfinite(vhi) & np.isfinite(sf) & (sf > 0)
    got_sf = np.ascontiguousarray(params[1, part]).view(np.float32)
    assert np.array_equal(got_sf > 0, lin)
    assert np.array_equal(got_sf[lin].view(np.int32), sf[lin].view(np.int32)) and (params[1, part][~lin] == 0).all()
    assert np.array_equal(params[0, :20], win[0, :20] ^ np.int32(-2 ** 31))                # klo's own bits
    key_linear = {names[c] for c in part[~lin]}
    assert key_linear == {"signed_zeros", "third_pinf", "quarter_ninf", "both_inf", "span_overflow", "subnormals",
                          "scale_overflow"}, key_linear
    # the shift: the least s with span >> s <= 255
    for c, l in zip(part, lin):
        s, d = int(params[2, c]), int(hi[c] - lo[c])
        if l:
            assert s == 0
        else:
            assert d >> s <= dh.NB - 1 and (s == 0 or d >> (s - 1) > dh.NB - 1), (c, s, d)
    # every in-window score lands in [0, 255] - the key-linear map before any clamp; the ends: bucket 0 and the last occupied
    b, _ = dh.bucket_ref(data, params)
    raw = (dh.keys(data) - lo[None, :20]) >> np.maximum(params[2, :20], 0).astype(np.int64)[None]
    for c, l in zip(part, lin):
        assert 0 <= b[:, c].min() and b[:, c].max() <= dh.NB - 1
        if not l:
            assert 0 <= raw[:, c].min() and raw[:, c].max() <= dh.NB - 1, c
        col = dh.keys(data[:, c])
        assert b[np.argmin(col), c] == 0 and b[np.argmax(col), c] == b[:, c].max(), c
        assert b[:, c].max() >= (1 if names[c] == "signed_zeros" else 2), c               # the window is spread over the buckets
        o = np.argsort(col, kind="stable")
        assert (np.diff(b[o, c]) >= 0).all(), c                                           # monotone in the key order


def test_dist_unpack_halves():
    vals = (0, 1, 32767)
    lo = np.array([[a for a in vals for _ in vals]] * 2, np.int64)                       # [2 cells, 9 words]
    hi = np.array([[b for _ in vals for b in vals]] * 2, np.int64)
    h = torch.from_numpy((lo | (hi << 16)).astype(np.int32).T.copy())                    # [words, Co]
    got = pipeline._dist_unpack(h, True).numpy()
    assert got.shape == (2, 18) and np.array_equal(got[:, :9], lo) and np.array_equal(got[:, 9:], hi)
    assert np.array_equal(dh.unpack_ref(h.numpy(), True), got)
    plain = torch.tensor([[0, 1], [32767, 65536], [2 ** 31 - 1, 5]], dtype=torch.int32)
    assert np.array_equal(pipeline._dist_unpack(plain, False).numpy(), plain.numpy().T)


# ================================================================================================ the checks on the double
SHAPES = [(dict(), 0, 100, 1, 100), (dict(row_pad=3), 5, 70, 3, 27), (dict(planes=4, plane_pad=5), 20, 60, 2, 40)]


@pytest.mark.parametrize("n", [37, 300])
def test_single_sweep_checks_pass_on_the_double(n):
    data = dh.cells(1, n)
    for kw, c0, C, W, Co in SHAPES:
        S = dh.Source(data, **kw)
        win = dh.check_window(DistOps, S, c0, C, W, Co)
        params = _params(win)[0].numpy()
        for packed in (True, False):
            counts = dh.check_hist(DistOps, S, c0, C, W, Co, params, packed)
        dh.check_partition(DistOps, S, c0, C, W, Co, params, counts)
        want = np.full((W * Co, 3), -1, np.int32)
        for c in range(C):
            occ = np.flatnonzero(counts[c])[-2:]
            want[c, :len(occ)] = occ
        dh.check_collect(DistOps, S, c0, C, W, Co, params, want)      # (a short cnt: the kernel only, the double asserts its counts)


@pytest.mark.parametrize("name", sorted(dh.pick_cases()))
def test_pick_check_passes_on_the_double(name):
    lists, asks, W, nk = dh.pick_cases()[name]
    dh.check_pick(DistOps, lists, asks, W, nk, cap=1 << 30)             # (the double holds a list of any length)


@pytest.mark.parametrize("plus", [0, 7])
@pytest.mark.parametrize("W,n_local", GRID)
def test_simulate_with_the_double_equals_numpy_sort(W, n_local, plus):
    data = dh.cells(W, n_local)
    N = W * n_local
    q, t = dh.check_simulate(DistOps, data, W, dh.ranks(N), -(-100 // W) + plus)
    assert q.shape == (len(dh.ranks(N)), 100) and t["longest"] <= dh.PICK_CAP and t["packed"]
    if (W, plus) == (3, 7):                                               # one int32 per bucket, and a run that starts inside
        dh.check_simulate(DistOps, data, W, dh.ranks(N), 40, c0=9, packed=False)


def test_narrow_ref_by_hand():
    counts = np.zeros((3, dh.NB), np.int64)
    counts[0, [3, 7, 255]] = (2, 3, 1)                                    # ranks 0,1 | 2,3,4 | 5
    counts[1, 9] = 6
    want, slot, rnk = dh.narrow_ref(counts, [5, 0, 2, 4, 1])
    assert want[0].tolist() == [3, 7, 255, -1, -1] and slot[0].tolist() == [2, 0, 1, 1, 0] and rnk[0].tolist() == [0, 0, 0, 2, 1]
    assert want[1].tolist() == [9, -1, -1, -1, -1] and slot[1].tolist() == [0] * 5 and rnk[1].tolist() == [5, 0, 2, 4, 1]
    assert (want[2] == -1).all() and (slot[2] == -1).all()


# ================================================================================================ sensitivity: planted mistakes
def _with_map(bad):
    """A DistOps whose histogram and collect sweeps see the map ``bad(bucket)``."""
    class Planted(DistOps):
        @staticmethod
        def _run(f, *a):
            good = DistOps.__dict__["_map"]

            def m(rows, params, c0, C):
                b, part = good.__func__(rows, params, c0, C)
                return torch.where(part, bad(b), b), part
            DistOps._map = staticmethod(m)
            try:
                f(*a)
            finally:
                DistOps._map = good

        @staticmethod
        def dist_hist(*a):
            Planted._run(DistOps.dist_hist, *a)

        @staticmethod
        def dist_collect(*a):
            Planted._run(DistOps.dist_collect, *a)
    return Planted


ShiftedUp = _with_map(lambda b: (b + 1).clamp_max(dh.NB - 1))
NotMonotone = _with_map(lambda b: torch.where(b == 10, 11, torch.where(b == 11, 10, b)))


class DropsLastRow(DistOps):
    @staticmethod
    def dist_collect(src, c0, C, W, Co, params, want, cnt, off, send):
        DistOps.dist_collect(src, c0, C, W, Co, params, want, cnt, off, send)
        rows = pipeline._dist_rows(src, c0, C)
        b, part = DistOps._map(rows, params, c0, C)
        for c in range(C):                             # the double fills a list in row order: the last row is its last entry
            hit = (want[c].long() == b[-1, c]).nonzero().view(-1)
            if part[c] and len(hit):
                s = int(hit[0])
                send[off[c, s] + cnt[c, s] - 1] = float("nan")


def _counting_pick(vals, cnt, off, slot, rnk, out, strict=False, first_only=False):
    """The kernel's pick by counting (less <= rank < less-or-equal), with the two planted mistakes."""
    W, Co, S = cnt.shape
    for co in range(Co):
        for j in range(slot.shape[1]):
            s, r = int(slot[co, j]), int(rnk[co, j])
            if s < 0:
                continue
            k = dh.keys(np.concatenate([vals[int(off[w, co, s]):int(off[w, co, s]) + int(cnt[w, co, s])].numpy()
                                        for w in range(1 if first_only else W)]))
            for e in k:
                less = int((k < e).sum())
                leq = less + 1 if strict else int((k <= e).sum())
                if less <= r < leq:
                    out[j, co] = float(dh.key2f(e))


class StrictPick(DistOps):
    dist_pick = staticmethod(lambda *a: _counting_pick(*a, strict=True))


class FirstSegmentPick(DistOps):
    dist_pick = staticmethod(lambda *a: _counting_pick(*a, first_only=True))


class ForgetsPads(DistOps):
    @staticmethod
    def dist_hist(src, c0, C, W, Co, params, packed, hist):
        full = torch.empty_like(hist)
        DistOps.dist_hist(src, c0, C, W, Co, params, packed, full)
        flat, keep = hist.permute(0, 2, 1).reshape(W * Co, -1), full.permute(0, 2, 1).reshape(W * Co, -1)
        flat[:C] = keep[:C]
        hist.copy_(flat.view(W, Co, -1).permute(0, 2, 1))


@pytest.fixture(scope="module")
def planted_case():
    S = dh.Source(dh.cells(1, 1800, 40))
    c0, C, W, Co = 0, 40, 2, 23                                          # six pads
    params = _params(dh.window_ref(S.rows(c0, C), W * Co))[0].numpy()
    b, part = dh.bucket_ref(S.rows(c0, C), params)
    counts = np.zeros((W * Co, dh.NB), np.int64)
    for c in np.flatnonzero(part):
        counts[c] = np.bincount(b[:, c], minlength=dh.NB)
    return S, (c0, C, W, Co), params, counts


def _counts_of(ops, S, shape, params):
    c0, C, W, Co = shape
    h = torch.zeros(W, dh.NB, Co, dtype=torch.int32)
    ops.dist_hist(S.src, c0, C, W, Co, torch.from_numpy(params), False, h)
    return np.concatenate([dh.unpack_ref(h.numpy()[r], False) for r in range(W)], 0)


def test_the_unplanted_double_passes_every_check_used_below(planted_case):
    S, shape, params, counts = planted_case
    assert np.array_equal(dh.check_hist(DistOps, S, *shape, params, False), counts)
    dh.check_partition(DistOps, S, *shape, params, counts)
    lists, asks, W, nk = dh.pick_cases()["ties"]
    dh.check_pick(DistOps, lists, asks, W, nk)

    class Counting(DistOps):
        dist_pick = staticmethod(_counting_pick)
    dh.check_pick(Counting, lists, asks, W, nk)                           # the counting form itself is right without a plant


def test_planted_map_shifted_up_fails_the_histogram_comparison(planted_case):
    S, shape, params, _ = planted_case
    with pytest.raises(AssertionError, match="not bucket_ref"):         # the comparison with bucket_ref + bincount
        dh.check_hist(ShiftedUp, S, *shape, params, False)
    with pytest.raises(AssertionError, match="not bucket_ref"):
        dh.check_hist(ShiftedUp, S, *shape, params, True)
    # ... and is invisible to the partition property, which does not restate the map: hence both checks
    dh.check_partition(ShiftedUp, S, *shape, params, _counts_of(ShiftedUp, S, shape, params))


def test_planted_map_not_monotone_fails_the_partition_property(planted_case):
    S, shape, params, counts = planted_case
    own = _counts_of(NotMonotone, S, shape, params)                        # its own counts: histogram and collect agree
    assert (own[:, 10] > 0).any() and (own[:, 11] > 0).any() and not np.array_equal(own, counts)
    with pytest.raises(AssertionError, match="not the sorted column"):
        dh.check_partition(NotMonotone, S, *shape, params, own)


def test_planted_collect_dropping_the_last_row_fails_partition_and_simulate(planted_case):
    S, shape, params, counts = planted_case
    with pytest.raises(AssertionError, match="never written"):
        dh.check_partition(DropsLastRow, S, *shape, params, counts)
    data = dh.cells(2, 150, 20)
    with pytest.raises(AssertionError):
        dh.check_simulate(DropsLastRow, data, 2, list(range(0, 300, 7)) + [299], 10)


def test_planted_strict_pick_fails_under_ties():
    lists, asks, W, nk = dh.pick_cases()["ties"]
    with pytest.raises(AssertionError):
        dh.check_pick(StrictPick, lists, asks, W, nk)
    lists, asks, W, nk = dh.pick_cases()["one"]                           # (without ties it is right)
    dh.check_pick(StrictPick, lists, asks, W, nk)
    with pytest.raises(AssertionError):
        dh.check_simulate(StrictPick, dh.cells(2, 150, 20), 2, dh.ranks(300), 10)


def test_planted_first_segment_pick_fails_with_several_segments():
    for name in ("ties", "wide"):
        lists, asks, W, nk = dh.pick_cases()[name]
        with pytest.raises(AssertionError):
            dh.check_pick(FirstSegmentPick, lists, asks, W, nk)
    with pytest.raises(AssertionError):
        dh.check_simulate(FirstSegmentPick, dh.cells(2, 150, 20), 2, dh.ranks(300), 10)
    dh.check_simulate(FirstSegmentPick, dh.cells(1, 37, 20), 1, dh.ranks(37), 20)          # (one segment: right)


def test_planted_hist_forgetting_pads_fails_the_zero_check(planted_case):
    S, shape, params, _ = planted_case
    for packed in (False, True):
        with pytest.raises(AssertionError, match="takes no part"):
            dh.check_hist(ForgetsPads, S, *shape, params, packed)
