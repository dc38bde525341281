"""GPU tests (pytest -m gpu) of the sample-acceptance bounds kernels of cp_pre_amd/csrc/sample_bounds.hip at their seams:
called through the C ABI (``_lib.load_bounds().pre_bounds_*``) at shapes on both sides of every branch of the launch plan,
with mixed mask kinds, more than 16 levels, special values, cells where fma contraction would show, prior contents of the
outputs, pitches and a workspace of exactly the queried size, and, last, through ``sample_bounds`` on layouts whose operands
disagree - against the plain numpy references of tests/bounds_helpers.py (checked on the CPU by
tests/test_bounds_ref_cpu.py).  Every output and the workspace lie inside a larger allocation of the test's filled with NaN
or a bit pattern, which must be unchanged after each call; results are compared bit for bit (any NaN equals any NaN, a zero
may carry either sign).  tests/BOUNDS_TESTS.md says which branch each shape reaches."""
import ctypes

import numpy as np
import pytest
import torch

import bounds_helpers as bh

pytestmark = pytest.mark.gpu

NAN, INF = np.float32(np.nan), np.float32(np.inf)
PRE_E_NULL, PRE_E_SHAPE = -1, -2
DEV = "cuda:0"
I32, I64, F32, U8 = torch.int32, torch.int64, torch.float32, torch.uint8


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    from cp_pre_amd import _lib
    _lib.load_bounds()
    return torch.device(DEV)


def _L():
    from cp_pre_amd import _lib
    return _lib, _lib.load_bounds()


def dev(x):
    return torch.from_numpy(np.require(x, requirements="CW")).to(DEV) if x is not None else None


def P(x):
    if x is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p(x.data_ptr())


def host(f, *shape):
    return f.view.cpu().numpy().reshape(*shape)


def normal(rng, *shape):
    return rng.standard_normal(shape, dtype=np.float32)


def query(entry, n, ext, nk):
    """the workspace size the library reports, which must be the one the restated plan gives"""
    _lib, lib = _L()
    b = ctypes.c_int64(-1)
    fn = lib.pre_bounds_envelope_workspace if entry == "envelope" else lib.pre_bounds_cellwise_workspace
    assert fn(n, ext[0], ext[1], ext[2], nk, ctypes.byref(b)) == 0
    assert b.value == bh.workspace_bytes(n, ext[0] * ext[1] * ext[2], nk, entry), (entry, n, ext, nk, b.value)
    return b.value


# ================================================================================================ the three entry points
def envelope(cells, acc, prior=None, accept_ld=None, off=0, times=1):
    """pre_bounds_envelope_f32 on framed outputs that start from ``prior`` (default +inf, -inf, 0) and a framed workspace of
    exactly the queried size; ``times`` calls into the same outputs.  Returns [(lo, hi, count)] after each call."""
    _lib, lib = _L()
    n, M, nk = cells.n, cells.M, acc.shape[0]
    ld = n if accept_ld is None else accept_ld
    a = np.ones((nk, ld), np.uint8)                                # (beyond n: accepting, so that a wrong pitch shows)
    a[:, :n] = acc
    if prior is None:
        prior = (np.full((nk, M), INF), np.full((nk, M), -INF), np.zeros(nk, np.int64))
    lo, hi = bh.framed(nk * M, F32, off, DEV).set(prior[0]), bh.framed(nk * M, F32, off, DEV).set(prior[1])
    cnt = bh.framed(nk, I64, 0, DEV).set(prior[2])
    wb = query("envelope", n, cells.ext, nk)
    work = bh.framed(wb, U8, 4 * off, DEV)
    ud, ad = dev(cells.buf), dev(a)
    sN, sA, sB = cells.strides
    out = []
    for _ in range(times):
        rc = lib.pre_bounds_envelope_f32(P(ud), sN, sA, sB, n, *cells.ext, P(ad), ld, nk, P(lo), P(hi), P(cnt), P(work), wb,
                                         _lib.stream())
        torch.cuda.synchronize()
        assert rc == 0 and lo.untouched() and hi.untouched() and cnt.untouched() and work.untouched()
        out.append((host(lo, nk, M), host(hi, nk, M), host(cnt, nk)))
    return out


def check_envelope(cells, acc, prior=None, **kw):
    got = envelope(cells, acc, prior, **kw)[0]
    want = bh.envelope_ref(cells.data, acc)
    if prior is not None:
        want = bh.merge_ref(want, prior)
    bh.same_bits(got[0], want[0])
    bh.same_bits(got[1], want[1])
    bh.same_ints(got[2], want[2])
    return want


def cellwise(uc, rc_, nk, q=None, m=None, c=None, blo=None, bhi=None, prior=None, off=0, times=1):
    """pre_bounds_cellwise_f32; ``q`` [nk] or [nk, q_ld >= M]; outputs and workspace as in ``envelope`` (a shape that needs
    no workspace gets a null pointer and 0 bytes)."""
    _lib, lib = _L()
    n, M = uc.n, uc.M
    assert rc_.ext == uc.ext and rc_.n == n
    if prior is None:
        prior = (np.full((nk, M), INF), np.full((nk, M), -INF), np.zeros((nk, M), np.int32))
    lo, hi = bh.framed(nk * M, F32, off, DEV).set(prior[0]), bh.framed(nk * M, F32, off, DEV).set(prior[1])
    cnt = bh.framed(nk * M, I32, off, DEV).set(prior[2])
    wb = query("cellwise", n, uc.ext, nk)
    assert (wb == 0) == (bh.plan(n, M).P == 1)
    work = bh.framed(wb, U8, 4 * off, DEV) if wb else None
    ud, rd = dev(uc.buf), (dev(rc_.buf) if rc_ is not uc else None)
    rd = ud if rd is None else rd
    q_ld = 0 if q is None or np.ndim(q) == 1 else np.shape(q)[1]
    qd, md, cd, bl, bh_ = dev(bh.f32(q) if q is not None else None), dev(m), dev(c), dev(blo), dev(bhi)
    out = []
    for _ in range(times):
        rc = lib.pre_bounds_cellwise_f32(P(ud), *uc.strides, P(rd), *rc_.strides, n, *uc.ext, P(qd), q_ld, P(md), P(cd), P(bl),
                                         P(bh_), nk, P(lo), P(hi), P(cnt), P(work), wb, _lib.stream())
        torch.cuda.synchronize()
        assert rc == 0 and lo.untouched() and hi.untouched() and cnt.untouched() and (work is None or work.untouched())
        out.append((host(lo, nk, M), host(hi, nk, M), host(cnt, nk, M)))
    return out


def check_cellwise(uc, rc_, q=None, m=None, c=None, given=False, prior=None, **kw):
    """``given``: the bounds of (q, m, c) are handed over as blo / bhi outright"""
    M = uc.M
    q2 = None if q is None else (bh.f32(q) if np.ndim(q) == 1 else bh.f32(q)[:, :M])
    blo, bhi = bh.sets_f32(q2, m, c)
    nk = blo.shape[0]
    blo, bhi = np.broadcast_to(blo, (nk, M)), np.broadcast_to(bhi, (nk, M))
    if given:
        got = cellwise(uc, rc_, nk, blo=np.ascontiguousarray(blo), bhi=np.ascontiguousarray(bhi), prior=prior, **kw)[0]
    else:
        got = cellwise(uc, rc_, nk, q=q, m=m, c=c, prior=prior, **kw)[0]
    want = bh.cellwise_ref(uc.data, rc_.data, blo, bhi)
    if prior is not None:
        want = bh.merge_ref(want, prior)
    bh.same_bits(got[0], want[0])
    bh.same_bits(got[1], want[1])
    bh.same_ints(got[2], want[2])
    return want


def rowcount(rc_, nk, q, m=None, c=None, counts_ld=None, prior=None):
    """pre_bounds_rowcount_f32; ``c``: None, fp32 [M] (per cell: sample stride 0, dense) or Cells (per sample).  ``counts``
    [nk, counts_ld] framed, starting from ``prior`` [nk, counts_ld]; the columns beyond n must come back as they were."""
    _lib, lib = _L()
    n, M = rc_.n, rc_.M
    A, B, C = rc_.ext
    ld = n if counts_ld is None else counts_ld
    prior = np.zeros((nk, ld), np.int32) if prior is None else prior
    counts = bh.framed(nk * ld, I32, 1, DEV).set(prior)
    rd = dev(rc_.buf)
    if c is None:
        cd, cs = None, (0, 0, 0)
    elif isinstance(c, bh.Cells):
        assert c.ext == rc_.ext
        cd, cs = dev(c.buf), c.strides
    else:
        cd, cs = dev(bh.f32(c)), (0, B * C, C)
    q_ld = 0 if np.ndim(q) == 1 else np.shape(q)[1]
    qd, md = dev(bh.f32(q)), dev(m)
    rc = lib.pre_bounds_rowcount_f32(P(rd), *rc_.strides, P(cd), *cs, n, A, B, C, P(qd), q_ld, P(md), nk, P(counts), ld, _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and counts.untouched()
    got = host(counts, nk, ld)
    assert np.array_equal(got[:, n:], prior[:, n:])
    return got[:, :n].astype(np.int64) - prior[:, :n]


def check_rowcount(rc_, q, m=None, c=None, **kw):
    M = rc_.M
    q2 = bh.f32(q) if np.ndim(q) == 1 else bh.f32(q)[:, :M]
    blo, bhi = bh.sets_f32(q2, m, c.data if isinstance(c, bh.Cells) else c)
    nk = blo.shape[0]
    if blo.ndim == 2:
        blo, bhi = np.broadcast_to(blo, (nk, M)), np.broadcast_to(bhi, (nk, M))
    got = rowcount(rc_, nk, q, m, c, **kw)
    want = bh.rowcount_ref(rc_.data, blo, bhi)
    bh.same_ints(got, want)
    return want


# ================================================================================================ the plan's edges
ROWS = list(bh.TABLE)
Q5 = np.array([0.2, 0.5, 1.0, 1.5, 3.0], np.float32)


def _table_cells(i, rng, n, M):
    return bh.Cells(normal(rng, n, M), **bh.split_of(M, i % 3))


@pytest.mark.parametrize("i", range(len(ROWS)), ids=[f"{n}x{M}" for n, M in ROWS])
def test_envelope_at_every_edge_of_the_plan(gpu, i):
    """random masks at nk = 5; the (A, B, C) split rotates over the rows: one dense row, (M, 1, 1), a cropped three-axis view"""
    n, M = ROWS[i]
    bh.assert_plan(n, M)
    rng = np.random.default_rng(100 + i)
    cells = _table_cells(i, rng, n, M)
    acc = rng.random((5, n)) < 0.4
    if n > 3:
        cells.data[n - 1, M // 2] = NAN                            # in the last (short) split, accepted at level 0 only
        cells.buf[n - 1, cells.idx[M // 2]] = NAN
        acc[:, n - 1] = (True, False, False, False, False)
        acc[3] = False                                             # a level that accepts nothing
    want = check_envelope(cells, acc, off=i % 2)
    assert n <= 3 or (np.isnan(want[0][0, M // 2]) and np.isnan(want[0]).sum() == 1 and (want[0][3] == INF).all())


@pytest.mark.parametrize("i", range(len(ROWS)), ids=[f"{n}x{M}" for n, M in ROWS])
def test_cellwise_at_every_edge_of_the_plan(gpu, i):
    """scalar q at nk = 5 without a centre (|r| <= hw); P == 1 rows write straight into lo / hi / count with no workspace"""
    n, M = ROWS[i]
    p = bh.assert_plan(n, M)
    rng = np.random.default_rng(200 + i)
    uc = _table_cells(i, rng, n, M)
    rc_ = bh.Cells(normal(rng, n, M), *uc.ext)                     # u and r share A, B, C; r is dense where u is cropped
    if n > 3:
        for cc, s, j in ((uc, n - 1, M // 2), (rc_, n - 2, 0)):    # NaN in u (inside: r = 0) and NaN in r (outside)
            cc.data[s, j] = NAN
            cc.buf[s, cc.idx[j]] = NAN
        rc_.data[n - 1, M // 2] = 0.0
        rc_.buf[n - 1, rc_.idx[M // 2]] = 0.0
    want = check_cellwise(uc, rc_, q=Q5, off=i % 2)
    assert n <= 3 or np.isnan(want[0][:, M // 2]).all()
    assert (p.P == 1) == (p.folds == 0)


def test_envelope_at_the_most_partials_the_fold_holds(gpu):
    """(262144, 64), nk = 3: S = 1024 splits x 4 rows = 4096 partials, folded 64 x 64"""
    n, M = bh.LARGE_ENVELOPE
    bh.assert_plan(n, M)
    rng = np.random.default_rng(7)
    cells = bh.Cells(normal(rng, n, M))
    acc = rng.random((3, n)) < np.array([[0.5], [0.001], [0.0]])   # half, a few per split at most, none
    cells.data[n - 1, 5] = NAN
    acc[:, n - 1] = (False, True, False)
    want = check_envelope(cells, acc)
    assert np.isnan(want[0][1, 5]) and np.isnan(want[0]).sum() == 1


def test_cellwise_counts_through_two_fold_levels(gpu):
    """(262145, 33), nk = 2: P = 4084, the last split has 5 samples; the counts are summed over both fold levels"""
    n, M = bh.LARGE_CELLWISE
    bh.assert_plan(n, M)
    rng = np.random.default_rng(8)
    uc, rc_ = bh.Cells(normal(rng, n, M)), bh.Cells(normal(rng, n, M))
    for s in range(n - 5, n):                                      # the last split alone decides the maximum of cell s % 33
        uc.data[s, s % M], rc_.data[s, s % M] = 100.0 + s % M, 0.0
    want = check_cellwise(uc, rc_, q=np.array([0.7, 1e-3], np.float32))
    assert want[2][0].min() > 100000 and (want[1][1, [(n - 1) % M, (n - 5) % M]] >= 100).all()


# ================================================================================================ more than 16 levels
@pytest.mark.parametrize("nk", [1, 16, 17, 32, 33])
def test_levels_beyond_one_launch_in_all_three_entry_points(gpu, nk):
    """the k0 loop: accept, q (scalar: q + k0; per cell: q + k0 * q_ld), blo / bhi, lo / hi / count(s) offset per launch of
    16 levels, the workspace reused; accept_ld = n + 5, counts_ld = n + 3, every level different from every other"""
    n, M = bh.LEVELS_SHAPE
    bh.assert_plan(n, M)
    rng = np.random.default_rng(nk)
    uc = bh.Cells(normal(rng, n, M), **bh.split_of(M, 2))
    rc_ = bh.Cells(normal(rng, n, M), **bh.split_of(M, 2))
    check_envelope(uc, rng.random((nk, n)) < np.linspace(0.05, 0.9, nk)[:, None], accept_ld=n + 5)
    q = np.linspace(0.05, 2.5, nk).astype(np.float32)
    qc = (q[:, None] * (0.5 + rng.random((nk, M)))).astype(np.float32)
    m = (0.5 + rng.random(M)).astype(np.float32)
    c = (0.3 * normal(rng, M)).astype(np.float32)
    cs = bh.Cells(0.3 * normal(rng, n, M), *rc_.ext)               # the per-sample centre dense, the residual cropped
    for qq, mm, cc in ((q, None, None), (q, m, c), (qc, None, None), (qc, m, c)):
        want = check_cellwise(uc, rc_, q=qq, m=mm, c=cc)
        assert len({want[2][k].tobytes() for k in range(nk)}) == nk           # no two levels count alike
        counts = check_rowcount(rc_, qq, mm, cc, counts_ld=n + 3, prior=rng.integers(0, 9, (nk, n + 3)).astype(np.int32))
        bh.same_ints(counts.sum(1), want[2].astype(np.int64).sum(1))          # per level: the same cells, summed the other way
        check_rowcount(rc_, qq, mm, cs, counts_ld=n + 3)
    check_cellwise(uc, rc_, q=qc, m=m, c=c, given=True)


def _sets(q, m, c, M):
    blo, bhi = bh.sets_f32(q, m, c)
    return np.broadcast_to(blo, (blo.shape[0], M)), np.broadcast_to(bhi, (bhi.shape[0], M))


# ================================================================================================ mask kinds
KINDS = ("grow", "shrink", "arbitrary", "full", "empty", "top", "bottom")


def _kind_masks(rng, n, nk):
    """bool [nk, n]: every sample draws its kind"""
    acc = np.zeros((nk, n), bool)
    lev = np.arange(nk)
    for s in range(n):
        kind = KINDS[rng.integers(len(KINDS))]
        if kind == "grow":
            acc[:, s] = lev >= rng.integers(0, nk)
        elif kind == "shrink":
            acc[:, s] = lev <= rng.integers(0, nk)
        elif kind == "arbitrary":
            acc[:, s] = rng.random(nk) < 0.5
        elif kind == "full":
            acc[:, s] = True
        elif kind == "top":
            acc[nk - 1, s] = True
        elif kind == "bottom":
            acc[0, s] = True
    return acc


def _plant(acc, u, nk):
    """Samples 0 .. 6 nk - 1 are planted: for level k (launch L = k // 16 of NK levels, kk = k % 16 within it), each register
    set X of the kernel (A: a run to the launch's last level; D: a run from level 0 that stops short of it; R: anything else)
    that can accept level kk gets two samples whose masks put them into X in that launch, one with the lowest and one with
    the highest value of all at cell 3 kk + x.  A's run starts one level BEFORE k and D's ends one level AFTER it where there
    is one, so that the value reaches level k through the epilogue's forward / backward fold alone."""
    M = u.shape[1]
    s = 0
    for k in range(nk):
        k0 = k - k % bh.MAX_LEVELS
        NK = min(bh.MAX_LEVELS, nk - k0)
        kk = k - k0
        masks = {"A": np.arange(nk) >= max(k - 1, k0)}
        if kk < NK - 1:
            masks["D"] = np.arange(nk) <= min(k + 1, k0 + NK - 2)
        if NK >= 3:
            other = {0: 2}.get(kk, kk - 2 if kk == NK - 1 else None)
            masks["R"] = np.isin(np.arange(nk), [k] + ([k0 + other] if other is not None else []))
        for x, name in enumerate("ADR"):
            if name in masks:
                for sign in (-1.0, 1.0):
                    acc[:, s] = masks[name]
                    u[s, (3 * kk + x) % M] = sign * (1000.0 + s)
                    s += 1
    return s


def _sets_of(acc, nk):
    """[launch][sample] -> "A" / "D" / "R" / None, by the restated classification"""
    out = []
    for k0 in range(0, nk, bh.MAX_LEVELS):
        NK = min(bh.MAX_LEVELS, nk - k0)
        bits = (acc[k0:k0 + NK] * (1 << np.arange(NK))[:, None]).sum(0)
        out.append(np.array([bh.mask_set(int(b), NK) for b in bits], object))
    return out


@pytest.mark.parametrize("n,M", [(1000, 257), (257, 64)])
@pytest.mark.parametrize("nk", [1, 2, 16, 17])
def test_envelope_mixed_mask_kinds_in_one_launch(gpu, nk, n, M):
    """every sample draws its kind; asserted on the reference before the launch: at every level, each register set that can
    accept the level decides the minimum of one cell and the maximum of one cell against the other two"""
    rng = np.random.default_rng(nk * 1000 + n)
    u = normal(rng, n, M)
    acc = _kind_masks(rng, n, nk)
    assert _plant(acc, u, nk) <= 6 * nk < n
    sets = _sets_of(acc, nk)
    for k in range(nk):
        L, kk, NK = k // bh.MAX_LEVELS, k % bh.MAX_LEVELS, min(bh.MAX_LEVELS, nk - k // bh.MAX_LEVELS * bh.MAX_LEVELS)
        expect = ["A"] + (["D"] if kk < NK - 1 else []) + (["R"] if NK >= 3 else [])
        env = {x: bh.envelope_ref(u, acc[k:k + 1] & (sets[L] == x)[None]) for x in "ADR"}
        for x in expect:
            others_lo = np.minimum.reduce([env[y][0][0] for y in "ADR" if y != x])
            others_hi = np.maximum.reduce([env[y][1][0] for y in "ADR" if y != x])
            assert env[x][2][0] > 0 and (env[x][0][0] < others_lo).any() and (env[x][1][0] > others_hi).any(), (k, x)
        assert all(env[x][2][0] == 0 for x in "ADR" if x not in expect)
    check_envelope(bh.Cells(u, **bh.split_of(M, 2)), acc)


@pytest.mark.parametrize("kind", ["grow", "shrink"])
@pytest.mark.parametrize("nk", [16, 17])
def test_envelope_purely_nested_levels(gpu, nk, kind):
    """nested sets in either direction at nk = 16 (FULL = 0xffff) and 17 (a second launch with NK = 1)"""
    n, M = 1000, 257
    rng = np.random.default_rng(nk)
    lev = np.arange(nk)[:, None]
    acc = lev >= rng.integers(0, nk + 1, n)[None] if kind == "grow" else lev <= rng.integers(-1, nk, n)[None]
    want = check_envelope(bh.Cells(normal(rng, n, M)), acc)
    assert len(set(want[2].tolist())) >= nk - 1


# ================================================================================================ special values
def test_envelope_special_values_in_u(gpu):
    """+-inf, +-0, subnormals (which come back unchanged), NaN in an accepted sample, in a rejected one and in a sample of
    the last, short split (55 of 1000 samples)"""
    n, M, nk = 1000, 257, 5
    p = bh.assert_plan(n, M)
    rng = np.random.default_rng(3)
    u = normal(rng, n, M)
    acc = rng.random((nk, n)) < 0.5
    u[:, 0] = rng.integers(-2000, 2000, n) * np.float32(2.0 ** -149)          # a column of subnormals
    u[:, 1] = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0))
    u[:, 2] = np.abs(u[:, 2])
    u[5, 2], u[6, 3], u[7, 3], u[8, 4], u[9, 5] = -0.0, INF, 1e38, -INF, 2.0 ** -149
    acc[:, [5, 6, 8, 9]] = True
    acc[:, 7] = False
    u[10, 6], u[11, 7], u[n - 3, 8] = NAN, NAN, NAN
    acc[:, 10], acc[:, 11], acc[:, n - 3] = (True, False, True, False, False), False, (False, False, False, True, False)
    assert n - 3 >= (p.S - 1) * p.per
    want = check_envelope(bh.Cells(u, **bh.split_of(M, 0)), acc)
    lo, hi, _ = want
    assert (np.abs(lo[:, 0]) < 1.2e-38).all() and (lo[:, 0] != 0).all() and (hi[:, 0] != 0).all()
    assert (lo[:, 2] == 0).all() and (hi[:, 3] == INF).all() and (lo[:, 4] == -INF).all()
    assert np.isnan(lo[[0, 2], 6]).all() and not np.isnan(lo[[1, 3, 4], 6]).any() and not np.isnan(lo[:, 7]).any() and np.isnan(hi[3, 8])


SPECIAL_R = (INF, -INF, NAN, 0.0, -0.0, 1.0, -1.0, 3.0e38, 1e-45)
# (q, m, c) per cell: hw = inf under +-inf residuals; a centre of inf under hw = inf (NaN bounds: nothing inside); q negative;
# q NaN; m zero; m negative; m = inf with q = 0 (NaN); a plain cell; m NaN; c NaN; c = -inf; hw overflowing to inf
SPECIAL_QMC = ((INF, 1.0, 0.0), (INF, 1.0, INF), (-1.0, 1.0, 0.0), (NAN, 1.0, 0.0), (1.0, 0.0, 0.0), (1.0, -1.0, 0.0), (0.0, INF, 0.0),
               (1.0, 1.0, 0.25), (1.0, NAN, 0.0), (1.0, 1.0, NAN), (1.0, 1.0, -INF), (3e38, 3e38, 1.0), (0.0, 1.0, 0.0), (0.0, 1.0, -0.0))


def test_cellwise_and_rowcount_special_values_in_r_q_m_c(gpu):
    """the reference decides every case, nothing is tolerated; the same operands through rowcount"""
    n, M = 40, 3 * len(SPECIAL_QMC)
    rng = np.random.default_rng(4)
    u, r = normal(rng, n, M), normal(rng, n, M)
    for i, v in enumerate(SPECIAL_R):
        r[2 * i] = v
    r[1, :] = 0.25
    qmc = np.array([SPECIAL_QMC[j % len(SPECIAL_QMC)] for j in range(M)], np.float32)
    with np.errstate(over="ignore"):
        qc = np.stack([qmc[:, 0], qmc[:, 0] * np.float32(2), np.abs(qmc[:, 0])]).astype(np.float32)
    m, c = qmc[:, 1].copy(), qmc[:, 2].copy()
    rc_ = bh.Cells(r, **bh.split_of(M, 2))
    uc = bh.Cells(u, *rc_.ext)                                     # dense beside the cropped residual
    for qq, mm, cc in ((qc, m, None), (qc, m, c), (qc, None, c), (np.array([-1.0, NAN, INF, 0.0, 1.0], np.float32), m, None),
                       (np.array([-1.0, NAN, INF, 0.0, 1.0], np.float32), m, c)):
        want = check_cellwise(uc, rc_, q=qq, m=mm, c=cc)
        check_cellwise(uc, rc_, q=qq, m=mm, c=cc, given=True)
        counts = check_rowcount(rc_, qq, mm, cc)
        bh.same_ints(counts.sum(1), want[2].astype(np.int64).sum(1))
        assert 0 < want[2].sum() < want[2].size * n
    blo, bhi = _sets(qc, m, c, M)
    assert np.isnan(blo[0, 1]) and bhi[0, 0] == INF and np.isnan(bhi[0, 6]) and bhi[0, 11] == INF


@pytest.mark.parametrize("form", ["abs", "centre", "percell"])
def test_bounds_round_twice_where_fma_contraction_would_show(gpu, form):
    """hw = q * m and c -+ hw are separate fp32 operations: at cells where fl(c -+ fl(q m)) != fl(fma) (no centre: where q m
    is inexact), a sample with r exactly ON the twice-rounded bound is inside and one an ulp beyond it outside, on the low
    side and on the high side; through cellwise and rowcount"""
    cells = bh.contraction_cells(q=None if form == "percell" else np.float32(1.37))
    if form == "abs":
        q0, m, c = cells.product[:, 0], cells.product[:, 1].copy(), None
    else:
        tri = np.concatenate([cells.plus, cells.minus])
        q0, m, c = tri[:, 0], tri[:, 1].copy(), tri[:, 2].copy()
    M = len(m)
    q = np.stack([q0, q0 * np.float32(1.5)]) if form == "percell" else np.array([q0[0], q0[0] * np.float32(1.5)], np.float32)
    blo, bhi = _sets(q, m, c, M)
    mid = c if c is not None else np.zeros(M, np.float32)
    r = np.stack([blo[0], bh.ulp_step(blo[0], False), bhi[0], bh.ulp_step(bhi[0], True), mid]).astype(np.float32)
    u = np.repeat(np.array([[-1.0], [-2.0], [1.0], [2.0], [0.0]], np.float32), M, 1)
    want = bh.cellwise_ref(u, r, blo, bhi)
    assert (want[0][0] == -1).all() and (want[1][0] == 1).all() and (want[2][0] == 3).all()      # on: inside; beyond: outside
    uc, rc_ = bh.Cells(u), bh.Cells(r)
    check_cellwise(uc, rc_, q=q, m=m, c=c)
    counts = check_rowcount(rc_, q, m, c)
    assert counts[0].tolist() == [M, 0, M, 0, M]
    if c is not None:                                              # the centre per sample (stride n): the same bounds
        check_rowcount(rc_, q, m, bh.Cells(np.repeat(c[None], 5, 0)))


# ================================================================================================ accumulation
@pytest.mark.parametrize("n,M", [(64, 129), (4097, 64)], ids=["P1", "P68"])
def test_results_accumulate_into_what_lo_hi_and_count_hold(gpu, n, M):
    """lo / hi start from finite per-cell values, some below and some above the data's envelope, counts from non-zero
    values; a second, identical call leaves lo / hi as they are and adds the same counts again"""
    p = bh.assert_plan(n, M)
    assert p.P == 1 or p.P > 64
    rng = np.random.default_rng(n)
    nk = 5
    uc, rc_ = bh.Cells(normal(rng, n, M), **bh.split_of(M, 2)), bh.Cells(normal(rng, n, M), **bh.split_of(M, 2))
    lo0 = np.where(rng.random((nk, M)) < 0.5, -9.0, 9.0).astype(np.float32) + normal(rng, nk, M)
    hi0 = np.where(rng.random((nk, M)) < 0.5, -9.0, 9.0).astype(np.float32) + normal(rng, nk, M)
    acc = rng.random((nk, n)) < 0.5
    prior = (lo0, hi0, rng.integers(1, 1 << 40, nk))
    first, second = envelope(uc, acc, prior, times=2)
    want = bh.merge_ref(bh.envelope_ref(uc.data, acc), prior)
    assert (want[0] == lo0).any() and (want[0] < lo0).any() and (want[1] == hi0).any() and (want[1] > hi0).any()
    for got, calls in ((first, 1), (second, 2)):
        bh.same_bits(got[0], want[0])
        bh.same_bits(got[1], want[1])
        bh.same_ints(got[2], prior[2] + calls * acc.sum(1))
    prior = (lo0, hi0, rng.integers(1, 1000, (nk, M)).astype(np.int32))
    first, second = cellwise(uc, rc_, nk, q=Q5, prior=prior, times=2)
    new = bh.cellwise_ref(uc.data, rc_.data, *_sets(Q5, None, None, M))
    want = bh.merge_ref(new, prior)
    assert (want[0] == lo0).any() and (want[0] < lo0).any() and (want[1] == hi0).any() and (want[1] > hi0).any()
    for got, calls in ((first, 1), (second, 2)):
        bh.same_bits(got[0], want[0])
        bh.same_bits(got[1], want[1])
        bh.same_ints(got[2], prior[2].astype(np.int64) + calls * new[2])


# ================================================================================================ rowcount
RC_N = (1, 7, 8, 9, 63, 64, 65, 129)


def _rowcount_case(rng, n, M, nk, kind, large=False):
    """centre absent, per cell and per sample on one residual; the first two also against the sum of cellwise's per-cell
    counts on the same operands (``large``: without comparing those per-cell counts with their own reference once more)"""
    rc_ = bh.Cells(normal(rng, n, M), **bh.split_of(M, kind))
    q = np.linspace(0.3, 2.0, nk).astype(np.float32)
    qc = (q[:, None] * (0.5 + rng.random((nk, M)))).astype(np.float32)
    m = (0.5 + rng.random(M)).astype(np.float32)
    c = (0.3 * normal(rng, M)).astype(np.float32)
    cs = bh.Cells(0.3 * normal(rng, n, M), *rc_.ext)               # dense, where the residual may be cropped
    for qq, mm, cc in ((q, None, None), (qc, m, c), (q, m, cs)):
        counts = check_rowcount(rc_, qq, mm, cc)
        if not isinstance(cc, bh.Cells):
            got = cellwise(rc_, rc_, nk, q=qq, m=mm, c=cc)[0]
            bh.same_ints(got[2].astype(np.int64).sum(1), counts.sum(1))
            if not large:
                bh.same_ints(got[2], bh.cellwise_ref(rc_.data, rc_.data, *_sets(qq, mm, cc, M))[2])
    return rc_


@pytest.mark.parametrize("M", [1, 255, 256, 257, 513])
def test_rowcount_sample_groups_and_cell_chunks(gpu, M):
    """n % 64 and n % 8 (the group of 64 samples, the loop unrolled by 8 and its tail), M % 256 (lanes past the last cell)"""
    for i, n in enumerate(RC_N):
        _rowcount_case(np.random.default_rng(M * 1000 + n), n, M, 5, i % 3)


def test_rowcount_fewer_splits_than_chunks(gpu):
    """(65537, 513), nk = 2: 1025 groups, 2 splits over 3 chunks (chunk ranges 0..1 and 1..3), a last group of one sample"""
    n, M = 65537, 513
    groups, chunks = (n + 63) // 64, (M + 255) // 256
    assert groups == 1025 and chunks == 3 and min(chunks, (2048 + groups - 1) // groups) == 2 and n % 64 == 1
    _rowcount_case(np.random.default_rng(5), n, M, 2, 0, large=True)


def test_rowcount_more_groups_than_the_grid_holds(gpu):
    """(4194241, 2), nk = 1: 65536 groups on a gridDim.y of 65535 - the stride loop takes one group in its second trip"""
    n, M = 4194241, 2
    assert (n + 63) // 64 == 65536
    _rowcount_case(np.random.default_rng(6), n, M, 1, 0, large=True)


# ================================================================================================ error returns
def test_error_returns_leave_the_outputs_alone(gpu):
    """every refusal returns before any launch: the framed outputs hold what they held"""
    _lib, lib = _L()
    n, M, nk = 300, 65, 3
    rng = np.random.default_rng(9)
    ud, rd = dev(normal(rng, n, M)), dev(normal(rng, n, M))
    ad = dev(np.ones((nk, n), np.uint8))
    qd, md = dev(Q5[:nk]), dev(np.ones(M, np.float32))
    qcd = dev(np.ones((nk, M), np.float32))
    lo, hi = bh.framed(nk * M, F32, 0, DEV).set(np.full(nk * M, 5.0)), bh.framed(nk * M, F32, 0, DEV).set(np.full(nk * M, -5.0))
    c64, c32 = bh.framed(nk, I64, 0, DEV).set(np.full(nk, 7)), bh.framed(nk * M, I32, 0, DEV).set(np.full(nk * M, 7))
    cnts = bh.framed(nk * n, I32, 0, DEV).set(np.full(nk * n, 7))
    we, wc = query("envelope", n, (1, 1, M), nk), query("cellwise", n, (1, 1, M), nk)
    assert wc > 0
    work = bh.framed(max(we, wc), U8, 0, DEV)
    st = _lib.stream()
    big = 1 << 16

    def env(n_=n, ext=(1, 1, M), ld=n, nk_=nk, w=work, wb=we):
        return lib.pre_bounds_envelope_f32(P(ud), M, 0, 0, n_, *ext, P(ad), ld, nk_, P(lo), P(hi), P(c64), P(w), wb, st)

    def cell(ext=(1, 1, M), q=qd, q_ld=0, m=None, blo=None, bhi=None, nk_=nk, w=work, wb=wc):
        return lib.pre_bounds_cellwise_f32(P(ud), M, 0, 0, P(rd), M, 0, 0, n, *ext, P(q), q_ld, P(m), None, P(blo), P(bhi), nk_,
                                           P(lo), P(hi), P(c32), P(w), wb, st)

    def rows(ext=(1, 1, M), q=qd, q_ld=0, nk_=nk, ld=n):
        return lib.pre_bounds_rowcount_f32(P(rd), M, 0, 0, None, 0, 0, 0, n, *ext, P(q), q_ld, None, nk_, P(cnts), ld, st)

    cases = [
        ("envelope: workspace one byte short", env(wb=we - 1), PRE_E_NULL),
        ("envelope: null workspace", env(w=None), PRE_E_NULL),
        ("envelope: accept_ld < n", env(ld=n - 1), PRE_E_NULL),
        ("envelope: nk = 0", env(nk_=0), PRE_E_NULL),
        ("envelope: A*B*C above int32", env(ext=(big, big, 1)), PRE_E_SHAPE),
        ("cellwise: workspace one byte short", cell(wb=wc - 1), PRE_E_NULL),
        ("cellwise: null workspace", cell(w=None), PRE_E_NULL),
        ("cellwise: 0 < q_ld < M", cell(q=qcd, q_ld=M - 1), PRE_E_SHAPE),
        ("cellwise: nk = 0", cell(nk_=0), PRE_E_NULL),
        ("cellwise: blo together with q", cell(blo=qcd, bhi=qcd), PRE_E_NULL),
        ("cellwise: blo together with m", cell(q=None, m=md, blo=qcd, bhi=qcd), PRE_E_NULL),
        ("cellwise: bhi without blo", cell(bhi=qcd), PRE_E_NULL),
        ("cellwise: blo without bhi", cell(q=None, blo=qcd), PRE_E_NULL),
        ("cellwise: A*B*C above int32", cell(ext=(big, big, 1)), PRE_E_SHAPE),
        ("rowcount: counts_ld < n", rows(ld=n - 1), PRE_E_NULL),
        ("rowcount: 0 < q_ld < M", rows(q=qcd, q_ld=M - 1), PRE_E_SHAPE),
        ("rowcount: nk = 0", rows(nk_=0), PRE_E_NULL),
        ("rowcount: A*B*C above int32", rows(ext=(big, big, 1)), PRE_E_SHAPE),
    ]
    torch.cuda.synchronize()
    for what, rc, want in cases:
        assert rc == want, (what, rc)
    b = ctypes.c_int64(-1)
    assert lib.pre_bounds_envelope_workspace(n, big, big, 1, nk, ctypes.byref(b)) == PRE_E_SHAPE
    assert lib.pre_bounds_cellwise_workspace(n, 1, 1, M, 0, ctypes.byref(b)) == PRE_E_NULL and b.value == -1
    for f, v in ((lo, 5.0), (hi, -5.0), (c64, 7), (c32, 7), (cnts, 7)):
        assert f.untouched() and (f.view == v).all()
    assert work.untouched() and (work.view == 0xA5).all()
    # the same calls with nothing wrong: accepted
    assert env() == 0 and cell() == 0 and rows() == 0 and cell(q=qcd, q_ld=M) == 0 and cell(q=None, blo=qcd, bhi=qcd) == 0
    torch.cuda.synchronize()


# ================================================================================================ through sample_bounds
API_N, API_CELLS = 48, (20, 9, 10)


def _api_layouts(gen):
    """(name, u, r) device views [48, 20, 9, 10] whose memory orders disagree, or that are cropped / row-padded"""
    from cp_pre_amd import pipeline
    n, (T, X, Y) = API_N, API_CELLS

    def rand(*shape):
        return torch.randn(*shape, device=DEV, generator=gen)
    ntf = lambda: rand(n, X, Y, T).permute(0, 3, 1, 2)             # Nt fastest in memory
    rp = pipeline.row_padded(n, API_CELLS, device=DEV)
    rp.copy_(rand(n, T, X, Y))
    return [("u_ntfast_r_contiguous", ntf(), rand(n, T, X, Y)), ("u_contiguous_r_ntfast", rand(n, T, X, Y), ntf()),
            ("u_cropped", rand(n, T + 2, X + 2, Y + 2)[:, 1:-1, 1:-1, 1:-1], rand(n, T, X, Y)),
            ("u_row_padded_r_ntfast", rp, ntf()), ("both_ntfast", ntf(), ntf())]


@pytest.mark.parametrize("nk", [5, 17])
def test_sample_bounds_cellwise_on_operands_laid_out_differently(gpu, nk):
    """the copy route of _operands (u and r in different memory orders), per-cell q / modulation / centre carried into a
    permuted flat order, a cropped and a row-padded u; at 5 and at 17 levels"""
    from cp_pre_amd import sample_bounds as sb
    gen = torch.Generator(device=DEV).manual_seed(nk)
    rng = np.random.default_rng(nk)
    n, cells = API_N, API_CELLS
    M = int(np.prod(cells))
    q = np.linspace(0.1, 2.0, nk).astype(np.float32)
    qc = (q[:, None] * (0.5 + rng.random((nk, M)))).astype(np.float32)
    m, c = (0.5 + rng.random(M)).astype(np.float32), (0.3 * normal(rng, M)).astype(np.float32)
    c[1] = 0.0                                                     # (cell (0, 0, 1): r = 0 is inside at every level)
    for name, u, r in _api_layouts(gen):
        u[3, 0, 0, 1] = float("nan")
        r[3, 0, 0, 1] = 0.0
        r[4, 1, 2, 3] = float("nan")
        un, rn = u.cpu().numpy().reshape(n, M), r.cpu().numpy().reshape(n, M)
        for qq, mm, cc in ((q, None, None), (qc, m, c)):
            got = sb.sample_bounds(u, r, dev(qq.reshape((nk,) + (cells if qq.ndim == 2 else ()))), rule="cellwise",
                                   modulation=dev(mm.reshape(cells)) if mm is not None else None,
                                   centre=dev(cc.reshape(cells)) if cc is not None else None)
            want = bh.cellwise_ref(un, rn, *_sets(qq, mm, cc, M))
            assert tuple(got[0].shape) == (nk,) + cells and got[2].dtype == torch.int32, name
            bh.same_bits(got[0].cpu().numpy(), want[0])
            bh.same_bits(got[1].cpu().numpy(), want[1])
            bh.same_ints(got[2].cpu().numpy(), want[2])
            assert np.isnan(want[0][:, 1]).all()


def test_sample_bounds_threshold_met_exactly_with_a_centre_laid_out_differently(gpu):
    """res Nt-fastest, the per-sample centre contiguous; the threshold is the fraction of inside cells of one sample at one
    level, which that sample must meet (>=)"""
    from cp_pre_amd import sample_bounds as sb
    gen = torch.Generator(device=DEV).manual_seed(11)
    n, cells = API_N, API_CELLS
    T, X, Y = cells
    M, nk = T * X * Y, 6
    u = torch.randn(n, T, X, Y, device=DEV, generator=gen)
    res = torch.randn(n, X, Y, T, device=DEV, generator=gen).permute(0, 3, 1, 2)
    centre = 0.3 * torch.randn(n, T, X, Y, device=DEV, generator=gen)
    q = np.linspace(0.5, 1.6, nk).astype(np.float32)
    un, rn, cn = (t.cpu().numpy().reshape(n, M) for t in (u, res, centre))
    counts = bh.rowcount_ref(rn, *bh.sets_f32(q, None, cn))
    k_star = 2
    s_star = int(np.argsort(counts[k_star])[n // 2])               # the sample with the median count
    thr = float(counts[k_star, s_star]) / float(M)
    acc = counts.astype(np.float64) / float(M) >= thr
    assert acc[k_star, s_star] and 0 < acc[k_star].sum() < n
    want = bh.envelope_ref(un, acc)
    for cc, ref in ((centre, want), (None, None)):
        if cc is None:                                             # no centre, the same residual: its own reference
            cnt0 = bh.rowcount_ref(rn, *_sets(q, None, None, M))
            thr0 = float(cnt0[k_star, s_star]) / float(M)
            ref = bh.envelope_ref(un, cnt0.astype(np.float64) / float(M) >= thr0)
            got = sb.sample_bounds(u, res, dev(q), rule="threshold", threshold=thr0)
        else:
            got = sb.sample_bounds(u, res, dev(q), rule="threshold", threshold=thr, centre=cc)
        bh.same_bits(got[0].cpu().numpy(), ref[0])
        bh.same_bits(got[1].cpu().numpy(), ref[1])
        bh.same_ints(got[2].cpu().numpy(), ref[2])
    rc_counts = torch.zeros(nk, n, dtype=torch.int32, device=DEV)
    sb.rowcount_launch(res, dev(q), centre, None, rc_counts)
    bh.same_ints(rc_counts.cpu().numpy(), counts)
