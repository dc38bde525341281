"""Plain numpy references of the sample-acceptance bounds kernels (cp_pre_amd/csrc/sample_bounds.hip), a Python
restatement of their launch plan and the memory layouts their tests use (tests/test_gpu_bounds_seams.py on the GPU,
tests/test_bounds_ref_cpu.py for what stands here; the page that goes with them is tests/BOUNDS_TESTS.md).  No GPU is
needed to import or call anything here and nothing of cp_pre_amd is imported: ``framed`` lays out memory with torch alone.

The references work in the kernels' number format: fp32 numpy arrays stay fp32 (numpy's fp32 *, +, - are single correctly
rounded IEEE operations, subnormals included); min / max round nothing."""
import collections

import numpy as np
import torch

NAN_BITS = 0x7FC00000
_IGNORE = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")
MAX_LEVELS = 16                                        # PRE_BOUNDS_MAX_LEVELS: levels per launch


def f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


# ------------------------------------------------------------------------------------------------ references
def envelope_ref(u, acc):
    """u [n, M], acc bool [nk, n] -> (lo, hi fp32 [nk, M], count int64 [nk]): per level ``u[acc[k]].min(0)`` / ``.max(0)``
    (np.min / np.max propagate a NaN); +inf / -inf and 0 for a level that accepts nothing."""
    u = f32(u)
    u = u.reshape(u.shape[0], -1)
    acc = np.asarray(acc).astype(bool)
    nk = acc.shape[0]
    lo = np.full((nk, u.shape[1]), np.inf, np.float32)
    hi = np.full((nk, u.shape[1]), -np.inf, np.float32)
    for k in range(nk):
        if acc[k].any():
            sel = u[acc[k]]
            lo[k], hi[k] = sel.min(0), sel.max(0)
    return lo, hi, acc.sum(1).astype(np.int64)


def cellwise_ref(u, r, blo, bhi):
    """u, r [n, M], blo, bhi [nk, M] -> (lo, hi fp32 [nk, M], count int32 [nk, M]): cell j of sample s counts at level k iff
    blo[k, j] <= r[s, j] <= bhi[k, j] (fp32 comparisons: a NaN on either side is outside, a value on a bound inside)."""
    u, r = f32(u), f32(r)
    u, r = u.reshape(u.shape[0], -1), r.reshape(r.shape[0], -1)
    blo, bhi = f32(blo), f32(bhi)
    nk, M = blo.shape[0], u.shape[1]
    lo, hi = np.empty((nk, M), np.float32), np.empty((nk, M), np.float32)
    cnt = np.empty((nk, M), np.int32)
    for k in range(nk):
        inside = (r >= blo[k][None]) & (r <= bhi[k][None])
        lo[k] = np.where(inside, u, np.float32(np.inf)).min(0)
        hi[k] = np.where(inside, u, np.float32(-np.inf)).max(0)
        cnt[k] = inside.sum(0)
    return lo, hi, cnt


def rowcount_ref(r, blo, bhi):
    """r [n, M]; blo, bhi [nk, M] (per cell) or [nk, n, M] (a per-sample centre) -> int64 [nk, n]: the cells of each sample
    inside at each level."""
    r = f32(r)
    r = r.reshape(r.shape[0], -1)
    blo, bhi = f32(blo), f32(bhi)
    out = np.empty((blo.shape[0], r.shape[0]), np.int64)
    for k in range(blo.shape[0]):
        lo_k, hi_k = (blo[k][None], bhi[k][None]) if blo.ndim == 2 else (blo[k], bhi[k])
        out[k] = ((r >= lo_k) & (r <= hi_k)).sum(1)
    return out


def sets_f32(q, m=None, c=None):
    """The bounds in fp32, one rounded operation per numpy operation: hw = q (q [nk] or [nk, M]), hw = q * m with a
    modulation m [M]; (c - hw, c + hw) with a centre c [M] (-> [nk, M]) or [n, M] (-> [nk, n, M]); no centre: (-hw, hw)."""
    q = f32(q)
    with np.errstate(**_IGNORE):
        hw = q[:, None] if q.ndim == 1 else q
        if m is not None:
            hw = hw * f32(m)[None]
        if c is None:
            lo, hi = -hw, hw
        else:
            c = f32(c)
            if c.ndim == 2:
                hw = hw[:, None, :]
            lo, hi = c[None] - hw, c[None] + hw
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    return lo, hi


def merge_ref(new, prior):
    """Results accumulate: (lo, hi, count) of a call that started from ``prior`` - np.minimum, np.maximum (both propagate a
    NaN) and +."""
    with np.errstate(**_IGNORE):
        return np.minimum(prior[0], new[0]), np.maximum(prior[1], new[1]), prior[2] + new[2].astype(prior[2].dtype)


# ------------------------------------------------------------------------------------------------ comparison
def bits32(x):
    """int32 bit patterns of an fp32 array (a copy): every NaN as one NaN, a zero of either sign as +0 (the header leaves
    the sign of a zero result open); everything else, subnormals included, as it is."""
    x = f32(x).copy()
    b = x.view(np.int32)
    b[np.isnan(x)] = NAN_BITS
    b[x == 0] = 0
    return b


def same_bits(got, ref):
    got, ref = bits32(got).reshape(-1), bits32(ref).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (bad.size, bad[:8].tolist(), got[bad[:8]].view(np.float32).tolist(), ref[bad[:8]].view(np.float32).tolist())


def same_ints(got, ref):
    got, ref = np.asarray(got).astype(np.int64).reshape(-1), np.asarray(ref).astype(np.int64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), ref[bad[:8]].tolist())


# ------------------------------------------------------------------------------------------------ the launch plan
Plan = collections.namedtuple("Plan", "W rows chunks S per last P P2 folds batches tail")


def plan(n, M):
    """``make_plan`` of sample_bounds.hip restated, with what follows from it: W cells per row of a workgroup and its
    ``rows`` sample rows, ``chunks`` of W cells, S sample splits of ``per`` samples (the last one ``last``), P = S * rows
    partial slots (1: no workspace), P2 = ceil(P / 64) second-level partials, the number of fold launches (0, 1, 2), and
    the full batches of 8 / the tail of the sample loop of row 0 in a full split.  Only ever used to assert which branch a
    shape reaches, never to compute an expected result."""
    cw_log = 8 if M > 128 else (7 if M > 64 else 6)
    W = 1 << cw_log
    rows = 256 // W
    chunks = (M + W - 1) // W
    S = (1024 + chunks - 1) // chunks
    S = min(S, (n + rows * 64 - 1) // (rows * 64))
    S = max(1, min(S, 4096 // rows))
    per = (n + S - 1) // S
    S = (n + per - 1) // per
    P = S * rows
    P2 = (P + 63) // 64
    mine = (per + rows - 1) // rows
    return Plan(W, rows, chunks, S, per, n - (S - 1) * per, P, P2, 0 if P == 1 else (1 if P2 == 1 else 2), mine // 8, mine % 8)


# (n, M) of the envelope / cellwise table of tests/BOUNDS_TESTS.md: what each row claims of its plan
TABLE = {
    (1, 1): dict(W=64, rows=4, S=1, P=4, folds=1),
    (3, 64): dict(W=64, rows=4, S=1, P=4, folds=1),
    (256, 64): dict(W=64, S=1, P=4),
    (257, 64): dict(W=64, S=2, per=129, last=128, P=8),
    (4096, 64): dict(S=16, P=64, P2=1, folds=1),
    (4097, 64): dict(S=17, P=68, P2=2, folds=2),
    (4161, 63): dict(W=64, chunks=1, S=17, P=68, P2=2, folds=2),
    (128, 65): dict(W=128, rows=2, S=1, P=2),
    (129, 128): dict(W=128, rows=2, S=2, per=65, last=64, P=4),
    (8193, 100): dict(W=128, P=130, P2=3, folds=2),
    (7, 129): dict(W=256, rows=1, P=1, folds=0, batches=0, tail=7),
    (8, 129): dict(W=256, P=1, folds=0, batches=1, tail=0),
    (9, 129): dict(W=256, P=1, folds=0, batches=1, tail=1),
    (16, 129): dict(W=256, P=1, folds=0, batches=2, tail=0),
    (17, 129): dict(W=256, P=1, folds=0, batches=2, tail=1),
    (64, 129): dict(W=256, P=1, folds=0, batches=8, tail=0),
    (65, 129): dict(W=256, S=2, per=33, last=32, P=2),
    (64, 513): dict(W=256, chunks=3, P=1, folds=0),
    (1000, 257): dict(W=256, chunks=2, S=16, per=63, last=55, batches=7, tail=7, P=16),
}
# the two large rows (envelope at nk = 3, cellwise at nk = 2) and the shape of the level tests
LARGE_ENVELOPE, LARGE_CELLWISE, LEVELS_SHAPE = (262144, 64), (262145, 33), (300, 65)
TABLE_MORE = {
    LARGE_ENVELOPE: dict(S=1024, P=4096, P2=64, folds=2),
    LARGE_CELLWISE: dict(S=1021, per=257, last=5, P=4084, P2=64, folds=2),
    LEVELS_SHAPE: dict(W=128, rows=2, S=3, per=100, P=6, folds=1),
}


def assert_plan(n, M):
    """the plan of (n, M) is what its row of the table claims"""
    p = plan(n, M)
    for key, want in {**TABLE, **TABLE_MORE}[(n, M)].items():
        assert getattr(p, key) == want, ((n, M), key, p)
    return p


def _up256(x):
    return (x + 255) & ~255


def workspace_bytes(n, M, nk, entry):
    """``workspace_bytes`` restated for ``entry`` = "envelope" / "cellwise": the mask bits of the envelope, the partials
    [P][min(nk, 16)][M] (lo, hi, and the cellwise count) and the second fold level, each rounded up to 256 bytes."""
    p = plan(n, M)
    b = _up256(4 * n) if entry == "envelope" else 0
    if p.P > 1:
        per = min(nk, MAX_LEVELS) * M * (12 if entry == "cellwise" else 8)
        b += _up256(p.P * per) + (_up256(p.P2 * per) if p.P2 > 1 else 0)
    return b


def mask_set(mask, NK):
    """The register set of ``envelope_kernel<NK>`` that a sample with the accept bits ``mask`` (of one launch) updates: "A"
    (levels f..NK-1, the full mask included), "D" (levels 0..t, t < NK-1), "R" (any other mask), None (no level)."""
    full = (1 << NK) - 1
    mask &= full
    if mask == 0:
        return None
    low = mask & -mask
    if mask + low == full + 1:
        return "A"
    if mask & (mask + 1) == 0:
        return "D"
    return "R"


# ------------------------------------------------------------------------------------------------ memory
_INT_OF = {torch.float32: torch.int32, torch.int32: torch.int32, torch.int64: torch.int64, torch.uint8: torch.uint8}
_FILL = {torch.int32: 0x5A5AC3C3, torch.int64: 0x5A5AC3C35A5AC3C3, torch.uint8: 0xA5}


class Framed:
    """``n_elems`` elements of ``dtype`` inside a larger allocation of the test's: ``alloc`` (1-D, filled with NaN for
    floats, a bit pattern for integers), ``view`` (``guard + offset`` elements from its start; exactly ``n_elems`` long -
    a workspace of the queried size has not a byte more) and the frame around it, which ``untouched`` compares bit for bit
    with what it held at the start.  The guard is 64 elements (256 for uint8: the byte workspace keeps its 256-byte
    alignment at offset 0; its offset is a multiple of 4, as its uint32 and fp32 contents need)."""

    def __init__(self, n_elems, dtype, offset=0, device=None):
        guard = 256 if dtype == torch.uint8 else 64
        assert 0 <= offset < guard and (dtype != torch.int64 or offset % 2 == 0)
        self.alloc = torch.empty(guard + offset + n_elems + guard, dtype=dtype, device=device)
        self.alloc.fill_(float("nan") if dtype.is_floating_point else _FILL[dtype])
        self.lo, self.hi = guard + offset, guard + offset + n_elems
        self.view = self.alloc[self.lo:self.hi]
        self._frame = self.frame()

    def set(self, values):
        self.view.copy_(torch.as_tensor(values).reshape(-1).to(self.alloc.dtype))
        return self

    def data_ptr(self):
        # (from the allocation: torch gives an empty view a null data_ptr)
        return self.alloc.data_ptr() + self.lo * self.alloc.element_size()

    def frame(self):
        raw = self.alloc.view(_INT_OF[self.alloc.dtype])
        return torch.cat([raw[:self.lo], raw[self.hi:]]).clone()

    def untouched(self):
        return torch.equal(self.frame(), self._frame)


def framed(n_elems, dtype, offset=0, device=None):
    return Framed(n_elems, dtype, offset, device)


class Cells:
    """n samples of M = A * B * C cells where a kernel reads them: cell (a, b, x) of sample s at element s*sN + a*sA + b*sB
    + x of ``buf``, flat cell j = (a*B + b)*C + x.  ``buf`` is NaN wherever no cell lies (between the rows of a cropped
    view, between samples), so a read beside a cell shows in a minimum."""

    def __init__(self, data, A=1, B=1, C=None, sA=None, sB=None, sN=None):
        data = f32(data)
        n, M = data.shape
        C = M if C is None else C
        assert A * B * C == M
        sB = C if sB is None else sB
        sA = B * sB if sA is None else sA
        sN = A * sA if sN is None else sN
        assert sB >= C and sA >= B * sB and sN >= A * sA
        a, b, x = np.unravel_index(np.arange(M), (A, B, C))
        self.idx = a * sA + b * sB + x
        if sN == M:                                    # dense: the data as they are
            self.buf = data
        else:
            self.buf = np.full((n, sN), np.nan, np.float32)
            self.buf[:, self.idx] = data
        self.data, self.n, self.M, self.ext, self.strides = data, n, M, (A, B, C), (sN, sA, sB)


def factor3(M):
    """(A, B, C) with A * B * C == M and B, C > 1 (A > 1 too where M has three factors), or None."""
    best = None
    for c in range(2, M):
        if M % c:
            continue
        rest = M // c
        for b in range(2, rest + 1):
            if rest % b == 0:
                cand = (rest // b, b, c)
                if cand[0] > 1:
                    return cand
                best = best or cand
    return best


def split_of(M, kind):
    """The (A, B, C, sA, sB) of a table row: kind 0 one dense row (1, 1, M), kind 1 (M, 1, 1) (every cell an outermost
    index), kind 2 a cropped view (sB, sA larger than dense) where M factors, else kind 0."""
    if kind == 1:
        return dict(A=M, B=1, C=1)
    f = factor3(M) if kind == 2 else None
    if f is None:
        return dict(A=1, B=1, C=M)
    A, B, C = f
    return dict(A=A, B=B, C=C, sB=C + 3, sA=B * (C + 3) + 5)


# ------------------------------------------------------------------------------------------------ contraction
def fma_f32(q, m, c):
    """fl32(q * m + c) with ONE rounding, emulated in fp64: q * m is exact there (48 bits), the sum is rounded to odd (its
    error from TwoSum decides the sticky bit), and a round-to-odd fp64 value rounds to fp32 as the exact one does (53 >= 24
    + 2 bits).  For operands whose product and sum stay in fp32's normal range."""
    q, m, c = (np.asarray(v, np.float32).astype(np.float64) for v in (q, m, c))
    p = q * m
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                    # TwoSum: p + c == s + err exactly
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


ContractionCells = collections.namedtuple("ContractionCells", "plus minus product")


def contraction_cells(count=12, seed=20240607, q=None):
    """Cells at which fma contraction shows, found by a seeded search: ``plus`` fp32 [count, 3] triples (q, m, c) with
    fl(c + fl(q*m)) != fl(fma(q, m, c)), ``minus`` the same for fl(c - fl(q*m)) != fl(fma(-q, m, c)), ``product`` [count,
    2] pairs (q, m) whose product is inexact in fp32 (the no-centre form has no addition to fuse: its bound is the rounded
    product itself).  ``q``: one level shared by every cell (a scalar q-hat) instead of a random one per cell.  q and m lie
    in [0.5, 2), c in [1, 4): products and sums are normal numbers."""
    rng = np.random.default_rng(seed)
    qs = (0.5 + 1.5 * rng.random(4096)).astype(np.float32)
    m = (0.5 + 1.5 * rng.random(4096)).astype(np.float32)
    c = (1.0 + 3.0 * rng.random(4096)).astype(np.float32)
    if q is not None:
        qs = np.full(4096, q, np.float32)
    hw = qs * m
    plus = np.flatnonzero((c + hw) != fma_f32(qs, m, c))[:count]
    minus = np.flatnonzero((c - hw) != fma_f32(-qs, m, c))[:count]
    inexact = np.flatnonzero(hw.astype(np.float64) != qs.astype(np.float64) * m.astype(np.float64))[:count]
    assert len(plus) == len(minus) == len(inexact) == count
    tri = np.stack([qs, m, c], 1)
    return ContractionCells(tri[plus], tri[minus], tri[inexact][:, :2])


def ulp_step(x, up):
    """The fp32 neighbour of x (finite, non-zero) above (``up``) or below it."""
    return np.nextafter(f32(x), np.float32(np.inf if up else -np.inf))
