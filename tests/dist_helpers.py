"""Plain numpy references of the histogram-exchange sweeps (cp_pre_amd/csrc/dist_select.hip, include/cp_pre_dist.h), the
checks their tests share and the memory layouts they use (tests/test_gpu_dist_seams.py on the GPU with ``pipeline.HipOps``,
tests/test_dist_seams_cpu.py on the CPU with the torch double ``DistOps``; the page that goes with them is
tests/DIST_TESTS.md).  No GPU is needed to import or call anything here.

Nothing below restates ``DistOps`` or the tensor code of ``pipeline._marginal_histogram``: keys, window, bucket map and
narrowing are written from the sentences of the header, in numpy, one rounded fp32 operation per numpy operation.  Every
``check_*`` raises AssertionError: the CPU file plants mistakes in ``DistOps`` and shows the check meant for each failing."""
import numpy as np
import torch

NB, PICK_CAP, MAX_SLOTS = 256, 2048, 64
_IGNORE = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")
_FILL = {torch.int32: 0x5A5AC3C3, torch.int64: 0x5A5AC3C35A5AC3C3}
_INT_OF = {torch.float32: torch.int32, torch.int32: torch.int32, torch.int64: torch.int64}
HIST_POISON = 0x5A5AC3C3


def f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


# ------------------------------------------------------------------------------------------------ keys
def keys(a):
    """The order-preserving uint32 image of fp32, as int64: ascending floats <-> ascending keys, -0.0 right below +0.0.
    A set sign bit flips every bit, a clear one sets the sign bit."""
    u = f32(a).view(np.uint32).astype(np.int64)
    return np.where(u >= 1 << 31, 0xFFFFFFFF - u, u + (1 << 31))


def key2f(k):
    k = np.asarray(k, dtype=np.int64)
    u = np.where(k >= 1 << 31, k - (1 << 31), 0xFFFFFFFF - k)
    return u.astype(np.uint32).view(np.float32)


def _i32(u):
    """int64 values in [0, 2^32) -> the int32 with the same 32 bits."""
    u = np.asarray(u, dtype=np.int64)
    return np.where(u >= 1 << 31, u - (1 << 32), u).astype(np.int32)


def sort_ref(col_rows, ks):
    """[len(ks), C] fp32: ``np.sort`` of every column of [N, C] by key (np.sort leaves -0.0 against +0.0 open, keys do not),
    ranks ``ks``; NaN for every rank of a column that holds a NaN."""
    x = f32(col_rows)
    out = key2f(np.sort(keys(x), axis=0)[np.asarray(ks, dtype=np.int64)])
    out[:, np.isnan(x).any(0)] = np.nan
    return out


def ident(got, ref):
    """Bit for bit where the reference is not NaN, NaN where it is."""
    got, ref = f32(got), f32(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nan = np.isnan(ref)
    bad = np.flatnonzero((np.isnan(got) != nan).reshape(-1) | ((got.view(np.int32) != ref.view(np.int32)) & ~nan).reshape(-1))
    assert bad.size == 0, (bad[:8].tolist(), got.reshape(-1)[bad[:8]].tolist(), ref.reshape(-1)[bad[:8]].tolist())


# ------------------------------------------------------------------------------------------------ window
def window_ref(rows, Cp):
    """int32 [3, Cp] of the header: (klo ^ 2^31, ~khi ^ 2^31, 0 if a NaN else 1) per column of rows [n, C]; a column
    without a non-NaN score: the MIN identities (klo = 2^32 - 1, khi = 0); pad cells C <= c < Cp: the constant 0.0."""
    rows = f32(rows)
    C = rows.shape[1]
    zero = int(keys(np.float32(0.0)).reshape(-1)[0])
    lo, hi = np.full(Cp, zero, np.int64), np.full(Cp, zero, np.int64)
    flag = np.ones(Cp, np.int32)
    if C:
        k, isn = keys(rows), np.isnan(rows)
        lo[:C] = np.where(isn, 0xFFFFFFFF, k).min(0)
        hi[:C] = np.where(isn, 0, k).max(0)
        flag[:C] = np.where(isn.any(0), 0, 1)
    return np.stack([_i32(lo ^ (1 << 31)), _i32((0xFFFFFFFF - hi) ^ (1 << 31)), flag])


# ------------------------------------------------------------------------------------------------ bucket map
def bucket_ref(rows, params):
    """(bucket [n, C] int64, taking-part [C]) of rows [n, C] under params int32 [3, >= C], the header's formula:
    value-linear where the scale's bits are a positive float: (v - key2f(klo)) * sf in fp32, truncated, clamped to
    [0, NB - 1]; key-linear elsewhere: (key(v) - klo) >> s, clamped to [0, NB - 1].  Only for scores inside the window."""
    rows, params = f32(rows), np.asarray(params, dtype=np.int32)
    C = rows.shape[1]
    klo = params[0, :C].astype(np.int64) & 0xFFFFFFFF
    sf = np.ascontiguousarray(params[1, :C]).view(np.float32)
    sh = params[2, :C].astype(np.int64)
    vlo = key2f(klo)
    with np.errstate(**_IGNORE):
        d = rows - vlo[None]
        t = d * sf[None]
        assert d.dtype == np.float32 and t.dtype == np.float32
        vb = np.clip(np.nan_to_num(np.trunc(t), nan=0.0, posinf=NB - 1, neginf=0.0), 0, NB - 1).astype(np.int64)
    kb = np.clip((keys(rows) - klo[None]) >> np.maximum(sh, 0)[None], 0, NB - 1)
    part = sh >= 0
    return np.where(part[None], np.where((sf > 0)[None], vb, kb), 0), part


def hist_ref(rows, params, W, Co, packed):
    """int32 [W, words, Co]: np.bincount of ``bucket_ref`` per taking-part cell, zero elsewhere (pads too); packed: word
    w = bucket w + (bucket w + NB/2 << 16)."""
    b, part = bucket_ref(rows, params)
    C = rows.shape[1]
    cnt = np.zeros((W * Co, NB), np.int64)
    for c in np.flatnonzero(part):
        cnt[c] = np.bincount(b[:, c], minlength=NB)
    assert C <= W * Co
    if packed:
        cnt = cnt[:, :NB // 2] | (cnt[:, NB // 2:] << 16)
    return _i32(cnt.reshape(W, Co, -1).transpose(0, 2, 1))


def unpack_ref(h, packed):
    """hist block [words, Co] (int64 or int32, non-negative halves) -> counts [Co, NB] int64."""
    h = np.asarray(h).astype(np.int64) & 0xFFFFFFFF
    return np.concatenate([h & 0xFFFF, h >> 16], 0).T.copy() if packed else h.T.copy()


# ------------------------------------------------------------------------------------------------ narrow
def narrow_ref(counts, ks):
    """counts [Co, NB], ranks ks (any order, duplicates allowed) -> (want [Co, S] int32, slot [Co, nk] int32, rnk [Co, nk]
    int32), S = nk: the bucket of rank k is the number of buckets whose cumulative count is <= k, its rank inside the bucket
    is k less the cumulative count below; a cell's distinct buckets fill its slots in ascending order (-1: unused); a cell
    without counts takes no part (every slot -1)."""
    counts = np.asarray(counts, dtype=np.int64)
    Co, nk = counts.shape[0], len(ks)
    want, slot = np.full((Co, nk), -1, np.int32), np.full((Co, nk), -1, np.int32)
    rnk = np.zeros((Co, nk), np.int32)
    for c in range(Co):
        cum = np.cumsum(counts[c])
        if cum[-1] == 0:
            continue
        b = np.array([min(int((cum <= k).sum()), NB - 1) for k in ks])
        distinct = np.unique(b)
        want[c, :len(distinct)] = distinct
        slot[c] = np.searchsorted(distinct, b)
        rnk[c] = [k - (cum[bb - 1] if bb else 0) for k, bb in zip(ks, b)]
    return want, slot, rnk


# ------------------------------------------------------------------------------------------------ memory
class Framed:
    """A view ``guard + offset`` elements into an allocation of the test's, filled with NaN (floats) or a bit pattern
    (integers): ``view`` (contiguous, the asked shape), ``alloc`` (1-D) and ``untouched()``: the frame around the view
    holds the bits it held when it was made.  ``offset`` = 1 puts the base 4 (int64: 8) bytes past a 16-byte boundary."""

    def __init__(self, shape, dtype, offset=0, device="cpu", guard=64, fill=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape)) if shape else 1
        self.alloc = torch.empty(guard + offset + n + guard + (4 - offset), dtype=dtype, device=device)
        self.alloc.fill_(fill if fill is not None else (float("nan") if dtype.is_floating_point else _FILL[dtype]))
        self.lo, self.hi = guard + offset, guard + offset + n
        self.view = self.alloc[self.lo:self.hi].view(shape)
        self._frame = self.frame()

    def put(self, x):
        self.view.copy_(torch.as_tensor(x).reshape(self.view.shape))
        return self

    def frame(self):
        raw = self.alloc.view(_INT_OF[self.alloc.dtype])
        return torch.cat([raw[:self.lo], raw[self.hi:]]).clone()

    def untouched(self):
        return torch.equal(self.frame(), self._frame)

    def bits(self):
        return self.view.view(_INT_OF[self.alloc.dtype]).clone()

    def np(self):
        return self.view.cpu().numpy()


def framed(shape, dtype, offset=0, device="cpu", guard=64, fill=None):
    return Framed(shape, dtype, offset, device, guard, fill)


def put(x, offset=0, device="cpu", dtype=None):
    """numpy array -> Framed holding it."""
    t = torch.as_tensor(np.ascontiguousarray(x))
    if dtype is not None:
        t = t.to(dtype)
    return Framed(tuple(t.shape), t.dtype, offset, device).put(t)


class Source:
    """Scores [n, cells] laid out as the sweeps address them: ``planes`` matrices [n, per], plane p ``PS`` floats behind
    the base, rows ``RS`` apart, inside a NaN-filled Framed - the gaps between rows and planes and the frame are NaN, which a
    sweep that reads them shows as a NaN flag or a wrong count.  ``src`` is the tuple ``HipOps.dist_*`` / ``DistOps`` take."""

    def __init__(self, data, planes=1, row_pad=0, plane_pad=0, offset=0, device="cpu"):
        data = f32(data)
        n, cells = data.shape
        assert cells % planes == 0
        per = cells // planes
        RS = per + row_pad
        PS = (n - 1) * RS + per + plane_pad if planes > 1 else per
        self.data, self.n, self.per, self.planes = data, n, per, planes
        self.f = Framed((planes - 1) * PS + (n - 1) * RS + per, torch.float32, offset, device)
        v = torch.as_strided(self.f.view, (planes, n, per), (PS, RS, 1))
        v.copy_(torch.from_numpy(data.reshape(n, planes, per).transpose(1, 0, 2).copy()))
        self._bits = self.f.alloc.view(torch.int32).clone()
        self.src = (self.f.view, PS, RS, planes, n, per)

    def rows(self, c0, C):
        return self.data[:, c0:c0 + C]

    def untouched(self):
        return torch.equal(self.f.alloc.view(torch.int32), self._bits)


# ------------------------------------------------------------------------------------------------ column families
FAMILIES = ("half_normal", "uniform", "two_adjacent", "consecutive_keys", "signed_zeros", "zeros_and_unit", "three_ties",
            "third_pinf", "quarter_ninf", "both_inf", "span_overflow", "subnormals", "scale_overflow", "pow2", "outlier",
            "constant", "one_nan", "all_nan", "sorted_across_ranks", "rank0_constant")


def family_columns(W, n_local, seed=0, n0=None):
    """fp32 [W * n_local, 20]: one column per family of FAMILIES; rank r holds rows [r * n_local, (r + 1) * n_local);
    ``n0``: the rows that are constant in the last family (default: rank 0's)."""
    N = W * n_local
    n0 = n_local if n0 is None else n0
    rng = np.random.default_rng(1000 * seed + 7 * N + W)
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    z = np.where(rng.random(N) < 0.5, np.float32(-0.0), np.float32(0.0))
    with np.errstate(**_IGNORE):
        cols = [
            np.abs(rng.standard_normal(N)),
            rng.uniform(-3.0, 5.0, N),
            np.where(rng.random(N) < 0.5, one, up),
            (one.view(np.int32) + rng.integers(1, 201, N).astype(np.int32)).view(np.float32),
            z,
            np.where(rng.random(N) < 0.3, z, rng.random(N)),
            rng.integers(0, 3, N),
            np.where(np.arange(N) % 3 == 0, np.inf, rng.random(N)),
            np.where(np.arange(N) % 4 == 1, -np.inf, rng.random(N)),
            np.where(np.arange(N) % 5 == 0, np.inf, np.where(np.arange(N) % 5 == 1, -np.inf, rng.standard_normal(N))),
            f32(rng.standard_normal(N)) * np.float32(2e38),
            rng.integers(-3000, 3000, N).astype(np.float32) * np.float32(2.0 ** -149),
            f32(rng.random(N)) * np.float32(1e-38),
            np.exp2(rng.uniform(-30.0, 30.0, N)),
            np.where(np.arange(N) == N // 2, 1e6, rng.random(N)),
            np.full(N, 2.5),
            np.where(np.arange(N) == N - 1, np.nan, rng.random(N)),
            np.full(N, np.nan),
            np.sort(rng.standard_normal(N)),
            np.where(np.arange(N) < n0, 0.5, rng.random(N)),
        ]
    out = np.stack([f32(c) for c in cols], 1)
    out[~np.isfinite(out[:, 10]), 10] = np.float32(3e38)              # (randn * 2e38 beyond fp32: kept finite ...)
    out[:2, 10] = (3e38, -3e38)[:N]                                     # (... and vhi - vlo overflows at every N)
    assert out.shape == (N, len(FAMILIES))
    return out


def cells(W, n_local, M=100):
    """fp32 [W * n_local, M]: cell g is family g % 20, a fresh draw every 20 cells."""
    return np.concatenate([family_columns(W, n_local, seed=s) for s in range(-(-M // len(FAMILIES)))], 1)[:, :M]


def ranks(N):
    """The ranks of ALPHA levels 0.05 .. 0.95 (numpy's method='higher' of the level ceil((N+1)(1-a))/N, where it is at most
    1) plus 0, 1, N//2, N-2, N-1; ascending, distinct."""
    ks = {0, 1, N // 2, N - 2, N - 1}
    for a in np.arange(0.05, 0.95 + 0.1, 0.1):
        q = np.ceil((N + 1) * (1 - a)) / N
        if 0.0 <= q <= 1.0:
            ks.add(int(np.ceil((N - 1) * q)))
    return sorted(k for k in ks if 0 <= k < N)


# ------------------------------------------------------------------------------------------------ checks of single sweeps
def _dev(src):
    return src[0].device


def check_window(ops, S, c0, C, W, Co, offset=0):
    """``ops.dist_window`` of the run [c0, c0 + C) of Source ``S`` == window_ref, bit for bit; returns it (numpy)."""
    win = framed((3, W * Co), torch.int32, offset, _dev(S.src))
    ops.dist_window(S.src, c0, C, W, Co, win.view)
    got = win.np()
    assert win.untouched() and S.untouched(), "a write outside the window's view"
    ref = window_ref(S.rows(c0, C), W * Co)
    assert np.array_equal(got, ref), (np.argwhere(got != ref)[:8].tolist(), c0, C, W, Co)
    return got


def check_hist(ops, S, c0, C, W, Co, params, packed, offset=0):
    """``ops.dist_hist`` into a poisoned hist: == bucket_ref + np.bincount in [W][words][Co]; every taking-part cell sums to
    n, every other cell (pads included) is zero.  Returns the counts [Cp, NB] int64."""
    dev = _dev(S.src)
    words = NB // 2 if packed else NB
    p = put(params, offset, dev)
    hist = framed((W, words, Co), torch.int32, offset, dev, fill=HIST_POISON)
    hist.view.fill_(HIST_POISON)
    ops.dist_hist(S.src, c0, C, W, Co, p.view, packed, hist.view)
    got = hist.np()
    assert hist.untouched() and p.untouched() and S.untouched(), "a write outside the histogram's view"
    counts = np.concatenate([unpack_ref(got[r], packed) for r in range(W)], 0)            # [Cp, NB]
    part = np.zeros(W * Co, bool)
    part[:C] = np.asarray(params)[2, :C] >= 0
    sums = counts.sum(1)
    assert np.array_equal(sums[part], np.full(int(part.sum()), S.n)), "a taking-part cell does not sum to n"
    assert not counts[~part].any(), "a cell that takes no part (a pad, a constant, a NaN cell) is not zero"
    ref = hist_ref(S.rows(c0, C), params, W, Co, packed)
    assert np.array_equal(got, ref), f"not bucket_ref + np.bincount at [rank, word, cell] {np.argwhere(got != ref)[:8].tolist()}"
    return counts


def check_partition(ops, S, c0, C, W, Co, params, counts, offset=0):
    """The partition property, which does not restate the map: collect EVERY occupied bucket of every cell (four calls of
    64 slots), sort each list, concatenate in bucket order: the sorted column, key for key.  Shows that map, histogram
    and collect agree and that the map is monotone."""
    dev = _dev(S.src)
    Cp = W * Co
    p = put(params, offset, dev)
    rows = S.rows(c0, C)
    part = np.flatnonzero(np.asarray(params)[2, :C] >= 0)
    trip_cell, trip_bucket, trip_key = [], [], []
    for j in range(NB // MAX_SLOTS):
        want = np.full((Cp, MAX_SLOTS), -1, np.int32)
        cnt = np.zeros((Cp, MAX_SLOTS), np.int32)
        for c in part:
            occ = np.flatnonzero(counts[c])[j * MAX_SLOTS:(j + 1) * MAX_SLOTS]
            want[c, :len(occ)] = occ
            cnt[c, :len(occ)] = counts[c, occ]
        off = (np.cumsum(cnt.reshape(-1), dtype=np.int64) - cnt.reshape(-1)).reshape(Cp, MAX_SLOTS)
        total = int(cnt.sum())
        send = framed(total, torch.float32, offset, dev)
        w_, c_, o_ = put(want, offset, dev), put(cnt, offset, dev), put(off, offset, dev)
        ops.dist_collect(S.src, c0, C, W, Co, p.view, w_.view, c_.view, o_.view, send.view)
        got = send.np()
        assert send.untouched() and all(x.untouched() for x in (w_, c_, o_, p)) and S.untouched()
        assert not np.isnan(got).any(), "a list entry was never written"
        trip_cell.append(np.repeat(np.repeat(np.arange(Cp), MAX_SLOTS), cnt.reshape(-1)))
        trip_bucket.append(np.repeat(want.reshape(-1), cnt.reshape(-1)))
        trip_key.append(keys(got))
    cell, bucket, key = np.concatenate(trip_cell), np.concatenate(trip_bucket), np.concatenate(trip_key)
    order = np.lexsort((key, bucket, cell))
    ref = np.sort(keys(rows[:, part]), axis=0).T.reshape(-1)                                # by cell, then key
    assert len(key) == len(ref), (len(key), len(ref))
    assert np.array_equal(np.repeat(part, S.n), cell[order])
    assert np.array_equal(key[order], ref), "sorted lists in bucket order are not the sorted column"


def check_collect(ops, S, c0, C, W, Co, params, want, short=(), offset=0):
    """``ops.dist_collect`` of the buckets want [Cp, S] on their own: every list, sorted, holds the keys ``bucket_ref`` puts in
    its bucket; a sentinel (NaN) sits behind every list and stays; the (cell, slot) pairs of ``short`` get a ``cnt`` one
    below what the bucket holds: such a list is filled with scores of its bucket and nothing is written past it."""
    dev = _dev(S.src)
    rows = S.rows(c0, C)
    b, part = bucket_ref(rows, params)
    Cp, nS = want.shape
    held = np.zeros((Cp, nS), np.int64)
    for c in np.flatnonzero(part):
        for s in range(nS):
            if want[c, s] >= 0:
                held[c, s] = (b[:, c] == want[c, s]).sum()
    cnt = held.copy()
    for c, s in short:
        assert held[c, s] > 1
        cnt[c, s] -= 1
    gap = cnt.reshape(-1) + 1                                                              # one sentinel behind every list
    off = (np.cumsum(gap) - gap).reshape(Cp, nS)
    send = framed(int(gap.sum()), torch.float32, offset, dev)
    p, w_, c_, o_ = (put(x, offset, dev) for x in (params, want, cnt.astype(np.int32), off.astype(np.int64)))
    ops.dist_collect(S.src, c0, C, W, Co, p.view, w_.view, c_.view, o_.view, send.view)
    got = send.np()
    assert send.untouched() and all(x.untouched() for x in (w_, c_, o_, p)) and S.untouched()
    written = ~np.isnan(got)
    expect = np.ones(len(got), bool)
    expect[off.reshape(-1) + cnt.reshape(-1)] = False
    assert np.array_equal(written, expect), "a sentinel behind a list was overwritten, or a list entry never written"
    for c in range(Cp):
        for s in range(nS):
            n = int(cnt[c, s])
            if not n:
                continue
            lst = np.sort(keys(got[off[c, s]:off[c, s] + n]))
            full = np.sort(keys(rows[b[:, c] == want[c, s], c]))
            if (c, s) in short:                                     # a sub-multiset of the bucket's keys
                u, k = np.unique(lst, return_counts=True)
                uf, kf = np.unique(full, return_counts=True)
                assert np.isin(u, uf).all() and (k <= kf[np.searchsorted(uf, u)]).all(), (c, s)
            else:
                assert np.array_equal(lst, full), (c, s)
    return cnt


PICK_SENTINEL = np.float32(-123.25)


def check_pick(ops, lists, asks, W, nk, dev="cpu", offset=0, cap=PICK_CAP):
    """``ops.dist_pick`` on hand-made lists.  ``lists[co][s]`` = the W segments (fp32 arrays, some empty) of cell co's slot
    s; ``asks[co]`` = [(slot, rank), ...] (at most nk; slot -1: nothing to pick).  The reference is np.sort of the
    concatenated segments' keys; an output whose slot is -1 or whose list is longer than ``cap`` keeps its sentinel.
    Outputs are compared on bits (-0.0 is not +0.0)."""
    Co, nS = len(lists), len(lists[0])
    cnt = np.zeros((W, Co, nS), np.int32)
    for co in range(Co):
        for s in range(nS):
            assert len(lists[co][s]) == W
            for w in range(W):
                cnt[w, co, s] = len(lists[co][s][w])
    flat = cnt.reshape(-1).astype(np.int64)
    off = (np.cumsum(flat) - flat).reshape(W, Co, nS)
    vals = np.full(int(flat.sum()), np.nan, np.float32)
    for co in range(Co):
        for s in range(nS):
            for w in range(W):
                vals[off[w, co, s]:off[w, co, s] + cnt[w, co, s]] = lists[co][s][w]
    slot = np.full((Co, nk), -1, np.int32)
    rnk = np.zeros((Co, nk), np.int32)
    ref = np.full((nk, Co), PICK_SENTINEL, np.float32)
    for co in range(Co):
        for j, (s, r) in enumerate(asks[co]):
            slot[co, j], rnk[co, j] = s, r
            if s >= 0:
                k = np.sort(keys(np.concatenate([f32(x) for x in lists[co][s]])))
                if 0 < len(k) <= cap:
                    ref[j, co] = key2f(k[r])
    v_, c_, o_, s_, r_ = (put(x, offset, dev) for x in (vals, cnt, off, slot, rnk))
    out = framed((nk, Co), torch.float32, offset, dev)
    out.view.fill_(float(PICK_SENTINEL))
    ops.dist_pick(v_.view, c_.view, o_.view, s_.view, r_.view, out.view)
    got = out.np()
    assert out.untouched() and all(x.untouched() for x in (v_, c_, o_, s_, r_)), "a write outside the pick's output"
    bad = np.argwhere(got.view(np.int32) != ref.view(np.int32))
    assert bad.size == 0, (bad[:8].tolist(), [float(got[tuple(i)]) for i in bad[:8]], [float(ref[tuple(i)]) for i in bad[:8]])
    return got


def split(lst, W, rng, empty=()):
    """A list cut into W segments at random places, the segments named in ``empty`` left empty."""
    live = [w for w in range(W) if w not in empty]
    cuts = np.sort(rng.integers(0, len(lst) + 1, len(live) - 1))
    parts = np.split(f32(lst), cuts)
    out = [np.zeros(0, np.float32) for _ in range(W)]
    for w, p in zip(live, parts):
        out[w] = p
    return out


def pick_cases(seed=5):
    """{name: (lists, asks, W, nk)} for ``check_pick``: see tests/DIST_TESTS.md for the seam each one sits on."""
    rng = np.random.default_rng(seed)
    cases = {}
    # list lengths around the wave (64) and the cap (2048; 2049 keeps its sentinel), three segments of which one is empty;
    # slot 1 is a short second list; the last ask has slot -1
    lens = (1, 63, 64, 65, 2047, 2048, 2049)
    lists, asks = [], []
    for L in lens:
        big = rng.standard_normal(L).astype(np.float32)
        big[::7] = big[0]                                                              # ties inside the long list too
        lists.append([split(big, 3, rng, empty=(1,)), split(np.arange(5, 0, -1), 3, rng, empty=(0,))])
        r0 = sorted({0, L - 1, L // 2, L // 7, min(L - 1, 63), min(L - 1, 64)})
        asks.append(([(0, r) for r in r0] + [(1, 0), (1, 4), (1, 2)])[:9] + [(-1, 0)])
    cases["lengths"] = (lists, asks, 3, 10)
    # three distinct values, ranks on every tie boundary, all asks in one slot; signed zeros compared on bits
    tied = np.array([1.0] * 5 + [2.0] * 4 + [3.0] * 6, np.float32)
    zeros = np.array([-0.0] * 3 + [0.0] * 4, np.float32)
    lists = [[split(rng.permutation(tied), 2, rng)], [split(rng.permutation(zeros), 2, rng)]]
    asks = [[(0, r) for r in (0, 4, 5, 8, 9, 14, 3, 6, 10, 13)], [(0, r) for r in (0, 2, 3, 6, 1, 4, 5, 2, 3, 0)]]
    cases["ties"] = (lists, asks, 2, 10)
    # 64 segments, most of them empty, 64 slots, 64 ranks
    lists, asks = [], []
    for co in range(3):
        cell = []
        for s in range(64):
            segs = [np.zeros(0, np.float32) for _ in range(64)]
            for w in rng.choice(64, size=int(rng.integers(1, 6)), replace=False):
                segs[w] = rng.integers(-4, 5, int(rng.integers(1, 4))).astype(np.float32)
            cell.append(segs)
        lists.append(cell)
        asks.append([(s, int(rng.integers(sum(len(x) for x in cell[s])))) for s in rng.integers(0, 64, 64)])
    cases["wide"] = (lists, asks, 64, 64)
    cases["one"] = ([[[np.array([7.5], np.float32)]]], [[(0, 0)]], 1, 1)
    # nothing received: vals is None, every slot -1
    cases["empty"] = ([[[np.zeros(0, np.float32)] * 2] * 2] * 3, [[(-1, 0)] * 2] * 3, 2, 2)
    return cases


# ------------------------------------------------------------------------------------------------ the four sweeps together
def simulate(shards, ks, ops, Co, c0=0, packed=None, offset=0):
    """W ranks in ONE process, no process group: what ``pipeline._marginal_histogram`` does in one run, with the collectives
    replaced by numpy and the narrowing by ``narrow_ref``.  ``shards``: W Sources of equal shape (rank r's local scores); the
    run is the cells [c0, cells) padded to W * Co.  Every table a sweep reads or writes is Framed (``offset`` elements off a
    16-byte boundary) and checked; the histogram is pre-filled with a bit pattern.  There is NO fallback branch: a list
    longer than PICK_CAP is an assertion.  Returns (q-hats [len(ks), C] numpy, the intermediate tables)."""
    from cp_pre_amd import pipeline
    W = len(shards)
    dev = _dev(shards[0].src)
    n, M = shards[0].n, shards[0].planes * shards[0].per
    C, Cp, N, nk = M - c0, W * Co, W * shards[0].n, len(ks)
    assert 0 < C <= Cp and nk <= MAX_SLOTS
    packed = N <= 32767 if packed is None else packed
    words = NB // 2 if packed else NB
    # 1. window, 2. MIN-reduce -> params
    wins = []
    for S in shards:
        f = framed((3, Cp), torch.int32, offset, dev)
        ops.dist_window(S.src, c0, C, W, Co, f.view)
        assert f.untouched() and S.untouched()
        wins.append(f.view.clone())
    win = torch.stack(wins).amin(0)
    params_t, nan, const, vconst = pipeline._dist_params(win)
    params = params_t.cpu().numpy()
    pf = put(params, offset, dev)
    # 3. histogram into a poisoned table, 4. sum, narrow every owner's block
    hists = []
    for S in shards:
        f = framed((W, words, Co), torch.int32, offset, dev, fill=HIST_POISON)
        f.view.fill_(HIST_POISON)
        ops.dist_hist(S.src, c0, C, W, Co, pf.view, packed, f.view)
        assert f.untouched() and S.untouched()
        hists.append(f.np().astype(np.int64))
    total = np.sum(hists, axis=0)                                                            # [W, words, Co]
    owned = [unpack_ref(total[o], packed) for o in range(W)]
    narrowed = [narrow_ref(cnt, ks) for cnt in owned]
    want = np.concatenate([w for w, _, _ in narrowed], 0)                                   # [Cp, S]
    # 5. collect on every shard: the local counts of the wanted buckets are read off its own histogram
    cnt_out, send = [], []
    wf = put(want, offset, dev)
    for S, h in zip(shards, hists):
        local = np.concatenate([unpack_ref(h[o], packed) for o in range(W)], 0)           # [Cp, NB]
        cnt = np.where(want >= 0, np.take_along_axis(local, np.maximum(want, 0).astype(np.int64), 1), 0)
        off = (np.cumsum(cnt.reshape(-1)) - cnt.reshape(-1)).reshape(Cp, nk)
        f = framed(int(cnt.sum()), torch.float32, offset, dev)
        cf, of = put(cnt.astype(np.int32), offset, dev), put(off.astype(np.int64), offset, dev)
        ops.dist_collect(S.src, c0, C, W, Co, pf.view, wf.view, cf.view, of.view, f.view)
        assert f.untouched() and cf.untouched() and of.untouched() and S.untouched()
        got = f.np()
        assert not np.isnan(got).any(), "a list entry was never written"
        cnt_out.append(cnt)
        send.append(got)
    assert wf.untouched() and pf.untouched()
    # 6. every owner's lists as [W, Co, S] segments -> pick; 7. const and NaN cells patched as the protocol does
    q = np.empty((nk, Cp), np.float32)
    longest = 0
    for o in range(W):
        blk = slice(o * Co, (o + 1) * Co)
        cnt_in = np.stack([c[blk] for c in cnt_out])                                        # [W, Co, S]
        starts = [int(c[:o * Co].sum()) for c in cnt_out]
        recv = np.concatenate([s[a:a + int(c[blk].sum())] for s, a, c in zip(send, starts, cnt_out)])
        flat = cnt_in.reshape(-1).astype(np.int64)
        off_in = (np.cumsum(flat) - flat).reshape(W, Co, nk)
        longest = max(longest, int(cnt_in.sum(0).max()))
        assert longest <= PICK_CAP, "a list longer than the pick holds: the harness has no fallback"
        _, slot, rnk = narrowed[o]
        out = framed((nk, Co), torch.float32, offset, dev)
        tabs = [put(x, offset, dev) for x in (recv, cnt_in.astype(np.int32), off_in, slot, rnk)]
        ops.dist_pick(tabs[0].view, tabs[1].view, tabs[2].view, tabs[3].view, tabs[4].view, out.view)
        assert out.untouched() and all(t.untouched() for t in tabs)
        q[:, blk] = out.np()
    const, nan, vconst = const.cpu().numpy(), nan.cpu().numpy(), vconst.cpu().numpy()
    q = np.where(const[None], vconst[None], q)
    q = np.where(nan[None], np.float32(np.nan), q).astype(np.float32)
    tables = dict(win=win.cpu().numpy(), params=params, hists=hists, owned=owned, want=want, cnt_out=cnt_out, longest=longest,
                  packed=packed)
    return q[:, :C], tables


def check_simulate(ops, data, W, ks, Co, dev="cpu", c0=0, packed=None, offset=0):
    """``simulate`` on data [W * n_local, M] split by rank == np.sort(all shards)[ks] per column, bit for bit, NaN where a
    column holds one.  No cell is left out.  Returns (q, tables)."""
    n_local = data.shape[0] // W
    shards = [Source(data[r * n_local:(r + 1) * n_local], offset=offset, device=dev) for r in range(W)]
    q, tables = simulate(shards, ks, ops, Co, c0, packed, offset)
    ident(q, sort_ref(data[:, c0:], ks))
    return q, tables
