"""What tests/test_ode_ref_cpu.py and tests/test_gpu_ode_seams.py share: the numpy references of the ODE stencil, the fused
residual and the kernel gradient (cp_pre_amd/csrc/ode_march.hip), the conditions under which small-integer data make fp32
arithmetic exact, the launch plans restated, and the memory the GPU tests hand to the library (framed outputs, strided
inputs with NaN wherever no element lies).  tests/ODE_TESTS.md says which branch each shape reaches."""
import collections

import numpy as np
import torch

U24, U53 = 2.0 ** -24, 2.0 ** -53
ODE_BLOCK, ODE_V, WGRAD_BLOCKS, WG_BLOCK = 256, 4, 1024, 256      # ode_march.hip / cp_pre_ode.h
MAX_TAPS, MAX_TERMS = 7, 6
GUARD = 64
_IGNORE = dict(invalid="ignore", over="ignore")


# ------------------------------------------------------------------------------------------------ references
def conv_ref(x, taps, dtype=np.float64):
    """(K * x)[b, t] = sum_j taps[j] x[b, t + j - k//2], x zero outside [0, Nt), the taps summed in order, in ``dtype``
    (int64 for integer data, float64 otherwise).  Every tap is multiplied, zero taps and the zero padding included, so a NaN
    or inf spreads as in the kernel."""
    x, taps = np.asarray(x, dtype), np.asarray(taps, dtype)
    bs, nt = x.shape
    k = taps.size
    h = k // 2
    pad = np.zeros((bs, nt + 2 * h), dtype)
    pad[:, h:h + nt] = x
    out = np.zeros((bs, nt), dtype)
    with np.errstate(**_IGNORE):
        for j in range(k):
            out = out + taps[j] * pad[:, j:j + nt]
    return out


def residual_ref(terms, dtype=np.float64):
    """sum_i c_i[t] (K_i * x_i)[b, t], term by term in the order given; ``terms`` = [(x [BS, Nt], taps, c [Nt] or None)]."""
    out = None
    with np.errstate(**_IGNORE):
        for x, taps, c in terms:
            d = conv_ref(x, taps, dtype)
            if c is not None:
                d = np.asarray(c, dtype)[None, :] * d
            out = d if out is None else out + d
    return out


def magnitude(terms):
    """S[b, t] = sum_i |c_i[t]| sum_j |w_ij x_i[b, t + j - k/2]| in float64 (non-finite values counted as 0): the yardstick of
    the per-element bound and of the exactness condition."""
    return residual_ref([(np.abs(np.nan_to_num(np.asarray(x, np.float64), nan=0.0, posinf=0.0, neginf=0.0)), np.abs(taps),
                          None if c is None else np.abs(c)) for x, taps, c in terms])


def assert_exact_f32(terms):
    """Integer data whose sums of magnitudes stay below 2^24: every partial sum is an integer fp32 holds, so the result is
    the same in any order, with or without fma contraction."""
    for x, taps, c in terms:
        for v in (x, taps) + (() if c is None else (c,)):
            v = np.asarray(v, np.float64)
            fin = v[np.isfinite(v)]
            assert np.array_equal(fin, np.rint(fin)), "not integer data"
    s = magnitude(terms)
    assert s.size == 0 or s.max() < 2 ** 24, s.max()


def residual_tol(terms):
    """(k_max + nterms + 2) 2^-24 S[b, t]: k roundings of the fma chain, one of the coefficient, at most nterms of the sum
    (two units for second-order terms); holds whether or not c*d + acc is contracted."""
    kmax = max(len(t[1]) for t in terms)
    return (kmax + len(terms) + 2) * U24 * magnitude(terms)


def wgrad_ref(x, g, k, dtype=np.float64):
    """dK[j] = sum_{b, t} g[b, t] x[b, t + j - k//2] in ``dtype``."""
    x, g = np.asarray(x, dtype), np.asarray(g, dtype)
    bs, nt = x.shape
    h = k // 2
    pad = np.zeros((bs, nt + 2 * h), dtype)
    pad[:, h:h + nt] = x
    return np.array([(g * pad[:, j:j + nt]).sum() for j in range(k)], dtype)


def wgrad_magnitude(x, g, k):
    return wgrad_ref(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(g, np.float64)), k)


def assert_exact_wgrad(x, g, k):
    """integer x and g with sum |g x| < 2^24: the fp64 partials, their sum and its fp32 rounding are all exact"""
    for v in (x, g):
        assert np.array_equal(np.asarray(v, np.float64), np.rint(v)), "not integer data"
    s = wgrad_magnitude(x, g, k)
    assert s.max() < 2 ** 24, s.max()


def wgrad_tol(x, g, k):
    """n 2^-53 sum |g x| + 2^-24 |ref|, n = BS Nt: products of fp32 values are exact in fp64, so any order of n fp64
    additions meets the first term; the second is the rounding of the result to fp32."""
    n = np.asarray(x).size
    return n * U53 * wgrad_magnitude(x, g, k) + U24 * np.abs(wgrad_ref(x, g, k))


# ------------------------------------------------------------------------------------------------ comparison
def same_f32(got, ref):
    """every element equal: any NaN equals any NaN, +-inf by sign, a zero of either sign equals 0, nothing tolerated"""
    got = np.asarray(got, np.float32).reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    with np.errstate(**_IGNORE):
        ok = (got.astype(np.float64) == ref) | (np.isnan(got) & np.isnan(ref))
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), ref[bad[:8]].tolist())


def footprint(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf"""
    a = np.asarray(a)
    return np.isnan(a) * 1 + np.isposinf(a) * 2 + np.isneginf(a) * 3


def within(got, ref, tol):
    """|got - ref| <= tol element by element; returns the largest fraction of the bound used (0 where ref == got)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref)
    bad = np.flatnonzero(~(err <= tol).reshape(-1))
    assert bad.size == 0, (bad.size, bad[:8].tolist(), got.reshape(-1)[bad[:8]].tolist(), ref.reshape(-1)[bad[:8]].tolist(),
                           np.broadcast_to(tol, got.shape).reshape(-1)[bad[:8]].tolist())
    pos = np.broadcast_to(tol, got.shape) > 0
    return float((err[pos] / np.broadcast_to(tol, got.shape)[pos]).max()) if pos.any() else 0.0


# ------------------------------------------------------------------------------------------------ the launch plans
OdePlan = collections.namedtuple("OdePlan", "total blocks threads last_run cross_v multi first_cross")


def plan(bs, nt):
    """The work split of ``ode_residual_kernel`` restated: ``blocks`` of 256 threads x 4 outputs, ``threads`` with work, the
    run length of the last one, the set ``cross_v`` of v in 1..3 at which some thread's run enters the next row (where the
    window is reloaded by ``t == 0``), ``multi`` the most crossings inside one run and ``first_cross`` the first
    (thread, v) that crosses.  Only ever used to assert which branch a shape reaches."""
    total = bs * nt
    if total == 0:
        return OdePlan(0, 0, 0, 0, (), 0, None)
    threads = (total + ODE_V - 1) // ODE_V
    cross, multi, first = set(), 0, None
    for th in range(threads):
        n = 0
        for v in range(1, ODE_V):
            e = th * ODE_V + v
            if e < total and e % nt == 0:
                cross.add(v)
                n += 1
                if first is None:
                    first = (th, v)
        multi = max(multi, n)
    per_block = ODE_BLOCK * ODE_V
    return OdePlan(total, (total + per_block - 1) // per_block, threads, total - ODE_V * (threads - 1), tuple(sorted(cross)),
                   multi, first)


WgPlan = collections.namedtuple("WgPlan", "total per nonempty second rows_cross")


def wgrad_plan(bs, nt):
    """``pre_ode_wgrad_f32`` restated: 1024 fixed block ranges of ``per`` = ceil(total / 1024) flat elements, of which
    ``nonempty`` hold any; ``second``: a thread of a full block takes a second element (per > 256); ``rows_cross``: some
    block range holds elements of more than one row."""
    total = bs * nt
    per = (total + WGRAD_BLOCKS - 1) // WGRAD_BLOCKS
    nonempty = (total + per - 1) // per if per else 0
    cross = any((b * per) // nt != (min((b + 1) * per, total) - 1) // nt for b in range(nonempty)) if nt else False
    return WgPlan(total, per, nonempty, per > WG_BLOCK, cross)


# (BS, Nt) of the residual table of tests/ODE_TESTS.md: what each row claims of its plan
TABLE = {
    (1, 1): dict(total=1, blocks=1, threads=1, last_run=1, cross_v=()),
    (3, 1): dict(total=3, last_run=3, cross_v=(1, 2), multi=2),
    (4, 1): dict(total=4, last_run=4, cross_v=(1, 2, 3), multi=3),
    (5, 1): dict(total=5, threads=2, last_run=1, multi=3),
    (1023, 1): dict(blocks=1, threads=256, last_run=3),
    (1024, 1): dict(blocks=1, threads=256, last_run=4),
    (1025, 1): dict(blocks=2, threads=257, last_run=1),
    (2049, 1): dict(blocks=3, threads=513, last_run=1),
    (1, 2): dict(total=2, last_run=2, cross_v=()),
    (512, 2): dict(total=1024, blocks=1, cross_v=(2,), multi=1),
    (513, 2): dict(total=1026, blocks=2, last_run=2),
    (1, 3): dict(total=3, last_run=3, cross_v=()),
    (341, 3): dict(total=1023, blocks=1, last_run=3, cross_v=(1, 2, 3), multi=1, first_cross=(0, 3)),
    (683, 3): dict(total=2049, blocks=3, last_run=1, cross_v=(1, 2, 3)),
    (1, 4): dict(total=4, cross_v=()),
    (256, 4): dict(total=1024, blocks=1, cross_v=()),
    (1, 5): dict(total=5, threads=2, last_run=1, cross_v=()),
    (3, 5): dict(total=15, last_run=3, cross_v=(1, 2), first_cross=(1, 1)),
    (205, 5): dict(total=1025, blocks=2, last_run=1, cross_v=(1, 2, 3)),
    (171, 6): dict(total=1026, blocks=2, last_run=2, cross_v=(2,)),
    (5, 7): dict(total=35, last_run=3, cross_v=(1, 2, 3), first_cross=(1, 3)),
    (147, 7): dict(total=1029, blocks=2, last_run=1, cross_v=(1, 2, 3)),
    (128, 8): dict(total=1024, blocks=1, cross_v=()),
    (129, 8): dict(total=1032, blocks=2, last_run=4, cross_v=()),
    (1, 1023): dict(total=1023, blocks=1, last_run=3, cross_v=()),
    (2, 1023): dict(total=2046, blocks=2, last_run=2, cross_v=(3,), first_cross=(255, 3)),
    (3, 1023): dict(total=3069, blocks=3, last_run=1, cross_v=(2, 3)),
    (1, 1025): dict(blocks=2, last_run=1, cross_v=()),
    (1, 2049): dict(blocks=3, last_run=1, cross_v=()),
}
# (BS, Nt) of the wgrad table
WGRAD_TABLE = {
    (1, 1): dict(total=1, per=1, nonempty=1, second=False),
    (1023, 1): dict(per=1, nonempty=1023),
    (1, 1023): dict(per=1, nonempty=1023, rows_cross=False),
    (1024, 1): dict(per=1, nonempty=1024),
    (512, 2): dict(per=1, nonempty=1024),
    (1025, 1): dict(per=2, nonempty=513),
    (147, 7): dict(total=1029, per=2, nonempty=515, rows_cross=True),
    (2, 1023): dict(total=2046, per=2, nonempty=1023, rows_cross=True),
    (262145, 1): dict(per=257, nonempty=1021, second=True, rows_cross=True),
    (131072, 2): dict(total=262144, per=256, nonempty=1024, second=False),
    (37449, 7): dict(total=262143, per=256, nonempty=1024, second=False, rows_cross=True),
    (2405, 109): dict(total=262145, per=257, nonempty=1021, second=True, rows_cross=True),
}
LARGEST = 262145                                          # elements of the largest operand of any test


def assert_plan(bs, nt):
    p = plan(bs, nt)
    for key, want in TABLE[(bs, nt)].items():
        assert getattr(p, key) == want, ((bs, nt), key, p)
    return p


def assert_wgrad_plan(bs, nt):
    p = wgrad_plan(bs, nt)
    for key, want in WGRAD_TABLE[(bs, nt)].items():
        assert getattr(p, key) == want, ((bs, nt), key, p)
    return p


# ------------------------------------------------------------------------------------------------ memory
_INT_OF = {torch.float32: torch.int32, torch.float64: torch.int64}


class Framed:
    """The elements ``idx`` (offsets from the view's origin, any order, all distinct) of a view that starts ``GUARD + offset``
    elements into an allocation of the test's, filled with NaN.  ``lo`` .. ``hi`` is the span the view addresses; everything
    of the allocation that is not an element of the view - the guards and the gaps of a strided view - is the frame, which
    ``untouched`` compares bit for bit with what it held.  ``ptr`` is the address of offset 0 of the view."""

    def __init__(self, idx, dtype=torch.float32, offset=0, device=None):
        idx = np.asarray(idx, np.int64).reshape(-1)
        assert 0 <= offset < GUARD
        lo, hi = (int(idx.min()), int(idx.max()) + 1) if idx.size else (0, 0)
        assert np.unique(idx).size == idx.size, "an output view that overlaps itself"
        self.origin = GUARD + offset - lo
        self.alloc = torch.full((GUARD + offset + (hi - lo) + GUARD,), float("nan"), dtype=dtype, device=device)
        self.idx = torch.from_numpy(idx + self.origin).to(device)
        self.mask = torch.ones(self.alloc.numel(), dtype=torch.bool, device=device)
        self.mask[self.idx] = False
        self._frame = self.frame()

    @property
    def ptr(self):
        return self.alloc.data_ptr() + self.origin * self.alloc.element_size()

    def set(self, values):
        self.alloc[self.idx] = torch.as_tensor(np.asarray(values).reshape(-1)).to(self.alloc.dtype).to(self.alloc.device)
        return self

    def get(self):
        return self.alloc[self.idx].cpu().numpy()

    def frame(self):
        return self.alloc.view(_INT_OF[self.alloc.dtype])[self.mask].clone()

    def untouched(self):
        return torch.equal(self.frame(), self._frame)

    def all_nan_bits(self):
        """nothing of the allocation, view included, was written (a refused or empty call)"""
        fresh = torch.full_like(self.alloc, float("nan"))
        return torch.equal(self.alloc.view(_INT_OF[self.alloc.dtype]), fresh.view(_INT_OF[self.alloc.dtype]))


def layout(kind, bs, nt):
    """(sB, sT) element strides of a [BS, Nt] view laid out as ``kind``; the offsets of its elements follow from them."""
    if kind == "dense":
        return nt, 1
    if kind == "padded":                                   # row-padded: pipeline.row_padded's pitch
        return nt + 64, 1
    if kind == "pitch3":                                   # three NaN between rows: a halo read past a row end meets one
        return nt + 3, 1
    if kind.startswith("comp"):                            # component c of a [BS, Nt, S] state: "comp31" is S = 3, c = 1
        s = int(kind[4])
        return nt * s, s
    if kind == "transposed":                               # a [Nt, BS] buffer seen as [BS, Nt]
        return 1, bs
    if kind == "negB":
        return -nt, 1
    if kind == "negT":
        return nt, -1
    if kind == "negBT":
        return -(nt + 2), -1
    if kind == "zeroB":                                    # one row broadcast over the batch (inputs only)
        return 0, 1
    raise ValueError(kind)


def offsets(bs, nt, sB, sT):
    return (np.arange(bs, dtype=np.int64)[:, None] * sB + np.arange(nt, dtype=np.int64)[None, :] * sT)


class Source:
    """A [BS, Nt] input where a kernel reads it: element (b, t) at ``ptr + (b sB + t sT) * itemsize`` of a device buffer that
    is NaN wherever no element of the view lies, so that a read beside the view, or into the next row in place of the zero
    padding, turns an output NaN.  ``data`` is what the view holds (for ``zeroB`` row 0 repeated)."""

    def __init__(self, data, kind="dense", device=None, dtype=np.float32, lead=0):
        data = np.asarray(data, dtype)
        bs, nt = data.shape
        self.kind, self.sB, self.sT = kind, *layout(kind, bs, nt)
        if kind == "zeroB":
            data = np.repeat(data[:1], bs, 0)
        off = offsets(bs, nt, self.sB, self.sT)
        lo = int(off.min()) if off.size else 0
        span = int(off.max()) + 1 - lo if off.size else 1
        self.origin = lead - lo                            # ``lead`` NaN in front: a component view starts inside its tensor
        buf = np.full(lead + span + (int(kind[4]) - 1 if kind.startswith("comp") else 0), np.nan, dtype)
        if off.size:
            buf[off + self.origin] = data                  # (zeroB: the same row written BS times)
        self.data, self.host = data, buf
        self.dev = torch.from_numpy(buf).to(device) if device is not None else None

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.origin * self.dev.element_size()

    @property
    def strides(self):
        return self.sB, self.sT


# ------------------------------------------------------------------------------------------------ data
def ints(rng, lo, hi, *shape):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def int_taps(rng, k, nonzero=True):
    """k integer taps in [-3, 3]; ``nonzero``: none of them 0, so that every tap's read shows"""
    t = rng.integers(-3, 4, size=k)
    if nonzero:
        t[t == 0] = 2
    return t.astype(np.float32)


def coeff_row(nt, seed=0):
    """integer coefficients in [-4, 4], never 0, different at neighbouring t: one kept from before a row crossing shows"""
    t = np.arange(nt) + seed
    c = (t % 4) + 1.0
    c[(t // 4) % 2 == 1] *= -1
    return c.astype(np.float32)
