"""Plain numpy references of the joint-CP calibration kernels (cp_pre_amd/csrc/calib.hip) and the memory layouts their
tests use (tests/test_gpu_calib_seams.py on the GPU, tests/test_calib_ref_cpu.py for the references themselves; the page
that goes with them is tests/CALIB_TESTS.md).  No GPU is needed to import or call anything here and nothing of
cp_pre_amd is imported: ``embed`` lays out memory with torch alone.

Every reference works in the number format of the kernel it describes: fp32 numpy arrays stay fp32 (numpy's fp32
+, -, *, /, sqrt are single correctly rounded IEEE operations, subnormals included), fp64 where the kernel is fp64."""
import numpy as np
import torch

NAN_BITS = 0x7FC00000
F32_MIN_NORMAL = np.float32(1.17549435e-38)
C_THR = np.float32(0.99999905)                         # 1 - 2^-20, exact in fp32
_IGNORE = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def bits32(x):
    """int32 bit patterns of an fp32 array (a copy), every NaN as the canonical quiet NaN the kernels write."""
    x = f32(x).copy()
    b = x.view(np.int32)
    b[np.isnan(x)] = NAN_BITS
    return b


# ------------------------------------------------------------------------------------------------ select, |a-b|
def kth_ref(s, ks):
    """``np.sort(s)[ks]`` in fp32; NaN for every rank if any element is NaN of either sign, as np.quantile gives.
    The sort is by the total order of the bit patterns (-0.0 before +0.0), which is np.sort's order wherever np.sort
    has one: np.sort leaves the order of -0.0 and +0.0 open, the kernel's radix keys do not."""
    s = f32(s).reshape(-1)
    ks = np.asarray(ks, dtype=np.int64)
    if np.isnan(s).any():
        return np.full(ks.shape, np.nan, np.float32)
    u = s.view(np.uint32)
    key = np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key = np.sort(key)[ks]
    back = np.where(key >> 31 != 0, key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32)
    return back.view(np.float32)


def absdiff_ref(a, b=None):
    with np.errstate(**_IGNORE):
        return np.abs(f32(a) - f32(b)) if b is not None else np.abs(f32(a))


# ------------------------------------------------------------------------------------------------ modulation
def std_seq_ref(a, b=None, eps=0.0):
    """The sequential fp32 recipe calib.hip states for std over axis 0 of [n, M]: s = s + x[i] row by row, mean = s / n,
    acc = acc + (x[i] - mean)^2 row by row, sqrt(acc / n) + eps - one fp32 rounding per operation, in this order.  (An
    explicit loop over rows: np.std / np.add.reduce may sum a contiguous axis pairwise.)"""
    a = f32(a)
    n = a.shape[0]
    with np.errstate(**_IGNORE):
        x = a - f32(b) if b is not None else a
        x = x.reshape(n, -1)
        s = np.zeros(x.shape[1], np.float32)
        for i in range(n):
            s = s + x[i]
        mean = s / np.float32(n)
        acc = np.zeros(x.shape[1], np.float32)
        for i in range(n):
            d = x[i] - mean
            dd = d * d
            acc = acc + dd
        out = np.sqrt(acc / np.float32(n)) + np.float32(eps)
    assert out.dtype == np.float32
    return out


def moments_ref(a, b=None):
    """(sum, sum of squares) over axis 0 in fp64 of the fp32 data (a - b rounded to fp32 first, as the kernel forms it)."""
    with np.errstate(**_IGNORE):
        x = (f32(a) - f32(b) if b is not None else f32(a)).astype(np.float64)
        x = x.reshape(x.shape[0], -1)
        return x.sum(0), (x * x).sum(0)


def std64_ref(a, b=None):
    """Two-pass population std in fp64 of the fp32 data."""
    with np.errstate(**_IGNORE):
        x = (f32(a) - f32(b) if b is not None else f32(a)).astype(np.float64)
        return np.std(x.reshape(x.shape[0], -1), axis=0)


def std_from_moments_ref(s, q, n, eps=0.0):
    """pre_std_from_moments_f32 restated: fp64 E[x^2] - mean^2, clamped at 0 (NaN stays), sqrt, one rounding to fp32, + eps."""
    with np.errstate(**_IGNORE):
        mean = np.asarray(s, np.float64) / float(n)
        var = np.asarray(q, np.float64) / float(n) - mean * mean
        var = np.where(var < 0.0, 0.0, var)
        return np.sqrt(var).astype(np.float32) + np.float32(eps)


def moments_std_bound(n, ex2):
    """|var_got - var_ref| <= (n + 8) 2^-53 E[x^2]: tests/CALIB_TESTS.md derives it (any order of the fp64 additions)."""
    return (n + 8) * 2.0 ** -53 * np.asarray(ex2, np.float64)


MOMENT_LEVELS = (0.0, 1.0, 1e3, 1e6)


def moments_columns(n, seed=11):
    """fp32 [n, 16 + 5]: a column for every (mean, std) in MOMENT_LEVELS^2 (std 0: exactly constant at the mean), then
    exactly constant columns at 0.1, -3.3, 1e6 + 0.5, 2^-130 and 16777215."""
    rng = np.random.default_rng(seed + n)
    cols = [np.float32(mu) + np.float32(sd) * rng.standard_normal(n).astype(np.float32) for mu in MOMENT_LEVELS for sd in MOMENT_LEVELS]
    cols += [np.full(n, c, np.float32) for c in (0.1, -3.3, 1e6 + 0.5, 2.0 ** -130, 16777215.0)]
    return np.stack(cols, 1).astype(np.float32)


def sum_is_exact(x):
    """per column of fp32 x [n, C]: True if the fp64 sum over axis 0 is exact in EVERY order of the additions - all values
    are multiples of a granule g (the smallest unit in the last place among them) and sum |x| < 2^53 g, so every partial sum is
    a multiple of g below 2^53 g.  (The condition under which tests/CALIB_TESTS.md derives the moments-std bound.)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    m, e = np.frexp(np.where(x == 0, 1.0, np.abs(x)))
    g = np.exp2((e - 24).min(0).astype(np.float64))               # an fp32 number is a multiple of 2^(exponent - 24)
    g = np.maximum(g, 2.0 ** -149)
    return np.abs(x).sum(0) < 2.0 ** 53 * g


# ------------------------------------------------------------------------------------------------ joint score
def _kept(q, crop):
    n, T, X, Y = q.shape
    ct, cx, cy = crop
    return q[:, ct:max(ct, T - ct), cx:max(cx, X - cx), cy:max(cy, Y - cy)].reshape(n, -1)


def joint_score_ref(a, b, mod, crop=(0, 0, 0), init=None):
    """fp32 np.abs(a - b) / mod, maximum over the kept cells of each sample, NaN sticky (np.max propagates it); a quotient
    <= 0 never raises the maximum; the result is max(init, new) with a NaN init sticky; a sample with no kept cell keeps
    its incoming score.  a, b [n, T, X, Y], mod [T, X, Y]; ``init`` [n], non-negative or NaN (default 0)."""
    a = f32(a)
    n = a.shape[0]
    init = np.zeros(n, np.float32) if init is None else f32(init)
    with np.errstate(**_IGNORE):
        r = np.abs(a - f32(b)) if b is not None else np.abs(a)
        q = _kept(r / f32(mod)[None], crop)
    assert q.dtype == np.float32
    if q.shape[1] == 0:
        return init.copy()
    nan = np.isnan(q).any(1) | np.isnan(init)
    mx = np.where(np.isnan(q) | (q <= 0), np.float32(0), q).max(1)
    return np.where(nan, np.float32(np.nan), np.maximum(np.where(np.isnan(init), np.float32(0), init), mx)).astype(np.float32)


def guarded_max_model(av, sv, parent=False):
    """fp32 model of the guarded divide (csrc/guarded_divide.h), vectorised over lanes: av, sv [L, K] are K cells that each
    of L independent lanes sees in turn, starting from m = 0.  Returns (m [L], nan [L], divided [L, K]).  ``parent``: the
    form before guarded_divide.h (skip if av <= fl(thr * sv) and sv, not the product, is at least the smallest normal)."""
    av, sv = np.atleast_2d(f32(av)), np.atleast_2d(f32(sv))
    L, K = av.shape
    m, thr = np.zeros(L, np.float32), np.zeros(L, np.float32)
    nan, divided = np.zeros(L, bool), np.zeros((L, K), bool)
    with np.errstate(**_IGNORE):
        for k in range(K):
            a, s = av[:, k], sv[:, k]
            p = thr * s
            if parent:
                div = ~(a <= p) | (s < F32_MIN_NORMAL)
            else:
                normal = np.isfinite(p) & (np.abs(p) >= F32_MIN_NORMAL)
                div = ~(a <= p) | ~normal
            q = a / s
            isn = np.isnan(q)
            nan |= div & isn
            up = div & ~isn & (q > m)
            m = np.where(up, q, m)
            thr = np.where(up, m * C_THR, thr)
            divided[:, k] = div
    assert m.dtype == np.float32 and thr.dtype == np.float32
    return m, nan, divided


def plain_max(av, sv):
    """(m, nan) of dividing every cell: what guarded_max_model must return."""
    with np.errstate(**_IGNORE):
        q = np.atleast_2d(f32(av)) / np.atleast_2d(f32(sv))
    nan = np.isnan(q).any(1)
    return np.where(np.isnan(q) | (q <= 0), np.float32(0), q).max(1), nan


# The counterexamples of the parent's guard: (m, sv, av) - after a cell sets the maximum m, the cell av over sv is skipped
# by the parent although fl(av / sv) > m.  First: m subnormal.  Second: m and sv normal, thr * sv subnormal.
_SUB = np.float32(2.0 ** -149)
COUNTEREXAMPLES = (
    (np.float32(3) * _SUB, np.float32(0.5), np.float32(2) * _SUB),
    (np.float32(float.fromhex("0x1.a30fecp-107")), np.float32(float.fromhex("0x1.d710bep-30")),
     np.float32(float.fromhex("0x1.819p-136"))),
)


def planted_cells():
    """[(name, first (av, sv), second (av, sv))]: two cells for one sample of a guarded-divide test, the rest of which is
    all-zero residual over modulation 1.  The counterexamples above with the candidate after and before the cell that sets
    m, then, around each, av at fl(thr * sv) and 1, 2 ulp below it, and a grid of neighbouring m, sv."""
    out = []
    with np.errstate(**_IGNORE):
        for ci, (m, sv, av) in enumerate(COUNTEREXAMPLES):
            out.append((f"cx{ci}_after", (m, np.float32(1)), (av, sv)))
            out.append((f"cx{ci}_before", (av, sv), (m, np.float32(1))))
            p = np.float32(np.float32(m * C_THR) * sv)
            for d in (0, 1, 2):
                cand = (p.view(np.int32) - np.int32(d)).view(np.float32)
                if cand > 0:
                    out.append((f"cx{ci}_thr_minus{d}ulp", (m, np.float32(1)), (np.float32(cand), sv)))
            for dm in (-1, 1, 2):
                for ds in (-1, 1):
                    m2 = (m.view(np.int32) + np.int32(dm)).view(np.float32)
                    sv2 = (sv.view(np.int32) + np.int32(ds)).view(np.float32)
                    p2 = np.float32(np.float32(m2 * C_THR) * sv2)
                    out.append((f"cx{ci}_grid_m{dm:+d}_s{ds:+d}", (np.float32(m2), np.float32(1)), (p2, np.float32(sv2))))
    return out


# ------------------------------------------------------------------------------------------------ pruned route
def segmin_ref(mod, cx, cy):
    """mod [T, X, Y] -> fp32 [TC, NS]: the minimum of the modulation over a segment's kept cells (64 consecutive cells of
    the flattened plane x 16 planes; cells within cx / cy of the x / y rim are not kept), 0 if a kept cell is NaN or <= 0,
    +inf for a segment with no kept cell."""
    mod = f32(mod)
    T, X, Y = mod.shape
    NS, TC = (X * Y + 63) // 64, (T + 15) // 16
    keep = np.zeros((X, Y), bool)
    keep[cx:max(cx, X - cx), cy:max(cy, Y - cy)] = True
    v = np.full((TC * 16, NS * 64), np.inf, np.float32)
    v[:T, :X * Y] = np.where(keep.reshape(-1)[None], mod.reshape(T, -1), np.float32(np.inf))
    kept = np.zeros((TC * 16, NS * 64), bool)
    kept[:T, :X * Y] = keep.reshape(-1)[None]
    bad = kept & ~(v > 0)
    v = v.reshape(TC, 16, NS, 64)
    bad = bad.reshape(TC, 16, NS, 64).any(axis=(1, 3))
    with np.errstate(**_IGNORE):
        m = np.where(np.isnan(v), np.float32(np.inf), v).min(axis=(1, 3))
    return np.where(bad, np.float32(0), m).astype(np.float32)


# ------------------------------------------------------------------------------------------------ coverage
def _bounds(lo, hi, n, M, per_sample):
    lo, hi = f32(lo), f32(hi)
    return (lo.reshape(n, M), hi.reshape(n, M)) if per_sample else (lo.reshape(1, M), hi.reshape(1, M))


def cov_count_ref(y, lo, hi, per_sample):
    """cells of y [n, M] with lo <= y <= hi as fp32 comparisons (a NaN on either side: not inside)."""
    y = f32(y)
    n, M = y.shape
    lo, hi = _bounds(lo, hi, n, M, per_sample)
    return int(((y >= lo) & (y <= hi)).sum())


def cov_rowcount_ref(y, lo, hi, per_sample, outside):
    """per sample: cells inside [lo, hi] (outside == 0) or with y <= lo or y >= hi (a cell ON a bound counts in both)."""
    y = f32(y)
    n, M = y.shape
    lo, hi = _bounds(lo, hi, n, M, per_sample)
    hit = ((y <= lo) | (y >= hi)) if outside else ((y >= lo) & (y <= hi))
    return hit.sum(1).astype(np.int64)


def cov_joint_ref(y, lo, hi, per_sample):
    """per sample: every cell inside [lo, hi]."""
    y = f32(y)
    n, M = y.shape
    lo, hi = _bounds(lo, hi, n, M, per_sample)
    return ((y >= lo) & (y <= hi)).all(1)


def cov_special_rows(M):
    """(y, lo, hi) [k, M] fp32 rows of special values with per-sample bounds, one kind per row, the rest of a row plainly
    inside [-1, 1] at 0.25: y on lo, y on hi, NaN y, NaN lo, NaN hi, lo > hi, -inf/+inf bounds around +-inf y, a +inf lower
    bound, -0.0 against +0.0 bounds and +0.0 against -0.0 bounds."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    kinds = [(0.5, 0.5, 1.0), (1.0, -1.0, 1.0), (nan, -1.0, 1.0), (0.0, nan, 1.0), (0.0, -1.0, nan), (0.0, 1.0, -1.0),
             (inf, -inf, inf), (-inf, -inf, inf), (3.0, inf, inf), (-0.0, 0.0, 0.0), (0.0, -0.0, -0.0), (0.0, -inf, 0.0)]
    y = np.full((len(kinds), M), 0.25, np.float32)
    lo, hi = np.full_like(y, -1.0), np.full_like(y, 1.0)
    for i, (v, a, b) in enumerate(kinds):
        c = (i * 5) % M
        y[i, c], lo[i, c], hi[i, c] = v, a, b
    return y, lo, hi


# ------------------------------------------------------------------------------------------------ memory
_INT_OF = {torch.float32: torch.int32, torch.float64: torch.int64, torch.int32: torch.int32, torch.int64: torch.int64,
           torch.uint8: torch.uint8}
_FILL = {torch.int32: 0x5A5AC3C3, torch.int64: 0x5A5AC3C35A5AC3C3, torch.uint8: 0xA5}


class Embedded:
    """(Not ``stencil_guards.guarded`` / ``guarded_out``: those size the band from the pitches of a 4-D fp32 grid and fill it
    with zeros or one fp32 pattern; here operands are 1-D to 4-D, fp32, fp64, int32, int64 and uint8, inputs need a NaN frame
    - a select that reads past N must show it - and an empty operand (n == 0) must keep a valid address.)
    An operand inside a larger allocation the test owns: ``alloc`` (1-D), ``view`` (the operand's shape, contiguous,
    ``guard + offset`` elements from the start of the allocation) and the frame around it, which ``untouched`` compares bit
    for bit with what it held when the operand was placed."""

    def __init__(self, t, offset=0, guard=64, fill=None, device=None):
        assert guard % 4 == 0 and guard > 0 and 0 <= offset < 4
        t = torch.as_tensor(t)
        device = t.device if device is None else device
        n = t.numel()
        self.alloc = torch.empty(guard + offset + n + guard + (4 - offset), dtype=t.dtype, device=device)
        if fill is None:
            fill = float("nan") if t.dtype.is_floating_point else _FILL[t.dtype]
        self.alloc.fill_(fill)
        self.lo, self.hi = guard + offset, guard + offset + n
        self.view = self.alloc[self.lo:self.hi].view(t.shape)
        self.view.copy_(t)
        self._frame = self.frame()

    def frame(self):
        raw = self.alloc.view(_INT_OF[self.alloc.dtype])
        return torch.cat([raw[:self.lo], raw[self.hi:]]).clone()

    def untouched(self):
        return torch.equal(self.frame(), self._frame)


def embed(t, offset_floats=0, guard=64, fill=None, device=None):
    """``Embedded`` of ``t``: ``offset_floats`` = 1 puts the operand's base one element (4 bytes for fp32) past a 16-byte
    boundary; ``guard`` elements of ``fill`` (NaN for floating point, a bit pattern for integers) lie before and after it."""
    return Embedded(t, offset_floats, guard, fill, device)
