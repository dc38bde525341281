"""What tests/test_setprop_ref_cpu.py and tests/test_gpu_setprop_seams.py share: the closed form of PRE set propagation and the
recipe's interval set as loops written out from include/cp_pre_setprop.h, the condition under which integer data make fp64
arithmetic exact, the derived agreement bound, and the launch plan of cp_pre_amd/csrc/set_prop.hip restated.  The memory
helpers (framed outputs, strided inputs with NaN wherever no element lies) are those of tests/ode_helpers.py."""
import collections

import numpy as np

from ode_helpers import Framed, Source, layout, offsets, within  # noqa: F401  (re-exported to the tests)

U53 = 2.0 ** -53
SP_BLOCK, SP_TB, SP_TJ, MAX_TAPS = 256, 8, 32, 7              # set_prop.hip / cp_pre_setprop.h
_IGNORE = dict(invalid="ignore", over="ignore")


# ------------------------------------------------------------------------------------------------ references
def bounds_ref(c, r, g, a, bad=None):
    """lower / upper [B, N] in float64: centre_k = sum_j c_j g[(k - j) mod N], radius_k = sum_j r_j a[(k - j) mod N], the sum
    over j ascending as the header states it.  A row with a non-finite c or r (or flagged ``bad``) is NaN throughout; an
    element whose centre or radius overflows is NaN."""
    c, r, g, a = (np.asarray(v, np.float64) for v in (c, r, g, a))
    B, N = c.shape
    k = np.arange(N)
    cen, rad = np.zeros((B, N)), np.zeros((B, N))
    with np.errstate(**_IGNORE):
        for j in range(N):
            m = (k - j) % N
            cen = cen + c[:, j:j + 1] * g[m][None, :]
            rad = rad + r[:, j:j + 1] * a[m][None, :]
        lo, hi = cen - rad, cen + rad
    ok = np.isfinite(cen) & np.isfinite(rad)
    ok &= np.isfinite(c).all(axis=1, keepdims=True) & np.isfinite(r).all(axis=1, keepdims=True)
    if bad is not None:
        ok &= ~np.asarray(bad, bool)[:, None]
    lo[~ok] = np.nan
    hi[~ok] = np.nan
    return lo, hi


def bounds_magnitude(c, r, g, a):
    """sum_j |terms| per output (non-finite values counted as 0)"""
    z = dict(nan=0.0, posinf=0.0, neginf=0.0)
    lo, hi = bounds_ref(np.abs(np.nan_to_num(np.asarray(c, np.float64), **z)), np.abs(np.nan_to_num(np.asarray(r, np.float64), **z)),
                        np.abs(g), np.abs(a))
    return hi                                              # |c| (*) |g| + |r| (*) |a|


def qhat_shift(k, correlation):
    """t = n + shift (header): n - (k+1)/2 for a symmetric kernel without correlation, n + (k-3)/2 with it"""
    return (k - 3) // 2 if correlation else -((k + 1) // 2)


def recipe_conv(x, taps, correlation):
    """conv[b, n], n < Nt + 2, of the padded rows s = [0, x, 0] in float64, tap by tap in order"""
    x, taps = np.asarray(x, np.float64), np.asarray(taps, np.float64)
    B, nt = x.shape
    Ns = nt + 2
    s = np.zeros((B, Ns))
    s[:, 1:nt + 1] = x
    n = np.arange(Ns)
    conv = np.zeros((B, Ns))
    with np.errstate(**_IGNORE):
        for i, w in enumerate(taps):
            conv = conv + w * s[:, (n + i) % Ns if correlation else (n - i) % Ns]
    return conv


def recipe_sets(x, taps, correlation=False, q=None):
    """(c, r, bad) of the recipe, written out from the header: j = n - 1; points conv[1..3] and conv[Nt + 1]; symmetric
    [-|conv[n]|, |conv[n]|] for n = 4 .. Nt, where q[b, t] (``q`` broadcastable to [B, Nt]) stands in when
    t = n + qhat_shift lies in [0, Nt); ``bad`` rows hold a non-finite conv[n], n >= 1."""
    x = np.asarray(x, np.float64)
    B, nt = x.shape
    N = nt + 1
    conv = recipe_conv(x, taps, correlation)
    c, r = np.zeros((B, N)), np.zeros((B, N))
    for n in (1, 2, 3, nt + 1):
        c[:, n - 1] = conv[:, n]
    qq = None if q is None else np.broadcast_to(np.asarray(q, np.float64), (B, nt))
    for n in range(4, nt + 1):
        t = n + qhat_shift(len(taps), correlation)
        r[:, n - 1] = qq[:, t] if qq is not None and 0 <= t < nt else np.abs(conv[:, n])
    bad = ~np.isfinite(conv[:, 1:]).all(axis=1)
    return c, r, bad


def steps_outside(nt, k, correlation):
    """the interior n (4 .. Nt) whose q-hat step falls outside [0, Nt): these keep |conv[n]|"""
    return [n for n in range(4, nt + 1) if not 0 <= n + qhat_shift(k, correlation) < nt]


def recipe_ref(x, taps, correlation, q, g, a):
    c, r, bad = recipe_sets(x, taps, correlation, q)
    return bounds_ref(c, r, g, a, bad)


def recipe_magnitude(x, taps, correlation, q, g, a):
    """the sets of |x| through |taps| (q as it is): sum |terms| with the convolution's own products included"""
    z = dict(nan=0.0, posinf=0.0, neginf=0.0)
    c, r, _ = recipe_sets(np.abs(np.nan_to_num(np.asarray(x, np.float64), **z)), np.abs(taps), correlation, q)
    return bounds_magnitude(c, r, g, a)


def tol(nterms, magnitude):
    """8 nterms 2^-53 sum |terms|: the bound tests/test_gpu_set_prop.py uses"""
    return 8 * nterms * U53 * magnitude


def assert_exact_f64(magnitude, *operands):
    """integer operands and sum |terms| < 2^53: every partial sum is an integer fp64 holds, so the bounds are the same in
    any order and with or without fma"""
    for v in operands:
        v = np.asarray(v, np.float64)
        fin = v[np.isfinite(v)]
        assert np.array_equal(fin, np.rint(fin)), "not integer data"
    assert magnitude.size == 0 or magnitude.max() < 2 ** 53, magnitude.max()


def same_f64(got, ref):
    """every element equal; any NaN equals any NaN, a zero of either sign equals 0"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    ok = (got == ref) | (np.isnan(got) & np.isnan(ref))
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), ref[bad[:8]].tolist())


# ------------------------------------------------------------------------------------------------ the launch plan
Plan = collections.namedtuple("Plan", "TK RB tiles groups blocks chunks jmax window wraps last_tile_cols last_group_rows")


def plan(B, N):
    """``launch`` of set_prop.hip restated: TK = 64 / 128 / 256 columns per workgroup for N <= 64 / <= 128 / larger,
    RB = 8 * 256 / TK rows, ``tiles`` x ``groups`` workgroups, ``chunks`` of 32 j with ``jmax`` in the last one, the staged
    ``window`` of TK + 31 table entries and ``wraps`` = (window - 1) // N, the table lengths it spans (>= 1: some entry is
    staged more than once), the live columns of the last tile and the live rows of the last row group."""
    TK = 64 if N <= 64 else 128 if N <= 128 else 256
    RB = SP_TB * (SP_BLOCK // TK)
    tiles = (N + TK - 1) // TK
    groups = (B + RB - 1) // RB
    chunks = (N + SP_TJ - 1) // SP_TJ
    W = TK + SP_TJ - 1
    return Plan(TK, RB, tiles, groups, tiles * groups, chunks, N - SP_TJ * (chunks - 1), W, (W - 1) // N,
                N - TK * (tiles - 1), B - RB * (groups - 1) if B else 0)


# N of the table of tests/ODE_TESTS.md: what each row claims of its plan (at B = RB + 1: two row groups, one live row in the last)
NS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
TABLE = {
    1: dict(TK=64, RB=32, tiles=1, chunks=1, jmax=1, wraps=94),
    2: dict(TK=64, chunks=1, jmax=2, wraps=47),
    3: dict(TK=64, chunks=1, jmax=3, wraps=31),
    31: dict(TK=64, chunks=1, jmax=31, wraps=3),
    32: dict(TK=64, chunks=1, jmax=32, wraps=2),
    33: dict(TK=64, chunks=2, jmax=1, wraps=2),
    63: dict(TK=64, RB=32, chunks=2, jmax=31, wraps=1, last_tile_cols=63),
    64: dict(TK=64, RB=32, tiles=1, chunks=2, jmax=32, wraps=1, last_tile_cols=64),
    65: dict(TK=128, RB=16, tiles=1, chunks=3, jmax=1, wraps=2, last_tile_cols=65),
    127: dict(TK=128, RB=16, chunks=4, jmax=31, wraps=1),
    128: dict(TK=128, RB=16, tiles=1, chunks=4, jmax=32, wraps=1),
    129: dict(TK=256, RB=8, tiles=1, chunks=5, jmax=1, wraps=2),
    255: dict(TK=256, RB=8, tiles=1, chunks=8, jmax=31, wraps=1),
    256: dict(TK=256, RB=8, tiles=1, chunks=8, jmax=32, wraps=1, last_tile_cols=256),
    257: dict(TK=256, RB=8, tiles=2, chunks=9, jmax=1, wraps=1, last_tile_cols=1),
    513: dict(TK=256, RB=8, tiles=3, chunks=17, jmax=1, wraps=0, last_tile_cols=1),
}


def batches(N):
    """the B of one N: a single row, and RB - 1 | RB | RB + 1"""
    RB = plan(1, N).RB
    return (1, RB - 1, RB, RB + 1)


def assert_plan(B, N):
    p = plan(B, N)
    for key, want in TABLE[N].items():
        assert getattr(p, key) == want, ((B, N), key, p)
    assert p.groups == (1 if B <= p.RB else 2) and p.last_group_rows == (B if B <= p.RB else B - p.RB)
    return p


# ------------------------------------------------------------------------------------------------ data
def ints(rng, lo, hi, *shape):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def int_tables(rng, N):
    """integer tables g (any sign) and a (>= 0), no entry 0: every entry's use shows"""
    g = rng.integers(1, 4, size=N) * rng.choice([-1, 1], size=N)
    a = rng.integers(1, 4, size=N)
    return g.astype(np.float64), a.astype(np.float64)


def H_of(n, seed):
    """an inverse spectrum as tests/test_gpu_set_prop.py draws it"""
    rng = np.random.default_rng(seed)
    return 1 / (np.fft.fft(np.r_[rng.standard_normal(min(3, n)), np.zeros(n - min(3, n))]) + 0.3)
