"""What the tests of the per-cell select (cp_pre_amd/csrc/kth_axis0.hip) and of the coverage at every level
(cp_pre_amd/csrc/coverage_levels.hip) share: the dispatcher of ``pre_kth_axis0_planes_f32`` restated (``regime``), the
table of row counts on both sides of every branch (``SEAM_N``), the column kinds (``columns`` / ``matrix``), the rank
lists, the plain numpy references and the bit-for-bit comparison.  tests/test_select_ref_cpu.py checks what stands here
without a GPU, tests/test_gpu_select_seams.py and tests/test_gpu_covlevels_seams.py use it on the MI355X, and
tests/SELECT_TESTS.md says which branch each row reaches.  Nothing of cp_pre_amd is imported and no GPU is needed."""
import collections
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KTH_SOURCE = os.path.join(ROOT, "cp_pre_amd", "csrc", "kth_axis0.hip")
NEG_NAN_BITS = 0xFFC00000                              # what host-side inf - inf produces: a NaN with the sign bit set
MAXK = 10                                              # KA_MAXK: ranks per launch
MAX_RANKS = 64                                         # ranks per call (the host's sk[64] / rows[64])

# ------------------------------------------------------------------------------------------------ the dispatcher, restated
SMALL_MAX = 168                                        # kth_small_kernel<N>, N = 8 ceil(n / 8)
PAIR_MAX = 240                                         # kth_pair_kernel<NW>, NW = 8 ceil(ceil(n / 2) / 8)
# kth_tile_kernel<LOG_NB1, R, WGS, C32>: (largest n, LOG_NB1, R, WGS, C32)
TILES = ((256, 8, 16, 2, False), (384, 8, 24, 2, False), (512, 8, 32, 2, False), (768, 9, 48, 1, False),
         (1024, 9, 64, 1, False), (2048, 9, 64, 1, True))
TAGS_MAX = 4096                                        # kth_axis0_kernel<10, false>, tags in the histogram words
TAG_ARRAY_MAX = 12288                                  # kth_axis0_kernel<10, false, 48>, tags in an array of their own
WIDE_MIN = 65536                                       # kth_axis0_kernel<9, true>, 32-bit counters
KEEP_ROWS = 1280                                       # rows the tag forms keep in registers (KA_KEEP x KA_WAVES); sweeps of 256

Regime = collections.namedtuple("Regime", "kernel R WGS C32 live pads")


def tile_live(n, R, WGS, C32):
    """(live, pads) of kth_tile_kernel: the registers its sweeps run over and the padding rows per cell."""
    RPT = 32 if C32 else 16
    Q = R // 4
    BATCH = 8 if Q % 8 == 0 else 6 if Q % 6 == 0 else 4
    STEP = Q if WGS == 2 else BATCH
    FIRST = R // 2 + (BATCH if C32 else Q)
    per_thread = -(-n // RPT)
    live = max(FIRST, min(R, -(-per_thread // STEP) * STEP))
    return live, live * RPT - n


def regime(n):
    """The kernel instantiation ``pre_kth_axis0_planes_f32`` launches for n rows (row pitches below the fallbacks of
    the pair and tile kernels, which no test can afford); for the register tiles also (R, WGS, C32, live, pads)."""
    assert n >= 1
    if n <= SMALL_MAX:
        return Regime("kth_small_kernel<%d>" % (8 * ((n + 7) // 8)), None, None, None, None, None)
    if n <= PAIR_MAX:
        return Regime("kth_pair_kernel<%d>" % (8 * (((n + 1) // 2 + 7) // 8)), None, None, None, None, None)
    for nmax, lognb, R, WGS, C32 in TILES:
        if n <= nmax:
            live, pads = tile_live(n, R, WGS, C32)
            name = "kth_tile_kernel<%d, %d, %d, %s>" % (lognb, R, WGS, "true" if C32 else "false")
            return Regime(name, R, WGS, C32, live, pads)
    if n >= WIDE_MIN:
        return Regime("kth_axis0_kernel<9, true>", None, None, None, None, None)
    if TAGS_MAX < n <= TAG_ARRAY_MAX:
        return Regime("kth_axis0_kernel<10, false, 48> fast", None, None, None, None, None)
    # (the launcher's `fast` flag of this instantiation: n <= 6 * 1024, of which the dispatcher sends it n <= 4096 only)
    return Regime("kth_axis0_kernel<10, false> " + ("fast" if n <= TAGS_MAX else "general"), None, None, None, None, None)


def dispatcher_text():
    """The dispatcher as written: from the entry point's signature to ``#undef KA_ARGS``."""
    src = open(KTH_SOURCE).read()
    a = src.index('extern "C" int pre_kth_axis0_planes_f32')
    return src[a:src.index("#undef KA_ARGS", a)]


def dispatcher_thresholds():
    """The thresholds read off the dispatcher's text, in the shape of the constants above."""
    t = dispatcher_text()
    nb_small = int(re.search(r"#define KT_NB_SMALL (\d+)", t).group(1))
    small = [(int(c), int(N)) for c, N in re.findall(r"case (\d+): return launch_kth_small<(\d+)>\(KA_ARGS\);", t)]
    pair = [(int(c), int(N)) for c, N in re.findall(r"case (\d+): return launch_kth_pair<(\d+)>\(KA_ARGS\);", t)]
    pair_max = [int(x) for x in re.findall(r"if \(n <= (\d+) && \(long long\)\(\(n \+ 1\) / 2\) \* S \* 4 < \(1LL << 31\)\)", t)]
    tiles = [(int(nmax), nb_small if nb == "KT_NB_SMALL" else int(nb), int(R), int(W), False)
             for nmax, nb, R, W in re.findall(r"if \(n <= (\d+) && tile_ok\) return launch_kth_tile<(\w+), (\d+), (\d+)>\(KA_ARGS\);", t)]
    tiles += [(int(nmax), int(nb), int(R), int(W), True) for nmax, nb, R, W in
              re.findall(r"if \(n <= (\d+) && S \* 388 \+ 128 < \(1LL << 32\)\) return launch_kth_tile<(\d+), (\d+), (\d+), true>\(KA_ARGS\);", t)]
    wide = [int(x) for x in re.findall(r"if \(n >= (\d+)\) return launch_kth<9, true>\(KA_ARGS\);", t)]
    arr = [(int(a), int(b)) for a, b in re.findall(r"if \(n > (\d+) && n <= (\d+)\) return launch_kth<10, false, 48>\(KA_ARGS\);", t)]
    tags = [int(x) for x in re.findall(r"if \(n > (\d+)\) return launch_kth<10, false>\(KA_ARGS\);", t)]
    return dict(small=small, small_switch="switch ((n + 7) / 8) {" in t, pair=pair, pair_max=pair_max,
                pair_switch="switch (((n + 1) / 2 + 7) / 8) {" in t, tiles=tuple(tiles), wide=wide, arr=arr, tags=tags)


# ------------------------------------------------------------------------------------------------ the seam table
SMALL_N = [v for j in range(1, 22) for v in (8 * j - 7, 8 * j)]           # first and full row count of every N
SMALL_M = (1, 63, 64, 65, 257)
PAIR_N = [169, 170, 175, 176, 177, 191, 192, 193, 207, 208, 209, 223, 224, 225, 239, 240]
PAIR_M = (1, 31, 32, 33, 97)
TILE_N = [241, 256, 257, 288, 289, 384, 385, 512, 513, 576, 577, 672, 673, 768, 769, 896, 897, 1024, 1025, 1026, 1280, 1281,
          1536, 1537, 1792, 1793, 2047, 2048]
TILE_M = (1, 31, 32, 33, 64, 65, 200)
STREAM_N = [2049, 2303, 2304, 2305, 4095, 4096, 4097, 4352, 4353, 12287, 12288, 12289, 20000, 65535]
STREAM_M = (33, 64, 130)
WIDE_N = [65536]                                       # (run by test_gpu_parity.py / test_gpu_fuzz.py; named here for the table)
SEAM_N = SMALL_N + PAIR_N + TILE_N + STREAM_N + WIDE_N


# ------------------------------------------------------------------------------------------------ ranks
def levels(n):
    """The ranks of the ten reference levels alpha = 0.05, 0.15 .. 0.95 on n rows (np.quantile's method='higher' of the
    level ceil((n + 1)(1 - alpha)) / n), those whose level does not exceed 1."""
    out = []
    for a in np.arange(0.05, 0.95 + 0.1, 0.1):
        q = np.ceil((n + 1) * (1 - a)) / n
        if q <= 1.0:
            out.append(int(np.ceil((n - 1) * q)))
    return out


def all_ranks(n, rng):
    """Every rank 0 .. n-1 once, shuffled, in groups of at most 64 (the most one call takes): results then scatter
    through the host's rows[] and the groups of more than ten take several launches."""
    p = [int(k) for k in rng.permutation(n)]
    return [p[i:i + MAX_RANKS] for i in range(0, n, MAX_RANKS)]


def duplicates(n):
    """[k, k, k+1, n-1, n-1]: equal prefixes, one list for two owners."""
    k = n // 2
    return [k, k, min(k + 1, n - 1), n - 1, n - 1]


def tile_ranks(n):
    return sorted({0, 1 % n, n // 2, max(n - 2, 0), n - 1} | set(levels(n)))


# ------------------------------------------------------------------------------------------------ column kinds
# The first CLEAN kinds leave a register tile to its fast form (window finite, no bucket above the list capacity); the
# others send their tile to the streaming form.  `matrix` keeps the two apart, so that the fast form's own handling of
# a constant column, of a NaN (row 0 of its histogram against the padding) and of signed zeros is what answers.
KINDS = ("abs", "signed", "constant", "sorted_up", "sorted_down", "zeros", "nan_pos", "nan_neg", "nan_last",
         "two_valued", "ties", "outlier", "pos_inf", "neg_inf", "all_inf", "denormal", "few_ulps", "all_nan")
CLEAN = 9


def neg_nan():
    return np.array([NEG_NAN_BITS], np.uint32).view(np.float32)[0]


def column(kind, n, rng):
    x = rng.standard_normal(n).astype(np.float32)
    scale = np.float32(math.exp(2.0 * rng.standard_normal()))
    if kind == "abs":
        return np.abs(x) * scale
    if kind == "signed":
        return x * scale
    if kind == "constant":
        return np.full(n, -4.0, np.float32)
    if kind == "sorted_up":
        return np.sort(x * scale)
    if kind == "sorted_down":
        return np.sort(x * scale)[::-1].copy()
    if kind == "zeros":
        z = np.zeros(n, np.float32)
        z[1::2] = -0.0
        return z
    if kind == "nan_pos":
        x = np.abs(x) * scale
        x[n // 3] = np.float32(np.nan)
        return x
    if kind == "nan_neg":
        x = np.abs(x) * scale
        x[(2 * n) // 3] = neg_nan()
        return x
    if kind == "nan_last":
        x = x * scale
        x[n - 1] = np.float32(np.nan)
        return x
    if kind == "two_valued":
        x[: n // 2] = 3.0
        x[n // 2:] = -3.0
        return x
    if kind == "ties":
        return (np.round(2 * x * scale) / 2).astype(np.float32)
    if kind == "outlier":
        x = x * scale
        x[n // 3] = np.float32(1e30)
        return x
    if kind == "pos_inf":
        x = x * scale
        x[5 % n] = np.float32(np.inf)
        return x
    if kind == "neg_inf":
        x = x * scale
        x[n - 1] = np.float32(-np.inf)
        return x
    if kind == "all_inf":
        return np.full(n, np.inf, np.float32)
    if kind == "denormal":
        with np.errstate(under="ignore"):
            return (x * np.float32(1e-42)).astype(np.float32)
    if kind == "few_ulps":
        return (np.float32(1) + np.float32(1e-7) * x).astype(np.float32)
    if kind == "all_nan":
        return np.full(n, np.nan, np.float32)
    raise ValueError(kind)


def columns(n, rng, kinds=KINDS):
    """[n, len(kinds)] fp32: one column of every kind."""
    return np.stack([column(k, n, rng) for k in kinds], axis=1)


def kind_of(n, M):
    """Which kind column j of ``matrix(n, M, rng)`` holds (None: |N(0,1)| times a per-column scale, the background).
    M >= 24: the clean kinds in columns 0 .. 8, the others in the last nine - every kind at every n; narrower matrices
    rotate the kinds by n."""
    out = [None] * M
    if M >= 24:
        for i in range(CLEAN):
            out[i] = KINDS[i]
        for i in range(CLEAN, len(KINDS)):
            out[M - len(KINDS) + i] = KINDS[i]
    else:
        for j in range(M):
            out[j] = KINDS[(n + j) % len(KINDS)]
    return out


def matrix(n, M, rng):
    s = np.abs(rng.standard_normal((n, M)).astype(np.float32)) * np.exp(2.0 * rng.standard_normal(M)).astype(np.float32)
    for j, kind in enumerate(kind_of(n, M)):
        if kind is not None:
            s[:, j] = column(kind, n, rng)
    return s


# ------------------------------------------------------------------------------------------------ reference and measure
def select_ref(s, ks):
    """np.sort(s, axis=0)[ks]; every rank of a column that holds a NaN of either sign is NaN.  s [n, M] fp32."""
    s = np.asarray(s, np.float32)
    srt = np.sort(s, axis=0)
    out = srt[np.asarray(ks, np.int64)].copy()
    out[:, np.isnan(s).any(axis=0)] = np.float32(np.nan)
    return out


def sorted_columns(s):
    """np.sort(s, axis=0) with the NaN columns marked, for tests that ask several rank lists of one matrix."""
    s = np.asarray(s, np.float32)
    return np.sort(s, axis=0), np.isnan(s).any(axis=0)


def pick(srt_nan, ks):
    srt, nan = srt_nan
    out = srt[np.asarray(ks, np.int64)].copy()
    out[:, nan] = np.float32(np.nan)
    return out


def mismatches(got, want):
    """Indices where ``got`` is not ``want`` bit for bit on the int32 view - but every NaN equals every NaN and a zero may
    carry either sign (the key order puts -0 before +0, numpy does not).  A denormal must be the same denormal."""
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    same = got.view(np.int32) == want.view(np.int32)
    same |= np.isnan(got) & np.isnan(want)
    same |= (got == 0) & (want == 0)
    return np.argwhere(~same)


# ------------------------------------------------------------------------------------------------ persistent grids
def walk(tiles, tpp, grid):
    """ka_advance restated: the (plane, tile in plane) sequence of every workgroup of a persistent grid, and how often the
    wrap branch (c0 >= tpp W) was taken / not taken on the way to a tile that exists."""
    sp, sc = grid // tpp, grid % tpp
    taken = passed = 0
    seq = []
    for b in range(min(grid, tiles)):
        plane, t = b // tpp, b % tpp
        tile = b
        mine = []
        while tile < tiles:
            assert (plane, t) == (tile // tpp, tile % tpp)
            mine.append((plane, t))
            nplane, nt = plane + sp, t + sc
            if nt >= tpp:
                nt -= tpp
                nplane += 1
                taken += tile + grid < tiles
            else:
                passed += tile + grid < tiles
            plane, t, tile = nplane, nt, tile + grid
        seq.append(mine)
    return dict(sp=sp, sc=sc, taken=taken, passed=passed, seq=seq)


# ------------------------------------------------------------------------------------------------ coverage at every level
COV_BLOCK, COV_G, COV_UNROLL, COV_TARGET_BLOCKS, COV_MAX_LEVELS = 256, 64, 8, 2048, 16


def cov_plan(n, M):
    """pre_cov_levels_f32's grid: (sample groups, cell chunks, workgroups that split the chunks)."""
    groups, chunks = -(-n // COV_G), -(-M // COV_BLOCK)
    splits = max(1, min(chunks, -(-COV_TARGET_BLOCKS // groups)))
    return groups, chunks, splits


def cov_chunk_runs(chunks, splits):
    return [(chunks * b // splits, chunks * (b + 1) // splits) for b in range(splits)]


def cov_bounds(q, m, c):
    """The bounds of one level in fp32, one rounded operation per numpy operation: hw = q m, c - hw, c + hw."""
    with np.errstate(all="ignore"):
        hw = np.asarray(q, np.float32) if m is None else (np.asarray(q, np.float32) * np.asarray(m, np.float32)).astype(np.float32)
        if c is None:
            return (-hw).astype(np.float32), hw.astype(np.float32)
        c = np.asarray(c, np.float32)
        return (c - hw).astype(np.float32), (c + hw).astype(np.float32)


def cov_inside(y, q, m=None, c=None):
    """bool [nk, n, M]: sample s, cell j inside at level k - lo <= y <= hi in float64 (a NaN on either side: outside).
    y [n, M]; q [nk] or [nk, M]; m [M] or None; c [n, M] or None."""
    y = np.asarray(y, np.float32)
    out = np.empty((len(q),) + y.shape, bool)
    rows = max(1, (1 << 18) // y.shape[1])                 # (a block of samples at a time: the float64 copies stay in cache)
    for s0 in range(0, y.shape[0], rows):
        y64 = y[s0:s0 + rows].astype(np.float64)
        for k in range(len(q)):
            lo, hi = cov_bounds(q[k], m, None if c is None else c[s0:s0 + rows])
            with np.errstate(invalid="ignore"):
                out[k, s0:s0 + rows] = (y64 >= lo.astype(np.float64)) & (y64 <= hi.astype(np.float64))
    return out


def cov_marginal(inside):
    """emp_cov at every level: the inside cells over all cells, count / total in float64."""
    nk = inside.shape[0]
    counts = inside.reshape(nk, -1).sum(1)
    return counts, np.array([float(c) / float(inside[0].size) for c in counts], np.float64)


def cov_joint(inside):
    """(bool [nk, n]: every cell of the sample inside; the counts; emp_cov_joint at every level)."""
    keep = inside.all(axis=2)
    counts = keep.sum(1)
    return keep, counts, np.array([float(c) / float(keep.shape[1]) for c in counts], np.float64)
