"""What tests/select_helpers.py states, checked without a GPU: the numpy reference of the per-cell select against a loop
written out by hand, the comparison rule, the restated dispatcher against the text of the dispatcher itself (a moved
threshold fails here, before a row of the seam table silently stops reaching its branch), that the table names every
instantiation and every live-register count, the restated ka_advance, and the coverage reference against a scalar loop."""
import math
import re

import numpy as np

import select_helpers as sh


# ------------------------------------------------------------------------------------------------ the select reference
def _by_hand(col, k):
    """rank k of one column, one element at a time: NaN if any element is a NaN of either sign"""
    vals = []
    for v in col.tolist():
        if v != v:
            return float("nan")
        vals.append(v)
    vals.sort()
    return vals[k]


def test_reference_equals_a_loop_written_out_by_hand():
    rng = np.random.default_rng(1)
    for n in (1, 2, 7, 64, 169):
        s = sh.columns(n, rng)
        assert s.dtype == np.float32 and s.shape == (n, len(sh.KINDS))
        ks = sorted({0, n // 2, n - 1})
        want = sh.select_ref(s, ks)
        again = sh.pick(sh.sorted_columns(s), ks)
        assert len(sh.mismatches(again, want)) == 0
        for j in range(s.shape[1]):
            for i, k in enumerate(ks):
                h = _by_hand(s[:, j], k)
                g = float(want[i, j])
                assert (math.isnan(h) and math.isnan(g)) or h == g, (n, sh.KINDS[j], k)


def test_negative_nan_is_the_stated_bit_pattern_and_a_nan():
    v = sh.neg_nan()
    assert v.dtype == np.float32 and np.isnan(v) and int(np.array([v]).view(np.uint32)[0]) == 0xFFC00000
    # host-side inf - inf is what produces it
    with np.errstate(invalid="ignore"):
        w = np.float32(np.inf) - np.float32(np.inf)
    assert np.isnan(w)
    for n in (3, 10):
        col = sh.column("nan_neg", n, np.random.default_rng(n))
        bits = col.view(np.uint32)
        assert (bits == 0xFFC00000).sum() == 1 and np.isnan(col).sum() == 1
        assert np.isnan(sh.select_ref(col[:, None], [0, n - 1])).all()


def test_every_kind_is_what_its_name_says():
    rng = np.random.default_rng(2)
    n = 50
    c = {k: sh.column(k, n, rng) for k in sh.KINDS}
    assert (c["abs"] >= 0).all() and (c["signed"] < 0).any() and (c["signed"] > 0).any()
    assert len(set(c["constant"].tolist())) == 1 and sorted(set(c["two_valued"].tolist())) == [-3.0, 3.0]
    assert (np.diff(c["sorted_up"]) >= 0).all() and (np.diff(c["sorted_down"]) <= 0).all()
    assert (c["zeros"] == 0).all() and np.signbit(c["zeros"]).sum() == n // 2
    assert np.isnan(c["nan_pos"]).sum() == 1 and not np.signbit(c["nan_pos"][np.isnan(c["nan_pos"])]).any()
    assert np.isnan(c["nan_last"][n - 1]) and np.isnan(c["nan_last"]).sum() == 1
    assert (c["ties"] * 2 == np.round(c["ties"] * 2)).all()
    assert (c["outlier"] == np.float32(1e30)).sum() == 1
    assert np.isposinf(c["pos_inf"]).sum() == 1 and np.isneginf(c["neg_inf"]).sum() == 1 and np.isposinf(c["all_inf"]).all()
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert (np.abs(c["denormal"]) < tiny).all() and (c["denormal"] != 0).any()
    assert len(set(c["few_ulps"].tolist())) < n and (np.abs(c["few_ulps"] - 1) < 1e-5).all()
    assert np.isnan(c["all_nan"]).all()


def test_every_kind_occurs_in_every_matrix_of_24_cells_or_more():
    for M in sorted(set(sh.SMALL_M + sh.PAIR_M + sh.TILE_M + sh.STREAM_M)):
        for n in (1, 8, 169, 2048):
            kinds = sh.kind_of(n, M)
            assert len(kinds) == M
            if M >= 24:
                assert set(kinds) - {None} == set(sh.KINDS)
                # the kinds that send a register tile to the streaming form sit in the matrix's last nine cells
                assert kinds[:sh.CLEAN] == list(sh.KINDS[:sh.CLEAN]) and kinds[M - 9:] == list(sh.KINDS[sh.CLEAN:])
            else:
                assert kinds[0] == sh.KINDS[n % len(sh.KINDS)]
    # M = 1 over the rows of the table: the kinds rotate with n
    assert len({sh.kind_of(n, 1)[0] for n in sh.SMALL_N}) >= 12
    s = sh.matrix(40, 30, np.random.default_rng(0))
    assert s.shape == (40, 30) and s.dtype == np.float32 and np.isnan(s[:, 29]).all() and (s[:, 2] == -4.0).all()


def test_comparison_rule():
    a = np.array([1.0, 0.0, -0.0, np.nan, 1e-42, np.inf], np.float32)
    b = a.copy()
    assert len(sh.mismatches(a, b)) == 0
    b[1], b[2] = -0.0, 0.0                                           # a zero may carry either sign
    b[3] = sh.neg_nan()                                              # every NaN equals every NaN
    assert len(sh.mismatches(a, b)) == 0
    b[4] = np.float32(2e-42)                                         # a denormal must be the same denormal
    assert sh.mismatches(a, b).ravel().tolist() == [4]
    b = a.copy()
    b[0] = np.nextafter(np.float32(1.0), np.float32(2.0))            # one ulp is a mismatch
    b[5] = np.float32(np.nan)
    assert sh.mismatches(a, b).ravel().tolist() == [0, 5]
    b = a.copy()
    b[1] = np.float32(1e-45)                                         # the smallest denormal is not a zero
    assert sh.mismatches(a, b).ravel().tolist() == [1]


def test_rank_lists():
    rng = np.random.default_rng(3)
    for n in (1, 9, 64, 65, 168, 240):
        groups = sh.all_ranks(n, rng)
        assert all(1 <= len(g) <= 64 for g in groups) and sorted(k for g in groups for k in g) == list(range(n))
        if n > 10:
            assert any(g != sorted(g) for g in groups)
        d = sh.duplicates(n)
        assert len(d) == 5 and all(0 <= k < n for k in d) and d[0] == d[1] and d[3] == d[4] == n - 1
    assert sh.levels(1000) == [int(np.ceil(999 * np.ceil(1001 * (1 - a)) / 1000)) for a in np.arange(0.05, 1.05, 0.1)]
    assert sh.levels(1) == [0] * 5 and len(sh.levels(241)) == 10 and all(0 <= k < 241 for k in sh.levels(241))
    from cp_pre_amd import inductive_cp as icp
    for n in (7, 100, 241, 2048, 65535):
        assert sh.levels(n) == [icp.kth_index(n, n, float(a)) for a in icp.ALPHA_LEVELS if icp.quantile_level(n, float(a)) <= 1]


# ------------------------------------------------------------------------------------------------ the dispatcher
def test_thresholds_are_the_ones_the_dispatcher_writes():
    t = sh.dispatcher_thresholds()
    assert t["small_switch"] and t["small"] == [(j, 8 * j) for j in range(1, 22)]
    assert sh.SMALL_MAX == 8 * t["small"][-1][0] == 168
    assert t["pair_switch"] and t["pair"] == [(j, 8 * j) for j in range(11, 16)]
    assert t["pair_max"] == [sh.PAIR_MAX] and sh.PAIR_MAX == 240 == 2 * 8 * t["pair"][-1][0]
    assert t["tiles"] == sh.TILES
    assert [x[0] for x in sh.TILES] == [256, 384, 512, 768, 1024, 2048]
    assert t["wide"] == [sh.WIDE_MIN] and sh.WIDE_MIN == 65536
    assert t["arr"] == [(sh.TAGS_MAX, sh.TAG_ARRAY_MAX)] and (sh.TAGS_MAX, sh.TAG_ARRAY_MAX) == (4096, 12288)
    assert t["tags"] == [sh.TILES[-1][0]]
    # the order of the tests in the text is the order regime() applies them in
    text = sh.dispatcher_text()
    order = [text.index(x) for x in ("switch ((n + 7) / 8)", "if (n <= 240 &&", "if (n <= 256 && tile_ok)", "if (n <= 1024 && tile_ok)",
                                     "if (n <= 2048 &&", "if (n >= 65536)", "if (n > 4096 && n <= 12288)", "if (n > 2048)",
                                     "return launch_kth<9, false>(KA_ARGS);")]
    assert order == sorted(order)


def test_live_registers_are_computed_as_the_kernel_writes_them():
    src = open(sh.KTH_SOURCE).read()
    for line in ("constexpr int RPT = C32 ? 32 : KA_WAVES;", "constexpr int Q = R / 4;",
                 "constexpr int BATCH = Q % 8 == 0 ? 8 : Q % 6 == 0 ? 6 : 4;", "constexpr int STEP = WGS == 2 ? Q : BATCH;",
                 "constexpr int FIRST = C32 ? R / 2 + BATCH : R / 2 + Q;",
                 "const int live = max(FIRST, min(R, ((n + RPT - 1) / RPT + STEP - 1) / STEP * STEP));",
                 "const unsigned int pads = (unsigned)(live * RPT - n);", "nancell = state && row0 != pads;",
                 "constexpr int KA_W = 64, KA_MAXK = 10, KA_WAVES = 16, KA_MAPROW = 68;",
                 "#define KA_KEEP 80", "constexpr int KA_TAGS_MAX_N = 4096;"):
        assert line in src, line
    assert sh.KEEP_ROWS == 80 * 16
    # the launcher's `fast` flag: n <= (LSX ? 12 : 6) << LOG_NB1 - every n the tag-array form gets is fast, none above 12288 is
    assert "n <= (LSX ? 12 : 6) * (1 << LOG_NB1) ? 1 : 0" in src and 12 * 1024 == sh.TAG_ARRAY_MAX and 6 * 1024 > sh.TAGS_MAX
    # where live steps inside an instantiation: the table has both sides of each
    steps = {}
    for n in range(242, 2049):
        a, b = sh.regime(n - 1), sh.regime(n)
        if a.kernel == b.kernel and a.live != b.live:
            steps[n - 1] = (b.R, a.live, b.live)
    assert steps == {288: (24, 18, 24), 576: (48, 36, 42), 672: (48, 42, 48), 896: (64, 56, 64), 1280: (64, 40, 48),
                     1536: (64, 48, 56), 1792: (64, 56, 64)}
    for n in range(241, 2049):
        r = sh.regime(n)
        rpt = 32 if r.C32 else 16
        assert r.R // 2 < r.live <= r.R and r.live * rpt >= n and r.pads == r.live * rpt - n, n


def test_table_names_every_instantiation_and_every_live_count():
    names = {}
    for n in sh.SEAM_N:
        r = sh.regime(n)
        names.setdefault(r.kernel, set()).add(r.live)
    small = {"kth_small_kernel<%d>" % (8 * j) for j in range(1, 22)}
    pair = {"kth_pair_kernel<%d>" % w for w in (88, 96, 104, 112, 120)}
    tile = {"kth_tile_kernel<8, 16, 2, false>": {16}, "kth_tile_kernel<8, 24, 2, false>": {18, 24},
            "kth_tile_kernel<8, 32, 2, false>": {32}, "kth_tile_kernel<9, 48, 1, false>": {36, 42, 48},
            "kth_tile_kernel<9, 64, 1, false>": {56, 64}, "kth_tile_kernel<9, 64, 1, true>": {40, 48, 56, 64}}
    stream = {"kth_axis0_kernel<10, false> fast", "kth_axis0_kernel<10, false, 48> fast", "kth_axis0_kernel<10, false> general",
              "kth_axis0_kernel<9, true>"}
    assert set(names) == small | pair | set(tile) | stream and len(names) == 21 + 5 + 6 + 4
    for k, lives in tile.items():
        assert names[k] == lives, k
        # ... and these are all the live counts the instantiation has over the n it is sent
        nmax = [t[0] for t in sh.TILES if k == "kth_tile_kernel<%d, %d, %d, %s>" % (t[1], t[2], t[3], "true" if t[4] else "false")][0]
        assert {sh.regime(n).live for n in range(241, nmax + 1) if sh.regime(n).kernel == k} == lives
    # first and last n of every small and pair instantiation, both parities of the pair kernel
    for j in range(1, 22):
        assert 8 * j - 7 in sh.SMALL_N and 8 * j in sh.SMALL_N
    for w in (88, 96, 104, 112, 120):
        mine = [n for n in range(169, 241) if sh.regime(n).kernel == "kth_pair_kernel<%d>" % w]
        assert {mine[0], mine[-2], mine[-1]} <= set(sh.PAIR_N) and mine[0] % 2 == 1 and mine[-1] % 2 == 0, w
    # every neighbour pair of a threshold is in the table
    for nmax in (168, 240, 256, 384, 512, 768, 1024, 2048, 4096, 12288):
        assert nmax in sh.SEAM_N and nmax + 1 in sh.SEAM_N, nmax
    assert 65535 in sh.SEAM_N and 65536 in sh.SEAM_N
    assert {(n - sh.KEEP_ROWS) % 256 for n in sh.STREAM_N} >= {0, 1, 255}


def test_walk_restates_ka_advance():
    for tiles, tpp, grid in ((1224, 204, 512), (612, 102, 256), (50, 7, 16), (9, 9, 4), (100, 3, 8)):
        w = sh.walk(tiles, tpp, grid)
        seen = sorted(p * tpp + t for m in w["seq"] for p, t in m)
        assert seen == list(range(tiles))                            # (walk itself asserts each step against the division)
        assert (w["sp"], w["sc"]) == divmod(grid, tpp)
    w = sh.walk(1224, 204, 512)
    assert w["taken"] > 0 and w["passed"] > 0 and max(len(m) for m in w["seq"]) == 3
    text = open(sh.KTH_SOURCE).read()
    assert re.search(r"plane \+= pl\.sp;\s+c0 \+= pl\.sc \* W;\s+if \(c0 >= pl\.tpp \* W\) \{ c0 -= pl\.tpp \* W; \+\+plane; \}", text)


# ------------------------------------------------------------------------------------------------ coverage
def test_coverage_reference_equals_a_scalar_loop():
    rng = np.random.default_rng(5)
    n, M, nk = 9, 11, 3
    y = rng.standard_normal((n, M)).astype(np.float32)
    c = (0.3 * rng.standard_normal((n, M))).astype(np.float32)
    m = (0.5 + rng.random(M)).astype(np.float32)
    q = np.array([0.4, 0.9, 1.7], np.float32)
    qc = (q[:, None] * (0.5 + rng.random((nk, M)))).astype(np.float32)
    y[0, 0], y[1, 1], c[2, 2], m[3] = np.nan, np.inf, np.nan, np.inf
    qc[1, 4], qc[2, 5], qc[0, 6] = np.nan, -0.5, 0.0
    lo, hi = sh.cov_bounds(q[1], m, c)
    y[4, 7], y[5, 8] = lo[4, 7], hi[5, 8]                            # exactly on a bound: inside
    for qq, mm, cc in ((q, m, c), (q, m, None), (qc, None, c), (qc, None, None)):
        ins = sh.cov_inside(y, qq, mm, cc)
        for k in range(nk):
            for s in range(n):
                for j in range(M):
                    qv = np.float32(qq[k] if np.ndim(qq[k]) == 0 else qq[k][j])
                    with np.errstate(all="ignore"):
                        hw = qv if mm is None else np.float32(qv * mm[j])
                        ctr = np.float32(0) if cc is None else cc[s, j]
                        l, h = np.float32(ctr - hw), np.float32(ctr + hw)
                    assert bool(ins[k, s, j]) == (float(y[s, j]) >= float(l) and float(y[s, j]) <= float(h)), (k, s, j)
        counts, curve = sh.cov_marginal(ins)
        assert counts.tolist() == [int(ins[k].sum()) for k in range(nk)] and curve.dtype == np.float64
        assert np.array_equal(curve, np.array([ins[k].mean() for k in range(nk)]))
        keep, jc, jcurve = sh.cov_joint(ins)
        assert np.array_equal(keep, np.array([[ins[k, s].all() for s in range(n)] for k in range(nk)]))
        assert np.array_equal(jcurve, keep.mean(1))
    assert sh.cov_inside(y, q, m, c)[1, 4, 7] and sh.cov_inside(y, q, m, c)[1, 5, 8]


def test_coverage_plan_restates_the_host_loop():
    src = open(sh.KTH_SOURCE.replace("kth_axis0.hip", "coverage_levels.hip")).read()
    for line in ("constexpr int COV_BLOCK = 256;", "constexpr int COV_G = 64;", "constexpr int COV_UNROLL = 8;",
                 "constexpr long long COV_TARGET_BLOCKS = 2048;", "static_assert(PRE_COV_MAX_LEVELS == 16",
                 "long long splits = (COV_TARGET_BLOCKS + groups - 1) / groups;",
                 "splits = splits < 1 ? 1 : (splits > chunks ? chunks : splits);",
                 "const int ch0 = (int)((long long)a.chunks * blockIdx.x / gridDim.x);"):
        assert line in src, line
    assert sh.cov_plan(65, 257) == (2, 2, 2)
    groups, chunks, splits = sh.cov_plan(4099, 256 * 64 + 7)
    assert (groups, chunks, splits) == (65, 65, 32)
    runs = sh.cov_chunk_runs(chunks, splits)
    assert runs[0][0] == 0 and runs[-1][1] == chunks and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
    assert {b - a for a, b in runs} == {2, 3}
