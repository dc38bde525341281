"""GPU tests (pytest -m gpu) of the per-cell select of cp_pre_amd/csrc/kth_axis0.hip at every instantiation its dispatcher
can reach: the 21 pruned networks of kth_small_kernel at their first and full row count with EVERY rank asked, the five
kth_pair_kernel instantiations in both parities of n, the six register-tile instantiations on both sides of every
live-register step, the persistent loops of the 32-cell tiles and of a multi-plane launch, and the streaming forms at their
thresholds and sweep tails - against np.sort on the host (tests/select_helpers.py, checked on the CPU by
tests/test_select_ref_cpu.py), bit for bit: every NaN equals every NaN, a zero may carry either sign, nothing else is
tolerated.  tests/SELECT_TESTS.md says which branch each n reaches."""
import numpy as np
import pytest
import torch

import select_helpers as sh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = np.float32(-7.0)


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    from cp_pre_amd import _lib
    _lib.load()
    return torch.device(DEV)


def select(d, ks):
    """icp.kth_axis0 on the device matrix d [n, M] -> numpy [len(ks), M]"""
    from cp_pre_amd import inductive_cp as icp
    return icp.kth_axis0(d, [int(k) for k in ks]).cpu().numpy()


def check(d, ref, ks, what):
    got = select(d, ks)
    bad = sh.mismatches(got, sh.pick(ref, ks))
    assert len(bad) == 0, (what, [(int(ks[j]), int(c)) for j, c in bad[:8]], len(bad))


def planes_call(buf, ps, pitch, planes, n, M, ks, out_rank_stride, out_plane_stride, frame=64):
    """pre_kth_axis0_planes_f32 into a flat output filled with a sentinel, `frame` floats of it before and behind; returns
    (the whole flat output, the index of every expected result [planes, nk, M])."""
    from cp_pre_amd import _lib
    lib = _lib.load()
    nk = len(ks)
    size = (planes - 1) * out_plane_stride + (nk - 1) * out_rank_stride + M
    flat = torch.full((size + 2 * frame,), float(SENTINEL), device=DEV)
    out = flat[frame:]
    with torch.cuda.device(buf.device):
        _lib.check(lib.pre_kth_axis0_planes_f32(_lib.ptr(buf), ps, pitch, planes, n, M, _lib.iarr32([int(k) for k in ks]), nk,
                                                _lib.ptr(out), out_rank_stride, out_plane_stride, _lib.stream()), "planes")
    idx = (frame + np.arange(planes)[:, None, None] * out_plane_stride + np.arange(nk)[None, :, None] * out_rank_stride
           + np.arange(M)[None, None, :])
    return flat.cpu().numpy(), idx


def check_framed(flat, idx, want, what):
    """the results where they belong, the sentinel everywhere else"""
    expect = np.full(flat.shape, SENTINEL, np.float32)
    expect[idx] = want
    bad = sh.mismatches(flat, expect)
    assert len(bad) == 0, (what, bad[:8].ravel().tolist(), len(bad))


# ================================================================================================ 1. kth_small_kernel<N>
@pytest.mark.parametrize("n", sh.SMALL_N)
def test_small_every_rank_of_every_network(gpu, n):
    """n = 8j - 7 and 8j, j = 1 .. 21: the first and the full row count of every kth_small_kernel<N>, each a differently
    pruned Batcher network - EVERY rank 0 .. n-1 (a wrong compare-exchange moves only some), asked in shuffled groups of up
    to 64 (several launches, results scattered through rows[]), and one call with duplicate ranks.  M = 257 is five tiles:
    a second workgroup whose last three waves return early."""
    assert sh.regime(n).kernel == "kth_small_kernel<%d>" % (8 * ((n + 7) // 8))
    rng = np.random.default_rng(1000 + n)
    for M in sh.SMALL_M:
        s = sh.matrix(n, M, rng)
        d, ref = torch.from_numpy(s).to(gpu), sh.sorted_columns(s)
        for group in sh.all_ranks(n, rng):
            check(d, ref, group, (n, M, "all ranks"))
        check(d, ref, sh.duplicates(n), (n, M, "duplicates"))


# ================================================================================================ 2. kth_pair_kernel<NW>
@pytest.mark.parametrize("n", sh.PAIR_N)
def test_pair_every_rank_in_both_parities(gpu, n):
    """The first and last n of every kth_pair_kernel<NW> (88 .. 120), odd and even: with odd n the upper lane holds one row
    fewer (pU odd, the third case of `rec`).  Every rank, the two ranks at the lane boundary n0 - 1 and n0 on their own,
    duplicates, and a NaN of each sign once in the lower lane's rows (< n0) and once in the upper lane's (>= n0)."""
    n0 = (n + 1) // 2
    assert sh.regime(n).kernel == "kth_pair_kernel<%d>" % (8 * ((n0 + 7) // 8))
    rng = np.random.default_rng(2000 + n)
    for M in sh.PAIR_M:
        s = sh.matrix(n, M, rng)
        if M >= 31:                                                  # (columns 9 .. M-10 hold the background)
            s[n0 - 1, 10] = np.float32(np.nan)                       # the lower lane's last row
            s[n0, 11] = np.float32(np.nan)                           # the upper lane's first
            s[0, 12] = sh.neg_nan()
            s[n - 1, 13] = sh.neg_nan()                              # the upper lane's last (odd n: register n0 - 2)
        else:
            s[(n0 - 1, n0, 0, n - 1)[n % 4], 0] = (np.float32(np.nan), sh.neg_nan())[(n // 4) % 2]
        d, ref = torch.from_numpy(s).to(gpu), sh.sorted_columns(s)
        for group in sh.all_ranks(n, rng):
            check(d, ref, group, (n, M, "all ranks"))
        check(d, ref, [n0 - 1, n0], (n, M, "lane boundary"))
        check(d, ref, [n0], (n, M, "upper lane's first"))
        check(d, ref, sh.duplicates(n), (n, M, "duplicates"))


# ================================================================================================ 3. kth_tile_kernel
@pytest.mark.parametrize("n", sh.TILE_N)
def test_tiles_on_both_sides_of_every_live_step(gpu, n):
    """Both sides of every step of the tile kernels' live-register count (and of every instantiation), 1025 / 1026 and
    2047 / 2048 because the two half-waves of a 32-cell tile differ by one row: ranks {0, 1, n/2, n-2, n-1} and the ten
    reference levels as one rank, as ten and as all of them (more than ten: two launches), duplicates; every column kind,
    the ones that leave a tile to its fast form apart from the ones that send it to the streaming form.  `pads` = live RPT - n
    feeds the NaN test row0 != pads: in the last matrix a cell's single NaN (either sign, first / middle / last row) is all
    that makes row 0 differ from the padding, and every other cell of its tile must NOT come out NaN."""
    reg = sh.regime(n)
    assert reg.kernel.startswith("kth_tile_kernel") and reg.pads == reg.live * (32 if reg.C32 else 16) - n >= 0
    rng = np.random.default_rng(3000 + n)
    ks = sh.tile_ranks(n)
    assert len(ks) > sh.MAXK
    groups = (ks[5:6], ks[:10], ks, sh.duplicates(n))
    for M in sh.TILE_M:
        s = sh.matrix(n, M, rng)
        d, ref = torch.from_numpy(s).to(gpu), sh.sorted_columns(s)
        for g in groups:
            check(d, ref, g, (n, M, len(g)))
    s = np.abs(rng.standard_normal((n, 70)).astype(np.float32)) + np.float32(0.5)
    s[n - 1, 3] = np.float32(np.nan)
    s[0, 40] = sh.neg_nan()
    s[n // 2, 69] = np.float32(np.nan)                               # (the second 64-cell tile, the third 32-cell one)
    s[n - 2, 33] = sh.neg_nan()
    d, ref = torch.from_numpy(s).to(gpu), sh.sorted_columns(s)
    assert ref[1].sum() == 4
    for g in groups:
        check(d, ref, g, (n, "one NaN", len(g)))


# ================================================================================================ 4. persistent loops
@pytest.mark.parametrize("n", [1025, 2048])
def test_c32_tiles_persistent_loop(gpu, n):
    """32-cell tiles with more tiles than twice the workgroups (tiles = 2 cus + 37: the first 37 workgroups run three tiles,
    each loaded into the registers of the one before): a whole tile of ties at a tile index above cus (marked in a
    workgroup's second round, redone after its third), a NaN cell and a constant cell in the last, partial tile."""
    reg = sh.regime(n)
    assert reg.C32 and reg.WGS == 1
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    tiles = 2 * cus + 37
    M = 32 * tiles - 5
    rng = np.random.default_rng(4000 + n)
    s = np.abs(rng.standard_normal((n, M), dtype=np.float32))
    tt = cus + 5
    s[:, 32 * tt:32 * tt + 32] = np.round(4 * s[:, 32 * tt:32 * tt + 32])
    s[n // 3, M - 1] = np.float32(np.nan)
    s[:, M - 2] = np.float32(1.75)
    d, ref = torch.from_numpy(s).to(gpu), sh.sorted_columns(s)
    check(d, ref, sh.levels(n), (n, M, "levels"))
    check(d, ref, [0, n - 1] + sh.duplicates(n), (n, M, "extremes and duplicates"))


@pytest.mark.parametrize("n", [241, 1025])
def test_persistent_grid_crosses_plane_boundaries(gpu, n):
    """pre_kth_axis0_planes_f32 with more than twice as many tiles as persistent workgroups, spread over six planes that
    are narrower than the grid (sp > 0) and do not divide it (sc > 0): ka_advance's wrap into the next plane is taken on
    some steps and not on others (asserted on the walk restated in select_helpers).  Rows with a pitch, a gap between the
    planes, results into a sentinel-filled output at out_rank_stride = M + 7: per plane np.sort's values, and the sentinel
    untouched everywhere else.  n = 241: 64-cell tiles, two workgroups per CU; n = 1025: 32-cell tiles."""
    reg = sh.regime(n)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    W, grid = (32 if reg.C32 else 64), reg.WGS * cus
    tpp = max(2, (2 * grid) // 5)
    while grid % tpp == 0 or tpp > grid:
        tpp -= 1
    planes = -(-(2 * grid + 1) // tpp)
    tiles = tpp * planes
    walk = sh.walk(tiles, tpp, grid)
    assert tiles > 2 * grid and walk["sp"] > 0 and walk["sc"] > 0 and walk["taken"] > 0 and walk["passed"] > 0
    assert max(len(m) for m in walk["seq"]) >= 3
    M = W * tpp - 5
    pitch, gap = M + 3, 11
    ps = n * pitch + gap
    rng = np.random.default_rng(5000 + n)
    buf = np.full(planes * ps, np.nan, np.float32)                   # (a read beside a row would turn its cell NaN)
    view = np.lib.stride_tricks.as_strided(buf, (planes, n, M), (4 * ps, 4 * pitch, 4))
    view[...] = np.abs(rng.standard_normal((planes, n, M), dtype=np.float32))
    kinds = sh.columns(n, rng)
    for p in range(planes):
        # the clean kinds in one tile, the others in another (marked, redone after the loop), at places that move with the plane
        a = (p * 7 * W + 3) % (M - 2 * W)
        view[p, :, a:a + sh.CLEAN] = kinds[:, :sh.CLEAN]
        b = (a + W * (tpp // 2)) % (M - 2 * W)
        view[p, :, b:b + len(sh.KINDS) - sh.CLEAN] = kinds[:, sh.CLEAN:]
    view[planes - 1, n // 2, M - 1] = np.float32(np.nan)             # the last cell of the last tile of the last plane
    view[0, n - 1, M - 1] = sh.neg_nan()                             # ... of the first plane: the next tile is plane 1's first
    ks = sh.levels(n)
    want = np.stack([sh.select_ref(view[p], ks) for p in range(planes)])
    d = torch.from_numpy(buf).to(gpu)
    nk = len(ks)
    flat, idx = planes_call(d, ps, pitch, planes, n, M, ks, M + 7, nk * (M + 7) + 13)
    check_framed(flat, idx, want, (n, planes, M, "ten levels"))
    ks2 = [n - 1, 0, n // 2, n // 2]
    want2 = np.stack([sh.select_ref(view[p], ks2) for p in range(planes)])
    flat, idx = planes_call(d, ps, pitch, planes, n, M, ks2, M + 7, 4 * (M + 7))
    check_framed(flat, idx, want2, (n, planes, M, "unsorted, duplicate"))


# ================================================================================================ 5. streaming forms
@pytest.mark.parametrize("n", sh.STREAM_N)
def test_streaming_thresholds_and_sweep_tails(gpu, n):
    """The streaming kernel on both sides of 4096 (tags in the histogram words / in an array of their own) and 12288 (the
    general form), at the last n its 16-bit counters hold (65535), and at sweep tails (n - 1280) mod 256 in {0, 1, 255}: the
    ten levels and both extremes (two launches), duplicates, every column kind.  Cells c and c + 32 share a counter word:
    both constant, each half of the word reaches n (0xffff at n = 65535), with ordinary cells beside them."""
    reg = sh.regime(n)
    assert reg.kernel.startswith("kth_axis0_kernel<10, false")
    rng = np.random.default_rng(6000 + n)
    ks = sorted(set(sh.levels(n)) | {0, n - 1})
    assert len(ks) > sh.MAXK
    for M in sh.STREAM_M:
        s = sh.matrix(n, M, rng)
        if M >= 64:
            s[:, 10] = np.float32(2.5)
            s[:, 42] = np.float32(-1.5)
        d, ref = torch.from_numpy(s).to(gpu), sh.sorted_columns(s)
        check(d, ref, ks, (n, M, "levels and extremes"))
        check(d, ref, sh.duplicates(n), (n, M, "duplicates"))


# ================================================================================================ 6. lanes beyond M
@pytest.mark.parametrize("n", [1, 9, 100, 168, 169, 192, 240])
def test_small_and_pair_write_nothing_beyond_the_cells(gpu, n):
    """M = 1, 31, 33 through the planes entry into a sentinel-filled output with a rank stride of M + 7: the lanes of a wave
    beyond the last cell (63, 33, 63 of the last small-kernel tile; 31, 1, 31 of the pair kernel's) write nothing."""
    assert sh.regime(n).kernel.startswith(("kth_small", "kth_pair"))
    rng = np.random.default_rng(7000 + n)
    ks = sorted({0, n // 2, n - 1} | set(sh.levels(n)))
    for M in (1, 31, 33):
        for planes in (1, 3):
            pitch = M + 2
            ps = n * pitch + 5
            buf = np.full(planes * ps, np.nan, np.float32)           # (a read beside a row would turn its cell NaN)
            view = np.lib.stride_tricks.as_strided(buf, (planes, n, M), (4 * ps, 4 * pitch, 4))
            view[...] = np.abs(rng.standard_normal((planes, n, M), dtype=np.float32))
            view[planes - 1, n // 2, M - 1] = np.float32(np.nan)
            want = np.stack([sh.select_ref(view[p], ks) for p in range(planes)])
            flat, idx = planes_call(torch.from_numpy(buf).to(gpu), ps, pitch, planes, n, M, ks, M + 7, len(ks) * (M + 7) + 3)
            check_framed(flat, idx, want, (n, M, planes))
