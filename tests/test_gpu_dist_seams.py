"""GPU tests (pytest -m gpu) of the four histogram-exchange sweeps of cp_pre_amd/csrc/dist_select.hip at their seams, called
through ``pipeline.HipOps.dist_*`` (and ``_lib.load_dist().pre_dist_*`` for return codes) on operands the protocol never
builds: row counts on both sides of every unroll trip and of the 65535-row counter flush, cell counts on both sides of
the 64-cell tile, owners' blocks smaller than a tile, hand-made windows, lists at the pick's capacity.  The references are
the plain numpy of tests/dist_helpers.py (checked on the CPU by tests/test_dist_seams_cpu.py, which also shows every check
below failing on a planted mistake).  Every operand lies inside a larger allocation of the test's filled with NaN or a
bit pattern, 0 or 1 element past a 16-byte boundary, which must be unchanged after each call; every comparison is bit
for bit or an exact integer count.  tests/DIST_TESTS.md says which branch each shape reaches."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dist_helpers as dh  # noqa: E402

from cp_pre_amd import pipeline  # noqa: E402

pytestmark = pytest.mark.gpu
OPS = pipeline.HipOps
PRE_OK, PRE_E_NULL, PRE_E_RANGE = 0, -1, -4

ROWS = [1, 15, 16, 17, 112, 113, 114, 127, 128, 129, 255, 256, 257, 600]
CELLS = [1, 31, 32, 33, 63, 64, 65, 129]
OWNERS = [(1, None), (2, 40), (3, 7), (5, 1), (2, 70)]                  # (W, Co); None: Co = C
PER, PLANES = 33 * 9, 3
# (c0, layout): 277 + C crosses the plane boundary at 297, which is no multiple of 64, in the time-major source
PLACES = [(0, "dense"), (5, "row_padded"), (PER - 20, "time_major"), (0, "time_major"), (5, "dense"), (PER - 20, "row_padded"),
          (2 * PER - 3, "time_major")]
LAYOUTS = {"dense": dict(), "row_padded": dict(row_pad=3), "time_major": dict(planes=PLANES, plane_pad=5)}


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    from cp_pre_amd import _lib
    _lib.load_dist()
    return torch.device("cuda:0")


def rc(name, *args):
    """The return code of one ``pre_dist_*`` entry (tensors and None as pointers, the current stream)."""
    from cp_pre_amd import _lib
    fn = getattr(_lib.load_dist(), name)
    with torch.cuda.device(0):
        r = fn(*[_lib.ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], _lib.stream())
    torch.cuda.synchronize()
    return r


def _params_of(win):
    return pipeline._dist_params(torch.from_numpy(np.ascontiguousarray(win)))[0].numpy()


def _shapes():
    out = []
    for W, Co in OWNERS:
        for C in sorted({C if Co is None else min(C, W * Co) for C in CELLS}):
            out.append((C, W, C if Co is None else Co))
    return out


# ================================================================================================ a, b: window, histogram
@pytest.mark.parametrize("n", ROWS)
def test_window_hist_and_partition_at_every_tile_and_row_seam(gpu, n):
    data = dh.cells(1, n, PLANES * PER)
    src = {(k, o): dh.Source(data, offset=o, device=gpu, **kw) for k, kw in LAYOUTS.items() for o in (0, 1)}
    shapes = _shapes()
    assert len(shapes) == 28 and {Cp % 64 == 0 for _, W, Co in shapes for Cp in [W * Co]} == {True, False}
    for i, (C, W, Co) in enumerate(shapes):
        c0, layout = PLACES[(i + n) % len(PLACES)]
        off = (i // 2 + n) % 2
        S = src[layout, off]
        win = dh.check_window(OPS, S, c0, C, W, Co, off)
        params = _params_of(win)
        for packed in (True, False):
            counts = dh.check_hist(OPS, S, c0, C, W, Co, params, packed, off)
        dh.check_partition(OPS, S, c0, C, W, Co, params, counts, off)


@pytest.mark.parametrize("W,Co", [(1, 1), (2, 40), (1, 64), (3, 43)])
def test_a_run_of_pads_only(gpu, W, Co):
    S = dh.Source(dh.cells(1, 17, 40), offset=1, device=gpu)
    win = dh.check_window(OPS, S, 40, 0, W, Co, 1)                       # C = 0 at the very end of the cells
    assert (win[0] == 0).all() and (win[1] == -1).all() and (win[2] == 1).all()
    params = _params_of(win)
    assert (params[2] == -1).all()
    for packed in (True, False):
        counts = dh.check_hist(OPS, S, 40, 0, W, Co, params, packed, 1)
        assert not counts.any()
    dh.check_partition(OPS, S, 40, 0, W, Co, params, counts, 1)


def test_window_does_not_see_a_nan_behind_the_last_row_and_cell(gpu):
    """The Source's frame and the gaps between its rows are NaN: a read one element past the last cell of any row, or past the
    last row, would clear the NaN flag of a NaN-free column."""
    for n in (1, 16, 113, 129):
        for kw in LAYOUTS.values():
            data = np.abs(np.random.default_rng(n).standard_normal((n, PLANES * 64))).astype(np.float32)
            S = dh.Source(data, device=gpu, **kw)
            M = data.shape[1]
            win = dh.check_window(OPS, S, M - 64, 64, 1, 64)
            assert (win[2] == 1).all()
            win = dh.check_window(OPS, S, M - 33, 33, 2, 17, 1)
            assert (win[2] == 1).all()


# ---- counter capacity and the chunk flush
CAP_N = [65535, 65536, 65537, 131071]


@pytest.fixture(scope="module")
def capacity():
    """(data [131071, 96], hand-made params for 128 cells, the reference buckets): the window [0.0, 1.0) with sf = 256, what a
    rank sees when other ranks hold the rest of the window."""
    n = max(CAP_N)
    rng = np.random.default_rng(65535)
    x = rng.random((n, 96), dtype=np.float32)
    assert x.max() < 1.0
    x[:, 0:16] = 0.5                                                      # bucket 128 takes every row
    x[::4, 32:48] = 0.5                                                   # their word partners: rand, every fourth row 0.5
    x[65535:, 16:32] = 0.75                                               # the second trip must add, not overwrite
    x[:, 48:64] = 0.25                                                    # the upper half-word, full
    x[:, 64:96] = 0.5                                                     # partners 96..127: pads, or absent
    params = np.zeros((3, 128), np.int32)
    params[0] = np.int32(-2 ** 31)                                        # klo = key(0.0) = 2^31
    params[1] = np.float32(256.0).view(np.int32)
    params[2, 96:] = -1
    b = np.trunc(x * np.float32(256.0)).astype(np.int16)                  # (v - 0.0) * 256, truncated: exact in fp32
    assert b.min() >= 0 and b.max() <= 255
    return x, params, b


@pytest.mark.parametrize("Co", [128, 96])
@pytest.mark.parametrize("n", CAP_N)
def test_hist_counter_capacity_and_chunk_flush(gpu, capacity, n, Co):
    x, params, b = capacity
    params = np.ascontiguousarray(params[:, :Co])
    S = dh.Source(x[:n], offset=n % 2, device=gpu)
    p = dh.put(params, 1, gpu)
    hist = dh.framed((1, dh.NB, Co), torch.int32, 1, gpu, fill=dh.HIST_POISON)
    hist.view.fill_(dh.HIST_POISON)
    OPS.dist_hist(S.src, 0, 96, 1, Co, p.view, False, hist.view)
    got = hist.np()[0].T.astype(np.int64)                                 # [Co, NB]
    assert hist.untouched() and p.untouched() and S.untouched()
    ref = np.zeros((Co, dh.NB), np.int64)
    for c in range(96):
        ref[c] = np.bincount(b[:n, c], minlength=dh.NB)
    assert ref[0, 128] == n and ref[48, 64] == n and ref[20, 192] >= n - 65535 and ref[95, 128] == n
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (bad[:8].tolist(), got[got != ref][:8].tolist(), ref[got != ref][:8].tolist())
    if n == 65537 and Co == 128:                                          # the map agrees with the reference restated here
        assert np.array_equal(dh.bucket_ref(x[:300], params)[0], b[:300].astype(np.int64))


# ---- packed capacity
def _quarters(n, C):
    x = np.empty((n, C), np.float32)
    x[:, 0::3] = 0.25                                                     # bucket 64: the low half of word 64
    x[:, 1::3] = 0.75                                                     # bucket 192: the high half of the same word
    x[:, 2::3] = np.where(np.arange(n) % 2 == 0, np.float32(0.25), np.float32(0.75))[:, None]
    return x


def _unit_params(Cp, C):
    params = np.zeros((3, Cp), np.int32)
    params[0] = np.int32(-2 ** 31)
    params[1] = np.float32(256.0).view(np.int32)
    params[2, C:] = -1
    return params


@pytest.mark.parametrize("n,W,Co", [(32767, 1, 70), (10922, 3, 24)])
def test_packed_hist_holds_32767_in_either_half(gpu, n, W, Co):
    S = dh.Source(_quarters(n, 70), offset=1, device=gpu)
    counts = dh.check_hist(OPS, S, 0, 70, W, Co, _unit_params(W * Co, 70), True, 1)
    assert counts[0, 64] == n and counts[1, 192] == n and counts[2, 64] == (n + 1) // 2 and counts[2, 192] == n // 2
    assert counts[33, 64] == n and counts[34, 192] == n                  # cells of the upper LDS half-word too


@pytest.mark.parametrize("n,W,Co", [(32768, 1, 70), (10923, 3, 24)])
def test_packed_hist_refuses_a_count_that_could_carry(gpu, n, W, Co):
    S = dh.Source(_quarters(n, 70), device=gpu)
    p = dh.put(_unit_params(W * Co, 70), 0, gpu)
    hist = dh.framed((W, dh.NB // 2, Co), torch.int32, 0, gpu)
    before = hist.bits()
    assert rc("pre_dist_hist_f32", *S.src, 0, 70, W, Co, p.view, 1, hist.view) == PRE_E_RANGE
    assert torch.equal(hist.bits(), before) and hist.untouched()
    big = dh.framed((W, dh.NB, Co), torch.int32, 0, gpu)                   # one int32 per bucket takes it
    assert rc("pre_dist_hist_f32", *S.src, 0, 70, W, Co, p.view, 0, big.view) == PRE_OK
    assert big.np()[0, 64, 0] == n and big.untouched()


# ================================================================================================ c: collect, pick
@pytest.fixture(scope="module")
def collect_case(gpu):
    data = dh.cells(1, 600, 70)
    C, W, Co = 70, 2, 37                                                  # four pads, an owner's block that ends inside a tile
    src = [dh.Source(data, offset=o, device=gpu, row_pad=o) for o in (0, 1)]
    params = _params_of(dh.window_ref(data, W * Co))
    b, part = dh.bucket_ref(data, params)
    occupied = [np.unique(b[:, c]) if part[c] else np.zeros(0, np.int64) for c in range(C)]
    return src, (0, C, W, Co), params, occupied, b


@pytest.mark.parametrize("nS", [1, 2, 63, 64])
def test_collect_slots_sentinels_and_a_short_count(gpu, collect_case, nS):
    src, (c0, C, W, Co), params, occupied, b = collect_case
    want = np.full((W * Co, nS), -1, np.int32)
    for c in range(C):
        occ = occupied[c][-nS:] if c % 2 else occupied[c][:nS]           # ascending; fewer than nS: trailing -1 slots
        want[c, :len(occ)] = occ
    assert (want[0] >= 0).all() and want[21, 0] >= 0
    want[21] = -1                                                         # a taking-part cell that wants nothing
    if nS > 2:
        assert (want[:C] >= 0).sum(1).max() == nS and ((want[:C] >= 0).sum(1) == 2).any()
    held = np.array([[(b[:, c] == want[c, s]).sum() if want[c, s] >= 0 else 0 for s in range(nS)] for c in range(C)])
    short = [tuple(int(i) for i in np.argwhere(held > 1)[k]) for k in (0, -1)]
    for off in (0, 1):
        dh.check_collect(OPS, src[off], c0, C, W, Co, params, want, short=short, offset=off)
        dh.check_collect(OPS, src[off], c0, C, W, Co, params, want, offset=off)


def test_collect_without_a_send_buffer_and_beyond_64_slots(gpu, collect_case):
    src, (c0, C, W, Co), params, occupied, _ = collect_case
    S, Cp = src[0], W * Co
    want = np.full((Cp, 3), -1, np.int32)
    for c in range(C):
        want[c, :len(occupied[c][:3])] = occupied[c][:3]
    p, w_ = dh.put(params, 0, gpu), dh.put(want, 0, gpu)
    cnt, off = dh.put(np.zeros((Cp, 3), np.int32), 0, gpu), dh.put(np.zeros((Cp, 3), np.int64), 0, gpu)
    OPS.dist_collect(S.src, c0, C, W, Co, p.view, w_.view, cnt.view, off.view, torch.empty(0, device=gpu))    # send = None
    assert rc("pre_dist_collect_f32", *S.src, c0, C, W, Co, p.view, w_.view, 3, cnt.view, off.view, None) == PRE_OK
    assert all(x.untouched() for x in (p, w_, cnt, off)) and S.untouched()
    assert torch.equal(off.view, torch.zeros_like(off.view)) and torch.equal(cnt.view, torch.zeros_like(cnt.view))
    send = dh.framed(16, torch.float32, 0, gpu)
    w65, c65, o65 = (dh.put(np.zeros((Cp, 65), d), 0, gpu) for d in (np.int32, np.int32, np.int64))
    for nS in (65, 0, -1):
        assert rc("pre_dist_collect_f32", *S.src, c0, C, W, Co, p.view, w65.view, nS, c65.view, o65.view, send.view) == PRE_E_RANGE
    assert send.untouched() and bool(send.view.isnan().all())


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name", sorted(dh.pick_cases()))
def test_pick_on_hand_made_lists(gpu, name, offset):
    lists, asks, W, nk = dh.pick_cases()[name]
    got = dh.check_pick(OPS, lists, asks, W, nk, gpu, offset)
    if name == "lengths":                                                 # the list of 2049 kept its sentinel, 2048 did not
        assert (got[:6, 6] == dh.PICK_SENTINEL).all() and (got[:6, 5] != dh.PICK_SENTINEL).all()
        assert (got[6:9, 6] != dh.PICK_SENTINEL).all() and (got[9] == dh.PICK_SENTINEL).all()


def test_pick_asked_for_an_empty_list_leaves_the_output(gpu):
    """vals = None with all-empty lists, and slots that point at them: nothing is read, nothing is written."""
    empty = np.zeros(0, np.float32)
    dh.check_pick(OPS, [[[empty] * 3] * 2] * 4, [[(0, 0), (1, 0), (-1, 0)]] * 4, 3, 3, gpu)


def test_pick_refuses_65_ranks_and_65_slots(gpu):
    cnt, off = dh.put(np.zeros((1, 2, 65), np.int32), 0, gpu), dh.put(np.zeros((1, 2, 65), np.int64), 0, gpu)
    slot, rnk = dh.put(np.zeros((2, 65), np.int32), 0, gpu), dh.put(np.zeros((2, 65), np.int32), 0, gpu)
    out = dh.framed((65, 2), torch.float32, 0, gpu)
    before = out.bits()
    for nS, nk in ((65, 1), (1, 65), (0, 1), (1, 0)):
        assert rc("pre_dist_pick_f32", None, cnt.view, off.view, 1, 2, nS, slot.view, rnk.view, nk, out.view) == PRE_E_RANGE
    assert rc("pre_dist_pick_f32", None, cnt.view, off.view, 1, 2 ** 31, 1, slot.view, rnk.view, 1, out.view) == PRE_E_RANGE
    assert torch.equal(out.bits(), before) and out.untouched()
    assert rc("pre_dist_pick_f32", None, cnt.view, off.view, 1, 2, 64, slot.view, rnk.view, 64, out.view) == PRE_OK
    assert torch.equal(out.bits(), before) and out.untouched()           # (every list empty: still nothing written)


# ================================================================================================ d: the four sweeps together
@pytest.mark.parametrize("plus", [0, 7])
@pytest.mark.parametrize("W,n_local", [(1, 37), (2, 150), (3, 129), (3, 600), (5, 409)])
def test_simulated_ranks_equal_numpy_sort(gpu, W, n_local, plus):
    data = dh.cells(W, n_local)
    N = W * n_local
    assert N <= dh.PICK_CAP
    ks = dh.ranks(N)
    q, t = dh.check_simulate(OPS, data, W, ks, -(-100 // W) + plus, gpu, offset=(W + plus) % 2)
    assert q.shape == (len(ks), 100) and 0 < t["longest"] <= dh.PICK_CAP and t["packed"]
    if plus:                                                              # one int32 per bucket, a run that starts inside
        dh.check_simulate(OPS, data, W, ks, -(-91 // W) + 2, gpu, c0=9, packed=False, offset=W % 2)


def test_the_protocol_at_world_size_one_equals_the_simulation(gpu):
    import torch.distributed as dist
    created = False
    if dist.is_initialized():
        if not (dist.get_backend() == "nccl" and dist.get_world_size() == 1):
            pytest.skip("a process group of another kind is already up in this process")
    else:
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=gpu)
        created = True
    try:
        data = dh.cells(1, 600)
        alphas = [float(a) for a in np.arange(0.05, 0.95 + 0.1, 0.1) if 0.0 <= np.ceil(601 * (1 - a)) / 600 <= 1.0]
        ks = pipeline._ranks(600, alphas)
        st = {}
        x = torch.from_numpy(data).to(gpu).view(600, 4, 25)
        got = pipeline._marginal_histogram(x, alphas, dist.group.WORLD, OPS, 4 << 30, st).reshape(len(ks), 100)
        torch.cuda.synchronize()
        q, t = dh.check_simulate(OPS, data, 1, ks, 100, gpu)
        assert st["runs"] == 1 and st["fallback_runs"] in (0, 1), st
        dh.ident(got.cpu().numpy(), q)                                   # the select is exact on either route
    finally:
        if created:
            dist.destroy_process_group()


# ================================================================================================ e: return codes
def test_every_refusal_returns_its_code_and_writes_nothing(gpu):
    n, per, planes = 4, 8, 3
    S = dh.Source(dh.cells(1, n, per * planes), planes=planes, plane_pad=3, device=gpu)
    base, PS, RS = S.src[0], S.src[1], S.src[2]
    W, Co, C = 2, 8, 16
    big = 65536                                                           # (tables large enough for the refused W too)
    win = dh.framed((3, big), torch.int32, 0, gpu)
    hist = dh.framed((1, dh.NB, big), torch.int32, 0, gpu)
    send = dh.framed(64, torch.float32, 0, gpu)
    p = dh.put(_unit_params(big, 0), 0, gpu)
    want, cnt, off = (dh.put(np.zeros((big, 1), d), 0, gpu) for d in (np.int32, np.int32, np.int64))
    outs = (win, hist, send)
    good = dict(scores=base, PS=PS, RS=RS, planes=planes, n=n, per=per, c0=0, C=C, W=W, Co=Co)
    bad = [dict(scores=None), dict(n=0), dict(n=-1), dict(per=0), dict(planes=0), dict(W=0), dict(Co=0), dict(Co=-3),
           dict(C=-1), dict(c0=-1), dict(C=W * Co + 1), dict(c0=9), dict(c0=per * planes, C=1), dict(RS=per - 1),
           dict(PS=per - 1), dict(W=65536, Co=1, C=1)]

    def window_of(**kw):
        assert rc("pre_dist_window_f32", *{**good, **kw}.values(), win.view) == PRE_OK, kw
        return win.np().reshape(-1)[:3 * W * Co].reshape(3, -1)
    # accepted: the baseline; one row, whose stride is then free; one plane, whose stride is then free; the run's last cell
    assert np.array_equal(window_of(), dh.window_ref(S.rows(0, C), W * Co))
    assert np.array_equal(window_of(n=1, RS=per - 1), dh.window_ref(S.rows(0, C)[:1], W * Co))
    assert np.array_equal(window_of(planes=1, PS=0, C=per), dh.window_ref(S.rows(0, per), W * Co))
    assert np.array_equal(window_of(c0=per * planes - C), dh.window_ref(S.rows(per * planes - C, C), W * Co))
    before = [o.bits() for o in outs]
    for b_ in bad:
        a = list({**good, **b_}.values())
        assert rc("pre_dist_window_f32", *a, win.view) == PRE_E_NULL, b_
        assert rc("pre_dist_hist_f32", *a, p.view, 0, hist.view) == PRE_E_NULL, b_
        assert rc("pre_dist_hist_f32", *a, p.view, 1, hist.view) == PRE_E_NULL, b_
        assert rc("pre_dist_collect_f32", *a, p.view, want.view, 1, cnt.view, off.view, send.view) == PRE_E_NULL, b_
    a = list(good.values())
    assert rc("pre_dist_window_f32", *a, None) == PRE_E_NULL
    assert rc("pre_dist_hist_f32", *a, None, 0, hist.view) == PRE_E_NULL
    assert rc("pre_dist_hist_f32", *a, p.view, 0, None) == PRE_E_NULL
    for k in range(4):
        tabs = [p.view, want.view, cnt.view, off.view]
        tabs[k] = None
        assert rc("pre_dist_collect_f32", *a, tabs[0], tabs[1], 1, tabs[2], tabs[3], send.view) == PRE_E_NULL, k
    for o, b_ in zip(outs, before):
        assert torch.equal(o.bits(), b_) and o.untouched()
    # the pick: null tables, W beyond 64 * 1024, Co <= 0
    Wp = 64 * 1024 + 1
    pc, po = dh.put(np.zeros((Wp, 1, 1), np.int32), 0, gpu), dh.put(np.zeros((Wp, 1, 1), np.int64), 0, gpu)
    slot, rnk = dh.put(np.zeros((1, 1), np.int32), 0, gpu), dh.put(np.zeros((1, 1), np.int32), 0, gpu)
    out = dh.framed((1, 1), torch.float32, 0, gpu)
    ob = out.bits()
    vals = dh.put(np.ones(4, np.float32), 0, gpu)
    ok = [vals.view, pc.view, po.view, 1, 1, 1, slot.view, rnk.view, 1, out.view]
    for k in (1, 2, 6, 7, 9):
        a = list(ok)
        a[k] = None
        assert rc("pre_dist_pick_f32", *a) == PRE_E_NULL, k
    for k, v in ((3, Wp), (3, 0), (3, -1), (4, 0), (4, -1)):
        a = list(ok)
        a[k] = v
        assert rc("pre_dist_pick_f32", *a) == PRE_E_NULL, (k, v)
    assert torch.equal(out.bits(), ob) and out.untouched()
    assert rc("pre_dist_pick_f32", *ok) == PRE_OK and torch.equal(out.bits(), ob)             # (an empty list: nothing written)
    ok[3] = 64 * 1024
    assert rc("pre_dist_pick_f32", *ok) == PRE_OK and torch.equal(out.bits(), ob)             # the most segments accepted
