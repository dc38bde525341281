"""MI355X tests of solution bounds by sample acceptance (``libcp_pre_bounds.so``): ``sample_envelope``, ``sample_bounds``
(joint, threshold, cellwise) and ``SampleBounds`` against fresh numpy restatements of the reference recipe
(``u[accepted].min(0)`` / ``.max(0)``, Tests/test_advection_inv_sampling_marginal.py:312-359, 363-387, 476-491), equal
with NaN at the same places (``np.array_equal`` on the rest), on every layout the package produces."""
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from cp_pre_amd import _lib, ode, pipeline
from cp_pre_amd import inductive_cp as icp
from cp_pre_amd import sample_bounds as sb
from cp_pre_amd.residuals import PRE_NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    assert os.path.exists(_lib.BOUNDS_SO_PATH), "libcp_pre_bounds.so is built by __graft_entry__.build()"
    _lib.load_bounds()
    return torch.device("cuda:0")


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _same(a, b):
    a, b = _np(a), _np(b)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])


def _envelope_np(u, acc):
    """The recipe restated in numpy: per level the min / max over the accepted samples (+inf / -inf for none)."""
    lo = np.full((acc.shape[0],) + u.shape[1:], np.inf, np.float32)
    hi = np.full((acc.shape[0],) + u.shape[1:], -np.inf, np.float32)
    for k in range(acc.shape[0]):
        if acc[k].any():
            lo[k], hi[k] = u[acc[k]].min(0), u[acc[k]].max(0)
    return lo, hi, acc.sum(1).astype(np.int64)


def _check_envelope(u_dev, acc, squeeze=False):
    lo, hi, cnt = sb.sample_envelope(u_dev, torch.from_numpy(acc[0] if squeeze else acc).to(u_dev.device))
    want = _envelope_np(u_dev.cpu().numpy(), acc)
    if squeeze:
        want = tuple(w[0] for w in want)
    assert lo.device == u_dev.device
    assert _same(lo, want[0]) and _same(hi, want[1]) and np.array_equal(_np(cnt), want[2])


def _layouts(gpu, gen):
    """(name, device view) of every layout: tall, wide, cropped, the reference callers' Nt-fastest view, row_padded and
    time_major buffers."""
    tall = torch.randn(1 << 16, 100, device=gpu, generator=gen)
    wide = torch.randn(64, 6, 66, 66, device=gpu, generator=gen)
    ntf = torch.randn(48, 30, 31, 20, device=gpu, generator=gen).permute(0, 3, 1, 2)      # [n, Nt, Nx, Ny], Nt fastest
    rp = pipeline.row_padded(96, (8, 9, 10), device=gpu)
    rp.copy_(torch.randn(96, 8, 9, 10, device=gpu, generator=gen))
    tm = pipeline.time_major(96, (8, 9, 10), pad=64, device=gpu)
    tm.copy_(torch.randn(96, 8, 9, 10, device=gpu, generator=gen))
    return [("tall", tall), ("wide", wide), ("cropped", wide[:, 1:-1, 1:-1, 1:-1]), ("ntfast", ntf),
            ("ntfast_cropped", ntf[:, 1:-1, 1:-1, 1:-1]), ("row_padded", rp), ("time_major", tm)]


@pytest.mark.parametrize("nk", [1, 10, 16, 17])
def test_envelope_random_masks_every_layout(gpu, nk):
    gen = torch.Generator(device=gpu).manual_seed(nk)
    rng = np.random.default_rng(nk)
    for name, u in _layouts(gpu, gen):
        n = u.shape[0]
        u[(3,) + (0,) * (u.dim() - 1)] = float("nan")    # (written through the view, where it lies)
        acc = rng.random((nk, n)) < 0.4
        acc[:, 3] = True                                 # NaN in an accepted sample
        if nk > 2:
            acc[1] = False                          # a level that accepts nothing
        _check_envelope(u, acc)
        if nk == 1:
            _check_envelope(u, acc, squeeze=True)


@pytest.mark.parametrize("kind", ["grow", "shrink"])
def test_envelope_nested_levels(gpu, kind):
    gen = torch.Generator(device=gpu).manual_seed(5)
    rng = np.random.default_rng(5)
    for name, u in _layouts(gpu, gen):
        n, nk = u.shape[0], 10
        if kind == "grow":
            acc = np.arange(nk)[:, None] >= rng.integers(0, nk + 1, n)[None, :]
        else:
            acc = np.arange(nk)[:, None] <= rng.integers(-1, nk, n)[None, :]
        _check_envelope(u, acc)


def test_nan_in_accepted_and_rejected_samples_and_all_rejected_level(gpu):
    rng = np.random.default_rng(1)
    u = rng.standard_normal((300, 7, 9)).astype(np.float32)
    u[4, 2, 3] = np.nan                    # accepted at level 0 only
    u[5, 1, 1] = np.nan                    # never accepted
    acc = np.zeros((3, 300), bool)
    acc[0, ::2] = True
    acc[0, 5] = False
    acc[2, 1::3] = True
    lo, hi, cnt = sb.sample_envelope(u, acc)                    # numpy in, numpy out
    assert isinstance(lo, np.ndarray)
    want = _envelope_np(u, acc)
    assert _same(lo, want[0]) and _same(hi, want[1]) and np.array_equal(cnt, want[2])
    assert np.isnan(lo[0, 2, 3]) and np.isnan(hi[0, 2, 3]) and not np.isnan(lo[:, 1, 1]).any()
    assert np.all(lo[1] == np.inf) and np.all(hi[1] == -np.inf) and cnt[1] == 0


# ---------------------------------------------------------------- the rules
def _ns_case(gpu):
    torch.manual_seed(0)
    dt, dx, dy = 0.01, 1 / 64, 1 / 64
    vars_ = torch.rand(96, 3, 8, 16, 64, device=gpu) + 0.5
    res = PRE_NS(dt, dx, dy).residual(vars_, boundary=True)[..., 1:-1, 1:-1, 1:-1]
    u = vars_[:, 0]
    return u, res


def _joint_want(u, res, q, m, c):
    un = u.cpu().numpy()
    acc = np.stack([_np(icp.filter_sims_joint(icp._loop_sets(qk, c, m), res)) for qk in q])
    return _envelope_np(un, acc)


def test_joint_on_a_fused_ns_residual(gpu):
    u, res = _ns_case(gpu)
    mod = icp.modulation_func(res, None)
    js = icp.ncf_metric_joint(res, None, mod)
    q = torch.stack([torch.as_tensor(icp.calibrate(js, js.shape[0], a), device=gpu).reshape(())
                     for a in (0.05, 0.2, 0.4, 0.6, 0.8, 0.95)]).to(torch.float32)
    centre = res[0]                                                       # prediction_sets[0][0]: per cell
    for m, c in ((None, None), (mod, None), (mod, centre), (None, res * 0.5)):
        qq = q if m is not None else q * 0.05
        lo, hi, cnt = sb.sample_bounds(u, res, qq, rule="joint", modulation=m, centre=c)
        want = _joint_want(u, res, qq, m, c)
        assert _same(lo, want[0]) and _same(hi, want[1]) and np.array_equal(_np(cnt), want[2]), (m is None, c is None)
    # float64 levels (Python floats): per-level acceptance, one envelope
    qf = [float(v) for v in q.cpu()]
    lo, hi, cnt = sb.sample_bounds(u, res, qf, rule="joint", modulation=mod)
    want = _joint_want(u, res, qf, mod, None)
    assert _same(lo, want[0]) and _same(hi, want[1]) and np.array_equal(_np(cnt), want[2])


def test_joint_on_an_ode_residual(gpu):
    gen = torch.Generator(device=gpu).manual_seed(2)
    t = torch.linspace(0, 5, 100, device=gpu)
    amp = 1 + 0.05 * torch.randn(1 << 15, 1, device=gpu, generator=gen)
    x = amp * torch.cos(1.7 * t)[None, :] + 0.01 * torch.randn(1 << 15, 100, device=gpu, generator=gen)
    res = ode.SHO(1.7, float(t[1] - t[0])).residual([x])
    scale = res.abs().amax(1).cpu().numpy()
    q = torch.from_numpy(np.quantile(scale, np.linspace(0.05, 0.95, 10)).astype(np.float32)).to(gpu)
    lo, hi, cnt = sb.sample_bounds(x, res, q, rule="joint")
    want = _joint_want(x, res, q, None, None)
    assert _same(lo, want[0]) and _same(hi, want[1]) and np.array_equal(_np(cnt), want[2])
    assert 0 < want[2][0] < want[2][-1] < x.shape[0]


def test_threshold_equals_the_per_level_filter_and_counts_equal_rowcount(gpu):
    u, res = _ns_case(gpu)
    q = torch.quantile(res.abs().reshape(-1)[::7], torch.linspace(0.5, 0.99, 12, device=gpu)).to(torch.float32)
    centre = res[1]
    for c in (None, centre):
        lo, hi, cnt = sb.sample_bounds(u, res, q, rule="threshold", threshold=0.9, centre=c)
        acc = np.stack([_np(icp.filter_sims_within_bounds(*icp._loop_sets(qk, c, None), res, 0.9, within=True)) for qk in q])
        want = _envelope_np(u.cpu().numpy(), acc)
        assert _same(lo, want[0]) and _same(hi, want[1]) and np.array_equal(_np(cnt), want[2])
    # the multi-level counts of one pass equal pre_cov_rowcount_f32 level by level
    rd = res.contiguous()
    n, M = rd.shape[0], rd[0].numel()
    counts = torch.zeros(q.shape[0], n, dtype=torch.int32, device=gpu)
    sb.rowcount_launch(res, q, centre, None, counts)
    for k in range(q.shape[0]):
        lo_k = (centre - q[k]).contiguous()
        hi_k = (centre + q[k]).contiguous()
        one = torch.zeros(n, dtype=torch.int32, device=gpu)
        _lib.check(_lib.load().pre_cov_rowcount_f32(_lib.ptr(rd), _lib.ptr(lo_k), _lib.ptr(hi_k), n, M, 0, 0, _lib.ptr(one),
                                                    _lib.stream()), "pre_cov_rowcount_f32")
        assert torch.equal(counts[k], one), k


def _cellwise_want(u, r, lo_b, hi_b):
    un, rn = _np(u), _np(r)
    nk = lo_b.shape[0]
    lo = np.full((nk,) + un.shape[1:], np.inf, np.float32)
    hi = np.full((nk,) + un.shape[1:], -np.inf, np.float32)
    cnt = np.zeros((nk,) + un.shape[1:], np.int32)
    for k in range(nk):
        ins = (rn >= lo_b[k]) & (rn <= hi_b[k])
        for idx in np.ndindex(*un.shape[1:]):            # the per-cell loop
            sel = un[(slice(None),) + idx][ins[(slice(None),) + idx]]
            cnt[k][idx] = sel.size
            if sel.size:
                lo[k][idx], hi[k][idx] = sel.min(), sel.max()
    return lo, hi, cnt


def test_cellwise_equals_the_per_cell_loop(gpu):
    gen = torch.Generator(device=gpu).manual_seed(4)
    for n, cells in ((512, (3, 6, 7)), (1 << 14, (20,))):
        u = torch.randn(n, *cells, device=gpu, generator=gen)
        r = torch.randn(n, *cells, device=gpu, generator=gen)
        u[7].view(-1)[0] = float("nan")
        r[9].view(-1)[1] = float("nan")                  # NaN in r: outside
        m = 0.5 + torch.rand(cells, device=gpu, generator=gen)
        c = 0.2 * torch.randn(cells, device=gpu, generator=gen)
        qs = torch.linspace(0.2, 2.0, 5, device=gpu)
        qc = torch.rand(5, *cells, device=gpu, generator=gen) * 2
        mn, cn = m.cpu().numpy(), c.cpu().numpy()
        for q, mm, cc in ((qs, None, None), (qs, m, c), (qc, None, c), (qc, m, None)):
            qn = q.cpu().numpy().reshape((5,) + (1,) * len(cells) if q.dim() == 1 else q.shape)
            hw = qn * mn if mm is not None else qn
            lo_b, hi_b = ((-hw, hw) if cc is None else (cn - hw, cn + hw))
            lo_b, hi_b = np.broadcast_to(lo_b, (5,) + cells), np.broadcast_to(hi_b, (5,) + cells)
            got = sb.sample_bounds(u, r, q, rule="cellwise", modulation=mm, centre=cc)
            want = _cellwise_want(u, r, lo_b, hi_b)
            for g, w in zip(got, want):
                assert _same(g, w), (n, q.dim(), mm is None, cc is None)
    # float64 q: numpy's float64 bounds, decided exactly through the inward rounding
    u = torch.randn(400, 5, 8, device=gpu, generator=gen)
    r = torch.randn(400, 5, 8, device=gpu, generator=gen)
    qf = [0.3, 0.7000000001, 1.1]
    c64 = np.asarray(0.1 * torch.randn(5, 8, generator=torch.Generator().manual_seed(0)).numpy(), np.float64)
    got = sb.sample_bounds(u, r, qf, rule="cellwise", centre=c64)
    lo_b = np.stack([c64 - q for q in qf])
    hi_b = np.stack([c64 + q for q in qf])
    want = _cellwise_want(u, r.cpu().numpy().astype(np.float64), lo_b, hi_b)
    for g, w in zip(got, want):
        assert _same(g, w)


# ---------------------------------------------------------------- streaming, graphs, a group
def test_two_slabs_equal_one_call_and_add_slab_captures_in_a_graph(gpu):
    gen = torch.Generator(device=gpu).manual_seed(6)
    u = torch.randn(2000, 4, 50, device=gpu, generator=gen)
    acc = torch.rand(10, 2000, device=gpu, generator=gen) < 0.3
    want = sb.sample_envelope(u, acc)
    b = sb.SampleBounds(10, (4, 50), gpu)
    b.add_slab(u[:700], acc[:, :700])
    b.add_slab(u[700:], acc[:, 700:])
    for g, w in zip(b.finish(), want):
        assert _same(g, w)
    g2 = sb.SampleBounds(10, (4, 50), gpu)
    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):                           # warm-up: code objects load outside the capture
        sb.SampleBounds(10, (4, 50), gpu).add_slab(u[:700], acc[:, :700])
    torch.cuda.current_stream(gpu).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g2.add_slab(u[:700], acc[:, :700])
        g2.add_slab(u[700:], acc[:, 700:])
    graph.replay()
    torch.cuda.synchronize()
    for g, w in zip(g2.finish(), want):
        assert _same(g, w)


_CHILD = textwrap.dedent("""
    import os, sys
    import numpy as np
    import torch
    import torch.distributed as dist
    sys.path.insert(0, {root!r})
    from cp_pre_amd import sample_bounds as sb
    port, out = sys.argv[1], sys.argv[2]
    dev = torch.device("cuda:0")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:" + port, rank=0, world_size=1, device_id=dev)
    try:
        z = np.load(os.path.join(out, "data.npz"))
        u, acc = torch.from_numpy(z["u"]).to(dev), torch.from_numpy(z["acc"]).to(dev)
        b = sb.SampleBounds(acc.shape[0], tuple(u.shape[1:]), dev, group=dist.group.WORLD)
        b.add_slab(u[:50], acc[:, :50])
        b.add_slab(u[50:], acc[:, 50:])
        lo, hi, cnt = b.finish()
        torch.cuda.synchronize()
        np.savez(os.path.join(out, "r0.npz"), lo=lo.cpu().numpy(), hi=hi.cpu().numpy(), cnt=cnt.cpu().numpy())
    finally:
        dist.destroy_process_group()
""")


def test_finish_on_a_one_rank_rccl_group_equals_the_local_result(gpu, tmp_path):
    rng = np.random.default_rng(8)
    u = rng.standard_normal((130, 6, 11)).astype(np.float32)
    u[3, 1, 1] = np.nan
    acc = rng.random((5, 130)) < 0.5
    acc[0, 3] = True
    acc[4] = False
    np.savez(tmp_path / "data.npz", u=u, acc=acc)
    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(root=ROOT))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    p = subprocess.Popen([sys.executable, str(script), str(port), str(tmp_path)])
    try:
        code = p.wait(timeout=240)
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
    assert code == 0
    z = np.load(tmp_path / "r0.npz")
    want = sb.sample_envelope(u, acc)
    assert _same(z["lo"], want[0]) and _same(z["hi"], want[1]) and np.array_equal(z["cnt"], want[2])
    assert np.isnan(z["lo"][0, 1, 1]) and np.all(z["lo"][4] == np.inf) and z["cnt"][4] == 0
