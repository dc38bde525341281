"""MI355X tests of coverage at every calibration level in one pass (``libcp_pre_cov.so``): ``emp_cov_levels``,
``emp_cov_joint_levels``, ``filter_sims_joint_levels`` and ``pipeline.CoverageLevels`` against the goldens and against the
loop of the existing per-level functions, bit for bit (``==`` on float64), on every layout the package produces."""
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from cp_pre_amd import _lib, pipeline
from cp_pre_amd import inductive_cp as icp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    assert os.path.exists(_lib.COV_SO_PATH), "libcp_pre_cov.so is built by __graft_entry__.build()"
    _lib.load_cov()
    return torch.device("cuda:0")


def _golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name), allow_pickle=False)


def _loop(qs, y, centre=None, modulation=None, joint=False):
    out = []
    for q in qs:
        hw = q if modulation is None else q * modulation
        sets = [-hw, hw] if centre is None else [centre - hw, centre + hw]
        out.append(icp.emp_cov_joint(sets, y) if joint else icp.emp_cov(sets, y))
    return np.array(out, np.float64)


# ---------------------------------------------------------------- goldens
def test_golden_curves(gpu):
    g = _golden("conformal.npz")
    for n in (7, 100, 256):
        r, mod = g[f"res|{n}"], g[f"mod|{n}"]
        idx = [i for i in range(10) if f"cov|{n}|{i}" in g.files]
        q = np.stack([g[f"qhat|{n}|{i}"] for i in idx])
        qj = np.array([g[f"qhat_joint|{n}|{i}"] for i in idx], np.float32)
        want = np.array([float(g[f"cov|{n}|{i}"]) for i in idx])
        want_j = np.array([float(g[f"cov_joint|{n}|{i}"]) for i in idx])
        got = icp.emp_cov_levels(q, r)
        assert got.dtype == np.float64 and np.array_equal(got, want), n
        assert np.array_equal(icp.emp_cov_joint_levels(qj, r, mod), want_j), n
        assert np.array_equal(icp.emp_cov_levels(torch.from_numpy(q).to(gpu), torch.from_numpy(r).to(gpu)), want), n


def test_reference_executed_centred_joint_loop(gpu):
    """conformal_ref.npz's joint coverage, produced by executing the reference's loop: q = fp32 of the q-hats, centre
    pred[:, 1:-1, 1:-1] against val[:, 1:-1, 1:-1], passed as views the way the loop crops them."""
    g = _golden("conformal_ref.npz")
    for n in (7, 100, 256):
        pred, val, mod = g[f"pred|{n}"], g[f"val|{n}"], g[f"mod|{n}"]
        q = g[f"qhats|{n}"].astype(np.float32)
        want = g[f"cov_joint|{n}"]
        assert np.array_equal(icp.emp_cov_joint_levels(q, val[:, 1:-1, 1:-1], mod, centre=pred[:, 1:-1, 1:-1]), want), n
        pd, vd = torch.from_numpy(pred).to(gpu), torch.from_numpy(val).to(gpu)
        got = icp.emp_cov_joint_levels(torch.from_numpy(q).to(gpu), vd[:, 1:-1, 1:-1], torch.from_numpy(mod).to(gpu),
                                       centre=pd[:, 1:-1, 1:-1])
        assert np.array_equal(got, want), n
        flags = icp.filter_sims_joint_levels(q, val[:, 1:-1, 1:-1], mod, centre=pred[:, 1:-1, 1:-1])
        assert isinstance(flags, np.ndarray) and flags.shape == (len(q), val.shape[0])
        assert np.array_equal(flags.mean(1), want)


# ---------------------------------------------------------------- fuzz against the per-level loop
def _layout(x, kind, dev):
    """x [n, T, X, Y] (host) as a device tensor of the given layout, same logical values."""
    n, T, X, Y = x.shape
    if kind == "contiguous":
        return x.to(dev)
    if kind == "offset":                                 # unaligned base: one float into its buffer
        buf = torch.empty(x.numel() + 1, device=dev)
        t = buf[1:].view(x.shape)
        return t.copy_(x)
    if kind == "nt_fastest":                             # the surrogate's [n, X, Y, T] memory
        return x.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)
    if kind == "cropped":                                # a crop of a larger slab
        big = torch.empty(n, T + 2, X + 2, Y + 2, device=dev)
        big[:, 1:-1, 1:-1, 1:-1] = x.to(dev)
        return big[:, 1:-1, 1:-1, 1:-1]
    if kind == "row_padded":
        return pipeline.row_padded(n, (T, X, Y), device=dev).copy_(x.to(dev))
    if kind == "time_major":
        return pipeline.time_major(n, (T, X, Y), pad=64, device=dev).copy_(x.to(dev))
    raise ValueError(kind)


def _specials(y, c, q, m, rng):
    """NaN / inf in every operand, q = 0, negative q, subnormal q*m, y exactly on a bound."""
    yf, cf, qf, mf = (t.view(-1) for t in (y, c, q, m))
    for t in (yf, cf, qf, mf):
        idx = torch.from_numpy(rng.choice(t.numel(), size=min(4, t.numel()), replace=False))
        t[idx[:1]] = float("nan")
        t[idx[1:2]] = float("inf")
        t[idx[2:3]] = float("-inf")
    qf[rng.integers(qf.numel())] = 0.0
    qf[rng.integers(qf.numel())] = -0.5
    qf[rng.integers(qf.numel())] = 1e-30
    mf[rng.integers(mf.numel())] = 1e-10                 # 1e-30 * 1e-10 is subnormal (or 0) in fp32
    M = m.numel()
    j = int(rng.integers(M))
    yf[j] = qf[j]                                        # sample 0, cell j: exactly on +q of level 0
    yf[(y.shape[0] - 1) * M + j] = -qf[j]


CASES = [(1, (3, 5, 7)), (3, (2, 4, 8)), (7, (5, 9, 13)), (1000, (3, 6, 10)), (4097, (1, 3, 20))]


@pytest.mark.parametrize("n,cells", CASES)
def test_marginal_levels_equal_the_loop(gpu, n, cells):
    rng = np.random.default_rng(n)
    y = torch.from_numpy(rng.standard_normal((n,) + cells).astype(np.float32))
    c = torch.from_numpy((0.4 * rng.standard_normal((n,) + cells)).astype(np.float32))
    m = torch.from_numpy((0.5 + rng.random(cells)).astype(np.float32))
    for nk in (1, 10, 16, 17):
        q = torch.from_numpy(np.abs(rng.standard_normal((nk,) + cells)).astype(np.float32) * 1.3)
        _specials(y, c, q, m, rng)
        yd, qd = y.to(gpu), q.to(gpu)
        base = _loop(qd, yd)
        base_c = _loop(qd, yd, centre=c.to(gpu))
        for kind in ("contiguous", "offset", "nt_fastest", "cropped", "row_padded", "time_major"):
            yl = _layout(y, kind, gpu)
            assert np.array_equal(icp.emp_cov_levels(qd, yl), base), (kind, nk)
            for ckind in ("contiguous", kind, "nt_fastest"):
                got = icp.emp_cov_levels(qd, yl, centre=_layout(c, ckind, gpu))
                assert np.array_equal(got, base_c), (kind, ckind, nk)
    # numpy in, numpy out; float64 levels take the per-level functions
    q = np.abs(rng.standard_normal((4,) + cells)).astype(np.float32)
    yn = y.numpy()
    assert np.array_equal(icp.emp_cov_levels(q, yn), _loop(q, yn))
    q64 = q.astype(np.float64)
    assert np.array_equal(icp.emp_cov_levels(q64, yn), _loop(q64, yn))
    assert np.array_equal(icp.emp_cov_levels([float(v) for v in q[:, 0, 0, 0]], yn),
                          _loop([float(v) for v in q[:, 0, 0, 0]], yn))


@pytest.mark.parametrize("n,cells", CASES)
def test_joint_levels_equal_the_loop(gpu, n, cells):
    rng = np.random.default_rng(100 + n)
    y = torch.from_numpy(rng.standard_normal((n,) + cells).astype(np.float32))
    c = torch.from_numpy((0.3 * rng.standard_normal((n,) + cells)).astype(np.float32))
    m = torch.from_numpy((0.5 + rng.random(cells)).astype(np.float32))
    for nk in (1, 10, 16, 17):
        qj = torch.from_numpy(np.sort(rng.random(nk).astype(np.float32) * 6.0))
        qq = qj.clone().reshape(nk, 1, 1, 1).expand((nk,) + cells).contiguous()
        _specials(y, c, qq, m, rng)                      # (specials in y, c, m; a scalar q keeps its own below)
        qj[0] = 0.0 if nk > 1 else qj[0]
        yd, qd, md, cd = y.to(gpu), qj.to(gpu), m.to(gpu), c.to(gpu)
        base = _loop(qd, yd, modulation=md, joint=True)
        base_c = _loop(qd, yd, centre=cd, modulation=md, joint=True)
        flags_c = torch.stack([icp.filter_sims_joint([cd - q * md, cd + q * md], yd) for q in qd])
        for kind in ("contiguous", "offset", "nt_fastest", "cropped", "row_padded", "time_major"):
            yl = _layout(y, kind, gpu)
            assert np.array_equal(icp.emp_cov_joint_levels(qd, yl, md), base), (kind, nk)
            for ckind in ("contiguous", kind):
                cl = _layout(c, ckind, gpu)
                assert np.array_equal(icp.emp_cov_joint_levels(qd, yl, md, centre=cl), base_c), (kind, ckind, nk)
                f = icp.filter_sims_joint_levels(qd, yl, md, centre=cl)
                assert isinstance(f, torch.Tensor) and f.device == yl.device and torch.equal(f, flags_c), (kind, ckind)
        # per-cell q in the joint form, and float64 levels
        assert np.array_equal(icp.emp_cov_joint_levels(qq.to(gpu), yd, md), _loop(qq.to(gpu), yd, modulation=md, joint=True))
    q64 = [float(v) for v in qj]
    assert np.array_equal(icp.emp_cov_joint_levels(q64, y.numpy(), m.numpy()), _loop(q64, y.numpy(), modulation=m.numpy(), joint=True))


def test_empty_test_set_is_refused(gpu):
    with pytest.raises(ValueError):
        icp.emp_cov_levels(np.ones((2, 3), np.float32), np.zeros((0, 3), np.float32))


# ---------------------------------------------------------------- no copy of y
def test_cropped_view_is_not_copied(gpu):
    nk = 10
    big = torch.randn(64, 66, 258, 258, device=gpu)                   # 1.1 GB
    y = big[:, 1:-1, 1:-1, 1:-1]
    M = y[0].numel()
    q = torch.rand(nk, *y.shape[1:], device=gpu) * 2
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu)
    before = torch.cuda.max_memory_allocated(gpu)
    got = icp.emp_cov_levels(q, y)
    rise = torch.cuda.max_memory_allocated(gpu) - before
    assert rise < nk * M * 4 + (64 << 20), rise
    want = np.array([float(((y >= -q[k]) & (y <= q[k])).sum()) / y.numel() for k in range(nk)])
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- full size
def test_c4_per_rank_marginal_full_size(gpu):
    gen = torch.Generator(device=gpu).manual_seed(4)
    shape = (1024, 62, 254, 254)
    cal = torch.randn(200, *shape[1:], device=gpu, generator=gen).abs_()
    alphas = [0.05 + 0.1 * i for i in range(10)]
    q = pipeline.marginal_qhat(cal, alphas)
    del cal
    y = torch.randn(*shape, device=gpu, generator=gen)
    assert np.array_equal(icp.emp_cov_levels(q, y), _loop(q, y))
    c = torch.randn(*shape, device=gpu, generator=gen).mul_(0.1)
    assert np.array_equal(icp.emp_cov_levels(q, y, centre=c), _loop(q, y, centre=c))


def test_c5_joint_shard_full_size(gpu):
    gen = torch.Generator(device=gpu).manual_seed(5)
    shape = (8192, 198, 510)
    cal = torch.randn(*shape, device=gpu, generator=gen)
    mod = icp.modulation_func(cal, None)
    scores = icp.ncf_metric_joint(cal, None, mod)
    alphas = [0.05 + 0.1 * i for i in range(10)]
    q = icp.calibrate_multi(scores, scores.shape[0], alphas)
    del cal
    y = torch.randn(*shape, device=gpu, generator=gen)
    assert np.array_equal(icp.emp_cov_joint_levels(q, y, mod), _loop(q, y, modulation=mod, joint=True))


# ---------------------------------------------------------------- graph capture: add_slab never synchronises
def test_add_slab_captures_in_a_graph(gpu):
    gen = torch.Generator(device=gpu).manual_seed(9)
    y = torch.randn(300, 7, 40, 33, device=gpu, generator=gen)
    q = torch.rand(10, 7, 40, 33, device=gpu, generator=gen) * 2
    eager = pipeline.CoverageLevels(300, 10, gpu)
    eager.add_slab(y, q)
    want = eager.finish()
    cov = pipeline.CoverageLevels(300, 10, gpu)
    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):                   # warm-up: code objects load outside the capture
        icp.cov_operands(y)
        pipeline.HipOps.cov_levels(y, q, None, None, pipeline.HipOps.zeros_coverage(10, 300, False, gpu))
    torch.cuda.current_stream(gpu).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cov.add_slab(y, q)
    cov.acc.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(cov.finish(), want)
    cov.acc.zero_()
    graph.replay()
    graph.replay()                               # counts accumulate: twice the cells, the same fractions
    cov.cells = 2 * y[0].numel()
    assert np.array_equal(cov.finish(), want)


# ---------------------------------------------------------------- sharded, in fresh child processes
_CHILD = textwrap.dedent("""
    import os, sys
    import numpy as np
    import torch
    import torch.distributed as dist
    sys.path.insert(0, {root!r})
    from cp_pre_amd import pipeline
    rank, world, port, backend, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    dev = torch.device("cuda:0")
    kw = dict(device_id=dev) if backend == "nccl" else {{}}
    dist.init_process_group(backend, init_method="tcp://127.0.0.1:" + port, rank=rank, world_size=world, **kw)
    try:
        z = np.load(os.path.join(out, "data.npz"))
        cut = [int(v) for v in z["cut"]]
        y = torch.from_numpy(z["y"][cut[rank]:cut[rank + 1]]).to(dev)
        c = torch.from_numpy(z["c"][cut[rank]:cut[rank + 1]]).to(dev)
        q, qj, m = (torch.from_numpy(z[k]).to(dev) for k in ("q", "qj", "m"))
        res = {{}}
        for joint in (False, True):
            cov = pipeline.CoverageLevels(y.shape[0], q.shape[0], dev, joint=joint, group=dist.group.WORLD)
            for a0, a1 in ((0, 2), (2, 5)):             # slabs along the first cell axis
                if joint:
                    cov.add_slab(y[:, a0:a1], qj, centre=c[:, a0:a1], modulation=m[a0:a1])
                else:
                    cov.add_slab(y[:, a0:a1], q[:, a0:a1].contiguous(), centre=c[:, a0:a1])
            res[str(int(joint))] = cov.finish()
        torch.cuda.synchronize()
        np.savez(os.path.join(out, "r%d.npz" % rank), **res)
    finally:
        dist.destroy_process_group()
""")


def _sharded(tmp_path, world, backend, gpu):
    rng = np.random.default_rng(world)
    n, cells = 301, (5, 17, 23)
    y = rng.standard_normal((n,) + cells).astype(np.float32)
    c = (0.2 * rng.standard_normal((n,) + cells)).astype(np.float32)
    q = np.abs(rng.standard_normal((10,) + cells)).astype(np.float32) * 1.5
    qj = np.linspace(0.5, 4.0, 10).astype(np.float32)
    m = (0.5 + rng.random(cells)).astype(np.float32)
    cut = np.array([0, 100, n][:1] + ([n] if world == 1 else [100, n]))
    np.savez(tmp_path / "data.npz", y=y, c=c, q=q, qj=qj, m=m, cut=cut)
    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(root=ROOT))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(world), str(port), backend, str(tmp_path)])
             for r in range(world)]
    try:
        codes = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert codes == [0] * world, codes
    yd, cd = torch.from_numpy(y).to(gpu), torch.from_numpy(c).to(gpu)
    want_m = icp.emp_cov_levels(torch.from_numpy(q).to(gpu), yd, centre=cd)
    want_j = icp.emp_cov_joint_levels(torch.from_numpy(qj).to(gpu), yd, torch.from_numpy(m).to(gpu), centre=cd)
    assert np.array_equal(want_m, _loop(torch.from_numpy(q).to(gpu), yd, centre=cd))
    for r in range(world):
        z = np.load(tmp_path / f"r{r}.npz")
        assert np.array_equal(z["0"], want_m) and np.array_equal(z["1"], want_j), r


def test_sharded_two_ranks_sharing_one_gpu(gpu, tmp_path):
    _sharded(tmp_path, 2, "gloo", gpu)


def test_sharded_on_rccl_at_world_size_one(gpu, tmp_path):
    _sharded(tmp_path, 1, "nccl", gpu)
