"""CPU tests of solution bounds by sample acceptance (cp_pre_amd.sample_bounds, libcp_pre_bounds.so's exported ABI).

SampleBounds runs sharded under `gloo` at world sizes 2 and 3 with unequal n_local, on a torch-CPU back end that is a test
double of sample_bounds.HipBoundsOps; every rank's result must equal one process over the concatenated set, which must
equal a fresh numpy restatement of the reference recipe (``u[accepted].min(0)`` / ``.max(0)``, Tests/
test_advection_inv_sampling_marginal.py:476-491).  The device passes are covered by the -m gpu tests."""
import os
import re
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cp_pre_amd import _lib
from cp_pre_amd import sample_bounds as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NK = 4
CELLS = (3, 5, 4)


class CpuBoundsOps:
    """sample_bounds.HipBoundsOps in torch-CPU arithmetic (test double): masked min / max that propagate NaN."""

    @staticmethod
    def zeros_bounds(nk, M, device):
        return sb.HipBoundsOps.zeros_bounds(nk, M, "cpu")

    @staticmethod
    def envelope(u, accept, order, lo, hi, count):
        flat = u.permute(0, *order).reshape(u.shape[0], -1)
        for k in range(accept.shape[0]):
            sel = flat[accept[k].bool()]
            if sel.shape[0]:
                lo[k] = torch.minimum(lo[k], sel.amin(0))
                hi[k] = torch.maximum(hi[k], sel.amax(0))
            count[k] += sel.shape[0]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _data(n_total, seed=0):
    """Samples with NaN in accepted and rejected samples, a level that accepts nothing, and a stretch of samples (the
    middle rank's) that no level accepts."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n_total,) + CELLS).astype(np.float32)
    acc = rng.random((NK, n_total)) < 0.5
    acc[2] = False                                   # a level with no accepted sample
    acc[:, 8:13] = False                             # samples no level accepts (a whole rank at world 3)
    u[1, 0, 0, 0] = np.nan
    acc[0, 1] = True                                 # NaN in an accepted sample
    u[9, 1, 1, 1] = np.nan                           # NaN in a rejected sample only
    u[3, 2, 2, 2] = -0.0
    return u, acc


def _numpy(u, acc):
    """The reference recipe restated: per level, min / max over the accepted samples (+inf / -inf when there is none)."""
    lo = np.full((acc.shape[0],) + u.shape[1:], np.inf, np.float32)
    hi = np.full((acc.shape[0],) + u.shape[1:], -np.inf, np.float32)
    for k in range(acc.shape[0]):
        if acc[k].any():
            lo[k], hi[k] = u[acc[k]].min(0), u[acc[k]].max(0)
    return lo, hi, acc.sum(1).astype(np.int64)


def _shares(world, n_total):
    cuts = {2: [0, 8, n_total], 3: [0, 8, 13, n_total]}[world]
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


def _worker(rank, world, port, n_total, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        u, acc = _data(n_total)
        s0, s1 = _shares(world, n_total)[rank]
        b = sb.SampleBounds(NK, CELLS, "cpu", group=dist.group.WORLD, ops=CpuBoundsOps)
        for a0 in range(s0, s1, 3):                  # slabs of up to three samples
            a1 = min(s1, a0 + 3)
            b.add_slab(torch.from_numpy(u[a0:a1]), torch.from_numpy(acc[:, a0:a1]))
        lo, hi, count = b.finish()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), lo=lo.numpy(), hi=hi.numpy(), count=count.numpy())
    finally:
        dist.destroy_process_group()


def _equal(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_envelope_equals_one_process(tmp_path, world):
    n_total = 21
    mp.spawn(_worker, args=(world, _free_port(), n_total, str(tmp_path)), nprocs=world, join=True)
    u, acc = _data(n_total)
    want = _numpy(u, acc)
    one = sb.SampleBounds(NK, CELLS, "cpu", ops=CpuBoundsOps)
    one.add_slab(torch.from_numpy(u), torch.from_numpy(acc))
    single = [t.numpy() for t in one.finish()]
    for w, s in zip(want, single):
        assert _equal(w, s)
    assert np.isnan(want[0][0, 0, 0, 0]) and not np.isnan(want[0][:, 1, 1, 1]).any()
    assert np.all(want[0][2] == np.inf) and np.all(want[1][2] == -np.inf) and want[2][2] == 0
    for r in range(world):
        got = np.load(tmp_path / f"r{r}.npz")
        for key, w in zip(("lo", "hi", "count"), single):
            assert _equal(got[key], w), (world, r, key)


def _record_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    orig = {nm: getattr(dist, nm) for nm in ("all_reduce", "all_gather", "broadcast", "barrier", "reduce",
                                             "all_gather_into_tensor", "reduce_scatter_tensor", "all_to_all_single")}

    def wrap(nm, fn):
        def rec(*a, **kw):
            t = a[0] if a and isinstance(a[0], torch.Tensor) else None
            calls.append((nm, str(t.dtype) if t is not None else None, tuple(t.shape) if t is not None else None))
            return fn(*a, **kw)
        return rec
    try:
        for nm, fn in orig.items():
            setattr(dist, nm, wrap(nm, fn))
        u, acc = _data(14 + 5 * rank, seed=rank)
        b = sb.SampleBounds(NK, CELLS, "cpu", group=dist.group.WORLD, ops=CpuBoundsOps)
        b.add_slab(torch.from_numpy(u), torch.from_numpy(acc))
        after = repr(calls)
        b.finish()
        np.save(os.path.join(out_dir, f"calls{rank}.npy"), np.array([after, repr(calls)]))
    finally:
        for nm, fn in orig.items():
            setattr(dist, nm, fn)
        dist.destroy_process_group()


def test_add_slab_communicates_nothing_and_finish_two_fixed_size_collectives(tmp_path):
    mp.spawn(_record_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    M = int(np.prod(CELLS))
    for r in range(2):
        after, total = np.load(tmp_path / f"calls{r}.npy")
        assert after == "[]"
        assert total == repr([("all_reduce", "torch.float32", (2, NK, M)), ("all_reduce", "torch.int64", (NK + NK * M,))])


def test_permuted_slabs_accumulate_in_the_first_slabs_order():
    u, acc = _data(12)
    b = sb.SampleBounds(NK, CELLS, "cpu", ops=CpuBoundsOps)
    first = torch.from_numpy(u[:6]).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)    # last cell axis slowest
    b.add_slab(first, torch.from_numpy(acc[:, :6]))
    b.add_slab(torch.from_numpy(u[6:]), torch.from_numpy(acc[:, 6:]))
    for w, g in zip(_numpy(u, acc), b.finish()):
        assert _equal(w, g.numpy())


# ---------------------------------------------------------------- argument validation and level handling
def test_bad_arguments_are_refused_before_any_device_work():
    u = np.zeros((4,) + CELLS, np.float32)
    with pytest.raises(ValueError):
        sb.sample_envelope(np.zeros((0,) + CELLS, np.float32), np.zeros(0, bool))            # n == 0
    with pytest.raises(ValueError):
        sb.sample_envelope(u, np.zeros((0, 4), bool))                                          # nk == 0
    with pytest.raises(ValueError):
        sb.sample_envelope(u, np.zeros((2, 5), bool))                                          # n mismatch
    with pytest.raises(TypeError):
        sb.sample_envelope(u.astype(np.float64), np.ones(4, bool))                             # not fp32
    with pytest.raises(TypeError):
        sb.sample_envelope(torch.zeros((4,) + CELLS, dtype=torch.float16), np.ones(4, bool))
    r = np.zeros((4, 3, 5), np.float32)
    with pytest.raises(ValueError):
        sb.sample_bounds(u, r, np.ones(2, np.float32), rule="cellwise")                        # cellwise cell mismatch
    with pytest.raises(ValueError):
        sb.sample_bounds(u, np.zeros((3,) + CELLS, np.float32), np.ones(2, np.float32))        # sample count mismatch
    with pytest.raises(ValueError):
        sb.sample_bounds(u, u, np.ones(2, np.float32), rule="marginal")                         # unknown rule
    with pytest.raises(ValueError):
        sb.sample_bounds(u, u, np.zeros(0, np.float32))                                         # nk == 0
    with pytest.raises(ValueError):
        sb.sample_bounds(u, u, [])
    with pytest.raises(ValueError):
        sb.sample_bounds(u, u, np.ones(2, np.float32), rule="threshold", threshold=1.5)
    with pytest.raises(ValueError):
        sb.sample_bounds(u, r, np.ones(2, np.float32), modulation=np.ones(CELLS, np.float32))  # modulation of u's cells
    with pytest.raises(TypeError):
        sb.sample_bounds(u.astype(np.float64), u, np.ones(2, np.float32))
    b = sb.SampleBounds(NK, CELLS, "cpu", ops=CpuBoundsOps)
    with pytest.raises(ValueError):
        b.add_slab(torch.zeros((3, 2)), torch.ones(NK, 3, dtype=torch.bool))                  # other cells
    with pytest.raises(ValueError):
        b.add_slab(torch.zeros((3,) + CELLS), torch.ones(NK - 1, 3, dtype=torch.bool))        # other level count
    with pytest.raises(TypeError):
        b.add_slab(torch.zeros((3,) + CELLS, dtype=torch.float64), torch.ones(NK, 3, dtype=torch.bool))
    with pytest.raises(ValueError):
        sb.SampleBounds(0, CELLS, "cpu", ops=CpuBoundsOps)


def test_level_route_fp32_one_pass_float64_per_level():
    q32 = np.array([0.5, 1.0], np.float32)
    assert sb.level_route(q32)[1] == "f32"
    assert sb.level_route([np.float32(0.5), np.float32(1.0)])[1] == "f32"
    assert sb.level_route(torch.tensor([0.5, 1.0]))[1] == "f32"
    assert sb.level_route([0.5, 1.0])[1] == "f64"                                  # Python floats: numpy's float64
    assert sb.level_route(q32.astype(np.float64))[1] == "f64"
    assert sb.level_route(q32, centre=np.zeros(3))[1] == "f64"                     # a float64 centre
    assert sb.level_route(q32, modulation=np.ones(3))[1] == "f64"
    assert sb.level_route(q32, modulation=np.ones(3, np.float32))[1] == "f32"


def _kernel_scheme(masks, vals, nk):
    """The envelope kernel's register scheme (csrc/sample_bounds.hip) restated: a mask that is a run up to the last level
    updates the pair of its first level, a run from level 0 the pair of its last level, any other mask every accepting
    level's own pair; the epilogue folds the first kind forwards and the second backwards."""
    full = (1 << nk) - 1
    A, D, R = ([[np.inf, -np.inf] for _ in range(nk)] for _ in range(3))

    def upd(p, v):
        p[0], p[1] = min(p[0], v), max(p[1], v)
    for m, v in zip(masks, vals):
        if m == 0:
            continue
        low = m & -m
        if m + low == full + 1:
            upd(A[low.bit_length() - 1], v)
        elif m & (m + 1) == 0:
            upd(D[m.bit_length() - 1], v)
        else:
            for k in range(nk):
                if m >> k & 1:
                    upd(R[k], v)
    out = []
    for k in range(nk):
        pairs = [R[k]] + A[:k + 1] + D[k:]
        out.append((min(p[0] for p in pairs), max(p[1] for p in pairs)))
    return out


@pytest.mark.parametrize("kind", ["grow", "shrink", "arbitrary"])
def test_nested_and_arbitrary_level_masks(kind):
    rng = np.random.default_rng(3)
    nk, n = 6, 200
    vals = rng.standard_normal(n)
    if kind == "grow":                          # sets grow with k: a run from the first accepting level to the last
        first = rng.integers(0, nk + 1, n)
        acc = np.arange(nk)[:, None] >= first[None, :]
    elif kind == "shrink":                      # sets shrink with k (alphas 0.05 .. 0.95): a run from level 0
        last = rng.integers(-1, nk, n)
        acc = np.arange(nk)[:, None] <= last[None, :]
    else:
        acc = rng.random((nk, n)) < 0.5
    masks = [int(sum(int(acc[k, s]) << k for k in range(nk))) for s in range(n)]
    got = _kernel_scheme(masks, vals, nk)
    for k in range(nk):
        sel = vals[acc[k]]
        want = (sel.min(), sel.max()) if sel.size else (np.inf, -np.inf)
        assert got[k] == want, (kind, k)


# ---------------------------------------------------------------- the library's ABI
def test_bounds_library_exports_what_its_header_declares():
    so = _lib.BOUNDS_SO_PATH
    assert os.path.exists(so), "libcp_pre_bounds.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(os.path.join(ROOT, "include", "cp_pre_bounds.h")).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared and exported == declared
    assert set(_lib.BOUNDS_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_BOUNDS_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_BOUNDS_ABI_VERSION
    assert int(re.search(r"#define\s+PRE_BOUNDS_MAX_LEVELS\s+(\d+)", header).group(1)) == _lib.PRE_BOUNDS_MAX_LEVELS


def test_workspace_query_needs_no_device():
    """The workspace size is host arithmetic on the shape: none for wide shapes, partials for tall ones."""
    lib = _lib.load_bounds()
    from ctypes import byref, c_int64
    b = c_int64(-1)
    assert lib.pre_bounds_cellwise_workspace(1024, 16, 256, 256, 10, byref(b)) == 0 and b.value == 0
    assert lib.pre_bounds_envelope_workspace(1024, 16, 256, 256, 10, byref(b)) == 0 and b.value == 4096   # the masks
    assert lib.pre_bounds_envelope_workspace(1 << 20, 1, 1, 100, 10, byref(b)) == 0 and b.value > (1 << 22)
    assert lib.pre_bounds_envelope_workspace(0, 1, 1, 100, 10, byref(b)) == _lib.PRE_E_NULL
    assert lib.pre_bounds_envelope_workspace(8, 1, 1, 100, 0, byref(b)) == _lib.PRE_E_NULL
