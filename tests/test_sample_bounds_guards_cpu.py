"""CPU tests of what cp_pre_amd.sample_bounds refuses or copies before any launch: host operands never reach a kernel
(a host pointer faults the GPU), a host accept mask is moved to the slab's device, ``SampleBounds.finish`` returns new
tensors, and a per-cell centre is laid out so that the coverage pass reads it beside the residual without a full copy."""
import numpy as np
import pytest
import torch

from cp_pre_amd import inductive_cp as icp
from cp_pre_amd import sample_bounds as sb

CELLS = (3, 5, 4)


class RecordingOps:
    """Test double of sample_bounds.HipBoundsOps that records the devices the envelope is handed (torch-CPU arithmetic)."""
    seen = []

    @staticmethod
    def zeros_bounds(nk, M, device):
        return sb.HipBoundsOps.zeros_bounds(nk, M, "cpu")

    @staticmethod
    def envelope(u, accept, order, lo, hi, count):
        RecordingOps.seen.append((u.device, accept.device, type(accept)))
        flat = u.permute(0, *order).reshape(u.shape[0], -1)
        for k in range(accept.shape[0]):
            sel = flat[accept[k].bool()]
            if sel.shape[0]:
                lo[k] = torch.minimum(lo[k], sel.amin(0))
                hi[k] = torch.maximum(hi[k], sel.amax(0))
            count[k] += sel.shape[0]


def test_launches_refuse_host_operands_before_touching_the_library():
    u = torch.zeros((4,) + CELLS)
    acc = torch.ones(2, 4, dtype=torch.bool)
    lo, hi, cnt = sb.HipBoundsOps.zeros_bounds(2, 60, "cpu")
    with pytest.raises(TypeError):
        sb.envelope_launch(u, acc, [1, 2, 3], lo, hi, cnt)
    with pytest.raises(TypeError):
        sb.rowcount_launch(u, torch.ones(2), None, None, torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(TypeError):
        sb.cellwise_launch(u, u, [1, 2, 3], lo, hi, torch.zeros(2, 60, dtype=torch.int32), q=torch.ones(2))


def test_add_slab_refuses_a_host_slab_with_the_device_back_end():
    b = sb.SampleBounds(2, CELLS, "cpu")                   # default ops: the HIP passes
    with pytest.raises(TypeError):
        b.add_slab(torch.zeros((4,) + CELLS), np.ones((2, 4), bool))
    b2 = sb.SampleBounds(2, CELLS, "cpu", ops=RecordingOps)
    with pytest.raises(TypeError):
        b2.add_slab(torch.zeros((4,) + CELLS, device="meta"), np.ones((2, 4), bool))     # not on this object's device


def test_add_slab_moves_a_host_mask_to_the_slab_device():
    RecordingOps.seen = []
    rng = np.random.default_rng(0)
    u = rng.standard_normal((9,) + CELLS).astype(np.float32)
    acc = rng.random((2, 9)) < 0.5
    b = sb.SampleBounds(2, CELLS, "cpu", ops=RecordingOps)
    b.add_slab(torch.from_numpy(u[:5]), acc[:, :5])                  # numpy mask
    b.add_slab(torch.from_numpy(u[5:]), torch.from_numpy(acc[:, 5:]))
    assert len(RecordingOps.seen) == 2
    assert all(ud == ad and t is torch.Tensor for ud, ad, t in RecordingOps.seen)
    lo, hi, cnt = b.finish()
    for k in range(2):
        assert np.array_equal(lo[k].numpy(), u[acc[k]].min(0)) and np.array_equal(hi[k].numpy(), u[acc[k]].max(0))
    assert np.array_equal(cnt.numpy(), acc.sum(1))


def test_finish_returns_new_tensors():
    u = np.arange(2 * 60, dtype=np.float32).reshape((2,) + CELLS)
    b = sb.SampleBounds(1, CELLS, "cpu", ops=RecordingOps)
    b.add_slab(torch.from_numpy(u[:1]), np.ones((1, 1), bool))
    lo, hi, cnt = b.finish()
    lo0, hi0, cnt0 = lo.clone(), hi.clone(), cnt.clone()
    b.add_slab(torch.from_numpy(u[1:]) + 1000, np.ones((1, 1), bool))
    assert torch.equal(lo, lo0) and torch.equal(hi, hi0) and torch.equal(cnt, cnt0)
    assert not torch.equal(b.finish()[1], hi0)


def _residuals():
    base = torch.arange(5 * 8 * 9 * 10, dtype=torch.float32).reshape(5, 8, 9, 10)
    ntf = base.permute(0, 3, 1, 2)                                   # Nt-fastest view
    return {"cropped": base[:, 1:-1, 1:-1, 1:-1], "ntfast": ntf, "ntfast_cropped": ntf[:, 1:-1, 1:-1, 1:-1],
            "contiguous": base}


@pytest.mark.parametrize("name", ["cropped", "ntfast", "ntfast_cropped", "contiguous"])
def test_per_cell_centre_is_read_beside_the_residual_without_a_copy(name):
    r = _residuals()[name]
    c = torch.randn(r.shape[1:])                                      # a dense per-cell centre in logical order
    cl = sb.centre_like(c, r)
    assert torch.equal(cl, c.expand(r.shape))                         # the same values
    yv, cv, ext, ys, cs, order = icp.cov_operands(r, cl)
    assert yv.data_ptr() == r.data_ptr()                              # the residual where it lies
    assert cs[0] == 0                                                 # the centre not copied per sample
    flat = cv.as_strided((r.shape[0],) + tuple(ext), (cs[0], cs[1], cs[2], 1)).reshape(r.shape[0], -1)
    assert torch.equal(flat, c.expand(r.shape).permute(0, *order).reshape(r.shape[0], -1))
