"""MI355X tests of sample_bounds' host-side guards on the device path: a numpy accept mask given to SampleBounds.add_slab
is moved to the slab's device (and equals the device-mask result), host slabs are refused before any launch, and the
joint rule with a per-cell centre on the reference callers' Nt-fastest residual equals the per-level filter."""
import numpy as np
import pytest
import torch

from cp_pre_amd import inductive_cp as icp
from cp_pre_amd import sample_bounds as sb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    return torch.device("cuda:0")


def _same(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])


def test_host_masks_are_moved_and_host_slabs_refused(gpu):
    gen = torch.Generator(device=gpu).manual_seed(11)
    u = torch.randn(600, 7, 30, device=gpu, generator=gen)
    acc = np.random.default_rng(11).random((4, 600)) < 0.5
    want = sb.sample_envelope(u, torch.from_numpy(acc).to(gpu))
    b = sb.SampleBounds(4, (7, 30), gpu)
    b.add_slab(u[:250], acc[:, :250])                         # numpy mask
    b.add_slab(u[250:], torch.from_numpy(acc[:, 250:]))       # host torch mask
    got = b.finish()
    for g, w in zip(got, want):
        assert g.device == w.device and _same(g, w)
    with pytest.raises(TypeError):
        b.add_slab(u[:10].cpu(), acc[:, :10])                 # a host slab never reaches the kernel
    with pytest.raises(TypeError):
        sb.envelope_launch(u, torch.from_numpy(acc), [1, 2], b.lo, b.hi, b.count)     # nor a host mask


def test_joint_per_cell_centre_on_an_nt_fastest_residual(gpu):
    gen = torch.Generator(device=gpu).manual_seed(12)
    r = torch.randn(200, 20, 24, 16, device=gpu, generator=gen).permute(0, 3, 1, 2)[:, 1:-1, 1:-1, 1:-1]
    u = torch.randn(200, 16, 20, 24, device=gpu, generator=gen)
    centre = 0.1 * torch.randn(r.shape[1:], device=gpu, generator=gen)          # dense, logical order
    q = torch.tensor([3.2, 3.6, 4.0, 4.6], device=gpu)
    lo, hi, cnt = sb.sample_bounds(u, r, q, rule="joint", centre=centre)
    un = u.cpu().numpy()
    for k in range(4):
        keep = icp.filter_sims_joint([centre - q[k], centre + q[k]], r).cpu().numpy()
        assert cnt[k].item() == keep.sum()
        if keep.any():
            assert np.array_equal(lo[k].cpu().numpy(), un[keep].min(0)) and np.array_equal(hi[k].cpu().numpy(), un[keep].max(0))
        else:
            assert torch.all(lo[k] == float("inf")) and torch.all(hi[k] == float("-inf"))
    assert cnt[0].item() <= cnt[-1].item() and cnt[-1].item() > 0
