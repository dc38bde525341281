"""CPU tests of tests/stencil_guards.py: the guard-band allocations and the non-finite footprint sets the GPU tests rely on
(no device call).  The footprint sets are tied to the reference's arithmetic: ``F.conv3d`` / ``F.conv2d`` in float64 must
put its non-finite cells between them."""
import numpy as np
import pytest
import torch

import stencil_guards as sg


@pytest.mark.parametrize("shape,order,gaps,offset", [((2, 3, 5, 8), None, None, 0), ((2, 3, 5, 8), None, {2: 3, 1: 7}, 1),
                                                     ((2, 3, 5, 8), (0, 2, 3, 1), None, 0), ((1, 1, 1, 1), None, None, 0),
                                                     ((2, 4, 6), None, {1: 2}, 0), ((2, 3, 4, 5), (0, 1, 3, 2), {3: 1}, 0),
                                                     ((2, 3, 4, 5), None, {3: 1}, 0)])
def test_guarded_view_lies_inside_its_band(shape, order, gaps, offset):
    alloc, view = sg.guarded(shape, order, gaps, offset)
    assert view.shape == shape and view.untyped_storage().data_ptr() == alloc.untyped_storage().data_ptr()
    g = sg.guard_elems(shape, view.stride())
    grid = sorted(view.stride()[1:], reverse=True)[:3]
    assert g % 4 == 0 and g >= 4 * grid[0] + 4 * (grid[1] if len(grid) > 1 else 0)     # four planes + four rows
    assert view.storage_offset() == g + offset
    mask = sg.outside_mask(alloc, view)
    assert mask[:g + offset].all() and mask[-g:].all() and int((~mask).sum()) == view.numel()
    # writing the view never touches the band, and the band never shows in the view
    out_alloc, out, omask = sg.guarded_out(shape, order, gaps, offset)
    out.fill_(1.0)
    assert sg.untouched(out_alloc, omask) and torch.equal(omask, mask)
    out_alloc[g + offset - 1] = 0.0
    assert not sg.untouched(out_alloc, omask)
    for v in sg.POISONS:
        view.copy_(torch.arange(view.numel(), dtype=torch.float32).reshape(shape))
        sg.poison(alloc, mask, v)
        assert torch.equal(view.contiguous().reshape(-1), torch.arange(view.numel(), dtype=torch.float32))
        band = alloc[mask]
        assert torch.isnan(band).all() if v != v else bool((band == v).all())
    if gaps:
        assert int(mask.sum()) > 2 * g + offset                                       # the pitches leave poisoned gaps


def test_outside_mask_of_a_field_slice_keeps_the_neighbouring_fields_outside():
    alloc, vars_ = sg.guarded((2, 3, 2, 4, 8))
    mask = sg.outside_mask(alloc, vars_[:, 1])
    assert int((~mask).sum()) == vars_[:, 1].numel()
    sg.poison(alloc, mask, float("nan"))
    assert torch.isnan(vars_[:, 0]).all() and torch.isnan(vars_[:, 2]).all() and not torch.isnan(vars_[:, 1]).any()
    slab = vars_[:, 1, :, 1:3]                                  # an x-slab and its halo rows 0 and 3
    m2 = sg.outside_mask(alloc, vars_[:, 1, :, 0:4])
    assert int((~m2).sum()) == 2 * slab.numel()


def _conv(x, k):
    f = torch.nn.functional.conv3d if k.ndim == 3 else torch.nn.functional.conv2d
    return f(x[:, None], k[None, None], padding=[s // 2 for s in k.shape])[:, 0]


@pytest.mark.parametrize("nd", [3, 2])
def test_footprint_sets_sandwich_the_dense_conv(nd):
    """The reference's dense conv (float64, CPU) puts its non-finite cells between ``must`` and ``may`` for random dense and
    sparse 3^nd kernels with a NaN, a +inf and a -inf cell; with a lone NaN the ``must`` cells are NaN."""
    g = torch.Generator().manual_seed(5 + nd)
    grid = (6, 7, 9)[:nd] if nd == 3 else (7, 9)
    for trial in range(50):
        k = torch.randn((3,) * nd, generator=g, dtype=torch.float64)
        if trial % 2:
            k = k * (torch.rand((3,) * nd, generator=g) < 0.3)
        x = torch.randn(2, *grid, generator=g, dtype=torch.float64)
        cells = sg.bad_positions(grid)
        pick = [cells[int(i)] for i in torch.randperm(len(cells), generator=g)[:3]]
        for vals in ((float("nan"), float("inf"), float("-inf")), (float("nan"),)):
            xb, bad = x.clone(), np.zeros(x.shape, bool)
            for c, v in zip(pick, vals):
                xb[(trial % 2,) + c] = v
                bad[(trial % 2,) + c] = True
            must, may = sg.footprint(k.numpy(), bad)
            assert not (must & ~may).any()
            y = _conv(xb, k).numpy()
            nonfinite = ~np.isfinite(y)
            assert not (must & ~nonfinite).any(), "lower bound violated by the dense conv"
            assert not (nonfinite & ~may).any(), "upper bound violated by the dense conv"
            if len(vals) == 1:
                assert np.isnan(y[must]).all()
            sg.check_sandwich(y, _conv(torch.where(torch.from_numpy(bad), torch.zeros_like(x), x), k).numpy(), must, may, 1e-12,
                              lone_nan=len(vals) == 1)


def test_footprint_geometry_by_hand():
    k = np.zeros((3, 3, 3))
    k[1, 1, 0], k[1, 1, 2] = -0.5, 0.5                          # d/dy: taps at y-1, y+1
    bad = np.zeros((1, 3, 3, 5), bool)
    bad[0, 0, 0, 0] = bad[0, 1, 2, 4] = True
    must, may = sg.footprint(k, bad)
    assert sorted(map(tuple, np.argwhere(must))) == [(0, 0, 0, 1), (0, 1, 2, 3)]      # the centre tap is zero: not the cell itself
    assert may.sum() == 2 * 2 * 2 + 3 * 2 * 2 and may[0, 1, 1, 1] and may[0, 0, 1, 3] and not may[0, 2, 0, 0]
    # union: a pointwise use of the field adds the cells themselves
    must, _ = sg.footprint_union([(k, bad), (np.ones((1, 1, 1)), bad)])
    assert must.sum() == 4 and must[0, 0, 0, 0]
    # extents larger than the grid (a 7-wide kernel on a 2-wide axis) and a 1-cell axis
    m7, y7 = sg.footprint(np.ones((7, 7, 7)), np.ones((1, 1, 2, 1), bool))
    assert m7.all() and y7.all()
    cells = sg.bad_positions((1, 2, 9), extra=[(0, 1, 7), (5, 5, 5)])
    assert (0, 0, 0) in cells and (0, 1, 8) in cells and (0, 1, 7) in cells and (5, 5, 5) not in cells and len(cells) == 7


def test_check_sandwich_rejects_hidden_and_leaked_values():
    must = np.array([True, False, False])
    may = np.array([True, True, False])
    ref = np.array([1.0, 2.0, 3.0])
    sg.check_sandwich(np.array([np.nan, 7.0, 3.0]), ref, must, may, 1e-5, lone_nan=True)
    sg.check_sandwich(np.array([np.inf, np.nan, 3.0]), ref, must, may, 1e-5)
    with pytest.raises(AssertionError, match="hidden"):
        sg.check_sandwich(np.array([1.0, 2.0, 3.0]), ref, must, may, 1e-5)
    with pytest.raises(AssertionError, match="as NaN"):
        sg.check_sandwich(np.array([np.inf, 2.0, 3.0]), ref, must, may, 1e-5, lone_nan=True)
    with pytest.raises(AssertionError, match="leaked"):
        sg.check_sandwich(np.array([np.nan, 2.0, np.nan]), ref, must, may, 1e-5)
    with pytest.raises(AssertionError, match="differ"):
        sg.check_sandwich(np.array([np.nan, 2.0, 3.1]), ref, must, may, 1e-5)
