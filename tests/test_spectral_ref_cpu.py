"""The fp64 reference of the spectral tests checked against itself, without a GPU (spectral_helpers.py).

On every shape and kernel test_gpu_spectral.py uses: the FFT reference agrees with the direct-space circular sum wherever
that sum is defined (1e-10 * max|ref|: both are fp64, a generous margin over an fp64 FFT's round-off), and the kernels
of the inverting modes keep |K^ + eps| >= 0.5 on every bin (by construction >= 0.7: a tap of 2, perturbations that sum to
at most 1, eps = 0.3).  The singular eps = 1e-6 of ``integrate`` is out of scope (it routes through torch.fft; see
``_spectral.integrate``).
"""
import numpy as np
import pytest

import spectral_helpers as H

ORACLE_TOL = 1e-10


def _small(case):
    """The plane-loop fields are 65600 / 9400 samples of the same few cells: the oracles are compared on the first and the
    last 64 (every sample is an independent transform)."""
    x = case.x()
    return np.concatenate([x[:64], x[-64:]]) if x.shape[0] > 128 else x


@pytest.mark.parametrize("case", H.ALL_CASES, ids=repr)
def test_fft_reference_agrees_with_the_direct_circular_sum(case):
    x, seen = _small(case), 0
    for op in case.ops:
        if H.is_inverting(op):
            continue
        name, kw = H.op_args(op)
        k = case.kernel(op)
        if not H.direct_defined(x, k, name):
            continue
        ref, ds = H.reference(x, k, name, **kw), H.direct(x, k, name, **kw)
        assert ref.shape == ds.shape
        scale = np.max(np.abs(ref))
        assert scale > 0 and np.max(np.abs(ref - ds)) <= ORACLE_TOL * scale, (case, op)
        seen += 1
    if all(H.padded_size(case.shape, case.kshape, H.op_args(op)[0])[0][-1] % 2 for op in case.ops):
        assert seen == 0          # odd padded last axis everywhere: the inverse comes back one shorter, no circular sum
    else:
        assert seen > 0 or all(H.is_inverting(op) for op in case.ops)


@pytest.mark.parametrize("case", [c for c in H.ALL_CASES if any(H.is_inverting(op) for op in c.ops)], ids=repr)
def test_inverting_inputs_are_well_conditioned(case):
    k = H.inv_kernel(case.kshape)
    centre = tuple(s // 2 for s in case.kshape)
    rest = np.abs(k.astype(np.float64)).sum() - abs(float(k[centre]))
    assert k[centre] == 2.0 and rest <= 1.0
    for op in case.ops:
        if not H.is_inverting(op):
            continue
        name, kw = H.op_args(op)
        n, _ = H.padded_size(case.shape, case.kshape, name)
        conj = True if name == "xcorr" else kw["correlation"]
        d = np.min(np.abs(H.denominator(k, n, conj, H.EPS)))
        assert d >= H.MIN_DENOMINATOR, (case, op, d)
        assert d >= 2.0 - rest - H.EPS - 1e-12          # the triangle inequality the construction rests on


def test_reference_shapes_follow_the_recipe():
    """Odd padded last axis: ``irfftn`` without a size comes back one shorter; the crop keeps at most what is there."""
    x = H.field((2, 5, 6, 9), 1)
    k = H.mul_kernel((3, 3, 3))
    assert H.reference(x, k, "diff", slice_pad=False).shape == (2, 7, 8, 10)        # padded 7 x 8 x 11
    assert H.reference(x, k, "diff", slice_pad=True).shape == (2, 5, 6, 9)
    assert H.reference(x, k, "xcorr").shape == (2, 5, 6, 9)                          # evened to 12 first
    assert H.reference(H.field((2, 6, 7, 8), 2), H.mul_kernel((2, 2, 2)), "xcorr").shape == (2, 7, 8, 9)
    assert H.reference(H.field((2, 3, 6, 8), 3), H.mul_kernel((3, 3)), "diff").shape == (2, 3, 6, 8)
    # an identity kernel at the origin returns the padded field
    one = np.zeros((3, 3, 3), np.float32)
    one[0, 0, 0] = 1.0
    got = H.reference(H.field((2, 4, 5, 6), 4), one, "diff", slice_pad=False)
    assert np.allclose(got[:, 1:5, 1:6, 1:7], H.field((2, 4, 5, 6), 4), atol=1e-12)


def test_the_direct_sum_shifts_the_way_the_spectrum_says():
    """A single tap at p: plain multiplication moves the field by +p, the conjugate spectrum by -p."""
    x = H.field((1, 6, 8), 5)
    k = np.zeros((3, 3), np.float32)
    k[2, 1] = 1.0
    xp = np.pad(x.astype(np.float64), [(0, 0), (1, 1), (1, 1)])
    assert np.array_equal(H.direct(x, k, "diff", correlation=False, slice_pad=False), np.roll(xp, (2, 1), (1, 2)))
    assert np.array_equal(H.direct(x, k, "diff", correlation=True, slice_pad=False), np.roll(xp, (-2, -1), (1, 2)))
    assert np.allclose(H.reference(x, k, "diff", correlation=True, slice_pad=False), np.roll(xp, (-2, -1), (1, 2)), atol=1e-12)


def test_the_number_of_distinct_transform_sizes_stays_modest():
    """rocFFT may compile kernels for a size it has not seen: the GPU file reuses sizes (around forty in all)."""
    assert len(H.plan_sizes()) <= 45
    assert H.plan_sizes(H.CACHE) <= H.plan_sizes([c for c in H.ALL_CASES if c not in H.CACHE])
    assert len(H.plan_sizes(H.CACHE)) == 17
