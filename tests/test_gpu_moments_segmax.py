"""GPU tests (pytest -m gpu) of the moments + segment-maxima pass, pre_moments_segmax_f64, called through the C ABI on
views the pipeline never builds (strided rows, odd bases, uneven chunks), against torch: segment maxima bit for bit,
fp64 sums to 1e-12, and the pruned joint score after ``add_slab`` against the full score pass."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    from cp_pre_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _run(a, row_stride, n, T, X, Y, cx, cy):
    """pre_moments_segmax_f64 on the n x [T, X, Y] samples at a.data_ptr() + i * row_stride floats."""
    from cp_pre_amd import _lib
    mom = torch.zeros(2, T * X * Y, dtype=torch.float64, device=a.device)
    segmax = torch.full((n, (T + 15) // 16, (X * Y + 63) // 64), -1, dtype=torch.int32, device=a.device)
    _lib.check(_lib.load().pre_moments_segmax_f64(_lib.ptr(a), row_stride, n, T, X, Y, cx, cy, _lib.ptr(mom[0]),
                                                  _lib.ptr(mom[1]), _lib.ptr(segmax), _lib.stream()), "pre_moments_segmax_f64")
    torch.cuda.synchronize()
    return mom, segmax


def _ref_segmax(v, cx, cy):
    """v [n, T, X, Y] -> int32 bit patterns [n, TC, NS] of max |v| per segment (64 consecutive cells of the flattened plane
    x 16 planes), cropped cells 0, a segment holding a NaN -> the canonical NaN pattern."""
    n, T, X, Y = v.shape
    NS, TC = (X * Y + 63) // 64, (T + 15) // 16
    a = v.abs()
    if cy:
        a[..., :cy] = 0.0
        a[..., Y - cy:] = 0.0
    if cx:
        a[:, :, :cx] = 0.0
        a[:, :, X - cx:] = 0.0
    a = torch.nn.functional.pad(a.reshape(n, T, X * Y), (0, NS * 64 - X * Y))
    a = torch.nn.functional.pad(a.permute(0, 2, 1), (0, TC * 16 - T)).reshape(n, NS, 64, TC, 16)
    nanseg = torch.isnan(a).any(-1).any(2)
    m = torch.where(torch.isnan(a), torch.zeros((), device=v.device), a).amax(-1).amax(2)
    bits = torch.where(nanseg, torch.full((), NAN_BITS, dtype=torch.int32, device=v.device), m.view(torch.int32))
    return bits.permute(0, 2, 1).contiguous()


def _check(v, mom, segmax, cx, cy, what):
    n, T, X, Y = v.shape
    ref = _ref_segmax(v, cx, cy)
    bad = (segmax != ref).nonzero()
    assert bad.numel() == 0, (what, bad[:8].tolist(), segmax[tuple(bad[0])].item(), ref[tuple(bad[0])].item())
    d = v.reshape(n, T * X * Y).double()
    s, q = d.sum(0), (d * d).sum(0)
    assert torch.allclose(mom[0], s, rtol=1e-12, atol=0.0, equal_nan=True), what
    assert torch.allclose(mom[1], q, rtol=1e-12, atol=0.0, equal_nan=True), what


# (n, T, X, Y, cx, cy, extra floats per row, base offset in floats)
CASES = [
    (9, 62, 16, 64, 1, 1, 0, 0),          # the C3 chunking (16, 16, 16, 14 planes), n odd
    (3, 21, 13, 20, 0, 0, 0, 0),          # X*Y = 260: segments straddle rows, last block partial; n below the unroll depth
    (1, 5, 8, 36, 1, 1, 0, 0),            # five planes (one chunk, one plane in the last plane group); one sample
    (17, 40, 12, 100, 1, 0, 0, 0),        # X*Y = 1200: neither 64 nor 256 divides it; 17 = two groups of 8 + 1
    (7, 33, 10, 32, 0, 1, 64, 0),         # row_stride > T*X*Y (a multiple of 4 floats)
    (6, 18, 9, 28, 1, 1, 3, 0),           # row_stride not a multiple of 4 floats
    (5, 19, 11, 24, 1, 1, 0, 1),          # a base that is not 16-byte aligned
    (4, 23, 7, 9, 1, 1, 0, 0),            # X*Y = 63: not a multiple of 4
    (70, 9, 64, 64, 0, 0, 0, 0),          # more samples than one split
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n{}_T{}_X{}_Y{}_c{}{}_pad{}_off{}".format(*c))
def test_moments_segmax_vs_torch(gpu, case):
    n, T, X, Y, cx, cy, pad, off = case
    g = torch.Generator().manual_seed(n * 1000 + T * 10 + X + Y)
    row = T * X * Y + pad
    buf = (torch.randn(off + n * row, generator=g) * 3.0).to(gpu)
    v = buf[off:].view(n, row)[:, :T * X * Y].view(n, T, X, Y)
    mom, segmax = _run(buf[off:], row, n, T, X, Y, cx, cy)
    _check(v, mom, segmax, cx, cy, case)


def test_moments_segmax_nan_inf(gpu):
    n, T, X, Y = 11, 35, 12, 40
    g = torch.Generator().manual_seed(5)
    v = torch.randn(n, T, X, Y, generator=g)
    v[2, 3, 5, 7] = float("inf")
    v[4, 20, 6, 30] = float("-inf")
    v[5, 34, 11, 39] = float("-inf")                      # in the x rim: cropped
    v[6, 17, 4, 9] = float("nan")
    v[7, 33, 8, 20] = -float("nan")
    v[8, 0, 0, 0] = float("nan")                          # cropped
    v[9] = -0.0
    v = v.to(gpu)
    for cx, cy in ((0, 0), (1, 1)):
        mom, segmax = _run(v, T * X * Y, n, T, X, Y, cx, cy)
        _check(v, mom, segmax, cx, cy, (cx, cy))


@pytest.mark.parametrize("X", [128, 127])
def test_moments_segmax_c3_slab(gpu, X):
    """A reduced-batch C3 slab [256, 64, X, 512] with its t crop, through the pipeline's entry point."""
    from cp_pre_amd import pipeline
    ops = pipeline.HipOps
    n, T, Y, crop = 256, 64, 512, (1, 1, 1)
    g = torch.Generator(device=gpu).manual_seed(X)
    res = torch.randn(n, T, X, Y, device=gpu, generator=g)
    res[17, 30, 64, 100] = 50.0
    mom = ops.zeros_moments((T - 2) * X * Y, gpu)
    segmax = ops.add_moments_segmax(res, mom, crop)
    torch.cuda.synchronize()
    v = res[:, 1:T - 1]
    ref = _ref_segmax(v, 1, 1)
    assert torch.equal(segmax, ref)
    s = torch.zeros((T - 2) * X * Y, dtype=torch.float64, device=gpu)
    q = torch.zeros_like(s)
    for i in range(0, n, 32):                             # (fp64 copies of the slab in pieces)
        d = v[i:i + 32].reshape(-1, (T - 2) * X * Y).double()
        s += d.sum(0)
        q += (d * d).sum(0)
    assert torch.allclose(mom[0], s, rtol=1e-12, atol=0.0)
    assert torch.allclose(mom[1], q, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("shape", [(33, 62, 24, 64), (8, 20, 13, 20)])
def test_add_slab_pruned_scores_match_full_pass(gpu, monkeypatch, shape):
    """After add_slab on the pruned route, the scores are those of the full score pass for the same modulation, bit for
    bit, and the modulation is the plain route's up to the order of the fp64 additions."""
    from cp_pre_amd import pipeline
    ops = pipeline.HipOps
    monkeypatch.setattr(ops, "PRUNE_MIN_CELLS", 0)
    monkeypatch.setattr(ops, "PRUNE_MIN_SAMPLES", 0)
    n, T, X, Y = shape
    crop = (1, 1, 1)
    g = torch.Generator().manual_seed(sum(shape))
    pruned, plain = pipeline.JointCalibration(n, gpu), pipeline.JointCalibration(n, gpu, prune=False)
    s_full = torch.zeros(n, device=gpu)
    for slab in range(2):
        res = (torch.randn(n, T, X, Y, generator=g) * (0.5 + torch.rand(T, X, Y, generator=g))).to(gpu)
        res[n // 2, T // 2, X // 2, Y // 3] = 30.0
        assert ops.can_prune(res, crop)
        mod = pruned.add_slab(res, crop=crop)
        ops.max_scores(res, mod, crop, s_full)
        assert torch.equal(pruned.scores, s_full), slab
        mod_plain = plain.add_slab(res, crop=crop)
        assert torch.allclose(mod, mod_plain, rtol=1e-6, atol=0.0, equal_nan=True), slab
