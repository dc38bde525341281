"""GPU tests of the spectral family (csrc/spectral.hip -> libcp_pre_fft.so, cp_pre_amd/_spectral.py) on the MI355X
(pytest -m gpu) at its seams, against the float64 reference of tests/spectral_helpers.py.

``rel_err = max|got - ref| / max|ref|`` with ``ref`` the fp64 recipe.  Tolerances are the project's own (the ones
``test_spectral_native_route_equals_torch_fft_composition`` uses): 2e-5 for the multiplicative modes, 1e-4 for the
inverting modes at eps = 0.3.  Every accuracy check also measures the fp32 torch.fft composition of the same recipe
against the same reference; the worst values per group are printed when the module ends (and written, as JSON, to the
file ``CP_PRE_SPECTRAL_REPORT`` names).  tests/SPECTRAL_TESTS.md records what they showed."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import spectral_helpers as H
import stencil_guards as G
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL_MUL, TOL_INV = 2e-5, 1e-4
REFUSALS = (RuntimeError, ValueError, NotImplementedError)

_WORST = {}          # group -> {"native_mul", "torch_mul", "native_inv", "torch_inv"}: worst rel_err seen
_FINDINGS = []       # (group, case, op, native, torch): native error above four times the torch composition's
_REF = {}            # (case name, op) -> fp64 reference, computed once and never written to


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    from cp_pre_amd import _lib
    _lib.load_fft()
    yield torch.device("cuda:0")
    report = {"worst": _WORST, "native_above_4x_torch": _FINDINGS}
    print("\nspectral rel_err against fp64 (worst per group):")
    for group, w in sorted(_WORST.items()):
        print(f"  {group:10s} " + "  ".join(f"{k}={v:.3e}" for k, v in sorted(w.items())))
    for f in _FINDINGS:
        print("  native > 4 x torch composition:", f)
    if os.environ.get("CP_PRE_SPECTRAL_REPORT"):
        with open(os.environ["CP_PRE_SPECTRAL_REPORT"], "w") as fh:
            json.dump(report, fh, indent=1)


@pytest.fixture
def S():
    from cp_pre_amd import _spectral
    return _spectral


def tol_of(op):
    return TOL_INV if H.is_inverting(op) else TOL_MUL


def ref_of(case, op):
    key = (case.name, op)
    if key not in _REF:
        _REF[key] = case.ref(op)
        _REF[key].setflags(write=False)
    return _REF[key]


def kernel_of(case, op):
    return torch.from_numpy(case.kernel(op))


def native(S, x, k, op, keep_channel=False):
    if op[0] == "xcorr":
        return S.fft_xcorr(x, k, keep_channel=keep_channel)
    if op[0] == "xinv":
        return S._native_fft_xcorr_inverse(x, k, eps=H.EPS, keep_channel=keep_channel)
    if op[0] == "diff":
        return S.differentiate(x, k, op[1], op[2], keep_channel=keep_channel)
    return S._native_integrate(x, k, op[1], op[2], H.EPS, keep_channel=keep_channel)


def _torch_xinv(x, k, eps, keep_channel):
    """``fft_conv(..., inverse=True)`` with a chosen eps, from fp32 torch.fft ops (``_torch_fft_xcorr`` fixes 1e-6)."""
    F = torch.nn.functional
    nd = k.dim()
    xx = x.unsqueeze(1) if x.dim() == nd + 1 else x
    xx = F.pad(xx, [p for d in reversed(range(nd)) for p in (k.shape[d] // 2,) * 2])
    size = xx.shape
    if xx.size(-1) % 2:
        xx = F.pad(xx, [0, 1])
    dims = tuple(range(2, xx.ndim))
    kk = k.to(x.device)[None, None]
    kf = torch.fft.rfftn(F.pad(kk, [v for i in reversed(range(2, xx.ndim)) for v in (0, xx.size(i) - kk.size(i))]), dim=dims)
    out = torch.fft.irfftn(torch.fft.rfftn(xx, dim=dims) / (torch.conj(kf) + eps), dim=dims)
    out = out[(slice(None), slice(None)) + tuple(slice(0, size[i] - kk.size(i) + 1) for i in range(2, xx.ndim))].contiguous()
    return out if keep_channel else out.squeeze(1)


def composed(S, x, k, op, keep_channel=False):
    """The same recipe from fp32 torch.fft device ops: the yardstick the native route's error is set against."""
    if op[0] == "xcorr":
        return S._torch_fft_xcorr(x, k, False, keep_channel)
    if op[0] == "xinv":
        return _torch_xinv(x, k, H.EPS, keep_channel)
    if op[0] == "diff":
        return S._torch_differentiate(x, k, op[1], op[2], keep_channel)
    return S._torch_integrate(x, k, op[1], op[2], H.EPS, keep_channel)


def record(group, case, op, e_native, e_torch):
    kind = "inv" if H.is_inverting(op) else "mul"
    w = _WORST.setdefault(group, {})
    w["native_" + kind] = max(w.get("native_" + kind, 0.0), e_native)
    w["torch_" + kind] = max(w.get("torch_" + kind, 0.0), e_torch)
    if e_native > 4 * e_torch:
        _FINDINGS.append((group, case.name, list(op), e_native, e_torch))


def check_case(S, gpu, group, case, parts=None):
    """Every op of ``case`` through the native route against the fp64 reference (and the torch composition measured on the
    side).  ``parts``: slices of the batch that must each meet the tolerance on their own scale."""
    x = torch.from_numpy(case.x()).to(gpu)
    for op in case.ops:
        k, ref = kernel_of(case, op), ref_of(case, op)
        got = native(S, x, k, op, case.keep_channel)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == ref.shape, (case, op, tuple(got.shape), ref.shape)
        got = got.cpu().numpy()
        comp = composed(S, x, k, op, case.keep_channel).cpu().numpy()
        assert comp.shape == ref.shape, (case, op)
        e_native, e_torch = rel_err(got, ref), rel_err(comp, ref)
        print(f"{group} {case.name} {op}: native {e_native:.3e} torch {e_torch:.3e}")
        record(group, case, op, e_native, e_torch)
        assert e_native <= tol_of(op), (case, op, e_native, e_torch)
        for sl in parts or ():
            e = rel_err(got[sl], ref[sl])
            assert e <= tol_of(op), (case, op, sl, e)


# ------------------------------------------------------------------------------------------------ accuracy at the seams
@pytest.mark.parametrize("case", H.MODES, ids=repr)
def test_every_mode_matches_fp64(gpu, S, case):
    """fft_xcorr, differentiate (correlation and slice_pad on and off), the native integrate and the native inverse
    cross-correlation on a 3-D field (even and odd padded last axis), a 2-D field and a [B,C,X,Y] field."""
    check_case(S, gpu, "modes", case)


@pytest.mark.parametrize("case", H.SEAMS, ids=repr)
def test_last_axis_seams_match_fp64(gpu, S, case):
    """Padded last axes 2 .. 514: one bin pair, a full first x-block of the multiply, a second x-block of one and of two
    bins, odd lengths whose inverse comes back one shorter."""
    check_case(S, gpu, "last-axis", case)


@pytest.mark.parametrize("case", H.PLANES, ids=repr)
def test_more_planes_than_the_grid_is_deep(gpu, S, case):
    """batch * n0 > 65535 in the embed and in the crop: the plane loop runs a second trip; the last samples are held to
    the tolerance as closely as the first."""
    n, _ = H.padded_size(case.shape, case.kshape, "diff")
    assert case.shape[0] * (n[0] if len(n) == 3 else 1) > 65535
    check_case(S, gpu, "planes", case, parts=(slice(0, 128), slice(-128, None)))


@pytest.mark.parametrize("case", H.EXTENTS, ids=repr)
def test_kernel_extents_match_fp64(gpu, S, case):
    """Anisotropic, 7-wide and even-sized kernels (k//2 padding and the s - k + 1 crop stop being symmetric)."""
    check_case(S, gpu, "extents", case)


def _raises_or_matches(S, gpu, x, k, op):
    """A refusal, or numbers that match the reference: never unchecked numbers."""
    try:
        got = native(S, torch.from_numpy(x).to(gpu), torch.from_numpy(k), op)
    except REFUSALS:
        return "raised"
    name, kw = H.op_args(op)
    ref = H.reference(x, k, name, **kw)
    assert tuple(got.shape) == ref.shape and rel_err(got.cpu().numpy(), ref) <= tol_of(op), (k.shape, op)
    return "matched"


@pytest.mark.parametrize("kshape", [(8, 3, 3), (3, 3, 9), (9, 9)], ids=str)
def test_kernels_wider_than_seven_are_refused(gpu, S, kshape):
    x = H.field((2, 8, 4, 6) if len(kshape) == 3 else (2, 4, 6), 70)       # every s - k + 1 stays positive
    for op in (H.XCORR, ("diff", False, True)):
        assert _raises_or_matches(S, gpu, x, H.mul_kernel(kshape), op) == "raised"


def test_a_padded_last_axis_of_one(gpu, S):
    """differentiate with a (3,1,1) kernel pads nothing: a last axis of 1 stays 1 and has no real transform - refused;
    fft_conv evens it to 2, which is a transform like any other."""
    x, k = H.field((2, 3, 3, 1), 71), H.mul_kernel((3, 1, 1))
    assert _raises_or_matches(S, gpu, x, k, ("diff", False, False)) == "raised"
    assert _raises_or_matches(S, gpu, x, k, ("diff", True, True)) == "raised"
    assert _raises_or_matches(S, gpu, x, k, H.XCORR) == "matched"


# ------------------------------------------------------------------------------------------------ layouts
def _layouts(case, gpu):
    """(label, allocation, view) of ``case``'s field in NaN-surrounded allocations."""
    x = torch.from_numpy(case.x())
    nd1 = x.dim() - 1
    yield ("permuted",) + G.embed(x, order=(0,) + tuple(range(nd1, 0, -1)), device=gpu)
    yield ("cropped",) + G.embed(x, gaps={0: 101, 1: 24, nd1 - 1: 5}, device=gpu)
    yield ("offset1",) + G.embed(x, offset=1, device=gpu)
    yield ("no-unit-stride",) + G.embed(x, gaps={nd1: 1}, offset=1, device=gpu)


@pytest.mark.parametrize("case", [H.LAYOUT, H.LAYOUT_C], ids=repr)
def test_views_in_poisoned_allocations_equal_the_dense_copy(gpu, S, case):
    dense = torch.from_numpy(case.x()).to(gpu)
    for op in case.ops:
        k = kernel_of(case, op)
        want = G.bits(native(S, dense, k, op, case.keep_channel))
        assert rel_err(native(S, dense, k, op, case.keep_channel).cpu().numpy(), ref_of(case, op)) <= tol_of(op)
        for label, alloc, view in _layouts(case, gpu):
            assert torch.equal(view, dense), label
            got = G.three_ways(alloc, [view], lambda: native(S, view, k, op, case.keep_channel))
            assert torch.equal(G.bits(got), want), (case, op, label)


def test_a_batch_channel_pair_that_does_not_collapse(gpu, S):
    """x[:, ::2] of five channels: (B, C) cannot be merged into one stride; the skipped channels hold the poison."""
    case = H.LAYOUT_C
    x = torch.from_numpy(case.x())                                           # [2, 3, 6, 8]
    B, C, X, Y = x.shape
    g = 4 * X * Y
    alloc = torch.zeros(g + B * (2 * C - 1) * X * Y + g, device=gpu)
    big = alloc[g:g + B * (2 * C - 1) * X * Y].view(B, 2 * C - 1, X, Y)
    view = big[:, ::2]
    view.copy_(x.to(gpu))
    assert view.stride(0) != C * view.stride(1)
    dense = x.to(gpu)
    for op in case.ops:
        k = kernel_of(case, op)
        want = G.bits(native(S, dense, k, op, True))
        got = G.three_ways(alloc, [view], lambda: native(S, view, k, op, True))
        assert torch.equal(G.bits(got), want), op


# ------------------------------------------------------------------------------------------------ the C ABI
def _i64(v):
    return (ctypes.c_int64 * len(v))(*[int(a) for a in v])


def _apply(lib, plan, x, k, mode, eps, out, od, work, pad_lo=(1, 1, 1), kd=None, in_ptr=None, work_ptr=None):
    from cp_pre_amd import _lib
    karr = np.ascontiguousarray(k, np.float32)
    return lib.pre_spectral_apply_f32(plan.handle, _lib.ptr(x) if in_ptr is None else in_ptr, _i64(x.stride()), _i64(x.shape[1:]),
                                      _i64(pad_lo), karr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                      _i64(karr.shape if kd is None else kd), mode, eps, _lib.ptr(out), _i64(out.stride()), _i64(od),
                                      _lib.ptr(work) if work_ptr is None else work_ptr, _lib.stream())


@pytest.fixture
def abi(gpu, S):
    """(library, plan for 2 x (7, 8, 10), its work buffer, field [2,5,6,8] on the device, kernel)."""
    from cp_pre_amd import _lib
    lib = _lib.load_fft()
    plan = S._Plan(3, (7, 8, 10), 10, 2)
    work = torch.empty(plan.work_bytes, dtype=torch.uint8, device=gpu)
    return lib, plan, work, torch.from_numpy(H.LAYOUT.x()).to(gpu), H.mul_kernel((3, 3, 3))


@pytest.mark.parametrize("order,gaps,offset", [(None, None, 0), ((0, 2, 1, 3), {3: 1, 1: 7}, 1), ((3, 2, 1, 0), {0: 3}, 0)],
                         ids=["dense", "pitched-no-unit-stride", "reversed"])
def test_c_abi_writes_a_strided_out_and_nothing_else(gpu, S, abi, order, gaps, offset):
    from cp_pre_amd import _lib
    lib, plan, work, x, k = abi
    for mode, od, op in ((_lib.PRE_FFT_CONJ, (5, 6, 8), H.XCORR), (0, (7, 8, 10), ("diff", False, False))):
        alloc, view, mask = G.guarded_out((2,) + od, order, gaps, offset, device=gpu)
        assert _apply(lib, plan, x, k, mode, 0.0, view, od, work) == _lib.PRE_OK
        torch.cuda.synchronize()
        assert G.untouched(alloc, mask), (mode, "a byte outside the out view was written")
        assert torch.equal(G.bits(view), G.bits(native(S, x, torch.from_numpy(k), op))), mode
        assert rel_err(view.cpu().numpy(), H.reference(H.LAYOUT.x(), k, H.op_args(op)[0], **H.op_args(op)[1])) <= TOL_MUL


def test_c_abi_refusals_of_create(gpu):
    from cp_pre_amd import _lib
    lib = _lib.load_fft()
    for nd, n, inv, batch, what in ((1, (1, 1, 8), 8, 2, "nd = 1"), (3, (3, 3, 1), 1, 2, "n2 = 1"), (3, (4, 5, 7), 5, 2, "inv_last 5 of 7"),
                                    (3, (4, 5, 7), 8, 2, "inv_last 8 of 7"), (3, (4, 5, 8), 7, 2, "inv_last 7 of even 8"),
                                    (3, (4, 5, 8), 8, 0, "batch = 0"), (2, (2, 5, 8), 8, 2, "nd = 2 with n0 = 2")):
        handle = ctypes.c_void_p()
        assert lib.pre_fft_create(ctypes.byref(handle), nd, _i64(n), inv, batch) == _lib.PRE_E_SHAPE, what
        assert handle.value is None, what
    assert lib.pre_fft_create(None, 3, _i64((4, 5, 8)), 8, 2) == _lib.PRE_E_NULL
    assert lib.pre_fft_create(ctypes.byref(ctypes.c_void_p()), 3, None, 8, 2) == _lib.PRE_E_NULL


def test_c_abi_refusals_of_apply_leave_out_untouched(gpu, abi):
    from cp_pre_amd import _lib
    lib, plan, work, x, k = abi
    alloc, view, mask = G.guarded_out((2, 7, 8, 10), device=gpu)
    everything = torch.ones_like(mask)
    null = ctypes.c_void_p(0)
    k8 = np.zeros((8, 3, 3), np.float32)
    calls = {
        "kd = 8": (dict(k=k8, od=(5, 6, 8)), _lib.PRE_E_SHAPE),
        "kd = 0": (dict(kd=(0, 3, 3), od=(5, 6, 8)), _lib.PRE_E_SHAPE),
        "od[0] beyond n": (dict(od=(8, 8, 10)), _lib.PRE_E_SHAPE),
        "od[2] beyond inv_last": (dict(od=(7, 8, 11)), _lib.PRE_E_SHAPE),
        "od = 0": (dict(od=(0, 8, 10)), _lib.PRE_E_SHAPE),
        "dims + pad beyond n": (dict(od=(5, 6, 8), pad_lo=(3, 1, 1)), _lib.PRE_E_SHAPE),
        "unknown mode bit": (dict(od=(5, 6, 8), mode=4), _lib.PRE_E_UNSUPPORTED),
        "null in": (dict(od=(5, 6, 8), in_ptr=null), _lib.PRE_E_NULL),
        "null work": (dict(od=(5, 6, 8), work_ptr=null), _lib.PRE_E_NULL),
    }
    for what, (kw, code) in calls.items():
        kw = dict(kw)
        rc = _apply(lib, plan, x, kw.pop("k", k), kw.pop("mode", 0), 0.0, view, kw.pop("od"), work, **kw)
        torch.cuda.synchronize()
        assert rc == code, (what, rc)
        assert G.untouched(alloc, everything), what
    assert lib.pre_spectral_apply_f32(None, *([None] * 6), 0, 0.0, *([None] * 5)) == _lib.PRE_E_NULL
    assert lib.pre_fft_destroy(None) == _lib.PRE_E_NULL and lib.pre_fft_work_bytes(plan.handle, None) == _lib.PRE_E_NULL


# ------------------------------------------------------------------------------------------------ samples, chunks, plans
def _per_sample(case, op):
    n, _ = H.padded_size(case.shape, case.kshape, H.op_args(op)[0])
    n = (1,) * (3 - len(n)) + tuple(n)
    return 4 * n[0] * n[1] * n[2] + 8 * n[0] * n[1] * (n[2] // 2 + 1) + 256


def _count_calls(monkeypatch):
    from cp_pre_amd import _lib
    lib, calls = _lib.load_fft(), []
    real = lib.pre_spectral_apply_f32

    def counting(*args):
        calls.append(args)
        return real(*args)
    monkeypatch.setattr(lib, "pre_spectral_apply_f32", counting)
    return calls


@pytest.mark.parametrize("per_chunk,launches", [(3, 3), (1, 7)], ids=["3+3+1", "7x1"])
def test_chunked_staging_equals_the_single_chunk_call(gpu, S, monkeypatch, per_chunk, launches):
    case = H.BATCH7
    x = torch.from_numpy(case.x()).to(gpu)
    for op in case.ops:
        k = kernel_of(case, op)
        whole = native(S, x, k, op)
        assert rel_err(whole.cpu().numpy(), ref_of(case, op)) <= tol_of(op)
        with monkeypatch.context() as m:
            m.setattr(S, "_STAGE_BYTES", per_chunk * _per_sample(case, op) + 100)
            calls = _count_calls(m)
            chunked = native(S, x, k, op)
            assert len(calls) == launches
        assert torch.equal(G.bits(chunked), G.bits(whole)), op


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("per_chunk,sample", [(7, 2), (3, 4)], ids=["one-chunk", "second-chunk"])
def test_a_non_finite_sample_stays_in_its_sample(gpu, S, monkeypatch, bad, per_chunk, sample):
    case = H.BATCH7
    x = torch.from_numpy(case.x()).to(gpu)
    xb = x.clone()
    xb[sample, 2, 3, 4] = bad
    others = [b for b in range(7) if b != sample]
    for op in case.ops:
        k = kernel_of(case, op)
        monkeypatch.setattr(S, "_STAGE_BYTES", per_chunk * _per_sample(case, op) + 100)
        clean, got = native(S, x, k, op), native(S, xb, k, op)
        assert not torch.isfinite(got[sample]).all(), (op, "the bad value vanished")
        assert torch.isfinite(got[others]).all(), (op, "a non-finite value reached another sample")
        assert torch.equal(G.bits(got[others]), G.bits(clean[others])), op


def test_the_seventeenth_plan_evicts_the_first(gpu, S):
    S._plans.clear()
    op = H.CACHE[0].ops[0]

    def run(case):
        x, k = torch.from_numpy(case.x()).to(gpu), kernel_of(case, op)
        got = native(S, x, k, op)
        e = rel_err(got.cpu().numpy(), ref_of(case, op))
        record("plan-cache", case, op, e, rel_err(composed(S, x, k, op).cpu().numpy(), ref_of(case, op)))
        assert e <= TOL_MUL, (case, e)
        return G.bits(got)
    first = run(H.CACHE[0])
    first_key = next(iter(S._plans))
    for i, case in enumerate(H.CACHE[1:], 2):
        run(case)
        assert len(S._plans) == min(i, 16)
    assert first_key not in S._plans and len(S._plans) == 16
    assert torch.equal(run(H.CACHE[0]), first)
    assert first_key in S._plans and len(S._plans) == 16


def test_a_smaller_transform_after_a_larger_one(gpu, S):
    """The work buffer of a call: a size that needs more, then one that needs less (and back), stay correct."""
    big, small = next(c for c in H.SEAMS if c.name == "last514"), H.MODES[0]
    for case in (big, small, big):
        op = case.ops[0]
        got = native(S, torch.from_numpy(case.x()).to(gpu), kernel_of(case, op), op)
        assert rel_err(got.cpu().numpy(), ref_of(case, op)) <= tol_of(op), case


# ------------------------------------------------------------------------------------------------ streams, bytes, devices
def test_a_side_stream_gives_the_default_streams_bytes(gpu, S):
    case = H.LAYOUT
    x = torch.from_numpy(case.x()).to(gpu)
    side = torch.cuda.Stream(device=gpu)
    for op in case.ops:
        k = kernel_of(case, op)
        want = G.bits(native(S, x, k, op))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            got = native(S, x, k, op)
        side.synchronize()
        assert torch.equal(G.bits(got), want), op


@pytest.mark.parametrize("case", [H.MODES[1], H.SEAMS[4], H.SEAMS[-1], H.EXTENTS[2]], ids=repr)
def test_two_runs_give_the_same_bytes(gpu, S, case):
    x = torch.from_numpy(case.x()).to(gpu)
    for op in case.ops:
        k = kernel_of(case, op)
        assert torch.equal(G.bits(native(S, x, k, op, case.keep_channel)), G.bits(native(S, x, k, op, case.keep_channel))), op


def test_cpu_tensors_come_back_on_the_cpu(gpu, S):
    for case in (H.MODES[0], H.MODES[3]):
        x = torch.from_numpy(case.x())
        for op in case.ops:
            k = kernel_of(case, op)
            got = native(S, x, k, op, case.keep_channel)
            assert not got.is_cuda and got.dtype == torch.float32
            assert torch.equal(G.bits(got), G.bits(native(S, x.to(gpu), k, op, case.keep_channel)).cpu()), (case, op)


@pytest.mark.parametrize("case", [H.MODES[1], H.SEAMS[6], H.EXTENTS[2]], ids=repr)
def test_linearity(gpu, S, case):
    """op(a x + y) - a op(x) - op(y) within the mode's tolerance of |a| |op(x)| + |op(y)|."""
    a = 1.7
    x = torch.from_numpy(case.x()).to(gpu)
    y = torch.from_numpy(H.field(case.shape, 900 + case.seed)).to(gpu)
    for op in case.ops:
        k = kernel_of(case, op)
        fx, fy = native(S, x, k, op, case.keep_channel).double(), native(S, y, k, op, case.keep_channel).double()
        both = native(S, (a * x.double() + y.double()).float(), k, op, case.keep_channel).double()
        scale = (abs(a) * fx.abs() + fy.abs()).max().item()
        e = (both - a * fx - fy).abs().max().item() / scale
        print(f"linearity {case.name} {op}: {e:.3e}")
        assert e <= tol_of(op), (case, op, e)


# ------------------------------------------------------------------------------------------------ routing and gradients
def _recipe64(x, k, op, correlation=False, slice_pad=True, eps=H.EPS, invert=False):
    """The reference recipe in float64 torch ops on the CPU (for autograd); its forward is checked against numpy."""
    F = torch.nn.functional
    nd = k.dim()
    pads = [s // 2 for s in k.shape] if op == "xcorr" else [k.shape[-1] // 2] * nd
    xp = F.pad(x, [p for d in reversed(range(nd)) for p in (pads[d], pads[d])])
    size = xp.shape[-nd:]
    if op == "xcorr" and xp.size(-1) % 2:
        xp = F.pad(xp, [0, 1])
    dims = tuple(range(-nd, 0))
    kf = torch.fft.rfftn(F.pad(k, [v for d in reversed(range(nd)) for v in (0, xp.shape[d - nd] - k.shape[d])]), dim=dims)
    if op == "xcorr" or correlation:
        kf = torch.conj(kf)
    g = 1 / (kf + eps) if (invert or op == "integ") else kf
    out = torch.fft.irfftn(torch.fft.rfftn(xp, dim=dims) * g, dim=dims)
    if op == "xcorr" or slice_pad:
        out = out[(Ellipsis,) + tuple(slice(0, s - ks + 1) for s, ks in zip(size, k.shape))]
    return out


def test_singular_modes_and_gradient_requests_stay_off_the_native_entry(gpu, S, monkeypatch):
    calls = _count_calls(monkeypatch)
    case = H.MODES[1]
    x, k = torch.from_numpy(case.x()).to(gpu), torch.from_numpy(H.inv_kernel(case.kshape))
    S.fft_xcorr(x, k)
    assert len(calls) == 1                                   # the counter sees the native route
    del calls[:]
    got = S.integrate(x, k, eps=H.EPS)
    assert rel_err(got.cpu().numpy(), H.reference(case.x(), k.numpy(), "integ", slice_pad=False)) <= TOL_INV
    S.integrate(x, k, True, True)
    S.fft_xcorr(x, k, inverse=True)
    S.fft_xcorr(x.clone().requires_grad_(True), k)
    S.differentiate(x, k.clone().requires_grad_(True))
    assert len(calls) == 0
    with torch.no_grad():                                    # no gradient wanted after all: native
        S.differentiate(x.clone().requires_grad_(True), k)
    assert len(calls) == 1


@pytest.mark.parametrize("op", [H.XCORR, ("diff", False, True), ("diff", True, False), ("integ", False, False)], ids=str)
def test_gradients_match_fp64_autograd_of_the_recipe(gpu, S, monkeypatch, op):
    calls = _count_calls(monkeypatch)
    case = H.MODES[1]                                        # [2,5,6,9]: odd padded last axis in differentiate / integrate
    name, kw = H.op_args(op)
    k_np = case.kernel(op)
    x64 = torch.from_numpy(case.x()).double().requires_grad_(True)
    k64 = torch.from_numpy(k_np).double().requires_grad_(True)
    out64 = _recipe64(x64, k64, name, **kw)
    ref = ref_of(case, op)
    assert out64.shape == ref.shape and rel_err(out64.detach().numpy(), ref) <= 1e-12
    out64.square().sum().backward()
    x = torch.from_numpy(case.x()).to(gpu).requires_grad_(True)
    k = torch.from_numpy(k_np).to(gpu).requires_grad_(True)
    if op[0] == "xcorr":
        out = S.fft_xcorr(x, k)
    elif op[0] == "diff":
        out = S.differentiate(x, k, op[1], op[2])
    else:
        out = S.integrate(x, k, op[1], op[2], eps=H.EPS)
    assert len(calls) == 0 and rel_err(out.detach().cpu().numpy(), ref) <= tol_of(op)
    out.square().sum().backward()
    ex, ek = rel_err(x.grad.cpu().numpy(), x64.grad.numpy()), rel_err(k.grad.cpu().numpy(), k64.grad.numpy())
    print(f"gradient {op}: field {ex:.3e} kernel {ek:.3e}")
    assert ex <= 1e-4 and ek <= 1e-4, (op, ex, ek)
