"""CPU tests of the fused kernel gradient of the residual losses (``wgrad=True`` / ``kernel_vjp`` of cp_pre_amd.losses,
libcp_pre_wgrad.so):
  * the exported ABI against include/cp_pre_wgrad.h and the ctypes binding, the C99 client compiled against the header;
  * the host decisions of ``_Spec`` with and without ``wgrad``;
  * on CPU inputs the fallback and its gradients against plain autograd;
  * the float64 reference of tests/wgrad_helpers.py against ``F.conv3d`` / ``F.conv2d`` autograd; the rule it restates.
The device pass is covered by tests/test_gpu_wgrad.py."""
import inspect
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import wgrad_helpers as wh
from losses_helpers import D, Route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cp_pre_wgrad.h")
DECLARED = {"pre_wgrad_abi_version", "pre_wgrad_stencil3d_f32"}


def c_client_command(exe, link=True):
    cmd = ["gcc", "-std=c99", "-pedantic", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "c_abi", "wgrad_check.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if not link:
        return cmd + ["-c", "-o", str(exe)]
    return cmd + ["-L" + os.path.join(ROOT, "cp_pre_amd"), "-l:libcp_pre_wgrad.so", "-Wl,-rpath," + os.path.join(ROOT, "cp_pre_amd"),
                  "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)]


# ------------------------------------------------------------------ the ABI
def test_wgrad_library_exports_exactly_its_entry_points():
    from cp_pre_amd import _lib
    so = _lib.WGRAD_SO_PATH
    assert os.path.exists(so), "libcp_pre_wgrad.so is built by __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.match(r"^[0-9a-f]+ T pre_", ln)}
    header = open(HEADER).read()
    declared = set(re.findall(r"^int\s+(pre_\w+)\s*\(", header, flags=re.M))
    assert declared == DECLARED and exported == declared and set(_lib.WGRAD_SIGNATURES) == declared
    assert int(re.search(r"#define\s+PRE_WGRAD_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.PRE_WGRAD_ABI_VERSION == 1
    assert int(re.search(r"#define\s+PRE_WGRAD_WORKSPACE\s+(\d+)", header).group(1)) == _lib.PRE_WGRAD_WORKSPACE == wh.WORKSPACE
    assert _lib.load_wgrad().pre_wgrad_abi_version() == _lib.PRE_WGRAD_ABI_VERSION
    assert _lib.load_wgrad() is _lib._load("wgrad") and "wgrad" in _lib._LIBS_MORE and "wgrad" not in _lib._LIBS
    # the binding has one ctypes type per argument of the header's declaration
    strip = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    args = re.search(r"int pre_wgrad_stencil3d_f32 ?\(([^;]*)\);", strip).group(1)
    assert len(args.split(",")) == len(_lib.WGRAD_SIGNATURES["pre_wgrad_stencil3d_f32"]) == 16


def test_wgrad_wrong_abi_version_and_missing_library_raise(monkeypatch, tmp_path):
    from cp_pre_amd import _lib
    monkeypatch.setattr(_lib, "_wgrad", None)
    monkeypatch.setattr(_lib, "PRE_WGRAD_ABI_VERSION", _lib.PRE_WGRAD_ABI_VERSION + 1)
    with pytest.raises(ImportError, match="libcp_pre_wgrad.so has ABI version 1"):
        _lib._load("wgrad")
    monkeypatch.setattr(_lib, "WGRAD_SO_PATH", str(tmp_path / "libcp_pre_wgrad.so"))
    with pytest.raises(ImportError, match="is missing"):
        _lib.load_wgrad()


def test_wgrad_header_and_c_client_compile_as_c99(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c",
                           "-I" + os.path.join(ROOT, "include"), HEADER])
    obj = tmp_path / "wgrad_check.o"
    subprocess.check_call(c_client_command(obj, link=False))
    assert obj.exists()


def test_wgrad_translation_unit_restates_its_rule_and_has_no_atomics():
    src = open(os.path.join(ROOT, "cp_pre_amd", "csrc", "loss_wgrad.hip")).read()
    assert "atomic" not in src.split("namespace {", 1)[1]
    for name, val in (("WG_FLUSH_PLANES", wh.FLUSH_PLANES), ("WG_MIN_UNITS", wh.MIN_UNITS), ("WG_MIN_TSEG", wh.MIN_TSEG),
                      ("WG_NARROW_Y", wh.NARROW_Y)):
        assert re.search(r"constexpr int %s = %d;" % (name, val), src), name
    assert wh.WORKSPACE // 27 == wh.MAX_BLOCKS and wh.L == 32
    mk = open(os.path.join(ROOT, "cp_pre_amd", "csrc", "Makefile")).read()
    assert re.search(r"^wgrad_OBJS\s+:= loss_wgrad\.o", mk, flags=re.M) and re.search(r"^LIBS\s+:=.*\bwgrad\b", mk, flags=re.M)


def test_the_seam_shapes_cross_the_seams_they_are_named_for():
    g = {k: wh.geometry(*s) for k, s in wh.SEAM_SHAPES.items()}
    assert (g["base"]["rows"], g["base"]["cols"], g["base"]["units"], g["base"]["tSeg"]) == (32, 32, 2, 6)
    assert g["Y=32"]["cols"] == 32 and g["Y=33"]["cols"] == 64 and g["Y=64"]["tilesC"] == 1 and g["Y=65"]["tilesC"] == g["Y=68"]["tilesC"] == 2
    assert g["X=32"]["tilesR"] == 1 and g["X=33"]["tilesR"] == 2 and g["X=16,wide"]["tilesR"] == 1 and g["X=17,wide"]["tilesR"] == 2
    assert (g["T=8"]["tSeg"], g["T=8"]["nSeg"]) == (8, 1) and (g["T=9"]["tSeg"], g["T=9"]["nSeg"]) == (5, 2)
    assert g["batch"]["batch_extent"] + 1 == wh.SEAM_SHAPES["batch"][0] and g["batch"]["units"] == g["batch"]["grid"] + 1
    assert g["flush"]["tSeg"] == 12 > wh.FLUSH_PLANES and g["flush"]["nSeg"] == 1
    # the bound is below what tests/test_gpu_parity.py grants the atomics kernel
    assert wh.BOUND_FACTOR < 1e-4


# ------------------------------------------------------------------ host decisions
def dev(t, requires_grad=False):
    return type("Dev", (), {"is_cuda": True, "numel": t.numel, "stride": t.stride, "dim": t.dim, "shape": t.shape,
                            "requires_grad": requires_grad})()


def test_spec_host_logic_with_and_without_wgrad():
    from cp_pre_amd import losses
    from cp_pre_amd import residuals as R
    S = losses._Spec
    for fn in (losses.pi_loss, losses.pisl_loss):
        assert inspect.signature(fn).parameters["wgrad"].default is False
    x4, x3 = dev(torch.empty((2, 6, 10, 16), device="meta")), dev(torch.empty((4, 10, 16), device="meta"))
    for name, x in (("wave", x4), ("op3d", x4), ("advection", x3), ("op2d", x3)):
        route = Route(name)
        route.ops[0].kernel.requires_grad_(True)
        spec = S(route.method)
        assert spec.prepare(x) == ("operator kernel requires grad", ()) == spec.prepare(x, None, False), name
        why, ks = spec.prepare(x, None, True)
        assert why is None and len(ks) == 2, name
        assert spec.trains_kernel()
    nt = torch.empty_strided((2, 8, 10, 16), (1280, 1, 128, 8), device="meta")
    live = Route("wave")
    live.ops[0].kernel.requires_grad_(True)
    assert S(live.method).prepare_flat(nt) == ("operator kernel requires grad", ())
    assert S(live.method).prepare_flat(nt, None, True)[0] is None
    # several operators: declined as before, with wgrad too
    x5 = dev(torch.empty((2, 3, 8, 10, 16), device="meta"))
    ns = R.NavierStokes(0.01, 0.1, 0.1)
    ns.D_x.kernel.requires_grad_(True)
    for m in (ns.residual_momentum, ns.residual_continuity):
        assert S(m).prepare(x5, None, True) == ("operator kernel requires grad", ())
    bg = R.Burgers(0.05, 0.01, 0.002)
    bg.D_t.kernel.requires_grad_(True)
    assert S(bg.residual).prepare(x3, None, True) == ("operator kernel requires grad", ())
    # unchanged: off-star, spectral, fused=False, yy requires grad
    box = Route("op3d")
    box.ops[0].kernel = torch.rand(3, 3, 3).requires_grad_(True)
    assert S(box.method).prepare(x4, None, True)[0] == "operator kernel off the 7-point star"
    from cp_pre_amd.convops_2d import ConvOperator as C2
    sp = C2(("x", "y"), 2, conv="spectral") if "conv" in inspect.signature(C2.__init__).parameters else None
    if sp is not None:
        assert S(sp).prepare(x4, None, True) == ("spectral operator", ())
    assert S(R.NavierStokes(0.01, 0.1, 0.1, fused=False).residual_momentum).prepare(x5, None, True) == ("fused=False", ())
    assert S(live.method).prepare(x4, dev(torch.empty((2, 6, 10, 16), device="meta"), True), True) == ("yy requires grad", ())


# ------------------------------------------------------------------ CPU inputs: the fallback and its gradients
def cpu_call(route):
    """what ``_Spec.call`` evaluates, from torch ops on the CPU: D(x, kernel) (- D(minus, kernel)), cropped"""
    def call(self, x, boundary, minus=None):
        k = route.ops[0].kernel
        f = lambda v: D(v[:, 0] if v.dim() == route.nd + 2 else v, k)                       # noqa: E731
        r = f(x) if minus is None else f(x) - f(minus)
        return r if boundary else r[(Ellipsis,) + (slice(1, -1),) * route.nd]
    return call


@pytest.mark.parametrize("name,shape", [("wave", (2, 6, 10, 16)), ("op3d", (2, 6, 10, 16)), ("advection", (4, 10, 16)), ("op2d", (4, 10, 16))])
def test_cpu_inputs_take_the_fallback_and_match_plain_autograd(monkeypatch, name, shape):
    from cp_pre_amd import _lib, losses

    def boom():
        raise AssertionError("a CPU input loaded libcp_pre_wgrad.so")
    monkeypatch.setattr(_lib, "load_wgrad", boom)
    route = Route(name)
    monkeypatch.setattr(losses._Spec, "call", cpu_call(route))
    g, x, y = wh.inputs(shape)
    crop = (Ellipsis,) + (slice(1, -1),) * route.nd
    for yy in (None, y):
        k = route.ops[0].kernel.detach().clone().requires_grad_(True)
        route.ops[0].kernel = k
        xr = x.clone().requires_grad_(True)
        loss = losses.pi_loss(route.method, xr, wgrad=True) if yy is None else losses.pisl_loss(route.method, xr, yy, wgrad=True)
        assert losses.last_route() == "fallback:input on the CPU"
        loss.backward()
        k2, x2 = k.detach().clone().requires_grad_(True), x.clone().requires_grad_(True)
        r = D(x2, k2) if yy is None else D(x2, k2) - D(yy, k2)
        r[crop].pow(2).mean().backward()
        assert torch.equal(k.grad, k2.grad) and torch.equal(xr.grad, x2.grad)
        # kernel_vjp: the same gradient torch.autograd.grad gives, the kernel need not require grad
        route.ops[0].kernel = k.detach()
        gc = g[crop].contiguous()
        got = losses.kernel_vjp(route.method, x, gc, minus=yy)
        assert losses.last_route() == "fallback:input on the CPU" and not route.ops[0].kernel.requires_grad
        k3 = k.detach().clone().requires_grad_(True)
        want = torch.autograd.grad((D(x, k3) if yy is None else D(x, k3) - D(yy, k3))[crop], k3, gc)[0]
        assert torch.equal(got, want)
    with pytest.raises(TypeError, match="one linear operator"):
        losses.kernel_vjp(Route("ns_momentum").method, torch.rand(2, 3, 6, 10, 16), torch.rand(2, 4, 8, 14))


# ------------------------------------------------------------------ the float64 reference
@pytest.mark.parametrize("ext", [(3, 3, 3), (3, 1, 1), (1, 3, 3), (3, 3), (1, 3)])
@pytest.mark.parametrize("crop", [False, True])
def test_the_fp64_reference_is_conv_autograd(ext, crop):
    shape = (2, 5, 6, 7)[: len(ext) + 1]
    g, x, y = wh.inputs(shape, seed=3)
    conv = F.conv3d if len(ext) == 3 else F.conv2d
    k = torch.zeros(ext, dtype=torch.float64, requires_grad=True)
    r = conv((x.double() - y.double()).unsqueeze(1), k[None, None], padding=tuple(e // 2 for e in ext)).squeeze(1)
    m = wh.mask(shape, range(1, len(shape))) if crop else torch.ones(shape, dtype=torch.float64)
    want = torch.autograd.grad(r, k, 0.75 * m * g.double())[0]
    dk, S = wh.ref_dk(g, x, y, ext, crop, 0.75)
    assert torch.allclose(dk, want, rtol=1e-12, atol=1e-12) and bool((S >= dk.abs() * (1 - 1e-12)).all())
    # a non-finite g in the rim does not reach the reference either
    if crop:
        gn = g.clone()
        gn[:, 0], gn[..., -1] = float("nan"), float("inf")
        dkn, Sn = wh.ref_dk(gn, x, y, ext, True, 0.75)
        assert torch.equal(dkn, dk) and torch.equal(Sn, S)
