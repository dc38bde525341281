"""Per-sample statistics of the 2-D residuals on Ny-fastest fields (cp_pre_amd.screen.screen_stats, csrc/screen_stats.hip)
on the GPU, against float64 (pytest -m gpu).  Reference, tolerances and cases: tests/screenstats_helpers.py."""
import ctypes
import subprocess

import pytest
import torch

import screen_helpers as sh
import screenstats_helpers as st

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def run(c, gpu, x=None, method=None):
    from cp_pre_amd import screen
    return screen.screen_stats(method or sh.method_of(c.kind, gpu), c.x.to(gpu) if x is None else x, boundary=c.boundary)


# ------------------------------------------------------------------ 1. every kind, both boundary values, and the fallback
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("kind", sh.KINDS)
def test_stats_every_kind_against_fp64_and_the_fallback(gpu, kind, boundary):
    from cp_pre_amd import screen
    for name in st.NY_MAIN:
        c = st.ny_case(kind, sh.SEAM_SHAPES[name], boundary)
        got = run(c, gpu)
        assert screen.last_route() == st.route(kind, "ny")
        assert got.sum.device.type == "cuda" and got.max_abs.device.type == "cuda"
        st.check(got, c.ref, f"{kind} {name} boundary={boundary}")
        fb = screen.screen_stats(sh.method_of(kind), c.x, boundary=boundary)       # (CPU inputs: staged, stored, reduced)
        assert screen.last_route() == "fallback:input on the CPU" and not fb.sum.is_cuda
        st.check(fb, c.ref, "  fallback")


# ------------------------------------------------------------------ 2. the seams, B = 1 and B = 5
@pytest.mark.parametrize("name", list(sh.SEAM_SHAPES))
@pytest.mark.parametrize("kind", st.NY_SEAM_KINDS)
def test_stats_at_the_seams(gpu, kind, name):
    from cp_pre_amd import screen
    for boundary in (False, True):
        c = st.ny_case(kind, sh.SEAM_SHAPES[name], boundary)
        got = run(c, gpu)
        assert screen.last_route() == st.route(kind, "ny")
        st.check(got, c.ref, f"{kind} {name} boundary={boundary}")


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("kind", st.NY_SEAM_KINDS)
def test_stats_one_and_five_samples(gpu, kind, B):
    from cp_pre_amd import screen
    c = st.ny_case(kind, (B,) + sh.SEAM_SHAPES["two_tseg"][1:])
    got = run(c, gpu)
    assert screen.last_route() == st.route(kind, "ny")
    st.check(got, c.ref, f"{kind} B={B}")


# ------------------------------------------------------------------ 3. against the parent's own kernel
@pytest.mark.parametrize("kind", ["ns_momentum", "wave"])
def test_stats_max_abs_has_the_bits_of_the_joint_screens_score(gpu, kind):
    """the same march and the same functor; with m == 1 the guarded divide keeps max |r| itself"""
    from cp_pre_amd import screen
    for name in st.NY_MAIN:
        c = st.ny_case(kind, sh.SEAM_SHAPES[name])
        xd = c.x.to(gpu)
        s = screen.screen(sh.method_of(kind, gpu), xd, torch.ones(1, device=gpu), None)
        assert screen.last_route() == "fused:" + sh.FUSED_KIND[kind]
        got = run(c, gpu, xd)
        assert torch.equal(got.max_abs.view(torch.int32), s.score.view(torch.int32)), (kind, name)


# ------------------------------------------------------------------ 4. bytes
@pytest.mark.parametrize("kind", ["ns_momentum", "mhd_energy"])
def test_stats_same_bytes_on_every_run_whatever_the_workspace_held(gpu, kind):
    from cp_pre_amd import screen
    c = st.ny_case(kind, sh.SEAM_SHAPES["three_tseg_last_one"])          # (cropped: the last march is one plane)
    xd = c.x.to(gpu)
    first = run(c, gpu, xd)
    assert screen._stats_ws, "the cached workspace exists after a fused call"
    for ws in screen._stats_ws.values():
        ws.fill_(float("nan"))
    second = run(c, gpu, xd)
    assert screen.last_route() == st.route(kind, "ny")
    assert st.same_bits(first, second)
    assert not bool(torch.isnan(second.sum).any())


# ------------------------------------------------------------------ 5. slabs
def test_stats_slabs_compose(gpu):
    from cp_pre_amd import screen
    kind, shape = "ns_momentum", st.SLAB_SHAPE
    c = st.ny_case(kind, shape)
    method, xd, X = sh.method_of(kind, gpu), c.x.to(gpu), shape[2]
    whole = run(c, gpu, xd)
    st.check(whole, c.ref, "whole grid")
    xs = ((1, 10), (10, 33), (33, X - 1))
    for order in (xs, xs[::-1]):
        s = screen.ScreenStats(shape[0], gpu)
        for x0, x1 in order:
            s.add_slab(method, xd[:, :, :, x0:x1], crop=(1, 0, 1), halo_x=True)
            assert screen.last_route() == "fused:stats_ns_momentum"
        got = s.finish()
        assert got.cells == whole.cells
        assert torch.equal(got.max_abs.view(torch.int32), whole.max_abs.view(torch.int32))
        assert st.sums_close(got, whole)
    ts = ((0, 8), (6, 12))
    for order in (ts, ts[::-1]):
        s = screen.ScreenStats(shape[0], gpu)
        for t0, t1 in order:
            s.add_slab(method, xd[:, :, t0:t1], crop=(1, 1, 1))
        got = s.finish()
        assert got.cells == whole.cells
        assert torch.equal(got.max_abs.view(torch.int32), whole.max_abs.view(torch.int32))
        assert st.sums_close(got, whole)
    # halo_x raises where Screen.add_slab raises: a ConvOperator reads no halo rows ... and never on a fused slab above
    lap = st.ny_case("lap", (3, 5, 9, 13))
    with pytest.raises(RuntimeError, match="halo_x"):
        screen.ScreenStats(3, gpu).add_slab(sh.method_of("lap", gpu), lap.x.to(gpu)[:, :, 1:8], crop=(1, 0, 1), halo_x=True)


# ------------------------------------------------------------------ 6. non-finite values
def test_stats_non_finite_contract(gpu):
    from cp_pre_amd import _lib, screen
    c = st.ny_case("ns_momentum", sh.SEAM_SHAPES["rows2_narrow"])
    base = run(c, gpu)
    B, T, X, Y = c.shape
    # a NaN / inf in a cropped rim cell: p at the corner reaches, through the star, only cells with a zero index
    for value in (float("nan"), float("inf")):
        x = c.x.clone()
        x[1, 2, 0, 0, 0] = value
        x[2, 0, -1, -1, -1] = value
        assert st.same_bits(run(c, gpu, x.to(gpu)), base), value
    # a NaN in one counted cell of sample 1: its four statistics are NaN, the other samples keep their bytes
    x = c.x.clone()
    x[1, 0, 2, 5, 7] = float("nan")
    got = run(c, gpu, x.to(gpu))
    for t, b in ((got.sum, base.sum), (got.sum_abs, base.sum_abs), (got.sum_sq, base.sum_sq), (got.max_abs, base.max_abs)):
        assert bool(torch.isnan(t[1])) and torch.equal(t[[0, 2]], b[[0, 2]])
    # halo rows under halo_x: non-finite values in the row before the first slab and in the row after the last one, at
    # positions no counted cell's star reaches (the first / last column, the first / last plane)
    cs = st.ny_case("ns_momentum", st.SLAB_SHAPE)
    method, Xs = sh.method_of("ns_momentum", gpu), st.SLAB_SHAPE[2]
    xp = cs.x.clone()
    xp[:, :, :, 0, 0], xp[:, :, 0, 0, :] = float("nan"), float("inf")
    xp[:, :, :, Xs - 1, -1], xp[:, :, -1, Xs - 1, :] = float("inf"), float("nan")
    outs = []
    for xd in (cs.x.to(gpu), xp.to(gpu)):
        s = screen.ScreenStats(3, gpu)
        for x0, x1 in ((1, 10), (10, 33), (33, Xs - 1)):
            s.add_slab(method, xd[:, :, :, x0:x1], crop=(1, 0, 1), halo_x=True)
            assert screen.last_route() == "fused:stats_ns_momentum"
        outs.append(s.finish())
    assert st.same_bits(outs[0], outs[1])
    # the t-rim under PRE_FLAG_INTERIOR_T (ct = 0): the corners of the first and the last plane reach no counted cell
    w = st.ny_case("wave", sh.SEAM_SHAPES["two_tseg"])
    spec = screen._Spec(sh.method_of("wave", gpu))
    res = []
    for plant in (False, True):
        x = w.x.clone()
        if plant:
            x[:, 0, 0, 0], x[:, -1, -1, -1] = float("nan"), float("inf")
        xd = x.to(gpu)
        why, kernels = spec.prepare(xd, None, screen._F32, None)
        assert why is None
        mx = torch.zeros(3, dtype=torch.int32, device=gpu)
        sums = torch.zeros(3, 3, dtype=torch.float64, device=gpu)
        need = _lib.load_screenstats().pre_screenstats_workspace_len(0, *w.shape)
        ws = torch.full((need,), float("nan"), dtype=torch.float64, device=gpu)
        d = _lib.PreScreenStats(0, 1, 1, ctypes.c_void_p(mx.data_ptr()), ctypes.c_void_p(sums.data_ptr()), 3,
                                ctypes.c_void_p(ws.data_ptr()), need)
        assert spec.launch(kernels, xd, d, _lib.PRE_FLAG_INTERIOR_T, "", stats=True) == _lib.PRE_OK
        torch.cuda.synchronize()
        res.append((mx.clone(), sums.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1].view(torch.int64), res[1][1].view(torch.int64))
    ref = run(w, gpu)                                            # (ct = 0 with the flag is ct = 1 without it)
    assert torch.equal(res[0][0], ref.max_abs.view(torch.int32)) and torch.equal(res[0][1][1].view(torch.int64), ref.sum_abs.view(torch.int64))


# ------------------------------------------------------------------ 7. pitched views
@pytest.mark.parametrize("kind", ["ns_momentum", "wave", "mhd_energy"])
def test_stats_pitched_views(gpu, kind):
    """``vars[:, i]`` of a stacked tensor with more channels, rows padded beyond their length, the padding poisoned"""
    from cp_pre_amd import screen
    c = st.ny_case(kind, sh.SEAM_SHAPES["rows2_narrow"])
    dense = run(c, gpu)
    x = c.x if c.x.dim() == 5 else c.x[:, None]
    B, F, T, X, Y = x.shape
    for pad, value in ((4, float("nan")), (8, float("inf"))):
        big = torch.full((B, F + 2, T, X, Y + pad), value, device=gpu)
        big[:, 1:-1, :, :, :Y] = x.to(gpu)
        view = big[:, 1:-1, :, :, :Y]
        view = view if c.x.dim() == 5 else view[:, 0]
        assert view.stride(-2) == Y + pad and view.stride(-1) == 1
        got = run(c, gpu, view)
        assert screen.last_route() == st.route(kind, "ny")
        assert st.same_bits(got, dense), (kind, pad)


# ------------------------------------------------------------------ 8. odd widths
@pytest.mark.parametrize("shape", sh.ODD_SHAPES)
@pytest.mark.parametrize("kind", ["ns_momentum", "wave"])
def test_stats_odd_widths_take_the_fallback(gpu, kind, shape):
    from cp_pre_amd import screen
    for boundary in (False, True):
        c = st.ny_case(kind, shape, boundary)
        got = run(c, gpu)
        assert screen.last_route() == "fallback:row width not a multiple of 4"
        st.check(got, c.ref, f"{kind} {shape} boundary={boundary}")


def test_stats_fallback_reasons(gpu):
    from cp_pre_amd import residuals as R
    from cp_pre_amd import screen
    c = st.ny_case("ns_momentum", sh.SEAM_SHAPES["two_tseg"])
    xd = c.x.to(gpu)
    off = R.NavierStokes(sh.NS_DT, sh.NS_DX, sh.NS_DY, nu=sh.NS_NU, device=gpu, fused=False).residual_momentum
    st.check(screen.screen_stats(off, xd), c.ref, "fused=False")
    assert screen.last_route() == "fallback:fused=False"
    strided = xd.repeat_interleave(2, -1)[..., ::2]              # (the same values, every other float of a wider row)
    assert strided.stride(-1) == 2 and torch.equal(strided, xd)
    st.check(screen.screen_stats(sh.method_of("ns_momentum", gpu), strided), c.ref, "no unit stride")
    assert screen.last_route() == "fallback:no unit stride on the last axis"
    m =st.ny_case("mhd_continuity", sh.SEAM_SHAPES["two_tseg"])
    got = screen.screen_stats(sh.method_of("mhd_continuity", gpu), m.x.to(gpu)[:, :3])
    assert screen.last_route() == "fallback:fewer than six MHD channels"
    st.check(got, m.ref, "three MHD channels")
    # the general star of the MHD momentum equation is not built: the library declines, the fallback answers
    meth = sh.method_with_taps("mhd_momentum", "general", gpu)
    mm = st.ny_case("mhd_momentum", sh.SEAM_SHAPES["two_tseg"])
    got = screen.screen_stats(meth, mm.x.to(gpu))
    assert screen.last_route() == "fallback:declined by the library"
    stored = meth(mm.x.to(gpu), boundary=True)
    assert torch.equal(got.max_abs, stored[:, 1:-1, 1:-1, 1:-1].abs().flatten(1).max(dim=1).values)


# ------------------------------------------------------------------ 9. live kernels
def test_stats_see_the_kernels_the_operators_hold_now(gpu):
    from cp_pre_amd import screen
    c = st.ny_case("lap", sh.SEAM_SHAPES["rows2_narrow"])
    op = sh.method_of("lap", gpu)
    xd = c.x.to(gpu)
    base = screen.screen_stats(op, xd)
    op.kernel = 2 * op.kernel
    got = screen.screen_stats(op, xd)
    assert screen.last_route() == "fused:stats_stencil3d"
    # (a factor of two is exact in fp32 and in fp64: the doubled operator's statistics to the bit)
    assert torch.equal(got.sum, 2 * base.sum) and torch.equal(got.sum_abs, 2 * base.sum_abs)
    assert torch.equal(got.sum_sq, 4 * base.sum_sq) and torch.equal(got.max_abs, 2 * base.max_abs)


# ------------------------------------------------------------------ 10. the C client, and which libraries a call loads
def test_screenstats_c_client_runs(gpu, tmp_path):
    from test_screenstats_cpu import c_client_command
    exe = tmp_path / "screenstats_check"
    subprocess.check_call(c_client_command(exe))
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-6000:])
    assert out.returncode == 0 and "FAIL" not in out.stdout, out.stdout + out.stderr
    assert "no device" not in out.stdout and out.stdout.count("ok:") >= 60, out.stdout


def test_stats_calls_load_their_own_library_only(gpu):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, torch\n"
            "sys.path.insert(0, 'tests')\n"
            "import screen_helpers as sh, screen1d_helpers as s1\n"
            "from cp_pre_amd import screen\n"
            "g = torch.device('cuda:0')\n"
            "libs = lambda: sorted({ln.split('/')[-1] for ln in open('/proc/self/maps').read().splitlines() if 'libcp_pre_screen' in ln})\n"
            "screen.screen_stats(sh.method_of('wave', g), torch.rand(2, 6, 8, 12, device=g))\n"
            "screen.screen_stats(s1.method_of('burgers', g), torch.rand(2, 12, 24, device=g))\n"
            "assert screen.last_route() == 'fused:rows_stats_burgers', screen.last_route()\n"
            "assert libs() == ['libcp_pre_screenstats.so'], libs()\n"
            "screen.screen(sh.method_of('wave', g), torch.rand(2, 6, 8, 12, device=g), torch.ones(1, device=g))\n"
            "assert libs() == ['libcp_pre_screen.so', 'libcp_pre_screenstats.so'], libs()\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
