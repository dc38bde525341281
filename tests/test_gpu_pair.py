"""Data-driven residual scores on the MI355X: ``residual*(vars, minus=...)`` = r(vars) - r(minus) (the scripts'
``cal_out_residual - cal_pred_residual``, Marginal/NS_Residuals_CP.py:284-289, Joint/Burgers_Residuals_CP.py:217-220) -
one paired pass (libcp_pre_pair.so) or the two-pass route - against reference-executed residuals
(tests/golden/residuals.npz) and against the oracle's r(a) - r(b) over the layouts and flags real callers use."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import conformal as oc
from oracle import residuals as orr

pytestmark = pytest.mark.gpu
RES_TOL = 1e-5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def _scaled_err(d, ra, rb):
    """max |d - (ra - rb)| against the scale of the residuals themselves, max(|ra|, |rb|) (not |d|: a near-cancelling
    pair has a tiny d whose relative error says nothing about the arithmetic)."""
    d = np.asarray(d, np.float64)
    ref = np.asarray(ra, np.float64) - np.asarray(rb, np.float64)
    scale = max(np.abs(ra).max(initial=0.0), np.abs(rb).max(initial=0.0)) or 1.0
    return float(np.abs(d - ref).max(initial=0.0) / scale)


def _golden_cases(g):
    from cp_pre_amd import residuals as R
    dt, dx, dy = g["coef"].tolist()
    bdx, bdt, bnu = g["burgers_coef"].tolist()
    ns, mhd = R.NavierStokes(dt, dx, dy), R.MHD()
    return {   # name -> (fn(vars, minus, boundary, absolute), which input)
        "PRE_Wave": (lambda a, m, b, ab: R.PRE_Wave(dt=0.01, dx=0.02, c=1.0).residual(a[:, :1], b, ab, minus=m[:, :1]), "vars6"),
        "PRE_NS": (lambda a, m, b, ab: R.PRE_NS(dt, dx, dy).residual(a[:, :3], b, minus=m[:, :3]), "vars6"),
        "PRE_MHD": (lambda a, m, b, ab: R.PRE_MHD(dt, dx, dy).residual(a, b, minus=m), "vars6"),
        "ns_continuity": (lambda a, m, b, ab: ns.residual_continuity(a[:, :2], b, ab, minus=m[:, :2]), "vars6"),
        "ns_momentum": (lambda a, m, b, ab: ns.residual_momentum(a[:, :3], b, ab, minus=m[:, :3]), "vars6"),
        "mhd_continuity": (lambda a, m, b, ab: mhd.residual_continuity(a, b, ab, minus=m), "vars6"),
        "mhd_momentum": (lambda a, m, b, ab: mhd.residual_momentum(a, b, ab, minus=m), "vars6"),
        "mhd_energy": (lambda a, m, b, ab: mhd.residual_energy(a, b, ab, minus=m), "vars6"),
        "mhd_induction": (lambda a, m, b, ab: mhd.residual_induction(a, b, ab, minus=m), "vars6"),
        "mhd_gauss": (lambda a, m, b, ab: mhd.residual_gauss(a, b, ab, minus=m), "vars6"),
        "burgers": (lambda a, m, b, ab: R.Burgers(bdx, bdt, bnu).residual(a, b, ab, minus=m), "u1d"),
        "advection": (lambda a, m, b, ab: R.Advection(1.0, 0.005, 0.01, disc=2).residual(a, b, ab, minus=m), "u1d"),
    }


def test_data_driven_scores_match_reference_golden(gpu, golden):
    """golden[:2] - golden[2:4] of the reference-executed residuals, for vars6[:2] paired with vars6[2:] and u1d[:2]
    with u1d[2:4], both boundary values, |.| on and off."""
    g = golden["residuals"]
    for name, (fn, key) in _golden_cases(g).items():
        x = torch.from_numpy(g[key]).to(gpu)
        a, m = x[:2], x[2:4]
        for b in (0, 1):
            ref = g[f"{name}|{b}"]
            ra, rb = ref[:2], ref[2:4]
            for ab in (False, True):
                if name in ("PRE_NS", "PRE_MHD") and ab:
                    continue                                   # (the PRE_* classes have no absolute=)
                got = fn(a, m, bool(b), ab)
                assert got.is_cuda and tuple(got.shape) == ra.shape, name
                want = np.abs(ra.astype(np.float64) - rb) if ab else ra.astype(np.float64) - rb
                assert np.abs(got.cpu().numpy() - want).max() <= RES_TOL * max(np.abs(ra).max(), np.abs(rb).max()), (name, b, ab)


# ---------------------------------------------------------------- oracle fuzz over layouts and flags
def _ns_oracle(v, bnd=True):
    return orr.ns_momentum(v, 0.01, 1 / 64, 1 / 64, nu=0.001, boundary=bnd)


def _layouts(x, gpu):
    """contiguous, the vars[:, i] views of a stacked tensor (already so), and the surrogate's Nt-fastest views"""
    yield "contiguous", x.to(gpu)
    nt_fast = x.permute(0, 1, 3, 4, 2).contiguous().to(gpu).permute(0, 1, 4, 2, 3)
    assert not nt_fast.is_contiguous()
    yield "nt_fastest", nt_fast


@pytest.mark.parametrize("shape", [(3, 3, 9, 12, 64), (2, 3, 6, 17, 36), (2, 3, 12, 10, 20), (2, 3, 7, 9, 200)])
def test_ns_momentum_pair_vs_oracle(gpu, shape):
    from cp_pre_amd.residuals import NavierStokes
    torch.manual_seed(sum(shape))
    ns = NavierStokes(0.01, 1 / 64, 1 / 64)
    a = torch.rand(shape) + 0.5
    for near in (False, True):
        b = a + 1e-3 * torch.randn(shape) if near else torch.rand(shape) + 0.5
        ra, rb = _ns_oracle(a).numpy(), _ns_oracle(b).numpy()
        for (la, da), (lb, db) in zip(_layouts(a, gpu), _layouts(b, gpu)):
            for ab in (False, True):
                d = ns.residual_momentum(da, boundary=True, absolute=ab, minus=db)
                ref = np.abs(ra.astype(np.float64) - rb) if ab else ra.astype(np.float64) - rb
                scale = max(np.abs(ra).max(), np.abs(rb).max())
                assert np.abs(d.cpu().numpy() - ref).max() <= RES_TOL * scale, (shape, la, near, ab)
            # mixed layouts: the two sets need not share strides (then both are staged to one layout)
            d = ns.residual_momentum(da, boundary=True, minus=_layouts(b, gpu).__next__()[1])
            assert _scaled_err(d.cpu().numpy(), ra, rb) <= RES_TOL


def test_every_paired_equation_vs_oracle(gpu):
    """All equations, the one-pass ones (NS continuity, MHD continuity / gauss, wave, advection, Burgers) and the
    two-pass ones (MHD momentum / energy / induction, JOREK), contiguous and Nt-fastest, with an odd width and a
    near-cancelling pair."""
    from cp_pre_amd import residuals as R
    torch.manual_seed(3)
    for shape in ((2, 6, 6, 10, 64), (2, 6, 5, 9, 37)):
        a = torch.rand(shape) + 0.5
        b = a + 1e-3 * torch.randn(shape)
        mhd = R.MHD()
        cases = {
            "ns_continuity": (lambda v, m: R.NavierStokes(0.01, 0.1, 0.1).residual_continuity(v[:, :2], True, minus=m[:, :2]),
                              lambda v: orr.ns_continuity(v, 0.1, 0.1, boundary=True)),
            "mhd_continuity": (lambda v, m: mhd.residual_continuity(v, True, minus=m), lambda v: orr.mhd_continuity(v, True)),
            "mhd_momentum": (lambda v, m: mhd.residual_momentum(v, True, minus=m), lambda v: orr.mhd_momentum(v, True)),
            "mhd_energy": (lambda v, m: mhd.residual_energy(v, True, minus=m), lambda v: orr.mhd_energy(v, boundary=True)),
            "mhd_induction": (lambda v, m: mhd.residual_induction(v, True, minus=m), lambda v: orr.mhd_induction(v, True)),
            "mhd_gauss": (lambda v, m: mhd.residual_gauss(v, True, minus=m), lambda v: orr.mhd_gauss(v, True)),
            "wave": (lambda v, m: R.PRE_Wave(0.01, 0.02).residual(v[:, :1], True, minus=m[:, :1]),
                     lambda v: orr.wave_residual(v[:, 0], 1.0, 0.01, 0.02, boundary=True)),
        }
        for name, (fn, ref) in cases.items():
            ra, rb = ref(a).numpy(), ref(b).numpy()
            for (_, da), (_, db) in zip(_layouts(a, gpu), _layouts(b, gpu)):
                assert _scaled_err(fn(da, db).cpu().numpy(), ra, rb) <= RES_TOL, (name, shape)
        # JOREK on the script's [BS, F, Nx, Ny, Nt] layout (two-pass)
        J = a[:, :3].permute(0, 1, 3, 4, 2).contiguous()
        Jb = b[:, :3].permute(0, 1, 3, 4, 2).contiguous()
        Rg = torch.linspace(1.0, 2.0, J.shape[3])
        jk = R.JOREK(Rg)
        for name, got, ref in (("jorek_continuity", jk.residual_continuity(J.to(gpu), True, minus=Jb.to(gpu)),
                                lambda v: orr.jorek_continuity(v, Rg, boundary=True)),
                               ("jorek_temperature", jk.residual_temperature(J.to(gpu), True, minus=Jb.to(gpu)),
                                lambda v: orr.jorek_temperature(v, Rg, boundary=True))):
            assert _scaled_err(got.cpu().numpy(), ref(J).numpy(), ref(Jb).numpy()) <= RES_TOL, name
    # 1-D: Burgers and advection on [BS, Nt, Nx] (odd and multiple-of-4 widths)
    for shape in ((3, 20, 64), (3, 17, 45)):
        u, w = torch.rand(shape), None
        w = u + 1e-3 * torch.randn(shape)
        for name, fn, ref in (("burgers", lambda x, m: R.Burgers(0.05, 0.01, 0.002).residual(x, True, minus=m),
                               lambda x: orr.burgers_residual(x, 0.05, 0.01, 0.002, boundary=True)),
                              ("advection", lambda x, m: R.Advection(1.0, 0.005, 0.01).residual(x, True, minus=m),
                               lambda x: orr.advection_residual(x, 1.0, 2, 0.005, 0.01, boundary=True))):
            assert _scaled_err(fn(u.to(gpu), w.to(gpu)).cpu().numpy(), ref(u).numpy(), ref(w).numpy()) <= RES_TOL, (name, shape)
            nt = u.transpose(1, 2).contiguous().to(gpu).transpose(1, 2)
            ntw = w.transpose(1, 2).contiguous().to(gpu).transpose(1, 2)
            assert _scaled_err(fn(nt, ntw).cpu().numpy(), ref(u).numpy(), ref(w).numpy()) <= RES_TOL, (name, shape, "nt")


def test_halo_x_skip_t_rim_and_row_padded_out(gpu):
    """x-slabs with their halo rows (PRE_FLAG_HALO_X) of both sets, interior-plane out (skip_t_rim), a row-padded out."""
    from cp_pre_amd import pipeline
    from cp_pre_amd.residuals import NavierStokes, MHD, PRE_Wave
    torch.manual_seed(5)
    B, T, X, Y = 3, 8, 12, 64
    fa, fb = torch.rand(B, 3, T, X, Y).to(gpu) + 0.5, torch.rand(B, 3, T, X, Y).to(gpu) + 0.5
    ns = NavierStokes(0.01, 1 / 64, 1 / 64)
    ra, rb = _ns_oracle(fa.cpu()).numpy(), _ns_oracle(fb.cpu()).numpy()
    x0, x1 = 3, 9
    d = ns.residual_momentum(fa[:, :, :, x0:x1], True, minus=fb[:, :, :, x0:x1], halo_x=True)
    assert _scaled_err(d.cpu().numpy(), ra[:, :, x0:x1], rb[:, :, x0:x1]) <= RES_TOL
    out = torch.empty(B, T - 2, X, Y, device=gpu)
    got = ns.residual_momentum(fa, True, minus=fb, skip_t_rim=True, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert _scaled_err(got.cpu().numpy(), ra[:, 1:-1], rb[:, 1:-1]) <= RES_TOL
    rp = pipeline.row_padded(B, (T, X, Y), device=gpu)
    got = ns.residual_momentum(fa, True, absolute=True, minus=fb, out=rp)
    assert got.data_ptr() == rp.data_ptr()
    assert np.abs(got.cpu().numpy() - np.abs(ra.astype(np.float64) - rb)).max() <= RES_TOL * np.abs(ra).max()
    # two-pass with halo_x and out: MHD induction; one pass: continuity; the wave kernel
    ma, mb = torch.rand(B, 6, T, X, Y).to(gpu) + 0.5, torch.rand(B, 6, T, X, Y).to(gpu) + 0.5
    mhd = MHD()
    for eq, ref in (("induction", orr.mhd_induction), ("continuity", orr.mhd_continuity)):
        r_a, r_b = ref(ma.cpu(), True).numpy(), ref(mb.cpu(), True).numpy()
        d = getattr(mhd, "residual_" + eq)(ma[..., x0:x1, :], True, minus=mb[..., x0:x1, :], halo_x=True)
        assert _scaled_err(d.cpu().numpy(), r_a[:, :, x0:x1], r_b[:, :, x0:x1]) <= RES_TOL, eq
        o = torch.empty(B, T, X, Y, device=gpu)
        d = getattr(mhd, "residual_" + eq)(ma, True, minus=mb, out=o)
        assert d.data_ptr() == o.data_ptr() and _scaled_err(d.cpu().numpy(), r_a, r_b) <= RES_TOL, eq
    wv = PRE_Wave(0.01, 0.02)
    r_a = orr.wave_residual(ma[:, 0].cpu(), 1.0, 0.01, 0.02, boundary=True).numpy()
    r_b = orr.wave_residual(mb[:, 0].cpu(), 1.0, 0.01, 0.02, boundary=True).numpy()
    d = wv.residual(ma[:, :1, :, x0:x1], True, minus=mb[:, :1, :, x0:x1], halo_x=True)
    assert _scaled_err(d.cpu().numpy(), r_a[:, :, x0:x1], r_b[:, :, x0:x1]) <= RES_TOL


def test_alias_nonfinite_empty_and_repeat(gpu):
    from cp_pre_amd.residuals import NavierStokes, MHD, PRE_Wave, Burgers
    torch.manual_seed(9)
    v = torch.rand(2, 6, 6, 10, 64).to(gpu) + 0.5
    ns, mhd = NavierStokes(0.01, 0.1, 0.1), MHD()
    calls = [lambda a, m: ns.residual_momentum(a[:, :3], True, minus=m[:, :3]),
             lambda a, m: ns.residual_continuity(a[:, :2], True, minus=m[:, :2]),
             lambda a, m: mhd.residual_continuity(a, True, minus=m),
             lambda a, m: mhd.residual_induction(a, True, minus=m),
             lambda a, m: PRE_Wave(0.01, 0.02).residual(a[:, :1], True, minus=m[:, :1]),
             lambda a, m: Burgers(0.05, 0.01, 0.002).residual(a[:, 0, 0], True, minus=m[:, 0, 0])]
    for fn in calls:
        assert torch.count_nonzero(fn(v, v)) == 0                                   # minus aliasing vars: exactly 0
        first = fn(v, v.flip(0))
        assert torch.equal(first, fn(v, v.flip(0)))                                # repeat calls: bitwise equal
    # NaN / inf in either set: against the footprint reference (index arithmetic on the operators' dense kernels and the
    # positions of the bad cells: non-finite wherever a non-zero tap of either set's expression lies on a bad cell, finite
    # and equal to the float64 oracles' difference wherever no tap of the kernels' extent boxes reaches one) - and, as
    # before, in the cells the two-pass route puts them in
    import stencil_guards as sg
    from test_gpu_footprint import mhd_continuity_terms, ns_momentum_terms
    bad = v.clone()
    bad[0, 0, 3, 4, 10] = float("nan")
    bad[1, 1, 2, 5, 33] = float("inf")
    bad[1, 2, 5, 9, 63] = float("-inf")
    bad[0, 1, 0, 0, 0] = float("nan")
    where = ~np.isfinite(bad.cpu().numpy())
    none = np.zeros_like(where)
    vc = v.cpu()
    for fn, single, terms, clean in (
            (calls[0], lambda x: ns.residual_momentum(x[:, :3], True), lambda w: ns_momentum_terms(ns, w[:, :3]),
             orr.ns_momentum(vc[:, :3], 0.01, 0.1, 0.1, boundary=True).numpy()),
            (calls[2], lambda x: mhd.residual_continuity(x, True), lambda w: mhd_continuity_terms(mhd, w),
             orr.mhd_continuity(vc, boundary=True).numpy())):
        for a, m, wa, wm in ((bad, v, where, none), (v, bad, none, where), (bad, bad, where, where)):
            d, two = fn(a, m), single(a) - single(m)
            assert torch.equal(torch.isnan(d), torch.isnan(two)) and torch.equal(torch.isinf(d), torch.isinf(two))
            must, may = sg.footprint_union(terms(wa) + terms(wm))
            got = d.cpu().numpy()
            assert (~np.isfinite(got[must])).all() and np.isfinite(got[~may]).all()
            # off the footprint both sets are the clean field: r(a) - r(b) = 0 within what the paired pass resolves
            assert np.abs(got[~may]).max() <= RES_TOL * np.abs(clean).max()
    # empty batch
    e = torch.empty(0, 6, 6, 10, 64, device=gpu)
    assert ns.residual_momentum(e[:, :3], minus=e[:, :3]).shape == (0, 4, 8, 62)
    assert mhd.residual_energy(e, True, minus=e).shape == (0, 6, 10, 64)


def test_autograd_reaches_both_sets(gpu):
    from cp_pre_amd.residuals import NavierStokes, MHD
    from cp_pre_amd import residuals as R
    torch.manual_seed(11)
    base_a, base_b = torch.rand(2, 6, 5, 8, 16) + 0.5, torch.rand(2, 6, 5, 8, 16) + 0.5
    ns = NavierStokes(0.01, 0.1, 0.1)
    mhd = MHD()
    for name, fn, ref in (("ns", lambda a, b: ns.residual_momentum(a[:, :3], minus=b[:, :3], absolute=True),
                           lambda a, b: (orr.ns_momentum(a[:, :3], 0.01, 0.1, 0.1) - orr.ns_momentum(b[:, :3], 0.01, 0.1, 0.1)).abs()),
                          ("mhd_continuity", lambda a, b: mhd.residual_continuity(a, minus=b),
                           lambda a, b: orr.mhd_continuity(a) - orr.mhd_continuity(b)),
                          ("mhd_energy", lambda a, b: mhd.residual_energy(a, minus=b),
                           lambda a, b: orr.mhd_energy(a) - orr.mhd_energy(b))):
        a, b = base_a.to(gpu).requires_grad_(), base_b.to(gpu).requires_grad_()
        y = fn(a, b)
        w = torch.randn(y.shape)
        (y * w.to(gpu)).sum().backward()
        ac, bc = base_a.clone().requires_grad_(), base_b.clone().requires_grad_()
        (ref(ac, bc) * w).sum().backward()
        assert rel_err(a.grad.cpu().numpy(), ac.grad.numpy()) <= 1e-4, name
        assert rel_err(b.grad.cpu().numpy(), bc.grad.numpy()) <= 1e-4, name


def test_calibration_recipe_on_d(gpu):
    """d feeds the existing calibration unchanged: JointCalibration.add_slab(d) == the oracle's modulation_func(a, b) /
    ncf_metric_joint(a, b, mod) q-hats; calibrate(|d|) == numpy on the same d, bit for bit."""
    from cp_pre_amd import inductive_cp as icp
    from cp_pre_amd import pipeline
    from cp_pre_amd.residuals import NavierStokes
    torch.manual_seed(13)
    n = 64
    a, b = torch.rand(n, 3, 8, 16, 64) + 0.5, torch.rand(n, 3, 8, 16, 64) + 0.5
    ns = NavierStokes(0.01, 1 / 64, 1 / 64)
    d = ns.residual_momentum(a.to(gpu), boundary=True, minus=b.to(gpu))
    ra, rb = _ns_oracle(a, False).numpy(), _ns_oracle(b, False).numpy()
    mod_ref = oc.modulation_func(ra, rb)
    scores_ref = oc.ncf_metric_joint(ra, rb, mod_ref)
    alphas = [0.1, 0.5, 0.9]
    jc = pipeline.JointCalibration(n, gpu)
    jc.add_slab(d, crop=(1, 1, 1))
    q = jc.finish(alphas).cpu().numpy()
    q_ref = np.array([oc.calibrate(scores_ref, n, al) for al in alphas], np.float32)
    assert np.abs(q - q_ref).max() <= 1e-5 * np.abs(q_ref).max()
    mod = icp.modulation_func(d[..., 1:-1, 1:-1, 1:-1].contiguous(), None).cpu().numpy()
    assert rel_err(mod, mod_ref) <= 1e-5
    dabs = ns.residual_momentum(a.to(gpu), absolute=True, minus=b.to(gpu)).contiguous()
    qm = icp.calibrate(dabs, n, 0.1).cpu().numpy()
    assert np.array_equal(qm, oc.calibrate(dabs.cpu().numpy(), n, 0.1))


@pytest.mark.timeout(900)
def test_full_size_c3_xslab_pair(gpu):
    """The C3 x-slab geometry of the headline job, data-driven: two [4096, 3, 64, 64+2, 512] field slabs (the 64-row
    slab both sets and one residual slab fit beside: 212.8 + 34.4 GB) through the paired NS momentum with halo_x;
    samples {0, 2047, 4095} against the oracle's r(a) - r(b) on the same rows with their halo rows."""
    from cp_pre_amd.residuals import NavierStokes
    torch.cuda.empty_cache()
    B, T, sl, Y = 4096, 64, 64, 512
    g = torch.Generator(device=gpu).manual_seed(17)
    va = torch.rand(B, 3, T, sl + 2, Y, device=gpu, generator=g).add_(0.5)
    vb = torch.rand(B, 3, T, sl + 2, Y, device=gpu, generator=g).add_(0.5)
    out = torch.empty(B, T, sl, Y, device=gpu)
    ns = NavierStokes(0.01, 1 / 512, 1 / 512)
    d = ns.residual_momentum(va[:, :, :, 1:sl + 1], boundary=True, out=out, halo_x=True, minus=vb[:, :, :, 1:sl + 1])
    assert d.data_ptr() == out.data_ptr()
    for s in (0, 2047, B - 1):
        sa, sb = va[s:s + 1].cpu(), vb[s:s + 1].cpu()
        r_a = orr.ns_momentum(sa, 0.01, 1 / 512, 1 / 512, nu=0.001, boundary=True)[:, :, 1:sl + 1].numpy()
        r_b = orr.ns_momentum(sb, 0.01, 1 / 512, 1 / 512, nu=0.001, boundary=True)[:, :, 1:sl + 1].numpy()
        assert _scaled_err(d[s:s + 1].cpu().numpy(), r_a, r_b) <= RES_TOL, s
    del va, vb, out, d
    torch.cuda.empty_cache()


def test_general_star_operators_take_the_two_pass_route(gpu):
    """Operators off the reference's tap structure and its Ny-fixed form (the general 7-point star): the paired NS
    momentum / MHD continuity kernels are not built for it (they would spill), so ``minus=`` runs the two single-set fused
    passes and an in-place subtract - bit for bit their difference, with ``halo_x`` and an interior-plane ``out`` too."""
    from cp_pre_amd.residuals import NavierStokes, MHD
    torch.manual_seed(19)
    B, T, X, Y = 2, 8, 12, 64
    ns, mhd = NavierStokes(0.01, 0.1, 0.1), MHD()
    for op in (ns, mhd):
        k = op.D_y.kernel.clone()
        k[1, 1, 0], k[1, 1, 2] = -0.25, 0.25                      # taps on Nt (the reference's D_y) AND on Ny
        op.D_y.kernel = k
    a, b = torch.rand(B, 6, T, X, Y).to(gpu) + 0.5, torch.rand(B, 6, T, X, Y).to(gpu) + 0.5
    d = ns.residual_momentum(a[:, :3], True, minus=b[:, :3])
    assert torch.equal(d, ns.residual_momentum(a[:, :3], True) - ns.residual_momentum(b[:, :3], True))
    x0, x1 = 3, 9
    d = ns.residual_momentum(a[:, :3, :, x0:x1], True, absolute=True, minus=b[:, :3, :, x0:x1], halo_x=True)
    ref = (ns.residual_momentum(a[:, :3, :, x0:x1], True, halo_x=True) - ns.residual_momentum(b[:, :3, :, x0:x1], True, halo_x=True)).abs()
    assert torch.equal(d, ref)
    out = torch.empty(B, T - 2, X, Y, device=gpu)
    d = ns.residual_momentum(a[:, :3], True, minus=b[:, :3], skip_t_rim=True, out=out)
    full = ns.residual_momentum(a[:, :3], True) - ns.residual_momentum(b[:, :3], True)
    assert d.data_ptr() == out.data_ptr() and torch.equal(d, full[:, 1:-1])
    assert torch.equal(ns.residual_momentum(a[:, :3], minus=b[:, :3], skip_t_rim=True, out=out), full[:, 1:-1, 1:-1, 1:-1])
    d = mhd.residual_continuity(a, True, minus=b)
    assert torch.equal(d, mhd.residual_continuity(a, True) - mhd.residual_continuity(b, True))


def test_halo_x_refuses_views_that_staging_would_copy(gpu):
    """PRE_FLAG_HALO_X reads the rows beyond an x-slab: it is only sound on the caller's own Ny-contiguous views.  An
    x-slab of the surrogate's Nt-fastest layout paired with a Ny-contiguous one shares no unit-stride axis, so staging
    would copy both - the kernel would read past fresh buffers.  Every route refuses it before any launch."""
    from cp_pre_amd import _dispatch, _lib
    from cp_pre_amd.residuals import MHD, NavierStokes, PRE_Wave
    B, T, X, Y, x0, x1 = 2, 8, 12, 64, 3, 9
    nt_fast = lambda F: torch.rand(B, F, X, Y, T, device=gpu).permute(0, 1, 4, 2, 3)[..., x0:x1, :]     # noqa: E731
    ny_fast = lambda F: torch.rand(B, F, T, X, Y, device=gpu)[..., x0:x1, :]                            # noqa: E731
    wv = PRE_Wave(0.01, 0.02)
    for a, b in ((nt_fast(1), ny_fast(1)), (ny_fast(1), nt_fast(1)), (nt_fast(1), nt_fast(1))):
        with pytest.raises(ValueError, match="halo_x"):
            wv.residual(a, True, minus=b, halo_x=True)
        with pytest.raises(ValueError, match="halo_x"):
            _dispatch.xcorr_pair(a[:, 0], b[:, 0], wv.D.kernel, 3, _lib.PRE_FLAG_HALO_X)
    ns, mhd = NavierStokes(0.01, 0.1, 0.1), MHD()
    for a, b in ((nt_fast(6), ny_fast(6)), (ny_fast(6), nt_fast(6))):
        with pytest.raises(ValueError, match="halo_x"):
            ns.residual_momentum(a[:, :3], True, minus=b[:, :3], halo_x=True)
        for eq in ("continuity", "induction", "energy"):
            with pytest.raises(ValueError, match="halo_x"):
                getattr(mhd, "residual_" + eq)(a, True, minus=b, halo_x=True)


def test_one_pass_kernels_serve_the_paired_equations(gpu, monkeypatch):
    """The paired equations are served by the pre_pair_* kernels themselves, on every layout the tests cover: with the
    single-set library, the two-pass route and the composed route all made to raise, each call still returns the
    difference of the single-set residuals computed beforehand."""
    from cp_pre_amd import _lib, pipeline
    from cp_pre_amd import residuals as R
    torch.manual_seed(23)
    ns, mhd, wv = R.NavierStokes(0.01, 1 / 64, 1 / 64), R.MHD(), R.PRE_Wave(0.01, 0.02)
    bu, ad = R.Burgers(0.05, 0.01, 0.002), R.Advection(1.0, 0.005, 0.01)
    nt = lambda t: t.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)                # noqa: E731
    cases = []
    for Y in (64, 256, 36):                                       # flat form, 8x64 tiles, a width of 4k + 0 below 64
        a, b = torch.rand(2, 6, 8, 12, Y, device=gpu) + 0.5, torch.rand(2, 6, 8, 12, Y, device=gpu) + 0.5
        for la, lb in ((a, b), (nt(a), nt(b))):
            cases += [
                ("ns_momentum", lambda x, m, **k: ns.residual_momentum(x[:, :3], True, minus=m[:, :3], **k),
                 lambda x, **k: ns.residual_momentum(x[:, :3], True, **k), la, lb, {}),
                ("ns_continuity", lambda x, m, **k: ns.residual_continuity(x[:, :2], True, minus=m[:, :2]),
                 lambda x, **k: ns.residual_continuity(x[:, :2], True), la, lb, {}),
                ("mhd_continuity", lambda x, m, **k: mhd.residual_continuity(x, True, minus=m, **k),
                 lambda x, **k: mhd.residual_continuity(x, True, **k), la, lb, {}),
                ("mhd_gauss", lambda x, m, **k: mhd.residual_gauss(x, True, minus=m),
                 lambda x, **k: mhd.residual_gauss(x, True), la, lb, {}),
                ("wave", lambda x, m, **k: wv.residual(x[:, :1], True, minus=m[:, :1], **k),
                 lambda x, **k: wv.residual(x[:, :1], True, **k), la, lb, {}),
            ]
        sl = (slice(None),) * 3 + (slice(3, 9),)                 # x-slabs with their halo rows
        for name in ("ns_momentum", "mhd_continuity", "wave"):
            c = next(c for c in cases if c[0] == name)
            cases.append((name + "_halo_x", c[1], c[2], a[sl], b[sl], {"halo_x": True}))
    w67 = torch.rand(2, 1, 8, 12, 67, device=gpu), torch.rand(2, 1, 8, 12, 67, device=gpu)    # odd width: march + tail
    cases.append(("wave_odd", lambda x, m, **k: wv.residual(x, True, minus=m), lambda x, **k: wv.residual(x, True),
                  w67[0], w67[1], {}))
    u, w = torch.rand(3, 20, 64, device=gpu), torch.rand(3, 20, 64, device=gpu)
    cases.append(("burgers", lambda x, m, **k: bu.residual(x, True, minus=m), lambda x, **k: bu.residual(x, True), u, w, {}))
    cases.append(("advection", lambda x, m, **k: ad.residual(x, True, minus=m), lambda x, **k: ad.residual(x, True), u, w, {}))
    refs = [(one(a, **kw).cpu().numpy(), one(b, **kw).cpu().numpy()) for _, _, one, a, b, kw in cases]
    rows = (2, 8, 12, 64)
    interior_ref = ns.residual_momentum(cases[0][3][:, :3], True) - ns.residual_momentum(cases[0][4][:, :3], True)

    def refuse(*a, **k):
        raise AssertionError("a paired equation left the one-pass kernels")
    monkeypatch.setattr(_lib, "load", refuse)                     # the single-set library (two-pass and composed routes)
    monkeypatch.setattr(R, "_two_pass", refuse)
    monkeypatch.setattr(R, "_pair_composed", refuse)
    for (name, pair, _, a, b, kw), (ra, rb) in zip(cases, refs):
        assert _scaled_err(pair(a, b, **kw).cpu().numpy(), ra, rb) <= RES_TOL, name
    out = torch.empty(2, 6, 12, 64, device=gpu)                   # interior-plane out (PRE_FLAG_OUT_INTERIOR_T)
    got = ns.residual_momentum(cases[0][3][:, :3], True, minus=cases[0][4][:, :3], skip_t_rim=True, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert _scaled_err(got.cpu().numpy(), interior_ref[:, 1:-1].cpu().numpy(), np.zeros(1, np.float32)) <= RES_TOL
    rp = pipeline.row_padded(*rows[:1], rows[1:], device=gpu)     # row-padded |d| out
    got = ns.residual_momentum(cases[0][3][:, :3], True, absolute=True, minus=cases[0][4][:, :3], out=rp)
    assert got.data_ptr() == rp.data_ptr()
    assert np.abs(got.cpu().numpy() - interior_ref.abs().cpu().numpy()).max() <= RES_TOL * interior_ref.abs().max().item()


def test_c_abi_pair_client_runs(gpu, tmp_path):
    """tests/c_abi/pair_check.c on the device: |r(a) - r(b)| of the wave star against plain C loops (odd width: the march
    and the tail kernel) and the argument errors of every pre_pair_* entry."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "pair_check"
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(root, "tests", "c_abi", "pair_check.c"), "-I" + os.path.join(root, "include"),
                           "-I/opt/rocm/include", "-L" + os.path.join(root, "cp_pre_amd"), "-l:libcp_pre_pair.so",
                           "-Wl,-rpath," + os.path.join(root, "cp_pre_amd"), "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "FAIL" not in run.stdout, run.stdout + run.stderr
    assert "no device" not in run.stdout and run.stdout.count("ok:") >= 10, run.stdout
