"""The per-cell screen (cp_pre_amd.screen.screen_cells, csrc/screen_cells.hip) on Nt-fastest views - ``pred.permute(0,1,4,2,3)``,
what the NS and MHD scripts pass - on the GPU, against float64 (pytest -m gpu).

Reference, level fields, tolerances and cases: tests/screencells_helpers.py; layout and seams: tests/screenflat_helpers.py.
tests/test_screencells_cpu.py asserts the reference's own caps for every case used here."""
import pytest
import torch

import screen_helpers as sh
import screencells_helpers as ch
import screenflat_helpers as fh
import stencil_guards as sg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


def run(c, gpu, x=None, q=None, mod=None, method=None):
    from cp_pre_amd import screen
    xd = fh.to_layout(c.x, gpu) if x is None else x
    qd = fh.to_layout(c.q, gpu) if q is None else q
    md = (fh.to_layout(c.mod, gpu) if c.mod is not None else None) if mod is None else mod
    return screen.screen_cells(method or sh.method_of(c.kind, gpu), xd, qd, md, boundary=c.boundary)


def same(a, b):
    return torch.equal(sg.bits(a.score), sg.bits(b.score)) and torch.equal(a.inside, b.inside)


def three_pass(c, gpu):
    """The package's own three-pass route on the same Nt-fastest views, with per-cell levels."""
    from cp_pre_amd import inductive_cp as icp
    from cp_pre_amd import pipeline, screen
    method = sh.method_of(c.kind, gpu)
    xd = fh.to_layout(c.x, gpu)
    res = method(xd) if c.kind == "lap" else method(xd, boundary=True)
    mod = c.mod.to(gpu) if c.mod is not None else torch.ones(c.shape[1:], device=gpu)
    score = icp.ncf_metric_joint(res, None, mod) if c.boundary else icp.ncf_metric_joint(res, None, mod, crop=1)
    q = c.q.to(gpu)[(slice(None),) + c.reg[1:]]
    counts = torch.empty(c.nk, c.shape[0], dtype=torch.int64, device=gpu)
    cov = pipeline.CoverageLevels(1, c.nk, gpu)
    for i in range(c.shape[0]):
        cov.acc.zero_()
        cov.add_slab(res[c.reg][i:i + 1], q, modulation=mod[c.reg[1:]] if c.mod is not None else None)
        counts[:, i] = cov.acc
    return screen.Screened(score, counts, c.cells)


@pytest.mark.parametrize("with_mod", [True, False], ids=["mod", "nomod"])
@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("kind", fh.KINDS)
def test_screencells_flat_every_kind_against_fp64_and_three_pass(gpu, kind, boundary, with_mod):
    from cp_pre_amd import screen
    for nk, name in ch.MAIN:
        c = ch.case(kind, sh.SEAM_SHAPES[name], boundary, with_mod, nk)
        s = run(c, gpu)
        assert screen.last_route() == ch.route(kind, flat=True)
        ch.check(c, s, f"flat fused boundary={boundary} mod={with_mod}")
        s3 = three_pass(c, gpu)
        ch.check(c, s3, "  three-pass")
        print(f"  fused and three-pass bit-identical: {same(s, s3)}")


@pytest.mark.parametrize("name", ch.FLAT_SEAMS)
@pytest.mark.parametrize("kind", fh.SEAM_KINDS)
def test_screencells_flat_at_the_seams(gpu, kind, name):
    from cp_pre_amd import screen
    c = ch.case(kind, fh.SEAM_SHAPES[name], False, True, 10)
    s = run(c, gpu)
    assert screen.last_route() == ch.route(kind, flat=True)
    ch.check(c, s, name)


@pytest.mark.parametrize("kind", ch.GROUP_KINDS)
def test_screencells_flat_across_the_sample_group(gpu, kind):
    from cp_pre_amd import screen
    G = screen.sample_group()
    for B in ch.group_batches(G):
        c = ch.case(kind, (B,) + ch.GROUP_TXY, True, True, 10)
        s = run(c, gpu)
        assert screen.last_route() == ch.route(kind, flat=True)
        ch.check(c, s, f"flat G={G} B={B}")


def test_screencells_flat_levels_are_per_level_and_per_cell(gpu):
    c = ch.case("ns_momentum", sh.SEAM_SHAPES["two_tseg"], False, True, 10)
    base = run(c, gpu)
    perm = torch.tensor([3, 0, 9, 1, 7, 2, 8, 4, 6, 5])
    got = run(c, gpu, q=fh.to_layout(c.q[perm], gpu))
    assert torch.equal(got.inside, base.inside[perm.to(gpu)]) and torch.equal(sg.bits(got.score), sg.bits(base.score))
    lo, hi = c.q.clone(), c.q.clone()
    lo[4, 9, 2, 6], hi[4, 9, 2, 6] = -1.0, float("inf")
    glo, ghi = run(c, gpu, q=fh.to_layout(lo, gpu)), run(c, gpu, q=fh.to_layout(hi, gpu))
    others = [k for k in range(10) if k != 4]
    assert torch.equal(glo.inside[others], base.inside[others]) and torch.equal(ghi.inside[others], base.inside[others])
    assert bool((ghi.inside[4] - glo.inside[4] == 1).all())
    assert bool(((glo.inside[4] - base.inside[4]).abs() <= 1).all()) and bool(((ghi.inside[4] - base.inside[4]).abs() <= 1).all())


def test_screencells_flat_rim_and_non_finite_contract(gpu):
    c = ch.case("ns_momentum", sh.SEAM_SHAPES["rows2_narrow"], False, True, 10)
    base = run(c, gpu)
    q, mod = c.q.clone(), c.mod.clone()
    for v, t in ((float("nan"), q), (float("inf"), mod)):
        t[..., 0, :, :], t[..., -1, :, :], t[..., :, 0, :], t[..., :, -1, :], t[..., :, :, 0], t[..., :, :, -1] = [v] * 6
    assert same(run(c, gpu, q=fh.to_layout(q, gpu), mod=fh.to_layout(mod, gpu)), base)
    # cropped levels (dense [nk, T-2, X-2, Y-2], as calibrate_multi returns them): padded in the fields' layout, same bits
    assert same(run(c, gpu, q=c.q_cropped().to(gpu)), base)
    # levels in the other layout (Ny-fastest): copied once, same bits
    from cp_pre_amd import screen
    assert same(run(c, gpu, q=c.q.to(gpu)), base) and screen.last_route() == ch.route(c.kind, flat=True)
    x = c.x.clone()
    x[1, 2, 0, 0, 0] = float("nan")
    assert same(run(c, gpu, x=fh.to_layout(x, gpu)), base)
    q = c.q.clone()
    q[:, 2, 5, 7] = float("inf")
    allin = run(c, gpu, q=fh.to_layout(q, gpu))
    rest = [0, 1, 2, 4, 5, 6, 7, 8, 9]
    for v in (float("nan"), -0.5):
        q[3, 2, 5, 7] = v
        got = run(c, gpu, q=fh.to_layout(q, gpu))
        assert bool((got.inside[3] == allin.inside[3] - 1).all()) and torch.equal(got.inside[rest], allin.inside[rest])
    x = c.x.clone()
    x[1, 0, 2, 5, 7] = float("nan")
    r = sh.method_of("ns_momentum", gpu)(x.to(gpu), boundary=True)
    nbad = int(torch.isnan(r[c.reg][1]).sum())
    got = run(c, gpu, x=fh.to_layout(x, gpu), q=fh.to_layout(torch.full_like(c.q, float("inf")), gpu))
    assert bool(torch.isnan(got.score[1])) and bool((got.inside[:, 1] == c.cells - nbad).all())
    assert bool((got.inside[:, [0, 2]] == c.cells).all())


@pytest.mark.parametrize("shape", list(fh.FALLBACK_SHAPES))
def test_screencells_flat_fallback_shapes_keep_their_reasons(gpu, shape):
    from cp_pre_amd import screen
    c = ch.case("ns_momentum", shape, False, True, 10)
    got = run(c, gpu)
    assert screen.last_route() == fh.FALLBACK_SHAPES[shape]
    ch.check(c, got, screen.last_route())


def test_screencells_flat_t_slab_is_not_dense(gpu):
    from cp_pre_amd import screen
    shape, sl = fh.SLAB
    c = ch.case("ns_momentum", shape, False, True, 10)
    xd, qd, md = fh.to_layout(c.x, gpu), fh.to_layout(c.q, gpu), fh.to_layout(c.mod, gpu)
    s = screen.ScreenCells(shape[0], 10, gpu)
    s.add_slab(sh.method_of("ns_momentum", gpu), xd[:, :, sl], qd[:, sl], md[sl])
    assert screen.last_route() == "fallback:rows not dense"


# ------------------------------------------------------------------ the tap structures beside the reference's
@pytest.mark.parametrize("structure", sh.TAP_STRUCTURES)
@pytest.mark.parametrize("kind", sh.TAP_KINDS)
def test_screencells_flat_other_tap_structures_against_the_stored_residual(gpu, kind, structure):
    """The y-fixed (<4>) and general-star (<2>) instantiations of every functor compiled per tap structure, which the
    default operators never reach, against the residual stored with the same operators on the same Nt-fastest views
    (``sh.check_against_stored`` has the bounds; the level fields are the default operators' case's) - and not the default
    operators' answer.  The general stars of the MHD momentum and energy are not built with per-cell sets: the library
    declines."""
    from cp_pre_amd import screen
    nk, name = ch.MAIN[0]
    c = ch.case(kind, sh.SEAM_SHAPES[name], False, True, nk)
    method = sh.method_with_taps(kind, structure, gpu)
    xd = fh.to_layout(c.x, gpu)
    s = run(c, gpu, x=xd, method=method)
    built = structure != "general" or kind not in ("mhd_momentum", "mhd_energy")
    assert screen.last_route() == (ch.route(kind, flat=True) if built else "fallback:declined by the library")
    assert not same(s, run(c, gpu, x=xd))
    sh.check_against_stored(c, s, method(xd, boundary=True), c.q, f"{kind} {structure} flat")
