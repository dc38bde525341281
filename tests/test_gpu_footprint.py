"""GPU non-finite footprint tests (pytest -m gpu): the two-sided contract of include/cp_pre_hip.h for ``pre_stencil*`` and
the fused residuals.  A single NaN, +inf or -inf cell (and the three together) is put into an otherwise random field - in
the interior, on every face, edge and corner, in the last quad / the tail columns and on the planes next to the cut of an
8-plane segment.  The expected sets come from index arithmetic on the host (stencil_guards.footprint: the dense kernel and
the bad cells, nothing else): every output cell with a NON-ZERO tap on a bad cell is non-finite (NaN for a lone NaN); every
output cell whose kernel extent box reaches no bad cell is finite and equals the float64 oracle of the clean field within
RES_TOL.  Between the two the value is unspecified and only counted.

Each bad position gets a batch sample of its own (the samples do not interact), so one launch covers all positions."""
import numpy as np
import pytest
import torch

import stencil_guards as sg
from test_gpu_guards import _k, gpu  # noqa: F401  (the tap-set families and the fixture of the guard tests)

pytestmark = pytest.mark.gpu

RES_TOL = 1e-5
VALUES = {"nan": (float("nan"),), "+inf": (float("inf"),), "-inf": (float("-inf"),), "all three": (float("nan"), float("inf"), float("-inf"))}


def _positions(grid):
    T, X, Y = grid if len(grid) == 3 else (1,) + tuple(grid)
    extra = [(t, x, y) for t in (7, 8) for x in (0, X // 2) for y in (0, Y - 1)]                    # both sides of a segment cut
    extra += [(T // 2, X // 2, y) for y in range(max(0, Y - 5), Y)]                                  # last quad, tail columns
    extra += [(T // 2, x, Y // 2) for x in (7, 8)]                                                   # a row-tile edge
    cells = sg.bad_positions((T, X, Y), extra)
    return cells if len(grid) == 3 else sorted({c[1:] for c in cells})


def _spoil(base, cells, values):
    """[P, *grid] copies of ``base`` with ``values`` at cell p (and, for several values, at the next cells of the list);
    the bad mask."""
    P = len(cells)
    x = base[None].repeat(P, *([1] * base.dim())).clone()
    bad = np.zeros(tuple(x.shape), bool)
    for p in range(P):
        for j, v in enumerate(values):
            c = cells[(p + 5 * j) % P]
            x[(p,) + c] = v
            bad[(p,) + c] = True
    return x, bad


CASES = [("star", (5, 16, 64), None, 0), ("star", (9, 11, 260), None, 0), ("star", (17, 9, 66), None, 0), ("lap", (3, 6, 5), None, 0),
         ("dt", (9, 4, 101), None, 0), ("lap4", (3, 20, 64), None, 0), ("lap6", (4, 3, 128), None, 0), ("wave4", (9, 19, 64), None, 0),
         ("dense3", (16, 9, 320), None, 0), ("corners", (1, 12, 128), None, 0), ("two_planes", (4, 7, 128), None, 0),
         ("dense5", (5, 37, 130), None, 0), ("dense7", (2, 16, 259), None, 0), ("dense3", (1, 1, 4), None, 0), ("dense5", (3, 4, 7), None, 0),
         ("star", (10, 9, 14), (0, 2, 3, 1), 0), ("dense3", (12, 9, 14), (0, 2, 3, 1), 0), ("lap4", (72, 9, 14), (0, 2, 3, 1), 0),
         ("star", (5, 64, 12), (0, 1, 3, 2), 0), ("star", (9, 10, 64), None, 1), ("dense3", (9, 10, 64), None, 1)]


@pytest.mark.parametrize("kname,grid,order,offset", CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}-{i}" for i, c in enumerate(CASES)])
def test_stencil3d_nonfinite_footprint(gpu, kname, grid, order, offset):
    from cp_pre_amd import _dispatch
    from oracle.cstencil import xcorr_c
    k = _k(kname)
    g = torch.Generator().manual_seed(sum(grid))
    base = torch.randn(*grid, generator=g)
    cells = _positions(grid)
    clean = xcorr_c(base[None].numpy(), k.numpy())[0]
    between = 0
    for name, values in VALUES.items():
        x, bad = _spoil(base, cells, values)
        _, view = sg.embed(x, order, None, offset, gpu)
        got = _dispatch._xcorr_impl(view, k, 3).cpu().numpy()
        must, may = sg.footprint(k.numpy(), bad)
        sg.check_sandwich(got, np.broadcast_to(clean, got.shape), must, may, RES_TOL, lone_nan=name == "nan")
        between += int((may & ~must & ~np.isfinite(got)).sum())
    print(f"{kname} {grid}: {between} non-finite cells between the bounds")            # unspecified: recorded only


@pytest.mark.parametrize("kname", ["star", "lap4", "dense3", "dense5"])
def test_stencil3d_nonfinite_footprint_pitched_sliced_and_cropped_views(gpu, kname):
    """The remaining layouts of the guard tests: pitched rows / planes, a view with no unit stride, an Nx-fastest pitched
    view, ``vars[:, i]`` of a [P,F,T,X,Y] tensor and a cropped ``[..., 1:-1]`` view (the bad cells lie inside the view; the
    neighbouring fields and the cropped cells are finite: what lies outside the view is the business of the guard tests)."""
    from cp_pre_amd import _dispatch
    from oracle.cstencil import xcorr_c
    k = _k(kname)
    g = torch.Generator().manual_seed(len(kname) + 1)
    grid = (9, 10, 64)
    base = torch.randn(*grid, generator=g)
    cells = _positions(grid)
    clean = xcorr_c(base[None].numpy(), k.numpy())[0]
    for name, values in VALUES.items():
        x, bad = _spoil(base, cells, values)
        must, may = sg.footprint(k.numpy(), bad)
        views = [sg.embed(x, None, {2: 8}, 0, gpu)[1], sg.embed(x, None, {1: 64 * 3 + 4, 0: 12}, 0, gpu)[1],
                 sg.embed(x, None, {2: 5}, 1, gpu)[1], sg.embed(x, None, {3: 1}, 0, gpu)[1],
                 sg.embed(x, (0, 1, 3, 2), {3: 4}, 0, gpu)[1]]
        five = torch.randn(x.shape[0], 3, *grid, generator=g)
        five[:, 1] = x
        views.append(sg.embed(five, device=gpu)[1][:, 1])                                      # vars[:, i]
        wide = torch.randn(x.shape[0], grid[0], grid[1], grid[2] + 2, generator=g)
        wide[..., 1:-1] = x
        views.append(sg.embed(wide, device=gpu)[1][..., 1:-1])                                 # cropped, base 4 bytes off
        for n, view in enumerate(views):
            got = _dispatch._xcorr_impl(view, k, 3).cpu().numpy()
            try:
                sg.check_sandwich(got, np.broadcast_to(clean, got.shape), must, may, RES_TOL, lone_nan=name == "nan")
            except AssertionError as e:
                raise AssertionError(f"view {n} ({name}): {e}") from None


@pytest.mark.parametrize("Y", [64, 128])
def test_stencil3d_nonfinite_footprint_crosses_the_halo_rows(gpu, Y):
    """PRE_FLAG_HALO_X: rows -1 and X belong to the input, so a bad cell THERE reaches rows 0 / X-1 - the one place where
    the footprint crosses the view's edge.  The footprint is computed on the slab with its two halo rows and cut to the
    slab; bad cells sit in both halo rows, in the first and last row of the slab and in its interior."""
    from cp_pre_amd import _dispatch, _lib
    from oracle.cstencil import xcorr_c
    k = _k("star")
    g = torch.Generator().manual_seed(Y)
    T, X = 9, 10                                                   # the slab with its halo rows: rows 0 and X-1 are the halo
    base = torch.randn(T, X, Y, generator=g)
    cells = sorted({(t, x, y) for t in (0, 4, 7, 8) for x in (0, 1, X // 2, X - 2, X - 1) for y in (0, 3, Y // 2, Y - 1)})
    clean = xcorr_c(base[None].numpy(), k.numpy())[0][:, 1:-1]
    for name, values in VALUES.items():
        x, bad = _spoil(base, cells, values)
        _, whole = sg.embed(x, device=gpu)
        got = _dispatch._xcorr_impl(whole[:, :, 1:-1], k, 3, flags=_lib.PRE_FLAG_HALO_X).cpu().numpy()
        must, may = sg.footprint(k.numpy(), bad)
        sg.check_sandwich(got, np.broadcast_to(clean, got.shape), must[:, :, 1:-1], may[:, :, 1:-1], RES_TOL, lone_nan=name == "nan")
        assert must[:, :, 1][bad[:, :, 0]].all()                   # (the geometry does cross the edge)


def test_stencil2d_nonfinite_footprint(gpu):
    from cp_pre_amd import _dispatch
    from oracle.cstencil import xcorr_c
    g = torch.Generator().manual_seed(3)
    for kname in ("d1_x", "d1_dense3", "d1_dense5"):
        k = _k(kname)
        for grid, order in (((9, 64), None), ((20, 130), None), ((10, 36), (0, 2, 1)), ((1, 5), None)):
            base = torch.randn(*grid, generator=g)
            cells = _positions(grid)
            clean = xcorr_c(base[None].numpy(), k.numpy())[0]
            for name, values in VALUES.items():
                x, bad = _spoil(base, cells, values)
                _, view = sg.embed(x, order, device=gpu)
                got = _dispatch._xcorr_impl(view, k, 2).cpu().numpy()
                must, may = sg.footprint(k.numpy(), bad)
                sg.check_sandwich(got, np.broadcast_to(clean, got.shape), must, may, RES_TOL, lone_nan=name == "nan")


_ID3 = np.ones((1, 1, 1), np.float32)


def ns_momentum_terms(ns, bad):
    """(kernel, bad mask) of every operator of the NS momentum residual; ``bad`` is [B,3,T,X,Y] (u, v, p).  u and v are
    also used pointwise (the advection products)."""
    k = {n: getattr(ns, n).kernel.numpy() for n in ("D_t", "D_x", "D_y", "D_xx_yy")}
    terms = []
    for f in (0, 1):
        terms += [(k[n], bad[:, f]) for n in k] + [(_ID3, bad[:, f])]
    return terms + [(k["D_x"], bad[:, 2]), (k["D_y"], bad[:, 2])]


def mhd_continuity_terms(mhd, bad):
    k = {n: getattr(mhd, n).kernel.numpy() for n in ("D_t", "D_x", "D_y")}
    return [(k[n], bad[:, 0]) for n in k] + [(_ID3, bad[:, 0]), (_ID3, bad[:, 1]), (k["D_x"], bad[:, 1]), (_ID3, bad[:, 2]),
                                              (k["D_y"], bad[:, 2])]


def _ops_terms(obj, spec, bad):
    """``spec``: {field index: operator attribute names, '1' for a pointwise use} -> the (kernel, bad mask) terms."""
    return [(_ID3 if n == "1" else getattr(obj, n).kernel.numpy(), bad[:, f]) for f, names in spec.items() for n in names]


# which operator reaches which field in each expression of oracle/residuals.py (rho, u, v, p, Bx, By)
MHD_SPECS = {
    "momentum": {0: ["1"], 1: ["D_t", "D_x", "D_y", "1"], 2: ["D_t", "D_x", "D_y", "1"], 3: ["D_x", "D_y"],
                 4: ["D_x", "D_y", "1"], 5: ["D_x", "D_y", "1"]},
    "energy": {0: ["D_t"], 1: ["1", "D_x", "D_y"], 2: ["1", "D_y", "D_x"], 3: ["1", "D_x", "D_y"], 4: ["1", "D_x"], 5: ["1", "D_y"]},
    "induction": {1: ["1", "D_x", "D_y"], 2: ["1", "D_x", "D_y"], 4: ["1", "D_t", "D_x", "D_y"], 5: ["1", "D_t", "D_x", "D_y"]},
    "gauss": {4: ["D_x"], 5: ["D_y"]},
}
NS_CONTINUITY_SPEC = {0: ["D_x"], 1: ["D_y"]}
JOREK_SPECS = {"continuity": {0: ["D_t", "D_R", "D_Z", "D_RR", "D_ZZ", "1"], 1: ["D_Z", "D_R"]},
               "temperature": {0: ["D_t", "1", "D_R", "D_Z"], 1: ["D_Z", "D_R"], 2: ["1", "D_t", "D_R", "D_Z", "D_RR", "D_ZZ"]}}


def _spoil_fields(base, cells, values, fields):
    """[P,F,T,X,Y]: sample p has ``values`` at cell p of field ``fields[p % len(fields)]``."""
    P = len(cells)
    x = base[None].repeat(P, 1, 1, 1, 1).clone()
    bad = np.zeros(tuple(x.shape), bool)
    for p in range(P):
        for j, v in enumerate(values):
            c = (fields[(p + j) % len(fields)],) + cells[(p + 5 * j) % P]
            x[(p,) + c] = v
            bad[(p,) + c] = True
    return x, bad


@pytest.mark.parametrize("grid,order", [((5, 10, 64), None), ((9, 9, 66), None), ((10, 9, 16), (0, 1, 3, 4, 2))])
def test_fused_residual_nonfinite_footprint(gpu, grid, order):
    """NS momentum, MHD continuity (the union over the operators of the expression; a product term spreads a NaN in one
    field as far as the operator applied to that field reaches), the wave's single additive kernel."""
    from cp_pre_amd import residuals as R
    from oracle import residuals as orr
    g = torch.Generator().manual_seed(sum(grid))
    T, X, Y = grid
    base = torch.rand(3, T, X, Y, generator=g) + 0.5
    cells = _positions(grid)
    ns, mhd, wv = R.NavierStokes(0.01, 0.1, 0.1), R.MHD(), R.PRE_Wave(0.01, 0.02)
    base6 = torch.rand(6, T, X, Y, generator=g) + 0.5
    clean_ns = orr.ns_momentum(base[None], 0.01, 0.1, 0.1, boundary=True).numpy()
    clean_mhd = orr.mhd_continuity(base6[None], boundary=True).numpy()
    clean_wv = orr.wave_residual(base[None, 0], 1.0, 0.01, 0.02, boundary=True).numpy()
    for name, values in VALUES.items():
        x, bad = _spoil_fields(base, cells, values, (0, 1, 2))
        _, view = sg.embed(x, order, device=gpu)
        got = ns.residual_momentum(view, boundary=True).cpu().numpy()
        must, may = sg.footprint_union(ns_momentum_terms(ns, bad))
        sg.check_sandwich(got, np.broadcast_to(clean_ns, got.shape), must, may, RES_TOL, lone_nan=name == "nan")
        x, bad = _spoil_fields(base6, cells, values, (0, 1, 2))
        _, view = sg.embed(x, order, device=gpu)
        got = mhd.residual_continuity(view, True).cpu().numpy()
        must, may = sg.footprint_union(mhd_continuity_terms(mhd, bad))
        sg.check_sandwich(got, np.broadcast_to(clean_mhd, got.shape), must, may, RES_TOL, lone_nan=name == "nan")
        x, bad = _spoil_fields(base[:1], cells, values, (0,))
        _, view = sg.embed(x[:, 0], None if order is None else (0, 2, 3, 1), device=gpu)
        got = wv.residual(view, boundary=True).cpu().numpy()
        must, may = sg.footprint(wv.D.kernel.numpy(), bad[:, 0])
        sg.check_sandwich(got, np.broadcast_to(clean_wv, got.shape), must, may, RES_TOL, lone_nan=name == "nan")


def test_burgers_nonfinite_footprint(gpu):
    from cp_pre_amd import residuals as R
    from oracle import residuals as orr
    g = torch.Generator().manual_seed(8)
    bu = R.Burgers(0.05, 0.01, 0.002)
    ks = [o.kernel.numpy() for o in (bu.D_t, bu.D_x, bu.D_xx)] + [np.ones((1, 1), np.float32)]
    for grid, order in (((9, 64), None), ((40, 130), None), ((10, 36), (0, 2, 1))):
        base = torch.rand(*grid, generator=g) + 0.5
        cells = _positions(grid)
        clean = orr.burgers_residual(base[None], 0.05, 0.01, 0.002, boundary=True).numpy()
        for name, values in VALUES.items():
            x, bad = _spoil(base, cells, values)
            _, view = sg.embed(x, order, device=gpu)
            got = bu.residual(view, boundary=True).cpu().numpy()
            must, may = sg.footprint_union([(k, bad) for k in ks])
            sg.check_sandwich(got, np.broadcast_to(clean, got.shape), must, may, RES_TOL, lone_nan=name == "nan")


@pytest.mark.parametrize("grid,order", [((5, 10, 64), None), ((9, 9, 66), None), ((10, 9, 16), (0, 1, 3, 4, 2))])
def test_remaining_fused_residuals_nonfinite_footprint(gpu, grid, order):
    """MHD momentum / energy / induction / gauss and NS continuity.  MHD momentum only ever divides by rho: an infinite rho
    gives 1/rho = 0 and a finite residual in the reference too, so rho takes part with NaN alone."""
    from cp_pre_amd import residuals as R
    from oracle import residuals as orr
    g = torch.Generator().manual_seed(sum(grid) + 1)
    T, X, Y = grid
    base6 = torch.rand(6, T, X, Y, generator=g) + 0.5
    cells = _positions(grid)
    ns, mhd = R.NavierStokes(0.01, 0.1, 0.1), R.MHD()
    for eq, spec in MHD_SPECS.items():
        clean = getattr(orr, "mhd_" + eq)(base6[None], boundary=True).numpy()
        for name, values in VALUES.items():
            fields = tuple(f for f in spec if not (eq == "momentum" and f == 0 and name != "nan"))
            x, bad = _spoil_fields(base6, cells, values, fields)
            _, view = sg.embed(x, order, device=gpu)
            got = getattr(mhd, "residual_" + eq)(view, True).cpu().numpy()
            must, may = sg.footprint_union(_ops_terms(mhd, spec, bad))
            try:
                sg.check_sandwich(got, np.broadcast_to(clean, got.shape), must, may, RES_TOL, lone_nan=name == "nan")
            except AssertionError as e:
                raise AssertionError(f"mhd {eq} ({name}): {e}") from None
    clean = orr.ns_continuity(base6[None, :2], 0.1, 0.1, boundary=True).numpy()
    for name, values in VALUES.items():
        x, bad = _spoil_fields(base6[:2], cells, values, (0, 1))
        _, view = sg.embed(x, order, device=gpu)
        got = ns.residual_continuity(view, boundary=True).cpu().numpy()
        must, may = sg.footprint_union(_ops_terms(ns, NS_CONTINUITY_SPEC, bad))
        sg.check_sandwich(got, np.broadcast_to(clean, got.shape), must, may, RES_TOL, lone_nan=name == "nan")


@pytest.mark.parametrize("N,Nt", [(16, 10), (40, 24)])
def test_jorek_nonfinite_footprint(gpu, N, Nt):
    """The two reduced-MHD equations on the script's [BS,F,Nx,Ny,Nt] layout (fields seen as [BS,Nt,Nx,Ny] views)."""
    from cp_pre_amd import residuals as R
    from oracle import residuals as orr
    g = torch.Generator().manual_seed(N)
    base = torch.rand(3, Nt, N, N, generator=g) + 0.5                       # (rho, phi, T) as [F,Nt,Nx,Ny]
    Rg = torch.linspace(1.0, 2.0, N)
    jo = R.JOREK(Rg, dx=0.1, dy=0.1, dt=0.02)
    cells = _positions((Nt, N, N))
    to_script = lambda v: v.permute(0, 1, 3, 4, 2)                          # noqa: E731  [P,F,Nt,Nx,Ny] -> [P,F,Nx,Ny,Nt]
    for eq, spec in JOREK_SPECS.items():
        ref = getattr(orr, "jorek_" + eq)
        clean = (ref(to_script(base[None]), Rg, 3.4, boundary=True) if eq == "continuity" else ref(to_script(base[None]), Rg, boundary=True)).numpy()
        for name, values in VALUES.items():
            x, bad = _spoil_fields(base, cells, values, tuple(spec))
            _, view = sg.embed(to_script(x).contiguous(), device=gpu)
            got = getattr(jo, "residual_" + eq)(view, True).cpu().numpy()
            must, may = sg.footprint_union(_ops_terms(jo, spec, bad))
            try:
                sg.check_sandwich(got, np.broadcast_to(clean, got.shape), must, may, RES_TOL, lone_nan=name == "nan")
            except AssertionError as e:
                raise AssertionError(f"jorek {eq} ({name}): {e}") from None


def _padded_bad(ref, x):
    """The bad mask of the boundary-padded field: the oracle's pad-then-valid-conv recipe pads with cells of the field
    (periodic wrap, mirrored, repeated) or with the side's value, so the padded copy of a spoiled field IS the geometry."""
    return ~np.isfinite(ref.pad(x).numpy())


def test_spatial_family_nonfinite_footprint(gpu):
    """The five vector operators with every boundary kind on every side and mixed: the footprint is computed on the
    boundary-padded field (a bad cell on an edge also sits in the pad cells the boundary kind copies it to) with the
    operator's 3x3 kernels as a same-size correlation, and cut to the valid region."""
    from cp_pre_amd import vector_convops_spatial as VS
    from oracle import spatial as osp
    g = torch.Generator().manual_seed(97)
    types = ["dirichlet", "neumann", "outflow", "periodic", "symmetric"]
    kinds = {"gradient": VS.Gradient, "laplace": VS.Laplace, "divergence": VS.Divergence, "curl": VS.Curl,
             "vector_gradient": VS.Vector_Gradient}
    sides_all = ("left", "right", "top", "bottom")
    cases = [{s: t for s in sides_all} for t in types] + [dict(zip(sides_all, types[i:] + types[:i])) for i in range(5)]
    for n, sides in enumerate(cases):
        for kind, cls in kinds.items():
            X, Y = [(9, 64), (4, 5), (17, 65), (6, 260)][(n + len(kind)) % 4]
            cells = sorted({c[1:] for c in _positions((1, X, Y))})
            base = torch.randn(2, 1, X, Y, generator=g)                     # the two input fields (a, b)
            vals = {s: 0.25 * (i + 1) for i, s in enumerate(sides_all)}
            ref = osp.VectorOp(kind, scale=1.5, boundary_cond="periodic")
            ref.types, ref.values = dict(sides), dict(vals)
            op = cls(scale=1.5, boundary_cond="periodic", device=gpu)
            for s in sides:
                op.bc.set_boundary_type(s, sides[s], vals[s])
            clean = (ref(base[0:1], base[1:2]) if kind != "laplace" else ref(base[0:1])).numpy()
            for name, values in VALUES.items():
                P = len(cells)
                ab = base[None].repeat(P, 1, 1, 1, 1).clone()               # [P, 2, 1, X, Y]
                for p in range(P):
                    for j, v in enumerate(values):
                        ab[(p, (p + j) % 2, 0) + cells[(p + 5 * j) % P]] = v
                a, b = ab[:, 0], ab[:, 1]
                with torch.no_grad():
                    got = (op(a.to(gpu), b.to(gpu)) if kind != "laplace" else op(a.to(gpu))).cpu().numpy()
                ba, bb = _padded_bad(ref, a)[:, 0], _padded_bad(ref, b)[:, 0]
                if kind == "laplace":
                    terms = [[(ref.lap.numpy(), ba)]]
                elif kind == "gradient":
                    terms = [[(ref.gx.numpy(), ba)], [(ref.gy.numpy(), bb)]]              # one channel each
                elif kind == "divergence":
                    terms = [[(ref.gx.numpy(), ba), (ref.gy.numpy(), bb)]]
                elif kind == "curl":
                    terms = [[(ref.gx.numpy(), bb), (ref.gy.numpy(), ba)]]
                else:
                    terms = [[(ref.gx.numpy(), ba), (ref.gy.numpy(), bb), (ref.gy.numpy(), ba), (ref.gx.numpy(), bb)]]
                for ch, tt in enumerate(terms):
                    must, may = sg.footprint_union(tt)
                    must, may = must[:, 1:-1, 1:-1], may[:, 1:-1, 1:-1]                   # the valid region
                    try:
                        sg.check_sandwich(got[:, ch], np.broadcast_to(clean[0, ch], got[:, ch].shape), must, may, RES_TOL,
                                          lone_nan=name == "nan")
                    except AssertionError as e:
                        raise AssertionError(f"{kind} {sides} ({X}, {Y}) {name}: {e}") from None
