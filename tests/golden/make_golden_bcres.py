#!/usr/bin/env python3
"""Generate tests/golden/bcres.npz by RUNNING THE REFERENCE in the build container.

Run once, with the reference checkout present where make_golden.py expects it (its ``REF``):
python tests/golden/make_golden_bcres.py.  The GPU box never sees the reference; only the .npz travels.  Nothing of the
reference is copied into this repo.

The reference never joined its ``BoundaryManager`` to the time-dependent residuals; the composition it would make is
``r(pad_signal(f) for f in fields)[..., :, 1:-1, 1:-1]``.  Both halves are executed from the reference as they stand:
  * ``Utils/boundary_conditions.py`` - ``BoundaryManager(3).pad_signal`` on every [BS,Nt,Nx,Ny] field (Nt rides as the channel
    axis); for the 1-D family ``BoundaryManager((1, 3))`` on [BS,1,Nt,Nx]: left / right on Nx, no padding of the rows (time);
  * ``Other_UQ/Evaluation/PRE_estimations.py`` - ``PRE_Wave`` / ``PRE_NS`` / ``PRE_MHD`` ``.residual(padded, boundary=True)``;
  * the residual defs of ``Marginal/NS_Residuals_CP.py`` (continuity), ``Marginal/MHD_Residuals_CP.py`` (all five) and
    ``Joint/Burgers_Residuals_CP.py``, and the additive advection kernel of ``Marginal/Advection_Residuals_CP.py``, located
    with ``ast`` and compiled from the reference files as make_golden.py does (its helpers are imported, not restated).
Every result is cropped by one cell per side of x and y (of x for the 1-D family) and stored; the time axis is left whole.
"""
import importlib
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
# the five conditions and one mixed condition the fused entries can express (bottom 'periodic' over top 'neumann' is a true
# wrap, right 'neumann' over left 'dirichlet' the edge itself)
CASES = {
    "periodic": {s: ("periodic", 0.0) for s in ("left", "right", "top", "bottom")},
    "dirichlet": {s: ("dirichlet", 0.75) for s in ("left", "right", "top", "bottom")},
    "neumann": {s: ("neumann", 0.0) for s in ("left", "right", "top", "bottom")},
    "outflow": {s: ("outflow", 0.0) for s in ("left", "right", "top", "bottom")},
    "symmetric": {s: ("symmetric", 0.0) for s in ("left", "right", "top", "bottom")},
    "mixed": {"left": ("dirichlet", 1.5), "right": ("neumann", 0.0), "top": ("neumann", 0.0), "bottom": ("periodic", 0.0)},
}


def main():
    os.environ.setdefault("MPLBACKEND", "Agg")
    warnings.filterwarnings("ignore")
    sys.path.insert(0, HERE)
    import make_golden as G                      # (puts the reference checkout on sys.path and imports its operators)
    bcm = importlib.import_module("boundary_conditions")

    def manager(sides, size):
        m = bcm.BoundaryManager(kernel_size=size)
        for side, (t, v) in sides.items():
            m.set_boundary_type(side, t, v)
        return m

    g = torch.Generator().manual_seed(31)
    v6 = torch.rand(2, 6, 4, 6, 8, generator=g) + 0.5            # U(0.5, 1.5): rho, p > 0
    u1 = torch.rand(2, 6, 8, generator=g) + 0.5
    dt, dx, dy = 0.01, 1.0 / 64, 1.0 / 48
    bdx, bdt, bnu = 2.0 / 14, 1.25 / 9, 0.002
    out = {"_note": np.array("the reference's BoundaryManager.pad_signal on every field, then the reference's own residual code "
                             "on the padded fields (boundary=True), cropped by one cell per side of x and y; see "
                             "make_golden_bcres.py"),
           "vars6": v6.numpy(), "u1d": u1.numpy(), "coef": np.array([dt, dx, dy], np.float64),
           "burgers_coef": np.array([bdx, bdt, bnu], np.float64), "cases": np.array(list(CASES)),
           "wave_coef": np.array([0.01, 0.02, 1.0], np.float64)}

    ns = dict(G.ops2d(), dx=dx, dy=dy, dt=dt, nu=0.001)
    exec(G.ref_defs("Marginal/NS_Residuals_CP.py", ["residual_continuity"]), ns)
    mhd = dict(G.ops2d(), gamma=5 / 3)
    mhd_names = ["residual_continuity", "residual_momentum", "residual_energy", "residual_induction", "residual_gauss"]
    exec(G.ref_defs("Marginal/MHD_Residuals_CP.py", mhd_names), mhd)
    bur = dict(D_t=G.Ref1D(domain="t", order=1), D_x=G.Ref1D(domain="x", order=1), D_xx=G.Ref1D(domain="x", order=2),
               dx=torch.tensor(bdx, dtype=torch.float32), dt=torch.tensor(bdt, dtype=torch.float32),
               nu=torch.tensor(bnu, dtype=torch.float32))
    exec(G.ref_defs("Joint/Burgers_Residuals_CP.py", ["residual"]), bur)
    adv = dict(D_t=G.Ref1D(domain="t", order=1), D_x=G.Ref1D(domain="x", order=1), v=1.0, disc=2, dt=0.005, dx=0.01)
    D_adv = G.Ref1D()
    D_adv.kernel = eval(G.ref_assign_value("Marginal/Advection_Residuals_CP.py", "D.kernel"), adv)
    out["advection_kernel"] = D_adv.kernel.numpy()

    crop2 = (Ellipsis, slice(1, -1), slice(1, -1))
    for name, sides in CASES.items():
        m3, m1 = manager(sides, 3), manager(sides, (1, 3))
        p6 = torch.stack([m3.pad_signal(v6[:, i]) for i in range(6)], dim=1)              # [2,6,4,8,10]
        p1 = m1.pad_signal(u1[:, None])[:, 0]                                             # [2,6,10]
        assert p6.shape == (2, 6, 4, 8, 10) and p1.shape == (2, 6, 10)
        out[f"PRE_Wave|{name}"] = G.pre.PRE_Wave(dt=0.01, dx=0.02, c=1.0).residual(p6[:, :1], boundary=True)[crop2].contiguous().numpy()
        out[f"PRE_NS|{name}"] = G.pre.PRE_NS(dt, dx, dy).residual(p6[:, :3], boundary=True)[crop2].contiguous().numpy()
        out[f"PRE_MHD|{name}"] = G.pre.PRE_MHD(dt, dx, dy).residual(p6, boundary=True)[crop2].contiguous().numpy()
        out[f"ns_continuity|{name}"] = ns["residual_continuity"](p6[:, :2], boundary=True)[crop2].contiguous().numpy()
        for n in mhd_names:
            out[f"mhd_{n.split('_')[1]}|{name}"] = mhd[n](p6, boundary=True)[crop2].contiguous().numpy()
        out[f"burgers|{name}"] = bur["residual"](p1, boundary=True)[..., 1:-1].contiguous().numpy()
        out[f"advection|{name}"] = D_adv(p1)[..., 1:-1].contiguous().numpy()
    path = os.path.join(HERE, "bcres.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
