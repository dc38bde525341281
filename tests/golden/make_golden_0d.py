#!/usr/bin/env python3
"""Generate tests/golden/convops_0d.npz by RUNNING THE REFERENCE's ODE operator in the build container.

Run once, here, with the reference checkout present:  python tests/golden/make_golden_0d.py
The GPU box never sees the reference; only the .npz travels.  Nothing of the reference is copied into this repo.

What is executed from the reference:
  * ``Utils/ConvOps_0d.py`` - imported: the whole ``get_stencil`` table (invalid pairs recorded as such); the
    constructor quirks; ``convolution``, ``spectral_convolution`` and ``differentiate`` / ``integrate`` for every
    ``correlation`` x ``slice_pad`` combination at Nt in {1, 2, 3, 7, 100, 150}, for a 3-, 5- and 7-tap kernel (``integrate``
    of the scaled stencils at eps = 0.3, and at the default eps for the integer [1, -2, 1], see ``gen_apply``);
  * the operator statements of ``Inverse_residuals/DHO/DHO_NODE.py`` - :469-485 (combined ``D_damped``), :505-515
    (split ``D_R1(v) + D_R2(x)``) and :558-565 (``-D_R4(v) + D_R3(x)``) - and of
    ``Inverse_residuals/SHO/SHO_node_test.py`` :334-342, compiled from the files' own lines on a seeded trajectory;
  * ``analyze_residuals`` of ``Inverse_residuals/Bessel/Bessel_NODE.py`` (:473-523, the loop of :502-518), compiled
    from the file with ``ast`` and run on a seeded trajectory.
"""
import ast
import os
import sys
import warnings

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
warnings.filterwarnings("ignore")
sys.path[:0] = [REF, os.path.join(REF, "Utils")]

from Utils.ConvOps_0d import ConvOperator as Ref0D, get_stencil as ref_stencil   # noqa: E402

NTS = (1, 2, 3, 7, 100, 150)
KERNELS = {3: (2, 2), 5: (2, 4), 7: (2, 6)}          # k -> (deriv_order, taylor_order)
EPS_INTEG = 0.3                                     # integrate of the scaled stencils (see gen_apply)


def lines(relpath, lo, hi, must_contain):
    """Source lines lo..hi (1-based, inclusive) of a reference file; refuse if the file drifted."""
    src = open(os.path.join(REF, relpath)).read().splitlines()[lo - 1:hi]
    text = "\n".join(src)
    for m in must_contain:
        assert m in text, (relpath, lo, hi, m)
    return compile(text, f"{relpath}:{lo}-{hi}", "exec")


def gen_stencils(out):
    for d in (0, 1, 2, 3, None):
        for t in (2, 4, 6, 8):
            key = f"stencil_d{d}_t{t}"
            try:
                out[key] = ref_stencil(d, t).numpy()
            except ValueError:
                out[key + "_invalid"] = np.array(1)
    op = Ref0D()
    out["ctor_default_has_kernel"] = np.array(hasattr(op, "kernel"))
    op = Ref0D(order=2, scale=0.5, taylor_order=4, requires_grad=True)
    out["ctor_scaled_kernel"] = op.kernel.numpy()
    out["ctor_scaled_requires_grad"] = np.array(op.kernel.requires_grad)
    out["ctor_scaled_requires_grad_attr"] = np.array(op.kernel.requires_grad_ is True)


def gen_apply(out):
    rng = np.random.default_rng(0)
    for nt in NTS:
        x = rng.standard_normal((3, nt)).astype(np.float32)
        out[f"x_nt{nt}"] = x
        for k, (d, t) in KERNELS.items():
            op = Ref0D(order=d, taylor_order=t, scale=0.7)
            xt = torch.from_numpy(x)
            out[f"conv_nt{nt}_k{k}"] = op.convolution(xt).numpy()
            try:
                out[f"spec_nt{nt}_k{k}"] = op.spectral_convolution(xt).numpy()
            except RuntimeError:
                out[f"spec_nt{nt}_k{k}_error"] = np.array(1)
            for corr in (False, True):
                for sp in (False, True):
                    tag = f"nt{nt}_k{k}_c{int(corr)}_s{int(sp)}"
                    # integrate divides by K^ + eps; a difference stencil has K^ = 0 at DC only up to the FFT's round-off,
                    # which differs between FFT libraries and CPUs, so at eps = 1e-6 the result is pinned only for taps
                    # whose sum is exact (the integer [1, -2, 1]); the scaled stencils are pinned at a conditioned eps
                    calls = (("diff", lambda: op.differentiate(xt, correlation=corr, slice_pad=sp)),
                             ("integ", lambda: op.integrate(xt, correlation=corr, slice_pad=sp, eps=EPS_INTEG)))
                    if k == 3:
                        calls += (("integ_exact", lambda: Ref0D(order=2).integrate(xt, correlation=corr, slice_pad=sp)),)
                    for name, fn in calls:
                        try:
                            out[f"{name}_{tag}"] = fn().numpy()
                        except RuntimeError:
                            out[f"{name}_{tag}_error"] = np.array(1)


def _trajectory(nt, seed):
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 10.0, nt)
    sol = np.stack([np.cos(1.3 * t) + 0.05 * rng.standard_normal(nt), -1.3 * np.sin(1.3 * t) + 0.05 * rng.standard_normal(nt)], 1)
    return t, sol


def gen_scripts(out):
    t, sol = _trajectory(150, 1)
    m, c, k = 1.5, 0.3, 2.0
    ns = {"torch": torch, "ConvOperator": Ref0D, "t": t, "neural_sol": sol, "m": m, "c": c, "k": k}
    rel = "Inverse_residuals/DHO/DHO_NODE.py"
    exec(lines(rel, 469, 485, ["D_damped.kernel = 2*m*D_tt.kernel", "residuals = D_damped(x)"]), ns)
    exec(lines(rel, 505, 515, ["D_R1.kernel", "D_R2.kernel", "residuals_r1r2 ="]), ns)
    exec(lines(rel, 558, 565, ["D_R3.kernel", "D_R4.kernel", "residuals_r3r4 ="]), ns)
    out["dho_t"], out["dho_sol"] = t, sol.astype(np.float32)
    out["dho_mck"] = np.array([m, c, k])
    out["dho_dt"] = np.array(ns["dt"])
    out["dho_kernel_combined"] = ns["D_damped"].kernel.numpy()
    out["dho_combined_spectral"] = ns["residuals"].numpy()
    out["dho_combined_direct"] = ns["D_damped"].convolution(ns["x"]).numpy()
    out["dho_kernel_r1"], out["dho_kernel_r2"] = ns["D_R1"].kernel.numpy(), ns["D_R2"].kernel.numpy()
    out["dho_split"] = ns["residuals_r1r2"].numpy()
    out["dho_kernel_r3"], out["dho_kernel_r4"] = ns["D_R3"].kernel.numpy(), ns["D_R4"].kernel.numpy()
    out["dho_kinematic"] = ns["residuals_r3r4"].numpy()

    t, sol = _trajectory(100, 2)
    omega = 1.3
    ns = {"torch": torch, "ConvOperator": Ref0D, "t": t, "m": 1.0, "k": omega ** 2,
          "x": torch.tensor(sol[:, 0], dtype=torch.float32).unsqueeze(0)}
    exec(lines("Inverse_residuals/SHO/SHO_node_test.py", 334, 342, ["D_pos.kernel = m*D_tt.kernel"]), ns)
    out["sho_t"], out["sho_sol"], out["sho_omega"] = t, sol.astype(np.float32), np.array(omega)
    out["sho_kernel"] = ns["D_pos"].kernel.numpy()
    out["sho_direct"] = ns["D_pos"](ns["x"]).numpy()


def gen_bessel(out):
    rel = "Inverse_residuals/Bessel/Bessel_NODE.py"
    tree = ast.parse(open(os.path.join(REF, rel)).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "analyze_residuals"]
    assert len(fn) == 1
    ns = {"torch": torch, "np": np, "ConvOperator": Ref0D}
    exec(compile(ast.Module(body=fn, type_ignores=[]), rel, "exec"), ns)
    rng = np.random.default_rng(3)
    x = np.linspace(-2.0, 8.0, 121)                     # passes through x = 0 (left at 0 by the loop)
    sol = np.stack([np.cos(x) + 0.01 * rng.standard_normal(x.size), -np.sin(x)], 1)
    for n in (0, 1, 2):
        res, _ = ns["analyze_residuals"](x, sol, n)
        out[f"bessel_res_n{n}"] = res.numpy()
    out["bessel_x"], out["bessel_sol"] = x, sol.astype(np.float32)


def main():
    out = {"_note": np.array("executed from the reference: Utils/ConvOps_0d.py; DHO_NODE.py:469-485,505-515,558-565; "
                             "SHO_node_test.py:334-342; Bessel_NODE.py analyze_residuals")}
    torch.manual_seed(0)
    gen_stencils(out)
    gen_apply(out)
    gen_scripts(out)
    gen_bessel(out)
    path = os.path.join(HERE, "convops_0d.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
