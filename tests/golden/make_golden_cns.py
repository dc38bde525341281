#!/usr/bin/env python3
"""Generate tests/golden/cns.npz by RUNNING THE REFERENCE's ``Euler_FV_OS_rhs.forward`` in the build container.

Run once, with the reference checkout present:  python tests/golden/make_golden_cns.py <path of the reference checkout>
The GPU box never sees the reference; only the .npz travels.  Nothing of the reference is copied into this repo.

What is executed from the reference:
  * ``Active_Learning/CNS.py`` - imported by file path; ``Euler_FV_OS_rhs.forward`` (:18-31) is called as it stands;
  * ``Utils/VectorConvOps_Spatial.py`` - its ``Divergence`` and ``Laplace`` (with their ``BoundaryManager``), built with the
    arguments of ``CNS.py:15-16``, and its ``dot``;
  * ``Utils/ConvOps_Spatial.py`` - two spatial ``ConvOperator`` objects on the CPU, built with the arguments ``Gradient``
    gives its sub-operators (``VectorConvOps_Spatial.py:37-38``).

What is NOT: ``Euler_FV_OS_rhs.__init__`` and ``Gradient.__init__``.  ``Gradient`` hard-codes ``device='cuda'`` for its
sub-operators and cannot be constructed in a CPU-only container, so the module is created without running its
constructor and gets a stand-in gradient: the two CPU sub-operators and a ``BoundaryManager``, applied the way
``Gradient.__call__`` applies them (``:46-56``: pad both inputs, concatenate the two results along the channels).
"""
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DX = 0.0078
SHAPES = ((3, 4, 9, 12), (2, 4, 8, 16))
BCS = (("periodic", 0.0), ("dirichlet", 0.75), ("neumann", 0.0), ("symmetric", 0.0))


class StandInGradient:
    """``Gradient`` with its sub-operators on the CPU."""

    def __init__(self, scale, boundary_cond):
        # (CNS.py rebinds the name ConvOperator to the [BS,Nt,Nx,Ny] operator at :41: the spatial one is taken from its module)
        from ConvOps_Spatial import ConvOperator
        from boundary_conditions import BoundaryManager
        self.grad_x = ConvOperator('x', 1, scale, 2, 'direct', device=torch.device("cpu"), requires_grad=True)
        self.grad_y = ConvOperator('y', 1, scale, 2, 'direct', device=torch.device("cpu"), requires_grad=True)
        self.bc = BoundaryManager(kernel_size=(3, 3))
        self.bc.set_all_boundaries(bc_type=boundary_cond)

    def __call__(self, input_x, input_y=None):
        padded = [self.bc.pad_signal(t) for t in (input_x, input_x if input_y is None else input_y)]
        return torch.cat((self.grad_x(padded[0]), self.grad_y(padded[1])), dim=1)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    warnings.filterwarnings("ignore")
    sys.path[:0] = [ref, os.path.join(ref, "Utils")]
    spec = importlib.util.spec_from_file_location("ref_cns", os.path.join(ref, "Active_Learning", "CNS.py"))
    ns = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ns)

    out = {"_note": np.array("Active_Learning/CNS.py Euler_FV_OS_rhs.forward on the reference's Divergence / Laplace and a "
                             "CPU stand-in for Gradient (see make_golden_cns.py)"),
           "dx": np.array(DX), "bcs": np.array([b for b, _ in BCS]), "bc_values": np.array([v for _, v in BCS])}
    rng = np.random.default_rng(20240702)
    for i, shape in enumerate(SHAPES):
        out[f"vars_{i}"] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
    for bc, value in BCS:
        m = ns.Euler_FV_OS_rhs.__new__(ns.Euler_FV_OS_rhs)
        torch.nn.Module.__init__(m)
        m.dx = torch.tensor(DX, dtype=torch.float32, requires_grad=True)
        m.dy = torch.tensor(DX, dtype=torch.float32, requires_grad=True)
        m.gamma = torch.tensor(5 / 3, dtype=torch.float32, requires_grad=True)
        m.gradient = StandInGradient(1 / (m.dx), bc)
        m.laplace = ns.Laplace(scale=1 / (m.dx ** 2), taylor_order=2, boundary_cond=bc, device='cpu', requires_grad=True)
        m.divergence = ns.Divergence(scale=1 / (m.dx), taylor_order=2, boundary_cond=bc, device='cpu', requires_grad=True)
        for op in (m.gradient, m.laplace, m.divergence):
            op.bc.set_all_boundaries(bc_type=bc, value=value)
        for i in range(len(SHAPES)):
            out[f"rhs_{bc}_{i}"] = m.forward(torch.from_numpy(out[f"vars_{i}"])).detach().numpy()
        if bc == "periodic":
            for name, op in (("gx", m.gradient.grad_x), ("gy", m.gradient.grad_y), ("dx", m.divergence.grad_x),
                             ("dy", m.divergence.grad_y), ("lap", m.laplace.laplace)):
                out["kernel_" + name] = op.kernel.detach().numpy()
            out["gamma"] = m.gamma.detach().numpy()
    path = os.path.join(HERE, "cns.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
