"""Helpers shared by tests/test_screen1d_cpu.py and tests/test_gpu_screen1d.py: the inputs of every screening case of the
1-D family on [B,Nt,Nx] and their float64 reference, from the oracle alone.

Reference and tolerances are those of tests/screen_helpers.py (``Case``: tau = 1e-5 max |r_ref|, score within tau / m_min
+ one fp32 ulp, counts within the undecided cells, accept exact), with ``oracle.residuals.burgers_residual``,
``advection_residual`` and ``oracle.convops.ConvOperator1D`` in float64 under ``oracle_fp64()``.

A case names a sample's PLANE (R rows x C columns, C the unit-stride axis: csrc/screen_rows.hip) and a layout: 'nx' is the
contiguous [B,Nt,Nx] tensor with (Nt, Nx) = (R, C); 'nt' is the Nt-fastest view ``u.permute(0,2,1)`` of a contiguous
[B,Nx,Nt] tensor, with (Nt, Nx) = (C, R).  ``split`` restates the kernel's split rule; the seams are named from it."""
import numpy as np
import torch

import screen_helpers as sh
from oracle import convops as ocv
from oracle import residuals as orr

DX, DT, NU, V, DISC = 1 / 64, 0.01, 0.002, 1.0, 2
KINDS = ("burgers", "advection", "dxx", "dt")
ROUTE = {"burgers": "fused:rows_burgers", "advection": "fused:rows_stencil2d", "dxx": "fused:rows_stencil2d",
         "dt": "fused:rows_stencil2d"}
LAYOUTS = ("nx", "nt")
N_CAL = 8


def oracle_residual(kind, x):
    """The uncropped residual of ``x`` [B,Nt,Nx] (float64 CPU) by the oracle."""
    with sh.oracle_fp64():
        if kind == "burgers":
            return orr.burgers_residual(x, DX, DT, NU, boundary=True)
        if kind == "advection":
            return orr.advection_residual(x, V, DISC, DT, DX, boundary=True)
        return ocv.ConvOperator1D("x", 2)(x) if kind == "dxx" else ocv.ConvOperator1D("t", 1)(x)


def method_of(kind, device="cpu"):
    """The ``cp_pre_amd`` method the screen takes for ``kind``."""
    from cp_pre_amd import residuals as R
    from cp_pre_amd.convops_1d import ConvOperator
    if kind == "burgers":
        return R.Burgers(DX, DT, NU, device=device).residual
    if kind == "advection":
        return R.Advection(V, DT, DX, disc=DISC, device=device).residual
    return ConvOperator("x", 2, device=device) if kind == "dxx" else ConvOperator("t", 1, device=device)


def fields(shape, seed=0, n=None):
    """float32 CPU [B,Nt,Nx]: 1 + 0.2 sin(2 pi (x + t) + phase) + noise whose amplitude grows by half from sample to sample
    (``screen_helpers.fields`` reduced to one channel and two axes)."""
    B, T, X = shape
    B = B if n is None else n
    gen = torch.Generator().manual_seed(7919 * seed + sum(shape))
    t = torch.arange(T, dtype=torch.float64)[:, None] / T
    x = torch.arange(X, dtype=torch.float64)[None, :] / X
    out = torch.empty(B, T, X, dtype=torch.float64)
    for b in range(B):
        ph = 2 * np.pi * torch.rand(1, generator=gen, dtype=torch.float64)
        out[b] = 1.0 + 0.2 * torch.sin(2 * np.pi * (x + t) + ph) + \
            0.02 * 1.5 ** (b % 8) * torch.randn(T, X, generator=gen, dtype=torch.float64)
    return out.float()


def modulation(kind, shape, seed=0):
    """float32 [Nt,Nx]: [0.5, 2] times the per-cell std of the residuals of a synthetic calibration set of N_CAL samples."""
    cal = oracle_residual(kind, fields(shape, seed + 100, n=N_CAL).double())
    gen = torch.Generator().manual_seed(31 * seed + sum(shape))
    u = 0.5 + 1.5 * torch.rand(cal.shape[1:], generator=gen, dtype=torch.float64)
    return (u * cal.std(dim=0, unbiased=False)).float()


def logical_shape(B, plane, layout):
    R, C = plane
    return (B, R, C) if layout == "nx" else (B, C, R)


class Case(sh.Case):
    """One screening case of the 1-D family; ``shape`` is the logical (B, Nt, Nx).  Levels and caps: ``screen_helpers.Case``."""

    def __init__(self, kind, shape, boundary, with_mod, nk, seed=0, crop=None):
        self.kind, self.shape, self.boundary, self.nk = kind, tuple(shape), boundary, nk
        self.crop = tuple(crop) if crop is not None else ((0, 0) if boundary else (1, 1))
        self.x = fields(self.shape, seed)
        self.mod = modulation(kind, self.shape, seed) if with_mod else None
        r = oracle_residual(kind, self.x.double())
        self.r_ref = r
        reg = sh.region(self.shape, self.crop)
        self.a = r[reg].abs().reshape(r.shape[0], -1)
        m = self.mod.double() if with_mod else torch.ones(r.shape[1:], dtype=torch.float64)
        self.m = m[reg[1:]].reshape(-1)
        self.cells = self.m.numel()
        self.tau = 1e-5 * float(r.abs().max())
        self.m_min = float(self.m.min())
        self.s_ref = (self.a / self.m).max(dim=1).values
        self.tol_s = self.tau / self.m_min
        self.q = self._levels()
        hw = self.q.double()[:, None] * self.m[None, :]
        d = self.a[None] - hw[:, None]
        self.count_ref = (d <= 0).sum(dim=2)
        self.undecided = (d.abs() <= self.tau).sum(dim=2)
        self.accept_ref = self.s_ref[None, :] <= self.q.double()[:, None]


def lay(t, layout, device):
    """``t`` ([B,Nt,Nx] or [Nt,Nx], CPU) on ``device`` in ``layout``: 'nt' = the same logical tensor with unit stride on Nt."""
    d = t.to(device)
    return d if layout == "nx" else d.transpose(-1, -2).contiguous().transpose(-1, -2)


# ------------------------------------------------------------------ the split rule of csrc/screen_rows.hip, restated
MIN_SLOTS = 256          # resident workgroups: at least one per CU of an MI355X


def split(B, R, C, slots=MIN_SLOTS):
    """dict(ws, nseg, nCT, rc, nChunk, rSeg) of rows_split(B, R, C, slots)."""
    strips = (C + 255) // 256
    ws = 4 if strips >= 3 else strips
    nseg = 4 // ws
    nCT = (strips + ws - 1) // ws
    rc = R
    while B * nCT * ((R + rc - 1) // rc) < slots and rc > 8 * nseg:
        rc = (rc + 1) // 2
    return dict(ws=ws, nseg=nseg, nCT=nCT, rc=rc, nChunk=(R + rc - 1) // rc, rSeg=(rc + nseg - 1) // nseg)


# (B, (R, C)) of the GPU cases, by the seam they cross; every one keeps >= 200 counted cells with the rim cropped
SEAM_PLANES = {
    "wave_segments": (3, (12, 64)),           # one workgroup, 4 row segments of 3 rows
    "chunks_and_idle_lanes": (3, (130, 12)),  # 8 workgroups per sample, segments of 5,5,5,2 rows; C = 12: 3 of 64 lanes work
    "chunks_odd_rows": (5, (33, 256)),        # 2 workgroups per sample (17 + 16 rows), one full strip
    "fewer_rows_than_segments": (3, (3, 256)),  # R = 3 on 4 segments of 1 row; cropped: exactly one counted row
    "partial_last_strip": (3, (5, 260)),      # 2 strips (the second holds one quad), 2 segments of 3 + 2 rows
    "two_strips_and_a_quad": (3, (40, 516)),  # 3 strips on 4 waves (one idle), 8 workgroups of 5 rows per sample
    "column_tiles": (3, (9, 1028)),           # 2 column tiles (1024 + 4 columns), 2 workgroups of 5 + 4 rows each
}
ODD_PLANES = [(3, (24, 13)), (3, (7, 66)), (3, (6, 258))]        # contiguous axis no multiple of 4: the three-pass route
