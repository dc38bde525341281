"""Helpers shared by tests/test_vjpflatmhd_cpu.py and tests/test_gpu_vjpflatmhd.py: the fused backward of the ideal-MHD
residual losses for Nt-fastest views (``mhd="flat"`` of cp_pre_amd.losses, csrc/vjp_flat_mhd.hip, libcp_pre_vjpflatmhd.so).

Nothing is restated here: the expressions, their closed forms, the operator sets and the tolerance are
``mhdvjp_helpers``' (``MHDRoute``, ``closed_form``, ``EQS``, ``CHAN``, ``OPSETS``, ``TOL``), the split rule, the seams and
the layouts are ``vjpflat_helpers``' (``SEAM_SHAPES``, ``split``, ``nt_fastest``, ``nt_fastest_embedded``).  Shapes are the
logical (BS, Nt, Nx, Ny).

The five-stream functors (induction, pass B of momentum and of energy) hold 92 160 B of LDS: ONE workgroup per CU, so the
resident slots of an MI355X are 256 - the ``MIN_SLOTS`` the seams of ``vjpflat_helpers`` were named with.  The assertion
below keeps every seam crossing what it is named for at that count (and at any larger one: the three- and four-stream
launches of the same equations fit more workgroups)."""
import torch

import vjpflat_helpers as vf
from mhdvjp_helpers import CHAN, EQS, OPSETS, TOL, MHDRoute, closed_form  # noqa: F401  (re-exported)
from vjpflat_helpers import SEAM_SHAPES, nt_fastest, nt_fastest_embedded, split  # noqa: F401

EQ4 = ("continuity", "induction", "momentum", "energy")            # the entries of libcp_pre_vjpflatmhd.so
SLOTS = 256
FIVE_STREAM_LDS = 2 * 5 * (vf.FLAT_NT + 2 * vf.FLAT_H) * 16
assert FIVE_STREAM_LDS == 92160 and 160 * 1024 // FIVE_STREAM_LDS == 1 and SLOTS == vf.MIN_SLOTS

_sp = {k: split(s, SLOTS) for k, s in SEAM_SHAPES.items()}
for _k, _s in SEAM_SHAPES.items():
    assert _s[0] * _sp[_k]["nCh"] * _sp[_k]["nTSeg"] < SLOTS and _sp[_k] == split(_s, 1 << 20), _k
assert _sp["one_chunk_one_march"]["nCh"] == 1 and _sp["one_chunk_one_march"]["nTSeg"] == 1
assert all(SEAM_SHAPES[k][1] % 4 == 2 and _sp[k]["nCh"] == 1 for k in ("straddle_10", "straddle_6"))
assert (_sp["chunk_seam"]["nCh"], _sp["chunk_seam"]["last"], _sp["chunk_seam"]["hq"]) == (2, 220, 15)
assert SEAM_SHAPES["bound"][1] == vf.FLAT_MAX_Y - 4 and _sp["bound"]["hq"] == 23 and _sp["bound"]["nCh"] == 2
assert (_sp["two_marches"]["nTSeg"], _sp["two_marches"]["last_planes"]) == (2, 8)
assert (_sp["full_last_march"]["nTSeg"], _sp["full_last_march"]["last_planes"]) == (2, 9)
assert (_sp["one_plane_last_march"]["nTSeg"], _sp["one_plane_last_march"]["last_planes"]) == (16, 1)

# One cell in all, one quad in all, and Nt = 1: the x-neighbour is the ADJACENT cell of the merged row, one halo quad per
# side, and no cell has a y-neighbour.  (With Nt = 1 the view has unit stride on Ny as well: the losses hand it to the
# tiled library, as any unit-stride input; the GPU file runs that shape through the entries themselves.)
DEGENERATE = [(1, 4, 1, 1), (1, 2, 3, 2), (2, 1, 3, 4)]
assert all((s[1] * s[3]) % 4 == 0 for s in DEGENERATE) and vf.halo_quads(1) == 1
GPU_SHAPES = list(SEAM_SHAPES.values()) + DEGENERATE
DECLINED = vf.DECLINED


def nt_fastest_exact(t, device):
    """``vjpflat_helpers.nt_fastest`` with the strides written out: the CPU tensor ``t`` ([BS,F,Nt,Nx,Ny] or [BS,Nt,Nx,Ny])
    on ``device``, memory [BS,(F),Nx,Ny,Nt], stride(Nt) = 1, stride(Ny) = Nt, stride(Nx) = Ny*Nt whatever the extents (torch
    is free to give an axis of extent 1 any stride; the library's layout conditions read them all)."""
    n = t.dim()
    Nt, Nx, Ny = t.shape[-3:]
    lead, acc = [], Nx * Ny * Nt
    for d in reversed(t.shape[:n - 3]):
        lead.insert(0, acc)
        acc *= d
    out = torch.empty_strided(tuple(t.shape), tuple(lead) + (1, Ny * Nt, Nt), dtype=t.dtype, device=device)
    out.copy_(t.to(device))
    return out


def is_flat_view(v):
    """does ``mhd="flat"`` offer ``v`` to the merged-row library?  (no unit stride on its last axis)"""
    return v.stride(-1) != 1


def expected_route(route, v):
    """the fused route of ``route`` on the device view ``v`` under ``mhd="flat"``"""
    return "fused:" + ("flat_" if is_flat_view(v) else "") + route.kind
