"""Helpers shared by tests/test_vjpflat_cpu.py and tests/test_gpu_vjpflat.py: the fused loss backward for Nt-fastest views
(``flat=True`` of cp_pre_amd.losses, csrc/vjp_flat.hip).

The reference is ``losses_helpers.ref_vjp`` / ``ref_loss`` in float64 - the mathematics has no layout - under the ``TOL`` of
the loss tests (tests/LOSSES_TESTS.md).  Shapes are the logical (BS, Nt, Nx, Ny); ``nt_fastest`` puts a tensor on the device
with memory [BS,(F),Nx,Ny,Nt].  ``split`` restates the kernel's split rule (the header of csrc/vjp_flat.hip: every stream is
staged); the seams are named from it."""
import torch

import stencil_guards as sg

TOL = 1e-5                       # tests/LOSSES_TESTS.md: tensor-scale relative error, overall and per gradient channel
ROUTES = ("wave", "ns_continuity", "ns_momentum")          # one per pre_vjpflat_*_f32 entry
FLAT_KIND = {"wave": "stencil3d", "op3d": "stencil3d", "ns_continuity": "linear2", "ns_continuity_yfix": "linear2",
             "ns_momentum": "ns_momentum", "ns_momentum_yfix": "ns_momentum", "pre_ns": "ns_momentum"}

# ------------------------------------------------------------------ the split rule of csrc/vjp_flat.hip, restated
FLAT_NT, FLAT_H, FLAT_NT_GAIN, FLAT_MAX_Y = 512, 32, 8, 96
MIN_SLOTS = 256          # resident workgroups: at least one per CU of an MI355X


def halo_quads(Nt):
    """quads staged per side of a chunk: as far as an x-neighbour (Nt cells away) reaches"""
    return min(FLAT_H, (Nt + 3) // 4)


def chunk(quads, Nt):
    """flat_chunk(): threads (= quads) per workgroup"""
    halo, nt = 2 * halo_quads(Nt), FLAT_NT
    for c in range(nt - 64, 255, -64):
        if -(-quads // c) * (c + halo) * 100 < -(-quads // nt) * (nt + halo) * (100 - FLAT_NT_GAIN):
            nt = c
    return nt


def pick_tseg(tiles, T, slots):
    """star_march.hip's pick_tseg"""
    best, bestc, tseg = T, 1e300, T
    while True:
        wgs = tiles * -(-T // tseg)
        rounds = wgs / slots
        full = (1.0 if rounds <= 1.0 else float(-(-wgs // slots))) + 0.5
        cost = (1.0 + 3.0 / tseg) * full / rounds
        if cost < bestc * 0.99:
            best, bestc = tseg, cost
        if tseg <= 16:
            return best
        tseg = (tseg + 1) // 2


def split(shape, slots=MIN_SLOTS):
    """dict(nt, nCh, last, hq, tSeg, nTSeg, last_planes) for the logical (BS, Nt, Nx, Ny): chunk width in quads, chunks per
    merged row, quads of the row's last chunk, halo quads per side, planes per march of Nx, marches, planes of the last."""
    B, Nt, Nx, Ny = shape
    assert (Ny * Nt) % 4 == 0 and Nt < FLAT_MAX_Y
    quads = Ny * Nt // 4
    nt = chunk(quads, Nt)
    nch = -(-quads // nt)
    tseg = pick_tseg(B * nch, Nx, slots)
    nseg = -(-Nx // tseg)
    return dict(nt=nt, nCh=nch, last=quads - (nch - 1) * nt, hq=halo_quads(Nt), tSeg=tseg, nTSeg=nseg,
                last_planes=Nx - (nseg - 1) * tseg)


# logical (BS, Nt, Nx, Ny) of the GPU cases, by the seam they cross
SEAM_SHAPES = {
    "one_chunk_one_march": (2, 8, 10, 16),    # the shape of test_residual_vjp_fallbacks_still_match
    "straddle_10": (2, 10, 5, 6),             # Nt % 4 = 2, L = 60: row ends inside quads
    "straddle_6": (2, 6, 5, 10),
    "chunk_seam": (2, 60, 5, 36),             # L = 2160 cells: chunks of 320 + 220 quads, 15 halo quads staged per side
    "bound": (2, 92, 5, 24),                  # Nt just under the merged-row form's bound: 23 halo quads
    "two_marches": (2, 8, 17, 16),            # the smallest Nx that is cut: marches of 9 + 8 planes
    "full_last_march": (2, 8, 18, 16),        # 9 + 9
    "one_plane_last_march": (2, 8, 136, 16),  # 15 x 9 + 1
}
DECLINED = {(2, 96, 5, 12): "fallback:Nt >= 96", (2, 7, 5, 9): "fallback:merged row Ny*Nt not a multiple of 4"}


# ------------------------------------------------------------------ layouts
def nt_fastest(t, device):
    """The CPU tensor ``t`` ([BS,F,Nt,Nx,Ny] or [BS,Nt,Nx,Ny]) on ``device`` as the ``permute`` view of a contiguous
    [BS,(F),Nx,Ny,Nt] one: the same logical tensor, Nt-fastest."""
    d, n = t.to(device), t.dim()
    fwd = tuple(range(n - 3)) + (n - 2, n - 1, n - 3)
    back = tuple(range(n - 3)) + (n - 1, n - 3, n - 2)
    return d.permute(fwd).contiguous().permute(back)


def nt_fastest_embedded(t, device, offset=1, batch_gap=12):
    """(allocation, view): the same Nt-fastest view inside an allocation the test owns (``stencil_guards.embed``), samples
    ``batch_gap`` floats further apart than they are long and the base ``offset`` floats off a 16-byte boundary; the rows
    of the view stay dense."""
    n = t.dim()
    order = list(range(n - 3)) + [n - 2, n - 1, n - 3]             # slowest first: ..., Nx, Ny, Nt
    return sg.embed(t, order, {0: batch_gap}, offset, device)


def is_nt_fastest_dense(v):
    """dense rows in memory order [.., Nx, Ny, Nt] (what the flat entries accept)"""
    Nt, Ny = v.shape[-3], v.shape[-1]
    return v.stride(-3) == 1 and v.stride(-1) == Nt and v.stride(-2) == Ny * Nt


def script_view(pred):
    """Physics_Informed/Wave_FNO_PISL.py:209-211: [BS,1,Nx,Ny,Nt] -> the cropped Nt-fastest view [BS,Nt-2,Nx-2,Ny-2]"""
    return pred[:, 0, 1:-1, 1:-1, 1:-1].permute(0, 3, 1, 2)
