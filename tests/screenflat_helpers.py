"""Helpers shared by tests/test_screenflat_cpu.py and tests/test_gpu_screenflat.py: the fused screen of Nt-fastest views of
the 2-D residuals (cp_pre_amd.screen's flat route, csrc/screen_flat.hip).

Reference and tolerances are those of tests/screen_helpers.py (``Case``: the oracle in float64, tau = 1e-5 max |r_ref|,
score within tau / m_min + one fp32 ulp, counts within the undecided cells, accept exact).  Shapes are the logical
(B, T, X, Y); ``to_layout`` puts a tensor on the device with memory [B,(F),X,Y,T].  ``split`` restates the kernel's split
rule (the header of csrc/screen_flat.hip); the seams are named from it.  ``SEEDS`` holds, per (kind, shape), the seed of
``screen_helpers.fields`` for which the oracle meets the caps of tests/test_screenflat_cpu.py (default 0)."""
import screen_helpers as sh

KINDS = tuple(k for k in sh.KINDS if sh.FUSED_KIND.get(k))
ROUTE = {k: "fused:flat_" + sh.FUSED_KIND[k] for k in KINDS}
# does the functor of ``kind`` stage a field through LDS in this layout (default operators: the reference's tap structure
# relabelled, MODE 3)?  Every MHD equation has its taps on the kernel's marched and y axes only.
STAGED = {k: not k.startswith("mhd_") or k == "mhd_gauss" for k in KINDS}


def to_layout(t, device):
    """The CPU tensor ``t`` ([B,F,T,X,Y], [B,T,X,Y] or a modulation [T,X,Y]) on ``device`` as the ``permute`` view of a
    contiguous [B,(F),X,Y,T] one: the same logical tensor, Nt-fastest."""
    d, n = t.to(device), t.dim()
    fwd = tuple(range(n - 3)) + (n - 2, n - 1, n - 3)
    back = tuple(range(n - 3)) + (n - 1, n - 3, n - 2)
    return d.permute(fwd).contiguous().permute(back)


# ------------------------------------------------------------------ the split rule of csrc/screen_flat.hip, restated
FLAT_NT, FLAT_H, FLAT_NT_GAIN, FLAT_MAX_Y = 512, 32, 8, 96
MIN_SLOTS = 256          # resident workgroups: at least one per CU of an MI355X


def halo_quads(T, staged):
    """quads staged per side of a chunk: as far as an x-neighbour (Nt cells away) reaches"""
    return min(FLAT_H, (T + 3) // 4) if staged else 0


def chunk(quads, T, staged):
    """flat_chunk(): threads (= quads) per workgroup"""
    halo, nt = 2 * halo_quads(T, staged), FLAT_NT
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


def split(shape, staged, slots=MIN_SLOTS):
    """dict(nt, nCh, last, hq, tSeg, nTSeg) for the logical (B, T, X, Y): chunk width in quads, chunks per merged row, quads
    of the row's last chunk, halo quads per side, planes per march of Nx and marches."""
    B, T, X, Y = shape
    assert (Y * T) % 4 == 0 and T < FLAT_MAX_Y and Y > 1
    quads = Y * T // 4
    nt = chunk(quads, T, staged)
    nch = -(-quads // nt)
    tseg = pick_tseg(B * nch, X, slots)
    return dict(nt=nt, nCh=nch, last=quads - (nch - 1) * nt, hq=halo_quads(T, staged), tSeg=tseg, nTSeg=-(-X // tseg))


BASE = (3, 10, 5, 12)
# logical (B, T, X, Y) of the GPU cases, by the seam they cross
SEAM_SHAPES = {
    "straddle_10": (3, 10, 5, 12),            # Nt % 4 = 2: every other row end lies inside a quad
    "straddle_18": (3, 18, 5, 12),
    "straddle_30": (3, 30, 5, 12),
    "whole_rows": (3, 64, 5, 4),              # a wave's 256 cells are four whole rows
    "widest_halo": (3, 95, 5, 12),            # 24 halo quads per side, just under the limit
    "two_chunks": (3, 20, 5, 128),            # merged row of 2560 cells: two chunks of 320 quads
    "chunk_seam": (3, 30, 5, 70),             # 525 quads: chunks of 320 + 205, row ends inside quads on both sides of the seam
    "one_counted_plane": (3, 10, 3, 12),      # Nx = 3: cropped, one marched plane is counted
    "two_marches": (3, 10, 17, 12),           # Nx = 17: marches of 9 + 8 planes
    "many_marches_last_one": (3, 10, 65, 12),  # Nx = 65: 7 x 9 + 2 planes; cropped, the last march counts one plane
}
SMALLEST_Y = (3, 10, 5, 2)                    # boundary=True only: the crop leaves no cell of two columns
SEAM_KINDS = ("wave", "ns_momentum", "mhd_induction")
FALLBACK_SHAPES = {(3, 96, 5, 12): "fallback:Nt >= 96", (3, 10, 5, 13): "fallback:merged row Ny*Nt not a multiple of 4"}
SLAB = ((3, 10, 5, 12), slice(2, 8))          # a t-slab [:, :, 2:8] of an Nt-fastest tensor: "fallback:rows not dense"

SEEDS = {("wave", (3, 10, 3, 12)): 1, ("wave", (3, 10, 5, 2)): 1}


def case(kind, shape, boundary=False, with_mod=True, nk=10, crop=None):
    return sh.Case(kind, shape, boundary, with_mod, nk, seed=SEEDS.get((kind, tuple(shape)), 0), crop=crop)
