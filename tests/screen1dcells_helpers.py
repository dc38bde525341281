"""Helpers shared by tests/test_screen1dcells_cpu.py and tests/test_gpu_screen1dcells.py: the per-cell screen of the 1-D
family (``cp_pre_amd.screen.screen_cells`` / ``ScreenCells`` with ``rows=True``, csrc/screen_rows_cells.hip).

Built on tests/screen1d_helpers.py (the fields, the float64 oracle residual, ``lay``, ``split``, ``SEAM_PLANES``) and the
recipe of tests/screencells_helpers.py (``ranks``, ``N_CAL`` = 12, ``SHARE_CAP``, ``check``).

Inputs: the screened set is ``screen1d_helpers.fields(shape, seed)``; for a pair the second set is the first plus noise of
standard deviation ``PAIR_NOISE`` (seed + 50), and the residual of the case is ``d = r(a) - r(b)``.  The modulation is
``screen1d_helpers.modulation``.  The level fields are order statistics of ``|r_cal| / m`` (``m == 1`` without a modulation)
of ``N_CAL`` calibration samples drawn with ANOTHER seed (seed + 200; for pairs ``|r(a_cal) - r(b_cal)| / m`` with
``b_cal = a_cal`` + noise, seed + 250): for nk = 10 the ranks of the reference's ten alphas, for nk = 16 all twelve ranks and
four midpoints, for nk = 1 the median.  float32 ``[nk,Nt,Nx]``, uncropped.

Reference: ``count_ref[k, b] = #{|r_ref| <= q32_k * m32}`` over the counted cells in float64.  Tolerances: ``tau = 1e-5 max
|r_ref|``; a count may differ from ``count_ref`` by at most the cells with ``||r_ref| - hw| <= tau`` of that (level, sample);
the score within ``tau / m_min`` plus one fp32 ulp.  tests/test_screen1dcells_cpu.py asserts from the reference alone that in
every GPU case the undecided share stays within ``SHARE_CAP`` and that a level splits a sample's cells."""
import torch

import screen1d_helpers as s1
import screen_helpers as sh
import screencells_helpers as ch

N_CAL, SHARE_CAP, ranks, check = ch.N_CAL, ch.SHARE_CAP, ch.ranks, ch.check
KINDS, LAYOUTS = s1.KINDS, s1.LAYOUTS
ROUTE = {k: v.replace("rows_", "rows_cells_") for k, v in s1.ROUTE.items()}
ROUTE_PAIR = {k: v.replace("rows_", "rows_cells_pair_") for k, v in s1.ROUTE.items()}
FALLBACK = "fallback:1-D family: the marched axis is the batch"
PAIR_NOISE = 0.05
# (nk, name of the plane in screen1d_helpers.SEAM_PLANES) of the cases every kind runs, in both layouts
MAIN = ((10, "wave_segments"), (1, "chunks_and_idle_lanes"), (16, "partial_last_strip"))
SEAM_KINDS = ("burgers", "dxx")
PAIR_KINDS = ("burgers", "advection")
GROUP_PLANE = (12, 64)


def second_set(x, seed):
    gen = torch.Generator().manual_seed(104729 * seed + 50 + x.numel())
    return x + PAIR_NOISE * torch.randn(x.shape, generator=gen, dtype=torch.float64).float()


def residual(kind, x, y=None):
    r = s1.oracle_residual(kind, x.double())
    return r if y is None else r - s1.oracle_residual(kind, y.double())


class CellCase:
    """One per-cell screening case of the 1-D family; ``shape`` is the logical (B, Nt, Nx); ``pair``: two field sets."""

    def __init__(self, kind, shape, boundary, with_mod, nk, pair=False, seed=0):
        self.kind, self.shape, self.boundary, self.nk, self.pair = kind, tuple(shape), boundary, nk, pair
        self.crop = (0, 0) if boundary else (1, 1)
        self.x = s1.fields(self.shape, seed)
        self.y = second_set(self.x, seed) if pair else None
        self.mod = s1.modulation(kind, self.shape, seed) if with_mod else None
        self.r_ref = r = residual(kind, self.x, self.y)
        m = self.mod.double() if with_mod else torch.ones(r.shape[1:], dtype=torch.float64)
        xc = s1.fields(self.shape, seed + 200, n=N_CAL)
        cal = residual(kind, xc, second_set(xc, seed + 250) if pair else None).abs()
        s = torch.sort(cal / m, dim=0).values                                          # [12, Nt, Nx]
        self.q = torch.stack([0.5 * (s[i] + s[j]) for i, j in ranks(nk)]).float()      # [nk, Nt, Nx]
        self.reg = reg = sh.region(self.shape, self.crop)
        a = r[reg].abs().reshape(r.shape[0], -1)
        mc = m[reg[1:]].reshape(-1)
        self.cells = mc.numel()
        self.tau = 1e-5 * float(r.abs().max())
        self.s_ref = (a / mc).max(dim=1).values
        self.tol_s = self.tau / float(mc.min())
        hw = (self.q.double() * m.float().double())[(slice(None),) + reg[1:]].reshape(nk, -1)      # [nk, cells]
        d = a[None] - hw[:, None]                                                      # [nk, B, cells]
        self.a = a
        self.count_ref = (d <= 0).sum(dim=2)
        self.undecided = (d.abs() <= self.tau).sum(dim=2)

    def q_cropped(self):
        return self.q[(slice(None),) + self.reg[1:]].contiguous()

    def caps(self):
        """(largest share of undecided cells over (level, sample), does a level split the cells of a sample)"""
        share = float(self.undecided.max()) / self.cells
        return share, bool(((self.count_ref > 0) & (self.count_ref < self.cells)).any())


# key of ``case`` -> the seed at which the reference meets the caps (default 0); tests/test_screen1dcells_cpu.py asserts the
# caps at the seed tabulated here, it does not search
SEEDS = {
}
_cache = {}


def case(kind, B, plane, layout, boundary=False, with_mod=True, nk=10, pair=False):
    """The case, built once and shared: the tests read it and leave it unchanged."""
    key = (kind, s1.logical_shape(B, tuple(plane), layout), bool(boundary), bool(with_mod), nk, bool(pair))
    if key not in _cache:
        _cache[key] = CellCase(*key, seed=SEEDS.get(key, 0))
    return _cache[key]


def group_batches(G):
    """The batch sizes that cross the seam of a sample group of G: one past a group, one short of two groups."""
    return (3,) if G == 1 else tuple(sorted({G + 1, 2 * G - 1}))


def gpu_cases(G):
    """Every (kind, B, plane, layout, boundary, with_mod, nk, pair) that tests/test_gpu_screen1dcells.py compares with the
    reference; ``G``: the sample group of the build."""
    out = []
    for nk, name in MAIN:
        B, plane = s1.SEAM_PLANES[name]
        for kind in KINDS:
            for layout in LAYOUTS:
                for boundary in (False, True):
                    for with_mod in (False, True):
                        out.append((kind, B, plane, layout, boundary, with_mod, nk, False))
    for B, plane in s1.SEAM_PLANES.values():
        for kind in SEAM_KINDS:
            for layout in LAYOUTS:
                out.append((kind, B, plane, layout, False, True, 10, False))
    for B in group_batches(G):
        for layout in LAYOUTS:
            out.append(("burgers", B, GROUP_PLANE, layout, True, True, 10, False))
    for kind in PAIR_KINDS:
        for layout in LAYOUTS:
            out.append((kind, *s1.SEAM_PLANES["wave_segments"], layout, False, True, 10, True))
    for layout in LAYOUTS:                                       # an odd contiguous length: the three-pass route
        out.append(("burgers", *s1.ODD_PLANES[1], layout, False, True, 10, False))
    return sorted(set(out), key=repr)


def run(c, layout, device, **kw):
    """``screen_cells(..., rows=True)`` on case ``c`` laid out as ``layout`` on ``device`` (``kw`` overrides)."""
    from cp_pre_amd import screen
    args = dict(modulation=s1.lay(c.mod, layout, device) if c.mod is not None else None, boundary=c.boundary, rows=True)
    if c.pair:
        args["minus"] = s1.lay(c.y, layout, device)
    args.update(kw)
    q = args.pop("qcells", None)
    q = s1.lay(c.q, layout, device) if q is None else q
    return screen.screen_cells(s1.method_of(c.kind, device), s1.lay(c.x, layout, device), q, **args)


# ------------------------------------------------------------------ the block order of screen_rows_kernel under CellSets
def visits(B, R, C, G, slots=s1.MIN_SLOTS):
    """The (sample, chunk, column tile) every logical block index of the grid decodes to, None for a surplus workgroup of a
    partial last group: the decode of csrc/screen_rows.h, restated."""
    sp = s1.split(B, R, C, slots)
    nb = (B + G - 1) // G * G
    out = []
    for L in range(nb * sp["nChunk"] * sp["nCT"]):
        bl, L = L % G, L // G
        ct, L = L % sp["nCT"], L // sp["nCT"]
        ch_, grp = L % sp["nChunk"], L // sp["nChunk"]
        b = grp * G + bl
        out.append((b, ch_, ct) if b < B else None)
    return out, sp
