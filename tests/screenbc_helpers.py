"""Shared by tests/test_screenbc_cpu.py and tests/test_gpu_screenbc.py: the inputs of every case of the screens and
statistics under boundary conditions on the x-y rim, and their float64 reference.  No code of the package is used here.

Reference: ``bcres_helpers.residual64(kind, vars, cond)`` - the fp64 restatement that tests/golden/bcres.npz pins to the
reference's ``pad_signal`` - uncropped.  Inputs: ``screen_helpers.fields(kind, shape, seed)`` (the wave unsqueezed to one
channel; the noise grows from sample to sample, so the scores lie apart).  Modulation and levels: the recipe of
``screen_helpers.modulation`` / ``Case._levels`` applied to the bc residual.  Tolerances: ``screen_helpers``' own
(tau = 1e-5 max |r_ref|; score within tau / m_min + one fp32 ulp; a count off by no more than the cells with
``||r_ref| - q_k m| <= tau``; ``accept`` exact), and for the statistics those of tests/SCREENSTATS_TESTS.md (``max_abs``
within tau + one ulp, the means within tau, the mean square within tau (2 max |r_ref| + tau)).

Conditions on the reference alone (asserted by tests/test_screenbc_cpu.py for every case the GPU tests use): undecided
cells at most 1 % of the counted cells for every (level, sample); every level at least 2 tau / m_min from every score; some
level splits the samples (where there is more than one sample: one sample cannot be split).  A case that misses one gets
another seed or shape here, never a wider cap."""
import contextlib
import functools

import numpy as np
import torch

import bcres_helpers as bh
import screen_helpers as sh

KINDS = bh.KINDS_2D
CONDS = {**{t: t for t in bh.BC_KINDS}, "mixed": bh.MIXED, "wrap": "wrap"}       # name -> what ``bc=`` takes
CYCLE = tuple(CONDS)                                                              # the five types, MIXED, 'wrap'
DIRICHLET_25 = {s: ("dirichlet", 2.5) for s in bh.SIDES}
CONDS["dirichlet25"] = DIRICHLET_25
CONDS["inexpressible"] = bh.MIXED_INEXPRESSIBLE          # (no pre_bc_t says it: the three-pass route)


@contextlib.contextmanager
def one_thread():
    """The fp64 convolutions of these small grids on one thread (many threads on a few thousand cells are several times
    slower); the setting is put back."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def fields(kind, shape, seed=0, n=None):
    """float32 CPU [B,F,T,X,Y]: what ``bcres_helpers.residual64`` takes (the wave as one channel)."""
    x = sh.fields(kind, shape, seed, n)
    return x[:, None] if sh.NCHAN[kind] is None else x


def package_input(kind, x):
    return x[:, 0] if kind == "wave" else x


def modulation(kind, shape, cond, seed=0):
    cal = bh.residual64(kind, fields(kind, shape, seed + 100, n=sh.N_CAL).double(), cond)
    gen = torch.Generator().manual_seed(31 * seed + sum(shape))
    u = 0.5 + 1.5 * torch.rand(cal.shape[1:], generator=gen, dtype=torch.float64)
    return (u * cal.std(dim=0, unbiased=False)).float()


class Case(sh.Case):
    """One case under ``cond`` (a key of ``CONDS``): ``screen_helpers.Case`` with the bc residual as ``r_ref``; ``ref``:
    the statistics of the counted region in float64."""

    def __init__(self, kind, shape, cond, crop, with_mod=True, nk=4, seed=0):
        self.kind, self.shape, self.cond, self.nk, self.coef = kind, tuple(shape), cond, nk, None
        self.crop, self.boundary = tuple(crop), tuple(crop) == (0, 0, 0)
        self.bc = CONDS[cond]
        self.x = fields(kind, shape, seed)
        self.mod = modulation(kind, shape, self.bc, seed) if with_mod else None
        r = self.r_ref = bh.residual64(kind, self.x.double(), self.bc)
        reg = sh.region(self.shape, self.crop)
        self.a = r[reg].abs().reshape(r.shape[0], -1)
        m = self.mod.double() if with_mod else torch.ones(r.shape[1:], dtype=torch.float64)
        self.m = m[reg[1:]].reshape(-1)
        self.cells = self.m.numel()
        self.rmax = float(r.abs().max())
        self.tau = 1e-5 * self.rmax
        self.m_min = float(self.m.min())
        self.s_ref = (self.a / self.m).max(dim=1).values
        self.tol_s = self.tau / self.m_min
        self.q = self._levels()
        hw = self.q.double()[:, None] * self.m[None, :]
        d = self.a[None] - hw[:, None]
        self.count_ref = (d <= 0).sum(dim=2)
        self.undecided = (d.abs() <= self.tau).sum(dim=2)
        self.accept_ref = self.s_ref[None, :] <= self.q.double()[:, None]
        rr = r[reg].reshape(r.shape[0], -1)
        self.ref = {"sum": rr.sum(dim=1), "sum_abs": rr.abs().sum(dim=1), "sum_sq": (rr * rr).sum(dim=1),
                    "max_abs": rr.abs().max(dim=1).values}

    def conditions(self):
        """(ok, text): the three conditions of the module docstring on the reference alone."""
        share, dist, split = self.caps()
        ok = share <= 0.01 and dist >= 2.0 and (split or self.shape[0] == 1)
        return ok, f"{self.kind} {self.shape} {self.cond} crop {self.crop}: undecided {share:.4f}, distance {dist:.2f}, split {split}"


@functools.lru_cache(maxsize=None)
def case(kind, shape, cond, crop, with_mod=True, nk=4, seed=0):
    """Computed once, shared by the tests that need it, never modified."""
    with one_thread():
        return Case(kind, shape, cond, crop, with_mod, nk, seed)


# ------------------------------------------------------------------ the cases of tests/test_gpu_screenbc.py
# (tiles: 32 x 64 below Ny = 96, 16 x 128 below 192, 8 x 256 from there)
SEAM_X = (2, 7, 8, 9, 17)            # a ghost row in the only tile; X = 8: none, the mapped halo row hx == X; partial last tiles
SEAM_Y = (4, 8, 252, 256, 260)       # one quad (left and right edge in one lane); a last quad short of the tile edge; a tile
                                     # edge that is the grid edge; a second tile of one quad
EXTRA_XY = ((17, 128), (16, 100), (33, 16), (32, 64))
SEAM_T = (3, 9, 1, 40, 2)            # T = 1 and 2 at crop (0, 0, 0) only
SEAM_B = (3, 1)


def seam_cases(kind):
    """(kind, shape, cond, crop) over SEAM_X x SEAM_Y and EXTRA_XY; T, B and the condition cycle, the crop alternates where
    T allows the time rim to be cropped.  T = 40 is kept to the narrow grids (the fp64 reference is computed on the CPU)."""
    out = []
    xy = [(x, y) for x in SEAM_X for y in SEAM_Y] + list(EXTRA_XY)
    for i, (X, Y) in enumerate(xy):
        T = SEAM_T[i % len(SEAM_T)]
        if T == 40 and Y > 16:
            T = 9
        B = SEAM_B[(i // 2) % 2]
        crop = (0, 0, 0) if T <= 2 or i % 3 == 0 else (1, 0, 0)
        out.append((kind, (B, T, X, Y), CYCLE[i % len(CYCLE)], crop))
    out.append((kind, (3, 40, 8, 8), "wrap", (1, 0, 0)))                 # (T = 40 whatever the cycle gave)
    out.append((kind, (3, 40, 8, 256), "mixed", (1, 0, 0)))              # (... and on the 8 x 256 tile: three marches of its T axis)
    return out


DIAGONAL = ((4, 3, 2, 4), (3, 9, 7, 8), (3, 3, 8, 252), (3, 2, 9, 256), (3, 3, 17, 260), (3, 9, 33, 16), (3, 3, 16, 100),
            (3, 3, 16, 128))
OTHER_KINDS = ("ns_continuity", "mhd_continuity", "mhd_momentum", "mhd_energy", "mhd_induction", "mhd_gauss")


def diagonal_cases():
    out = []
    for j, kind in enumerate(OTHER_KINDS):
        for i, shape in enumerate(DIAGONAL):
            crop = (0, 0, 0) if shape[1] <= 2 or (i + j) % 2 else (1, 0, 0)
            out.append((kind, shape, CYCLE[(i + j) % len(CYCLE)], crop))
    return out


INTERIOR_SHAPES = ((3, 3, 9, 260), (3, 3, 17, 8), (3, 3, 16, 128), (3, 3, 8, 256))
TIME_RIM = tuple(("wave", (3, T, 9, 8), "dirichlet25", (0, 0, 0)) for T in (1, 2, 3)) + \
    tuple(("ns_momentum", (3, T, 9, 8), "dirichlet25", (0, 0, 0)) for T in (1, 2, 3))
FALLBACK_SHAPE, ODD_SHAPE = (3, 3, 9, 8), (3, 3, 9, 10)
EXTRA_REF_CASES = (("ns_momentum", FALLBACK_SHAPE, "wrap", (1, 0, 0)), ("ns_momentum", ODD_SHAPE, "symmetric", (1, 0, 0)),
                   ("ns_momentum", FALLBACK_SHAPE, "inexpressible", (1, 0, 0)), ("ns_momentum", FALLBACK_SHAPE, "neumann", (1, 0, 0)),
                   ("ns_momentum", FALLBACK_SHAPE, "symmetric", (1, 0, 0)))


def gpu_cases():
    """Every (kind, shape, cond, crop) with levels that tests/test_gpu_screenbc.py screens against the fp64 reference."""
    out = seam_cases("wave") + seam_cases("ns_momentum") + diagonal_cases() + list(TIME_RIM) + list(EXTRA_REF_CASES)
    return list(dict.fromkeys(out))


def stats_tolerances(c):
    """name -> allowed error of the per-sample ``max_abs``, ``mean``, ``mean_abs``, ``mean_sq`` (SCREENSTATS_TESTS.md)."""
    ulp = torch.from_numpy(np.spacing(c.ref["max_abs"].float().numpy()).astype(np.float64))
    return {"max_abs": c.tau + ulp, "mean": c.tau, "mean_abs": c.tau, "mean_sq": c.tau * (2 * c.rmax + c.tau)}
