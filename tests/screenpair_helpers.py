"""Helpers shared by tests/test_screenpair_cpu.py and tests/test_gpu_screenpair.py: the paired screen of the data-driven
scores (cp_pre_amd.screen with ``minus=`` and ``pair=True``, csrc/screen_pair.hip), its inputs and their float64 reference.

Inputs: the truth is ``screen_helpers.fields(kind, shape, seed)``, the prediction ``fields(kind, shape, seed + 50)``, the
modulation U[0.5, 2] times the per-cell std of the difference of the residuals of two calibration sets (seeds + 100 and
+ 150, ``N_CAL`` samples each).

Reference: the oracle in float64 (``screen_helpers.oracle_residual``) on both sets, ``d_ref = r_ref(a) - r_ref(b)``; from it
``s_ref``, ``count_ref`` and the levels exactly as ``screen_helpers.Case`` builds them from a single residual.

Tolerances: each half is held to DESIGN section 3's tensor-scale bound, so ``tau = 1e-5 * (max |r_ref(a)| + max |r_ref(b)|)``;
the score within ``tau / m_min`` plus one fp32 ulp; a cell is undecided at level k if ``||d_ref| - q_k m| <= tau`` and the
counts may differ from ``count_ref`` by the undecided cells of that (level, sample); ``accept`` is exact.  That rests on caps
which tests/test_screenpair_cpu.py asserts, from the oracle alone, for every case the GPU file uses (``gpu_cases``): at most
max(1 cell, 1 %) of the counted cells undecided per (level, sample), every level further than ``2 tau / m_min`` from every
``s_ref`` (the GPU's score and the three-pass route's may each be ``tau / m_min`` off), one level that splits the samples.
``SEEDS`` holds the seed of a case that misses a cap at seed 0."""
import torch

import screen_helpers as sh
import screenflat_helpers as sf

KINDS = ("wave", "ns_continuity", "ns_momentum", "mhd_continuity", "mhd_gauss")
PAIR_KIND = {k: sh.FUSED_KIND[k] for k in KINDS}
# what has no paired screen, with the reason the host gives
UNPAIRED = {"mhd_momentum": "no paired screen for mhd_momentum", "mhd_energy": "no paired screen for mhd_energy",
            "mhd_induction": "no paired screen for mhd_induction"}
NY_BASE = sh.SEAM_SHAPES["two_tseg"]          # (3, 17, 5, 12)
FLAT_BASE = sf.BASE                           # (3, 10, 5, 12)
NK = {"ny": 6, "flat": 10}
NY_SEAM_KINDS = ("wave", "ns_momentum")
FLAT_SEAM_KINDS = ("wave", "ns_momentum", "mhd_continuity")
ODD_NY = (3, 5, 9, 13)                        # "row width not a multiple of 4"
ODD_FLAT = (3, 10, 5, 13)                     # "merged row Ny*Nt not a multiple of 4"


def route(kind, form):
    return "fused:" + ("flat_" if form == "flat" else "") + "pair_" + PAIR_KIND[kind]


def modulation(kind, shape, seed=0, coef=None):
    """float32 [T,X,Y]: U[0.5, 2] times the per-cell std of r(cal_a) - r(cal_b) over ``sh.N_CAL`` calibration pairs."""
    kw = {} if coef is None else {"coef": coef}
    ca = sh.oracle_residual(kind, sh.fields(kind, shape, seed + 100, n=sh.N_CAL).double(), **kw)
    cb = sh.oracle_residual(kind, sh.fields(kind, shape, seed + 150, n=sh.N_CAL).double(), **kw)
    gen = torch.Generator().manual_seed(31 * seed + sum(shape))
    u = 0.5 + 1.5 * torch.rand(ca.shape[1:], generator=gen, dtype=torch.float64)
    return (u * (ca - cb).std(dim=0, unbiased=False)).float()


class PairCase(sh.Case):
    """``screen_helpers.Case`` for the difference of two residuals: ``x`` the truth, ``y`` the prediction."""

    def __init__(self, kind, shape, boundary, with_mod, nk, seed=0, crop=None, coef=None):
        self.kind, self.shape, self.boundary, self.nk, self.seed, self.coef = kind, tuple(shape), boundary, nk, seed, coef
        self.crop = tuple(crop) if crop is not None else ((0, 0, 0) if boundary else (1, 1, 1))
        kw = {} if coef is None else {"coef": coef}                                   # (``coef``: as ``sh.Case`` takes it)
        self.x, self.y = sh.fields(kind, shape, seed), sh.fields(kind, shape, seed + 50)
        self.mod = modulation(kind, shape, seed, **kw) if with_mod else None
        ra, rb = sh.oracle_residual(kind, self.x.double(), **kw), sh.oracle_residual(kind, self.y.double(), **kw)
        self.r_ref = r = ra - rb
        reg = sh.region(self.shape, self.crop)
        self.a = r[reg].abs().reshape(r.shape[0], -1)
        m = self.mod.double() if with_mod else torch.ones(r.shape[1:], dtype=torch.float64)
        self.m = m[reg[1:]].reshape(-1)
        self.cells = self.m.numel()
        self.tau = 1e-5 * (float(ra.abs().max()) + float(rb.abs().max()))
        self.m_min = float(self.m.min())
        self.s_ref = (self.a / self.m).max(dim=1).values
        self.tol_s = self.tau / self.m_min
        self.q = self._levels()
        hw = self.q.double()[:, None] * self.m[None, :]
        d = self.a[None] - hw[:, None]
        self.count_ref = (d <= 0).sum(dim=2)
        self.undecided = (d.abs() <= self.tau).sum(dim=2)
        self.accept_ref = self.s_ref[None, :] <= self.q.double()[:, None]

    def caps_hold(self):
        """(do the caps hold, (undecided cells at the worst (level, sample), counted cells, distance of the closest level
        from a score in units of tau / m_min, does a level split the samples))"""
        share, dist, split = self.caps()
        worst = int(self.undecided.max())
        return (worst <= max(1, self.cells // 100) and dist > 2.0 and split and self.m_min > 0), (worst, self.cells, dist, split)


# (kind, shape, boundary, with_mod) -> the seed for which the oracle meets the caps (default 0).  Chosen by hand: every
# case of ``gpu_cases`` was built at seeds 0, 1, ... and the first seed at which ``caps_hold`` is true was taken; one case
# needed another seed than 0.  tests/test_screenpair_cpu.py asserts the caps at the seed tabulated here and that no entry
# names a case no test uses; it does not search.
SEEDS = {
    ("mhd_continuity", (3, 18, 5, 12), False, False): 1,       # straddle_18, cropped, no modulation: a level 0.9 tau from a score
}

_cache = {}


def case(kind, shape, boundary=False, with_mod=True, nk=None, form="ny"):
    """The case of (kind, shape, boundary, with_mod) at ``nk`` levels (default: ``NK[form]``), built once and shared: the
    tests read it and leave it unchanged."""
    nk = NK[form] if nk is None else nk
    key = (kind, tuple(shape), bool(boundary), bool(with_mod), nk)
    if key not in _cache:
        _cache[key] = PairCase(kind, shape, boundary, with_mod, nk, seed=SEEDS.get(key[:4], 0))
    return _cache[key]


def gpu_cases():
    """Every (kind, shape, boundary, with_mod, nk) that tests/test_gpu_screenpair.py compares with the reference."""
    out = []
    for kind in KINDS:                                           # 1. every kind x form x boundary x modulation
        for form, shape in (("ny", NY_BASE), ("flat", FLAT_BASE)):
            for boundary in (False, True):
                for with_mod in (False, True):
                    out.append((kind, shape, boundary, with_mod, NK[form]))
    for kind in NY_SEAM_KINDS:                                   # 2. the seams, with and without modulation
        for shape in sh.SEAM_SHAPES.values():
            for boundary in (False, True):
                for with_mod in (False, True):
                    out.append((kind, shape, boundary, with_mod, NK["ny"]))
    for kind in FLAT_SEAM_KINDS:
        for with_mod in (False, True):
            for shape in sf.SEAM_SHAPES.values():
                for boundary in (False, True):
                    out.append((kind, shape, boundary, with_mod, NK["flat"]))
            out.append((kind, sf.SMALLEST_Y, True, with_mod, NK["flat"]))
    for kind in ("ns_momentum", "wave"):                         # 6. the fallbacks by shape
        out.append((kind, ODD_NY, False, True, NK["ny"]))
        out.append((kind, ODD_FLAT, False, True, NK["flat"]))
        out.append((kind, next(iter(sf.FALLBACK_SHAPES)), False, True, NK["flat"]))
    for kind in UNPAIRED:
        out.append((kind, NY_BASE, False, True, NK["ny"]))
    return sorted(set(out), key=repr)
