"""Helpers shared by tests/test_screenstats_cpu.py and tests/test_gpu_screenstats*.py: the per-sample statistics of a
residual (cp_pre_amd.screen.screen_stats / ScreenStats, libcp_pre_screenstats.so) and their float64 reference.

Reference: the residual in float64 by the oracle, built as tests/screen_helpers.py, screenflat_helpers.py and
screen1d_helpers.py build theirs (their ``Case`` classes without a modulation; one level, which nothing here uses).  From it,
over the counted region and in float64: sum r, sum |r|, sum r^2, max |r|.

Tolerances, from the project's parity rule: the device's fp32 residual is within
tau = 1e-5 max |r_ref| of the exact one in every cell.  Hence
  max_abs             within tau + one fp32 ulp (the result is an fp32 number);
  mean, mean_abs      within tau (a mean of per-cell errors is at most the largest of them; the fp64 additions add
                      cells * 2^-53 relative, nothing next to 1e-5);
  mean_sq             within tau (2 max |r_ref| + tau)  (|a^2 - b^2| = |a - b| |a + b|)."""
import functools

import numpy as np
import torch

import screen1d_helpers as s1
import screen_helpers as sh
import screenflat_helpers as sf

NY_MAIN = ("two_tseg", "rows2_narrow", "rows3_wide")
FLAT_MAIN = ("straddle_10", "two_chunks", "two_marches")
NY_SEAM_KINDS = ("ns_momentum", "lap", "mhd_momentum")
FLAT_SEAM_KINDS = sf.SEAM_KINDS                       # wave, ns_momentum, mhd_induction
ROWS_SEAM_KINDS = ("burgers", "advection")
SLAB_SHAPE = (3, 12, 41, 64)                          # the grid tests/test_gpu_screen.py cuts into slabs
PARENT_KINDS = ("ns_momentum", "wave", "burgers")     # max_abs against the joint screen's score, bit for bit


def route(kind, form):
    """The route string of the statistics of ``kind`` in ``form`` ('ny', 'flat', 'rows')."""
    if form == "rows":
        return s1.ROUTE[kind].replace("rows_", "rows_stats_")
    return "fused:" + ("flat_" if form == "flat" else "") + "stats_" + sh.FUSED_KIND[kind]


class Ref:
    """The float64 statistics of an uncropped reference residual ``r`` [B, ...] over the region ``crop`` leaves."""

    def __init__(self, r, crop):
        reg = sh.region(tuple(r.shape), crop)
        c = r[reg].double().reshape(r.shape[0], -1)
        self.cells = c.shape[1]
        self.sum, self.sum_abs, self.sum_sq = c.sum(dim=1), c.abs().sum(dim=1), (c * c).sum(dim=1)
        self.max_abs = c.abs().max(dim=1).values
        self.rmax = float(r.abs().max())
        self.tau = 1e-5 * self.rmax

    def mean(self):
        return self.sum / self.cells

    def mean_abs(self):
        return self.sum_abs / self.cells

    def mean_sq(self):
        return self.sum_sq / self.cells


def check(stats, ref, what):
    """``stats`` (a ``SampleStats``) against ``ref`` with the module's tolerances; prints every figure before it asserts."""
    n = ref.sum.shape[0]
    assert stats.cells == ref.cells, (what, stats.cells, ref.cells)
    for name in ("sum", "sum_abs", "sum_sq"):
        t = getattr(stats, name)
        assert t.dtype == torch.float64 and tuple(t.shape) == (n,), (what, name, t.dtype, t.shape)
    assert stats.max_abs.dtype == torch.float32 and tuple(stats.max_abs.shape) == (n,)
    got_max = stats.max_abs.double().cpu()
    ulp = torch.from_numpy(np.spacing(ref.max_abs.float().numpy()).astype(np.float64))
    e_max = (got_max - ref.max_abs).abs()
    e_mean = (stats.mean().cpu() - ref.mean()).abs()
    e_abs = (stats.mean_abs().cpu() - ref.mean_abs()).abs()
    e_sq = (stats.mean_sq().cpu() - ref.mean_sq()).abs()
    tol_sq = ref.tau * (2 * ref.rmax + ref.tau)
    print(f"{what}: max_abs err {float(e_max.max()):.3e}, mean err {float(e_mean.max()):.3e}, mean_abs err "
          f"{float(e_abs.max()):.3e} (allowed tau = {ref.tau:.3e}); mean_sq err {float(e_sq.max()):.3e} (allowed {tol_sq:.3e})")
    assert bool((e_max <= ref.tau + ulp).all()), (what, "max_abs", e_max, ref.tau)
    assert bool((e_mean <= ref.tau).all()), (what, "mean", e_mean, ref.tau)
    assert bool((e_abs <= ref.tau).all()), (what, "mean_abs", e_abs, ref.tau)
    assert bool((e_sq <= tol_sq).all()), (what, "mean_sq", e_sq, tol_sq)
    assert torch.equal(stats.rms(), torch.sqrt(stats.mean_sq()))      # (on the statistics' own device: one square root)


# ---- the cases: inputs and reference, computed once and shared (never modified: tests clone what they change) -----------
@functools.lru_cache(maxsize=None)
def ny_case(kind, shape, boundary=False):
    c = sh.Case(kind, shape, boundary, False, 1)
    c.ref = Ref(c.r_ref, c.crop)
    return c


@functools.lru_cache(maxsize=None)
def flat_case(kind, shape, boundary=False):
    c = sh.Case(kind, shape, boundary, False, 1, seed=sf.SEEDS.get((kind, tuple(shape)), 0))
    c.ref = Ref(c.r_ref, c.crop)
    return c


@functools.lru_cache(maxsize=None)
def rows_case(kind, B, plane, layout, boundary=False):
    c = s1.Case(kind, s1.logical_shape(B, plane, layout), boundary, False, 1)
    c.ref = Ref(c.r_ref, c.crop)
    return c


def same_bits(a, b):
    """Do two ``SampleStats`` hold the same bit patterns in all four outputs?"""
    return all(torch.equal(getattr(a, n).view(torch.int64), getattr(b, n).view(torch.int64)) for n in ("sum", "sum_abs", "sum_sq")) \
        and torch.equal(a.max_abs.view(torch.int32), b.max_abs.view(torch.int32))


def sums_close(a, whole):
    """Each sum of ``a`` within cells * 2^-52 * sum_abs of ``whole``'s: the bound of two fp64 recursive sums of the same
    terms in different orders.  The terms of sum_sq are r^2, whose absolute sum is sum_sq itself: it is held to the smaller
    of the two bounds."""
    bound = whole.cells * 2.0 ** -52 * whole.sum_abs
    d = [(getattr(a, n) - getattr(whole, n)).abs() for n in ("sum", "sum_abs", "sum_sq")]
    print("slab sums: largest differences", [float(x.max()) for x in d], "bound", float(bound.min()))
    return bool((d[0] <= bound).all()) and bool((d[1] <= bound).all()) and \
        bool((d[2] <= torch.minimum(bound, whole.cells * 2.0 ** -52 * whole.sum_sq)).all())


# ---- the ordering cases: sample b has amplitude 1 + 0.05 b -----------------------------------------------------------------
def amplitude_fields(base):
    """``base`` ([T,X,Y] or [F,T,X,Y] or [T,X], float64) scaled per sample: x[b] = (1 + 0.05 b) * base, 8 samples, float32."""
    amp = 1.0 + 0.05 * torch.arange(8, dtype=torch.float64)
    return (amp.reshape(-1, *([1] * base.dim())) * base[None]).float()


def wave_order_input():
    """[8,T,X,Y] for the wave residual (linear: the per-sample mean |r| scales with the amplitude)."""
    base = sh.fields("wave", (1, 8, 12, 16), seed=3)[0].double()
    return amplitude_fields(base)


def advection_order_input():
    base = s1.fields((1, 16, 24), seed=3)[0].double()
    return amplitude_fields(base)


def burgers_order_input():
    """[8,Nt,Nx] for the signed mean of the Burgers residual: a ramp in t under a smooth mode, so that dx * D_t(u) has a
    mean well away from zero that grows with the amplitude."""
    T, X = 16, 24
    t = torch.arange(T, dtype=torch.float64)[:, None] / T
    x = torch.arange(X, dtype=torch.float64)[None, :] / X
    base = 1.0 + 2.0 * t + 0.1 * torch.sin(2 * np.pi * (x + t))
    return amplitude_fields(base)


def order_is_decided(values, tau):
    """Neighbouring values (sorted) differ by more than 4 tau: the order is the data's, not the rounding's."""
    v = torch.sort(values).values
    return bool(((v[1:] - v[:-1]) > 4 * tau).all())
