"""GPU tests (pytest -m gpu) of the coverage at every calibration level (cp_pre_amd/csrc/coverage_levels.hip) at every
instantiation and seam: cov_levels_kernel<NK, CENTRE, JOINT> for NK = 1 .. 16 in all four forms and the host loop's second
and third launch (17, 32, 33 levels), the tails of the eight-deep sample loop, the 64-sample group edge and the 256-cell
chunk edge, and a grid whose workgroups each walk two or three chunks - through ``icp.emp_cov_levels``,
``icp.emp_cov_joint_levels`` and ``icp.filter_sims_joint_levels``, against tests/select_helpers.py's numpy reference (bounds in
fp32, one rounded operation per operation; counted in float64), compared with ``==``.  tests/SELECT_TESTS.md has the table."""
import numpy as np
import pytest
import torch

import select_helpers as sh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN, INF = np.float32(np.nan), np.float32(np.inf)


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    from cp_pre_amd import _lib
    _lib.load_cov()
    return torch.device(DEV)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if x is not None else None


def marginal(yd, q, cd, inside, what):
    """emp_cov_levels on per-cell (or scalar) levels == the reference's count / total, level by level"""
    from cp_pre_amd import inductive_cp as icp
    got = icp.emp_cov_levels(dev(q), yd, centre=cd)
    counts, want = sh.cov_marginal(inside)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    assert np.array_equal(got, want), (what, (got * inside[0].size).round().astype(np.int64).tolist(), counts.tolist())
    return counts


def joint(yd, q, md, cd, inside, what):
    """emp_cov_joint_levels and filter_sims_joint_levels == the reference's samples with every cell inside"""
    from cp_pre_amd import inductive_cp as icp
    keep, counts, want = sh.cov_joint(inside)
    got = icp.emp_cov_joint_levels(dev(q), yd, md, centre=cd)
    assert got.dtype == np.float64 and np.array_equal(got, want), (what, (got * keep.shape[1]).round().tolist(), counts.tolist())
    flags = icp.filter_sims_joint_levels(dev(q), yd, md, centre=cd)
    assert flags.dtype == torch.bool and tuple(flags.shape) == keep.shape, what
    assert np.array_equal(flags.cpu().numpy(), keep), (what, np.argwhere(flags.cpu().numpy() != keep)[:8].tolist())
    return counts


def distinct(counts, what):
    """every level different from every other: a level swapped with its neighbour cannot pass"""
    assert len(set(int(c) for c in counts)) == len(counts), (what, [int(c) for c in counts])


# ================================================================================================ 1. every level count
N1, M1 = 65, 257                                       # one full group of 64 samples and a group of one; two chunks, the second of one cell
LEVEL_COUNTS = list(range(1, 17)) + [17, 32, 33]


def marginal_operands(nk, rng):
    """y, c [n, M], per-cell levels q [nk, M] that grow with k; NaN and +-inf in y, c and q, q = 0 (with a sample on it),
    negative q, subnormal q, and a sample exactly on the low and on the high bound of the middle level."""
    y = rng.standard_normal((N1, M1)).astype(np.float32)
    c = (0.4 * rng.standard_normal((N1, M1))).astype(np.float32)
    base = (0.7 + 0.6 * rng.random(M1)).astype(np.float32)
    q = ((0.15 + 0.09 * np.arange(nk, dtype=np.float32))[:, None] * base[None, :]).astype(np.float32)
    y[3, 5], y[4, 6], y[5, 7] = NAN, INF, -INF
    c[6, 8], c[7, 9], c[8, 10] = NAN, INF, -INF
    y[7, 9] = INF                                                    # y = c = inf: inf - hw <= inf <= inf + hw, inside
    kb = nk // 2
    q[0, 11], q[nk - 1, 12], q[kb, 13] = NAN, INF, -INF
    q[0, 14], q[nk - 1, 15], q[kb, 16] = 0.0, -0.5, 1e-42
    y[9, 14] = c[9, 14]                                              # on a half-width of 0, with a centre ...
    y[10, 14] = 0.0                                                  # ... and without
    y[11, 16], y[12, 16] = 5e-43, -2e-42                             # inside / outside a subnormal half-width (no centre)
    return y, c, q, kb


@pytest.mark.parametrize("nk", LEVEL_COUNTS)
def test_marginal_every_level_count(gpu, nk):
    """cov_levels_kernel<NK, CENTRE, false> for every NK (nk = 17, 32, 33: a second and a third launch, whose levels start at
    q + k0 q_ld and whose counts at count + k0), every level different from every other."""
    rng = np.random.default_rng(100 + nk)
    y, c, q, kb = marginal_operands(nk, rng)
    with np.errstate(all="ignore"):
        yc = y.copy()
        yc[11, 20] = c[11, 20] - q[kb, 20]                           # exactly on the low bound of level kb
        yc[12, 21] = c[12, 21] + q[kb, 21]                           # ... on the high bound
        y[11, 22], y[12, 23] = -q[kb, 22], q[kb, 23]
    for name, yy, cc, cells in (("no centre", y, None, ((11, 22), (12, 23))), ("centre", yc, c, ((11, 20), (12, 21)))):
        inside = sh.cov_inside(yy, q, None, cc)
        for s, j in cells:
            assert inside[kb, s, j] and (kb == 0 or not inside[kb - 1, s, j]), (name, s, j)
        assert inside[0, 10 if cc is None else 9, 14] and not inside[0, 9 if cc is None else 10, 14]
        if cc is None:
            assert inside[kb, 11, 16] and not inside[kb, 12, 16]
        counts = marginal(dev(yy), q, dev(cc), inside, (nk, name))
        distinct(counts, (nk, name))


def joint_operands(nk, rng):
    """Residual r [n, M] (y without a centre), centre c, modulation m, levels q [nk] such that level k keeps the samples
    s + 1 <= 2k + 1: sample s is decided by one cell that holds (s + 1) delta m against a half-width (2k + 1.5) delta m, every
    other cell stays below 0.9 of it.  The test then breaks samples 4, 10, 28 by NaN / +inf / -inf in y and 16, 22, 34 by
    NaN / +inf / -inf in c (at most one of the two samples a level adds); m holds inf (always inside), 0 and a subnormal
    (inside only where r is 0, and sample 1 waits behind a subnormal half-width until level 3)."""
    delta = np.float32(0.05)
    m = (0.5 + rng.random(M1)).astype(np.float32)
    u = (0.9 * (2 * rng.random((N1, M1)) - 1)).astype(np.float32)
    amp = np.arange(1, N1 + 1, dtype=np.float32)[:, None] * delta
    with np.errstate(all="ignore"):
        r = (u * amp * m[None, :]).astype(np.float32)
        dec = 30 + (np.arange(N1) * 3) % 200                         # the deciding cell of each sample
        r[np.arange(N1), dec] = (amp[:, 0] * m[dec] * np.where(np.arange(N1) % 2 == 0, 1, -1)).astype(np.float32)
        q = (delta * (2 * np.arange(nk, dtype=np.float32) + np.float32(1.5))).astype(np.float32)
        m[2], m[3], m[4] = INF, 0.0, 1e-39
        r[:, 3] = 0.0
        r[:, 4] = 0.0
        r[1, 4] = 3e-40                                              # inside from q_k 1e-39 >= 3e-40 on: level 3
        r[:, 2] = (1000 * u[:, 2]).astype(np.float32)                # anything finite is inside an infinite half-width
    c = (0.4 * rng.standard_normal((N1, M1))).astype(np.float32)
    c[:, 3:5] = 0.0                                                  # (so that y = c + r keeps the subnormal)
    return r, c, m, q


SPECIAL_LEVELS = (NAN, INF, -INF, np.float32(0.0), np.float32(-0.5), np.float32(1e-30), np.float32(0.7), np.float32(2.5))


@pytest.mark.parametrize("nk", LEVEL_COUNTS)
def test_joint_every_level_count(gpu, nk):
    """cov_levels_kernel<NK, CENTRE, true> for every NK and the later launches' `inside + k0 inside_ld`: level k keeps
    2k + 1 samples less the broken ones, every level different from every other; a sample's deciding cell is exactly on
    its bound at the level that first keeps it.  Then the same operands at levels NaN, +-inf, 0, negative, 1e-30 (times a
    modulation of 1e-10: a subnormal or zero half-width), and with a NaN and a -inf in the modulation (nothing inside)."""
    rng = np.random.default_rng(200 + nk)
    r, c, m, q = joint_operands(nk, rng)
    with np.errstate(all="ignore"):
        # samples 2k (s + 1 = 2k + 1) sit 0.5 delta m inside level k's bound; put every fourth exactly ON it, on the high
        # bound and on the low one in turn
        for k in range(0, nk, 2):
            s = 2 * k
            if s < N1:
                j = 30 + (s * 3) % 200
                r[s, j] = q[k] * m[j] if k % 4 == 0 else -(q[k] * m[j])
        yc = (c + r).astype(np.float32)
        for k in range(0, nk, 2):
            s = 2 * k
            if s < N1:
                j = 30 + (s * 3) % 200
                hw = (q[k] * m[j]).astype(np.float32)
                yc[s, j] = c[s, j] + hw if k % 4 == 0 else c[s, j] - hw
    r[4, 100], r[10, 101], r[28, 102] = NAN, INF, -INF
    yc[4, 100], yc[10, 101], yc[28, 102] = NAN, INF, -INF
    c[16, 103], c[22, 104], c[34, 105] = NAN, INF, -INF
    rb = r.copy()
    rb[16, 103], rb[22, 104], rb[34, 105] = NAN, INF, -INF           # (the centre-free form breaks the same samples)
    md = dev(m)
    for name, yy, cc in (("no centre", rb, None), ("centre", yc, c)):
        inside = sh.cov_inside(yy, q, m, cc)
        keep = inside.all(axis=2)
        for k in range(0, nk, 2):
            if 2 * k < N1 and 2 * k not in (4, 10, 16, 22, 28):
                assert keep[k, 2 * k] and (k == 0 or not keep[k - 1, 2 * k]), (name, k)
        assert not keep[:min(nk, 3), 1].any() and (nk <= 3 or keep[3, 1])
        counts = joint(dev(yy), q, md, dev(cc), inside, (nk, name))
        distinct(counts, (nk, name))
        # special levels, a tiny modulation, a NaN in the modulation
        q2 = np.array([SPECIAL_LEVELS[(k + nk) % len(SPECIAL_LEVELS)] for k in range(nk)], np.float32)
        m2 = m.copy()
        m2[5] = 1e-10
        y2 = yy.copy()
        y2[:, 5] = 0.0 if cc is None else cc[:, 5]
        joint(dev(y2), q2, dev(m2), dev(cc), sh.cov_inside(y2, q2, m2, cc), (nk, name, "special levels"))
        m2[6], m2[7] = NAN, -INF
        ins = sh.cov_inside(y2, q2, m2, cc)
        assert not ins.all(axis=2).any()
        joint(dev(y2), q2, dev(m2), dev(cc), ins, (nk, name, "NaN modulation"))


# ================================================================================================ 2. loop and chunk edges
@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 128, 129])
def test_sample_loop_and_chunk_edges(gpu, n):
    """nk = 3: the tails of the eight-deep unrolled sample loop (n mod 8 in 0, 1, 7), the 64-sample group edge, and cell counts
    around the 256-cell chunk (a last chunk of 255, 1 and 256 cells; one, two and three chunks), in all four forms."""
    rng = np.random.default_rng(300 + n)
    for M in (1, 255, 256, 257, 513):
        m = (1.0 + 0.5 * rng.random(M)).astype(np.float32)
        amp = ((np.arange(n) % 7 + 1) / 7.0).astype(np.float32)[:, None]
        r = ((2 * rng.random((n, M)) - 1) * amp * m[None, :]).astype(np.float32)
        c = (0.4 * rng.standard_normal((n, M))).astype(np.float32)
        yc = (c + r).astype(np.float32)
        qj = np.array([0.3, 0.6, 0.95], np.float32)
        qm = (qj[:, None] * (0.7 + 0.6 * rng.random((3, M)))).astype(np.float32)
        r[n - 1, M - 1] = NAN                                        # the last sample's last cell
        yc[n - 1, M - 1] = NAN
        for name, yy, cc in (("no centre", r, None), ("centre", yc, c)):
            yd, cd = dev(yy), dev(cc)
            marginal(yd, qm, cd, sh.cov_inside(yy, qm, None, cc), (n, M, name))
            joint(yd, qj, dev(m), cd, sh.cov_inside(yy, qj, m, cc), (n, M, name))


# ================================================================================================ 3. several chunks per workgroup
N3, M3 = 4099, 256 * 64 + 7


def test_workgroups_walk_several_chunks(gpu):
    """n = 4099 (65 sample groups, the last of 3: 32 workgroups split the cells), M = 256 x 64 + 7 (65 chunks, the last of 7
    cells): every workgroup walks two or three chunks and carries tot[] (marginal) and flags[] (joint) across them.  nk = 2,
    all four forms.  The marginal levels are per cell and cover part of the cells; the joint levels keep every sample but the
    planted ones, whose ONLY violation lies in the last chunk of some workgroup's run (the last, partial chunk among them) or
    in its first - at level 0 alone or at both levels."""
    groups, chunks, splits = sh.cov_plan(N3, M3)
    runs = sh.cov_chunk_runs(chunks, splits)
    assert (groups, chunks, splits) == (65, 65, 32) and {b - a for a, b in runs} == {2, 3} and M3 - 256 * (chunks - 1) == 7
    rng = np.random.default_rng(3)
    r = rng.random((N3, M3), dtype=np.float32)
    r -= np.float32(0.5)                                             # |r| <= 0.5
    m = (1.0 + 0.5 * rng.random(M3)).astype(np.float32)
    qj = np.array([1.0, 2.0], np.float32)
    qm = (np.array([0.15, 0.35], np.float32)[:, None] * (0.7 + 0.6 * rng.random((2, M3)))).astype(np.float32)
    planted = {}
    for i, (a, b) in enumerate(runs):
        s = (i * 131 + 7) % N3                                       # (distinct samples, spread over the groups)
        first = i % 5 == 4                                           # a few in the run's FIRST chunk, the others in its last
        ch = a if first else b - 1
        j = min(ch * 256 + (i * 37) % 256, M3 - 1)
        both = i % 2 == 1
        r[s, j] = (3.0 if both else 1.5) * m[j] * (-1 if i % 3 == 0 else 1)
        planted[s] = both
    s_last = N3 - 1                                                  # the last group's last sample, the last cell of the partial chunk
    r[s_last, M3 - 1] = 1.5 * m[M3 - 1]
    planted[s_last] = False
    assert len(planted) == splits + 1
    c = np.ascontiguousarray(r[::-1]) * np.float32(0.25)
    yc = c + r
    md = dev(m)
    for name, yy, cc in (("no centre", r, None), ("centre", yc, c)):
        inside = np.empty((2, 2, N3, M3), bool)                      # [marginal / joint, level]
        inside[0] = sh.cov_inside(yy, qm, None, cc)
        inside[1] = sh.cov_inside(yy, qj, m, cc)
        keep = inside[1].all(axis=2)
        want = np.ones((2, N3), bool)
        for s, both in planted.items():
            want[0, s] = False
            want[1, s] = not both
        assert np.array_equal(keep, want)
        assert (inside[1, 0].sum(axis=1)[list(planted)] == M3 - 1).all()      # one violation per planted sample, no more
        yd, cd = dev(yy), dev(cc)
        counts = marginal(yd, qm, cd, inside[0], name)
        distinct(counts, name)
        assert 0 < counts[0] < counts[1] < N3 * M3
        joint(yd, qj, md, cd, inside[1], name)
