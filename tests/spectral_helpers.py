"""fp64 reference of the spectral family and the case tables of test_spectral_ref_cpu.py / test_gpu_spectral.py.

Pure numpy: nothing here reads ``cp_pre_amd``.  Two independent oracles:

``reference``  the recipe itself in float64 with ``numpy.fft``: zero-pad, ``rfftn`` of the padded field and of the kernel
               placed at the origin of a zero array, multiply by K^ | conj(K^) | 1/(K^+eps) | 1/(conj(K^)+eps), ``irfftn``
               WITHOUT a size (an odd last axis comes back one shorter, as with torch), keep the leading
               ``padded - k + 1`` samples per axis or everything.
``direct``     the direct-space circular sum ``out[i] = sum_p k[p] * xp[(i - p) mod n]`` (``(i + p)`` for the conjugate
               spectrum), with ``np.roll`` over the taps.  Defined for the multiplicative modes, and only where the
               inverse length equals the forward length (even padded last axis).

Operations (``op``): ``"xcorr"`` = ``fft_conv(x, K, padding=k//2)`` - pad k//2 per axis plus one trailing zero when the
padded last axis is odd, conjugate spectrum, always cropped; ``"diff"`` / ``"integ"`` = ``differentiate`` /
``integrate`` - pad k_last//2 on EVERY axis, no evening, K^ (conjugated for ``correlation``), cropped for ``slice_pad``.
A field is [..., *spatial]: the last ``k.ndim`` axes are transformed, every leading axis is batch.
"""
import numpy as np

EPS = 0.3                       # the well-conditioned eps of the inverting modes (the singular 1e-6 is out of scope)
MIN_DENOMINATOR = 0.5           # input condition of the inverting cases: min over bins |K^ + eps|, in fp64


# ------------------------------------------------------------------------------------------------ the recipe
def pad_field(x, k, op):
    """(padded fp64 field, its spatial extents BEFORE the evening zero)."""
    nd = k.ndim
    pads = [s // 2 for s in k.shape] if op == "xcorr" else [k.shape[-1] // 2] * nd
    lead = [(0, 0)] * (x.ndim - nd)
    xp = np.pad(np.asarray(x, np.float64), lead + [(p, p) for p in pads])
    size = xp.shape[-nd:]
    if op == "xcorr" and xp.shape[-1] % 2:
        xp = np.pad(xp, [(0, 0)] * (xp.ndim - 1) + [(0, 1)])
    return xp, size


def kernel_spectrum(k, shape):
    kz = np.zeros(shape, np.float64)
    kz[tuple(slice(0, s) for s in k.shape)] = k
    return np.fft.rfftn(kz)


def denominator(k, shape, conj, eps):
    """What the inverting modes divide by, per bin: K^ + eps or conj(K^) + eps."""
    kf = kernel_spectrum(np.asarray(k, np.float64), shape)
    return (np.conj(kf) if conj else kf) + eps


def _conj_invert(op, correlation, invert):
    if op == "xcorr":
        return True, invert
    return correlation, op == "integ"


def _crop(out, size, k, crop):
    if not crop:
        return out
    keep = tuple(slice(0, s - ks + 1) for s, ks in zip(size, k.shape))
    return out[(Ellipsis,) + keep]


def reference(x, k, op, correlation=False, slice_pad=True, eps=EPS, invert=False):
    k = np.asarray(k, np.float64)
    nd = k.ndim
    xp, size = pad_field(x, k, op)
    axes = tuple(range(-nd, 0))
    conj, inv = _conj_invert(op, correlation, invert)
    kf = kernel_spectrum(k, xp.shape[-nd:])
    if conj:
        kf = np.conj(kf)
    g = 1.0 / (kf + eps) if inv else kf
    out = np.fft.irfftn(np.fft.rfftn(xp, axes=axes) * g, axes=axes)
    return np.ascontiguousarray(_crop(out, size, k, op == "xcorr" or slice_pad))


def direct_defined(x, k, op):
    return pad_field(np.zeros(np.shape(x)), np.asarray(k), op)[0].shape[-1] % 2 == 0


def direct(x, k, op, correlation=False, slice_pad=True):
    """The multiplicative modes as a circular sum over the taps (no FFT anywhere)."""
    k = np.asarray(k, np.float64)
    nd = k.ndim
    xp, size = pad_field(x, k, op)
    assert xp.shape[-1] % 2 == 0, "the inverse transform would come back one shorter: the circular sum is another operation"
    conj, _ = _conj_invert(op, correlation, False)
    axes = tuple(range(-nd, 0))
    out = np.zeros_like(xp)
    for p in np.ndindex(*k.shape):
        if k[p] != 0:
            out += k[p] * np.roll(xp, tuple(-q for q in p) if conj else p, axes)
    return np.ascontiguousarray(_crop(out, size, k, op == "xcorr" or slice_pad))


def padded_size(shape, kshape, op):
    """(transform extents, inverse length of the last axis) of a field of ``shape`` - the key of a hipFFT plan pair."""
    xp, _ = pad_field(np.zeros(shape[-len(kshape):]), np.zeros(kshape), op)
    n = xp.shape
    return tuple(n), n[-1] - n[-1] % 2


# ------------------------------------------------------------------------------------------------ inputs
def field(shape, seed):
    return np.random.RandomState(seed).randn(*shape).astype(np.float32)


def mul_kernel(shape, seed=7):
    """Kernel of the multiplicative modes: randn taps."""
    return np.random.RandomState(seed + 1000 * len(shape) + sum(s * 10 ** i for i, s in enumerate(shape))).randn(*shape).astype(np.float32)


def inv_kernel(shape, seed=11):
    """Kernel of the inverting modes: the centre tap is 2, the other taps have absolute values that sum to at most 1, so
    |K^| >= 2 - 1 on every bin whatever the transform size, and |K^ + eps| >= 2 - 1 - 0.3 = 0.7 for eps = 0.3."""
    r = np.random.RandomState(seed + 1000 * len(shape) + sum(s * 10 ** i for i, s in enumerate(shape))).randn(*shape)
    centre = tuple(s // 2 for s in shape)
    r[centre] = 0.0
    total = np.abs(r).sum()
    if total > 0:
        r *= 0.99 / total                       # 1 % under the bound: the fp32 rounding of the taps cannot cross it
    r[centre] = 2.0
    return r.astype(np.float32)


# ------------------------------------------------------------------------------------------------ cases
# An op is ("xcorr",) | ("xinv",) | ("diff", correlation, slice_pad) | ("integ", correlation, slice_pad).
XCORR, XINV = ("xcorr",), ("xinv",)
DIFFS = tuple(("diff", c, s) for c in (False, True) for s in (True, False))
INTEGS = tuple(("integ", c, s) for c in (False, True) for s in (True, False))
ALL_OPS = (XCORR, XINV) + DIFFS + INTEGS


def is_inverting(op):
    return op[0] in ("xinv", "integ")


def op_args(op):
    """(reference's op name, keyword arguments of ``reference``)."""
    if op[0] == "xcorr":
        return "xcorr", {}
    if op[0] == "xinv":
        return "xcorr", {"invert": True}
    return op[0], {"correlation": op[1], "slice_pad": op[2]}


class Case:
    """One field shape with one kernel extent: ``shape`` = [B, *spatial] or [B, C, *spatial] (``keep_channel``)."""

    def __init__(self, name, shape, kshape, ops, keep_channel=False, seed=0):
        self.name, self.shape, self.kshape, self.ops, self.keep_channel, self.seed = name, tuple(shape), tuple(kshape), ops, \
            keep_channel, seed

    def x(self):
        return field(self.shape, 100 + self.seed)

    def kernel(self, op):
        return inv_kernel(self.kshape) if is_inverting(op) else mul_kernel(self.kshape)

    def ref(self, op, x=None):
        name, kw = op_args(op)
        return reference(self.x() if x is None else x, self.kernel(op), name, **kw)

    def __repr__(self):
        return self.name


# every mode on a 3-D field (even and odd padded last axis), a 2-D field and a [B,C,X,Y] field with its channels kept
MODES = [Case("3d-even", (2, 5, 6, 8), (3, 3, 3), ALL_OPS), Case("3d-odd", (2, 5, 6, 9), (3, 3, 3), ALL_OPS),
         Case("2d", (3, 6, 9), (3, 3), ALL_OPS), Case("bcxy", (2, 3, 6, 8), (3, 3), ALL_OPS, keep_channel=True)]

# padded last axes 2 .. 514: m = n2/2 + 1 = 2, 2, 128, 129, 129, 256, 257, 257, 258 bins (256 per x-block of the multiply)
_LAST = (("diff", False, False), ("diff", True, True), ("integ", False, False), ("integ", True, True))
SEAMS = [Case(f"last{L}", (2, 3, 3, L), (3, 1, 1), _LAST, seed=L) for L in (2, 3)] + \
        [Case(f"last{L}", (2, 2, 3, L - 2), (1, 1, 3), _LAST, seed=L) for L in (255, 256, 257, 511, 512, 513, 514)] + \
        [Case(f"xcorr-last{L}", (2, 2, 3, L), (1, 1, 3), (XCORR, XINV), seed=L) for L in (253, 254, 510, 512)]

# batch * n0 > 65535 planes in the embed and in the crop (the grid's z extent is capped at 65535)
PLANES = [Case("planes-2d", (65600, 2, 4), (3, 3), (XCORR, ("diff", False, False), ("integ", True, False))),
          Case("planes-3d", (9400, 5, 2, 4), (3, 3, 3), (XCORR, ("diff", True, False), ("integ", False, False)))]

_EXT = (XCORR, XINV, ("diff", False, True), ("diff", True, False), ("integ", False, False), ("integ", True, True))
EXTENTS = [Case("k" + "x".join(map(str, ks)), (2, 6, 7, 8), ks, _EXT, seed=sum(ks))
           for ks in ((1, 1, 3), (3, 1, 1), (3, 5, 7), (7, 7, 7), (2, 2, 2), (4, 4, 4))] + \
          [Case("k" + "x".join(map(str, ks)), (3, 6, 9), ks, _EXT, seed=sum(ks)) for ks in ((7, 7), (1, 3))]

# the layout / chunk / isolation / stream / repeatability tests run on these (sizes the tables above already have)
LAYOUT = Case("layout-3d", (2, 5, 6, 8), (3, 3, 3), (XCORR, ("diff", False, False), ("integ", True, True)), seed=41)
LAYOUT_C = Case("layout-bcxy", (2, 3, 6, 8), (3, 3), (XCORR, ("diff", True, False)), keep_channel=True, seed=42)
BATCH7 = Case("batch7", (7, 5, 6, 8), (3, 3, 3), (XCORR, ("diff", False, False), ("integ", False, True)), seed=43)

# seventeen distinct padded sizes (all of them sizes of the tables above): a (3,1,1) / (3,1) kernel pads nothing in
# differentiate, so the field's extents are the transform's
CACHE = [Case(f"cache{i}", (2,) + n, (3, 1, 1) if len(n) == 3 else (3, 1), (("diff", False, False),), seed=60 + i)
         for i, n in enumerate([(7, 8, 10), (7, 8, 11), (7, 8, 12), (6, 7, 10), (8, 9, 10), (8, 7, 8), (6, 7, 8), (8, 11, 14),
                                (12, 13, 14), (10, 11, 12), (7, 4, 6), (8, 11), (8, 12), (8, 10), (12, 16), (12, 15), (6, 12)])]

ALL_CASES = MODES + SEAMS + PLANES + EXTENTS + [LAYOUT, LAYOUT_C, BATCH7] + CACHE


def plan_sizes(cases=None):
    """The distinct (nd, extents, inverse last length) of the hipFFT plans the cases need."""
    out = set()
    for c in ALL_CASES if cases is None else cases:
        for op in c.ops:
            n, inv = padded_size(c.shape, c.kshape, op_args(op)[0])
            out.add((len(c.kshape), n, inv))
    return out
