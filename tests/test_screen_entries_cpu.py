"""CPU tests of the return codes of the sixteen entries of libcp_pre_screen.so, libcp_pre_screenflat.so and
libcp_pre_screencells.so, whose host side is csrc/screen_entries.h (the paired and JOREK libraries on the same bodies have
theirs in tests/test_screenpair_cpu.py and tests/test_screenjorek_cpu.py):
  * one fault for each check of an entry, in the order the checks are made;
  * pairs of simultaneous faults with different codes, which fix that order: kernel and tap-list nulls, then ``eq``, then
    everything the prepare step checks in its own order, then kernels off the star, then a tap structure that is not built;
  * every (kind, tap structure) that is not built, with well-formed arguments.
Every call returns before a launch: the addresses are not mapped and nothing is dereferenced on the host, so a refusal
that reached a launch could not return its code here.  The expected codes were recorded from the build of the commit before
the entries moved onto the shared bodies."""
import ctypes

import pytest

from cp_pre_amd import _lib

NULL, SHAPE, UNSUPPORTED, RANGE = _lib.PRE_E_NULL, _lib.PRE_E_SHAPE, _lib.PRE_E_UNSUPPORTED, _lib.PRE_E_RANGE
KINDS = ("stencil3d", "linear2", "ns_momentum", "mhd")
NVIEWS = {"stencil3d": 1, "linear2": 2, "ns_momentum": 3, "mhd": 6}
NKERNELS = {"linear2": 2, "ns_momentum": 4, "mhd": 3}
# (library, flat?) -> loader, prefix of the entry names, set descriptor
TARGETS = {
    ("screen", False): (_lib.load_screen, "pre_screen_", _lib.PreScreen),
    ("screenflat", True): (_lib.load_screenflat, "pre_screenflat_", _lib.PreScreenFlat),
    ("screencells", False): (_lib.load_screencells, "pre_screencells_", _lib.PreScreenCells),
    ("screencells", True): (_lib.load_screencells, "pre_screencells_flat_", _lib.PreScreenCellsFlat),
}
ENTRIES = [(lib, flat, kind) for (lib, flat) in TARGETS for kind in KINDS]
# the tap structures that are not built, from the entries as they were: (library, flat?) -> the eq of pre_*_mhd_f32 whose
# general star is declined; every other (kind, tap structure) launches
UNBUILT = {("screen", False): (2,), ("screenflat", True): (1,), ("screencells", False): (1, 2), ("screencells", True): (1, 2)}
F0, Q0, S0, C0, M0 = 0x10000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000      # (not mapped)

STAR = [0.0] * 27
STAR[13] = 1.0
BOX = list(STAR)
BOX[0] = 0.5                                            # weight off the 7-point star
GEN = [0.0] * 27
GEN[4] = GEN[10] = GEN[12] = 1.0                        # weight on all three axes: the general star


class Call:
    """One entry with well-formed arguments (which would launch); a test changes what it faults and calls ``rc()``."""

    def __init__(self, lib, flat, kind):
        load, prefix, self.desc_t = TARGETS[(lib, flat)]
        self.fn = getattr(load(), prefix + kind + "_f32")
        self.cells, self.flat, self.kind = lib == "screencells", flat, kind
        self.shape = [2, 6, 5, 12]                      # B, T, X, Y
        self.view_flat = flat                           # the layout of the field views
        self.null_view = None
        self.kernels = [list(STAR) for _ in range(NKERNELS.get(kind, 0))]
        self.taps, self.ntaps = ([1.0], [0, 0, 0]), 1   # (stencil3d)
        self.eq, self.flags, self.desc = 0, 0, {}
        self.no_desc = False

    def view(self, i):
        B, T, X, Y = self.shape
        strides = (T * X * Y, 1, Y * T, T) if self.view_flat else (T * X * Y, X * Y, Y, 1)
        return _lib.PreField(None if i == self.null_view else F0 + i * 0x01000000, *strides)

    def descriptor(self):
        B, T, X, Y = self.shape
        d = dict(nk=3, modulation=None, mT=0, mX=0, ct=1, cx=1, cy=1, score=S0, count=C0, count_ld=B)
        if self.flat:
            d.update(mY=0)
        if self.cells:
            d.update(levels=Q0, lK=T * X * Y, lT=X * Y, lX=Y)
            if self.flat:
                d.update(lT=1, lX=Y * T, lY=T)
        else:
            d.update(q=Q0)
        d.update(self.desc)
        return self.desc_t(**d)

    def rc(self):
        n = NVIEWS[self.kind]
        views = (_lib.PreField * n)(*[self.view(i) for i in range(n)])
        ks = [None if k is None else _lib.farr(k) for k in self.kernels]
        if self.kind == "stencil3d":
            w, off = self.taps
            head = [ctypes.byref(views[0]), None if w is None else _lib.farr(w), None if off is None else _lib.iarr32(off), self.ntaps]
        elif self.kind == "linear2":
            head = [ctypes.byref(views[0]), ctypes.byref(views[1]), *ks, 1.5]
        elif self.kind == "ns_momentum":
            head = [ctypes.byref(views[i]) for i in range(3)] + ks + [0.01, 0.02, 0.03, 0.001]
        else:
            head = [self.eq, views, *ks, 5 / 3]
        d = self.descriptor()
        return self.fn(*head, None if self.no_desc else ctypes.byref(d), *self.shape, self.flags, None)

    # ---- faults
    def null_kernel(self):
        if self.kind == "stencil3d":
            self.taps = (None, self.taps[1])
        else:
            self.kernels[-1] = None

    def off_star(self):
        if self.kind == "stencil3d":
            self.taps, self.ntaps = ([1.0, 0.5], [0, 0, 0, 0, 1, 1]), 2
        else:
            self.kernels[1] = list(BOX)

    def general(self):
        """a star with weight on all three axes (stencil3d and linear2 have one tap structure: any star)"""
        if self.kind == "stencil3d":
            self.taps, self.ntaps = ([1.0, 1.0, 1.0], [-1, 0, 0, 0, -1, 0, 0, 0, -1]), 3
        else:
            self.kernels[1] = list(GEN)

    def ragged(self):
        """rows that are not whole quads: Y % 4 != 0 on Ny-fastest fields, (Y * T) % 4 != 0 on Nt-fastest ones"""
        self.shape[1:] = [6, 5, 10] if not self.flat else [6, 4, 5]


def entry_id(e):
    return "%s-%s-%s" % (e[0], "flat" if e[1] else "ny", e[2])


def single_faults(c):
    """(name, fault, code) in the order of the checks; ``fault`` changes a fresh Call"""
    B, T, X, Y = c.shape
    out = [("null_kernel", Call.null_kernel, NULL)]
    if c.kind == "stencil3d":
        out += [("negative_ntaps", lambda k: setattr(k, "ntaps", -1), NULL),
                ("null_offsets", lambda k: setattr(k, "taps", (k.taps[0], None)), NULL),
                ("too_many_taps", lambda k: (setattr(k, "taps", tuple(a and a * 344 for a in k.taps)), setattr(k, "ntaps", 344)), SHAPE)]
    if c.kind == "mhd":
        out += [("eq_below", lambda k: setattr(k, "eq", -1), RANGE), ("eq_above", lambda k: setattr(k, "eq", 4), RANGE)]
    levels = "levels" if c.cells else "q"
    out += [("null_descriptor", lambda k: setattr(k, "no_desc", True), NULL),
            ("null_levels", lambda k: k.desc.update({levels: None}), NULL),
            ("null_score", lambda k: k.desc.update(score=None), NULL),
            ("null_count", lambda k: k.desc.update(count=None), NULL),
            ("empty_batch", lambda k: k.shape.__setitem__(0, 0), NULL),
            # (eq 0 of the MHD entries reads views 0-2, eq 3 views 1, 2, 4, 5, eq 1 and 2 all six)
            ("null_view", lambda k: setattr(k, "null_view", 2 if k.kind == "mhd" else NVIEWS[k.kind] - 1), NULL)]
    if c.kind == "mhd":
        out += [("null_view_of_induction", lambda k: (setattr(k, "eq", 3), setattr(k, "null_view", 5)), NULL),
                ("null_view_of_momentum", lambda k: (setattr(k, "eq", 1), setattr(k, "null_view", 3)), NULL)]
    out += [
            ("no_levels", lambda k: k.desc.update(nk=0), RANGE),
            ("too_many_levels", lambda k: k.desc.update(nk=17), RANGE),
            ("negative_crop", lambda k: k.desc.update(cx=-1), RANGE),
            ("short_count_ld", lambda k: k.desc.update(count_ld=B - 1), NULL),
            ("counts_past_32_bits", lambda k: k.shape.__setitem__(slice(1, 4), [2048, 2048, 1024]), SHAPE),
            ("flag_abs", lambda k: setattr(k, "flags", _lib.PRE_FLAG_ABS), UNSUPPORTED),
            ("other_layout", lambda k: setattr(k, "view_flat", not k.flat), UNSUPPORTED),
            ("ragged_rows", Call.ragged, UNSUPPORTED)]
    if c.flat:
        out += [("flag_halo_x", lambda k: setattr(k, "flags", _lib.PRE_FLAG_HALO_X), UNSUPPORTED),
                ("long_nt", lambda k: k.shape.__setitem__(1, 96), UNSUPPORTED),
                ("one_row", lambda k: k.shape.__setitem__(3, 1), UNSUPPORTED),
                ("modulation_layout", lambda k: k.desc.update(modulation=M0, mT=2, mX=Y * T, mY=T), UNSUPPORTED),
                ("plane_past_32_bit_offsets", lambda k: k.shape.__setitem__(slice(1, 4), [16, 1, 1 << 26]), SHAPE)]
    if c.cells:
        out += [("negative_level_stride", lambda k: k.desc.update(lK=-1), SHAPE)]
        if c.flat:
            out += [("level_layout", lambda k: k.desc.update(lT=2), UNSUPPORTED),
                    ("negative_level_row_stride", lambda k: k.desc.update(lX=-1), SHAPE)]
        else:
            out += [("negative_level_plane_stride", lambda k: k.desc.update(lT=-1), SHAPE)]
    out += [("off_star", Call.off_star, UNSUPPORTED)]
    if c.kind == "stencil3d":
        out += [("far_tap", lambda k: (setattr(k, "taps", ([1.0, 0.5], [0, 0, 0, 4, 0, 0])), setattr(k, "ntaps", 2)), SHAPE)]
    return out


@pytest.mark.parametrize("entry", ENTRIES, ids=entry_id)
def test_screen_entry_refuses_each_single_fault_with_its_code(entry):
    got, want = {}, {}
    for name, fault, code in single_faults(Call(*entry)):
        c = Call(*entry)
        fault(c)
        got[name], want[name] = c.rc(), code
    assert got == want


@pytest.mark.parametrize("entry", ENTRIES, ids=entry_id)
def test_screen_entry_checks_in_the_order_of_the_precedence_pairs(entry):
    """two faults with different codes in one call: the code is that of the check made first"""
    faults = {name: (fault, code) for name, fault, code in single_faults(Call(*entry))}
    pairs = [("null_descriptor", "off_star"), ("too_many_levels", "off_star"), ("too_many_levels", "short_count_ld"),
             ("short_count_ld", "counts_past_32_bits"), ("counts_past_32_bits", "flag_abs"), ("null_kernel", "too_many_levels")]
    if entry[2] == "mhd":
        pairs += [("null_kernel", "eq_above"), ("eq_above", "null_descriptor"), ("eq_below", "null_view"), ("eq_above", "off_star")]
    if entry[2] == "stencil3d":
        pairs += [("null_kernel", "too_many_taps"), ("too_many_taps", "null_descriptor"), ("ragged_rows", "far_tap"),
                  ("too_many_levels", "far_tap")]
    if entry[1]:
        pairs += [("modulation_layout", "plane_past_32_bit_offsets")]
    if entry[0] == "screencells":
        pairs += [("flag_abs", "negative_level_stride"), ("negative_level_stride", "off_star")]
        if entry[1]:
            pairs += [("level_layout", "negative_level_row_stride"), ("plane_past_32_bit_offsets", "level_layout")]
    got, want = {}, {}
    for first, second in pairs:
        assert faults[first][1] != faults[second][1], (first, second)
        c = Call(*entry)
        faults[first][0](c)
        faults[second][0](c)
        got[first, second], want[first, second] = c.rc(), faults[first][1]
    # rows that are not whole quads decline before the tap structure is looked at, whatever it is (the same code for an
    # unbuilt one; a built one would have launched)
    c = Call(*entry)
    c.ragged()
    c.general()
    got["ragged_rows", "general"], want["ragged_rows", "general"] = c.rc(), UNSUPPORTED
    assert got == want


@pytest.mark.parametrize("target", sorted(UNBUILT), ids=lambda t: "%s-%s" % (t[0], "flat" if t[1] else "ny"))
def test_screen_unbuilt_tap_structures_decline_with_well_formed_arguments(target):
    for eq in UNBUILT[target]:
        for k in range(3):                              # the general star in any of the three operators
            c = Call(*target, "mhd")
            c.eq = eq
            c.kernels[k] = list(GEN)
            assert c.rc() == UNSUPPORTED, (eq, k)
        # ... and not because of the kernel: a fault checked before the tap structure keeps its own code
        c = Call(*target, "mhd")
        c.eq = eq
        c.kernels[1] = list(GEN)
        c.desc.update(nk=17)
        assert c.rc() == RANGE
