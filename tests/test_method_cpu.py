"""``cp_pre_amd._method``: one resolution of a residual method behind ``losses._Spec`` and ``screen._Spec``, host only.

Every row of what the two consumers make of a method - kind, rows_kind, why, nd, chan, ops, eq, ratio, the TypeErrors -
is pinned here, and where both fuse a method they read the same channels, operators and scalars.  No library is loaded."""
import pytest
import torch

import losses_helpers as lh
import screen_helpers as sh

ROWS_WHY = "1-D family: the marched axis is the batch"
TYPE_ERROR = "residual_method must be a bound residual method of cp_pre_amd.residuals or a ConvOperator"
MHD_CHAN = {"continuity": (0, 1, 2), "momentum": tuple(range(6)), "energy": tuple(range(6)), "induction": (1, 2, 4, 5)}


def specs(method):
    from cp_pre_amd import losses, screen
    return losses._Spec(method), screen._Spec(method)


def same(ops, want):
    return isinstance(ops, tuple) and len(ops) == len(want) and all(a is b for a, b in zip(ops, want))


def check(sp, method, obj, is_op, kind, why, nd, chan, ops):
    assert sp.method is method or sp.method == method            # (a bound method is made anew at every attribute access)
    assert sp.obj is obj and sp.is_op is is_op
    assert (sp.kind, sp.why, sp.nd, sp.chan) == (kind, why, nd, chan)
    assert same(sp.ops, ops)


def test_a_conv_operator():
    from cp_pre_amd.convops_1d import ConvOperator as C1
    from cp_pre_amd.convops_2d import ConvOperator as C2
    for op in (sh.method_of("lap"), lh.Route("op3d").method):
        L, S = specs(op)
        check(L, op, op, True, "stencil3d", None, 3, None, (op,))
        check(S, op, op, True, "stencil3d", None, 3, None, (op,))
        assert S.rows_kind is None and L.scalars() == S.scalars() == ()
    op = lh.Route("op2d").method
    L, S = specs(op)
    check(L, op, op, True, "stencil2d", None, 2, None, (op,))
    check(S, op, op, True, None, ROWS_WHY, 2, None, (op,))
    assert S.rows_kind == "stencil2d" and L.scalars() == S.scalars() == ()
    for op, nd in ((C2(("x", "y"), 2, conv="spectral"), 3), (C1("x", 2, conv="spectral"), 2)):
        for sp in specs(op):                             # (ops: the operator itself, for the screens too - kernel_vjp reads ops[0])
            check(sp, op, op, True, None, "spectral operator", nd, None, (op,))
            assert sp.rows_kind is None


def test_navier_stokes():
    from cp_pre_amd import residuals as R
    for method in (sh.method_of("ns_momentum"), lh.Route("pre_ns").method):
        o = method.__self__
        for sp in specs(method):
            check(sp, method, o, False, "ns_momentum", None, 3, (0, 1, 2), (o.D_t, o.D_x, o.D_y, o.D_xx_yy))
            assert sp.rows_kind is None and sp.scalars() == (float(o.dt), float(o.dx), float(o.dy), float(o.nu))
    method = sh.method_of("ns_continuity")
    o = method.__self__
    L, S = specs(method)
    for sp in (L, S):
        check(sp, method, o, False, "linear2", None, 3, (0, 1), (o.D_x, o.D_y))
        assert sp.scalars() == (sh.NS_DX / sh.NS_DY,)
    assert S.ratio == sh.NS_DX / sh.NS_DY
    ns = R.NavierStokes(0.1, 0.1, 0.1)
    from cp_pre_amd import losses, screen
    for cls in (losses._Spec, screen._Spec):
        for bad in (ns.periodic_bc_residual, torch.relu, lambda v: v, "residual", None):
            with pytest.raises(TypeError) as e:
                cls(bad)
            assert str(e.value) == TYPE_ERROR


def test_mhd():
    from cp_pre_amd import losses, screen
    from cp_pre_amd import residuals as R
    method = sh.method_of("mhd_gauss")
    o = method.__self__
    check(losses._Spec(method), method, o, False, None, "no fused VJP for MHD", 3, (), ())
    S = screen._Spec(method)
    check(S, method, o, False, "linear2", None, 3, (4, 5), (o.D_x, o.D_y))
    assert S.ratio == 1.0 and S.scalars() == (1.0,) and S.rows_kind is None
    pre = R.PRE_MHD(0.1, 0.1, 0.1)
    for eq, name in enumerate(("continuity", "momentum", "energy", "induction")):
        for method, cls_name in [(sh.method_of("mhd_" + name), "MHD")] + ([(pre.residual, "PRE_MHD")] if name == "induction" else []):
            o = method.__self__
            check(losses._Spec(method), method, o, False, None, "no fused VJP for " + cls_name, 3, (), ())
            S = screen._Spec(method)
            check(S, method, o, False, "mhd_" + name, None, 3, MHD_CHAN[name], (o.D_t, o.D_x, o.D_y))
            assert S.eq == eq and S.scalars() == (float(o.gamma),) and S.rows_kind is None
    # any other bound method of an MHD: the losses name the fallback, the screen has no such method
    other = R.MHD()._want_fused
    check(losses._Spec(other), other, other.__self__, False, None, "no fused VJP for MHD", 3, (), ())
    with pytest.raises(TypeError) as e:
        screen._Spec(other)
    assert str(e.value) == TYPE_ERROR


def test_wave_advection_burgers():
    method = sh.method_of("wave")
    o = method.__self__
    for sp in specs(method):
        check(sp, method, o, False, "stencil3d", None, 3, None, (o.D,))
        assert sp.rows_kind is None and sp.scalars() == ()
    method = lh.Route("advection").method
    o = method.__self__
    L, S = specs(method)
    check(L, method, o, False, "stencil2d", None, 2, None, (o.D,))
    check(S, method, o, False, None, ROWS_WHY, 2, None, (o.D,))
    assert S.rows_kind == "stencil2d" and L.scalars() == S.scalars() == ()
    method = lh.Route("burgers").method
    o = method.__self__
    L, S = specs(method)
    check(L, method, o, False, "burgers", None, 2, None, (o.D_t, o.D_x, o.D_xx))
    check(S, method, o, False, None, ROWS_WHY, 2, None, (o.D_t, o.D_x, o.D_xx))
    assert S.rows_kind == "burgers"
    # 2 dt / dx in the arithmetic of Burgers.residual (the object's own dt and dx), then widened
    assert L.scalars() == S.scalars() == (float(o.dx), float(o.dt), float(o.nu), float(2 * o.dt / o.dx))


def test_jorek():
    from cp_pre_amd import losses, screen
    from cp_pre_amd import residuals as R
    jo = R.JOREK(torch.linspace(1.0, 2.0, 8))
    for method in (jo.residual_continuity, jo.residual_temperature):
        check(losses._Spec(method), method, jo, False, None, "no fused VJP for JOREK", 3, (), ())
        S = screen._Spec(method)
        check(S, method, jo, False, None, "no fused screen for JOREK", 3, (), ())
        assert S.rows_kind is None
    check(losses._Spec(jo._ops), jo._ops, jo, False, None, "no fused VJP for JOREK", 3, (), ())
    with pytest.raises(TypeError) as e:
        screen._Spec(jo._ops)
    assert str(e.value) == TYPE_ERROR


def test_where_both_fuse_they_read_the_same():
    """every method with a fused VJP and a fused screen (of either family): nd, chan, ops and the scalar tail agree"""
    methods = [sh.method_of(k) for k in ("lap", "wave", "ns_momentum", "ns_continuity")] + \
              [lh.Route(k).method for k in ("op3d", "op2d", "pre_ns", "advection", "burgers")]
    for method in methods:
        L, S = specs(method)
        assert L.kind is not None and L.kind == (S.kind or S.rows_kind)
        assert (L.nd, L.chan) == (S.nd, S.chan) and same(L.ops, S.ops) and L.scalars() == S.scalars()


def test_field_shape_and_fields():
    """the channel requirement is max(chan) + 1 (0 for ()), and [BS,1,Nt,Nx] is the screen's alone"""
    from cp_pre_amd import losses, screen
    m = lambda *s: torch.empty(s, device="meta")                                            # noqa: E731
    for sp in specs(sh.method_of("ns_continuity")):
        assert sp.field_shape(m(2, 2, 6, 8, 12)) == (2, 6, 8, 12) and len(sp.fields(m(2, 4, 6, 8, 12))) == 2
        with pytest.raises(ValueError, match=r"F>=2"):
            sp.field_shape(m(2, 1, 6, 8, 12))
    S = screen._Spec(sh.method_of("mhd_gauss"))
    assert S.field_shape(m(2, 6, 6, 8, 12)) == (2, 6, 8, 12) and [f.shape for f in S.fields(m(2, 6, 6, 8, 12))] == [(2, 6, 8, 12)] * 2
    with pytest.raises(ValueError, match=r"F>=6"):
        S.field_shape(m(2, 5, 6, 8, 12))
    assert losses._Spec(sh.method_of("mhd_gauss")).field_shape(m(2, 0, 6, 8, 12)) == (2, 6, 8, 12)     # (F>=0: not checked here)
    for sp in specs(sh.method_of("wave")):
        assert sp.field_shape(m(2, 6, 8, 12)) == sp.field_shape(m(2, 1, 6, 8, 12)) == (2, 6, 8, 12)
        assert sp.fields(m(2, 1, 6, 8, 12))[0].shape == (2, 6, 8, 12)
    L, S = specs(lh.Route("burgers").method)
    assert L.field_shape(m(3, 8, 12)) == S.field_shape(m(3, 8, 12)) == S.field_shape(m(3, 1, 8, 12)) == (3, 8, 12)
    with pytest.raises(ValueError, match="expected a 3-D field"):
        L.field_shape(m(3, 1, 8, 12))
    from cp_pre_amd import residuals as R
    jo = specs(R.JOREK(torch.linspace(1.0, 2.0, 8)).residual_continuity)
    assert all(sp.field_shape(m(2, 3, 8, 8, 5)) == (2, 5, 8, 8) for sp in jo)
