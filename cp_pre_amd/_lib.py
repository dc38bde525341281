"""ctypes binding of ``libcp_pre_hip.so`` (C ABI: ``include/cp_pre_hip.h``).

The library is the product; this module only marshals device pointers, sizes and the
current HIP stream.  There is no CPU fallback: if the shared object is missing, or no
MI355X is visible when a compute entry point is called, the call raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_double, c_float, c_int, c_int32, c_int64, c_void_p

import torch  # imported first on purpose: the .so must bind to the HIP runtime torch already loaded

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libcp_pre_hip.so")

PRE_ABI_VERSION = 8            # include/cp_pre_hip.h: the version SIGNATURES below was written for
PRE_OK, PRE_E_NULL, PRE_E_SHAPE, PRE_E_UNSUPPORTED, PRE_E_RANGE = 0, -1, -2, -3, -4
PRE_FLAG_ABS = 1
PRE_FLAG_INTERIOR_T = 2
PRE_FLAG_OUT_INTERIOR_T = 4
PRE_FLAG_HALO_X = 8
_ERR = {PRE_E_NULL: "null pointer / bad size", PRE_E_SHAPE: "unsupported shape",
        PRE_E_UNSUPPORTED: "operator kernels not star-shaped or layout not streamable",
        PRE_E_RANGE: "rank / crop out of range"}


class PreField(ctypes.Structure):
    """``pre_field_t`` / ``pre_out_t`` (same layout): a strided [B,T,X,Y] view (element strides)."""
    _fields_ = [("ptr", c_void_p), ("sB", c_int64), ("sT", c_int64), ("sX", c_int64), ("sY", c_int64)]


class PreBC(ctypes.Structure):
    """``pre_bc_t``: boundary mode / value for left, right (columns) and top, bottom (rows)."""
    _fields_ = [("mode", c_int * 4), ("value", c_float * 4)]


_fp, _fld = c_void_p, POINTER(PreField)
# name -> argtypes; every symbol include/cp_pre_hip.h declares
SIGNATURES = {
    "pre_abi_version": [],
    "pre_stencil3d_f32": [_fld, _fld, POINTER(c_float), POINTER(c_int32), c_int, c_int64, c_int64, c_int64, c_int64, c_int, c_void_p],
    "pre_stencil2d_f32": [_fp, POINTER(c_int64), _fp, POINTER(c_int64), POINTER(c_float), POINTER(c_int32), c_int, c_int64, c_int64, c_int64, c_int, c_void_p],
    "pre_stencil3d_wgrad_f32": [_fld, _fld, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int64, _fp, c_void_p],
    "pre_residual_ns_momentum_f32": [_fld, _fld, _fld, _fld] + [POINTER(c_float)] * 4 + [c_float] * 4 + [c_int64] * 4 + [c_int, c_void_p],
    "pre_moments_segmax_f64": [_fp, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_int, _fp, _fp, _fp, c_void_p],
    "pre_segmin_mod_f32": [_fp, c_int64, c_int64, c_int64, c_int, c_int, _fp, c_void_p],
    "pre_joint_score_pruned_f32": [_fp, c_int64, _fp, _fp, _fp, c_int64, c_int64, c_int64, c_int64, c_int, c_int, _fp, _fp, _fp, c_void_p],
    "pre_joint_score_flagged_f32": [_fp, _fp, _fp, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, _fp, _fp, c_void_p],
    "pre_residual_linear2_f32": [_fld, _fld, _fld, POINTER(c_float), POINTER(c_float), c_float] + [c_int64] * 4 + [c_int, c_void_p],
    "pre_residual_burgers_f32": [_fp, POINTER(c_int64), _fp, POINTER(c_int64)] + [POINTER(c_float)] * 3 + [c_float] * 4 + [c_int64] * 3 + [c_int, c_void_p],
    "pre_residual_mhd_f32": [c_int, POINTER(PreField), _fld] + [POINTER(c_float)] * 3 + [c_double] + [c_int64] * 4 + [c_int, c_void_p],
    "pre_residual_jorek_f32": [c_int, POINTER(PreField), _fld, _fld] + [POINTER(c_float)] * 6 + [c_int64] * 4 + [c_int, c_void_p],
    "pre_spatial2d_bc_f32": [_fp, POINTER(c_int64), _fp, POINTER(c_int64), POINTER(c_float), POINTER(PreBC), c_int64, c_int64, c_int64, c_int, c_void_p],
    "pre_spatial2d_linear2_bc_f32": [_fp, POINTER(c_int64), _fp, POINTER(c_int64), _fp, POINTER(c_int64), POINTER(c_float), POINTER(c_float),
                                     c_float, POINTER(PreBC), c_int64, c_int64, c_int64, c_int, c_void_p],
    "pre_edge_residual_f32": [_fld, c_int, c_float, c_int64, c_int64, c_int64, c_int64, _fp, c_void_p],
    "pre_absdiff_f32": [_fp, _fp, _fp, c_int64, c_void_p],
    "pre_std_axis0_f32": [_fp, _fp, c_int64, c_int64, c_float, _fp, c_void_p],
    "pre_moments_axis0_f64": [_fp, _fp, c_int64, c_int64, c_int64, _fp, _fp, c_void_p],
    "pre_std_from_moments_f32": [_fp, _fp, c_int64, c_int64, c_float, _fp, c_void_p],
    "pre_joint_score_f32": [_fp, _fp, _fp, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, _fp, c_void_p],
    "pre_kth_f32": [_fp, c_int64, POINTER(c_int64), c_int, _fp, c_void_p],
    "pre_kth_axis0_f32": [_fp, c_int64, c_int64, POINTER(c_int32), c_int, _fp, c_void_p],
    "pre_kth_axis0_strided_f32": [_fp, c_int64, c_int64, c_int64, POINTER(c_int32), c_int, _fp, c_void_p],
    "pre_kth_axis0_planes_f32": [_fp, c_int64, c_int64, c_int64, c_int64, c_int64, POINTER(c_int32), c_int, _fp, c_int64, c_int64, c_void_p],
    "pre_joint_score_pruned_max_segments": [],
    "pre_cov_count_f32": [_fp, _fp, _fp, c_int64, c_int64, c_int, _fp, c_void_p],
    "pre_cov_rowcount_f32": [_fp, _fp, _fp, c_int64, c_int64, c_int, c_int, _fp, c_void_p],
    "pre_cov_joint_f32": [_fp, _fp, _fp, c_int64, c_int64, c_int, _fp, c_void_p],
}

# libcp_pre_fft.so (include/cp_pre_fft.h): the spectral family; separate because it links hipFFT
FFT_SO_PATH = os.path.join(_HERE, "libcp_pre_fft.so")
PRE_FFT_CONJ, PRE_FFT_INVERT = 1, 2
_i64p = POINTER(c_int64)
FFT_SIGNATURES = {
    "pre_fft_abi_version": [],
    "pre_fft_create": [POINTER(c_void_p), c_int, _i64p, c_int64, c_int64],
    "pre_fft_destroy": [c_void_p],
    "pre_fft_work_bytes": [c_void_p, POINTER(ctypes.c_size_t)],
    "pre_spectral_apply_f32": [c_void_p, _fp, _i64p, _i64p, _i64p, POINTER(c_float), _i64p, c_int, c_float, _fp, _i64p, _i64p,
                               c_void_p, c_void_p],
}

# libcp_pre_dist.so (include/cp_pre_dist.h): the sweeps of the sharded marginal calibration by histogram exchange
DIST_SO_PATH = os.path.join(_HERE, "libcp_pre_dist.so")
PRE_DIST_ABI_VERSION = 1
PRE_DIST_NB, PRE_DIST_PICK_CAP, PRE_DIST_MAX_SLOTS = 256, 2048, 64
_src = [_fp, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64]     # scores .. W, Co
DIST_SIGNATURES = {
    "pre_dist_abi_version": [],
    "pre_dist_window_f32": _src + [_fp, c_void_p],
    "pre_dist_hist_f32": _src + [_fp, c_int, _fp, c_void_p],
    "pre_dist_collect_f32": _src + [_fp, _fp, c_int, _fp, _fp, _fp, c_void_p],
    "pre_dist_pick_f32": [_fp, _fp, _fp, c_int64, c_int64, c_int, _fp, _fp, c_int, _fp, c_void_p],
}

# libcp_pre_cov.so (include/cp_pre_cov.h): coverage at several calibration levels in one pass over the test residual
COV_SO_PATH = os.path.join(_HERE, "libcp_pre_cov.so")
PRE_COV_ABI_VERSION = 1
PRE_COV_MAX_LEVELS = 16
_opnd = [_fp, c_int64, c_int64, c_int64]                 # ptr, sample stride, strides of the two outer cell axes
COV_SIGNATURES = {
    "pre_cov_abi_version": [],
    "pre_cov_levels_f32": _opnd + _opnd + [c_int64] * 4 + [_fp, c_int64, _fp, c_int, _fp, _fp, c_int64, c_void_p],
}

# libcp_pre_ode.so (include/cp_pre_ode.h): the ODE operators of Utils/ConvOps_0d.py and the fused ODE residuals
ODE_SO_PATH = os.path.join(_HERE, "libcp_pre_ode.so")
PRE_ODE_ABI_VERSION = 1
PRE_ODE_MAX_TAPS, PRE_ODE_MAX_TERMS, PRE_ODE_FLAG_ABS, PRE_ODE_WGRAD_BLOCKS = 7, 6, 1, 1024


class PreOdeTerm(ctypes.Structure):
    """``pre_ode_term_t``: one residual term c[t] * (K * x)[b, t] (field pointer, element strides, coefficient row, taps)."""
    _fields_ = [("x", c_void_p), ("sB", c_int64), ("sT", c_int64), ("c", c_void_p), ("k", c_int),
                ("taps", c_float * PRE_ODE_MAX_TAPS)]


ODE_SIGNATURES = {
    "pre_ode_abi_version": [],
    "pre_ode_stencil_f32": [_fp, _i64p, _fp, _i64p, c_int64, c_int64, POINTER(c_float), c_int, c_int, c_void_p],
    "pre_ode_residual_f32": [POINTER(PreOdeTerm), c_int, _fp, _i64p, c_int64, c_int64, c_int, c_void_p],
    "pre_ode_wgrad_f32": [_fp, _i64p, _fp, _i64p, c_int64, c_int64, c_int, _fp, _fp, c_void_p],
}

# libcp_pre_setprop.so (include/cp_pre_setprop.h): PRE set propagation, residual-space intervals to solution bounds
SETPROP_SO_PATH = os.path.join(_HERE, "libcp_pre_setprop.so")
PRE_SETPROP_ABI_VERSION = 1
PRE_SETPROP_MAX_TAPS, PRE_SETPROP_FLAG_F64, PRE_SETPROP_FLAG_CORRELATION = 7, 1, 2
SETPROP_SIGNATURES = {
    "pre_setprop_abi_version": [],
    "pre_setprop_bounds_f64": [_fp, _i64p, _fp, _i64p, c_int64, c_int64, _fp, _fp, _fp, _fp, c_int, c_void_p],
    "pre_setprop_recipe_f32": [_fp, _i64p, c_int64, c_int64, POINTER(c_double), c_int, _fp, _i64p, _fp, _fp, _fp, _fp, c_int,
                               c_void_p],
}

# libcp_pre_pair.so (include/cp_pre_pair.h): data-driven residual scores r(a) - r(b) of two field sets in one pass
PAIR_SO_PATH = os.path.join(_HERE, "libcp_pre_pair.so")
PRE_PAIR_ABI_VERSION = 1
PAIR_SIGNATURES = {
    "pre_pair_abi_version": [],
    "pre_pair_stencil3d_f32": [_fld, _fld, _fld, POINTER(c_float), POINTER(c_int32), c_int] + [c_int64] * 4 + [c_int, c_void_p],
    "pre_pair_stencil2d_f32": [_fp, _i64p, _fp, _i64p, _fp, _i64p, POINTER(c_float), POINTER(c_int32), c_int] + [c_int64] * 3 +
                              [c_int, c_void_p],
    "pre_pair_linear2_f32": [POINTER(PreField), POINTER(PreField), _fld, POINTER(c_float), POINTER(c_float), c_float] +
                            [c_int64] * 4 + [c_int, c_void_p],
    "pre_pair_ns_momentum_f32": [POINTER(PreField), POINTER(PreField), _fld] + [POINTER(c_float)] * 4 + [c_float] * 4 +
                                [c_int64] * 4 + [c_int, c_void_p],
    "pre_pair_mhd_continuity_f32": [POINTER(PreField), POINTER(PreField), _fld] + [POINTER(c_float)] * 3 + [c_double] +
                                   [c_int64] * 4 + [c_int, c_void_p],
    "pre_pair_burgers_f32": [_fp, _i64p, _fp, _i64p, _fp, _i64p] + [POINTER(c_float)] * 3 + [c_float] * 4 + [c_int64] * 3 +
                            [c_int, c_void_p],
}

# libcp_pre_bounds.so (include/cp_pre_bounds.h): solution bounds by sample acceptance (envelope, cellwise, row counts)
BOUNDS_SO_PATH = os.path.join(_HERE, "libcp_pre_bounds.so")
PRE_BOUNDS_ABI_VERSION = 1
PRE_BOUNDS_MAX_LEVELS = 16
BOUNDS_SIGNATURES = {
    "pre_bounds_abi_version": [],
    "pre_bounds_envelope_workspace": [c_int64] * 4 + [c_int, _i64p],
    "pre_bounds_envelope_f32": _opnd + [c_int64] * 4 + [_fp, c_int64, c_int, _fp, _fp, _fp, _fp, c_int64, c_void_p],
    "pre_bounds_cellwise_workspace": [c_int64] * 4 + [c_int, _i64p],
    "pre_bounds_cellwise_f32": _opnd + _opnd + [c_int64] * 4 + [_fp, c_int64, _fp, _fp, _fp, _fp, c_int, _fp, _fp, _fp, _fp,
                                                                 c_int64, c_void_p],
    "pre_bounds_rowcount_f32": _opnd + _opnd + [c_int64] * 4 + [_fp, c_int64, _fp, c_int, _fp, c_int64, c_void_p],
}

# libcp_pre_vjp.so (include/cp_pre_vjp.h): vector-Jacobian products of the residuals and the deterministic sum of squares
VJP_SO_PATH = os.path.join(_HERE, "libcp_pre_vjp.so")
PRE_VJP_ABI_VERSION = 1
PRE_VJP_CROP, PRE_VJP_VIEW3D, PRE_VJP_SUMSQ_WORKSPACE = 1, 2, 2048
_scale = [c_float, _fp]                                   # host_scale, dev_scale
VJP_SIGNATURES = {
    "pre_vjp_abi_version": [],
    "pre_vjp_stencil3d_f32": [_fld, _fld, POINTER(c_float), POINTER(c_int32), c_int] + _scale + [c_int64] * 4 + [c_int, c_void_p],
    "pre_vjp_stencil2d_f32": [_fp, _i64p, _fp, _i64p, POINTER(c_float), POINTER(c_int32), c_int] + _scale + [c_int64] * 3 +
                             [c_int, c_void_p],
    "pre_vjp_linear2_f32": [_fld, POINTER(PreField), POINTER(c_float), POINTER(c_float), c_float] + _scale + [c_int64] * 4 +
                           [c_int, c_void_p],
    "pre_vjp_burgers_f32": [_fp, _i64p, _fp, _i64p, _fp, _i64p] + [POINTER(c_float)] * 3 + [c_float] * 4 + _scale +
                           [c_int64] * 3 + [c_int, c_void_p],
    "pre_vjp_ns_momentum_f32": [_fld, POINTER(PreField), POINTER(PreField)] + [POINTER(c_float)] * 4 + [c_float] * 4 + _scale +
                               [c_int64] * 4 + [c_int, c_void_p],
    "pre_vjp_sumsq_f32": [_fld] + [c_int64] * 4 + [c_int, _fp, _fp, c_void_p],
}

# libcp_pre_screen.so (include/cp_pre_screen.h): per-sample score and per-level inside counts in the residual's own launch
SCREEN_SO_PATH = os.path.join(_HERE, "libcp_pre_screen.so")
PRE_SCREEN_ABI_VERSION = 1
PRE_SCREEN_MAX_LEVELS = 16


class PreScreen(ctypes.Structure):
    """``pre_screen_t``: the levels, the modulation view, the crop and the accumulators of one screening launch."""
    _fields_ = [("q", c_void_p), ("nk", c_int), ("modulation", c_void_p), ("mT", c_int64), ("mX", c_int64),
                ("ct", c_int), ("cx", c_int), ("cy", c_int), ("score", c_void_p), ("count", c_void_p), ("count_ld", c_int64)]


_scr = [POINTER(PreScreen)] + [c_int64] * 4 + [c_int, c_void_p]          # s, B, T, X, Y, flags, stream
SCREEN_SIGNATURES = {
    "pre_screen_abi_version": [],
    "pre_screen_stencil3d_f32": [_fld, POINTER(c_float), POINTER(c_int32), c_int] + _scr,
    "pre_screen_linear2_f32": [_fld, _fld, POINTER(c_float), POINTER(c_float), c_float] + _scr,
    "pre_screen_ns_momentum_f32": [_fld, _fld, _fld] + [POINTER(c_float)] * 4 + [c_float] * 4 + _scr,
    "pre_screen_mhd_f32": [c_int, POINTER(PreField)] + [POINTER(c_float)] * 3 + [c_double] + _scr,
}

# libcp_pre_screen1d.so (include/cp_pre_screen1d.h): the same screen for the 1-D residuals on [B,Nt,Nx] (PreScreen reused)
SCREEN1D_SO_PATH = os.path.join(_HERE, "libcp_pre_screen1d.so")
PRE_SCREEN1D_ABI_VERSION = 1
_scr1 = [POINTER(PreScreen)] + [c_int64] * 3 + [c_int, c_void_p]         # s, B, T, X, flags, stream
SCREEN1D_SIGNATURES = {
    "pre_screen1d_abi_version": [],
    "pre_screen1d_stencil2d_f32": [_fp, _i64p, POINTER(c_float), POINTER(c_int32), c_int] + _scr1,
    "pre_screen1d_burgers_f32": [_fp, _i64p] + [POINTER(c_float)] * 3 + [c_float] * 4 + _scr1,
}

# libcp_pre_screenflat.so (include/cp_pre_screenflat.h): the same screen for Nt-fastest views of the 2-D residuals
SCREENFLAT_SO_PATH = os.path.join(_HERE, "libcp_pre_screenflat.so")
PRE_SCREENFLAT_ABI_VERSION = 1


class PreScreenFlat(ctypes.Structure):
    """``pre_screenflat_t``: ``pre_screen_t`` with three modulation strides (the unit-stride axis is T)."""
    _fields_ = [("q", c_void_p), ("nk", c_int), ("modulation", c_void_p), ("mT", c_int64), ("mX", c_int64), ("mY", c_int64),
                ("ct", c_int), ("cx", c_int), ("cy", c_int), ("score", c_void_p), ("count", c_void_p), ("count_ld", c_int64)]


_scrf = [POINTER(PreScreenFlat)] + [c_int64] * 4 + [c_int, c_void_p]     # s, B, T, X, Y, flags, stream
SCREENFLAT_SIGNATURES = {
    "pre_screenflat_abi_version": [],
    "pre_screenflat_stencil3d_f32": [_fld, POINTER(c_float), POINTER(c_int32), c_int] + _scrf,
    "pre_screenflat_linear2_f32": [_fld, _fld, POINTER(c_float), POINTER(c_float), c_float] + _scrf,
    "pre_screenflat_ns_momentum_f32": [_fld, _fld, _fld] + [POINTER(c_float)] * 4 + [c_float] * 4 + _scrf,
    "pre_screenflat_mhd_f32": [c_int, POINTER(PreField)] + [POINTER(c_float)] * 3 + [c_double] + _scrf,
}

# libcp_pre_vjpflat.so (include/cp_pre_vjpflat.h): the vector-Jacobian products of libcp_pre_vjp.so for Nt-fastest views
VJPFLAT_SO_PATH = os.path.join(_HERE, "libcp_pre_vjpflat.so")
PRE_VJPFLAT_ABI_VERSION = 1
VJPFLAT_SIGNATURES = {
    "pre_vjpflat_abi_version": [],
    "pre_vjpflat_stencil3d_f32": VJP_SIGNATURES["pre_vjp_stencil3d_f32"],
    "pre_vjpflat_linear2_f32": VJP_SIGNATURES["pre_vjp_linear2_f32"],
    "pre_vjpflat_ns_momentum_f32": VJP_SIGNATURES["pre_vjp_ns_momentum_f32"],
}

# libcp_pre_wgrad.so (include/cp_pre_wgrad.h): the gradient of the losses with respect to a trainable operator kernel
WGRAD_SO_PATH = os.path.join(_HERE, "libcp_pre_wgrad.so")
PRE_WGRAD_ABI_VERSION = 1
PRE_WGRAD_WORKSPACE = 55296                              # doubles
WGRAD_SIGNATURES = {
    "pre_wgrad_abi_version": [],
    "pre_wgrad_stencil3d_f32": [_fld, _fld, _fld, c_int, c_int, c_int] + _scale + [c_int64] * 4 + [c_int, _fp, _fp, c_void_p],
}

# libcp_pre_cns.so (include/cp_pre_cns.h): the compressible-NS right-hand side on the 2-D spatial operators, one pass
CNS_SO_PATH = os.path.join(_HERE, "libcp_pre_cns.so")
PRE_CNS_ABI_VERSION = 1
PRE_CNS_TILE_ROWS, PRE_CNS_TILE_COLS = 16, 64


class PreCnsPlane(ctypes.Structure):
    """``pre_cns_plane_t`` / ``pre_cns_out_t`` (same layout): a [B,X,Y] plane view, unit stride along Y."""
    _fields_ = [("ptr", c_void_p), ("sB", c_int64), ("sX", c_int64)]


CNS_SIGNATURES = {
    "pre_cns_abi_version": [],
    "pre_cns_rhs_f32": [POINTER(PreCnsPlane), POINTER(PreCnsPlane)] + [POINTER(c_float)] * 5 + [POINTER(PreBC), c_float,
                        POINTER(PreCnsPlane), c_float] + [c_int64] * 3 + [c_int, c_void_p],
}

# libcp_pre_cnsvjp.so (include/cp_pre_cnsvjp.h): the vector-Jacobian product of that right-hand side, one pass (PreCnsPlane reused)
CNSVJP_SO_PATH = os.path.join(_HERE, "libcp_pre_cnsvjp.so")
PRE_CNSVJP_ABI_VERSION = 1
PRE_CNSVJP_TILE_ROWS, PRE_CNSVJP_TILE_COLS = 16, 64
CNSVJP_SIGNATURES = {
    "pre_cnsvjp_abi_version": [],
    "pre_cns_vjp_f32": [POINTER(PreCnsPlane)] * 3 + [POINTER(c_float)] * 5 + [POINTER(PreBC), c_float, POINTER(PreCnsPlane),
                        c_float] + [c_int64] * 3 + [c_int, c_void_p],
}

# libcp_pre_vjpmhd.so (include/cp_pre_vjpmhd.h): the vector-Jacobian products of the ideal-MHD residuals (the march of libcp_pre_vjp.so)
VJPMHD_SO_PATH = os.path.join(_HERE, "libcp_pre_vjpmhd.so")
PRE_VJPMHD_ABI_VERSION = 1
_mhdvjp = [_fld, POINTER(PreField), POINTER(PreField)] + [POINTER(c_float)] * 3          # g, fields, out, K_t, K_x, K_y
_mhdtail = _scale + [c_int64] * 4 + [c_int, c_void_p]
VJPMHD_SIGNATURES = {
    "pre_vjpmhd_abi_version": [],
    "pre_vjpmhd_supported": [c_int] + [POINTER(c_float)] * 3,
    "pre_vjpmhd_continuity_f32": _mhdvjp + _mhdtail,
    "pre_vjpmhd_induction_f32": _mhdvjp + _mhdtail,
    "pre_vjpmhd_momentum_f32": _mhdvjp + _mhdtail,
    "pre_vjpmhd_energy_f32": _mhdvjp + [c_double] + _mhdtail,
}

# libcp_pre_screenjorek.so (include/cp_pre_screenjorek.h): the two 2-D screens for the reduced-MHD (JOREK) residuals; the set
# descriptors are PreScreen (Ny-fastest fields) and PreScreenFlat (Nt-fastest fields)
SCREENJOREK_SO_PATH = os.path.join(_HERE, "libcp_pre_screenjorek.so")
PRE_SCREENJOREK_ABI_VERSION = 1
_jrk = [c_int, POINTER(PreField), _fld] + [POINTER(c_float)] * 5 + [POINTER(c_float)]     # eq, fields, Rb, K_t .. K_ZZ, coef
SCREENJOREK_SIGNATURES = {
    "pre_screenjorek_abi_version": [],
    "pre_screenjorek_f32": _jrk + _scr,
    "pre_screenjorek_flat_f32": _jrk + _scrf,
}

# libcp_pre_screenpair.so (include/cp_pre_screenpair.h): the two 2-D screens for the data-driven scores r(a) - r(b): each entry
# takes its single-set twin's arguments with the two field sets in place of the twin's views (PreScreen / PreScreenFlat reused)
SCREENPAIR_SO_PATH = os.path.join(_HERE, "libcp_pre_screenpair.so")
PRE_SCREENPAIR_ABI_VERSION = 1
_arr2 = [POINTER(PreField)] * 2                                         # the two sets: pre_field_t[F] each
SCREENPAIR_SIGNATURES = {"pre_screenpair_abi_version": []}
for _form, _tail in (("", _scr), ("flat_", _scrf)):
    SCREENPAIR_SIGNATURES.update({
        "pre_screenpair_%sstencil3d_f32" % _form: [_fld, _fld, POINTER(c_float), POINTER(c_int32), c_int] + _tail,
        "pre_screenpair_%slinear2_f32" % _form: _arr2 + [POINTER(c_float), POINTER(c_float), c_float] + _tail,
        "pre_screenpair_%sns_momentum_f32" % _form: _arr2 + [POINTER(c_float)] * 4 + [c_float] * 4 + _tail,
        "pre_screenpair_%smhd_continuity_f32" % _form: _arr2 + [POINTER(c_float)] * 3 + [c_double] + _tail,
    })

# libcp_pre_screencells.so (include/cp_pre_screencells.h): the two 2-D screens against per-cell sets: each entry takes its
# joint twin's arguments with nk level fields in place of the nk levels
SCREENCELLS_SO_PATH = os.path.join(_HERE, "libcp_pre_screencells.so")
PRE_SCREENCELLS_ABI_VERSION = 1


class PreScreenCells(ctypes.Structure):
    """``pre_screencells_t``: ``pre_screen_t`` with nk level fields (level, plane and row strides) in place of ``q``."""
    _fields_ = [("levels", c_void_p), ("nk", c_int), ("lK", c_int64), ("lT", c_int64), ("lX", c_int64),
                ("modulation", c_void_p), ("mT", c_int64), ("mX", c_int64), ("ct", c_int), ("cx", c_int), ("cy", c_int),
                ("score", c_void_p), ("count", c_void_p), ("count_ld", c_int64)]


class PreScreenCellsFlat(ctypes.Structure):
    """``pre_screencellsflat_t``: ``pre_screenflat_t`` with nk level fields (level stride, then the three logical strides)."""
    _fields_ = [("levels", c_void_p), ("nk", c_int), ("lK", c_int64), ("lT", c_int64), ("lX", c_int64), ("lY", c_int64),
                ("modulation", c_void_p), ("mT", c_int64), ("mX", c_int64), ("mY", c_int64), ("ct", c_int), ("cx", c_int),
                ("cy", c_int), ("score", c_void_p), ("count", c_void_p), ("count_ld", c_int64)]


SCREENCELLS_SIGNATURES = {"pre_screencells_abi_version": [], "pre_screencells_sample_group": []}
for _form, _st in (("", PreScreenCells), ("flat_", PreScreenCellsFlat)):
    _tail = [POINTER(_st)] + [c_int64] * 4 + [c_int, c_void_p]            # s, B, T, X, Y, flags, stream
    SCREENCELLS_SIGNATURES.update({
        "pre_screencells_%sstencil3d_f32" % _form: [_fld, POINTER(c_float), POINTER(c_int32), c_int] + _tail,
        "pre_screencells_%slinear2_f32" % _form: [_fld, _fld, POINTER(c_float), POINTER(c_float), c_float] + _tail,
        "pre_screencells_%sns_momentum_f32" % _form: [_fld, _fld, _fld] + [POINTER(c_float)] * 4 + [c_float] * 4 + _tail,
        "pre_screencells_%smhd_f32" % _form: [c_int, POINTER(PreField)] + [POINTER(c_float)] * 3 + [c_double] + _tail,
    })

# libcp_pre_screen1dpair.so (include/cp_pre_screen1dpair.h): the 1-D screen for the data-driven scores r(a) - r(b): each entry
# takes its single-set twin's arguments with the two field sets (pointer, strides each) in place of the twin's field
SCREEN1DPAIR_SO_PATH = os.path.join(_HERE, "libcp_pre_screen1dpair.so")
PRE_SCREEN1DPAIR_ABI_VERSION = 1
_sets1 = [_fp, _i64p, _fp, _i64p]                                       # a, strides_a, b, strides_b
SCREEN1DPAIR_SIGNATURES = {
    "pre_screen1dpair_abi_version": [],
    "pre_screen1dpair_stencil2d_f32": _sets1 + SCREEN1D_SIGNATURES["pre_screen1d_stencil2d_f32"][2:],
    "pre_screen1dpair_burgers_f32": _sets1 + SCREEN1D_SIGNATURES["pre_screen1d_burgers_f32"][2:],
}

# libcp_pre_screen1dcells.so (include/cp_pre_screen1dcells.h): the 1-D screens (one field set, and the pair a / b) against
# per-cell sets: each entry takes its joint twin's arguments with nk level fields in place of the nk levels
SCREEN1DCELLS_SO_PATH = os.path.join(_HERE, "libcp_pre_screen1dcells.so")
PRE_SCREEN1DCELLS_ABI_VERSION = 1


class PreScreen1dCells(ctypes.Structure):
    """``pre_screen1dcells_t``: ``pre_screen_t`` as the 1-D screens read it, with nk level fields [Nt,Nx] (level, Nt and Nx
    strides) in place of ``q``."""
    _fields_ = [("levels", c_void_p), ("nk", c_int), ("lK", c_int64), ("lT", c_int64), ("lX", c_int64),
                ("modulation", c_void_p), ("mT", c_int64), ("mX", c_int64), ("ct", c_int), ("cx", c_int),
                ("score", c_void_p), ("count", c_void_p), ("count_ld", c_int64)]


_scr1c = [POINTER(PreScreen1dCells)] + _scr1[1:]                        # s, B, T, X, flags, stream
SCREEN1DCELLS_SIGNATURES = {
    "pre_screen1dcells_abi_version": [],
    "pre_screen1dcells_sample_group": [],
    "pre_screen1dcells_stencil2d_f32": SCREEN1D_SIGNATURES["pre_screen1d_stencil2d_f32"][:-len(_scr1)] + _scr1c,
    "pre_screen1dcells_burgers_f32": SCREEN1D_SIGNATURES["pre_screen1d_burgers_f32"][:-len(_scr1)] + _scr1c,
    "pre_screen1dcells_pair_stencil2d_f32": SCREEN1DPAIR_SIGNATURES["pre_screen1dpair_stencil2d_f32"][:-len(_scr1)] + _scr1c,
    "pre_screen1dcells_pair_burgers_f32": SCREEN1DPAIR_SIGNATURES["pre_screen1dpair_burgers_f32"][:-len(_scr1)] + _scr1c,
}

# libcp_pre_screencellspair.so (include/cp_pre_screencellspair.h): the two 2-D screens against per-cell sets for the data-driven
# scores r(a) - r(b): each entry takes its twin's arguments in libcp_pre_screenpair.so with the set descriptor swapped for the
# per-cell one (PreScreenCells / PreScreenCellsFlat reused)
SCREENCELLSPAIR_SO_PATH = os.path.join(_HERE, "libcp_pre_screencellspair.so")
PRE_SCREENCELLSPAIR_ABI_VERSION = 1
_CELLS_DESC = {POINTER(PreScreen): POINTER(PreScreenCells), POINTER(PreScreenFlat): POINTER(PreScreenCellsFlat)}
SCREENCELLSPAIR_SIGNATURES = {"pre_screencellspair_abi_version": [], "pre_screencellspair_sample_group": []}
SCREENCELLSPAIR_SIGNATURES.update({
    _name.replace("pre_screenpair_", "pre_screencellspair_"): [_CELLS_DESC.get(_a, _a) for _a in _sig]
    for _name, _sig in SCREENPAIR_SIGNATURES.items() if _sig})

# libcp_pre_screenjorekcells.so (include/cp_pre_screenjorekcells.h): the two 2-D screens against per-cell sets for the
# reduced-MHD (JOREK) residuals: each entry takes its twin's arguments in libcp_pre_screenjorek.so with the set descriptor
# swapped for the per-cell one (PreScreenCells / PreScreenCellsFlat reused)
SCREENJOREKCELLS_SO_PATH = os.path.join(_HERE, "libcp_pre_screenjorekcells.so")
PRE_SCREENJOREKCELLS_ABI_VERSION = 1
_cellstail = [c_int64] * 4 + [c_int, c_void_p]                          # B, T, X, Y, flags, stream
SCREENJOREKCELLS_SIGNATURES = {
    "pre_screenjorekcells_abi_version": [],
    "pre_screenjorekcells_sample_group": [],
    "pre_screenjorekcells_f32": _jrk + [POINTER(PreScreenCells)] + _cellstail,
    "pre_screenjorekcells_flat_f32": _jrk + [POINTER(PreScreenCellsFlat)] + _cellstail,
}

# libcp_pre_screenstats.so (include/cp_pre_screenstats.h): per-sample statistics of the residual (sum r, sum |r|, sum r^2 in
# float64, max |r|) in one launch that stores no residual: each entry takes its twin's arguments in libcp_pre_screen.so /
# libcp_pre_screenflat.so / libcp_pre_screen1d.so with the set descriptor swapped for the statistics one
SCREENSTATS_SO_PATH = os.path.join(_HERE, "libcp_pre_screenstats.so")
PRE_SCREENSTATS_ABI_VERSION = 1
PRE_SCREENSTATS_FORM = {"": 0, "flat": 1, "rows": 2}                   # form of the fused screen -> PRE_SCREENSTATS_FORM_*


class PreScreenStats(ctypes.Structure):
    """``pre_screenstats_t``: the crop, the accumulators (bits of max |r| [B], float64 sums [3][sum_ld]) and the workspace."""
    _fields_ = [("ct", c_int), ("cx", c_int), ("cy", c_int), ("max_abs", c_void_p), ("sums", c_void_p), ("sum_ld", c_int64),
                ("workspace", c_void_p), ("workspace_len", c_int64)]


_STATS_DESC = {POINTER(PreScreen): POINTER(PreScreenStats), POINTER(PreScreenFlat): POINTER(PreScreenStats)}
SCREENSTATS_SIGNATURES = {
    "pre_screenstats_abi_version": [],
    "pre_screenstats_workspace_len": [c_int] + [c_int64] * 4,
    **{_name.replace(_old, _new): [_STATS_DESC.get(_a, _a) for _a in _sig]
       for _sigs, _old, _new in ((SCREEN_SIGNATURES, "pre_screen_", "pre_screenstats_"),
                                 (SCREENFLAT_SIGNATURES, "pre_screenflat_", "pre_screenstats_flat_"),
                                 (SCREEN1D_SIGNATURES, "pre_screen1d_", "pre_screenstats_rows_"))
       for _name, _sig in _sigs.items() if _sig},
}

# libcp_pre_vjpflatmhd.so (include/cp_pre_vjpflatmhd.h): the entries of libcp_pre_vjpmhd.so for Nt-fastest views (the march of
# libcp_pre_vjpflat.so), argument for argument
VJPFLATMHD_SO_PATH = os.path.join(_HERE, "libcp_pre_vjpflatmhd.so")
PRE_VJPFLATMHD_ABI_VERSION = 1
VJPFLATMHD_SIGNATURES = {name.replace("pre_vjpmhd_", "pre_vjpflatmhd_"): sig for name, sig in VJPMHD_SIGNATURES.items()}

# libcp_pre_vjpjorek.so (include/cp_pre_vjpjorek.h): the vector-Jacobian products of the reduced-MHD (JOREK) residuals for
# Nt-fastest views: the merged-row geometry of libcp_pre_vjpflat.so with three planes in LDS
VJPJOREK_SO_PATH = os.path.join(_HERE, "libcp_pre_vjpjorek.so")
PRE_VJPJOREK_ABI_VERSION = 1
VJPJOREK_SIGNATURES = {
    "pre_vjpjorek_abi_version": [],
    "pre_vjpjorek_supported": [c_int] + [POINTER(c_float)] * 5,
    # eq, g, fields, Rb, out, K_t .. K_ZZ, coef, then the tail of the MHD entries
    "pre_vjpjorek_flat_f32": [c_int, _fld, POINTER(PreField), _fld, POINTER(PreField)] + [POINTER(c_float)] * 6 + _mhdtail,
}

# libcp_pre_bcres.so (include/cp_pre_bcres.h): the fused residuals under boundary conditions on the x-y rim: each entry takes
# its zero-pad twin's arguments in libcp_pre_hip.so with a pre_bc_t (PreBC) before the extents; the 1-D linear entry takes a
# dense 3x3 kernel in place of a tap list
BCRES_SO_PATH = os.path.join(_HERE, "libcp_pre_bcres.so")
PRE_BCRES_ABI_VERSION = 1
PRE_BC_CONSTANT, PRE_BC_REPLICATE, PRE_BC_PERIODIC, PRE_BC_REFLECT = 0, 1, 2, 3


def _with_bc(sig, n_tail):
    """A zero-pad entry's signature with the boundary conditions before its last ``n_tail`` arguments (extents, flags, stream)."""
    return sig[:-n_tail] + [POINTER(PreBC)] + sig[-n_tail:]


BCRES_SIGNATURES = {
    "pre_bcres_abi_version": [],
    "pre_bcres_linear1_f32": [_fld, _fld, POINTER(c_float), POINTER(PreBC)] + [c_int64] * 4 + [c_int, c_void_p],
    "pre_bcres_linear2_f32": _with_bc(SIGNATURES["pre_residual_linear2_f32"], 6),
    "pre_bcres_ns_momentum_f32": _with_bc(SIGNATURES["pre_residual_ns_momentum_f32"], 6),
    "pre_bcres_mhd_f32": _with_bc(SIGNATURES["pre_residual_mhd_f32"], 6),
    "pre_bcres_burgers_f32": _with_bc(SIGNATURES["pre_residual_burgers_f32"], 5),
    "pre_bcres_linear1_rows_f32": [_fp, _i64p, _fp, _i64p, POINTER(c_float), POINTER(PreBC)] + [c_int64] * 3 + [c_int, c_void_p],
}

# libcp_pre_screenbc.so (include/cp_pre_screenbc.h): the screen and the per-sample statistics of the 2-D residuals under
# boundary conditions on the x-y rim: each entry takes its zero-pad twin's arguments in libcp_pre_screen.so /
# libcp_pre_screenstats.so (Ny-fastest form) with a pre_bc_t (PreBC) before the extents
SCREENBC_SO_PATH = os.path.join(_HERE, "libcp_pre_screenbc.so")
PRE_SCREENBC_ABI_VERSION = 1
SCREENBC_SIGNATURES = {
    "pre_screenbc_abi_version": [],
    "pre_screenbc_stats_workspace_len": [c_int64] * 4,
    **{_name.replace("pre_screen_", "pre_screenbc_"): _with_bc(_sig, 6) for _name, _sig in SCREEN_SIGNATURES.items() if _sig},
    **{_name.replace("pre_screen_", "pre_screenbc_stats_"): _with_bc(SCREENSTATS_SIGNATURES[_name.replace("pre_screen_", "pre_screenstats_")], 6)
       for _name, _sig in SCREEN_SIGNATURES.items() if _sig},
}

PRE_FFT_ABI_VERSION = 1        # include/cp_pre_fft.h (pre_fft_abi_version)

# One row per shared object: (module attribute that caches the handle, prefix of <P>SO_PATH / <P>SIGNATURES, version
# symbol, module attribute with the version the signatures were written for, entry points that return int64_t - stated
# by name: pre_fft_work_bytes, for one, returns int).  Paths, signatures and versions are read from the module at call
# time, so a tool or a test may point a library elsewhere and reset its cache attribute.
_LIBS = {
    "hip": ("_lib", "", "pre_abi_version", "PRE_ABI_VERSION", ("pre_joint_score_pruned_max_segments",)),
    "fft": ("_fft", "FFT_", "pre_fft_abi_version", "PRE_FFT_ABI_VERSION", ()),
    "dist": ("_dist", "DIST_", "pre_dist_abi_version", "PRE_DIST_ABI_VERSION", ()),
    "cov": ("_cov", "COV_", "pre_cov_abi_version", "PRE_COV_ABI_VERSION", ()),
    "ode": ("_ode", "ODE_", "pre_ode_abi_version", "PRE_ODE_ABI_VERSION", ()),
    "setprop": ("_setprop", "SETPROP_", "pre_setprop_abi_version", "PRE_SETPROP_ABI_VERSION", ()),
    "pair": ("_pair", "PAIR_", "pre_pair_abi_version", "PRE_PAIR_ABI_VERSION", ()),
    "bounds": ("_bounds", "BOUNDS_", "pre_bounds_abi_version", "PRE_BOUNDS_ABI_VERSION", ()),
}
# The libraries added since: same five-tuple, a table of their own (``_load`` consults both)
_LIBS_MORE = {
    "vjp": ("_vjp", "VJP_", "pre_vjp_abi_version", "PRE_VJP_ABI_VERSION", ()),
    "screen": ("_screen", "SCREEN_", "pre_screen_abi_version", "PRE_SCREEN_ABI_VERSION", ()),
    "screen1d": ("_screen1d", "SCREEN1D_", "pre_screen1d_abi_version", "PRE_SCREEN1D_ABI_VERSION", ()),
    "screenflat": ("_screenflat", "SCREENFLAT_", "pre_screenflat_abi_version", "PRE_SCREENFLAT_ABI_VERSION", ()),
    "vjpflat": ("_vjpflat", "VJPFLAT_", "pre_vjpflat_abi_version", "PRE_VJPFLAT_ABI_VERSION", ()),
    "wgrad": ("_wgrad", "WGRAD_", "pre_wgrad_abi_version", "PRE_WGRAD_ABI_VERSION", ()),
    "cns": ("_cns", "CNS_", "pre_cns_abi_version", "PRE_CNS_ABI_VERSION", ()),
    "cnsvjp": ("_cnsvjp", "CNSVJP_", "pre_cnsvjp_abi_version", "PRE_CNSVJP_ABI_VERSION", ()),
    "vjpmhd": ("_vjpmhd", "VJPMHD_", "pre_vjpmhd_abi_version", "PRE_VJPMHD_ABI_VERSION", ()),
    "screenjorek": ("_screenjorek", "SCREENJOREK_", "pre_screenjorek_abi_version", "PRE_SCREENJOREK_ABI_VERSION", ()),
    "vjpflatmhd": ("_vjpflatmhd", "VJPFLATMHD_", "pre_vjpflatmhd_abi_version", "PRE_VJPFLATMHD_ABI_VERSION", ()),
    "vjpjorek": ("_vjpjorek", "VJPJOREK_", "pre_vjpjorek_abi_version", "PRE_VJPJOREK_ABI_VERSION", ()),
    "screenpair": ("_screenpair", "SCREENPAIR_", "pre_screenpair_abi_version", "PRE_SCREENPAIR_ABI_VERSION", ()),
    "screen1dpair": ("_screen1dpair", "SCREEN1DPAIR_", "pre_screen1dpair_abi_version", "PRE_SCREEN1DPAIR_ABI_VERSION", ()),
    "screencells": ("_screencells", "SCREENCELLS_", "pre_screencells_abi_version", "PRE_SCREENCELLS_ABI_VERSION", ()),
    "screen1dcells": ("_screen1dcells", "SCREEN1DCELLS_", "pre_screen1dcells_abi_version", "PRE_SCREEN1DCELLS_ABI_VERSION", ()),
    "screencellspair": ("_screencellspair", "SCREENCELLSPAIR_", "pre_screencellspair_abi_version",
                        "PRE_SCREENCELLSPAIR_ABI_VERSION", ()),
    "screenjorekcells": ("_screenjorekcells", "SCREENJOREKCELLS_", "pre_screenjorekcells_abi_version",
                         "PRE_SCREENJOREKCELLS_ABI_VERSION", ()),
    "screenstats": ("_screenstats", "SCREENSTATS_", "pre_screenstats_abi_version", "PRE_SCREENSTATS_ABI_VERSION",
                    ("pre_screenstats_workspace_len",)),
    "bcres": ("_bcres", "BCRES_", "pre_bcres_abi_version", "PRE_BCRES_ABI_VERSION", ()),
    "screenbc": ("_screenbc", "SCREENBC_", "pre_screenbc_abi_version", "PRE_SCREENBC_ABI_VERSION",
                 ("pre_screenbc_stats_workspace_len",)),
}
_lib = _fft = _dist = _cov = _ode = _setprop = _pair = _bounds = _vjp = _screen = _screen1d = _screenflat = _vjpflat = _wgrad = _cns = _cnsvjp = _vjpmhd = _screenjorek = _vjpflatmhd = _vjpjorek = _screenpair = _screen1dpair = _screencells = _screen1dcells = _screencellspair = _screenjorekcells = _screenstats = _bcres = _screenbc = None
_BUILD_HINT = "`python -c 'import __graft_entry__ as g; g.build()'`"


def _load(key):
    """ctypes handle of one library (loaded once, after torch, so that it binds to the HIP / hipFFT runtime torch already
    loaded); raises ImportError loudly if the file is absent or of another ABI version."""
    g = globals()
    cache, prefix, version_fn, version, int64_returns = _LIBS[key] if key in _LIBS else _LIBS_MORE[key]
    if g[cache] is None:
        path, want = g[prefix + "SO_PATH"], g[version]
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing: build it with {_BUILD_HINT}" +
                              (" (hipcc --offload-arch=gfx950).  cp_pre_amd has no CPU fallback." if key == "hip" else ""))
        lib = ctypes.CDLL(path)
        # first: a stale .so with the same symbol names but other signatures would pass misaligned arguments into a
        # kernel launch
        fn = getattr(lib, version_fn)
        fn.argtypes, fn.restype = [], c_int
        have = fn()
        if have != want:
            raise ImportError(f"{path} has ABI version {have}, this binding was written for {want}: rebuild it ({_BUILD_HINT})")
        for name, argtypes in g[prefix + "SIGNATURES"].items():
            fn = getattr(lib, name)        # AttributeError here = header / library out of sync
            fn.argtypes = argtypes
            fn.restype = c_int64 if name in int64_returns else c_int
        g[cache] = lib
    return g[cache]


def load():
    """Load (once) and return the handle of libcp_pre_hip.so; raise loudly if the extension is absent."""
    return _lib or _load("hip")


def load_fft():
    return _fft or _load("fft")


def load_dist():
    return _dist or _load("dist")


def load_cov():
    return _cov or _load("cov")


def load_ode():
    return _ode or _load("ode")


def load_setprop():
    return _setprop or _load("setprop")


def load_pair():
    return _pair or _load("pair")


def load_bounds():
    return _bounds or _load("bounds")


def load_vjp():
    return _vjp or _load("vjp")


def load_screen():
    return _screen or _load("screen")


def load_screen1d():
    return _screen1d or _load("screen1d")


def load_screenflat():
    return _screenflat or _load("screenflat")


def load_vjpflat():
    return _vjpflat or _load("vjpflat")


def load_wgrad():
    return _wgrad or _load("wgrad")


def load_cns():
    return _cns or _load("cns")


def load_cnsvjp():
    return _cnsvjp or _load("cnsvjp")


def load_vjpmhd():
    return _vjpmhd or _load("vjpmhd")


def load_screenjorek():
    return _screenjorek or _load("screenjorek")


def load_vjpflatmhd():
    return _vjpflatmhd or _load("vjpflatmhd")


def load_vjpjorek():
    return _vjpjorek or _load("vjpjorek")


def load_screenpair():
    return _screenpair or _load("screenpair")


def load_screen1dpair():
    return _screen1dpair or _load("screen1dpair")


def load_screencells():
    return _screencells or _load("screencells")


def load_screen1dcells():
    return _screen1dcells or _load("screen1dcells")


def load_screencellspair():
    return _screencellspair or _load("screencellspair")


def load_screenjorekcells():
    return _screenjorekcells or _load("screenjorekcells")


def load_screenstats():
    return _screenstats or _load("screenstats")


def load_screenbc():
    """libcp_pre_screenbc.so: loaded only by a screen or statistics call with ``bc=`` (``screen``)."""
    return _screenbc or _load("screenbc")


def load_bcres():
    """Loaded on the first residual with ``bc=``, never otherwise."""
    return _bcres or _load("bcres")


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("cp_pre_amd: no HIP device visible; the residual / calibration path runs only on "
                           "an MI355X (there is deliberately no CPU fallback)")


def check(rc, what):
    if rc == PRE_OK:
        return
    if rc < 0:
        raise RuntimeError(f"{what}: {_ERR.get(rc, 'error')} (rc={rc})")
    if rc >= 1000:
        raise RuntimeError(f"{what}: hipfftResult {rc - 1000}")
    raise RuntimeError(f"{what}: hipError_t {rc}")


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def field(t):
    """PreField for a 4-D fp32 device view (any strides)."""
    assert t.dim() == 4
    s = t.stride()
    return PreField(t.data_ptr(), s[0], s[1], s[2], s[3])


# A row pitch that is a multiple of a large power of two puts every row of a per-cell select's column tile on the same HBM
# channels: the same kernel on the same bytes runs 2.5 instead of 3.4 TB/s at n = 1200-2048 rows, 2.8 / 2.5 instead of
# 3.3 / 3.0 at n = 4096 / 8192 (profiles/r05/select_scan.txt, column "pitch M"; the register-sort forms below 241 rows do
# not care, and rows up to 32 KiB long lose nothing: profiles/r04/rowpage.txt).  Score matrices THIS package allocates
# (|residual| outputs, device copies of host score arrays) therefore get rows PAD floats further apart than they are
# long; tensors the caller owns are selected where they lie.
PAD_MIN_ROWS, PAD_ROW_MULTIPLE, PAD = 241, 1 << 14, 64


def wants_row_pad(n, M):
    return n >= PAD_MIN_ROWS and M >= PAD_ROW_MULTIPLE and M % PAD_ROW_MULTIPLE == 0


def empty_like_layout(t, score_rows=False):
    """Uninitialised fp32 tensor with ``t``'s shape and ``t``'s axis order in memory (dense): a
    [BS,Nt,Nx,Ny] view of a [BS,Nx,Ny,Nt] buffer gets an output laid out the same way, so the
    streaming kernels read and write along the same contiguous axis.
    ``score_rows``: the result is a score matrix [n, *cells] (an |residual| output, about to be selected along axis 0):
    its rows are PAD floats further apart than they are long when ``wants_row_pad`` says that pays."""
    order = sorted(range(t.dim()), key=lambda d: (-t.stride(d), d))         # slowest axis first
    M = 1
    for n in t.shape[1:]:                                                    # (from the shape: t[0] does not exist at n == 0)
        M *= n
    if score_rows and t.dim() >= 2 and order[0] == 0 and wants_row_pad(t.shape[0], M):
        strides, acc = [0] * t.dim(), 1
        for d in reversed(order[1:]):
            strides[d] = acc
            acc *= t.shape[d]
        strides[0] = M + PAD
        buf = torch.empty(t.shape[0] * (M + PAD), dtype=torch.float32, device=t.device)
        return buf.as_strided(tuple(t.shape), tuple(strides))
    if t.is_contiguous():
        return torch.empty(t.shape, dtype=torch.float32, device=t.device)
    strides, acc = [0] * t.dim(), 1
    for d in reversed(order):
        strides[d] = acc
        acc *= t.shape[d]
    return torch.empty_strided(tuple(t.shape), tuple(strides), dtype=torch.float32, device=t.device)


def streamable(*views):
    """True if one of the last three axes has unit stride in every view (library relabels axes)."""
    return any(all(v.stride(ax) == 1 for v in views) for ax in (-1, -2, -3) if views[0].dim() >= -ax)


def farr(values):
    return (c_float * len(values))(*[float(v) for v in values])


def iarr32(values):
    return (c_int32 * len(values))(*[int(v) for v in values])


def iarr64(values):
    return (c_int64 * len(values))(*[int(v) for v in values])
