"""
ctypes binding of libglimship.so (the only compute backend; there is no CPU fallback).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C glimslib_amd/csrc``.
Signatures mirror ``include/glims_hip.h`` one to one.
"""
from __future__ import annotations

import ctypes as C
import logging
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libglimship.so")

GLIMS_OK, GLIMS_NOT_CONVERGED, GLIMS_NAN = 0, 1, 2
GLIMS_E_USAGE, GLIMS_E_HIP, GLIMS_E_RCCL, GLIMS_E_NO_DEVICE = -1, -2, -3, -4
GLIMS_UNIQUE_ID_BYTES = 256
FLAG_EXTRAPOLATE_GUESS = 1
FLAG_WARM_START = 2
FLAG_FP32_JACOBIAN = 4
FLAG_MG_FP32_SMOOTHER = 8
FLAG_INT32_COLUMNS = 16
FLAG_MG_FP64_VECTORS = 32
FLAG_MG_WHOLE_GRID = 64
FLAG_FULL_NEWTON = 128
FLAG_FIXED_FORCING = 256
FLAG_MG_NO_LUMPING = 512
FLAG_NO_FUSED_GUESS = 1024
FLAG_NO_FUSED_MASS = 2048
FLAG_SLOT_WORDS32 = 4096
FLAG_RECORD_WORDS_FULL = 8192
FLAG_NO_VALUE_CODES = 16384
FLAG_STORE_LINEAR_SLICES = 32768
PRECOND_BLOCK_JACOBI, PRECOND_MULTIGRID = 0, 1
RD_PRECOND_AUTO, RD_PRECOND_JACOBI, RD_PRECOND_MULTIGRID = 0, 1, 2
RD_LINEAR_AUTO, RD_LINEAR_PCG, RD_LINEAR_CHEBYSHEV = 0, 1, 2
STREAM_AUTO, STREAM_NONTEMPORAL, STREAM_CACHED = 0, 1, 2
FIELD_C, FIELD_U, FIELD_SNAPSHOT_C, FIELD_HOST = 0, 1, 2, 3
FIELD_DERIVED = 4       # the result of the last glims_derive, sampled from its device buffer
FIELD_XYZ = 5           # the mesh's reference coordinates: on a deformed sampler the back map X(x_p)
DERIVE_CURRENT, DERIVE_HOST = -1, -2
# glims_derive kinds by name (GLIMS_DERIVE_*); the first two are tensors
DERIVE_KINDS = {"strain_tensor": 0, "stress_tensor": 1, "pressure": 2, "van_mises_stress": 3, "displacement_norm": 4,
                "log_growth": 5, "mech_expansion": 6, "total_jacobian": 7, "growth_induced_jacobian": 8,
                "concentration_deformed_config": 9}
# glims_observe kinds by name (GLIMS_OBSERVE_*)
OBSERVE_KINDS = {"mass": 0, "sharp": 1, "smooth": 2}
OBSERVE_MAX_QUERIES = 8
SAMPLE_EPS = 1e-10      # GLIMS_SAMPLE_EPS: a cell accepts a point iff min lambda >= -SAMPLE_EPS
SAMPLE_MAX_COMP = 8
ABI_VERSION = 6


class BackendError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libglimship: %s (status %d)" % (msg, code))
        self.code = code


class Options(C.Structure):
    _fields_ = [("dt", C.c_double), ("newton_rtol", C.c_double), ("newton_atol", C.c_double),
                ("newton_maxit", C.c_int), ("cg_rtol", C.c_double), ("cg_atol", C.c_double),
                ("cg_maxit", C.c_int), ("mech_rtol", C.c_double), ("mech_atol", C.c_double),
                ("mech_maxit", C.c_int), ("check_every", C.c_int), ("flags", C.c_int),
                ("mech_precond", C.c_int), ("mech_mixed", C.c_int), ("mech_history", C.c_int),
                ("mg_smooth", C.c_int), ("mg_coarse_nodes", C.c_int), ("mg_h_factor", C.c_double),
                ("mg_cheb_ratio", C.c_double), ("time_kernels", C.c_int),
                ("rd_precond", C.c_int), ("rd_mg_smooth", C.c_int),
                ("rd_linear", C.c_int), ("stream_policy", C.c_int)]


class Stats(C.Structure):
    _fields_ = [("steps", C.c_int64), ("newton_its", C.c_int64), ("rd_assemblies", C.c_int64),
                ("cg_its", C.c_int64), ("mech_solves", C.c_int64), ("mech_cg_its", C.c_int64),
                ("last_newton_res", C.c_double), ("last_cg_res", C.c_double), ("last_mech_res", C.c_double),
                ("ms_steps", C.c_double), ("ms_spmv", C.c_double), ("n_rows", C.c_int64), ("nnz", C.c_int64),
                ("nnz_padded", C.c_int64), ("n_corners", C.c_int64), ("nnz_idx16", C.c_int64),
                ("ms_spmv_steps", C.c_double), ("n_spmv_steps", C.c_int64),
                ("failed_steps", C.c_int64), ("mg_levels", C.c_int64), ("mg_cycles", C.c_int64),
                ("mg_complexity", C.c_double), ("ms_mg_setup", C.c_double), ("ms_mech", C.c_double),
                ("ms_sweep_steps", C.c_double), ("n_sweep_steps", C.c_int64), ("ms_update_steps", C.c_double),
                ("n_update_steps", C.c_int64), ("us_spmv_median", C.c_double), ("us_sweep_median", C.c_double),
                ("us_update_median", C.c_double),
                ("rd_precond_used", C.c_int64), ("rd_stiffness_ratio", C.c_double), ("rd_mg_levels", C.c_int64),
                ("rd_mg_cycles", C.c_int64), ("rd_mg_complexity", C.c_double), ("ms_rd_mg_setup", C.c_double),
                ("ms_mgfine_mech", C.c_double), ("n_mgfine_mech", C.c_int64), ("us_mgfine_median", C.c_double),
                ("ms_spmvb_mech", C.c_double), ("n_spmvb_mech", C.c_int64), ("us_spmvb_median", C.c_double),
                ("rd_quad_updates", C.c_int64), ("ms_quad_steps", C.c_double), ("n_quad_steps", C.c_int64),
                ("us_quad_median", C.c_double),
                ("midpoint_steps", C.c_int64), ("rebase_events", C.c_int64),
                ("halo_exchanges", C.c_int64), ("halo_bytes", C.c_int64), ("ms_exchange", C.c_double),
                ("ms_exchange_exposed", C.c_double), ("allreduces", C.c_int64), ("reduce_transport", C.c_int64),
                ("mg_grid1_bytes", C.c_int64),
                ("halo_exchanges_timed", C.c_int64), ("cheb_solves", C.c_int64), ("cheb_its", C.c_int64),
                ("cheb_fallbacks", C.c_int64), ("cheb_learn_solves", C.c_int64), ("cheb_lmin", C.c_double),
                ("cheb_lmax", C.c_double), ("ms_cheb_steps", C.c_double), ("n_cheb_steps", C.c_int64),
                ("us_cheb_median", C.c_double), ("stream_nontemporal", C.c_int64), ("krylov_working_set", C.c_int64),
                ("mg_box_fraction", C.c_double), ("cheb_fused_passes", C.c_int64),
                ("rd_mass_in_sweep", C.c_int64), ("rd_mass_fallback_rows", C.c_int64),
                ("cheb_host_counts", C.c_int64), ("cheb_fused_zero_starts", C.c_int64),
                ("rd_slot16_sweeps", C.c_int64), ("rd_rec_compact_slices", C.c_int64),
                ("rd_rec_full_slices", C.c_int64), ("rd_rec32_sweeps", C.c_int64),
                ("rd_scode_slices", C.c_int64), ("rd_scode_uncoded_slices", C.c_int64),
                ("rd_lin_slices", C.c_int64), ("cheb_coded_passes", C.c_int64),
                ("rd_lin_kept_slices", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


MISFIT_C_L2, MISFIT_C_THRESH, MISFIT_U_L2 = 0, 1, 2


class Misfit(C.Structure):
    _fields_ = [("step", C.c_int64), ("kind", C.c_int), ("level", C.c_double), ("smooth", C.c_double),
                ("weight", C.c_double), ("target", C.POINTER(C.c_double))]


MISFIT_IMG_L2, MISFIT_IMG_THRESH = 0, 1
_IMAGE_KINDS = {"img_l2": MISFIT_IMG_L2, "img_thresh": MISFIT_IMG_THRESH}


class ImageMisfit(C.Structure):
    """glims_image_misfit: an image-space misfit term (target / pweight in the point order of the sampler)."""
    _fields_ = [("step", C.c_int64), ("sampler", C.c_int64), ("kind", C.c_int), ("level", C.c_double),
                ("smooth", C.c_double), ("weight", C.c_double), ("target", C.POINTER(C.c_double)),
                ("pweight", C.POINTER(C.c_double))]


class DisplacementImageMisfit(C.Structure):
    """glims_displacement_image_misfit: a displacement-image misfit term (target [n_points][dim] / pweight [n_points] in the
    point order of the sampler, cweight the per-component weights)."""
    _fields_ = [("step", C.c_int64), ("sampler", C.c_int64), ("weight", C.c_double), ("scale", C.c_double),
                ("cweight", C.c_double * 3), ("target", C.POINTER(C.c_double)), ("pweight", C.POINTER(C.c_double))]


class DeformedImageMisfit(C.Structure):
    """glims_deformed_image_misfit: an image term of the deformed configuration; it carries its own point set (xyz, or the
    grid origin / spacing / size when xyz is NULL)."""
    _fields_ = [("step", C.c_int64), ("kind", C.c_int), ("level", C.c_double), ("smooth", C.c_double),
                ("weight", C.c_double), ("scale", C.c_double), ("n_points", C.c_int64), ("xyz", C.POINTER(C.c_double)),
                ("origin", C.c_double * 3), ("spacing", C.c_double * 3), ("size", C.c_int64 * 3),
                ("target", C.POINTER(C.c_double)), ("pweight", C.POINTER(C.c_double))]


class Observable(C.Structure):
    """glims_observable: one query of glims_observe (kind: OBSERVE_KINDS; smooth: 'smooth' only)."""
    _fields_ = [("kind", C.c_int), ("level", C.c_double), ("smooth", C.c_double)]


class ObservableMisfit(C.Structure):
    """glims_observable_misfit: a volume misfit term J = 1/2 weight (V - target)^2 of a glims_observe measure (labels: a uint8
    mask [n_labels] of the counted labels, or NULL for the whole domain)."""
    _fields_ = [("step", C.c_int64), ("kind", C.c_int), ("level", C.c_double), ("smooth", C.c_double),
                ("weight", C.c_double), ("target", C.c_double), ("labels", C.POINTER(C.c_uint8))]


class ObservableMisfit2(C.Structure):
    """glims_observable_misfit2: ObservableMisfit, then the configuration the cells are measured in (deformed: at X + scale u_k,
    with the gradient through u_k)."""
    _fields_ = ObservableMisfit._fields_ + [("deformed", C.c_int), ("scale", C.c_double)]


class ObservableMisfit3(C.Structure):
    """glims_observable_misfit3: ObservableMisfit2, then what the term compares (moment 0: the volume with target; 1: the
    centre of mass M / V with target_x [dim])."""
    _fields_ = ObservableMisfit2._fields_ + [("moment", C.c_int), ("target_x", C.c_double * 3)]


_dp = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_h = C.c_void_p

# name -> (restype, argtypes); every symbol declared in include/glims_hip.h
SIGNATURES = {
    "glims_abi_version": (C.c_int, []),
    "glims_create": (C.c_int, [C.POINTER(_h), C.c_int, C.c_int64, C.c_int64, C.c_int64, _dp, _i32p, _i32p, C.c_int]),
    "glims_destroy": (C.c_int, [_h]),
    "glims_last_error": (C.c_char_p, [_h]),
    "glims_set_materials": (C.c_int, [_h, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    "glims_set_diffusion_tensor": (C.c_int, [_h, _dp]),
    "glims_diffusion_tensor_info": (C.c_int, [_h, _i64p, _dp]),
    "glims_set_diffusion_tensor_tangents": (C.c_int, [_h, C.c_int, _dp]),
    "glims_adjoint_tensor_gradient": (C.c_int, [_h, C.c_int, C.c_int, _dp]),
    "glims_options_default": (C.c_int, [C.POINTER(Options)]),
    "glims_set_options": (C.c_int, [_h, C.POINTER(Options)]),
    "glims_set_dirichlet_u": (C.c_int, [_h, C.c_int64, _i64p, _dp]),
    "glims_set_dirichlet_c": (C.c_int, [_h, C.c_int64, _i64p, _dp]),
    "glims_set_rd_load": (C.c_int, [_h, _dp]),
    "glims_set_mech_load": (C.c_int, [_h, _dp]),
    "glims_setup": (C.c_int, [_h, C.c_int]),
    "glims_set_state": (C.c_int, [_h, _dp, _dp]),
    "glims_get_state": (C.c_int, [_h, _dp, _dp]),
    "glims_step": (C.c_int, [_h, C.c_int]),
    "glims_solve_mechanics": (C.c_int, [_h]),
    "glims_get_stats": (C.c_int, [_h, C.POINTER(Stats)]),
    "glims_reset_stats": (C.c_int, [_h]),
    "glims_apply": (C.c_int, [_h, C.c_int, _dp, _dp, C.c_int, _dp]),
    "glims_rd_residual": (C.c_int, [_h, _dp, _dp, _dp]),
    "glims_peek_partials": (C.c_int, [_h, _dp]),
    "glims_get_numbering": (C.c_int, [_h, _i32p]),
    "glims_pattern_checksum": (C.c_int, [_h, C.POINTER(C.c_uint64)]),
    "glims_snapshot_save": (C.c_int, [_h, _i64p]),
    "glims_snapshot_load": (C.c_int, [_h, C.c_int64, _dp]),
    "glims_snapshot_mechanics": (C.c_int, [_h, C.c_int64, _dp]),
    "glims_snapshot_clear": (C.c_int, [_h]),
    "glims_project": (C.c_int, [_h, _dp, _dp, C.c_int, C.c_double]),
    "glims_derive": (C.c_int, [_h, C.c_int, C.c_int64, _dp, _dp, C.c_double, _dp]),
    "glims_derive_info": (C.c_int, [_h, _i64p]),
    "glims_observe": (C.c_int, [_h, C.c_int, _i64p, _dp, _dp, C.c_int, C.c_double, C.c_int, C.POINTER(Observable), _dp]),
    "glims_observe_info": (C.c_int, [_h, _i64p]),
    "glims_adjoint_record": (C.c_int, [_h, C.c_int]),
    "glims_adjoint_gradient": (C.c_int, [_h, C.c_int, C.POINTER(Misfit), _dp, _dp, _dp, _dp, _dp]),
    "glims_adjoint_gradient_full": (C.c_int, [_h, C.c_int, C.POINTER(Misfit), _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "glims_adjoint_hessian": (C.c_int, [_h, C.c_int, C.POINTER(Misfit), C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                        _dp, _dp, _dp, _dp, _dp, _dp]),
    "glims_adjoint_hessian_spmd": (C.c_int, [_h, C.c_int, C.POINTER(Misfit), C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                             _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "glims_adjoint_hessian_full": (C.c_int, [_h, C.c_int, C.POINTER(Misfit), C.c_int] + [_dp] * 20),
    "glims_adjoint_stats": (C.c_int, [_h, _i64p, _dp]),
    "glims_sampler_create_points": (C.c_int, [_h, C.c_int64, _dp, C.c_int, _i64p]),
    "glims_sampler_create_grid": (C.c_int, [_h, _dp, _dp, _i64p, C.c_int, _i64p]),
    "glims_sampler_create_grid_deformed": (C.c_int, [_h, _dp, _dp, _i64p, C.c_int64, _dp, C.c_double, C.c_int, _i64p]),
    "glims_sampler_create_points_deformed": (C.c_int, [_h, C.c_int64, _dp, C.c_int64, _dp, C.c_double, C.c_int, _i64p]),
    "glims_sampler_deformation_info": (C.c_int, [_h, C.c_int64, _i64p, _dp]),
    "glims_sampler_warp": (C.c_int, [_h, C.c_int64, _dp, _dp, _dp, _i64p, C.c_int, C.c_int, C.c_double, _dp]),
    "glims_sampler_info": (C.c_int, [_h, C.c_int64, _i64p, _i64p]),
    "glims_sampler_get": (C.c_int, [_h, C.c_int64, _i32p, _dp]),
    "glims_sampler_apply": (C.c_int, [_h, C.c_int64, C.c_int, C.c_int64, _dp, C.c_int, C.c_double, _dp]),
    "glims_sampler_apply_t": (C.c_int, [_h, C.c_int64, _dp, C.c_int, _dp]),
    "glims_sampler_resolve": (C.c_int, [_h, C.c_int64, _i64p]),
    "glims_sampler_get_counted": (C.c_int, [_h, C.c_int64, C.POINTER(C.c_uint8)]),
    "glims_sampler_destroy": (C.c_int, [_h, C.c_int64]),
    "glims_adjoint_image_terms": (C.c_int, [_h, C.c_int, C.POINTER(ImageMisfit)]),
    "glims_adjoint_image_info": (C.c_int, [_h, C.c_int, _i64p]),
    "glims_adjoint_displacement_image_terms": (C.c_int, [_h, C.c_int, C.POINTER(DisplacementImageMisfit)]),
    "glims_adjoint_displacement_image_info": (C.c_int, [_h, C.c_int, _i64p]),
    "glims_adjoint_deformed_image_terms": (C.c_int, [_h, C.c_int, C.POINTER(DeformedImageMisfit)]),
    "glims_adjoint_deformed_image_info": (C.c_int, [_h, C.c_int, _i64p, _dp]),
    "glims_adjoint_observable_terms": (C.c_int, [_h, C.c_int, C.POINTER(ObservableMisfit)]),
    "glims_adjoint_observable_info": (C.c_int, [_h, C.c_int, _i64p, _dp]),
    "glims_adjoint_observable_terms2": (C.c_int, [_h, C.c_int, C.POINTER(ObservableMisfit2)]),
    "glims_adjoint_observable_info2": (C.c_int, [_h, C.c_int, _i64p, _dp, _dp]),
    "glims_adjoint_observable_terms3": (C.c_int, [_h, C.c_int, C.POINTER(ObservableMisfit3)]),
    "glims_adjoint_observable_info3": (C.c_int, [_h, C.c_int, _i64p, _dp, _dp, _dp]),
    "glims_comm_unique_id": (C.c_int, [C.c_char_p]),
    "glims_comm_init": (C.c_int, [_h, C.c_int, C.c_int, C.c_char_p]),
    "glims_comm_selftest": (C.c_int, [_h]),
    "glims_comm_mailbox": (C.c_int, [_h, C.c_char_p]),
    "glims_comm_mailbox_selftest": (C.c_int, [_h]),
    "glims_set_halo": (C.c_int, [_h, C.c_int, _i32p, _i64p, _i32p, _i64p]),
    "glims_set_mg_frame": (C.c_int, [_h, _dp, _dp]),
    "glims_set_transport": (C.c_int, [_h, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}

HALO_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, _i64p, C.c_void_p, _i64p, C.c_int, _i32p, C.c_int, C.c_void_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)

_lib = None


def load_library():
    """Load libglimship.so or fail loudly -- there is no alternative compute path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "glimslib_amd: %s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C glimslib_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.glims_abi_version.restype = C.c_int
    if lib.glims_abi_version() != ABI_VERSION:
        raise ImportError("glimslib_amd: %s has ABI version %d, this binding needs %d -- rebuild it (make -C glimslib_amd/csrc)"
                          % (LIB_PATH, lib.glims_abi_version(), ABI_VERSION))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        assert a.shape == shape, (a.shape, shape)
    return a


def _ptr(a, typ):
    return a.ctypes.data_as(typ) if a is not None else None


def pack_diffusion_tensor(T, n_cells, dim):
    """The packed field [n_cells, d (d + 1) / 2] (upper triangle row by row, the ITK order) of a tensor field given as
    [n_cells, d, d], as the packed array itself, or as ONE [d, d] matrix for every cell.  ValueError for any other shape and
    for a full matrix that is not symmetric (to 1e-12 of its largest entry); positive definiteness is the library's check."""
    T = np.asarray(T, dtype=np.float64)
    nt = dim * (dim + 1) // 2
    iu = np.triu_indices(dim)
    if T.shape == (dim, dim):
        T = np.broadcast_to(T, (n_cells, dim, dim))
    if T.shape == (n_cells, dim, dim):
        asym = np.abs(T - np.swapaxes(T, 1, 2)).max(axis=(1, 2)) if n_cells else np.zeros(0)
        scale = np.abs(T).max(axis=(1, 2)) if n_cells else np.zeros(0)
        bad = np.nonzero(asym > 1e-12 * scale)[0]   # (a NaN compares False here and goes on to the library's check)
        if len(bad):
            raise ValueError("diffusion tensor of cell %d is not symmetric (%d such cells)" % (bad[0], len(bad)))
        return np.ascontiguousarray(T[:, iu[0], iu[1]])
    if T.shape == (n_cells, nt):
        return np.ascontiguousarray(T)
    raise ValueError("diffusion tensor of shape %s: need [%d, %d, %d], the packed [%d, %d] or one [%d, %d] matrix"
                     % (T.shape, n_cells, dim, dim, n_cells, nt, dim, dim))


DT_MAX_TANGENTS = 4   # GLIMS_DT_MAX_TANGENTS


def pack_diffusion_tensor_tangents(dT, n_cells, dim):
    """The packed tangent fields [K, n_cells, d (d + 1) / 2] of dT given as [K, n_cells, d, d], as the packed array itself, or
    as a list of K fields in any form ``pack_diffusion_tensor`` takes (its ValueErrors: shape, a full matrix that is not
    symmetric).  More than DT_MAX_TANGENTS fields go on to the library's refusal."""
    if isinstance(dT, np.ndarray) and dT.ndim in (3, 4):
        dT = list(dT)
    elif isinstance(dT, np.ndarray):
        raise ValueError("diffusion tensor tangents of shape %s: need [K, %d, %d, %d], the packed [K, %d, %d] or a list of fields"
                         % (dT.shape, n_cells, dim, dim, n_cells, dim * (dim + 1) // 2))
    fields = [pack_diffusion_tensor(f, n_cells, dim) for f in dT]
    return np.ascontiguousarray(np.stack(fields)) if fields else np.zeros((0, n_cells, dim * (dim + 1) // 2))


class Handle:
    """Thin OO view of one ``glims_ctx`` (one mesh on one GPU)."""

    def __init__(self, points, cells, cell_label, n_own=None, device=0):
        lib = load_library()
        self.lib = lib
        pts = _f64(points)
        cl = np.ascontiguousarray(cells, dtype=np.int32)
        lab = np.ascontiguousarray(cell_label, dtype=np.int32)
        self.dim = pts.shape[1]
        self.n_nodes = pts.shape[0]
        self.n_own = self.n_nodes if n_own is None else int(n_own)
        self.n_cells = cl.shape[0]
        assert cl.shape[1] == self.dim + 1 and lab.shape == (self.n_cells,)
        h = _h()
        st = lib.glims_create(C.byref(h), self.dim, self.n_nodes, self.n_own, self.n_cells,
                              _ptr(pts, _dp), _ptr(cl, _i32p), _ptr(lab, _i32p), int(device))
        if st != GLIMS_OK:
            raise BackendError(st, (lib.glims_last_error(None) or b"").decode())
        self._h = h
        self.options = Options()
        lib.glims_options_default(C.byref(self.options))
        self.n_labels = None   # label count of the last successful set_materials
        self.n_tangents = 0    # tangent fields of the last successful set_diffusion_tensor_tangents
        self._image_terms = []   # what the library's stored image terms were made from (see _sync_image_terms)
        self._deformed_terms = []   # ... and the stored deformed image terms (see _split_terms)
        self._displacement_terms = []   # ... and the stored displacement image terms
        self._observable_terms = []   # ... and the keys of the stored volume terms
        self._observable_from_list = False
        self._warned_folded = False

    # -- plumbing --------------------------------------------------------------------------------
    def _check(self, st, allow=()):
        if st != GLIMS_OK and st not in allow:
            raise BackendError(st, (self.lib.glims_last_error(self._h) or b"").decode())
        return st

    def close(self):
        if getattr(self, "_h", None):
            self.lib.glims_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- model data ------------------------------------------------------------------------------
    def set_materials(self, D, rho, gamma, E, nu):
        arrs = [_f64(a) for a in (D, rho, gamma, E, nu)]
        n = len(arrs[0])
        assert all(a.shape == (n,) for a in arrs)
        self._check(self.lib.glims_set_materials(self._h, n, *[_ptr(a, _dp) for a in arrs]))
        self.n_labels = n

    def set_diffusion_tensor(self, T):
        """glims_set_diffusion_tensor: the per-cell tensor field of the anisotropic model, flux D_t * T_cell grad c.  T is
        [n_cells, d, d] (symmetric) or the packed [n_cells, d (d + 1) / 2] upper triangles row by row -- (xx, xy, yy) /
        (xx, xy, xz, yy, yz, zz) -- in the caller's cell order; None clears the field.  Takes effect with the next setup()
        (the contract of set_materials).  A non-finite or not positive-definite tensor raises BackendError(GLIMS_E_USAGE)
        naming the first bad cell, and the previous field stays."""
        if T is None:
            self._check(self.lib.glims_set_diffusion_tensor(self._h, None))
            return
        T = pack_diffusion_tensor(T, self.n_cells, self.dim)
        self._check(self.lib.glims_set_diffusion_tensor(self._h, _ptr(T, _dp)))

    def set_diffusion_tensor_tangents(self, dT):
        """glims_set_diffusion_tensor_tangents: K <= 4 tangent fields dT/dtheta_k of the tensor field -- [K, n_cells, d, d],
        the packed [K, n_cells, d (d + 1) / 2], or a list of fields in any form set_diffusion_tensor takes -- in the caller's
        cell order; None (or no field) clears them.  Symmetric, not necessarily definite.  Every backward sweep that follows
        (adjoint_gradient, adjoint_hessian*) adds up dJ/dtheta_k per label: adjoint_tensor_gradient().  Nothing of the set-up
        or a recording is invalidated.  A non-finite entry raises BackendError(GLIMS_E_USAGE) naming the tangent and the
        first bad cell, more than 4 fields likewise, and the stored tangents stay."""
        if dT is None:
            self._check(self.lib.glims_set_diffusion_tensor_tangents(self._h, 0, None))
            self.n_tangents = 0
            return
        dT = pack_diffusion_tensor_tangents(dT, self.n_cells, self.dim)
        self._check(self.lib.glims_set_diffusion_tensor_tangents(self._h, len(dT), _ptr(dT, _dp) if len(dT) else None))
        self.n_tangents = len(dT)

    def adjoint_tensor_gradient(self):
        """glims_adjoint_tensor_gradient: [K, n_labels], dJ/dtheta_k per label from the last completed backward sweep
        (-dt D_t sum_steps sum_cells |T| grad lambda^T dT_k grad c).  BackendError(GLIMS_E_USAGE) when no sweep has completed
        since the tangents were set."""
        K, L = int(getattr(self, "n_tangents", 0)), int(self.n_labels or 0)
        out = np.zeros((K, L))
        self._check(self.lib.glims_adjoint_tensor_gradient(self._h, K, L, _ptr(out, _dp)))
        return out

    def diffusion_tensor_info(self):
        """dict(present, n_cells, max_ratio): whether a tensor field is set and the largest lambda_max / lambda_min over its
        cells (1.0 without a field)."""
        out = np.zeros(2, dtype=np.int64)
        r = C.c_double(0.0)
        self._check(self.lib.glims_diffusion_tensor_info(self._h, _ptr(out, _i64p), C.byref(r)))
        return dict(present=bool(out[0]), n_cells=int(out[1]), max_ratio=r.value)

    def set_options(self, **kw):
        for k, v in kw.items():
            if not hasattr(self.options, k):
                raise KeyError(k)
            setattr(self.options, k, v)
        self._check(self.lib.glims_set_options(self._h, C.byref(self.options)))

    def set_dirichlet_u(self, dofs, values):
        dofs = np.ascontiguousarray(dofs, dtype=np.int64)
        values = _f64(np.broadcast_to(values, dofs.shape))
        self._check(self.lib.glims_set_dirichlet_u(self._h, len(dofs), _ptr(dofs, _i64p), _ptr(values, _dp)))

    def set_dirichlet_c(self, nodes, values):
        nodes = np.ascontiguousarray(nodes, dtype=np.int64)
        values = _f64(np.broadcast_to(values, nodes.shape))
        self._check(self.lib.glims_set_dirichlet_c(self._h, len(nodes), _ptr(nodes, _i64p), _ptr(values, _dp)))

    def set_rd_load(self, f):
        f = None if f is None else _f64(f, (self.n_nodes,))
        self._check(self.lib.glims_set_rd_load(self._h, _ptr(f, _dp)))

    def set_mech_load(self, f):
        f = None if f is None else _f64(np.asarray(f).reshape(-1), (self.n_nodes * self.dim,))
        self._check(self.lib.glims_set_mech_load(self._h, _ptr(f, _dp)))

    def setup(self, with_mechanics=True):
        self._check(self.lib.glims_setup(self._h, 1 if with_mechanics else 0))
        self.with_mechanics = bool(with_mechanics)   # (derive: the kinds that need u are refused without it)

    # -- state -----------------------------------------------------------------------------------
    def set_state(self, c, u=None):
        c = _f64(c, (self.n_nodes,))
        u = None if u is None else _f64(np.asarray(u).reshape(-1), (self.n_nodes * self.dim,))
        self._check(self.lib.glims_set_state(self._h, _ptr(c, _dp), _ptr(u, _dp)))

    def get_state(self, want_u=True):
        c = np.empty(self.n_nodes)
        u = np.empty(self.n_nodes * self.dim) if want_u else None
        self._check(self.lib.glims_get_state(self._h, _ptr(c, _dp), _ptr(u, _dp)))
        return c, u

    def step(self, n_steps=1):
        """Returns the status (GLIMS_OK / GLIMS_NOT_CONVERGED / GLIMS_NAN); raises on usage/HIP/RCCL errors."""
        return self._check(self.lib.glims_step(self._h, int(n_steps)), allow=(GLIMS_NOT_CONVERGED, GLIMS_NAN))

    def solve_mechanics(self):
        return self._check(self.lib.glims_solve_mechanics(self._h), allow=(GLIMS_NOT_CONVERGED, GLIMS_NAN))

    def stats(self):
        s = Stats()
        self._check(self.lib.glims_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    def reset_stats(self):
        self._check(self.lib.glims_reset_stats(self._h))

    # -- operator hooks --------------------------------------------------------------------------
    def apply(self, which, x, reps=1):
        """which: 0 A(c), 1 S, 2 M, 3 K_el, 4 G; 7 the matrix-free A(c) x; 8 the assembly sweep at c = x with b = 0,
        y = -1/2 (A(x) + S) x; 9 the quadratic-term pass with a = delta = x, y = -reps dt N(x) x; 10 = M x + rd_load as the
        stepping path's sweep forms it; 11 the quadratic-term pass prepared as the stepper prepares it from x and the state c,
        y = -reps dt N(x + c) (x - c) (needs a state); 12 (test hook) y_i = dinv_i x_i with the inverse diagonal the most
        recent assembly sweep left (1 on Dirichlet rows; GLIMS_E_USAGE before any sweep).  Hooks 9 and 11 return Dirichlet
        rows as 0 (glims_hip.h).
        Returns (y, ms_total)."""
        d = self.dim
        nin = self.n_nodes * (d if which == 3 else 1)
        nout = self.n_nodes * (d if which in (3, 4) else 1)
        x = _f64(np.asarray(x).reshape(-1), (nin,))
        y = np.empty(nout)
        ms = C.c_double(0.0)
        self._check(self.lib.glims_apply(self._h, int(which), _ptr(x, _dp), _ptr(y, _dp), int(reps), C.byref(ms)))
        return y, ms.value

    def rd_residual(self, c, c_prev):
        c = _f64(c, (self.n_nodes,))
        cp = _f64(c_prev, (self.n_nodes,))
        R = np.empty(self.n_nodes)
        self._check(self.lib.glims_rd_residual(self._h, _ptr(c, _dp), _ptr(cp, _dp), _ptr(R, _dp)))
        return R

    def peek_partials(self):
        """(sum of |row|^2, sum of the second right-hand side's) over the slice sums the last sweep or quadratic-term pass left
        (glims_peek_partials)."""
        a = np.zeros(2)
        self._check(self.lib.glims_peek_partials(self._h, _ptr(a, _dp)))
        return a

    def numbering(self):
        """old2new: internal index of every node of the caller's numbering."""
        a = np.empty(self.n_nodes, dtype=np.int32)
        self._check(self.lib.glims_get_numbering(self._h, _ptr(a, _i32p)))
        return a

    def pattern_checksum(self):
        """Thirteen 64-bit hashes of the device-resident discretisation structures (see glims_pattern_checksum)."""
        a = (C.c_uint64 * 13)()
        self._check(self.lib.glims_pattern_checksum(self._h, a))
        return [int(v) for v in a]

    def snapshot_save(self):
        sid = C.c_int64(-1)
        self._check(self.lib.glims_snapshot_save(self._h, C.byref(sid)))
        return int(sid.value)

    def snapshot_load(self, sid):
        c = np.empty(self.n_nodes)
        self._check(self.lib.glims_snapshot_load(self._h, int(sid), _ptr(c, _dp)))
        return c

    def snapshot_mechanics(self, sid):
        u = np.empty(self.n_nodes * self.dim)
        st = self._check(self.lib.glims_snapshot_mechanics(self._h, int(sid), _ptr(u, _dp)),
                         allow=(GLIMS_NOT_CONVERGED, GLIMS_NAN))
        return u, st

    def snapshot_clear(self):
        self._check(self.lib.glims_snapshot_clear(self._h))

    def project(self, rhs, rtol=1e-12):
        """Solve M x = rhs for rhs [n_nodes] or [n_nodes, k] (L2 projection onto P1 given integrated loads)."""
        rhs = np.asarray(rhs, dtype=np.float64)
        k = 1 if rhs.ndim == 1 else rhs.shape[1]
        r = _f64(rhs.reshape(self.n_nodes, k))
        x = np.empty_like(r)
        self._check(self.lib.glims_project(self._h, _ptr(r, _dp), _ptr(x, _dp), int(k), float(rtol)))
        return x.reshape(rhs.shape)

    # -- derived fields (glims_derive) -----------------------------------------------------------------
    def derive(self, kind, snapshot=None, c=None, u=None, rtol=1e-12, fetch=True):
        """One derived field of a step, computed on the device (glims_derive).  ``kind``: a name of DERIVE_KINDS or its
        number.  Source: ``snapshot`` (an id of snapshot_save; the displacement is solved on the device where the kind needs
        it), host arrays ``c`` [n_nodes] / ``u`` [n_nodes, dim] in the caller's node order (either may be None where the kind
        needs none), or neither: the handle's current c and U as they stand.  Returns the nodal field ([n_nodes], tensors
        [n_nodes, dim, dim]); with fetch=False nothing is copied back and None is returned -- the result stays on the device
        for ``Sampler.apply('derived')``.  ``last_derive_status`` holds the call's status: GLIMS_NOT_CONVERGED (a solve stopped
        at its iteration cap: the field comes from what it reached, as solve_mechanics / snapshot_mechanics hand back their
        displacement) does not raise, GLIMS_NAN and the refusals do."""
        k = DERIVE_KINDS[kind] if isinstance(kind, str) else int(kind)
        if snapshot is not None and (c is not None or u is not None):
            raise ValueError("derive: give a snapshot or host arrays, not both")
        if snapshot is not None:
            src = int(snapshot)
        elif c is not None or u is not None:
            src = DERIVE_HOST
            c = None if c is None else _f64(c, (self.n_nodes,))
            u = None if u is None else _f64(np.asarray(u, dtype=np.float64).reshape(-1), (self.n_nodes * self.dim,))
        else:
            src = DERIVE_CURRENT
        out = None
        if fetch:
            out = np.empty((self.n_nodes, self.dim, self.dim) if k in (0, 1) else (self.n_nodes,))
        st = self.lib.glims_derive(self._h, k, src, _ptr(c, _dp), _ptr(u, _dp), float(rtol), _ptr(out, _dp))
        if st >= 0:   # (a refused call changes nothing: the earlier result stays where it was)
            self._derived_ncomp = self.dim * (self.dim + 1) // 2 if k in (0, 1) else 1
        self.last_derive_status = st
        self._check(st, allow=(GLIMS_NOT_CONVERGED,))
        return out

    def derive_info(self):
        """Cumulative counters of derive(): cell passes, mass solves, elastic solves, hits of the projected-stress cache."""
        a = np.zeros(4, dtype=np.int64)
        self._check(self.lib.glims_derive_info(self._h, _ptr(a, _i64p)))
        return dict(zip(("cell_passes", "mass_solves", "elastic_solves", "cache_hits"), (int(v) for v in a)))

    # -- volumes and centres of mass per label (glims_observe) ---------------------------------------------
    def observe(self, queries, snapshots=None, c=None, u=None, deformed=False, scale=1.0):
        """Measure and first moments of the queries per label, computed on the device (glims_observe).  ``queries``: a list of
        (kind, level, smooth) -- kind a name of OBSERVE_KINDS or its number; level and smooth may be left out where the kind
        reads none.  Source: ``snapshots`` (ids of snapshot_save, one cell pass each), host arrays ``c`` [n_nodes] (and ``u``
        [n_nodes, dim] when ``deformed``) in the caller's node order, or neither: the handle's current c and U as they stand.
        ``deformed``: the configuration x = X + scale u (a snapshot's displacement is solved on the device).  Returns
        [n_src, n_q, n_labels, 1 + dim] = (V, M_0 ..); more than OBSERVE_MAX_QUERIES queries go in several calls.
        ``last_observe_status`` holds the worst status of the calls: GLIMS_NOT_CONVERGED does not raise, GLIMS_NAN and the
        refusals do."""
        qs = []
        for q in queries:
            q = tuple(q) if isinstance(q, (tuple, list)) else (q,)
            kind = OBSERVE_KINDS[q[0]] if isinstance(q[0], str) else int(q[0])
            qs.append((kind, float(q[1]) if len(q) > 1 else 0.0, float(q[2]) if len(q) > 2 else 1.0))
        if snapshots is not None and (c is not None or u is not None):
            raise ValueError("observe: give snapshots or host arrays, not both")
        if snapshots is not None:
            src = np.ascontiguousarray(np.atleast_1d(snapshots), dtype=np.int64)
        elif c is not None or u is not None:
            src = np.array([DERIVE_HOST], dtype=np.int64)
            c = None if c is None else _f64(c, (self.n_nodes,))
            u = None if u is None else _f64(np.asarray(u, dtype=np.float64).reshape(-1), (self.n_nodes * self.dim,))
        else:
            src = np.array([DERIVE_CURRENT], dtype=np.int64)
        if self.n_labels is None:
            raise BackendError(GLIMS_E_USAGE, "observe before set_materials")
        out = np.zeros((len(src), len(qs), self.n_labels, 1 + self.dim))
        worst = GLIMS_OK
        for q0 in range(0, max(len(qs), 1), OBSERVE_MAX_QUERIES):
            part = qs[q0:q0 + OBSERVE_MAX_QUERIES]
            arr = (Observable * max(len(part), 1))()
            for k, (kind, level, smooth) in enumerate(part):
                arr[k].kind, arr[k].level, arr[k].smooth = kind, level, smooth
            res = np.zeros((len(src), len(part), self.n_labels, 1 + self.dim))
            st = self.lib.glims_observe(self._h, len(src), _ptr(src, _i64p), _ptr(c, _dp), _ptr(u, _dp),
                                        1 if deformed else 0, float(scale), len(part), arr, _ptr(res, _dp))
            self.last_observe_status = st
            self._check(st, allow=(GLIMS_NOT_CONVERGED,))
            worst = max(worst, st)
            out[:, q0:q0 + len(part)] = res
        self.last_observe_status = worst
        return out

    def observe_info(self):
        """Cumulative counters of observe(): cell passes, elastic solves, sources observed."""
        a = np.zeros(4, dtype=np.int64)
        self._check(self.lib.glims_observe_info(self._h, _ptr(a, _i64p)))
        return dict(zip(("cell_passes", "elastic_solves", "sources"), (int(v) for v in a[:3])))

    # -- discrete adjoint (glims_adjoint_*) -----------------------------------------------------------
    def adjoint_record(self, on=True):
        """on: clear the trajectory, keep the current state as c_0 and a device copy of c_n after every converged step."""
        self._check(self.lib.glims_adjoint_record(self._h, 1 if on else 0))

    def adjoint_gradient(self, terms, n_labels=None, want_dc0=True, elastic=False):
        """terms: iterable of dicts {step, kind ('c_l2' | 'c_thresh' | 'u_l2' or MISFIT_*), target, weight=1, level=0,
        smooth=1}; targets in the caller's node order ([n_nodes] or [n_nodes, dim]).  Image-space terms go in the same list:
        {step, kind ('img_l2' | 'img_thresh'), sampler (a :class:`Sampler` of this handle), target ([n_points], any shape;
        NaN = not observed), pweight=None, weight=1, level=0, smooth=1}; they are stored on the device (set_image_terms) and
        re-sent only when they differ from what the handle holds.  A displacement image term {step, kind: 'img_u_l2',
        sampler, target [n_points, dim], pweight=None, weight=1, scale=1, cweight=None} compares the sampled displacement
        with a warp field or landmark displacements (set_displacement_image_terms).  An image term with ``deformed=True`` observes the DEFORMED
        configuration x = X + scale u_k and carries its own points instead of a sampler: {..., deformed=True, scale=1.0,
        grid=(origin, spacing, size) or points=[n_points, dim]} (set_deformed_image_terms; the gradient through the location).
        Returns (J, dJ/dD [n_labels], dJ/drho, dJ/dgamma, dJ/dc0 [n_nodes] or None); with elastic=True (glims_adjoint_gradient_full)
        (J, dJ/dD, dJ/drho, dJ/dgamma, dJ/dc0, dJ/dE [n_labels], dJ/dnu [n_labels]).  The library writes one entry per label
        of the last set_materials: n_labels, when given, must be that count (ValueError otherwise, before any call)."""
        if self.n_labels is None:
            raise ValueError("adjoint_gradient before set_materials")
        if n_labels is not None and int(n_labels) != self.n_labels:
            raise ValueError("adjoint_gradient: n_labels = %d, but set_materials gave %d labels" % (n_labels, self.n_labels))
        n_labels = self.n_labels
        terms = self._split_terms(terms)
        arr, keep = self._misfit_array(terms)   # (keep: the target arrays the structs point into)
        J = C.c_double(0.0)
        out = [np.zeros(int(n_labels)) for _ in range(5 if elastic else 3)]
        dc0 = np.zeros(self.n_nodes) if want_dc0 else None
        if elastic:
            self._check(self.lib.glims_adjoint_gradient_full(self._h, len(terms), arr, C.byref(J),
                                                             *[_ptr(a, _dp) for a in out[:3]], _ptr(dc0, _dp),
                                                             _ptr(out[3], _dp), _ptr(out[4], _dp)))
            self._warn_folded()
            return (J.value, out[0], out[1], out[2], dc0, out[3], out[4])
        self._check(self.lib.glims_adjoint_gradient(self._h, len(terms), arr, C.byref(J), *[_ptr(a, _dp) for a in out],
                                                    _ptr(dc0, _dp)))
        self._warn_folded()
        return (J.value, out[0], out[1], out[2], dc0)

    # -- image-space misfit terms (glims_adjoint_image_*) ---------------------------------------------
    @staticmethod
    def _image_key(t):
        """What identifies a stored image term: its scalars and the IDENTITY of its target / pweight arrays."""
        sm = t["sampler"]
        return (int(t["step"]), _IMAGE_KINDS.get(t["kind"], t["kind"]), int(getattr(sm, "id", sm)),
                float(t.get("level", 0.0)), float(t.get("smooth", 1.0)), float(t.get("weight", 1.0)),
                id(t["target"]), id(t.get("pweight")))

    def set_image_terms(self, terms, _from_list=False):
        """glims_adjoint_image_terms: replace the handle's stored image terms (an empty list clears them).  The target and
        pweight arrays are copied to the device once; every later adjoint_gradient / adjoint_hessian adds these terms
        (until a term list that carries image terms of its own replaces them)."""
        terms = list(terms)
        arr = (ImageMisfit * max(1, len(terms)))()
        keep = []
        for k, t in enumerate(terms):
            sm = t["sampler"]
            if isinstance(sm, Sampler) and sm.handle is not self:
                raise ValueError("image term %d: its sampler belongs to another handle" % k)
            kind = _IMAGE_KINDS.get(t["kind"], t["kind"])
            n = sm.n_points if isinstance(sm, Sampler) else None
            tg = _f64(np.asarray(t["target"], dtype=np.float64).reshape(-1), None if n is None else (n,))
            q = t.get("pweight")
            if q is not None:
                q = _f64(np.asarray(q, dtype=np.float64).reshape(-1), tg.shape)
            keep.append((tg, q))
            arr[k] = ImageMisfit(int(t["step"]), int(getattr(sm, "id", sm)), int(kind), float(t.get("level", 0.0)),
                                 float(t.get("smooth", 1.0)), float(t.get("weight", 1.0)), _ptr(tg, _dp), _ptr(q, _dp))
        self._check(self.lib.glims_adjoint_image_terms(self._h, len(terms), arr))
        # (the caller's arrays are kept alive: their identity is what _split_terms compares)
        self._image_terms = [(self._image_key(t), t["target"], t.get("pweight")) for t in terms]
        self._image_from_list = bool(_from_list)

    def image_term_info(self, k):
        """(sampler id, number of points, number of observed points) of stored image term k."""
        out = np.zeros(3, dtype=np.int64)
        self._check(self.lib.glims_adjoint_image_info(self._h, int(k), _ptr(out, _i64p)))
        return tuple(int(v) for v in out)

    # -- displacement-image misfit terms (glims_adjoint_displacement_image_*) --------------------------
    def _displacement_key(self, t):
        """What identifies a stored displacement image term: its scalars and the IDENTITY of its target / pweight arrays."""
        sm = t["sampler"]
        cw = t.get("cweight")
        cw = None if cw is None else tuple(float(v) for v in np.ravel(cw))
        return (int(t["step"]), int(getattr(sm, "id", sm)), float(t.get("weight", 1.0)), float(t.get("scale", 1.0)), cw,
                id(t["target"]), id(t.get("pweight")))

    def set_displacement_image_terms(self, terms, _from_list=False):
        """glims_adjoint_displacement_image_terms: replace the handle's stored displacement image terms (an empty list
        clears them).  Each term: {step, kind: 'img_u_l2', sampler (a fixed :class:`Sampler` of this handle), target
        [n_points, dim] (NaN = not observed), pweight=None, weight=1, scale=1, cweight=None ([dim] component weights, default
        1)}.  J = 1/2 weight sum_p q_p sum_a cweight_a (scale (P u_k)_pa - target_pa)^2.  Target and pweight are copied to the
        device once; every later adjoint_gradient / adjoint_hessian adds these terms."""
        terms = list(terms)
        arr = (DisplacementImageMisfit * max(1, len(terms)))()
        keep = []
        for k, t in enumerate(terms):
            sm = t["sampler"]
            if isinstance(sm, Sampler) and sm.handle is not self:
                raise ValueError("displacement image term %d: its sampler belongs to another handle" % k)
            tg = np.asarray(t["target"], dtype=np.float64)
            if tg.size % self.dim or (isinstance(sm, Sampler) and tg.size != sm.n_points * self.dim):
                raise ValueError("displacement image term %d: target has %d values, not n_points x %d" % (k, tg.size, self.dim))
            tg = _f64(tg.reshape(-1, self.dim))
            q = t.get("pweight")
            if q is not None:
                q = _f64(np.asarray(q, dtype=np.float64).reshape(-1), (tg.shape[0],))
            cw = t.get("cweight")
            cw = np.ones(self.dim) if cw is None else np.asarray(cw, dtype=np.float64).reshape(-1)
            if cw.size != self.dim:
                raise ValueError("displacement image term %d: cweight has %d entries, the mesh %d dimensions"
                                 % (k, cw.size, self.dim))
            keep.append((tg, q))
            m = DisplacementImageMisfit()
            m.step, m.sampler = int(t["step"]), int(getattr(sm, "id", sm))
            m.weight, m.scale = float(t.get("weight", 1.0)), float(t.get("scale", 1.0))
            for a in range(3):
                m.cweight[a] = float(cw[a]) if a < self.dim else 0.0
            m.target, m.pweight = _ptr(tg, _dp), _ptr(q, _dp)
            arr[k] = m
        self._check(self.lib.glims_adjoint_displacement_image_terms(self._h, len(terms), arr))
        # (the caller's arrays are kept alive: their identity is what _split_terms compares)
        self._displacement_terms = [(self._displacement_key(t), t["target"], t.get("pweight")) for t in terms]
        self._displacement_from_list = bool(_from_list)

    def displacement_image_term_info(self, k):
        """(sampler id, number of points, number of observed points) of stored displacement image term k."""
        out = np.zeros(3, dtype=np.int64)
        self._check(self.lib.glims_adjoint_displacement_image_info(self._h, int(k), _ptr(out, _i64p)))
        return tuple(int(v) for v in out)

    # -- image terms of the deformed configuration (glims_adjoint_deformed_image_*) -------------------
    @staticmethod
    def _deformed_key(t):
        pts = t.get("points")
        grid = t.get("grid")
        gk = None if grid is None else tuple(tuple(float(v) for v in np.ravel(a)) for a in grid)
        return (int(t["step"]), _IMAGE_KINDS.get(t["kind"], t["kind"]), float(t.get("level", 0.0)),
                float(t.get("smooth", 1.0)), float(t.get("weight", 1.0)), float(t.get("scale", 1.0)), gk, id(pts),
                id(t["target"]), id(t.get("pweight")))

    def set_deformed_image_terms(self, terms, _from_list=False):
        """glims_adjoint_deformed_image_terms: replace the handle's stored DEFORMED image terms (an empty list clears them).
        Each term: {step, kind ('img_l2' | 'img_thresh'), target, pweight=None, weight=1, level=0, smooth=1, scale=1.0} and
        either grid=(origin, spacing, size) (target in the order of an image array [z,] y, x) or points=[n_points, dim].
        Points, target and pweight are copied to the device once; every later adjoint_gradient locates the points in the mesh
        at X + scale u_k and adds the term with its gradient through the location."""
        terms = list(terms)
        arr = (DeformedImageMisfit * max(1, len(terms)))()
        keep = []
        for k, t in enumerate(terms):
            kind = _IMAGE_KINDS.get(t["kind"], t["kind"])
            m = DeformedImageMisfit()
            m.step, m.kind = int(t["step"]), int(kind)
            m.level, m.smooth = float(t.get("level", 0.0)), float(t.get("smooth", 1.0))
            m.weight, m.scale = float(t.get("weight", 1.0)), float(t.get("scale", 1.0))
            if t.get("points") is not None:
                xyz = _f64(np.asarray(t["points"], dtype=np.float64).reshape(-1, self.dim))
                n = xyz.shape[0]
                m.n_points, m.xyz = n, _ptr(xyz, _dp)
                keep.append(xyz)
            elif t.get("grid") is not None:
                origin, spacing, size = t["grid"]
                size = [int(v) for v in np.ravel(size)]
                if not (len(size) == len(np.ravel(origin)) == len(np.ravel(spacing)) == self.dim):
                    raise ValueError("deformed image term %d: the grid has not %d axes" % (k, self.dim))
                for a in range(self.dim):
                    m.origin[a], m.spacing[a], m.size[a] = float(np.ravel(origin)[a]), float(np.ravel(spacing)[a]), size[a]
                n = int(np.prod(size)) if min(size) > 0 else None
                m.n_points, m.xyz = 0, None
            else:
                raise ValueError("deformed image term %d: needs grid=(origin, spacing, size) or points" % k)
            tg = t["target"]
            if tg is not None:
                tg = _f64(np.asarray(tg, dtype=np.float64).reshape(-1))
                if n is not None and tg.shape != (n,):
                    raise ValueError("deformed image term %d: target has %d values, the term %d points" % (k, tg.size, n))
            q = t.get("pweight")
            if q is not None:
                q = _f64(np.asarray(q, dtype=np.float64).reshape(-1))
                if n is not None and q.shape != (n,):
                    raise ValueError("deformed image term %d: pweight has %d values, the term %d points" % (k, q.size, n))
            keep.append((tg, q))
            m.target, m.pweight = _ptr(tg, _dp), _ptr(q, _dp)
            arr[k] = m
        self._check(self.lib.glims_adjoint_deformed_image_terms(self._h, len(terms), arr))
        del keep
        self._deformed_terms = [(self._deformed_key(t), t) for t in terms]   # (the dicts keep the compared arrays alive)
        self._deformed_from_list = bool(_from_list)
        self._warned_folded = False

    def deformed_image_term_info(self, k):
        """Stored deformed image term k at its LAST evaluation: a dict n_points, found, observed, folded (cells of the mesh
        at X + scale u_k whose determinant ratio is not > 0), min_ratio; found / observed / folded are -1 before the first."""
        out = np.zeros(4, dtype=np.int64)
        mr = C.c_double(1.0)
        self._check(self.lib.glims_adjoint_deformed_image_info(self._h, int(k), _ptr(out, _i64p), C.byref(mr)))
        return dict(n_points=int(out[0]), found=int(out[1]), observed=int(out[2]), folded=int(out[3]), min_ratio=mr.value)

    def has_deformed_image_terms(self):
        return bool(self._deformed_terms)

    def _warn_empty_com(self):
        """Once per stored list: the last gradient call found the measure of a centre-of-mass term empty."""
        if getattr(self, "_warned_empty_com", True):
            return
        for k, key in enumerate(self._observable_terms):
            if isinstance(key[5], tuple) and self.observable_term_info(k)["empty"]:
                import warnings
                warnings.warn("centre-of-mass term %d: its measure was empty (V not > 0) at the last evaluation; the term "
                              "contributed J = 0 and no gradient there" % k, RuntimeWarning, stacklevel=4)
                self._warned_empty_com = True
                return

    def _warn_folded(self):
        """Once per stored list: the last gradient call located points in a mesh with folded cells."""
        self._warn_empty_com()
        self._warn_folded_volumes()
        if self._warned_folded or not self._deformed_terms:
            return
        for k in range(len(self._deformed_terms)):
            info = self.deformed_image_term_info(k)
            if info["folded"] > 0:
                import warnings
                warnings.warn("deformed image term %d: %d cells of the displaced mesh are folded (smallest determinant ratio "
                              "min_ratio = %.3g); points in such cells carry no gradient through their location"
                              % (k, info["folded"], info["min_ratio"]), RuntimeWarning, stacklevel=3)
                self._warned_folded = True
                return

    def _warn_folded_volumes(self):
        """Once per stored list: the last gradient call measured a deformed volume term on a mesh with folded cells."""
        if getattr(self, "_warned_folded_volumes", True):
            return
        for k, key in enumerate(self._observable_terms):
            if not key[-2]:
                continue
            info = self.observable_term_info2(k)
            if info["folded"] > 0:
                import warnings
                warnings.warn("deformed volume term %d: %d counted cells of the displaced mesh are folded (smallest volume "
                              "ratio min_ratio = %.3g); they count negatively" % (k, info["folded"], info["min_ratio"]),
                              RuntimeWarning, stacklevel=4)
                self._warned_folded_volumes = True
                return

    # -- volume misfit terms (glims_adjoint_observable_*) ----------------------------------------------
    @staticmethod
    def _observable_key(t):
        """What identifies a stored volume term: its scalars and the counted labels."""
        lab = t.get("labels")
        kind = t.get("observable", "smooth")
        deformed = bool(t.get("deformed", False))
        com = t.get("kind") == "obs_com"
        return (int(t["step"]), OBSERVE_KINDS.get(kind, kind), float(t.get("level", 0.0)), float(t.get("smooth", 1.0)),
                float(t.get("weight", 1.0)),
                ("com",) + tuple(float(v) for v in np.ravel(t["target"])) if com else float(t["target"]),
                None if lab is None else tuple(bool(v) for v in np.ravel(lab)),
                deformed, float(t.get("scale", 1.0)) if deformed else 1.0)

    def set_observable_terms(self, terms, _from_list=False):
        """glims_adjoint_observable_terms: replace the handle's stored volume terms (an empty list clears them).  Each term:
        {step, observable ('mass' | 'sharp' | 'smooth' or GLIMS_OBSERVE_*), target, weight=1, level=0, smooth=1, labels=None,
        deformed=False, scale=1.0} with J = 1/2 weight (V - target)^2, V the measure observe() returns for (observable, level,
        smooth) on recorded step ``step``, summed over the labels whose entry of ``labels`` ([n_labels], truthy = counted) is
        set, or over the whole domain -- in the reference configuration, or with ``deformed=True`` of the cells at
        X + scale u_k (observe(..., deformed=True, scale)); the gradient of such a term goes through u_k as well, so it reaches
        the coupling, E and nu (a handle with mechanics; first order only).  Every later adjoint_gradient / adjoint_hessian
        adds these terms.

        A dict with kind='obs_com' is a CENTRE-OF-MASS term (glims_adjoint_observable_terms3): J = 1/2 weight |M / V - target|^2
        with target = [x, y(, z)] and V, M the measure and first moments observe() returns for the same query, labels and
        configuration.  Where V is not > 0 at an evaluation the term contributes nothing there (observable_term_info(k)
        ['empty']); first order only.  A list without such a term goes through glims_adjoint_observable_terms2 as before."""
        terms = list(terms)
        any_com = any(t.get("kind") == "obs_com" for t in terms)
        arr = ((ObservableMisfit3 if any_com else ObservableMisfit2) * max(1, len(terms)))()
        keep = []
        for k, t in enumerate(terms):
            kind = t.get("observable", "smooth")
            kind = OBSERVE_KINDS[kind] if isinstance(kind, str) else int(kind)
            lab = t.get("labels")
            if lab is not None:
                if self.n_labels is None:
                    raise BackendError(GLIMS_E_USAGE, "set_observable_terms before set_materials")
                lab = np.ascontiguousarray(np.asarray(lab).reshape(-1) != 0, dtype=np.uint8)
                if lab.shape != (self.n_labels,):
                    raise ValueError("volume term %d: labels has %d entries, set_materials gave %d labels"
                                     % (k, lab.size, self.n_labels))
                keep.append(lab)
            deformed = bool(t.get("deformed", False))
            com = t.get("kind") == "obs_com"
            fields = (int(t["step"]), kind, float(t.get("level", 0.0)), float(t.get("smooth", 1.0)),
                      float(t.get("weight", 1.0)), 0.0 if com else float(t["target"]),
                      None if lab is None else lab.ctypes.data_as(C.POINTER(C.c_uint8)),
                      1 if deformed else 0, float(t.get("scale", 1.0)) if deformed else 1.0)
            if any_com:
                tx = np.zeros(3)
                if com:
                    x = np.asarray(t["target"], dtype=np.float64).reshape(-1)
                    if x.shape != (self.dim,):
                        raise ValueError("centre-of-mass term %d: target has %d entries, the mesh has dimension %d"
                                         % (k, x.size, self.dim))
                    tx[:self.dim] = x
                arr[k] = ObservableMisfit3(*fields, int(t.get("moment", 1)) if com else 0, (C.c_double * 3)(*tx))
            else:
                arr[k] = ObservableMisfit2(*fields)
        if any_com:
            self._check(self.lib.glims_adjoint_observable_terms3(self._h, len(terms), arr))
        else:
            self._check(self.lib.glims_adjoint_observable_terms2(self._h, len(terms), arr))
        del keep
        self._observable_terms = [self._observable_key(t) for t in terms]
        self._observable_from_list = bool(_from_list)
        self._warned_folded_volumes = not any(key[-2] for key in self._observable_terms)
        self._warned_empty_com = not any_com

    def has_com_terms(self):
        return any(isinstance(key[5], tuple) for key in getattr(self, "_observable_terms", []))

    def observable_term_info3(self, k):
        """glims_adjoint_observable_info3: observable_term_info2(k) with empty (the LAST evaluation found the measure of this
        centre-of-mass term not > 0) and com ([dim]: the last M / V; NaN before the first evaluation, when empty and for a
        volume term)."""
        out = np.zeros(4, dtype=np.int64)
        V, mr = C.c_double(0.0), C.c_double(0.0)
        com = np.full(3, np.nan)
        self._check(self.lib.glims_adjoint_observable_info3(self._h, int(k), _ptr(out, _i64p), C.byref(V), C.byref(mr),
                                                            _ptr(com, _dp)))
        return dict(counted=int(out[0]), cut=int(out[1]), folded=int(out[2]), V=V.value, min_ratio=mr.value,
                    empty=bool(out[3]), com=com[:self.dim].copy())

    def has_deformed_volume_terms(self):
        return any(key[-2] for key in getattr(self, "_observable_terms", []))

    def observable_term_info2(self, k):
        """glims_adjoint_observable_info2: observable_term_info(k) with folded (the counted cells of the displaced mesh whose
        volume ratio vol(y) / vol(X) is not > 0 at the LAST evaluation; -1 before the first and for a reference term) and
        min_ratio (the smallest ratio over the counted cells; NaN before the first evaluation and for a reference term)."""
        out = np.zeros(4, dtype=np.int64)
        V, mr = C.c_double(0.0), C.c_double(0.0)
        self._check(self.lib.glims_adjoint_observable_info2(self._h, int(k), _ptr(out, _i64p), C.byref(V), C.byref(mr)))
        return dict(counted=int(out[0]), cut=int(out[1]), folded=int(out[2]), V=V.value, min_ratio=mr.value)

    def observable_term_info(self, k):
        """Stored volume term k: a dict counted (cells of the counted labels), cut (cells the level set cut at the LAST
        evaluation; -1 before the first and for 'mass' / 'smooth'), V (the last measure; NaN before the first).  A
        centre-of-mass term gains com and empty (observable_term_info3)."""
        keys = getattr(self, "_observable_terms", [])
        if 0 <= int(k) < len(keys) and isinstance(keys[int(k)][5], tuple):
            info = self.observable_term_info3(k)
            return dict(counted=info["counted"], cut=info["cut"], V=info["V"], com=info["com"], empty=info["empty"])
        out = np.zeros(2, dtype=np.int64)
        V = C.c_double(0.0)
        self._check(self.lib.glims_adjoint_observable_info(self._h, int(k), _ptr(out, _i64p), C.byref(V)))
        return dict(counted=int(out[0]), cut=int(out[1]), V=V.value)

    def _split_terms(self, terms):
        """The nodal terms of a mixed list; its image terms become the handle's stored lists -- the fixed ones and those with
        deformed=True -- and its volume terms (kind 'obs_volume') the third, each re-sent only on a change."""
        terms = list(terms)
        volume = [t for t in terms if t["kind"] in ("obs_volume", "obs_com")]
        if volume or getattr(self, "_observable_from_list", False):
            if [self._observable_key(t) for t in volume] != getattr(self, "_observable_terms", []):
                self.set_observable_terms(volume, _from_list=True)
            terms = [t for t in terms if t["kind"] not in ("obs_volume", "obs_com")]
        warp = [t for t in terms if t["kind"] == "img_u_l2"]
        if warp or getattr(self, "_displacement_from_list", False):
            if [self._displacement_key(t) for t in warp] != [k for k, _, _ in self._displacement_terms]:
                self.set_displacement_image_terms(warp, _from_list=True)
            terms = [t for t in terms if t["kind"] != "img_u_l2"]
        moving = [t for t in terms if _IMAGE_KINDS.get(t["kind"]) is not None and t.get("deformed")]
        if moving or getattr(self, "_deformed_from_list", False):
            if [self._deformed_key(t) for t in moving] != [k for k, _ in self._deformed_terms]:
                self.set_deformed_image_terms(moving, _from_list=True)
            terms = [t for t in terms if not (_IMAGE_KINDS.get(t["kind"]) is not None and t.get("deformed"))]
        image = [t for t in terms if _IMAGE_KINDS.get(t["kind"]) is not None]
        if not image and not getattr(self, "_image_from_list", False):
            return terms   # (terms stored by set_image_terms itself stay)
        if [self._image_key(t) for t in image] != [k for k, _, _ in self._image_terms]:
            self.set_image_terms(image, _from_list=True)
        return [t for t in terms if _IMAGE_KINDS.get(t["kind"]) is None]

    def _misfit_array(self, terms):
        """ctypes array of glims_misfit for the term dicts, and the target arrays it points into (keep them alive)."""
        kinds = {"c_l2": MISFIT_C_L2, "c_thresh": MISFIT_C_THRESH, "u_l2": MISFIT_U_L2}
        arr = (Misfit * max(1, len(terms)))()
        keep = []
        for k, t in enumerate(terms):
            kind = kinds.get(t["kind"], t["kind"])
            n = self.n_nodes * (self.dim if kind == MISFIT_U_L2 else 1)
            tg = _f64(np.asarray(t["target"]).reshape(-1), (n,))
            keep.append(tg)
            arr[k] = Misfit(int(t["step"]), int(kind), float(t.get("level", 0.0)), float(t.get("smooth", 1.0)),
                            float(t.get("weight", 1.0)), _ptr(tg, _dp))
        return arr, keep

    def adjoint_hessian(self, terms, directions, n_labels=None, collective=False):
        """glims_adjoint_hessian: J, the gradient and the Hessian-vector products of the recorded run for the misfit ``terms``
        (as in adjoint_gradient) along 1 .. 8 ``directions``, each a dict {'D', 'rho', 'gamma' ([n_labels] or a scalar for
        every label), 'c0' ([n_nodes], caller's order)} whose missing keys are 0.  Returns a dict {'J', 'D', 'rho', 'gamma',
        'c0' (the gradient, as adjoint_gradient), 'hv_D', 'hv_rho', 'hv_gamma' ([n_dir, n_labels]), 'hv_c0' ([n_dir, n_nodes]),
        'stats' (tangent-linear / second-order PCG iterations, extra elastic solves, ms)}.
        collective=True calls glims_adjoint_hessian_spmd: the same call on one GPU, and on a partitioned handle the
        collective one (every rank with the same terms and directions; 'c0' entries in the local numbering, ghosts of
        'hv_c0' are 0).  The default keeps refusing partitioned handles.  E and nu are first order here: a direction keyed
        'E' or 'nu' is a ValueError (adjoint_hessian_full takes them)."""
        return self._adjoint_hessian(terms, directions, n_labels, collective, False)

    def adjoint_hessian_full(self, terms, directions, n_labels=None):
        """glims_adjoint_hessian_full (one GPU): adjoint_hessian whose directions take 'E' and 'nu' ([n_labels] or a scalar
        for every label) as well -- the exact second-order elastic adjoint -- and whose result gains 'E', 'nu' (dJ/dE, dJ/dnu
        as adjoint_gradient(elastic=True)) and 'hv_E', 'hv_nu' ([n_dir, n_labels]).  No elastic solve is added
        ('stats'['mech_solves'] as adjoint_hessian).  A partitioned handle is refused by the library (BackendError,
        GLIMS_E_USAGE), and so is a direction in 'E' / 'nu' on a handle set up without mechanics; without such a direction
        that handle gets the call with NULL hv_E / hv_nu (no displacement term can exist there: the products are 0)."""
        return self._adjoint_hessian(terms, directions, n_labels, False, True)

    def _adjoint_hessian(self, terms, directions, n_labels, collective, elastic):
        if self.n_labels is None:
            raise ValueError("adjoint_hessian before set_materials")
        if n_labels is not None and int(n_labels) != self.n_labels:
            raise ValueError("adjoint_hessian: n_labels = %d, but set_materials gave %d labels" % (n_labels, self.n_labels))
        L, n = self.n_labels, self.n_nodes
        directions = list(directions)
        P = len(directions)
        terms = list(terms)
        if not elastic and any(k in d for d in directions for k in ("E", "nu")):
            raise ValueError("adjoint_hessian: E / nu are first order here; directions in 'E' / 'nu' go to adjoint_hessian_full")
        if any(_IMAGE_KINDS.get(t["kind"]) is not None and t.get("deformed") for t in terms):
            raise NotImplementedError("adjoint_hessian: second order through the location of a deformed image term is not "
                                      "built (glims_adjoint_hessian refuses while such a term is stored)")
        if any(t["kind"] == "obs_com" for t in terms):
            raise NotImplementedError("adjoint_hessian: second order of a centre-of-mass term (the quotient M / V) is not "
                                      "built (glims_adjoint_hessian refuses while such a term is stored)")
        if any(t["kind"] == "obs_volume" and t.get("deformed") for t in terms):
            raise NotImplementedError("adjoint_hessian: second order through the displacement of a deformed volume term is "
                                      "not built (glims_adjoint_hessian refuses while such a term is stored)")
        if any(t["kind"] == "obs_volume" and OBSERVE_KINDS.get(t.get("observable", "smooth"), t.get("observable")) == 1
               for t in terms):
            raise NotImplementedError("adjoint_hessian: a sharp volume term is piecewise smooth, with jumps in its second "
                                      "derivative; second order is built for 'mass' and 'smooth' (glims_adjoint_hessian "
                                      "refuses while such a term is stored)")
        terms = self._split_terms(terms)
        arr, keep = self._misfit_array(terms)

        def table(key, size):
            if not any(key in d for d in directions):
                return None
            t = np.zeros((max(1, P), size))
            for p, d in enumerate(directions):
                if d.get(key) is not None:
                    t[p] = np.broadcast_to(np.asarray(d[key], dtype=np.float64), (size,))
            return _f64(t)

        dirs = [table("D", L), table("rho", L), table("gamma", L), table("c0", n)]
        J = C.c_double(0.0)
        g = [np.zeros(L) for _ in range(3)] + [np.zeros(n)]
        hv = [np.zeros((max(1, P), L)) for _ in range(3)] + [np.zeros((max(1, P), n))]
        st = np.zeros(4)
        if elastic:
            edirs = [table("E", L), table("nu", L)]
            eg = [np.zeros(L) for _ in range(2)]
            ehv = [np.zeros((max(1, P), L)) for _ in range(2)]
            # (the library refuses non-NULL hv_E / hv_nu on a handle without mechanics: asked for only where they can be non-zero)
            want = getattr(self, "with_mechanics", True) or any(d is not None for d in edirs)
            self._check(self.lib.glims_adjoint_hessian_full(
                self._h, len(terms), arr, int(P), *[_ptr(d, _dp) for d in dirs + edirs], C.byref(J),
                *[_ptr(a, _dp) for a in g + eg], *[_ptr(a, _dp) for a in hv], *[_ptr(a if want else None, _dp) for a in ehv],
                _ptr(st, _dp)))
            del keep
            return {"J": J.value, "D": g[0], "rho": g[1], "gamma": g[2], "c0": g[3], "E": eg[0], "nu": eg[1],
                    "hv_D": hv[0][:P], "hv_rho": hv[1][:P], "hv_gamma": hv[2][:P], "hv_c0": hv[3][:P], "hv_E": ehv[0][:P],
                    "hv_nu": ehv[1][:P],
                    "stats": {"tlm_pcg_its": int(st[0]), "soa_pcg_its": int(st[1]), "mech_solves": int(st[2]), "ms": st[3]}}
        call = self.lib.glims_adjoint_hessian_spmd if collective else self.lib.glims_adjoint_hessian
        self._check(call(self._h, len(terms), arr, int(P), *[_ptr(d, _dp) for d in dirs], C.byref(J),
                         *[_ptr(a, _dp) for a in g], *[_ptr(a, _dp) for a in hv], _ptr(st, _dp)))
        del keep
        return {"J": J.value, "D": g[0], "rho": g[1], "gamma": g[2], "c0": g[3], "hv_D": hv[0][:P], "hv_rho": hv[1][:P],
                "hv_gamma": hv[2][:P], "hv_c0": hv[3][:P],
                "stats": {"tlm_pcg_its": int(st[0]), "soa_pcg_its": int(st[1]), "mech_solves": int(st[2]), "ms": st[3]}}

    def adjoint_stats(self):
        a = np.zeros(6, dtype=np.int64)
        ms = C.c_double(0.0)
        self._check(self.lib.glims_adjoint_stats(self._h, _ptr(a, _i64p), C.byref(ms)))
        keys = ("gradients", "backward_steps", "pcg_its", "mech_solves", "mech_its", "recorded_states")
        d = {k: int(v) for k, v in zip(keys, a)}
        d["ms_backward"] = ms.value
        return d

    # -- samplers --------------------------------------------------------------------------------
    def _deformation_source(self, deformed_by):
        """(u_source, u_host) of the deformed creators: a snapshot id, 'current', or a nodal array [n_nodes, dim]."""
        if isinstance(deformed_by, str):
            if deformed_by != 'current':
                raise ValueError("deformed_by must be a snapshot id, 'current' or a nodal array [n_nodes, dim]")
            return DERIVE_CURRENT, None
        if isinstance(deformed_by, (int, np.integer)):
            if deformed_by < 0:
                raise ValueError("deformed_by: snapshot ids are not negative")
            return int(deformed_by), None
        u = np.asarray(deformed_by, dtype=np.float64)
        if u.size != self.n_nodes * self.dim:
            raise ValueError("deformed_by has %d entries, the mesh %d nodes x %d" % (u.size, self.n_nodes, self.dim))
        return DERIVE_HOST, _f64(u.reshape(-1), (self.n_nodes * self.dim,))

    def _deformed_status(self, st):
        self.last_sampler_status = st
        self._check(st, allow=(GLIMS_NOT_CONVERGED,))
        if st == GLIMS_NOT_CONVERGED:
            logging.getLogger(__name__).warning(
                "deformed sampler: the displacement solve stopped at its iteration cap; the points are located in the mesh "
                "displaced by what it reached")

    def sampler_points(self, xyz, deformed_by=None, scale=1.0):
        """Locate the points xyz [n, dim] in the mesh once; returns a :class:`Sampler`.  With ``deformed_by`` (a snapshot id,
        'current', or a nodal displacement [n_nodes, dim] in the caller's node order) the points are located in the mesh
        displaced by ``scale`` times that displacement (glims_sampler_create_points_deformed): the sampler then evaluates
        fields at the material points that sit at xyz, and stays as it is whatever the handle does later.
        ``last_sampler_status`` holds the status of the displacement solve (GLIMS_NOT_CONVERGED is a logged warning)."""
        xyz = _f64(np.asarray(xyz, dtype=np.float64).reshape(-1, self.dim))
        sid = C.c_int64(-1)
        if deformed_by is None:
            self._check(self.lib.glims_sampler_create_points(self._h, xyz.shape[0], _ptr(xyz, _dp), 0, C.byref(sid)))
        else:
            src, u = self._deformation_source(deformed_by)
            self._deformed_status(self.lib.glims_sampler_create_points_deformed(
                self._h, xyz.shape[0], _ptr(xyz, _dp), src, _ptr(u, _dp), float(scale), 0, C.byref(sid)))
        return Sampler(self, int(sid.value), None)

    def sampler_grid(self, origin, spacing, size, deformed_by=None, scale=1.0):
        """Locate the points origin + index * spacing of a grid with size[a] points along axis a (x fastest).  ``deformed_by``
        / ``scale``: as for sampler_points (glims_sampler_create_grid_deformed)."""
        o, sp = _f64(origin, (self.dim,)), _f64(spacing, (self.dim,))
        sz = np.ascontiguousarray(size, dtype=np.int64)
        assert sz.shape == (self.dim,)
        sid = C.c_int64(-1)
        if deformed_by is None:
            self._check(self.lib.glims_sampler_create_grid(self._h, _ptr(o, _dp), _ptr(sp, _dp), _ptr(sz, _i64p), 0,
                                                           C.byref(sid)))
        else:
            src, u = self._deformation_source(deformed_by)
            self._deformed_status(self.lib.glims_sampler_create_grid_deformed(
                self._h, _ptr(o, _dp), _ptr(sp, _dp), _ptr(sz, _i64p), src, _ptr(u, _dp), float(scale), 0, C.byref(sid)))
        return Sampler(self, int(sid.value), tuple(int(v) for v in sz))

    # -- multi-GPU -------------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        lib = load_library()
        buf = C.create_string_buffer(GLIMS_UNIQUE_ID_BYTES)
        st = lib.glims_comm_unique_id(buf)
        if st != GLIMS_OK:
            raise BackendError(st, "ncclGetUniqueId failed")
        return buf.raw

    def comm_init(self, rank, world, uid):
        assert len(uid) == GLIMS_UNIQUE_ID_BYTES
        self._check(self.lib.glims_comm_init(self._h, int(rank), int(world), uid))

    def comm_selftest(self):
        self._check(self.lib.glims_comm_selftest(self._h))

    def comm_mailbox(self, shm_name):
        """Node-local all-reduce through the POSIX shm object `shm_name` ('/...'); None switches it off."""
        self._check(self.lib.glims_comm_mailbox(self._h, None if shm_name is None else shm_name.encode()))

    def comm_mailbox_selftest(self):
        self._check(self.lib.glims_comm_mailbox_selftest(self._h))

    def set_transport(self, rank, world, halo_cb, allreduce_cb):
        """halo_cb / allreduce_cb: HALO_FN / ALLREDUCE_FN instances (kept alive by this handle)."""
        self._transport_refs = (halo_cb, allreduce_cb)
        self._check(self.lib.glims_set_transport(self._h, int(rank), int(world), C.cast(halo_cb, C.c_void_p),
                                                 C.cast(allreduce_cb, C.c_void_p), None))

    def set_mg_frame(self, lo, hi):
        """Bounding box of the WHOLE (global) mesh: the elasticity multigrid of a partitioned run gets replicated coarse
        levels on one global grid frame (see glims_set_mg_frame)."""
        lo, hi = _f64(lo, (self.dim,)), _f64(hi, (self.dim,))
        self._check(self.lib.glims_set_mg_frame(self._h, _ptr(lo, _dp), _ptr(hi, _dp)))

    def set_halo(self, peer_rank, send_ptr, send_idx, recv_count):
        pr = np.ascontiguousarray(peer_rank, dtype=np.int32)
        sp = np.ascontiguousarray(send_ptr, dtype=np.int64)
        si = np.ascontiguousarray(send_idx, dtype=np.int32)
        rc = np.ascontiguousarray(recv_count, dtype=np.int64)
        assert len(sp) == len(pr) + 1 and len(rc) == len(pr)
        self._check(self.lib.glims_set_halo(self._h, len(pr), _ptr(pr, _i32p), _ptr(sp, _i64p), _ptr(si, _i32p),
                                            _ptr(rc, _i64p)))


class Sampler:
    """A set of query points located once in a handle's mesh (``glims_sampler_*``): ``cells`` (the caller's cell index, -1
    outside the mesh) and barycentric ``weights`` stay on the device and serve any number of ``apply`` calls."""

    def __init__(self, handle, sid, grid_size):
        self.handle, self.id, self.grid_size = handle, sid, grid_size
        n, nf = C.c_int64(0), C.c_int64(0)
        handle._check(handle.lib.glims_sampler_info(handle._h, sid, C.byref(n), C.byref(nf)))
        self.n_points, self.n_found = int(n.value), int(nf.value)
        # deformed samplers (glims_sampler_deformation_info): cells whose det(E_deformed) / det(E_reference) is not > 0, and
        # the smallest such ratio = min_T det(I + scale grad u_h); 0 and 1 on an undeformed sampler
        info = np.zeros(2, dtype=np.int64)
        mr = C.c_double(1.0)
        handle._check(handle.lib.glims_sampler_deformation_info(handle._h, sid, _ptr(info, _i64p), C.byref(mr)))
        self.deformed, self.n_inverted, self.min_jacobian = bool(info[0]), int(info[1]), float(mr.value)

    def _get(self, want_cells, want_weights):
        h = self.handle
        cells = np.empty(self.n_points, dtype=np.int32) if want_cells else None
        w = np.empty((self.n_points, h.dim + 1)) if want_weights else None
        h._check(h.lib.glims_sampler_get(h._h, self.id, _ptr(cells, _i32p), _ptr(w, _dp)))
        return cells, w

    @property
    def cells(self):
        return self._get(True, False)[0]

    @property
    def weights(self):
        return self._get(False, True)[1]

    def resolve(self, cell_gid):
        """glims_sampler_resolve (collective on a partitioned handle, every rank with the same points): cell_gid [n_cells] =
        the global id of each of this handle's cells, strictly increasing (``partition_mesh``'s ``cell_ids``).  Afterwards
        the sampler keeps only the points whose local winner is the global winner, ``n_found`` counts those, and ``apply_t``
        works (owned rows complete, ghost rows 0).  A no-op on a single-GPU handle."""
        h = self.handle
        gid = np.ascontiguousarray(cell_gid, dtype=np.int64).reshape(-1)
        if gid.shape != (h.n_cells,):
            raise ValueError("cell_gid has %d entries, the handle %d cells" % (gid.size, h.n_cells))
        h._check(h.lib.glims_sampler_resolve(h._h, self.id, _ptr(gid, _i64p)))
        nf = C.c_int64(0)
        h._check(h.lib.glims_sampler_info(h._h, self.id, None, C.byref(nf)))
        self.n_found = int(nf.value)

    @property
    def counted(self):
        """bool [n_points]: the points this rank adds to J and to the observed count (resolved samplers; otherwise the found
        points)."""
        h = self.handle
        out = np.zeros(self.n_points, dtype=np.uint8)
        h._check(h.lib.glims_sampler_get_counted(h._h, self.id, _ptr(out, C.POINTER(C.c_uint8))))
        return out.astype(bool)

    def apply(self, field, snapshot=None, fill=np.nan):
        """P f at every point: ``field`` = 'c' (current concentration, or the device snapshot ``snapshot``), 'u' (current
        displacement), 'x' (the mesh's reference coordinates: on a deformed sampler the back map X(x_p)), 'derived' (the result of the handle's last ``derive``, from its device buffer: [n_points] for a scalar,
        [n_points, d(d+1)/2] symmetric components xx, yy, (zz,) xy, (xz, yz) for a tensor) or a nodal array [n_nodes] /
        [n_nodes, k] in the caller's node order.  Returns [n_points] for a one-dimensional field, [n_points, k] otherwise;
        points outside the mesh hold ``fill``."""
        h = self.handle
        nodal, flat = None, False
        if isinstance(field, str):
            if field == 'c':
                kind, ncomp, flat = (FIELD_C if snapshot is None else FIELD_SNAPSHOT_C), 1, True
            elif field == 'u':
                if snapshot is not None:
                    raise ValueError("snapshots hold the concentration only")
                kind, ncomp = FIELD_U, h.dim
            elif field == 'x':
                if snapshot is not None:
                    raise ValueError("'x' takes no snapshot")
                kind, ncomp = FIELD_XYZ, h.dim
            elif field == 'derived':
                if snapshot is not None:
                    raise ValueError("'derived' is the last derive()'s result; it takes no snapshot")
                ncomp = getattr(h, "_derived_ncomp", 1)
                kind, flat = FIELD_DERIVED, ncomp == 1
            else:
                raise ValueError("field must be 'c', 'u', 'x', 'derived' or a nodal array")
        else:
            a = np.asarray(field, dtype=np.float64)
            if a.shape[0] != h.n_nodes:
                raise ValueError("nodal array has %d rows, the mesh %d nodes" % (a.shape[0], h.n_nodes))
            flat = a.ndim == 1
            nodal = _f64(a.reshape(h.n_nodes, 1) if flat else a.reshape(h.n_nodes, -1))
            kind, ncomp = FIELD_HOST, nodal.shape[1]
        out = np.empty((self.n_points, ncomp))
        h._check(h.lib.glims_sampler_apply(h._h, self.id, kind, -1 if snapshot is None else int(snapshot),
                                           _ptr(nodal, _dp), int(ncomp), float(fill), _ptr(out, _dp)))
        return out[:, 0] if flat else out

    def apply_t(self, r):
        """P^T r: r [n_points] or [n_points, k] -> nodal [n_nodes] / [n_nodes, k] (caller's node order)."""
        h = self.handle
        a = np.asarray(r, dtype=np.float64)
        flat = a.ndim == 1
        a = _f64(a.reshape(self.n_points, 1) if flat else a.reshape(self.n_points, a.shape[-1]))
        g = np.empty((h.n_nodes, a.shape[1]))
        h._check(h.lib.glims_sampler_apply_t(h._h, self.id, _ptr(a, _dp), int(a.shape[1]), _ptr(g, _dp)))
        return g[:, 0] if flat else g

    def back_map(self, fill=np.nan):
        """X(x_p) [n_points, dim]: the reference position of the material point that sits at x_p (``apply('x')``)."""
        return self.apply('x', fill=fill)

    def warp(self, array, origin, spacing, order='linear', fill=np.nan):
        """image(X(x_p)) at every point (glims_sampler_warp): ``array`` [z,] y, x [, component] with voxel centres origin +
        index * spacing, ``order`` 'linear' (d-linear) or 'nearest'.  Returns [n_points] or [n_points, k]; points outside
        the mesh and points whose X lies outside the source image hold ``fill``."""
        h = self.handle
        if order not in ('linear', 'nearest', 0, 1):
            raise ValueError("order must be 'linear' or 'nearest'")
        o = 1 if order in ('linear', 1) else 0
        a = np.asarray(array, dtype=np.float64)
        if a.ndim not in (h.dim, h.dim + 1):
            raise ValueError("the source image has %d axes, the mesh %d dimensions" % (a.ndim, h.dim))
        flat = a.ndim == h.dim
        size = np.ascontiguousarray(a.shape[:h.dim][::-1], dtype=np.int64)
        ncomp = 1 if flat else a.shape[-1]
        a = _f64(a.reshape(-1))
        og, sp = _f64(origin, (h.dim,)), _f64(spacing, (h.dim,))
        out = np.empty((self.n_points, max(1, ncomp)))
        h._check(h.lib.glims_sampler_warp(h._h, self.id, _ptr(a, _dp), _ptr(og, _dp), _ptr(sp, _dp), _ptr(size, _i64p),
                                          int(ncomp), o, float(fill), _ptr(out, _dp)))
        return out[:, 0] if flat else out

    def close(self):
        h = self.handle
        if self.id is not None and getattr(h, "_h", None):
            h._check(h.lib.glims_sampler_destroy(h._h, self.id))
        self.id = None
