"""ctypes binding of libgamd_hip.so (C ABI: include/gamd_hip.h).

There is deliberately no fallback: if the HIP library is missing or no GPU is
present, loading / gamd_create fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# GAMD_LIB: load another build of the SAME C ABI instead (tools/ point it at libgamd_hip_prof.so, the -DGAMD_PROFILING
# build with s_memtime segment marks).  It must exist: there is no fallback either way.
LIB_PATH = os.environ.get("GAMD_LIB") or os.path.join(_HERE, "libgamd_hip.so")


class GamdConfig(C.Structure):
    _fields_ = [("n_atoms", C.c_int32), ("kind", C.c_int32), ("n_layers", C.c_int32),
                ("use_bond", C.c_int32), ("nbr_flavour", C.c_int32), ("device", C.c_int32),
                ("cutoff", C.c_float), ("box", C.c_float * 3), ("edge_capacity", C.c_int64),
                ("keep_stages", C.c_int32), ("edge_dtype", C.c_int32),
                ("encoding_size", C.c_int32), ("edge_embedding_dim", C.c_int32), ("hidden_dim", C.c_int32),
                ("no_expand_edge", C.c_int32), ("neighbor_skin", C.c_float), ("self_loop_mode", C.c_int32),
                ("kernel_select", C.c_int32), ("small_tile_limit", C.c_int32), ("n_boxes", C.c_int32)]


# common tail of both integrator parameter blocks (masses per species, length unit, rigid water)
_MD_EXT = [("mass_h_amu", C.c_float), ("length_per_nm", C.c_float), ("rigid_water", C.c_int32),
           ("r_oh", C.c_float), ("r_hh", C.c_float), ("remove_cm_motion", C.c_int32)]


class GamdNhcParams(C.Structure):
    _fields_ = [("dt_ps", C.c_float), ("mass_amu", C.c_float), ("temperature_k", C.c_float),
                ("frequency_per_ps", C.c_float), ("chain_length", C.c_int32), ("num_mts", C.c_int32),
                ("num_yoshidasuzuki", C.c_int32), ("reset", C.c_int32), ("ndf", C.c_double)] + _MD_EXT


class GamdMdParams(C.Structure):
    _fields_ = [("dt_ps", C.c_float), ("mass_amu", C.c_float), ("temperature_k", C.c_float),
                ("gamma_per_ps", C.c_float), ("seed", C.c_uint64), ("first_step", C.c_uint64)] + _MD_EXT


class GamdReportParams(C.Structure):
    _fields_ = [("interval", C.c_int64), ("max_samples", C.c_int64), ("ndf", C.c_double), ("rdf_bins", C.c_int32),
                ("rdf_rmax", C.c_float), ("exclude_same_molecule", C.c_int32), ("reserved", C.c_int32)]


class GamdTrajParams(C.Structure):
    _fields_ = [("interval", C.c_int64), ("max_frames", C.c_int64), ("fields", C.c_int32), ("n_lags", C.c_int32),
                ("subtract_com", C.c_int32), ("reserved", C.c_int32)]


class GamdStructParams(C.Structure):
    _fields_ = [("interval", C.c_int64), ("rdf_bins", C.c_int32), ("rdf_rmax", C.c_float), ("exclude_same_molecule", C.c_int32),
                ("sk_n2max", C.c_int32), ("reserved", C.c_int32 * 2)]


class GamdClassicalParams(C.Structure):
    _fields_ = [("interval", C.c_int64), ("max_samples", C.c_int64), ("sigma", C.c_double), ("epsilon", C.c_double),
                ("r_cut", C.c_double), ("r_switch", C.c_double), ("shift", C.c_int32), ("reserved", C.c_int32)]


class GamdWaterParams(C.Structure):
    _fields_ = [("interval", C.c_int64), ("max_samples", C.c_int64), ("q_h", C.c_double), ("sigma_o", C.c_double),
                ("epsilon_o", C.c_double), ("r_cut", C.c_double), ("r_switch", C.c_double), ("shift", C.c_int32),
                ("reserved", C.c_int32), ("alpha", C.c_double), ("k_cut", C.c_double), ("coulomb_const", C.c_double)]


class GamdWaterPmeParams(C.Structure):
    _fields_ = [("order", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32)]


class GamdMinimizeParams(C.Structure):
    _fields_ = [("tolerance", C.c_double), ("max_iter", C.c_int64), ("check_every", C.c_int64), ("dt_start", C.c_double),
                ("dt_max", C.c_double), ("f_inc", C.c_double), ("f_dec", C.c_double), ("alpha_start", C.c_double),
                ("f_alpha", C.c_double), ("max_step", C.c_double), ("n_min", C.c_int32), ("reserved", C.c_int32)]


class GamdLbfgsParams(C.Structure):
    _fields_ = [("tolerance", C.c_double), ("max_iter", C.c_int64), ("check_every", C.c_int64), ("max_step", C.c_double),
                ("c1", C.c_double), ("curv", C.c_double), ("m", C.c_int32), ("max_ls", C.c_int32), ("reserved", C.c_int64)]


MINIMIZE_ROW = 8                                            # GAMD_MINIMIZE_ROW: doubles per box of gamd_minimize's rows
MINIMIZE_STATE = ("converged", "max_iter", "failed")        # GAMD_MIN_*: a row's state and the call's return value
LBFGS_ROW = 10                                              # GAMD_LBFGS_ROW: doubles per box of gamd_minimize_lbfgs's rows
LBFGS_STATE = ("converged", "max_iter", "failed", "line_search")   # GAMD_LBFGS_*: a row's state and the call's return value
CLASSICAL_ROW = 9                                           # GAMD_CLASSICAL_ROW: doubles per box and row of gamd_classical_read
WATER_ROW = 12                                              # GAMD_WATER_ROW: doubles per box and row of gamd_water_read
WATER_VIRIAL_ROW = 6                                        # GAMD_WATER_VIRIAL_ROW: doubles per box and row of gamd_water_virial_read
TRAJ_FIELDS = {"x": 1, "v": 2, "f": 4, "image": 8}          # GAMD_TRAJ_*
FORCE_SOURCE = {"network": 0, "classical": 1}               # GAMD_FORCE_*
WATER_FORCE_SOURCE = {"water_classical": 2}                 # GAMD_FORCE_WATER_CLASSICAL (GAMD_KIND_WATER handles)


# every symbol include/gamd_hip.h declares: name -> (restype, argtypes)
_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
SYMBOLS = {
    "gamd_version": (C.c_char_p, []),
    "gamd_last_error": (C.c_char_p, []),
    "gamd_create": (_i32, [C.POINTER(GamdConfig), C.POINTER(_vp)]),
    "gamd_destroy": (_i32, [_vp]),
    "gamd_load_weight": (_i32, [_vp, C.c_char_p, _vp, C.POINTER(_i64), _i32]),
    "gamd_finalize_weights": (_i32, [_vp]),
    "gamd_set_scaler": (_i32, [_vp, C.c_double, C.c_double]),
    "gamd_set_bonds": (_i32, [_vp, _vp, _i64]),
    "gamd_forces_async": (_i32, [_vp, _vp, _vp, C.POINTER(C.c_float), _vp, _vp, _vp]),
    "gamd_set_node_features": (_i32, [_vp, _vp]),
    "gamd_get_device_flags": (_i32, [_vp, C.POINTER(_i32)]),
    "gamd_sync_status": (_i32, [_vp, _vp]),
    "gamd_forces_host": (_i32, [_vp, _vp, _vp, C.POINTER(C.c_float), _vp, _i32, _vp]),
    "gamd_forces": (_i32, [_vp, _vp, _vp, C.POINTER(C.c_float), _vp, _vp, _vp]),
    "gamd_forces_edges": (_i32, [_vp, _vp, _vp, C.POINTER(C.c_float), _vp, _vp, _i64, _vp, _vp, _vp]),
    "gamd_build_neighbors": (_i32, [_vp, _vp, _vp, C.POINTER(C.c_float), _vp]),
    "gamd_get_counts": (_i32, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "gamd_get_skin_stats": (_i32, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "gamd_debug_get": (_i32, [_vp, _i32, _vp, C.c_size_t]),
    "gamd_md_run": (_i32, [_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_float), C.POINTER(GamdMdParams), _i64, _vp]),
    "gamd_md_run_nhc": (_i32, [_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_float), C.POINTER(GamdNhcParams), _vp, _i64, _vp]),
    "gamd_report_configure": (_i32, [_vp, C.POINTER(GamdReportParams)]),
    "gamd_report_reset": (_i32, [_vp]),
    "gamd_report_read": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, C.POINTER(_i64), _vp, _i64, C.POINTER(_i64), C.POINTER(_i64),
                                C.POINTER(_i32)]),
    "gamd_traj_configure": (_i32, [_vp, C.POINTER(GamdTrajParams)]),
    "gamd_traj_reset": (_i32, [_vp]),
    "gamd_traj_read_frames": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "gamd_traj_read_dynamics": (_i32, [_vp, _vp, _vp, _vp, _i64, C.POINTER(_i64), C.POINTER(C.c_uint64), _vp, C.POINTER(_i32)]),
    "gamd_struct_configure": (_i32, [_vp, C.POINTER(GamdStructParams)]),
    "gamd_struct_reset": (_i32, [_vp]),
    "gamd_struct_read": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, C.POINTER(_i64), C.POINTER(_i32)]),
    "gamd_classical_configure": (_i32, [_vp, C.POINTER(GamdClassicalParams)]),
    "gamd_classical_reset": (_i32, [_vp]),
    "gamd_classical_read": (_i32, [_vp, _vp, _vp, _vp, _i64, C.POINTER(_i64), C.POINTER(_i64), _vp, _i64]),
    "gamd_classical_eval": (_i32, [_vp, _vp, C.POINTER(C.c_float), C.c_float, _vp, _vp, _vp, _vp, _vp]),
    "gamd_classical_cells": (_i32, [_vp, _i32]),
    "gamd_classical_cells_read": (_i32, [_vp, _vp, _i32, C.POINTER(_i32), _vp, _i64, _vp, _i64]),
    "gamd_md_force_source": (_i32, [_vp, _i32]),
    "gamd_minimize": (_i32, [_vp, _vp, C.POINTER(C.c_float), C.c_float, _vp, _vp, C.POINTER(GamdMinimizeParams), _vp, _vp]),
    "gamd_minimize_lbfgs": (_i32, [_vp, _vp, C.POINTER(C.c_float), C.c_float, _vp, _vp, C.POINTER(GamdLbfgsParams), _vp, _vp]),
    "gamd_water_configure": (_i32, [_vp, C.POINTER(GamdWaterParams)]),
    "gamd_water_msite": (_i32, [_vp, C.c_double]),
    "gamd_water_pme": (_i32, [_vp, C.POINTER(GamdWaterPmeParams)]),
    "gamd_water_cells": (_i32, [_vp, _i32]),
    "gamd_water_cells_read": (_i32, [_vp, _vp, _i32, C.POINTER(_i32), _vp, _i64, _vp, _i64]),
    "gamd_water_reset": (_i32, [_vp]),
    "gamd_water_read": (_i32, [_vp, _vp, _vp, _vp, _i64, C.POINTER(_i64), C.POINTER(_i64), _vp, _i64]),
    "gamd_water_eval": (_i32, [_vp, _vp, _vp, C.POINTER(C.c_float), C.c_float, _vp, _vp, _vp]),
    "gamd_water_virial": (_i32, [_vp, _i32]),
    "gamd_water_virial_read": (_i32, [_vp, _vp, _vp, _i64, C.POINTER(_i64)]),
    "gamd_water_virial_eval": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(C.c_float), C.c_float, C.c_double, C.c_double, _vp, _vp, _vp]),
    "gamd_water_minimize": (_i32, [_vp, _vp, _vp, C.POINTER(C.c_float), C.c_float, C.c_double, C.c_double, _vp, _vp,
                                   C.POINTER(GamdMinimizeParams), _vp, _vp]),
    "gamd_water_minimize_lbfgs": (_i32, [_vp, _vp, _vp, C.POINTER(C.c_float), C.c_float, C.c_double, C.c_double, _vp, _vp,
                                         C.POINTER(GamdLbfgsParams), _vp, _vp]),
    "gamd_water_minimize_potential": (_i32, [_vp, _i32]),
    "gamd_profile": (_i32, [_vp, _vp, _vp, C.POINTER(C.c_float), _vp, _vp, C.c_char_p, C.c_size_t,
                            C.POINTER(C.c_float), _i32, C.POINTER(_i32)]),
    "gamd_timing_enable": (_i32, [_vp, _i32]),
    "gamd_timing_read": (_i32, [_vp, _vp, C.POINTER(C.c_double), C.POINTER(_i64)]),
    "gamd_timing_read_stages": (_i32, [_vp, _vp, C.POINTER(C.c_double), C.POINTER(_i64)]),
    "gamd_timing_read_steps": (_i32, [_vp, _vp, C.POINTER(C.c_float), _i64, C.POINTER(_i64)]),
}

_lib = None


def load() -> C.CDLL:
    """Load the shared library (once) and type every entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension was not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C gamd_amd/csrc`). "
            "gamd_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class GamdError(RuntimeError):
    pass


def check(status: int, what: str) -> int:
    if status < 0:
        msg = load().gamd_last_error().decode("utf-8", "replace")
        raise GamdError(f"{what} failed with status {status}: {msg}")
    return status
