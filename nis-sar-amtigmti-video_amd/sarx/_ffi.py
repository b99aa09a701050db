"""ctypes binding of libsarx.so (include/sarx.h).  No torch, no cffi.

The library is built in-tree by ``csrc/Makefile`` (``__graft_entry__.build()``).
There is no CPU fallback: every compute entry point needs a gfx950 device and
raises :class:`SarxError` otherwise.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SARX_LIB") or os.path.join(_HERE, "libsarx.so")

MAX_SLOT_BYTES = 32768          # SARX_MAX_SLOT_BYTES: 256 partial maxima, 32 floats apart
COMM_ID_BYTES = 128
OUT_AZ_MAJOR, OUT_RG_MAJOR, FUSE_RANGE = 0, 1, 2
PASS_AZ_FFT_PHI1, PASS_RG_FFT_PHI2, PASS_RG_IFFT_PHI3, PASS_AZ_IFFT, PASS_RG_FUSED_23 = 1, 2, 3, 4, 23
PASS_TEST_RG_FFT, PASS_TEST_RG_IFFT = 100, 101
PASS_RG_FFT_PHI2_PERM, PASS_RG_IFFT_PHI3_PERM = 12, 13      # n_rg = 16384: spectrum order P[(k // 16 // 64) * 1024 + (k % 16) * 64 + (k // 16) % 64] = X[k]


class SarxError(RuntimeError):
    """Raised with sarx_last_error() text when a libsarx call fails."""

    def __init__(self, code, msg):
        super().__init__(f"libsarx error {code}: {msg}")
        self.code = code


class RadarParams(C.Structure):
    """sarx_radar_params: positional args of sar_focus_csa after phist
    (sar_ati_dcpa_sim_csa.py:202)."""
    _fields_ = [(n, C.c_double) for n in (
        "wavelength_m", "pulse_width_s", "chirp_rate_hz_s", "sample_rate_hz", "prf_hz",
        "platform_speed_mps", "range_ref_m", "t_start_fast_s")]


class TdbpParams(C.Structure):
    """sarx_tdbp_params: the module constants tdbp_gpu reads (sar_batch_sim.py:13,20,23-25)."""
    _fields_ = [(n, C.c_double) for n in ("c", "fc", "fs", "t_p", "k_rate")]


class AtiOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "ati_phase", "slc1_mag", "dpca_mag", "ati_interf", "dpca_diff", "slc2_mag", "slc1_phase",
        "slc2_phase", "dpca_phase")]


# name -> (restype, argtypes): every symbol declared in include/sarx.h
_vp, _i, _sz, _u64, _d, _f = C.c_void_p, C.c_int, C.c_size_t, C.c_uint64, C.c_double, C.c_float
_P = C.POINTER
SIGNATURES = {
    "sarx_version": (_i, []),
    "sarx_init": (_i, [_i, _P(_vp)]),
    "sarx_destroy": (_i, [_vp]),
    "sarx_last_error": (C.c_char_p, [_vp]),
    "sarx_device_count": (_i, [_P(_i)]),
    "sarx_device_info": (_i, [_vp, C.c_char_p, _sz, _P(_i), _P(_u64), C.c_char_p, _sz]),
    "sarx_malloc": (_i, [_vp, _sz, _P(_vp)]),
    "sarx_free": (_i, [_vp, _vp]),
    "sarx_host_alloc": (_i, [_vp, _sz, C.POINTER(_vp)]),
    "sarx_host_free": (_i, [_vp, _vp]),
    "sarx_memcpy_h2d": (_i, [_vp, _vp, _vp, _sz]),
    "sarx_memcpy_d2h": (_i, [_vp, _vp, _vp, _sz]),
    "sarx_memcpy_d2d": (_i, [_vp, _vp, _vp, _sz]),
    "sarx_memcpy_h2d_unordered": (_i, [_vp, _vp, _vp, _sz]),
    "sarx_memcpy_h2d_lane": (_i, [_vp, _vp, _vp, _sz]),
    "sarx_memcpy_d2h_begin": (_i, [_vp, _vp, _vp, _sz, _P(_i)]),
    "sarx_memcpy_d2h_end": (_i, [_vp, _i]),
    "sarx_memcpy2d_d2h": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _sz]),
    "sarx_memcpy2d_h2d": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _sz]),
    "sarx_memset": (_i, [_vp, _vp, _i, _sz]),
    "sarx_persistent_grid": (_i, [_i, _i, _i]),
    "sarx_sync": (_i, [_vp]),
    "sarx_select_lane": (_i, [_vp, _i]),
    "sarx_lanes_join": (_i, [_vp]),
    "sarx_set_range_cus": (_i, [_vp, _i]),
    "sarx_probe_lanes": (_i, [_vp, _i, _i, _i, _P(_d)]),
    "sarx_event_record": (_i, [_vp, _i]),
    "sarx_event_elapsed_ms": (_i, [_vp, _i, _i, _P(_f)]),
    "sarx_csa_plan_create": (_i, [_vp, _i, _i, _P(RadarParams), C.c_uint, _P(_vp)]),
    "sarx_csa_plan_destroy": (_i, [_vp]),
    "sarx_csa_axes": (_i, [_vp, _vp, _vp]),
    "sarx_csa_focus_host": (_i, [_vp, _vp, _vp]),
    "sarx_csa_focus_host_begin": (_i, [_vp, _vp, _vp, _P(_i)]),
    "sarx_csa_focus_host_end": (_i, [_vp, _i]),
    "sarx_csa_focus_host_c128": (_i, [_vp, _vp, _vp]),
    "sarx_csa_focus_dev": (_i, [_vp, _vp, _vp]),
    "sarx_csa_pass": (_i, [_vp, _i, _vp, _vp]),
    "sarx_csa_plan_mark_range": (_i, [_vp, _i, _i]),
    "sarx_csa_plan_stamp_range": (_i, [_vp, _vp]),
    "sarx_csa_plan_set_look_slot": (_i, [_vp, _i, _vp]),
    "sarx_csa_plan_set_max_slot": (_i, [_vp, _vp]),
    "sarx_csa_plan_set_ati": (_i, [_vp, _vp, _vp, _f, _d, _vp, _vp, _vp, _i]),
    "sarx_csa_plan_bytes": (_i, [_vp, _P(_u64)]),
    "sarx_rda_plan_create": (_i, [_vp, _i, _i, _P(RadarParams), _P(_vp)]),
    "sarx_rda_plan_destroy": (_i, [_vp]),
    "sarx_rda_focus_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "sarx_rda_focus_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "sarx_rda_focus_host2": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sarx_rda_focus_dev2": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sarx_rda_axes": (_i, [_vp, _vp, _vp, _vp]),
    "sarx_ati_dpca_dev": (_i, [_vp, _vp, _vp, _sz, _d, _P(AtiOutputs), _P(_d), _P(_d)]),
    "sarx_ati_stats": (_i, [_vp, _P(_d), _P(_d)]),
    "sarx_ati_dpca_masked_dev": (_i, [_vp, _vp, _vp, _sz, _d, _vp, _f, _P(AtiOutputs)]),
    "sarx_mask_phase_frac_dev": (_i, [_vp, _vp, _vp, _sz, _f, _vp]),
    "sarx_magnitude_dev": (_i, [_vp, _vp, _vp, _sz]),
    "sarx_max_abs_f32_dev": (_i, [_vp, _vp, _sz, _vp]),
    "sarx_mask_phase_dev": (_i, [_vp, _vp, _vp, _sz, _f, _vp]),
    "sarx_corner_turn_dev": (_i, [_vp, _vp, _vp, _i, _i]),
    "sarx_multilook_dev": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "sarx_fill_noise_c64": (_i, [_vp, _vp, _sz, _u64]),
    "sarx_add_ocean_noise_dev": (_i, [_vp, _vp, _sz, _d, _d, _d, _u64]),
    "sarx_add_ocean_noise_rel_dev": (_i, [_vp, _vp, _sz, _i, _d, _d, _d, _u64]),
    "sarx_power_stats_dev": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "sarx_echo_synth_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _d, _d, _vp, _i]),
    "sarx_echo_geometry_dev": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _d, _d, _d, _d, _vp, _vp]),
    "sarx_echo_spotlight_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _d, _d, _vp]),
    "sarx_tdbp_plan_create": (_i, [_vp, _i, _i, _i, _i, _P(TdbpParams), _P(_vp)]),
    "sarx_tdbp_plan_destroy": (_i, [_vp]),
    "sarx_tdbp_last_window": (_i, [_vp, _vp, _vp]),
    "sarx_tdbp_focus_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _d, _vp, _d, _vp]),
    "sarx_tdbp_focus_host": (_i, [_vp, _vp, _vp, _vp, _vp, _d, _vp, _d, _vp, _vp]),
    "sarx_comm_unique_id": (_i, [_vp]),
    "sarx_rccl_info": (_i, [C.c_char_p, _sz, _P(_i), _P(_i)]),
    "sarx_comm_init": (_i, [_vp, _vp, _i, _i]),
    "sarx_allgather_dev": (_i, [_vp, _vp, _vp, _sz]),
    "sarx_allreduce_max_dev": (_i, [_vp, _vp, _sz]),
    "sarx_comm_sync": (_i, [_vp]),
    "sarx_comm_fence_compute": (_i, [_vp]),
    "sarx_comm_mark": (_i, [_vp, _i]),
    "sarx_comm_wait_mark": (_i, [_vp, _i]),
    "sarx_comm_destroy": (_i, [_vp]),
}

# include/sarx_gmti.h: the GMTI detector's structs and entry points, bound by load() beside SIGNATURES (a table of its own: sarx.h
# and SIGNATURES stay exactly what they are)
class GmtiParams(C.Structure):
    """sarx_gmti_params"""
    _fields_ = [("guard_az", C.c_int32), ("guard_rg", C.c_int32), ("train_az", C.c_int32), ("train_rg", C.c_int32),
                ("alpha", C.c_double), ("min_train", C.c_int32), ("max_detections", C.c_int32)]


class GmtiHeader(C.Structure):
    """sarx_gmti_header: the first 16 bytes of a detection slot"""
    _fields_ = [("count", C.c_uint32), ("overflow", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class GmtiReport(C.Structure):
    """sarx_gmti_report (48 bytes)"""
    _fields_ = [("i", C.c_int32), ("j", C.c_int32), ("power", C.c_double), ("mean", C.c_double), ("interf_re", C.c_double),
                ("interf_im", C.c_double), ("mag1", C.c_float), ("mag2", C.c_float)]


GMTI_MAX_HALF = 32              # SARX_GMTI_MAX_HALF
GMTI_SIGNATURES = {
    "sarx_gmti_slot_bytes": (_i, [_P(GmtiParams), _P(_sz)]),
    "sarx_gmti_cfar_dev": (_i, [_vp, _vp, _i, _i, _P(GmtiParams), _vp, _vp]),
    "sarx_gmti_refine_dev": (_i, [_vp, _vp, _vp, _i, _i, _d, _vp, _vp, _i]),
}

# include/sarx_refocus.h: the GMTI refocus, a third table bound the same way
REFOCUS_MAX_HYP = 64            # SARX_REFOCUS_MAX_HYP
REFOCUS_MAX_W = 15              # SARX_REFOCUS_MAX_W
REFOCUS_DPCA, REFOCUS_SLC1 = 0, 1


class RefocusParams(C.Structure):
    """sarx_refocus_params (576 bytes)"""
    _fields_ = [("chip_az", C.c_int32), ("chip_rg", C.c_int32), ("source", C.c_int32), ("n_hyp", C.c_int32),
                ("wavelength_m", C.c_double), ("platform_speed_mps", C.c_double), ("prf_hz", C.c_double), ("r0_m", C.c_double),
                ("dr_m", C.c_double), ("cal_phase", C.c_double), ("speed_mps", C.c_double * REFOCUS_MAX_HYP)]


class RefocusRecord(C.Structure):
    """sarx_refocus_record (48 bytes)"""
    _fields_ = [("k_best", C.c_int32), ("i0", C.c_int32), ("peak_i", C.c_int32), ("peak_j", C.c_int32), ("s_prev", C.c_float),
                ("s_best", C.c_float), ("s_next", C.c_float), ("s_identity", C.c_float), ("peak_power", C.c_float),
                ("orig_power", C.c_float), ("reserved", C.c_int32 * 2)]


REFOCUS_SIGNATURES = {
    "sarx_refocus_check": (_i, [_P(RefocusParams), _i, _i]),
    "sarx_refocus_dev": (_i, [_vp, _vp, _vp, _i, _i, _P(RefocusParams), _vp, _vp, _i, _vp, _vp, _vp]),
}

# include/sarx_balance.h: the two-channel balance, a fourth table bound the same way
BALANCE_MIN_BLOCK, BALANCE_MAX_BLOCK, BALANCE_MAX_BLOCKS = 8, 4096, 65536     # SARX_BALANCE_MIN_BLOCK, _MAX_BLOCK, _MAX_BLOCKS
BALANCE_LS, BALANCE_PHASE = 0, 1
BALANCE_NEAREST, BALANCE_BILINEAR = 0, 1


class BalanceParams(C.Structure):
    """sarx_balance_params (40 bytes)"""
    _fields_ = [("block_az", C.c_int32), ("block_rg", C.c_int32), ("mode", C.c_int32), ("interp", C.c_int32),
                ("min_count", C.c_int32), ("reserved", C.c_int32), ("clip_power", C.c_double), ("min_coherence", C.c_double)]


class BalanceHeader(C.Structure):
    """sarx_balance_header: the first 64 bytes of a balance table"""
    _fields_ = [("nb_az", C.c_uint32), ("nb_rg", C.c_uint32), ("n_valid", C.c_uint32), ("reserved", C.c_uint32),
                ("w_re", C.c_double), ("w_im", C.c_double), ("coherence", C.c_double), ("s11", C.c_double), ("s22", C.c_double),
                ("n", C.c_uint64)]


class BalanceRecord(C.Structure):
    """sarx_balance_record (64 bytes)"""
    _fields_ = [("s12_re", C.c_double), ("s12_im", C.c_double), ("s11", C.c_double), ("s22", C.c_double), ("w_re", C.c_double),
                ("w_im", C.c_double), ("coherence", C.c_float), ("n", C.c_uint32), ("valid", C.c_uint32), ("reserved", C.c_uint32)]


BALANCE_SIGNATURES = {
    "sarx_balance_check": (_i, [_P(BalanceParams), _i, _i]),
    "sarx_balance_table_bytes": (_i, [_P(BalanceParams), _i, _i, _P(_sz)]),
    "sarx_balance_workspace_bytes": (_i, [_P(BalanceParams), _i, _i, _P(_sz)]),
    "sarx_balance_estimate_dev": (_i, [_vp, _vp, _vp, _i, _i, _P(BalanceParams), _vp, _vp]),
    "sarx_balance_apply_dev": (_i, [_vp, _vp, _vp, _i, _i, _P(BalanceParams), _vp, _vp, _vp]),
}

# include/sarx_track.h: the GMTI tracker, a fifth table bound the same way
TRACK_MAX_TRACKS, TRACK_MAX_DETECTIONS = 16384, 65536                         # SARX_TRACK_MAX_TRACKS, _MAX_DETECTIONS
TRACK_FREE, TRACK_TENTATIVE, TRACK_CONFIRMED = 0, 1, 2
TRACK_OK, TRACK_ERR_SLOT_OVERFLOW, TRACK_ERR_TABLE_OVERFLOW = 0, 1, 2


class TrackParams(C.Structure):
    """sarx_track_params (64 bytes)"""
    _fields_ = [("gate_az", C.c_double), ("gate_rg", C.c_double), ("alpha", C.c_double), ("beta", C.c_double),
                ("birth_ratio", C.c_double), ("confirm_hits", C.c_int32), ("confirm_window", C.c_int32), ("max_misses", C.c_int32),
                ("max_tracks", C.c_int32), ("max_detections", C.c_int32), ("reserved", C.c_int32)]


class TrackHeader(C.Structure):
    """sarx_track_header: the first 64 bytes of a track table"""
    _fields_ = [("n_live", C.c_uint32), ("n_confirmed", C.c_uint32), ("next_id", C.c_int32), ("frames_done", C.c_uint32),
                ("births_total", C.c_uint32), ("drops_total", C.c_uint32), ("error", C.c_uint32), ("error_frame", C.c_int32),
                ("max_tracks", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class TrackSlot(C.Structure):
    """sarx_track_slot (96 bytes)"""
    _fields_ = [("p_i", C.c_double), ("p_j", C.c_double), ("v_i", C.c_double), ("v_j", C.c_double), ("sum_re", C.c_double),
                ("sum_im", C.c_double), ("sum_power", C.c_double), ("max_ratio", C.c_double), ("id", C.c_int32),
                ("status", C.c_uint32), ("hits", C.c_uint32), ("misses", C.c_uint32), ("age", C.c_uint32), ("hist", C.c_uint32),
                ("last_frame", C.c_int32), ("last_report", C.c_int32)]


TRACK_SIGNATURES = {
    "sarx_track_check": (_i, [_P(TrackParams)]),
    "sarx_track_table_bytes": (_i, [_P(TrackParams), _P(_sz)]),
    "sarx_track_workspace_bytes": (_i, [_P(TrackParams), _P(_sz)]),
    "sarx_track_init_dev": (_i, [_vp, _P(TrackParams), _vp]),
    "sarx_track_step_dev": (_i, [_vp, _P(TrackParams), _vp, _i, _vp, _vp, _vp]),
    "sarx_track_run_dev": (_i, [_vp, _P(TrackParams), _vp, _sz, _i, _vp, _vp, _vp]),
}

# include/sarx_coherence.h: the sliding-window coherence, a sixth table bound the same way
COH_MAX_HALF = 16               # SARX_COH_MAX_HALF


class CoherenceParams(C.Structure):
    """sarx_coherence_params (32 bytes)"""
    _fields_ = [("ha", C.c_int32), ("hr", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32), ("threshold", C.c_double),
                ("power_floor", C.c_double)]


class CoherenceSummary(C.Structure):
    """sarx_coherence_summary (64 bytes)"""
    _fields_ = [("n_tested", C.c_uint64), ("n_changed", C.c_uint64), ("sum_coh", C.c_double), ("n_az", C.c_uint32),
                ("n_rg", C.c_uint32), ("reserved", C.c_uint32 * 8)]


COHERENCE_SIGNATURES = {
    "sarx_coherence_check": (_i, [_P(CoherenceParams), _i, _i]),
    "sarx_coherence_workspace_bytes": (_i, [_P(CoherenceParams), _i, _i, _P(_sz)]),
    "sarx_coherence_pair_dev": (_i, [_vp, _vp, _vp, _i, _i, _P(CoherenceParams), _vp, _vp, _vp, _vp, _vp]),
    "sarx_coherence_stack_dev": (_i, [_vp, _vp, _i, _sz, _i, _i, _i, _P(CoherenceParams), _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
}

# include/sarx_oscfar.h: the ordered-statistic CFAR launch, a seventh table bound the same way
class OscfarParams(C.Structure):
    """sarx_oscfar_params (40 bytes)"""
    _fields_ = [("base", GmtiParams), ("rank", C.c_int32), ("flags", C.c_int32)]


OSCFAR_SIGNATURES = {
    "sarx_oscfar_check": (_i, [_P(OscfarParams)]),
    "sarx_gmti_oscfar_dev": (_i, [_vp, _vp, _i, _i, _P(OscfarParams), _vp, _vp]),
}

# include/sarx_cluster.h: the GMTI plot extraction, an eighth table bound the same way
CLUSTER_MAX_LINK, CLUSTER_MAX_DETECTIONS = 64, 16384                          # SARX_CLUSTER_MAX_LINK, _MAX_DETECTIONS


class ClusterParams(C.Structure):
    """sarx_cluster_params (16 bytes)"""
    _fields_ = [("link_az", C.c_int32), ("link_rg", C.c_int32), ("min_members", C.c_int32), ("max_detections", C.c_int32)]


class ClusterPlot(C.Structure):
    """sarx_cluster_plot (64 bytes)"""
    _fields_ = [("n_members", C.c_int32), ("peak_report", C.c_int32), ("i_min", C.c_int32), ("i_max", C.c_int32), ("j_min", C.c_int32),
                ("j_max", C.c_int32), ("sum_power", C.c_double), ("centroid_i", C.c_double), ("centroid_j", C.c_double),
                ("max_ratio", C.c_double), ("reserved", C.c_uint32 * 2)]


CLUSTER_SIGNATURES = {
    "sarx_cluster_check": (_i, [_P(ClusterParams)]),
    "sarx_cluster_plots_bytes": (_i, [_P(ClusterParams), _P(_sz)]),
    "sarx_cluster_step_dev": (_i, [_vp, _P(ClusterParams), _vp, _vp, _vp, _vp]),
    "sarx_cluster_run_dev": (_i, [_vp, _P(ClusterParams), _vp, _sz, _vp, _sz, _i, _vp, _sz, _vp]),
}

# include/sarx_atigate.h: the GMTI ATI gate, a ninth table bound the same way
ATIGATE_MAX_LOOK, ATIGATE_MAX_DETECTIONS, ATIGATE_KEEP_UNTESTED = 4, 16384, 1  # SARX_ATIGATE_MAX_LOOK, _MAX_DETECTIONS, _KEEP_UNTESTED


class AtiGateParams(C.Structure):
    """sarx_atigate_params (64 bytes)"""
    _fields_ = [("guard_az", C.c_int32), ("guard_rg", C.c_int32), ("train_az", C.c_int32), ("train_rg", C.c_int32),
                ("look_az", C.c_int32), ("look_rg", C.c_int32), ("k_sigma", C.c_double), ("phase_min", C.c_double),
                ("min_coh", C.c_double), ("min_train", C.c_int32), ("max_detections", C.c_int32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class AtiGateStat(C.Structure):
    """sarx_atigate_stat (96 bytes)"""
    _fields_ = [(n, C.c_double) for n in ("c11", "c22", "c12_re", "c12_im", "i_re", "i_im", "coh", "psi", "sigma")] + \
               [(n, C.c_int32) for n in ("n_train", "n_look", "status", "reason", "out_index", "reserved")]


ATIGATE_SIGNATURES = {
    "sarx_atigate_check": (_i, [_P(AtiGateParams)]),
    "sarx_atigate_stats_bytes": (_i, [_P(AtiGateParams), _P(_sz)]),
    "sarx_atigate_step_dev": (_i, [_vp, _P(AtiGateParams), _vp, _vp, _i, _i, _vp, _vp, _vp]),
}

# include/sarx_tdbp_search.h: the back-projection's focus-velocity search, a tenth table bound the same way
TDBP_SEARCH_MAX_HYP, TDBP_SEARCH_MAX_CHUNKS = 1024, 64                        # SARX_TDBP_SEARCH_MAX_HYP, _MAX_CHUNKS


class TdbpSearchRecord(C.Structure):
    """sarx_tdbp_search_record (32 bytes)"""
    _fields_ = [("s2", C.c_double), ("s4", C.c_double), ("peak", C.c_double), ("peak_ix", C.c_int32), ("peak_iy", C.c_int32)]


TDBP_SEARCH_SIGNATURES = {
    "sarx_tdbp_search_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _d, _vp, _i, _d, _vp, _vp]),
    "sarx_tdbp_search_host": (_i, [_vp, _vp, _vp, _vp, _vp, _d, _vp, _i, _d, _vp, _vp]),
    "sarx_tdbp_search_route": (_i, [_vp, _P(_i)]),
    "sarx_tdbp_search_set_chunks": (_i, [_vp, _i]),
    "sarx_tdbp_search_metric_dev": (_i, [_vp, _vp, _i, _vp]),
}

# include/sarx_tdbp_pair.h: the two-receiver back-projection, an eleventh table bound the same way


class TdbpPairParams(C.Structure):
    """sarx_tdbp_pair_params (40 bytes)"""
    _fields_ = [("rx_offset_m", C.c_double * 2), ("chirp_centre_s", C.c_double), ("first_pulse", C.c_int32 * 2), ("n_used", C.c_int32),
                ("reserved", C.c_int32)]


TDBP_PAIR_SIGNATURES = {
    "sarx_tdbp_pair_check": (_i, [_i, _P(TdbpPairParams)]),
    "sarx_tdbp_pair_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _d, _vp, _d, _P(TdbpPairParams), _vp, _vp]),
    "sarx_tdbp_pair_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _d, _vp, _d, _P(TdbpPairParams), _vp, _vp]),
    "sarx_tdbp_pair_route": (_i, [_vp, _P(_i)]),
}

# include/sarx_tdbp_pair_search.h: the focus-velocity search on the pair per GMTI report, a twelfth table bound the same way
TDBP_PAIR_SEARCH_MAX_HYP, TDBP_PAIR_SEARCH_MIN_CHIP, TDBP_PAIR_SEARCH_MAX_CHIP = 64, 4, 64      # SARX_TDBP_PAIR_SEARCH_MAX_HYP, _MIN_CHIP, _MAX_CHIP
TDBP_PAIR_SEARCH_MAX_CHIPS = 65535                                                              # SARX_TDBP_PAIR_SEARCH_MAX_CHIPS
TDBP_PAIR_SEARCH_DPCA, TDBP_PAIR_SEARCH_CH0 = 0, 1


class TdbpPairSearchParams(C.Structure):
    """sarx_tdbp_pair_search_params (16 bytes)"""
    _fields_ = [("chip_x", C.c_int32), ("chip_y", C.c_int32), ("n_hyp", C.c_int32), ("source", C.c_int32)]


class TdbpPairSearchBest(C.Structure):
    """sarx_tdbp_pair_search_best (80 bytes)"""
    _fields_ = [("k_best", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("peak_ix", C.c_int32), ("peak_iy", C.c_int32),
                ("reserved", C.c_int32), ("s4_prev", C.c_double), ("s4_best", C.c_double), ("s4_next", C.c_double),
                ("interf_re", C.c_double), ("interf_im", C.c_double), ("p0", C.c_double), ("p1", C.c_double)]


_PAIR_SEARCH_ARGS = [_vp, _vp, _vp, _vp, _vp, _vp, _d, _d, _P(TdbpPairParams), _vp, _vp, _vp, _i, _P(TdbpPairSearchParams), _vp, _vp, _vp]
TDBP_PAIR_SEARCH_SIGNATURES = {
    "sarx_tdbp_pair_search_check": (_i, [_P(TdbpPairSearchParams), _i, _i]),
    "sarx_tdbp_pair_search_dev": (_i, _PAIR_SEARCH_ARGS),
    "sarx_tdbp_pair_search_host": (_i, _PAIR_SEARCH_ARGS),
    "sarx_tdbp_pair_search_route": (_i, [_vp, _P(_i)]),
}

# include/sarx_tdbp_multi.h: the N-receiver back-projection and the multi-baseline ATI resolver, a thirteenth table bound the same way
TDBP_MULTI_MAX_RX, TDBP_MULTI_MAX_HALF, TDBP_MULTI_MAX_CANDIDATES, TDBP_MULTI_MAX_DETECTIONS = 4, 4, 129, 16384      # SARX_TDBP_MULTI_MAX_*
TDBP_MULTI_OK, TDBP_MULTI_NO_CANDIDATE, TDBP_MULTI_ZERO, TDBP_MULTI_OVERFLOW = 0, 1, 2, 3


class TdbpMultiParams(C.Structure):
    """sarx_tdbp_multi_params (64 bytes)"""
    _fields_ = [("rx_offset_m", C.c_double * 4), ("chirp_centre_s", C.c_double), ("first_pulse", C.c_int32 * 4), ("n_used", C.c_int32),
                ("n_rx", C.c_int32)]


class TdbpMultiResolveParams(C.Structure):
    """sarx_tdbp_multi_resolve_params (56 bytes)"""
    _fields_ = [("lag_s", C.c_double * 3), ("wavelength_m", C.c_double), ("v_max_mps", C.c_double), ("n_rx", C.c_int32), ("half", C.c_int32),
                ("max_detections", C.c_int32), ("reserved", C.c_int32)]


class TdbpMultiRecord(C.Structure):
    """sarx_tdbp_multi_record (64 bytes)"""
    _fields_ = [("v_los", C.c_double), ("v_coarse", C.c_double), ("cost", C.c_double), ("cost_next", C.c_double), ("phase", C.c_double * 3),
                ("k", C.c_int32), ("status", C.c_uint32)]


_MULTI_ARGS = [_vp, _P(_vp), _vp, _vp, _vp, _d, _vp, _d, _P(TdbpMultiParams), _vp, _vp]
TDBP_MULTI_SIGNATURES = {
    "sarx_tdbp_multi_check": (_i, [_i, _P(TdbpMultiParams)]),
    "sarx_tdbp_multi_dev": (_i, _MULTI_ARGS),
    "sarx_tdbp_multi_host": (_i, _MULTI_ARGS),
    "sarx_tdbp_multi_route": (_i, [_vp, _P(_i)]),
    "sarx_tdbp_multi_scratch": (_i, [_vp, _P(_u64), _P(_u64)]),
    "sarx_tdbp_multi_resolve_check": (_i, [_P(TdbpMultiResolveParams)]),
    "sarx_tdbp_multi_resolve_dev": (_i, [_vp, _P(TdbpMultiResolveParams), _vp, _i, _i, _vp, _vp]),
}

# include/sarx_relocate.h: the ground relocation of GMTI reports, a fourteenth table bound the same way
RELOCATE_OK, RELOCATE_NO_SPEED, RELOCATE_NO_SOLUTION, RELOCATE_OFF_GRID, RELOCATE_OVERFLOW = 0, 1, 2, 3, 4      # SARX_RELOCATE_*
RELOCATE_HAS_VELOCITY = 1


class RelocateParams(C.Structure):
    """sarx_relocate_params (128 bytes)"""
    _fields_ = [("pos_ref", C.c_double * 3), ("vel_ref", C.c_double * 3), ("in_x0", C.c_double), ("in_y0", C.c_double), ("in_dx", C.c_double),
                ("in_dy", C.c_double), ("out_x0", C.c_double), ("out_y0", C.c_double), ("out_dx", C.c_double), ("out_dy", C.c_double),
                ("out_nx", C.c_int32), ("out_ny", C.c_int32), ("max_detections", C.c_int32), ("reserved", C.c_int32)]


class RelocateRecord(C.Structure):
    """sarx_relocate_record (64 bytes)"""
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("shift_x", C.c_double), ("shift_y", C.c_double), ("vx", C.c_double), ("vy", C.c_double),
                ("rank", C.c_int32), ("status", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


RELOCATE_SIGNATURES = {
    "sarx_relocate_check": (_i, [_P(RelocateParams)]),
    "sarx_relocate_dev": (_i, [_vp, _P(RelocateParams), _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
}

# include/sarx_ktrack.h: the Kalman ground tracker, a fifteenth table bound the same way
KTRACK_MAX_TRACKS, KTRACK_MAX_DETECTIONS = 16384, 16384                       # SARX_KTRACK_MAX_TRACKS, _MAX_DETECTIONS
KTRACK_FREE, KTRACK_TENTATIVE, KTRACK_CONFIRMED = 0, 1, 2
KTRACK_OK, KTRACK_ERR_SLOT_OVERFLOW, KTRACK_ERR_TABLE_OVERFLOW, KTRACK_ERR_TIME = 0, 1, 2, 3


class KtrackParams(C.Structure):
    """sarx_ktrack_params (80 bytes)"""
    _fields_ = [("sigma_pos", C.c_double), ("sigma_v", C.c_double), ("sigma_v_tan", C.c_double), ("q", C.c_double), ("gate_d2", C.c_double),
                ("gate_m", C.c_double), ("birth_ratio", C.c_double), ("confirm_hits", C.c_int32), ("confirm_window", C.c_int32),
                ("max_misses", C.c_int32), ("max_tracks", C.c_int32), ("max_detections", C.c_int32), ("reserved", C.c_int32)]


class KtrackFrame(C.Structure):
    """sarx_ktrack_frame (64 bytes)"""
    _fields_ = [("t", C.c_double), ("pos_ref", C.c_double * 3), ("vel_ref", C.c_double * 3), ("frame_index", C.c_int32), ("reserved", C.c_int32)]


class KtrackHeader(C.Structure):
    """sarx_ktrack_header: the first 64 bytes of a Kalman track table"""
    _fields_ = [("n_live", C.c_uint32), ("n_confirmed", C.c_uint32), ("next_id", C.c_int32), ("frames_done", C.c_uint32),
                ("births_total", C.c_uint32), ("drops_total", C.c_uint32), ("error", C.c_uint32), ("error_frame", C.c_int32),
                ("max_tracks", C.c_uint32), ("reserved0", C.c_uint32), ("t_last", C.c_double), ("reserved", C.c_uint32 * 4)]


class KtrackSlot(C.Structure):
    """sarx_ktrack_slot (192 bytes)"""
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("vx", C.c_double), ("vy", C.c_double), ("p", C.c_double * 10), ("sum_re", C.c_double),
                ("sum_im", C.c_double), ("sum_power", C.c_double), ("max_ratio", C.c_double), ("nis_last", C.c_double), ("nis_sum", C.c_double),
                ("id", C.c_int32), ("status", C.c_uint32), ("hits", C.c_uint32), ("misses", C.c_uint32), ("age", C.c_uint32),
                ("hist", C.c_uint32), ("last_frame", C.c_int32), ("last_report", C.c_int32)]


KTRACK_SIGNATURES = {
    "sarx_ktrack_check": (_i, [_P(KtrackParams)]),
    "sarx_ktrack_table_bytes": (_i, [_P(KtrackParams), _P(_sz)]),
    "sarx_ktrack_workspace_bytes": (_i, [_P(KtrackParams), _P(_sz)]),
    "sarx_ktrack_init_dev": (_i, [_vp, _P(KtrackParams), _vp]),
    "sarx_ktrack_step_dev": (_i, [_vp, _P(KtrackParams), _P(KtrackFrame), _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "sarx_ktrack_run_dev": (_i, [_vp, _P(KtrackParams), _P(KtrackFrame), _i, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp]),
}

# include/sarx_pga.h: the phase-gradient autofocus, a sixteenth table bound the same way
PGA_MAX_ITER, PGA_MAX_RG, PGA_MAX_FRAMES = 8, 1 << 20, 65535                  # SARX_PGA_MAX_ITER, _MAX_RG, _MAX_FRAMES
PGA_SIZES = (64, 128, 256, 512, 1024)


class PgaParams(C.Structure):
    """sarx_pga_params (56 bytes)"""
    _fields_ = [("n_iter", C.c_int32), ("half_width", C.c_int32 * PGA_MAX_ITER), ("reserved", C.c_int32), ("min_contrast", C.c_double),
                ("power_floor", C.c_double)]


class PgaRecord(C.Structure):
    """sarx_pga_record (32 bytes)"""
    _fields_ = [("s2", C.c_double), ("s4", C.c_double), ("rms_phase", C.c_double), ("n_cols_used", C.c_int32),
                ("n_bins_supported", C.c_int32)]


PGA_SIGNATURES = {
    "sarx_pga_check": (_i, [_P(PgaParams), _i, _i, _sz, _i, _sz]),
    "sarx_pga_workspace_bytes": (_i, [_P(PgaParams), _i, _i, _sz, _i, _sz, _P(_sz)]),
    "sarx_pga_dev": (_i, [_vp, _vp, _vp, _i, _i, _sz, _i, _sz, _P(PgaParams), _vp, _vp, _vp]),
    "sarx_pga_apply_dev": (_i, [_vp, _vp, _vp, _i, _i, _sz, _i, _sz, _vp, _sz, _i]),
}

_lib = None


def load():
    """Load libsarx.so once and attach prototypes.  Fails loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SarxError(-3, f"{LIB_PATH} not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "or `make -C nis-sar-amtigmti-video_amd/csrc` (hipcc, gfx950). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(GMTI_SIGNATURES.items()) + list(REFOCUS_SIGNATURES.items()) + \
            list(BALANCE_SIGNATURES.items()) + list(TRACK_SIGNATURES.items()) + list(COHERENCE_SIGNATURES.items()) + list(OSCFAR_SIGNATURES.items()) + \
            list(CLUSTER_SIGNATURES.items()) + list(ATIGATE_SIGNATURES.items()) + list(TDBP_SEARCH_SIGNATURES.items()) + \
            list(TDBP_PAIR_SIGNATURES.items()) + list(TDBP_PAIR_SEARCH_SIGNATURES.items()) + list(TDBP_MULTI_SIGNATURES.items()) + \
            list(RELOCATE_SIGNATURES.items()) + list(KTRACK_SIGNATURES.items()) + list(PGA_SIGNATURES.items()):
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, ctx=None):
    if rc != 0:
        msg = load().sarx_last_error(ctx)
        raise SarxError(rc, msg.decode() if msg else "unknown")
