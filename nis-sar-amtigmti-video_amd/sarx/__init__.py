"""sarx: MI355X-native backend for the CSA focus + ATI/DPCA path.

Python host code with the reference's function signatures over a ctypes C ABI
(include/sarx.h) to hand-written HIP kernels (csrc/).  No torch on this path.
"""
from ._ffi import SarxError
from .engine import Context, CsaPlan, DeviceArray, DeviceBuffer, FocusLanes, default_context, device_count
from .echo import run_bistatic_physics_gpu, run_custom_physics, run_moving_physics, run_physics_engine
from .rda import sar_focus_rda
from .noise import calculate_snr_db, add_ocean_noise, add_noise_dev, add_noise_rel_dev, power_stats
from .tdbp import (tdbp_gpu, run_physics_spotlight, calculate_raw_snr_db, generate_noise_tensor, batch_constants,
                   orbit_arc, TdbpPlan)
from .gmti import GmtiOverflowError, GmtiParams, GmtiReport, gmti_detect
from .refocus import RefocusParams, RefocusResult, gmti_refocus
from .balance import BalanceParams, ChannelBalance, channel_balance
from .coherence import CoherenceParams, CoherenceResult, coherence, coherence_stack
from .track import GmtiTracker, TrackOverflowError, TrackParams, TrackResult, gmti_track
from .cluster import ClusterParams, GmtiPlots, gmti_cluster
from .atigate import AtiGateParams, gmti_ati_gate
from .tdbp_search import TdbpSearchResult, tdbp_autofocus, tdbp_search, tdbp_velocity_line
from .tdbp_pair import TdbpPairResult, tdbp_pair
from .tdbp_pair_search import TdbpPairSearchResult, tdbp_pair_search
from .tdbp_multi import TdbpMultiResult, tdbp_multi
from .relocate import RelocateResult, ground_relocate, reference_geometry, relocate_frames
from .ktrack import GroundTracker, KalmanTrackParams, KalmanTrackResult, TrackTimeError, ground_track
from .pga import PgaParams, PgaResult, apply_azimuth_phase, pga
from .focus import (FocusFuture, ati_dpca, clear_plan_cache, dpca_pulse_shift, focus_ati_dpca, focus_stream, phase_balance,
                    sar_focus_csa, sar_focus_csa_async, two_channel_workspace)

__all__ = ["SarxError", "Context", "CsaPlan", "FocusLanes", "add_noise_rel_dev", "DeviceArray", "DeviceBuffer", "default_context", "device_count", "sar_focus_csa", "sar_focus_csa_async", "focus_stream", "FocusFuture", "ati_dpca",
           "dpca_pulse_shift", "phase_balance", "focus_ati_dpca", "two_channel_workspace", "clear_plan_cache", "run_physics_engine",
           "run_bistatic_physics_gpu", "run_moving_physics", "run_custom_physics", "sar_focus_rda", "calculate_snr_db", "add_ocean_noise", "add_noise_dev", "power_stats", "tdbp_gpu", "run_physics_spotlight", "calculate_raw_snr_db",
           "generate_noise_tensor", "batch_constants", "orbit_arc", "TdbpPlan", "gmti_detect", "GmtiParams", "GmtiReport",
           "GmtiOverflowError", "gmti_refocus", "RefocusParams", "RefocusResult", "channel_balance", "BalanceParams", "ChannelBalance",
           "coherence", "coherence_stack", "CoherenceParams", "CoherenceResult",
           "gmti_track", "GmtiTracker", "TrackParams", "TrackResult", "TrackOverflowError",
           "gmti_cluster", "ClusterParams", "GmtiPlots", "gmti_ati_gate", "AtiGateParams",
           "tdbp_search", "tdbp_velocity_line", "tdbp_autofocus", "TdbpSearchResult",
           "tdbp_pair", "TdbpPairResult", "tdbp_pair_search", "TdbpPairSearchResult",
           "tdbp_multi", "TdbpMultiResult",
           "ground_relocate", "reference_geometry", "relocate_frames", "RelocateResult",
           "ground_track", "GroundTracker", "KalmanTrackParams", "KalmanTrackResult", "TrackTimeError",
           "pga", "apply_azimuth_phase", "PgaParams", "PgaResult"]
