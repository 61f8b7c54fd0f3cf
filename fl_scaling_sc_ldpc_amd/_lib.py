"""ctypes binding of libscldpc_hip.so (C-ABI: include/scldpc.h).

The library is built in-tree by `make -C fl_scaling_sc_ldpc_amd/csrc` (or __graft_entry__.build()).
There is NO fallback: if the shared object is missing or a call fails, an exception is raised.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# SCLDPC_LIB_PATH: diagnostics only (tools/stamps.py loads the stamped build of the same sources)
LIB_PATH = os.environ.get("SCLDPC_LIB_PATH") or os.path.join(HERE, "libscldpc_hip.so")

NCOUNTERS = 8
NRUN = 9
MAX_CAPS = 16                   # SCLDPC_MAX_CAPS
NPEELRUN = 8
PEELRUN_NAMES = ("trials", "fuckups", "lost", "fuckups_exp", "lost_exp", "blocks_exp")     # SCLDPC_PR_*
COUNTER_NAMES = ("num_erasures", "num_blocks_err", "num_erasures_exp", "num_blocks_err_exp",
                 "num_erasures_p1", "iterations", "status", "channel_erasures")
RUN_NAMES = ("users_err", "frame_err", "frame_err_p1", "block_err", "users_err_exp", "frame_err_exp",
             "block_err_exp", "frames", "iterations")

# every symbol include/scldpc.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "scldpc_abi_version", "scldpc_last_error", "scldpc_device_count",
    "scldpc_sample_glibc_host", "scldpc_glibc_state_bytes", "scldpc_glibc_state_init",
    "scldpc_glibc_state_reset_perm", "scldpc_sample_glibc_next_host",
    "scldpc_sample_philox_device", "scldpc_full_bp_device", "scldpc_sw_bp_device",
    "scldpc_accumulate_run_device", "scldpc_full_bp_lds_bytes",
    "scldpc_sample_philox_device_adj16", "scldpc_full_bp_device_adj16", "scldpc_sw_bp_device_adj16",
    "scldpc_peel_sweep_device", "scldpc_peel_sweep_device_adj16",
    "scldpc_peel_pick_device", "scldpc_peel_pick_device_adj16", "scldpc_r1_moments_device",
    "scldpc_stream_state_bytes", "scldpc_stream_run_device",
    "scldpc_swc_bp_device", "scldpc_swc_bp_device_adj16", "scldpc_sample_philox_ensemble_device",
    "scldpc_full_bp_fixpoint_device", "scldpc_full_bp_fixpoint_device_adj16",
    "scldpc_sample_philox_cn16_supported", "scldpc_sample_philox_device_cn16",
    "scldpc_sample_philox_sock16_supported", "scldpc_sample_philox_device_sock16",
    "scldpc_full_bp_cn16_supported", "scldpc_full_bp_fixpoint_device_cn16", "scldpc_full_bp_device_cn16",
    "scldpc_stream_glibc_inputs_host", "scldpc_stream_run_device_inputs", "scldpc_workspace_bytes",
    "scldpc_sw_bp_ring_supported", "scldpc_cn_sockets_device", "scldpc_sw_bp_ring_device",
    "scldpc_accumulate_peel_device", "scldpc_clear_channel_range_device",
    "scldpc_stream_glibc_next_host", "scldpc_stream_run_device_inputs_at",
    "scldpc_full_bp_sock16_supported", "scldpc_full_bp_fixpoint_device_sock16", "scldpc_full_bp_device_sock16",
    "scldpc_full_bp_traj_device_cn16", "scldpc_full_bp_traj_device_sock16",
    "scldpc_full_bp_caps_device_cn16", "scldpc_full_bp_caps_device_sock16",
    "scldpc_full_bp_wide_supported", "scldpc_full_bp_device_wide", "scldpc_full_bp_traj_device_wide",
    "scldpc_full_bp_deg_supported", "scldpc_full_bp_deg_wide_supported", "scldpc_full_bp_fixpoint_device_deg",
    "scldpc_full_bp_device_deg", "scldpc_full_bp_traj_device_deg", "scldpc_full_bp_device_deg_wide",
    "scldpc_full_bp_traj_device_deg_wide",
    "scldpc_full_bp_caps_device_wide", "scldpc_full_bp_caps_device_deg", "scldpc_full_bp_caps_device_deg_wide",
    "scldpc_sw_bp_ring_deg_supported", "scldpc_sw_bp_ring_device_deg",
    "scldpc_stream_supported",
    "scldpc_swc_bp_ring_supported", "scldpc_swc_bp_ring_device",
    "scldpc_sample_philox_adj16_sock_supported", "scldpc_sample_philox_device_adj16_sock",
    "scldpc_sample_philox_deg_sock16_supported", "scldpc_sample_philox_device_deg_sock16",
    "scldpc_sample_philox_wide_sock16_supported", "scldpc_sample_philox_device_wide_sock16",
    "scldpc_peel_sweep_sock16_supported", "scldpc_peel_sweep_device_sock16",
    "scldpc_peel_sweep_wide_supported", "scldpc_peel_sweep_device_sock16_wide",
    "scldpc_peel_pick_deg_supported", "scldpc_peel_pick_deg_workspace_bytes", "scldpc_peel_pick_device_adj16_deg",
)

# every symbol the extension header include/scldpc_ensembles.h declares (the same shared object; tests/test_sweep_ens_host.py)
EXPORTS_ENSEMBLES = (
    "scldpc_sample_philox_ensemble_adj16_sock_supported", "scldpc_sample_philox_ensemble_device_adj16_sock",
    "scldpc_peel_sweep_tb_supported", "scldpc_peel_sweep_tb_wide_supported",
    "scldpc_peel_sweep_device_sock16_tb", "scldpc_peel_sweep_device_sock16_tb_wide",
)

# every symbol the extension header include/scldpc_uncoupled.h declares (the same shared object; tests/test_uncoupled_host.py)
EXPORTS_UNCOUPLED = ("scldpc_sample_philox_uncoupled_supported", "scldpc_sample_philox_uncoupled_device")

# every symbol the extension header include/scldpc_uncoupled_wide.h declares (the same shared object;
# tests/test_uncoupled_wide_host.py)
EXPORTS_UNCOUPLED_WIDE = ("scldpc_sample_philox_uncoupled_wide_supported", "scldpc_sample_philox_uncoupled_wide_device")

# every symbol the extension header include/scldpc_cov.h declares (the same shared object; tests/test_cov_host.py)
EXPORTS_COV = ("scldpc_r1_gram_workspace_bytes", "scldpc_r1_gram_trial_splits", "scldpc_r1_gram_device")
COV_MAX_STEPS = 4096            # SCLDPC_COV_MAX_STEPS

# every symbol the extension header include/scldpc_ss.h declares (the same shared object; tests/test_ss_host.py)
EXPORTS_SS = ("scldpc_ss_spectrum_form", "scldpc_ss_spectrum_workspace_bytes", "scldpc_ss_spectrum_device")
SS_MAX_BINS = 4096              # SCLDPC_SS_MAX_BINS
SS_POS_SIZES = 8                # SCLDPC_SS_POS_SIZES
SS_BAD_CN = 1                   # SCLDPC_SS_BAD_CN

# every symbol the extension header include/scldpc_runs.h declares (the same shared object; tests/test_runs_host.py)
EXPORTS_RUNS = ("scldpc_chain_runs_device", "scldpc_stream_runs_device")
RUNS_MAX_L = 1024               # SCLDPC_RUNS_MAX_L
RUNS_MAX_BINS = 4096            # SCLDPC_RUNS_MAX_BINS
RUNS_MAX_PERIOD = 4096          # SCLDPC_RUNS_MAX_PERIOD
RUNS_CARRY = 8                  # SCLDPC_RUNS_CARRY

# every symbol the extension header include/scldpc_eps.h declares (the same shared object; tests/test_eps_host.py)
EXPORTS_EPS = ("scldpc_channel_levels_device", "scldpc_peel_sweep_eps_device", "scldpc_peel_sweep_eps_device_adj16",
               "scldpc_peel_sweep_eps_workspace_query")
EPS_MAX_POINTS = 64             # SCLDPC_EPS_MAX_POINTS

# every symbol the extension header include/scldpc_bp_eps.h declares (the same shared object; tests/test_bp_eps_host.py)
EXPORTS_BP_EPS = ("scldpc_full_bp_eps_device", "scldpc_full_bp_eps_device_adj16", "scldpc_full_bp_eps_workspace_query")

# every symbol the extension header include/scldpc_thresh.h declares (the same shared object; tests/test_thresh_host.py)
EXPORTS_THRESH = ("scldpc_channel_keys_device", "scldpc_frame_threshold_device", "scldpc_frame_threshold_device_adj16",
                  "scldpc_frame_threshold_workspace_query")
THRESH_NCOLS = 8                # SCLDPC_THRESH_NCOLS
THRESH_MAX = 2147483647         # SCLDPC_THRESH_MAX
THRESH_NAMES = ("thresh", "status", "size", "first_pos", "last_pos", "stages", "rescans", "channel_erasures")

# every symbol the extension header include/scldpc_vn_thresh.h declares (the same shared object; tests/test_vn_thresh_host.py)
EXPORTS_VN_THRESH = ("scldpc_vn_threshold_device", "scldpc_vn_threshold_device_adj16", "scldpc_vn_threshold_workspace_query")
VNT_NCOLS = 8                   # SCLDPC_VNT_NCOLS
VNT_MAX_POINTS = 256            # SCLDPC_VNT_MAX_POINTS
VNT_NONE = 0xFFFFFFFF           # SCLDPC_VNT_NONE
VNT_NAMES = ("thresh", "status", "top_size", "size", "steps", "scans", "rescans", "channel_erasures")


class ScldpcError(RuntimeError):
    pass


class CodeParams(C.Structure):
    """scldpc_code_params — (dv, dc, L, cns_pos, vns_pos); see include/scldpc.h for the naming trap."""
    _fields_ = [("dv", C.c_int32), ("dc", C.c_int32), ("L", C.c_int32), ("cns_pos", C.c_int32),
                ("vns_pos", C.c_int32)]

    @property
    def n(self):
        return self.vns_pos * self.L

    @property
    def nk(self):
        return (self.L + self.dv - 1) * self.cns_pos

    @property
    def nw(self):
        return (self.n + 31) // 32

    @property
    def edges(self):
        return self.n * self.dv

    def key(self):
        return (self.dv, self.dc, self.L, self.cns_pos, self.vns_pos)


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ScldpcError(f"{LIB_PATH} is missing — build it with `make -C fl_scaling_sc_ldpc_amd/csrc` "
                          "(hipcc, gfx950).  There is no CPU fallback.")
    # PyTorch's copy of the HIP runtime first: loaded after this library it would be a second runtime in the process, and
    # whichever of the two touches the GPU second finds no device
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    vp, i32, i64, u32, u64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_double
    pp = P(CodeParams)
    L.scldpc_abi_version.restype = C.c_int
    L.scldpc_last_error.restype = C.c_char_p
    L.scldpc_device_count.restype = C.c_int
    L.scldpc_sample_glibc_host.argtypes = [pp, u32, dbl, i32, vp, vp, vp]
    L.scldpc_glibc_state_bytes.argtypes = [pp]
    L.scldpc_glibc_state_bytes.restype = i64
    L.scldpc_glibc_state_init.argtypes = [pp, u32, vp]
    L.scldpc_glibc_state_reset_perm.argtypes = [pp, vp]
    L.scldpc_sample_glibc_next_host.argtypes = [pp, vp, dbl, i32, vp, i32, vp, vp]
    L.scldpc_workspace_bytes.argtypes = [i32, pp, i32, i32, i32]
    L.scldpc_workspace_bytes.restype = i64
    L.scldpc_sample_philox_device.argtypes = [pp, u64, u64, i32, dbl, i32, vp, vp, vp, vp, u64, vp]
    L.scldpc_sample_philox_ensemble_device.argtypes = [pp, i32, u64, u64, i32, dbl, i32, vp, vp, vp, vp]
    L.scldpc_full_bp_fixpoint_device.argtypes = [pp, i32, vp, vp, i32, vp, vp, vp, u64, vp]
    L.scldpc_full_bp_fixpoint_device_adj16.argtypes = L.scldpc_full_bp_fixpoint_device.argtypes
    L.scldpc_sample_philox_cn16_supported.argtypes = [pp]
    L.scldpc_full_bp_cn16_supported.argtypes = [pp]
    L.scldpc_sample_philox_device_cn16.argtypes = [pp, u64, u64, i32, dbl, i32, vp, vp, vp, vp, vp]
    L.scldpc_sample_philox_sock16_supported.argtypes = [pp]
    L.scldpc_sample_philox_device_sock16.argtypes = [pp, u64, u64, i32, dbl, i32, vp, vp, vp, vp, vp]
    L.scldpc_sample_philox_deg_sock16_supported.argtypes = [pp]
    L.scldpc_sample_philox_device_deg_sock16.argtypes = [pp, u64, u64, i32, dbl, i32, vp, vp, vp, vp, vp]
    L.scldpc_sample_philox_wide_sock16_supported.argtypes = [pp]
    L.scldpc_sample_philox_device_wide_sock16.argtypes = [pp, u64, u64, i32, dbl, i32, vp, vp, vp, vp, vp]
    L.scldpc_sample_philox_adj16_sock_supported.argtypes = [pp]
    L.scldpc_sample_philox_device_adj16_sock.argtypes = [pp, u64, u64, i32, dbl, i32, vp, vp, vp, vp, vp, u64, vp]
    L.scldpc_full_bp_fixpoint_device_cn16.argtypes = [pp, i32, vp, vp, vp, i32, vp, vp, vp]
    L.scldpc_full_bp_device_cn16.argtypes = [pp, i32, vp, vp, vp, i32, i32, vp, vp, vp]
    L.scldpc_full_bp_sock16_supported.argtypes = [pp]
    L.scldpc_full_bp_fixpoint_device_sock16.argtypes = L.scldpc_full_bp_fixpoint_device_cn16.argtypes
    L.scldpc_full_bp_device_sock16.argtypes = L.scldpc_full_bp_device_cn16.argtypes
    L.scldpc_full_bp_traj_device_cn16.argtypes = [pp, i32, vp, vp, vp, i32, i32, vp, vp, i32, vp, vp]
    L.scldpc_full_bp_traj_device_sock16.argtypes = L.scldpc_full_bp_traj_device_cn16.argtypes
    L.scldpc_full_bp_caps_device_cn16.argtypes = [pp, i32, vp, vp, vp, i32, vp, i32, vp, vp]
    L.scldpc_full_bp_caps_device_sock16.argtypes = L.scldpc_full_bp_caps_device_cn16.argtypes
    L.scldpc_full_bp_wide_supported.argtypes = [pp]
    L.scldpc_full_bp_device_wide.argtypes = L.scldpc_full_bp_device_cn16.argtypes
    L.scldpc_full_bp_traj_device_wide.argtypes = L.scldpc_full_bp_traj_device_cn16.argtypes
    L.scldpc_full_bp_deg_supported.argtypes = [pp]
    L.scldpc_full_bp_deg_wide_supported.argtypes = [pp]
    L.scldpc_full_bp_fixpoint_device_deg.argtypes = L.scldpc_full_bp_fixpoint_device_cn16.argtypes
    L.scldpc_full_bp_device_deg.argtypes = L.scldpc_full_bp_device_cn16.argtypes
    L.scldpc_full_bp_device_deg_wide.argtypes = L.scldpc_full_bp_device_cn16.argtypes
    L.scldpc_full_bp_traj_device_deg.argtypes = L.scldpc_full_bp_traj_device_cn16.argtypes
    L.scldpc_full_bp_traj_device_deg_wide.argtypes = L.scldpc_full_bp_traj_device_cn16.argtypes
    L.scldpc_full_bp_caps_device_wide.argtypes = L.scldpc_full_bp_caps_device_cn16.argtypes
    L.scldpc_full_bp_caps_device_deg.argtypes = L.scldpc_full_bp_caps_device_cn16.argtypes
    L.scldpc_full_bp_caps_device_deg_wide.argtypes = L.scldpc_full_bp_caps_device_cn16.argtypes
    L.scldpc_full_bp_device.argtypes = [pp, i32, vp, vp, i32, i32, vp, vp, i32, vp, vp, u64, vp]
    L.scldpc_sw_bp_device.argtypes = [pp, i32, vp, vp, i32, i32, i32, vp, vp, vp, u64, vp]
    L.scldpc_sample_philox_device_adj16.argtypes = L.scldpc_sample_philox_device.argtypes
    L.scldpc_full_bp_device_adj16.argtypes = L.scldpc_full_bp_device.argtypes
    L.scldpc_sw_bp_device_adj16.argtypes = L.scldpc_sw_bp_device.argtypes
    L.scldpc_peel_sweep_device.argtypes = [pp, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, u64, vp]
    L.scldpc_peel_sweep_device_adj16.argtypes = L.scldpc_peel_sweep_device.argtypes
    L.scldpc_peel_sweep_sock16_supported.argtypes = [pp]
    L.scldpc_peel_sweep_device_sock16.argtypes = [pp, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]
    L.scldpc_peel_sweep_wide_supported.argtypes = [pp]
    L.scldpc_peel_sweep_device_sock16_wide.argtypes = L.scldpc_peel_sweep_device_sock16.argtypes
    L.scldpc_sample_philox_ensemble_adj16_sock_supported.argtypes = [pp, i32]
    L.scldpc_sample_philox_ensemble_device_adj16_sock.argtypes = [pp, i32, u64, u64, i32, dbl, i32, vp, vp, vp, vp, vp]
    L.scldpc_peel_sweep_tb_supported.argtypes = [pp]
    L.scldpc_peel_sweep_tb_wide_supported.argtypes = [pp]
    L.scldpc_peel_sweep_device_sock16_tb.argtypes = L.scldpc_peel_sweep_device_sock16.argtypes
    L.scldpc_peel_sweep_device_sock16_tb_wide.argtypes = L.scldpc_peel_sweep_device_sock16.argtypes
    L.scldpc_sample_philox_uncoupled_supported.argtypes = [pp]
    L.scldpc_sample_philox_uncoupled_device.argtypes = [pp, u64, u64, i32, dbl, i32, vp, vp, vp, vp]
    L.scldpc_sample_philox_uncoupled_wide_supported.argtypes = [pp]
    L.scldpc_sample_philox_uncoupled_wide_device.argtypes = L.scldpc_sample_philox_uncoupled_device.argtypes
    L.scldpc_peel_pick_device.argtypes = [pp, i32, vp, vp, i32, i32, vp, u64, u64, vp, vp, vp, vp, u64, vp]
    L.scldpc_peel_pick_device_adj16.argtypes = L.scldpc_peel_pick_device.argtypes
    L.scldpc_peel_pick_deg_supported.argtypes = [pp, i32]
    L.scldpc_peel_pick_deg_workspace_bytes.argtypes = [pp, i32, i32]
    L.scldpc_peel_pick_deg_workspace_bytes.restype = i64
    L.scldpc_peel_pick_device_adj16_deg.argtypes = [pp, i32, vp, vp, i32, i32, u64, u64, vp, vp, vp, u64, vp]
    L.scldpc_r1_moments_device.argtypes = [i32, i32, vp, vp, vp]
    L.scldpc_r1_gram_workspace_bytes.argtypes = [i32, i32]
    L.scldpc_r1_gram_workspace_bytes.restype = i64
    L.scldpc_r1_gram_trial_splits.argtypes = [i32, i32]
    L.scldpc_r1_gram_trial_splits.restype = i32
    L.scldpc_r1_gram_device.argtypes = [i32, i32, vp, i32, vp, vp, vp, i64, vp]
    L.scldpc_ss_spectrum_form.argtypes = [pp]
    L.scldpc_ss_spectrum_workspace_bytes.argtypes = [pp, i32]
    L.scldpc_ss_spectrum_workspace_bytes.restype = i64
    L.scldpc_ss_spectrum_device.argtypes = [pp, i32, vp, i32, vp, i32, vp, vp, vp, vp, i64, vp]
    L.scldpc_chain_runs_device.argtypes = [pp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.scldpc_stream_runs_device.argtypes = [pp, i32, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    L.scldpc_channel_levels_device.argtypes = [pp, u64, u64, i32, i32, vp, i32, vp, vp, vp]
    L.scldpc_peel_sweep_eps_device.argtypes = [pp, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, u64, vp]
    L.scldpc_peel_sweep_eps_device_adj16.argtypes = L.scldpc_peel_sweep_eps_device.argtypes
    L.scldpc_peel_sweep_eps_workspace_query.argtypes = [pp, i32, i32]
    L.scldpc_peel_sweep_eps_workspace_query.restype = i64
    L.scldpc_full_bp_eps_device.argtypes = [pp, i32, vp, vp, i32, i32, vp, vp, vp, u64, vp]
    L.scldpc_full_bp_eps_device_adj16.argtypes = L.scldpc_full_bp_eps_device.argtypes
    L.scldpc_full_bp_eps_workspace_query.argtypes = [pp, i32, i32]
    L.scldpc_full_bp_eps_workspace_query.restype = i64
    L.scldpc_channel_keys_device.argtypes = [pp, u64, u64, i32, i32, vp, vp, vp]
    L.scldpc_frame_threshold_device.argtypes = [pp, i32, vp, vp, u32, u32, i32, vp, vp, vp, u64, vp]
    L.scldpc_frame_threshold_device_adj16.argtypes = L.scldpc_frame_threshold_device.argtypes
    L.scldpc_frame_threshold_workspace_query.argtypes = [pp, i32, i32]
    L.scldpc_frame_threshold_workspace_query.restype = i64
    L.scldpc_vn_threshold_device.argtypes = [pp, i32, vp, vp, u32, u32, i32, i32, vp, vp, vp, vp, vp, vp, u64, vp]
    L.scldpc_vn_threshold_device_adj16.argtypes = L.scldpc_vn_threshold_device.argtypes
    L.scldpc_vn_threshold_workspace_query.argtypes = [pp, i32, i32]
    L.scldpc_vn_threshold_workspace_query.restype = i64
    L.scldpc_swc_bp_device.argtypes = [pp, i32, vp, vp, i32, i32, vp, vp, vp, u64, vp]
    L.scldpc_swc_bp_device_adj16.argtypes = L.scldpc_swc_bp_device.argtypes
    L.scldpc_stream_supported.argtypes = [pp, i32]
    L.scldpc_stream_state_bytes.argtypes = [pp, i32]
    L.scldpc_stream_state_bytes.restype = i64
    L.scldpc_stream_run_device.argtypes = [pp, i32, u64, u64, dbl, i32, i32, vp, i32, vp, vp, vp, vp]
    L.scldpc_stream_glibc_inputs_host.argtypes = [pp, u32, dbl, i32, vp, i32, vp, vp]
    L.scldpc_stream_run_device_inputs.argtypes = [pp, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, i32, i64, vp]
    L.scldpc_stream_glibc_next_host.argtypes = [pp, vp, dbl, i32, vp, i32, i64, i32, vp, vp]
    L.scldpc_stream_run_device_inputs_at.argtypes = [pp, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, i64, i32, i64, vp]
    L.scldpc_sw_bp_ring_supported.argtypes = [pp, i32]
    L.scldpc_cn_sockets_device.argtypes = [pp, i32, vp, vp, vp]
    L.scldpc_sw_bp_ring_device.argtypes = [pp, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    L.scldpc_sw_bp_ring_deg_supported.argtypes = L.scldpc_sw_bp_ring_supported.argtypes
    L.scldpc_sw_bp_ring_device_deg.argtypes = L.scldpc_sw_bp_ring_device.argtypes
    L.scldpc_swc_bp_ring_supported.argtypes = L.scldpc_sw_bp_ring_supported.argtypes
    L.scldpc_swc_bp_ring_device.argtypes = [pp, i32, vp, vp, vp, i32, i32, vp, vp, vp]
    L.scldpc_accumulate_run_device.argtypes = [i32, vp, i64, vp, vp]
    L.scldpc_accumulate_peel_device.argtypes = [i32, vp, i64, vp, vp]
    L.scldpc_clear_channel_range_device.argtypes = [pp, i32, i32, i32, vp, vp]
    L.scldpc_full_bp_lds_bytes.argtypes = [pp]
    L.scldpc_full_bp_lds_bytes.restype = i64
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise ScldpcError(f"libscldpc_hip error {rc}: {lib().scldpc_last_error().decode()}")


def doped_array(doped):
    arr = np.ascontiguousarray(doped, dtype=np.int32).reshape(-1)
    return arr, (arr.ctypes.data if arr.size else None)
