"""Host-side mirror of the reference's three BP executables (simulators_sc_ldpc/bp_decoding):

    bp_lim_iter INDEX W NUM_DOPED MAX_IT              (BPF main_terminated, BPF:2057-2161)
    sw_lim_iter INDEX W NUM_DOPED MAX_IT INIT_IT      (BPW:2099-2158)
    bp_traj     INDEX W NUM_DOPED MAX_IT IS_TERM      (BPT:2095-2178)

Same positional argv, same ε grid / stop rule / output files (names and row formats of `risultati`,
BPF:458-519, and of the trajectory dump, BPT:988,1051,1145), but the ensemble size and grid — compile
time #defines in the reference (BPF:22-67) — are options with the reference's values as defaults, the
frames of an ε point are decoded in device batches.  Under torch.distributed (one process per GPU) the work
is sharded the way the reference is run on a cluster — one process per subset of ε points (NB cell 35:21-25,
loop BPF:2111-2114): point `sim` belongs to rank `sim % world`, no collective on the data path, and after
every wave of `world` points one all-reduce of the 9 run counters per point lets rank 0 append the rows in
grid order.  With fewer points than ranks (or --shard frames) the frames of a point are split evenly over
the ranks instead; the only exchange is then an all-gather of the per-trial counter rows (32 B per trial),
so that the ordered stop rule `frame_err >= 1000` cuts at the same frame on every rank.

`bp_traj` is a one-point program that the reference runs as an array of processes, one per INDEX (BPT:2095, file name
BPT:2131-2134; NB cell 35:21): under torch.distributed rank r IS process INDEX + r — it decodes that replica's frames
alone and writes that replica's file, so an N-rank job leaves the N files that N single runs leave.

Two sampling modes:
  * rng="philox" (default): codes and channels drawn on the device, counter-based, trial t of point s of
    replica INDEX keyed by (seed, INDEX·2^52 + s·2^40 + t) — any batch size / GPU count gives the same files, and the
    processes of an array job (same --seed, different INDEX) draw disjoint streams.
  * rng="glibc": the reference's own stream, srandom(seed) once and frames drawn back to back with
    perm_code carried over — reproduces a reference run bit for bit on an identical seed (the
    reference seeds from gettimeofday, BPF:2059-2062; pass --seed to pin it).  Sampling is then a
    sequential host loop (as in the reference); decoding still runs on the device.  Single rank only.

`bp_lim_iter … --caps 175,200,250` writes the files of several MAX_IT from one run: one file per cap, each the file that
`bp_lim_iter` with that MAX_IT writes.  Where that is exact and the level-synchronous decoder takes the ensemble (Philox
sampling, NUM_DOPED = 0) the frames are sampled and decoded once, with a checkpoint at every cap
(engine.full_bp_caps_cn16); otherwise the caps run one after another.  `--caps-fused on` extends the one decode to trials of
more than 65536 CNs (engine.full_bp_caps_wide) and to the pairs (3,6) and (5,10) (engine.full_bp_caps_deg).

`bp_lim_iter INDEX W NUM_DOPED MAX_IT --window classical` decodes with the classical sliding window kept in the full-BP source
(decodeBP_SW, BPF:627-897; the reference runs it with the commented call at BPF:2137-2138 swapped in): W positions per window,
MAX_IT iterations per window, the file name and rows of `bp_lim_iter`.  `--ring on|off|auto` picks the ring window decoder or
the whole-chain kernel; both write the same file.

`--sampled-table on|off|auto` (bp_lim_iter, bp_traj, sw_lim_iter): where the first-generation sampler is followed by a pass that
builds the decoder's CN -> socket table, the sampler writes that table in its own launch (engine.sample_philox_sock); same files.

`--sampler2 on|off|auto` (bp_lim_iter, bp_traj, sw_lim_iter): with --dv/--dc 3/6 or 5/10 and at most 8192 sockets per position,
the second-generation sampler of these pairs (engine.sample_philox_deg_sock16) draws the code and writes the CN -> socket table in
one launch, instead of the first-generation sampler and its table pass; same files.

`--sampler2-wide on|off|auto` (bp_lim_iter, bp_traj, sw_lim_iter): with --dv/--dc 3/6, 4/8 or 5/10 and more than 8192 but at most
20480 sockets per position (bp_traj's default N = 5000), the wide second-generation sampler (engine.sample_philox_wide_sock16)
draws the code and writes the CN -> socket table in one launch, instead of the first-generation sampler and its table pass; same
files.

`--runs` (bp_lim_iter, also with --window classical; sw_lim_iter; sw): the error-propagation statistics of the frames each ε point
consumed — where the failed positions sit and how long their runs are (engine.chain_runs over the decoder's erased bits), for `sw`
runs, events, gaps, time to first failure and the error rate by offset in the doping period (engine.StreamRuns over the trace) —
pickled by rank 0 as one dict per ε point beside the result file (`<file>.runs.pkl`), which itself is written as without the switch.

`bp_lim_iter INDEX W NUM_DOPED MAX_IT --schedule fixpoint --eps-fused on` (MAX_IT >= 10^6) decodes every ε point of the grid from
ONE sampled code per frame: one sampler call, engine.channel_levels and one engine.full_bp_eps per batch instead of a sampler and a
decode per point (run_grid_fused).  This is the one switch that does NOT write the same file: the unfused program keys frame f of
point sim as trial_key(INDEX, sim, f), so its points see different codes; the fused run keys every point's frame f as
trial_key(INDEX, 0, f).  Row 0 is byte for byte the unfused row 0, and row k is byte for byte what the unfused program's point 0
gives at ε_k — another sample of the same distribution than the unfused row k, and positively correlated with the other rows
(common random numbers).  `off`, and `auto` while BP_EPS_FUSED_BY_DEFAULT is False, write the unfused file.  With --runs the
.runs.pkl has the same layout, over the frames each point consumed.

`bp_thresholds INDEX W NUM_DOPED FRAMES [doped…]` (no counterpart in the reference; W = 0) takes the nesting to its end: not a
grid but, for every frame trial_key(INDEX, 0, f), the one integer threshold T* at which unlimited full BP starts to fail
(run_thresholds: engine.channel_keys + engine.frame_threshold, a bisection on the device inside the residual of the decode at
--eps-hi).  The frame fails at ε iff T* <= erasure_threshold(ε), so the rows give FER(ε) at every ε of [--eps-lo, --eps-hi] from
the same frames, the moments of ε*, and the stopping set that kills each frame; rank 0 pickles them to
`<bp_lim_iter's result file at MAX_IT 1000000>.thresholds.pkl`.

`bp_curves INDEX W NUM_DOPED FRAMES [doped…] [--points K]` (no counterpart in the reference; W = 0) resolves those frames by
position: for every VN the one integer tau at which it starts to be lost (run_vn_thresholds: engine.channel_keys +
engine.vn_threshold, one walk down the keys of the residual of the decode at --eps-hi, no rebuild of the CN words), reduced on
the device to the threshold of every position and the lost VNs at K points.  BER at the K points, and the block error rate of
every position and FER at every ε of the window, come from the same frames; rank 0 pickles them to
`<bp_lim_iter's result file at MAX_IT 1000000>.curves.pkl` and prints the K rows in the column order of `risultati`.

All compute is in libscldpc_hip.so; this file is orchestration and file formats.
"""
import argparse
import collections
import copy
import functools
import os
import pickle
import sys
import time

import numpy as np
import torch

from . import engine as E
from .engine import CodeParams, NCOUNTERS, NRUN, RUN_NAMES  # noqa: F401

POINT_STRIDE = 1 << 40          # philox trial index = replica * REPLICA_STRIDE + point * POINT_STRIDE + frame
REPLICA_STRIDE = 1 << 52        # replica = the executable's INDEX argument (one process of the reference's array jobs)


def trial_key(index, sim, frame=0):
    """Philox trial index of frame `frame` of ε point `sim` in the run of replica `index`."""
    if not (0 <= index < 4096 and 0 <= sim < 4096 and 0 <= frame < POINT_STRIDE):
        raise ValueError("INDEX and the point number must lie in [0, 4096)")
    return index * REPLICA_STRIDE + sim * POINT_STRIDE + frame


class GridSpec:
    """ε grid and stop rule: Def_epsIni − sim·Def_epsDelta for sim < Def_NUM_POINTS (BPF:55-61,301);
    stop at frame_err >= min_frame_err or after max_frames frames (BPF:63-65, 440-451, 2117)."""

    def __init__(self, eps_ini, eps_delta, num_points, min_frame_err, max_frames):
        self.eps_ini, self.eps_delta, self.num_points = eps_ini, eps_delta, num_points
        self.min_frame_err, self.max_frames = min_frame_err, max_frames

    def eps(self, sim):
        return float(self.eps_ini) - sim * float(self.eps_delta)


# the shipped #defines of the three sources
DEFAULTS = {
    "bp_lim_iter": dict(N=1000, L=50, grid=GridSpec(0.48, 0.00125, 26, 1000, 1000)),
    "sw_lim_iter": dict(N=1000, L=50, grid=GridSpec(0.475, 0.00125, 18, 1000, 1000)),
    "bp_traj": dict(N=5000, L=50, grid=GridSpec(0.46, 0.005, 1, 500, 500)),
}


def runs_shapes(L):
    """Names and shapes of the error-propagation accumulators of one ε point (engine.chain_runs), in the order in which they
    are flattened for an all-reduce."""
    return (("pos", (L, 4)), ("run_hist", (L + 1, 2)), ("fail_hist", (L + 1,)))


def runs_unflatten(L, flat):
    out, at = {}, 0
    for name, shape in runs_shapes(L):
        k = int(np.prod(shape))
        out[name] = np.array(flat[at:at + k], dtype=np.int64).reshape(shape)
        at += k
    return out


def runs_flatten(L, runs):
    return np.concatenate([np.asarray(runs[name], dtype=np.int64).reshape(-1) for name, _ in runs_shapes(L)])


def _dist():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist, dist.get_rank(), dist.get_world_size()
    return None, 0, 1


class PointResult:
    """Counters of one ε point after the stop rule, as `risultati` needs them (BPF:499-515)."""

    def __init__(self, eps, n, L, run, bad=False, runs=None):
        self.eps, self.n, self.L = eps, n, L
        self.runs = runs                # Simulator(runs=True): {"pos", "run_hist", "fail_hist"} of the point's frames, numpy
        self.run = {k: int(v) for k, v in zip(RUN_NAMES, run)}
        self.f = self.run["frames"]
        self.bad = bool(bad)            # a frame broke decodeBP's invariant (BPF:1035-1039): the reference aborts there

    def row(self):
        r, f, n, L = self.run, self.f, self.n, self.L
        vals = (self.eps, r["users_err"] / n / f, r["frame_err"] / f, r["block_err"] / L / f,
                r["users_err_exp"] / n / f, r["frame_err_exp"] / f, r["block_err_exp"] / L / f)
        ints = (n, L, f, r["users_err"], r["frame_err"], r["block_err"], r["users_err_exp"],
                r["frame_err_exp"], r["block_err_exp"])
        return "%f %e %e %e %e %e %e " % vals + " ".join("%d" % v for v in ints) + "\n"


RISULTATI_HEADER = ("p BER FER BLER BER_EXP FER_EXP BLER_EXP n L f users_err frame_err block_err "
                    "users_err_exp frame_err_exp block_err_exp\n")


def result_filename(prog, p, W, max_it, init_it, index):
    """BPF:487 / BPW:488.  (The reference prints Def_M = CNs per position as `M`.)"""
    if prog == "sw_lim_iter":
        return "SC_LDPC_%d_%d_L%d_M%d_BP_SW%d_%dit_%dinit_Random_BLER_%d.dat" % (
            p.dv, p.dc, p.L, p.cns_pos, W, max_it, init_it, index)
    return "SC_LDPC_%d_%d_L%d_M%d_BP_SW%d_%dit_Random_BLER_%d.dat" % (p.dv, p.dc, p.L, p.cns_pos, W, max_it, index)


def traj_filename(p, eps, max_it, is_term, index):
    """BPT:2131-2134."""
    kind = "terminated" if is_term else "truncated"
    return "trajectories_%.4f_%s_SC_LDPC_%d_%d_L%d_M%d_BP_Full_%dit_Random_BLER_%d.dat" % (
        eps, kind, p.dv, p.dc, p.L, p.cns_pos, max_it, index)


def write_risultati(path, sim, point):
    """First point truncates and writes the header, later points append (BPF:489-497)."""
    with open(path, "w" if sim == 0 else "a") as f:
        if sim == 0:
            f.write(RISULTATI_HEADER)
        f.write(point.row())


# Whether Simulator(wide=None) takes the wide 4-bit level decoder where it applies: decided by the end-to-end A/B of
# tools/traj_wide_speedup.py against the first-generation path — 1.62x and 1.78x at N = 5000, spread below 0.3 %
# (profiles/traj_wide_speedup.json)
WIDE_BY_DEFAULT = True

# Whether Simulator(deg=None) takes the 4-bit level decoder for the pairs (3,6) and (5,10) where it applies: True only if every
# repetition of the new path beats every repetition of the first-generation path end to end on every shape of
# tools/deg_speedup.py (profiles/deg_speedup.json)
DEG_BY_DEFAULT = False

# Whether Simulator(ring=None) takes the ring window decoder for the pairs (3,6) and (5,10) where it applies: True only if every
# repetition of the new path beats every repetition of the whole-chain kernel end to end on every shape of
# tools/ring_deg_speedup.py, with identical counters (profiles/ring_deg_speedup.json)
RING_DEG_BY_DEFAULT = False

# Whether Simulator(decoder="swc", ring=None) takes the classical ring window decoder where it applies, under the same rule:
# every repetition of the ring path beats every repetition of the whole-chain kernel end to end on every shape of
# tools/classical_ring_speedup.py, with identical counters (profiles/classical_ring_speedup.json)
CLASSICAL_RING_BY_DEFAULT = False

# Whether Simulator(fused_caps=None) and `bp_lim_iter --caps` take the cap checkpoints of the wide form and of the pairs (3,6) and
# (5,10) where they apply, instead of one single-cap pass per cap (tools/caps_forms_speedup.py, profiles/caps_forms_speedup.json).
# The (4,8) forms of at most 65536 CNs fuse without this switch.
CAPS_FORMS_BY_DEFAULT = False

# Whether Simulator(sampled_table=None) lets the first-generation sampler write the CN -> socket table with the code
# (engine.sample_philox_sock) wherever a path would run the cn_sockets pass after it, or leaves the table to engine.sw_bp
# (tools/sampled_table_speedup.py, profiles/sampled_table_speedup.json).  Same tables as a set per CN, same files.
SAMPLED_TABLE_BY_DEFAULT = False

# Whether Simulator(sampler2=None) takes the second-generation sampler of the pairs (3,6) and (5,10) (engine.sample_philox_deg_sock16)
# where it applies, instead of the first-generation sampler and the cn_sockets pass: True only if every repetition of the new path
# beats every repetition of both old forms end to end on every shape of tools/sampler_deg_speedup.py, with equal outputs
# (profiles/sampler_deg_speedup.json).  Same rows, channel and files; the same table as a set per CN.
# Measured: the condition holds on all three shapes (1.24-1.32x end to end).  Kept False here because --deg, --ring, --caps-fused
# and --sampled-table are specified, and tested, as starting from the first-generation sampler: the flip is a change of its own.
SAMPLER2_DEG_BY_DEFAULT = False

# Whether Simulator(sampler2_wide=None) takes the wide second-generation sampler (engine.sample_philox_wide_sock16: the pairs (3,6),
# (4,8) and (5,10) with more than 8192 and at most 20480 sockets per position) where it applies, instead of the first-generation
# sampler and the cn_sockets pass: SAMPLER2_DEG_BY_DEFAULT's rule on the shapes of tools/sampler_wide_speedup.py
# (profiles/sampler_wide_speedup.json).  Same rows, channel and files; the same table as a set per CN.  Kept False
# here whatever is measured: the selection tests specify the default path, and the flip is a change of its own.
SAMPLER2_WIDE_BY_DEFAULT = False


# The path of a Simulator, decided once in select_path:
#   adj_dtype    VN -> CN table: torch.int16 (position-local ids) or torch.int32 (the reference's VNdegree)
#   sampler      what fills a batch: "glibc" (host replay), "first" (first-generation sampler), "first_sock" (the same with the
#                CN -> socket table from its own launch), "cn16" / "sock16" (second generation, with the CN -> VN / CN -> socket
#                table), "deg_sock16" (second generation of the pairs (3,6) and (5,10), with the CN -> socket table), "wide_sock16"
#                (second generation beyond 8192 sockets per position, with the CN -> socket table)
#   cn_table     the CN table kept next to the VN -> CN one: None, "vn" or "sock"
#   cn_pass      that table comes from the cn_sockets pass (the sampler does not emit it)
#   decoder      "sw_ring" / "sw_chain" (E.sw_bp; "sw_ring" of the pairs (3,6) and (5,10): the _deg entry points),
#                "swc_ring" / "swc_chain" (E.sw_bp(classical=True): the classical window of decoder="swc"), or the full-BP call
#                that walks the iterations: "level16", "wide", "full_bp",
#                "deg16" / "degwide" (the 4-bit level decoder of the pairs (3,6) and (5,10), 16- / 32-bit queue entries)
#   fix_decoder  the fixpoint kernel an unlimited fixpoint run takes for calls without rows: "fixpoint16", "fixpoint_deg",
#                "fixpoint" or None
Path = collections.namedtuple("Path", "adj_dtype sampler cn_table cn_pass decoder fix_decoder")


def _cn16_table(p):
    """The CN table from which the 16-bit forms of the 4-bit decoder take this ensemble with device sampling: "vn", "sock"
    (n >= 65535) or None (they do not)."""
    return "vn" if E.cn16_supported(p) else "sock" if E.full_bp_sock16_supported(p) else None


# What select_path decides from.  Config: the ensemble's numbers, the run's arguments (caps: whether caps are given) and the
# seven switches as booleans, None resolved against the *_BY_DEFAULT (ring: the one of the decoder's ring); wide_off / deg_off:
# the switch was given as False, which vetoes its family's caps form where None does not.  Capabilities: what the library's
# *_supported rules answer for this ensemble and window (cn16_table: _cn16_table).
Config = collections.namedtuple(
    "Config", "dv dc L vns_pos cns_pos W decoder rng schedule max_it rows_cap caps num_doped "
              "wide deg ring fused_caps sampled_table sampler2 sampler2_wide wide_off deg_off")
Capabilities = collections.namedtuple(
    "Capabilities", "cn16_table full_bp_wide full_bp_deg full_bp_deg_wide sw_ring sw_ring_deg swc_ring "
                    "sock16 deg_sock16 wide_sock16 first_sock")
# select_path's answer: the path, why each sampler switch left it alone (None: it did not), the ValueError of caps or None
Selection = collections.namedtuple("Selection", "path sampler2_deg_reason sampler2_wide_reason sampled_table_reason caps_error")
CAPS_ERROR = ("caps: the fused decode takes Philox sampling, no doping and an ensemble of the level-synchronous 4-bit decoder "
              "(caps_sequential_reason)")


def _config(p, W=0, decoder="full", rng="philox", schedule="flooding", max_it=0, rows_cap=0, caps=False, num_doped=0,
            wide=None, deg=None, ring=None, fused_caps=None, sampled_table=None, sampler2=None, sampler2_wide=None):
    """The Config of a Simulator's arguments; the *_BY_DEFAULT are read here, at call time."""
    def on(want, default):
        return default if want is None else bool(want)
    return Config(p.dv, p.dc, p.L, p.vns_pos, p.cns_pos, W, decoder, rng, schedule, max_it, rows_cap, bool(caps), num_doped,
                  on(wide, WIDE_BY_DEFAULT), on(deg, DEG_BY_DEFAULT),
                  on(ring, CLASSICAL_RING_BY_DEFAULT if decoder == "swc" else RING_DEG_BY_DEFAULT),
                  on(fused_caps, CAPS_FORMS_BY_DEFAULT), on(sampled_table, SAMPLED_TABLE_BY_DEFAULT),
                  on(sampler2, SAMPLER2_DEG_BY_DEFAULT), on(sampler2_wide, SAMPLER2_WIDE_BY_DEFAULT), wide is False, deg is False)


def _capabilities(p, W=0):
    """The Capabilities of ensemble p and window W: the one place that asks the library (host functions, no device)."""
    return Capabilities(_cn16_table(p), E.full_bp_wide_supported(p), E.full_bp_deg_supported(p),
                        E.full_bp_deg_supported(p, wide=True), E.sw_ring_supported(p, W), E.sw_ring_deg_supported(p, W),
                        E.swc_ring_supported(p, W), E.sock16_supported(p), E.deg_sock16_supported(p), E.wide_sock16_supported(p),
                        E.sample_philox_sock_supported(p))


# -- the rules: pure functions of a Config c and the Capabilities k, each the one statement of its limit and of its text --------
def _ring_rule(c, k):
    """ring_deg_reason (c.decoder "sw": the ring of the pairs (3,6) and (5,10)) and classical_ring_reason ("swc")."""
    classical = c.decoder == "swc"
    if not classical and (c.dv, c.dc) == (4, 8):
        return "dv = 4, dc = 8 has a ring path of its own, chosen without this switch"
    if not c.ring:
        return "switched off"
    if c.rng != "philox":
        return "--rng %s samples the 4-byte VN -> CN table on the host: the ring kernel reads the 2-byte tables" % c.rng
    if c.cns_pos > 65536:
        return "more than 65536 CNs per position: no 2-byte VN -> CN table"
    if not (k.swc_ring if classical else k.sw_ring_deg):
        return ("the %sring kernel takes the pairs (3,6), (4,8) and (5,10) with W >= 1, vns_pos * dv <= 65535, L + dv - 1 <= 65535 "
                "and a window state that fits the LDS (dv = %d, dc = %d, L = %d, N = %d, W = %d)"
                % ("classical " if classical else "", c.dv, c.dc, c.L, c.vns_pos, c.W))
    return None


def _caps_rule(c, k):
    """(form, None): the one decode whose checkpoints give every cap's file — "level16", or beyond the (4,8) forms of at most
    65536 CNs (the fused_caps switch) "wide" / "deg16" / "degwide" — or (None, why the caps run one after another).  A caps
    form takes exactly the shapes of its family's level form, so the library's *_supported rules decide."""
    if c.rng != "philox":
        return None, "--rng %s: each cap's run replays srandom(seed) from the start and stops drawing at its own frame" % c.rng
    if c.num_doped > 0:
        return None, "NUM_DOPED > 0: the first doped position is MAX_IT (BPF:2083-2091), so every cap is a different experiment"
    if c.schedule != "flooding":
        return None, "--schedule %s has no iteration caps" % c.schedule
    if k.cn16_table is not None:
        return "level16", None
    if not c.fused_caps:
        if k.full_bp_wide:
            return None, "more than 65536 CNs per trial: the wide form of the level-synchronous 4-bit decoder has no cap checkpoints"
        return None, "the level-synchronous 4-bit decoder takes dv = 4, dc = 8 and at most 65536 CNs per trial"
    if (c.dv, c.dc) == (4, 8):
        if c.wide_off:
            return None, "--wide off: more than 65536 CNs per trial take the wide form of the level-synchronous 4-bit decoder"
        if not k.full_bp_wide:
            return None, ("the wide form of the level-synchronous 4-bit decoder takes a state that leaves 1024 queue entries per "
                          "queue in one CU's LDS, and vns_pos * dv <= 65535 (L = %d, N = %d)" % (c.L, c.vns_pos))
        return "wide", None
    if (c.dv, c.dc) not in ((3, 6), (5, 10)):
        return None, "the level-synchronous 4-bit decoder takes the pairs (3,6), (4,8) and (5,10) (dv = %d, dc = %d)" % (c.dv, c.dc)
    if c.deg_off:
        return None, "--deg off: dv = %d, dc = %d takes the _deg forms of the level-synchronous 4-bit decoder" % (c.dv, c.dc)
    if c.cns_pos > 65536:
        return None, "more than 65536 CNs per position: no 2-byte VN -> CN table"
    if k.full_bp_deg:
        return "deg16", None
    if k.full_bp_deg_wide:
        return "degwide", None
    return None, ("the _deg forms of the level-synchronous 4-bit decoder take at most 65536 CNs per trial, or a state that leaves "
                  "1024 queue entries per queue in one CU's LDS, and vns_pos * dv <= 65535 (dv = %d, dc = %d, L = %d, N = %d)"
                  % (c.dv, c.dc, c.L, c.vns_pos))


def _sampler2_deg_rule(c, k, path):
    """sampler2_deg_reason on the records."""
    if not c.sampler2:
        return "switched off"
    if c.rng != "philox":
        return "--rng %s samples the code on the host" % c.rng
    if (c.dv, c.dc) == (4, 8):
        return "dv = 4, dc = 8 has a second-generation sampler of its own, chosen without this switch"
    if (c.dv, c.dc) not in ((3, 6), (5, 10)):
        return "the second-generation sampler takes the pairs (3,6), (4,8) and (5,10) (dv = %d, dc = %d)" % (c.dv, c.dc)
    # what runs the cn_sockets pass after the first-generation sampler, or a ring decoder on a table of sockets
    if not (path.sampler == "first" and path.adj_dtype == torch.int16
            and (path.cn_pass or (path.decoder in ("sw_ring", "swc_ring") and path.cn_table == "sock"))):
        return "the decoder of this configuration (%s) reads no CN -> socket table" % path.decoder
    if not k.deg_sock16:
        return ("the second-generation sampler of the pairs (3,6) and (5,10) takes at most 8192 sockets per position "
                "(dv = %d, dc = %d, N = %d: %d sockets)" % (c.dv, c.dc, c.vns_pos, c.cns_pos * c.dc))
    return None


def _sampler2_wide_rule(c, k, path):
    """sampler2_wide_reason on the records."""
    if not c.sampler2_wide:
        return "switched off"
    if c.rng != "philox":
        return "--rng %s samples the code on the host" % c.rng
    if path.sampler in ("cn16", "sock16", "deg_sock16"):
        return ("the second-generation sampler of at most 8192 sockets per position takes this ensemble and writes the CN table "
                "with the code already")
    if not k.wide_sock16:
        return ("the wide second-generation sampler takes the pairs (3,6), (4,8) and (5,10) with more than 8192 and at most 20480 "
                "sockets per position (dv = %d, dc = %d, N = %d: %d sockets)" % (c.dv, c.dc, c.vns_pos, c.cns_pos * c.dc))
    # what runs the cn_sockets pass after the first-generation sampler, a ring decoder on a table of sockets, and the (4,8) ring
    # whose table E.sw_bp builds per call
    if not (path.sampler == "first" and path.adj_dtype == torch.int16
            and (path.cn_pass or (path.decoder in ("sw_ring", "swc_ring") and path.cn_table == "sock")
                 or (path.decoder == "sw_ring" and path.cn_table is None))):
        return "the decoder of this configuration (%s) reads no CN -> socket table" % path.decoder
    return None


def _sampled_table_rule(c, k, path):
    """sampled_table_reason on the records."""
    if not c.sampled_table:
        return "switched off"
    if c.rng != "philox":
        return "--rng %s samples the code on the host" % c.rng
    if path.sampler in ("cn16", "sock16", "deg_sock16", "wide_sock16"):
        return "the second-generation sampler takes this ensemble and writes the CN table with the code already"
    # what runs the cn_sockets pass after the first-generation sampler, and the (4,8) ring whose table E.sw_bp builds per call
    if not (path.sampler == "first" and path.adj_dtype == torch.int16
            and (path.cn_pass or (path.decoder == "sw_ring" and path.cn_table is None))):
        return "the decoder of this configuration (%s) reads no CN -> socket table" % path.decoder
    if not k.first_sock:
        return ("the first-generation sampler writes the table for vns_pos * dv <= 65535, cns_pos <= 65536 and, beyond 8192 "
                "sockets per position, dc <= 255 and cns_pos <= 32768 (dv = %d, dc = %d, L = %d, N = %d)"
                % (c.dv, c.dc, c.L, c.vns_pos))
    return None


def select_path(c, k):
    """The path of configuration c where the library answers k: a Selection.  A function of its two arguments — it asks no
    library rule, reads no *_BY_DEFAULT and touches no device.  One rule per decoder family, asked in order, the first that
    takes the configuration decides; then the three sampler switches, each judged on the path the one before it left."""
    philox = c.rng == "philox"
    first = "first" if philox else "glibc"
    # compact 2-byte position-local ids for device-sampled codes; the reference's int32 VNdegree for host replays
    adj = torch.int16 if (philox and c.cns_pos <= 65536) else torch.int32
    full16 = c.decoder == "full" and adj == torch.int16
    # the one place that knows an unlimited fixpoint run: no iteration cap to honour, no iteration statistics.  Without rows it
    # takes a fixpoint kernel (decided per call in decode_batch: a call that wants rows walks the iterations); no_walk: no call
    # of this run wants rows
    unlimited_fix = c.schedule == "fixpoint" and (c.max_it <= 0 or c.max_it >= 1000000)
    no_walk = unlimited_fix and c.rows_cap == 0

    def on_sockets(decoder, fix=None, sampled=False):
        # a decoder that reads the CN -> socket table: sampled with the code where the (4,8) second-generation sampler takes the
        # ensemble (sampled=True), else the first-generation sampler writes the 2-byte VN -> CN table for every dv and the
        # cn_sockets pass the table of sockets
        if sampled and k.sock16:
            return Path(adj, "sock16", "sock", False, decoder, fix)
        return Path(adj, first, "sock", True, decoder, fix)

    def no_table(decoder, fix=None):
        return Path(adj, first, None, False, decoder, fix)

    def sw():
        # square windows: the ring kernel keeps the window's state in LDS and reads a CN -> socket table — sampled with the
        # code, else built by E.sw_bp per call ((4,8)) or by the cn_sockets pass (the _deg entry points of the other pairs)
        if c.decoder != "sw":
            return None
        ring = adj == torch.int16 and k.sw_ring
        if ring and k.sock16:
            return Path(adj, "sock16", "sock", False, "sw_ring", None)
        if _ring_rule(c, k) is None:
            return on_sockets("sw_ring")
        return no_table("sw_ring" if ring else "sw_chain")

    def swc():
        # classical windows: the ring kernel of all three pairs; everything else keeps the whole-chain kernel
        if c.decoder != "swc":
            return None
        return on_sockets("swc_ring", sampled=True) if _ring_rule(c, k) is None else no_table("swc_chain")

    def level16():
        # full BP on the BASELINE ensemble family: the second-generation pair (sampler_v2 + the 4-bits-per-CN decoder) on the
        # CN -> VN table (n >= 65535: the CN -> socket table).  Unlimited, no iteration statistics: its fixpoint form; else the
        # same decoder walked one flooding iteration per round — iteration caps, counts and rows
        table = k.cn16_table if (philox and c.decoder == "full") else None
        if table is None:
            return None
        sampler = "cn16" if table == "vn" else "sock16"
        if no_walk:                                     # (a call that wants rows all the same gets full_bp's iterations)
            return Path(adj, sampler, table, False, "full_bp", "fixpoint16")
        return Path(adj, sampler, table, False, "level16", None)

    def caps_forms():
        # cap checkpoints beyond level16 (opt-in): the path a single-cap run of the family takes
        form = _caps_rule(c, k)[0] if (c.caps and full16 and c.rows_cap == 0) else None
        return on_sockets(form, sampled=form == "wide") if form is not None else None

    def deg_forms():
        # the 4-bit decoder of the pairs (3,6) and (5,10); doped positions come with the channel.  Unlimited, no rows: the narrow
        # fixpoint form — there is no wide fixpoint kernel, so such a run of a wide shape keeps the first-generation path
        if not (c.deg and (c.dv, c.dc) != (4, 8) and full16 and not c.caps):
            return None
        form = "deg16" if k.full_bp_deg else "degwide" if (k.full_bp_deg_wide and not no_walk) else None
        fix = ("fixpoint_deg" if form == "deg16" else "fixpoint") if unlimited_fix else None
        return on_sockets(form, fix) if form is not None else None

    def wide():
        # more than 65536 CNs per trial (bp_traj's default N = 5000; L = 100, N = 2000): the wide form of the level decoder.  An
        # unlimited fixpoint run keeps full_bp_fixpoint (there is no wide fixpoint kernel)
        if not (c.wide and full16 and not no_walk and not c.caps and k.full_bp_wide):
            return None
        return on_sockets("wide", "fixpoint" if unlimited_fix else None, sampled=True)

    def first_generation():
        return no_table("full_bp", "fixpoint" if unlimited_fix else None)

    path = sw() or swc() or level16() or caps_forms() or deg_forms() or wide() or first_generation()
    # code and CN -> socket table from one launch instead of the first-generation sampler and the cn_sockets pass (opt-in): the
    # second-generation sampler of the pairs (3,6) and (5,10); behind it the wide one, whose shapes the first does not take;
    # last the first-generation sampler's own table, which then finds no first-generation sampler where either took the path
    reasons = []
    for rule, sampler in ((_sampler2_deg_rule, "deg_sock16"), (_sampler2_wide_rule, "wide_sock16"),
                          (_sampled_table_rule, "first_sock")):
        reasons.append(rule(c, k, path))
        if reasons[-1] is None:
            path = path._replace(sampler=sampler, cn_table="sock", cn_pass=False)
    # caps need a decode with checkpoints (the wide and _deg forms are reached with caps through caps_forms only)
    fused = path.decoder in ("level16", "wide", "deg16", "degwide") and c.rows_cap == 0 and c.num_doped == 0
    return Selection(path, *reasons, CAPS_ERROR if (c.caps and not fused) else None)


class Simulator:
    """Batched Monte-Carlo driver around the device decoders."""

    def __init__(self, p, decoder="full", W=0, max_it=0, init_it=0, is_term=True, doped=(), batch=2048,
                 rng="philox", seed=1, device=None, rows_cap=0, schedule="flooding", shard_frames=True, index=0,
                 verbose=False, caps=None, wide=None, deg=None, ring=None, fused_caps=None, sampled_table=None,
                 sampler2=None, sampler2_wide=None, runs=False):
        # runs: every point also returns the error-propagation statistics of its frames (engine.chain_runs over the decoder's
        # erased bits): PointResult.runs.  The cap checkpoints keep no erased bits
        self.runs = bool(runs)
        if self.runs and caps is not None:
            raise ValueError("runs=True: the cap checkpoints of one decode (caps) keep no erased bits; run one cap at a time")
        # wide: the 1024-thread 4-bit level decoder for trials of more than 65536 CNs (full_bp_small wide).  None = where
        # WIDE_BY_DEFAULT says, True = wherever it applies, False = never (the first-generation path, for A/B and tests)
        self.want_wide = wide
        # deg: the 4-bit level decoder for dv, dc other than (4,8) (full_bp_small's (3,6) and (5,10) instances).  None = where
        # DEG_BY_DEFAULT says, True = wherever it applies, False = never (the first-generation path)
        self.want_deg = deg
        # ring: the ring window decoder (sw_ring) for dv, dc other than (4,8), decoder="sw" only.  None = where RING_DEG_BY_DEFAULT
        # says, True = wherever it applies, False = never (the whole-chain kernel).  decoder="swc" (the classical window, W and
        # max_it per window): the classical ring decoder of all three pairs, None = where CLASSICAL_RING_BY_DEFAULT says
        self.want_ring = ring
        # fused_caps: with caps, the cap checkpoints of the wide form and of the pairs (3,6) and (5,10).  None = where
        # CAPS_FORMS_BY_DEFAULT says, True = wherever an instance applies (wide=False / deg=False veto their family), False = never
        self.want_fused_caps = fused_caps
        # sampled_table: the CN -> socket table from the first-generation sampler's own launch instead of the cn_sockets pass.
        # None = where SAMPLED_TABLE_BY_DEFAULT says, True = wherever it applies, False = never
        self.want_sampled_table = sampled_table
        # sampler2: the second-generation sampler of the pairs (3,6) and (5,10) instead of the first-generation sampler and the
        # cn_sockets pass.  None = where SAMPLER2_DEG_BY_DEFAULT says, True = wherever it applies, False = never
        self.want_sampler2 = sampler2
        # sampler2_wide: the wide second-generation sampler (more than 8192 sockets per position) instead of the first-generation
        # sampler and the cn_sockets pass.  None = where SAMPLER2_WIDE_BY_DEFAULT says, True = wherever it applies, False = never
        self.want_sampler2_wide = sampler2_wide
        self.p, self.decoder, self.W, self.max_it, self.init_it = p, decoder, W, max_it, init_it
        # caps: several MaxNumIt from one decode (run_point_caps; the level-synchronous 4-bit decoder only)
        self.caps = E.check_caps(caps) if caps is not None else None
        if self.caps is not None:
            self.max_it = self.caps[-1]
        self.index = index              # replica (the executables' INDEX): part of the Philox key
        self.schedule = schedule        # "fixpoint": unlimited full BP without the iteration count (1.2x faster)
        self.is_term, self.doped, self.batch, self.rng, self.seed = is_term, tuple(doped), batch, rng, seed
        self.rows_cap, self.verbose = rows_cap, verbose
        self.dist, self.rank, self.world = _dist()
        job_world = self.world
        if not shard_frames:                    # ε points / replicas are sharded by the caller: every point runs on one rank
            self.dist, self.rank, self.world = None, 0, 1
        self.device = torch.device(device) if device is not None else E.local_device()
        if rng == "glibc":
            # checked on the JOB's world size: with the points sharded every rank would otherwise replay the same
            # srandom(seed) stream from its start, where the reference carries random() and perm_code from point to point
            if job_world != 1:
                raise ValueError("rng='glibc' replays one sequential reference stream: single rank only")
            self.glibc = E.GlibcRun(p, seed)
        elif rng != "philox":
            raise ValueError("rng must be 'philox' or 'glibc'")
        self._alloc()

    def _select(self):
        """Decides the path of this configuration, once (no device work): self.path, which _alloc, fill_batch, decode_batch,
        decode_batch_caps and kernel_choice read.  Returns the dtype of the VN -> CN table."""
        config = _config(self.p, self.W, self.decoder, self.rng, self.schedule, self.max_it, self.rows_cap, self.caps is not None,
                         len(self.doped), self.want_wide, self.want_deg, self.want_ring, self.want_fused_caps,
                         self.want_sampled_table, self.want_sampler2, self.want_sampler2_wide)
        self.path, self.sampler2_deg_reason, self.sampler2_wide_reason, self.sampled_table_reason, caps_error = \
            select_path(config, _capabilities(self.p, self.W))
        if caps_error is not None:
            raise ValueError(caps_error)
        return self.path.adj_dtype

    # the path as the flags it used to be kept in
    gen2 = property(lambda self: self.path.fix_decoder == "fixpoint16")
    lvl2 = property(lambda self: self.path.decoder == "level16")
    wide = property(lambda self: self.path.decoder == "wide")
    sock = property(lambda self: (self.gen2 or self.lvl2) and self.path.cn_table == "sock")
    ring2 = property(lambda self: self.path.decoder == "sw_ring" and self.path.cn_table == "sock")
    wide_sock = property(lambda self: self.wide and not self.path.cn_pass)
    deg = property(lambda self: self.path.decoder in ("deg16", "degwide"))
    # the _deg entry points of the ring window decoder: every ring of another pair than (4,8), whose own ring E.sw_ring_supported
    # keeps to itself (the cn_sockets pass that marks them in select_path is gone where a sampler switch took the table)
    ring_deg = property(lambda self: self.path.decoder == "sw_ring" and (self.p.dv, self.p.dc) != (4, 8))

    def _alloc(self):
        p, batch = self.p, self.batch
        adj_dtype = self._select()
        self.d_adj = torch.empty((batch, p.n, p.dv), dtype=adj_dtype, device=self.device)
        self.d_ch = torch.empty((batch, p.nw), dtype=torch.int32, device=self.device)
        self.d_cnt = torch.empty((batch, NCOUNTERS), dtype=torch.int32, device=self.device)
        self.d_cn = (torch.empty((batch, p.nk, p.dc), dtype=torch.int16, device=self.device)
                     if self.path.cn_table is not None else None)
        if self.caps is not None:
            self.d_cnt_caps = torch.empty(len(self.caps) * batch * NCOUNTERS, dtype=torch.int32, device=self.device)
        if self.verbose:
            print("[scldpc] kernels: " + self.kernel_choice(), file=sys.stderr, flush=True)

    def kernel_choice(self):
        """Which device kernels this configuration runs."""
        return self._sampler_label() + " + " + self._decoder_label()

    def _sampler_label(self):
        path, pair = self.path, "dv = %d, dc = %d" % (self.p.dv, self.p.dc)
        sampler = path.sampler
        if path.decoder in ("sw_ring", "sw_chain"):
            # decoder="sw" names the host replay and the (4,8) second-generation sampler as it always has (pinned)
            sampler = {"glibc": "first", "sock16": "sock16 under sw"}.get(sampler, sampler)
        label = {"glibc": "glibc replay on the host", "first": "sampler (first generation)",
                 "first_sock": "sampler (first generation, CN->socket table)", "cn16": "sampler_v3 (CN->VN table)",
                 "sock16": "sampler_v3 (CN->socket table)", "sock16 under sw": "sampler_v2 (CN->socket table)",
                 "deg_sock16": "sampler_v2 (%s, CN->socket table)" % pair,
                 "wide_sock16": "sampler_v2 wide (%s, CN->socket table)" % pair}[sampler]
        return label + (" + cn_sockets pass" if path.cn_pass else "")

    def _decoder_label(self):
        path, pair = self.path, "dv = %d, dc = %d" % (self.p.dv, self.p.dc)
        if path.decoder == "sw_ring" and path.cn_table is None:
            return "sw_ring + cn_sockets pass"                          # (the (4,8) ring whose table E.sw_bp builds; pinned)
        if path.decoder == "sw_ring":
            return "sw_ring (window state in LDS" + (", " + pair if self.ring_deg else "") + ")"
        if path.decoder == "sw_chain":
            return "sw_bp (whole chain)"
        if path.decoder == "swc_ring":
            return "sw_ring classical window (window state in LDS, %s)" % pair
        if path.decoder == "swc_chain":
            return "sw_bp classical window (whole chain)"
        rows = ", trajectory rows)" if self.rows_cap else ")"
        if path.decoder == "full_bp" and path.fix_decoder != "fixpoint16":
            return ("full_bp (16-bit CN words" + rows + ": the 4-bit decoders take dv = 4, dc = 8 with device sampling and at most "
                    "65536 CNs per trial, or (the wide form, unless switched off) a state that leaves 1024 queue entries in one "
                    "CU's LDS")
        # the 4-bit decoder: its fixpoint form (a run none of whose calls wants rows), its cap checkpoints, or one flooding
        # iteration per round; the _deg forms name their pair, the wide forms their queue entries
        counts = "4-bit CN counts" + (", " + pair if self.deg else "")
        wide, q32 = ("wide ", ", 32-bit queue entries") if path.decoder in ("wide", "degwide") else ("", "")
        if path.fix_decoder in ("fixpoint16", "fixpoint_deg") and not self.rows_cap:
            return "full_bp_small fixpoint (%s)" % counts
        if self.caps is not None:
            return "full_bp_small %slevel-synchronous with %d cap checkpoints per decode (%s%s)" % (wide, len(self.caps), counts, q32)
        return "full_bp_small %slevel-synchronous (%s%s%s" % (wide, counts, q32, rows)

    def _accumulate(self, allcnt, run, stop_frame_err):
        return E.accumulate_run(allcnt, run, stop_frame_err)

    def _new_run(self):
        return E.new_run(self.device)

    # -- one device batch ------------------------------------------------------------------------
    def decode_batch(self, nb, want_rows=False):
        path, adj, ch, cnt = self.path, self.d_adj[:nb], self.d_ch[:nb], self.d_cnt[:nb]
        er = {"want_erased": True} if self.runs else {}                 # (without runs every call is what it was)
        if path.decoder in ("sw_ring", "sw_chain"):
            return E.sw_bp(self.p, adj, ch, self.W, self.max_it, self.init_it, counters=cnt,
                           d_cn_sock=self.d_cn[:nb] if path.cn_table is not None else None,
                           ring=True if self.ring_deg else None, deg=self.ring_deg, **er)
        if path.decoder in ("swc_ring", "swc_chain"):
            return E.sw_bp(self.p, adj, ch, self.W, self.max_it, counters=cnt, classical=True, ring=path.decoder == "swc_ring",
                           d_cn_sock=self.d_cn[:nb] if path.cn_table is not None else None, **er)
        # the fixpoint kernels report neither iteration counts nor rows: a call that wants rows walks the iterations
        decoder = path.fix_decoder if (path.fix_decoder is not None and not want_rows) else path.decoder
        sockets, rows_cap = path.cn_table == "sock", self.rows_cap if want_rows else 0
        if decoder == "fixpoint16":
            return E.full_bp_fixpoint_cn16(self.p, adj, self.d_cn[:nb], ch, is_term=self.is_term, counters=cnt, sockets=sockets,
                                           **er)
        if decoder == "level16":
            return E.full_bp_cn16(self.p, adj, self.d_cn[:nb], ch, max_it=self.max_it, is_term=self.is_term, counters=cnt,
                                  sockets=sockets, rows_cap=rows_cap, **er)
        if decoder == "fixpoint":
            return E.full_bp_fixpoint(self.p, adj, ch, is_term=self.is_term, counters=cnt, **er)    # no iteration counts
        if decoder == "fixpoint_deg":
            return E.full_bp_fixpoint_deg(self.p, adj, self.d_cn[:nb], ch, is_term=self.is_term, counters=cnt, **er)
        if decoder in ("deg16", "degwide"):
            return E.full_bp_deg(self.p, adj, self.d_cn[:nb], ch, max_it=self.max_it, is_term=self.is_term, rows_cap=rows_cap,
                                 counters=cnt, wide=decoder == "degwide", **er)
        if decoder == "wide":
            return E.full_bp_wide(self.p, adj, self.d_cn[:nb], ch, max_it=self.max_it, is_term=self.is_term,
                                  rows_cap=rows_cap, counters=cnt, **er)
        return E.full_bp(self.p, adj, ch, max_it=self.max_it, is_term=self.is_term, rows_cap=rows_cap, counters=cnt, **er)

    def decode_batch_caps(self, nb):
        """The counters [K, nb, 8] of every cap of self.caps for the batch in place (one decode)."""
        cnt = self.d_cnt_caps[:len(self.caps) * nb * NCOUNTERS].view(len(self.caps), nb, NCOUNTERS)
        decoder = self.path.decoder
        if decoder == "wide":
            return E.full_bp_caps_wide(self.p, self.d_adj[:nb], self.d_cn[:nb], self.d_ch[:nb], self.caps, is_term=self.is_term,
                                       counters=cnt)
        if decoder in ("deg16", "degwide"):
            return E.full_bp_caps_deg(self.p, self.d_adj[:nb], self.d_cn[:nb], self.d_ch[:nb], self.caps, is_term=self.is_term,
                                      counters=cnt, wide=decoder == "degwide")
        return E.full_bp_caps_cn16(self.p, self.d_adj[:nb], self.d_cn[:nb], self.d_ch[:nb], self.caps, is_term=self.is_term,
                                   counters=cnt, sockets=self.path.cn_table == "sock")

    def fill_batch(self, sim, eps, frame0, nb):
        path = self.path
        if path.sampler == "glibc":
            adj, ch = self.glibc.next_frames(nb, eps, self.doped)
            self.d_adj[:nb].copy_(torch.from_numpy(adj))
            self.d_ch[:nb].copy_(torch.from_numpy(ch.view(np.int32)))
        elif path.sampler == "first":
            E.sample_philox(self.p, self.seed, trial_key(self.index, sim, frame0), nb, eps, self.doped,
                            out=(self.d_adj[:nb], self.d_ch[:nb]))
            if path.cn_pass:                       # more sockets per position than the second-generation sampler takes
                E.cn_sockets(self.p, self.d_adj[:nb], out=self.d_cn[:nb])
        else:                                          # the samplers that write the CN table with the code
            sample = {"first_sock": E.sample_philox_sock, "cn16": E.sample_philox_cn16, "sock16": E.sample_philox_sock16,
                      "deg_sock16": E.sample_philox_deg_sock16, "wide_sock16": E.sample_philox_wide_sock16}[path.sampler]
            sample(self.p, self.seed, trial_key(self.index, sim, frame0), nb, eps, self.doped,
                   out=(self.d_adj[:nb], self.d_cn[:nb], self.d_ch[:nb]))

    # -- one ε point -------------------------------------------------------------------------------
    @staticmethod
    def split_round(frames_left, batch, world):
        """Frames of one round and their even split over the ranks (contiguous ranges in frame order): a round
        takes min(frames_left, world*batch) frames, rank r gets ⌈·⌉ or ⌊·⌋ of them — at the reference's defaults
        (1000 frames per point, BPF:65) every rank of an 8-GPU job decodes 125 frames, none idles."""
        R = min(frames_left, world * batch)
        base, rem = divmod(R, world)
        sizes = [base + (1 if r < rem else 0) for r in range(world)]
        offs = [sum(sizes[:r]) for r in range(world)]
        return R, sizes, offs

    def run_point(self, sim, eps, min_frame_err, max_frames, on_batch=None, defer_abort=False):
        """Frames 0,1,2,… of the point until frame_err >= min_frame_err or max_frames frames, in frame
        order (BPF:2117-2144).  Every round takes the next min(frames left, world·batch) frames and splits them
        evenly over the ranks; the per-trial counter rows are all-gathered and accumulated in frame order on
        every rank, so all ranks cut at the same frame.  The host looks at the run counters only in rounds in
        which the stop rule could trip (frames so far + this round >= min_frame_err); other rounds stay
        asynchronous.  on_batch(frame0, frames_used, result) sees this rank's batches.
        A frame that breaks decodeBP's invariant aborts the process as in the reference (BPF:1035-1039) — every rank of a
        frame-sharded job sees it in the gathered rows and leaves together; with defer_abort the point comes back with
        .bad set instead, for callers whose other ranks are busy elsewhere and must be told first.
        With runs=True the point's .runs holds engine.chain_runs over exactly the frames the point consumed — of every round
        this rank's first max(0, min(nb, used_round - off)) trials, what on_batch is told — summed over the ranks of a
        frame-sharded job by one all-reduce."""
        p, B, W = self.p, self.batch, self.world
        i_frames, i_ferr, i_status = RUN_NAMES.index("frames"), RUN_NAMES.index("frame_err"), \
            E.COUNTER_NAMES.index("status")
        if self.rng == "glibc":
            self.glibc.new_point()
        run = self._new_run()
        bad = torch.zeros((), dtype=torch.bool, device=run.device)
        frame0, consumed = 0, 0
        racc = None
        while frame0 < max_frames:
            R, sizes, offs = self.split_round(max_frames - frame0, B, W)
            nb, off = sizes[self.rank], offs[self.rank]
            res = None
            snap = self.glibc.snapshot() if self.rng == "glibc" else None
            if nb:
                self.fill_batch(sim, eps, frame0 + off, nb)
                res = self.decode_batch(nb, want_rows=on_batch is not None and self.rows_cap > 0)
            if W > 1:
                m = max(sizes)
                if nb < m:
                    self.d_cnt[nb:m].zero_()
                gathered = [torch.empty_like(self.d_cnt[:m]) for _ in range(W)]
                self.dist.all_gather(gathered, self.d_cnt[:m].contiguous())
                allcnt = torch.cat([g[:s] for g, s in zip(gathered, sizes)], dim=0).contiguous()
            else:
                allcnt = self.d_cnt[:nb]
            self._accumulate(allcnt, run, min_frame_err)
            can_trip = min_frame_err > 0 and frame0 + R >= min_frame_err
            if can_trip:
                r = run.cpu().numpy()
                used_round = int(r[i_frames]) - consumed
                consumed = int(r[i_frames])
                stopped = r[i_ferr] >= min_frame_err
            else:
                used_round, stopped = R, False
                consumed += R
            bad |= (allcnt[:used_round, i_status] != 0).any()
            if on_batch is not None and nb:
                on_batch(frame0 + off, max(0, min(nb, used_round - off)), res)
            if self.runs and nb and used_round - off > 0:
                racc = E.chain_runs(p, res["erased"][:min(nb, used_round - off)], acc=racc)
            if stopped and snap is not None and used_round < nb:
                # the reference stops drawing at the tripping frame: rewind the stream to just after it
                self.glibc.restore(snap)
                self.glibc.next_frames(used_round, eps, self.doped)
            frame0 += R
            if stopped:
                break
        if bool(bad) and not defer_abort:
            abort_invariant()
        return PointResult(eps, p.n, p.L, run.cpu().numpy(), bad=bool(bad), runs=self._point_runs(racc, run.device))

    def _point_runs(self, racc, device):
        """run_point's .runs: the three accumulators as numpy arrays (zeros from a rank that decoded nothing), summed over the
        ranks of a frame-sharded job; None without runs=True."""
        if not self.runs:
            return None
        shapes = runs_shapes(self.p.L)
        if racc is None:
            flat = torch.zeros(sum(int(np.prod(sh)) for _, sh in shapes), dtype=torch.int64, device=device)
        else:
            flat = torch.cat([racc[name].reshape(-1) for name, _ in shapes])
        if self.world > 1:
            self.dist.all_reduce(flat)
        return runs_unflatten(self.p.L, flat.cpu().numpy())

    def run_point_caps(self, sim, eps, min_frame_err, max_frames):
        """run_point for every cap of self.caps from one sampling pass and one decode per batch: one PointResult per cap,
        each what run_point with max_it = that cap returns.  Every cap keeps its own ordered stop (its own frame_err; frames
        past its tripping frame are not counted for it); the point ends when every cap has stopped.  Rounds, batches and
        the frame split over the ranks are run_point's, so each cap sees the frames a single-cap run sees.  A cap whose
        frames broke decodeBP's invariant comes back with .bad set (the caller decides when to abort: the other caps go on)."""
        p, B, W, K = self.p, self.batch, self.world, len(self.caps)
        i_frames, i_ferr, i_status = RUN_NAMES.index("frames"), RUN_NAMES.index("frame_err"), \
            E.COUNTER_NAMES.index("status")
        runs = [self._new_run() for _ in range(K)]
        bad = torch.zeros(K, dtype=torch.bool, device=runs[0].device)
        stopped = [False] * K
        consumed = [0] * K
        frame0 = 0
        while frame0 < max_frames and not all(stopped):
            R, sizes, offs = self.split_round(max_frames - frame0, B, W)
            nb, off = sizes[self.rank], offs[self.rank]
            cnt = None
            if nb:
                self.fill_batch(sim, eps, frame0 + off, nb)
                cnt = self.decode_batch_caps(nb)
            allcnt = E.gather_frames(self.dist, cnt, sizes, dim=1, shape=(K, 0, NCOUNTERS), device=self.d_cnt.device)
            can_trip = min_frame_err > 0 and frame0 + R >= min_frame_err
            live = [k for k in range(K) if not stopped[k]]
            for k in live:
                self._accumulate(allcnt[k].contiguous(), runs[k], min_frame_err)
            for k in live:
                if can_trip:
                    r = runs[k].cpu().numpy()
                    used_round = int(r[i_frames]) - consumed[k]
                    consumed[k] = int(r[i_frames])
                    stopped[k] = bool(r[i_ferr] >= min_frame_err)
                else:
                    used_round = R
                    consumed[k] += R
                bad[k] |= (allcnt[k, :used_round, i_status] != 0).any()
            frame0 += R
        bad = bad.cpu().tolist()
        return [PointResult(eps, p.n, p.L, runs[k].cpu().numpy(), bad=bad[k]) for k in range(K)]


def sampled_table_reason(p, rng, path, want=True):
    """Why a configuration whose path (before this switch) is `path` does not take the CN -> socket table from the
    first-generation sampler's own launch, or None where it does.  want: the Simulator's sampled_table argument (None:
    SAMPLED_TABLE_BY_DEFAULT)."""
    return _sampled_table_rule(_config(p, rng=rng, sampled_table=want), _capabilities(p), path)


def sampler2_deg_reason(p, rng, path, want=True):
    """Why a configuration whose path (before this switch) is `path` does not take the second-generation sampler of the pairs
    (3,6) and (5,10), or None where it does.  want: the Simulator's sampler2 argument (None: SAMPLER2_DEG_BY_DEFAULT)."""
    return _sampler2_deg_rule(_config(p, rng=rng, sampler2=want), _capabilities(p), path)


def sampler2_wide_reason(p, rng, path, want=True):
    """Why a configuration whose path (before this switch) is `path` does not take the wide second-generation sampler (more than
    8192 sockets per position), or None where it does.  want: the Simulator's sampler2_wide argument (None:
    SAMPLER2_WIDE_BY_DEFAULT)."""
    return _sampler2_wide_rule(_config(p, rng=rng, sampler2_wide=want), _capabilities(p), path)


def ring_deg_reason(p, W, rng, want=True):
    """Why decoder="sw" does not take the ring window decoder of the pairs (3,6) and (5,10) — sampler (first generation) +
    cn_sockets pass + sw_ring through the _deg entry points — on this configuration, or None where it does.  want: the
    Simulator's ring argument (None: RING_DEG_BY_DEFAULT)."""
    return _ring_rule(_config(p, W, "sw", rng, ring=want), _capabilities(p, W))


def classical_ring_reason(p, W, rng, want=True):
    """Why decoder="swc" does not take the classical ring window decoder on this configuration, or None where it does.
    want: the Simulator's ring argument (None: CLASSICAL_RING_BY_DEFAULT)."""
    return _ring_rule(_config(p, W, "swc", rng, ring=want), _capabilities(p, W))


def caps_sequential_reason(p, rng, num_doped, schedule, fused=None, wide=None, deg=None):
    """Why `bp_lim_iter --caps` runs its caps one after another instead of from one decode, or None.  The fused decode is
    used only where each cap's file is exactly the single-cap file and the level-synchronous 4-bit decoder takes the ensemble.
    fused, wide, deg: the Simulator's fused_caps, wide and deg (None: CAPS_FORMS_BY_DEFAULT; no veto) — with the fused path on,
    the wide form and the pairs (3,6) and (5,10) fuse as well (_caps_rule)."""
    config = _config(p, rng=rng, schedule=schedule, caps=True, num_doped=num_doped, wide=wide, deg=deg, fused_caps=fused)
    return _caps_rule(config, _capabilities(p))[1]


def _caps_list(text):
    """--caps 175,200,250 → [175, 200, 250]"""
    try:
        return [int(x) for x in text.split(",") if x.strip()]
    except ValueError:
        raise argparse.ArgumentTypeError("--caps takes a comma-separated list of integers: %r" % text)


def abort_invariant():
    """The reference aborts the process at a frame that recovers more VNs than it had degree-1 CNs (BPF:1035-1039)."""
    print("ARGH! RECOVERED MORE VNs THAN deg-1 CNs! Aborting!", flush=True)
    raise SystemExit(-1)


def _run_caps(prog, index, W, num_doped, max_it, extra, opts, p, grid, doped, shard, by_points):
    """`bp_lim_iter … --caps`: the files of MAX_IT and of every --caps value, each what `bp_lim_iter` with that MAX_IT
    writes — from one decode per batch with a checkpoint at every cap where that is exact, else one run per cap."""
    dist, rank, world = _dist()
    file_its = sorted(set(opts.caps) | {max_it})                  # the MAX_IT of each file
    fused, wide, deg = (_switch(opts, name) for name in ("caps_fused", "wide", "deg"))
    reason = caps_sequential_reason(p, opts.rng, num_doped, getattr(opts, "schedule", "flooding"), fused, wide, deg)
    verbose = rank == 0 and not opts.quiet
    if reason is not None and fused:
        raise SystemExit("--caps-fused on: " + reason)
    if reason is not None:
        if verbose:
            print("[scldpc] kernels: --caps runs %d single-cap passes one after another (%s)" % (len(file_its), reason),
                  file=sys.stderr, flush=True)
        one = copy.copy(opts)
        one.caps = None
        aborted = False
        for v in file_its:
            try:
                run_program(prog, index, W, num_doped, v, extra, one)
            except SystemExit as e:                               # abort_invariant: the other caps go on
                if e.code != -1:
                    raise
                aborted = True
        if aborted:
            raise SystemExit(-1)
        return 0
    caps = sorted(set(max(1, v) for v in file_its))               # at least one iteration runs (BPF:1065), as run_program
    if len(caps) > E.MAX_CAPS:
        raise SystemExit("--caps: at most %d distinct caps per run (%d given)" % (E.MAX_CAPS, len(caps)))
    slot = {v: caps.index(max(1, v)) for v in file_its}
    sim_obj = Simulator(p, decoder="full", W=W, max_it=caps[-1], is_term=True, doped=doped, batch=opts.batch, rng=opts.rng,
                        seed=opts.seed, schedule="flooding", shard_frames=shard == "frames",
                        device=getattr(opts, "device", None), index=index, verbose=verbose, caps=caps, wide=wide, deg=deg,
                        fused_caps=fused, sampled_table=_switch(opts, "sampled_table"), sampler2=_switch(opts, "sampler2"),
                        sampler2_wide=_switch(opts, "sampler2_wide"))
    _check_sampler_switches(opts, sim_obj)
    outdir = opts.outdir
    os.makedirs(outdir, exist_ok=True)
    paths = {v: os.path.join(outdir, result_filename(prog, p, W, v, 0, index)) for v in file_its}
    t0 = time.time()

    def report(v, point):
        if verbose:
            r = point.run
            print("[%dit] %f %e %e %e   (f=%d, %.1fs)" % (v, point.eps, r["users_err"] / p.n / point.f, r["frame_err"] / point.f,
                                                         r["block_err"] / p.L / point.f, point.f, time.time() - t0), flush=True)

    K = len(caps)
    if by_points:
        # run_program's points mode with a cap axis: table [points][K][NRUN counters + abort flag], one all-reduce at the
        # end, rank 0 writes the K files in grid order, each up to its own first broken point
        parts = {v: paths[v] + ".rank%d.part" % rank for v in file_its}
        table = torch.zeros((grid.num_points, K, NRUN + 1), dtype=torch.int64, device=sim_obj.device)
        gone = [False] * K                                        # this rank's single-cap process of that cap has aborted
        for sim in range(rank, grid.num_points, world):
            points = sim_obj.run_point_caps(sim, grid.eps(sim), grid.min_frame_err, grid.max_frames)
            for k, point in enumerate(points):
                if not gone[k]:
                    table[sim, k, :NRUN] = torch.tensor([point.run[n] for n in RUN_NAMES], dtype=torch.int64,
                                                        device=sim_obj.device)
                    table[sim, k, NRUN] = int(point.bad)
            for v in file_its:
                if not gone[slot[v]]:
                    with open(parts[v], "a" if sim != rank else "w") as f:
                        f.write("%d %s" % (sim, points[slot[v]].row()))
            gone = [g or pt.bad for g, pt in zip(gone, points)]
            if all(gone):
                break
        dist.all_reduce(table)
        rows = table.cpu().numpy()
        any_bad = False
        for v in file_its:
            k = slot[v]
            first_bad = next((s for s in range(grid.num_points) if rows[s, k, NRUN]), None)
            any_bad = any_bad or first_bad is not None
            if rank == 0:
                for sim in range(grid.num_points if first_bad is None else first_bad):
                    pt = PointResult(grid.eps(sim), p.n, p.L, rows[sim, k, :NRUN])
                    if pt.f == 0:
                        break
                    write_risultati(paths[v], sim, pt)
                    report(v, pt)
        dist.barrier()
        for v in file_its:
            if os.path.exists(parts[v]):
                os.remove(parts[v])
        if any_bad:
            abort_invariant()
        return 0

    gone = [False] * K                                            # the single-cap run of that cap has aborted
    for sim in range(grid.num_points):
        points = sim_obj.run_point_caps(sim, grid.eps(sim), grid.min_frame_err, grid.max_frames)
        for k, point in enumerate(points):
            gone[k] = gone[k] or point.bad
        for v in file_its:
            if not gone[slot[v]] and rank == 0:
                write_risultati(paths[v], sim, points[slot[v]])
                report(v, points[slot[v]])
    if any(gone):
        abort_invariant()
    return 0


def _write_traj_rows(fh, rows, counters, nb, cols=4):
    """Per frame: one line per iteration `iter\\tdeg1\\trecovered\\tfirst_pos`, then an empty line
    (BPT:988,1051,1145).  cols=3 drops the last column: the layout of the published `…L50_M2500…` files
    (an older build of the program; read by NB cell 40:10-19 with a 3-column unpack)."""
    rows = rows.cpu().numpy()
    its = counters[:, E.COUNTER_NAMES.index("iterations")].cpu().numpy()
    out = []
    for t in range(nb):
        k = int(its[t])
        if k > rows.shape[1]:
            raise RuntimeError(f"trajectory of {k} iterations exceeds rows_cap={rows.shape[1]}; raise --rows-cap")
        r = rows[t, :k]
        if cols == 3:
            out.append("".join("%d\t%d\t%d\n" % (i, r[i, 0], r[i, 1]) for i in range(k)))
        else:
            out.append("".join("%d\t%d\t%d\t%d\n" % (i, r[i, 0], r[i, 1], r[i, 2]) for i in range(k)))
        out.append("\n")
    fh.write("".join(out))


# Whether bp_lim_iter --schedule fixpoint takes run_grid_fused (one sampled code and one decoder launch per batch for the whole ε
# grid: engine.channel_levels + engine.full_bp_eps) where --eps-fused is "auto" or absent, instead of one run_point per ε.  Unlike
# the other *_BY_DEFAULT this switch changes the FILE (every point decodes the codes of point 0, see run_grid_fused), so no
# measurement alone can flip it; kept False here: the flip is a change of its own.
BP_EPS_FUSED_BY_DEFAULT = False


def eps_fused_reason(prog, p, es, schedule="fixpoint", max_it=0, caps=None, window="off", rng="philox", shard="auto"):
    """Why `--eps-fused on` cannot run this configuration, or None where it can.  A pure function (the shape rule is the
    library's workspace query, a host function): no device work.  prog: the program; es: the ε of the grid; max_it: the cap as
    the Simulator takes it (0: none — the command line's MAX_IT = 0 arrives here as 1, BPF:1065); caps: --caps; shard: --shard
    as given."""
    if prog != "bp_lim_iter":
        return ("the ε walk is unlimited full BP on one sampled code (bp_lim_iter --schedule fixpoint); %s takes no such path"
                % prog)
    if schedule != "fixpoint":
        return ("--schedule %s counts flooding iterations, which the ε walk does not have: peeling on from the residual of the "
                "point before gives the fixpoint, not the iterations (pass --schedule fixpoint)" % schedule)
    if 0 < max_it < 1000000:
        return ("MAX_IT = %d binds: a capped result depends on the schedule, and only the fixpoint of unlimited full BP is the "
                "maximal stopping set the ε walk computes (pass MAX_IT >= 1000000)" % max_it)
    if caps:
        return "--caps asks for capped results, which depend on the schedule: the ε walk computes the fixpoint only"
    if window == "classical":
        return ("--window classical decodes window by window with MAX_IT iterations each: its result depends on the schedule, "
                "not on the stopping sets alone")
    if rng != "philox":
        return ("--rng %s replays one sequential random() stream, a fresh code for every frame of every point: nothing is shared "
                "between the points (pass --rng philox)" % rng)
    if shard == "points":
        return ("--shard points gives every rank ε points of its own, and the ε walk decodes all points of a frame in one launch: "
                "its ranks share the frames (--shard frames, or auto)")
    from .peeling_decoding import curve_stages
    K = len(curve_stages(es)[0])
    if K > E.EPS_MAX_POINTS:
        return "at most %d distinct ε points in one run (got %d)" % (E.EPS_MAX_POINTS, K)
    try:
        E.full_bp_eps_workspace_bytes(p, 1, p.cns_pos <= 65536)             # the entry's own shape rule; needs no device
    except E.ScldpcError as err:
        return str(err)
    return None


def _refuse_shape(workspace_bytes, p, who):
    """ValueError(who + the library's text) for a shape the entry of the workspace query refuses; needs no device."""
    try:
        workspace_bytes(p, 1, p.cns_pos <= 65536)
    except E.ScldpcError as err:
        raise ValueError("%s: %s" % (who, err))


class _CodeRounds:
    """The rounds of the drivers that decode one sampled code per frame (run_grid_fused, run_thresholds, run_vn_thresholds):
    the ranks and the device, the code buffers of `batch` frames (2-byte rows where the sampler offers them), and per round
    run_point's split (split_round) with the first-generation sampler call at eps_top for this rank's frames, keyed
    trial_key(index, 0, frame); the sampler's channel is not used."""

    def __init__(self, p, seed, index, eps_top, doped, batch, device, shard_frames):
        self.p, self.seed, self.index, self.eps_top, self.doped, self.B = p, seed, index, eps_top, tuple(doped), int(batch)
        self.dist, self.rank, self.W = _dist() if shard_frames else (None, 0, 1)
        self.device = torch.device(device) if device is not None else E.local_device()
        adj16 = p.cns_pos <= 65536
        self.d_adj = self.buffer(p.n, p.dv, dtype=torch.int16 if adj16 else torch.int32)
        self.d_ch = self.buffer(p.nw)

    def buffer(self, *width, dtype=torch.int32):
        return torch.empty((self.B,) + width, dtype=dtype, device=self.device)

    def __call__(self, frames):
        """Yields (frame0, R, nb, off, key, d_adj[:nb], gather) per round of up to `frames` frames: the round's first frame and
        size, this rank's share, its offset in the round and first key, its codes (sampled only where nb > 0), and
        engine.gather_frames bound to the round's split.  Lazy: a caller that leaves the loop samples nothing further."""
        frame0 = 0
        while frame0 < frames:
            R, sizes, offs = Simulator.split_round(frames - frame0, self.B, self.W)
            nb, off = sizes[self.rank], offs[self.rank]
            key = trial_key(self.index, 0, frame0 + off) if nb else None
            if nb:
                E.sample_philox(self.p, self.seed, key, nb, self.eps_top, self.doped, out=(self.d_adj[:nb], self.d_ch[:nb]))

            def gather(part, dim=0, shape=None, sizes=sizes):
                return E.gather_frames(self.dist, part, sizes, dim, shape, device=self.device)
            yield frame0, R, nb, off, key, self.d_adj[:nb], gather
            frame0 += R


def run_grid_fused(p, es, min_frame_err, max_frames, seed, index=0, is_term=True, doped=(), batch=2048, device=None,
                   shard_frames=True, runs=False, defer_abort=False, verbose=False):
    """Unlimited full BP at every ε of es from ONE sampled code per frame: a list of PointResult in the caller's order, point i
    what Simulator(p, schedule="fixpoint", seed=seed, index=index, …).run_point(0, es[i], min_frame_err, max_frames) returns,
    value for value (.runs included with runs=True) — except run["iterations"], the sum of the kernels' round counts, which every
    fixpoint kernel fills with rounds of its own and no file holds.

    NOT what a loop over run_point(sim, es[sim], …) returns: that loop keys frame f of point sim as trial_key(index, sim, f), so
    its points see different codes; here every point decodes the frames trial_key(index, 0, f), the codes of point 0.  Point 0
    is the same; every other point is another sample of the same distribution, and the points are positively correlated with
    each other (common random numbers) — differences between neighbouring points are less noisy, a sum over points more.

    Per round: one first-generation sampler call at max(es) for the codes (2-byte rows where the sampler offers them; its
    channel is not used), engine.channel_levels over the live points, one engine.full_bp_eps (the fixpoint of point k by
    peeling on from the residual of point k - 1: the erased sets of a descending grid are nested, and what unlimited flooding
    converges to is the maximal stopping set of the erased set, whatever the schedule), engine.accumulate_run per live point.
    ε with one threshold are one stage.  A point is finished when its frame_err reaches min_frame_err or its frames reach
    max_frames, and leaves the later rounds.  Rounds and the frame split over the ranks are run_point's (split_round); one
    all-gather per round carries the [K_live, m, 8] rows, so every rank cuts every point at the same frame; the host looks at the
    run counters only in rounds in which the stop rule could trip.  A frame that breaks decodeBP's invariant (status != 0) aborts
    as in run_point; with defer_abort the points come back with .bad set."""
    from .peeling_decoding import curve_stages
    es = [float(e) for e in es]
    if not es:
        return []
    stage_eps, stage_of = curve_stages(es)
    K = len(stage_eps)
    if K > E.EPS_MAX_POINTS:
        raise ValueError("eps_fused: at most %d distinct ε points in one run (got %d)" % (E.EPS_MAX_POINTS, K))
    _refuse_shape(E.full_bp_eps_workspace_bytes, p, "eps_fused")
    rounds = _CodeRounds(p, seed, index, stage_eps[0], doped, batch, device, shard_frames)
    device, doped = rounds.device, rounds.doped
    if verbose:
        print("[scldpc] kernels: sampler (first generation) + channel_levels + full_bp_eps (%d ε points from one code)" % K,
              file=sys.stderr, flush=True)
    i_frames, i_ferr, i_status = RUN_NAMES.index("frames"), RUN_NAMES.index("frame_err"), E.COUNTER_NAMES.index("status")
    d_lev = rounds.buffer(p.n, dtype=torch.uint8)
    d_cnt = torch.empty(K * rounds.B * NCOUNTERS, dtype=torch.int32, device=device)
    run = torch.zeros((K, NRUN), dtype=torch.int64, device=device)
    bad = torch.zeros(K, dtype=torch.bool, device=device)
    racc = [None] * K
    consumed = [0] * K
    live = list(range(K))                                               # stages still running, by descending ε
    for frame0, R, nb, off, key, d_adj, gather in rounds(max_frames):
        Kl = len(live)
        res = None
        if nb:
            E.channel_levels(p, seed, key, nb, [stage_eps[k] for k in live], doped, device=device, out=d_lev[:nb])
            res = E.full_bp_eps(p, d_adj, d_lev[:nb], Kl, is_term=is_term, want_erased=runs,
                                counters=d_cnt[:Kl * nb * NCOUNTERS].view(Kl, nb, NCOUNTERS))
        allcnt = gather(res["counters"] if nb else None, dim=1, shape=(Kl, 0, NCOUNTERS))
        for i, k in enumerate(live):
            E.accumulate_run(allcnt[i], run[k], min_frame_err)
        can_trip = min_frame_err > 0 and frame0 + R >= min_frame_err
        tot = run.cpu().numpy() if can_trip else None                   # every row in one transfer
        still = []
        for i, k in enumerate(live):
            if can_trip:
                used_round = int(tot[k, i_frames]) - consumed[k]
                consumed[k] = int(tot[k, i_frames])
                stopped = tot[k, i_ferr] >= min_frame_err
            else:
                used_round, stopped = R, False
                consumed[k] += R
            bad[k] |= (allcnt[i, :used_round, i_status] != 0).any()
            if runs and nb and used_round - off > 0:
                racc[k] = E.chain_runs(p, res["erased"][i][:min(nb, used_round - off)], acc=racc[k])
            if not stopped:
                still.append(k)
        live = still
        if not live:
            break                                                       # (before the generator samples the next round)
    bad = bad.cpu().tolist()
    if any(bad) and not defer_abort:
        abort_invariant()
    tot = run.cpu().numpy()
    stage_runs = [None] * K
    if runs:
        shapes = runs_shapes(p.L)
        for k in range(K):                                              # one all-reduce per point, as run_point's
            flat = (torch.cat([racc[k][name].reshape(-1) for name, _ in shapes]) if racc[k] is not None else
                    torch.zeros(sum(int(np.prod(sh)) for _, sh in shapes), dtype=torch.int64, device=device))
            if rounds.W > 1:
                rounds.dist.all_reduce(flat)
            stage_runs[k] = runs_unflatten(p.L, flat.cpu().numpy())
    return [PointResult(e, p.n, p.L, tot[k], bad=bad[k], runs=copy.deepcopy(stage_runs[k])) for e, k in zip(es, stage_of)]


def _check_eps_fused(prog, opts):
    """--eps-fused against the rest of the command line: exits with the reason for `on` where the ε walk cannot run (before any
    device work); else whether the run takes it."""
    explicit = _switch(opts, "eps_fused")                               # auto: where it applies, if BP_EPS_FUSED_BY_DEFAULT
    want = BP_EPS_FUSED_BY_DEFAULT if explicit is None else explicit
    if not want:
        return False
    p, grid = _ensemble_and_grid(prog, opts)
    reason = eps_fused_reason(prog, p, [grid.eps(k) for k in range(grid.num_points)], getattr(opts, "schedule", "flooding"),
                              max(1, opts.MAX_IT), getattr(opts, "caps", None), getattr(opts, "window", "off"), opts.rng,
                              getattr(opts, "shard", "auto"))
    if reason is not None and explicit:
        raise SystemExit("--eps-fused on: " + reason)
    return reason is None


def _run_eps_fused(prog, index, W, max_it, opts, p, grid, doped, want_runs):
    """`bp_lim_iter … --schedule fixpoint --eps-fused on`: the file (and .runs.pkl) of the grid from run_grid_fused.  The ranks
    of a job share the frames."""
    dist, rank, world = _dist()
    es = [grid.eps(k) for k in range(grid.num_points)]
    t0 = time.time()
    points = run_grid_fused(p, es, grid.min_frame_err, grid.max_frames, opts.seed, index=index, doped=doped, batch=opts.batch,
                            device=getattr(opts, "device", None), runs=want_runs, defer_abort=True,
                            verbose=rank == 0 and not opts.quiet)
    first_bad = next((k for k, pt in enumerate(points) if pt.bad), None)
    points = points[:first_bad]                                         # the reference's process is gone at that point
    os.makedirs(opts.outdir, exist_ok=True)
    path = os.path.join(opts.outdir, result_filename(prog, p, W, max_it, 0, index))
    if rank == 0:
        for sim, pt in enumerate(points):
            write_risultati(path, sim, pt)
            if not opts.quiet:
                r = pt.run
                print("%f %e %e %e   (f=%d, %.1fs)" % (pt.eps, r["users_err"] / p.n / pt.f, r["frame_err"] / pt.f,
                                                       r["block_err"] / p.L / pt.f, pt.f, time.time() - t0), flush=True)
        if want_runs:
            with open(path + ".runs.pkl", "wb") as f:
                pickle.dump([dict(eps=pt.eps, frames=pt.f, **pt.runs) for pt in points], f)
    if first_bad is not None:
        abort_invariant()
    return 0


def _threshold_inside(e, t_lo, t_hi):
    """erasure_threshold(ε), or ValueError where it lies outside the window, in which the rows do not decide it."""
    th = E.erasure_threshold(e)
    if not t_lo <= th <= t_hi:
        raise ValueError("thresholds: ε = %.17g (threshold %d) lies outside the window [%d, %d]" % (e, th, t_lo, t_hi))
    return th


class FrameThresholds:
    """What run_thresholds returns: one row per frame, in frame order.
      rows    int64 [frames, 8], engine.frame_threshold's columns (E.THRESH_NAMES): thresh, status, size, first_pos, last_pos,
              stages, rescans, channel_erasures
      t_lo, t_hi   the window as integer thresholds, erasure_threshold(eps_lo) and erasure_threshold(eps_hi)
      bits    uint32 [frames, nw], the critical residuals (run_thresholds(want_bits=True)), else None"""

    def __init__(self, rows, t_lo, t_hi, bits=None):
        self.rows, self.t_lo, self.t_hi, self.bits = rows, int(t_lo), int(t_hi), bits

    def eps_star(self):
        """float64 [frames]: thresh / RAND_MAX of the frames whose threshold lies in the window, nan where it is censored
        (status 1: above the window; status 2: at or below its lower end)."""
        out = np.full(len(self.rows), np.nan)
        inside = self.rows[:, 1] == 0
        out[inside] = self.rows[inside, 0] / 2147483647.0
        return out

    def fer_at(self, es):
        """int64 [len(es)]: the number of frames that fail at each ε — status 2, or status 0 with thresh <=
        erasure_threshold(ε): what unlimited full BP of the same frames at ε counts as frame errors.  ValueError for an ε whose
        threshold lies outside [t_lo, t_hi], where the rows do not decide it."""
        thresh, status = self.rows[:, 0], self.rows[:, 1]
        out = []
        for e in np.asarray(es, dtype=np.float64).reshape(-1):
            th = _threshold_inside(e, self.t_lo, self.t_hi)
            out.append(int(((status == 2) | ((status == 0) & (thresh <= th))).sum()))
        return np.array(out, dtype=np.int64)


def _window(eps_lo, eps_hi, frames):
    """(t_lo, t_hi, frames) of a threshold driver's window and frame count, or the ValueError of either."""
    t_lo, t_hi = E.erasure_threshold(eps_lo), E.erasure_threshold(eps_hi)
    if not (0.0 <= float(eps_lo) <= 1.0 and 0.0 <= float(eps_hi) <= 1.0 and t_lo < t_hi):
        raise ValueError("thresholds: the window needs 0 <= eps_lo < eps_hi <= 1 with two distinct thresholds (got [%.17g, %.17g])"
                         % (eps_lo, eps_hi))
    if int(frames) < 0:
        raise ValueError("thresholds: a negative number of frames (%d)" % int(frames))
    return t_lo, t_hi, int(frames)


def _threshold_rounds(rounds, frames, ncols, widths, entry):
    """The rounds of run_thresholds and run_vn_thresholds: engine.channel_keys on the round's keys, entry(d_adj, d_keys, rows)
    with rows the round's slice of one [batch, ncols] buffer, and of its result the outputs named in widths (name -> columns),
    gathered over the ranks and copied to the host (a copy: the row buffer is written again in the next round).  Returns
    name -> int32 [frames, width], in frame order."""
    p = rounds.p
    d_keys, d_rows = rounds.buffer(p.n), rounds.buffer(ncols)
    parts = {name: [] for name in widths}
    for _, _, nb, _, key, d_adj, gather in rounds(frames):
        res = None
        if nb:
            E.channel_keys(p, rounds.seed, key, nb, rounds.doped, device=rounds.device, out=d_keys[:nb])
            res = entry(d_adj, d_keys[:nb], d_rows[:nb])
        for name, width in widths.items():
            parts[name].append(gather(res[name] if nb else None, shape=(0, width)).to("cpu", copy=True))
    return {name: np.ascontiguousarray(torch.cat(parts[name], dim=0).numpy()) if parts[name] else np.zeros((0, width), dtype=np.int32)
            for name, width in widths.items()}


def run_thresholds(p, eps_lo, eps_hi, frames, seed, index=0, is_term=True, doped=(), batch=2048, device=None, shard_frames=True,
                   want_bits=False, verbose=False):
    """The exact erasure threshold of every frame under unlimited full BP, for the window [eps_lo, eps_hi]: a FrameThresholds
    over the frames f = 0 … frames - 1, keyed trial_key(index, 0, f) — the codes and draws run_grid_fused decodes, so that
    .fer_at(es) is the frame_err column of run_grid_fused(p, es, 0, frames, seed, index=index, …), point for point, at every ε
    of the window and without a grid.

    Per round: one first-generation sampler call at eps_hi for the codes (2-byte rows where the sampler offers them; its
    channel is not used), engine.channel_keys, one engine.frame_threshold (the decode at erasure_threshold(eps_hi), then a
    bisection on the integer threshold inside its residual).  Rounds and the frame split over the ranks are run_point's
    (split_round); under torch.distributed one all-gather per round carries the [m, 8] rows.  A shape the entry refuses is a
    ValueError("thresholds: …") with the library's text, before anything is allocated."""
    t_lo, t_hi, frames = _window(eps_lo, eps_hi, frames)
    _refuse_shape(E.frame_threshold_workspace_bytes, p, "thresholds")
    rounds = _CodeRounds(p, seed, index, eps_hi, doped, batch, device, shard_frames)
    if verbose:
        print("[scldpc] kernels: sampler (first generation) + channel_keys + frame_threshold (window [%d, %d])" % (t_lo, t_hi),
              file=sys.stderr, flush=True)
    got = _threshold_rounds(rounds, frames, E.THRESH_NCOLS, {"rows": E.THRESH_NCOLS, **({"bits": p.nw} if want_bits else {})},
                            lambda d_adj, d_keys, rows: E.frame_threshold(p, d_adj, d_keys, t_lo, t_hi, is_term=is_term,
                                                                          want_bits=want_bits, rows=rows))
    return FrameThresholds(got["rows"].astype(np.int64), t_lo, t_hi, got["bits"].view(np.uint32) if want_bits else None)


class VnThresholds:
    """What run_vn_thresholds returns: the thresholds of every frame's positions (and VNs), in frame order.
      rows        int64 [frames, 8], engine.vn_threshold's columns (E.VNT_NAMES): thresh, status, top_size, size, steps, scans,
                  rescans, channel_erasures
      pos_thresh  int64 [frames, L]: the least tau over the VNs of the position, E.VNT_NONE where it never fails in the window;
                  t_lo means "at or below t_lo"
      counts      int64 [frames, len(grid)]: the VNs lost at each threshold of grid
      grid        the distinct thresholds of the caller's es, ascending
      t_lo, t_hi  the window as integer thresholds
      tau         int64 [frames, n], tau of every VN (run_vn_thresholds(want_tau=True)), else None"""

    def __init__(self, rows, pos_thresh, counts, grid, t_lo, t_hi, tau=None):
        self.rows, self.pos_thresh, self.counts, self.grid = rows, pos_thresh, counts, [int(t) for t in grid]
        self.t_lo, self.t_hi, self.tau = int(t_lo), int(t_hi), tau

    def _thresholds(self, es):
        return [_threshold_inside(e, self.t_lo, self.t_hi) for e in np.asarray(es, dtype=np.float64).reshape(-1)]

    def fer_at(self, es):
        """int64 [len(es)]: the frames that fail at each ε; FrameThresholds.fer_at of the same frames."""
        return FrameThresholds(self.rows, self.t_lo, self.t_hi).fer_at(es)

    def bler_at(self, es):
        """int64 [len(es), L]: the frames in which position q fails at each ε, for any ε of the window."""
        ths = self._thresholds(es)
        return np.array([(self.pos_thresh <= th).sum(axis=0) for th in ths], dtype=np.int64).reshape(len(ths), self.pos_thresh.shape[1])

    def block_err_at(self, es):
        """int64 [len(es)]: the failing positions summed over the frames: the block_err column of the grid decoders."""
        return self.bler_at(es).sum(axis=1)

    def ber_at(self, es):
        """int64 [len(es)]: the lost VNs summed over the frames (users_err): for ε whose threshold is on the grid, or for any ε
        of the window where tau was kept."""
        out = []
        for e, th in zip(np.asarray(es, dtype=np.float64).reshape(-1), self._thresholds(es)):
            if self.tau is not None:
                out.append(int((self.tau <= th).sum()))
            elif th in self.grid:
                out.append(int(self.counts[:, self.grid.index(th)].sum()))
            else:
                raise ValueError("thresholds: ε = %.17g (threshold %d) is not on the grid of counts, and tau was not kept" % (e, th))
        return np.array(out, dtype=np.int64)

    def pos_eps_star(self):
        """float64 [frames, L]: pos_thresh / RAND_MAX where the position's threshold lies inside the window, nan where it is
        censored (never fails in the window, or fails at or below its lower end)."""
        out = np.full(self.pos_thresh.shape, np.nan)
        inside = (self.pos_thresh > self.t_lo) & (self.pos_thresh <= self.t_hi)
        out[inside] = self.pos_thresh[inside] / 2147483647.0
        return out


def run_vn_thresholds(p, eps_lo, eps_hi, frames, seed, es=(), index=0, is_term=True, doped=(), batch=2048, device=None,
                      shard_frames=True, want_tau=False, verbose=False):
    """The exact erasure threshold of every position (and, with want_tau, of every VN) under unlimited full BP, for the window
    [eps_lo, eps_hi]: a VnThresholds over the frames run_thresholds decodes, keyed trial_key(index, 0, f), so that bler_at,
    block_err_at and fer_at give the block_err and frame_err of run_grid_fused on the same frames at every ε of the window, and
    ber_at its users_err at the points of es (their thresholds, sorted, merged where equal: the grid of `counts`).

    Per round: run_thresholds' sampler call and engine.channel_keys, then one engine.vn_threshold.  Under torch.distributed one
    all-gather per round carries the rows, positions, counts (and tau) of the round.  A shape the entry refuses, a grid outside
    the window or of more than E.VNT_MAX_POINTS thresholds is a ValueError("thresholds: …") before anything is allocated."""
    t_lo, t_hi, frames = _window(eps_lo, eps_hi, frames)
    grid = sorted(set(E.erasure_threshold(e) for e in np.asarray(es, dtype=np.float64).reshape(-1)))
    if grid and not (t_lo <= grid[0] and grid[-1] <= t_hi):
        raise ValueError("thresholds: the points of es lie outside the window [%d, %d]" % (t_lo, t_hi))
    if len(grid) > E.VNT_MAX_POINTS:
        raise ValueError("thresholds: %d distinct thresholds in es, at most %d" % (len(grid), E.VNT_MAX_POINTS))
    _refuse_shape(E.vn_threshold_workspace_bytes, p, "thresholds")
    rounds = _CodeRounds(p, seed, index, eps_hi, doped, batch, device, shard_frames)
    if verbose:
        print("[scldpc] kernels: sampler (first generation) + channel_keys + vn_threshold (window [%d, %d], %d grid points)"
              % (t_lo, t_hi, len(grid)), file=sys.stderr, flush=True)
    widths = {"rows": E.VNT_NCOLS, "pos_thresh": p.L, **({"counts": len(grid)} if grid else {}), **({"tau": p.n} if want_tau else {})}
    got = _threshold_rounds(rounds, frames, E.VNT_NCOLS, widths,
                            lambda d_adj, d_keys, rows: E.vn_threshold(p, d_adj, d_keys, t_lo, t_hi, grid=grid, is_term=is_term,
                                                                       want_tau=want_tau, rows=rows))
    return VnThresholds(got["rows"].astype(np.int64), got["pos_thresh"].view(np.uint32).astype(np.int64),
                        got["counts"].astype(np.int64) if grid else np.zeros((frames, 0), dtype=np.int64), grid, t_lo, t_hi,
                        got["tau"].view(np.uint32).astype(np.int64) if want_tau else None)


def _ensemble_and_grid(prog, opts):
    """The ensemble and the ε grid of a command line: the program's shipped #defines where no option overrides them."""
    d = DEFAULTS[prog]
    N = opts.N if opts.N else d["N"]
    L = opts.L if opts.L else d["L"]
    g = d["grid"]
    grid = GridSpec(opts.eps_ini if opts.eps_ini is not None else g.eps_ini,
                    opts.eps_delta if opts.eps_delta is not None else g.eps_delta,
                    opts.num_points if opts.num_points else g.num_points,
                    opts.min_frame_err if opts.min_frame_err is not None else g.min_frame_err,
                    opts.max_frames if opts.max_frames else g.max_frames)
    return E.make_params(opts.dv, opts.dc, L, N), grid


def run_program(prog, index, W, num_doped, max_it, extra, opts):
    """The body of main_terminated for one of the three executables."""
    p, grid = _ensemble_and_grid(prog, opts)
    # argv quirk kept: main_terminated reads the doped positions starting at argv[4], which is also
    # MAX_IT (BPF:2083-2091) — so with NUM_DOPED > 0 the first doped position equals MAX_IT.
    tail = [max_it] + list(opts.doped_argv)
    doped = [int(x) for x in tail[:num_doped]]
    if len(doped) < num_doped:
        raise SystemExit("NUM_DOPED=%d but only %d position arguments" % (num_doped, len(doped)))
    init_it, is_term = 0, True
    decoder = "full"
    if prog == "sw_lim_iter":
        decoder = "sw"
        init_it = extra if extra else max_it                       # BPW:2101-2102
    elif prog == "bp_traj":
        is_term = bool(extra)
    ring = _switch(opts, "ring")
    if prog == "bp_lim_iter":
        _check_window(opts)
        if getattr(opts, "window", "off") == "classical":
            # the reference with the commented call at BPF:2137-2138 swapped in: same file, MAX_IT iterations per window
            decoder = "swc"
            why = classical_ring_reason(p, W, opts.rng) if ring else None
            if why is not None:
                raise SystemExit("--ring on: " + why)
    dist, rank, world = _dist()
    if opts.rng == "glibc" and world > 1:
        # one srandom(seed) stream carried from frame to frame and from point to point (BPF:2057-2131): there is nothing to
        # shard, and ranks replaying it from its start would write correlated points that look like a reference replay
        raise SystemExit("--rng glibc replays the reference's one sequential random() stream: run it as a single process "
                         "(%d ranks here); use --rng philox for multi-GPU jobs" % world)
    # Sharding (module docstring): bp_traj — one replica (INDEX + rank) per rank; else ε points over the ranks when there
    # are at least as many points as ranks (the reference's own cluster model), else the frames of every point.
    shard = getattr(opts, "shard", "auto")
    if prog == "bp_traj":
        shard = "replicas"
    elif shard == "auto":
        shard = "points" if (world > 1 and grid.num_points >= world) else "frames"
    by_points = shard == "points" and world > 1
    replica = index + rank if shard == "replicas" else index
    want_runs = _check_runs(prog, opts)
    if _check_eps_fused(prog, opts):
        return _run_eps_fused(prog, index, W, max_it, opts, p, grid, doped, want_runs)
    if getattr(opts, "caps", None) and prog == "bp_lim_iter":
        return _run_caps(prog, index, W, num_doped, max_it, extra, opts, p, grid, doped, shard, by_points)
    # the decoders' loop is do { … } while (iter < MaxNumIt) (BPF:1065, BPT:1076): at least one iteration runs
    cap = max(1, max_it)
    if ring and prog == "sw_lim_iter":
        why = ring_deg_reason(p, W, opts.rng)
        if why is not None:
            raise SystemExit("--ring on: " + why)
    sim_obj = Simulator(p, decoder=decoder, W=W, max_it=cap, init_it=init_it,
                        is_term=is_term, doped=doped, batch=opts.batch, rng=opts.rng, seed=opts.seed,
                        rows_cap=opts.rows_cap if prog == "bp_traj" else 0, schedule=getattr(opts, "schedule", "flooding"),
                        shard_frames=shard == "frames", device=getattr(opts, "device", None), index=replica,
                        verbose=rank == 0 and not opts.quiet,
                        wide=_switch(opts, "wide"), deg=_switch(opts, "deg"), ring=ring if decoder in ("sw", "swc") else None,
                        sampled_table=_switch(opts, "sampled_table"), sampler2=_switch(opts, "sampler2"),
                        sampler2_wide=_switch(opts, "sampler2_wide"), **({"runs": True} if want_runs else {}))
    _check_sampler_switches(opts, sim_obj)
    outdir = opts.outdir
    os.makedirs(outdir, exist_ok=True)
    t0 = time.time()
    runs_out = []                                                   # --runs: one dict per ε point, pickled by rank 0
    nruns = sum(int(np.prod(sh)) for _, sh in runs_shapes(p.L))

    def keep_runs(point):
        runs_out.append(dict(eps=point.eps, frames=point.f, **point.runs))

    def write_runs():
        if want_runs and rank == 0:
            with open(os.path.join(outdir, result_filename(prog, p, W, max_it, init_it, index)) + ".runs.pkl", "wb") as f:
                pickle.dump(runs_out, f)

    def report(eps, point):
        if rank == 0 and not opts.quiet:
            r = point.run
            print("%f %e %e %e   (f=%d, %.1fs)" % (eps, r["users_err"] / p.n / point.f, r["frame_err"] / point.f,
                                                   r["block_err"] / p.L / point.f, point.f, time.time() - t0),
                  flush=True)

    if by_points:
        # Rank r runs points r, r + world, r + 2·world, … back to back — no barrier between points, so a rank whose points
        # stop early (frame_err >= 1000 long before max_frames) is not held up by the others.  Every finished point is
        # appended to the rank's own part file at once (what a killed job leaves behind, like the reference's per-point
        # fopen("a"), BPF:494-497); ONE all-reduce of the table [points][NRUN counters + abort flag] at the end hands the
        # rows to rank 0, which writes the file in grid order and removes the parts.  A point that breaks decodeBP's
        # invariant (BPF:1035-1039) only raises the flag: every rank reaches the all-reduce and all leave together.
        path = os.path.join(outdir, result_filename(prog, p, W, max_it, init_it, index))
        part = path + ".rank%d.part" % rank
        table = torch.zeros((grid.num_points, NRUN + 1), dtype=torch.int64, device=sim_obj.device)
        rtable = torch.zeros((grid.num_points, nruns), dtype=torch.int64, device=sim_obj.device) if want_runs else None
        for sim in range(rank, grid.num_points, world):
            point = sim_obj.run_point(sim, grid.eps(sim), grid.min_frame_err, grid.max_frames, defer_abort=True)
            table[sim, :NRUN] = torch.tensor([point.run[k] for k in RUN_NAMES], dtype=torch.int64, device=sim_obj.device)
            table[sim, NRUN] = int(point.bad)
            if want_runs:
                rtable[sim] = torch.from_numpy(runs_flatten(p.L, point.runs)).to(sim_obj.device)
            with open(part, "a" if sim != rank else "w") as f:
                f.write("%d %s" % (sim, point.row()))
            if point.bad:
                break                                   # the reference's process is gone at this point
        dist.all_reduce(table)
        if want_runs:
            dist.all_reduce(rtable)                     # the stacked per-point accumulators, once, next to the table
            rrows = rtable.cpu().numpy()
        rows = table.cpu().numpy()
        first_bad = next((s for s in range(grid.num_points) if rows[s, NRUN]), None)
        if rank == 0:
            for sim in range(grid.num_points if first_bad is None else first_bad):
                pt = PointResult(grid.eps(sim), p.n, p.L, rows[sim, :NRUN],
                                 runs=runs_unflatten(p.L, rrows[sim]) if want_runs else None)
                if pt.f == 0:
                    break                               # a rank stopped at an abort before reaching this point
                write_risultati(path, sim, pt)
                if want_runs:
                    keep_runs(pt)
                report(pt.eps, pt)
        write_runs()
        dist.barrier()
        if os.path.exists(part):
            os.remove(part)
        if first_bad is not None:
            abort_invariant()
        return 0

    for sim in range(grid.num_points):
        eps = grid.eps(sim)
        if prog == "bp_traj":
            # one file per ε point and per replica; this rank's replica writes its frames in order
            path = os.path.join(outdir, traj_filename(p, eps, max_it, is_term, replica))
            with open(path, "w") as fh:
                def on_batch(frame0, used, res):
                    _write_traj_rows(fh, res["rows"], res["counters"], used, cols=getattr(opts, "cols", 4))
                point = sim_obj.run_point(sim, eps, grid.min_frame_err, grid.max_frames, on_batch=on_batch,
                                          defer_abort=world > 1)
        else:
            point = sim_obj.run_point(sim, eps, grid.min_frame_err, grid.max_frames)
            if rank == 0:
                write_risultati(os.path.join(outdir, result_filename(prog, p, W, max_it, init_it, index)), sim, point)
            if want_runs:
                keep_runs(point)
        if prog == "bp_traj" and world > 1:
            # the replicas run independently; an abort in one of them (BPF:1035-1039) ends the job for all, together
            flag = torch.tensor([int(point.bad)], dtype=torch.int64, device=sim_obj.device)
            dist.all_reduce(flag)
            if int(flag.item()):
                abort_invariant()
        report(eps, point)
    write_runs()
    return 0


def _switch(opts, name):
    """An `--x on|off|auto` option as the Simulator's argument: True, False or None (auto, or a program without the option)."""
    return {"auto": None, "on": True, "off": False}[getattr(opts, name, "auto")]


def _check_sampler_switches(opts, sim_obj):
    """--sampler2 on, --sampler2-wide on or --sampled-table on where the Simulator did not take that sampler: exits with the
    reason (in the order in which the Simulator judges them)."""
    for name, reason in (("sampler2", "sampler2_deg_reason"), ("sampler2_wide", "sampler2_wide_reason"),
                         ("sampled_table", "sampled_table_reason")):
        if getattr(opts, name, "auto") == "on" and getattr(sim_obj, reason) is not None:
            raise SystemExit("--%s on: %s" % (name.replace("_", "-"), getattr(sim_obj, reason)))


def _check_runs(prog, opts):
    """--runs against the rest of the command line: exits with the reason (before any device work); else whether it is set."""
    want_runs = bool(getattr(opts, "runs", False))
    if want_runs and prog == "bp_traj":
        raise SystemExit("--runs: bp_traj writes trajectories, not block error rates; use bp_lim_iter or sw_lim_iter")
    if want_runs and getattr(opts, "caps", None):
        raise SystemExit("--runs: the cap checkpoints of --caps keep no erased bits; run one MAX_IT at a time")
    return want_runs


def _check_window(opts):
    """bp_lim_iter's --window / --ring against the rest of the command line: exits with the reason."""
    window, ring = getattr(opts, "window", "off"), getattr(opts, "ring", "auto")
    if window != "classical":
        if ring == "on":
            raise SystemExit("--ring on: needs --window classical (full BP has no window to keep in a ring)")
        return
    if getattr(opts, "caps", None):
        raise SystemExit("--window classical: --caps belongs to full BP (the cap checkpoints of one decode); MAX_IT is the cap of "
                         "every window here")
    if getattr(opts, "schedule", "flooding") != "flooding":
        raise SystemExit("--window classical: --schedule %s belongs to unlimited full BP; a window counts its flooding iterations"
                         % opts.schedule)


class _LimIterParser(argparse.ArgumentParser):
    """bp_lim_iter: combinations that cannot run end the program where the command line is read."""

    def parse_args(self, args=None, namespace=None):
        opts = super().parse_args(args, namespace)
        _check_window(opts)
        return opts


def _parser(prog):
    ap = (_LimIterParser if prog == "bp_lim_iter" else argparse.ArgumentParser)(prog=prog, description=__doc__.split("\n\n")[0])
    ap.add_argument("INDEX", type=int)
    ap.add_argument("W", type=int)
    ap.add_argument("NUM_DOPED", type=int)
    ap.add_argument("MAX_IT", type=int)
    if prog == "sw_lim_iter":
        ap.add_argument("INIT_IT", type=int)
    elif prog == "bp_traj":
        ap.add_argument("IS_TERM", type=int)
    ap.add_argument("doped_argv", nargs="*", type=int, help="further doped positions (see the argv quirk)")
    ap.add_argument("--dv", type=int, default=4)
    ap.add_argument("--dc", type=int, default=8)
    ap.add_argument("--L", type=int, default=0, help="Def_L (default: the source's value)")
    ap.add_argument("--N", type=int, default=0, help="VNs per position = Def_VNsPos = 2*Def_M")
    ap.add_argument("--eps-ini", type=float, default=None)
    ap.add_argument("--eps-delta", type=float, default=None)
    ap.add_argument("--num-points", type=int, default=0)
    ap.add_argument("--min-frame-err", type=int, default=None)
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--batch", type=int, default=2048, help="frames per device batch and rank")
    ap.add_argument("--rng", choices=("philox", "glibc"), default="philox")
    ap.add_argument("--seed", type=int, default=None, help="default: time-based like the reference (BPF:2059-2062)")
    ap.add_argument("--rows-cap", type=int, default=4096, help="bp_traj: max iterations kept per frame")
    ap.add_argument("--schedule", choices=("flooding", "fixpoint"), default="flooding",
                    help="bp_lim_iter with MAX_IT >= 10^6: 'fixpoint' decodes to the same residual without walking "
                         "the flooding iterations (same files; no iteration statistics)")
    if prog == "bp_lim_iter":
        ap.add_argument("--caps", type=_caps_list, default=None, metavar="K1,K2,…",
                        help="also write the files of these MAX_IT (one file per cap, each the file of a run with that "
                             "MAX_IT); from one decode per frame where that is exact, else one run per cap")
        ap.add_argument("--caps-fused", choices=("auto", "on", "off"), default="auto",
                        help="--caps with more than 65536 CNs per trial (e.g. --N 5000) or --dv/--dc 3/6 or 5/10: one decode "
                             "with a checkpoint at every cap (on), one run per cap (off), or the measured default (auto); same "
                             "files.  'on' where the one decode cannot apply is an error that names the limit")
    ap.add_argument("--wide", choices=("auto", "on", "off"), default="auto",
                    help="full BP of trials with more than 65536 CNs (e.g. the default N = 5000): the wide 4-bit level "
                         "decoder (on), the first-generation decoder (off), or the measured default (auto); same files")
    if prog != "sw_lim_iter":
        ap.add_argument("--deg", choices=("auto", "on", "off"), default="auto",
                        help="full BP with --dv/--dc 3/6 or 5/10: the 4-bit level decoder (on), the first-generation decoder "
                             "(off), or the measured default (auto); same files")
    if prog == "sw_lim_iter":
        ap.add_argument("--ring", choices=("auto", "on", "off"), default="auto",
                        help="--dv/--dc 3/6 or 5/10: the ring window decoder (on), the whole-chain kernel (off), or the measured "
                             "default (auto); same files")
    if prog == "bp_lim_iter":
        ap.add_argument("--window", choices=("off", "classical"), default="off",
                        help="classical: the classical sliding window of W positions (decodeBP_SW of the full-BP source, "
                             "BPF:627-897, whose call is commented out at BPF:2137-2138) with MAX_IT iterations per window, "
                             "instead of full BP; same file name and rows")
        ap.add_argument("--ring", choices=("auto", "on", "off"), default="auto",
                        help="--window classical with --dv/--dc 3/6, 4/8 or 5/10: the ring window decoder (on), the whole-chain "
                             "kernel (off), or the measured default (auto); same files.  'on' where the ring cannot apply is an "
                             "error that names the limit")
    ap.add_argument("--sampled-table", choices=("auto", "on", "off"), default="auto",
                    help="where the first-generation sampler is followed by a pass that builds the CN -> socket table: the sampler "
                         "writes the table itself (on), the separate pass (off), or the measured default (auto); same files.  "
                         "'on' where no such pass runs is an error that says why")
    ap.add_argument("--sampler2", choices=("auto", "on", "off"), default="auto",
                    help="--dv/--dc 3/6 or 5/10 with at most 8192 sockets per position, where the decoder reads a CN -> socket "
                         "table: the second-generation sampler draws the code and writes the table in one launch (on), the "
                         "first-generation sampler and its table pass (off), or the measured default (auto); same files.  'on' "
                         "where it does not apply is an error that says why")
    ap.add_argument("--sampler2-wide", choices=("auto", "on", "off"), default="auto",
                    help="--dv/--dc 3/6, 4/8 or 5/10 with more than 8192 and at most 20480 sockets per position (e.g. the default "
                         "N = 5000), where the decoder reads a CN -> socket table: the wide second-generation sampler draws the "
                         "code and writes the table in one launch (on), the first-generation sampler and its table pass (off), or "
                         "the measured default (auto); same files.  'on' where it does not apply is an error that says why")
    ap.add_argument("--runs", action="store_true",
                    help="bp_lim_iter, sw_lim_iter: also write <result file>.runs.pkl, a pickled list with one dict per ε point "
                         "{eps, frames, pos, run_hist, fail_hist}: where the failed positions of the point's frames sit and how "
                         "long their runs are (engine.chain_runs; include/scldpc_runs.h); the .dat is unchanged.  Not with --caps")
    ap.add_argument("--eps-fused", choices=("auto", "on", "off"), default="auto",
                    help="bp_lim_iter --schedule fixpoint with MAX_IT >= 10^6: every ε point of the grid from ONE sampled code per "
                         "frame and one decoder launch per batch (engine.channel_levels + engine.full_bp_eps).  NOT the same "
                         "file: every point decodes the codes of point 0 (frame f of every point is keyed as frame f of point "
                         "0), so row 0 is the unfused row 0 and every row k is the unfused program's point-0 run at ε_k — "
                         "another sample of the same distribution than the unfused row k, and positively correlated with the "
                         "other rows (common random numbers).  off, and auto for now: one sampler and one decode per point.  "
                         "'on' where it cannot apply is an error that says why")
    ap.add_argument("--shard", choices=("auto", "points", "frames"), default="auto",
                    help="multi-GPU: ε points over the ranks (the reference's cluster model; default when there are at "
                         "least as many points as ranks) or the frames of every point")
    if prog == "bp_traj":
        ap.add_argument("--cols", type=int, choices=(3, 4), default=4,
                        help="4: iter, deg1, recovered, first erased position (BPT:988,1051); 3: without the last "
                             "(the published L50_M2500 files, NB cell 40)")
    ap.add_argument("--outdir", default=".")
    ap.add_argument("--quiet", action="store_true")
    return ap


def main(prog, argv=None):
    opts = _parser(prog).parse_args(argv)
    _check_runs(prog, opts)
    _check_eps_fused(prog, opts)
    if opts.seed is None:
        opts.seed = int((time.time() % 1) * 1e6)                      # te.tv_usec (BPF:2061)
    joined = E.init_distributed()                                     # one process per GPU under torch.distributed.run
    extra = getattr(opts, "INIT_IT", None) if prog == "sw_lim_iter" else getattr(opts, "IS_TERM", None)
    rc = run_program(prog, opts.INDEX, opts.W, opts.NUM_DOPED, opts.MAX_IT, extra, opts)
    if joined:
        import torch.distributed as dist
        dist.destroy_process_group()
    return rc


def bp_lim_iter(argv=None):
    return main("bp_lim_iter", argv)


def sw_lim_iter(argv=None):
    return main("sw_lim_iter", argv)


def bp_traj(argv=None):
    return main("bp_traj", argv)


# ------------------------------------------------------------------------------------------------
# bp_thresholds: the exact erasure threshold of every frame (no counterpart in the reference)
# ------------------------------------------------------------------------------------------------
def _thresholds_parser():
    g = DEFAULTS["bp_lim_iter"]["grid"]
    ap = argparse.ArgumentParser(prog="bp_thresholds",
                                 description="exact per-frame erasure thresholds of unlimited full BP: for every frame the least "
                                             "integer threshold at which the decoder leaves a residual, bisected on the device")
    ap.add_argument("INDEX", type=int)
    ap.add_argument("W", type=int, help="0: full BP (a window decoder's result depends on the schedule, not on the stopping sets)")
    ap.add_argument("NUM_DOPED", type=int)
    ap.add_argument("FRAMES", type=int, help="frames 0 … FRAMES - 1 of the replica: the codes of bp_lim_iter's point 0")
    ap.add_argument("doped_argv", nargs="*", type=int, help="the NUM_DOPED doped positions")
    ap.add_argument("--dv", type=int, default=4)
    ap.add_argument("--dc", type=int, default=8)
    ap.add_argument("--L", type=int, default=0, help="Def_L (default: bp_lim_iter's)")
    ap.add_argument("--N", type=int, default=0, help="VNs per position (default: bp_lim_iter's)")
    ap.add_argument("--eps-lo", type=float, default=g.eps(g.num_points - 1), help="lower end of the window (default: the last "
                                                                                  "point of bp_lim_iter's grid)")
    ap.add_argument("--eps-hi", type=float, default=g.eps(0), help="upper end of the window (default: the first point of that grid)")
    ap.add_argument("--is-term", type=int, default=1, help="0: the truncated chain (the CNs beyond position L never fire)")
    ap.add_argument("--batch", type=int, default=2048, help="frames per device batch and rank")
    ap.add_argument("--seed", type=int, default=None, help="default: time-based, as bp_lim_iter's")
    ap.add_argument("--outdir", default=".")
    ap.add_argument("--quiet", action="store_true")
    return ap


def _check_thresholds(opts, prog="bp_thresholds", workspace_bytes=None):
    """The command line of `prog` — bp_thresholds, or bp_curves, which shares its arguments — against what the run can do: exits
    with `<prog>: <reason>` (before any device work), else (p, doped).  workspace_bytes: the workspace query of the program's
    entry, whose shape rule decides (default: frame_threshold's)."""
    def refuse(why):
        raise SystemExit(prog + ": " + why)
    d = DEFAULTS["bp_lim_iter"]
    if opts.W != 0:
        refuse("W = %d: a threshold is defined for unlimited full BP only (W = 0); a window decoder's result depends on its "
               "schedule" % opts.W)
    if opts.FRAMES < 1:
        refuse("FRAMES = %d: at least one frame" % opts.FRAMES)
    if not (0.0 <= opts.eps_lo < opts.eps_hi <= 1.0) or E.erasure_threshold(opts.eps_lo) >= E.erasure_threshold(opts.eps_hi):
        refuse("the window needs 0 <= --eps-lo < --eps-hi <= 1 with two distinct thresholds (got [%.17g, %.17g])"
               % (opts.eps_lo, opts.eps_hi))
    if opts.batch < 1:
        refuse("--batch %d: at least one frame per batch" % opts.batch)
    try:
        p = E.make_params(opts.dv, opts.dc, opts.L if opts.L else d["L"], opts.N if opts.N else d["N"])
    except ValueError as err:
        refuse(str(err))
    # (bp_lim_iter's argv quirk — its first doped position is MAX_IT, BPF:2083-2091 — has nothing to mirror here)
    if opts.NUM_DOPED < 0 or len(opts.doped_argv) < opts.NUM_DOPED:
        refuse("NUM_DOPED=%d but only %d position arguments" % (opts.NUM_DOPED, len(opts.doped_argv)))
    doped = [int(x) for x in opts.doped_argv[:opts.NUM_DOPED]]
    if any(not 0 <= x < p.L for x in doped):
        refuse("doped positions outside [0,%d): %s" % (p.L, doped))
    try:
        (workspace_bytes or E.frame_threshold_workspace_bytes)(p, 1, p.cns_pos <= 65536)   # the entry's own shape rule; needs no device
    except E.ScldpcError as err:
        refuse(str(err))
    return p, doped


def _thresholds_main(prog, argv, parser, workspace_bytes, run, suffix, payload, report, check=lambda opts: None):
    """A program over the thresholds of a replica's frames (bp_thresholds, bp_curves): the command line against check(opts) and
    _check_thresholds, the time-based seed, the job, run(opts)(p, eps_lo, eps_hi, FRAMES, seed, …) — run_thresholds' arguments —
    and on rank 0 the pickle dict(eps_lo, eps_hi, t_lo, t_hi, seed, index, **payload(opts, res)) at <bp_lim_iter's result file at
    MAX_IT 1000000> + suffix, then report(opts, p, res) unless --quiet."""
    opts = parser.parse_args(argv)
    check(opts)
    p, doped = _check_thresholds(opts, prog, workspace_bytes)
    if opts.seed is None:
        opts.seed = int((time.time() % 1) * 1e6)
    joined = E.init_distributed()
    rank = _dist()[1]
    res = run(opts)(p, opts.eps_lo, opts.eps_hi, opts.FRAMES, opts.seed, index=opts.INDEX, is_term=bool(opts.is_term),
                    doped=doped, batch=opts.batch, verbose=rank == 0 and not opts.quiet)
    if rank == 0:
        os.makedirs(opts.outdir, exist_ok=True)
        path = os.path.join(opts.outdir, result_filename("bp_lim_iter", p, 0, 1000000, 0, opts.INDEX) + suffix)
        with open(path, "wb") as f:
            pickle.dump(dict(eps_lo=opts.eps_lo, eps_hi=opts.eps_hi, t_lo=res.t_lo, t_hi=res.t_hi, seed=opts.seed, index=opts.INDEX,
                             **payload(opts, res)), f)
        if not opts.quiet:
            report(opts, p, res)
    if joined:
        import torch.distributed as dist_mod
        dist_mod.destroy_process_group()
    return 0


def bp_thresholds(argv=None):
    """`bp_thresholds INDEX W NUM_DOPED FRAMES [doped…]`: run_thresholds over the frames of the replica; rank 0 pickles
    dict(eps_lo, eps_hi, t_lo, t_hi, seed, index, rows) to <bp_lim_iter's result file at MAX_IT 1000000>.thresholds.pkl."""
    def report(opts, p, res):
        status = res.rows[:, 1]
        share = [float((status == s).mean()) for s in (0, 1, 2)]
        es = res.eps_star()[status == 0]
        print("frames %d   inside the window %.4f   above (decode at eps_hi) %.4f   at or below eps_lo %.4f"
              % (len(status), share[0], share[1], share[2]), flush=True)
        if es.size:
            print("eps*: mean %.6f   std %.6f   (%d uncensored frames)" % (es.mean(), es.std(ddof=1) if es.size > 1 else 0.0,
                                                                          es.size), flush=True)
    return _thresholds_main("bp_thresholds", argv, _thresholds_parser(), E.frame_threshold_workspace_bytes,
                            lambda opts: run_thresholds, ".thresholds.pkl", lambda opts, res: dict(rows=res.rows), report)


# ------------------------------------------------------------------------------------------------
# bp_curves: BER, FER and block error rate over a window from the exact thresholds of every VN (no counterpart in the reference)
# ------------------------------------------------------------------------------------------------
def _curves_parser():
    ap = _thresholds_parser()
    ap.prog = "bp_curves"
    ap.description = ("exact per-position erasure thresholds of unlimited full BP and, from the same frames, BER, FER and block "
                      "error rate at K evenly spaced points of the window")
    ap.add_argument("--points", type=int, default=DEFAULTS["bp_lim_iter"]["grid"].num_points,
                    help="K, the points printed and counted (default: bp_lim_iter's grid)")
    return ap


def _curves_points(opts):
    """The K points of the command line, descending from --eps-hi; bp_lim_iter's own grid where nothing moved it."""
    g = DEFAULTS["bp_lim_iter"]["grid"]
    if (opts.eps_lo, opts.eps_hi, opts.points) == (g.eps(g.num_points - 1), g.eps(0), g.num_points):
        return [g.eps(i) for i in range(g.num_points)]
    if opts.points == 1:
        return [opts.eps_hi]
    return [opts.eps_hi + (opts.eps_lo - opts.eps_hi) * i / (opts.points - 1) if i < opts.points - 1 else opts.eps_lo
            for i in range(opts.points)]


def bp_curves(argv=None):
    """`bp_curves INDEX W NUM_DOPED FRAMES [doped…]`: run_vn_thresholds over the frames of the replica; rank 0 pickles
    dict(eps_lo, eps_hi, t_lo, t_hi, seed, index, es, rows, pos_thresh, counts) to <bp_lim_iter's result file at MAX_IT
    1000000>.curves.pkl and prints, per point, the columns of PointResult.row() it has (the expurgated ones are 0)."""
    def check(opts):
        if not 1 <= opts.points <= E.VNT_MAX_POINTS:
            raise SystemExit("bp_curves: --points %d: between 1 and %d points" % (opts.points, E.VNT_MAX_POINTS))

    def report(opts, p, res):
        es = _curves_points(opts)
        users, frame, block = res.ber_at(es), res.fer_at(es), res.block_err_at(es)
        sys.stdout.write(RISULTATI_HEADER)
        for e, u, fe, b in zip(es, users, frame, block):
            run = dict.fromkeys(RUN_NAMES, 0)
            run.update(users_err=int(u), frame_err=int(fe), block_err=int(b), frames=opts.FRAMES)
            sys.stdout.write(PointResult(e, p.n, p.L, [run[k] for k in RUN_NAMES]).row())
        sys.stdout.flush()
    return _thresholds_main(
        "bp_curves", argv, _curves_parser(), E.vn_threshold_workspace_bytes,
        lambda opts: functools.partial(run_vn_thresholds, es=_curves_points(opts)), ".curves.pkl",
        lambda opts, res: dict(es=_curves_points(opts), rows=res.rows, pos_thresh=res.pos_thresh, counts=res.counts), report, check)


# ------------------------------------------------------------------------------------------------
# streaming mode: the CIRCULAR build of the reference (`sw INDEX W NUM_DOPED DOPED_POSITIONS…`, BPF:1934-2054)
# ------------------------------------------------------------------------------------------------
STREAM_HEADER = ("p BER BLER BER_EXP BLER_EXP bit_err bit_gen block_err block_gen bit_err_exp bit_gen_exp "
                 "block_err_exp block_gen_exp\n")


def stream_filename(p, num_doped, W, index):
    """results_circular, BPF:535."""
    return "SC_LDPC_%d_%d_L%d_M%d_DOP%d_BP_Stream_SW%d_Random_BLER_%d.dat" % (p.dv, p.dc, p.L, p.cns_pos, num_doped, W, index)


def stream_row(eps, c):
    """results_circular's row (BPF:547-560) from the eight counters (order of engine.STREAM_COUNTERS)."""
    ne, be, ee, bee, gb, gbl, gbe, gble = (int(x) for x in c[:8])
    return "%f %e %e %e %e %d %d %d %d %d %d %d %d\n" % (eps, ne / gb, be / gbl, ee / gbe, bee / gble,
                                                          ne, gb, be, gbl, ee, gbe, bee, gble)


def run_streaming(index, W, doped, opts):
    """main_streaming: per ε point, decode positions until num_blocks_err_exp >= max_blocks_err or
    num_blocks_generated_exp >= max_blocks (Def_MaxNumberBlocksError / Def_MaxNumberBlocksSim, BPF:41-42, 2033).
    The reference runs ONE stream; here `--streams` independent streams (× ranks) advance in lock step, `--chunk`
    positions per launch, and their counters are summed — the stop rule is applied to the sums after every chunk.
    opts.runs: every chunk is traced and fed to an engine.StreamRuns (with --rng glibc: the rows that count); rank 0 pickles one
    dict per ε point into <stream file>.runs.pkl, the .dat is what it is without the switch."""
    g0 = DEFAULTS["bp_lim_iter"]["grid"]
    N = opts.N if opts.N else 1000
    L = opts.L if opts.L else 50
    p = E.make_params(opts.dv, opts.dc, L, N)
    grid = GridSpec(opts.eps_ini if opts.eps_ini is not None else g0.eps_ini,
                    opts.eps_delta if opts.eps_delta is not None else g0.eps_delta,
                    opts.num_points if opts.num_points else g0.num_points, 0, 0)
    dist, rank, world = _dist()
    device = E.local_device()
    os.makedirs(opts.outdir, exist_ok=True)
    path = os.path.join(opts.outdir, stream_filename(p, len(doped), W, index))
    want_runs, nbins = bool(getattr(opts, "runs", False)), getattr(opts, "nbins", None)
    nbins = 256 if nbins is None else nbins
    runs_out = []

    def keep_runs(eps, sr, streams):
        """The point's statistics, summed over the ranks by one all-reduce, as the dict of the pickle."""
        parts = [sr.hist.reshape(-1), sr.sums, sr.open_hist().reshape(-1)] + ([sr.phase.reshape(-1)] if sr.phase is not None else [])
        flat = torch.cat(parts)
        if dist is not None:
            dist.all_reduce(flat)
        flat = flat.cpu().numpy()
        h, o = 4 * nbins, 4 * nbins + 8
        runs_out.append(dict(eps=eps, nbins=nbins, doped=tuple(int(d) for d in doped), period=sr.period, streams=streams,
                             hist=flat[:h].reshape(4, nbins).copy(), sums=flat[h:o].copy(),
                             phase=flat[o + 2 * nbins:].reshape(sr.period, 3).copy() if sr.phase is not None else None,
                             open_hist=flat[o:o + 2 * nbins].reshape(2, nbins).copy()))
        if rank == 0:
            with open(path + ".runs.pkl", "wb") as f:
                pickle.dump(runs_out, f)

    if getattr(opts, "rng", "philox") == "glibc":
        # The reference's own experiment, row for row: ONE stream, ONE srandom(seed), the points back to back with random()
        # carried over, every point stopped at the very position at which main_streaming stops (BPF:2033).
        if world > 1:
            raise SystemExit("--rng glibc replays the reference's one sequential random() stream: run it as a single process")
        run = E.GlibcStreamRun(p, opts.seed, W, doped, device=device)

        def tripped(c):
            return c[3] >= opts.max_blocks_err or c[7] >= opts.max_blocks

        for sim in range(grid.num_points):
            eps = grid.eps(sim)
            run.new_point(eps)
            sr = E.StreamRuns(p, 1, doped, nbins, device=device) if want_runs else None
            while True:
                rows = run.run(opts.chunk, stop=tripped)
                if want_runs:                           # the rows that count: up to the position at which the reference stops
                    sr.update(torch.from_numpy(rows.astype(np.int32)[None]).to(device).contiguous())
                if tripped(rows[-1, 2:]):
                    break
            tot = rows[-1, 2:]
            with open(path, "w" if sim == 0 else "a") as f:
                if sim == 0:
                    f.write(STREAM_HEADER)
                f.write(stream_row(eps, tot))
            if not opts.quiet:
                print("%f %e %e %e %e" % (eps, tot[0] / tot[4], tot[1] / tot[5], tot[2] / tot[6], tot[3] / tot[7]), flush=True)
            if want_runs:
                keep_runs(eps, sr, 1)
        return 0
    for sim in range(grid.num_points):
        eps = grid.eps(sim)
        st = E.Streams(p, opts.streams, opts.seed, eps, W, doped,
                       stream0=(sim * world + rank) * opts.streams, device=device)
        sr = E.StreamRuns(p, opts.streams, doped, nbins, device=device) if want_runs else None
        while True:
            if want_runs:
                cnt, tr = st.run(opts.chunk, trace=True)
                sr.update(tr, cnt)
            else:
                cnt, _ = st.run(opts.chunk)
            # (column 9 = positions generated; negative = the stream was marked unusable, include/scldpc.h)
            tot = torch.cat([cnt[:, :8].sum(dim=0), (cnt[:, 9] < 0).sum().reshape(1)])
            if dist is not None:
                dist.all_reduce(tot)                    # the only exchange: nine int64 per chunk
            tot = tot.cpu().numpy()
            if tot[8] > 0:                              # every rank sees the same sum and leaves together
                raise SystemExit("sw: %d stream(s) marked unusable by the generation kernel (a ranking bucket overflowed)" % tot[8])
            tot = tot[:8]
            if tot[3] >= opts.max_blocks_err or tot[7] >= opts.max_blocks:
                break
        if rank == 0:
            with open(path, "w" if sim == 0 else "a") as f:
                if sim == 0:
                    f.write(STREAM_HEADER)
                f.write(stream_row(eps, tot))
            if not opts.quiet:
                print("%f %e %e %e %e" % (eps, tot[0] / tot[4], tot[1] / tot[5], tot[2] / tot[6], tot[3] / tot[7]), flush=True)
        if want_runs:
            keep_runs(eps, sr, opts.streams * world)
    return 0


def streaming(argv=None):
    ap = argparse.ArgumentParser(prog="sw", description="doped SC-LDPC streaming window decoder (CIRCULAR build)")
    ap.add_argument("INDEX", type=int)
    ap.add_argument("W", type=int)
    ap.add_argument("NUM_DOPED", type=int)
    ap.add_argument("DOPED", nargs="*", type=int)
    ap.add_argument("--dv", type=int, default=4)
    ap.add_argument("--dc", type=int, default=8)
    ap.add_argument("--L", type=int, default=0, help="circular buffer length Def_L")
    ap.add_argument("--N", type=int, default=0)
    ap.add_argument("--eps-ini", type=float, default=None)
    ap.add_argument("--eps-delta", type=float, default=None)
    ap.add_argument("--num-points", type=int, default=0)
    ap.add_argument("--max-blocks-err", type=int, default=1000, help="Def_MaxNumberBlocksError (BPF:41)")
    ap.add_argument("--max-blocks", type=int, default=1000000, help="Def_MaxNumberBlocksSim (BPF:42)")
    ap.add_argument("--streams", type=int, default=512, help="independent streams per rank (--rng philox)")
    ap.add_argument("--rng", choices=("philox", "glibc"), default="philox",
                    help="glibc: the reference's own experiment — one stream drawn from srandom(--seed) exactly as "
                         "main_streaming draws it (BPF:1942-1945), reproduced row for row; single process")
    ap.add_argument("--chunk", type=int, default=64, help="positions per stream and launch")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--runs", action="store_true",
                    help="also write <stream file>.runs.pkl, a pickled list with one dict per ε point {eps, nbins, doped, period, "
                         "streams, hist, sums, phase, open_hist}: runs and events of failed positions, gaps between events, time "
                         "to first failure and the block error rate by offset in the doping period (engine.StreamRuns; "
                         "include/scldpc_runs.h); the .dat is unchanged")
    ap.add_argument("--nbins", type=int, default=None, help="--runs: bins per histogram, the last takes everything beyond (256)")
    ap.add_argument("--outdir", default=".")
    ap.add_argument("--quiet", action="store_true")
    opts = ap.parse_args(argv)
    if opts.nbins is not None and not opts.runs:
        raise SystemExit("--nbins sizes the histograms of --runs")
    if opts.runs and opts.nbins is not None and not 2 <= opts.nbins <= E.RUNS_MAX_BINS:
        raise SystemExit("--nbins: 2 <= nbins <= %d" % E.RUNS_MAX_BINS)
    if opts.seed is None:
        opts.seed = int((time.time() % 1) * 1e6)
    if len(opts.DOPED) < opts.NUM_DOPED:
        raise SystemExit("NUM_DOPED=%d but only %d positions given" % (opts.NUM_DOPED, len(opts.DOPED)))
    joined = E.init_distributed()
    rc = run_streaming(opts.INDEX, opts.W, opts.DOPED[:opts.NUM_DOPED], opts)
    if joined:
        import torch.distributed as dist
        dist.destroy_process_group()
    return rc


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "sw":
        sys.exit(streaming(sys.argv[2:]))
    if len(sys.argv) >= 2 and sys.argv[1] == "bp_thresholds":
        sys.exit(bp_thresholds(sys.argv[2:]))
    if len(sys.argv) >= 2 and sys.argv[1] == "bp_curves":
        sys.exit(bp_curves(sys.argv[2:]))
    if len(sys.argv) < 2 or sys.argv[1] not in DEFAULTS:
        raise SystemExit("usage: python -m fl_scaling_sc_ldpc_amd.bp_decoding {bp_lim_iter|sw_lim_iter|bp_traj|sw|bp_thresholds|bp_curves} ARGS…")
    sys.exit(main(sys.argv[1], sys.argv[2:]))
