"""Thin host layer over the C-ABI: device buffers (torch, plumbing only) + kernel launches.

Everything that computes runs inside libscldpc_hip.so; this module only owns memory and streams.
Reference routines replaced (see include/scldpc.h for line citations): generate_code /
channel_doped (sampling), decodeBP / decodeBP_SW (decoding), plr_computation / willIstop (run
accumulation).
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import (CodeParams, MAX_CAPS, NCOUNTERS, NRUN, NPEELRUN, COUNTER_NAMES, RUN_NAMES, PEELRUN_NAMES, ScldpcError,  # noqa: F401
                   SS_MAX_BINS, SS_POS_SIZES, RUNS_MAX_L, RUNS_MAX_BINS, RUNS_MAX_PERIOD, RUNS_CARRY, EPS_MAX_POINTS, THRESH_NCOLS, THRESH_MAX,
                   THRESH_NAMES, VNT_NCOLS, VNT_MAX_POINTS, VNT_NONE, VNT_NAMES, check, lib)


def make_params(dv=4, dc=8, L=50, N=1000):
    """(dv, dc, L, N) as in BASELINE.json: N = VNs per position (Def_VNsPos, Python's M);
    cns_pos = N*dv/dc (Def_M)."""
    if (N * dv) % dc:
        raise ValueError(f"N*dv must be divisible by dc (N={N}, dv={dv}, dc={dc})")
    return CodeParams(dv, dc, L, N * dv // dc, N)


def _stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


WS_SAMPLE, WS_FULL_BP, WS_SW_BP, WS_PEEL_SWEEP, WS_PEEL_PICK = range(5)      # SCLDPC_WS_*


def _uninit(shape, dtype, device):
    """Every kernel output and workspace of this module is allocated here, uninitialised: the kernels define every element the
    header's "Buffers" paragraph lists and rely on no earlier content.  (The one seam the buffer-contract tests replace.)"""
    return torch.empty(shape, dtype=dtype, device=device)


def _zeroed(shape, dtype, device):
    """The trajectory rows of the full_bp* wrappers: the kernels write rows [0, min(iterations, rows_cap)) of a trial and leave
    the rest alone; every wrapper hands the rest back as zeros."""
    return _uninit(shape, dtype, device).zero_()


def _workspace(op, p, ntrials, device, arg0=0, arg1=0):
    """(device pointer, bytes) of a caller-owned workspace for one call, or (None, 0) when the ensemble needs none.
    A fresh torch buffer per call: the caching allocator hands memory back only to the stream that used it, so calls
    on different streams never share scratch (the library itself allocates nothing)."""
    nbytes = lib().scldpc_workspace_bytes(op, C.byref(p), int(ntrials), int(arg0), int(arg1))
    if nbytes < 0:
        check(int(nbytes))
    if nbytes == 0:
        return None, 0, None
    buf = _uninit(int(nbytes), dtype=torch.uint8, device=device)
    return buf.data_ptr(), int(nbytes), buf


def _require_gpu():
    if not torch.cuda.is_available():
        raise ScldpcError("no HIP device visible: the decoders run only on the GPU (no CPU fallback)")


# ------------------------------------------------------------------------------------------------
# sampling
# ------------------------------------------------------------------------------------------------
def sample_glibc_trials(p, seeds, eps, doped=()):
    """Self-contained trials exactly as the reference draws them after `inizio_sim(); srandom(seed)`.
    Returns host arrays vn_adj int32 [T,n,dv], chan_bits uint32 [T,nw]."""
    seeds = np.asarray(seeds, dtype=np.uint32).reshape(-1)
    T = seeds.size
    vn_adj = np.empty((T, p.n, p.dv), dtype=np.int32)
    chan = np.empty((T, p.nw), dtype=np.uint32)
    darr, dptr = _lib.doped_array(doped)
    for t in range(T):
        check(lib().scldpc_sample_glibc_host(C.byref(p), int(seeds[t]), float(eps), darr.size, dptr,
                                             vn_adj[t].ctypes.data, chan[t].ctypes.data))
    return vn_adj, chan


class GlibcRun:
    """One reference run: a single srandom(seed), frames drawn back to back with perm_code and the
    random() stream carried over (main_terminated, BPF:2057-2131)."""

    def __init__(self, p, seed):
        self.p = p
        nbytes = lib().scldpc_glibc_state_bytes(C.byref(p))
        if nbytes < 0:
            check(int(nbytes))
        self._state = np.zeros(nbytes, dtype=np.uint8)
        check(lib().scldpc_glibc_state_init(C.byref(p), int(seed) & 0xFFFFFFFF, self._state.ctypes.data))

    def new_point(self):
        """inizio_sim(): perm_code := identity at the start of every ε point (BPF:308-311)."""
        check(lib().scldpc_glibc_state_reset_perm(C.byref(self.p), self._state.ctypes.data))

    def snapshot(self):
        return self._state.copy()

    def restore(self, snap):
        self._state[:] = snap

    def next_frames(self, nframes, eps, doped=()):
        p = self.p
        vn_adj = np.empty((nframes, p.n, p.dv), dtype=np.int32)
        chan = np.empty((nframes, p.nw), dtype=np.uint32)
        darr, dptr = _lib.doped_array(doped)
        check(lib().scldpc_sample_glibc_next_host(C.byref(p), self._state.ctypes.data, float(eps), darr.size, dptr,
                                                  nframes, vn_adj.ctypes.data, chan.ctypes.data))
        return vn_adj, chan


def to_device(vn_adj, chan, device="cuda:0"):
    _require_gpu()
    vn_adj = np.ascontiguousarray(vn_adj)
    if vn_adj.dtype != np.int16:
        vn_adj = vn_adj.astype(np.int32, copy=False)
    d_adj = torch.from_numpy(vn_adj).to(device)
    d_ch = torch.from_numpy(np.ascontiguousarray(chan).view(np.int32)).to(device)
    return d_adj, d_ch


def _is_adj16(d_adj):
    """int16 tensors carry the compact position-local adjacency (uint16 bit patterns)."""
    return d_adj.dtype == torch.int16


ENSEMBLES = {"olmos": 0, "tail_biting": 1, "protograph": 2}      # SCLDPC_ENS_*


def sample_philox(p, seed, trial0, ntrials, eps, doped=(), device="cuda:0", out=None, adj16=False, ensemble="olmos"):
    """Throughput-mode sampling on the device (counter-based; see scldpc_sample_philox_device).
    adj16=True: compact adjacency, int16 tensor [T,n,dv] holding uint16 position-local CN ids (Olmos chain only).
    ensemble: "olmos" (generate_code / sc_ldpc.gen_slots), "tail_biting" or "protograph" (global CN ids)."""
    _require_gpu()
    if out is None:
        d_adj = _uninit((ntrials, p.n, p.dv), dtype=torch.int16 if adj16 else torch.int32, device=device)
        d_ch = _uninit((ntrials, p.nw), dtype=torch.int32, device=device)
    else:
        d_adj, d_ch = out
    darr, dptr = _lib.doped_array(doped)
    if ensemble != "olmos":
        if _is_adj16(d_adj):
            raise ValueError("the tail-biting / protograph samplers write global CN ids: use adj16=False")
        check(lib().scldpc_sample_philox_ensemble_device(C.byref(p), ENSEMBLES[ensemble], int(seed), int(trial0),
                                                         int(ntrials), float(eps), darr.size, dptr, d_adj.data_ptr(),
                                                         d_ch.data_ptr(), _stream_ptr(d_adj.device)))
        return d_adj, d_ch
    fn = lib().scldpc_sample_philox_device_adj16 if _is_adj16(d_adj) else lib().scldpc_sample_philox_device
    ws, wsb, _keep = _workspace(WS_SAMPLE, p, ntrials, d_adj.device)
    check(fn(C.byref(p), int(seed), int(trial0), int(ntrials), float(eps), darr.size, dptr, d_adj.data_ptr(),
             d_ch.data_ptr(), ws, wsb, _stream_ptr(d_adj.device)))
    return d_adj, d_ch


def local_device():
    """This rank's GPU: cuda:LOCAL_RANK, as torch.distributed.run numbers the processes of a node.  In the rehearsal mode of
    the tests (SCLDPC_DIST_BACKEND set to something other than nccl) ranks may share a GPU: LOCAL_RANK wraps around."""
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("SCLDPC_DIST_BACKEND", "nccl") != "nccl":
        local %= max(1, torch.cuda.device_count())
    return torch.device("cuda", local)


def init_distributed():
    """Under torch.distributed.run (WORLD_SIZE > 1) join the job: one process per GPU, RCCL (backend "nccl") over xGMI.
    Returns True when this call created the process group (the caller then destroys it).  SCLDPC_DIST_BACKEND=gloo is the
    tests' rehearsal of the multi-rank drivers on a box with fewer GPUs than ranks."""
    import torch.distributed as dist
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1 or dist.is_initialized():
        return False
    _require_gpu()
    dev = local_device()
    torch.cuda.set_device(dev)
    backend = os.environ.get("SCLDPC_DIST_BACKEND", "nccl")
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=dev)
    else:
        dist.init_process_group(backend)
    return True


def gather_frames(dist, part, sizes, dim=0, shape=None, dtype=torch.int32, device=None):
    """The frames of one round from every rank, in frame order: rank r holds sizes[r] entries of `part` along `dim`; every rank
    pads to max(sizes) with zeros, all-gathers, and gets the concatenation of each rank's first sizes[r] entries, contiguous.
    A rank without frames may pass None with the shape (its entry at `dim` is ignored), dtype and device its part would have had.
    With one rank, or dist None, `part` itself comes back."""
    if dist is None or len(sizes) == 1:
        return part
    shape = list(part.shape if part is not None else shape)
    shape[dim] = max(sizes)
    pad = torch.zeros(shape, dtype=part.dtype if part is not None else dtype, device=part.device if part is not None else device)
    if part is not None:
        pad.narrow(dim, 0, part.shape[dim]).copy_(part)
    got = [_uninit(pad.shape, pad.dtype, pad.device) for _ in sizes]
    dist.all_gather(got, pad)
    return torch.cat([g.narrow(dim, 0, s) for g, s in zip(got, sizes)], dim=dim).contiguous()


def cn16_supported(p):
    """The (4,8) chain with N <= 2048 and fewer than 65535 VNs: the second-generation sampler + the 4-bits-per-CN decoder take it."""
    return bool(lib().scldpc_sample_philox_cn16_supported(C.byref(p))) and bool(lib().scldpc_full_bp_cn16_supported(C.byref(p)))


def _sample_philox_tables(fn, p, seed, trial0, ntrials, eps, doped, device, out, want_cn=True):
    """The one body of sample_philox_cn16 / sample_philox_sock16 / sample_philox_deg_sock16 / sample_philox_wide_sock16: both tables and the channel from the
    second-generation sampler."""
    _require_gpu()
    if out is None:
        d_adj = _uninit((ntrials, p.n, p.dv), dtype=torch.int16, device=device)
        d_cn = _uninit((ntrials, p.nk, p.dc), dtype=torch.int16, device=device) if want_cn else None
        d_ch = _uninit((ntrials, p.nw), dtype=torch.int32, device=device)
    else:
        d_adj, d_cn, d_ch = out
    darr, dptr = _lib.doped_array(doped)
    check(fn(C.byref(p), int(seed), int(trial0), int(ntrials), float(eps), darr.size, dptr, d_adj.data_ptr(),
             d_cn.data_ptr() if d_cn is not None else None, d_ch.data_ptr(), _stream_ptr(d_adj.device)))
    return d_adj, d_cn, d_ch


def sample_philox_cn16(p, seed, trial0, ntrials, eps, doped=(), device="cuda:0", out=None, want_cn=True):
    """scldpc_sample_philox_device_cn16: (vn_adj16 int16 [T,n,4], cn_adj16 int16 [T,nk,8] | None, chan int32 [T,nw]);
    the first and the last are bit for bit sample_philox(..., adj16=True)'s; cn_adj16 holds the VNs of every CN as
    uint16 bit patterns (0xFFFF: none), in unspecified order."""
    return _sample_philox_tables(lib().scldpc_sample_philox_device_cn16, p, seed, trial0, ntrials, eps, doped, device, out, want_cn)


def sw_ring_supported(p, W):
    """Whether the window-state-in-LDS decoder (sw_ring.hip) takes the square window W on this ensemble."""
    return bool(lib().scldpc_sw_bp_ring_supported(C.byref(p), int(W)))


def sw_ring_deg_supported(p, W):
    """Whether scldpc_sw_bp_ring_device_deg takes the square window W on this ensemble: the pairs (3,6), (4,8) and (5,10)."""
    return bool(lib().scldpc_sw_bp_ring_deg_supported(C.byref(p), int(W)))


def swc_ring_supported(p, W):
    """Whether scldpc_swc_bp_ring_device takes the classical window W on this ensemble: the pairs (3,6), (4,8) and (5,10)."""
    return bool(lib().scldpc_swc_bp_ring_supported(C.byref(p), int(W)))


def sock16_supported(p):
    """The (4,8) chain with N <= 2048: the second-generation sampler emits the ring window decoder's CN -> socket table."""
    return bool(lib().scldpc_sample_philox_sock16_supported(C.byref(p)))


def sample_philox_sock16(p, seed, trial0, ntrials, eps, doped=(), device="cuda:0", out=None):
    """scldpc_sample_philox_device_sock16: (vn_adj16 int16 [T,n,4], cn_sock16 int16 [T,nk,8], chan int32 [T,nw]); the first
    and the last are bit for bit sample_philox(..., adj16=True)'s, cn_sock16 is cn_sockets(p, vn_adj16) as a set per CN."""
    return _sample_philox_tables(lib().scldpc_sample_philox_device_sock16, p, seed, trial0, ntrials, eps, doped, device, out)


def deg_sock16_supported(p):
    """The pairs (3,6) and (5,10) with at most 8192 sockets per CN position: the second-generation sampler of these pairs
    (sampler_v2_deg.hip) takes the ensemble.  Needs no device."""
    return bool(lib().scldpc_sample_philox_deg_sock16_supported(C.byref(p)))


def sample_philox_deg_sock16(p, seed, trial0, ntrials, eps, doped=(), device="cuda:0", out=None):
    """scldpc_sample_philox_device_deg_sock16: (vn_adj16 int16 [T,n,dv], cn_sock16 int16 [T,nk,dc], chan int32 [T,nw]); the first
    and the last are bit for bit sample_philox(..., adj16=True)'s, cn_sock16 is cn_sockets(p, vn_adj16) as a set per CN.
    out = (vn_adj16, None, chan): no table."""
    return _sample_philox_tables(lib().scldpc_sample_philox_device_deg_sock16, p, seed, trial0, ntrials, eps, doped, device, out)


def wide_sock16_supported(p):
    """The pairs (3,6), (4,8) and (5,10) with more than 8192 and at most 20480 sockets per CN position: the wide second-generation
    sampler (sampler_v2_wide.hip) takes the ensemble.  Needs no device."""
    return bool(lib().scldpc_sample_philox_wide_sock16_supported(C.byref(p)))


def sample_philox_wide_sock16(p, seed, trial0, ntrials, eps, doped=(), device="cuda:0", out=None):
    """scldpc_sample_philox_device_wide_sock16: (vn_adj16 int16 [T,n,dv], cn_sock16 int16 [T,nk,dc], chan int32 [T,nw]); the first
    and the last are bit for bit sample_philox(..., adj16=True)'s, cn_sock16 is cn_sockets(p, vn_adj16) as a set per CN.
    out = (vn_adj16, None, chan): no table."""
    return _sample_philox_tables(lib().scldpc_sample_philox_device_wide_sock16, p, seed, trial0, ntrials, eps, doped, device, out)


def sample_philox_sock_supported(p):
    """Whether the first-generation sampler writes the CN -> socket table with the code on this ensemble (sample_philox_sock)."""
    return bool(lib().scldpc_sample_philox_adj16_sock_supported(C.byref(p)))


def sample_philox_sock(p, seed, trial0, ntrials, eps, doped=(), device="cuda:0", out=None):
    """scldpc_sample_philox_device_adj16_sock: (vn_adj16 int16 [T,n,dv], cn_sock16 int16 [T,nk,dc], chan int32 [T,nw]); the first
    and the last are bit for bit sample_philox(..., adj16=True)'s, cn_sock16 is cn_sockets(p, vn_adj16) as a set per CN — from
    the sampler's own launch, for every ensemble sample_philox takes with 16-bit sockets."""
    _require_gpu()
    if out is None:
        d_adj = _uninit((ntrials, p.n, p.dv), dtype=torch.int16, device=device)
        d_cn = _uninit((ntrials, p.nk, p.dc), dtype=torch.int16, device=device)
        d_ch = _uninit((ntrials, p.nw), dtype=torch.int32, device=device)
    else:
        d_adj, d_cn, d_ch = out
    darr, dptr = _lib.doped_array(doped)
    ws, wsb, _keep = _workspace(WS_SAMPLE, p, ntrials, d_adj.device)
    check(lib().scldpc_sample_philox_device_adj16_sock(C.byref(p), int(seed), int(trial0), int(ntrials), float(eps), darr.size, dptr,
                                                       d_adj.data_ptr(), d_cn.data_ptr(), d_ch.data_ptr(), ws, wsb,
                                                       _stream_ptr(d_adj.device)))
    return d_adj, d_cn, d_ch


def ens_sock16_supported(p, ensemble):
    """Whether sample_philox_ens_sock16 takes this ensemble ("tail_biting" | "protograph"; "olmos" never: its rows are
    position-local already) — scldpc_sample_philox_ensemble_adj16_sock_supported; on False lib().scldpc_last_error() names the
    limit.  Needs no device."""
    return bool(lib().scldpc_sample_philox_ensemble_adj16_sock_supported(C.byref(p), ENSEMBLES[ensemble]))


def sample_philox_ens_sock16(p, ensemble, seed, trial0, ntrials, eps, doped=(), device="cuda:0", out=None):
    """scldpc_sample_philox_ensemble_device_adj16_sock: (vn_adj16 int16 [T,n,dv], cn_sock16 int16 [T,nk,dc], chan int32 [T,nw])
    of the tail-biting or protograph ensemble.  chan is bit for bit sample_philox(..., ensemble=ensemble)'s, vn_adj16 holds its
    rows as position-local ids (edge i of VN position q in CN position (q + i) mod L, protograph: q + i), cn_sock16 the sockets
    dv * t + i of every CN (0xFFFF: none)."""
    _require_gpu()
    if out is None:
        d_adj = _uninit((ntrials, p.n, p.dv), dtype=torch.int16, device=device)
        d_cn = _uninit((ntrials, p.nk, p.dc), dtype=torch.int16, device=device)
        d_ch = _uninit((ntrials, p.nw), dtype=torch.int32, device=device)
    else:
        d_adj, d_cn, d_ch = out
    darr, dptr = _lib.doped_array(doped)
    check(lib().scldpc_sample_philox_ensemble_device_adj16_sock(C.byref(p), ENSEMBLES[ensemble], int(seed), int(trial0), int(ntrials),
                                                                float(eps), darr.size, dptr, d_adj.data_ptr(), d_cn.data_ptr(),
                                                                d_ch.data_ptr(), _stream_ptr(d_adj.device)))
    return d_adj, d_cn, d_ch


def uncoupled_supported(p):
    """Whether sample_philox_uncoupled takes p = CodeParams(dv, dc, 1, cns_pos, M): L = 1, dv <= 8, at most 8192 sockets and
    dv <= cns_pos (scldpc_sample_philox_uncoupled_supported; on False lib().scldpc_last_error() names the limit).  Needs no
    device."""
    return bool(lib().scldpc_sample_philox_uncoupled_supported(C.byref(p)))


def sample_philox_uncoupled(p, seed, trial0, ntrials, eps, max_attempts, device="cuda:0", out=None):
    """scldpc_sample_philox_uncoupled_device: (vn_adj int32 [T,M,dv], chan int32 [T,nw], attempts int32 [T]) of the uncoupled
    (dv, dc) ensemble with its repeat rejection (ldpc.gen_slots), redrawn on the device: attempts[t] candidates were drawn for
    trial trial0 + t (0: none accepted within max_attempts, negative: the ranking gave up; rows and words are zeros then — the
    caller decides what that means, nothing is raised here)."""
    _require_gpu()
    if out is None:
        d_adj = _uninit((ntrials, p.n, p.dv), dtype=torch.int32, device=device)
        d_ch = _uninit((ntrials, p.nw), dtype=torch.int32, device=device)
        d_att = _uninit((ntrials,), dtype=torch.int32, device=device)
    else:
        d_adj, d_ch, d_att = out
    check(lib().scldpc_sample_philox_uncoupled_device(C.byref(p), int(seed), int(trial0), int(ntrials), float(eps),
                                                      int(max_attempts), d_adj.data_ptr(), d_ch.data_ptr(), d_att.data_ptr(),
                                                      _stream_ptr(d_adj.device)))
    return d_adj, d_ch, d_att


def uncoupled_wide_supported(p):
    """Whether sample_philox_uncoupled_wide takes p = CodeParams(dv, dc, 1, cns_pos, M): L = 1, dv <= 8, at most 32768 sockets
    and dv <= cns_pos (scldpc_sample_philox_uncoupled_wide_supported; on False lib().scldpc_last_error() names the limit).
    Needs no device."""
    return bool(lib().scldpc_sample_philox_uncoupled_wide_supported(C.byref(p)))


def sample_philox_uncoupled_wide(p, seed, trial0, ntrials, eps, max_attempts, device="cuda:0", out=None):
    """scldpc_sample_philox_uncoupled_wide_device: sample_philox_uncoupled's three outputs — bit for bit where both take the
    shape — up to 32768 sockets (include/scldpc_uncoupled_wide.h).  attempts[t]: 0 none accepted within max_attempts, negative:
    a part of the keys outgrew its room; rows and words are zeros then, and nothing is raised here."""
    _require_gpu()
    if out is None:
        d_adj = _uninit((ntrials, p.n, p.dv), dtype=torch.int32, device=device)
        d_ch = _uninit((ntrials, p.nw), dtype=torch.int32, device=device)
        d_att = _uninit((ntrials,), dtype=torch.int32, device=device)
    else:
        d_adj, d_ch, d_att = out
    check(lib().scldpc_sample_philox_uncoupled_wide_device(C.byref(p), int(seed), int(trial0), int(ntrials), float(eps),
                                                           int(max_attempts), d_adj.data_ptr(), d_ch.data_ptr(), d_att.data_ptr(),
                                                           _stream_ptr(d_adj.device)))
    return d_adj, d_ch, d_att


def cn_adj_from_vn_adj(p, adj16):
    """Host: the CN -> VN table (uint16 [.., nk, dc] as int16 bit patterns: the VNs of every CN in ascending order,
    0xFFFF where a chain-end CN has fewer than dc) from the position-local VN -> CN table — for feeding host-sampled
    codes (glibc replay, fixtures) to full_bp_fixpoint_cn16, and for checking the device table."""
    a = np.ascontiguousarray(adj16).view(np.uint16).astype(np.int64).reshape(-1, p.n, p.dv)
    if p.n >= 0xFFFF:
        raise ValueError("the CN -> VN table holds 16-bit VN indices: n must be below 65535")
    T = a.shape[0]
    out = np.full((T, p.nk, p.dc), 0xFFFF, dtype=np.uint16)
    pos = np.arange(p.n) // p.vns_pos
    for k in range(T):
        cn = ((pos[:, None] + np.arange(p.dv)[None, :]) * p.cns_pos + a[k]).ravel()      # CN of every edge, VN-major
        vn = np.repeat(np.arange(p.n), p.dv)
        order = np.lexsort((vn, cn))
        cn_s, vn_s = cn[order], vn[order]
        start = np.searchsorted(cn_s, np.arange(p.nk))
        slot = np.arange(cn_s.size) - start[cn_s]
        if slot.max() >= p.dc:
            raise ValueError("a CN has more than dc neighbours")
        out[k, cn_s, slot] = vn_s
    return out.view(np.int16)


def adj16_to_global(p, adj16):
    """Host: uint16 position-local ids [.., n, dv] → the int32 global CN ids of the reference's VNdegree."""
    a = np.ascontiguousarray(adj16).view(np.uint16).astype(np.int32)
    pos = (np.arange(p.n, dtype=np.int32) // p.vns_pos)[:, None] + np.arange(p.dv, dtype=np.int32)[None, :]
    return a + pos * p.cns_pos


def global_to_adj16(p, adj):
    """Host: int32 global CN ids → uint16 position-local ids (as int16 bit patterns for torch)."""
    adj = np.asarray(adj, dtype=np.int32)
    pos = (np.arange(p.n, dtype=np.int32) // p.vns_pos)[:, None] + np.arange(p.dv, dtype=np.int32)[None, :]
    loc = adj - pos * p.cns_pos
    if loc.min() < 0 or loc.max() >= p.cns_pos:
        raise ValueError("adjacency is not position-structured (edge i of a VN must land in CN position pos+i)")
    return loc.astype(np.uint16).view(np.int16)


# ------------------------------------------------------------------------------------------------
# decoding
# ------------------------------------------------------------------------------------------------
def _full_bp(p, d_adj, d_cn, d_chan, call, counters=None, want_erased=False, rows_cap=0, new_rows=None, ncaps=0):
    """The one body of the full_bp* wrappers.  Checks the tensors against p — d_cn None: the first-generation decoders, which
    take the 4-byte VN -> CN table too; else the 2-byte tables of the 4-bit decoders — allocates counters [T,8] ([ncaps,T,8]),
    rows [T,rows_cap,3] (by new_rows; None: _uninit, looked up at call time) and erased [T,nw] where asked, and calls
    call(head, counters, rows, erased, stream) with head = (p, T, the tables, the channel) and every tensor as its pointer."""
    _require_gpu()
    T = d_adj.shape[0]
    assert d_adj.is_cuda and d_adj.dtype in ((torch.int32, torch.int16) if d_cn is None else (torch.int16,)) and d_adj.is_contiguous()
    assert d_cn is None or (d_cn.is_cuda and d_cn.dtype == torch.int16 and d_cn.is_contiguous())
    assert d_chan.is_cuda and d_chan.dtype == torch.int32 and d_chan.is_contiguous()
    assert tuple(d_adj.shape[1:]) == (p.n, p.dv) and tuple(d_chan.shape) == (T, p.nw)
    assert d_cn is None or tuple(d_cn.shape) == (T, p.nk, p.dc)
    dev = d_adj.device
    shape = (ncaps, T, NCOUNTERS) if ncaps else (T, NCOUNTERS)
    if counters is None:
        counters = _uninit(shape, dtype=torch.int32, device=dev)
    assert not ncaps or (counters.is_contiguous() and counters.dtype == torch.int32 and tuple(counters.shape) == shape)
    rows = (new_rows or _uninit)((T, rows_cap, 3), dtype=torch.int32, device=dev) if rows_cap > 0 else None
    erased = _uninit((T, p.nw), dtype=torch.int32, device=dev) if want_erased else None
    head = (C.byref(p), T, d_adj.data_ptr()) + ((d_cn.data_ptr(),) if d_cn is not None else ()) + (d_chan.data_ptr(),)
    check(call(head, counters.data_ptr(), rows.data_ptr() if rows is not None else None,
               erased.data_ptr() if erased is not None else None, _stream_ptr(dev)))
    return {"counters": counters, "rows": rows, "erased": erased}


def full_bp(p, d_adj, d_chan, max_it=0, is_term=True, rows_cap=0, want_erased=False, counters=None):
    """decodeBP for a batch resident on the device.  Returns dict of device tensors:
    counters int32 [T,8] (+ rows int32 [T,rows_cap,3], erased int32 [T,nw] when asked).  Rows beyond a trial's iteration count
    (counters[t, 5]) are zeros, here and in every full_bp* wrapper that takes rows_cap."""
    fn = lib().scldpc_full_bp_device_adj16 if _is_adj16(d_adj) else lib().scldpc_full_bp_device

    def call(head, cnt, rows, erased, stream):
        ws, wsb, _keep = _workspace(WS_FULL_BP, p, head[1], d_adj.device, 1 if rows is not None else 0)
        return fn(*head, int(max_it), 1 if is_term else 0, cnt, rows, int(rows_cap), erased, ws, wsb, stream)
    return _full_bp(p, d_adj, None, d_chan, call, counters, want_erased, rows_cap, _zeroed)


def full_bp_fixpoint(p, d_adj, d_chan, is_term=True, want_erased=False, counters=None):
    """What unlimited decodeBP converges to, without its iteration count (scldpc_full_bp_fixpoint_device): counters as
    full_bp's except column 5 (barrier rounds of the kernel) — for runs with no iteration cap and no trajectory rows."""
    fn = lib().scldpc_full_bp_fixpoint_device_adj16 if _is_adj16(d_adj) else lib().scldpc_full_bp_fixpoint_device

    def call(head, cnt, rows, erased, stream):
        ws, wsb, _keep = _workspace(WS_FULL_BP, p, head[1], d_adj.device, 0)
        return fn(*head, 1 if is_term else 0, cnt, erased, ws, wsb, stream)
    return _full_bp(p, d_adj, None, d_chan, call, counters, want_erased)


def full_bp_sock16_supported(p):
    """The (4,8) chain with at most 65536 CNs per trial, any number of VNs: sampler (CN -> socket table) + 4-bits-per-CN decoder."""
    return bool(lib().scldpc_sample_philox_sock16_supported(C.byref(p))) and bool(lib().scldpc_full_bp_sock16_supported(C.byref(p)))


def full_bp_fixpoint_cn16(p, d_adj16, d_cn16, d_chan, is_term=True, want_erased=False, counters=None, sockets=False):
    """scldpc_full_bp_fixpoint_device_cn16: full_bp_fixpoint's counters from the VN -> CN and CN -> VN tables
    (sockets=True: the CN -> socket table, scldpc_full_bp_fixpoint_device_sock16)."""
    fn = lib().scldpc_full_bp_fixpoint_device_sock16 if sockets else lib().scldpc_full_bp_fixpoint_device_cn16
    return _full_bp(p, d_adj16, d_cn16, d_chan, lambda head, cnt, rows, erased, stream:
                    fn(*head, 1 if is_term else 0, cnt, erased, stream), counters, want_erased)


def _level_call(fn, max_it, is_term, rows_cap):
    """The call of a level-synchronous 4-bit decoder for _full_bp: the trajectory symbols take the rows too."""
    if rows_cap > 0:
        return lambda head, cnt, rows, erased, stream: fn(*head, int(max_it), 1 if is_term else 0, cnt, rows, int(rows_cap), erased, stream)
    return lambda head, cnt, rows, erased, stream: fn(*head, int(max_it), 1 if is_term else 0, cnt, erased, stream)


def full_bp_cn16(p, d_adj16, d_cn16, d_chan, max_it=0, is_term=True, want_erased=False, counters=None, sockets=False,
                 rows_cap=0):
    """scldpc_full_bp_device_cn16: decodeBP with its iterations (count, cap, stop tests) from the VN -> CN and CN -> VN
    tables — every counter of full_bp; rows_cap > 0: the trajectory build's rows too (scldpc_full_bp_traj_device_cn16);
    sockets=True: the _sock16 symbols."""
    L = lib()
    if rows_cap > 0:
        fn = L.scldpc_full_bp_traj_device_sock16 if sockets else L.scldpc_full_bp_traj_device_cn16
    else:
        fn = L.scldpc_full_bp_device_sock16 if sockets else L.scldpc_full_bp_device_cn16
    return _full_bp(p, d_adj16, d_cn16, d_chan, _level_call(fn, max_it, is_term, rows_cap), counters, want_erased, rows_cap,
                    _zeroed)                        # zeros, as full_bp's


def full_bp_wide_supported(p):
    """The (4,8) chain whose 4-bit state leaves at least 1024 32-bit queue entries per queue in one CU's LDS (e.g. L = 50,
    N = 5000; L = 100, N = 2000): scldpc_full_bp_device_wide takes it."""
    return bool(lib().scldpc_full_bp_wide_supported(C.byref(p)))


def full_bp_wide(p, d_adj16, d_cn_sock, d_chan, max_it=0, is_term=True, rows_cap=0, want_erased=False, counters=None):
    """scldpc_full_bp_device_wide / scldpc_full_bp_traj_device_wide (rows_cap > 0): full_bp_cn16(sockets=True) for trials of
    more than 65536 CNs — the same dict: counters int32 [T,8], rows int32 [T,rows_cap,3] | None, erased int32 [T,nw] | None.
    d_cn_sock: cn_sockets(p, d_adj16) or sample_philox_sock16's table."""
    fn = lib().scldpc_full_bp_traj_device_wide if rows_cap > 0 else lib().scldpc_full_bp_device_wide
    return _full_bp(p, d_adj16, d_cn_sock, d_chan, _level_call(fn, max_it, is_term, rows_cap), counters, want_erased, rows_cap,
                    _zeroed)                        # zeros, as full_bp's


def full_bp_deg_supported(p, wide=False):
    """The (3,6), (4,8) and (5,10) chains the _deg forms of the 4-bit decoder take: at most 65536 CNs per trial, or (wide=True)
    a state that leaves 1024 32-bit queue entries per queue in one CU's LDS."""
    fn = lib().scldpc_full_bp_deg_wide_supported if wide else lib().scldpc_full_bp_deg_supported
    return bool(fn(C.byref(p)))


def full_bp_deg(p, d_adj16, d_cn_sock, d_chan, max_it=0, is_term=True, rows_cap=0, want_erased=False, counters=None, wide=False):
    """scldpc_full_bp_device_deg / scldpc_full_bp_traj_device_deg (rows_cap > 0), wide=True: their _wide forms — full_bp's
    counters, rows and erased bitmap for the pairs (3,6), (4,8), (5,10) from the 2-byte VN -> CN table and
    cn_sockets(p, d_adj16); the same dict as full_bp_cn16 / full_bp_wide."""
    name = "scldpc_full_bp_%sdevice_deg%s" % ("traj_" if rows_cap > 0 else "", "_wide" if wide else "")
    return _full_bp(p, d_adj16, d_cn_sock, d_chan, _level_call(getattr(lib(), name), max_it, is_term, rows_cap), counters,
                    want_erased, rows_cap, _zeroed)                 # zeros, as full_bp's


def full_bp_fixpoint_deg(p, d_adj16, d_cn_sock, d_chan, is_term=True, want_erased=False, counters=None):
    """scldpc_full_bp_fixpoint_device_deg: full_bp_fixpoint's counters for the same pairs and tables (narrow shapes only)."""
    fn = lib().scldpc_full_bp_fixpoint_device_deg
    return _full_bp(p, d_adj16, d_cn_sock, d_chan, lambda head, cnt, rows, erased, stream:
                    fn(*head, 1 if is_term else 0, cnt, erased, stream), counters, want_erased)


def check_caps(caps):
    """The cap list of full_bp_caps_cn16 as a tuple, with the C side's rules: 1 .. MAX_CAPS strictly increasing caps >= 1."""
    caps = tuple(int(k) for k in caps)
    if not 1 <= len(caps) <= MAX_CAPS:
        raise ValueError("takes 1 .. %d caps, got %d" % (MAX_CAPS, len(caps)))
    if caps[0] < 1 or any(b <= a for a, b in zip(caps, caps[1:])):
        raise ValueError("caps must be strictly increasing and >= 1: %r" % (caps,))
    return caps


def full_bp_caps_cn16(p, d_adj16, d_cn16, d_chan, caps, is_term=True, counters=None, sockets=False):
    """scldpc_full_bp_caps_device_cn16 (sockets=True: _sock16): one decode, the counters of several iteration caps —
    counters [K, T, 8], where counters[k] == full_bp_cn16(..., max_it=caps[k])["counters"] on all eight columns."""
    fn = lib().scldpc_full_bp_caps_device_sock16 if sockets else lib().scldpc_full_bp_caps_device_cn16
    return _full_bp_caps(fn, p, d_adj16, d_cn16, d_chan, caps, is_term, counters)


def _full_bp_caps(fn, p, d_adj16, d_cn, d_chan, caps, is_term, counters):
    """The call of a caps entry point (they share their arguments) through _full_bp: counters [K, T, 8]."""
    caps = check_caps(caps)
    arr = (C.c_int32 * len(caps))(*caps)
    return _full_bp(p, d_adj16, d_cn, d_chan, lambda head, cnt, rows, erased, stream:
                    fn(*head, len(caps), arr, 1 if is_term else 0, cnt, stream), counters, ncaps=len(caps))["counters"]


def full_bp_caps_wide(p, d_adj16, d_cn_sock, d_chan, caps, is_term=True, counters=None):
    """scldpc_full_bp_caps_device_wide: full_bp_caps_cn16(sockets=True) for trials of more than 65536 CNs — counters [K, T, 8],
    where counters[k] == full_bp_wide(..., max_it=caps[k])["counters"] on all eight columns.  The shapes of full_bp_wide."""
    return _full_bp_caps(lib().scldpc_full_bp_caps_device_wide, p, d_adj16, d_cn_sock, d_chan, caps, is_term, counters)


def full_bp_caps_deg(p, d_adj16, d_cn_sock, d_chan, caps, is_term=True, counters=None, wide=False):
    """scldpc_full_bp_caps_device_deg (wide=True: _deg_wide): one decode, the counters of several iteration caps for the pairs
    (3,6), (4,8), (5,10) — counters [K, T, 8], where counters[k] == full_bp_deg(..., max_it=caps[k], wide=wide)["counters"] on
    all eight columns.  The shapes of full_bp_deg_supported(p, wide)."""
    fn = lib().scldpc_full_bp_caps_device_deg_wide if wide else lib().scldpc_full_bp_caps_device_deg
    return _full_bp_caps(fn, p, d_adj16, d_cn_sock, d_chan, caps, is_term, counters)


def cn_sockets(p, d_adj16, out=None):
    """scldpc_cn_sockets_device: the CN -> socket table int16 [T, nk, dc] (uint16 bit patterns) of a 2-byte VN -> CN table."""
    _require_gpu()
    T = d_adj16.shape[0]
    assert d_adj16.is_cuda and d_adj16.dtype == torch.int16 and d_adj16.is_contiguous()
    if out is None:
        out = _uninit((T, p.nk, p.dc), dtype=torch.int16, device=d_adj16.device)
    check(lib().scldpc_cn_sockets_device(C.byref(p), T, d_adj16.data_ptr(), out.data_ptr(), _stream_ptr(d_adj16.device)))
    return out


def sw_bp(p, d_adj, d_chan, W, max_it, init_it=0, want_erased=False, counters=None, classical=False, ring=None, d_cn_sock=None,
          deg=False):
    """decodeBP_SW for a batch resident on the device: square window (BPW:628-912) or, with classical=True, the
    classical window kept in BPF:627-897 (init_it unused).  ring: None = use the window-state-in-LDS kernel (sw_ring.hip)
    whenever it takes the ensemble (square window, 2-byte tables; the CN -> socket table is built on the fly unless
    d_cn_sock is given), False = the whole-chain kernel, True = insist on the ring kernel.  deg=True: the ring decision and the
    launch go through scldpc_sw_bp_ring_deg_supported / scldpc_sw_bp_ring_device_deg, which take the pairs (3,6) and (5,10) too.
    classical=True takes the ring kernel (scldpc_swc_bp_ring_device, all three pairs) only with ring=True."""
    _require_gpu()
    T = d_adj.shape[0]
    use_ring = ring
    if classical:
        use_ring = bool(ring)
        if use_ring and not _is_adj16(d_adj):
            raise ScldpcError("the classical ring window kernel takes 2-byte tables only")
    elif ring is None or ring:
        supported = lib().scldpc_sw_bp_ring_deg_supported if deg else lib().scldpc_sw_bp_ring_supported
        ok = (not classical) and _is_adj16(d_adj) and bool(supported(C.byref(p), int(W)))
        if ring and not ok:
            raise ScldpcError("the ring window kernel takes the square window on 2-byte tables of the (3,6), (4,8) and (5,10) "
                              "chains only" if deg else
                              "the ring window kernel takes the square window on 2-byte tables of the (4,8) chain only")
        use_ring = ok
    assert d_adj.is_cuda and d_adj.dtype in (torch.int32, torch.int16) and d_adj.is_contiguous()
    assert d_chan.is_cuda and d_chan.dtype == torch.int32 and d_chan.is_contiguous()
    dev = d_adj.device
    if counters is None:
        counters = _uninit((T, NCOUNTERS), dtype=torch.int32, device=dev)
    erased = _uninit((T, p.nw), dtype=torch.int32, device=dev) if want_erased else None
    head = (C.byref(p), T, d_adj.data_ptr())
    tail = (counters.data_ptr(), erased.data_ptr() if erased is not None else None)
    if use_ring and classical:
        fn = lib().scldpc_swc_bp_ring_device
        check(fn(C.byref(p), 0, None, None, None, int(W), int(max_it), None, None, None))    # a refusal names its limit before any device work
        if d_cn_sock is None:
            d_cn_sock = cn_sockets(p, d_adj)
        check(fn(*head, d_cn_sock.data_ptr(), d_chan.data_ptr(), int(W), int(max_it), *tail, _stream_ptr(dev)))
        return {"counters": counters, "erased": erased}
    if use_ring:
        if d_cn_sock is None:
            d_cn_sock = cn_sockets(p, d_adj)
        fn = lib().scldpc_sw_bp_ring_device_deg if deg else lib().scldpc_sw_bp_ring_device
        check(fn(*head, d_cn_sock.data_ptr(), d_chan.data_ptr(), int(W), int(max_it), int(init_it), *tail, _stream_ptr(dev)))
        return {"counters": counters, "erased": erased}
    ws, wsb, _keep = _workspace(WS_SW_BP, p, T, dev, int(W))
    if classical:
        fn = lib().scldpc_swc_bp_device_adj16 if _is_adj16(d_adj) else lib().scldpc_swc_bp_device
        check(fn(*head, d_chan.data_ptr(), int(W), int(max_it), *tail, ws, wsb, _stream_ptr(dev)))
    else:
        fn = lib().scldpc_sw_bp_device_adj16 if _is_adj16(d_adj) else lib().scldpc_sw_bp_device
        check(fn(*head, d_chan.data_ptr(), int(W), int(max_it), int(init_it), *tail, ws, wsb, _stream_ptr(dev)))
    return {"counters": counters, "erased": erased}


def accumulate_run(d_counters, d_run, stop_frame_err=0):
    """plr_computation + willIstop in trial order; d_run int64 [NRUN] accumulated in place."""
    check(lib().scldpc_accumulate_run_device(d_counters.shape[0], d_counters.data_ptr(), int(stop_frame_err),
                                             d_run.data_ptr(), _stream_ptr(d_counters.device)))
    return d_run


def accumulate_peel(d_out, d_run, max_fuckups=0):
    """simulate_sc_ldpc's ordered bookkeeping + stop rule (PD:668-699) over a batch of peel_sweep rows; d_run int64
    [NPEELRUN] (order of _lib.PEELRUN_NAMES) accumulated in place."""
    check(lib().scldpc_accumulate_peel_device(d_out.shape[0], d_out.data_ptr(), int(max_fuckups), d_run.data_ptr(),
                                              _stream_ptr(d_out.device)))
    return d_run


def clear_channel_range(p, d_ch, vn_lo, vn_hi):
    """Soft doping (PD:176-183): VNs vn_lo .. vn_hi-1 of every trial become known."""
    check(lib().scldpc_clear_channel_range_device(C.byref(p), d_ch.shape[0], int(vn_lo), int(vn_hi), d_ch.data_ptr(),
                                                  _stream_ptr(d_ch.device)))
    return d_ch


def new_run(device="cuda:0"):
    return torch.zeros(NRUN, dtype=torch.int64, device=device)


def unpack_bits(words, n):
    """uint32/int32 words [.., nw] → uint8 [.., n] (host)."""
    w = np.ascontiguousarray(words).view(np.uint32)
    bits = np.unpackbits(w.view(np.uint8).reshape(*w.shape[:-1], -1), axis=-1, bitorder="little")
    return bits[..., :n]


def pack_bits(bits):
    """uint8 [.., n] → uint32 words [.., nw] (host)."""
    bits = np.asarray(bits, dtype=np.uint8)
    n = bits.shape[-1]
    pad = (-n) % 32
    if pad:
        bits = np.concatenate([bits, np.zeros(bits.shape[:-1] + (pad,), np.uint8)], axis=-1)
    return np.packbits(bits, axis=-1, bitorder="little").view(np.uint32)


# ------------------------------------------------------------------------------------------------
# Python peeling path (PD)
# ------------------------------------------------------------------------------------------------
def peel_sweep(p, d_adj, d_chan, total_size, sweep_start=0, lost_lo=0, lost_hi=None, want_lost=False):
    """One trial of simulate_sc_ldpc's loop body per batch entry (PD:650-691).  Returns dict with
    out int32 [T,8] ([0] #lost, [1] #lost_exp, [2] #blocks_failed_exp, [5] rounds, [7] #erased) and `lost` bits."""
    _require_gpu()
    T = d_adj.shape[0]
    assert d_adj.is_cuda and d_adj.dtype in (torch.int32, torch.int16) and d_adj.is_contiguous()
    assert d_chan.is_cuda and d_chan.dtype == torch.int32 and d_chan.is_contiguous()
    dev = d_adj.device
    out = _uninit((T, 8), dtype=torch.int32, device=dev)
    lost = _uninit((T, p.nw), dtype=torch.int32, device=dev) if want_lost else None
    fn = lib().scldpc_peel_sweep_device_adj16 if _is_adj16(d_adj) else lib().scldpc_peel_sweep_device
    ws, wsb, _keep = _workspace(WS_PEEL_SWEEP, p, T, dev, 1 if _is_adj16(d_adj) else 0)
    check(fn(C.byref(p), T, d_adj.data_ptr(), d_chan.data_ptr(), int(total_size), int(sweep_start), int(lost_lo),
             int(total_size if lost_hi is None else lost_hi), out.data_ptr(),
             lost.data_ptr() if lost is not None else None, ws, wsb, _stream_ptr(dev)))
    return {"out": out, "lost": lost}


def erasure_threshold(eps):
    """The samplers' threshold of an erasure probability: a VN is erased iff its 31-bit draw is below ceil(eps * RAND_MAX)
    (erasure_threshold, csrc/sampler_common.h).  Two eps with one threshold are one channel."""
    return int(math.ceil(float(eps) * 2147483647.0))


def channel_levels(p, seed, trial0, ntrials, es_desc, doped=(), device="cuda:0", out=None):
    """The channel of trials trial0 .. trial0 + ntrials - 1 at every point of es_desc (strictly decreasing thresholds, at most
    _lib.EPS_MAX_POINTS points) as levels: uint8 [T, n], lev[j] = the number of points at which VN j is erased, so that
    pack(lev > k) is the channel sample_philox writes for es_desc[k] on the same (seed, trial, doped)
    (scldpc_channel_levels_device)."""
    _require_gpu()
    eps = np.ascontiguousarray(es_desc, dtype=np.float64).reshape(-1)
    d_lev = _uninit((ntrials, p.n), dtype=torch.uint8, device=device) if out is None else out
    darr, dptr = _lib.doped_array(doped)
    check(lib().scldpc_channel_levels_device(C.byref(p), int(seed), int(trial0), int(ntrials), eps.size,
                                             eps.ctypes.data if eps.size else None, darr.size, dptr, d_lev.data_ptr(),
                                             _stream_ptr(d_lev.device)))
    return d_lev


def _eps_workspace_bytes(query, p, ntrials, adj16):
    nbytes = getattr(lib(), query)(C.byref(p), int(ntrials), 1 if adj16 else 0)
    if nbytes < 0:
        check(int(nbytes))
    return int(nbytes)


def _ptr(t):
    """The device pointer of an optional tensor."""
    return t.data_ptr() if t is not None else None


def _walk_call(entry, p, d_adj):
    """The front of the four wrappers over one sampled code per frame (peel_sweep_eps, full_bp_eps, frame_threshold,
    vn_threshold): the adjacency's contract and the workspace query, which also refuses the shape before anything is allocated.
    Returns (T, device, call); call(*args) allocates the workspace, after the wrapper's outputs, and launches
    scldpc_<entry>_device or its _adj16 twin with the entry's own arguments between the adjacency and the workspace."""
    assert d_adj.is_cuda and d_adj.dtype in (torch.int32, torch.int16) and d_adj.is_contiguous()
    assert tuple(d_adj.shape[1:]) == (p.n, p.dv)
    T, dev, adj16 = d_adj.shape[0], d_adj.device, _is_adj16(d_adj)
    nbytes = _eps_workspace_bytes("scldpc_%s_workspace_query" % entry, p, T, adj16)
    fn = getattr(lib(), "scldpc_%s_device%s" % (entry, "_adj16" if adj16 else ""))

    def call(*args):
        ws = _uninit(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        check(fn(C.byref(p), T, d_adj.data_ptr(), *args, _ptr(ws), nbytes, _stream_ptr(dev)))
    return T, dev, call


def peel_sweep_eps_workspace_bytes(p, ntrials, adj16):
    """Bytes of workspace peel_sweep_eps needs for ntrials trials (0: the CN words stay in LDS); ScldpcError for a shape the
    entry refuses.  Needs no device."""
    return _eps_workspace_bytes("scldpc_peel_sweep_eps_workspace_query", p, ntrials, adj16)


def peel_sweep_eps(p, d_adj, d_levels, npoints, total_size, lost_lo=0, lost_hi=None, want_lost=False):
    """peel_sweep with sweep_start = 0 at every point of a descending eps grid in one launch: the code d_adj once, the channel
    as levels (channel_levels), stage k peeling on from the residual of stage k - 1.  Returns dict with out int32 [K, T, 8] —
    out[k] is peel_sweep's block for the channel of point k ([0] #lost, [1] #lost_exp, [2] #blocks_failed_exp, [7] #erased;
    [5] the rounds of stage k, [6] its re-scans after a queue overflow) — and `lost` int32 [K, T, nw] or None (scldpc_peel_sweep_eps_device)."""
    _require_gpu()
    (T, dev, call), K = _walk_call("peel_sweep_eps", p, d_adj), int(npoints)
    assert d_levels.is_cuda and d_levels.dtype == torch.uint8 and d_levels.is_contiguous() and d_levels.shape == (T, p.n)
    out = _uninit((max(K, 0), T, 8), dtype=torch.int32, device=dev)
    lost = _uninit((max(K, 0), T, p.nw), dtype=torch.int32, device=dev) if want_lost else None
    call(d_levels.data_ptr(), K, int(total_size), int(lost_lo), int(total_size if lost_hi is None else lost_hi), out.data_ptr(),
         _ptr(lost))
    return {"out": out, "lost": lost}


def full_bp_eps_workspace_bytes(p, ntrials, adj16):
    """Bytes of workspace full_bp_eps needs for ntrials trials (0: the CN words stay in LDS); ScldpcError for a shape the
    entry refuses.  Needs no device."""
    return _eps_workspace_bytes("scldpc_full_bp_eps_workspace_query", p, ntrials, adj16)


def full_bp_eps(p, d_adj, d_levels, npoints, is_term=True, want_erased=False, counters=None):
    """full_bp_fixpoint at every point of a descending eps grid in one launch: the code d_adj once, the channel as levels
    (channel_levels), stage k peeling on from the residual of stage k - 1.  Returns dict with counters int32 [K, T, 8] —
    counters[k] is full_bp_fixpoint's block for the channel of point k except column 5 (the peeling rounds of stage k), what
    accumulate_run reads — and `erased` int32 [K, T, nw] or None (scldpc_full_bp_eps_device).  counters: a contiguous int32
    [K, T, 8] tensor to write into."""
    _require_gpu()
    (T, dev, call), K = _walk_call("full_bp_eps", p, d_adj), int(npoints)
    assert d_levels.is_cuda and d_levels.dtype == torch.uint8 and d_levels.is_contiguous() and d_levels.shape == (T, p.n)
    shape = (max(K, 0), T, NCOUNTERS)
    if counters is None:
        counters = _uninit(shape, dtype=torch.int32, device=dev)
    assert counters.is_cuda and counters.is_contiguous() and counters.dtype == torch.int32 and tuple(counters.shape) == shape
    erased = _uninit((max(K, 0), T, p.nw), dtype=torch.int32, device=dev) if want_erased else None
    call(d_levels.data_ptr(), K, 1 if is_term else 0, counters.data_ptr(), _ptr(erased))
    return {"counters": counters, "erased": erased}


def channel_keys(p, seed, trial0, ntrials, doped=(), device="cuda:0", out=None):
    """The 31-bit channel keys of trials trial0 .. trial0 + ntrials - 1: int32 [T, n] holding uint32 bit patterns, key[j] = the
    draw >> 1 the samplers compare with the erasure threshold, -1 (0xFFFFFFFF, never erased) in a doped position — so that
    pack(key.view(uint32) < erasure_threshold(eps)) is the channel sample_philox writes at eps on the same (seed, trial, doped),
    for every eps (scldpc_channel_keys_device)."""
    _require_gpu()
    d_keys = _uninit((ntrials, p.n), dtype=torch.int32, device=device) if out is None else out
    darr, dptr = _lib.doped_array(doped)
    check(lib().scldpc_channel_keys_device(C.byref(p), int(seed), int(trial0), int(ntrials), darr.size, dptr, d_keys.data_ptr(),
                                           _stream_ptr(d_keys.device)))
    return d_keys


def frame_threshold_workspace_bytes(p, ntrials, adj16):
    """Bytes of workspace frame_threshold needs for ntrials frames (0: the CN words stay in LDS); ScldpcError for a shape the
    entry refuses.  Needs no device."""
    return _eps_workspace_bytes("scldpc_frame_threshold_workspace_query", p, ntrials, adj16)


def frame_threshold(p, d_adj, d_keys, t_lo, t_hi, is_term=True, want_bits=False, rows=None):
    """The critical erasure threshold of every frame under unlimited full BP: VN j of frame f is erased at threshold t iff
    d_keys[f, j] (as uint32; channel_keys, or any keys) < t, and T*(f) is the least t in (t_lo, t_hi] at which full_bp without a
    cap leaves a residual, found by bisection inside the residual of the decode at t_hi.  Returns dict with rows int32 [T, 8] —
    _lib.THRESH_NAMES: [0] T* (status 0), t_lo (status 2) or -1 (status 1); [1] status 0: t_lo < T* <= t_hi, 1: decodes at t_hi,
    2: fails at t_lo; [2] the size of the critical residual, [3], [4] its first and last position; [5] stages, [6] re-scans;
    [7] #VNs erased at t_hi — and `bits` int32 [T, nw], the critical residual in the layout of `erased`, or None
    (scldpc_frame_threshold_device).  rows: a contiguous int32 [T, 8] tensor to write into."""
    _require_gpu()
    if not 0 <= int(t_lo) <= 0xFFFFFFFF or not 0 <= int(t_hi) <= 0xFFFFFFFF:
        raise ValueError("frame_threshold: the thresholds are unsigned 32-bit integers (got t_lo = %d, t_hi = %d)" % (t_lo, t_hi))
    T, dev, call = _walk_call("frame_threshold", p, d_adj)
    assert d_keys.is_cuda and d_keys.dtype == torch.int32 and d_keys.is_contiguous() and d_keys.shape == (T, p.n)
    shape = (T, _lib.THRESH_NCOLS)
    if rows is None:
        rows = _uninit(shape, dtype=torch.int32, device=dev)
    assert rows.is_cuda and rows.is_contiguous() and rows.dtype == torch.int32 and tuple(rows.shape) == shape
    bits = _uninit((T, p.nw), dtype=torch.int32, device=dev) if want_bits else None
    call(d_keys.data_ptr(), int(t_lo), int(t_hi), 1 if is_term else 0, rows.data_ptr(), _ptr(bits))
    return {"rows": rows, "bits": bits}


def vn_threshold_workspace_bytes(p, ntrials, adj16):
    """Bytes of workspace vn_threshold needs for ntrials frames (0: the CN words stay in LDS); ScldpcError for a shape the
    entry refuses.  Needs no device."""
    return _eps_workspace_bytes("scldpc_vn_threshold_workspace_query", p, ntrials, adj16)


def vn_threshold(p, d_adj, d_keys, t_lo, t_hi, grid=(), is_term=True, want_tau=False, rows=None):
    """The erasure threshold of every VN under unlimited full BP: tau(j) = the least t at which VN j is in the residual S(t) that
    full_bp without a cap leaves of {key < t}, walked down from the decode at t_hi with no rebuild of the CN words.  Returns dict
    with rows int32 [T, 8] — _lib.VNT_NAMES: [0] T* / t_lo / -1 and [1] the status, both frame_threshold's; [2] |S(t_hi)|; [3] the
    size of the critical residual; [4] steps = the distinct tau in (t_lo, t_hi]; [5] candidate scans, [6] re-scans; [7] #VNs
    erased at t_hi —, pos_thresh int32 [T, L] holding uint32 bit patterns (the least tau of the position, -1 = VNT_NONE where it
    never fails), counts int32 [T, len(grid)] or None (counts[k] = #{j : tau(j) <= grid[k]}, grid: ascending thresholds inside
    the window, at most _lib.VNT_MAX_POINTS) and tau int32 [T, n] (uint32 bit patterns; t_lo means "at or below t_lo") or None
    (scldpc_vn_threshold_device).  rows: a contiguous int32 [T, 8] tensor to write into."""
    _require_gpu()
    if not 0 <= int(t_lo) <= 0xFFFFFFFF or not 0 <= int(t_hi) <= 0xFFFFFFFF:
        raise ValueError("vn_threshold: the thresholds are unsigned 32-bit integers (got t_lo = %d, t_hi = %d)" % (t_lo, t_hi))
    g = [int(t) for t in grid]
    if any(not 0 <= t <= 0xFFFFFFFF for t in g):
        raise ValueError("vn_threshold: the grid's thresholds are unsigned 32-bit integers")
    garr = np.ascontiguousarray(g, dtype=np.uint32)
    (T, dev, call), K = _walk_call("vn_threshold", p, d_adj), garr.size
    assert d_keys.is_cuda and d_keys.dtype == torch.int32 and d_keys.is_contiguous() and d_keys.shape == (T, p.n)
    shape = (T, _lib.VNT_NCOLS)
    if rows is None:
        rows = _uninit(shape, dtype=torch.int32, device=dev)
    assert rows.is_cuda and rows.is_contiguous() and rows.dtype == torch.int32 and tuple(rows.shape) == shape
    pos = _uninit((T, p.L), dtype=torch.int32, device=dev)
    counts = _uninit((T, K), dtype=torch.int32, device=dev) if K else None
    tau = _uninit((T, p.n), dtype=torch.int32, device=dev) if want_tau else None
    call(d_keys.data_ptr(), int(t_lo), int(t_hi), 1 if is_term else 0, K, garr.ctypes.data if K else None, rows.data_ptr(),
         pos.data_ptr(), _ptr(counts), _ptr(tau))
    return {"rows": rows, "pos_thresh": pos, "counts": counts, "tau": tau}


def peel_sweep_sock16_supported(p):
    """The pairs (3,6), (4,8), (5,10) with 16-bit sockets and at most 65536 CNs per trial: peel_sweep_sock16 takes the ensemble
    (scldpc_peel_sweep_sock16_supported).  Needs no device."""
    return bool(lib().scldpc_peel_sweep_sock16_supported(C.byref(p)))


def _peel_sweep_tables(entry, p, d_adj16, d_cn_sock, d_chan, total_size, sweep_start, lost_lo, lost_hi, want_lost):
    """The one body of peel_sweep_sock16 / peel_sweep_sock16_wide."""
    _require_gpu()
    T = d_adj16.shape[0]
    assert d_adj16.is_cuda and d_adj16.dtype == torch.int16 and d_adj16.is_contiguous() and tuple(d_adj16.shape[1:]) == (p.n, p.dv)
    assert d_cn_sock.is_cuda and d_cn_sock.dtype == torch.int16 and d_cn_sock.is_contiguous() and tuple(d_cn_sock.shape) == (T, p.nk, p.dc)
    assert d_chan.is_cuda and d_chan.dtype == torch.int32 and d_chan.is_contiguous() and tuple(d_chan.shape) == (T, p.nw)
    dev = d_adj16.device
    out = _uninit((T, 8), dtype=torch.int32, device=dev)
    lost = _uninit((T, p.nw), dtype=torch.int32, device=dev) if want_lost else None
    check(getattr(lib(), entry)(C.byref(p), T, d_adj16.data_ptr(), d_cn_sock.data_ptr(), d_chan.data_ptr(),
                                 int(total_size), int(sweep_start), int(lost_lo),
                                 int(total_size if lost_hi is None else lost_hi), out.data_ptr(),
                                 lost.data_ptr() if lost is not None else None, _stream_ptr(dev)))
    return {"out": out, "lost": lost}


def _sweep_entry(ensemble, wide):
    """The entry of peel_sweep_sock16(_wide) for the tables of `ensemble`: a tail-biting code is a ring (the _tb entries), the
    Olmos and protograph codes are chains."""
    if ensemble not in ENSEMBLES:
        raise ValueError("ensemble must be one of %s" % (sorted(ENSEMBLES),))
    return "scldpc_peel_sweep_device_sock16" + ("_tb" if ensemble == "tail_biting" else "") + ("_wide" if wide else "")


def peel_sweep_tb_supported(p, wide=False):
    """Whether peel_sweep_sock16(..., ensemble="tail_biting") — wide: peel_sweep_sock16_wide — takes this ensemble as a ring:
    the chain's shape rule and L >= dv (scldpc_peel_sweep_tb_supported / _tb_wide_supported).  Needs no device."""
    fn = lib().scldpc_peel_sweep_tb_wide_supported if wide else lib().scldpc_peel_sweep_tb_supported
    return bool(fn(C.byref(p)))


def peel_sweep_sock16(p, d_adj16, d_cn_sock, d_chan, total_size, sweep_start=0, lost_lo=0, lost_hi=None, want_lost=False,
                      ensemble="olmos"):
    """scldpc_peel_sweep_device_sock16: peel_sweep from the 2-byte VN -> CN table and the CN -> socket table (cn_sockets(p,
    d_adj16) or a second-generation sampler's) with 4 bits of LDS per CN — the same dict, columns 0, 1, 2, 7 of `out` and the
    `lost` bits bit for bit; column 5 counts this kernel's rounds, column 6 its re-scans.  No workspace, no fallback: an
    ensemble it does not take raises.  ensemble: whose tables these are (sample_philox_ens_sock16) — "tail_biting" runs
    scldpc_peel_sweep_device_sock16_tb, "protograph" this entry."""
    return _peel_sweep_tables(_sweep_entry(ensemble, False), p, d_adj16, d_cn_sock, d_chan, total_size, sweep_start, lost_lo,
                              lost_hi, want_lost)


def peel_sweep_wide_supported(p):
    """The pairs (3,6), (4,8), (5,10) with 16-bit sockets whose 4-bit state leaves two queues of 1024 32-bit entries in one
    CU's LDS, any number of CNs per trial: peel_sweep_sock16_wide takes the ensemble (scldpc_peel_sweep_wide_supported,
    judged at sweep_start = 0).  Needs no device."""
    return bool(lib().scldpc_peel_sweep_wide_supported(C.byref(p)))


def peel_sweep_sock16_wide(p, d_adj16, d_cn_sock, d_chan, total_size, sweep_start=0, lost_lo=0, lost_hi=None, want_lost=False,
                           ensemble="olmos"):
    """scldpc_peel_sweep_device_sock16_wide: peel_sweep_sock16 with 32-bit queue entries and one 1024-thread workgroup per CU,
    for trials of more than 65536 CNs (and any smaller one) — the same arguments, the same dict.  No workspace, no fallback:
    an ensemble it does not take raises.  ensemble="tail_biting": scldpc_peel_sweep_device_sock16_tb_wide."""
    return _peel_sweep_tables(_sweep_entry(ensemble, True), p, d_adj16, d_cn_sock, d_chan, total_size, sweep_start,
                              lost_lo, lost_hi, want_lost)


def peel_pick(p, d_adj, d_chan, total_size, num_steps, mt_state=None, seed=0, trial0=0, want_r1=True, moments=None):
    """One trial of simulate_peeling_decoder_ldpc's loop body per batch entry (PD:750-785).
    mt_state: int32/uint32-as-int32 tensor [T,625] (CPython MT19937 state, updated in place) or None (Philox)."""
    _require_gpu()
    T = d_adj.shape[0]
    assert d_adj.is_cuda and d_adj.dtype in (torch.int32, torch.int16) and d_adj.is_contiguous()
    dev = d_adj.device
    out = _uninit((T, 4), dtype=torch.int32, device=dev)
    r1 = _uninit((T, num_steps + 1), dtype=torch.int32, device=dev) if want_r1 else None
    if mt_state is not None:
        assert mt_state.is_cuda and mt_state.dtype == torch.int32 and tuple(mt_state.shape) == (T, 625)
    fn = lib().scldpc_peel_pick_device_adj16 if _is_adj16(d_adj) else lib().scldpc_peel_pick_device
    ws, wsb, _keep = _workspace(WS_PEEL_PICK, p, T, dev, int(total_size), 1 if mt_state is not None else 0)
    check(fn(C.byref(p), T, d_adj.data_ptr(), d_chan.data_ptr(), int(total_size), int(num_steps),
             mt_state.data_ptr() if mt_state is not None else None, int(seed), int(trial0),
             r1.data_ptr() if r1 is not None else None, moments.data_ptr() if moments is not None else None,
             out.data_ptr(), ws, wsb, _stream_ptr(dev)))
    return {"out": out, "r1": r1, "moments": moments}


def peel_pick_deg_supported(p, total_size):
    """The pairs (3,6), (4,8), (5,10) with 2-byte rows, at most 4096 words of degree-1 bitmap and a ring of dv CN positions
    within the LDS: peel_pick_deg takes the ensemble at this total_size (scldpc_peel_pick_deg_supported; on False
    lib().scldpc_last_error() names the limit).  Needs no device."""
    return bool(lib().scldpc_peel_pick_deg_supported(C.byref(p), int(total_size)))


def peel_pick_deg(p, d_adj16, d_chan, total_size, num_steps, seed=0, trial0=0, want_r1=True):
    """scldpc_peel_pick_device_adj16_deg: peel_pick with Philox draws from the 2-byte rows of the pairs (3,6), (4,8), (5,10),
    the CN words built through an LDS ring and two trials stepped per wave — `out` and `r1` value for value peel_pick's.
    No fallback: a shape it does not take raises."""
    _require_gpu()
    T = d_adj16.shape[0]
    assert d_adj16.is_cuda and d_adj16.dtype == torch.int16 and d_adj16.is_contiguous() and tuple(d_adj16.shape[1:]) == (p.n, p.dv)
    assert d_chan.is_cuda and d_chan.dtype == torch.int32 and d_chan.is_contiguous() and tuple(d_chan.shape) == (T, p.nw)
    dev = d_adj16.device
    out = _uninit((T, 4), dtype=torch.int32, device=dev)
    r1 = _uninit((T, num_steps + 1), dtype=torch.int32, device=dev) if want_r1 else None
    nbytes = lib().scldpc_peel_pick_deg_workspace_bytes(C.byref(p), T, int(total_size))
    if nbytes < 0:
        check(int(nbytes))
    ws = _uninit(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
    check(lib().scldpc_peel_pick_device_adj16_deg(C.byref(p), T, d_adj16.data_ptr(), d_chan.data_ptr(), int(total_size),
                                                  int(num_steps), int(seed), int(trial0),
                                                  r1.data_ptr() if r1 is not None else None, out.data_ptr(), ws.data_ptr(),
                                                  int(nbytes), _stream_ptr(dev)))
    return {"out": out, "r1": r1}


def r1_moments(d_r1, moments=None):
    """(cnt, Σr1, Σr1²) per step over a batch of trajectories, accumulated into int64 [3, steps+1]."""
    T, ncols = d_r1.shape
    if moments is None:
        moments = torch.zeros((3, ncols), dtype=torch.int64, device=d_r1.device)
    check(lib().scldpc_r1_moments_device(T, ncols, d_r1.data_ptr(), moments.data_ptr(), _stream_ptr(d_r1.device)))
    return moments


def r1_gram_trial_splits(ntrials, k):
    """Over how many workgroups per 64 x 64 output tile r1_gram's launch splits `ntrials` trials at `k` steps
    (scldpc_r1_gram_trial_splits).  Needs no device."""
    n = lib().scldpc_r1_gram_trial_splits(int(ntrials), int(k))
    if n < 0:
        check(int(n))
    return int(n)


def r1_gram(d_r1, steps, gram=None):
    """scldpc_r1_gram_device: with x = d_r1[:, steps] and m = (x != 0), the exact integer Gram matrices (mᵀm, xᵀm, xᵀx) over
    the trials of the batch, accumulated into int64 [3, K, K] (zeros where `gram` is None).  d_r1: int32 [T, ncols] on the
    device, as peel_pick and peel_pick_deg write it; steps: any integer sequence or tensor of K <= 4096 column indices.
    A step outside [0, ncols) is never read out of bounds: the kernel clamps it and says so in its status word, which is
    read back here (one synchronisation) and raised as ScldpcError."""
    _require_gpu()
    assert d_r1.is_cuda and d_r1.dtype == torch.int32 and d_r1.dim() == 2 and d_r1.is_contiguous()
    T, ncols = d_r1.shape
    dev = d_r1.device
    d_steps = torch.as_tensor(steps).reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    K = int(d_steps.numel())
    if gram is None:
        gram = torch.zeros((3, K, K), dtype=torch.int64, device=dev)
    assert gram.is_cuda and gram.dtype == torch.int64 and tuple(gram.shape) == (3, K, K) and gram.is_contiguous()
    nbytes = lib().scldpc_r1_gram_workspace_bytes(T, K)
    if nbytes < 0:
        check(int(nbytes))
    ws = _uninit(int(nbytes), dtype=torch.uint8, device=dev)
    check(lib().scldpc_r1_gram_device(T, ncols, d_r1.data_ptr(), K, d_steps.data_ptr(), gram.data_ptr(), ws.data_ptr(),
                                      int(nbytes), _stream_ptr(dev)))
    if T > 0:
        status = int(ws[:4].view(torch.int32).item())
        if status:
            raise ScldpcError("r1_gram: a step lies outside [0, %d): the kernel clamped it (status %d) and `gram` holds the "
                              "sums of the clamped columns" % (ncols, status))
    return gram


def ss_spectrum_form(p):
    """Where ss_spectrum keeps its union-find state for ensemble p: 1 = in LDS, 2 = in its workspace
    (scldpc_ss_spectrum_form; SCLDPC_DEBUG_SS_FORCE_WORKSPACE=1 sends every shape to 2).  Needs no device."""
    form = lib().scldpc_ss_spectrum_form(C.byref(p))
    if form < 0:
        check(int(form))
    return int(form)


def ss_spectrum(p, d_adj, d_members, nbins, hist=None, pos_hist=None, want_trial=False):
    """scldpc_ss_spectrum_device: the connected components (through every shared CN, pd_oracle.components) of the VNs whose
    bits are set in d_members int32 [T, nw] — a sweep decoder's `lost`, full BP's `erased`, or any subset — one trial per
    row.  d_adj: int32 [T, n, dv] global CN ids (any ensemble) or int16 [T, n, dv] position-local ids (the chains' 2-byte rows).
    Accumulates into hist int64 [nbins] (hist[0] += trials without a member, hist[min(s, nbins - 1)] += 1 per component of s
    VNs) and pos_hist int64 [L, 8] ([q, min(s, 8) - 1] += 1, q the position of the component's lowest-index member), zeros
    where None; want_trial: also int32 [T, 4] = (components, largest size, members, members in components of more than 2).
    Returns {"hist", "pos_hist", "trial"}.  A CN id outside [0, ncn) is skipped, never used as an index, and flagged in the
    status word, which is read back here (one synchronisation) and raised as RuntimeError."""
    _require_gpu()
    assert d_adj.is_cuda and d_adj.dtype in (torch.int32, torch.int16) and d_adj.is_contiguous() and tuple(d_adj.shape[1:]) == (p.n, p.dv)
    T = d_adj.shape[0]
    assert d_members.is_cuda and d_members.dtype == torch.int32 and d_members.is_contiguous() and tuple(d_members.shape) == (T, p.nw)
    dev = d_adj.device
    nbins = int(nbins)
    if hist is None:
        hist = torch.zeros((max(nbins, 0),), dtype=torch.int64, device=dev)
    if pos_hist is None:
        pos_hist = torch.zeros((p.L, _lib.SS_POS_SIZES), dtype=torch.int64, device=dev)
    assert hist.is_cuda and hist.dtype == torch.int64 and tuple(hist.shape) == (nbins,) and hist.is_contiguous()
    assert pos_hist.is_cuda and pos_hist.dtype == torch.int64 and tuple(pos_hist.shape) == (p.L, _lib.SS_POS_SIZES) and pos_hist.is_contiguous()
    nbytes = lib().scldpc_ss_spectrum_workspace_bytes(C.byref(p), T)
    if nbytes < 0:
        check(int(nbytes))
    ws = _uninit(int(nbytes), dtype=torch.uint8, device=dev)
    trial = _uninit((T, 4), dtype=torch.int32, device=dev) if want_trial else None
    check(lib().scldpc_ss_spectrum_device(C.byref(p), T, d_adj.data_ptr(), 1 if _is_adj16(d_adj) else 0, d_members.data_ptr(),
                                          nbins, hist.data_ptr(), pos_hist.data_ptr(),
                                          trial.data_ptr() if trial is not None else None, ws.data_ptr(), int(nbytes),
                                          _stream_ptr(dev)))
    if T > 0:
        status = int(ws[:4].view(torch.int32).item())
        if status & _lib.SS_BAD_CN:
            raise RuntimeError("ss_spectrum: a CN id lies outside [0, %d): the kernel skipped that edge (status %d, SS_BAD_CN) "
                               "and the sums hold the components without it" % (p.nk, status))
    return {"hist": hist, "pos_hist": pos_hist, "trial": trial}


def chain_runs(p, d_bits, acc=None, want_trial=False, want_fail_bits=False):
    """scldpc_chain_runs_device: the runs of failed positions of a batch of chain trials, one per row of d_bits int32 [T, nw]
    (a chain decoder's `erased`, a sweep decoder's `lost`).  A position fails where any of its vns_pos bits is set.
    Accumulates into acc["pos"] int64 [L, 4] (failed, set bits, first failing position, run starts), acc["run_hist"] int64
    [L + 1, 2] ([0, 0] trials without a failure; per run length: runs, runs that reach the end of the chain) and
    acc["fail_hist"] int64 [L + 1] (trials by their number of failing positions); zeros where acc is None or lacks the key.
    want_trial: also int32 [T, 4] = (failing positions, first failing position or L, runs, longest run); want_fail_bits: also
    the flags as int32 [T, ceil(L / 32)].  Returns {"pos", "run_hist", "fail_hist", "trial", "fail_bits"}.  Enqueue only."""
    _require_gpu()
    assert d_bits.is_cuda and d_bits.dtype == torch.int32 and d_bits.is_contiguous() and d_bits.dim() == 2 and d_bits.shape[1] == p.nw
    T, dev = d_bits.shape[0], d_bits.device
    acc = dict(acc) if acc is not None else {}
    out = {}
    for name, shape in (("pos", (p.L, 4)), ("run_hist", (p.L + 1, 2)), ("fail_hist", (p.L + 1,))):
        a = acc.get(name)
        if a is None:
            a = torch.zeros(shape, dtype=torch.int64, device=dev)
        assert a.is_cuda and a.dtype == torch.int64 and tuple(a.shape) == shape and a.is_contiguous()
        out[name] = a
    trial = _uninit((T, 4), dtype=torch.int32, device=dev) if want_trial else None
    fail_bits = _uninit((T, (p.L + 31) // 32), dtype=torch.int32, device=dev) if want_fail_bits else None
    check(lib().scldpc_chain_runs_device(C.byref(p), T, d_bits.data_ptr(), out["pos"].data_ptr(), out["run_hist"].data_ptr(),
                                         out["fail_hist"].data_ptr(), trial.data_ptr() if trial is not None else None,
                                         fail_bits.data_ptr() if fail_bits is not None else None, _stream_ptr(dev)))
    out["trial"], out["fail_bits"] = trial, fail_bits
    return out


class StreamRuns:
    """Runs, events, gaps and time to first failure of nstreams streaming-decoder streams (scldpc_stream_runs_device), fed with
    the trace rows of successive Streams.run(npos, trace=True) calls in order.  hist int64 [4, nbins] (runs, events, gaps
    between events, time to first failure; the last bin takes everything beyond), sums int64 [8], phase int64 [period, 3]
    (decided, failed, erased bits by offset in the doping period) and the per-stream carry int64 [nstreams, 8] live on the
    device; include/scldpc_runs.h defines every entry."""

    def __init__(self, p, nstreams, doped=(), nbins=256, device="cuda:0"):
        _require_gpu()
        self.p, self.n, self.doped, self.nbins = p, int(nstreams), tuple(int(d) for d in doped), int(nbins)
        self.period = self.doped[-1] + 1 if self.doped else 1
        darr, dptr = _lib.doped_array(self.doped)
        # the parameter checks, before any buffer exists (a refusal names its limit)
        check(lib().scldpc_stream_runs_device(C.byref(p), 0, 0, None, None, darr.size, dptr, self.nbins, None, None, None,
                                              C.c_void_p(8) if self.period <= _lib.RUNS_MAX_PERIOD else None, None))
        self.hist = torch.zeros((4, self.nbins), dtype=torch.int64, device=device)
        self.sums = torch.zeros((8,), dtype=torch.int64, device=device)
        self.phase = (torch.zeros((self.period, 3), dtype=torch.int64, device=device)
                      if self.period <= _lib.RUNS_MAX_PERIOD else None)
        self.carry = torch.zeros((self.n, _lib.RUNS_CARRY), dtype=torch.int64, device=device)

    def update(self, trace, counters=None):
        """Feed the next rows: trace int32 [nstreams, npos, 10]; counters int64 [nstreams, 10] (Streams.counters) lets the
        kernel skip the streams marked unusable.  Enqueue only."""
        assert trace.is_cuda and trace.dtype == torch.int32 and trace.is_contiguous() and trace.dim() == 3
        assert trace.shape[0] == self.n and trace.shape[2] == 10
        if counters is not None:
            assert counters.is_cuda and counters.dtype == torch.int64 and counters.is_contiguous() and tuple(counters.shape) == (self.n, 10)
        darr, dptr = _lib.doped_array(self.doped)
        check(lib().scldpc_stream_runs_device(C.byref(self.p), self.n, int(trace.shape[1]), trace.data_ptr(),
                                              counters.data_ptr() if counters is not None else None, darr.size, dptr,
                                              self.nbins, self.carry.data_ptr(), self.hist.data_ptr(), self.sums.data_ptr(),
                                              self.phase.data_ptr() if self.phase is not None else None,
                                              _stream_ptr(trace.device)))
        return self

    def open_hist(self):
        """int64 [2, nbins]: the runs (row 0) and events (row 1) still open in the carry, by their length so far (censored: they
        are in none of hist's rows)."""
        out = torch.zeros((2, self.nbins), dtype=torch.int64, device=self.carry.device)
        for row, col in ((0, 1), (1, 2)):
            v = self.carry[:, col]
            v = v[v > 0].clamp(max=self.nbins - 1)
            out[row].index_add_(0, v, torch.ones_like(v))
        return out


# ------------------------------------------------------------------------------------------------
# streaming mode (main_streaming, BPF:1934-2054)
# ------------------------------------------------------------------------------------------------
STREAM_COUNTERS = ("num_erasures", "num_blocks_err", "num_erasures_exp", "num_blocks_err_exp", "num_bits_generated",
                   "num_blocks_generated", "num_bits_generated_exp", "num_blocks_generated_exp", "positions", "generated")


def stream_supported(p, W):
    """True if the streaming kernels take ensemble p with window W (scldpc_stream_supported: dv = 3, 4 or 5, dc <= 15, at most
    65 536 sockets per position, 2 dv <= L <= 256, W + dv - 1 <= L/2, the window's state within the LDS); on False
    lib().scldpc_last_error() names the limit.  Streams, InputStreams and GlibcStreamRun raise on such an ensemble."""
    return bool(lib().scldpc_stream_supported(C.byref(p), int(W)))


class Streams:
    """nstreams independent doped SC-LDPC streams on the device, each a circular buffer of p.L positions."""

    def __init__(self, p, nstreams, seed, eps, W, doped=(), stream0=0, device="cuda:0"):
        _require_gpu()
        nbytes = lib().scldpc_stream_state_bytes(C.byref(p), int(W))
        if nbytes < 0:
            check(int(nbytes))
        self.p, self.n, self.seed, self.eps, self.W, self.stream0 = p, nstreams, seed, eps, W, stream0
        self.doped = tuple(doped)
        self.state = torch.zeros((nstreams, nbytes), dtype=torch.uint8, device=device)
        self.counters = torch.zeros((nstreams, 10), dtype=torch.int64, device=device)

    def run(self, npos, trace=False):
        """Decode npos further positions on every stream; returns (counters int64 [n,10], trace int32 [n,npos,10] | None)."""
        tr = _uninit((self.n, npos, 10), dtype=torch.int32, device=self.state.device) if trace else None
        darr, dptr = _lib.doped_array(self.doped)
        check(lib().scldpc_stream_run_device(C.byref(self.p), self.n, int(self.seed), int(self.stream0), float(self.eps),
                                             int(self.W), darr.size, dptr, int(npos), self.state.data_ptr(),
                                             self.counters.data_ptr(), tr.data_ptr() if tr is not None else None,
                                             _stream_ptr(self.state.device)))
        return self.counters, tr


def stream_glibc_inputs(p, seed, eps, doped, npos_gen):
    """Host: main_streaming's draws for the first npos_gen generated positions of one stream after srandom(seed)
    (scldpc_stream_glibc_inputs_host): (inter uint16 [npos_gen + dv - 1, S], chan uint32 [npos_gen, wpp])."""
    S, wpp = p.cns_pos * p.dc, (p.vns_pos + 31) // 32
    inter = np.empty((npos_gen + p.dv - 1, S), dtype=np.uint16)
    chan = np.empty((npos_gen, wpp), dtype=np.uint32)
    darr, dptr = _lib.doped_array(doped)
    check(lib().scldpc_stream_glibc_inputs_host(C.byref(p), int(seed) & 0xFFFFFFFF, float(eps), darr.size, dptr, int(npos_gen),
                                                inter.ctypes.data, chan.ctypes.data))
    return inter, chan


class GlibcStreamRun:
    """main_streaming on the reference's OWN stream (BPF:1934-2054): ONE srandom(seed) for the whole run (BPF:1942-1945),
    the ε points back to back with random() carried from point to point; the draws are replayed on the host piece by piece
    (scldpc_stream_glibc_next_host) and decoded on the device (scldpc_stream_run_device_inputs_at).  One stream, as the
    reference runs it."""

    def __init__(self, p, seed, W, doped=(), device="cuda:0"):
        _require_gpu()
        self.p, self.W, self.doped, self.device = p, int(W), tuple(doped), device
        nbytes = lib().scldpc_glibc_state_bytes(C.byref(p))
        if nbytes < 0:
            check(int(nbytes))
        self._host = np.zeros(nbytes, dtype=np.uint8)
        check(lib().scldpc_glibc_state_init(C.byref(p), int(seed) & 0xFFFFFFFF, self._host.ctypes.data))     # srandom(seed)
        self.S, self.wpp = p.cns_pos * p.dc, (p.vns_pos + 31) // 32
        self.st = None

    def new_point(self, eps):
        """inizio_sim (perm_code := identity, BPF:308-311) + a fresh buffer (initialize_arrays_circular, BPF:1998)."""
        check(lib().scldpc_glibc_state_reset_perm(C.byref(self.p), self._host.ctypes.data))
        self.eps, self.done = float(eps), 0
        self.st = Streams(self.p, 1, 0, 0.0, self.W, self.doped, device=self.device)

    def _draw(self, ninit, gpos0, npos):
        inter = np.empty((ninit + npos, self.S), dtype=np.uint16)
        chan = np.empty((max(npos, 1), self.wpp), dtype=np.uint32)
        darr, dptr = _lib.doped_array(self.doped)
        check(lib().scldpc_stream_glibc_next_host(C.byref(self.p), self._host.ctypes.data, self.eps, darr.size, dptr, int(ninit),
                                                  int(gpos0), int(npos), inter.ctypes.data, chan.ctypes.data))
        return inter, chan[:npos]

    def run(self, npos, stop=None):
        """Decode npos further positions.  Returns the trace rows int64 [k, 10] (position, value of decodeBP_SW_circular, the
        eight running counters) of the positions that count: all npos, or — with stop(counters) -> bool — up to and including
        the first position at which main_streaming's rule trips (BPF:2033); the host stream is then left exactly where the
        reference leaves it (it does not generate beyond that position), ready for the next point."""
        p, dv, half = self.p, self.p.dv, self.p.L // 2
        snap = self._host.copy()
        first = self.done == 0
        g0 = 0 if first else half + self.done
        ng = (half if first else 0) + npos
        inter, chan = self._draw(dv - 1 if first else 0, g0, ng)
        d_inter = torch.zeros((1, ng + dv - 1, self.S), dtype=torch.int16, device=self.device)
        d_inter[0, (0 if first else dv - 1):] = torch.from_numpy(inter.view(np.int16)).to(self.device)
        d_chan = torch.from_numpy(np.ascontiguousarray(chan).view(np.int32)).to(self.device).reshape(1, ng, self.wpp)
        tr = _uninit((1, npos, 10), dtype=torch.int32, device=self.device)
        darr, dptr = _lib.doped_array(self.doped)
        check(lib().scldpc_stream_run_device_inputs_at(C.byref(p), 1, self.W, darr.size, dptr, int(npos),
                                                       self.st.state.data_ptr(), self.st.counters.data_ptr(), tr.data_ptr(),
                                                       d_inter.data_ptr(), d_chan.data_ptr(), int(g0), int(ng), int(self.done),
                                                       _stream_ptr(self.st.state.device)))
        rows = tr[0].cpu().numpy().astype(np.int64)
        used = npos
        if stop is not None:
            for k in range(npos):
                if stop(rows[k, 2:]):
                    used = k + 1
                    break
        if used < npos:
            # the reference generated L/2 + (positions decoded before the tripping one) positions at this point: rewind and
            # draw exactly those
            self._host[:] = snap
            self._draw(dv - 1 if first else 0, g0, (half if first else 0) + used - 1)
        elif stop is not None and stop(rows[npos - 1, 2:]):
            self._host[:] = snap
            self._draw(dv - 1 if first else 0, g0, (half if first else 0) + used - 1)
        self.done += used
        return rows[:used]


class InputStreams(Streams):
    """Streams decoded from given per-position inputs (same-input mode): inter [nstreams, G + dv - 1, S] uint16 and
    chan [nstreams, G, wpp] uint32 as stream_glibc_inputs produces them, G = positions generated."""

    def __init__(self, p, inter, chan, W, doped=(), device="cuda:0"):
        inter, chan = np.ascontiguousarray(inter, dtype=np.uint16), np.ascontiguousarray(chan, dtype=np.uint32)
        super().__init__(p, inter.shape[0], 0, 0.0, W, doped, device=device)
        self.G = chan.shape[1]
        assert inter.shape[1] == self.G + p.dv - 1 and inter.shape[2] == p.cns_pos * p.dc
        self.d_inter = torch.from_numpy(inter.view(np.int16)).to(device)
        self.d_chan = torch.from_numpy(chan.view(np.int32)).to(device)
        self.done = 0

    def run(self, npos, trace=False):
        tr = _uninit((self.n, npos, 10), dtype=torch.int32, device=self.state.device) if trace else None
        darr, dptr = _lib.doped_array(self.doped)
        check(lib().scldpc_stream_run_device_inputs(C.byref(self.p), self.n, int(self.W), darr.size, dptr, int(npos),
                                                    self.state.data_ptr(), self.counters.data_ptr(),
                                                    tr.data_ptr() if tr is not None else None, self.d_inter.data_ptr(),
                                                    self.d_chan.data_ptr(), int(self.G), int(self.done),
                                                    _stream_ptr(self.state.device)))
        self.done += npos
        return self.counters, tr
