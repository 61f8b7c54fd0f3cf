"""Host-side mirror of the reference's Python peeling simulators
(simulators_sc_ldpc/peeling_decoding/peeling_decoding.py = PD): same function names, argument meaning, return
tuples, argv contracts and output formats — with the per-trial work (sweep peeling + stopping-set components,
random-pick peeling with the degree-1 trajectory) done by the HIP kernels of libscldpc_hip.so.

    simulate_sc_ldpc(e, l, r, L, M, is_terminated, is_protograph, is_bounded, is_tail_biting,
                     num_repeats=int(1e5), max_fuckups=2000, doping_points=[])          → 13-tuple   (PD:591-701)
    simulate_peeling_decoder_ldpc(e, l_deg, r_deg, L, M, is_terminated, is_protograph,
                                  num_repeats=None, doping_points=[])                   → (None, r1, plrs)  (PD:705-789)
    main_simulate_sc_ldpc()   = ber_sim.py            (PD:1327-1356)
    main_simulate_variance()  = simulate_variance.py  (PD:1264-1294)
    test_sc_ldpc()            = `python3 peeling_decoding.py`  (PD:1212-1245)

Two sampling modes (keyword `rng`, not in the reference's signatures):
  * rng="numpy" (default): the reference's own streams — the GLOBAL numpy RandomState for codes and channels
    (sc_ldpc.gen_slots → np.random.permutation, np.random.rand; PD:153-154) and the GLOBAL Python `random` for the
    picks (random.choice, PD:1026).  After `np.random.seed(s); random.seed(s)` the results equal the reference's
    bit for bit, and both streams are left exactly where the reference leaves them.
  * rng="philox": codes, channels and picks drawn on the device (counter-based, keyed by (seed, trial)); same
    ensemble law, any batch size / GPU count gives the same numbers.
Ensembles: the Olmos semi-structured chain (default), its tail-biting closure (flag TB, sc_ldpc.py:41-62), the
protograph-based chain (flag P, sc_ldpc_protograph.py) and the uncoupled (l,r) ensemble with repeat rejection
(ldpc.py; simulate_peeling_decoder_ldpc_uncoupled).  P together with TB is refused: the reference reduces the CN
indices mod L there (PD:204-205), which is not an ensemble.
"""
import ast
import math
import os
import pickle
import random
import sys

import numpy as np
import torch

from . import engine as E
from .engine import uncoupled_supported as _unc_first_ok, uncoupled_wide_supported as _unc_wide_ok     # shape rules: no device
from .engine import gather_frames as _gather_frames                 # host plumbing over torch.distributed: no device call


# ------------------------------------------------------------------------------------------------
# sampling with the reference's own streams (sc_ldpc.py:22-56; PD:147-195)
# ------------------------------------------------------------------------------------------------
def gen_slots(l, r, L, M):
    """sc_ldpc.gen_slots from the global numpy stream: `transmissions` int32 [L*M, l]."""
    num_cns = int(l * M / r)
    D = L + l - 1
    cn = np.stack([i * num_cns + np.random.permutation(l * M).reshape(l, M) // r for i in range(D)])
    tr = np.empty((L, M, l), dtype=np.int32)
    for d in range(l):
        tr[:, :, d] = cn[d:d + L, d, :]
    return tr.reshape(L * M, l)


def gen_erasures(e, L, M, doping_points):
    """np.random.rand(L*M) <= e (PD:154) with hard / soft doping applied (PD:166-195)."""
    mask = np.random.rand(L * M) <= e
    if isinstance(doping_points, dict):
        for pos, alpha in doping_points.items():
            mask[pos * M: pos * M + int(alpha * M)] = False
    elif len(doping_points):
        mask &= ~np.isin(np.arange(L * M) // M, list(doping_points))
    return mask


def gen_slots_tail_biting(l, r, L, M):
    """sc_ldpc.gen_slots_tail_biting from the global numpy stream: L permutations, edge d of VN position i lands in
    CN position (i+d) % L (sc_ldpc.py:41-45)."""
    num_cns = int(l * M / r)
    cn = np.stack([i * num_cns + np.random.permutation(l * M).reshape(l, M) // r for i in range(L)])
    tr = np.empty((L, M, l), dtype=np.int32)
    for d in range(l):
        tr[:, :, d] = cn[(np.arange(L) + d) % L, d, :]
    return tr.reshape(L * M, l)


def gen_protograph(e, l, r, L, M, doping_points):
    """gen_users_sc_ldpc_protograph(_doping) (PD:198-241) from the global numpy stream → (transmissions, mask).
    Position by position: M/num_cns portions × l permutations of num_cns (edge i of VN u of a portion → CN
    pos*num_cns + i*num_cns + perm_i[u], sc_ldpc_protograph.py:6-20), then rand(M) <= e."""
    if isinstance(doping_points, dict):
        raise NameError("name 'position' is not defined")      # the reference's own failure for soft doping (PD:228)
    num_cns = int(l * M / r)
    portions = int(M / num_cns)
    tr = np.empty((L, M, l), dtype=np.int32)
    mask = np.empty((L, M), dtype=bool)
    for pos in range(L):
        rows = [np.stack([i * num_cns + np.random.permutation(num_cns) for i in range(l)]).T for _ in range(portions)]
        tr[pos] = pos * num_cns + np.vstack(rows)
        mask[pos] = np.random.rand(M) <= e
        if pos in doping_points:
            mask[pos] = False                                   # PD:237
    return tr.reshape(L * M, l), mask.reshape(L * M)


def gen_slots_uncoupled(l, r, N):
    """ldpc.gen_slots from the global numpy stream: redraw until no VN meets a CN twice (ldpc.py:67-84)."""
    while True:
        tr = (np.random.permutation(l * N).reshape(l, N) // r).T
        if not any(len(np.unique(row)) != l for row in tr):
            return np.ascontiguousarray(tr, dtype=np.int32)


def _sample_numpy(e, l, r, L, M, doping_points, is_protograph, is_tail_biting):
    """One generate_users() of the reference (PD:618-627, 729-737) → (transmissions int32 [L*M, l], mask)."""
    if is_protograph:
        return gen_protograph(e, l, r, L, M, doping_points)
    tr = gen_slots_tail_biting(l, r, L, M) if is_tail_biting else gen_slots(l, r, L, M)
    return tr, gen_erasures(e, L, M, doping_points)


def _dist():
    """(torch.distributed | None, rank, world) — one process per GPU (see bp_decoding.py)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist, dist.get_rank(), dist.get_world_size()
    return None, 0, 1


def _free_bytes(device):
    """Free memory on `device` right now (the row buffers and batch sizes are budgeted against it, so that a smaller
    part, or a GPU shared between ranks, is not driven out of memory)."""
    dev = torch.device(device)
    return torch.cuda.mem_get_info(dev)[0] if dev.type == "cuda" else int(32e9)


def _device(device):
    """Default device: this rank's GPU (LOCAL_RANK), as torch.distributed.run sets it."""
    return device if device is not None else str(E.local_device())


def _split(total, world):
    """Contiguous, even shares of `total` trials: offsets [world + 1]."""
    base, rem = divmod(total, world)
    offs = [0]
    for r in range(world):
        offs.append(offs[-1] + base + (1 if r < rem else 0))
    return offs


def _check_flags(is_protograph, is_tail_biting=False):
    if is_protograph and is_tail_biting:
        raise NotImplementedError("protograph + tail-biting: the reference reduces CN indices mod L (PD:204-205), "
                                  "which merges all CNs of a residue class — not an ensemble this path implements")


def _doped_positions(doping_points):
    return sorted(doping_points.keys()) if isinstance(doping_points, dict) else list(doping_points)


class _Geometry:
    """The index bookkeeping of simulate_sc_ldpc (PD:604-611, 635-648)."""

    def __init__(self, l, r, L, M, is_terminated, is_bounded, doping_points):
        self.ignored_head = 0 if is_bounded else 20
        self.ignored_head_schedule = 0 if is_bounded else 10
        self.ignored_tail = 0 if is_terminated else 20
        self.L = L + self.ignored_head + self.ignored_tail
        self.cpp = int(l / r * M)
        self.num_positions = self.L + l - 1 if is_terminated else self.L
        self.total_size = self.cpp * self.num_positions
        nd = len(doping_points)
        if isinstance(doping_points, dict):
            self.generated = (self.L - self.ignored_head - self.ignored_tail) * M - \
                sum(int(a * M) for a in doping_points.values())
        else:
            self.generated = (self.L - nd - self.ignored_head - self.ignored_tail) * M
        self.blocks = self.L - nd - self.ignored_head - self.ignored_tail
        self.params = E.CodeParams(l, r, self.L, self.cpp, M)
        self.sweep_start = self.ignored_head_schedule * self.cpp
        self.lost_lo = self.cpp * self.ignored_head
        self.lost_hi = self.total_size - self.cpp * self.ignored_tail


# Whether simulate_sc_ldpc(sweep="auto") takes the 4-bit sweep decoder (engine.peel_sweep_sock16, peel_sweep_small.hip) and the
# sampler that writes its CN -> socket table where select_sweep allows it, instead of sample_philox(adj16=True) + peel_sweep:
# True only if every repetition of the new path beats every repetition of the old one on every shape of
# tools/sweep_small_speedup.py, with equal outputs (profiles/sweep_small_speedup.json).  Kept False here whatever
# is measured: the flip is a change of its own.
SWEEP_SMALL_BY_DEFAULT = False

# The same for the wide form of that decoder (engine.peel_sweep_sock16_wide: 32-bit queue entries, one trial per CU, more than
# 65 536 CNs per trial), which sweep="auto" consults only where SWEEP_SMALL_BY_DEFAULT's rule has declined: True only if every
# repetition of the new path beats every repetition of the old one on every shape of tools/sweep_wide_speedup.py
# (profiles/sweep_wide_speedup.json).  Kept False here whatever is measured.
SWEEP_WIDE_BY_DEFAULT = False

# Whether simulate_sc_ldpc(local_tables=None) lets sweep "small" / "wide" (and "auto" where a flag above sends it there) take
# the tail-biting and protograph ensembles: engine.sample_philox_ens_sock16 — their rows as position-local 2-byte ids with the
# CN -> socket table — and the 4-bit sweep decoder, whose tail-biting instances close the chain into a ring, instead of
# sample_philox(ensemble=...) + peel_sweep: True only if every repetition of the new path beats every repetition of the old one
# on every shape of tools/sweep_ens_speedup.py, with equal outputs (profiles/sweep_ens_speedup.json).  Kept False
# here whatever is measured: the flip is a change of its own.
LOCAL_TABLES_BY_DEFAULT = False

SWEEP_SAMPLERS = ("sample_philox_sock16", "sample_philox_deg_sock16", "sample_philox+cn_sockets", "sample_philox_ens_sock16")
SWEEP_WIDE_SAMPLERS = ("sample_philox_sock16", "sample_philox_deg_sock16", "sample_philox_wide_sock16", "sample_philox+cn_sockets",
                       "sample_philox_ens_sock16")

_SMALL_SHAPES = ("the 4-bit sweep decoder takes the pairs (3,6), (4,8), (5,10) with vns_pos * dv <= 65535 and at most "
                 "65536 CNs per trial")
_WIDE_SHAPES = ("the wide 4-bit sweep decoder takes the pairs (3,6), (4,8), (5,10) with vns_pos * dv <= 65535 (16-bit "
                "sockets) whose CN counts, VN bits and sweep_start bitmap leave two queues of 1024 entries in one CU's LDS")


def _select_local(p, ensemble, form, chain_ok, ens_sock16_ok, tb_ok):
    """select_sweep's rule for the tail-biting and protograph ensembles under local_tables: (form, "sample_philox_ens_sock16")
    where the decoder of that form takes the shape — protograph: the chain's instances (chain_ok), tail-biting: the ring's
    (tb_ok) — and the sampler takes the ensemble (ens_sock16_ok); else ("first", the limit that refused)."""
    shape = "(dv = %d, dc = %d, L = %d, M = %d: %d CNs)" % (p.dv, p.dc, p.L, p.vns_pos, p.nk)
    if not (tb_ok if ensemble == "tail_biting" else chain_ok):
        return "first", "%s%s %s" % (_WIDE_SHAPES if form == "wide" else _SMALL_SHAPES,
                                     ", tail-biting with L >= dv" if ensemble == "tail_biting" else "", shape)
    if not ens_sock16_ok:
        return "first", ("sample_philox_ens_sock16 takes at most 8192 sockets per position with vns_pos * dv <= 65535, tail-biting "
                         "with L >= dv and protograph with dv | dc " + shape)
    return form, "sample_philox_ens_sock16"


def _select_wide(p, rng, ensemble, sock16_ok, deg_sock16_ok, wide_ok, wide_sock16_ok, local_tables=False, ens_sock16_ok=False,
                 tb_ok=False):
    """select_sweep's rule for the wide form: ("wide", one of SWEEP_WIDE_SAMPLERS) or ("first", reason)."""
    if rng != "philox":
        return "first", "rng=%r draws the codes on the host: the 4-bit sweep decoder reads the device samplers' tables" % (rng,)
    if ensemble != "olmos" and local_tables:
        return _select_local(p, ensemble, "wide", wide_ok, ens_sock16_ok, tb_ok)
    if ensemble != "olmos":
        return "first", "the %s tables hold global CN ids: the 4-bit sweep decoder reads position-local 2-byte rows" % ensemble
    if not wide_ok:
        return "first", ("the wide 4-bit sweep decoder takes the pairs (3,6), (4,8), (5,10) with vns_pos * dv <= 65535 (16-bit "
                         "sockets) whose CN counts, VN bits and sweep_start bitmap leave two queues of 1024 entries in one CU's LDS "
                         "(dv = %d, dc = %d, L = %d, M = %d: %d CNs)" % (p.dv, p.dc, p.L, p.vns_pos, p.nk))
    if (p.dv, p.dc) == (4, 8) and sock16_ok:
        return "wide", "sample_philox_sock16"
    if (p.dv, p.dc) in ((3, 6), (5, 10)) and deg_sock16_ok:
        return "wide", "sample_philox_deg_sock16"
    if wide_sock16_ok:
        return "wide", "sample_philox_wide_sock16"
    return "wide", "sample_philox+cn_sockets"


def select_sweep(p, rng, ensemble, decoder_ok, sock16_ok, deg_sock16_ok, sweep="auto", wide_ok=False, wide_sock16_ok=False,
                 local_tables=False, ens_sock16_ok=False, tb_ok=False):
    """Which sampler and sweep decoder a simulate_sc_ldpc run takes: ("first", reason) — sample_philox / the host streams and
    peel_sweep —, ("small", sampler) — peel_sweep_sock16 behind one of SWEEP_SAMPLERS — or ("wide", sampler) —
    peel_sweep_sock16_wide behind one of SWEEP_WIDE_SAMPLERS.  A pure function of its arguments:
    p the _Geometry's parameters, ensemble "olmos" | "tail_biting" | "protograph", decoder_ok / sock16_ok / deg_sock16_ok the
    answers of engine.peel_sweep_sock16_supported / sock16_supported / deg_sock16_supported, sweep the requested mode,
    wide_ok / wide_sock16_ok the answers of engine.peel_sweep_wide_supported / wide_sock16_supported (read by "wide", and by
    "auto" under SWEEP_WIDE_BY_DEFAULT where the small rule has declined).
    local_tables: the tail-biting and protograph ensembles may take "small" / "wide" behind "sample_philox_ens_sock16"
    (_select_local) instead of being refused for their global CN ids; ens_sock16_ok is engine.ens_sock16_supported's answer and
    tb_ok engine.peel_sweep_tb_supported's for the requested form (read for tail-biting, where decoder_ok / wide_ok are read
    for protograph).  With local_tables false every answer and text is what it was without these three."""
    local = dict(local_tables=local_tables, ens_sock16_ok=ens_sock16_ok, tb_ok=tb_ok)
    if sweep not in ("auto", "first", "small", "wide"):
        raise ValueError("sweep must be 'auto', 'first', 'small' or 'wide'")
    if sweep == "first":
        return "first", "sweep='first'"
    if sweep == "wide":
        return _select_wide(p, rng, ensemble, sock16_ok, deg_sock16_ok, wide_ok, wide_sock16_ok, **local)
    if sweep == "auto" and SWEEP_WIDE_BY_DEFAULT:
        small = select_sweep(p, rng, ensemble, decoder_ok, sock16_ok, deg_sock16_ok, "small", **local) if SWEEP_SMALL_BY_DEFAULT else None
        if small and small[0] == "small":
            return small
        wide = _select_wide(p, rng, ensemble, sock16_ok, deg_sock16_ok, wide_ok, wide_sock16_ok, **local)
        return wide if wide[0] == "wide" or not small else small
    if sweep == "auto" and not SWEEP_SMALL_BY_DEFAULT:
        return "first", "sweep='auto' is 'first' (SWEEP_SMALL_BY_DEFAULT)"
    if rng != "philox":
        return "first", "rng=%r draws the codes on the host: the 4-bit sweep decoder reads the device samplers' tables" % (rng,)
    if ensemble != "olmos" and local_tables:
        return _select_local(p, ensemble, "small", decoder_ok, ens_sock16_ok, tb_ok)
    if ensemble != "olmos":
        return "first", "the %s tables hold global CN ids: the 4-bit sweep decoder reads position-local 2-byte rows" % ensemble
    if not decoder_ok:
        return "first", ("the 4-bit sweep decoder takes the pairs (3,6), (4,8), (5,10) with vns_pos * dv <= 65535 and at most "
                         "65536 CNs per trial (dv = %d, dc = %d, L = %d, M = %d: %d CNs)" % (p.dv, p.dc, p.L, p.vns_pos, p.nk))
    if (p.dv, p.dc) == (4, 8) and sock16_ok:
        return "small", "sample_philox_sock16"
    if (p.dv, p.dc) in ((3, 6), (5, 10)) and deg_sock16_ok:
        return "small", "sample_philox_deg_sock16"
    return "small", "sample_philox+cn_sockets"


def _sweep_choice(p, rng, ensemble, sweep, local_tables=None):
    """select_sweep with the library's answers; sweep='small' / 'wide' on a run it refuses raises, and so does
    local_tables=True on a run that does not take the position-local tables of a tail-biting or protograph ensemble."""
    if sweep not in ("auto", "first", "small", "wide"):
        raise ValueError("sweep must be 'auto', 'first', 'small' or 'wide'")
    asked = local_tables is True                                         # None: what LOCAL_TABLES_BY_DEFAULT says, never an error
    local = LOCAL_TABLES_BY_DEFAULT if local_tables is None else bool(local_tables)
    if asked and ensemble == "olmos":
        raise ValueError("local_tables=True: the Olmos chain's tables are position-local already (the switch is for the "
                         "tail-biting and protograph ensembles)")
    # the default path asks the library nothing it did not ask before
    small = sweep == "small" or (sweep == "auto" and SWEEP_SMALL_BY_DEFAULT)
    wide = sweep == "wide" or (sweep == "auto" and SWEEP_WIDE_BY_DEFAULT)
    decoder_ok = E.peel_sweep_sock16_supported(p) if small else False
    sock16_ok, deg_sock16_ok = (E.sock16_supported(p), E.deg_sock16_supported(p)) if small or wide else (False, False)
    wide_ok, wide_sock16_ok = (E.peel_sweep_wide_supported(p), E.wide_sock16_supported(p)) if wide else (False, False)
    ens_ok = tb_ok = False
    if local and ensemble != "olmos" and rng == "philox" and (small or wide):
        ens_ok = E.ens_sock16_supported(p, ensemble)
        # (sweep="auto" under both flags: the narrow ring's answer also stands for the wide one, which takes every shape it takes)
        tb_ok = E.peel_sweep_tb_supported(p, wide=wide and not small) if ensemble == "tail_biting" else False
    kind, what = select_sweep(p, rng, ensemble, decoder_ok, sock16_ok, deg_sock16_ok, sweep, wide_ok=wide_ok,
                              wide_sock16_ok=wide_sock16_ok, local_tables=local, ens_sock16_ok=ens_ok, tb_ok=tb_ok)
    if asked and kind == "first":
        raise ValueError("local_tables=True: %s" % what)
    if sweep in ("small", "wide") and kind != sweep:
        raise ValueError("sweep='%s': %s" % (sweep, what))
    if sweep != "auto" or kind != "first":
        ring = ", tail-biting" if ensemble == "tail_biting" else ""
        line = (what.replace("+", " + ") + " + peel_sweep_small (4-bit CN counts%s)" % ring if kind == "small" else
                what.replace("+", " + ") + " + peel_sweep_wide (4-bit CN counts, 32-bit queues%s)" % ring if kind == "wide" else
                "%s + peel_sweep (16- or 32-bit CN words): %s" % ("sampler (first generation)" if rng == "philox" else
                                                                  "host streams", what))
        print("[scldpc] kernels: " + line, file=sys.stderr, flush=True)
    return kind, what


def _sample_small(sampler, p, seed, trial0, ntrials, e, doped, device, ensemble="olmos"):
    """(vn_adj16, cn_sock16, chan) from the sampler select_sweep named."""
    if sampler == "sample_philox_ens_sock16":
        return E.sample_philox_ens_sock16(p, ensemble, seed, trial0, ntrials, e, doped, device=device)
    if sampler == "sample_philox_sock16":
        return E.sample_philox_sock16(p, seed, trial0, ntrials, e, doped, device=device)
    if sampler == "sample_philox_deg_sock16":
        return E.sample_philox_deg_sock16(p, seed, trial0, ntrials, e, doped, device=device)
    if sampler == "sample_philox_wide_sock16":
        return E.sample_philox_wide_sock16(p, seed, trial0, ntrials, e, doped, device=device)
    d_adj, d_ch = E.sample_philox(p, seed, trial0, ntrials, e, doped, device=device, adj16=True)
    return d_adj, E.cn_sockets(p, d_adj), d_ch


def simulate_sc_ldpc(e, l, r, L, M, is_terminated, is_protograph, is_bounded, is_tail_biting, num_repeats=int(1e5),
                     max_fuckups=2000, doping_points=[], rng="numpy", seed=0, batch=None, device=None, sweep="auto",
                     local_tables=None):
    """Error-rate Monte-Carlo of the sweep peeling decoder (PD:591-701); returns the reference's 13-tuple.
    rng="philox" under torch.distributed: every round of world*batch trials is split evenly over the ranks, the
    per-trial result rows (32 B each) are all-gathered and every rank runs the same ordered accumulation, so the stop
    rule (max_fuckups, PD:698) cuts at the same trial and every rank returns the same tuple as a single rank would.
    sweep: "first" = peel_sweep, "small" = the 4-bit sweep decoder and the sampler select_sweep names (ValueError where it
    does not apply), "wide" = its wide form for more than 65 536 CNs per trial (the same), "auto" = what SWEEP_SMALL_BY_DEFAULT
    and then SWEEP_WIDE_BY_DEFAULT say; the same 13-tuple either way.
    local_tables: True = a tail-biting or protograph run takes sweep "small" / "wide" on position-local tables
    (sample_philox_ens_sock16; ValueError("local_tables=True: ...") for the Olmos chain, whose tables are position-local
    already, for a sweep that resolves to "first", for rng="numpy" and for a shape the sampler or the decoder refuses), False =
    never, None = what LOCAL_TABLES_BY_DEFAULT says."""
    return _simulate_sc_ldpc(e, l, r, L, M, is_terminated, is_protograph, is_bounded, is_tail_biting, num_repeats, max_fuckups,
                             doping_points, rng, seed, batch, device, sweep, local_tables, None)[0]


def _simulate_sc_ldpc(e, l, r, L, M, is_terminated, is_protograph, is_bounded, is_tail_biting, num_repeats, max_fuckups,
                      doping_points, rng, seed, batch, device, sweep, local_tables, nbins):
    """The one round loop of simulate_sc_ldpc and simulate_sc_ldpc_spectrum: (tuple13, hist, pos_hist).  nbins None: the
    calls simulate_sc_ldpc has always made and (tuple13, None, None); else every decoder also writes its lost bits and
    engine.ss_spectrum runs over exactly the trials the stop rule used."""
    _check_flags(is_protograph, is_tail_biting)
    device = _device(device)
    dist, rank, world = _dist()
    if rng == "numpy" and world > 1:
        raise ValueError("rng='numpy' replays the reference's one sequential stream: single rank only")
    g = _Geometry(l, r, L, M, is_terminated, is_bounded, doping_points)
    p = g.params
    ens = "protograph" if is_protograph else "tail_biting" if is_tail_biting else "olmos"
    kind, small_sampler = _sweep_choice(p, rng, ens, sweep, local_tables)
    # whose tables the decoder reads: passed on only where it is not the Olmos chain's (sample_philox_ens_sock16)
    ens_kw = {"ensemble": ens} if small_sampler == "sample_philox_ens_sock16" and kind != "first" else {}
    if nbins is not None and ens == "tail_biting" and ens_kw:
        raise ValueError(_SPECTRUM_RING)
    if batch is None:
        batch = 64 if rng == "numpy" else 2048
    # the spectrum pass reads the lost bits: asked for only there, so that simulate_sc_ldpc's calls are what they were
    lost_kw = {"want_lost": True} if nbins is not None else {}
    hist = pos_hist = None
    if nbins is not None:
        hist = torch.zeros(nbins, dtype=torch.int64, device=device)
        pos_hist = torch.zeros((p.L, E.SS_POS_SIZES), dtype=torch.int64, device=device)

    def spectrum(d_adj, d_lost, take):
        """The trials [0, take) of this rank's share of the round: those the stop rule used."""
        if nbins is not None and take > 0:
            E.ss_spectrum(p, d_adj[:take], d_lost[:take], nbins, hist, pos_hist)
    # The reference's per-trial bookkeeping and its stop rule (PD:668-699) run on the device, in trial order
    # (scldpc_accumulate_peel_device): the host reads the six totals only in rounds in which max_fuckups could trip.
    run = torch.zeros(E.NPEELRUN, dtype=torch.int64, device=device)
    i_tr, i_fu = E.PEELRUN_NAMES.index("trials"), E.PEELRUN_NAMES.index("fuckups")
    done = 0
    fuckups_bound = 0                                   # upper bound on num_fuckups while nobody has looked
    soft = isinstance(doping_points, dict)
    while done < num_repeats:
        nb = min(batch * world, num_repeats - done)         # trials of this round (all ranks)
        offs = _split(nb, world)
        lo, mine = offs[rank], offs[rank + 1] - offs[rank]
        states = None
        if rng == "numpy":
            adj = np.empty((nb, p.n, l), dtype=np.int32)
            ch = np.empty((nb, p.nw), dtype=np.uint32)
            states = []
            for t in range(nb):
                adj[t], mask = _sample_numpy(e, l, r, g.L, M, doping_points, is_protograph, is_tail_biting)
                ch[t] = E.pack_bits(mask.astype(np.uint8))
                states.append(np.random.get_state())
            d_adj, d_ch = E.to_device(adj, ch, device)
        elif rng == "philox":
            if soft and is_protograph:
                raise NameError("name 'position' is not defined")   # the reference's own failure for soft doping (PD:228)
            doped = [] if soft else _doped_positions(doping_points)
            if kind in ("small", "wide"):
                d_adj, d_cn, d_ch = _sample_small(small_sampler, p, seed, done + lo, mine, e, doped, device, ens)
            else:
                d_adj, d_ch = E.sample_philox(p, seed, done + lo, mine, e, doped, device=device, adj16=(ens == "olmos"),
                                              ensemble=ens)
            if soft:                                        # PD:176-183: the first int(alpha*M) VNs of the position are known
                for pos, alpha in doping_points.items():
                    E.clear_channel_range(p, d_ch, pos * M, pos * M + int(alpha * M))
        else:
            raise ValueError("rng must be 'numpy' or 'philox'")
        if kind == "small":
            res = E.peel_sweep_sock16(p, d_adj, d_cn, d_ch, g.total_size, g.sweep_start, g.lost_lo, g.lost_hi, **lost_kw, **ens_kw)
        elif kind == "wide":
            res = E.peel_sweep_sock16_wide(p, d_adj, d_cn, d_ch, g.total_size, g.sweep_start, g.lost_lo, g.lost_hi, **lost_kw, **ens_kw)
        else:
            res = E.peel_sweep(p, d_adj, d_ch, g.total_size, g.sweep_start, g.lost_lo, g.lost_hi, **lost_kw)
        d_out, d_lost = res["out"], res.get("lost")
        d_out = _gather_frames(dist, d_out, [offs[r + 1] - offs[r] for r in range(world)])
        E.accumulate_peel(d_out, run, max_fuckups)
        fuckups_bound += nb
        if fuckups_bound < max_fuckups and states is None:
            done += nb                                      # cannot have tripped: stay asynchronous
            spectrum(d_adj, d_lost, mine)
            continue
        tot = run.cpu().numpy()
        used = int(tot[i_tr]) - done
        fuckups_bound = int(tot[i_fu])
        done += used
        spectrum(d_adj, d_lost, min(max(used - lo, 0), mine))
        if used < nb or tot[i_fu] >= max_fuckups:
            if states is not None:
                np.random.set_state(states[used - 1])       # leave the stream where the reference stops drawing
            break
    tot = {k: int(v) for k, v in zip(E.PEELRUN_NAMES, run.cpu().numpy())}
    assert tot["trials"] == done
    num_fuckups, num_fuckups_truncated = tot["fuckups"], tot["fuckups_exp"]
    total_failed, total_failed_expurgated, total_blocks_failed_exp = tot["lost"], tot["lost_exp"], tot["blocks_exp"]
    total_generated, total_blocks_generated = done * g.generated, done * g.blocks
    o1 = done
    failures, gens = np.zeros(num_repeats), np.zeros(num_repeats)
    tuple13 = (num_fuckups / o1, num_fuckups_truncated / o1, total_failed / total_generated,
               total_failed_expurgated / total_generated, num_fuckups_truncated, o1, total_failed_expurgated,
               total_generated, failures, gens, total_blocks_failed_exp, total_blocks_generated,
               total_blocks_failed_exp / total_blocks_generated)
    if nbins is None:
        return tuple13, None, None
    if world > 1:                                           # integer sums: one all-reduce, the same arrays on every rank
        dist.all_reduce(hist)
        dist.all_reduce(pos_hist)
    return tuple13, hist.cpu().numpy(), pos_hist.cpu().numpy()


_SPECTRUM_RING = ("spectrum: a tail-biting run on position-local tables (local_tables) has ring-local 2-byte rows, a table form "
                  "engine.ss_spectrum does not read: pass local_tables=False")


def simulate_sc_ldpc_spectrum(e, l, r, L, M, is_terminated, is_protograph, is_bounded, is_tail_biting, num_repeats=int(1e5),
                              max_fuckups=2000, doping_points=[], rng="numpy", seed=0, batch=None, device=None, sweep="auto",
                              local_tables=None, nbins=256):
    """simulate_sc_ldpc with the size spectrum of the stopping sets it leaves behind (extract_stopping_sets, PD:1077-1095, on
    the device: engine.ss_spectrum on every round's lost bits).  Returns (tuple13, hist, pos_hist) as numpy arrays: tuple13 is
    value for value simulate_sc_ldpc's for the same arguments; hist int64 [nbins] counts, over exactly the o1 = tuple13[5]
    trials of the tuple, hist[0] = trials that lost nothing and hist[min(s, nbins - 1)] = stopping sets of s VNs; pos_hist int64
    [L', 8] counts them by the position of their lowest-index VN (L' the widened L of the run) and min(s, 8) - 1.  Under
    torch.distributed every rank returns the same sums.  2 <= nbins <= 4096 (ValueError); a tail-biting run with
    local_tables=True raises ValueError("spectrum: ...")."""
    if not (isinstance(nbins, (int, np.integer)) and 2 <= nbins <= E.SS_MAX_BINS):
        raise ValueError("spectrum: 2 <= nbins <= %d (got %r)" % (E.SS_MAX_BINS, nbins))
    if is_tail_biting and local_tables is True:
        raise ValueError(_SPECTRUM_RING)
    return _simulate_sc_ldpc(e, l, r, L, M, is_terminated, is_protograph, is_bounded, is_tail_biting, num_repeats, max_fuckups,
                             doping_points, rng, seed, batch, device, sweep, local_tables, int(nbins))


# Whether ber_sim --rng philox takes simulate_sc_ldpc_curve (one sampled code and one decoder launch per batch for the whole eps
# grid: engine.channel_levels + engine.peel_sweep_eps) where --eps-fused is "auto" or absent, instead of one simulate_sc_ldpc per
# eps: True only if every repetition of the fused run beats every repetition of the loop it replaces on every shape of
# tools/eps_fused_speed.py, with equal outputs (profiles/eps_fused_speed.json).  Kept False here whatever is
# measured: the flip is a change of its own.
EPS_FUSED_BY_DEFAULT = False

_EPS_UNBOUNDED = ("eps_fused: an unbounded chain sweeps from CN position 10 (sweep_start > 0), where a CN below the sweep start "
                  "fires only on a transition and the residual at one eps is not the residual of the residual at a higher one")


def curve_stages(es):
    """The host side of simulate_sc_ldpc_curve, a pure function: es in the caller's order -> (stage_eps, stage_of) with
    stage_eps the eps of the distinct thresholds (engine.erasure_threshold) in strictly descending order, the first eps of
    the caller's that has the threshold standing for it, and stage_of[i] the stage of es[i]."""
    es = [float(e) for e in es]
    th = [E.erasure_threshold(e) for e in es]
    uniq = sorted(set(th), reverse=True)
    return [es[th.index(t)] for t in uniq], [uniq.index(t) for t in th]


def simulate_sc_ldpc_curve(es, l, r, L, M, is_terminated, is_protograph, is_bounded, is_tail_biting, num_repeats=int(1e5),
                           max_fuckups=2000, doping_points=[], seed=0, batch=None, device=None, rng="philox", sweep="first",
                           local_tables=None):
    """simulate_sc_ldpc(e, ..., rng="philox", seed=seed, sweep="first") for every e of es, as a list of 13-tuples in the caller's
    order, value for value — from ONE sampled code per trial and one decoder launch per batch: the codes depend on (seed, trial)
    only and the erased sets of a descending eps grid are nested, so the channel goes to the device as levels
    (engine.channel_levels) and engine.peel_sweep_eps peels point k on from the residual of point k - 1.  Points with one
    threshold are one stage; a point leaves the following rounds once its fuckups reach max_fuckups.  Under torch.distributed one
    all-gather per round carries the rows of every live point.
    ValueError("eps_fused: ...") for rng="numpy" (a fresh stream per eps: nothing is shared), is_bounded=False (the sweep starts
    above CN 0), sweep "small" / "wide" and local_tables=True (this decoder is its own path), more than 64 distinct points, and a
    shape the entry refuses."""
    if rng != "philox":
        raise ValueError("eps_fused: rng=%r draws a fresh stream of codes and channels for every eps: nothing is shared between "
                         "the points (pass rng='philox')" % (rng,))
    if not is_bounded:
        raise ValueError(_EPS_UNBOUNDED)
    if sweep not in ("first", "auto"):
        raise ValueError("eps_fused: sweep=%r chooses the 4-bit sweep decoder, which this path does not run: the eps walk is a "
                         "decoder of its own (engine.peel_sweep_eps)" % (sweep,))
    if local_tables:
        raise ValueError("eps_fused: local_tables=True chooses the tables of the 4-bit sweep decoder, which this path does not run")
    _check_flags(is_protograph, is_tail_biting)
    es = list(es)
    if not es:
        return []
    stage_eps, stage_of = curve_stages(es)
    K = len(stage_eps)
    if K > E.EPS_MAX_POINTS:
        raise ValueError("eps_fused: at most %d distinct eps points in one run (got %d)" % (E.EPS_MAX_POINTS, K))
    g = _Geometry(l, r, L, M, is_terminated, is_bounded, doping_points)
    p = g.params
    assert g.sweep_start == 0
    ens = "protograph" if is_protograph else "tail_biting" if is_tail_biting else "olmos"
    try:
        E.peel_sweep_eps_workspace_bytes(p, 1, ens == "olmos")              # the entry's own shape rule; needs no device
    except E.ScldpcError as err:
        raise ValueError("eps_fused: %s" % err)
    soft = isinstance(doping_points, dict)
    if soft and is_protograph:
        raise NameError("name 'position' is not defined")                   # the reference's own failure for soft doping (PD:228)
    device = _device(device)
    dist, rank, world = _dist()
    print("[scldpc] kernels: sampler (first generation) + channel_levels + peel_sweep_eps (%d eps points from one code)" % K,
          file=sys.stderr, flush=True)
    if batch is None:
        batch = 2048
    doped = [] if soft else _doped_positions(doping_points)
    run = torch.zeros((K, E.NPEELRUN), dtype=torch.int64, device=device)
    i_tr, i_fu = E.PEELRUN_NAMES.index("trials"), E.PEELRUN_NAMES.index("fuckups")
    live = list(range(K))                                                   # stages still running, by descending eps
    bound = [0] * K                                                         # upper bound on a stage's fuckups while nobody has looked
    done = 0                                                                # trials fed to every live stage
    while live and done < num_repeats:
        nb = min(batch * world, num_repeats - done)                         # the round of simulate_sc_ldpc: same keys, same split
        offs = _split(nb, world)
        lo, mine = offs[rank], offs[rank + 1] - offs[rank]
        d_adj, _ = E.sample_philox(p, seed, done + lo, mine, max(es), doped, device=device, adj16=(ens == "olmos"), ensemble=ens)
        d_lev = E.channel_levels(p, seed, done + lo, mine, [stage_eps[k] for k in live], doped, device=device)
        if soft:                                                            # PD:176-183: the first int(alpha*M) VNs of the position are known
            for pos, alpha in doping_points.items():
                d_lev[:, pos * M: pos * M + int(alpha * M)] = 0
        d_out = E.peel_sweep_eps(p, d_adj, d_lev, len(live), g.total_size, g.lost_lo, g.lost_hi)["out"]
        d_out = _gather_frames(dist, d_out, [offs[r + 1] - offs[r] for r in range(world)], dim=1)
        for i, k in enumerate(live):
            E.accumulate_peel(d_out[i], run[k], max_fuckups)
            bound[k] += nb
        if all(bound[k] < max_fuckups for k in live):
            done += nb                                                      # no stage can have tripped: stay asynchronous
            continue
        tot = run.cpu().numpy()                                             # every row in one transfer
        still = []
        for k in live:
            bound[k] = int(tot[k, i_fu])
            if int(tot[k, i_tr]) - done == nb and tot[k, i_fu] < max_fuckups:
                still.append(k)
        live = still
        done += nb
    tot = run.cpu().numpy()
    tuples = []
    for k in range(K):
        t = {name: int(v) for name, v in zip(E.PEELRUN_NAMES, tot[k])}
        o1 = t["trials"]
        total_generated, total_blocks_generated = o1 * g.generated, o1 * g.blocks
        tuples.append((t["fuckups"] / o1, t["fuckups_exp"] / o1, t["lost"] / total_generated, t["lost_exp"] / total_generated,
                       t["fuckups_exp"], o1, t["lost_exp"], total_generated, t["blocks_exp"], total_blocks_generated,
                       t["blocks_exp"] / total_blocks_generated))
    out = []
    for k in stage_of:                                                      # the caller's order, duplicates included
        a = tuples[k]
        out.append(a[:8] + (np.zeros(num_repeats), np.zeros(num_repeats)) + a[8:])
    return out


# Whether simulate_peeling_decoder_ldpc(pick="auto") takes engine.peel_pick_deg (the CN words through cn_build.hip's LDS ring,
# two trials per wave in peel_pick_multi_kernel, for the pairs (3,6), (4,8), (5,10)) where select_pick allows it, instead of
# engine.peel_pick: True only if every repetition of the new path beats every repetition of the old one on every shape of
# tools/pick_deg_speedup.py, with equal outputs (profiles/pick_deg_speedup.json).  Kept False here whatever is
# measured: the flip is a change of its own.
PICK_DEG_BY_DEFAULT = False


def select_pick(p, total_size, rng, ensemble, moments_from, deg_ok, pick="auto"):
    """Which random-pick decoder a simulate_peeling_decoder_ldpc run takes: ("first", reason) — engine.peel_pick — or
    ("multi", "cn_build ring + peel_pick_multi") — engine.peel_pick_deg.  A pure function of its arguments: ensemble is
    "olmos" or "protograph", moments_from the resolved source of the moments ("rows" where none are wanted), deg_ok the
    answer of engine.peel_pick_deg_supported(p, total_size), pick the requested mode."""
    if pick not in ("auto", "first", "multi"):
        raise ValueError("pick must be 'auto', 'first' or 'multi'")
    if pick == "first":
        return "first", "pick='first'"
    if pick == "auto" and not PICK_DEG_BY_DEFAULT:
        return "first", "pick='auto' is 'first' (PICK_DEG_BY_DEFAULT)"
    if rng != "philox":
        return "first", "rng=%r replays the MT19937 stream, which is sequential: the multi-trial pick kernel draws from Philox" % (rng,)
    if ensemble == "protograph":
        return "first", "the protograph tables hold global CN ids in 4-byte rows: the multi-trial pick kernel reads position-local 2-byte rows"
    if moments_from == "kernel":
        return "first", "moments_from='kernel': the multi-trial pick kernel has no in-chain moments (use 'rows')"
    if not deg_ok:
        return "first", ("the multi-trial pick kernel takes the pairs (3,6), (4,8), (5,10) with cns_pos <= 65536, at most 4096 "
                         "words of degree-1 bitmap and a ring of dv CN positions within the LDS (dv = %d, dc = %d, L = %d, M = %d, "
                         "total_size = %d)" % (p.dv, p.dc, p.L, p.vns_pos, total_size))
    return "multi", "cn_build ring + peel_pick_multi"


def _pick_choice(p, total_size, rng, ensemble, moments_from, pick):
    """select_pick with the library's answer; pick='multi' on a run it refuses raises."""
    # the default path asks the library nothing it did not ask before
    ask = pick == "multi" or (pick == "auto" and PICK_DEG_BY_DEFAULT)
    deg_ok = E.peel_pick_deg_supported(p, total_size) if ask else False
    kind, what = select_pick(p, total_size, rng, ensemble, moments_from, deg_ok, pick)
    if pick == "multi" and kind != "multi":
        raise ValueError("pick='multi': %s" % what)
    if pick != "auto" or kind != "first":
        sampler = "sampler (first generation)" if rng == "philox" else "host streams"
        line = ("%s + %s" % (sampler, what) if kind == "multi" else "%s + peel_pick: %s" % (sampler, what))
        print("[scldpc] kernels: " + line, file=sys.stderr, flush=True)
    return kind


def simulate_peeling_decoder_ldpc(e, l_deg, r_deg, L, M, is_terminated, is_protograph, num_repeats=None,
                                  doping_points=[], rng="numpy", seed=0, batch=None, device=None,
                                  want_moments=False, moments_from="auto", pick="auto"):
    """Random-pick peeling with the degree-1-CN trajectory (PD:705-789): returns (None, r1, plrs) with
    r1 int64 [num_repeats, num_pd_steps+1] and plrs float64 [num_repeats].  want_moments=True (philox mode) returns
    (None, moments int64 [3, num_pd_steps+1], plrs) instead of the full trajectories; moments_from: "rows" (the batch's
    trajectories stay on the device and one pass reduces them), "kernel" (three atomics per step inside the pick chain, no
    row buffer) or "auto" (rows where they fit 24 GB).
    rng="philox" under torch.distributed: rank r runs a contiguous share of the trials (global trial indices, so the
    draws do not depend on the sharding); one all-reduce sums the moment vectors (24 B per step) and fills in plrs —
    and the r1 rows when they are asked for — so every rank returns what a single rank would.
    pick: "first" = engine.peel_pick, "multi" = engine.peel_pick_deg (ValueError where select_pick refuses; with want_moments
    it resolves moments_from="auto" to "rows"), "auto" = what PICK_DEG_BY_DEFAULT says; the same arrays either way."""
    if not num_repeats:
        num_repeats = 100
    device = _device(device)
    dist, rank, world = _dist()
    if rng == "numpy" and world > 1:
        raise ValueError("rng='numpy' replays the reference's one sequential stream: single rank only")
    if isinstance(doping_points, dict):
        raise NotImplementedError("simulate_peeling_decoder_ldpc takes hard doping points only (PD:747)")
    cpp = int(l_deg / r_deg * M)
    num_positions = L + l_deg - 1 if is_terminated else L
    total_size = cpp * num_positions
    num_pd_steps = int(M * num_positions * (e + 0.1))                      # PD:721
    nd = len(doping_points)
    p = E.CodeParams(l_deg, r_deg, L, cpp, M)
    total_generated = (L - nd) * M                                         # PD:747
    kind = _pick_choice(p, total_size, rng, "protograph" if is_protograph else "olmos", moments_from if want_moments else "rows", pick)
    if kind == "multi" and want_moments and moments_from == "auto":
        moments_from = "rows"
    plrs = np.zeros(num_repeats)
    if rng == "numpy":
        r1 = np.zeros((num_repeats, num_pd_steps + 1), dtype="int")
        for o in range(num_repeats):                                       # one shared `random` stream: sequential
            adj, mask = _sample_numpy(e, l_deg, r_deg, L, M, doping_points, is_protograph, False)
            d_adj, d_ch = E.to_device(adj[None], E.pack_bits(mask.astype(np.uint8))[None], device)
            st = random.getstate()
            mt = torch.from_numpy(np.array(st[1], dtype=np.uint32).view(np.int32).copy()[None]).to(device)
            res = E.peel_pick(p, d_adj, d_ch, total_size, num_pd_steps, mt_state=mt)
            new = mt.cpu().numpy().view(np.uint32)[0]
            random.setstate((st[0], tuple(int(x) for x in new), st[2]))
            r1[o] = res["r1"][0].cpu().numpy()
            n_users, picked = (int(x) for x in res["out"][0, :2].cpu())
            plrs[o] = (n_users - picked) / total_generated               # (generated − recovered)/generated, PD:753,785
            if r1[o, -1] == 1:
                print("The number of degree-1 CNs at the end of the iterations is 1!!!")
        return None, r1, plrs
    if rng != "philox":
        raise ValueError("rng must be 'numpy' or 'philox'")
    r1_all = None if want_moments else np.zeros((num_repeats, num_pd_steps + 1), dtype="int")
    moments = None
    if batch is None:
        # one wave steps one trial: the kernel wants ~8192 trials in flight; stay below ~16 GB of device buffers
        # (tables + CN words + picks' scratch ~ 3 x the int32 adjacency; r1 rows 4 B per step where they are written)
        rows_wanted = (not want_moments) or moments_from in ("auto", "rows")
        per_trial = 3 * L * M * l_deg * 4 + (4 * (num_pd_steps + 1) if rows_wanted else 0)
        free = _free_bytes(device)
        batch = max(64, min(8192, int(min(16e9 + (24e9 if rows_wanted and want_moments else 0), 0.6 * free) // per_trial)))
    offs = _split(num_repeats, world)
    if want_moments:
        moments = torch.zeros((3, num_pd_steps + 1), dtype=torch.int64, device=device)
    for done in range(offs[rank], offs[rank + 1], batch):
        nb = min(batch, offs[rank + 1] - done)
        d_adj, d_ch = E.sample_philox(p, seed, done, nb, e, list(doping_points), device=device,
                                      adj16=not is_protograph, ensemble="protograph" if is_protograph else "olmos")
        # moments: three global atomics per step inside the pick chain cost 7 % (tools/ab_c3.py); where the batch's rows fit
        # (4 B per step and trial) they are written instead and reduced by one pass of r1_moments
        if moments_from not in ("auto", "rows", "kernel"):
            raise ValueError("moments_from must be 'auto', 'rows' or 'kernel'")
        # "auto": rows where they fit a quarter of what is free on THIS device right now (shared / smaller parts included)
        rows_first = want_moments and (moments_from == "rows" or
                                       (moments_from == "auto" and
                                        4 * (num_pd_steps + 1) * nb <= min(24e9, 0.25 * _free_bytes(device))))
        if kind == "multi":
            res = E.peel_pick_deg(p, d_adj, d_ch, total_size, num_pd_steps, seed=seed, trial0=done, want_r1=True)
        else:
            res = E.peel_pick(p, d_adj, d_ch, total_size, num_pd_steps, mt_state=None, seed=seed, trial0=done,
                              want_r1=not want_moments or rows_first, moments=None if rows_first else moments)
        if rows_first:
            E.r1_moments(res["r1"], moments)
            res["r1"] = None
        o = res["out"].cpu().numpy()
        plrs[done:done + nb] = (o[:, 0] - o[:, 1]) / total_generated
        if not want_moments:
            r1_all[done:done + nb] = res["r1"].cpu().numpy()
    if world > 1:                                           # shares are disjoint: a sum puts them together
        t_plr = torch.from_numpy(plrs).to(device)
        dist.all_reduce(t_plr)
        plrs = t_plr.cpu().numpy()
        if want_moments:
            dist.all_reduce(moments)
        else:
            t_r1 = torch.from_numpy(r1_all).to(device)
            dist.all_reduce(t_r1)
            r1_all = t_r1.cpu().numpy()
    return None, (moments.cpu().numpy() if want_moments else r1_all), plrs


COV_MAX_STEPS = 4096            # SCLDPC_COV_MAX_STEPS (include/scldpc_cov.h)


def _cov_steps(steps, num_pd_steps):
    """The steps of simulate_pd_covariance as int64 [K]: an int is a stride over range(0, num_pd_steps + 1, stride)."""
    if isinstance(steps, (int, np.integer)) and not isinstance(steps, bool):
        if steps < 1:
            raise ValueError("steps: a stride must be at least 1 (got %d)" % steps)
        steps = range(0, num_pd_steps + 1, int(steps))
    if isinstance(steps, torch.Tensor):
        steps = steps.cpu().numpy()
    arr = np.asarray(list(steps) if isinstance(steps, range) else steps)
    if arr.ndim != 1 or arr.size == 0 or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError("steps must be a stride or a non-empty one-dimensional sequence of integers")
    arr = arr.astype(np.int64)
    if arr.size > COV_MAX_STEPS:
        raise ValueError("steps: at most %d steps (got K = %d)" % (COV_MAX_STEPS, arr.size))
    if arr[0] < 0 or arr[-1] > num_pd_steps or arr.min() < 0 or arr.max() > num_pd_steps:
        raise ValueError("steps: a step out of range [0, %d]" % num_pd_steps)
    if arr.size > 1 and (np.diff(arr) <= 0).any():
        raise ValueError("steps must be strictly increasing (unsorted or repeated steps)")
    return arr


def simulate_pd_covariance(e, l_deg, r_deg, L, M, is_terminated, is_protograph, num_repeats, steps, doping_points=[],
                           seed=0, batch=None, device=None, pick="auto"):
    """The second moments of the degree-1 trajectories between K chosen peeling steps, at a size where the rows cannot be kept:
    returns (steps int64 [K], gram int64 [3, K, K], moments int64 [3, num_pd_steps+1], plrs float64 [num_repeats]) with, for
    x[t, i] = r1[t, steps[i]] and m = (x != 0) over all num_repeats trials, gram = (mᵀm, xᵀm, xᵀx) in exact integers
    (engine.r1_gram; cov_from_gram reduces it).  Philox mode only: the loop of simulate_peeling_decoder_ldpc(rng="philox",
    want_moments=True, moments_from="rows") — the same sampler, decoder selection (pick), trial keys and batch budget, so
    moments and plrs equal that call's value for value — in which each batch's rows go through r1_moments AND r1_gram before
    they are dropped.  gram depends neither on batch nor on the number of ranks (integer sums); under torch.distributed one
    more all-reduce sums it.  steps: K <= 4096 strictly increasing steps in [0, num_pd_steps], or an int stride meaning
    range(0, num_pd_steps + 1, stride).  ValueError for other steps, a soft-doping dict, and a run whose sums could leave 63
    bits (total_size² · num_repeats >= 2⁶³: r1 never exceeds total_size)."""
    if isinstance(doping_points, dict):
        raise ValueError("simulate_pd_covariance takes hard doping points only (PD:747), not a soft-doping dict")
    num_repeats = int(num_repeats)
    if num_repeats < 1:
        raise ValueError("num_repeats must be at least 1")
    cpp = int(l_deg / r_deg * M)
    num_positions = L + l_deg - 1 if is_terminated else L
    total_size = cpp * num_positions
    num_pd_steps = int(M * num_positions * (e + 0.1))                      # PD:721
    steps = _cov_steps(steps, num_pd_steps)
    if total_size * total_size * num_repeats >= 1 << 63:
        raise ValueError("total_size^2 * num_repeats = %d^2 * %d >= 2^63: the 64-bit sums of the Gram matrices could overflow"
                         % (total_size, num_repeats))
    device = _device(device)
    dist, rank, world = _dist()
    nd = len(doping_points)
    p = E.CodeParams(l_deg, r_deg, L, cpp, M)
    total_generated = (L - nd) * M                                         # PD:747
    kind = _pick_choice(p, total_size, "philox", "protograph" if is_protograph else "olmos", "rows", pick)
    plrs = np.zeros(num_repeats)
    if batch is None:                                                      # simulate_peeling_decoder_ldpc's budget, rows wanted
        per_trial = 3 * L * M * l_deg * 4 + 4 * (num_pd_steps + 1)
        batch = max(64, min(8192, int(min(16e9 + 24e9, 0.6 * _free_bytes(device)) // per_trial)))
    offs = _split(num_repeats, world)
    moments = torch.zeros((3, num_pd_steps + 1), dtype=torch.int64, device=device)
    gram = torch.zeros((3, steps.size, steps.size), dtype=torch.int64, device=device)
    d_steps = torch.from_numpy(steps.astype(np.int32)).to(device)
    for done in range(offs[rank], offs[rank + 1], batch):
        nb = min(batch, offs[rank + 1] - done)
        d_adj, d_ch = E.sample_philox(p, seed, done, nb, e, list(doping_points), device=device,
                                      adj16=not is_protograph, ensemble="protograph" if is_protograph else "olmos")
        if kind == "multi":
            res = E.peel_pick_deg(p, d_adj, d_ch, total_size, num_pd_steps, seed=seed, trial0=done, want_r1=True)
        else:
            res = E.peel_pick(p, d_adj, d_ch, total_size, num_pd_steps, mt_state=None, seed=seed, trial0=done,
                              want_r1=True, moments=None)
        E.r1_moments(res["r1"], moments)
        E.r1_gram(res["r1"], d_steps, gram)
        res["r1"] = None
        o = res["out"].cpu().numpy()
        plrs[done:done + nb] = (o[:, 0] - o[:, 1]) / total_generated
    if world > 1:                                           # shares are disjoint: a sum puts them together
        t_plr = torch.from_numpy(plrs).to(device)
        dist.all_reduce(t_plr)
        plrs = t_plr.cpu().numpy()
        dist.all_reduce(moments)
        dist.all_reduce(gram)
    return steps, gram.cpu().numpy(), moments.cpu().numpy(), plrs


# simulate_peeling_decoder_ldpc_uncoupled(rng="philox"): the default batch keeps the expected attempts of one sampler launch,
# batch * exp((l-1)(r-1)/2), below this — about a second of scldpc_sample_philox_uncoupled_device at (4,8), M = 1000.
# Measured on MI355X (tools/uncoupled_speedup.py, profiles/uncoupled_speedup.json, taken with 1 << 24 here and --hard-trials 512):
# 13.1 M attempts/s at (4,8), M = 1000 in launches of 512 trials (1.54 s; 37 561 attempts per trial) — such a launch waits for
# its unluckiest trial, some 250 000 attempts at about 6 us each for a workgroup alone, so a smaller batch shortens it only
# logarithmically — and 51.0 M attempts/s at (3,6), M = 1000 in launches of 8192 trials (23.5 ms; 149.4 attempts per trial),
# which this cap leaves at the budget rule's 8192.  (4,8): batch 357.
UNCOUPLED_ATTEMPTS_PER_LAUNCH = 13_000_000
UNCOUPLED_MAX_ATTEMPTS = 1 << 24                # scldpc_sample_philox_uncoupled_device's range

# Beyond 8192 sockets the graphs come from engine.sample_philox_uncoupled_wide (csrc/sampler_uncoupled_wide.hip), and the budget
# of one launch is that kernel's: about a second at its measured rate at (3,6), M = 10000, as the first sampler's 13 M attempts
# are about a second of its 13.1 M attempts/s.  Measured on MI355X (tools/uncoupled_wide_speedup.py,
# profiles/uncoupled_wide_speedup.json, taken with 1_000_000 here; the tool passes its batch of 8192 itself): 2.02 M attempts/s at
# (3,6), M = 10000 in launches of 8192 trials (589 ms; 147.9 attempts per trial) — four parts of the key range per attempt — and
# 12.3 M attempts/s at M = 5000 (98.5 ms), where one part holds every key and this budget is the more cautious.  (3,6): the
# budget rule's 8192 stands (13 476 would be allowed); (4,8) beyond 8192 sockets: batch 55.
UNCOUPLED_WIDE_ATTEMPTS_PER_LAUNCH = 2_000_000
UNCOUPLED_FIRST_SOCKETS, UNCOUPLED_WIDE_SOCKETS = 8192, 32768

# Whether simulate_peeling_decoder_ldpc_uncoupled(rng="philox") takes the wide sampler also where the first one takes the shape
# (at most 8192 sockets).  The two write the same outputs there; tools/uncoupled_wide_speedup.py times them side by side
# (profiles/uncoupled_wide_speedup.json).  Kept False here whatever is measured: the flip is a change of its own.
UNCOUPLED_WIDE_BY_DEFAULT = False


def select_uncoupled(p, first_ok, wide_ok, wide_by_default=False):
    """Which rejection sampler a simulate_peeling_decoder_ldpc_uncoupled(rng="philox") run takes: "first" —
    engine.sample_philox_uncoupled — or "wide" — engine.sample_philox_uncoupled_wide.  A pure function of its arguments: p the
    CodeParams(l, r, 1, cns_pos, M), first_ok / wide_ok the answers of engine.uncoupled_supported / uncoupled_wide_supported,
    wide_by_default the module's UNCOUPLED_WIDE_BY_DEFAULT.  "first" wherever the first sampler takes the shape and
    wide_by_default is false, so such a run does what it did before there was a second one; "wide" where only the wide one
    does, and with wide_by_default wherever it does.  ValueError, naming the limits, where neither takes the shape."""
    if wide_ok and (wide_by_default or not first_ok):
        return "wide"
    if first_ok:
        return "first"
    raise ValueError("rng='philox': the uncoupled samplers take L = 1, dv <= 8, dv <= cns_pos and at most %d sockets "
                     "(sample_philox_uncoupled: %d); got dv = %d, dc = %d, cns_pos = %d, M = %d: %d sockets"
                     % (UNCOUPLED_WIDE_SOCKETS, UNCOUPLED_FIRST_SOCKETS, p.dv, p.dc, p.cns_pos, p.vns_pos, p.cns_pos * p.dc))


def _uncoupled_philox(e, l_deg, r_deg, M, num_repeats, device, seed, batch, want_moments, max_attempts):
    """The rng="philox" body of simulate_peeling_decoder_ldpc_uncoupled."""
    device = _device(device)
    dist, rank, world = _dist()
    cpp = l_deg * M // r_deg
    num_pd_steps = int(M * (e + 0.1))                                      # PD:804
    p = E.CodeParams(l_deg, r_deg, 1, cpp, M)
    expected = math.exp((l_deg - 1) * (r_deg - 1) / 2.0)                    # attempts per accepted graph, about
    sockets = cpp * r_deg
    if sockets <= UNCOUPLED_FIRST_SOCKETS and not UNCOUPLED_WIDE_BY_DEFAULT:
        path = "first"                                                      # the first sampler judges the shape itself, as before
    else:
        path = select_uncoupled(p, _unc_first_ok(p), _unc_wide_ok(p), UNCOUPLED_WIDE_BY_DEFAULT)
    sample = E.sample_philox_uncoupled_wide if path == "wide" else E.sample_philox_uncoupled
    budget = UNCOUPLED_WIDE_ATTEMPTS_PER_LAUNCH if sockets > UNCOUPLED_FIRST_SOCKETS else UNCOUPLED_ATTEMPTS_PER_LAUNCH
    if batch is None:
        # the sibling's budget (~8192 trials in flight, ~16 GB of device buffers: tables + CN words + picks' scratch ~ 3 x the
        # int32 adjacency, r1 rows 4 B per step), capped by the attempts one sampler launch may be expected to take
        per_trial = 3 * M * l_deg * 4 + 4 * (num_pd_steps + 1)
        free = _free_bytes(device)
        batch = max(64, min(8192, int(min(16e9 + (24e9 if want_moments else 0), 0.6 * free) // per_trial)))
        batch = max(1, min(batch, int(budget / expected)))
    plrs = np.zeros(num_repeats)
    erased = np.zeros(num_repeats, dtype=np.int64)
    r1_all = None if want_moments else np.zeros((num_repeats, num_pd_steps + 1), dtype="int")
    moments = torch.zeros((3, num_pd_steps + 1), dtype=torch.int64, device=device) if want_moments else None
    offs = _split(num_repeats, world)
    for done in range(offs[rank], offs[rank + 1], batch):
        nb = min(batch, offs[rank + 1] - done)
        d_adj, d_ch, d_att = sample(p, seed, done, nb, e, max_attempts, device=device)
        att = d_att.cpu().numpy()                                           # the one read of the batch's attempts
        if (att <= 0).any():
            k = int(np.flatnonzero(att <= 0)[0])
            if att[k] < 0 and path == "wide":
                raise RuntimeError("uncoupled sampler: trial %d: a part of the keys outgrew its room in the wide ranking "
                                   "(status %d)" % (done + k, int(att[k])))
            if att[k] < 0:
                raise RuntimeError("uncoupled sampler: trial %d: sixteen keys met in one bucket of the ranking (status %d)"
                                   % (done + k, int(att[k])))
            raise RuntimeError("uncoupled sampler: trial %d found no simple graph within max_attempts = %d; the expected number "
                               "of attempts of the pair (%d,%d) is about exp((l-1)(r-1)/2) = %.3g"
                               % (done + k, max_attempts, l_deg, r_deg, expected))
        res = E.peel_pick(p, d_adj, d_ch, cpp, num_pd_steps, mt_state=None, seed=seed, trial0=done, want_r1=True)
        if want_moments:
            E.r1_moments(res["r1"], moments)
        else:
            r1_all[done:done + nb] = res["r1"].cpu().numpy()
        o = res["out"].cpu().numpy()
        erased[done:done + nb] = o[:, 0]
        plrs[done:done + nb] = (o[:, 0] - o[:, 1]) / M                      # PD:823-826, 866
    if world > 1:                                           # shares are disjoint: a sum puts them together
        t_plr, t_er = torch.from_numpy(plrs).to(device), torch.from_numpy(erased).to(device)
        dist.all_reduce(t_plr)
        dist.all_reduce(t_er)
        plrs, erased = t_plr.cpu().numpy(), t_er.cpu().numpy()
        if want_moments:
            dist.all_reduce(moments)
        else:
            t_r1 = torch.from_numpy(r1_all).to(device)
            dist.all_reduce(t_r1)
            r1_all = t_r1.cpu().numpy()
    return None, (moments.cpu().numpy() if want_moments else r1_all), plrs, [int(x) for x in erased]


def simulate_peeling_decoder_ldpc_uncoupled(e, l_deg, r_deg, M, num_repeats=None, device=None, rng="numpy", seed=0, batch=None,
                                            want_moments=False, max_attempts=1 << 20):
    """Random-pick peeling on the uncoupled (l,r) ensemble (PD:793-869): returns (None, r1, plrs, num_vns_lst).
    rng="numpy": graphs and channels come from the global numpy stream (ldpc.gen_slots with its repeat rejection, PD:134-135),
    the picks from the global `random` stream; both are left where the reference leaves them.  One trial per launch.
    rng="philox": the same law in throughput mode — engine.sample_philox_uncoupled redraws every trial's graph on the device
    until it is simple (at most max_attempts candidates; a trial that finds none raises RuntimeError), engine.peel_pick
    decodes `batch` trials per launch with Philox picks keyed (seed, trial); results do not depend on batch or on the number of
    ranks.  want_moments=True returns the int64 [3, steps+1] moments (cnt, Σr1, Σr1²) in place of the r1 rows.  Under
    torch.distributed rank r runs a contiguous share of the trials (global trial indices) and one all-reduce puts plrs, the
    erased counts and the moments or rows together, so every rank returns what a single rank would."""
    if rng not in ("numpy", "philox"):
        raise ValueError("rng must be 'numpy' or 'philox'")
    if not 1 <= max_attempts <= UNCOUPLED_MAX_ATTEMPTS:
        raise ValueError("max_attempts must be in [1, 2^24] (got %r)" % (max_attempts,))
    if rng == "philox" and (l_deg * M) % r_deg:
        raise ValueError("rng='philox': l_deg * M must be divisible by r_deg (l_deg=%d, r_deg=%d, M=%d)" % (l_deg, r_deg, M))
    if not num_repeats:
        num_repeats = 100
    if rng == "philox":
        return _uncoupled_philox(e, l_deg, r_deg, M, num_repeats, device, seed, batch, want_moments, max_attempts)
    if _dist()[2] > 1:
        raise ValueError("rng='numpy' replays the reference's one sequential stream: single rank only")
    device = _device(device)
    cpp = int(l_deg / r_deg * M)
    num_pd_steps = int(M * (e + 0.1))                                      # PD:804
    # one CN position of cpp CNs; the device kernels only need CN ids < total_size = cpp (global-id adjacency)
    p = E.CodeParams(l_deg, r_deg, 1, cpp, M)
    r1 = np.zeros((num_repeats, num_pd_steps + 1), dtype="int")
    plrs = np.zeros(num_repeats)
    num_vns_lst = []
    for o in range(num_repeats):
        adj = gen_slots_uncoupled(l_deg, r_deg, M)
        mask = np.random.rand(M) <= e
        d_adj, d_ch = E.to_device(adj[None], E.pack_bits(mask.astype(np.uint8))[None], device)
        st = random.getstate()
        mt = torch.from_numpy(np.array(st[1], dtype=np.uint32).view(np.int32).copy()[None]).to(device)
        res = E.peel_pick(p, d_adj, d_ch, cpp, num_pd_steps, mt_state=mt)
        new = mt.cpu().numpy().view(np.uint32)[0]
        random.setstate((st[0], tuple(int(x) for x in new), st[2]))
        r1[o] = res["r1"][0].cpu().numpy()
        n_users, picked = (int(x) for x in res["out"][0, :2].cpu())
        num_vns_lst.append(n_users)
        plrs[o] = (n_users - picked) / M                                    # PD:823-826, 866
        if r1[o, -1] == 1:
            print("The number of degree-1 CNs at the end of the iterations is 1!!!")
    return None, r1, plrs, num_vns_lst


# ------------------------------------------------------------------------------------------------
# variance reduction (fl_scaling/est_scaling_params.py:42-49, 90-94, 131-138)
# ------------------------------------------------------------------------------------------------
def nu_chunk_from_moments(moments, r1s_theory, M):
    """calc_nu_chunk from the integer moments (cnt, Σr1, Σr1²) of a batch: ssquares[s] = Σ_{r1≠0} (r1/M − θ/M)²,
    counts[s] = cnt[s], over the support of the theory curve.  Equal to the reference's nansum up to float rounding
    (relative 1e-12; the reference sums squared float differences, this sums integers first).  θ is split into its
    nearest integer k and a fraction f: Σ(r1−θ)² = Σ(r1−k)² − 2f·Σ(r1−k) + cnt·f² with the first two sums exact in
    integers, so nothing cancels when the trajectories sit on the theory curve (s2 − 2θ·s1 + cnt·θ² loses five digits
    there)."""
    last = int(np.max(np.where(r1s_theory > 0))) + 1
    th = r1s_theory[r1s_theory > 0].astype(np.float64)
    cnt, s1, s2 = (np.asarray(moments[k])[:last][:r1s_theory.shape[0]].astype(np.int64) for k in range(3))
    k = np.rint(th).astype(np.int64)
    f = th - k
    a = s2 - 2 * k * s1 + cnt * k * k                                       # Σ (r1 − k)²   exact
    b = s1 - cnt * k                                                        # Σ (r1 − k)    exact
    return (a.astype(np.float64) - 2.0 * f * b + cnt * f * f) / (float(M) * float(M)), cnt


def cov_from_gram(gram):
    """(cov float64 [K, K], counts int64 [K, K]) from the integer Gram matrices of simulate_pd_covariance / engine.r1_gram:
    over the trials in which both steps are still decoding (calc_nu_chunk's mask, carried over to pairs; counts = gram[0]),
    cov[i][j] = g2/g0 − (g1[i][j]/g0)·(g1[j][i]/g0), nan where counts == 0.  Nothing cancels: with n = g0, a = g1[i][j],
    b = g1[j][i], s = g2 and the integers ki ≈ a/n, kj ≈ b/n (nu_chunk_from_moments's integer-plus-fraction split, per pair),
    s' = Σ(x_i − ki)(x_j − kj) = s − ki·b − kj·a + n·ki·kj, a' = a − n·ki and b' = b − n·kj are exact in 64-bit integers
    (|s'| <= n·max(x)², below 2⁶³ under simulate_pd_covariance's size check), and cov = (n·s' − a'·b') / n² has an exact integer numerator — formed in
    int64 where it fits, in Python integers where it does not — so trajectories that sit close to a constant lose no digits."""
    g = np.asarray(gram)
    if g.ndim != 3 or g.shape[0] != 3 or g.shape[1] != g.shape[2] or not np.issubdtype(g.dtype, np.integer):
        raise ValueError("gram must be an integer array [3, K, K]")
    g = g.astype(np.int64)
    n, a, b, s = g[0], g[1], g[1].T, g[2]
    ok = n > 0
    n1 = np.where(ok, n, 1)
    ki = np.rint(a / n1).astype(np.int64)
    kj = np.rint(b / n1).astype(np.int64)
    with np.errstate(over="ignore"):
        # wrapping int64 arithmetic: the intermediate products may leave 64 bits, the results do not
        s_ = s - ki * b - kj * a + n * ki * kj
        a_ = a - n * ki
        b_ = b - n * kj
    nf = n1.astype(np.float64)
    fits = np.abs(nf * s_.astype(np.float64)) + np.abs(a_.astype(np.float64) * b_.astype(np.float64)) < 2.0 ** 62
    num = np.where(fits, n * s_ - a_ * b_, 0).astype(np.float64)
    cov = num / (nf * nf)
    for i, j in zip(*np.nonzero(ok & ~fits)):                              # rare: Python integers, correctly rounded division
        nn = int(n[i, j])
        cov[i, j] = (nn * int(s_[i, j]) - int(a_[i, j]) * int(b_[i, j])) / (nn * nn)
    cov[~ok] = np.nan
    return cov, n.copy()


class _ArraysOnly(pickle.Unpickler):
    """The theory file is a pickle of numpy arrays (NB cell 20); nothing else is allowed to load."""
    _OK = {("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
           ("numpy", "ndarray"), ("numpy", "dtype"), ("numpy.core.multiarray", "scalar"),
           ("numpy._core.multiarray", "scalar")}

    def find_class(self, module, name):
        if (module, name) not in self._OK:
            raise pickle.UnpicklingError(f"refusing to load {module}.{name}: theory files hold numpy arrays only")
        return super().find_class(module, name)


def load_theory(path):
    if path.endswith(".npy"):
        return np.load(path)
    with open(path, "rb") as f:
        return np.asarray(_ArraysOnly(f).load()[0])


# ------------------------------------------------------------------------------------------------
# command-line entry points
# ------------------------------------------------------------------------------------------------
_SAFE_CALLS = {"arange": np.arange, "linspace": np.linspace, "range": range, "list": list}


def _safe_eval(text):
    """The reference eval()s its `es` and `doping_points` arguments (PD:1333,1340).  Same inputs accepted —
    numbers, lists/tuples/dicts, arithmetic, np.arange/np.linspace/range — without executing arbitrary code."""
    def ev(node):
        if isinstance(node, ast.Expression):
            return ev(node.body)
        if isinstance(node, ast.Constant) and isinstance(node.value, (int, float)):
            return node.value
        if isinstance(node, (ast.List, ast.Tuple)):
            return [ev(x) for x in node.elts]
        if isinstance(node, ast.Dict):
            return {ev(k): ev(v) for k, v in zip(node.keys, node.values)}
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
            v = ev(node.operand)
            return -v if isinstance(node.op, ast.USub) else v
        if isinstance(node, ast.BinOp) and isinstance(node.op, (ast.Add, ast.Sub, ast.Mult, ast.Div)):
            a, b = ev(node.left), ev(node.right)
            return {ast.Add: a + b, ast.Sub: a - b, ast.Mult: a * b, ast.Div: a / b}[type(node.op)] \
                if not isinstance(node.op, ast.Div) or b != 0 else a / b
        if isinstance(node, ast.Call) and not node.keywords:
            f = node.func
            name = f.attr if isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and f.value.id in ("np", "numpy") \
                else (f.id if isinstance(f, ast.Name) else None)
            if name in _SAFE_CALLS:
                return _SAFE_CALLS[name](*[ev(x) for x in node.args])
        raise ValueError("unsupported expression in argument: " + ast.dump(node)[:80])
    return ev(ast.parse(text, mode="eval"))


def _cli_options(args, kw):
    """The reference's command lines are positional only.  This mirror also takes, anywhere among them,
    `--rng philox|numpy`, `--seed S`, `--batch B`, `--device D` — the keyword arguments of the simulators (throughput mode:
    device sampling, trials sharded over the ranks of a torch.distributed.run job) — `--sweep first|small|wide|auto` and
    `--local-tables on|off|auto` (local_tables=True | False | None), which only ber_sim (simulate_sc_ldpc) takes, and
    `--pick first|multi|auto`, which only simulate_variance (simulate_peeling_decoder_ldpc) and simulate_covariance
    (simulate_pd_covariance) take, `--nbins N`, which only stopping_sets (simulate_sc_ldpc_spectrum) takes, and
    `--eps-fused on|off|auto` (eps_fused=True | False | None), which only ber_sim takes: the whole eps grid from one sampled code
    (simulate_sc_ldpc_curve); auto is what EPS_FUSED_BY_DEFAULT says."""
    kw, pos, it = dict(kw), [], iter(args)
    for x in it:
        if isinstance(x, str) and x == "--local-tables":
            v = next(it)
            if v not in ("on", "off", "auto"):
                raise SystemExit("--local-tables takes on, off or auto (got %r)" % (v,))
            kw["local_tables"] = {"on": True, "off": False, "auto": None}[v]
        elif isinstance(x, str) and x == "--eps-fused":
            v = next(it)
            if v not in ("on", "off", "auto"):
                raise SystemExit("--eps-fused takes on, off or auto (got %r)" % (v,))
            kw["eps_fused"] = {"on": True, "off": False, "auto": None}[v]
        elif isinstance(x, str) and x in ("--rng", "--seed", "--batch", "--device", "--sweep", "--pick", "--nbins"):
            v = next(it)
            if x == "--sweep" and v not in ("first", "small", "wide", "auto"):
                raise SystemExit("--sweep takes first, small, wide or auto (got %r)" % (v,))
            if x == "--pick" and v not in ("first", "multi", "auto"):
                raise SystemExit("--pick takes first, multi or auto (got %r)" % (v,))
            kw[x[2:]] = v if x in ("--rng", "--device", "--sweep", "--pick") else int(v)
        else:
            pos.append(x)
    return pos, kw


def _join_job(kw):
    """Under torch.distributed.run only the throughput mode shards: the reference's own streams (rng="numpy", the default)
    are one sequential sequence, and ranks that each believed to be rank 0 would all write the same output file."""
    import os
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and kw.get("rng") != "philox":
        raise SystemExit("rng='numpy' replays the reference's one sequential numpy / random stream: run it as a single "
                         "process, or pass --rng philox to shard the trials over the %s ranks of this job"
                         % os.environ["WORLD_SIZE"])
    return E.init_distributed() if kw.get("rng") == "philox" else False


def main_simulate_sc_ldpc(argv=None, **kw):
    """ber_sim.py: OUT l r L M "es" T|N U|P B|N TB|NTB num_repeats max_fuckups "doping" (PD:1327-1356)."""
    a, kw = _cli_options(sys.argv if argv is None else [None] + list(argv), kw)
    if "pick" in kw:
        raise SystemExit("--pick chooses the random-pick decoder of simulate_variance (simulate_peeling_decoder_ldpc): ber_sim "
                         "runs the sweep decoder and takes no such option")
    if "nbins" in kw:
        raise SystemExit(_NBINS_ELSEWHERE % "ber_sim")
    joined = _join_job(kw)
    try:
        return _main_simulate_sc_ldpc(a, kw)
    finally:
        if joined:
            import torch.distributed as dist
            dist.destroy_process_group()


_EPS_FUSED_ELSEWHERE = ("--eps-fused walks ber_sim's eps grid on one sampled code (simulate_sc_ldpc_curve): %s takes no such "
                        "option%s")
_NBINS_ELSEWHERE = "--nbins sizes the histogram of stopping_sets (simulate_sc_ldpc_spectrum): %s takes no such option"


def main_stopping_sets(argv=None, **kw):
    """stopping_sets: ber_sim's command line, OUT l r L M "es" T|N U|P B|N TB|NTB num_repeats max_fuckups "doping", and its
    options, plus `--nbins N` (256): for every e the row ber_sim would write goes to OUT, and rank 0 pickles
    (es, hist [E][nbins], pos_hist [E][L'][8]) to OUT + ".spectrum.pkl", numpy arrays only (simulate_sc_ldpc_spectrum)."""
    a, kw = _cli_options(sys.argv if argv is None else [None] + list(argv), kw)
    if "pick" in kw:
        raise SystemExit("--pick chooses the random-pick decoder of simulate_variance (simulate_peeling_decoder_ldpc): "
                         "stopping_sets runs the sweep decoder and takes no such option")
    if "eps_fused" in kw:
        raise SystemExit(_EPS_FUSED_ELSEWHERE % ("stopping_sets", " (the spectrum pass reads the lost bits of simulate_sc_ldpc's "
                                                 "rounds; engine.peel_sweep_eps writes them, the simulator does not pass them on yet)"))
    joined = _join_job(kw)
    try:
        return _main_simulate_sc_ldpc(a, kw, spectrum=True)
    finally:
        if joined:
            import torch.distributed as dist
            dist.destroy_process_group()


class _Tee:
    """Rank 0 writes the table; the other ranks of a job compute the same rows (the counters are all-gathered) and stay silent."""

    def __init__(self, path, active):
        self.f = open(path, "wt") if active else None

    def line(self, *vals):
        if self.f is not None:
            print(*vals, file=self.f)
            print(*vals)
            self.f.flush()
            sys.stdout.flush()

    def close(self):
        if self.f is not None:
            self.f.close()


def _main_simulate_sc_ldpc(a, kw, spectrum=False):
    fname, l, r, L, M = a[1], int(a[2]), int(a[3]), int(a[4]), int(a[5])
    es = _safe_eval(a[6])
    is_terminated, is_protograph = a[7] == "T", a[8] == "P"
    is_bounded, is_tail_biting = a[9] == "B", a[10] == "TB"
    num_repeats, max_fuckups = int(a[11]), int(a[12])
    doping_points = _safe_eval(a[13])
    L += len(doping_points)                                                 # PD:1343
    head = (f"# SC-LDPC ({l},{r},L={L},M={M}) terminated:{is_terminated}, proto:{is_protograph}, bounded:{is_bounded}, "
            f"tail biting:{is_tail_biting}. num_repeats={num_repeats}, max_fuckups={max_fuckups}, "
            f"doping_points={doping_points}.")
    out = _Tee(fname, _dist()[1] == 0)
    es = list(es if isinstance(es, (list, np.ndarray, range)) else [es])
    hists, pos_hists = [], []
    kw = dict(kw)
    fused = kw.pop("eps_fused", None)
    if fused is None:                                                       # absent or auto: only where the fused path applies
        fused = (EPS_FUSED_BY_DEFAULT and not spectrum and kw.get("rng") == "philox" and is_bounded
                 and kw.get("sweep", "auto") in ("auto", "first") and not kw.get("local_tables"))
    try:
        out.line(head)
        if fused:                                                           # the same lines in the same order, from one call
            rows = simulate_sc_ldpc_curve(es, l, r, L, M, is_terminated, is_protograph, is_bounded, is_tail_biting, num_repeats,
                                          max_fuckups, doping_points, **kw)
        for i, e in enumerate(es):
            args = (e, l, r, L, M, is_terminated, is_protograph, is_bounded, is_tail_biting, num_repeats, max_fuckups, doping_points)
            if fused:
                tuple13 = rows[i]
            elif spectrum:
                tuple13, hist, pos_hist = simulate_sc_ldpc_spectrum(*args, **kw)
                hists.append(hist)
                pos_hists.append(pos_hist)
            else:
                tuple13 = simulate_sc_ldpc(*args, **kw)
            ber, ber_truncated, plr, plr_exp, fbl, tbl, fbit, tgen, _flrs, _gens, fblocks, tblocks, bler = tuple13
            out.line(e, ber, ber_truncated, plr, plr_exp, fbl, tbl, fbit, tgen, fblocks, tblocks, bler)
    finally:
        out.close()
    if spectrum and _dist()[1] == 0:                                        # every rank holds the same sums: rank 0 writes
        with open(fname + ".spectrum.pkl", "wb") as f:
            pickle.dump((np.asarray(es, dtype=np.float64), np.stack(hists), np.stack(pos_hists)), f)


def main_simulate_variance(argv=None, **kw):
    """simulate_variance.py: OUT l r L M e T|N U|P num_runs num_runs_batch THEORY (PD:1264-1294): writes
    pickle.dump((ssquares, counts))."""
    a, kw = _cli_options(sys.argv if argv is None else [None] + list(argv), kw)
    if "sweep" in kw:
        raise SystemExit("--sweep chooses the sweep decoder of ber_sim (simulate_sc_ldpc): simulate_variance runs the "
                         "random-pick decoder and takes no such option")
    if "local_tables" in kw:
        raise SystemExit("--local-tables chooses the tables of ber_sim's sweep decoder (simulate_sc_ldpc): simulate_variance runs "
                         "the random-pick decoder and takes no such option")
    if "nbins" in kw:
        raise SystemExit(_NBINS_ELSEWHERE % "simulate_variance")
    if "eps_fused" in kw:
        raise SystemExit(_EPS_FUSED_ELSEWHERE % ("simulate_variance", ""))
    joined = _join_job(kw)
    try:
        return _main_simulate_variance(a, kw)
    finally:
        if joined:
            import torch.distributed as dist
            dist.destroy_process_group()


def _main_simulate_variance(a, kw):
    fname, l, r, L, M, e = a[1], int(a[2]), int(a[3]), int(a[4]), int(a[5]), float(a[6])
    is_terminated, is_protograph = a[7] == "T", a[8] == "P"
    num_runs, num_runs_batch, ftheory = int(a[9]), int(a[10]), a[11]
    r1s_theory = load_theory(ftheory)
    ssquares, counts = None, None
    for i in range(int(num_runs / num_runs_batch)):
        if kw.get("rng", "numpy") == "philox":
            _, mom, _ = simulate_peeling_decoder_ldpc(e, l, r, L, M, is_terminated, is_protograph, num_runs_batch,
                                                      want_moments=True, **dict(kw, seed=kw.get("seed", 0) + i))
        else:
            _, r1s, _ = simulate_peeling_decoder_ldpc(e, l, r, L, M, is_terminated, is_protograph, num_runs_batch, **kw)
            mom = E.r1_moments(torch.from_numpy(r1s.astype(np.int32)).to(_device(kw.get("device")))).cpu().numpy()
        ss, cn = nu_chunk_from_moments(mom, r1s_theory, M)
        ssquares = ss if ssquares is None else ssquares + ss
        counts = cn if counts is None else counts + cn
    if _dist()[1] == 0:                                                     # every rank holds the same sums: rank 0 writes
        with open(fname, "wb") as f:
            pickle.dump((ssquares, counts), f)
    return ssquares, counts


def main_simulate_covariance(argv=None, **kw):
    """simulate_covariance: OUT l r L M e T|N U|P num_runs STRIDE [--seed S --batch B --device D --pick first|multi|auto]:
    simulate_pd_covariance at every STRIDE-th step; rank 0 writes pickle.dump((steps, gram, moments, plrs)), numpy arrays
    only.  Philox mode only, sharded over the ranks of a torch.distributed.run job."""
    a, kw = _cli_options(sys.argv if argv is None else [None] + list(argv), kw)
    if kw.get("rng", "philox") != "philox":
        raise SystemExit("--rng %s: simulate_covariance runs in Philox mode only (the reference's host stream is sequential; its "
                         "rows can be fed to engine.r1_gram by hand)" % kw["rng"])
    if "sweep" in kw:
        raise SystemExit("--sweep chooses the sweep decoder of ber_sim (simulate_sc_ldpc): simulate_covariance runs the "
                         "random-pick decoder and takes no such option")
    if "local_tables" in kw:
        raise SystemExit("--local-tables chooses the tables of ber_sim's sweep decoder (simulate_sc_ldpc): simulate_covariance "
                         "runs the random-pick decoder and takes no such option")
    if "nbins" in kw:
        raise SystemExit(_NBINS_ELSEWHERE % "simulate_covariance")
    if "eps_fused" in kw:
        raise SystemExit(_EPS_FUSED_ELSEWHERE % ("simulate_covariance", ""))
    if len(a) != 11:
        raise SystemExit("simulate_covariance takes OUT l r L M e T|N U|P num_runs STRIDE (got %d arguments)" % (len(a) - 1))
    joined = _join_job(dict(kw, rng="philox"))
    try:
        return _main_simulate_covariance(a, {k: v for k, v in kw.items() if k != "rng"})
    finally:
        if joined:
            import torch.distributed as dist
            dist.destroy_process_group()


def _main_simulate_covariance(a, kw):
    fname, l, r, L, M, e = a[1], int(a[2]), int(a[3]), int(a[4]), int(a[5]), float(a[6])
    is_terminated, is_protograph = a[7] == "T", a[8] == "P"
    num_runs, stride = int(a[9]), int(a[10])
    out = simulate_pd_covariance(e, l, r, L, M, is_terminated, is_protograph, num_runs, stride, **kw)
    if _dist()[1] == 0:                                                     # every rank holds the same sums: rank 0 writes
        with open(fname, "wb") as f:
            pickle.dump(tuple(np.asarray(x) for x in out), f)
    return out


def test_sc_ldpc(l=4, r=8, L=50, M=10000, e=0.48, is_terminated=False, num_runs=100, num_runs_batch=100,
                 out_pattern="r1_sc_ldpc_{l}_{r}_{L}_{M}_{etag}_{term}_{i}.pkl", **kw):
    """`python3 peeling_decoding.py` (PD:1212-1245): batches of trajectories pickled as (r1, plrs)."""
    for i in range(int(num_runs / num_runs_batch)):
        _, r1, plrs = simulate_peeling_decoder_ldpc(e, l, r, L, M, is_terminated, False, num_runs_batch, [], **kw)
        name = out_pattern.format(l=l, r=r, L=L, M=M, etag=("%.3f" % e).replace(".", "")[:4],
                                  term="terminated" if is_terminated else "nonterminated", i=i)
        with open(name, "wb") as f:
            pickle.dump((r1, plrs), f)


if __name__ == "__main__":
    prog = sys.argv[1] if len(sys.argv) > 1 else "test_sc_ldpc"
    if prog == "ber_sim":
        main_simulate_sc_ldpc(sys.argv[2:])
    elif prog == "simulate_variance":
        main_simulate_variance(sys.argv[2:])
    elif prog == "simulate_covariance":
        main_simulate_covariance(sys.argv[2:])
    elif prog == "stopping_sets":
        main_stopping_sets(sys.argv[2:])
    else:
        test_sc_ldpc()
