"""Which kernel instance the eps-grid and threshold decoders take, on the CPU: peel_sweep_eps, full_bp_eps, frame_threshold and
vn_threshold pick one of CN-word policy (16-bit Packed, 32-bit Wide in LDS, 32-bit WideG in the workspace) x adjacency width
(2-byte position-local rows, 4-byte global rows) x the dv = 4 or the generic-dv code, and which one a shape takes is host
arithmetic: the four *_workspace_query entries (0: the CN words stay in LDS; T * 4 * nk: they go to the workspace) and the
Packed rule, 2-byte rows and dv * vns_pos <= 4096.  The table below holds, for each of (4,8), (3,6) and (5,10) at L = 6, the
last N on the Packed side of the rule, the first N past it, and the smallest even N whose CN words leave the LDS; every entry is
asserted, with the N - 2 neighbours of the workspace shapes, so that a shape of tests/test_gpu_eps_forms.py that moved to
another rung fails here, without a device.  The two production paths this file protects are the shipped shapes whose forms no
other test runs: (5,10), L = 50, N = 1000 — Wide x 2-byte rows x generic dv, dv * N = 5000 — and (4,8), L = 50, N = 5000 —
WideG x 2-byte rows x dv = 4, bp_traj's shipped size."""
import ctypes as C
import os

import pytest

from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc")
QUERIES = {"peel_sweep_eps": "scldpc_peel_sweep_eps_workspace_query", "full_bp_eps": "scldpc_full_bp_eps_workspace_query",
           "frame_threshold": "scldpc_frame_threshold_workspace_query", "vn_threshold": "scldpc_vn_threshold_workspace_query"}
PACK_LIMIT = 4096

# (dv, dc, L, N) -> dv * N
WIDE = {(4, 8, 6, 1026): 4104, (3, 6, 6, 1366): 4098, (5, 10, 6, 820): 4100}          # the first N past the Packed rule
PACKED = {(4, 8, 6, 1024): 4096, (3, 6, 6, 1364): 4092, (5, 10, 6, 818): 4090}        # the last N on its Packed side
# (dv, dc, L, N) -> (n, nk): the smallest even N at which peel_sweep_eps, full_bp_eps and frame_threshold go to the workspace
WIDE_G = {(4, 8, 6, 8044): (48264, 36198), (3, 6, 6, 8966): (53796, 35864), (5, 10, 6, 7296): (43776, 36480)}
# ... and vn_threshold, whose LDS carve is its own (csrc/vn_threshold.hip, the floor it gives pos_b: the grid, the count differences
# and the candidate list where the siblings keep R and the level counts): the same N at (4,8) and (3,6), earlier at (5,10)
VN_FIRST_WIDE_G = {(4, 8, 6): 8044, (3, 6, 6): 8966, (5, 10, 6): 7276}
SHIPPED_WIDE = (5, 10, 50, 1000)
SHIPPED_WIDE_G = (4, 8, 50, 5000)


def query(kernel, shape, T, adj16):
    p = E.make_params(*shape)
    return getattr(_lib.lib(), QUERIES[kernel])(C.byref(p), T, 1 if adj16 else 0)


def form(shape, adj16, kernel="full_bp_eps"):
    """The instance a shape takes, as the host decides it: (policy, rows, dv code)."""
    dv, N = shape[0], shape[3]
    nbytes = query(kernel, shape, 1, adj16)
    assert nbytes >= 0, (kernel, shape, _lib.lib().scldpc_last_error().decode())
    policy = "WideG" if nbytes else "Packed" if adj16 and dv * N <= PACK_LIMIT else "Wide"
    return policy, "A16" if adj16 else "int32", "DV4" if dv == 4 else "generic"


def test_the_packed_rule_is_the_one_the_launches_apply():
    """The arithmetic of this file is the launches': 2-byte rows and dv * vns_pos <= 4096, once, in the front that chooses the
    words of the four kernels (walk_launch, eps_stages.h), which every launch goes through and none repeats."""
    rule = "adj16 && (int64_t)p->dv * p->vns_pos <= %d, carve" % PACK_LIMIT
    assert open(os.path.join(CSRC, "eps_stages.h")).read().count(rule) == 1
    for name in ("eps_stages.h", "frame_threshold.hip", "vn_threshold.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert text.count("walk_launch<") == 1, name
        assert name == "eps_stages.h" or "flood_choose_words" not in text, name
    for name in ("peel_sweep_eps.hip", "full_bp_eps.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert text.count("eps_walk_launch<") == 1 and "flood_choose_words" not in text, name


@pytest.mark.parametrize("shape", list(WIDE), ids=lambda s: "%d_%d_L%d_N%d" % s)
def test_wide_words_in_lds(shape):
    dv, dc, L, N = shape
    p = E.make_params(*shape)
    assert dv * N == WIDE[shape] > PACK_LIMIT and p.vns_pos == N and p.cns_pos <= 65536
    for kernel in QUERIES:
        for adj16 in (True, False):
            for T in (1, 8):
                assert query(kernel, shape, T, adj16) == 0, (kernel, adj16, T)
            assert form(shape, adj16, kernel) == ("Wide", "A16" if adj16 else "int32", "DV4" if dv == 4 else "generic")


@pytest.mark.parametrize("shape", list(PACKED), ids=lambda s: "%d_%d_L%d_N%d" % s)
def test_the_packed_twins(shape):
    dv, dc, L, N = shape
    twin = (dv, dc, L, N + 2)
    assert dv * N == PACKED[shape] <= PACK_LIMIT < dv * (N + 2) and twin in WIDE      # the last even N on the Packed side
    for kernel in QUERIES:
        for adj16 in (True, False):
            assert query(kernel, shape, 8, adj16) == 0, (kernel, adj16)
        assert form(shape, True, kernel)[0] == "Packed"
        assert form(shape, False, kernel)[0] == "Wide"                   # 4-byte rows never pack
        assert form(twin, True, kernel)[0] == "Wide"


@pytest.mark.parametrize("shape", list(WIDE_G), ids=lambda s: "%d_%d_L%d_N%d" % s)
def test_wide_words_in_the_workspace(shape):
    dv, dc, L, N = shape
    p = E.make_params(*shape)
    assert (p.n, p.nk) == WIDE_G[shape] and p.cns_pos <= 65536 and dc * p.n < 1 << 24
    below = (dv, dc, L, N - 2)
    for kernel in QUERIES:
        for adj16 in (True, False):
            for T in (1, 3):
                assert query(kernel, shape, T, adj16) == T * 4 * p.nk, (kernel, adj16, T)
            assert form(shape, adj16, kernel) == ("WideG", "A16" if adj16 else "int32", "DV4" if dv == 4 else "generic")
            if kernel != "vn_threshold":                                 # the smallest even N in the workspace at L = 6
                assert query(kernel, below, 3, adj16) == 0, (kernel, adj16)
    # vn_threshold's own boundary
    first = VN_FIRST_WIDE_G[dv, dc, L]
    assert first <= N
    for adj16 in (True, False):
        for M in range(first, N + 1, 2):
            pm = E.make_params(dv, dc, L, M)
            assert query("vn_threshold", (dv, dc, L, M), 3, adj16) == 3 * 4 * pm.nk, (M, adj16)
        assert query("vn_threshold", (dv, dc, L, first - 2), 3, adj16) == 0, adj16
    if (dv, dc) == (5, 10):
        assert first == 7276 < N                                         # ... differs from its siblings' here, and only here
    else:
        assert first == N


def test_the_workspace_shapes_are_the_smallest_even_ones():
    """Found with the query, not with the rule: the first even N that answers non-zero, searched from 1000 N below."""
    for (dv, dc, L, N) in WIDE_G:
        for kernel in ("peel_sweep_eps", "full_bp_eps", "frame_threshold"):
            found = next(M for M in range(N - 1000, N + 1000, 2) if query(kernel, (dv, dc, L, M), 1, True))
            assert found == N, (kernel, dv, dc, found)
        found = next(M for M in range(N - 1000, N + 1000, 2) if query("vn_threshold", (dv, dc, L, M), 1, True))
        assert found == VN_FIRST_WIDE_G[dv, dc, L]


def test_the_shipped_shapes():
    """What production runs (the drivers set adj16 = cns_pos <= 65536, so always the 2-byte rows)."""
    from fl_scaling_sc_ldpc_amd import bp_decoding as BP
    src = open(os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "bp_decoding.py")).read()
    assert src.count("adj16 = p.cns_pos <= 65536") == 1                  # the code buffers of the rounds the three drivers share
    assert src.count("rounds = _CodeRounds(p, ") == 3                     # run_grid_fused, run_thresholds, run_vn_thresholds
    for kernel in QUERIES:
        assert form(SHIPPED_WIDE, True, kernel) == ("Wide", "A16", "generic"), kernel
        assert form(SHIPPED_WIDE_G, True, kernel) == ("WideG", "A16", "DV4"), kernel
        for T in (1, 5):
            assert query(kernel, SHIPPED_WIDE, T, True) == 0
            assert query(kernel, SHIPPED_WIDE_G, T, True) == T * 4 * E.make_params(*SHIPPED_WIDE_G).nk == T * 4 * 132500
        for pair in ((4, 8), (3, 6)):                                     # the other two pairs at N = 1000 pack
            assert form(pair + (50, 1000), True, kernel)[0] == "Packed"
    assert SHIPPED_WIDE[0] * SHIPPED_WIDE[3] == 5000 > PACK_LIMIT
    for shape in (SHIPPED_WIDE, SHIPPED_WIDE_G):
        assert E.make_params(*shape).cns_pos <= 65536
