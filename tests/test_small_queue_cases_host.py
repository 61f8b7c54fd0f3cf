"""tests/test_gpu_small_queue_forms.py without a GPU: its form table is kernel_of()'s list of non-persistent instances, and the
conditions on its inputs — which queue branches a forced capacity must reach — hold on the reference alone for every overflow
case and fail for the control (tests/small_queue_cases.py)."""
import pytest

import small_queue_cases as S


def test_the_form_table_is_kernel_ofs_list_of_non_persistent_instances():
    keys = S.kernel_of_keys()
    assert len(keys) == 25 and len(set(keys)) == 25                      # twelve (4,8) instances less the two persistent, 5 + 5 + 5
    assert len(set(S.FORMS)) == len(S.FORMS) and sorted(S.FORMS) == sorted(keys)


def test_the_carve_in_host_arithmetic_gives_the_known_capacities():
    from fl_scaling_sc_ldpc_amd import engine as E
    assert S.natural_qcap(E.make_params(4, 8, 50, 5000), "level", True) == 6092      # tests/test_gpu_wide.py
    assert S.natural_qcap(E.make_params(4, 8, 50, 1000), "fix", False) == 720        # seven trials per CU
    assert S.natural_qcap(E.make_params(4, 8, 50, 1000), "level", False) == 864      # six per CU: the snapshot bytes cost one
    for pair in S.PAIRS:
        for size in S.SIZES:
            p = S.params(pair, size)
            for mode in S.MODES:
                assert S.natural_qcap(p, mode, False) > 4000 and S.natural_qcap(p, mode, True) > 19000
                assert max(q for q in S.QCAPS[size] if q) < 4000         # every forced capacity shrinks the queues


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("size,qcap", [(size, q) for size in S.SIZES for q in S.QCAPS[size]],
                         ids=lambda v: v if isinstance(v, str) else "q%s" % ("full" if v is None else v))
@pytest.mark.parametrize("pair", S.PAIRS, ids=lambda pr: "dv%d-dc%d" % pr)
def test_the_inputs_reach_the_branches_they_are_meant_for(pair, size, qcap, wide):
    held = S.check_conditions(pair, size, qcap, "level", wide)
    if qcap is not None:                                                 # every condition is met somewhere, and high eps stops at once
        for name in S.EXPECT[size, qcap]:
            assert any(h[name] for h in held.values()), name
    for eps in S.EPS_OF[size]:
        for is_term in (True, False):
            ref = S.case(pair, size, eps).ref[is_term]
            if eps == S.EPS[-1]:
                assert (ref.counters[:, 0] > 0).all()                    # above threshold: every trial fails
            if eps == S.EPS[0] and is_term:
                assert (ref.counters[:, 0] == 0).all() and (ref.counters[:, 5] <= 2).all()


def test_the_tiny_private_half_queue_is_below_64_and_the_mid_one_is_exactly_64():
    """The fixpoint form lets its waves go private only with half-queues of at least 64 entries: (qcap / 4 & ~1) / 2."""
    half = lambda q: ((q // 4) & ~1) // 2
    assert all(half(q) < 64 for q in S.QCAPS["tiny"] if q) and [half(q) for q in S.QCAPS["mid"] + S.QCAPS["priv"]] == [64, 64]
