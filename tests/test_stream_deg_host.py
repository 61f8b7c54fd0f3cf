"""The streaming decoder's shape rule for the VN degrees 3, 4 and 5 on the CPU: scldpc_stream_supported, the state size that
answers through the same function, the (4,8) blob sizes of the build before the degrees were added, and the two decoders of
the streaming oracle against each other at the shapes tests/test_gpu_stream_deg.py compares the kernels with."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from fl_scaling_sc_ldpc_amd import _lib
from fl_scaling_sc_ldpc_amd import engine as E

P = _lib.CodeParams
TOO_LARGE, BAD_ARG = -2, -1

# dv, dc, L, N, W: the shapes of the GPU tests
TAKEN = [(3, 6, 20, 10, 6), (3, 6, 20, 10, 7), (5, 10, 20, 10, 6), (5, 10, 20, 10, 5), (3, 6, 30, 100, 12), (5, 10, 30, 100, 11),
         (5, 10, 30, 100, 10), (3, 9, 30, 99, 10), (5, 15, 30, 99, 8), (3, 6, 50, 1000, 20), (5, 10, 50, 1000, 20),
         (3, 6, 50, 5000, 20), (5, 10, 50, 5000, 20), (4, 8, 20, 10, 6), (4, 8, 50, 1000, 20), (4, 8, 50, 5000, 20)]

# (parameters, W, return code of the entry points, part of the message)
REFUSED = [
    (P(2, 4, 30, 10, 20), 4, TOO_LARGE, "dv = 3, 4 or 5 (dv=2)"),
    (P(6, 12, 30, 10, 20), 4, TOO_LARGE, "dv = 3, 4 or 5 (dv=6)"),
    (P(4, 16, 30, 5, 20), 4, TOO_LARGE, "dc must be at most 15"),
    (P(3, 16, 30, 15, 80), 4, TOO_LARGE, "dc must be at most 15"),
    (P(4, 10, 30, 6554, 16385), 4, TOO_LARGE, "at most 65536 sockets per position (cns_pos * dc = 65540)"),
    (P(5, 10, 30, 6554, 13108), 4, TOO_LARGE, "at most 65536 sockets per position (cns_pos * dc = 65540)"),
    (E.make_params(5, 10, 20, 10), 7, BAD_ARG, "W + dv - 1 <= L/2"),
    (E.make_params(3, 6, 20, 10), 0, BAD_ARG, "need 1 <= W"),
    (E.make_params(5, 10, 9, 10), 1, BAD_ARG, "buffer length L=9 outside [10, 256]"),
    (E.make_params(3, 6, 300, 10), 10, BAD_ARG, "buffer length L=300 outside [6, 256]"),
    (E.make_params(5, 10, 80, 13000), 30, TOO_LARGE, "does not fit the LDS"),
]


def test_library_exports_and_header_declares_the_symbol():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "scldpc.h")).read()
    assert "scldpc_stream_supported" in _lib.EXPORTS and hasattr(L, "scldpc_stream_supported")
    assert re.search(r"\bint\s+scldpc_stream_supported\s*\(\s*const scldpc_code_params \*p,\s*int32_t W\s*\)", hdr)
    assert L.scldpc_abi_version() == 2                                   # an addition only


@pytest.mark.parametrize("dv,dc,L,N,W", TAKEN)
def test_the_predicate_takes_the_three_degrees_and_the_state_has_a_size(dv, dc, L, N, W):
    p = E.make_params(dv, dc, L, N)
    assert _lib.lib().scldpc_stream_supported(C.byref(p), W) == 1 and E.stream_supported(p, W)
    assert _lib.lib().scldpc_stream_state_bytes(C.byref(p), W) > 0


@pytest.mark.parametrize("p,W,rc,part", REFUSED, ids=[re.sub(r"\W+", "_", r[3])[:40] for r in REFUSED])
def test_a_refusal_names_the_limit_and_every_entry_point_agrees(p, W, rc, part):
    L = _lib.lib()
    assert L.scldpc_stream_supported(C.byref(p), W) == 0 and not E.stream_supported(p, W)
    msg = L.scldpc_last_error().decode()
    assert msg.startswith("scldpc_stream_supported: ") and part in msg, msg
    assert L.scldpc_stream_state_bytes(C.byref(p), W) == rc
    assert L.scldpc_last_error().decode() == msg.replace("scldpc_stream_supported", "scldpc_stream_state_bytes")
    # decided before any device work: null buffers are never reached
    assert L.scldpc_stream_run_device(C.byref(p), 1, 0, 0, 0.4, W, 0, None, 1, None, None, None, None) == rc
    assert part in L.scldpc_last_error().decode()
    assert L.scldpc_stream_run_device_inputs(C.byref(p), 1, W, 0, None, 1, None, None, None, C.c_void_p(16), C.c_void_p(16),
                                             200, 0, None) == rc


def test_null_parameters_are_refused():
    assert _lib.lib().scldpc_stream_supported(None, 4) == 0
    assert "null scldpc_code_params" in _lib.lib().scldpc_last_error().decode()


# scldpc_stream_state_bytes of the build before dv = 3 and 5 were taken (recorded from it): a saved dv = 4 state continues
@pytest.mark.parametrize("L,N,W,nbytes", [(20, 10, 6, 7168), (50, 1000, 20, 920064), (50, 5000, 20, 4595200)])
def test_the_4_8_blob_keeps_its_size(L, N, W, nbytes):
    p = E.make_params(4, 8, L, N)
    assert _lib.lib().scldpc_stream_state_bytes(C.byref(p), W) == nbytes


@pytest.mark.parametrize("dv,dc,L,N,eps,W,doped,npos", [
    (3, 6, 20, 10, 0.42, 6, (), 135), (3, 6, 20, 10, 0.45, 7, (5, 6), 150), (5, 10, 20, 10, 0.45, 6, (), 135),
    (5, 10, 20, 10, 0.47, 5, (7, 8, 9, 10), 150), (3, 6, 30, 100, 0.46, 12, (10, 11), 100),
    (5, 10, 30, 100, 0.48, 11, (9, 10, 11, 12), 100), (5, 10, 30, 100, 0.46, 10, (), 100), (3, 9, 30, 99, 0.28, 10, (7, 8), 85),
    (5, 15, 30, 99, 0.30, 8, (), 85),
    # buffers in which the reference re-uses CN rows before it expurgates (one or two of the dv positions)
    (5, 10, 24, 10, 0.45, 6, (), 135), (5, 10, 22, 10, 0.45, 6, (7, 8, 9, 10), 135), (4, 8, 18, 10, 0.45, 5, (), 135),
    (3, 6, 12, 10, 0.42, 4, (), 135)])
def test_the_two_oracle_decoders_agree_at_the_gpu_test_shapes(oracle, dv, dc, L, N, eps, W, doped, npos):
    """The literal message decoder and the node-level model on the Philox-keyed stream 5 of seed 17: the reference of the GPU
    tests, pinned from both sides."""
    p = E.make_params(dv, dc, L, N)
    po = oracle.Params(dv, dc, L, p.cns_pos, p.vns_pos)
    a = oracle.Stream(po, 17, eps, W, doped, rng_mode=1, decoder=0, sid=5)
    b = oracle.Stream(po, 17, eps, W, doped, rng_mode=1, decoder=1, sid=5)
    for k in range(npos):
        assert a.step() == b.step(), k
