"""The LDS carve and the launch front of the first-generation flooding decoders (csrc/flood_common.h), pinned through the public
calls that expose them — pure host arithmetic, no device.  full_bp, sw_bp and peel_sweep choose between 16-bit CN words, 32-bit
words in LDS and 32-bit words in a caller-owned workspace by what fits the 160 KiB of LDS; the table below holds what the library
answered before the three launchers shared one carve, on a grid that straddles every flip for (3,6), (4,8) and (5,10):
  * dv * vns_pos around 4096 (the 16-bit words end; it shows in the LDS bytes),
  * (4,8), vns_pos = 1024: L = 58 / 59 (trajectory rows: the side array of boundary degrees stops fitting queue 1 — both sides
    answer 0 bytes of workspace, the 32-bit words still fit), L = 61 / 62 (the packed layout's queues drop below 256 entries),
    L = 67 .. 70 (the 32-bit words leave the LDS: first peel_sweep with 4-byte rows, then full_bp; sw_bp stays packed),
  * the largest vns_pos whose 32-bit words fit the LDS and the first that goes to the workspace, for each of the three kernels
    (peel_sweep keeps a second bitmap, sw_bp accepts shorter queues),
  * the sizes at which the bitmaps alone no longer fit (-2), and one shape refused for dc * n >= 2^24."""
import ctypes as C

import pytest

WS_FULL_BP, WS_SW_BP, WS_PEEL_SWEEP = 1, 2, 3                          # SCLDPC_WS_*
T, W = 3, 3

# (dv, dc, L, vns_pos): (scldpc_full_bp_lds_bytes, workspace of full_bp without rows, with rows, sw_bp, peel_sweep 4-byte rows,
#                        peel_sweep 2-byte rows), for T trials
CARVE = [
    ((3, 6, 14, 1364), (80896, 0, 0, 0, 0, 0)),
    ((3, 6, 14, 1366), (113216, 0, 0, 0, 0, 0)),
    ((3, 6, 6, 9108), (163840, 0, 0, 0, 0, 0)),
    ((3, 6, 6, 9110), (163824, 0, 0, 0, 437280, 437280)),
    ((3, 6, 6, 9370), (163824, 0, 0, 0, 449760, 449760)),
    ((3, 6, 6, 9372), (77392, 449856, 449856, 0, 449856, 449856)),
    ((3, 6, 6, 9460), (77504, 454080, 454080, 0, 454080, 454080)),
    ((3, 6, 6, 9462), (77504, 454176, 454176, 454176, 454176, 454176)),
    ((4, 8, 9, 1024), (79904, 0, 0, 0, 0, 0)),
    ((4, 8, 9, 1026), (92272, 0, 0, 0, 0, 0)),
    ((4, 8, 5, 9172), (163840, 0, 0, 0, 0, 0)),
    ((4, 8, 5, 9174), (163840, 0, 0, 0, 440352, 440352)),
    ((4, 8, 5, 9440), (163840, 0, 0, 0, 453120, 453120)),
    ((4, 8, 5, 9442), (76304, 453216, 453216, 0, 453216, 453216)),
    ((4, 8, 5, 9528), (76400, 457344, 457344, 0, 457344, 457344)),
    ((4, 8, 5, 9530), (76400, 457440, 457440, 457440, 457440, 457440)),
    ((4, 8, 58, 1024), (80896, 0, 0, 0, 0, 0)),
    ((4, 8, 59, 1024), (80896, 0, 0, 0, 0, 0)),
    ((4, 8, 61, 1024), (80896, 0, 0, 0, 0, 0)),
    ((4, 8, 62, 1024), (163840, 0, 0, 0, 0, 0)),
    ((4, 8, 67, 1024), (163840, 0, 0, 0, 0, 0)),
    ((4, 8, 68, 1024), (163840, 0, 0, 0, 436224, 0)),
    ((4, 8, 69, 1024), (163840, 0, 0, 0, 442368, 0)),
    ((4, 8, 70, 1024), (79808, 448512, 448512, 0, 448512, 0)),
    ((4, 8, 50, 12544), (163824, 3988992, 3988992, 3988992, 3988992, 3988992)),
    ((4, 8, 50, 12546), (163824, 3989628, 3989628, 3989628, -2, -2)),
    ((4, 8, 50, 16866), (163824, 5363388, 5363388, 5363388, -2, -2)),
    ((4, 8, 50, 16868), (170964, -2, -2, 5364024, -2, -2)),
    ((4, 8, 50, 17028), (171964, -2, -2, 5414904, -2, -2)),
    ((4, 8, 50, 17030), (171976, -2, -2, -2, -2, -2)),
    ((4, 8, 50, 42000), (328036, -2, -2, -2, -2, -2)),
    ((5, 10, 4, 818), (73008, 0, 0, 0, 0, 0)),
    ((5, 10, 4, 820), (79584, 0, 0, 0, 0, 0)),
    ((5, 10, 4, 9238), (163840, 0, 0, 0, 0, 0)),
    ((5, 10, 4, 9240), (163840, 0, 0, 0, 443520, 443520)),
    ((5, 10, 4, 9510), (163840, 0, 0, 0, 456480, 456480)),
    ((5, 10, 4, 9512), (75168, 456576, 456576, 0, 456576, 456576)),
    ((5, 10, 4, 9600), (75232, 460800, 460800, 0, 460800, 460800)),
    ((5, 10, 4, 9602), (75264, 460896, 460896, 460896, 460896, 460896)),
]


@pytest.fixture(scope="module")
def L():
    from fl_scaling_sc_ldpc_amd import _lib
    return _lib.lib()


def _params(shape):
    from fl_scaling_sc_ldpc_amd import _lib
    dv, dc, Lc, N = shape
    return _lib.CodeParams(dv, dc, Lc, N * dv // dc, N)


@pytest.mark.parametrize("shape,want", CARVE, ids=["%d_%d_L%d_N%d" % s for s, _ in CARVE])
def test_carve_is_what_it_was(L, shape, want):
    r = C.byref(_params(shape))
    got = (L.scldpc_full_bp_lds_bytes(r), L.scldpc_workspace_bytes(WS_FULL_BP, r, T, 0, 0),
           L.scldpc_workspace_bytes(WS_FULL_BP, r, T, 1, 0), L.scldpc_workspace_bytes(WS_SW_BP, r, T, W, 0),
           L.scldpc_workspace_bytes(WS_PEEL_SWEEP, r, T, 0, 0), L.scldpc_workspace_bytes(WS_PEEL_SWEEP, r, T, 1, 0))
    assert got == want


def test_workspace_is_one_word_per_cn_and_trial(L):
    for shape, want in CARVE:
        p = _params(shape)
        assert all(w in (0, -2, T * p.nk * 4) for w in want[1:]), shape


def test_refusals_name_their_entry_point(L):
    err = lambda: L.scldpc_last_error().decode()
    too_long = C.byref(_params((4, 8, 50, 42000)))                      # dc * n = 16.8e6 >= 2^24
    assert L.scldpc_workspace_bytes(WS_FULL_BP, too_long, T, 0, 0) == -2
    assert err() == "scldpc_full_bp_device: needs dc <= 15, dv <= 8, dc*n < 2^24 (got dc=8 dv=4 n=2100000)"
    assert L.scldpc_workspace_bytes(WS_SW_BP, too_long, T, W, 0) == -2
    assert err() == "scldpc_sw_bp_device: needs dc <= 15, dv <= 8, dc*n < 2^24"
    assert L.scldpc_workspace_bytes(WS_PEEL_SWEEP, too_long, T, 1, 0) == -2
    assert err() == "scldpc_peel_sweep_device: needs dc <= 15, dv <= 8, dc*n < 2^24"
    big = _params((4, 8, 50, 17030))                                    # the bitmaps alone exceed the LDS
    assert L.scldpc_workspace_bytes(WS_FULL_BP, C.byref(big), T, 0, 0) == -2
    assert err() == "scldpc_full_bp_device: n=%d VN bits + nk=%d scan bits do not fit 160 KiB of LDS" % (big.n, big.nk)
    assert L.scldpc_workspace_bytes(WS_SW_BP, C.byref(big), T, W, 0) == -2
    assert err() == "scldpc_sw_bp_device: n=%d VN bits + nk=%d scan bits do not fit 160 KiB of LDS" % (big.n, big.nk)
    assert L.scldpc_workspace_bytes(WS_PEEL_SWEEP, C.byref(big), T, 1, 0) == -2
    assert err() == "scldpc_peel_sweep_device: %d VN bits + %d scan bits do not fit 160 KiB of LDS" % (big.n, big.nk)
    assert L.scldpc_workspace_bytes(WS_SW_BP, C.byref(big), T, 0, 0) == -1
    assert err() == "scldpc_sw_bp_device: need W >= 1, max_it >= 0, init_it >= 0"
    # null buffers and bad arguments, in the order the launchers test them
    ok, odd = C.byref(_params((4, 8, 50, 1000))), C.byref(_params((3, 6, 20, 200)))
    assert L.scldpc_full_bp_device(ok, 1, None, None, 0, 1, None, None, 0, None, None, 0, None) == -1
    assert err() == "scldpc_full_bp_device: null buffer or negative ntrials"
    assert L.scldpc_full_bp_device(ok, 0, None, None, 0, 1, None, C.c_void_p(16), 0, None, None, 0, None) == -1
    assert err() == "scldpc_full_bp_device: d_rows given but rows_cap <= 0"
    assert L.scldpc_full_bp_fixpoint_device(ok, 1, None, None, 1, None, None, None, 0, None) == -1
    assert err() == "scldpc_full_bp_fixpoint_device: null buffer or negative ntrials"
    assert L.scldpc_full_bp_fixpoint_device(ok, 0, None, None, 1, None, None, None, 0, None) == 0
    assert L.scldpc_full_bp_fixpoint_device_adj16(odd, -1, None, None, 1, None, None, None, 0, None) == -1    # dv = 3: the level kernel
    assert err() == "scldpc_full_bp_device: null buffer or negative ntrials"
    assert L.scldpc_sw_bp_device(ok, 1, None, None, W, 1, 1, None, None, None, 0, None) == -1
    assert err() == "scldpc_sw_bp_device: null buffer or negative ntrials"
    assert L.scldpc_swc_bp_device_adj16(ok, 0, None, None, 0, 1, None, None, None, 0, None) == -1
    assert err() == "scldpc_sw_bp_device: need W >= 1, max_it >= 0, init_it >= 0"
    assert L.scldpc_peel_sweep_device(ok, 1, None, None, 0, 0, 0, 0, None, None, None, 0, None) == -1
    assert err() == "scldpc_peel_sweep_device: null buffer or negative ntrials"
    assert L.scldpc_peel_sweep_device_adj16(ok, 0, None, None, 53 * 500 + 1, 0, 0, 0, None, None, None, 0, None) == -1
    assert err() == "scldpc_peel_sweep_device: CN ranges outside [0,%d]" % (53 * 500)
    assert L.scldpc_peel_sweep_device(ok, 0, None, None, 0, 0, 0, 0, None, None, None, 0, None) == 0
