"""Poisoned buffers and red zones for the buffer-contract tests (a plain helper module; works on CPU and device tensors).

An Arena stands in for engine._uninit: every output and workspace a wrapper allocates comes out of it with a guard on either
side — GUARD bytes, or one slice along dim 0 rounded up to a multiple of GUARD where that is more, so that a store one whole
trial past the end (or before the start) lands in it — filled with GUARD_BYTE, and an interior filled according to the mode:

  0xFF   a CN word reads cnt = 15, a 4-bit count reads 15, a flag reads as set, an int32 reads -1
  0x5A   a second pattern with both bit values in every nibble
  stale  the interior handed out for the same byte size before the last recycle(), exactly as that call left it
         (a size met for the first time is filled with 0xFF)

check_guards() — after a device synchronise — raises GuardError naming the allocation if a guard byte changed.  The
*_defined helpers say which elements of an output the contract of include/scldpc.h ("Buffers") defines."""
import numpy as np
import torch

GUARD = 512                     # guards are multiples of 512: the interior keeps the 256-byte alignment the workspaces need
GUARD_BYTE = 0xC3
MODES = (0xFF, 0x5A, "stale")


class GuardError(AssertionError):
    pass


def _device_key(device):
    return str(torch.empty(0, dtype=torch.uint8, device=device).device)            # "cuda" and "cuda:0" are one device


def guard_bytes(shape, nbytes):
    """GUARD, or one slice along dim 0 (a trial's row of the output) rounded up to a multiple of GUARD where that is more."""
    per_slice = nbytes // shape[0] if len(shape) > 1 and shape[0] > 0 else 0
    return max(GUARD, -(-per_slice // GUARD) * GUARD)


class _Alloc:
    def __init__(self, order, raw, nbytes, shape, dtype, guard):
        self.order, self.raw, self.nbytes, self.shape, self.dtype, self.guard = order, raw, nbytes, shape, dtype, guard

    def interior(self):
        return self.raw[self.guard:self.guard + self.nbytes]

    def describe(self):
        return "allocation #%d (%d bytes, shape %s, %s)" % (self.order, self.nbytes, tuple(self.shape), self.dtype)


class Arena:
    def __init__(self, mode):
        assert mode in MODES, mode
        self.mode = mode
        self.records = []               # every allocation since the last recycle(), in order
        self._pool = {}                 # stale mode: (nbytes, guard, device) -> raw buffers of the previous call
        self.total = 0

    def __call__(self, shape, dtype=torch.uint8, device=None):
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * item
        guard = guard_bytes(shape, nbytes)
        key = (nbytes, guard, _device_key(device))
        raw = None
        if self.mode == "stale" and self._pool.get(key):
            raw = self._pool[key].pop(0)                                    # interior left as the previous call left it
        if raw is None:
            raw = torch.empty(guard + nbytes + guard, dtype=torch.uint8, device=device)
            raw[guard:guard + nbytes] = 0xFF if self.mode == "stale" else self.mode
        raw[:guard] = GUARD_BYTE
        raw[guard + nbytes:] = GUARD_BYTE
        rec = _Alloc(self.total, raw, nbytes, shape, dtype, guard)
        self.total += 1
        self.records.append(rec)
        return rec.interior().view(dtype).view(shape)

    def poison_value(self, dtype):
        """What an untouched element of this arena reads as (0xFF / 0x5A modes)."""
        assert self.mode != "stale"
        return torch.full((torch.empty((), dtype=dtype).element_size(),), self.mode, dtype=torch.uint8).view(dtype)[0].item()

    def check_guards(self):
        for rec in self.records:
            for side, g in (("before the start", rec.raw[:rec.guard]), ("past the end", rec.raw[rec.guard + rec.nbytes:])):
                bad = torch.nonzero(g != GUARD_BYTE)
                if bad.numel():
                    k = int(bad[-1 if side == "before the start" else 0].item())
                    dist = rec.guard - k if side == "before the start" else k + 1
                    raise GuardError("%s: guard byte changed %d byte(s) %s (%d guard bytes changed on that side)"
                                     % (rec.describe(), dist, side, bad.numel()))

    def recycle(self):
        """End of a call: what it allocated becomes the stale content of the next call's allocations of the same size."""
        if self.mode == "stale":
            for rec in self.records:
                key = (rec.nbytes, rec.guard, str(rec.raw.device))
                self._pool.setdefault(key, []).append(rec.raw)
        self.records = []


# ---- which elements the contract defines ---------------------------------------------------------------------------------
def padding_mask(n):
    """uint32 mask of the padding bits of the last word of an n-bit bitmap (0 when n is a multiple of 32)."""
    return np.uint32(0) if n % 32 == 0 else np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)


def bitmap_expected(bits):
    """uint8 [.., n] -> the uint32 words [.., ceil(n/32)] an output bitmap (d_erased_bits, d_lost_bits) must hold: every word
    is defined and the padding bits of the last word are 0."""
    bits = np.asarray(bits, dtype=np.uint8)
    pad = (-bits.shape[-1]) % 32
    if pad:
        bits = np.concatenate([bits, np.zeros(bits.shape[:-1] + (pad,), np.uint8)], axis=-1)
    return np.packbits(bits, axis=-1, bitorder="little").view(np.uint32)


def rows_defined(iterations, rows_cap):
    """bool [T, rows_cap, 3]: d_rows[t, :min(iterations[t], rows_cap)] is defined, nothing beyond."""
    it = np.minimum(np.asarray(iterations, dtype=np.int64), rows_cap)
    return np.broadcast_to((np.arange(rows_cap)[None, :] < it[:, None])[:, :, None], (len(it), rows_cap, 3)).copy()


def r1_defined(T, num_steps):
    """bool [T, num_steps + 1]: every element of d_r1[:, :num_steps + 1] is defined (steps without a degree-1 CN repeat
    the previous value)."""
    return np.ones((T, num_steps + 1), dtype=bool)


def all_defined(shape):
    """counters, out, sampler tables, the trace of a streaming call: every element."""
    return np.ones(shape, dtype=bool)


def assert_defined_equal(what, got, want, mask=None):
    """got == want on every defined element; names the first mismatch."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ne = got != want
    if mask is not None:
        ne &= np.asarray(mask, dtype=bool)
    if ne.any():
        k = tuple(int(x) for x in np.argwhere(ne)[0])
        raise AssertionError("%s: %d defined element(s) differ, first at %s: got %s, want %s"
                             % (what, int(ne.sum()), k, got[k], want[k]))
