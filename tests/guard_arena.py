"""A guard arena: buffers for a call under test, each with a band of known bytes on either side, all inside ONE allocation.  No
tests and no GPU code here: tests/guard_cases.py holds the calls, tests/test_guard_bands.py walks them and holds the controls.

Why.  The suite pins values; it says little about where a kernel touches memory.  torch's caching allocator rounds every
allocation up to 512 bytes and packs small ones into shared blocks, so a store a few elements past a tensor lands in slack or in
another live tensor and every parity test still passes.  A buffer carved here has ``band_bytes`` of this allocation on both sides:
a store that strays less than a band from the buffer is legal memory, faults nothing, and is seen by ``check()``.

``GuardArena(device, band_bytes=65536)`` works on "cpu" and "cuda" alike (``pinned=True``: page-locked host memory, for the host
pointers of calls that read or write them from the device).  ``carve(shape, dtype, skew_bytes, kind, name)`` returns a contiguous
view whose ``data_ptr() % 16 == skew_bytes``, with the bands adjoining it:

  kind "in"    bands of NaN bit patterns of the buffer's dtype, laid on the buffer's own element grid: an element read from
               beyond either end and used makes the result differ from the same call on plain tensors.  (Integer dtypes have no
               NaN: all-ones bytes, i.e. -1 / 255 -- an index outside every buffer, a label that is no state.)  ``data`` is copied in.
  kind "out"   bands of BAND_BYTE; the buffer itself is prefilled with FILL_BYTE in every byte -- a NaN of every float type, -1 of
  kind "work"  every integer -- so that an element the call never wrote differs from the reference (``same_bits`` says so).

``check()`` asserts that every band still holds its pattern and names, for each damaged one, the buffer, the side and the first and
last damaged byte relative to the buffer's edge (low side: -1 is the byte just below the buffer; high side: 0 is the byte just
past its end).

The band is a condition, not a measurement: 64 KiB is wider than any unit a kernel of this library stores at once (a 64-frame tile
of 48 columns is 12 KiB, a z-score block's stride 4 KiB), so a wild store that stays within one unit of an edge lands in a band.
Do not shrink it to save memory: a whole case needs a few MiB."""
import numpy as np
import torch

BAND_BYTES = 65536
BAND_BYTE = 0xA5                                         # the bands of outputs and workspaces
FILL_BYTE = 0xFF                                         # every byte of an output before the call: NaN as a float, -1 as an integer
_NAN = {                                                 # one quiet NaN per float type, as little-endian bytes
    torch.float16: (0x00, 0x7E), torch.bfloat16: (0xC0, 0x7F), torch.float32: (0x00, 0x00, 0xC0, 0x7F),
    torch.float64: (0, 0, 0, 0, 0, 0, 0xF8, 0x7F), torch.complex64: (0x00, 0x00, 0xC0, 0x7F),
}


def elem_size(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def band_pattern(dtype, kind):
    """The bytes one element's worth of a band repeats."""
    if kind != "in":
        return (BAND_BYTE,)
    return _NAN.get(dtype, (0xFF,))


class GuardError(AssertionError):
    """What check() and same_bits() raise."""


class GuardArena:
    def __init__(self, device="cpu", band_bytes=BAND_BYTES, capacity_bytes=8 << 20, pinned=False):
        self.device = torch.device(device)
        self.band = int(band_bytes)
        assert self.band >= 16 and self.band % 16 == 0, "a band is whole 16-byte units"
        if pinned:
            assert self.device.type == "cpu", "pinned memory is host memory"
        self.mem = torch.empty(int(capacity_bytes), dtype=torch.uint8, device=self.device, pin_memory=bool(pinned))
        self._patterns = {}
        self.reset()

    # ------------------------------------------------------------------ carving
    def reset(self):
        """Forget every buffer: the allocation is carved from its start again."""
        self._cursor = 0
        self._bufs = []                                  # (name, kind, start, nbytes, pattern)

    def _band_of(self, pattern):
        """band_bytes of ``pattern`` repeated, on the arena's device."""
        t = self._patterns.get(pattern)
        if t is None:
            reps = self.band // len(pattern)
            t = torch.tensor(list(pattern) * reps, dtype=torch.uint8).to(self.device)
            self._patterns[pattern] = t
        return t

    def carve(self, shape, dtype, skew_bytes=0, kind="out", name=None, data=None):
        """A contiguous ``dtype`` view of ``shape`` at an address that is ``skew_bytes`` past a 16-byte boundary, a band below it
        and a band above it.  ``skew_bytes``: 0 .. 15, a multiple of the element size.  ``data`` (kind "in"): copied in."""
        if kind not in ("in", "out", "work"):
            raise ValueError(f"GuardArena.carve: kind {kind!r}")
        es = elem_size(dtype)
        skew_bytes = int(skew_bytes)
        if not 0 <= skew_bytes < 16 or skew_bytes % es != 0:
            raise ValueError(f"GuardArena.carve: skew_bytes {skew_bytes} is not a multiple of the element size {es} in 0 .. 15")
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        nbytes = es * int(np.prod(shape, dtype=np.int64)) if shape else es
        base = self.mem.data_ptr()
        start = self._cursor + self.band                 # the lowest start that leaves room for the low band
        start += (skew_bytes - (base + start)) % 16
        end = start + nbytes
        if end + self.band > self.mem.numel():
            raise MemoryError(f"GuardArena: {name or 'buffer'} of {nbytes} bytes does not fit ({self.mem.numel()} bytes in all, "
                              f"{self._cursor} carved); make the arena with a larger capacity_bytes")
        pattern = band_pattern(dtype, kind)
        assert self.band % len(pattern) == 0
        band = self._band_of(pattern)
        self.mem[start - self.band:start] = band         # (both on the buffer's element grid: the band is whole elements)
        self.mem[end:end + self.band] = band
        view = self.mem[start:end].view(dtype).view(shape)
        if kind == "in":
            if data is None:
                raise ValueError("GuardArena.carve: an input buffer needs data=")
            view.copy_(data.reshape(shape))
        else:
            self.mem[start:end] = FILL_BYTE
        assert view.data_ptr() == base + start and view.data_ptr() % 16 == skew_bytes and view.is_contiguous()
        self._bufs.append((name or f"buffer {len(self._bufs)}", kind, start, nbytes, pattern))
        self._cursor = end + self.band
        return view

    def bands(self, index=-1):
        """(low band, high band) of a carved buffer as uint8 views (for the controls)."""
        _, _, start, nbytes, _ = self._bufs[index]
        return self.mem[start - self.band:start], self.mem[start + nbytes:start + nbytes + self.band]

    # ------------------------------------------------------------------ checking
    def damage(self):
        """[(buffer, "low" | "high", first, last)]: every band that no longer holds its pattern, with its first and last damaged
        byte relative to the buffer's edge."""
        out = []
        for name, _, start, nbytes, pattern in self._bufs:
            want = self._band_of(pattern)
            for side, lo, origin in (("low", start - self.band, start), ("high", start + nbytes, start + nbytes)):
                got = self.mem[lo:lo + self.band]
                if torch.equal(got, want):
                    continue
                bad = torch.nonzero(got != want).reshape(-1)
                out.append((name, side, int(bad[0]) + lo - origin, int(bad[-1]) + lo - origin))
        return out

    def check(self):
        """Every band intact, or a GuardError that names each damaged one."""
        found = self.damage()
        if found:
            raise GuardError("guard bands damaged: " + "; ".join(
                f"{name}: the {side} band, bytes {first} .. {last} relative to the buffer's {'start' if side == 'low' else 'end'}"
                for name, side, first, last in found))


# ---------------------------------------------------------------------------------------------------- comparing
def as_bytes(t):
    """The tensor's bytes as a flat uint8 numpy array."""
    t = t.detach()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.cpu().contiguous().reshape(-1).view(torch.uint8).numpy()


def same_bits(what, got, want):
    """``got`` has the shape, dtype and bytes of ``want``, or a GuardError that says how many elements differ, which is the first,
    and whether it still holds the arena's prefill, i.e. was never written."""
    if tuple(got.shape) != tuple(want.shape) or got.dtype != want.dtype:
        raise GuardError(f"{what}: {tuple(got.shape)} {got.dtype}, the plain call gave {tuple(want.shape)} {want.dtype}")
    a, b = as_bytes(got), as_bytes(want)
    if np.array_equal(a, b):
        return
    es = elem_size(got.dtype)
    bad = np.flatnonzero((a != b).reshape(-1, es).any(axis=1))
    first = int(bad[0])
    unwritten = int((a.reshape(-1, es)[bad] == FILL_BYTE).all(axis=1).sum())
    raise GuardError(f"{what}: {bad.size} of {a.size // es} elements differ from the plain call, the first at flat index {first}"
                     f" (last {int(bad[-1])}); {unwritten} of them still hold the prefill and were never written")
