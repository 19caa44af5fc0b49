"""Guarded buffers for tests: views that sit between guard bands inside ONE flat byte buffer (a plain module, no fixtures).

    arena = Arena(device, band=NAN_BAND)                     # or BIG_BAND
    x = arena.take('sp', (m, S), torch.float32, 'poison')    # a contiguous view
    ... run the code under test on x ...
    arena.check()                                            # raises GuardDamaged when a byte outside the views changed

Layout: every byte of the buffer that belongs to no view holds the band pattern, a 32-bit word repeated from the buffer's first
byte.  A view starts 256-byte aligned; its last byte is followed DIRECTLY by band bytes - no alignment slack behind the data - and
at least BAND_BYTES (64 KiB, the zone of tests/test_gpu_strided_views.py) of band lie in front of it and behind it.
The two patterns, reinterpreted for any dtype, give an out-of-extent read a different value in the two runs of a test:
    NAN_BAND 0x7fc0beef   fp32: a NaN with a payload (tests/test_gpu_fullsoftmax.py)   bf16 halves: 0xbeef = -0.46.., 0x7fc0 = NaN
    BIG_BAND 0x5d800000   fp32: 2^60, finite                                           bf16 halves: 0x0000 = 0,      0x5d80 = 2^60
``fill='poison'`` of take() goes with the band: NaN / 2^60 for the floating types, 0x5a.. for the integer types."""
import numpy as np
import torch

BAND_BYTES = 64 << 10
ALIGN = 256
NAN_BAND = 0x7fc0beef
BIG_BAND = 0x5d800000
INT_POISON = 0x5a5a5a5a
BIG = 2.0 ** 60


class GuardDamaged(AssertionError):
    pass


class Arena:
    def __init__(self, device, band=NAN_BAND, capacity=64 << 20, band_bytes=BAND_BYTES):
        if band not in (NAN_BAND, BIG_BAND):
            raise ValueError(f'band={band:#x} is neither NAN_BAND nor BIG_BAND')
        self.band, self.band_bytes = band, int(band_bytes)
        self.capacity = -(-int(capacity) // ALIGN) * ALIGN
        # the allocation is longer than the capacity by one alignment step, so that offset 0 can be moved onto a 256-byte border
        raw = torch.empty(self.capacity + ALIGN, dtype=torch.uint8, device=device)
        skew = (-raw.data_ptr()) % ALIGN
        self._raw = raw
        self.buf = raw[skew:skew + self.capacity]
        assert self.buf.data_ptr() % ALIGN == 0
        self._pattern = torch.tensor(list(int(band).to_bytes(4, 'little')), dtype=torch.uint8, device=device).repeat(self.capacity // 4)
        self.buf.copy_(self._pattern)
        self._is_band = torch.ones(self.capacity, dtype=torch.bool, device=device)
        self.views = []          # (name, first byte, byte behind the last), in take() order = ascending
        self._end = 0            # the byte behind the last view (0: none yet)

    @property
    def poison(self):
        """The floating-point poison that goes with the band."""
        return float('nan') if self.band == NAN_BAND else BIG

    def poison_of(self, dtype):
        if dtype.is_floating_point:
            return self.poison
        return INT_POISON >> (32 - 8 * min(torch.empty((), dtype=dtype).element_size(), 4))

    def take(self, name, shape, dtype, fill='poison'):
        """A contiguous view of ``shape`` and ``dtype``.  fill: 'poison' | 'zero' | a number | a tensor whose contents are copied
        (same number of elements; converted to ``dtype``)."""
        shape = tuple(int(d) for d in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        esize = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * esize
        start = -(-(self._end + self.band_bytes) // ALIGN) * ALIGN
        end = start + nbytes
        if end + self.band_bytes > self.capacity:
            raise MemoryError(f'arena of {self.capacity} bytes is full: {name} needs [{start}, {end + self.band_bytes})')
        view = self.buf[start:end].view(dtype).view(shape)
        self._is_band[start:end] = False
        self.views.append((name, start, end))
        self._end = end
        if isinstance(fill, torch.Tensor):
            view.copy_(fill.reshape(shape))
        elif fill == 'zero':
            view.zero_()
        elif fill == 'poison':
            view.fill_(self.poison_of(dtype))
        else:
            view.fill_(fill)
        assert view.is_contiguous() and start % ALIGN == 0 and (nbytes == 0 or view.data_ptr() == self.buf.data_ptr() + start)
        return view

    def holds(self, t):
        """Whether every byte of tensor ``t`` (contiguous) lies inside a view of this arena."""
        a = t.data_ptr() - self.buf.data_ptr()
        b = a + t.numel() * t.element_size()
        return any(s <= a and b <= e for _, s, e in self.views)

    def name_of(self, t):
        a = t.data_ptr() - self.buf.data_ptr()
        return next((n for n, s, e in self.views if s <= a < max(e, s + 1)), None)

    def damage(self):
        """None, or (name, side, first damaged byte as an offset into the arena, its distance from the view): side 'behind' = the
        band that begins at the byte after the view's last, distance 0 = that very byte; 'before' = the band that ends at the view's
        first byte, distance 1 = the byte in front of it.  A damaged byte between two views goes to the nearer one."""
        bad = (self.buf != self._pattern) & self._is_band
        if not bool(bad.any()):
            return None
        off = int(torch.nonzero(bad)[0])
        best = None
        for name, s, e in self.views:
            cand = (off - e, name, 'behind') if off >= e else (s - off, name, 'before')
            if best is None or cand[0] < best[0]:
                best = cand
        if best is None:
            return ('(no view)', 'band', off, off)
        return (best[1], best[2], off, best[0])

    def check(self):
        d = self.damage()
        if d is not None:
            name, side, off, dist = d
            raise GuardDamaged(f'guard band {side} {name!r} damaged: first changed byte at arena offset {off}, '
                               f'{dist} byte(s) {"behind its end" if side == "behind" else "in front of its start"}')
