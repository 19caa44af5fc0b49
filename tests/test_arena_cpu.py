"""tests/arena.py on CPU tensors: a checker that stays silent would let every test built on it pass, so it is shown to speak -
one element written past a view's end and one written in front of its start, each through the flat buffer, are reported by name,
side and offset - and the layout it promises is measured: 256-byte aligned starts, the band beginning at the very byte behind the
data whatever the size and the element type, at least 64 KiB of band on both sides."""
import struct

import pytest
import torch

from arena import ALIGN, BAND_BYTES, BIG, BIG_BAND, INT_POISON, NAN_BAND, Arena, GuardDamaged

BANDS = [pytest.param(NAN_BAND, id='nan'), pytest.param(BIG_BAND, id='2^60')]
# odd sizes, every element size: (name, shape, dtype)
VIEWS = [('a_f32', (7, 3), torch.float32), ('b_bf16', (5,), torch.bfloat16), ('c_i32', (1,), torch.int32), ('d_f64', (3, 1), torch.float64),
         ('e_bf16', (33, 3), torch.bfloat16), ('f_i16', (257,), torch.int16), ('g_u8', (13,), torch.uint8), ('h_i64', (9,), torch.int64),
         ('i_f32', (513, 33), torch.float32)]


def build(band, capacity=2 << 20):
    arena = Arena('cpu', band=band, capacity=capacity)
    views = {name: arena.take(name, shape, dtype) for name, shape, dtype in VIEWS}
    return arena, views


def offset(arena, t):
    return t.data_ptr() - arena.buf.data_ptr()


@pytest.mark.parametrize('band', BANDS)
def test_an_intact_arena_passes_and_has_the_promised_layout(band):
    arena, views = build(band)
    arena.check()
    assert arena.damage() is None
    word = torch.tensor(list(band.to_bytes(4, 'little')), dtype=torch.uint8)
    prev_end = 0
    for (name, shape, dtype), (n2, start, end) in zip(VIEWS, arena.views):
        v = views[name]
        assert name == n2 and tuple(v.shape) == shape and v.dtype is dtype and v.is_contiguous()
        assert offset(arena, v) == start and start % ALIGN == 0 and v.data_ptr() % ALIGN == 0
        assert end - start == v.numel() * v.element_size()
        assert start - prev_end >= BAND_BYTES                                   # 64 KiB of band in front ...
        # ... and behind, beginning at the byte after the data: every byte up to the next view (or 64 KiB) is pattern, phase kept
        behind = arena.buf[end:end + BAND_BYTES]
        assert behind.numel() == BAND_BYTES
        assert torch.equal(behind, word.repeat(BAND_BYTES // 4 + 2)[end % 4:end % 4 + BAND_BYTES]), name
        front = arena.buf[start - BAND_BYTES:start]
        assert torch.equal(front, word.repeat(BAND_BYTES // 4)), name
        assert arena.holds(v) and arena.name_of(v) == name
        prev_end = end
    # the data of an odd-sized view really ends off the alignment grid: the band has no slack to hide in
    assert any(e % 4 for _, _, e in arena.views) and any(e % ALIGN for _, _, e in arena.views)
    assert not arena.holds(torch.zeros(3))


def test_the_two_bands_read_differently_in_every_type():
    a, b = Arena('cpu', NAN_BAND, capacity=1 << 20), Arena('cpu', BIG_BAND, capacity=1 << 20)
    for dtype in (torch.float32, torch.bfloat16, torch.float64, torch.int32, torch.int16, torch.int64):
        x, y = a.buf[:64].view(dtype), b.buf[:64].view(dtype)
        same = (x == y) | ((x != x) & (y != y)) if dtype.is_floating_point else (x == y)
        assert not bool(same.any()), dtype
    f = a.buf[:8].view(torch.float32)
    assert bool(torch.isnan(f).all()) and struct.unpack('<I', bytes(a.buf[:4].tolist()))[0] == NAN_BAND
    g = b.buf[:8].view(torch.float32)
    assert bool((g == BIG).all()) and float(torch.tensor(BIG).bfloat16()) == BIG       # 2^60: finite, and exact in bf16
    assert bool((b.buf[:8].view(torch.bfloat16)[1::2] == BIG).all())


@pytest.mark.parametrize('band', BANDS)
def test_poison_goes_with_the_band_and_fills_are_what_they_say(band):
    arena = Arena('cpu', band, capacity=1 << 20)
    p = arena.take('p', (5, 3), torch.float32)
    assert bool(torch.isnan(p).all()) if band == NAN_BAND else bool((p == BIG).all())
    h = arena.take('h', (5,), torch.bfloat16, 'poison')
    assert bool(torch.isnan(h).all()) if band == NAN_BAND else bool((h == BIG).all())
    assert bool((arena.take('i', (3,), torch.int32) == INT_POISON).all())
    assert bool((arena.take('s', (3,), torch.int16) == 0x5a5a).all())
    assert not bool(arena.take('z', (4, 4), torch.float64, 'zero').any())
    assert bool((arena.take('seven', 6, torch.float32, 7.0) == 7.0).all())
    src = torch.arange(12, dtype=torch.float32).view(3, 4)
    assert torch.equal(arena.take('copy', (3, 4), torch.float32, src), src)
    assert arena.take('none', (0, 4), torch.float32).numel() == 0
    arena.check()


@pytest.mark.parametrize('band', BANDS)
@pytest.mark.parametrize('name', [n for n, _, _ in VIEWS])
def test_one_element_past_the_end_is_reported(band, name):
    arena, views = build(band)
    v = views[name]
    end = offset(arena, v) + v.numel() * v.element_size()
    arena.buf[end:end + v.element_size()].view(v.dtype)[0] = 1          # element [numel] of the view, through the flat buffer
    with pytest.raises(GuardDamaged) as e:
        arena.check()
    assert arena.damage()[:2] == (name, 'behind') and arena.damage()[2] >= end and arena.damage()[3] < v.element_size()
    assert repr(name) in str(e.value) and 'behind' in str(e.value) and str(arena.damage()[2]) in str(e.value)


@pytest.mark.parametrize('band', BANDS)
@pytest.mark.parametrize('name', [n for n, _, _ in VIEWS])
def test_one_element_before_the_start_is_reported(band, name):
    arena, views = build(band)
    v = views[name]
    start = offset(arena, v)
    arena.buf[start - v.element_size():start].view(v.dtype)[0] = 1      # element [-1]
    with pytest.raises(GuardDamaged) as e:
        arena.check()
    who, side, off, dist = arena.damage()
    assert (who, side) == (name, 'before') and start - v.element_size() <= off < start and dist == start - off
    assert repr(name) in str(e.value) and 'before' in str(e.value) and str(off) in str(e.value)


def test_a_write_of_the_band_pattern_far_from_any_view_and_inside_views_is_judged_right():
    arena, views = build(NAN_BAND)
    for v in views.values():            # anything may be written INSIDE a view
        v.view(-1).view(torch.uint8).fill_(0xff)
    arena.check()
    arena.buf[arena.capacity - 1] ^= 0xff                                # the very last byte of the arena: behind the last view
    assert arena.damage()[:3] == (VIEWS[-1][0], 'behind', arena.capacity - 1)


def test_a_full_arena_says_so():
    arena = Arena('cpu', NAN_BAND, capacity=3 * BAND_BYTES)
    arena.take('fits', (BAND_BYTES // 4,), torch.float32)
    with pytest.raises(MemoryError):
        arena.take('does not', (BAND_BYTES,), torch.float32)
