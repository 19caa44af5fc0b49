"""The host side of the device builder of the item-run score streams (tmf_s7plan_*: include/tmf.h, csrc/tmf_s7plan.hip), without a
GPU: the entry points are bound from the header, refuse bad arguments before anything is launched, Scores7Plan picks its builder as
documented, and the sub_wave helper both builders share reproduces order_by_fill's table."""
import ctypes

import pytest
import torch

from test_scores7_cpu import _lib_and_engine, _problem

ENTRY = ('tmf_s7plan_chunks', 'tmf_s7plan_subs', 'tmf_s7plan_streams')


def test_entry_points_are_bound_from_the_header():
    lib, _ = _lib_and_engine()
    from teamoflow_amd import _lib
    for name in ENTRY + ('tmf_s7plan_workspace_bytes',):
        assert name in _lib.HEADER.functions and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES['tmf_s7plan_workspace_bytes'][0] is ctypes.c_size_t
    sizes = [0, 1, 2, 31, 32, 1000, 50000, 10 ** 6, 2 ** 31 - 1]
    got = [lib.tmf_s7plan_workspace_bytes(n) for n in sizes]
    assert all(b > 0 for b in got) and got == sorted(got) and got[-1] > got[0]
    assert all(b >= 8 * (n + 1) for n, b in zip(sizes, got))   # the counts of n chunks / sub-chunks and the zero behind them


def _calls(lib, **change):
    """The three calls on a well-formed (host memory) argument list with `change` applied -> their return codes.  Nothing may be
    launched: there is no GPU here, and a launch on these host pointers would not return TMF_E_INVALID."""
    m, S, n, nnz = 3, 4, 50, 5
    a = dict(rowptr_u=torch.tensor([0, 2, 2, 5]), col_u=torch.tensor([1, 7, 0, 3, 9], dtype=torch.int32),
             R=torch.arange(m * S, dtype=torch.int32).reshape(m, S), nnz=nnz, m=m, S=S, n=n, width=25, slots=8,
             chunk_ent=torch.zeros(3, dtype=torch.int64), chunk_sub=torch.zeros(3, dtype=torch.int32), n_sub=2,
             sub_fill=torch.zeros(2, 4, dtype=torch.int32), sub_place=torch.zeros(3, dtype=torch.int64),
             sub_step=torch.zeros(3, dtype=torch.int64), steps=torch.zeros(9, 4, dtype=torch.int32),
             place=torch.zeros(nnz + m * S, dtype=torch.int32), ws=torch.zeros(4096, dtype=torch.uint8))
    a.update(change)
    head = (a['rowptr_u'], a['col_u'], a['R'], a['nnz'], a['m'], a['S'], a['n'], a['width'], a['slots'], a['chunk_ent'], a['chunk_sub'])
    ws = (a['ws'], a['ws'].numel() if a['ws'] is not None else 0)
    return (lib.tmf_s7plan_chunks(*head, *ws, None),
            lib.tmf_s7plan_subs(*head, a['n_sub'], a['sub_fill'], a['sub_place'], a['sub_step'], *ws, None),
            lib.tmf_s7plan_streams(*head, a['n_sub'], a['sub_step'], 8, 0, a['steps'], a['place'], None))


@pytest.mark.parametrize('change', [dict(rowptr_u=None), dict(col_u=None), dict(R=None), dict(slots=0), dict(slots=-1), dict(slots='cap+1'),
                                    dict(width=0), dict(width=-3), dict(n=2 ** 24), dict(n=2 ** 24 + 5), dict(n=0), dict(nnz=-1),
                                    dict(nnz=2 ** 31), dict(m=2 ** 29, S=4)],
                         ids=lambda c: ','.join(f'{k}={v}' for k, v in c.items()))
def test_bad_arguments_are_refused_before_any_launch(change):
    lib, _ = _lib_and_engine()
    from teamoflow_amd import _lib
    if change.get('slots') == 'cap+1':
        change = dict(slots=lib.tmf_wmrb_scores7_slots() + 1)
    assert _calls(lib, **change) == (_lib.HEADER.constants['TMF_E_INVALID'],) * 3
    assert b's7plan' in lib.tmf_last_error()


def test_null_outputs_and_short_workspaces_are_refused():
    lib, _ = _lib_and_engine()
    from teamoflow_amd import _lib
    bad = _lib.HEADER.constants['TMF_E_INVALID']
    assert _calls(lib, chunk_ent=None) == (bad,) * 3 and _calls(lib, chunk_sub=None) == (bad,) * 3
    assert _calls(lib, ws=None)[:2] == (bad, bad) and _calls(lib, ws=torch.zeros(8, dtype=torch.uint8))[:2] == (bad, bad)
    assert _calls(lib, sub_step=None)[1:] == (bad, bad) and _calls(lib, steps=None)[2] == bad
    assert _calls(lib, n_sub=-1)[1:] == (bad, bad) and _calls(lib, n_sub=2 ** 31)[1:] == (bad, bad)


def _plans(E, m=300, n=200, S=12, nnz=1500):
    idx, val, R = _problem(m, n, S, nnz, seed=4)
    plan = E.InteractionPlan(idx, val, m, n)
    return plan, E.WmrbPlan(plan, R, item_slices=2, n_components=128, sliced=True)


def test_the_device_builder_needs_a_gpu_and_the_default_on_cpu_tensors_is_torch(monkeypatch):
    _, E = _lib_and_engine()
    monkeypatch.delenv('TMF_S7_BUILD', raising=False)
    plan, wplan = _plans(E)
    kw = dict(slice_bytes=64 * 512, slots=128)
    with pytest.raises(ValueError, match="builder='device'"):
        E.Scores7Plan(plan, wplan, 128, torch.float32, builder='device', **kw)
    with pytest.raises(ValueError, match='rocprim'):
        E.Scores7Plan(plan, wplan, 128, torch.float32, builder='rocprim', **kw)
    a = E.Scores7Plan(plan, wplan, 128, torch.float32, builder=None, **kw).order_by_fill()
    b = E.Scores7Plan(plan, wplan, 128, torch.float32, builder='torch', **kw).order_by_fill()
    for name in ('steps', 'place', 'sub_step', 'sub_place', 'chunk_sub', 'sub_fill', 'sub_wave'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    monkeypatch.setenv('TMF_S7_BUILD', 'torch')
    c = E.Scores7Plan(plan, wplan, 128, torch.float32, **kw)
    assert torch.equal(c.place, b.place) and c.n_steps == b.n_steps
    monkeypatch.setenv('TMF_S7_BUILD', 'device')   # the variable is read where builder is None, and asks for the same thing
    with pytest.raises(ValueError, match="builder='device'"):
        E.Scores7Plan(plan, wplan, 128, torch.float32, **kw)


def test_sub_wave_helper_reproduces_the_table_of_order_by_fill():
    """W = 16 waves, cost 3 + 2 fill = 11 / 9 / 7 / 5 per step of fill 4 / 3 / 2 / 1; cuts at multiples of 8 steps, by hand:
    row 0: 160 steps of fill 4 only - total cost 1760, wave w starts at step 10 w, rounded to the nearest multiple of 8
           ((cut + 4) // 8 * 8): 0 8 24 32 40 48 64 72 80 88 104 112 120 128 144 152, then 160
    row 1: nothing but 5 steps of fill 1 (cost 25): point w sits at step 25 w // 80 = 0 .. 3 for w <= 12, which rounds to 0, and at
           step 4 for w = 13 .. 15, which rounds to 8 and is cut to the 5 steps there are
    row 2: 16 steps of fill 4 (cost 176) and 16 of fill 1 (cost 80), total 256 = 16 per wave: point w sits at cost 16 w; below 176
           that is step 16 w // 11 = 0 1 2 4 5 7 8 10 11 13 14 (w = 0 .. 10), from 176 on step 16 + (16 w - 176) // 5 = 16 19 22 25 28
           (w = 11 .. 15); rounded: 0 0 0 8 8 8 8 8 8 16 16 | 16 16 24 24 32, then 32"""
    lib, E = _lib_and_engine()
    W = lib.tmf_wmrb_scores7_waves()
    assert W == 16 and (E.SCORES7_COST_STEP, E.SCORES7_COST_SLOT) == (3, 2)
    fill = torch.tensor([[160, 0, 0, 0], [0, 0, 0, 5], [16, 0, 0, 16]], dtype=torch.int64)
    want = torch.tensor([[0, 8, 24, 32, 40, 48, 64, 72, 80, 88, 104, 112, 120, 128, 144, 152, 160],
                         [0] * 13 + [5] * 4,
                         [0, 0, 0, 8, 8, 8, 8, 8, 8, 16, 16, 16, 16, 24, 24, 32, 32]], dtype=torch.int32)
    got = E.scores7_sub_wave(fill, W)
    assert got.dtype == torch.int32 and torch.equal(got, want)
    # and it is the table order_by_fill stores, for a real plan
    plan, wplan = _plans(E)
    s7 = E.Scores7Plan(plan, wplan, 128, torch.float32, slice_bytes=64 * 512, slots=128, builder='torch').order_by_fill()
    assert torch.equal(E.scores7_sub_wave(s7.sub_fill.to(torch.int64), W), s7.sub_wave)
