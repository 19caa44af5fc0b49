"""The device builder of the item-run score streams (tmf_s7plan_chunks / _subs / _streams: csrc/tmf_s7plan.hip) against the torch
builder of _engine.Scores7Plan, bit for bit: steps, place, sub_step, sub_place, chunk_sub in item order; steps, sub_fill, sub_wave
after order_by_fill.  The cases sit where the chunk-local construction can go wrong: a last group of fewer than 256 users, runs of
many steps, sub-chunks that share their border item, one row per slice, a slice far wider than a sub-chunk (on both key widths of
the in-LDS sort), runs beyond 512 entries,
the highest item ids, slots = 1 and slots = the cap.  A fit must not see which builder made its plan."""
import numpy as np
import pytest
import torch

from test_scores7_cpu import _problem

pytestmark = pytest.mark.gpu
R128 = 128
ARRAYS = ('steps', 'place', 'sub_step', 'sub_place', 'chunk_sub')


@pytest.fixture(scope='module')
def eng():
    from teamoflow_amd import _engine, _lib
    _lib.get()
    return _engine


@pytest.fixture(autouse=True)
def no_form_variables(monkeypatch):
    for name in ('TMF_S7_SLOTS', 'TMF_S7_SLICE_BYTES', 'TMF_S7_BUILD'):
        monkeypatch.delenv(name, raising=False)


def both(eng, m, n, problem, slice_bytes=None, slots=None):
    """The two plans of one GPU problem, compared in item order and again in fill order."""
    idx, val, R = (t.cuda() for t in problem)
    plan = eng.InteractionPlan(idx, val, m, n)
    wplan = eng.WmrbPlan(plan, R, item_slices=2, n_components=R128, sliced=True)
    kw = dict(slice_bytes=slice_bytes, slots=slots)
    t = eng.Scores7Plan(plan, wplan, R128, torch.float32, builder='torch', **kw)
    d = eng.Scores7Plan(plan, wplan, R128, torch.float32, builder='device', **kw)
    torch.cuda.synchronize()
    assert (d.n_steps, d.n_sub, d.n_entries) == (t.n_steps, t.n_sub, t.n_entries)
    assert (d.width, d.n_slices, d.n_groups, d.slots, d.pad_slot) == (t.width, t.n_slices, t.n_groups, t.slots, t.pad_slot)
    for name in ARRAYS:
        a, b = getattr(d, name), getattr(t, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    assert d.sub_wave is None and d.sub_fill is None
    kept = {name: getattr(d, name).clone() for name in ARRAYS[1:]}
    assert t.order_by_fill() is t and d.order_by_fill() is d
    torch.cuda.synchronize()
    for name in ('steps', 'sub_fill', 'sub_wave'):
        a, b = getattr(d, name), getattr(t, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name + ' in fill order'
    for name in ARRAYS[1:]:
        assert torch.equal(getattr(d, name), kept[name]) and torch.equal(getattr(d, name), getattr(t, name)), name
    steps = d.steps
    assert d.order_by_fill() is d and d.steps is steps        # a second call changes nothing
    # fill order asked for before anything read the streams: written once, in that order, with the places
    f = eng.Scores7Plan(plan, wplan, R128, torch.float32, builder='device', **kw).order_by_fill()
    for name in ARRAYS + ('sub_fill', 'sub_wave'):
        assert torch.equal(getattr(f, name), getattr(t, name)), name + ' of a plan ordered at once'
    return d


@pytest.mark.parametrize('m', [1, 255, 257, 775])
def test_group_borders(eng, m):
    d = both(eng, m, 300, _problem(m, 300, 20, 6 * m, seed=m, empty_user=m // 2), slice_bytes=100 * 512)
    assert d.n_slices == 3 and d.n_groups == -(-m // 256)


def test_tiny_catalog_many_steps_per_run_and_shared_border_items(eng):
    d = both(eng, 300, 40, _problem(300, 40, 30, 3000, seed=5), slots=64)
    assert d.n_sub > 100 and d.n_steps < d.n_entries // 2


def test_one_row_per_slice(eng):
    d = both(eng, 300, 60, _problem(300, 60, 12, 2000, seed=6), slice_bytes=1)
    assert d.width == 1 and d.n_slices == 60


def test_whole_catalog_in_one_slice(eng):
    m, n, S = 300, 70000, 64
    g = torch.Generator().manual_seed(7)
    key = torch.unique(torch.randint(0, m, (4000,), generator=g) * n + torch.randint(0, n, (4000,), generator=g))
    idx = torch.stack([key // n, key % n], 1)
    val = torch.ones(key.numel())
    R = torch.randint(0, n, (m, S), generator=g).to(torch.int32)
    d = both(eng, m, n, (idx, val, R), slice_bytes=n * 512)
    assert d.n_slices == 1 and d.width == n


def test_sub_chunks_that_span_more_items_than_32_bit_keys_hold(eng):
    """One slice of 2^21 items, every group's entries in one sub-chunk: (item - first item, slot) does not fit 32 bits, the sort runs
    on 64-bit keys."""
    m, n, S = 300, 2 ** 21, 16
    g = torch.Generator().manual_seed(13)
    key = torch.unique(torch.randint(0, m, (900,), generator=g) * n + torch.randint(0, n, (900,), generator=g))
    idx = torch.stack([key // n, key % n], 1)
    R = torch.randint(0, n, (m, S), generator=g).to(torch.int32)
    d = both(eng, m, n, (idx, torch.ones(key.numel()), R), slice_bytes=n * 512)
    first = d.steps[d.sub_step[:-1], 0].long()
    last = d.steps[d.sub_step[1:] - 1, 0].long()
    assert d.n_slices == 1 and d.n_sub == 2 and int((last - first).max()) >= 2 ** 19


def test_long_run(eng):
    """Every user of a group holds item 7 as a positive twice and as a negative twice: a run of 1024 entries, 256 steps."""
    m, n, S = 256, 50, 6
    g = torch.Generator().manual_seed(8)
    u = torch.arange(m)
    idx = torch.cat([torch.stack([u, torch.full_like(u, 7)], 1)] * 2 + [torch.stack([u, torch.randint(0, n, (m,), generator=g)], 1)])
    val = torch.ones(idx.shape[0])
    R = torch.randint(0, n, (m, S), generator=g).to(torch.int32)
    R[:, 1] = R[:, 4] = 7
    d = both(eng, m, n, (idx, val, R))
    assert d.n_entries == 3 * m + m * S


def test_no_interactions(eng):
    m, n, S = 300, 200, 16
    _, _, R = _problem(m, n, S, 10, seed=9)
    d = both(eng, m, n, (torch.zeros(0, 2, dtype=torch.int64), torch.zeros(0), R), slice_bytes=64 * 512)
    assert d.n_entries == m * S


def test_every_interaction_in_one_user(eng):
    m, n, S = 300, 500, 16
    _, _, R = _problem(m, n, S, 10, seed=10)
    items = torch.randperm(n, generator=torch.Generator().manual_seed(10))[:400]
    idx = torch.stack([torch.full_like(items, 258), items], 1)
    both(eng, m, n, (idx, torch.ones(400), R), slice_bytes=128 * 512, slots=96)


def test_ids_at_the_top_of_the_supported_range(eng):
    m, n, S = 2, 2 ** 24 - 1, 8
    g = torch.Generator().manual_seed(11)
    R = (n - 100 + torch.randint(0, 100, (m, S), generator=g)).to(torch.int32)
    key = torch.unique(torch.randint(0, m, (60,), generator=g) * n + n - 100 + torch.randint(0, 100, (60,), generator=g))
    idx = torch.stack([key // n, key % n], 1)
    d = both(eng, m, n, (idx, torch.ones(key.numel()), R))
    assert d.n_slices == 2048 and int(d.steps[:d.n_steps, 0].max()) >= n - 100


@pytest.mark.parametrize('slots', [1, None])
def test_one_slot_and_the_cap(eng, slots):
    # slots = the cap: 300 * 40 + ~2900 entries in two chunks of a single slice, so full sub-chunks of 6144 and short ones
    m, n, S, nnz = (40, 30, 6, 150) if slots == 1 else (300, 700, 40, 3000)
    d = both(eng, m, n, _problem(m, n, S, nnz, seed=12), slots=slots)
    if slots == 1:
        assert d.n_sub == d.n_entries == d.n_steps
    else:
        assert d.slots == d.pad_slot and int((d.sub_place[1:] - d.sub_place[:-1]).max()) == d.pad_slot


@pytest.mark.parametrize('loss, resample', [('WARPLoss', 1), ('WMRBLoss', None)])
def test_a_fit_does_not_see_the_builder(monkeypatch, loss, resample):
    import test_gpu_resample as tr
    from teamoflow_amd import _engine, _lib, _ops
    from teamoflow_amd.mf import embedding_graphs as EG, loss_graphs as LG
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye

    class tm:
        lib, L, E, ops, MF, Fixed, Sparse = _lib.get(), _lib, _engine, _ops, MatrixFactorization, FixedInitializer, SparseInteractions
    tm.EG, tm.LG, tm.eye = EG, LG, staticmethod(eye)
    p = tr.problem(300, 500, 128, 32, seed=3)
    monkeypatch.setenv('TMF_SCORES7', '1')
    monkeypatch.setenv('TMF_FORCE_SLICED', '1')   # WMRBLoss at this size would take the one-kernel pass, which has no score streams
    built, made = [], _engine.Scores7Plan._build_device

    def spy(self, *a, **k):
        built.append(1)
        return made(self, *a, **k)
    monkeypatch.setattr(_engine.Scores7Plan, '_build_device', spy)
    out = {}
    for builder in ('device', 'torch'):
        monkeypatch.setenv('TMF_S7_BUILD', builder)
        del built[:]
        attrs = dict(resample_every=resample, sample_seed=5) if resample else {}
        model = tr.fit(tm, tr.make_model(tm, p, loss, **attrs), p, 4)
        assert bool(built) == (builder == 'device')            # the plans really came from the builder the variable names
        out[builder] = (model.user_embedding.clone(), model.item_embedding.clone(), list(model.loss_history_))
    a, b = out['device'], out['torch']
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] and np.isfinite(a[2]).all()
