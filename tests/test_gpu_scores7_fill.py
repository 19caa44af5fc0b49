"""tmf_wmrb_scores7_fill_f32 - the item-run scores kernel over steps classed by fill (Scores7Plan.order_by_fill: a pad slot costs no
work; csrc/tmf_wmrb.hip) - against the same kernel over the item-ordered plan (TMF_S7_FILL=0: every step runs as fill 4) and against
tmf_wmrb_scores3.  A score is one dot product with one summation tree wherever its step runs, so fill order against item order is
bit for bit on ANY tables; against scores3 the trees differ, so that comparison is on dyadic tables, where the whole epoch (hinge,
gradients, fresh Adam) is bit-identical too."""
import pytest
import torch

from test_gpu_scores5 import problem
from test_gpu_scores7 import epoch, make_state

pytestmark = pytest.mark.gpu

K = 4


@pytest.fixture(scope='module')
def eng():
    from teamoflow_amd import _engine, _lib
    _lib.get()
    return _engine


def _general(r):
    def make():
        m, n, S = 300, 2000, 50
        idx, val, R, _, _ = problem(m, n, r, S, 5000, seed=21 + r, dev='cpu')
        return idx, val, R, m, n, r, S
    return make


def _run_lengths(m):
    """The run-length case of test_gpu_scores7: n = 40, S = 30; items 0, 1, 2 get runs of K, K + 1 and 2 K + 1 users.  With 64 slots:
    sub-chunks with fewer steps than lane groups, waves with empty ranges, missing classes."""
    def make():
        n, S = 40, 30
        g = torch.Generator().manual_seed(3 + m)
        R = torch.stack([torch.randperm(n - 3, generator=g)[:S] + 3 for _ in range(m)]).to(torch.int32)
        for item, users in ((0, K), (1, K + 1), (2, 2 * K + 1)):
            R[:min(users, m), item] = item
        idx = torch.tensor([[u, 3 + (7 * u) % (n - 3)] for u in range(m) if u % 5 != 2] or [[0, 5]])
        return idx, torch.ones(idx.shape[0]), R, m, n, 128, S
    return make


def _only_fill_1():
    """8 users with disjoint negatives, one interaction on an item nobody samples: every step has one entry."""
    m, n, S = 8, 4096, 16
    R = ((torch.arange(m)[:, None] + m * torch.arange(S)[None, :]) * 32).to(torch.int32)
    return torch.tensor([[0, 5]]), torch.ones(1), R, m, n, 128, S


def _only_fill_4():
    """4 users with identical rows of R and the same interaction: every step is full."""
    m, n, S = 4, 500, 20
    R = torch.randperm(n, generator=torch.Generator().manual_seed(8))[:S].to(torch.int32).repeat(m, 1)
    return torch.tensor([[u, 7] for u in range(m)]), torch.ones(m), R, m, n, 128, S


# name -> (problem on the CPU, item slices of the WmrbPlan, bytes of a scores7 slice, slots per sub-chunk)
SHAPES = {
    'general': (_general(128), 2, 300 * 512, 512),      # second group of 44 users, slices of 300 rows
    'runs-70': (_run_lengths(70), 1, None, 64),
    'runs-1': (_run_lengths(1), 1, None, 64),
    'fill-1': (_only_fill_1, 1, 1024 * 512, None),
    'fill-4': (_only_fill_4, 1, None, None),
    'r65': (_general(65), 2, 300 * 512, 512),
    'r96': (_general(96), 2, 300 * 512, 512),
}


def _tables(m, n, r, seed, dyadic):
    g = torch.Generator().manual_seed(seed)
    if dyadic:
        return torch.randint(-8, 9, (m, r), generator=g).float() / 8, torch.randint(-8, 9, (n, r), generator=g).float() / 8
    return torch.randn(m, r, generator=g) * 0.3, torch.randn(n, r, generator=g) * 0.3


def _args(name, dyadic):
    make, slices, slice_bytes, slots = SHAPES[name]
    idx, val, R, m, n, r, S = make()
    U, V = _tables(m, n, r, 17 + m + n, dyadic)
    return [x.cuda() for x in (idx, val, R, U, V)] + [m, n, r, S, torch.float32, slices], dict(slice_bytes=slice_bytes, slots=slots)


def _classes(s7):
    """Which of the classes 4, 3, 2, 1 the plan has steps in."""
    return [bool(x) for x in (s7.sub_fill.sum(0) > 0).tolist()]


@pytest.mark.parametrize('name', list(SHAPES))
def test_fill_order_gives_the_scores_of_item_order_bit_for_bit(eng, monkeypatch, name):
    args, kw = _args(name, dyadic=False)
    monkeypatch.setenv('TMF_S7_FILL', '0')
    a = epoch(eng, monkeypatch, True, *args, **kw)
    monkeypatch.setenv('TMF_S7_FILL', '1')
    b = epoch(eng, monkeypatch, True, *args, **kw)
    sa, sb = a['wplan'].s7, b['wplan'].s7
    assert sa.sub_wave is None and sb.sub_wave is not None and sb.n_steps == sa.n_steps
    assert torch.equal(a['sp'], b['sp']) and torch.equal(a['pk'], b['pk'])
    if name == 'fill-1':
        assert _classes(sb) == [False, False, False, True]
    if name == 'fill-4':
        assert _classes(sb) == [True, False, False, False]
    if name in ('general', 'runs-70'):
        assert _classes(sb) == [True, True, True, True]
    if name.startswith('runs'):
        W = sb.sub_wave.shape[1] - 1
        assert bool((sb.sub_wave[:, 1:] == sb.sub_wave[:, :W]).any())   # waves with empty ranges


@pytest.mark.parametrize('name', list(SHAPES))
def test_fill_order_epoch_equals_scores3_on_dyadic_tables(eng, monkeypatch, name):
    args, kw = _args(name, dyadic=True)
    monkeypatch.setenv('TMF_S7_FILL', '1')
    a = epoch(eng, monkeypatch, False, *args)
    b = epoch(eng, monkeypatch, True, *args, **kw)
    assert b['wplan'].s7.sub_wave is not None
    for k in ('sp', 'pk', 'D', 'delta', 'U', 'V'):
        assert torch.equal(a[k], b[k]), k
    assert a['loss'] == b['loss']


def test_order_by_fill_on_46_million_synthetic_steps(eng):
    """4.6e7 synthetic step records in 20000 sub-chunks - past 2^25 rows, the most a test of a second can hold; the benchmark has
    4.4e8 - with the item field holding the record's index: afterwards every record is still in its sub-chunk, fills descend inside
    a sub-chunk, the original order is kept inside a class, sub_fill counts the classes, and no record is lost, doubled or torn.
    (A first form of order_by_fill, with repeat_interleave and index_select(out=), passed this size and still tore the plan at
    4.4e8 steps; tools/time_scores7_fill_c4.py checks the losses of the two orders against each other at that size.)"""
    from teamoflow_amd import _lib
    lib = _lib.get()
    cap, W = lib.tmf_wmrb_scores7_slots(), lib.tmf_wmrb_scores7_waves()
    g = torch.Generator(device='cuda').manual_seed(2)
    n_sub = 20000
    per_sub = torch.randint(2000, 2600, (n_sub,), generator=g, device='cuda')
    sub_step = torch.cat([torch.zeros(1, dtype=torch.int64, device='cuda'), torch.cumsum(per_sub, 0)])
    n = int(sub_step[-1])
    assert n > 2 ** 25
    fill = torch.randint(1, K + 1, (n,), generator=g, device='cuda')
    word = torch.randint(0, 2 ** 31 - 1, (n,), generator=g, device='cuda', dtype=torch.int64)
    slot = torch.where(torch.arange(K, device='cuda')[None, :] < fill[:, None], (word[:, None] >> torch.tensor([0, 7, 13, 17], device='cuda')) % cap, cap)
    steps = torch.zeros(n + 1, 4, dtype=torch.int32, device='cuda')
    steps[:n, 0] = torch.arange(n, device='cuda', dtype=torch.int32)
    steps[:n, 1] = (word % 2 ** 31).to(torch.int32)
    steps[:n, 2] = (slot[:, 0] | (slot[:, 1] << 16)).to(torch.int32)
    steps[:n, 3] = (slot[:, 2] | (slot[:, 3] << 16)).to(torch.int32)
    before = steps.clone()
    s7 = object.__new__(eng.Scores7Plan)
    s7.pad_slot, s7.n_steps, s7.n_sub, s7.steps, s7.sub_step = cap, n, n_sub, steps, sub_step
    s7.order_by_fill()
    after = s7.steps
    ident = after[:n, 0].long()
    assert torch.equal(after[:n], before[ident]) and bool((after[n:] == 0).all())      # whole records of the input ...
    assert torch.equal(torch.sort(ident)[0], torch.arange(n, device='cuda'))            # ... each exactly once
    sub_now = torch.searchsorted(sub_step, torch.arange(n, device='cuda'), right=True) - 1
    assert torch.equal(torch.searchsorted(sub_step, ident, right=True) - 1, sub_now)    # in the sub-chunk it came from
    f = fill[ident]
    same = sub_now[1:] == sub_now[:-1]
    assert bool((f[1:] <= f[:-1])[same].all())                                          # fills descend
    assert bool((ident[1:] > ident[:-1])[same & (f[1:] == f[:-1])].all())               # stable inside a class
    cnt = torch.bincount(sub_now * K + (K - f), minlength=K * n_sub).view(n_sub, K)
    assert torch.equal(cnt, s7.sub_fill.long())
    sw = s7.sub_wave.long()
    assert bool((sw[:, 0] == 0).all()) and torch.equal(sw[:, W], per_sub) and bool((sw[:, 1:] >= sw[:, :W]).all())


def _launch(lib, _lib, s7, st, m, n, r, sp, pk, fill):
    head = [_lib.ptr(s7.steps), _lib.ptr(s7.place), _lib.ptr(s7.sub_step), _lib.ptr(s7.sub_place), _lib.ptr(s7.chunk_sub)]
    tail = [s7.n_groups, s7.n_slices, m, n, _lib.ptr(st.U), _lib.ptr(st.V), _lib.ptr(sp), _lib.ptr(pk), r, _lib.stream_ptr()]
    if fill:
        _lib.check(lib.tmf_wmrb_scores7_fill_f32(*head, _lib.ptr(s7.sub_wave), _lib.ptr(s7.sub_fill), *tail), lib)
    else:
        _lib.check(lib.tmf_wmrb_scores7_f32(*head, *tail), lib)
    torch.cuda.synchronize()


@pytest.mark.parametrize('name', ['general', 'runs-70'])
def test_fill_entry_point_writes_every_score_and_nothing_else(eng, monkeypatch, name):
    """sp and pk prefilled with NaN, through the new entry point: every element is finite afterwards and a guard region behind each
    buffer stays untouched.  The old entry point on the SAME fill-ordered steps gives the same sp and pk."""
    from teamoflow_amd import _lib
    lib = _lib.get()
    (idx, val, R, U, V, m, n, r, S, dtype, slices), kw = _args(name, dyadic=False)
    monkeypatch.setenv('TMF_S7_FILL', '1')
    plan, wplan, st = make_state(eng, monkeypatch, True, idx, val, R, U, V, m, n, r, dtype, slices, **kw)
    s7, G = wplan.s7, 4096
    assert s7 is not None and s7.sub_wave is not None
    out = {}
    for fill in (True, False):
        sp = torch.full((m * S + G,), float('nan'), device='cuda')
        pk = torch.full((plan.nnz + G,), float('nan'), device='cuda')
        sp[m * S:] = 12345.0
        pk[plan.nnz:] = 54321.0
        _launch(lib, _lib, s7, st, m, n, r, sp, pk, fill)
        assert bool(torch.isfinite(sp[:m * S]).all()) and bool(torch.isfinite(pk[:plan.nnz]).all())
        assert bool((sp[m * S:] == 12345.0).all()) and bool((pk[plan.nnz:] == 54321.0).all())
        out[fill] = (sp, pk)
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    U64, V64 = st.U[:, :r].double(), st.V[:, :r].double()
    want = torch.einsum('ur,usr->us', U64, V64[wplan.R.long()])
    assert float((out[True][0][:m * S].view(m, S).double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
