"""Popularity-weighted negative sampling on the GPU.

tmf_sample_rows_weighted against its definition: the table utils.random_sampler_device(weights=...) draws on the CPU (integer
arithmetic only), bit for bit - at the row lengths around every step of the template ladder and of a wave, on weights exactly at
the border of the admission rule (4 H = 3 T: the most redraw rounds an admitted table takes) and on a catalog of 100 000 items with
runs of zero weight (the full depth of the bisection).  fit(negative_sampling='popularity') on the engine against the uniform fit
whose random_ind is the drawn table: the setting changes which table is read and nothing else."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
LR = 0.05
POISON = -7
GUARD_ROWS = 3


@pytest.fixture(scope='module')
def tm():
    from teamoflow_amd import _engine, _lib, _ops
    from teamoflow_amd.mf import loss_graphs as LG
    from teamoflow_amd.mf import utils
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye

    class NS:
        pass
    ns = NS()
    ns.lib, ns.L, ns.E, ns.ops, ns.LG, ns.MF, ns.Fixed, ns.Sparse, ns.eye, ns.utils = \
        _lib.get(), _lib, _engine, _ops, LG, MatrixFactorization, FixedInitializer, SparseInteractions, eye, utils
    ns.oracle = utils.random_sampler_device
    return ns


@pytest.fixture
def engine_only(tm, monkeypatch):
    """_fit_generic refuses to run: a fit that passes ran on the engine."""
    def refuse(self, *a, **k):
        raise AssertionError('_fit_generic was called')
    monkeypatch.setattr(tm.MF, '_fit_generic', refuse)


# ------------------------------------------------------------------------------------------------------------------------
# the kernel
# ------------------------------------------------------------------------------------------------------------------------
def border_weights(n, s):
    """s heavy items, spread over the ids, that hold exactly 3/4 of the total: H = 3 (n - s) s, T = 4 (n - s) s."""
    q = torch.full((n,), s, dtype=torch.int64)
    q[torch.arange(s) * (n // s)] = 3 * (n - s)
    assert 4 * int(torch.topk(q, s)[0].sum()) == 3 * int(q.sum())
    return q


def catalog_weights(n=100_000):
    """Zipf counts under power 0.75 with runs of zero weight at the front, in the middle and at the end (and single zeros)."""
    from teamoflow_amd.mf.utils import popularity_weights
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    q = popularity_weights(torch.floor(1e6 / (1.0 + perm.double())), 0.75)
    q[:1000] = 0
    q[n // 2:n // 2 + 5000] = 0
    q[-777:] = 0
    q[torch.arange(2000, n, 97)] = 0
    return q


def draw_guarded(tm, n, m, s, q, seed=0, offset=0):
    """The kernel's rows in a poisoned buffer with guard rows behind them, which must stay as they were."""
    assert tm.lib.tmf_sample_rows_weighted_supported(n, s) == 1
    buf = torch.full((m + GUARD_ROWS, s), POISON, dtype=torch.int32, device='cuda')
    out = tm.ops.sample_negatives(n, m, s, seed=seed, device='cuda', user_offset=offset, out=buf[:m], weights=q)
    assert out.shape == (m, s) and (m == 0 or out.data_ptr() == buf.data_ptr())
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[m:] == POISON).all()), 'the kernel wrote behind its rows'
    return host[:m]


def redraw_rounds(tm, n, m, s, q, seed):
    """Rounds of the definition's rejection loop that redraw something, restated with a counter."""
    u = tm.utils
    cum = torch.cumsum(q, 0)
    total = int(cum[-1])
    rows, pos = torch.arange(m)[:, None], torch.arange(s)[None, :]
    blk = torch.sort(u.weighted_item(u.hash_below(u.counter_hash(seed, rows, pos, 2), total), cum), dim=1)[0]
    for rnd in range(3, 259):
        dup = torch.zeros_like(blk, dtype=torch.bool)
        dup[:, 1:] = blk[:, 1:] == blk[:, :-1]
        if not bool(dup.any()):
            return rnd - 3
        blk = torch.sort(torch.where(dup, u.weighted_item(u.hash_below(u.counter_hash(seed, rows, pos, rnd), total), cum), blk), dim=1)[0]
    raise AssertionError('no table')


S_LADDER = [1, 63, 64, 65, 128, 129, 256, 1024, 1025, 4096]


@pytest.mark.parametrize('s', S_LADDER)
def test_rows_equal_the_definition_at_the_border_of_the_admission_rule(tm, s):
    """n_items = 2 S + 3 with S items that hold 3/4 of the mass: just inside the rule.  A number of users that is no multiple of
    the rows a workgroup holds, and a non-zero user_offset."""
    n, m = 2 * s + 3, 203 if s <= 256 else 37
    q = border_weights(n, s)
    got = draw_guarded(tm, n, m, s, q, seed=s, offset=5)
    assert torch.equal(got, tm.oracle(n, m, s, seed=s, device='cpu', user_offset=5, weights=q))
    if s >= 63:
        rounds = redraw_rounds(tm, n, 37, s, q, seed=s)
        print('redraw rounds', s, rounds)
        assert rounds >= 10, rounds    # far past the two or three rounds uniform rows need


@pytest.mark.parametrize('s', S_LADDER)
def test_rows_equal_the_definition_on_a_catalog_of_100k_with_zero_runs(tm, s):
    n, m = 100_000, 203 if s <= 256 else 37
    q = catalog_weights(n)
    got = draw_guarded(tm, n, m, s, q, seed=100 + s)
    assert torch.equal(got, tm.oracle(n, m, s, seed=100 + s, device='cpu', weights=q))
    assert bool((q[got.long()] > 0).all())


def test_grid_tail_seed_offset_and_no_rows(tm):
    n, m, s = 5000, 1001, 48      # four rows per workgroup: the last workgroup holds one
    q = catalog_weights(n)
    want = tm.oracle(n, m, s, seed=9, device='cpu', weights=q)
    got = draw_guarded(tm, n, m, s, q, seed=9)
    assert torch.equal(got, want)
    assert torch.equal(draw_guarded(tm, n, m, s, q, seed=9), got), 'a second call gives other bits'
    assert not torch.equal(draw_guarded(tm, n, 300, s, q, seed=10), got[:300])
    assert torch.equal(draw_guarded(tm, n, 300, s, q, seed=9, offset=555), want[555:855])
    assert torch.equal(draw_guarded(tm, n, 1, s, q, seed=9, offset=1000), want[1000:])
    assert tuple(draw_guarded(tm, n, 0, s, q, seed=9, offset=3).shape) == (0, s)
    fresh = tm.ops.sample_negatives(n, 50, s, seed=9, device='cuda', weights=q)         # without out=
    assert fresh.is_cuda and fresh.dtype == torch.int32 and torch.equal(fresh.cpu(), want[:50])
    big, offset = 2 ** 63 + 12345, 2 ** 33                                              # a seed that wraps, user ids beyond 32 bits
    assert torch.equal(draw_guarded(tm, n, 70, s, q, seed=big, offset=offset),
                       tm.oracle(n, 70, s, seed=big, device='cpu', user_offset=offset, weights=q))
    ones = torch.ones(n, dtype=torch.int64)                                             # unit weights: the uniform kernel's table
    assert torch.equal(draw_guarded(tm, n, 70, s, ones, seed=4), tm.ops.sample_negatives(n, 70, s, seed=4, device='cuda').cpu())


def test_a_total_of_almost_33_bits(tm):
    n, m, s = 3000, 60, 200
    q = torch.full((n,), (2 ** 33 - 1) // n, dtype=torch.int64)
    q[::7] //= 3
    assert 2 ** 32 < int(q.sum()) < 2 ** 33
    assert torch.equal(draw_guarded(tm, n, m, s, q, seed=5), tm.oracle(n, m, s, seed=5, device='cpu', weights=q))


def test_invalid_arguments_return_an_error_and_launch_nothing(tm):
    n, m, s = 500, 20, 32
    cum = torch.cumsum(torch.ones(n, dtype=torch.int64), 0).cuda()
    R = torch.full((m, s), POISON, dtype=torch.int32, device='cuda')
    failed = torch.zeros(1, dtype=torch.int32, device='cuda')
    P, stream = tm.L.ptr, tm.L.stream_ptr()
    call = tm.lib.tmf_sample_rows_weighted
    zero, wide = torch.zeros_like(cum), cum.clone()
    wide[-1] = 2 ** 33
    for args in ((None, n, m, s, 0, 0, P(R), P(failed)), (P(cum), n, m, s, 0, 0, None, P(failed)), (P(cum), n, m, s, 0, 0, P(R), None),
                 (P(cum), n, -1, s, 0, 0, P(R), P(failed)), (P(cum), n, m, s, 0, -1, P(R), P(failed)),
                 (P(cum), n, m, 0, 0, 0, P(R), P(failed)), (P(cum), n, m, 4097, 0, 0, P(R), P(failed)),
                 (P(cum), 0, m, s, 0, 0, P(R), P(failed)), (P(cum), -5, m, s, 0, 0, P(R), P(failed)),
                 (P(zero), n, m, s, 0, 0, P(R), P(failed)), (P(wide), n, m, s, 0, 0, P(R), P(failed))):
        assert call(*args, stream) == tm.L.HEADER.constants['TMF_E_INVALID'], args
        assert b'tmf_sample_rows_weighted' in tm.lib.tmf_last_error()
    torch.cuda.synchronize()
    assert bool((R == POISON).all()) and int(failed) == 0
    assert call(P(cum), n, 0, s, 0, 0, None, P(failed), stream) == 0      # no users: TMF_OK
    assert call(P(cum), n, m, s, 0, 0, P(R), P(failed), stream) == 0      # and the same buffers, valid, are drawn into
    torch.cuda.synchronize()
    assert int(R.min()) >= 0 and int(failed) == 0
    over = torch.ones(n, dtype=torch.int64)
    over[:s] = 10 * n                                                      # the wrapper refuses what the rule does not admit
    with pytest.raises(ValueError, match='smaller power or fewer samples'):
        tm.ops.sample_negatives(n, m, s, device='cuda', weights=over)
    with pytest.raises(ValueError, match='out must be'):
        tm.ops.sample_negatives(n, m, s, device='cuda', weights=torch.ones(n, dtype=torch.int64), out=R[:, :8])


def test_rows_longer_than_the_kernel_takes_get_the_torch_table(tm):
    n, m, s = 20_000, 9, 4097
    q = catalog_weights(n)
    assert tm.lib.tmf_sample_rows_weighted_supported(n, s) == 0
    got = tm.ops.sample_negatives(n, m, s, seed=3, device='cuda', user_offset=2, weights=q)
    assert got.is_cuda and torch.equal(got.cpu(), tm.oracle(n, m, s, seed=3, device='cpu', user_offset=2, weights=q))


# ------------------------------------------------------------------------------------------------------------------------
# the engine
# ------------------------------------------------------------------------------------------------------------------------
def problem(m=200, n=150, r=16, S=32, seed=4):
    rng = np.random.default_rng(seed)
    density = 0.25 / (1.0 + np.arange(n) / 8.0)                        # popular items first
    idx = np.argwhere(rng.random((m, n)) < density[None, :])          # row-major, no duplicates
    val = rng.choice(np.array([-1, 0, 1, 2, 3, 4, 5], np.float32), idx.shape[0])
    scale = 1.2 / r ** 0.25
    return dict(m=m, n=n, r=r, S=S, idx=idx, val=val, U0=(rng.standard_normal((m, r)) * scale).astype(np.float32),
                V0=(rng.standard_normal((n, r)) * scale).astype(np.float32),
                R=np.stack([rng.choice(n, S, replace=False) for _ in range(m)]).astype(np.int32))


def make_model(tm, p, loss, U0=None, V0=None, R=None, **attrs):
    model = tm.MF(p['r'], loss_graph=getattr(tm.LG, loss)(), user_weight_graph=tm.Fixed(p['U0'] if U0 is None else U0),
                  item_weight_graph=tm.Fixed(p['V0'] if V0 is None else V0), n_users=p['m'], n_items=p['n'], n_samples=p['S'])
    model.verbose = False
    model.random_ind = torch.as_tensor(p['R'] if R is None else R)
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


def fit(tm, model, p, epochs):
    model.fit(epochs, tm.eye(p['m']), tm.eye(p['n']), tm.Sparse(p['idx'], p['val'], (p['m'], p['n'])), lr=LR)
    return model


def weights_of(tm, p, power=0.75):
    counts = np.bincount(p['idx'][p['val'] > 0, 1], minlength=p['n'])
    assert counts.max() >= 5 * max(1, counts.min())
    return tm.utils.popularity_weights(torch.as_tensor(counts), power)


def same_fit(a, b):
    return a.loss_history_ == b.loss_history_ and torch.equal(a.user_embedding, b.user_embedding) \
        and torch.equal(a.item_embedding, b.item_embedding)


@pytest.mark.parametrize('loss, attrs, epochs', [('WMRBLoss', {}, 3), ('BPRLoss', {}, 3), ('WARPLoss', {}, 8), ('SampledSoftmaxLoss', {}, 3),
                                                 ('BPRLoss', dict(scalar_item_bias=True), 3)],
                         ids=['wmrb', 'bpr', 'warp-graph', 'softmax', 'bpr-item-bias'])
def test_a_popularity_fit_is_the_uniform_fit_on_the_drawn_table(tm, engine_only, loss, attrs, epochs):
    """Eight epochs of the tiny problem run as replays of a captured hipGraph: the drawn table is static like any other."""
    p, seed = problem(), 21
    q = weights_of(tm, p)
    table0 = tm.ops.sample_negatives(p['n'], p['m'], p['S'], seed=seed, device='cuda', weights=q)
    assert torch.equal(table0.cpu(), tm.oracle(p['n'], p['m'], p['S'], seed=seed, device='cpu', weights=q))
    pop = fit(tm, make_model(tm, p, loss, negative_sampling='popularity', sample_seed=seed, **attrs), p, epochs)
    uni = fit(tm, make_model(tm, p, loss, R=table0.cpu(), **attrs), p, epochs)
    assert same_fit(pop, uni) and pop.graph_epochs_ == uni.graph_epochs_ and (pop.graph_epochs_ == 8 or epochs != 8 or 'TMF_NO_GRAPH' in os.environ)
    assert pop.resample_rounds_ == 1 and pop.resample_seconds_ == 0.0
    assert torch.equal(pop._state.wplan.R_model, table0)
    assert torch.equal(torch.as_tensor(pop.random_ind), torch.as_tensor(p['R']))          # random_ind is never changed
    if attrs:
        assert pop.item_bias_ is not None and torch.equal(pop.item_bias_, uni.item_bias_) and bool(pop.item_bias_.abs().max() > 0)
    assert not same_fit(pop, fit(tm, make_model(tm, p, loss, **attrs), p, epochs))         # and the setting means something


def test_three_rounds_of_one_epoch_are_the_manual_sequence(tm, engine_only, monkeypatch):
    p, seed, loss = problem(seed=5), 7, 'WARPLoss'
    q = weights_of(tm, p, 0.5)
    drawn, real = [], tm.ops.sample_negatives

    def spy(*a, **k):
        drawn.append((k['seed'], torch.equal(k['weights'], q)))
        return real(*a, **k)
    monkeypatch.setattr(tm.ops, 'sample_negatives', spy)
    whole = fit(tm, make_model(tm, p, loss, negative_sampling='popularity', sampling_power=0.5, resample_every=1, sample_seed=seed), p, 3)
    monkeypatch.setattr(tm.ops, 'sample_negatives', real)
    assert drawn == [(seed + j, True) for j in range(3)]
    assert whole.resample_rounds_ == 3 and 0.0 < whole.resample_seconds_ < whole.fit_seconds_
    assert torch.equal(torch.as_tensor(whole.random_ind), torch.as_tensor(p['R']))
    U, V, history = p['U0'], p['V0'], []
    for j in range(3):
        table = real(p['n'], p['m'], p['S'], seed=seed + j, device='cuda', weights=q)
        assert torch.equal(table.cpu(), tm.oracle(p['n'], p['m'], p['S'], seed=seed + j, device='cpu', weights=q))
        step = fit(tm, make_model(tm, p, loss, U0=U, V0=V, R=table.cpu()), p, 1)
        U, V = step.user_embedding.float().cpu().numpy().copy(), step.item_embedding.float().cpu().numpy().copy()
        history += step.loss_history_
    assert whole.loss_history_ == history
    assert np.array_equal(whole.user_embedding.cpu().numpy(), U) and np.array_equal(whole.item_embedding.cpu().numpy(), V)
    assert torch.equal(whole._state.wplan.R_model.cpu(), table.cpu())
