"""Popularity-weighted negative sampling without a GPU: the weighted table's definition (utils.random_sampler_device(weights=...)) -
unit weights are the unweighted table, structure, marginals, the admission rule -, utils.popularity_weights, the CPU route of
_ops.sample_negatives(weights=...), and negative_sampling / sampling_power on the model through the generic loop: off is today's
fit, the schedule of seeds and weights, save / load, the refusals and their table."""
import importlib.util
import json
import os
import string

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

M, N, S, R_COMP = 40, 60, 12, 4
LR = 0.05
# two-level weights exactly at the border 4 H = 3 T of the admission rule: (n_items, n_samples)
BORDER_SHAPES = [(600, 256), (130, 65), (200, 100), (2100, 1024), (8200, 4096)]


@pytest.fixture
def no_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)


def border_weights(n, s):
    """s heavy items that hold exactly 3/4 of the total: H = 3 (n - s) s, T = 4 (n - s) s.  The heavy items are spread over the ids."""
    q = torch.full((n,), s, dtype=torch.int64)
    q[torch.arange(s) * (n // s)] = 3 * (n - s)
    return q


def sampler(n, m, s, **kw):
    from teamoflow_amd.mf.utils import random_sampler_device
    return random_sampler_device(n, m, s, device='cpu', **kw)


# ------------------------------------------------------------------------------------------------------------------------
# the distribution
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, m, s', [(300, 64, 32), (130, 50, 65), (1000, 20, 256)])
def test_unit_weights_give_the_unweighted_table_bit_for_bit(n, m, s):
    ones = torch.ones(n, dtype=torch.int64)
    for seed, offset in ((0, 0), (7, 12345), (2 ** 40 + 3, 2 ** 33)):
        want = sampler(n, m, s, seed=seed, user_offset=offset)
        got = sampler(n, m, s, seed=seed, user_offset=offset, weights=ones)
        assert got.dtype == torch.int32 and torch.equal(got, want), (seed, offset)


def zero_run_weights(n, seed=0):
    """Positive weights with runs of zeros at the front, in the middle and at the end."""
    q = torch.randint(1, 50, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)
    q[:n // 10] = 0
    q[n // 2:n // 2 + n // 8] = 0
    q[-(n // 9):] = 0
    q[n // 4] = 0
    return q


def test_rows_are_distinct_in_range_and_blocks_are_slices():
    n, m, s = 400, 90, 48
    q = zero_run_weights(n)
    table = sampler(n, m, s, seed=3, weights=q)
    assert tuple(table.shape) == (m, s) and table.dtype == torch.int32
    assert int(table.min()) >= 0 and int(table.max()) < n
    assert all(len(set(row)) == s for row in table.tolist())
    assert bool((q[table.long()] > 0).all())                      # an item of weight 0 never appears
    assert not torch.equal(torch.sort(table, 1)[0], table)        # the rows are shuffled, not sorted
    for b, e in ((0, 1), (17, 60), (89, 90)):
        assert torch.equal(sampler(n, e - b, s, seed=3, weights=q, user_offset=b), table[b:e])
    assert torch.equal(sampler(n, m, s, seed=3, weights=q, rows_per_block=7), table)   # the row of a user is its own
    assert not torch.equal(sampler(n, m, s, seed=4, weights=q), table)
    assert tuple(sampler(n, 0, s, seed=3, weights=q).shape) == (0, s)


def test_the_draw_reaches_the_first_and_last_item_of_nonzero_weight():
    from teamoflow_amd.mf.utils import weighted_cum, weighted_item
    q = torch.tensor([0, 0, 3, 0, 1, 5, 0, 0, 2, 0, 0], dtype=torch.int64)
    cum = weighted_cum(q, q.numel(), 1)
    total = int(cum[-1])
    assert total == 11
    x = torch.arange(total)
    assert weighted_item(x, cum).tolist() == [2, 2, 2, 4, 5, 5, 5, 5, 5, 8, 8]
    assert int(weighted_item(torch.tensor(0), cum)) == 2 and int(weighted_item(torch.tensor(total - 1), cum)) == 8
    counts = torch.bincount(weighted_item(x, cum), minlength=q.numel())
    assert torch.equal(counts, q)                                  # every x in [0, T) has an item, item i exactly q_i of them


def test_marginals_of_single_draws_follow_the_weights():
    """S = 1: no rejection, so the marginal is exactly q / T (up to the modulo bias, below T / 2^53).  Every count within 6 standard
    deviations of m p."""
    n, m = 50, 400_000
    from teamoflow_amd.mf.utils import popularity_weights
    q = popularity_weights(torch.floor(1000.0 / torch.arange(1, n + 1, dtype=torch.float64)), 0.75)   # (floor(1000 / i) + 1)^0.75
    table = sampler(n, m, 1, seed=1, weights=q)
    counts = torch.bincount(table.reshape(-1).long(), minlength=n).double()
    p = q.double() / q.sum()
    z = (counts - m * p) / torch.sqrt(m * p * (1 - p))
    print('worst deviation', float(z.abs().max()))
    assert float(z.abs().max()) < 6.0


# ------------------------------------------------------------------------------------------------------------------------
# the admission rule and the other refusals of the weights
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, s', BORDER_SHAPES)
def test_the_admission_rule_is_4h_le_3t_in_integers(n, s):
    from teamoflow_amd import _ops
    q = border_weights(n, s)
    heavy, total = int(torch.topk(q, s)[0].sum()), int(q.sum())
    assert 4 * heavy == 3 * total
    table = sampler(n, 24, s, seed=2, weights=q)                  # at the border: drawn
    assert all(len(set(row)) == s for row in table.tolist())
    over = q.clone()
    over[int(torch.argmax(q))] += 1                                # 4 (H + 1) > 3 (T + 1)
    for draw in (lambda: sampler(n, 24, s, seed=2, weights=over),
                 lambda: _ops.sample_negatives(n, 24, s, seed=2, device='cpu', weights=over)):
        with pytest.raises(ValueError, match='smaller power or fewer samples'):
            draw()
    under = q.clone()
    under[int(torch.argmin(q))] += 1                               # 4 H < 3 (T + 1)
    sampler(n, 2, s, seed=2, weights=under)


def test_the_rule_decides_on_random_weights_exactly():
    from teamoflow_amd.mf.utils import weighted_cum
    g = torch.Generator().manual_seed(9)
    seen = set()
    for _ in range(300):
        n = int(torch.randint(2, 40, (1,), generator=g))
        s = int(torch.randint(1, n + 1, (1,), generator=g))
        q = torch.randint(0, 6, (n,), generator=g, dtype=torch.int64) ** int(torch.randint(1, 4, (1,), generator=g))
        total = int(q.sum())
        if total == 0:
            continue
        admitted = 4 * sum(sorted(q.tolist(), reverse=True)[:s]) <= 3 * total
        seen.add(admitted)
        if admitted:
            assert torch.equal(weighted_cum(q, n, s), torch.cumsum(q, 0))
        else:
            with pytest.raises(ValueError, match='3/4'):
                weighted_cum(q, n, s)
    assert seen == {True, False}


def test_bad_weights_are_refused_before_anything_is_drawn():
    from teamoflow_amd import _ops
    n, s = 100, 10
    ones = torch.ones(n, dtype=torch.int64)
    neg = ones.clone()
    neg[5] = -1
    huge = ones.clone()
    huge[0] = 2 ** 33
    for bad, err in ((ones[:-1], ValueError), (ones.reshape(10, 10), ValueError), (ones.to(torch.int32), TypeError),
                     (ones.double(), TypeError), (ones.tolist(), TypeError), (neg, ValueError), (ones * 0, ValueError),
                     (huge, ValueError), (ones * (2 ** 33 // n + 1), ValueError)):
        with pytest.raises(err):
            _ops.sample_negatives(n, 3, s, device='cpu', weights=bad)
        with pytest.raises(err):
            sampler(n, 3, s, weights=bad)
    with pytest.raises(ValueError):
        _ops.sample_negatives(n, 3, n + 1, device='cpu', weights=ones)
    with pytest.raises(ValueError):
        _ops.sample_negatives(n, -1, s, device='cpu', weights=ones)
    # fewer items of non-zero weight than samples: they hold all the mass
    few = ones * 0
    few[:s - 1] = 1
    with pytest.raises(ValueError, match='3/4'):
        sampler(n, 3, s, weights=few)


@pytest.mark.parametrize('n, m, s, seed, offset', [(60, 40, 12, 3, 0), (400, 9, 48, 2 ** 40 + 1, 2 ** 33), (130, 5, 65, 1, 2)])
def test_sample_negatives_on_the_cpu_is_the_torch_function(no_gpu, n, m, s, seed, offset):
    from teamoflow_amd import _ops
    q = border_weights(n, s) if (n, s) in BORDER_SHAPES else zero_run_weights(n)
    want = sampler(n, m, s, seed=seed, user_offset=offset, weights=q)
    got = _ops.sample_negatives(n, m, s, seed=seed, device='cpu', user_offset=offset, weights=q)
    assert got.dtype == torch.int32 and got.device.type == 'cpu' and torch.equal(got, want)
    out = torch.full((m, s), -7, dtype=torch.int32)
    assert _ops.sample_negatives(n, m, s, seed=seed, device='cpu', user_offset=offset, out=out, weights=q) is out and torch.equal(out, want)


def test_the_entry_points_are_declared_bound_and_refuse_before_any_launch():
    """No GPU here: a call that got as far as reading cum or launching would fail differently; these return first."""
    import ctypes
    import re
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    declared = set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    lib = _lib.load_library()
    for name in ('tmf_sample_rows_weighted_supported', 'tmf_sample_rows_weighted'):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    make = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS :=.*\btmf_sample_weighted\.hip\b', make, re.M)
    ok = lib.tmf_sample_rows_weighted_supported
    assert ok(1, 1) == 1 and ok(100, 4096) == 1 and ok(100, 4097) == 0 and ok(100, 0) == 0 and ok(0, 1) == 0 and ok(2 ** 31 - 1, 64) == 1
    host = (ctypes.c_double * 8)()              # stands for any non-null buffer: never dereferenced
    H = ctypes.cast(host, ctypes.c_void_p)
    for args in ((None, 100, 5, 10, 0, 0, H, H), (H, 100, 5, 10, 0, 0, None, H), (H, 100, 5, 10, 0, 0, H, None),
                 (H, 100, -1, 10, 0, 0, H, H), (H, 100, 5, 10, 0, -1, H, H), (H, 100, 5, 0, 0, 0, H, H), (H, 100, 5, 4097, 0, 0, H, H),
                 (H, 0, 5, 10, 0, 0, H, H), (H, -3, 5, 10, 0, 0, H, H)):
        assert lib.tmf_sample_rows_weighted(*args, None) == -1 and b'tmf_sample_rows_weighted' in lib.tmf_last_error(), args
    assert lib.tmf_sample_rows_weighted(H, 100, 0, 10, 0, 0, None, H, None) == 0   # no users: nothing to do, nothing read


# ------------------------------------------------------------------------------------------------------------------------
# popularity_weights
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('power', [0.0, 0.5, 0.75, 1.0, 2.0])
def test_popularity_weights(power):
    from teamoflow_amd.mf.utils import popularity_weights
    g = torch.Generator().manual_seed(3)
    counts = torch.cat([torch.randint(0, 100_000, (4000,), generator=g), torch.zeros(1000, dtype=torch.int64), torch.tensor([10 ** 7])])
    q = popularity_weights(counts, power)
    assert q.dtype == torch.int64 and q.device.type == 'cpu' and tuple(q.shape) == tuple(counts.shape)
    assert int(q.min()) >= 1 and int(q.sum()) <= 2 ** 31 + counts.numel()
    order = torch.argsort(counts)
    assert bool((q[order][1:] >= q[order][:-1]).all())                       # monotone in the counts
    assert len(set(q[counts == 0].tolist())) == 1                            # equal counts, equal weights
    if power == 0.0:
        assert len(set(q.tolist())) == 1                                     # uniform in distribution
    else:
        assert int(q.max()) > int(q.min())
    want = np.maximum(1.0, np.floor((counts.numpy().astype(np.float64) + 1.0) ** power / ((counts.numpy().astype(np.float64) + 1.0) ** power).sum() * 2.0 ** 31))
    assert np.array_equal(q.numpy(), want.astype(np.int64))
    assert torch.equal(popularity_weights(counts.to(torch.int32).tolist(), power), q)   # any vector of counts, the host's float64


@pytest.mark.parametrize('bad', [-0.5, float('nan'), float('inf'), -float('inf'), 'x', None])
def test_a_bad_power_is_refused(bad):
    from teamoflow_amd.mf.utils import popularity_weights
    with pytest.raises(ValueError, match='power'):
        popularity_weights(torch.arange(10), bad)


def test_power_zero_is_uniform_in_distribution_not_in_bits():
    from teamoflow_amd.mf.utils import popularity_weights
    n, m, s = 300, 20, 32
    q = popularity_weights(torch.arange(n), 0.0)
    assert len(set(q.tolist())) == 1 and int(q[0]) > 1
    assert 'not the bits' in popularity_weights.__doc__.lower()
    assert not torch.equal(sampler(n, m, s, seed=1, weights=q), sampler(n, m, s, seed=1))


# ------------------------------------------------------------------------------------------------------------------------
# the model, through the generic loop with a plug-in table loss
# ------------------------------------------------------------------------------------------------------------------------
def problem(seed=5):
    rng = np.random.default_rng(seed)
    mask = rng.random((M, N)) < 0.2 * (1.0 / (1.0 + np.arange(N) / 6.0))[None, :] * 3.0   # popular items first
    idx = np.argwhere(mask)
    val = rng.choice(np.array([-1, 0, 1, 2, 3, 4, 5], np.float32), idx.shape[0])
    return dict(idx=idx, val=val, U0=(rng.standard_normal((M, R_COMP)) * 0.7).astype(np.float32),
                V0=(rng.standard_normal((N, R_COMP)) * 0.7).astype(np.float32),
                R=np.stack([rng.choice(N, S, replace=False) for _ in range(M)]))


def plugin_loss():
    from teamoflow_amd.mf import loss_graphs

    class PluginBPR(loss_graphs.BPRLoss):   # a subclass is a plug-in loss: the generic loop on every machine, fed the samples
        pass
    return PluginBPR()


def make(p, loss=None, R=None, init=None, **attrs):
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    model = MatrixFactorization(R_COMP, loss_graph=plugin_loss() if loss is None else loss,
                                user_weight_graph=init or FixedInitializer(p['U0']), item_weight_graph=init or FixedInitializer(p['V0']),
                                n_users=M, n_items=N, n_samples=S)
    model.verbose = False
    model.random_ind = torch.as_tensor(p['R'] if R is None else R)
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


def fit(model, p, epochs):
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    model.fit(epochs, eye(M), eye(N), SparseInteractions(p['idx'], p['val'], (M, N)), lr=LR)
    return model


def same_fit(a, b):
    return torch.equal(a.user_embedding, b.user_embedding) and torch.equal(a.item_embedding, b.item_embedding) \
        and a.loss_history_ == b.loss_history_


def weights_of(p, power):
    from teamoflow_amd.mf.utils import popularity_weights
    counts = np.bincount(p['idx'][p['val'] > 0, 1], minlength=N)
    assert counts.max() >= 4 * max(1, counts.min())
    return popularity_weights(torch.as_tensor(counts), power)


def test_uniform_or_absent_is_todays_fit(no_gpu, monkeypatch):
    from teamoflow_amd import _ops
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    p = problem()
    fresh = MatrixFactorization(3)
    assert (fresh.negative_sampling, fresh.sampling_power) == ('uniform', 0.75)
    calls = []
    real = _ops.sample_negatives

    def spy(*a, **k):
        calls.append(k)
        return real(*a, **k)
    monkeypatch.setattr(_ops, 'sample_negatives', spy)
    default = fit(make(p, resample_every=1, sample_seed=3), p, 3)
    assert len(calls) == 2 and all('weights' not in k for k in calls)        # the call of a uniform fit is the call it always was
    stated = fit(make(p, resample_every=1, sample_seed=3, negative_sampling='uniform', sampling_power=0.2), p, 3)
    bare = make(p, resample_every=1, sample_seed=3)
    del bare.negative_sampling, bare.sampling_power
    fit(bare, p, 3)
    assert same_fit(default, stated) and same_fit(default, bare)
    # the tables of that fit are the unweighted ones: chained by hand, as tests/test_resample_cpu.py does
    one = fit(make(p), p, 1)
    assert one.loss_history_ == default.loss_history_[:1]


def test_a_popularity_fit_is_a_uniform_fit_on_the_drawn_table(no_gpu):
    from teamoflow_amd import _ops
    p, seed = problem(), 21
    q = weights_of(p, 0.75)
    pop = fit(make(p, negative_sampling='popularity', sample_seed=seed), p, 3)
    table0 = _ops.sample_negatives(N, M, S, seed=seed, device='cpu', weights=q)
    assert same_fit(pop, fit(make(p, R=table0), p, 3))
    assert pop.resample_rounds_ == 1 and pop.resample_seconds_ == 0.0
    assert torch.equal(torch.as_tensor(pop.random_ind), torch.as_tensor(p['R']))          # random_ind is never changed
    assert not same_fit(pop, fit(make(p), p, 3))                                           # and the setting means something
    # popular items are drawn more often than under the uniform table
    top = np.argsort(-np.bincount(p['idx'][p['val'] > 0, 1], minlength=N))[:10]
    assert int(torch.isin(table0, torch.as_tensor(top)).sum()) > 1.3 * M * S * 10 / N
    # another power, other weights, another fit; a second fit of the same model starts again from round 0
    assert not same_fit(pop, fit(make(p, negative_sampling='popularity', sample_seed=seed, sampling_power=0.25), p, 3))
    assert same_fit(fit(pop, p, 3), fit(make(p, R=table0), p, 3))


def test_every_round_is_drawn_with_the_seed_of_the_round_and_the_weights(no_gpu, monkeypatch):
    from teamoflow_amd import _ops
    p, seed = problem(), 11
    q = weights_of(p, 0.5)
    calls, real = [], _ops.sample_negatives

    def spy(n_items, n_users, n_samples, **k):
        calls.append((n_items, n_users, n_samples, k['seed'], k['weights'].clone()))
        return real(n_items, n_users, n_samples, **k)
    monkeypatch.setattr(_ops, 'sample_negatives', spy)
    model = fit(make(p, negative_sampling='popularity', sampling_power=0.5, resample_every=1, sample_seed=seed), p, 3)
    assert [c[:4] for c in calls] == [(N, M, S, seed + j) for j in range(3)]
    assert all(c[4].dtype == torch.int64 and torch.equal(c[4], q) for c in calls)
    assert model.resample_rounds_ == 3 and model.fit_seconds_ >= model.resample_seconds_ >= 0.0
    assert torch.equal(torch.as_tensor(model.random_ind), torch.as_tensor(p['R']))
    monkeypatch.setattr(_ops, 'sample_negatives', real)
    # the manual sequence: three one-epoch fits, each from the tables of the one before, on the table of its round
    U, V, history = p['U0'], p['V0'], []
    for j in range(3):
        step = fit(make(dict(p, U0=U, V0=V), R=real(N, M, S, seed=seed + j, device='cpu', weights=q)), p, 1)
        U, V = step.user_embedding.detach().numpy(), step.item_embedding.detach().numpy()
        history += step.loss_history_
    assert history == model.loss_history_ and np.array_equal(model.user_embedding.detach().numpy(), U)


def test_a_loss_without_a_table_ignores_the_setting(no_gpu, monkeypatch):
    from teamoflow_amd import _ops
    from teamoflow_amd.mf import loss_graphs as L

    class PluginSquares(L.LossGraph):   # a loss of the dense [m, n] matrix
        def get_loss(self, tf_interactions, predictions, tf_sample_predictions=None, tf_prediction_serial=None, n_items=None,
                     n_samples=None):
            idx = tf_interactions.indices
            return torch.square(tf_interactions.values.to(predictions.dtype) - predictions[idx[:, 0], idx[:, 1]])
    monkeypatch.setattr(_ops, 'sample_negatives', lambda *a, **k: pytest.fail('nothing to draw'))
    p = problem()
    a = fit(make(p, PluginSquares(), negative_sampling='popularity', sampling_power=0.5), p, 2)
    assert same_fit(a, fit(make(p, PluginSquares()), p, 2)) and a.resample_rounds_ == 0


def test_the_table_is_still_required(no_gpu):
    from teamoflow_amd.mf.matrix_factorization import SampleTableMissing
    p = problem()
    model = make(p, negative_sampling='popularity')
    model.random_ind = None
    with pytest.raises(SampleTableMissing):
        fit(model, p, 1)


def test_save_and_load_keep_both_attributes(no_gpu, tmp_path):
    from teamoflow_amd.mf import loss_graphs as L
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    p = problem()
    model = fit(make(p, negative_sampling='popularity', sampling_power=0.5, sample_seed=4), p, 2)
    history = list(model.loss_history_)
    model.loss_graph = L.BPRLoss()   # a file stores built-in plug-ins as plain data
    path = str(tmp_path / 'model.pt')
    model.save(path)
    blob = torch.load(path, weights_only=True)
    assert (blob['negative_sampling'], blob['sampling_power']) == ('popularity', 0.5)
    back = MatrixFactorization.load(path, device='cpu')
    assert (back.negative_sampling, back.sampling_power, back.sample_seed) == ('popularity', 0.5, 4)
    assert torch.equal(back.random_ind.cpu(), torch.as_tensor(p['R']))
    back.loss_graph = plugin_loss()
    assert fit(back, p, 2).loss_history_ == history
    del blob['negative_sampling'], blob['sampling_power']   # a file written before the attributes existed
    old = str(tmp_path / 'old.pt')
    torch.save(blob, old)
    older = MatrixFactorization.load(old, device='cpu')
    assert (older.negative_sampling, older.sampling_power) == ('uniform', 0.75)
    plain = fit(make(p), p, 1)
    plain.loss_graph = L.BPRLoss()
    plain.save(str(tmp_path / 'plain.pt'))                   # a model that never left the defaults writes the file it always wrote
    assert 'negative_sampling' not in torch.load(str(tmp_path / 'plain.pt'), weights_only=True)


# ------------------------------------------------------------------------------------------------------------------------
# the refusals
# ------------------------------------------------------------------------------------------------------------------------
class _Spy:
    def __init__(self):
        self.calls = 0

    def initialize_weights(self, n_features, n_components):
        self.calls += 1
        return torch.zeros(n_features, n_components)


def test_every_refusal_names_the_setting_before_a_weight_is_drawn(no_gpu, monkeypatch):
    from teamoflow_amd import _ops
    from teamoflow_amd.mf import loss_graphs as L
    monkeypatch.setattr(_ops, 'sample_negatives', lambda *a, **k: pytest.fail('nothing may be drawn'))
    p = problem()
    for named, loss, attrs in (('batch_users', L.BPRLoss(), dict(batch_users=8)), ('shard_items', L.WMRBLoss(), dict(shard_items=2)),
                               ('data_parallel', L.WARPLoss(), dict(data_parallel=True)),
                               ('data_parallel', L.SampledSoftmaxLoss(), dict(data_parallel='force')),
                               ('batch_users', plugin_loss(), dict(batch_users=8))):
        spy = _Spy()
        model = make(p, loss, init=spy, negative_sampling='popularity', **attrs)
        with pytest.raises(NotImplementedError, match=r"negative_sampling='popularity' with " + named) as e:
            fit(model, p, 1)
        assert 'back to its default' in str(e.value) and spy.calls == 0, (named, attrs)
    for attrs, match in ((dict(negative_sampling='zipf'), 'negative_sampling'), (dict(negative_sampling=None), 'negative_sampling'),
                         (dict(negative_sampling=True), 'negative_sampling'), (dict(negative_sampling='Popularity'), 'negative_sampling'),
                         (dict(negative_sampling='popularity', sampling_power=-0.1), 'sampling_power'),
                         (dict(negative_sampling='popularity', sampling_power=float('nan')), 'sampling_power'),
                         (dict(negative_sampling='popularity', sampling_power=float('inf')), 'sampling_power'),
                         (dict(negative_sampling='popularity', sampling_power='0.75'), 'sampling_power'),
                         (dict(negative_sampling='popularity', sampling_power=None), 'sampling_power')):
        spy = _Spy()
        with pytest.raises(ValueError, match=match):
            fit(make(p, init=spy, **attrs), p, 1)
        assert spy.calls == 0, attrs
    spy = _Spy()
    with pytest.raises(ValueError, match='negative_sampling'):   # the name is checked on every model, whatever its loss
        fit(make(p, L.MSELoss(), init=spy, negative_sampling='zipf'), p, 1)
    assert spy.calls == 0


def test_weights_the_rule_does_not_admit_end_the_fit_with_its_message(no_gpu):
    """Half the catalog per row and one item with most of the entries: power 4 puts more than 3/4 of the mass on 30 items."""
    p = problem()
    R = np.stack([np.random.default_rng(u).choice(N, N // 2, replace=False) for u in range(M)])
    with pytest.raises(ValueError, match='smaller power or fewer samples'):
        fit(make(p, R=R, negative_sampling='popularity', sampling_power=4.0), p, 1)


def test_the_table_of_the_refusals():
    from teamoflow_amd.mf import matrix_factorization as Mf
    row = Mf.SAMPLING_ROUTES['popularity']
    assert list(Mf.SAMPLING_ROUTES) == ['popularity'] and list(row) == list(Mf._SETTINGS)
    assert row == Mf.ROUTES['resample'] and row is not Mf.ROUTES['resample']                  # the cells of the resample row
    assert [s for s, a in row.items() if a == 'refuse'] == ['batch_users', 'shard_items', 'data_parallel set', 'data_parallel active']
    assert 'popularity' not in Mf.ROUTES
    with open(os.path.join(ROOT, 'DESIGN.md')) as f:
        design = f.read()
    head = ['feature \\ setting'] + list(Mf._SETTINGS)
    printed = '\n'.join('| ' + ' | '.join(cells) + ' |' for cells in (head, ['---'] * len(head), ['`popularity`'] + list(row.values())))
    assert '\n\n' + printed + '\n\n' in design, 'DESIGN.md, "What trains where", should print:\n' + printed


@pytest.mark.parametrize('state', ['uniform', 'absent'])
def test_every_recorded_route_is_unchanged_without_the_setting(state, monkeypatch):
    spec = importlib.util.spec_from_file_location('make_golden_pop', os.path.join(GOLDEN, 'make_golden.py'))
    make_golden = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make_golden)
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    if state == 'absent':
        init = MatrixFactorization.__init__

        def bare(self, *a, **k):
            init(self, *a, **k)
            del self.negative_sampling, self.sampling_power
        monkeypatch.setattr(MatrixFactorization, '__init__', bare)
    with open(os.path.join(GOLDEN, 'fit_routes.json')) as f:
        doc = json.load(f)
    texts = doc['outcomes']
    recorded = {kind: {key: [texts[string.ascii_letters.index(ch)] for ch in rows] for key, rows in doc[kind].items()}
                for kind in ('fit', 'als')}
    assert make_golden.fit_route_outcomes() == recorded
