"""resample_every / sample_seed without a GPU: the schedule of the generic loop (round j = epoch // k trains on the table of seed
sample_seed + j, round 0 on random_ind, which no fit changes), its refusals, save / load, the CPU route of
_ops.sample_negatives, and how many redraw rounds the sampler's definition (utils.random_sampler_device) needs where duplicates
are most likely - far below its cap of 64, which is why no test provokes the failure flag of tmf_sample_rows."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

M, N, S, R_COMP = 40, 60, 12, 4
LR = 0.05


@pytest.fixture
def no_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)


def problem(seed=5):
    rng = np.random.default_rng(seed)
    mask = rng.random((M, N)) < 0.2
    idx = np.argwhere(mask)
    val = rng.choice(np.array([-1, 0, 1, 2, 3, 4, 5], np.float32), idx.shape[0])
    return dict(idx=idx, val=val, U0=(rng.standard_normal((M, R_COMP)) * 0.7).astype(np.float32),
                V0=(rng.standard_normal((N, R_COMP)) * 0.7).astype(np.float32),
                R=np.stack([rng.choice(N, S, replace=False) for _ in range(M)]))


def make(p, loss, U0=None, V0=None, R=None, **attrs):
    from teamoflow_amd.mf import loss_graphs
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    model = MatrixFactorization(R_COMP, loss_graph=getattr(loss_graphs, loss)(),
                                user_weight_graph=FixedInitializer(p['U0'] if U0 is None else U0),
                                item_weight_graph=FixedInitializer(p['V0'] if V0 is None else V0), n_users=M, n_items=N, n_samples=S)
    model.verbose = False
    model.random_ind = torch.as_tensor(p['R'] if R is None else R)
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


def fit(model, p, epochs):
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    model.fit(epochs, eye(M), eye(N), SparseInteractions(p['idx'], p['val'], (M, N)), lr=LR)
    return model


def tables(model):
    return model.user_embedding.detach().clone(), model.item_embedding.detach().clone()


@pytest.mark.parametrize('loss', ['BPRLoss', 'WARPLoss'])
def test_two_rounds_are_two_chained_fits_on_the_generic_path(no_gpu, loss):
    """fit(4) with resample_every = 2 = fit(2) on random_ind, then fit(2) from those tables on the table of seed sample_seed + 1."""
    from teamoflow_amd.mf.utils import random_sampler_device
    p, seed = problem(), 11
    a = fit(make(p, loss, resample_every=2, sample_seed=seed), p, 4)
    b1 = fit(make(p, loss), p, 2)
    U1, V1 = tables(b1)
    T1 = random_sampler_device(N, M, S, seed=seed + 1, device='cpu')
    b2 = fit(make(p, loss, U0=U1.numpy(), V0=V1.numpy(), R=T1), p, 2)
    assert torch.equal(a.user_embedding, b2.user_embedding) and torch.equal(a.item_embedding, b2.item_embedding)
    assert a.loss_history_ == b1.loss_history_ + b2.loss_history_
    assert a.resample_rounds_ == 2 and a.resample_seconds_ >= 0.0 and a.fit_seconds_ >= a.resample_seconds_
    assert torch.equal(torch.as_tensor(a.random_ind), torch.as_tensor(p['R']))
    # the second round did train on another table: four epochs on random_ind alone end elsewhere
    static = fit(make(p, loss), p, 4)
    assert static.loss_history_[:2] == a.loss_history_[:2] and not torch.equal(static.user_embedding, a.user_embedding)


@pytest.mark.parametrize('loss', ['BPRLoss', 'WARPLoss'])   # WMRBLoss over plain tables has no form without a GPU
def test_a_single_round_is_the_default_fit(no_gpu, loss):
    p = problem()
    a, d = fit(make(p, loss, resample_every=4), p, 4), fit(make(p, loss), p, 4)
    assert torch.equal(a.user_embedding, d.user_embedding) and torch.equal(a.item_embedding, d.item_embedding)
    assert a.loss_history_ == d.loss_history_ and a.resample_rounds_ == d.resample_rounds_ == 1 and a.resample_seconds_ == 0.0
    assert torch.equal(torch.as_tensor(a.random_ind), torch.as_tensor(p['R']))
    again = fit(a, p, 4)   # and a second fit of the same model starts again from round 0
    assert again.loss_history_ == d.loss_history_


def test_sample_seed_changes_the_later_rounds_only(no_gpu):
    p = problem()
    a, b = (fit(make(p, 'WARPLoss', resample_every=1, sample_seed=s), p, 3) for s in (0, 1))
    assert a.loss_history_[0] == b.loss_history_[0] and a.loss_history_[1:] != b.loss_history_[1:]
    assert not torch.equal(a.user_embedding, b.user_embedding) and a.resample_rounds_ == 3
    assert fit(make(p, 'WARPLoss', resample_every=1), p, 3).loss_history_ == a.loss_history_   # deterministic


@pytest.mark.parametrize('bad', [-1, 2.0, 1.5, '2', None, True])
def test_a_negative_or_non_integer_setting_is_refused(no_gpu, bad):
    p = problem()
    with pytest.raises(ValueError, match='resample_every'):
        fit(make(p, 'BPRLoss', resample_every=bad), p, 1)
    with pytest.raises(ValueError, match='resample_every'):
        fit(make(p, 'LogisticLoss', resample_every=bad), p, 1)
    if bad != -1:
        with pytest.raises(ValueError, match='sample_seed'):
            fit(make(p, 'BPRLoss', resample_every=1, sample_seed=bad), p, 1)


@pytest.mark.parametrize('name, value', [('batch_users', 16), ('shard_items', 2), ('data_parallel', 'force')])
def test_the_forms_that_own_their_plans_are_refused(no_gpu, name, value):
    p = problem()
    with pytest.raises(NotImplementedError, match=f'resample_every=3 with {name}'):
        fit(make(p, 'WMRBLoss', resample_every=3, **{name: value}), p, 1)
    model = make(p, 'WMRBLoss', **{name: value})   # without the setting nothing is refused here: the refusal names its cause
    model._resample_setting()


def test_no_effect_on_a_loss_that_reads_no_table(no_gpu):
    p = problem()
    a, d = fit(make(p, 'LogisticLoss', resample_every=1, sample_seed=9), p, 3), fit(make(p, 'LogisticLoss'), p, 3)
    assert torch.equal(a.user_embedding, d.user_embedding) and a.loss_history_ == d.loss_history_
    assert a.resample_rounds_ == 0 and a.resample_seconds_ == 0.0


def test_save_and_load_carry_the_settings(no_gpu, tmp_path):
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    p = problem()
    model = fit(make(p, 'BPRLoss', resample_every=2, sample_seed=7), p, 4)
    path = str(tmp_path / 'model.pt')
    model.save(path)
    blob = torch.load(path, weights_only=True)
    assert (blob['resample_every'], blob['sample_seed']) == (2, 7)
    back = MatrixFactorization.load(path, device='cpu')
    assert (back.resample_every, back.sample_seed) == (2, 7) and torch.equal(back.random_ind.cpu(), torch.as_tensor(p['R']))
    assert fit(back, p, 4).loss_history_ == model.loss_history_
    del blob['resample_every'], blob['sample_seed']   # a file written before the attributes existed
    old = str(tmp_path / 'old.pt')
    torch.save(blob, old)
    older = MatrixFactorization.load(old, device='cpu')
    assert (older.resample_every, older.sample_seed) == (0, 0)
    fresh = MatrixFactorization(3)
    assert (fresh.resample_every, fresh.sample_seed, fresh.resample_rounds_, fresh.resample_seconds_) == (0, 0, 0, 0.0)


@pytest.mark.parametrize('n, m, s, seed, offset', [(60, 40, 12, 3, 0), (24, 7, 12, 0, 5), (10, 9, 8, 1, 2), (5000, 3, 1000, 2 ** 40 + 1, 2 ** 33)])
def test_sample_negatives_on_the_cpu_is_the_torch_function(no_gpu, n, m, s, seed, offset):
    from teamoflow_amd import _ops
    from teamoflow_amd.mf.utils import random_sampler_device
    want = random_sampler_device(n, m, s, seed=seed, device='cpu', user_offset=offset)
    got = _ops.sample_negatives(n, m, s, seed=seed, device='cpu', user_offset=offset)
    assert got.dtype == torch.int32 and got.device.type == 'cpu' and torch.equal(got, want)
    out = torch.full((m, s), -7, dtype=torch.int32)
    assert _ops.sample_negatives(n, m, s, seed=seed, device='cpu', user_offset=offset, out=out) is out and torch.equal(out, want)
    with pytest.raises(ValueError):
        _ops.sample_negatives(n, m, n + 1, device='cpu')


def redraw_rounds(n_items, n_users, n_samples, seed):
    """Rounds of random_sampler_device's rejection loop that redraw something: the definition, restated with a counter."""
    from teamoflow_amd.mf.utils import counter_hash, hash_below
    pos = torch.arange(n_samples, dtype=torch.int64)[None, :]
    u = torch.arange(n_users, dtype=torch.int64)[:, None]
    blk = torch.sort(hash_below(counter_hash(seed, u, pos, 2), n_items), dim=1)[0]
    for rnd in range(3, 67):
        dup = torch.zeros_like(blk, dtype=torch.bool)
        dup[:, 1:] = blk[:, 1:] == blk[:, :-1]
        if not bool(dup.any()):
            return rnd - 3, blk
        blk = torch.sort(torch.where(dup, hash_below(counter_hash(seed, u, pos, rnd), n_items), blk), dim=1)[0]
    raise AssertionError('ran out of rounds')


@pytest.mark.parametrize('s, users, limit', [(1024, 256, 21), (33, 2000, 19), (200, 1000, 19), (4096, 64, 19)])
def test_redraw_rounds_at_the_highest_duplicate_pressure(s, users, limit):
    """n_items = 2 S, the smallest catalog of the rejection branch: the rows settle within ``limit`` redraw rounds of the 64 allowed
    (a redraw collides with probability below 1 / 2, so the repeats of a row at least halve per round in expectation)."""
    from teamoflow_amd.mf.utils import random_sampler_device
    rounds, blk = redraw_rounds(2 * s, users, s, seed=0)
    assert 1 <= rounds <= limit, rounds
    table = random_sampler_device(2 * s, users, s, seed=0, device='cpu')
    assert torch.equal(torch.sort(table, dim=1)[0].to(torch.int64), blk)   # the restatement counts the rounds of the real thing


def test_c_abi_of_the_sampler_is_declared_bound_and_built():
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load_library()
    for name in ('tmf_sample_rows_supported', 'tmf_sample_rows'):
        assert re.search(r'\bint %s\(' % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.tmf_version() == 203
    # the supported shapes (host-side: no launch)
    assert lib.tmf_sample_rows_supported(2048, 1024) == 1 and lib.tmf_sample_rows_supported(2047, 1024) == 0
    assert lib.tmf_sample_rows_supported(100, 0) == 0 and lib.tmf_sample_rows_supported(2, 1) == 1
    assert lib.tmf_sample_rows_supported(8192, 4096) == 1 and lib.tmf_sample_rows_supported(2 ** 31 - 1, 4097) == 0
    # bad arguments return before any launch
    assert lib.tmf_sample_rows(100, 5, 51, 0, 0, None, None, None) != 0 and b'n_samples' in lib.tmf_last_error()
    assert lib.tmf_sample_rows(100, -1, 10, 0, 0, None, None, None) != 0
