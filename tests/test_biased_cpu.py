"""CPU side of BiasedLinearEmbedding on the sparse HIP engine (no GPU): the problem generator of tests/test_gpu_biased.py, the
C ABI of the four tmf_bias entry points (declared, bound, built, argument checks that fail before anything is launched), the
dispatch without a GPU, and the statements the GPU tolerances rest on, checked on the reference alone
(oracle.dense_ref.fit_dense_plugins, fp32 against fp64, one step):

  * every weight table of the fp32 oracle lies inside conftest.assert_step's interval at rtol = 1e-5;
  * every bias does with slack_c = 1e-5 sum_i |G_ref[i, c]| - the error a column sum inherits when each summand agrees to 1e-5;
  * with WMRB the item bias cancels analytically (every hinge argument is 1 - e_u . (e_pos - e_neg)): its fp64 gradient is
    rounding noise, so no test compares the WMRB item bias or the item embedding that carries it.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_step, report_slack, step_bounds

BIAS_NAMES = ('tmf_bias_colsum_part_rows', 'tmf_bias_colsum_f32', 'tmf_bias_adam_f32', 'tmf_adam_bias_rows_f32')
LR = 0.05
SIDES = (('biased', 'biased'), ('biased', 'linear'), ('linear', 'biased'))


def biased_problem(seed, m, n, r, loss, density=0.3):
    """COO pairs without duplicates (row-major), user ``empty_user`` and item ``empty_item`` without any interaction, values 1..5
    (a random sign for KL: both classes populated), tables ~ N(0, 0.3^2) and, for WMRB, an [m, S] negative table, S = n // 2."""
    rng = np.random.default_rng(seed)
    mask = rng.random((m, n)) < density
    empty_user, empty_item = m // 3, n // 2
    mask[empty_user, :] = False
    mask[:, empty_item] = False
    idx = np.argwhere(mask)
    val = rng.integers(1, 6, idx.shape[0]).astype(np.float32)
    if loss == 'kl':
        val *= rng.choice(np.array([-1.0, 1.0], np.float32), idx.shape[0])
    S = max(n // 2, 1)
    R = np.stack([rng.choice(n, S, replace=False) for _ in range(m)]) if loss == 'wmrb' else None
    U0 = (rng.standard_normal((m, r)) * 0.3).astype(np.float32)
    V0 = (rng.standard_normal((n, r)) * 0.3).astype(np.float32)
    return dict(idx=idx, val=val, U0=U0, V0=V0, R=R, S=S, m=m, n=n, r=r, loss=loss, empty_user=empty_user, empty_item=empty_item)


def biased_oracle(p, sides, epochs, lr=LR, dtype=torch.float64, U0=None, V0=None):
    """fit_dense_plugins on the problem over identity features; sides = (user, item) kinds, 'biased' | 'linear'."""
    from oracle import dense_ref as D
    return D.fit_dense_plugins(p['U0'] if U0 is None else U0, p['V0'] if V0 is None else V0, p['idx'], p['val'], p['loss'], epochs, lr,
                               np.eye(p['m']), np.eye(p['n']), user_embedding=sides[0], item_embedding=sides[1], random_ind=p['R'],
                               n_items=p['n'], n_samples=p['S'], dtype=dtype)


def bias_slack(G_ref):
    """[1, r]: 1e-5 sum_i |G_ref[i, c]| - what the column sum may be off by when every row's gradient agrees to 1e-5."""
    return 1e-5 * np.abs(np.asarray(G_ref, np.float64)).sum(0, keepdims=True)


def assert_bias_step(b_new, b0, g_ref, G_ref, lr, what):
    """assert_step with the column-sum slack; logs how many elements needed the slack and the largest share of it they used
    (the smallest t for which the element lies in the interval widened by t * slack, by bisection)."""
    b_new, b0 = np.asarray(b_new, np.float64).reshape(1, -1), np.asarray(b0, np.float64).reshape(1, -1)
    g_ref, slack = np.asarray(g_ref, np.float64).reshape(1, -1), bias_slack(G_ref)
    assert_step(b_new, b0, g_ref, lr, rtol=1e-5, what=what, slack=slack)

    def outside(t):
        lo, hi = step_bounds(b0, g_ref, lr, 1e-5, t * slack)
        return (b_new < lo) | (b_new > hi)
    need = outside(0.0)
    lo_t, hi_t = np.zeros_like(b_new), np.ones_like(b_new)
    for _ in range(30):
        mid = 0.5 * (lo_t + hi_t)
        out = outside(mid)
        lo_t, hi_t = np.where(out, mid, lo_t), np.where(out, hi_t, mid)
    report_slack(check=what, n_elements=int(b_new.size), n_needed_slack=int(need.sum()),
                 max_consumed=float(hi_t[need].max()) if need.any() else 0.0)


SHAPES = ((60, 40, 7), (300, 90, 33), (2000, 50, 3))


@pytest.fixture(scope='module')
def oracles():
    """(fp64, fp32) one-step oracle runs with both sides biased, computed once per (loss, shape)."""
    cache = {}

    def get(loss, shape):
        if (loss, shape) not in cache:
            p = biased_problem(sum(shape), *shape, loss)
            cache[loss, shape] = (p, biased_oracle(p, SIDES[0], 1), biased_oracle(p, SIDES[0], 1, dtype=torch.float32))
        return cache[loss, shape]
    return get


def test_problem_generator():
    for loss in ('mse', 'wmrb', 'kl'):
        p = biased_problem(3, 60, 40, 7, loss)
        idx, val = p['idx'], p['val']
        assert len({(int(u), int(i)) for u, i in idx}) == idx.shape[0] > 400
        assert p['empty_user'] not in idx[:, 0] and p['empty_item'] not in idx[:, 1]
        assert set(np.abs(val).astype(int)) == {1, 2, 3, 4, 5}
        assert ((val < 0).any() and (val > 0).any()) if loss == 'kl' else (val > 0).all()
        assert (p['R'].shape == (60, 20) and p['R'].min() >= 0 and p['R'].max() < 40) if loss == 'wmrb' else p['R'] is None


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('loss', ['mse', 'wmrb', 'kl'])
def test_fp32_oracle_lies_inside_the_intervals(oracles, loss, shape):
    p, ref64, ref32 = oracles(loss, shape)
    r = shape[2]
    (gU, gbu), (gV, gbv) = ref64['first_grads']
    assert_step(ref32['user_vars'][0], p['U0'], gU, LR, what=f'{loss} {shape} fp32 oracle U')
    assert_step(ref32['item_vars'][0], p['V0'], gV, LR, what=f'{loss} {shape} fp32 oracle V')
    zero = np.zeros((1, r))
    assert_bias_step(ref32['user_vars'][1], zero, gbu, gU, LR, f'{loss} {shape} fp32 oracle user bias')
    assert_bias_step(ref32['item_vars'][1], zero, gbv, gV, LR, f'{loss} {shape} fp32 oracle item bias')
    # the bias gradient is the column sum of the weight gradient, and untouched rows have none (WMRB samples the item without
    # interactions as a negative: only its user is untouched)
    assert np.abs(gbu - gU.sum(0, keepdims=True)).max() <= 1e-12 * np.abs(gU).sum(0).max()
    assert not gU[p['empty_user']].any() and (loss == 'wmrb' or not gV[p['empty_item']].any())


@pytest.mark.parametrize('shape', SHAPES)
def test_wmrb_item_bias_gradient_is_rounding_noise(oracles, shape):
    p, ref64, _ = oracles('wmrb', shape)
    gV, gbv = ref64['first_grads'][1]
    assert np.abs(gbv).max() < 1e-12 * np.abs(gV).sum(0).max()
    gU, gbu = ref64['first_grads'][0]
    assert np.abs(gbu).max() > 1e-3 * np.abs(gU).sum(0).max()      # the user bias is a real variable


def test_loss_of_a_biased_model_is_the_unbiased_loss_on_the_effective_tables():
    """E = W + 1 b^T: the closed form the engine path rests on, and the way the GPU tests start the oracle from a carried bias."""
    for loss in ('mse', 'wmrb', 'kl'):
        p = biased_problem(11, 30, 20, 4, loss)
        two = biased_oracle(p, SIDES[0], 2)
        snap = biased_oracle(p, SIDES[0], 1)
        EU, EV = snap['user_vars'][0] + snap['user_vars'][1], snap['item_vars'][0] + snap['item_vars'][1]
        lin = biased_oracle(p, ('linear', 'linear'), 1, U0=EU, V0=EV)
        assert abs(lin['loss'][0] - two['loss'][1]) <= 1e-12 * abs(two['loss'][1]), loss


def test_entry_points_are_declared_bound_and_built():
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    declared = set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    lib = _lib.load_library()
    for name in BIAS_NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name


def test_partition_of_the_column_sum_is_a_function_of_the_row_count():
    from teamoflow_amd import _lib
    rows = _lib.load_library().tmf_bias_colsum_part_rows
    assert [rows(x) for x in (-1, 0, 1, 63, 64, 65, 128, 129)] == [0, 1, 1, 1, 1, 2, 2, 3]
    assert rows(65536) == 1024 and rows(65537) == 1009 and rows(70001) == 1015 and rows(10 ** 9) == 1024
    assert all(1 <= rows(x) <= 1024 for x in range(0, 200000, 997))


def test_argument_checks_fail_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail differently (or crash); these return first."""
    from teamoflow_amd import _lib
    lib = _lib.load_library()
    adam = lib.tmf_adam_fresh(0.05)
    host = (ctypes.c_double * 8)()              # stands for any non-null, 16-byte aligned buffer: never dereferenced
    H = ctypes.c_void_p((ctypes.addressof(host) + 15) // 16 * 16)
    odd = ctypes.c_void_p(H.value + 4)

    def failed(rc, word):
        return rc != 0 and word in lib.tmf_last_error().decode()
    assert failed(lib.tmf_bias_colsum_f32(H, 10, 5000, H, 1, H, None), 'n_components')
    assert failed(lib.tmf_bias_colsum_f32(None, 10, 8, H, 1, H, None), 'bad arguments')
    assert failed(lib.tmf_bias_colsum_f32(H, 10, 8, None, 1, H, None), 'bad arguments')
    assert failed(lib.tmf_bias_colsum_f32(H, -1, 8, H, 1, H, None), 'bad arguments')
    assert failed(lib.tmf_bias_colsum_f32(H, 65, 8, H, 1, H, None), 'part_rows')
    assert failed(lib.tmf_bias_colsum_f32(odd, 10, 8, H, 1, H, None), 'aligned')
    assert failed(lib.tmf_bias_adam_f32(None, 1, H, H, 8, adam, None), 'bad arguments')
    assert failed(lib.tmf_bias_adam_f32(H, 1, None, H, 8, adam, None), 'bad arguments')
    assert failed(lib.tmf_bias_adam_f32(H, 0, H, H, 8, adam, None), 'bad arguments')
    assert failed(lib.tmf_bias_adam_f32(H, 1, H, H, 0, adam, None), 'n_components')
    assert lib.tmf_adam_bias_rows_f32(None, None, None, None, 0, 8, adam, None) == 0            # nothing to do
    for args in ((None, H, H, H), (H, None, H, H), (H, H, None, H), (H, H, H, None)):
        assert failed(lib.tmf_adam_bias_rows_f32(*args, 4, 8, adam, None), 'bad arguments')
    other = ctypes.c_void_p(H.value + 16)
    assert failed(lib.tmf_adam_bias_rows_f32(H, H, H, H, 4, 8, adam, None), 'same table')
    assert failed(lib.tmf_adam_bias_rows_f32(H, odd, H, other, 4, 8, adam, None), 'aligned')
    assert failed(lib.tmf_adam_bias_rows_f32(H, H, H, other, 4, 2000, adam, None), 'n_components')


def test_dispatch_without_a_gpu_stays_generic(monkeypatch):
    """A biased side over indicator features is an engine model only where the engine has a form for it: a GPU, float32 tables,
    the reference's optimizer, full-batch on one device.  Unbiased dispatch does not look at any of that."""
    from teamoflow_amd.mf.embedding_graphs import BiasedLinearEmbedding, LinearEmbedding, ReLUEmbedding
    from teamoflow_amd.mf.loss_graphs import KLDivergenceLoss, WMRBLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import eye

    class Mine(BiasedLinearEmbedding):
        pass

    def model(u=BiasedLinearEmbedding, i=BiasedLinearEmbedding, loss=None, **attrs):
        mf = MatrixFactorization(4, user_repr_graph=u(), item_repr_graph=i(), **({'loss_graph': loss} if loss else {}))
        for k, v in attrs.items():
            setattr(mf, k, v)
        return mf
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    assert model()._route(eye(6), eye(7)) == 'generic'
    assert model(i=LinearEmbedding)._route(eye(6), eye(7)) == 'generic' and model(u=LinearEmbedding)._route(eye(6), eye(7)) == 'generic'
    assert model(LinearEmbedding, LinearEmbedding)._route(eye(6), eye(7)) == 'engine'
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    for loss in (None, WMRBLoss(), KLDivergenceLoss()):
        assert model(loss=loss)._route(eye(6), eye(7)) == 'engine'
        assert model(i=LinearEmbedding, loss=loss)._route(eye(6), eye(7)) == 'engine'
        assert model(u=LinearEmbedding, loss=loss)._route(eye(6), eye(7)) == 'engine'
    dense = lambda k: torch.eye(k) + 0.05   # noqa: E731  (a dense identity matrix would count as an indicator)
    assert model()._route(dense(6), eye(7)) == 'generic' and model()._route(eye(6), dense(7)) == 'generic'
    assert model(u=Mine)._route(eye(6), eye(7)) == 'generic' and model(i=ReLUEmbedding)._route(eye(6), eye(7)) == 'generic'
    for name, value in (('batch_users', 8), ('shard_items', 2), ('data_parallel', 'force'), ('factor_dtype', torch.bfloat16),
                        ('optimizer', 'adam')):
        assert model(**{name: value})._route(eye(6), eye(7)) == 'generic', name
        assert model(LinearEmbedding, LinearEmbedding, **{name: value})._route(eye(6), eye(7)) == 'engine', name
