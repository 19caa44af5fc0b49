"""CPU side of ReLUEmbedding on the sparse HIP engine (no GPU): the problem generator and the oracle call of tests/test_gpu_relu.py,
the dispatch (``relu_engine`` is off by default; on, a ReLU side is an engine side under the conditions a biased side is), the C ABI
of the five tmf_relu entry points (declared, bound, built, argument checks that fail before anything is launched), and the
statements the GPU tolerances rest on, checked on the reference alone (oracle.dense_ref.fit_dense_plugins with 'relu' sides, fp32
against fp64):

  * one step: all six variables of the fp32 oracle lie inside conftest.step_bounds at rtol = 1e-5 without any slack and the loss
    agrees to 1e-5 (measured: 1.2e-7 or better);
  * the kink: the smallest non-zero |F relu_w0| of these problems is some 1e-5 .. 1e-4 against fp32 summation bounds of order 1e-7,
    so the fp32 and the fp64 forward agree on which hidden units are on;
  * trajectories on problem 77 (both sides hybrid ReLU): the loss agrees to 1e-5 over 3 epochs and to 1e-4 over 10 for MSE, WMRB and
    KL (START_SEED), and to 1e-3 over 40 epochs for MSE only - the reference itself drifts apart by 2 - 3e-2 at 40 epochs for WMRB and KL (a unit
    that switches in one precision and not in the other), so no test asks for that.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_step, rel_err
from test_biased_cpu import LR
from test_features_cpu import _model, featured_problem

RELU_NAMES = ('tmf_relu_embed_f32', 'tmf_relu_dhidden_f32', 'tmf_relu_part_rows', 'tmf_relu_dweights_f32', 'tmf_relu_adam_weights_f32')
LOSSES = ('mse', 'wmrb', 'kl')
LAYOUTS = ('eye', 'hybrid', 'pure')      # the features of a ReLU side: eye(), [I | tags] or the tags alone as SparseFeatures
BOTH = ('user', 'item')
SIDES = (('user',), ('item',), BOTH)
SIDE_IDS = ['user', 'item', 'both']
# The start values of the ReLU sides are drawn from default_rng(seed + START_SEED).  How long the reference's own fp32 and fp64 runs
# stay together depends on the draw - a hidden unit that switches in one precision and not in the other separates them: on problem 77
# the 10-epoch KL losses of draws 0, 1, 2, 3 agree to 9e-3, 2.7e-3, 4.7e-5, 1.9e-5 (WMRB: 2.9e-7 .. 2.4e-6).  The trajectory tests
# need a problem the reference itself follows to well below their 1e-3, so the draw is one of those that do (test_fp32_oracle_trajectory
# holds it to 1e-4 over 10 epochs); the choice looks at the reference alone.
START_SEED = 3


def relu_problem(seed, m, n, r, loss, layout, item_everywhere=True):
    """test_features_cpu.featured_problem plus, per side, the start of a ReLU side over ``layout``: output weights
    W0 [5 r, r] ~ 0.3 N(0, 1) (p['relu_Wu'], p['relu_Wv']), hidden weights relu_w0 [n_features, 5 r] ~ 0.2 N(0, 1) (p['relu_Wru'], ..)
    and the dense fp64 features (p['relu_Fu_dense'], ..; the identity for 'eye').  p['U0'] / p['V0'] stay the tables of a plain side."""
    p = featured_problem(seed, m, n, r, loss, 'pure' if layout == 'pure' else 'hybrid', item_everywhere)
    rng = np.random.default_rng(seed + START_SEED)
    for s, rows in (('u', m), ('v', n)):
        F = np.eye(rows) if layout == 'eye' else p['F' + s + '_dense']
        p['relu_F' + s + '_dense'] = F
        p['relu_W' + s] = (rng.standard_normal((5 * r, r)) * 0.3).astype(np.float32)
        p['relu_Wr' + s] = (rng.standard_normal((F.shape[1], 5 * r)) * 0.2).astype(np.float32)
    p['relu_layout'] = layout
    return p


def relu_oracle(p, relu, epochs, lr=LR, dtype=torch.float64):
    """fit_dense_plugins with a ReLU side (relu_bias zeros) on the sides named in ``relu`` and a plain side over the identity on
    the others."""
    from oracle import dense_ref as D
    ru, ri = 'user' in relu, 'item' in relu
    return D.fit_dense_plugins(p['relu_Wu'] if ru else p['U0'], p['relu_Wv'] if ri else p['V0'], p['idx'], p['val'], p['loss'], epochs, lr,
                               p['relu_Fu_dense'] if ru else np.eye(p['m']), p['relu_Fv_dense'] if ri else np.eye(p['n']),
                               user_embedding='relu' if ru else 'linear', item_embedding='relu' if ri else 'linear',
                               user_relu_weight0=p['relu_Wru'] if ru else None, item_relu_weight0=p['relu_Wrv'] if ri else None,
                               random_ind=p['R'], n_items=p['n'], n_samples=p['S'], dtype=dtype)


def relu_model(p, relu, relu_engine=True, **graphs):
    """A model with ReLUEmbedding on the sides named in ``relu``, started where relu_oracle starts: the output weights through
    FixedInitializer, relu_weight kept on the model (fit() continues from it), relu_bias left to its zeros."""
    from teamoflow_amd.mf.embedding_graphs import ReLUEmbedding
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.sparse import default_device
    kw = {}
    for s, name in (('u', 'user'), ('v', 'item')):
        if name in relu:
            kw[name + '_repr_graph'] = ReLUEmbedding()
            kw[name + '_weight_graph'] = FixedInitializer(p['relu_W' + s])
    kw.update(graphs)
    model = _model(p, (), **kw)
    for s, name in (('u', 'user'), ('v', 'item')):
        if name in relu:
            setattr(model, name + '_relu_weight', torch.tensor(p['relu_Wr' + s], device=default_device()).requires_grad_(True))
    model.relu_engine = relu_engine
    return model


def relu_features(p, relu):
    """(user_features, item_features) of a fit: eye() or SparseFeatures on the ReLU sides by the problem's layout, eye() elsewhere."""
    from teamoflow_amd.mf.sparse import SparseFeatures, eye
    sparse = p['relu_layout'] != 'eye'
    return tuple(SparseFeatures(*p['F' + s]) if sparse and name in relu else eye(rows)
                 for s, name, rows in (('u', 'user', p['m']), ('v', 'item', p['n'])))


def kink_margin(F_dense, Wr0):
    """(smallest non-zero |F relu_w0| in fp64, the largest fp32 summation bound (n_i + 2) 2^-24 sum |x w| of any pre-activation,
    the smallest ratio of a non-zero |z| to its own bound)."""
    F, W = np.asarray(F_dense, np.float64), np.asarray(Wr0, np.float64)
    z = F @ W
    bound = ((F != 0).sum(1, keepdims=True) + 2) * 2.0 ** -24 * (np.abs(F) @ np.abs(W))
    nz = z != 0
    return float(np.abs(z[nz]).min()), float(bound.max()), float((np.abs(z[nz]) / bound[nz]).min())


# ------------------------------------------------------------------------------------------------------------------------
# dispatch
# ------------------------------------------------------------------------------------------------------------------------
def test_dispatch_predicate(monkeypatch):
    from teamoflow_amd.mf.embedding_graphs import BiasedLinearEmbedding, LinearEmbedding, ReLUEmbedding
    from teamoflow_amd.mf.loss_graphs import KLDivergenceLoss, LogisticLoss, MSELoss, WMRBLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseFeatures, eye

    class Mine(ReLUEmbedding):
        pass

    class MyLoss(MSELoss):
        pass
    F6, F7 = SparseFeatures([[0, 1], [5, 2]], [1.0, 2.0], (6, 3), device='cpu'), SparseFeatures([[6, 0]], [1.0], (7, 9), device='cpu')
    none = SparseFeatures(np.zeros((0, 2)), np.zeros(0), (6, 3), device='cpu')

    def model(u=ReLUEmbedding, i=LinearEmbedding, loss=None, r=4, **attrs):
        mf = MatrixFactorization(r, user_repr_graph=u(), item_repr_graph=i(), **({'loss_graph': loss} if loss else {}))
        for k, v in attrs.items():
            setattr(mf, k, v)
        return mf
    assert MatrixFactorization(4).relu_engine is False                                  # off unless asked for
    feats = ((eye(6), eye(7)), (F6, eye(7)), (F6, F7))
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    for uf, vf in feats:
        assert model()._route(uf, vf) == 'generic'                                        # the default: generic, as before
        assert model(relu_engine=False)._route(uf, vf) == 'generic'
    for loss in (None, WMRBLoss(), KLDivergenceLoss(), LogisticLoss()):
        for uf, vf in feats:
            assert model(loss=loss, relu_engine=True)._route(uf, vf) == 'engine'
            assert model(u=LinearEmbedding, i=ReLUEmbedding, loss=loss, relu_engine=True)._route(uf, vf) == 'engine'
            assert model(i=ReLUEmbedding, loss=loss, relu_engine=True)._route(uf, vf) == 'engine'
        assert model(i=BiasedLinearEmbedding, loss=loss, relu_engine=True)._route(F6, eye(7)) == 'engine'   # beside a biased side
    assert model(u=Mine, relu_engine=True)._route(eye(6), eye(7)) == 'generic'            # exactly ReLUEmbedding
    assert model(u=LinearEmbedding, i=Mine, relu_engine=True)._route(eye(6), eye(7)) == 'generic'
    assert model(loss=MyLoss(), relu_engine=True)._route(eye(6), eye(7)) == 'generic'     # one of the four built-in losses
    assert model(relu_engine=True)._route(none, eye(7)) == 'generic'                      # SparseFeatures with entries
    dense = torch.eye(6)[:, :3].contiguous()
    assert model(relu_engine=True)._route(dense, eye(7)) == 'generic' and model(relu_engine=True)._route(dense.to_sparse(), eye(7)) == 'generic'
    assert model(r=204, relu_engine=True)._route(eye(6), eye(7)) == 'engine'                 # 5 r <= 1024
    assert model(r=205, relu_engine=True)._route(eye(6), eye(7)) == 'generic'
    assert model(u=LinearEmbedding, r=205, relu_engine=True)._route(eye(6), eye(7)) == 'engine'
    for name, value in (('batch_users', 8), ('shard_items', 2), ('data_parallel', 'force'), ('factor_dtype', torch.bfloat16),
                        ('optimizer', 'adam')):                                         # the 'side' row of ROUTES
        for uf, vf in feats:
            assert model(relu_engine=True, **{name: value})._route(uf, vf) == 'generic', name
        assert model(u=LinearEmbedding, relu_engine=True, **{name: value})._route(eye(6), eye(7)) == 'engine', name
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for uf, vf in feats:
        assert model(relu_engine=True)._route(uf, vf) == 'generic'


@pytest.mark.parametrize('relu_engine', [False, True])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_fit_without_a_gpu_is_generic(monkeypatch, layout, relu_engine):
    """No GPU: a ReLU fit is the generic fit whatever relu_engine says - and it starts from the relu_weight kept on the model, so it
    is the oracle's fit."""
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    calls, generic = [], MatrixFactorization._fit_generic

    def counted(self, *a, **k):
        calls.append(1)
        return generic(self, *a, **k)
    monkeypatch.setattr(MatrixFactorization, '_fit_generic', counted)
    p = relu_problem(13, 30, 20, 3, 'mse', layout)
    model = relu_model(p, BOTH, relu_engine=relu_engine)
    model.fit(2, *relu_features(p, BOTH), SparseInteractions(p['idx'], p['val'], (30, 20)), lr=LR)
    assert len(calls) == 1 and not hasattr(model, '_state')
    ref = relu_oracle(p, BOTH, 2, dtype=torch.float32)
    assert rel_err(model.loss_history_, ref['loss']) < 1e-5
    assert [tuple(t.shape) for t in model.user_trainable] == [(15, 3), (p['relu_Fu_dense'].shape[1], 15), (1, 15)]
    assert model.user_relu_weight is model.user_trainable[1] and model.user_relu_bias.requires_grad


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_built_and_listed():
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    declared = set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    lib = _lib.load_library()
    for name in RELU_NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    make = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS :=.*\btmf_relu\.hip\b', make, re.M)
    notes = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(name in notes for name in RELU_NAMES)


def test_part_rows_depend_on_the_row_count_alone():
    from teamoflow_amd import _lib
    lib = _lib.load_library()
    P = lib.tmf_relu_part_rows
    assert P(-5) == 0 and P(0) == 0 and P(1) == 1
    edge = next(n for n in range(1, 100000) if P(n) == 2) - 1
    assert edge >= 128 and P(edge) == 1 and P(2 * edge) == 2 and P(2 * edge + 1) == 3
    counts = [P(n) for n in (1, 1000, 10 ** 5, 10 ** 6, 10 ** 7, 10 ** 9)]
    assert counts == sorted(counts) and counts[-1] <= 256 and counts[3] > 64             # enough parts to fill the card at 1M rows


def test_argument_checks_fail_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail differently (or crash); these return first."""
    from teamoflow_amd import _lib
    lib = _lib.load_library()
    adam = lib.tmf_adam_fresh(0.05)
    host = (ctypes.c_double * 16)()             # stands for any non-null, aligned table: never dereferenced
    base = (ctypes.addressof(host) + 15) & ~15
    H, H2, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 16), ctypes.c_void_p(base + 4)

    def failed(rc, word):
        return rc == -1 and word in lib.tmf_last_error().decode()
    embed, dhid, dw, step = lib.tmf_relu_embed_f32, lib.tmf_relu_dhidden_f32, lib.tmf_relu_dweights_f32, lib.tmf_relu_adam_weights_f32
    P3 = lib.tmf_relu_part_rows(3)
    # nothing to do
    assert embed(None, None, None, None, 0, 15, 3, None) == 0 and dhid(None, None, None, None, None, 0, 15, 3, None) == 0
    assert dw(None, None, None, None, 0, 0, 15, 3, None) == 0
    # null tables
    for k in range(4):
        assert failed(embed(*[None if j == k else H for j in range(4)], 3, 15, 3, None), 'null table'), k
    for k in range(5):
        args = [H, H, H, H, H2]
        args[k] = None
        assert failed(dhid(*args, 3, 15, 3, None), 'null table'), k
    for k in range(4):
        assert failed(dw(*[None if j == k else H for j in range(4)], P3, 3, 15, 3, None), 'null table'), k
    assert failed(step(None, 1, H, H, None, 15, 3, adam, None), 'null table')
    assert failed(step(H, 1, None, H, None, 15, 3, adam, None), 'null table')
    assert failed(step(H, 1, H, None, None, 15, 3, adam, None), 'null table')
    # widths outside the row geometry
    for aux, r, word in ((0, 3, 'aux'), (1025, 3, 'aux'), (15, 0, 'n_components'), (15, 1025, 'n_components')):
        assert failed(embed(H, H, H, H, 3, aux, r, None), word)
        assert failed(dhid(H, H, H, H, H2, 3, aux, r, None), word)
        assert failed(dw(H, H, H, H, P3, 3, aux, r, None), word)
        assert failed(step(H, 1, H, H, None, aux, r, adam, None), word)
    # alignment, aliasing, row counts, part_rows
    assert failed(embed(odd, H, H, H, 3, 15, 3, None), 'aligned') and failed(embed(H, H, H, odd, 3, 15, 3, None), 'aligned')
    assert failed(dhid(H, odd, H, H, H2, 3, 15, 3, None), 'aligned') and failed(dw(H, H, odd, H, P3, 3, 15, 3, None), 'aligned')
    assert failed(step(H, 1, H, odd, None, 15, 3, adam, None), 'aligned') and failed(step(H, 1, H, H, odd, 15, 3, adam, None), 'aligned')
    assert failed(dhid(H, H, H, H, H, 3, 15, 3, None), 'same table')
    assert failed(embed(H, H, H, H, -1, 15, 3, None), 'n_rows') and failed(dhid(H, H, H, H, H2, -1, 15, 3, None), 'n_rows')
    for wrong in (P3 + 1, 0, -1):
        assert failed(dw(H, H, H, H, wrong, 3, 15, 3, None), 'part_rows')
    assert failed(dw(H, H, H, H, 1, 0, 15, 3, None), 'part_rows')
    assert failed(step(H, -1, H, H, None, 15, 3, adam, None), 'part_rows') and failed(step(H, 257, H, H, None, 15, 3, adam, None), 'part_rows')


# ------------------------------------------------------------------------------------------------------------------------
# what the GPU tolerances rest on: the fp32 reference against the fp64 reference
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ('hybrid', 'pure'))
@pytest.mark.parametrize('r', [3, 8, 33])
@pytest.mark.parametrize('loss', LOSSES)
def test_fp32_oracle_step_lies_inside_the_intervals(loss, r, layout):
    p = relu_problem(3000 + r, 60, 40, r, loss, layout)
    ref64, ref32 = relu_oracle(p, BOTH, 1), relu_oracle(p, BOTH, 1, dtype=torch.float32)
    what = f'{loss} r={r} {layout} fp32 oracle'
    d = rel_err(ref32['loss'][0], ref64['loss'][0])
    print(f'[relu oracle step] {what}: loss differs by {d:.3g}')
    assert d < 1e-5, what
    for side, s in (('user', 'u'), ('item', 'v')):
        start = [p['relu_W' + s], p['relu_Wr' + s], np.zeros((1, 5 * r), np.float32)]
        grads = ref64['first_grads'][0 if side == 'user' else 1]
        assert [g.shape for g in grads] == [w.shape for w in start]
        for name, new, w0, g in zip(('W', 'relu_weight', 'relu_bias'), ref32[side + '_vars'], start, grads):
            assert_step(new, w0, g, LR, what=f'{what} {side} {name}')                 # no slack
        smallest, bound, ratio = kink_margin(p['relu_F' + s + '_dense'], p['relu_Wr' + s])
        print(f'[relu kink] {what} {side}: smallest non-zero |z| {smallest:.3g}, largest summation bound {bound:.3g}, ratio {ratio:.3g}')
        assert ratio > 10


@pytest.mark.parametrize('loss', LOSSES)
def test_fp32_oracle_trajectory(loss):
    epochs = 40 if loss == 'mse' else 10
    p = relu_problem(77, 50, 35, 8, loss, 'hybrid', item_everywhere=False)
    ref64, ref32 = relu_oracle(p, BOTH, epochs), relu_oracle(p, BOTH, epochs, dtype=torch.float32)
    first, ten = rel_err(ref32['loss'][:3], ref64['loss'][:3]), rel_err(ref32['loss'][:10], ref64['loss'][:10])
    print(f'[relu oracle trajectory] {loss}: 3 epochs {first:.3g}, 10 epochs {ten:.3g}, {epochs} epochs {rel_err(ref32["loss"], ref64["loss"]):.3g}')
    assert first < 1e-5 and ten < 1e-4
    assert rel_err(ref32['loss'], ref64['loss']) < 1e-3
