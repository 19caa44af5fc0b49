"""L2 regularisation (model.user_alpha / model.item_alpha) without a GPU: LogisticLoss and BPRLoss through the autograd loop against
fp64 references "closed-form data gradient + 2 alpha W0", the argument checks, the refused training forms, persistence and the
declaration of the four regularised table steps.  The engine's side of it: tests/test_gpu_l2.py."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_step, rel_err
from test_biased_cpu import LR
from test_bpr_cpu import _model as bpr_model
from test_bpr_cpu import bpr_closed_form, bpr_problem
from test_logistic_cpu import _model as logistic_model
from test_logistic_cpu import logistic_closed_form, logistic_problem

ALPHAS = ((0.5, 0.0), (0.0, 0.5), (0.3, 0.7))
L2_NAMES = ('tmf_adam_fresh_rows_l2_f32', 'tmf_adam_fresh_rows_l2_bf16', 'tmf_adam_state_rows_l2_f32', 'tmf_adam_bias_rows_l2_f32')
TRAJECTORY_LR, TRAJECTORY_EPOCHS = 0.05, 12


def fresh_adam_fp64(W, g, lr):
    """conftest.step_bounds' step: the reference's first Adam step with its fp32 constants, evaluated in fp64."""
    f = np.float32
    omb1, omb2, eps = float(f(1) - f(0.9)), float(f(1) - f(0.999)), float(f(1e-7))
    alpha = float(f(f(lr) * np.sqrt(f(f(1) - f(0.999))) / f(f(1) - f(0.9))))
    return W - (g * omb1 * alpha) / (np.sqrt(g * g * omb2) + eps)


def l2_trajectory(U0, V0, idx, val, alphas, epochs=TRAJECTORY_EPOCHS, lr=TRAJECTORY_LR):
    """The regularised LogisticLoss fit in fp64: the data term's closed-form gradients + 2 alpha W, one fresh-Adam step per epoch.
    -> (mean DATA loss of every epoch, U, V)."""
    U, V, out = U0.astype(np.float64), V0.astype(np.float64), []
    for _ in range(epochs):
        loss, gU, gV, _ = logistic_closed_form(U, V, idx, val, False)
        out.append(loss / idx.shape[0])
        U, V = fresh_adam_fp64(U, gU + 2 * alphas[0] * U, lr), fresh_adam_fp64(V, gV + 2 * alphas[1] * V, lr)
    return out, U, V


def fit(model, p, epochs, lr=LR):
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    m, n = p['U0'].shape[0], p['V0'].shape[0]
    model.fit(epochs, eye(m), eye(n), SparseInteractions(p['idx'], p['val'], (m, n), device='cpu'), lr=lr)
    return model


def tables(model):
    return model.user_embedding.detach().numpy(), model.item_embedding.detach().numpy()


@pytest.fixture
def no_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)


# ------------------------------------------------------------------------------------------------------------------------
# one step
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def one_step_cases():
    """Per loss: the problem, its fp64 data loss mean and gradients, a model builder and the tables of the unregularised fit."""
    lp = logistic_problem(21, 60, 40, 7, zeros=True)
    loss, gU, gV, _ = logistic_closed_form(lp['U0'], lp['V0'], lp['idx'], lp['val'], False)
    bp = bpr_problem(22, 30, 20, 4, 8)
    bloss, _, _, bgU, bgV = bpr_closed_form(bp['U0'], bp['V0'], bp['idx'], bp['val'], bp['R'])
    return dict(logistic=(lp, loss / lp['idx'].shape[0], gU, gV, logistic_model),
                bpr=(bp, bloss / int((bp['val'] > 0).sum()), bgU, bgV, bpr_model))


@pytest.mark.parametrize('alphas', ALPHAS, ids=str)
@pytest.mark.parametrize('loss', ['logistic', 'bpr'])
def test_one_step_against_fp64(no_gpu, one_step_cases, loss, alphas):
    p, data_loss, gU, gV, make = one_step_cases[loss]
    plain = tables(fit(make(p), p, 1))
    model = fit(make(p, user_alpha=alphas[0], item_alpha=alphas[1]), p, 1)
    assert not hasattr(model, '_state')
    U1, V1 = tables(model)
    assert_step(U1, p['U0'], gU + 2 * alphas[0] * p['U0'].astype(np.float64), LR, rtol=1e-5, what=f'{loss} {alphas} U')
    assert_step(V1, p['V0'], gV + 2 * alphas[1] * p['V0'].astype(np.float64), LR, rtol=1e-5, what=f'{loss} {alphas} V')
    for got, ref, alpha in zip((U1, V1), plain, alphas):
        if alpha == 0:
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), 'the unpenalised side moved differently'
        else:
            assert not np.array_equal(got, ref), 'the penalty moved nothing'
    assert rel_err(model.loss_history_[0], data_loss) < 1e-5          # the data term alone, with its own denominator


# ------------------------------------------------------------------------------------------------------------------------
# twelve epochs
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alphas', [(2.0, 2.0), (0.3, 0.7), (0.0, 2.0)], ids=str)
@pytest.mark.parametrize('seed', [6, 7, 8])
def test_trajectory(no_gpu, seed, alphas):
    p = logistic_problem(seed, 70, 45, 5, zeros=True)
    ref, _, _ = l2_trajectory(p['U0'], p['V0'], p['idx'], p['val'], alphas)
    model = fit(logistic_model(p, user_alpha=alphas[0], item_alpha=alphas[1]), p, TRAJECTORY_EPOCHS, lr=TRAJECTORY_LR)
    h = model.loss_history_
    print(f'[trajectory] seed={seed} alphas={alphas}: first three {rel_err(h[:3], ref[:3]):.3g}, all {rel_err(h, ref):.3g}')
    assert len(h) == TRAJECTORY_EPOCHS and rel_err(h[:3], ref[:3]) < 1e-5 and rel_err(h, ref) < 1e-3


@pytest.mark.parametrize('seed', [6, 7, 8])
def test_the_penalty_shrinks_the_tables_and_costs_data_loss(no_gpu, seed):
    p = logistic_problem(seed, 70, 45, 5, zeros=True)
    plain = fit(logistic_model(p), p, TRAJECTORY_EPOCHS, lr=TRAJECTORY_LR)
    reg = fit(logistic_model(p, user_alpha=2.0, item_alpha=2.0), p, TRAJECTORY_EPOCHS, lr=TRAJECTORY_LR)
    for a, b in zip(tables(reg), tables(plain)):
        assert np.linalg.norm(a) < np.linalg.norm(b)
    assert reg.loss_history_[-1] > plain.loss_history_[-1]
    assert reg.loss_history_[0] == plain.loss_history_[0]             # the first loss is taken before any step


# ------------------------------------------------------------------------------------------------------------------------
# which variables carry the penalty
# ------------------------------------------------------------------------------------------------------------------------
def test_a_bias_is_never_penalised(no_gpu):
    from teamoflow_amd.mf.embedding_graphs import BiasedLinearEmbedding
    p = logistic_problem(23, 30, 20, 5)
    graphs = lambda: dict(user_repr_graph=BiasedLinearEmbedding(), item_repr_graph=BiasedLinearEmbedding())   # noqa: E731
    plain = fit(logistic_model(p, **graphs()), p, 1)
    reg = fit(logistic_model(p, user_alpha=0.4, item_alpha=0.6, **graphs()), p, 1)
    _, gU, gV, _ = logistic_closed_form(p['U0'], p['V0'], p['idx'], p['val'], False)   # the biases start at zero: E0 = W0
    for side, W0, g, alpha in (('user', p['U0'], gU, 0.4), ('item', p['V0'], gV, 0.6)):
        W, b = getattr(reg, side + '_trainable')
        assert torch.equal(b, getattr(plain, side + '_trainable')[1]), f'{side} bias'
        assert_step(W.detach().numpy(), W0, g + 2 * alpha * W0.astype(np.float64), LR, rtol=1e-5, what=f'{side} weights')


def test_relu_weight_is_penalised_and_relu_bias_is_not(no_gpu):
    """One step from hidden variables put on the model beforehand (what an earlier fit leaves), so that both fits start from the
    same values: weights and relu_weight step by the penalised gradient, relu_bias as without a penalty."""
    from teamoflow_amd.mf.embedding_graphs import ReLUEmbedding
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import LogisticLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    p = logistic_problem(24, 12, 9, 2)
    fits = []
    for alpha in (0.0, 0.8):
        W0 = np.random.default_rng(3).standard_normal((10, 2)).astype(np.float32) * 0.3
        model = MatrixFactorization(2, user_repr_graph=ReLUEmbedding(), loss_graph=LogisticLoss(), user_weight_graph=FixedInitializer(W0),
                                    item_weight_graph=FixedInitializer(p['V0']))
        model.verbose = False
        model.user_relu_weight = torch.tensor(np.random.default_rng(4).standard_normal((12, 10)).astype(np.float32)).requires_grad_(True)
        model.user_relu_bias = torch.zeros(1, 10, requires_grad=True)
        Wr0 = model.user_relu_weight.detach().clone()
        model.user_alpha = alpha
        fits.append((fit(model, p, 1), Wr0))
    (plain, Wr0), (reg, _) = fits
    assert torch.equal(reg.user_trainable[2], plain.user_trainable[2])                 # relu_bias: no penalty
    assert torch.equal(reg.item_embedding, plain.item_embedding)                       # the other side: alpha = 0
    assert not torch.equal(reg.user_trainable[0], plain.user_trainable[0])
    # relu_weight: where the data gradient is exactly zero (a unit no row switches on sees no data gradient) the penalised fit
    # moves the weight towards zero by a full step while the plain fit leaves it
    still = (plain.user_trainable[1].detach() == Wr0) & (Wr0 != 0)
    assert still.any()
    moved = reg.user_trainable[1].detach()[still]
    assert ((moved - Wr0[still]).abs() > 0.9 * LR).all() and ((moved.abs() < Wr0[still].abs()) | (Wr0[still].abs() < LR)).all()


# ------------------------------------------------------------------------------------------------------------------------
# argument checks and the refused forms
# ------------------------------------------------------------------------------------------------------------------------
class NoDraw:
    def initialize_weights(self, *a, **k):
        pytest.fail('a weight was drawn')


@pytest.mark.parametrize('gpu', [False, True], ids=['cpu', 'gpu'])
@pytest.mark.parametrize('bad', [-0.1, float('nan'), float('inf'), -float('inf'), 1e39], ids=str)
@pytest.mark.parametrize('name', ['user_alpha', 'item_alpha'])
def test_a_negative_or_non_finite_alpha_is_refused(monkeypatch, name, bad, gpu):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: gpu)
    p = logistic_problem(25, 12, 9, 4)
    model = logistic_model(p, **{name: bad})
    model.user_weight_graph = model.item_weight_graph = NoDraw()
    with pytest.raises(ValueError, match=name):
        fit(model, p, 1)


@pytest.mark.parametrize('gpu', [False, True], ids=['cpu', 'gpu'])
@pytest.mark.parametrize('setting', [('relu_engine', True), ('batch_users', 8), ('shard_items', 2), ('data_parallel', True),
                                     ('data_parallel', 'force')], ids=lambda s: f'{s[0]}={s[1]}')
@pytest.mark.parametrize('alphas', [(0.5, 0.0), (0.0, 0.5)], ids=str)
def test_unbuilt_forms_are_refused_before_anything_is_drawn(monkeypatch, setting, alphas, gpu):
    from teamoflow_amd import _engine
    from teamoflow_amd.mf.embedding_graphs import ReLUEmbedding
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: gpu)
    for fn in ('_fit_sparse', '_fit_generic'):
        monkeypatch.setattr(MatrixFactorization, fn, lambda self, *a, **k: pytest.fail('a fit was started'))
    monkeypatch.setattr(_engine, 'InteractionPlan', lambda *a, **k: pytest.fail('a plan was built'))
    p = logistic_problem(26, 12, 9, 4)
    graphs = dict(user_repr_graph=ReLUEmbedding()) if setting[0] == 'relu_engine' else {}
    model = logistic_model(p, user_alpha=alphas[0], item_alpha=alphas[1], **{setting[0]: setting[1]}, **graphs)
    model.user_weight_graph = model.item_weight_graph = NoDraw()
    with pytest.raises(NotImplementedError, match=setting[0]):
        fit(model, p, 1)


def test_the_same_settings_without_a_penalty_are_not_refused(monkeypatch):
    """The refusal is about the penalty: with both alphas 0 every one of these settings reaches its fit as before."""
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    started = []
    monkeypatch.setattr(MatrixFactorization, '_fit_generic', lambda self, *a, **k: started.append(1))
    p = logistic_problem(26, 12, 9, 4)
    for setting in (('relu_engine', True), ('batch_users', 8), ('shard_items', 2)):
        fit(logistic_model(p, **{setting[0]: setting[1]}), p, 1)
    assert len(started) == 3


# ------------------------------------------------------------------------------------------------------------------------
# persistence
# ------------------------------------------------------------------------------------------------------------------------
def test_save_and_load_carry_the_alphas(no_gpu, tmp_path):
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    p = logistic_problem(27, 12, 9, 4)
    model = fit(logistic_model(p, user_alpha=0.25, item_alpha=1.5), p, 2)
    path = str(tmp_path / 'model.pt')
    model.save(path)
    blob = torch.load(path, weights_only=True)
    assert blob['format'] == 'teamoflow_amd.mf/2' and (blob['user_alpha'], blob['item_alpha']) == (0.25, 1.5)
    back = MatrixFactorization.load(path, device='cpu')
    assert (back.user_alpha, back.item_alpha) == (0.25, 1.5)
    assert fit(back, p, 2).loss_history_ == model.loss_history_ and torch.equal(back.user_embedding, model.user_embedding)
    # a file written before the attributes existed
    del blob['user_alpha'], blob['item_alpha']
    old = str(tmp_path / 'old.pt')
    torch.save(blob, old)
    older = MatrixFactorization.load(old, device='cpu')
    assert (older.user_alpha, older.item_alpha) == (0.0, 0.0)
    fresh = MatrixFactorization(3)
    assert (fresh.user_alpha, fresh.item_alpha) == (0.0, 0.0)


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_built():
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load_library()
    for name in L2_NAMES:
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        base = _lib.SIGNATURES[name.replace('_l2', '')]
        assert res is base[0] and args == base[1][:-1] + [_lib._F, _lib._P], name      # the function extended + `float l2` before the stream


def test_argument_checks_fail_before_any_launch():
    """Bad arguments return TMF_E_INVALID from the host-side checks: no launch is attempted, so this runs without a GPU."""
    import ctypes
    from teamoflow_amd import _lib
    lib = _lib.load_library()
    adam = lib.tmf_adam_fresh(0.05)
    buf = (ctypes.c_float * 64)()
    P = ctypes.cast(buf, ctypes.c_void_p)
    nan = float('nan')
    for name in L2_NAMES:
        fn = getattr(lib, name)
        tabs = {'tmf_adam_fresh_rows_l2_f32': 2, 'tmf_adam_fresh_rows_l2_bf16': 2}.get(name, 4)
        for l2, r, null in ((-1.0, 8, None), (nan, 8, None), (float('inf'), 8, None), (0.25, 0, None), (0.25, 1025, None), (0.25, 8, 0),
                            (0.25, 8, 1)):
            ptrs = [None if k == null else P for k in range(tabs)]
            assert fn(*ptrs, 1, r, adam, l2, None) == -1, (name, l2, r, null)
            assert lib.tmf_last_error()
        assert fn(*([None] * tabs), 0, 8, adam, 0.25, None) == 0                       # no rows: nothing to do
    assert not any(buf)
