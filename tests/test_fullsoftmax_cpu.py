"""FullSoftmaxLoss without a GPU: the NumPy fp64 closed form the GPU tests compare against, pinned to the plug-in's own get_loss; an
fp32 restatement (torch fp32 matmul and logsumexp) that meets, on the GPU tests' inputs, the tolerances those tests use; the generic
loop; routing, refusals, loss_name / run_epoch, save and load; the C ABI's declarations and argument checks."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_step, rel_err
from test_bpr_cpu import LR, bpr_problem, fresh_adam_fp32

# the shapes of the kernel tests (tests/test_gpu_fullsoftmax.py): (m, n, r)
KERNEL_SHAPES = [(1, 1, 1), (130, 131, 5), (300, 257, 33), (257, 300, 128), (129, 1000, 64)]
TIMES_SIX = (33, 300, 257, 33, 8)   # bpr_problem's arguments of the case whose tables are scaled by 6: max |score| 94.6 > 88.7


def fullsoftmax_closed_form(U, V, idx, val):
    """One FullSoftmaxLoss epoch in fp64.  idx: (user, item) pairs, val their stored values.
    -> (loss sum over the entries with a value > 0, gU, gV): the gradients of that sum."""
    U, V = np.asarray(U, np.float64), np.asarray(V, np.float64)
    idx, val = np.asarray(idx, np.int64).reshape(-1, 2), np.asarray(val)
    u, i = idx[val > 0, 0], idx[val > 0, 1]
    s = U @ V.T
    mx = s.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(s - mx).sum(axis=1))
    n_u = np.bincount(u, minlength=U.shape[0]).astype(np.float64)
    P = n_u[:, None] * np.exp(s - lse[:, None])            # n_u pi_ui
    gU, gV = P @ V, P.T @ U
    np.subtract.at(gU, u, V[i])
    np.subtract.at(gV, i, U[u])
    return float((lse[u] - s[u, i]).sum()), gU, gV


def fullsoftmax_fp32(U, V, idx, val):
    """The same in fp32 with torch's matmul and logsumexp; the loss terms are summed in fp64 (as tmf_sum_f32 does).
    -> (loss sum, gU, gV, lse) with fp32 arrays."""
    U, V = torch.as_tensor(np.asarray(U, np.float32)), torch.as_tensor(np.asarray(V, np.float32))
    idx, val = np.asarray(idx, np.int64).reshape(-1, 2), np.asarray(val)
    u, i = torch.as_tensor(idx[val > 0, 0]), torch.as_tensor(idx[val > 0, 1])
    s = U @ V.T
    lse = torch.logsumexp(s, dim=1)
    n_u = torch.bincount(u, minlength=U.shape[0]).to(torch.float32)
    P = n_u[:, None] * torch.exp(s - lse[:, None])
    gU, gV = P @ V, P.T @ U
    gU.index_add_(0, u, -V[i])
    gV.index_add_(0, i, -U[u])
    return float((lse[u] - s[u, i]).double().sum()), gU.numpy(), gV.numpy(), lse.numpy()


def fresh_adam_fp64(W, g, lr):
    """conftest.step_bounds' step: the reference's first Adam step with its fp32 constants, evaluated in fp64."""
    f = np.float32
    omb1, omb2, eps = float(f(1) - f(0.9)), float(f(1) - f(0.999)), float(f(1e-7))
    alpha = float(f(f(lr) * np.sqrt(f(f(1) - f(0.999))) / f(f(1) - f(0.9))))
    return W - (g * omb1 * alpha) / (np.sqrt(g * g * omb2) + eps)


def times_six():
    p = dict(bpr_problem(*TIMES_SIX))
    p['U0'], p['V0'] = p['U0'] * np.float32(6), p['V0'] * np.float32(6)
    return p


# ------------------------------------------------------------------------------------------------------------------------
# the closed form
# ------------------------------------------------------------------------------------------------------------------------
def test_closed_form_on_a_problem_small_enough_to_write_out():
    """Two users, three items, r = 1.  User 0 stores item 0 (value 2) and item 2 (value -1: no part); user 1 stores nothing."""
    U, V = np.array([[1.0], [3.0]]), np.array([[0.0], [np.log(2.0)], [np.log(3.0)]])
    loss, gU, gV = fullsoftmax_closed_form(U, V, [[0, 0], [0, 2]], [2.0, -1.0])
    pi = np.array([1, 2, 3]) / 6.0                                            # exp(s) = 1, 2, 3
    assert abs(loss - np.log(6.0)) < 1e-14
    assert np.allclose(gU, [[pi @ V[:, 0] - 0.0], [0.0]], atol=1e-14)         # n_0 = 1; user 1 has no positive: a zero row
    assert np.allclose(gV[:, 0], pi * 1.0 - np.array([1.0, 0, 0]), atol=1e-14)  # every item moves, the stored non-positive like any other


def _autograd(U, V, idx, val, dtype=torch.float64):
    from teamoflow_amd.mf.loss_graphs import FullSoftmaxLoss
    from teamoflow_amd.mf.sparse import SparseInteractions
    U, V = (torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in (U, V))
    inter = SparseInteractions(idx, val, (U.shape[0], V.shape[0]), device='cpu')
    out = FullSoftmaxLoss().get_loss(tf_interactions=inter, tf_sample_predictions=None, tf_prediction_serial=None,
                                     predictions=U @ V.T, n_items=V.shape[0], n_samples=3)
    gU, gV = torch.autograd.grad(out.sum(), (U, V))
    return out.detach().numpy(), gU.numpy(), gV.numpy()


@pytest.mark.parametrize('shape', [(33, 47, 5), (60, 40, 7), (20, 15, 3)], ids=lambda s: 'x'.join(map(str, s)))
def test_get_loss_is_the_closed_form(shape):
    m, n, r = shape
    p = bpr_problem(sum(shape), m, n, r, 4)
    loss, gU, gV = fullsoftmax_closed_form(p['U0'], p['V0'], p['idx'], p['val'])
    out, aU, aV = _autograd(p['U0'], p['V0'], p['idx'], p['val'])
    assert out.shape == (int((p['val'] > 0).sum()),)                          # one term per stored value > 0: the mean's denominator
    assert max(rel_err(out.sum(), loss), rel_err(aU, gU), rel_err(aV, gV)) < 1e-12
    assert not gU[p['empty_user']].any() and not gU[p['nonpos_user']].any()    # n_u = 0
    assert gV[p['empty_item']].any()                                          # dense on the item side
    dup = np.concatenate([p['idx'], p['idx'][p['val'] > 0][:1]]), np.concatenate([p['val'], p['val'][p['val'] > 0][:1]])
    loss2, gU2, gV2 = fullsoftmax_closed_form(p['U0'], p['V0'], *dup)          # a duplicate counts as often as it is stored
    out2, aU2, aV2 = _autograd(p['U0'], p['V0'], *dup)
    assert loss2 > loss and max(rel_err(out2.sum(), loss2), rel_err(aU2, gU2), rel_err(aV2, gV2)) < 1e-12


def test_class_surface():
    from teamoflow_amd.mf import loss_graphs as LG
    from teamoflow_amd.mf import matrix_factorization as M
    assert issubclass(LG.FullSoftmaxLoss, LG.LossGraph) and not vars(LG.FullSoftmaxLoss()).keys()      # no parameters
    assert LG.FullSoftmaxLoss in M.ENGINE_LOSSES and LG.FullSoftmaxLoss not in M.TABLE_LOSSES + M.PAIR_STEP_LOSSES
    from teamoflow_amd import _engine
    assert 'full_softmax' not in _engine.PAIR_LOSSES


# ------------------------------------------------------------------------------------------------------------------------
# fp32 meets the GPU tests' tolerances on their inputs
# ------------------------------------------------------------------------------------------------------------------------
FP32_CASES = [(5, 300, 257, 5, 8), (33, 300, 257, 33, 8), (128, 300, 257, 128, 8), (131, 130, 131, 128, 8)]


@pytest.mark.parametrize('args', FP32_CASES + ['x6'], ids=lambda a: a if isinstance(a, str) else 'x'.join(map(str, a[1:4])))
def test_fp32_meets_the_gpu_tolerances(args):
    """torch fp32 against the fp64 closed form: rel_err < 1e-5 for the loss, lse and both gradients, and the fp32 step of those
    gradients inside assert_step(rtol=1e-5) - on bpr_problem tables, and on the case scaled by 6 whose largest |score| (94.6) is
    above 88.7, where an fp32 exp of a score overflows: only a running maximum keeps it finite."""
    p = times_six() if args == 'x6' else bpr_problem(*args)
    if args == 'x6':
        assert np.abs(p['U0'].astype(np.float64) @ p['V0'].astype(np.float64).T).max() > 88.73
    loss, gU, gV = fullsoftmax_closed_form(p['U0'], p['V0'], p['idx'], p['val'])
    l32, aU, aV, lse = fullsoftmax_fp32(p['U0'], p['V0'], p['idx'], p['val'])
    assert np.isfinite(lse).all() and np.isfinite(aU).all() and np.isfinite(aV).all()
    errs = rel_err(l32, loss), rel_err(aU, gU), rel_err(aV, gV)
    print(f'[fp32] {args}: loss {errs[0]:.3g} gU {errs[1]:.3g} gV {errs[2]:.3g}')
    assert max(errs) < 1e-5, errs
    assert_step(fresh_adam_fp32(p['U0'], aU, LR), p['U0'], gU, LR, rtol=1e-5, what=f'{args} U')
    assert_step(fresh_adam_fp32(p['V0'], aV, LR), p['V0'], gV, LR, rtol=1e-5, what=f'{args} V')


def test_ten_fp32_epochs_follow_fp64():
    """200 x 150, r = 16, lr 0.05: ten fp32 epochs keep every epoch's mean loss within 1e-7 of ten fp64 closed-form steps.  The
    tables drift (the step is nearly a sign function), so a trajectory compares losses, not tables."""
    p = bpr_problem(6, 200, 150, 16, 32)
    n_pos = int((p['val'] > 0).sum())
    U, V = p['U0'].astype(np.float64), p['V0'].astype(np.float64)
    U32, V32 = p['U0'].copy(), p['V0'].copy()
    errs = []
    for _ in range(10):
        loss, gU, gV = fullsoftmax_closed_form(U, V, p['idx'], p['val'])
        l32, aU, aV, _ = fullsoftmax_fp32(U32, V32, p['idx'], p['val'])
        errs.append(abs(l32 - loss) / loss)
        U, V = fresh_adam_fp64(U, gU, LR), fresh_adam_fp64(V, gV, LR)
        U32, V32 = fresh_adam_fp32(U32, aU, LR), fresh_adam_fp32(V32, aV, LR)
    print(f'[fp32 trajectory] per epoch: {" ".join(f"{e:.2g}" for e in errs)}; tables apart by {np.abs(U32 - U).max():.2g}')
    assert max(errs) < 1e-7 and loss / n_pos < np.log(150)


# ------------------------------------------------------------------------------------------------------------------------
# the model without a GPU
# ------------------------------------------------------------------------------------------------------------------------
def _model(p, loss=None, **attrs):
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import FullSoftmaxLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    model = MatrixFactorization(attrs.pop('r', p['r']), loss_graph=loss or FullSoftmaxLoss(), user_weight_graph=FixedInitializer(p['U0']),
                                item_weight_graph=FixedInitializer(p['V0']), n_users=p['m'], n_items=p['n'], n_samples=p['S'])
    model.verbose = False
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


def _fit(model, p, epochs):
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    model.fit(epochs, eye(p['m']), eye(p['n']), SparseInteractions(p['idx'], p['val'], (p['m'], p['n']), device='cpu'), lr=LR)
    return model


def test_generic_fit_without_a_gpu(monkeypatch):
    """30 x 20, r = 4 through _fit_generic: the first loss is the closed form's mean over the positives, one step moves both tables
    as the closed-form gradients say, 20 epochs lower the loss; no negative table is read or drawn."""
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    p = bpr_problem(14, 30, 20, 4, 8)
    loss, gU, gV = fullsoftmax_closed_form(p['U0'], p['V0'], p['idx'], p['val'])
    one = _fit(_model(p), p, 1)
    assert not hasattr(one, '_state') and one.random_ind is None and one.resample_rounds_ == 0
    assert rel_err(one.loss_history_[0], loss / int((p['val'] > 0).sum())) < 1e-5
    assert_step(one.user_embedding.detach().numpy(), p['U0'], gU, LR, rtol=1e-5, what='U')
    assert_step(one.item_embedding.detach().numpy(), p['V0'], gV, LR, rtol=1e-5, what='V')
    assert np.array_equal(one.user_embedding.detach().numpy()[p['empty_user']], p['U0'][p['empty_user']])
    h = _fit(_model(p, resample_every=1), p, 20).loss_history_               # resample_every has no effect on it
    assert len(h) == 20 and h[-1] < h[0] and all(b < a for a, b in zip(h[:5], h[1:6])), h
    assert h[0] == one.loss_history_[0]


def test_loss_name_and_routes(monkeypatch):
    from teamoflow_amd import _engine
    from teamoflow_amd.mf import loss_graphs as LG
    from teamoflow_amd.mf.sparse import eye

    class Mine(LG.FullSoftmaxLoss):
        pass
    assert _engine.loss_name(LG.FullSoftmaxLoss()) == 'full_softmax'
    with pytest.raises(TypeError, match='FullSoftmaxLoss'):
        _engine.loss_name(Mine())
    p = bpr_problem(16, 12, 9, 4, 4)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    for settings in ({}, dict(optimizer='adam'), dict(user_alpha=0.5), dict(resample_every=2), dict(r=_engine.FULL_SOFTMAX_MAX_COMPONENTS)):
        assert _model(p, **settings)._route(eye(12), eye(9)) == 'engine', settings
    assert _model(p, loss=Mine())._route(eye(12), eye(9)) == 'generic'
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    assert _model(p)._route(eye(12), eye(9)) == 'generic'
    assert _model(p, factor_dtype=torch.bfloat16)._route(eye(12), eye(9)) == 'generic'      # the refusals are the engine's


def test_a_full_softmax_epoch_needs_its_state():
    """run_epoch on no state, or on one built without full_softmax=True, is refused - never run as another loss."""
    from teamoflow_amd import _engine

    class State:
        wplan = None
    for st in (None, State()):
        with pytest.raises(ValueError, match="'full_softmax' on a state built without full_softmax=True"):
            _engine.run_epoch(st, None, None, 'full_softmax')


REFUSED = [('batch_users', 8), ('shard_items', 2), ('data_parallel', True), ('data_parallel', 'force'), ('factor_dtype', torch.bfloat16),
           ('r', 129)]


@pytest.mark.parametrize('setting', REFUSED, ids=lambda s: f'{s[0]}={s[1]}')
def test_unbuilt_forms_are_refused_before_anything_is_drawn(monkeypatch, setting):
    from teamoflow_amd import _engine
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    assert _engine.FULL_SOFTMAX_MAX_COMPONENTS + 1 == 129
    p = bpr_problem(17, 12, 9, 4, 4)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    for name in ('_fit_sparse', '_fit_generic'):
        monkeypatch.setattr(MatrixFactorization, name, lambda self, *a, **k: pytest.fail('a fit was started'))
    monkeypatch.setattr(_engine, 'InteractionPlan', lambda *a, **k: pytest.fail('a plan was built'))
    monkeypatch.setattr(FixedInitializer, 'initialize_weights', lambda self, *a, **k: pytest.fail('a weight was drawn'))
    match = {'factor_dtype': 'factor_dtype', 'r': 'n_components=129 > 128'}.get(setting[0], setting[0])
    with pytest.raises(NotImplementedError, match=match):
        _fit(_model(p, **{setting[0]: setting[1]}), p, 1)


def test_save_and_load(tmp_path, monkeypatch):
    from teamoflow_amd.mf.loss_graphs import FullSoftmaxLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    p = bpr_problem(18, 12, 9, 4, 4)
    model = _fit(_model(p), p, 2)
    path = str(tmp_path / 'model.pt')
    model.save(path)
    back = MatrixFactorization.load(path, device='cpu')
    assert type(back.loss_graph) is FullSoftmaxLoss and back.loss_history_ == model.loss_history_ and back.random_ind is None
    assert torch.equal(back.user_embedding, model.user_embedding.detach())
    again = _fit(back, p, 2)                                            # a loaded model trains again, through the same path
    assert again.loss_history_ == model.loss_history_


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------
FSM_NAMES = ('tmf_fsm_max_components', 'tmf_fsm_lse_f32', 'tmf_fsm_wsum_f32', 'tmf_fsm_pos_pass_f32')


def test_entry_points_are_declared_bound_and_built():
    from teamoflow_amd import _engine, _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    declared = set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    lib = _lib.load_library()
    for name in FSM_NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    make = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS :=.*\btmf_fullsoftmax\.hip\b', make, re.M)
    assert lib.tmf_fsm_max_components() == _engine.FULL_SOFTMAX_MAX_COMPONENTS >= 128
    assert lib.tmf_version() == _lib.MIN_LIB_VERSION


def test_argument_checks_fail_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail differently (or crash); these return first."""
    import ctypes

    from teamoflow_amd import _lib
    lib = _lib.load_library()
    buf = (ctypes.c_float * 1024)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    A = ctypes.c_void_p(addr)
    odd = ctypes.c_void_p(addr + 4)
    INVALID, UNSUPPORTED = -1, None
    assert lib.tmf_fsm_lse_f32(A, A, 0, 5, 4, 4, 4, A, None) == 0                      # no rows: nothing to do
    assert lib.tmf_fsm_wsum_f32(A, A, 0, 5, 4, 4, 4, A, A, 1, A, 4, None) == 0
    assert lib.tmf_fsm_wsum_f32(A, A, 5, 0, 4, 4, 4, A, A, 0, A, 4, None) == 0
    bad = [lib.tmf_fsm_lse_f32(None, A, 2, 2, 4, 4, 4, A, None), lib.tmf_fsm_lse_f32(A, A, 2, 2, 4, 4, 4, None, None),
           lib.tmf_fsm_lse_f32(A, A, 2, 0, 4, 4, 4, A, None), lib.tmf_fsm_lse_f32(A, A, 2, 2, 5, 4, 8, A, None),
           lib.tmf_fsm_lse_f32(A, A, 2, 2, 4, 6, 4, A, None), lib.tmf_fsm_lse_f32(odd, A, 2, 2, 4, 4, 4, A, None),
           lib.tmf_fsm_wsum_f32(A, A, 2, 2, 4, 4, 4, None, A, 1, A, 4, None), lib.tmf_fsm_wsum_f32(A, A, 2, 2, 4, 4, 4, A, A, 2, A, 4, None),
           lib.tmf_fsm_wsum_f32(A, A, 2, 2, 8, 8, 8, A, A, 1, A, 4, None), lib.tmf_fsm_wsum_f32(A, A, 2, 2, 4, 4, 4, A, A, 1, None, 4, None)]
    assert all(rc != 0 for rc in bad), bad
    wide = [lib.tmf_fsm_lse_f32(A, A, 2, 2, 129, 132, 132, A, None), lib.tmf_fsm_wsum_f32(A, A, 2, 2, 129, 132, 132, A, A, 1, A, 132, None)]
    assert all(rc != 0 for rc in wide) and b'128' in lib.tmf_last_error()
    assert lib.tmf_fsm_pos_pass_f32(None, A, A, A, A, A, A, A, A, 4, None) != 0
