"""CPU side of LogisticLoss (no GPU): the NumPy closed form the GPU tests compare the engine with, the statement their tolerances
rest on (that closed form in fp32 with a shuffled entry order against itself in fp64), the plug-in's own get_loss, the C ABI of
tmf_logistic_pass_* (declared, bound, built, argument checks that fail before anything is launched), the dispatch with and
without a GPU, save / load, and the row loads of the new kernel's gather loop (tests/test_isa_guard.py's statement)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_step, rel_err
from test_biased_cpu import LR, biased_problem
from test_isa_guard import _immediately_waited

LOGISTIC_NAMES = ('tmf_logistic_pass_f32', 'tmf_logistic_pass_bf16')
WEIGHTINGS = (False, True)


# ------------------------------------------------------------------------------------------------------------------------
# the reference: shares no code with the package
# ------------------------------------------------------------------------------------------------------------------------
def logistic_closed_form(U, V, idx, val, weighted, dtype=np.float64, order=None):
    """Loss and gradients of one LogisticLoss epoch in ``dtype``: y = +1 where val > 0 else -1, w = |val| or 1, x = -y p,
    loss_k = w softplus(x), d loss_k / d p = -y w sigma(x), both from t = exp(-|x|).  ``order``: the order in which the entries
    are added (a permutation; fp32 sums depend on it).  -> (loss sum, gU, gV, per-entry losses in the given order)."""
    U, V, val = np.asarray(U, dtype), np.asarray(V, dtype), np.asarray(val, dtype)
    if order is not None:
        idx, val = idx[order], val[order]
    u, i = idx[:, 0], idx[:, 1]
    p = np.einsum('kr,kr->k', U[u], V[i]).astype(dtype)
    y = np.where(val > 0, dtype(1), dtype(-1))
    w = np.abs(val) if weighted else np.ones_like(val)
    x = -y * p
    t = np.exp(-np.abs(x))
    loss_k = w * (np.maximum(x, dtype(0)) + np.log1p(t))
    c = -y * w * (np.where(x >= 0, dtype(1), t) / (dtype(1) + t))
    gU, gV = np.zeros_like(U), np.zeros_like(V)
    np.add.at(gU, u, c[:, None] * V[i])
    np.add.at(gV, i, c[:, None] * U[u])
    return loss_k.sum(dtype=dtype), gU, gV, loss_k


def logistic_problem(seed, m, n, r, zeros=False):
    """test_biased_cpu.biased_problem with signed values 1..5 (its 'kl' variant); ``zeros``: every seventh value a stored 0."""
    p = biased_problem(seed, m, n, r, 'kl')
    p['loss'] = 'logistic'   # the helpers of the biased / featured tests then leave the model's loss_graph alone
    if zeros:
        p['val'] = p['val'].copy()
        p['val'][::7] = 0.0
    return p


def fresh_adam_fp32(W0, g, lr):
    """The reference's step at iteration 1 in fp32 (matrix_factorization.py:176)."""
    f = np.float32
    omb1, omb2, eps = f(1) - f(0.9), f(1) - f(0.999), f(1e-7)
    alpha = f(f(lr) * np.sqrt(omb2) / omb1)
    W0, g = np.asarray(W0, f), np.asarray(g, f)
    return W0 - ((g * omb1) * alpha) / (np.sqrt((g * g) * omb2) + eps)


def test_problem_generator():
    p, q = logistic_problem(3, 60, 40, 7), logistic_problem(3, 60, 40, 7, zeros=True)
    assert (p['val'] > 0).any() and (p['val'] < 0).any() and not (p['val'] == 0).any()
    assert set(np.abs(p['val']).astype(int)) == {1, 2, 3, 4, 5}
    assert (q['val'] == 0).sum() == -(-q['val'].size // 7) and (q['val'] > 0).any() and (q['val'] < 0).any()
    assert np.array_equal(p['idx'], q['idx']) and p['empty_user'] not in p['idx'][:, 0] and p['empty_item'] not in p['idx'][:, 1]


SHAPES = [(60, 40, r) for r in (1, 3, 7, 33, 128, 200)] + [(300, 90, 33), (2000, 50, 3), (2000, 50, 64)]


@pytest.mark.parametrize('weighted', WEIGHTINGS, ids=['plain', 'weighted'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_fp32_closed_form_meets_the_tolerances(shape, weighted):
    """What the GPU tolerances rest on: fp32 arithmetic and another order of additions stay within rel_err 1e-5 of the fp64
    closed form (loss and raw gradients), and the fp32 step of the fp32 gradient inside assert_step's interval."""
    p = logistic_problem(sum(shape), *shape, zeros=shape[2] in (3, 33))
    idx, val, U0, V0 = p['idx'], p['val'], p['U0'], p['V0']
    loss, gU, gV, _ = logistic_closed_form(U0, V0, idx, val, weighted)
    order = np.random.default_rng(1).permutation(idx.shape[0])
    loss32, gU32, gV32, _ = logistic_closed_form(U0, V0, idx, val, weighted, np.float32, order)
    assert gU32.dtype == np.float32 and loss32.dtype == np.float32
    errs = rel_err(loss32, loss), rel_err(gU32, gU), rel_err(gV32, gV)
    print(f'[fp32 reference] {shape} weighted={weighted}: loss {errs[0]:.3g} gU {errs[1]:.3g} gV {errs[2]:.3g}')
    assert max(errs) < 1e-5, errs
    assert_step(fresh_adam_fp32(U0, gU32, LR), U0, gU, LR, rtol=1e-5, what=f'{shape} U')
    assert_step(fresh_adam_fp32(V0, gV32, LR), V0, gV, LR, rtol=1e-5, what=f'{shape} V')
    assert not gU[p['empty_user']].any() and not gV[p['empty_item']].any()


# ------------------------------------------------------------------------------------------------------------------------
# the plug-in
# ------------------------------------------------------------------------------------------------------------------------
def _get_loss(U, V, idx, val, weighted, dtype=torch.float64):
    """(per-entry losses, dL/dU, dL/dV) of LogisticLoss.get_loss on the dense scores, by autograd."""
    from teamoflow_amd.mf.loss_graphs import LogisticLoss
    from teamoflow_amd.mf.sparse import SparseInteractions
    U, V = (torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in (U, V))
    inter = SparseInteractions(idx, val, (U.shape[0], V.shape[0]), device='cpu')
    out = LogisticLoss(weighted).get_loss(tf_interactions=inter, tf_sample_predictions=None, tf_prediction_serial=None,
                                          predictions=U @ V.T, n_items=None, n_samples=None)
    gU, gV = torch.autograd.grad(out.sum(), (U, V))
    return out.detach().numpy(), gU.numpy(), gV.numpy()


def test_class_surface():
    import teamoflow.mf.loss_graphs as alias
    from teamoflow_amd.mf import loss_graphs as LG
    assert alias.LogisticLoss is LG.LogisticLoss and issubclass(LG.LogisticLoss, LG.LossGraph)
    assert LG.LogisticLoss().weighted is False and LG.LogisticLoss(weighted=True).weighted is True and LG.LogisticLoss(1).weighted is True


@pytest.mark.parametrize('weighted', WEIGHTINGS, ids=['plain', 'weighted'])
@pytest.mark.parametrize('zeros', [False, True], ids=['signed', 'zeros'])
def test_get_loss_is_the_closed_form(weighted, zeros):
    p = logistic_problem(11, 33, 47, 5, zeros=zeros)
    loss, gU, gV, loss_k = logistic_closed_form(p['U0'], p['V0'], p['idx'], p['val'], weighted)
    out, aU, aV = _get_loss(p['U0'], p['V0'], p['idx'], p['val'], weighted)
    assert out.shape == (p['idx'].shape[0],) and out.dtype == np.float64
    assert rel_err(out, loss_k) < 1e-13 and rel_err(aU, gU) < 1e-13 and rel_err(aV, gV) < 1e-13
    if zeros:   # a stored 0 is a negative: weight 1 plain, weight 0 weighted
        at = p['val'] == 0
        assert (out[at] == 0).all() if weighted else (out[at] > 0).all()


@pytest.mark.parametrize('weighted', WEIGHTINGS, ids=['plain', 'weighted'])
def test_a_score_of_exactly_zero(weighted):
    """A zero user row (the embedding of an empty row of a featured side): every score is 0, every coefficient -y w / 2."""
    p = logistic_problem(12, 20, 15, 6)
    U0 = p['U0'].copy()
    U0[4] = 0.0
    idx, val = p['idx'], p['val']
    mine = idx[:, 0] == 4
    assert mine.sum() >= 2
    y, w = np.where(val[mine] > 0, 1.0, -1.0), (np.abs(val[mine]) if weighted else np.ones(mine.sum()))
    want = ((-y * w / 2)[:, None] * p['V0'][idx[mine, 1]].astype(np.float64)).sum(0)
    for dtype, tol in ((torch.float64, 1e-15), (torch.float32, 1e-6)):
        out, gU, _ = _get_loss(U0, p['V0'], idx, val, weighted, dtype)
        assert rel_err(gU[4], want) < tol
        assert rel_err(out[mine], w * np.log(2.0)) < tol
    assert rel_err(logistic_closed_form(U0, p['V0'], idx, val, weighted)[1][4], want) < 1e-15


@pytest.mark.parametrize('weighted', WEIGHTINGS, ids=['plain', 'weighted'])
def test_large_scores_stay_finite(weighted):
    p = logistic_problem(13, 30, 20, 4)
    scores = np.abs(np.einsum('kr,kr->k', p['U0'][p['idx'][:, 0]], p['V0'][p['idx'][:, 1]]))
    U0 = p['U0'] * np.float32(200.0 / scores.max())
    loss, gU, gV, loss_k = logistic_closed_form(U0, p['V0'], p['idx'], p['val'], weighted)
    out, aU, aV = _get_loss(U0, p['V0'], p['idx'], p['val'], weighted, torch.float32)
    big = np.abs(np.einsum('kr,kr->k', U0[p['idx'][:, 0]], p['V0'][p['idx'][:, 1]]))
    assert 199.0 < big.max() < 201.0 and (big > 88.7).sum() >= 5
    assert np.isfinite(out).all() and np.isfinite(aU).all() and np.isfinite(aV).all() and np.isfinite(loss)
    assert rel_err(out, loss_k) < 1e-5 and rel_err(aU, gU) < 1e-5 and rel_err(aV, gV) < 1e-5


def _model(p, weighted=False, loss=None, **attrs):
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import LogisticLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    model = MatrixFactorization(p['r'], loss_graph=loss or LogisticLoss(weighted), user_weight_graph=FixedInitializer(p['U0']),
                                item_weight_graph=FixedInitializer(p['V0']))
    model.verbose = False
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


@pytest.mark.parametrize('weighted', WEIGHTINGS, ids=['plain', 'weighted'])
def test_generic_fit_without_a_gpu_lowers_the_loss(monkeypatch, weighted):
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    p = logistic_problem(14, 30, 20, 5, zeros=True)
    model = _model(p, weighted)
    model.fit(5, eye(30), eye(20), SparseInteractions(p['idx'], p['val'], (30, 20)), lr=LR)
    h = model.loss_history_
    assert not hasattr(model, '_state') and len(h) == 5 and all(b < a for a, b in zip(h, h[1:])), h
    loss, gU, _, _ = logistic_closed_form(p['U0'], p['V0'], p['idx'], p['val'], weighted)
    assert rel_err(h[0], loss / p['idx'].shape[0]) < 1e-5          # loss_history_ is the mean over all stored interactions


# ------------------------------------------------------------------------------------------------------------------------
# dispatch, persistence
# ------------------------------------------------------------------------------------------------------------------------
def test_dispatch(monkeypatch):
    """LogisticLoss takes the engine exactly when there is a GPU - in every training form MSE has; a subclass keeps the generic
    path either way."""
    from teamoflow_amd.mf.embedding_graphs import ReLUEmbedding
    from teamoflow_amd.mf.loss_graphs import LogisticLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye

    class MyLogistic(LogisticLoss):
        pass
    p = logistic_problem(15, 12, 9, 4)
    inter = SparseInteractions(p['idx'], p['val'], (12, 9), device='cpu')
    forms = (('batch_users', 8), ('shard_items', 2), ('data_parallel', 'force'), ('factor_dtype', torch.bfloat16), ('optimizer', 'adam'))

    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    for loss in (LogisticLoss(), LogisticLoss(weighted=True)):
        assert _model(p, loss=loss)._route(eye(12), eye(9)) == 'engine'
        for name, value in forms:
            assert _model(p, loss=loss, **{name: value})._route(eye(12), eye(9)) == 'engine', name
    assert _model(p, loss=MyLogistic())._route(eye(12), eye(9)) == 'generic'
    assert _model(p)._route(torch.eye(12)[:, :5].contiguous(), eye(9)) == 'generic'          # dense features
    assert _model(p, user_repr_graph=ReLUEmbedding())._route(eye(12), eye(9)) == 'generic'
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for loss in (LogisticLoss(), LogisticLoss(weighted=True), MyLogistic()):
        assert _model(p, loss=loss)._route(eye(12), eye(9)) == 'generic'
    # and fit() itself, where it can run here: without a GPU everything goes to _fit_generic
    calls = []
    monkeypatch.setattr(MatrixFactorization, '_fit_sparse', lambda self, *a, **k: calls.append('engine') or True)
    monkeypatch.setattr(MatrixFactorization, '_fit_generic', lambda self, *a, **k: calls.append(type(self.loss_graph).__name__))
    for model in [_model(p), _model(p, weighted=True), _model(p, loss=MyLogistic())] + [_model(p, **{k: v}) for k, v in forms]:
        model.fit(1, eye(12), eye(9), inter, lr=LR)
    assert calls == ['LogisticLoss'] * 2 + ['MyLogistic'] + ['LogisticLoss'] * len(forms)


def test_loss_name_maps_the_built_ins_and_raises_on_anything_else():
    from teamoflow_amd import _engine
    from teamoflow_amd.mf import loss_graphs as LG

    class MyMSE(LG.MSELoss):
        pass

    class Foreign(LG.LossGraph):
        def get_loss(self, **kw):
            return None
    assert [_engine.loss_name(x) for x in (LG.MSELoss(), LG.WMRBLoss(), LG.KLDivergenceLoss(), LG.LogisticLoss(),
                                           LG.LogisticLoss(weighted=True))] == ['mse', 'wmrb', 'kl', 'logistic', 'logistic_w']
    for bad in (MyMSE(), Foreign(), None, 'mse'):
        with pytest.raises(TypeError):
            _engine.loss_name(bad)
    with pytest.raises(ValueError, match='unknown loss'):
        _engine.run_epoch(None, None, None, 'bpr')


def test_save_and_load_keep_the_weighting(tmp_path, monkeypatch):
    from teamoflow_amd.mf.loss_graphs import LogisticLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    p = logistic_problem(16, 12, 9, 4)
    for weighted in WEIGHTINGS:
        model = _model(p, weighted)
        model.fit(2, eye(12), eye(9), SparseInteractions(p['idx'], p['val'], (12, 9)), lr=LR)
        path = str(tmp_path / f'model_{int(weighted)}.pt')
        model.save(path)
        back = MatrixFactorization.load(path, device='cpu')
        assert type(back.loss_graph) is LogisticLoss and back.loss_graph.weighted is weighted
        assert back.loss_history_ == model.loss_history_ and torch.equal(back.user_embedding, model.user_embedding.detach())


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_built():
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    declared = set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    lib = _lib.load_library()
    for name in LOGISTIC_NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES['tmf_mse_pass_f32'][1]) + 1      # ... plus `weighted`
    make = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS :=.*\btmf_logistic\.hip\b', make, re.M)


def test_argument_checks_fail_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail differently (or crash); these return first."""
    from teamoflow_amd import _lib
    lib = _lib.load_library()
    adam = lib.tmf_adam_fresh(0.05)
    i64, i32 = (ctypes.c_int64 * 2)(0, 1), (ctypes.c_int32 * 1)(0)
    slab = (ctypes.c_int32 * 1)(-1)
    host = (ctypes.c_double * 8)()              # stands for any non-null table / list / buffer: never dereferenced
    H = ctypes.cast(host, ctypes.c_void_p)
    G, A, INVALID = _lib.EPI_GRAD, _lib.EPI_ADAM, -1

    def seg(nseg, chunk=1024):
        return ctypes.byref(_lib.Segments(ctypes.addressof(i64), ctypes.addressof(i32), ctypes.addressof(i32), ctypes.addressof(slab),
                                          nseg, chunk, 0))

    def failed(rc, word):
        return rc == INVALID and word in lib.tmf_last_error().decode()

    for name in LOGISTIC_NAMES:
        lg = getattr(lib, name)
        for wt in (0, 1):
            assert lg(seg(0), None, None, None, None, None, None, None, 24, 7, adam, wt, None) == 0     # nothing to do
            assert failed(lg(seg(1), H, H, None, H, H, H, H, 24, A, adam, wt, None), 'null table')      # X_old
            assert failed(lg(seg(1), H, H, H, None, H, H, H, 24, A, adam, wt, None), 'null table')      # Y_old
            assert failed(lg(seg(1), H, H, H, H, None, H, None, 24, G, adam, wt, None), 'null table')   # X_out
            assert failed(lg(seg(1), None, H, H, H, H, H, H, 24, G, adam, wt, None), 'entry list')
            assert failed(lg(seg(1), H, None, H, H, H, H, H, 24, G, adam, wt, None), 'entry list')
            for epi in (2, -1, 7):
                assert failed(lg(seg(1), H, H, H, H, H, H, H, 24, epi, adam, wt, None), f'bad epilogue {epi}')
            for r in (0, 2000, -3, 1025):
                assert failed(lg(seg(1), H, H, H, H, H, H, H, r, A, adam, wt, None), f'n_components {r}')
            assert failed(lg(None, H, H, H, H, H, H, H, 24, A, adam, wt, None), 'segments')
            assert failed(lg(seg(1, chunk=0), H, H, H, H, H, H, H, 24, A, adam, wt, None), 'segments')


# ------------------------------------------------------------------------------------------------------------------------
# the gather loop keeps its row loads in flight (tests/test_isa_guard.py)
# ------------------------------------------------------------------------------------------------------------------------
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_row_loads_stay_in_flight(tmp_path):
    asm = tmp_path / 'tmf_logistic.s'
    subprocess.run([HIPCC, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-ffp-contract=on', '-S', '--cuda-device-only',
                    os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'tmf_logistic.hip'), '-o', str(asm)], check=True, stderr=subprocess.DEVNULL)
    stats = _immediately_waited(asm.read_text())
    name, found = 'k_logistic_pass', 0
    for sym, (loads, waited) in stats.items():
        if f'_ZN3tmf{len(name)}{name}I' not in sym or 'ILi1E' in sym:     # the single-lane geometries: their rows are one load
            continue
        found += 1
        if any(f'{name}ILi{g}E' in sym for g in (16, 32, 64)):
            assert loads >= 4, f'{sym}: only {loads} row loads found - is this still the gather kernel?'
        assert waited <= 1, f'{sym}: {waited} of {loads} row loads are waited for immediately (serialised gathers)'
    # fp32 and bf16, with and without the loss, 8 + 7 multi-lane geometries
    assert found == 2 * (8 + 7), found
