"""LogisticLoss on the sparse HIP engine (tmf_logistic_pass_*, _engine.epoch_logistic) against the NumPy fp64 closed form of
tests/test_logistic_cpu.py, which that file pins to the plug-in's own get_loss and whose fp32 form it shows to meet the
tolerances used here: rel_err < 1e-5 for the loss and the raw gradients, assert_step(rtol=1e-5) for the tables after one step."""
import gc
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_step, rel_err, step_bounds
from test_biased_cpu import LR, assert_bias_step
from test_features_cpu import featured_problem
from test_logistic_cpu import WEIGHTINGS, logistic_closed_form, logistic_problem

pytestmark = pytest.mark.gpu
IDS = ['plain', 'weighted']


@pytest.fixture(scope='module')
def tm():
    from teamoflow_amd import _engine, _lib
    from teamoflow_amd.mf import embedding_graphs as EG
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import LogisticLoss, MSELoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseFeatures, SparseInteractions, eye
    lib = _lib.get()

    class NS:
        pass
    ns = NS()
    ns.lib, ns.L, ns.E, ns.EG, ns.MF, ns.Fixed, ns.Logistic, ns.MSE, ns.Sparse, ns.SF, ns.eye = lib, _lib, _engine, EG, \
        MatrixFactorization, FixedInitializer, LogisticLoss, MSELoss, SparseInteractions, SparseFeatures, eye
    return ns


@pytest.fixture
def engine_only(tm, monkeypatch):
    """_fit_generic refuses to run: a fit that passes ran on the engine."""
    def refuse(self, *a, **k):
        raise AssertionError('_fit_generic was called')
    monkeypatch.setattr(tm.MF, '_fit_generic', refuse)


def fit_logistic(tm, U0, V0, idx, val, epochs, weighted=False, lr=LR, user_features=None, item_features=None, loss=None, **attrs):
    m, n = (U0.shape[0] if user_features is None else user_features.shape[0]), (V0.shape[0] if item_features is None else item_features.shape[0])
    graphs = {k: attrs.pop(k) for k in ('user_repr_graph', 'item_repr_graph') if k in attrs}
    model = tm.MF(U0.shape[1], loss_graph=loss or tm.Logistic(weighted), user_weight_graph=tm.Fixed(U0), item_weight_graph=tm.Fixed(V0),
                  **graphs)
    model.verbose = False
    for k, v in attrs.items():
        setattr(model, k, v)
    model.fit(epochs, tm.eye(m) if user_features is None else user_features, tm.eye(n) if item_features is None else item_features,
              tm.Sparse(idx, val, (m, n)), lr=lr)
    return model


def host(t):
    return t.detach().float().cpu().numpy()


def tables(model):
    return host(model.user_embedding), host(model.item_embedding)


def check_one_step(tm, U0, V0, idx, val, weighted=False, what='', **attrs):
    model = fit_logistic(tm, U0, V0, idx, val, 1, weighted, **attrs)
    loss, gU, gV, _ = logistic_closed_form(U0, V0, idx, val, weighted)
    assert hasattr(model, '_state'), 'the fit did not run on the engine'
    assert rel_err(model.loss_history_[0], loss / idx.shape[0]) < 1e-5, what      # the mean over all stored interactions
    U1, V1 = tables(model)
    assert_step(U1, U0, gU, LR, rtol=1e-5, what=f'{what} U')
    assert_step(V1, V0, gV, LR, rtol=1e-5, what=f'{what} V')
    return model


# ------------------------------------------------------------------------------------------------------------------------
# one step against the closed form
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [1, 3, 7, 16, 33, 64, 100, 128, 200, 256, 300, 512])
def test_every_row_geometry_one_step(tm, engine_only, r):
    p = logistic_problem(r, 60, 40, r)
    check_one_step(tm, p['U0'], p['V0'], p['idx'], p['val'], what=f'r={r}')


@pytest.mark.parametrize('r', [3, 33, 128])
@pytest.mark.parametrize('weighted', WEIGHTINGS, ids=IDS)
def test_both_weightings_one_step(tm, engine_only, weighted, r):
    p = logistic_problem(500 + r, 60, 40, r, zeros=True)
    check_one_step(tm, p['U0'], p['V0'], p['idx'], p['val'], weighted, what=f'r={r} weighted={weighted}')


def raw_pass(tm, U0, V0, idx, val, weighted, r):
    """Both kernels through the C ABI with TMF_EPI_GRAD: (gU, gV, loss sum) as NumPy."""
    L, lib = tm.L, tm.lib
    dev = torch.device('cuda')
    plan = tm.E.InteractionPlan(torch.as_tensor(idx, device=dev), torch.as_tensor(val, device=dev), U0.shape[0], V0.shape[0])
    st = tm.E.TrainState(U0, V0, plan, r)
    s, P, adam = L.stream_ptr(), L.ptr, tm.E.adam_constants(LR)
    gU, gV = torch.full_like(st.U, float('nan')), torch.full_like(st.V, float('nan'))
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    L.check(lib.tmf_logistic_pass_f32(plan.seg_u.cstruct(), P(plan.col_u), P(plan.val_u), P(st.U), P(st.V), P(gU), P(st.slab),
                                      P(st.loss_part), r, L.EPI_GRAD, adam, int(weighted), s), lib)
    tm.E._row_pass_finish(lib, plan.seg_u, st.slab, st.U, gU, r, L.EPI_GRAD, adam, s)
    L.check(lib.tmf_sum_f32(P(st.loss_part), plan.seg_u.nseg, P(loss), s), lib)
    L.check(lib.tmf_logistic_pass_f32(plan.seg_i.cstruct(), P(plan.row_i), P(plan.val_i), P(st.V), P(st.U), P(gV), P(st.slab),
                                      None, r, L.EPI_GRAD, adam, int(weighted), s), lib)
    tm.E._row_pass_finish(lib, plan.seg_i, st.slab, st.V, gV, r, L.EPI_GRAD, adam, s)
    assert not gU[:, r:].any() and not gV[:, r:].any()        # the padding columns of a gradient row are zeros
    return gU[:, :r].cpu().numpy(), gV[:, :r].cpu().numpy(), float(loss)


@pytest.mark.parametrize('weighted', WEIGHTINGS, ids=IDS)
def test_raw_gradients_and_loss_through_the_c_abi(tm, weighted):
    r = 24
    p = logistic_problem(24, 60, 40, r, zeros=True)
    gU, gV, loss = raw_pass(tm, p['U0'], p['V0'], p['idx'], p['val'], weighted, r)
    ref = logistic_closed_form(p['U0'], p['V0'], p['idx'], p['val'], weighted)
    errs = rel_err(loss, ref[0]), rel_err(gU, ref[1]), rel_err(gV, ref[2])
    print(f'[raw] weighted={weighted}: loss {errs[0]:.3g} gU {errs[1]:.3g} gV {errs[2]:.3g}')
    assert max(errs) < 1e-5, errs
    assert not gU[p['empty_user']].any() and not gV[p['empty_item']].any()


@pytest.mark.parametrize('weighted', WEIGHTINGS, ids=IDS)
def test_scores_from_zero_to_150_stay_finite(tm, weighted):
    """The user table scaled until the largest |p| is 150 - exp overflows beyond 88.7 if taken of the wrong sign, the tail of
    sigma underflows - and one user row set to zero: p = 0 exactly, the coefficient -y w / 2."""
    r = 24
    p = logistic_problem(25, 60, 40, r)
    idx, val, V0 = p['idx'], p['val'], p['V0']
    scores = np.abs(np.einsum('kr,kr->k', p['U0'][idx[:, 0]].astype(np.float64), V0[idx[:, 1]].astype(np.float64)))
    U0 = (p['U0'] * np.float32(150.0 / scores.max())).astype(np.float32)
    U0[7] = 0.0
    big = np.abs(np.einsum('kr,kr->k', U0[idx[:, 0]].astype(np.float64), V0[idx[:, 1]].astype(np.float64)))
    assert 149.0 < big.max() < 151.0 and (big > 88.7).sum() >= 5 and (big == 0).sum() >= 2 and ((big > 0) & (big < 1)).any()
    gU, gV, loss = raw_pass(tm, U0, V0, idx, val, weighted, r)
    assert np.isfinite(gU).all() and np.isfinite(gV).all() and np.isfinite(loss)
    ref = logistic_closed_form(U0, V0, idx, val, weighted)
    errs = rel_err(loss, ref[0]), rel_err(gU, ref[1]), rel_err(gV, ref[2])
    print(f'[raw, |p| <= 150] weighted={weighted}: loss {errs[0]:.3g} gU {errs[1]:.3g} gV {errs[2]:.3g}')
    assert max(errs) < 1e-5, errs
    mine = idx[:, 0] == 7
    y, w = np.where(val[mine] > 0, 1.0, -1.0), (np.abs(val[mine]) if weighted else np.ones(int(mine.sum())))
    assert rel_err(gU[7], ((-y * w / 2)[:, None] * V0[idx[mine, 1]].astype(np.float64)).sum(0)) < 1e-6


def test_a_single_entry_at_score_zero_gives_exactly_half(tm):
    """One entry per user against a zero user table: gU[u] = -y w / 2 V[j] to the bit (0.5 and the weights 1..5 are exact)."""
    r, n = 24, 9
    rng = np.random.default_rng(3)
    V0 = (rng.standard_normal((n, r)) * 0.3).astype(np.float32)
    U0 = np.zeros((n, r), np.float32)
    idx = np.stack([np.arange(n), rng.permutation(n)], 1)
    val = np.array([1, -2, 3, -4, 5, -1, 2, 0, 4], np.float32)
    for weighted in WEIGHTINGS:
        gU, gV, loss = raw_pass(tm, U0, V0, idx, val, weighted, r)
        y, w = np.where(val > 0, np.float32(1), np.float32(-1)), (np.abs(val) if weighted else np.ones(n, np.float32))
        assert np.array_equal(gU, (-y * w / 2)[:, None] * V0[idx[:, 1]])
        assert not gV.any()                                   # c U[u] with U = 0
        assert rel_err(loss, float(w.sum()) * np.log(2.0)) < 1e-6


# ------------------------------------------------------------------------------------------------------------------------
# segment paths (the shapes of tests/test_gpu_kl.py)
# ------------------------------------------------------------------------------------------------------------------------
def test_rows_cut_into_segments(tm, engine_only):
    """User 0 stores all 5000 items (5 segments of 1024), user 1 exactly 1024 (one full segment), user 2 1025 (two): the partial
    rows of users 0 and 2 go through the slab and tmf_combine_rows."""
    rng = np.random.default_rng(5)
    m, n, r = 6, 5000, 32
    rows = [np.arange(n), rng.choice(n, 1024, replace=False), rng.choice(n, 1025, replace=False), rng.choice(n, 40, replace=False),
            rng.choice(n, 3, replace=False), np.arange(0)]
    idx = np.concatenate([np.stack([np.full(c.size, u), np.sort(c)], 1) for u, c in enumerate(rows)])
    val = rng.integers(-5, 6, idx.shape[0]).astype(np.float32)
    U0 = (rng.standard_normal((m, r)) * 0.3).astype(np.float32)
    V0 = (rng.standard_normal((n, r)) * 0.3).astype(np.float32)
    for weighted in WEIGHTINGS:
        model = check_one_step(tm, U0, V0, idx, val, weighted, 'segmented')
        assert model._state.plan.seg_u.n_long == 2 and model._state.plan.seg_u.nseg == 5 + 1 + 2 + 3


def test_thousands_of_workgroups_and_long_item_lists(tm, engine_only):
    """4500 users of 1-3 entries over 7 items: thousands of workgroups, and every item list cut into segments."""
    rng = np.random.default_rng(11)
    m, n, r = 4500, 7, 3
    deg = rng.integers(1, 4, m)
    idx = np.concatenate([np.stack([np.full(d, u), np.sort(rng.choice(n, d, replace=False))], 1) for u, d in enumerate(deg)])
    val = rng.integers(-5, 6, idx.shape[0]).astype(np.float32)
    U0 = (rng.standard_normal((m, r)) * 0.3).astype(np.float32)
    V0 = (rng.standard_normal((n, r)) * 0.3).astype(np.float32)
    model = check_one_step(tm, U0, V0, idx, val, True, 'many segments')
    assert model._state.plan.seg_u.nseg == m and model._state.plan.seg_i.n_long == n


def test_user_blocked_item_lists(tm, engine_only, monkeypatch):
    monkeypatch.setenv('TMF_USER_CHUNKS', '4')
    p = logistic_problem(32, 60, 40, 32, zeros=True)
    model = check_one_step(tm, p['U0'], p['V0'], p['idx'], p['val'], True, 'TMF_USER_CHUNKS=4')
    assert model._state.plan.seg_i.row_mod == 40 and model._state.plan.user_chunks == 4


# ------------------------------------------------------------------------------------------------------------------------
# structure
# ------------------------------------------------------------------------------------------------------------------------
def test_untouched_rows_and_input_order(tm, engine_only):
    p = logistic_problem(4, 60, 40, 12)
    idx, val, U0, V0 = p['idx'], p['val'], p['U0'], p['V0']
    U1, V1 = tables(check_one_step(tm, U0, V0, idx, val, what='empty rows'))
    assert np.array_equal(U1[p['empty_user']], U0[p['empty_user']]) and np.array_equal(V1[p['empty_item']], V0[p['empty_item']])
    # a shuffled list with duplicate pairs: every stored entry counts on its own
    rng = np.random.default_rng(9)
    dup = rng.choice(idx.shape[0], 60, replace=False)
    idx2 = np.concatenate([idx, idx[dup]])
    val2 = np.concatenate([val, rng.integers(-5, 6, 60).astype(np.float32)])
    order = rng.permutation(idx2.shape[0])
    for weighted in WEIGHTINGS:
        check_one_step(tm, U0, V0, idx2[order], val2[order], weighted, 'shuffled with duplicates')


def test_a_stored_zero_is_a_negative(tm, engine_only):
    """The only entry of a user and of an item is a stored 0: weight 0 under weighted=True (both rows keep their bits), a
    negative of weight 1 otherwise (both rows move as the closed form says)."""
    p = logistic_problem(6, 60, 40, 12)
    eu, ei = p['empty_user'], p['empty_item']
    idx = np.concatenate([p['idx'], [[eu, ei]]])
    val = np.concatenate([p['val'], [0.0]]).astype(np.float32)
    U0, V0 = p['U0'], p['V0']
    U1, V1 = tables(check_one_step(tm, U0, V0, idx, val, True, 'stored zero, weighted'))
    assert np.array_equal(U1[eu], U0[eu]) and np.array_equal(V1[ei], V0[ei])
    U1, V1 = tables(check_one_step(tm, U0, V0, idx, val, False, 'stored zero, plain'))
    # d loss / d p = +sigma(p) > 0: the rows move against each other's direction by about lr per element
    assert np.abs(U1[eu] - U0[eu]).min() > 0.5 * LR and np.array_equal(np.sign(U0[eu] - U1[eu]), np.sign(V0[ei]))
    assert np.abs(V1[ei] - V0[ei]).min() > 0.5 * LR and np.array_equal(np.sign(V0[ei] - V1[ei]), np.sign(U0[eu]))


def test_all_positive_table(tm, engine_only):
    p = logistic_problem(8, 60, 40, 7)
    check_one_step(tm, p['U0'], p['V0'], p['idx'], np.abs(p['val']), True, 'all positive')


# ------------------------------------------------------------------------------------------------------------------------
# storage, trajectory, replay, optimiser
# ------------------------------------------------------------------------------------------------------------------------
def _bf16(x):
    return torch.tensor(np.asarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


@pytest.mark.parametrize('r', [8, 33, 128])
def test_bf16_storage_one_step(tm, engine_only, r):
    """bf16 factor storage / fp32 arithmetic: against the closed form on the bf16-rounded tables; the new rows must lie in the
    step interval rounded to bf16 (tests/test_gpu_kl.py::test_bf16_storage_one_step)."""
    p = logistic_problem(100 + r, 60, 40, r, zeros=True)
    idx, val, U0, V0 = p['idx'], p['val'], _bf16(p['U0']), _bf16(p['V0'])
    for weighted in WEIGHTINGS:
        model = fit_logistic(tm, U0, V0, idx, val, 1, weighted, factor_dtype=torch.bfloat16)
        assert model.user_embedding.dtype == torch.bfloat16 and hasattr(model, '_state')
        loss, gU, gV, _ = logistic_closed_form(U0, V0, idx, val, weighted)
        assert rel_err(model.loss_history_[0], loss / idx.shape[0]) < 1e-5
        for got, W0, g in zip(tables(model), (U0, V0), (gU, gV)):
            lo, hi = step_bounds(W0, g, LR)
            got = got.astype(np.float64)
            assert (got >= _bf16(lo) - 1e-12).all() and (got <= _bf16(hi) + 1e-12).all(), r


def fresh_adam_fp64(W, g, lr):
    """conftest.step_bounds' step: the reference's first Adam step with its fp32 constants, evaluated in fp64."""
    f = np.float32
    omb1, omb2, eps = float(f(1) - f(0.9)), float(f(1) - f(0.999)), float(f(1e-7))
    alpha = float(f(f(lr) * np.sqrt(f(f(1) - f(0.999))) / f(f(1) - f(0.9))))
    return W - (g * omb1 * alpha) / (np.sqrt(g * g * omb2) + eps)


def closed_form_trajectory(U0, V0, idx, val, weighted, epochs, lr):
    U, V, out = U0.astype(np.float64), V0.astype(np.float64), []
    for _ in range(epochs):
        loss, gU, gV, _ = logistic_closed_form(U, V, idx, val, weighted)
        out.append(loss / idx.shape[0])
        U, V = fresh_adam_fp64(U, gU, lr), fresh_adam_fp64(V, gV, lr)
    return out


@pytest.mark.parametrize('weighted', WEIGHTINGS, ids=IDS)
def test_trajectory(tm, engine_only, weighted):
    p = logistic_problem(6, 70, 45, 5, zeros=True)
    model = fit_logistic(tm, p['U0'], p['V0'], p['idx'], p['val'], 12, weighted)
    ref = closed_form_trajectory(p['U0'], p['V0'], p['idx'], p['val'], weighted, 12, LR)
    h = model.loss_history_
    print(f'[trajectory] weighted={weighted}: first three {rel_err(h[:3], ref[:3]):.3g}, all {rel_err(h, ref):.3g}')
    assert rel_err(h[:3], ref[:3]) < 1e-5 and rel_err(h, ref) < 1e-3   # near-sign Adam steps amplify rounding over the epochs
    assert h[-1] < h[0]


def test_graph_replay_equals_eager_and_fits_repeat(tm, engine_only, monkeypatch):
    p = logistic_problem(7, 60, 40, 12, zeros=True)
    args = (p['U0'], p['V0'], p['idx'], p['val'])
    for epochs in (10, 13):                               # 10 = one replay; 13 = one replay of 12 and an eager epoch
        monkeypatch.delenv('TMF_NO_GRAPH', raising=False)
        a, b = fit_logistic(tm, *args, epochs, True), fit_logistic(tm, *args, epochs, True)
        monkeypatch.setenv('TMF_NO_GRAPH', '1')
        c = fit_logistic(tm, *args, epochs, True)
        for other in (b, c):
            assert a.loss_history_ == other.loss_history_ and len(a.loss_history_) == epochs
            assert torch.equal(a.user_embedding, other.user_embedding) and torch.equal(a.item_embedding, other.item_embedding)
        assert np.isfinite(a.loss_history_).all()


def test_opt_in_persistent_adam(tm, engine_only):
    """optimizer='adam': the first step is the default's bit for bit; later steps follow Keras Adam with carried moments,
    evaluated in NumPy on the closed-form gradients (tests/test_gpu_kl.py's statement and tolerance)."""
    p = logistic_problem(8, 60, 40, 12)
    args = (p['U0'], p['V0'], p['idx'], p['val'])
    a1, f1 = fit_logistic(tm, *args, 1, optimizer='adam'), fit_logistic(tm, *args, 1)
    assert torch.equal(a1.user_embedding, f1.user_embedding) and torch.equal(a1.item_embedding, f1.item_embedding)
    assert a1.loss_history_ == f1.loss_history_
    got = fit_logistic(tm, *args, 5, optimizer='adam')
    U, V = p['U0'].astype(np.float64), p['V0'].astype(np.float64)
    mU, vU, mV, vV = (np.zeros_like(x) for x in (U, U, V, V))
    ref = []
    for t in range(1, 6):
        loss, gU, gV, _ = logistic_closed_form(U, V, p['idx'], p['val'], False)
        ref.append(loss / p['idx'].shape[0])
        alpha = LR * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        mU += (gU - mU) * 0.1
        vU += (gU ** 2 - vU) * 0.001
        mV += (gV - mV) * 0.1
        vV += (gV ** 2 - vV) * 0.001
        U = U - alpha * mU / (np.sqrt(vU) + 1e-7)
        V = V - alpha * mV / (np.sqrt(vV) + 1e-7)
    assert rel_err(got.loss_history_, ref) < 1e-4
    assert np.abs(host(got.user_embedding) - U).max() < 1e-3 and np.abs(host(got.item_embedding) - V).max() < 1e-3


# ------------------------------------------------------------------------------------------------------------------------
# sides: a biased side, a side over SparseFeatures (the closed form composed with the side's own rule)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weighted', WEIGHTINGS, ids=IDS)
@pytest.mark.parametrize('sides', [('biased', 'linear'), ('linear', 'biased'), ('biased', 'biased')], ids='-'.join)
def test_biased_sides_one_step(tm, engine_only, sides, weighted):
    """A bias starts at zero, so the effective tables are the weights: their gradient is the closed form's, and the bias gradient
    its column sum (tests/test_biased_cpu.py: compared with the slack a column sum inherits from its summands)."""
    r = 33
    p = logistic_problem(1000 + r, 60, 40, r, zeros=True)
    graph = {'biased': tm.EG.BiasedLinearEmbedding, 'linear': tm.EG.LinearEmbedding}
    model = fit_logistic(tm, p['U0'], p['V0'], p['idx'], p['val'], 1, weighted, user_repr_graph=graph[sides[0]](),
                         item_repr_graph=graph[sides[1]]())
    loss, gU, gV, _ = logistic_closed_form(p['U0'], p['V0'], p['idx'], p['val'], weighted)
    what = f'{sides} weighted={weighted}'
    assert hasattr(model, '_state') and (model._state.bias_u is not None) == (sides[0] == 'biased')
    assert (model._state.bias_v is not None) == (sides[1] == 'biased')
    assert rel_err(model.loss_history_[0], loss / p['idx'].shape[0]) < 1e-5
    zero = np.zeros((1, r))
    for side, kind, W0, got, emb, kept, G in (('user', sides[0], p['U0'], model.user_trainable, model.user_embedding, model.user_linear_bias, gU),
                                              ('item', sides[1], p['V0'], model.item_trainable, model.item_embedding, model.item_linear_bias, gV)):
        assert_step(host(got[0]), W0, G, LR, rtol=1e-5, what=f'{what} {side} weights')
        if kind == 'biased':
            assert len(got) == 2 and got[1] is kept
            assert_bias_step(host(kept), zero, G.sum(0, keepdims=True), G, LR, f'logistic {what} {side} bias')
            assert torch.equal(emb, got[0] + kept.detach())
        else:
            assert len(got) == 1 and kept is None and torch.equal(emb, got[0])


@pytest.mark.parametrize('weighted', WEIGHTINGS, ids=IDS)
def test_user_side_over_sparse_features_one_step(tm, engine_only, weighted):
    """F = [I | tags] (hstack_identity's layout): E = F W, dL/dW = F^T dL/dE with dL/dE the closed form on (E, V); every row's
    gradient agrees to 1e-5, so feature f's sum may be off by 1e-5 sum_i |x_if| |dL/dE[i]| (tests/test_gpu_features.py)."""
    from test_gpu_features import assert_step_with_slack
    from teamoflow_amd.mf.sparse import hstack_identity
    m, n, r = 60, 40, 33
    p = featured_problem(2000 + r, m, n, r, 'kl', 'hybrid')
    idx_f, val_f, shape_f = p['Fu']
    tags = idx_f[:, 1] >= m
    F = hstack_identity(m, tm.SF(idx_f[tags] - np.array([0, m]), val_f[tags], (m, shape_f[1] - m)))
    assert torch.equal(F.to_dense().cpu(), torch.tensor(p['Fu_dense'], dtype=torch.float32))
    model = fit_logistic(tm, p['Wu0'], p['V0'], p['idx'], p['val'], 1, weighted, user_features=F)
    E0 = p['Fu_dense'] @ p['Wu0'].astype(np.float64)
    loss, gE, gV, _ = logistic_closed_form(E0, p['V0'], p['idx'], p['val'], weighted)
    assert hasattr(model, '_state') and model._state.feat_u is not None and model._state.feat_v is None
    assert rel_err(model.loss_history_[0], loss / p['idx'].shape[0]) < 1e-5
    assert_step(host(model.item_embedding), p['V0'], gV, LR, rtol=1e-5, what='item table')
    slack = 1e-5 * np.abs(p['Fu_dense']).T @ np.abs(gE)
    assert_step_with_slack(host(model.user_trainable[0]), p['Wu0'], p['Fu_dense'].T @ gE, slack, LR, f'logistic weighted={weighted} user weights')
    assert model.user_embedding.shape == (m, r) and torch.equal(model.user_embedding, model.embed_users(F))


# ------------------------------------------------------------------------------------------------------------------------
# the other training forms
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weighted', WEIGHTINGS, ids=IDS)
def test_minibatch_over_user_batches(tm, engine_only, weighted):
    """batch_users = 8 on 30 x 20 (batches of 8, 8, 8, 6 users): every batch is the closed-form epoch of its sub-problem, the next
    batch sees the updated item table (tests/test_gpu_generic.py::test_minibatch_over_user_batches, its criteria)."""
    m, n, r, B, epochs = 30, 20, 5, 8, 2
    p = logistic_problem(21, m, n, r, zeros=True)
    idx, val = p['idx'], p['val']
    model = fit_logistic(tm, p['U0'], p['V0'], idx, val, epochs, weighted, batch_users=B)
    U, V, ref = p['U0'].astype(np.float64), p['V0'].astype(np.float64), []
    for _ in range(epochs):
        tot = 0.0
        for b0 in range(0, m, B):
            keep = (idx[:, 0] >= b0) & (idx[:, 0] < b0 + B)
            sub = idx[keep] - np.array([b0, 0])
            loss, gU, gV, _ = logistic_closed_form(U[b0:b0 + B], V, sub, val[keep], weighted)
            U[b0:b0 + B], V = fresh_adam_fp64(U[b0:b0 + B], gU, LR), fresh_adam_fp64(V, gV, LR)
            tot += loss
        ref.append(tot / idx.shape[0])
    assert isinstance(model._state, list) and len(model._state) == 4
    assert rel_err(model.loss_history_[:1], ref[:1]) < 1e-5 and rel_err(model.loss_history_, ref) < 2e-5
    dU, dV = np.abs(host(model.user_embedding) - U), np.abs(host(model.item_embedding) - V)
    assert (dU < 1e-4).mean() > 0.98 and dU.max() <= 2 * epochs * LR      # near-sign steps: elements with g ~ 0 may differ by a step
    assert (dV < 1e-4).mean() > 0.95 and dV.max() <= 2 * epochs * 4 * LR


def test_item_sharded_on_one_rank_follows_the_resident_fit(tm, engine_only):
    m, n, r = 157, 203, 16
    p = logistic_problem(12, m, n, r, zeros=True)
    args = (p['U0'], p['V0'], p['idx'], p['val'])
    for weighted in WEIGHTINGS:
        a, b = fit_logistic(tm, *args, 3, weighted, shard_items=2), fit_logistic(tm, *args, 3, weighted)
        assert a._state.T == 2 and a._state.loss == ('logistic_w' if weighted else 'logistic')
        assert rel_err(a.loss_history_, b.loss_history_) < 1e-5
        ref = closed_form_trajectory(*args, weighted, 1, LR)
        assert rel_err(a.loss_history_[:1], ref) < 1e-5


@pytest.mark.parametrize('q', [0, 1], ids=['data_parallel', 'item_sharded'])
def test_two_ranks_on_one_card(tmp_path, q):
    """Two ranks on cuda:0 (gloo group, host-staged collectives - tools/dp_rehearsal.py logistic), data-parallel and item-sharded
    with one window per rank, against the single-process resident fit: the assertions of
    tests/test_gpu_sharded.py::test_two_ranks_item_sharded_on_one_card."""
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    out = tmp_path / 'ranks.json'
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, 'tools', 'dp_rehearsal.py'), str(out), 'logistic'] + ([str(q)] if q else []),
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), '\n'.join(logs)
    res = json.loads(out.read_text())
    blocks = res['blocks']
    assert res['loss'] == 'logistic' and res['signed_values'] is True
    assert blocks[0][0] == 0 and blocks[-1][1] == 3001 and all(a[1] == b[0] for a, b in zip(blocks, blocks[1:])) and all(b0 < b1 for b0, b1 in blocks)
    if q:
        assert res['item_rows_partition_the_catalog'] and all(0 < c < 701 for c in res['item_rows_per_rank'])   # split, nobody owns all
        assert res['sharded_top10_equals_resident'] is True
    assert abs(res['loss_dp'][0] - res['loss_one'][0]) <= 1e-6 * abs(res['loss_one'][0])
    assert rel_err(res['loss_dp'], res['loss_one']) < 1e-5
    assert abs(res['recall_all_ranks'] - res['recall_assembled_tables']) <= 1e-12 and 0 < res['recall_all_ranks'] < 1
    assert res['U1_frac_close'] > 0.99 and res['U1_max_abs_diff'] <= 2.0 * 0.05 + 1e-6
    assert res['V1_frac_close'] > 0.99 and res['V1_max_abs_diff'] <= 2.0 * 0.05 + 1e-6


# ------------------------------------------------------------------------------------------------------------------------
# scale: no dense table anywhere
# ------------------------------------------------------------------------------------------------------------------------
def test_large_fit_allocates_what_the_mse_fit_allocates(tm, engine_only):
    """200 000 users x 2 000 items, r = 32, 2e6 signed interactions, 2 epochs: the peak of allocated memory is the MSE fit's of the
    same shape (tables + plans; + 10 %), far below the 1.6 GB of one [m, n] fp32 tensor."""
    m, n, r, per_user = 200_000, 2_000, 32, 10
    rng = np.random.default_rng(0)
    users = np.repeat(np.arange(m), per_user)
    items = (users * 7 + np.tile(np.arange(per_user), m) * 199) % n       # ten distinct items per user
    idx = np.stack([users, items], 1)
    val = (rng.integers(1, 6, idx.shape[0]) * rng.choice(np.array([-1, 1]), idx.shape[0])).astype(np.float32)
    U0, V0 = (rng.standard_normal((m, r)) * 0.3).astype(np.float32), (rng.standard_normal((n, r)) * 0.3).astype(np.float32)

    def peak_of(loss):
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        model = fit_logistic(tm, U0, V0, idx, val, 2, loss=loss)
        peak = torch.cuda.max_memory_allocated() - base
        assert hasattr(model, '_state') and model.user_embedding.shape == (m, r)
        h = model.loss_history_
        del model
        return peak, h
    peak_mse, _ = peak_of(tm.MSE())
    peak, h = peak_of(tm.Logistic(weighted=True))
    print(f'[scale] peak allocated: logistic {peak / 1e6:.0f} MB, mse {peak_mse / 1e6:.0f} MB')
    assert peak <= 1.1 * peak_mse and peak < m * n * 4 / 2
    assert len(h) == 2 and h[1] < h[0]
