"""CPU side of BPRLoss (no GPU): the NumPy fp64 closed form the GPU tests compare the engine with, the problem generators both files
use, the statement the GPU tolerances rest on (the same sums in fp32, in the order tmf_bpr_pairs adds them, against fp64 on the GPU
file's own inputs), the plug-in's get_loss, a fit through the generic loop, the dispatch and its refusals, save / load, and the C ABI
of tmf_bpr_pairs (declared, bound, built)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_step, rel_err

LR = 0.05
BPR_CHUNK, BPR_ROUND, BPR_TILE = 64, 32, 512    # csrc/tmf_bpr.hip: BCHUNK, BROUND, BTILE


# ------------------------------------------------------------------------------------------------------------------------
# the reference: shares no code with the package
# ------------------------------------------------------------------------------------------------------------------------
def bpr_pairs_ref(rowptr, val, p, sp):
    """tmf_bpr_pairs in fp64 on given scores: (delta [nnz], D [m, S], loss_part [m]).  sigma and softplus from e = exp(-|x|)."""
    rowptr, val = np.asarray(rowptr, np.int64), np.asarray(val, np.float64)
    p, sp = np.asarray(p, np.float64), np.asarray(sp, np.float64)
    m, S = sp.shape
    delta, D, loss = np.zeros(val.shape[0]), np.zeros((m, S)), np.zeros(m)
    with np.errstate(invalid='ignore', over='ignore'):
        for u in range(m):
            ks = np.arange(rowptr[u], rowptr[u + 1])
            ks = ks[val[ks] > 0]
            if not ks.size:
                continue
            x = sp[u][None, :] - p[ks][:, None]
            e = np.exp(-np.abs(x))
            sig = np.where(x >= 0, 1.0, e) / (1.0 + e)
            soft = np.maximum(x, 0.0) + np.log1p(e)
            delta[ks] = -sig.sum(1) / S
            D[u] = sig.sum(0) / S
            loss[u] = soft.sum() / S
    return delta, D, loss


def bpr_closed_form(U0, V0, idx, val, R):
    """One BPRLoss epoch in fp64.  idx: row-major (user, item) pairs (the CSR order), R [m, S] the negative table.
    -> (loss sum over the positives, delta [nnz], D [m, S] in R's order, gU, gV)."""
    U, V = np.asarray(U0, np.float64), np.asarray(V0, np.float64)
    idx, R = np.asarray(idx, np.int64), np.asarray(R, np.int64)
    m, S = R.shape
    u, i = idx[:, 0], idx[:, 1]
    assert (np.diff(u * V.shape[0] + i) >= 0).all(), 'row-major pairs'
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=m))])
    p = np.einsum('kr,kr->k', U[u], V[i])
    sp = np.einsum('ur,usr->us', U, V[R])
    delta, D, loss = bpr_pairs_ref(rowptr, val, p, sp)
    gU = np.einsum('us,usr->ur', D, V[R])
    np.add.at(gU, u, delta[:, None] * V[i])
    gV = np.zeros_like(V)
    np.add.at(gV, R.reshape(-1), (D[:, :, None] * U[:, None, :]).reshape(m * S, -1))
    np.add.at(gV, i, delta[:, None] * U[u])
    return loss.sum(), delta, D, gU, gV


def bpr_problem(seed, m, n, r, S, density=0.3):
    """Row-major COO pairs without duplicates; values from {-2, -1, 0, 1 .. 5}; user ``empty_user`` stores nothing, user
    ``nonpos_user`` only values <= 0; item ``empty_item`` is stored by nobody; an [m, S] negative table whose first column is one of
    the user's positives where it has one (negatives that coincide with positives are not filtered); tables ~ N(0, 0.3^2)."""
    rng = np.random.default_rng(seed)
    mask = rng.random((m, n)) < density
    empty_user, nonpos_user, empty_item = m // 3, m // 2, n // 2
    mask[empty_user, :] = False
    mask[:, empty_item] = False
    idx = np.argwhere(mask)
    val = rng.choice(np.array([-2, -1, 0, 1, 2, 3, 4, 5], np.float32), idx.shape[0], p=[.06, .06, .08, .16, .16, .16, .16, .16])
    val[idx[:, 0] == nonpos_user] = -np.abs(val[idx[:, 0] == nonpos_user])
    R = rng.integers(0, n, (m, S))
    R[R == empty_item] = (empty_item + 1) % n      # the empty item's row moves only if somebody samples it: keep it still
    hits = 0
    for u in range(m):
        mine = idx[(idx[:, 0] == u) & (val > 0), 1]
        if mine.size:
            R[u, 0] = mine[rng.integers(mine.size)]
            hits += 1
    U0 = (rng.standard_normal((m, r)) * 0.3).astype(np.float32)
    V0 = (rng.standard_normal((n, r)) * 0.3).astype(np.float32)
    return dict(idx=idx, val=val, U0=U0, V0=V0, R=R.astype(np.int32), S=S, m=m, n=n, r=r, empty_user=empty_user, nonpos_user=nonpos_user,
                empty_item=empty_item, hits=hits)


# the degrees every kernel case holds: nothing, one, two, a round of 32 and one more, a chunk of 64 and one more, two chunks + 3
KERNEL_DEGREES = (0, 1, 2, BPR_ROUND - 1, BPR_ROUND, BPR_ROUND + 1, BPR_CHUNK, BPR_CHUNK + 1, 2 * BPR_CHUNK + 3, 5, 40)
KERNEL_S = (1, 63, 64, 65, 511, 512, 513, 1100)


def kernel_case(S, n_users=67, seed=0, scale=None):
    """Synthetic inputs of tmf_bpr_pairs: user q has KERNEL_DEGREES[q % 11] stored entries - all positive but for the users with 5
    (only values <= 0) and 40 (mixed signs, zeros among them) -, scores ~ N(0, 1).  ``scale``: per-user magnitudes instead (the
    scores of user q are +-scale[q % len(scale)] (1 + 0.1 N(0, 1)); None in the tuple = every magnitude mixed inside the user)."""
    rng = np.random.default_rng(1000 * S + n_users + seed)
    deg = np.array([KERNEL_DEGREES[q % len(KERNEL_DEGREES)] for q in range(n_users)], np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    nnz = int(rowptr[-1])
    val = rng.integers(1, 6, nnz).astype(np.float32)
    for q in range(n_users):
        b, e = rowptr[q], rowptr[q + 1]
        if deg[q] == 5:
            val[b:e] = rng.choice(np.array([0, -1, -3], np.float32), 5)
        elif deg[q] == 40:
            val[b:e] = rng.choice(np.array([-2, 0, 1, 4], np.float32), 40)
    p = rng.standard_normal(nnz).astype(np.float32)
    sp = rng.standard_normal((n_users, S)).astype(np.float32)
    if scale is not None:
        mags = np.array([x for x in scale if x is not None], np.float32)
        for q in range(n_users):
            b, e = rowptr[q], rowptr[q + 1]
            mag = scale[q % len(scale)]
            for arr in (p[b:e], sp[q]):
                mg = rng.choice(mags, arr.shape[0]) if mag is None else np.float32(mag)
                arr[:] = (rng.choice(np.array([-1, 1], np.float32), arr.shape[0]) * mg * (1 + 0.1 * arr)).astype(np.float32)
    return rowptr, val, p, sp


MAGNITUDES = (0.0, 1e-3, 30.0, 88.0, 1e4, None)


def bpr_pairs_fp32_kernel_order(rowptr, val, p, sp):
    """tmf_bpr_pairs restated in NumPy fp32 with its order of additions: tiles of 512 samples outermost, lane = s % 64 holding the
    samples lane + 64 j; D adds sigma in ascending k; a positive's delta adds, per tile, the lanes' partials 0..31, then 32..63, then
    the halves, and the tiles in ascending order; the loss adds a lane's eight terms in fp32 and everything else in fp64."""
    f = np.float32
    rowptr, val, p, sp = np.asarray(rowptr, np.int64), np.asarray(val, f), np.asarray(p, f), np.asarray(sp, f)
    m, S = sp.shape
    inv_s = f(1) / f(S)
    delta, D, loss = np.zeros(val.shape[0], f), np.zeros((m, S), f), np.zeros(m, f)
    pad = -(-S // BPR_TILE) * BPR_TILE
    with np.errstate(invalid='ignore', over='ignore'):
        for u in range(m):
            ks = np.arange(rowptr[u], rowptr[u + 1])
            ks = ks[val[ks] > 0]
            if not ks.size:
                continue
            x = sp[u][None, :] - p[ks][:, None]
            e = np.exp(-np.abs(x)).astype(f)
            t = f(1) + e
            rcp = (f(1) / t).astype(f)
            sig = np.where(x >= 0, rcp, e * rcp).astype(f)
            soft = (np.maximum(x, f(0)) + (np.log(t).astype(f) + (e - (t - f(1))) * rcp)).astype(f)
            acc = np.zeros(S, f)
            for k in range(ks.size):
                acc = acc + sig[k]
            D[u] = acc * inv_s
            sig_p, soft_p = np.zeros((ks.size, pad), f), np.zeros((ks.size, pad), f)
            sig_p[:, :S], soft_p[:, :S] = sig, soft
            # [k, tile, j, lane]: sample = tile * 512 + j * 64 + lane
            sig_t, soft_t = sig_p.reshape(ks.size, -1, 8, 64), soft_p.reshape(ks.size, -1, 8, 64)
            lane_part = np.cumsum(sig_t, axis=2, dtype=f)[:, :, -1, :]                       # sequential over j
            halves = np.cumsum(lane_part.reshape(ks.size, -1, 2, 32), axis=3, dtype=f)[..., -1]  # sequential over 32 lanes
            tile_sum = (halves[:, :, 0] + halves[:, :, 1]).astype(f)
            dk = np.zeros(ks.size, f)
            for tl in range(tile_sum.shape[1]):
                dk = (dk + -(tile_sum[:, tl] * inv_s)).astype(f)
            delta[ks] = dk
            lane_loss = np.cumsum(soft_t, axis=2, dtype=f)[:, :, -1, :]
            loss[u] = f(lane_loss.astype(np.float64).sum() * np.float64(inv_s))
    return delta, D, loss


# ------------------------------------------------------------------------------------------------------------------------
# the closed form and the tolerances
# ------------------------------------------------------------------------------------------------------------------------
def test_problem_generator():
    p = bpr_problem(3, 60, 40, 7, 20)
    idx, val, R = p['idx'], p['val'], p['R']
    assert len({(int(u), int(i)) for u, i in idx}) == idx.shape[0] > 400 and (np.diff(idx[:, 0] * 40 + idx[:, 1]) > 0).all()
    assert (val > 0).any() and (val < 0).any() and (val == 0).any()
    assert p['empty_user'] not in idx[:, 0] and p['empty_item'] not in idx[:, 1] and p['empty_item'] not in R
    mine = idx[:, 0] == p['nonpos_user']
    assert mine.sum() >= 3 and (val[mine] <= 0).all()
    assert R.shape == (60, 20) and R.min() >= 0 and R.max() < 40 and p['hits'] >= 50
    pos = {(int(u), int(i)) for (u, i), a in zip(idx, val) if a > 0}
    assert sum((u, int(R[u, 0])) in pos for u in range(60)) == p['hits']


def test_closed_form_on_a_problem_small_enough_to_write_out():
    """One user, two positives and a stored zero, two negatives: every number by hand."""
    U0, V0 = np.array([[1.0, 0.0]]), np.array([[2.0, 0.0], [0.0, 1.0], [-1.0, 3.0], [0.5, 0.5]])
    idx, val, R = np.array([[0, 0], [0, 1], [0, 2]]), np.array([1.0, 0.0, 3.0]), np.array([[3, 1]])
    loss, delta, D, gU, gV = bpr_closed_form(U0, V0, idx, val, R)
    sg = lambda x: 1 / (1 + np.exp(-x))                                   # noqa: E731
    x = np.array([[0.5 - 2.0, 0.0 - 2.0], [0.5 + 1.0, 0.0 + 1.0]])          # [positive, sample] = sp - p
    assert rel_err(loss, np.log1p(np.exp(x)).sum() / 2) < 1e-15
    assert rel_err(delta, [-sg(x[0]).sum() / 2, 0.0, -sg(x[1]).sum() / 2]) < 1e-15 and rel_err(D, [sg(x).sum(0) / 2]) < 1e-15
    assert rel_err(gU, [D[0, 0] * V0[3] + D[0, 1] * V0[1] + delta[0] * V0[0] + delta[2] * V0[2]]) < 1e-15
    assert rel_err(gV, [delta[0] * U0[0], D[0, 1] * U0[0], delta[2] * U0[0], D[0, 0] * U0[0]]) < 1e-15


def _get_loss(U, V, idx, val, R, dtype=torch.float64):
    """(per-positive losses, dL/dU, dL/dV) of BPRLoss.get_loss fed as _fit_generic feeds it, by autograd."""
    from teamoflow_amd.mf.loss_graphs import BPRLoss
    from teamoflow_amd.mf.sparse import SparseInteractions
    U, V = (torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in (U, V))
    inter = SparseInteractions(idx, val, (U.shape[0], V.shape[0]), device='cpu')
    pred = U @ V.T
    out = BPRLoss().get_loss(tf_interactions=inter, tf_sample_predictions=torch.gather(pred, 1, torch.as_tensor(R, dtype=torch.int64)),
                             tf_prediction_serial=pred[inter.indices[:, 0], inter.indices[:, 1]], predictions=None,
                             n_items=V.shape[0], n_samples=R.shape[1])
    gU, gV = torch.autograd.grad(out.sum(), (U, V))
    return out.detach().numpy(), gU.numpy(), gV.numpy()


def test_class_surface():
    import teamoflow.mf.loss_graphs as alias
    from teamoflow_amd.mf import loss_graphs as LG
    assert alias.BPRLoss is LG.BPRLoss and issubclass(LG.BPRLoss, LG.LossGraph) and not issubclass(LG.BPRLoss, LG.WMRBLoss)


@pytest.mark.parametrize('shape', [(33, 47, 5, 12), (60, 40, 7, 1), (20, 15, 3, 40)], ids=lambda s: 'x'.join(map(str, s)))
def test_get_loss_is_the_closed_form(shape):
    m, n, r, S = shape
    p = bpr_problem(11 + S, m, n, r, S)
    loss, delta, D, gU, gV = bpr_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    out, aU, aV = _get_loss(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    assert out.shape == (int((p['val'] > 0).sum()),) and out.dtype == np.float64
    assert rel_err(out.sum(), loss) < 1e-12 and rel_err(aU, gU) < 1e-12 and rel_err(aV, gV) < 1e-12
    assert not gU[p['empty_user']].any() and not gU[p['nonpos_user']].any() and not gV[p['empty_item']].any()
    assert not delta[p['val'] <= 0].any() and (delta[p['val'] > 0] < 0).all() and not D[p['nonpos_user']].any()


@pytest.mark.parametrize('S', KERNEL_S)
def test_fp32_in_the_kernels_order_meets_the_gpu_tolerances(S):
    """What tests/test_gpu_bpr.py asks of the kernel - rel_err < 1e-5 for delta, D and the loss on kernel_case(S) - is reachable:
    fp32 arithmetic in the kernel's order of additions gets there on the same inputs."""
    case = kernel_case(S)
    ref, got = bpr_pairs_ref(*case), bpr_pairs_fp32_kernel_order(*case)
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    print(f'[fp32, kernel order] S={S}: delta {errs[0]:.3g} D {errs[1]:.3g} loss {errs[2]:.3g}')
    assert max(errs) < 1e-5 and all(g.dtype == np.float32 and np.isfinite(g).all() for g in got)


def test_fp32_in_the_kernels_order_at_every_magnitude():
    case = kernel_case(65, scale=MAGNITUDES)
    ref, got = bpr_pairs_ref(*case), bpr_pairs_fp32_kernel_order(*case)
    assert all(np.isfinite(r).all() for r in ref) and all(np.isfinite(g).all() for g in got)
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    print(f'[fp32, kernel order] magnitudes: delta {errs[0]:.3g} D {errs[1]:.3g} loss {errs[2]:.3g}')
    assert max(errs) < 1e-5


def fresh_adam_fp32(W0, g, lr):
    """The reference's step at iteration 1 in fp32 (matrix_factorization.py:176)."""
    f = np.float32
    omb1, omb2, eps = f(1) - f(0.9), f(1) - f(0.999), f(1e-7)
    alpha = f(f(lr) * np.sqrt(omb2) / omb1)
    W0, g = np.asarray(W0, f), np.asarray(g, f)
    return W0 - ((g * omb1) * alpha) / (np.sqrt((g * g) * omb2) + eps)


@pytest.mark.parametrize('shape', [(60, 40, 7, 5), (60, 40, 33, 64), (60, 40, 128, 70)], ids=lambda s: 'x'.join(map(str, s)))
def test_fp32_gradients_lie_inside_the_step_intervals(shape):
    """The other half of the GPU tolerances: the plug-in's own arithmetic in fp32 (torch autograd) stays within rel_err 1e-5 of
    the fp64 closed form, and the fp32 step of that gradient inside assert_step's interval."""
    m, n, r, S = shape
    p = bpr_problem(sum(shape), m, n, r, S)
    loss, _, _, gU, gV = bpr_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    out, aU, aV = _get_loss(p['U0'], p['V0'], p['idx'], p['val'], p['R'], torch.float32)
    errs = rel_err(out.astype(np.float64).sum(), loss), rel_err(aU, gU), rel_err(aV, gV)
    print(f'[fp32 autograd] {shape}: loss {errs[0]:.3g} gU {errs[1]:.3g} gV {errs[2]:.3g}')
    assert max(errs) < 1e-5, errs
    assert_step(fresh_adam_fp32(p['U0'], aU, LR), p['U0'], gU, LR, rtol=1e-5, what=f'{shape} U')
    assert_step(fresh_adam_fp32(p['V0'], aV, LR), p['V0'], gV, LR, rtol=1e-5, what=f'{shape} V')


# ------------------------------------------------------------------------------------------------------------------------
# the model without a GPU
# ------------------------------------------------------------------------------------------------------------------------
def _model(p, loss=None, table=True, **attrs):
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import BPRLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    model = MatrixFactorization(p['r'], loss_graph=loss or BPRLoss(), user_weight_graph=FixedInitializer(p['U0']),
                                item_weight_graph=FixedInitializer(p['V0']), n_users=p['m'], n_items=p['n'], n_samples=p['S'])
    model.verbose = False
    if table:
        model.random_ind = torch.as_tensor(p['R'])
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


def _fit(model, p, epochs):
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    model.fit(epochs, eye(p['m']), eye(p['n']), SparseInteractions(p['idx'], p['val'], (p['m'], p['n']), device='cpu'), lr=LR)
    return model


def test_generic_fit_without_a_gpu(monkeypatch):
    """30 x 20, r = 4, S = 8 through _fit_generic: 20 epochs lower the loss, the first is the closed form's mean over the positives,
    and one step moves the tables as the closed-form gradients say."""
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    p = bpr_problem(14, 30, 20, 4, 8)
    model = _fit(_model(p), p, 20)
    h = model.loss_history_
    assert not hasattr(model, '_state') and len(h) == 20 and h[-1] < h[0] and all(b < a for a, b in zip(h[:5], h[1:6])), h
    loss, _, _, gU, gV = bpr_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    assert rel_err(h[0], loss / int((p['val'] > 0).sum())) < 1e-5
    one = _fit(_model(p), p, 1)
    assert_step(one.user_embedding.detach().numpy(), p['U0'], gU, LR, rtol=1e-5, what='U')
    assert_step(one.item_embedding.detach().numpy(), p['V0'], gV, LR, rtol=1e-5, what='V')


def test_no_sample_table(monkeypatch):
    from teamoflow_amd.mf.matrix_factorization import SampleTableMissing
    p = bpr_problem(15, 12, 9, 4, 4)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(SampleTableMissing, match='BPRLoss'):
        _fit(_model(p, table=False), p, 1)


def test_loss_name_and_dispatch(monkeypatch):
    from teamoflow_amd import _engine
    from teamoflow_amd.mf import loss_graphs as LG
    from teamoflow_amd.mf.sparse import eye

    class MyBPR(LG.BPRLoss):
        pass
    assert _engine.loss_name(LG.BPRLoss()) == 'bpr' and 'bpr' in _engine.PAIR_LOSSES
    with pytest.raises(TypeError, match='BPRLoss'):
        _engine.loss_name(MyBPR())
    p = bpr_problem(16, 12, 9, 4, 4)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    for settings in ({}, dict(factor_dtype=torch.bfloat16), dict(optimizer='adam')):
        assert _model(p, **settings)._route(eye(12), eye(9)) == 'engine', settings
    assert _model(p, loss=MyBPR())._route(eye(12), eye(9)) == 'generic'
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    assert _model(p)._route(eye(12), eye(9)) == 'generic'


def test_a_bpr_epoch_needs_a_sliced_plan():
    """The one-kernel user pass has the hinge built in: a state without a sliced plan is refused, never run as WMRB."""
    from teamoflow_amd import _engine

    class Plan:
        sliced = False

    class State:
        wplan = Plan()
    with pytest.raises(ValueError, match="'bpr' on a state without a sliced WmrbPlan"):
        _engine.run_epoch(State(), None, None, 'bpr')


@pytest.mark.parametrize('setting', [('batch_users', 8), ('shard_items', 2), ('data_parallel', True), ('data_parallel', 'force')],
                         ids=lambda s: f'{s[0]}={s[1]}')
@pytest.mark.parametrize('gpu', [False, True], ids=['cpu', 'gpu'])
def test_unbuilt_forms_are_refused_before_anything_is_built(monkeypatch, setting, gpu):
    from teamoflow_amd import _engine
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    p = bpr_problem(17, 12, 9, 4, 4)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: gpu)
    for name in ('_fit_sparse', '_fit_generic'):
        monkeypatch.setattr(MatrixFactorization, name, lambda self, *a, **k: pytest.fail('a fit was started'))
    monkeypatch.setattr(_engine, 'InteractionPlan', lambda *a, **k: pytest.fail('a plan was built'))
    with pytest.raises(NotImplementedError, match=setting[0]):
        _fit(_model(p, **{setting[0]: setting[1]}), p, 1)


def test_save_and_load(tmp_path, monkeypatch):
    from teamoflow_amd.mf.loss_graphs import BPRLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    p = bpr_problem(18, 12, 9, 4, 4)
    model = _fit(_model(p), p, 2)
    path = str(tmp_path / 'model.pt')
    model.save(path)
    back = MatrixFactorization.load(path, device='cpu')
    assert type(back.loss_graph) is BPRLoss and back.loss_history_ == model.loss_history_
    assert torch.equal(back.user_embedding, model.user_embedding.detach()) and torch.equal(back.random_ind.cpu(), model.random_ind)
    again = _fit(back, p, 2)                                            # a loaded model trains again, through the same path
    assert again.loss_history_ == model.loss_history_


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_built():
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    declared = set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    lib = _lib.load_library()
    assert 'tmf_bpr_pairs' in declared and 'tmf_bpr_pairs' in _lib.SIGNATURES and hasattr(lib, 'tmf_bpr_pairs')
    # tmf_wmrb_hinge2_ordered's arguments without c
    assert len(_lib.SIGNATURES['tmf_bpr_pairs'][1]) == len(_lib.SIGNATURES['tmf_wmrb_hinge2_ordered'][1]) - 1
    make = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS :=.*\btmf_bpr\.hip\b', make, re.M)


def test_argument_checks_fail_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail differently; these return first."""
    import ctypes
    from teamoflow_amd import _lib
    lib = _lib.load_library()
    host = (ctypes.c_double * 8)()              # stands for any non-null buffer: never dereferenced
    H, i32 = ctypes.cast(host, ctypes.c_void_p), ctypes.c_int32
    assert lib.tmf_bpr_pairs(None, None, None, None, i32(0), i32(8), None, None, None, None, None) == 0     # no users: nothing to do
    for args in ((None, H, H, H, i32(3), i32(8), H, H, H), (H, H, H, None, i32(3), i32(8), H, H, H), (H, H, H, H, i32(3), i32(8), H, None, H),
                 (H, H, H, H, i32(3), i32(0), H, H, H), (H, H, H, H, i32(-1), i32(8), H, H, H)):
        assert lib.tmf_bpr_pairs(*args, None, None) == -1 and 'bpr_pairs' in lib.tmf_last_error().decode()
