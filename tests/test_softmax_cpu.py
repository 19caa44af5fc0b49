"""CPU side of SampledSoftmaxLoss (no GPU): the NumPy fp64 closed form the GPU tests compare the engine with, the statement the GPU
tolerances rest on (the same sums in fp32, in the order tmf_softmax_pairs adds them, against fp64 on the GPU file's own inputs), the
plug-in's get_loss, a fit through the generic loop, the dispatch and its refusals, save / load, and the C ABI of tmf_softmax_pairs
(declared, bound, built).  The problem generators are tests/test_bpr_cpu.py's."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_step, rel_err
from test_bpr_cpu import KERNEL_DEGREES, LR, MAGNITUDES, bpr_problem, fresh_adam_fp32, kernel_case

SM_SPL, SM_CAP, SM_CHUNK = 16, 1024, 64         # csrc/tmf_softmax.hip: XSPL, XCAP, XCHUNK
# rows below, at and above the lane count, half a tile, the register-resident tile, and over two tiles
KERNEL_S = (1, 63, 64, 65, 511, 512, 513, SM_CAP - 1, SM_CAP, SM_CAP + 1, 2100)
KERNEL_C = (1.0, 100_000 / 1024)                # c = 1 and an n_items / n_samples


# ------------------------------------------------------------------------------------------------------------------------
# the reference: shares no code with the package
# ------------------------------------------------------------------------------------------------------------------------
def softmax_pairs_ref(rowptr, val, p, sp, c=1.0):
    """tmf_softmax_pairs in fp64 on given scores: (delta [nnz], D [m, S], loss_part [m]).  Everything relative to
    m_k = max(p_k, max_s sp[u, s]): no exponential of a positive number."""
    rowptr, val = np.asarray(rowptr, np.int64), np.asarray(val, np.float64)
    p, sp = np.asarray(p, np.float64), np.asarray(sp, np.float64)
    m, S = sp.shape
    delta, D, loss = np.zeros(val.shape[0]), np.zeros((m, S)), np.zeros(m)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for u in range(m):
            ks = np.arange(rowptr[u], rowptr[u + 1])
            ks = ks[val[ks] > 0]
            if not ks.size:
                continue
            top = np.maximum(p[ks], sp[u].max())                       # [P]
            neg = c * np.exp(sp[u][None, :] - top[:, None])            # [P, S]: c exp(sp_s - m_k)
            own = np.exp(p[ks] - top)                                  # 1 where the positive is on top
            den = own + neg.sum(1)
            delta[ks] = -neg.sum(1) / den
            D[u] = (neg / den[:, None]).sum(0)
            loss[u] = (np.log1p((own - 1.0) + neg.sum(1)) + (top - p[ks])).sum()    # log(den): a den of 1 + 1e-25 still costs 1e-25
    return delta, D, loss


def softmax_closed_form(U0, V0, idx, val, R, c=1.0):
    """One SampledSoftmaxLoss epoch in fp64.  idx: row-major (user, item) pairs (the CSR order), R [m, S] the negative table.
    -> (loss sum over the positives, delta [nnz], D [m, S] in R's order, gU, gV)."""
    U, V = np.asarray(U0, np.float64), np.asarray(V0, np.float64)
    idx, R = np.asarray(idx, np.int64), np.asarray(R, np.int64)
    m, S = R.shape
    u, i = idx[:, 0], idx[:, 1]
    assert (np.diff(u * V.shape[0] + i) >= 0).all(), 'row-major pairs'
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=m))])
    p = np.einsum('kr,kr->k', U[u], V[i])
    sp = np.einsum('ur,usr->us', U, V[R])
    delta, D, loss = softmax_pairs_ref(rowptr, val, p, sp, c)
    gU = np.einsum('us,usr->ur', D, V[R])
    np.add.at(gU, u, delta[:, None] * V[i])
    gV = np.zeros_like(V)
    np.add.at(gV, R.reshape(-1), (D[:, :, None] * U[:, None, :]).reshape(m * S, -1))
    np.add.at(gV, i, delta[:, None] * U[u])
    return loss.sum(), delta, D, gU, gV


def _butterfly(v):
    """The kernel's fixed xor butterfly over 64 lanes, in the dtype of v: every lane ends with the same bits."""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[lanes ^ off]).astype(v.dtype)
    assert (v == v[0]).all() or np.isnan(v).all()
    return v[0]


def _exp32(x):
    """exp of an fp32 argument, rounded to fp32 (the kernel's exponential carries x log2(e) to 48 bits: about an ulp)."""
    return np.exp(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def softmax_pairs_fp32_kernel_order(rowptr, val, p, sp, c=1.0):
    """tmf_softmax_pairs restated in NumPy fp32 with its order of additions: lanes own the samples s = 1024 tile + 64 j + lane; Z adds a
    lane's e_s in ascending j, tile after tile, then the xor butterfly over the lanes; the stored interactions are taken 64 at a
    time in CSR order, one per lane: the pass's c t_k / den_k by the same butterfly (zeros from the lanes without a positive), the
    passes in ascending order; the loss in the lanes' fp64 accumulators and one butterfly at the end."""
    f = np.float32
    rowptr, val, p, sp, c = np.asarray(rowptr, np.int64), np.asarray(val, f), np.asarray(p, f), np.asarray(sp, f), f(c)
    m, S = sp.shape
    delta, D, loss = np.zeros(val.shape[0], f), np.zeros((m, S), f), np.zeros(m, f)
    tiles = -(-S // SM_CAP)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for u in range(m):
            b, e = int(rowptr[u]), int(rowptr[u + 1])
            if not (val[b:e] > 0).any():
                continue
            x = np.full(tiles * SM_CAP, -np.inf, f)
            x[:S] = sp[u]
            M = x.max()
            ex = _exp32(x - M).reshape(tiles, SM_SPL, 64)                          # [tile, j, lane]
            z = np.zeros(64, f)
            for tile in range(tiles):
                z = (z + np.cumsum(ex[tile], axis=0, dtype=f)[-1]).astype(f)      # a lane's sixteen in ascending j, then onto its sum
            cZ = f(c * _butterfly(z))
            C, lacc = f(0), np.zeros(64, np.float64)
            for cb in range(b, e, SM_CHUNK):
                n = min(SM_CHUNK, e - cb)
                pos = np.zeros(64, bool)
                pos[:n] = val[cb:cb + n] > 0
                pk = np.zeros(64, f)
                pk[:n] = p[cb:cb + n]
                top = np.maximum(pk, M)
                t, a = _exp32(M - top), _exp32(pk - top)
                bk = (cZ * t).astype(f)
                hi, lo = np.where(bk > a, bk, a), np.where(bk > a, a, bk)
                den = (hi + lo).astype(f)
                dk = np.where(pos, -(bk / den), f(0)).astype(f)
                w = np.where(pos, (c * t).astype(f) / den, f(0)).astype(f)
                lk = ((np.log(den).astype(f) + ((lo - (den - hi)).astype(f) / den).astype(f)).astype(f) + (top - pk).astype(f)).astype(f)
                lacc += np.where(pos, lk, f(0)).astype(np.float64)
                delta[cb:cb + n] = dk[:n]
                C = f(C + _butterfly(w))
            D[u] = (ex.reshape(-1)[:S] * C).astype(f)
            loss[u] = f(_butterfly(lacc))
    return delta, D, loss


def sum_identity_gaps(rowptr, val, delta, D):
    """Per user with a positive: (|sum_s D[u, s] + sum_k delta_k|, sum_k |delta_k|), the sums in fp64 - the probabilities sum to one."""
    out = []
    for u in range(D.shape[0]):
        ks = np.arange(rowptr[u], rowptr[u + 1])
        ks = ks[np.asarray(val)[ks] > 0]
        if ks.size:
            d = np.asarray(delta, np.float64)[ks]
            out.append((abs(np.asarray(D[u], np.float64).sum() + d.sum()), np.abs(d).sum()))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the closed form and the tolerances
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1.0, 2.0])
def test_closed_form_on_a_problem_small_enough_to_write_out(c):
    """One user, two positives and a stored zero, two negatives: every number by hand."""
    U0, V0 = np.array([[1.0, 0.0]]), np.array([[2.0, 0.0], [0.0, 1.0], [-1.0, 3.0], [0.5, 0.5]])
    idx, val, R = np.array([[0, 0], [0, 1], [0, 2]]), np.array([1.0, 0.0, 3.0]), np.array([[3, 1]])
    loss, delta, D, gU, gV = softmax_closed_form(U0, V0, idx, val, R, c)
    pk, neg = np.array([2.0, -1.0]), c * np.exp(np.array([0.5, 0.0]))           # the positives' scores; c exp(sp) of the two samples
    den = np.exp(pk) + neg.sum()
    assert rel_err(loss, -np.log(np.exp(pk) / den).sum()) < 1e-15
    assert rel_err(delta, [-neg.sum() / den[0], 0.0, -neg.sum() / den[1]]) < 1e-15
    assert rel_err(D, [neg / den[0] + neg / den[1]]) < 1e-15 and abs(D.sum() + delta.sum()) < 1e-15
    assert rel_err(gU, [D[0, 0] * V0[3] + D[0, 1] * V0[1] + delta[0] * V0[0] + delta[2] * V0[2]]) < 1e-15
    assert rel_err(gV, [delta[0] * U0[0], D[0, 1] * U0[0], delta[2] * U0[0], D[0, 0] * U0[0]]) < 1e-15


def _get_loss(U, V, idx, val, R, catalog_scale=False, dtype=torch.float64):
    """(per-positive losses, dL/dU, dL/dV, dL/dp, dL/dsp) of SampledSoftmaxLoss.get_loss fed as _fit_generic feeds it, by autograd."""
    from teamoflow_amd.mf.loss_graphs import SampledSoftmaxLoss
    from teamoflow_amd.mf.sparse import SparseInteractions
    U, V = (torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in (U, V))
    inter = SparseInteractions(idx, val, (U.shape[0], V.shape[0]), device='cpu')
    pred = U @ V.T
    sp, p = torch.gather(pred, 1, torch.as_tensor(R, dtype=torch.int64)), pred[inter.indices[:, 0], inter.indices[:, 1]]
    out = SampledSoftmaxLoss(catalog_scale).get_loss(tf_interactions=inter, tf_sample_predictions=sp, tf_prediction_serial=p,
                                                     predictions=None, n_items=V.shape[0], n_samples=R.shape[1])
    gU, gV, gp, gsp = torch.autograd.grad(out.sum(), (U, V, p, sp))
    return out.detach().numpy(), gU.numpy(), gV.numpy(), gp.numpy(), gsp.numpy()


def test_class_surface():
    import teamoflow.mf.loss_graphs as alias
    from teamoflow_amd.mf import loss_graphs as LG
    from teamoflow_amd.mf import matrix_factorization as M
    S = LG.SampledSoftmaxLoss
    assert alias.SampledSoftmaxLoss is S and issubclass(S, LG.LossGraph) and not issubclass(S, LG.WMRBLoss)
    assert S().catalog_scale is False and S(catalog_scale=True).catalog_scale is True and S(1).catalog_scale is True
    assert S in M.ENGINE_LOSSES and S in M.TABLE_LOSSES and S in M.PAIR_STEP_LOSSES


@pytest.mark.parametrize('catalog_scale', [False, True], ids=['c=1', 'c=n/S'])
@pytest.mark.parametrize('shape', [(33, 47, 5, 12), (60, 40, 7, 1), (20, 15, 3, 40)], ids=lambda s: 'x'.join(map(str, s)))
def test_get_loss_is_the_closed_form(shape, catalog_scale):
    m, n, r, S = shape
    p = bpr_problem(11 + S, m, n, r, S)
    c = n / S if catalog_scale else 1.0
    loss, delta, D, gU, gV = softmax_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'], c)
    out, aU, aV, ap, asp = _get_loss(p['U0'], p['V0'], p['idx'], p['val'], p['R'], catalog_scale)
    assert out.shape == (int((p['val'] > 0).sum()),) and out.dtype == np.float64 and (out > 0).all()
    assert rel_err(out.sum(), loss) < 1e-12 and rel_err(aU, gU) < 1e-12 and rel_err(aV, gV) < 1e-12
    assert rel_err(ap, delta) < 1e-12 and rel_err(asp, D) < 1e-12            # with respect to the scores themselves
    assert not gU[p['empty_user']].any() and not gU[p['nonpos_user']].any() and not gV[p['empty_item']].any()
    assert not delta[p['val'] <= 0].any() and (delta[p['val'] > 0] < 0).all() and not D[p['nonpos_user']].any()
    assert all(gap <= 1e-12 * size for gap, size in sum_identity_gaps(
        np.concatenate([[0], np.cumsum(np.bincount(p['idx'][:, 0], minlength=m))]), p['val'], delta, D))


def test_get_loss_is_stable_at_large_scores():
    """Scores of +-1e4 in fp32: a bare exp would overflow; logsumexp does not."""
    from teamoflow_amd.mf.loss_graphs import SampledSoftmaxLoss
    from teamoflow_amd.mf.sparse import SparseInteractions
    inter = SparseInteractions(np.array([[0, 0], [1, 1]]), np.array([1.0, 1.0], np.float32), (2, 3), device='cpu')
    sp = torch.tensor([[1e4, -1e4], [-1e4, -1e4]], requires_grad=True)
    p = torch.tensor([-1e4, 1e4], requires_grad=True)
    out = SampledSoftmaxLoss().get_loss(tf_interactions=inter, tf_sample_predictions=sp, tf_prediction_serial=p, predictions=None,
                                        n_items=3, n_samples=2)
    gp, gsp = torch.autograd.grad(out.sum(), (p, sp))
    assert out.tolist() == [2e4, 0.0] and torch.isfinite(gp).all() and torch.isfinite(gsp).all() and gp.tolist() == [-1.0, 0.0]


def check_restatement(case, c, what):
    ref, got = softmax_pairs_ref(*case, c), softmax_pairs_fp32_kernel_order(*case, c)
    assert all(np.isfinite(r).all() for r in ref) and all(g.dtype == np.float32 and np.isfinite(g).all() for g in got)
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    gaps = sum_identity_gaps(case[0], case[1], got[0], got[1])
    worst = max(gap / size for gap, size in gaps)
    print(f'[fp32, kernel order] {what} c={c:.4g}: delta {errs[0]:.3g} D {errs[1]:.3g} loss {errs[2]:.3g} identity {worst:.3g}')
    assert max(errs) < 1e-5, errs
    assert all(gap <= 1e-5 * size for gap, size in gaps), worst
    return ref, got


@pytest.mark.parametrize('c', KERNEL_C, ids=['c=1', 'c=n/S'])
@pytest.mark.parametrize('S', KERNEL_S)
def test_fp32_in_the_kernels_order_meets_the_gpu_tolerances(S, c):
    """What tests/test_gpu_softmax.py asks of the kernel - rel_err < 1e-5 for delta, D and the loss, and the sum identity, on
    kernel_case(S) - is reachable: fp32 arithmetic in the kernel's order of additions gets there on the same inputs."""
    check_restatement(kernel_case(S), c, f'S={S}')


@pytest.mark.parametrize('c', KERNEL_C, ids=['c=1', 'c=n/S'])
def test_fp32_in_the_kernels_order_at_every_magnitude(c):
    case = kernel_case(65, scale=MAGNITUDES)
    ref, got = check_restatement(case, c, 'magnitudes')
    rowptr, val = case[0], case[1]
    for u in range(67):                                       # user by user: the sizes differ by orders of magnitude between them
        if (val[rowptr[u]:rowptr[u + 1]] > 0).any():
            assert rel_err(got[2][u], ref[2][u]) < 1e-5, (u, MAGNITUDES[u % len(MAGNITUDES)])


def test_a_positive_far_above_every_sample_costs_b_not_zero():
    """p = +30 against samples near -30: 1 + b rounds to 1 in fp32, and the loss is still b (the second term of the logarithm)."""
    rowptr, val, p = np.array([0, 1], np.int64), np.array([1.0], np.float32), np.array([30.0], np.float32)
    sp = (-30 + 0.1 * np.random.default_rng(0).standard_normal((1, 65))).astype(np.float32)
    ref, got = softmax_pairs_ref(rowptr, val, p, sp), softmax_pairs_fp32_kernel_order(rowptr, val, p, sp)
    assert 0 < ref[2][0] < 1e-20 and got[2][0] > 0 and max(rel_err(g, r) for g, r in zip(got, ref)) < 1e-5


@pytest.mark.parametrize('catalog_scale', [False, True], ids=['c=1', 'c=n/S'])
@pytest.mark.parametrize('shape', [(60, 40, 7, 5), (60, 40, 33, 64), (60, 40, 128, 70)], ids=lambda s: 'x'.join(map(str, s)))
def test_fp32_gradients_lie_inside_the_step_intervals(shape, catalog_scale):
    """The other half of the GPU tolerances: fp32 scores through the restatement give gradients within rel_err 1e-5 of the fp64
    closed form, and the fp32 step of those gradients lies inside assert_step's interval."""
    m, n, r, S = shape
    p = bpr_problem(sum(shape), m, n, r, S)
    c = n / S if catalog_scale else 1.0
    loss, _, _, gU, gV = softmax_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'], c)
    u, i, R = p['idx'][:, 0], p['idx'][:, 1], p['R'].astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=m))])
    pk = np.einsum('kr,kr->k', p['U0'][u], p['V0'][i]).astype(np.float32)             # fp32 scores of fp32 tables
    sp = np.einsum('ur,usr->us', p['U0'], p['V0'][R]).astype(np.float32)
    delta, D, lp = (x.astype(np.float64) for x in softmax_pairs_fp32_kernel_order(rowptr, p['val'], pk, sp, c))
    aU = np.einsum('us,usr->ur', D, p['V0'][R].astype(np.float64))
    np.add.at(aU, u, delta[:, None] * p['V0'][i])
    aV = np.zeros((n, r))
    np.add.at(aV, R.reshape(-1), (D[:, :, None] * p['U0'][:, None, :]).reshape(m * S, -1))
    np.add.at(aV, i, delta[:, None] * p['U0'][u])
    errs = rel_err(lp.sum(), loss), rel_err(aU, gU), rel_err(aV, gV)
    print(f'[fp32, kernel order] {shape} c={c:.3g}: loss {errs[0]:.3g} gU {errs[1]:.3g} gV {errs[2]:.3g}')
    assert max(errs) < 1e-5, errs
    assert_step(fresh_adam_fp32(p['U0'], aU, LR), p['U0'], gU, LR, rtol=1e-5, what=f'{shape} U')
    assert_step(fresh_adam_fp32(p['V0'], aV, LR), p['V0'], gV, LR, rtol=1e-5, what=f'{shape} V')


# ------------------------------------------------------------------------------------------------------------------------
# the model without a GPU
# ------------------------------------------------------------------------------------------------------------------------
def _model(p, loss=None, table=True, **attrs):
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import SampledSoftmaxLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    model = MatrixFactorization(p['r'], loss_graph=loss or SampledSoftmaxLoss(), user_weight_graph=FixedInitializer(p['U0']),
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


@pytest.mark.parametrize('catalog_scale', [False, True], ids=['c=1', 'c=n/S'])
def test_generic_fit_without_a_gpu(monkeypatch, catalog_scale):
    """30 x 20, r = 4, S = 8 through _fit_generic: 20 epochs lower the loss, the first is the closed form's mean over the positives,
    and one step moves the tables as the closed-form gradients say."""
    from teamoflow_amd.mf.loss_graphs import SampledSoftmaxLoss
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    p = bpr_problem(14, 30, 20, 4, 8)
    model = _fit(_model(p, SampledSoftmaxLoss(catalog_scale)), p, 20)
    h = model.loss_history_
    assert not hasattr(model, '_state') and len(h) == 20 and h[-1] < h[0] and all(b < a for a, b in zip(h[:5], h[1:6])), h
    loss, _, _, gU, gV = softmax_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'], 20 / 8 if catalog_scale else 1.0)
    assert rel_err(h[0], loss / int((p['val'] > 0).sum())) < 1e-5
    one = _fit(_model(p, SampledSoftmaxLoss(catalog_scale)), p, 1)
    assert_step(one.user_embedding.detach().numpy(), p['U0'], gU, LR, rtol=1e-5, what='U')
    assert_step(one.item_embedding.detach().numpy(), p['V0'], gV, LR, rtol=1e-5, what='V')


def test_no_sample_table(monkeypatch):
    from teamoflow_amd.mf.matrix_factorization import SampleTableMissing
    p = bpr_problem(15, 12, 9, 4, 4)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(SampleTableMissing, match='SampledSoftmaxLoss'):
        _fit(_model(p, table=False), p, 1)


def test_loss_name_and_dispatch(monkeypatch):
    from teamoflow_amd import _engine
    from teamoflow_amd.mf import loss_graphs as LG
    from teamoflow_amd.mf.sparse import eye

    class MySoftmax(LG.SampledSoftmaxLoss):
        pass
    assert _engine.loss_name(LG.SampledSoftmaxLoss()) == _engine.loss_name(LG.SampledSoftmaxLoss(True)) == 'softmax'
    assert 'softmax' in _engine.PAIR_LOSSES
    with pytest.raises(TypeError, match='SampledSoftmaxLoss'):
        _engine.loss_name(MySoftmax())
    p = bpr_problem(16, 12, 9, 4, 4)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    for settings in ({}, dict(factor_dtype=torch.bfloat16), dict(optimizer='adam'), dict(user_alpha=0.1), dict(resample_every=2)):
        assert _model(p, **settings)._route(eye(12), eye(9)) == 'engine', settings
    assert _model(p, loss=MySoftmax())._route(eye(12), eye(9)) == 'generic'
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    assert _model(p)._route(eye(12), eye(9)) == 'generic'


def test_a_softmax_epoch_needs_a_sliced_plan():
    """The one-kernel user pass has the hinge built in: a state without a sliced plan is refused, never run as WMRB."""
    from teamoflow_amd import _engine

    class Plan:
        sliced = False

    class State:
        wplan = Plan()
    with pytest.raises(ValueError, match="'softmax' on a state without a sliced WmrbPlan"):
        _engine.run_epoch(State(), None, None, 'softmax', 1.0)
    with pytest.raises(ValueError, match='pairs=softmax needs the sliced user pass'):
        _engine.epoch_wmrb(State(), None, 1.0, None, pairs='softmax')


@pytest.mark.parametrize('setting', [('batch_users', 8), ('shard_items', 2), ('data_parallel', True), ('data_parallel', 'force')],
                         ids=lambda s: f'{s[0]}={s[1]}')
@pytest.mark.parametrize('gpu', [False, True], ids=['cpu', 'gpu'])
def test_unbuilt_forms_are_refused_before_anything_is_built(monkeypatch, setting, gpu):
    from teamoflow_amd import _engine
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    p = bpr_problem(17, 12, 9, 4, 4)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: gpu)
    for name in ('_fit_sparse', '_fit_generic'):
        monkeypatch.setattr(MatrixFactorization, name, lambda self, *a, **k: pytest.fail('a fit was started'))
    monkeypatch.setattr(_engine, 'InteractionPlan', lambda *a, **k: pytest.fail('a plan was built'))
    monkeypatch.setattr(FixedInitializer, 'initialize_weights', lambda self, *a, **k: pytest.fail('a weight was drawn'))
    with pytest.raises(NotImplementedError, match=f'SampledSoftmaxLoss with {setting[0]}='):
        _fit(_model(p, **{setting[0]: setting[1]}), p, 1)


def test_resample_every_is_accepted(monkeypatch):
    """A fresh table every epoch through the generic loop: three rounds, and another trajectory than the one table gives."""
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    p = bpr_problem(19, 30, 20, 4, 8)
    still, fresh = _fit(_model(p), p, 3), _fit(_model(p, resample_every=1), p, 3)
    assert still.resample_rounds_ == 1 and fresh.resample_rounds_ == 3
    assert fresh.loss_history_[0] == still.loss_history_[0] and fresh.loss_history_[1:] != still.loss_history_[1:]
    assert torch.equal(torch.as_tensor(fresh.random_ind), torch.as_tensor(p['R']))          # the model's own table stays


def test_save_and_load(tmp_path, monkeypatch):
    from teamoflow_amd.mf.loss_graphs import SampledSoftmaxLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    p = bpr_problem(18, 12, 9, 4, 4)
    for catalog_scale in (True, False):
        model = _fit(_model(p, SampledSoftmaxLoss(catalog_scale)), p, 2)
        path = str(tmp_path / f'model{int(catalog_scale)}.pt')
        model.save(path)
        back = MatrixFactorization.load(path, device='cpu')
        assert type(back.loss_graph) is SampledSoftmaxLoss and back.loss_graph.catalog_scale is catalog_scale
        assert back.loss_history_ == model.loss_history_
        assert torch.equal(back.user_embedding, model.user_embedding.detach()) and torch.equal(back.random_ind.cpu(), model.random_ind)
        again = _fit(back, p, 2)                                            # a loaded model trains again, through the same path
        assert again.loss_history_ == model.loss_history_
    assert _fit(_model(p), p, 2).loss_history_ == model.loss_history_ != _fit(_model(p, SampledSoftmaxLoss(True)), p, 2).loss_history_


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_built():
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    declared = set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    lib = _lib.load_library()
    assert 'tmf_softmax_pairs' in declared and 'tmf_softmax_pairs' in _lib.SIGNATURES and hasattr(lib, 'tmf_softmax_pairs')
    assert _lib.SIGNATURES['tmf_softmax_pairs'] == _lib.SIGNATURES['tmf_wmrb_hinge2_ordered']       # the hinge kernel's arguments
    make = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS :=.*\btmf_softmax\.hip\b', make, re.M)
    source = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'tmf_softmax.hip')).read()       # the restatement's constants are the kernel's
    assert all(line in source for line in (f'constexpr int XSPL = {SM_SPL};', 'constexpr int XCAP = 64 * XSPL;',
                                           f'constexpr int XCHUNK = {SM_CHUNK};')) and SM_CAP == 64 * SM_SPL


def test_argument_checks_fail_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail differently; these return first."""
    import ctypes
    from teamoflow_amd import _lib
    lib = _lib.load_library()
    host = (ctypes.c_double * 8)()              # stands for any non-null buffer: never dereferenced
    H, i32 = ctypes.cast(host, ctypes.c_void_p), ctypes.c_int32
    assert lib.tmf_softmax_pairs(None, None, None, None, i32(0), i32(8), 1.0, None, None, None, None, None) == 0     # no users: nothing to do
    for args in ((None, H, H, H, i32(3), i32(8), 1.0, H, H, H), (H, H, H, None, i32(3), i32(8), 1.0, H, H, H),
                 (H, H, H, H, i32(3), i32(8), 1.0, H, None, H), (H, H, H, H, i32(3), i32(0), 1.0, H, H, H),
                 (H, H, H, H, i32(-1), i32(8), 1.0, H, H, H)):
        assert lib.tmf_softmax_pairs(*args, None, None) == -1 and 'softmax_pairs' in lib.tmf_last_error().decode()
