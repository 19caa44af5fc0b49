"""CPU side of sampling_correction='logq' (no GPU): utils.log_expected_count, the NumPy fp64 closed form of the corrected sampled
softmax that the GPU tests compare the engine with (pinned here to the plug-in's own get_loss on sp - l[R]), the statement the GPU
tolerances rest on (the kernel's arithmetic restated in fp32 on fl32(sp - off), against fp64 on the exact difference), a fit
through the generic loop, the refusals, save / load, the printed table and the C ABI of the two entry points.  The problem
generators are tests/test_bpr_cpu.py's, the fp32 restatement tests/test_softmax_cpu.py's."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_step, rel_err
from test_bpr_cpu import LR, bpr_problem, kernel_case
from test_softmax_cpu import KERNEL_S, softmax_pairs_fp32_kernel_order, sum_identity_gaps

OFFSET_LOWS = (-25.0, -12.0)                    # off uniform in [low, 0]: logs of expected counts down to e^-25 and e^-12
# tests/test_bpr_cpu.py's MAGNITUDES without 88 and 1e4: the corrected score is ONE fp32 rounding of sp - off, which at |sp| = 1e4 is
# 5e-4 in the exponent of e_s - delta is then off by 2.0e-5 against fp64 on the exact difference, whatever the kernel does after it.
# Left out, not tolerated: the bound stays 1e-5
LOGQ_MAGNITUDES = (0.0, 1e-3, 30.0, None)


# ------------------------------------------------------------------------------------------------------------------------
# the reference: shares no code with the package
# ------------------------------------------------------------------------------------------------------------------------
def log_expected_count_ref(q, S):
    """l_i = log(min(1, S q_i / T)) in fp64, 0 where q_i = 0."""
    q = np.asarray(q, np.float64)
    count = np.minimum(1.0, S * q / q.sum())
    return np.array([math.log(c) if c > 0 else 0.0 for c in count])


def logq_pairs_ref(rowptr, val, p, x):
    """The corrected pair step in fp64 on given corrected scores x[u, s] = sp[u, s] - off[u, s] (float64) and raw p:
    (delta [nnz], D [m, S], loss_part [m]) with loss_k = logaddexp(p_k, logsumexp_s x[u, s]) - p_k for a stored value > 0."""
    rowptr, val, p, x = np.asarray(rowptr, np.int64), np.asarray(val), np.asarray(p, np.float64), np.asarray(x, np.float64)
    m, S = x.shape
    delta, D, loss = np.zeros(val.shape[0]), np.zeros((m, S)), np.zeros(m)
    for u in range(m):
        ks = np.arange(rowptr[u], rowptr[u + 1])
        ks = ks[val[ks] > 0]
        if not ks.size:
            continue
        M = x[u].max()
        lse = M + np.log(np.exp(x[u] - M).sum())
        tot = np.logaddexp(p[ks], lse)
        loss[u] = (tot - p[ks]).sum()
        delta[ks] = -np.exp(lse - tot)
        D[u] = np.exp(x[u][None, :] - tot[:, None]).sum(0)
    return delta, D, loss


def logq_closed_form(U0, V0, idx, val, R, ell):
    """One SampledSoftmaxLoss epoch under the logQ correction in fp64.  idx: row-major (user, item) pairs, R [m, S] the negative
    table, ell [n_items] the offsets.  -> (loss sum over the positives, delta [nnz], D [m, S] in R's order, gU, gV): D is the
    derivative with respect to the raw sampled score as well, the offset being a constant."""
    U, V = np.asarray(U0, np.float64), np.asarray(V0, np.float64)
    idx, R, ell = np.asarray(idx, np.int64), np.asarray(R, np.int64), np.asarray(ell, np.float64)
    m, S = R.shape
    u, i = idx[:, 0], idx[:, 1]
    assert (np.diff(u * V.shape[0] + i) >= 0).all(), 'row-major pairs'
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=m))])
    p = np.einsum('kr,kr->k', U[u], V[i])
    sp = np.einsum('ur,usr->us', U, V[R])
    delta, D, loss = logq_pairs_ref(rowptr, val, p, sp - ell[R])
    gU = np.einsum('us,usr->ur', D, V[R])
    np.add.at(gU, u, delta[:, None] * V[i])
    gV = np.zeros_like(V)
    np.add.at(gV, R.reshape(-1), (D[:, :, None] * U[:, None, :]).reshape(m * S, -1))
    np.add.at(gV, i, delta[:, None] * U[u])
    return loss.sum(), delta, D, gU, gV


def offset_case(S, low, scale=None):
    """kernel_case(S) with offsets uniform in [low, 0]: (rowptr, val, p, sp, off) in fp32."""
    rowptr, val, p, sp = kernel_case(S, scale=scale)
    off = np.random.default_rng(S).uniform(low, 0.0, sp.shape).astype(np.float32)
    return rowptr, val, p, sp, off


def exact_difference(sp, off):
    return np.asarray(sp, np.float64) - np.asarray(off, np.float64)


# ------------------------------------------------------------------------------------------------------------------------
# log_expected_count
# ------------------------------------------------------------------------------------------------------------------------
def test_log_expected_count():
    from teamoflow_amd.mf.utils import log_expected_count, popularity_weights
    q = torch.tensor([1, 2, 0, 5, 12], dtype=torch.int64)                         # T = 20
    got = log_expected_count(q, 3)                                                 # 3 q / 20 = .15 .3 0 .75 1.8 -> clamped at 1
    assert got.dtype == torch.float32 and got.device.type == 'cpu' and got.shape == (5,)
    want = np.array([math.log(0.15), math.log(0.3), 0.0, math.log(0.75), 0.0])
    assert np.array_equal(got.numpy(), want.astype(np.float32))
    assert got[4] == 0.0 and got[2] == 0.0 and (got[[0, 1, 3]] < 0).all()          # the clamp; the weight of zero
    assert np.array_equal(log_expected_count(q, 1).numpy(), log_expected_count_ref(q.numpy(), 1).astype(np.float32))
    for n, S in ((400, 64), (7, 3), (100_000, 1024)):                              # equal weights: one value, float32(log(S / n))
        for w in (1, 5368):
            flat = log_expected_count(torch.full((n,), w, dtype=torch.int64), S)
            assert (flat == np.float32(math.log(S / n))).all()
    assert not log_expected_count(torch.ones(4, dtype=torch.int64), 9).any()       # S >= n_items: every item expected once
    counts = torch.tensor([0, 3, 50, 1, 0, 7])
    qq = popularity_weights(counts, 0.75)
    ell = log_expected_count(qq, 2)
    assert np.array_equal(ell.numpy(), log_expected_count_ref(qq.numpy(), 2).astype(np.float32))
    assert ell[2] == ell.max() and ell[0] == ell[4] == ell.min()                   # monotone in the counts
    assert np.array_equal(log_expected_count(qq.to(torch.float64) * 0.5, 2).numpy(), ell.numpy())     # a function of q / T
    for bad in (torch.zeros(3), torch.tensor([1.0, -1.0]), torch.tensor([1.0, float('nan')]), torch.zeros(0)):
        with pytest.raises(ValueError):
            log_expected_count(bad, 2)
    with pytest.raises(ValueError):
        log_expected_count(q, 0)


# ------------------------------------------------------------------------------------------------------------------------
# the closed form and the tolerances
# ------------------------------------------------------------------------------------------------------------------------
def test_closed_form_on_a_problem_small_enough_to_write_out():
    """One user, two positives and a stored zero, two negatives with offsets log(1/4) and log(1/2): every number by hand."""
    U0, V0 = np.array([[1.0, 0.0]]), np.array([[2.0, 0.0], [0.0, 1.0], [-1.0, 3.0], [0.5, 0.5]])
    idx, val, R = np.array([[0, 0], [0, 1], [0, 2]]), np.array([1.0, 0.0, 3.0]), np.array([[3, 1]])
    ell = np.log(np.array([1.0, 0.5, 1.0, 0.25]))
    loss, delta, D, gU, gV = logq_closed_form(U0, V0, idx, val, R, ell)
    pk, neg = np.array([2.0, -1.0]), np.exp(np.array([0.5, 0.0])) / np.array([0.25, 0.5])     # exp(sp) / expected count
    den = np.exp(pk) + neg.sum()
    assert rel_err(loss, -np.log(np.exp(pk) / den).sum()) < 1e-15
    assert rel_err(delta, [-neg.sum() / den[0], 0.0, -neg.sum() / den[1]]) < 1e-15
    assert rel_err(D, [neg / den[0] + neg / den[1]]) < 1e-15 and abs(D.sum() + delta.sum()) < 1e-15
    assert rel_err(gU, [D[0, 0] * V0[3] + D[0, 1] * V0[1] + delta[0] * V0[0] + delta[2] * V0[2]]) < 1e-15
    assert rel_err(gV, [delta[0] * U0[0], D[0, 1] * U0[0], delta[2] * U0[0], D[0, 0] * U0[0]]) < 1e-15


@pytest.mark.parametrize('shape', [(33, 47, 5, 12), (60, 40, 7, 1), (20, 15, 3, 40)], ids=lambda s: 'x'.join(map(str, s)))
def test_the_closed_form_is_get_loss_on_the_corrected_scores(shape):
    """SampledSoftmaxLoss.get_loss fed sp - l[R] as _fit_generic feeds it, differentiated by autograd with respect to the tables and
    to the RAW scores."""
    from teamoflow_amd.mf.loss_graphs import SampledSoftmaxLoss
    from teamoflow_amd.mf.sparse import SparseInteractions
    m, n, r, S = shape
    p = bpr_problem(23 + S, m, n, r, S)
    ell = np.random.default_rng(S).uniform(-6.0, 0.0, n)
    loss, delta, D, gU, gV = logq_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'], ell)
    U, V = (torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True) for x in (p['U0'], p['V0']))
    inter = SparseInteractions(p['idx'], p['val'], (m, n), device='cpu')
    pred, R = U @ V.T, torch.as_tensor(p['R'], dtype=torch.int64)
    sp, pk = torch.gather(pred, 1, R), pred[inter.indices[:, 0], inter.indices[:, 1]]
    out = SampledSoftmaxLoss().get_loss(tf_interactions=inter, tf_sample_predictions=sp - torch.as_tensor(ell)[R],
                                        tf_prediction_serial=pk, predictions=None, n_items=n, n_samples=S)
    aU, aV, ap, asp = (g.numpy() for g in torch.autograd.grad(out.sum(), (U, V, pk, sp)))
    assert out.shape == (int((p['val'] > 0).sum()),) and (out > 0).all()
    assert rel_err(out.sum().item(), loss) < 1e-12 and rel_err(aU, gU) < 1e-12 and rel_err(aV, gV) < 1e-12
    assert rel_err(ap, delta) < 1e-12 and rel_err(asp, D) < 1e-12
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(p['idx'][:, 0], minlength=m))])
    assert all(gap <= 1e-12 * size for gap, size in sum_identity_gaps(rowptr, p['val'], delta, D))
    assert not gU[p['empty_user']].any() and not gU[p['nonpos_user']].any() and not D[p['nonpos_user']].any()
    # offsets that are all zero: the uncorrected loss
    from test_softmax_cpu import softmax_closed_form
    plain = softmax_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    zero = logq_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'], np.zeros(n))
    assert all(rel_err(a, b) < 1e-12 for a, b in zip(zero, plain))


def check_restatement(case, what):
    """The kernel's arithmetic in fp32 - ONE rounding of sp - off, then tests/test_softmax_cpu.py's restatement of tmf_softmax_pairs
    with c = 1 - against the fp64 form on the exact difference."""
    rowptr, val, p, sp, off = case
    x32 = (sp - off).astype(np.float32)
    got = softmax_pairs_fp32_kernel_order(rowptr, val, p, x32, 1.0)
    ref = logq_pairs_ref(rowptr, val, p, exact_difference(sp, off))
    assert all(np.isfinite(r).all() for r in ref) and all(g.dtype == np.float32 and np.isfinite(g).all() for g in got)
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    gaps = sum_identity_gaps(rowptr, val, got[0], got[1])
    worst = max(gap / size for gap, size in gaps)
    print(f'[fp32, kernel order] {what}: delta {errs[0]:.3g} D {errs[1]:.3g} loss {errs[2]:.3g} identity {worst:.3g}')
    assert max(errs) < 1e-5, errs
    assert all(gap <= 1e-5 * size for gap, size in gaps), worst
    return ref, got


@pytest.mark.parametrize('low', OFFSET_LOWS)
@pytest.mark.parametrize('S', KERNEL_S)
def test_fp32_in_the_kernels_order_meets_the_gpu_tolerances(S, low):
    """What tests/test_gpu_logq.py asks of tmf_softmax_pairs_offset - rel_err < 1e-5 for delta, D and the loss and the sum identity
    on kernel_case(S) with offsets in [low, 0] - is reachable in fp32 in the kernel's order of additions."""
    check_restatement(offset_case(S, low), f'S={S} off in [{low:g}, 0]')


def test_fp32_in_the_kernels_order_at_the_magnitudes():
    """Scores of magnitude 0, 1e-3 and 30 with both signs, one magnitude per user and all of them mixed inside a user (LOGQ_MAGNITUDES:
    why 88 and 1e4 are not among them), overall and user by user for the loss."""
    case = offset_case(65, -12.0, scale=LOGQ_MAGNITUDES)
    ref, got = check_restatement(case, 'magnitudes')
    rowptr, val = case[0], case[1]
    for u in range(67):
        if (val[rowptr[u]:rowptr[u + 1]] > 0).any():
            assert rel_err(got[2][u], ref[2][u]) < 1e-5, (u, LOGQ_MAGNITUDES[u % len(LOGQ_MAGNITUDES)])


# ------------------------------------------------------------------------------------------------------------------------
# the model without a GPU
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)


def make(p, loss=None, init=None, **attrs):
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import SampledSoftmaxLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    model = MatrixFactorization(p['r'], loss_graph=loss or SampledSoftmaxLoss(), user_weight_graph=init or FixedInitializer(p['U0']),
                                item_weight_graph=init or FixedInitializer(p['V0']), n_users=p['m'], n_items=p['n'], n_samples=p['S'])
    model.verbose = False
    model.random_ind = torch.as_tensor(p['R'])
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


def fit(model, p, epochs):
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    model.fit(epochs, eye(p['m']), eye(p['n']), SparseInteractions(p['idx'], p['val'], (p['m'], p['n']), device='cpu'), lr=LR)
    return model


def same_fit(a, b):
    return a.loss_history_ == b.loss_history_ and torch.equal(a.user_embedding, b.user_embedding) \
        and torch.equal(a.item_embedding, b.item_embedding)


def popularity_table(p, power, seed, S=None):
    """(q, the table of round 0 under negative_sampling='popularity', l in fp64 by the test's own formula)."""
    from teamoflow_amd import _ops
    from teamoflow_amd.mf.utils import popularity_weights
    S = p['S'] if S is None else S
    q = popularity_weights(torch.as_tensor(np.bincount(p['idx'][p['val'] > 0, 1], minlength=p['n'])), power)
    R = _ops.sample_negatives(p['n'], p['m'], S, seed=seed, device='cpu', weights=q)
    return q, R.numpy(), log_expected_count_ref(q.numpy(), S)


def test_generic_fit_under_popularity_is_the_corrected_closed_form(no_gpu):
    """30 x 20, r = 4, S = 8 through _fit_generic with tables drawn by popularity: the first loss is the corrected closed form's mean
    over the positives on the table the fit drew, one step moves the tables as its gradients say, and neither is what the
    uncorrected loss gives on that table."""
    from test_softmax_cpu import softmax_closed_form
    p, seed = bpr_problem(14, 30, 20, 4, 8), 5
    q, R, ell = popularity_table(p, 0.75, seed)
    one = fit(make(p, negative_sampling='popularity', sampling_correction='logq', sample_seed=seed), p, 1)
    assert not hasattr(one, '_state') and one.resample_rounds_ == 1
    assert one.sample_log_q_.dtype == torch.float32 and one.sample_log_q_.device.type == 'cpu'
    assert np.array_equal(one.sample_log_q_.numpy(), ell.astype(np.float32)) and (ell < 0).all() and np.ptp(ell) > 0.5
    n_pos = int((p['val'] > 0).sum())
    loss, _, _, gU, gV = logq_closed_form(p['U0'], p['V0'], p['idx'], p['val'], R, ell)
    assert rel_err(one.loss_history_[0], loss / n_pos) < 1e-5
    assert_step(one.user_embedding.detach().numpy(), p['U0'], gU, LR, rtol=1e-5, what='U')
    assert_step(one.item_embedding.detach().numpy(), p['V0'], gV, LR, rtol=1e-5, what='V')
    plain = softmax_closed_form(p['U0'], p['V0'], p['idx'], p['val'], R)[0]
    assert rel_err(plain, loss) > 0.1                                                       # the correction means something
    uncorrected = fit(make(p, negative_sampling='popularity', sample_seed=seed), p, 1)
    assert rel_err(uncorrected.loss_history_[0], plain / n_pos) < 1e-5 and uncorrected.sample_log_q_ is None
    many = fit(make(p, negative_sampling='popularity', sampling_correction='logq', sample_seed=seed, resample_every=1), p, 6)
    h = many.loss_history_
    assert h[0] == one.loss_history_[0] and many.resample_rounds_ == 6 and h[-1] < h[0]
    again = fit(many, p, 1)                                                                 # a second fit of the model: round 0 again
    assert same_fit(again, one)
    again.sampling_correction = 'none'                                                     # and a later fit without the setting
    assert same_fit(fit(again, p, 1), uncorrected) and again.sample_log_q_ is None


def test_a_subclass_is_corrected_in_the_generic_loop(no_gpu):
    from teamoflow_amd.mf.loss_graphs import SampledSoftmaxLoss

    class MySoftmax(SampledSoftmaxLoss):
        pass
    p = bpr_problem(14, 30, 20, 4, 8)
    a = fit(make(p, MySoftmax(), negative_sampling='popularity', sampling_correction='logq'), p, 2)
    b = fit(make(p, negative_sampling='popularity', sampling_correction='logq'), p, 2)
    assert same_fit(a, b) and not same_fit(a, fit(make(p, MySoftmax(), negative_sampling='popularity'), p, 2))


def test_under_uniform_tables_the_fit_is_catalog_scale(no_gpu, monkeypatch):
    """l is the constant log(S / n_items): the fit is SampledSoftmaxLoss(catalog_scale=True) bit for bit, and no offsets exist."""
    from teamoflow_amd.mf import utils
    from teamoflow_amd.mf import matrix_factorization as M
    from teamoflow_amd.mf.loss_graphs import SampledSoftmaxLoss
    p = bpr_problem(14, 30, 20, 4, 8)
    scaled = fit(make(p, SampledSoftmaxLoss(True)), p, 3)
    monkeypatch.setattr(M, 'log_expected_count', lambda *a, **k: pytest.fail('no table of offsets under uniform sampling'))
    model = make(p, sampling_correction='logq')
    logq = fit(model, p, 3)
    assert same_fit(logq, scaled) and logq.sample_log_q_ is None
    assert model.loss_graph.catalog_scale is False                                          # the model's own loss is not touched
    assert not same_fit(logq, fit(make(p), p, 3))
    fresh = fit(make(p, SampledSoftmaxLoss(True), resample_every=1, sample_seed=3), p, 3)   # and with a table per epoch
    assert same_fit(fit(make(p, sampling_correction='logq', resample_every=1, sample_seed=3), p, 3), fresh)
    assert utils.log_expected_count(torch.ones(20, dtype=torch.int64), 8)[0] == np.float32(math.log(8 / 20))


def test_a_loss_without_a_table_ignores_the_setting(no_gpu):
    from teamoflow_amd.mf import loss_graphs as L
    p = bpr_problem(14, 30, 20, 4, 8)
    for loss in (L.LogisticLoss, L.FullSoftmaxLoss):       # (unbiased MSE has no fit without a GPU)
        a, b = fit(make(p, loss(), sampling_correction='logq', negative_sampling='popularity'), p, 2), fit(make(p, loss()), p, 2)
        assert same_fit(a, b) and a.sample_log_q_ is None


# ------------------------------------------------------------------------------------------------------------------------
# the refusals
# ------------------------------------------------------------------------------------------------------------------------
class _Spy:
    def __init__(self):
        self.calls = 0

    def initialize_weights(self, n_features, n_components):
        self.calls += 1
        return torch.zeros(n_features, n_components)


@pytest.mark.parametrize('gpu', [False, True], ids=['cpu', 'gpu'])
def test_every_refusal_comes_before_anything_is_drawn(monkeypatch, gpu):
    from teamoflow_amd import _engine, _ops
    from teamoflow_amd.mf import loss_graphs as L
    from teamoflow_amd.mf import matrix_factorization as M
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: gpu)
    monkeypatch.setattr(_ops, 'sample_negatives', lambda *a, **k: pytest.fail('nothing may be drawn'))
    monkeypatch.setattr(M, 'popularity_weights', lambda *a, **k: pytest.fail('no weights may be made'))
    monkeypatch.setattr(M, 'log_expected_count', lambda *a, **k: pytest.fail('no offsets may be made'))
    monkeypatch.setattr(_engine, 'InteractionPlan', lambda *a, **k: pytest.fail('a plan was built'))
    for name in ('_fit_sparse', '_fit_generic'):
        monkeypatch.setattr(M.MatrixFactorization, name, lambda self, *a, **k: pytest.fail('a fit was started'))
    p = bpr_problem(17, 12, 9, 4, 4)

    def refused(error, match, loss=None, **attrs):
        spy = _Spy()
        with pytest.raises(error, match=match) as e:
            fit(make(p, loss, init=spy, **attrs), p, 1)
        assert spy.calls == 0, attrs
        return str(e.value)

    class MyWMRB(L.WMRBLoss):
        pass

    class MySoftmax(L.SampledSoftmaxLoss):
        pass
    for sampling in ('uniform', 'popularity'):
        for bad in ('logQ', 'log_q', '', None, True, 1):                                  # any other value, on every model
            refused(ValueError, 'sampling_correction', sampling_correction=bad, negative_sampling=sampling)
            refused(ValueError, 'sampling_correction', L.MSELoss(), sampling_correction=bad, negative_sampling=sampling)
        for loss in (L.SampledSoftmaxLoss(True), L.SampledSoftmaxLoss(catalog_scale=1)):
            refused(ValueError, r"sampling_correction='logq' with SampledSoftmaxLoss\(catalog_scale=True\)", loss,
                    sampling_correction='logq', negative_sampling=sampling)
        for loss in (L.WMRBLoss(), L.BPRLoss(), L.WARPLoss(), L.KOSWARPLoss(), MyWMRB()):
            text = refused(NotImplementedError, f"sampling_correction='logq' with {type(loss).__name__}", loss,
                           sampling_correction='logq', negative_sampling=sampling)
            assert 'SampledSoftmaxLoss' in text and 'back to its default' in text
    # the forms that draw their tables themselves, refused where 'popularity' is
    for named, loss, attrs in (('batch_users', None, dict(batch_users=8)), ('shard_items', None, dict(shard_items=2)),
                               ('data_parallel', None, dict(data_parallel=True)), ('data_parallel', None, dict(data_parallel='force')),
                               ('batch_users', MySoftmax(), dict(batch_users=8)), ('shard_items', MySoftmax(), dict(shard_items=2))):
        text = refused(NotImplementedError, "sampling_correction='logq' with " + named, loss, sampling_correction='logq', **attrs)
        assert 'back to its default' in text
        refused(NotImplementedError, "negative_sampling='popularity' with " + named, loss, sampling_correction='logq',
                negative_sampling='popularity', **attrs)                                   # that setting's refusal still comes first


def test_the_table_of_the_refusals():
    from teamoflow_amd.mf import matrix_factorization as Mf
    row = Mf.CORRECTION_ROUTES['logq']
    assert list(Mf.CORRECTION_ROUTES) == ['logq'] and list(row) == list(Mf._SETTINGS) and Mf.SAMPLING_CORRECTION == ('none', 'logq')
    assert row == Mf.SAMPLING_ROUTES['popularity'] and row is not Mf.SAMPLING_ROUTES['popularity']     # refused exactly where it is
    assert 'logq' not in Mf.ROUTES and len(Mf.ROUTES) == 7 and list(Mf.SAMPLING_ROUTES) == ['popularity']
    with open(os.path.join(ROOT, 'DESIGN.md')) as f:
        design = f.read()
    head = ['feature \\ setting'] + list(Mf._SETTINGS)
    printed = '\n'.join('| ' + ' | '.join(cells) + ' |' for cells in (head, ['---'] * len(head), ['`logq`'] + list(row.values())))
    assert '\n\n' + printed + '\n\n' in design, 'DESIGN.md, "What trains where", should print:\n' + printed


def test_the_correction_is_no_record_of_the_loss_table():
    from teamoflow_amd import _engine
    assert not any('logq' in name or 'offset' in name for name in _engine.LOSSES)
    assert _engine.LOSSES['softmax'].pair_step is _engine.softmax_pairs and _engine.LOSSES['softmax'].plan_needs == ()


def test_the_offsets_of_a_plan_follow_its_slot_order():
    """WmrbPlan.slot_offsets on a plan built from CPU tensors: off[u, s] = l[R[u, s]] in the plan's (item-sorted) order, built once,
    noted in ``prepared``, dropped by release."""
    from teamoflow_amd import _engine
    p = bpr_problem(3, 12, 9, 4, 5)
    plan = _engine.InteractionPlan(torch.as_tensor(p['idx']), torch.as_tensor(p['val']), 12, 9, user_chunks=1, csc=False)
    w = _engine.WmrbPlan(plan, torch.as_tensor(p['R']), sliced=True)
    assert w.off is None and w.prepared == []
    ell = torch.linspace(-3.0, 0.0, 9)
    off = w.slot_offsets(ell)
    assert off.dtype == torch.float32 and torch.equal(off, ell[w.R.long()]) and w.slot_offsets(ell) is off and w.off is off
    assert [name for name, _ in w.prepared] == ['slot_offsets'] and torch.equal(w.prepared[0][1][0], ell)
    assert torch.equal(torch.sort(off, dim=1)[0], torch.sort(ell[torch.as_tensor(p['R']).long()], dim=1)[0])
    with pytest.raises(ValueError, match='slot_offsets'):
        _engine.WmrbPlan(plan, torch.as_tensor(p['R']), sliced=True).slot_offsets(ell[:8])
    w.release()
    assert w.off is None


# ------------------------------------------------------------------------------------------------------------------------
# save / load
# ------------------------------------------------------------------------------------------------------------------------
def test_save_and_load_keep_the_setting(no_gpu, tmp_path):
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    p = bpr_problem(18, 30, 20, 4, 8)
    model = fit(make(p, negative_sampling='popularity', sampling_correction='logq', sample_seed=4), p, 2)
    path = str(tmp_path / 'model.pt')
    model.save(path)
    blob = torch.load(path, weights_only=True)
    assert blob['sampling_correction'] == 'logq'
    back = MatrixFactorization.load(path, device='cpu')
    assert (back.sampling_correction, back.negative_sampling, back.sample_seed) == ('logq', 'popularity', 4)
    assert same_fit(fit(back, p, 2), model) and torch.equal(back.sample_log_q_, model.sample_log_q_)
    del blob['sampling_correction']                                                # a file written before the attribute existed
    torch.save(blob, str(tmp_path / 'old.pt'))
    assert MatrixFactorization.load(str(tmp_path / 'old.pt'), device='cpu').sampling_correction == 'none'
    plain, bare = fit(make(p), p, 1), fit(make(p), p, 1)
    del bare.sampling_correction, bare.sample_log_q_                               # a model from before the attribute
    plain.save(str(tmp_path / 'plain.pt'))
    bare.save(str(tmp_path / 'bare.pt'))
    a, b = (torch.load(str(tmp_path / name), weights_only=True) for name in ('plain.pt', 'bare.pt'))
    assert 'sampling_correction' not in a and list(a) == list(b)                   # the default blob gains no key
    assert same_fit(fit(bare, p, 1), plain)


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_built():
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    declared = set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    lib, sig = _lib.load_library(), _lib.SIGNATURES
    for name in ('tmf_softmax_pairs_offset', 'tmf_slot_offsets'):
        assert name in declared and name in sig and hasattr(lib, name)
    plain, offset = sig['tmf_softmax_pairs'], sig['tmf_softmax_pairs_offset']
    assert plain == sig['tmf_wmrb_hinge2_ordered']                                  # the plain step keeps its prototype
    assert offset[0] is plain[0] and offset[1] == plain[1][:4] + [plain[1][3]] + plain[1][4:]   # one more fp32 stream behind sp
    source = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'tmf_softmax.hip')).read()
    assert 'k_softmax_pairs<false>' in source and 'k_softmax_pairs<true>' in source and source.count('void k_softmax_pairs(') == 1


def test_argument_checks_fail_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail differently; these return first."""
    from teamoflow_amd import _lib
    lib = _lib.load_library()
    host = (ctypes.c_double * 8)()              # stands for any non-null buffer: never dereferenced
    H, i32, i64 = ctypes.cast(host, ctypes.c_void_p), ctypes.c_int32, ctypes.c_int64
    assert lib.tmf_softmax_pairs_offset(None, None, None, None, None, i32(0), i32(8), 1.0, None, None, None, None, None) == 0
    for args in ((H, H, H, H, None, i32(3), i32(8), 1.0, H, H, H),                 # null off
                 (None, H, H, H, H, i32(3), i32(8), 1.0, H, H, H), (H, H, H, None, H, i32(3), i32(8), 1.0, H, H, H),
                 (H, H, H, H, H, i32(3), i32(8), 1.0, H, None, H), (H, H, H, H, H, i32(3), i32(0), 1.0, H, H, H),
                 (H, H, H, H, H, i32(-1), i32(8), 1.0, H, H, H), (H, H, H, H, H, i32(0), i32(-8), 1.0, H, H, H)):
        assert lib.tmf_softmax_pairs_offset(*args, None, None) == -1 and 'softmax_pairs_offset' in lib.tmf_last_error().decode()
    for users, samples in ((0, 8), (3, 0), (0, 0)):                                # nothing to fill: no launch
        assert lib.tmf_slot_offsets(None, i32(0), None, i64(users), i32(samples), None, None) == 0
    for args in ((None, i32(5), H, i64(3), i32(8), H),                             # null ell
                 (H, i32(5), None, i64(3), i32(8), H), (H, i32(5), H, i64(3), i32(8), None), (H, i32(0), H, i64(3), i32(8), H),
                 (H, i32(-5), H, i64(3), i32(8), H), (H, i32(5), H, i64(-3), i32(8), H), (H, i32(5), H, i64(3), i32(-8), H)):
        assert lib.tmf_slot_offsets(*args, None) == -1 and 'slot_offsets' in lib.tmf_last_error().decode()
