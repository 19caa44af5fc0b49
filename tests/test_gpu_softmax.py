"""SampledSoftmaxLoss on the sparse HIP engine (tmf_softmax_pairs, _engine.epoch_wmrb(pairs='softmax')) against the NumPy fp64 closed
form of tests/test_softmax_cpu.py, which that file pins to the plug-in's own get_loss and whose fp32 restatement in the kernel's
order of additions it shows to meet the tolerances used here, on the same inputs: rel_err < 1e-5 for delta, D, the loss and the raw
gradients, the sum identity |sum_s D[u, s] + sum_k delta_k| <= 1e-5 sum_k |delta_k|, assert_step(rtol=1e-5) for the tables after
one step (the project's own tolerances, tests/test_gpu_bpr.py)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_step, rel_err, step_bounds
from test_bpr_cpu import KERNEL_DEGREES, LR, MAGNITUDES, bpr_problem, kernel_case
from test_softmax_cpu import KERNEL_C, KERNEL_S, SM_CAP, softmax_closed_form, softmax_pairs_ref, sum_identity_gaps

pytestmark = pytest.mark.gpu
NAN = float('nan')
C_IDS = ['c=1', 'c=n/S']


@pytest.fixture(scope='module')
def tm():
    from teamoflow_amd import _engine, _lib, _ops
    from teamoflow_amd.mf import embedding_graphs as EG
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import SampledSoftmaxLoss, WMRBLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization, SampleTableMissing
    from teamoflow_amd.mf.sparse import SparseFeatures, SparseInteractions, eye, hstack_identity
    lib = _lib.get()

    class NS:
        pass
    ns = NS()
    ns.lib, ns.L, ns.E, ns.ops, ns.EG, ns.MF, ns.Fixed, ns.SM, ns.WMRB, ns.Sparse, ns.SF, ns.eye, ns.hstack, ns.Missing = lib, _lib, _engine, \
        _ops, EG, MatrixFactorization, FixedInitializer, SampledSoftmaxLoss, WMRBLoss, SparseInteractions, SparseFeatures, eye, \
        hstack_identity, SampleTableMissing
    return ns


@pytest.fixture
def engine_only(tm, monkeypatch):
    """_fit_generic refuses to run: a fit that passes ran on the engine."""
    def refuse(self, *a, **k):
        raise AssertionError('_fit_generic was called')
    monkeypatch.setattr(tm.MF, '_fit_generic', refuse)


# ------------------------------------------------------------------------------------------------------------------------
# the kernel alone
# ------------------------------------------------------------------------------------------------------------------------
def run_kernel(tm, rowptr, val, p, sp, c=1.0, order=None):
    """tmf_softmax_pairs on host arrays, every output pre-filled with NaN -> (delta, D, loss_part) as NumPy.  A table without entries
    passes NULL for val, p and delta (the pointer of an empty tensor)."""
    dev, P = torch.device('cuda'), tm.L.ptr
    m, S = sp.shape
    d_rowptr = torch.as_tensor(np.asarray(rowptr, np.int64), device=dev)
    d_val, d_p, d_sp = (torch.as_tensor(np.asarray(x, np.float32), device=dev).contiguous() for x in (val, p, sp))
    delta = torch.full((d_val.numel(),), NAN, device=dev)
    D = torch.full((m, S), NAN, device=dev)
    loss = torch.full((m,), NAN, device=dev)
    d_order = None if order is None else torch.as_tensor(np.asarray(order, np.int32), device=dev)
    entries = [P(x) if x.numel() else None for x in (d_val, d_p, delta)]
    tm.L.check(tm.lib.tmf_softmax_pairs(P(d_rowptr), entries[0], entries[1], P(d_sp), ctypes.c_int32(m), ctypes.c_int32(S), float(c),
                                        entries[2], P(D), P(loss), P(d_order), tm.L.stream_ptr()), tm.lib)
    torch.cuda.synchronize()
    return delta.cpu().numpy(), D.cpu().numpy(), loss.cpu().numpy()


def assert_bits(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def assert_sum_identity(rowptr, val, delta, D):
    gaps = sum_identity_gaps(rowptr, val, delta, D)
    worst = max(gap / size for gap, size in gaps)
    assert all(gap <= 1e-5 * size for gap, size in gaps), worst
    return worst


_CASE_REFS = {}


def case_and_reference(S, c):
    """kernel_case(S) and its fp64 outputs, computed once and left unchanged."""
    if (S, c) not in _CASE_REFS:
        case = kernel_case(S)
        ref = softmax_pairs_ref(*case, c)
        for a in ref:
            a.setflags(write=False)
        _CASE_REFS[S, c] = case, ref
    return _CASE_REFS[S, c]


@pytest.mark.parametrize('c', KERNEL_C, ids=C_IDS)
@pytest.mark.parametrize('S', KERNEL_S)
def test_kernel_against_fp64(tm, S, c):
    """67 users with 0, 1, 2, 31, 32, 33, 64, 65 and 131 positives (a pass is 64 stored interactions), one with only values <= 0 and
    one of mixed signs; S below, at and above the lane count, around half a tile, one below, at and one above the register-resident
    1024 samples, and over two tiles."""
    assert {SM_CAP - 1, SM_CAP, SM_CAP + 1} <= set(KERNEL_S) and set(KERNEL_DEGREES) == {0, 1, 2, 31, 32, 33, 64, 65, 131, 5, 40}
    case, ref = case_and_reference(S, c)
    rowptr, val = case[0], case[1]
    got = run_kernel(tm, *case, c)
    assert all(np.isfinite(g).all() for g in got)                     # no NaN left anywhere: every element was written
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    delta, D, loss = got
    worst = assert_sum_identity(rowptr, val, delta, D)
    print(f'[kernel] S={S} c={c:.4g}: delta {errs[0]:.3g} D {errs[1]:.3g} loss {errs[2]:.3g} identity {worst:.3g}')
    assert max(errs) < 1e-5, errs
    assert not delta[val <= 0].any() and (val <= 0).sum() > 50 and (delta[val > 0] < 0).all()
    no_pos = np.array([not (val[rowptr[u]:rowptr[u + 1]] > 0).any() for u in range(67)])
    assert no_pos.sum() >= 12 and not D[no_pos].any() and not loss[no_pos].any() and (D[~no_pos] > 0).all()
    assert_bits(run_kernel(tm, *case, c), got)                                                          # a second call
    assert_bits(run_kernel(tm, *case, c, order=np.random.default_rng(S).permutation(67)), got)          # a permuted user order
    assert_bits(run_kernel(tm, *case, c, order=np.arange(67)[::-1].copy()), got)


def test_kernel_on_tables_without_users_or_entries(tm):
    empty = np.zeros(0, np.float32)
    got = run_kernel(tm, np.zeros(1, np.int64), empty, empty, np.zeros((0, 65), np.float32))          # n_users = 0
    assert [g.shape for g in got] == [(0,), (0, 65), (0,)]
    case = kernel_case(65, n_users=1)                                                                # one user, nothing stored
    assert case[0].tolist() == [0, 0]
    delta, D, loss = run_kernel(tm, *case)                                                           # nnz = 0: NULL val / p / delta
    assert delta.shape == (0,) and not D.any() and not loss.any()
    rowptr = np.array([0, 3], np.int64)                                                              # one user with entries
    val, p, sp = np.array([2, -1, 1], np.float32), np.array([0.5, 9.0, -0.25], np.float32), np.linspace(-2, 2, 65, dtype=np.float32)[None]
    for c in KERNEL_C:
        got, ref = run_kernel(tm, rowptr, val, p, sp, c), softmax_pairs_ref(rowptr, val, p, sp, c)
        assert max(rel_err(g, r) for g, r in zip(got, ref)) < 1e-5 and got[0][1] == 0.0
    case = kernel_case(65, n_users=3)                                                                # users with 0, 1 and 2 entries
    got, ref = run_kernel(tm, *case), softmax_pairs_ref(*case)
    assert max(rel_err(g, r) for g, r in zip(got, ref)) < 1e-5


@pytest.mark.parametrize('c', KERNEL_C, ids=C_IDS)
def test_kernel_at_every_magnitude(tm, c):
    """Scores of magnitude 0, 1e-3, 30, 88 and 1e4 with both signs, one magnitude per user and all of them mixed inside a user."""
    case = kernel_case(65, scale=MAGNITUDES)
    got, ref = run_kernel(tm, *case, c), softmax_pairs_ref(*case, c)
    assert all(np.isfinite(g).all() for g in got) and all(np.isfinite(r).all() for r in ref)
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    print(f'[kernel] magnitudes c={c:.4g}: delta {errs[0]:.3g} D {errs[1]:.3g} loss {errs[2]:.3g}')
    assert max(errs) < 1e-5, errs
    assert_sum_identity(case[0], case[1], got[0], got[1])
    # and user by user for the loss, whose sizes differ by orders of magnitude between the users
    rowptr, val = case[0], case[1]
    for u in range(67):
        if (val[rowptr[u]:rowptr[u + 1]] > 0).any():
            assert rel_err(got[2][u], ref[2][u]) < 1e-5, (u, MAGNITUDES[u % len(MAGNITUDES)])


def test_a_positive_far_above_every_sample(tm):
    """One user with p = +30 and sp near -30: 1 + b is 1 in fp32; the loss is b > 0 all the same, within 1e-5 of fp64."""
    rowptr, val, p = np.array([0, 1], np.int64), np.array([1.0], np.float32), np.array([30.0], np.float32)
    sp = (-30 + 0.1 * np.random.default_rng(0).standard_normal((1, 65))).astype(np.float32)
    got, ref = run_kernel(tm, rowptr, val, p, sp), softmax_pairs_ref(rowptr, val, p, sp)
    print(f'[kernel] far apart: loss {got[2][0]!r} against {ref[2][0]!r}')
    assert 0 < ref[2][0] < 1e-20 and got[2][0] > 0 and got[0][0] < 0 and (got[1] > 0).all()
    assert max(rel_err(g, r) for g, r in zip(got, ref)) < 1e-5


def test_non_finite_scores_stay_inside_their_user(tm):
    """A NaN sample in one user and an infinite p_k in another: every other user's outputs keep their bits."""
    rowptr, val, p, sp = kernel_case(65, n_users=12)
    a, b = 5, 8                                                # 33 and 131 positives
    assert rowptr[a + 1] - rowptr[a] == 33 and rowptr[b + 1] - rowptr[b] == 131 and (val[rowptr[b]:rowptr[b + 1]] > 0).all()
    clean = run_kernel(tm, rowptr, val, p, sp)
    sp2, p2 = sp.copy(), p.copy()
    sp2[a, 20] = np.nan
    p2[rowptr[b] + 70] = np.inf
    delta, D, loss = run_kernel(tm, rowptr, val, p2, sp2)
    others = ~np.isin(np.arange(12), (a, b))
    ent = np.ones(val.shape[0], bool)
    ent[rowptr[a]:rowptr[a + 1]] = ent[rowptr[b]:rowptr[b + 1]] = False
    assert_bits((delta[ent], D[others], loss[others]), (clean[0][ent], clean[1][others], clean[2][others]))
    assert np.isfinite(delta[ent]).all() and np.isfinite(D[others]).all() and np.isfinite(loss[others]).all()
    assert not np.isfinite(loss[a]) and not np.isfinite(loss[b])        # nothing was silently dropped either


# ------------------------------------------------------------------------------------------------------------------------
# one step through the public API
# ------------------------------------------------------------------------------------------------------------------------
def fit_softmax(tm, p, epochs, U0=None, V0=None, loss=None, lr=LR, item_features=None, table=True, **attrs):
    U0, V0 = (p['U0'] if U0 is None else U0), (p['V0'] if V0 is None else V0)
    graphs = {k: attrs.pop(k) for k in ('user_repr_graph', 'item_repr_graph') if k in attrs}
    model = tm.MF(p['r'], loss_graph=loss or tm.SM(), user_weight_graph=tm.Fixed(U0), item_weight_graph=tm.Fixed(V0), n_users=p['m'],
                  n_items=p['n'], n_samples=p['S'], **graphs)
    model.verbose = False
    if table:
        model.random_ind = torch.as_tensor(p['R'])
    for k, v in attrs.items():
        setattr(model, k, v)
    model.fit(epochs, tm.eye(p['m']), tm.eye(p['n']) if item_features is None else item_features,
              tm.Sparse(p['idx'], p['val'], (p['m'], p['n'])), lr=lr)
    return model


def host(t):
    return t.detach().float().cpu().numpy()


_REFS = {}


def problem_and_reference(seed, m, n, r, S, c=1.0):
    """(problem, loss mean, gU, gV): the fp64 closed form of a shape, computed once and left unchanged."""
    key = (seed, m, n, r, S, c)
    if key not in _REFS:
        p = bpr_problem(seed, m, n, r, S)
        loss, _, _, gU, gV = softmax_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'], c)
        for a in (gU, gV):
            a.setflags(write=False)
        _REFS[key] = (p, loss / int((p['val'] > 0).sum()), gU, gV)
    return _REFS[key]


def check_one_step(tm, seed, r, S, what='', m=60, n=40, catalog_scale=False, **attrs):
    p, loss, gU, gV = problem_and_reference(seed, m, n, r, S, n / S if catalog_scale else 1.0)
    model = fit_softmax(tm, p, 1, loss=tm.SM(catalog_scale), **attrs)
    st = model._state
    assert st.wplan.sliced and st.plan.n_pos == int((p['val'] > 0).sum()), 'the fit did not take the sliced user pass'
    err = rel_err(model.loss_history_[0], loss)
    print(f'[one step] {what}: loss {err:.3g}')
    assert err < 1e-5, what                                                    # the mean over the positives
    assert_step(host(model.user_embedding), p['U0'], gU, LR, rtol=1e-5, what=f'{what} U')
    assert_step(host(model.item_embedding), p['V0'], gV, LR, rtol=1e-5, what=f'{what} V')
    for row, W1, W0 in ((p['empty_user'], model.user_embedding, p['U0']), (p['nonpos_user'], model.user_embedding, p['U0']),
                        (p['empty_item'], model.item_embedding, p['V0'])):
        assert np.array_equal(host(W1)[row], W0[row])                          # a zero gradient: the row keeps its bits
    return model


@pytest.mark.parametrize('r,S', [(1, 5), (7, 64), (33, 70), (64, 5), (128, 64), (200, 70), (256, 5)])
def test_every_row_geometry_one_step(tm, engine_only, r, S):
    check_one_step(tm, r, r, S, f'r={r} S={S}')


@pytest.mark.parametrize('env', [{'TMF_ITEM_SLICES': '3'}, {'TMF_ROW_STATIONARY': '1'}, {'TMF_SCORES6': '1'}, {'TMF_ROWS4': '1'}],
                         ids=lambda e: '='.join(*e.items()))
def test_the_forms_of_the_user_and_item_pass_one_step(tm, engine_only, monkeypatch, env):
    """Everything around the pair step is the WMRB pass in its other forms: three item slices, the row-stationary gradU, the flat
    score streams and the row-stationary item pass (r = 128: rows of 32 lanes, which all of them have kernels for)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = 128
    st = check_one_step(tm, 128, r, 64, str(env))._state
    if 'TMF_ITEM_SLICES' in env:
        assert st.wplan.n_slices == 3
    if 'TMF_ROW_STATIONARY' in env:
        assert st.row_stationary == bool(tm.lib.tmf_wmrb_gradu4_supported(r, 0))
    if 'TMF_SCORES6' in env:
        assert (st.wplan.s6 is not None) == bool(tm.lib.tmf_wmrb_scores6_supported(r, 0, 40))
    if 'TMF_ROWS4' in env:
        assert st.wplan.rows4 == bool(tm.lib.tmf_wsum_rows4_rows_per_group(r, 0))


def test_catalog_scale_one_step(tm, engine_only):
    """c = n_items / n_samples = 40 / 5 and 40 / 64 (below 1: more samples than items is legal) - and another fit than c = 1."""
    scaled = check_one_step(tm, 64, 64, 5, 'c=8', catalog_scale=True)
    check_one_step(tm, 7, 7, 64, 'c=0.625', catalog_scale=True)
    plain = check_one_step(tm, 64, 64, 5, 'c=1')
    assert scaled.loss_history_[0] > plain.loss_history_[0] and not torch.equal(scaled.user_embedding, plain.user_embedding)


def _bf16(x):
    return torch.tensor(np.asarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def test_bf16_storage_one_step(tm, engine_only):
    """bf16 factor storage / fp32 arithmetic: against the closed form on the bf16-rounded tables; the new rows must lie in the step
    interval rounded to bf16 (tests/test_gpu_logistic.py::test_bf16_storage_one_step, its tolerances)."""
    p = bpr_problem(133, 60, 40, 33, 64)
    U0, V0 = _bf16(p['U0']), _bf16(p['V0'])
    model = fit_softmax(tm, p, 1, U0=U0, V0=V0, factor_dtype=torch.bfloat16)
    assert model.user_embedding.dtype == torch.bfloat16 and model._state.wplan.sliced
    loss, _, _, gU, gV = softmax_closed_form(U0, V0, p['idx'], p['val'], p['R'])
    assert rel_err(model.loss_history_[0], loss / int((p['val'] > 0).sum())) < 1e-5
    for got, W0, g in zip((host(model.user_embedding), host(model.item_embedding)), (U0, V0), (gU, gV)):
        lo, hi = step_bounds(W0, g, LR)
        got = got.astype(np.float64)
        assert (got >= _bf16(lo) - 1e-12).all() and (got <= _bf16(hi) + 1e-12).all()


def test_opt_in_persistent_adam(tm, engine_only):
    """optimizer='adam': the first step is the default's bit for bit; later steps follow Keras Adam with carried moments, evaluated
    in NumPy on the closed-form gradients (tests/test_gpu_logistic.py's statement and tolerance), over three epochs."""
    p = bpr_problem(8, 60, 40, 12, 20)
    a1, f1 = fit_softmax(tm, p, 1, optimizer='adam'), fit_softmax(tm, p, 1)
    assert torch.equal(a1.user_embedding, f1.user_embedding) and torch.equal(a1.item_embedding, f1.item_embedding)
    assert a1.loss_history_ == f1.loss_history_
    got = fit_softmax(tm, p, 3, optimizer='adam')
    U, V = p['U0'].astype(np.float64), p['V0'].astype(np.float64)
    mU, vU, mV, vV = (np.zeros_like(x) for x in (U, U, V, V))
    ref, n_pos = [], int((p['val'] > 0).sum())
    for t in range(1, 4):
        loss, _, _, gU, gV = softmax_closed_form(U, V, p['idx'], p['val'], p['R'])
        ref.append(loss / n_pos)
        alpha = LR * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        mU += (gU - mU) * 0.1
        vU += (gU ** 2 - vU) * 0.001
        mV += (gV - mV) * 0.1
        vV += (gV ** 2 - vV) * 0.001
        U = U - alpha * mU / (np.sqrt(vU) + 1e-7)
        V = V - alpha * mV / (np.sqrt(vV) + 1e-7)
    assert rel_err(got.loss_history_, ref) < 1e-4
    assert np.abs(host(got.user_embedding) - U).max() < 1e-3 and np.abs(host(got.item_embedding) - V).max() < 1e-3


def test_biased_item_side_one_step(tm, engine_only):
    """A bias starts at zero, so the effective tables are the weights and their gradients the closed form's.  The item bias moves
    every score of a user alike and cancels in the softmax (as under WMRB, tests/test_biased_cpu.py): its gradient is rounding noise,
    so neither it nor the item embedding that carries it is compared."""
    p, loss, gU, gV = problem_and_reference(1033, 60, 40, 33, 64)
    model = fit_softmax(tm, p, 1, item_repr_graph=tm.EG.BiasedLinearEmbedding())
    st = model._state
    assert st.bias_v is not None and st.bias_u is None and st.wplan.sliced
    assert rel_err(model.loss_history_[0], loss) < 1e-5
    assert_step(host(model.user_embedding), p['U0'], gU, LR, rtol=1e-5, what='biased item side: U')
    assert len(model.item_trainable) == 2 and model.item_trainable[1] is model.item_linear_bias
    assert_step(host(model.item_trainable[0]), p['V0'], gV, LR, rtol=1e-5, what='biased item side: item weights')
    assert torch.equal(model.item_embedding, model.item_trainable[0] + model.item_linear_bias.detach())


def test_item_side_over_sparse_features_one_step(tm, engine_only):
    """F = [I | tags] (hstack_identity): E = F W, dL/dW = F^T dL/dE with dL/dE the closed form on (U, E); every row's gradient
    agrees to 1e-5, so feature f's sum may be off by 1e-5 sum_i |x_if| |dL/dE[i]| (tests/test_gpu_features.py)."""
    from test_gpu_features import assert_step_with_slack
    m, n, r, S, T = 60, 40, 33, 64, 6
    p = bpr_problem(2033, m, n, r, S)
    rng = np.random.default_rng(5)
    tag_mask = rng.random((n, T)) < 0.3
    tag_idx = np.argwhere(tag_mask)
    tag_val = rng.choice(np.array([1.0, 0.5, -0.25, 2.0], np.float32), tag_idx.shape[0])
    F = tm.hstack(n, tm.SF(tag_idx, tag_val, (n, T)))
    F_dense = np.zeros((n, n + T))
    F_dense[np.arange(n), np.arange(n)] = 1.0
    F_dense[tag_idx[:, 0], n + tag_idx[:, 1]] = tag_val
    assert torch.equal(F.to_dense().cpu(), torch.tensor(F_dense, dtype=torch.float32))
    W0 = (rng.standard_normal((n + T, r)) * 0.3).astype(np.float32)
    model = fit_softmax(tm, p, 1, V0=W0, item_features=F)
    E0 = F_dense @ W0.astype(np.float64)
    loss, _, _, gU, gE = softmax_closed_form(p['U0'], E0, p['idx'], p['val'], p['R'])
    st = model._state
    assert st.feat_v is not None and st.feat_u is None and st.wplan.sliced
    assert rel_err(model.loss_history_[0], loss / int((p['val'] > 0).sum())) < 1e-5
    assert_step(host(model.user_embedding), p['U0'], gU, LR, rtol=1e-5, what='user table')
    slack = 1e-5 * np.abs(F_dense).T @ np.abs(gE)
    assert_step_with_slack(host(model.item_trainable[0]), W0, F_dense.T @ gE, slack, LR, 'softmax item weights over sparse features')
    assert model.item_embedding.shape == (n, r) and torch.equal(model.item_embedding, model.embed_items(F))


def test_no_sample_table_on_the_engine(tm, engine_only):
    p = bpr_problem(15, 12, 9, 4, 4)
    with pytest.raises(tm.Missing, match='SampledSoftmaxLoss'):
        fit_softmax(tm, p, 1, table=False)


# ------------------------------------------------------------------------------------------------------------------------
# trajectory, replay, no leakage, resampling
# ------------------------------------------------------------------------------------------------------------------------
def fresh_adam_fp64(W, g, lr):
    """conftest.step_bounds' step: the reference's first Adam step with its fp32 constants, evaluated in fp64."""
    f = np.float32
    omb1, omb2, eps = float(f(1) - f(0.9)), float(f(1) - f(0.999)), float(f(1e-7))
    alpha = float(f(f(lr) * np.sqrt(f(f(1) - f(0.999))) / f(f(1) - f(0.9))))
    return W - (g * omb1 * alpha) / (np.sqrt(g * g * omb2) + eps)


def test_trajectory_and_graph_replay(tm, engine_only, monkeypatch):
    """200 x 150, r = 16, S = 32: ten epochs - one replay of a ten-epoch hipGraph - against ten closed-form steps in fp64, epoch by
    epoch.  TMF_NO_GRAPH=1 gives the same bits."""
    p = bpr_problem(6, 200, 150, 16, 32)
    n_pos = int((p['val'] > 0).sum())
    U, V, ref = p['U0'].astype(np.float64), p['V0'].astype(np.float64), []
    for _ in range(10):
        loss, _, _, gU, gV = softmax_closed_form(U, V, p['idx'], p['val'], p['R'])
        ref.append(loss / n_pos)
        U, V = fresh_adam_fp64(U, gU, LR), fresh_adam_fp64(V, gV, LR)
    monkeypatch.delenv('TMF_NO_GRAPH', raising=False)
    a = fit_softmax(tm, p, 10)
    monkeypatch.setenv('TMF_NO_GRAPH', '1')
    b = fit_softmax(tm, p, 10)
    assert a.loss_history_ == b.loss_history_ and len(a.loss_history_) == 10
    assert torch.equal(a.user_embedding, b.user_embedding) and torch.equal(a.item_embedding, b.item_embedding)
    errs = [abs(h - r) / r for h, r in zip(a.loss_history_, ref)]
    print(f'[trajectory] per epoch: {" ".join(f"{e:.2g}" for e in errs)}')
    assert max(errs) < 1e-5 and a.loss_history_[-1] < a.loss_history_[0]


def test_a_softmax_fit_leaves_nothing_behind_for_wmrb(tm, engine_only):
    p = bpr_problem(9, 60, 40, 33, 20)
    alone = fit_softmax(tm, p, 3, loss=tm.WMRB())
    model = fit_softmax(tm, p, 3)                                              # then a WMRB fit on the same model
    softmax_history, softmax_U = list(model.loss_history_), model.user_embedding.clone()
    model.loss_graph = tm.WMRB()
    model.fit(3, tm.eye(p['m']), tm.eye(p['n']), tm.Sparse(p['idx'], p['val'], (p['m'], p['n'])), lr=LR)
    assert model.loss_history_ == alone.loss_history_ and alone.loss_history_ != softmax_history
    assert torch.equal(model.user_embedding, alone.user_embedding) and torch.equal(model.item_embedding, alone.item_embedding)
    assert not torch.equal(alone.user_embedding, softmax_U)


def test_resample_every_is_three_one_epoch_fits(tm, engine_only):
    """resample_every=1 over three epochs = one epoch on random_ind, one on the table _ops.sample_negatives draws for seed + 1, one
    on seed + 2's, each from the tables the one before left: bit for bit (tests/test_gpu_resample.py's construction)."""
    p, seed = bpr_problem(4, 200, 150, 16, 32), 21
    whole = fit_softmax(tm, p, 3, resample_every=1, sample_seed=seed)
    assert whole.resample_rounds_ == 3 and torch.equal(torch.as_tensor(whole.random_ind), torch.as_tensor(p['R']))
    chain = fit_softmax(tm, p, 1)
    history = list(chain.loss_history_)
    for j in (1, 2):
        U, V = host(chain.user_embedding).copy(), host(chain.item_embedding).copy()
        chain.user_weight_graph, chain.item_weight_graph = tm.Fixed(U), tm.Fixed(V)
        chain.random_ind = tm.ops.sample_negatives(p['n'], p['m'], p['S'], seed=seed + j, device='cuda')
        chain.fit(1, tm.eye(p['m']), tm.eye(p['n']), tm.Sparse(p['idx'], p['val'], (p['m'], p['n'])), lr=LR)
        assert chain.resample_rounds_ == 1
        history += chain.loss_history_
    assert whole.loss_history_ == history
    assert torch.equal(whole.user_embedding, chain.user_embedding) and torch.equal(whole.item_embedding, chain.item_embedding)
    static = fit_softmax(tm, p, 3)
    assert static.loss_history_[0] == whole.loss_history_[0] and static.loss_history_[1:] != whole.loss_history_[1:]
