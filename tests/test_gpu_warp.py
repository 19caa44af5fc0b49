"""WARPLoss on the sparse HIP engine (tmf_warp_pairs, _engine.epoch_wmrb(pairs='warp')) against the NumPy reference of
tests/test_warp_cpu.py - a linear scan per positive, values in fp64 -, which that file pins to the plug-in's own get_loss and whose
fp32 restatement in the kernel's order of additions it shows to meet what is asked here on the same inputs: the reference's first
violators exactly (the non-zero pattern of D), rel_err < 1e-5 for delta, D and the loss, assert_step(rtol=1e-5) for the tables
after one step.  One step through fit() is compared with the fp64 closed form only on *decided* problems (no comparison within fp32
reach of its threshold: test_warp_cpu.decidedness), asserted again here before any engine call."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_step, rel_err, step_bounds
from test_warp_cpu import (ADAM_PROBLEM, BF16_PROBLEM, BIASED_PROBLEM, GEOMETRY_PROBLEMS, KERNEL_S, L2_PROBLEM, LR, REPLAY_PROBLEM,
                           SMALL_CATALOG_PROBLEM, bf16_round, decidedness, features_problem, kernel_case,
                           kernel_n_items, warp_closed_form, warp_pairs_ref, warp_problem)

pytestmark = pytest.mark.gpu
NAN = float('nan')


@pytest.fixture(scope='module')
def tm():
    from teamoflow_amd import _engine, _lib
    from teamoflow_amd.mf import embedding_graphs as EG
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import BPRLoss, WARPLoss, WMRBLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization, SampleTableMissing
    from teamoflow_amd.mf.sparse import SparseFeatures, SparseInteractions, eye, hstack_identity
    lib = _lib.get()

    class NS:
        pass
    ns = NS()
    ns.lib, ns.L, ns.E, ns.EG, ns.MF, ns.Fixed, ns.WARP, ns.BPR, ns.WMRB, ns.Sparse, ns.SF, ns.eye, ns.hstack, ns.Missing = lib, _lib, _engine, \
        EG, MatrixFactorization, FixedInitializer, WARPLoss, BPRLoss, WMRBLoss, SparseInteractions, SparseFeatures, eye, hstack_identity, \
        SampleTableMissing
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
def run_kernel(tm, rowptr, val, p, sp, n_items, order=None, rank=None):
    """tmf_warp_pairs on host arrays, every output pre-filled with NaN -> (delta, D, loss_part) as NumPy.  A table without entries
    passes NULL for val, p and delta (the pointer of an empty tensor).  rank [m, S]: tmf_warp_pairs_ranked - sp and D in another
    order than the table's, rank[u, pos] the table index of the sample at place pos."""
    dev, P = torch.device('cuda'), tm.L.ptr
    m, S = sp.shape
    d_rowptr = torch.as_tensor(np.asarray(rowptr, np.int64), device=dev)
    d_val, d_p, d_sp = (torch.as_tensor(np.asarray(x, np.float32), device=dev).contiguous() for x in (val, p, sp))
    delta = torch.full((d_val.numel(),), NAN, device=dev)
    D = torch.full((m, S), NAN, device=dev)
    loss = torch.full((m,), NAN, device=dev)
    d_order = None if order is None else torch.as_tensor(np.asarray(order, np.int32), device=dev)
    entries = [P(x) if x.numel() else None for x in (d_val, d_p, delta)]
    i32 = ctypes.c_int32
    if rank is None:
        tm.L.check(tm.lib.tmf_warp_pairs(P(d_rowptr), entries[0], entries[1], P(d_sp), i32(m), i32(S), i32(n_items), entries[2], P(D), P(loss),
                                         P(d_order), tm.L.stream_ptr()), tm.lib)
    else:
        d_rank = torch.as_tensor(np.ascontiguousarray(rank, np.uint16).view(np.int16), device=dev)
        tm.L.check(tm.lib.tmf_warp_pairs_ranked(P(d_rowptr), entries[0], entries[1], P(d_sp), P(d_rank), i32(m), i32(S), i32(n_items),
                                                entries[2], P(D), P(loss), P(d_order), tm.L.stream_ptr()), tm.lib)
    torch.cuda.synchronize()
    return delta.cpu().numpy(), D.cpu().numpy(), loss.cpu().numpy()


def assert_bits(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def assert_kernel_matches(got, ref, what):
    """No NaN left; the reference's first violators (where D and delta are not zero); values within 1e-5."""
    assert not any(np.isnan(g).any() for g in got), f'{what}: an element was not written'
    assert np.array_equal(got[1] != 0, ref[1] != 0), f'{what}: another first violator than the linear scan finds'
    assert np.array_equal(got[0] != 0, ref[0] != 0), what
    errs = [rel_err(g, r) for g, r in zip(got, ref[:3])]
    print(f'[kernel] {what}: delta {errs[0]:.3g} D {errs[1]:.3g} loss {errs[2]:.3g}')
    assert max(errs) < 1e-5, (what, errs)


@pytest.mark.parametrize('S', KERNEL_S)
def test_kernel_against_the_linear_scan(tm, S):
    """Random rows of 0, 1, 2, 31 .. 33, 64, 65 and 131 entries (a chunk is 64), one with only values <= 0 and one of mixed signs,
    and the constructed rows of kernel_case; S below, at and above the lane count, over several tiles and past what the LDS holds."""
    rowptr, val, p, sp, notes = kernel_case(S)
    m, n_items = sp.shape[0], kernel_n_items(S)
    got, ref = run_kernel(tm, rowptr, val, p, sp, n_items), warp_pairs_ref(rowptr, val, p, sp, n_items)
    assert_kernel_matches(got, ref, f'S={S}')
    delta, D, loss = got
    first = ref[3]
    assert not delta[val <= 0].any() and (val <= 0).sum() > 50 and (delta[first >= 0] < 0).all() and not delta[first < 0].any()
    quiet = np.array([(first[rowptr[u]:rowptr[u + 1]] < 0).all() for u in range(m)])       # users without a violator (or a positive)
    assert quiet.sum() >= 7 and quiet[notes['none']] and not D[quiet].any() and not loss[quiet].any() and (loss[~quiet] != 0).all()
    assert_bits(run_kernel(tm, rowptr, val, p, sp, n_items), got)                                                       # a second call
    assert_bits(run_kernel(tm, rowptr, val, p, sp, n_items, order=np.random.default_rng(S).permutation(m)), got)        # a permuted user order
    assert_bits(run_kernel(tm, rowptr, val, p, sp, n_items, order=np.arange(m)[::-1].copy()), got)
    # the form the engine calls: every row in another order, the ranks beside it - the same bits, D at the samples' places
    rank = np.argsort(np.random.default_rng(S + 1).random(sp.shape), axis=1)
    ranked = run_kernel(tm, rowptr, val, p, np.take_along_axis(sp, rank, 1), n_items, rank=rank,
                        order=np.random.default_rng(S + 2).permutation(m))
    assert_bits(ranked, (delta, np.take_along_axis(D, rank, 1), loss))


def test_kernel_on_tables_without_users_or_entries(tm):
    empty = np.zeros(0, np.float32)
    got = run_kernel(tm, np.zeros(1, np.int64), empty, empty, np.zeros((0, 65), np.float32), 1000)     # n_users = 0
    assert [g.shape for g in got] == [(0,), (0, 65), (0,)]
    rowptr, val, p, sp, _ = kernel_case(65, n_users=1)                                                # one user, nothing stored
    assert rowptr.tolist() == [0, 0]
    delta, D, loss = run_kernel(tm, rowptr, val, p, sp, 1000)                                         # nnz = 0: NULL val / p / delta
    assert delta.shape == (0,) and not D.any() and not loss.any()
    rowptr = np.array([0, 3], np.int64)                                                               # one user with entries
    val, p, sp = np.array([2, -1, 1], np.float32), np.array([0.5, 9.0, -0.25], np.float32), np.linspace(-2, 2, 65, dtype=np.float32)[None]
    got = run_kernel(tm, rowptr, val, p, sp, 1000)
    assert_kernel_matches(got, warp_pairs_ref(rowptr, val, p, sp, 1000), 'one user')
    assert got[0][1] == 0.0 and (got[1] != 0).sum() == 2
    rowptr, val, p, sp, _ = kernel_case(65, n_users=3)                                                # users with 0, 1 and 2 entries
    assert_kernel_matches(run_kernel(tm, rowptr, val, p, sp, 1000), warp_pairs_ref(rowptr, val, p, sp, 1000), '0, 1 and 2 entries')


@pytest.mark.parametrize('S', [65, 513])
def test_kernel_at_every_catalog_size(tm, S):
    """n_items = 1 and 2: floor((n - 1) / N) <= 1, every weight is 0; n_items = S: the violators with N > S - 1 weigh nothing and
    floor lands on 1 for N > (S - 1) / 2; n_items = 100 S: every violator counts."""
    rowptr, val, p, sp, _ = kernel_case(S)
    for n_items in (1, 2, S, 100 * S):
        got, ref = run_kernel(tm, rowptr, val, p, sp, n_items), warp_pairs_ref(rowptr, val, p, sp, n_items)
        if n_items <= 2:
            assert not any(g.any() for g in got) and not any(np.isnan(g).any() for g in got) and not any(r.any() for r in ref[:3])
        else:
            assert_kernel_matches(got, ref, f'S={S} n_items={n_items}')
        if n_items == S:
            assert ((ref[3] >= 0) & (ref[0] == 0)).sum() > 20, 'violators without a weight'


def test_kernel_on_infinite_and_nan_scores(tm):
    rowptr, val, p, sp, _ = kernel_case(65, n_users=12)
    n_items = kernel_n_items(65)
    a = 5                                                       # 33 positives
    b, e = rowptr[a], rowptr[a + 1]
    assert e - b == 33 and (val[b:e] > 0).all()
    clean, clean_first = run_kernel(tm, rowptr, val, p, sp, n_items), warp_pairs_ref(rowptr, val, p, sp, n_items)[3]
    others = np.arange(12) != a
    ent = np.ones(val.shape[0], bool)
    ent[b:e] = False

    def poisoned(sp2, p2=p):
        got, ref = run_kernel(tm, rowptr, val, p2, sp2, n_items), warp_pairs_ref(rowptr, val, p2, sp2, n_items)
        assert_bits((got[0][ent], got[1][others], got[2][others]), (clean[0][ent], clean[1][others], clean[2][others]))   # nobody else is touched
        assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
        assert np.array_equal(got[1] != 0, ref[1] != 0) and rel_err(got[0], ref[0]) < 1e-5 and rel_err(got[1], ref[1]) < 1e-5
        return got, ref
    # +inf at s = 7: the first violator of every positive that found none before it
    sp2 = sp.copy()
    sp2[a, 7] = np.inf
    (delta, D, loss), ref = poisoned(sp2)
    late = (clean_first[b:e] < 0) | (clean_first[b:e] > 7)
    assert late.sum() >= 5 and (ref[3][b:e][late] == 7).all() and np.array_equal(ref[3][b:e][~late], clean_first[b:e][~late])
    assert loss[a] == np.inf and D[a, 7] > 0 and not D[a, 8:].any()
    # a NaN sample is never chosen: where it was somebody's first violator, the search goes on behind it
    s_nan = int(np.bincount(clean_first[b:e][clean_first[b:e] >= 0]).argmax())
    sp2 = sp.copy()
    sp2[a, s_nan] = np.nan
    (delta, D, loss), ref = poisoned(sp2)
    assert D[a, s_nan] == 0 and clean[1][a, s_nan] > 0 and rel_err(loss[a], ref[2][a]) < 1e-5 and np.isfinite(loss[a])
    # -inf never violates
    sp2 = sp.copy()
    sp2[a, s_nan] = -np.inf
    (delta, D, loss), ref = poisoned(sp2)
    assert D[a, s_nan] == 0 and clean[1][a, s_nan] > 0 and rel_err(loss[a], ref[2][a]) < 1e-5
    # a NaN p_k: that positive takes no part, the user's other entries keep their bits
    k = int(b + np.flatnonzero(clean_first[b:e] >= 0)[0])
    p2 = p.copy()
    p2[k] = np.nan
    (delta, D, loss), ref = poisoned(sp, p2)
    mine = np.arange(b, e) != k
    assert delta[k] == 0 and clean[0][k] < 0 and np.array_equal(delta[b:e][mine].view(np.uint32), clean[0][b:e][mine].view(np.uint32))
    assert rel_err(loss[a], ref[2][a]) < 1e-5 and np.isfinite(loss[a])


# ------------------------------------------------------------------------------------------------------------------------
# one step through the public API
# ------------------------------------------------------------------------------------------------------------------------
def fit_warp(tm, p, epochs, U0=None, V0=None, loss=None, lr=LR, item_features=None, table=True, **attrs):
    U0, V0 = (p['U0'] if U0 is None else U0), (p['V0'] if V0 is None else V0)
    graphs = {k: attrs.pop(k) for k in ('user_repr_graph', 'item_repr_graph') if k in attrs}
    model = tm.MF(p['r'], loss_graph=loss or tm.WARP(), user_weight_graph=tm.Fixed(U0), item_weight_graph=tm.Fixed(V0), n_users=p['m'],
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


def problem_and_reference(problem):
    """(problem, loss mean, gU, gV): the fp64 closed form of a (seed, m, n, r, S), computed once and left unchanged - and only of a
    decided problem."""
    if problem not in _REFS:
        p = warp_problem(*problem)
        g_min, b = decidedness(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
        assert g_min > b, f'{problem} is not decided: smallest gap {g_min:.3g}, fp32 reach {b:.3g}'
        loss, _, _, gU, gV = warp_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
        for a in (gU, gV):
            a.setflags(write=False)
        _REFS[problem] = (p, loss / int((p['val'] > 0).sum()), gU, gV)
    return _REFS[problem]


def check_one_step(tm, problem, what='', **attrs):
    p, loss, gU, gV = problem_and_reference(problem)
    model = fit_warp(tm, p, 1, **attrs)
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


@pytest.mark.parametrize('r,S', list(GEOMETRY_PROBLEMS))
def test_every_row_geometry_one_step(tm, engine_only, r, S):
    check_one_step(tm, GEOMETRY_PROBLEMS[(r, S)], f'r={r} S={S}')


def test_a_catalog_no_larger_than_the_row_one_step(tm, engine_only):
    """60 x 40 with S = 64: n <= S, so violators found after more than n - 1 trials weigh nothing."""
    check_one_step(tm, SMALL_CATALOG_PROBLEM, 'n <= S')


@pytest.mark.parametrize('env', [{'TMF_ITEM_SLICES': '3'}, {'TMF_ROW_STATIONARY': '1'}, {'TMF_SCORES6': '1'}, {'TMF_ROWS4': '1'}],
                         ids=lambda e: '='.join(*e.items()))
def test_the_forms_of_the_user_and_item_pass_one_step(tm, engine_only, monkeypatch, env):
    """Everything around the pair step is the WMRB pass in its other forms: three item slices, the row-stationary gradU, the flat
    score streams and the row-stationary item pass (r = 128: rows of 32 lanes, which all of them have kernels for)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = 128
    problem = GEOMETRY_PROBLEMS[(r, 64)]
    st = check_one_step(tm, problem, str(env))._state
    if 'TMF_ITEM_SLICES' in env:
        assert st.wplan.n_slices == 3
    if 'TMF_ROW_STATIONARY' in env:
        assert st.row_stationary == bool(tm.lib.tmf_wmrb_gradu4_supported(r, 0))
    if 'TMF_SCORES6' in env:
        assert (st.wplan.s6 is not None) == bool(tm.lib.tmf_wmrb_scores6_supported(r, 0, problem[2]))
    if 'TMF_ROWS4' in env:
        assert st.wplan.rows4 == bool(tm.lib.tmf_wsum_rows4_rows_per_group(r, 0))


def test_bf16_storage_one_step(tm, engine_only):
    """bf16 factor storage / fp32 arithmetic: against the closed form on the bf16-rounded tables, which must be decided for those
    tables; the new rows must lie in the step interval rounded to bf16 (tests/test_gpu_bpr.py::test_bf16_storage_one_step)."""
    p = warp_problem(*BF16_PROBLEM)
    U0, V0 = bf16_round(p['U0']), bf16_round(p['V0'])
    g_min, b = decidedness(U0, V0, p['idx'], p['val'], p['R'])
    assert g_min > b
    model = fit_warp(tm, p, 1, U0=U0, V0=V0, factor_dtype=torch.bfloat16)
    assert model.user_embedding.dtype == torch.bfloat16 and model._state.wplan.sliced
    loss, _, _, gU, gV = warp_closed_form(U0, V0, p['idx'], p['val'], p['R'])
    assert rel_err(model.loss_history_[0], loss / int((p['val'] > 0).sum())) < 1e-5
    for got, W0, g in zip((host(model.user_embedding), host(model.item_embedding)), (U0, V0), (gU, gV)):
        lo, hi = step_bounds(W0, g, LR)
        got = got.astype(np.float64)
        assert (got >= bf16_round(lo) - 1e-12).all() and (got <= bf16_round(hi) + 1e-12).all()


def test_opt_in_persistent_adam_first_step(tm, engine_only):
    """optimizer='adam': the first step is the default's bit for bit (and the default's is the closed form's)."""
    p, _, _, _ = problem_and_reference(ADAM_PROBLEM)
    a1, f1 = fit_warp(tm, p, 1, optimizer='adam'), check_one_step(tm, ADAM_PROBLEM, 'fresh adam')
    assert torch.equal(a1.user_embedding, f1.user_embedding) and torch.equal(a1.item_embedding, f1.item_embedding)
    assert a1.loss_history_ == f1.loss_history_ and a1._state.wplan.sliced


def test_biased_item_side_one_step(tm, engine_only):
    """A bias starts at zero, so the effective tables are the weights and their gradients the closed form's.  The item bias itself
    cancels in every 1 - e_u . (e_pos - e_neg) (as under WMRB and BPR): its gradient is rounding noise, so neither it nor the item
    embedding that carries it is compared."""
    p, loss, gU, gV = problem_and_reference(BIASED_PROBLEM)
    model = fit_warp(tm, p, 1, item_repr_graph=tm.EG.BiasedLinearEmbedding())
    st = model._state
    assert st.bias_v is not None and st.bias_u is None and st.wplan.sliced
    assert rel_err(model.loss_history_[0], loss) < 1e-5
    assert_step(host(model.user_embedding), p['U0'], gU, LR, rtol=1e-5, what='biased item side: U')
    assert len(model.item_trainable) == 2 and model.item_trainable[1] is model.item_linear_bias
    assert_step(host(model.item_trainable[0]), p['V0'], gV, LR, rtol=1e-5, what='biased item side: item weights')
    assert torch.equal(model.item_embedding, model.item_trainable[0] + model.item_linear_bias.detach())


def test_item_side_over_sparse_features_one_step(tm, engine_only):
    """F = [I | tags] (hstack_identity): E = F W, dL/dW = F^T dL/dE with dL/dE the closed form on (U, E), decided on those tables;
    every row's gradient agrees to 1e-5, so feature f's sum may be off by 1e-5 sum_i |x_if| |dL/dE[i]| (tests/test_gpu_features.py)."""
    from test_gpu_features import assert_step_with_slack
    p, tag_idx, tag_val, F_dense, W0 = features_problem()
    n, T = p['n'], F_dense.shape[1] - p['n']
    E0 = F_dense @ W0.astype(np.float64)
    g_min, b = decidedness(p['U0'], E0, p['idx'], p['val'], p['R'])
    assert g_min > b
    F = tm.hstack(n, tm.SF(tag_idx, tag_val, (n, T)))
    assert torch.equal(F.to_dense().cpu(), torch.tensor(F_dense, dtype=torch.float32))
    model = fit_warp(tm, p, 1, V0=W0, item_features=F)
    loss, _, _, gU, gE = warp_closed_form(p['U0'], E0, p['idx'], p['val'], p['R'])
    st = model._state
    assert st.feat_v is not None and st.feat_u is None and st.wplan.sliced
    assert rel_err(model.loss_history_[0], loss / int((p['val'] > 0).sum())) < 1e-5
    assert_step(host(model.user_embedding), p['U0'], gU, LR, rtol=1e-5, what='user table')
    slack = 1e-5 * np.abs(F_dense).T @ np.abs(gE)
    assert_step_with_slack(host(model.item_trainable[0]), W0, F_dense.T @ gE, slack, LR, 'warp item weights over sparse features')
    assert model.item_embedding.shape == (n, p['r']) and torch.equal(model.item_embedding, model.embed_items(F))


def test_l2_regularisation_one_step(tm, engine_only):
    """user_alpha = item_alpha = 0.01: the step of the closed-form gradient plus 2 alpha W; loss_history_ stays the data term."""
    alpha = 0.01
    p, loss, gU, gV = problem_and_reference(L2_PROBLEM)
    model = fit_warp(tm, p, 1, user_alpha=alpha, item_alpha=alpha)
    assert model._state.wplan.sliced and model._state.l2 == [np.float32(2 * alpha)] * 2
    assert rel_err(model.loss_history_[0], loss) < 1e-5
    assert_step(host(model.user_embedding), p['U0'], gU + 2 * alpha * p['U0'].astype(np.float64), LR, rtol=1e-5, what='l2 U')
    assert_step(host(model.item_embedding), p['V0'], gV + 2 * alpha * p['V0'].astype(np.float64), LR, rtol=1e-5, what='l2 V')
    plain = fit_warp(tm, p, 1)
    assert not torch.equal(plain.user_embedding, model.user_embedding) and plain.loss_history_ == model.loss_history_


def test_relu_engine_runs_the_pair_step(tm, engine_only):
    """relu_engine: a ReLUEmbedding user side (aux = 5 r = 60 hidden units over eye(60)) trains through the engine's ReLU epoch
    around the same pair step: the fit stays on the engine, on the sliced pass, finite, and repeats bit for bit."""
    p = warp_problem(77, 60, 240, 12, 20)
    W0 = (np.random.default_rng(1).standard_normal((5 * p['r'], p['r'])) * 0.3).astype(np.float32)
    runs = []
    for _ in range(2):
        torch.manual_seed(0)                                                     # the hidden weights are drawn by the fit
        runs.append(fit_warp(tm, p, 3, U0=W0, user_repr_graph=tm.EG.ReLUEmbedding(), relu_engine=True))
    a, b = runs
    assert a._state.relu_u is not None and a._state.wplan.sliced and np.isfinite(a.loss_history_).all() and len(a.loss_history_) == 3
    assert a.loss_history_[0] > 0 and a.loss_history_ == b.loss_history_ and torch.equal(a.user_embedding, b.user_embedding)
    assert torch.equal(a.item_embedding, b.item_embedding) and a.user_embedding.shape == (p['m'], p['r'])


def test_no_sample_table_on_the_engine(tm, engine_only):
    p = warp_problem(15, 12, 9, 4, 4)
    with pytest.raises(tm.Missing, match='WARPLoss'):
        fit_warp(tm, p, 1, table=False)


# ------------------------------------------------------------------------------------------------------------------------
# replay, no leakage
# ------------------------------------------------------------------------------------------------------------------------
def test_graph_replay(tm, engine_only, monkeypatch):
    """200 x 150, r = 16, S = 32: twelve epochs - one replay of a twelve-epoch hipGraph - and thirteen - the replay and an eager epoch
    behind it - give with TMF_NO_GRAPH=1 the same history and the same tables, bit for bit.  The first loss is the closed form's
    (the problem is decided); the last is below it.  Later epochs are not compared with fp64: a first-violator choice flips
    where a gap closes along the trajectory."""
    p, loss, _, _ = problem_and_reference(REPLAY_PROBLEM)
    for epochs in (12, 13):
        monkeypatch.delenv('TMF_NO_GRAPH', raising=False)
        a = fit_warp(tm, p, epochs)
        monkeypatch.setenv('TMF_NO_GRAPH', '1')
        b = fit_warp(tm, p, epochs)
        assert a.loss_history_ == b.loss_history_ and len(a.loss_history_) == epochs
        assert torch.equal(a.user_embedding, b.user_embedding) and torch.equal(a.item_embedding, b.item_embedding)
        h = a.loss_history_
        print(f'[replay] {epochs} epochs: first {rel_err(h[0], loss):.3g}, history {h[0]:.4f} -> {h[-1]:.4f}')
        assert rel_err(h[0], loss) < 1e-5 and h[-1] < h[0]


@pytest.mark.parametrize('other', ['WMRB', 'BPR'])
def test_a_warp_fit_leaves_nothing_behind(tm, engine_only, other):
    p = warp_problem(9, 60, 40, 33, 20)
    loss = getattr(tm, other)
    before = fit_warp(tm, p, 3, loss=loss())
    warp = fit_warp(tm, p, 3)
    after = fit_warp(tm, p, 3, loss=loss())
    assert before.loss_history_ == after.loss_history_ and before.loss_history_ != warp.loss_history_
    assert torch.equal(before.user_embedding, after.user_embedding) and torch.equal(before.item_embedding, after.item_embedding)
    assert not torch.equal(before.user_embedding, warp.user_embedding)
