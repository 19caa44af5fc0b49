"""KOSWARPLoss on the sparse HIP engine (tmf_kos_weights, tmf_warp_pairs_kos, _engine.epoch_wmrb(pairs='warp_kos')) against the NumPy
fp64 references of tests/test_kos_cpu.py, which that file pins to an exhaustive enumeration of the draws and to the plug-in's own
get_loss.  The weights: |got - ref| <= 2^-23 ref + 1e-9 (one fp32 rounding; the fp64 sum of at most 64 terms and its one
cancellation).  The pair step: with omega = 1 the bits of tmf_warp_pairs / tmf_warp_pairs_ranked, with the reference's weights the
reference's non-zero pattern and rel_err < 1e-5 (tests/test_gpu_warp.py's bound).  One step through fit() is compared with the fp64
closed form only on *decided* problems - no first-violator choice and no order of two positives of a user within fp32 reach of
flipping (test_kos_cpu.assert_decided), asserted again here before any engine call."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_step, rel_err, step_bounds
from test_kos_cpu import (K, KOS_ADAM, KOS_BF16, KOS_BIASED, KOS_CAP, KOS_GEOMETRY, KOS_L2, KOS_REPLAY, N, assert_decided, kos_closed_form,
                          kos_features_problem, kos_pairs_ref, kos_problem, kos_weights_ref, single_positive_problem)
from test_warp_cpu import LR, WARP_CAP, bf16_round, decidedness, kernel_case, kernel_n_items

pytestmark = pytest.mark.gpu
NAN = float('nan')


@pytest.fixture(scope='module')
def tm():
    from teamoflow_amd import _engine, _lib, _ops
    from teamoflow_amd.mf import embedding_graphs as EG
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import KOSWARPLoss, WARPLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization, SampleTableMissing
    from teamoflow_amd.mf.sparse import SparseFeatures, SparseInteractions, eye, hstack_identity
    lib = _lib.get()

    class NS:
        pass
    ns = NS()
    ns.lib, ns.L, ns.E, ns.ops, ns.EG, ns.MF, ns.Fixed, ns.KOS, ns.WARP, ns.Sparse, ns.SF, ns.eye, ns.hstack, ns.Missing = lib, _lib, _engine, \
        _ops, EG, MatrixFactorization, FixedInitializer, KOSWARPLoss, WARPLoss, SparseInteractions, SparseFeatures, eye, hstack_identity, \
        SampleTableMissing
    return ns


@pytest.fixture
def engine_only(tm, monkeypatch):
    """_fit_generic refuses to run: a fit that passes ran on the engine."""
    def refuse(self, *a, **k):
        raise AssertionError('_fit_generic was called')
    monkeypatch.setattr(tm.MF, '_fit_generic', refuse)


def assert_bits(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------
# tmf_kos_weights alone
# ------------------------------------------------------------------------------------------------------------------------
def run_weights(tm, rowptr, val, p, k, n, order=None):
    """tmf_kos_weights on host arrays, omega pre-filled with NaN -> omega as NumPy.  A table without entries passes NULL for val, p
    and omega (the pointer of an empty tensor)."""
    dev, P, i32 = torch.device('cuda'), tm.L.ptr, ctypes.c_int32
    d_rowptr = torch.as_tensor(np.asarray(rowptr, np.int64), device=dev)
    d_val, d_p = (torch.as_tensor(np.asarray(x, np.float32), device=dev).contiguous() for x in (val, p))
    omega = torch.full((d_val.numel(),), NAN, device=dev)
    d_order = None if order is None else torch.as_tensor(np.asarray(order, np.int32), device=dev)
    entries = [P(x) if x.numel() else None for x in (d_val, d_p, omega)]
    tm.L.check(tm.lib.tmf_kos_weights(P(d_rowptr), entries[0], entries[1], i32(d_rowptr.numel() - 1), i32(k), i32(n), entries[2],
                                      P(d_order), tm.L.stream_ptr()), tm.lib)
    torch.cuda.synchronize()
    return omega.cpu().numpy()


WEIGHT_POSITIVES = (0, 1, 2, 4, 5, 9, 10, 11, 31, 32, 33, 63, 64, 65, 131)


def weights_case():
    """(rowptr, val, p, notes): a row for every count of WEIGHT_POSITIVES, each mixed with values <= 0 (scores ~ N(0, 1), no ties),
    then the rows named in ``notes``: only values <= 0; KOS_CAP + 5 and 2 KOS_CAP + 7 positives without ties, 2 KOS_CAP + 100 with
    scores from 37 values (tie blocks across segments) and KOS_CAP + 1 equal scores; a tie block at the top, in the middle and at
    the end of 12 positives; duplicates (one score stored three times and one twice among 9); +inf, -inf, NaN and -0 / +0."""
    rng = np.random.default_rng(7)
    f = np.float32
    rows, notes = [], {}

    def mixed(p_pos, n_other):
        val = np.concatenate([rng.integers(1, 6, p_pos.size), rng.choice(np.array([0, -1, -3]), n_other)]).astype(f)
        p = np.concatenate([p_pos, rng.standard_normal(n_other)]).astype(f)
        perm = rng.permutation(val.size)
        return val[perm], p[perm]
    for P in WEIGHT_POSITIVES:
        rows.append(mixed(rng.standard_normal(P), 3 + P // 4))

    def add(name, p_pos, n_other=0):
        notes[name] = len(rows)
        rows.append(mixed(np.asarray(p_pos, f), n_other))
    add('nonpositive', [], 5)
    add('long', rng.permutation(KOS_CAP + 5) * 0.001, 40)
    add('longer', rng.permutation(2 * KOS_CAP + 7) * 0.001 - 3.0, 300)
    add('long_ties', rng.integers(0, 37, 2 * KOS_CAP + 100) * 0.25, 100)
    add('long_equal', np.full(KOS_CAP + 1, 1.5), 3)
    base = np.arange(12.0)
    for name, block in (('ties_top', [9, 10, 11]), ('ties_middle', [4, 5, 6]), ('ties_end', [0, 1])):
        p = base.copy()
        p[block] = p[block[0]]
        add(name, rng.permutation(p), 4)
    add('duplicates', rng.permutation([0.5, 0.5, 0.5, -1.0, -1.0, 2.0, 3.0, 0.25, 0.75]), 2)
    add('special', rng.permutation([np.inf, -np.inf, np.nan, np.nan, np.inf, 1.0, -0.0, 0.0, -2.0, 7.0, 0.5]), 3)
    rowptr = np.concatenate([[0], np.cumsum([v.size for v, _ in rows])]).astype(np.int64)
    return rowptr, np.concatenate([v for v, _ in rows]), np.concatenate([p for _, p in rows]), notes


_WEIGHTS = {}


def weights_case_and_reference(k, n):
    if 'case' not in _WEIGHTS:
        _WEIGHTS['case'] = weights_case()
    if (k, n) not in _WEIGHTS:
        rowptr, val, p, _ = _WEIGHTS['case']
        ref = kos_weights_ref(rowptr, val, p, k, n)
        ref.setflags(write=False)
        _WEIGHTS[(k, n)] = ref
    return _WEIGHTS['case'] + (_WEIGHTS[(k, n)],)


def test_the_weights_case_holds_what_it_promises():
    rowptr, val, p, notes = weights_case()
    pos = np.array([(val[rowptr[u]:rowptr[u + 1]] > 0).sum() for u in range(rowptr.size - 1)])
    assert pos[:len(WEIGHT_POSITIVES)].tolist() == list(WEIGHT_POSITIVES) and ((np.diff(rowptr) - pos)[:len(WEIGHT_POSITIVES)] >= 3).all()
    assert pos[notes['nonpositive']] == 0 and pos[notes['long']] == KOS_CAP + 5 and pos[notes['longer']] == 2 * KOS_CAP + 7
    assert pos[notes['long_ties']] == 2 * KOS_CAP + 100 and pos[notes['long_equal']] == KOS_CAP + 1
    u = notes['special']
    mine = p[rowptr[u]:rowptr[u + 1]][val[rowptr[u]:rowptr[u + 1]] > 0]
    assert np.isnan(mine).sum() == 2 and np.isposinf(mine).sum() == 2 and np.isneginf(mine).sum() == 1 and np.signbit(mine[mine == 0]).sum() == 1


@pytest.mark.parametrize('k,n', [(5, 10), (1, 1), (10, 10), (1, 64)])
def test_weights_against_the_reference(tm, k, n):
    rowptr, val, p, notes, ref = weights_case_and_reference(k, n)
    m = rowptr.size - 1
    got = run_weights(tm, rowptr, val, p, k, n)
    assert not np.isnan(got).any(), 'a slot was not written'
    assert not got[val <= 0].any() and (got[val > 0] >= 0).all()
    err = np.abs(got.astype(np.float64) - ref)
    bound = 2.0 ** -23 * ref + 1e-9
    print(f'[weights] k={k} n={n}: largest |got - ref| / bound {(err / bound).max():.3g}, largest error {err.max():.3g}')
    assert (err <= bound).all(), (k, n, int(np.argmax(err / bound)))
    sums = np.add.reduceat(np.concatenate([got.astype(np.float64), [0.0]]), rowptr[:-1])[:m] * (np.diff(rowptr) > 0)
    has = np.array([(val[rowptr[u]:rowptr[u + 1]] > 0).any() for u in range(m)])
    assert np.abs(sums[has] - 1).max() < 1e-5 and not sums[~has].any(), np.abs(sums[has] - 1).max()
    assert_bits([run_weights(tm, rowptr, val, p, k, n)], [got])                                                         # a second call
    assert_bits([run_weights(tm, rowptr, val, p, k, n, order=np.random.default_rng(k).permutation(m))], [got])          # a permuted user order
    assert_bits([run_weights(tm, rowptr, val, p, k, n, order=np.arange(m)[::-1].copy())], [got])                        # a reversed one
    if (k, n) == (1, 1):                                                 # omega = 1 / P exactly where P is a power of two
        u = WEIGHT_POSITIVES.index(64)
        mine = got[rowptr[u]:rowptr[u + 1]]
        assert set(mine.tolist()) == {0.0, 1.0 / 64}
    for name in ('ties_top', 'ties_middle', 'ties_end', 'duplicates', 'long_equal', 'special'):      # a tie block shares one weight
        u = notes[name]
        sl = slice(rowptr[u], rowptr[u + 1])
        keys = np.where(np.isnan(p[sl]), -np.inf, p[sl]) + 0.0
        for key in np.unique(keys[val[sl] > 0]):
            for nan in (False, True):
                block = got[sl][(val[sl] > 0) & (keys == key) & (np.isnan(p[sl]) == nan)]
                assert np.unique(block.view(np.uint32)).size <= 1, (name, key)


def test_weights_on_tables_without_users_or_entries(tm):
    empty = np.zeros(0, np.float32)
    assert run_weights(tm, np.zeros(1, np.int64), empty, empty, K, N).shape == (0,)                    # n_users = 0
    assert run_weights(tm, np.zeros(4, np.int64), empty, empty, K, N).shape == (0,)                    # three users, nothing stored: NULLs
    rowptr = np.array([0, 0, 3, 3], np.int64)                                                          # a user with entries between two without
    got = run_weights(tm, rowptr, np.array([2, -1, 1], np.float32), np.array([0.5, 9.0, -0.25], np.float32), 1, 2)
    assert got.tolist() == [0.75, 0.0, 0.25]                                                           # the better of two draws from two


# ------------------------------------------------------------------------------------------------------------------------
# the weighted pair step
# ------------------------------------------------------------------------------------------------------------------------
def run_pairs(tm, rowptr, val, p, sp, n_items, omega=None, rank=None, order=None, plain=False):
    """tmf_warp_pairs_kos on host arrays (plain: tmf_warp_pairs / tmf_warp_pairs_ranked, no omega), every output pre-filled with NaN
    -> (delta, D, loss_part) as NumPy."""
    dev, P, i32 = torch.device('cuda'), tm.L.ptr, ctypes.c_int32
    m, S = sp.shape
    d_rowptr = torch.as_tensor(np.asarray(rowptr, np.int64), device=dev)
    d_val, d_p, d_sp = (torch.as_tensor(np.asarray(x, np.float32), device=dev).contiguous() for x in (val, p, sp))
    delta = torch.full((d_val.numel(),), NAN, device=dev)
    D = torch.full((m, S), NAN, device=dev)
    loss = torch.full((m,), NAN, device=dev)
    d_order = None if order is None else torch.as_tensor(np.asarray(order, np.int32), device=dev)
    d_rank = None if rank is None else torch.as_tensor(np.ascontiguousarray(rank, np.uint16).view(np.int16), device=dev)
    entries = [P(x) if x.numel() else None for x in (d_val, d_p, delta)]
    tail = (i32(m), i32(S), i32(n_items), entries[2], P(D), P(loss), P(d_order), tm.L.stream_ptr())
    if plain and rank is None:
        rc = tm.lib.tmf_warp_pairs(P(d_rowptr), entries[0], entries[1], P(d_sp), *tail)
    elif plain:
        rc = tm.lib.tmf_warp_pairs_ranked(P(d_rowptr), entries[0], entries[1], P(d_sp), P(d_rank), *tail)
    else:
        d_omega = torch.as_tensor(np.asarray(omega, np.float32), device=dev).contiguous()
        d_omega = d_omega if d_omega.numel() else torch.zeros(1, device=dev)                         # omega is required: never NULL
        rc = tm.lib.tmf_warp_pairs_kos(P(d_rowptr), entries[0], entries[1], P(d_sp), P(d_rank), P(d_omega), *tail)
    tm.L.check(rc, tm.lib)
    torch.cuda.synchronize()
    return delta.cpu().numpy(), D.cpu().numpy(), loss.cpu().numpy()


PAIR_S = (1, 64, 65, 513, 1100, WARP_CAP + 5)


@pytest.mark.parametrize('S', PAIR_S)
def test_unit_weights_give_the_bits_of_warp(tm, S):
    rowptr, val, p, sp, _ = kernel_case(S)
    n_items, ones = kernel_n_items(S), np.ones(val.shape[0], np.float32)
    plain = run_pairs(tm, rowptr, val, p, sp, n_items, plain=True)
    assert (plain[1] != 0).any() and not any(np.isnan(x).any() for x in plain)
    assert_bits(run_pairs(tm, rowptr, val, p, sp, n_items, omega=ones), plain)
    rank = np.argsort(np.random.default_rng(S + 1).random(sp.shape), axis=1)
    sp_r = np.take_along_axis(sp, rank, 1)
    ranked = run_pairs(tm, rowptr, val, p, sp_r, n_items, rank=rank, plain=True)
    assert_bits(run_pairs(tm, rowptr, val, p, sp_r, n_items, omega=ones, rank=rank), ranked)


@pytest.mark.parametrize('S', PAIR_S)
def test_weighted_pairs_against_the_reference(tm, S):
    rowptr, val, p, sp, _ = kernel_case(S)
    m, n_items = sp.shape[0], kernel_n_items(S)
    omega = kos_weights_ref(rowptr, val, p, K, N).astype(np.float32)
    assert (omega[val > 0] > 1e-30).all() and np.unique(omega).size > 100
    got, ref = run_pairs(tm, rowptr, val, p, sp, n_items, omega=omega), kos_pairs_ref(rowptr, val, p, sp, n_items, omega)
    assert not any(np.isnan(g).any() for g in got), 'an element was not written'
    assert np.array_equal(got[1] != 0, ref[1] != 0) and np.array_equal(got[0] != 0, ref[0] != 0) and (ref[1] != 0).any()
    errs = [rel_err(g, r) for g, r in zip(got, ref[:3])]
    print(f'[weighted pairs] S={S}: delta {errs[0]:.3g} D {errs[1]:.3g} loss {errs[2]:.3g}')
    assert max(errs) < 1e-5, errs
    assert_bits(run_pairs(tm, rowptr, val, p, sp, n_items, omega=omega, order=np.random.default_rng(S).permutation(m)), got)
    rank = np.argsort(np.random.default_rng(S + 1).random(sp.shape), axis=1)
    ranked = run_pairs(tm, rowptr, val, p, np.take_along_axis(sp, rank, 1), n_items, omega=omega, rank=rank,
                       order=np.random.default_rng(S + 2).permutation(m))
    assert_bits(ranked, (got[0], np.take_along_axis(got[1], rank, 1), got[2]))
    zeroed = omega.copy()                                                # a weight of zero: the entry takes no part
    zeroed[::3] = 0.0
    got0, ref0 = run_pairs(tm, rowptr, val, p, sp, n_items, omega=zeroed), kos_pairs_ref(rowptr, val, p, sp, n_items, zeroed)
    assert not got0[0][::3].any() and np.array_equal(got0[1] != 0, ref0[1] != 0) and max(rel_err(g, r) for g, r in zip(got0, ref0[:3])) < 1e-5


def test_pairs_on_tables_without_users_or_entries(tm):
    empty = np.zeros(0, np.float32)
    got = run_pairs(tm, np.zeros(1, np.int64), empty, empty, np.zeros((0, 65), np.float32), 1000, omega=empty)      # n_users = 0
    assert [g.shape for g in got] == [(0,), (0, 65), (0,)]
    rowptr, val, p, sp, _ = kernel_case(65, n_users=3)                                                # users with 0, 1 and 2 entries
    assert rowptr.tolist()[:2] == [0, 0]
    omega = kos_weights_ref(rowptr, val, p, K, N).astype(np.float32)
    got, ref = run_pairs(tm, rowptr, val, p, sp, 1000, omega=omega), kos_pairs_ref(rowptr, val, p, sp, 1000, omega)
    assert not got[1][0].any() and got[2][0] == 0 and not any(np.isnan(g).any() for g in got)
    assert np.array_equal(got[1] != 0, ref[1] != 0) and max(rel_err(g, r) for g, r in zip(got, ref[:3])) < 1e-5


# ------------------------------------------------------------------------------------------------------------------------
# through the public API
# ------------------------------------------------------------------------------------------------------------------------
def fit_kos(tm, p, epochs, U0=None, V0=None, loss=None, lr=LR, item_features=None, table=True, **attrs):
    U0, V0 = (p['U0'] if U0 is None else U0), (p['V0'] if V0 is None else V0)
    graphs = {k: attrs.pop(k) for k in ('user_repr_graph', 'item_repr_graph') if k in attrs}
    model = tm.MF(p['r'], loss_graph=loss or tm.KOS(), user_weight_graph=tm.Fixed(U0), item_weight_graph=tm.Fixed(V0), n_users=p['m'],
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
        p = kos_problem(problem)
        assert_decided(p['U0'], p['V0'], p['idx'], p['val'], p['R'], str(problem))
        loss, _, _, gU, gV = kos_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
        for a in (gU, gV):
            a.setflags(write=False)
        _REFS[problem] = (p, loss / int((p['val'] > 0).sum()), gU, gV)
    return _REFS[problem]


def check_one_step(tm, problem, what='', **attrs):
    p, loss, gU, gV = problem_and_reference(problem)
    model = fit_kos(tm, p, 1, **attrs)
    st = model._state
    assert st.wplan.sliced and st.plan.n_pos == int((p['val'] > 0).sum()) and st.wplan.omega.shape == (st.plan.nnz,)
    err = rel_err(model.loss_history_[0], loss)
    print(f'[one step] {what}: loss {err:.3g}')
    assert err < 1e-5, what                                                    # the mean over the positives
    assert_step(host(model.user_embedding), p['U0'], gU, LR, rtol=1e-5, what=f'{what} U')
    assert_step(host(model.item_embedding), p['V0'], gV, LR, rtol=1e-5, what=f'{what} V')
    for row, W1, W0 in ((p['empty_user'], model.user_embedding, p['U0']), (p['nonpos_user'], model.user_embedding, p['U0']),
                        (p['empty_item'], model.item_embedding, p['V0'])):
        assert np.array_equal(host(W1)[row], W0[row])                          # a user without positives keeps its row's bits
    return model


@pytest.mark.parametrize('r,S', list(KOS_GEOMETRY))
def test_every_row_geometry_one_step(tm, engine_only, r, S):
    check_one_step(tm, KOS_GEOMETRY[(r, S)], f'r={r} S={S}')


def test_the_engine_sees_the_weights_of_the_reference(tm, engine_only):
    """After one epoch the plan's omega holds the weights of the scores of the start tables, delta their product with WARP's."""
    problem = KOS_GEOMETRY[(33, 70)]
    p, _, _, _ = problem_and_reference(problem)
    st = fit_kos(tm, p, 1)._state
    from test_warp_cpu import _scores
    _, _, _, _, rowptr, pk, sp = _scores(p['U0'], p['V0'], p['idx'], p['R'])
    ref = kos_weights_ref(rowptr, p['val'], pk, K, N)
    got = st.wplan.omega.cpu().numpy().astype(np.float64)
    assert (np.abs(got - ref) <= 2.0 ** -23 * ref + 1e-9).all()
    assert rel_err(st.wplan.delta.cpu().numpy(), kos_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])[1]) < 1e-5


def test_other_k_and_n_one_step(tm, engine_only):
    problem = KOS_GEOMETRY[(33, 70)]
    p, default_loss, _, _ = problem_and_reference(problem)
    for k, n in ((1, 1), (2, 3), (10, 10), (1, 64)):
        loss, _, _, gU, gV = kos_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'], k, n)
        model = fit_kos(tm, p, 1, loss=tm.KOS(k, n))
        assert rel_err(model.loss_history_[0], loss / int((p['val'] > 0).sum())) < 1e-5 and abs(loss / int((p['val'] > 0).sum()) - default_loss) > 1e-4
        assert_step(host(model.user_embedding), p['U0'], gU, LR, rtol=1e-5, what=f'k={k} n={n} U')
        assert_step(host(model.item_embedding), p['V0'], gV, LR, rtol=1e-5, what=f'k={k} n={n} V')


def test_bf16_storage_one_step(tm, engine_only):
    """bf16 factor storage / fp32 arithmetic: against the closed form on the bf16-rounded tables, which must be decided for those
    tables; the new rows must lie in the step interval rounded to bf16 (tests/test_gpu_warp.py::test_bf16_storage_one_step)."""
    p = kos_problem(KOS_BF16)
    U0, V0 = bf16_round(p['U0']), bf16_round(p['V0'])
    assert_decided(U0, V0, p['idx'], p['val'], p['R'], 'bf16')
    model = fit_kos(tm, p, 1, U0=U0, V0=V0, factor_dtype=torch.bfloat16)
    assert model.user_embedding.dtype == torch.bfloat16 and model._state.wplan.sliced
    loss, _, _, gU, gV = kos_closed_form(U0, V0, p['idx'], p['val'], p['R'])
    assert rel_err(model.loss_history_[0], loss / int((p['val'] > 0).sum())) < 1e-5
    for got, W0, g in zip((host(model.user_embedding), host(model.item_embedding)), (U0, V0), (gU, gV)):
        lo, hi = step_bounds(W0, g, LR)
        got = got.astype(np.float64)
        assert (got >= bf16_round(lo) - 1e-12).all() and (got <= bf16_round(hi) + 1e-12).all()


def test_opt_in_persistent_adam_first_step(tm, engine_only):
    """optimizer='adam': the first step is the default's bit for bit (and the default's is the closed form's)."""
    p, _, _, _ = problem_and_reference(KOS_ADAM)
    a1, f1 = fit_kos(tm, p, 1, optimizer='adam'), check_one_step(tm, KOS_ADAM, 'fresh adam')
    assert torch.equal(a1.user_embedding, f1.user_embedding) and torch.equal(a1.item_embedding, f1.item_embedding)
    assert a1.loss_history_ == f1.loss_history_ and a1._state.wplan.sliced
    a3 = fit_kos(tm, p, 3, optimizer='adam')
    assert np.isfinite(a3.loss_history_).all() and a3.loss_history_[0] == a1.loss_history_[0]


def test_biased_item_side_one_step(tm, engine_only):
    """A bias starts at zero, so the effective tables are the weights and their gradients the closed form's; the item bias cancels in
    every 1 - e_u . (e_pos - e_neg) and is not compared (tests/test_gpu_warp.py::test_biased_item_side_one_step)."""
    p, loss, gU, gV = problem_and_reference(KOS_BIASED)
    model = fit_kos(tm, p, 1, item_repr_graph=tm.EG.BiasedLinearEmbedding())
    st = model._state
    assert st.bias_v is not None and st.bias_u is None and st.wplan.sliced
    assert rel_err(model.loss_history_[0], loss) < 1e-5
    assert_step(host(model.user_embedding), p['U0'], gU, LR, rtol=1e-5, what='biased item side: U')
    assert_step(host(model.item_trainable[0]), p['V0'], gV, LR, rtol=1e-5, what='biased item side: item weights')


def test_item_side_over_sparse_features_one_step(tm, engine_only):
    """F = [I | tags]: E = F W, dL/dW = F^T dL/dE with dL/dE the closed form on (U, E), decided on those tables
    (tests/test_gpu_warp.py::test_item_side_over_sparse_features_one_step)."""
    from test_gpu_features import assert_step_with_slack
    p, tag_idx, tag_val, F_dense, W0 = kos_features_problem()
    n, T = p['n'], F_dense.shape[1] - p['n']
    E0 = F_dense @ W0.astype(np.float64)
    assert_decided(p['U0'], E0, p['idx'], p['val'], p['R'], 'features')
    F = tm.hstack(n, tm.SF(tag_idx, tag_val, (n, T)))
    model = fit_kos(tm, p, 1, V0=W0, item_features=F)
    loss, _, _, gU, gE = kos_closed_form(p['U0'], E0, p['idx'], p['val'], p['R'])
    st = model._state
    assert st.feat_v is not None and st.feat_u is None and st.wplan.sliced
    assert rel_err(model.loss_history_[0], loss / int((p['val'] > 0).sum())) < 1e-5
    assert_step(host(model.user_embedding), p['U0'], gU, LR, rtol=1e-5, what='user table')
    slack = 1e-5 * np.abs(F_dense).T @ np.abs(gE)
    assert_step_with_slack(host(model.item_trainable[0]), W0, F_dense.T @ gE, slack, LR, 'kos item weights over sparse features')


def test_l2_regularisation_one_step(tm, engine_only):
    """user_alpha = item_alpha = 0.01: the step of the closed-form gradient plus 2 alpha W; loss_history_ stays the data term."""
    alpha = 0.01
    p, loss, gU, gV = problem_and_reference(KOS_L2)
    model = fit_kos(tm, p, 1, user_alpha=alpha, item_alpha=alpha)
    assert model._state.wplan.sliced and model._state.l2 == [np.float32(2 * alpha)] * 2
    assert rel_err(model.loss_history_[0], loss) < 1e-5
    assert_step(host(model.user_embedding), p['U0'], gU + 2 * alpha * p['U0'].astype(np.float64), LR, rtol=1e-5, what='l2 U')
    assert_step(host(model.item_embedding), p['V0'], gV + 2 * alpha * p['V0'].astype(np.float64), LR, rtol=1e-5, what='l2 V')


def test_resampling_every_epoch_is_three_chained_fits(tm, engine_only):
    """fit(3, resample_every=1) = fit(1) on random_ind, on T_1 and on T_2, each from the tables the one before left."""
    p, seed = kos_problem(KOS_REPLAY), 21
    whole = fit_kos(tm, p, 3, resample_every=1, sample_seed=seed)
    assert whole.resample_rounds_ == 3 and whole._state.wplan.omega is not None
    U, V, history = p['U0'], p['V0'], []
    for j in range(3):
        q = dict(p, R=p['R'] if j == 0 else tm.ops.sample_negatives(p['n'], p['m'], p['S'], seed=seed + j, device='cuda').cpu().numpy())
        one = fit_kos(tm, q, 1, U0=U, V0=V)
        U, V = host(one.user_embedding), host(one.item_embedding)
        history += one.loss_history_
    assert whole.loss_history_ == history
    assert np.array_equal(host(whole.user_embedding), U) and np.array_equal(host(whole.item_embedding), V)
    static = fit_kos(tm, p, 3)
    assert static.loss_history_[0] == whole.loss_history_[0] and static.loss_history_[1:] != whole.loss_history_[1:]


def test_graph_replay(tm, engine_only, monkeypatch):
    """200 x 150, r = 16, S = 32: twelve epochs - one replay of a twelve-epoch hipGraph - and thirteen give with TMF_NO_GRAPH=1 the
    same history and the same tables, bit for bit.  The first loss is the closed form's (the problem is decided)."""
    p, loss, _, _ = problem_and_reference(KOS_REPLAY)
    for epochs in (12, 13):
        monkeypatch.delenv('TMF_NO_GRAPH', raising=False)
        a = fit_kos(tm, p, epochs)
        monkeypatch.setenv('TMF_NO_GRAPH', '1')
        b = fit_kos(tm, p, epochs)
        assert a.graph_epochs_ == 12 and b.graph_epochs_ == 0
        assert a.loss_history_ == b.loss_history_ and len(a.loss_history_) == epochs
        assert torch.equal(a.user_embedding, b.user_embedding) and torch.equal(a.item_embedding, b.item_embedding)
        h = a.loss_history_
        print(f'[replay] {epochs} epochs: first {rel_err(h[0], loss):.3g}, history {h[0]:.4f} -> {h[-1]:.4f}')
        assert rel_err(h[0], loss) < 1e-5 and h[-1] < h[0]


def test_one_positive_per_user_is_a_warp_fit(tm, engine_only):
    """Every user has exactly one positive: omega is exactly 1, and KOSWARPLoss(1, 1) - any k and n - trains the bits of WARPLoss."""
    p = single_positive_problem()
    g_min, b = decidedness(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    assert g_min > b
    warp = fit_kos(tm, p, 3, loss=tm.WARP())
    for k, n in ((1, 1), (5, 10)):
        kos = fit_kos(tm, p, 3, loss=tm.KOS(k, n))
        assert set(kos._state.wplan.omega.cpu().tolist()) == {0.0, 1.0}
        assert kos.loss_history_ == warp.loss_history_ and warp.loss_history_[0] > 0
        assert torch.equal(kos.user_embedding, warp.user_embedding) and torch.equal(kos.item_embedding, warp.item_embedding)


def test_no_sample_table_on_the_engine(tm, engine_only):
    from test_warp_cpu import warp_problem
    p = warp_problem(15, 12, 9, 4, 4)
    with pytest.raises(tm.Missing, match='KOSWARPLoss'):
        fit_kos(tm, p, 1, table=False)


def test_a_kos_fit_leaves_nothing_behind(tm, engine_only):
    p = kos_problem(KOS_GEOMETRY[(33, 70)])
    before = fit_kos(tm, p, 3, loss=tm.WARP())
    kos = fit_kos(tm, p, 3)
    after = fit_kos(tm, p, 3, loss=tm.WARP())
    assert before.loss_history_ == after.loss_history_ and before.loss_history_ != kos.loss_history_
    assert torch.equal(before.user_embedding, after.user_embedding) and torch.equal(before.item_embedding, after.item_embedding)
    assert before._state.wplan.__dict__.get('omega') is None and kos._state.wplan.omega is not None
