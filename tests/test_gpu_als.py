"""tmf_gram_f32 / tmf_als_solve_rows_f32 and the ALS API on the GPU, against the NumPy fp64 oracle (als_ref.py).

Bounds.  A solved row is compared norm-wise (conftest.rel_err) with the fp64 oracle at the project bound 1e-5; on every case the test
first asserts that the oracle itself, run in fp32 (NumPy / LAPACK, the reference alone), is within 2.5e-6 of fp64 - the cases are
conditioned so that plain fp32 arithmetic has a factor 4 of room.  The one long row (3000 entries, repeated columns) is bounded by
max(1e-5, 4 x its own fp32-oracle error): the factor covers a summation order other than NumPy's over 3000 terms.
Rankings follow test_gpu_similar.py's per-position rule: where the fp64 score at a list position is more than 2e-5 x max |score|
from both neighbours in the oracle's top-(k + 1), the position must hold the oracle's id; at most 10 % of the queries may have an
undecided position."""
import ctypes

import numpy as np
import pytest
import torch

from als_ref import als_ref, entry_terms_ref, half_step_ref, solve_rows_ref
from conftest import rel_err
from test_als_cpu import ALPHA, EPOCHS, M, N, R, REG, make_data, make_model
from test_gpu_strided_views import GUARD, POISONS, embed

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 4, 63, 64, 65, 127, 128]
N_OTHER, N_ROWS, LONG = 257, 40, 39
EMPTY_ROW, ONE_ROW, FULL_ROW = 0, 1, 2
KERNEL_REG, KERNEL_ALPHA = 0.5, 2.0


@pytest.fixture(scope='module')
def ops():
    from teamoflow_amd import _lib, _ops
    _lib.get()
    return _ops


def make_case(r, implicit, seed=0):
    """dict(Y fp32, G0 fp32 or None, rowptr, col, w, t, ref fp64 [N_ROWS, r], err32: the fp32 oracle's rel_err on the short rows and on
    the long row) - cached per (r, implicit, seed)."""
    key = (r, implicit, seed)
    if key in make_case.cache:
        return make_case.cache[key]
    rng = np.random.default_rng(1000 * seed + 2 * r + implicit)
    Y = (rng.standard_normal((N_OTHER, r)) / np.sqrt(r)).astype(np.float32)
    cols, vals = [], []
    for i in range(N_ROWS):
        if i == EMPTY_ROW:
            c = np.zeros(0, np.int64)
        elif i == ONE_ROW:
            c = np.array([N_OTHER - 1])
        elif i == FULL_ROW:
            c = np.arange(N_OTHER)
        elif i == LONG:
            c = rng.integers(0, N_OTHER, 3000)
        else:
            c = np.flatnonzero(rng.random(N_OTHER) < 0.1)
        cols.append(c)
        vals.append(rng.integers(1, 6, len(c)) if i == LONG else rng.integers(-2, 6, len(c)))
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    col, a = np.concatenate(cols).astype(np.int32), np.concatenate(vals).astype(np.float32)
    w, t, _ = entry_terms_ref(a, KERNEL_ALPHA, implicit, np.float32)
    G0 = (Y.astype(np.float64).T @ Y.astype(np.float64)).astype(np.float32) if implicit else None
    ref = solve_rows_ref(Y, G0, rowptr, col, w, t, KERNEL_REG)
    ref32 = solve_rows_ref(Y, G0, rowptr, col, w, t, KERNEL_REG, dtype=np.float32)
    short = np.arange(N_ROWS) != LONG
    case = dict(Y=Y, G0=G0, rowptr=rowptr, col=col, w=w, t=t, ref=ref, short=short,
                err32=(rel_err(ref32[short], ref[short]), rel_err(ref32[LONG], ref[LONG])))
    make_case.cache[key] = case
    return case


make_case.cache = {}


def solve(ops, case, **kw):
    X, failed = ops.als_solve_rows(torch.tensor(case['Y']), torch.tensor(case['rowptr']), torch.tensor(case['col']),
                                   torch.tensor(case['w']), torch.tensor(case['t']), KERNEL_REG,
                                   G0=None if case['G0'] is None else torch.tensor(case['G0']), **kw)
    return X, failed


# ------------------------------------------------------------------ 1. the kernel against fp64
@pytest.mark.parametrize('implicit', [True, False])
@pytest.mark.parametrize('r', WIDTHS)
def test_solve_rows_against_fp64(ops, r, implicit):
    case = make_case(r, implicit)
    e_short, e_long = case['err32']
    print(f'r={r} implicit={implicit}: fp32 oracle {e_short:.3g} (short rows), {e_long:.3g} (long row)')
    assert e_short <= 2.5e-6, e_short
    X, failed = solve(ops, case)
    got = X.cpu().numpy()
    g_short, g_long = rel_err(got[case['short']], case['ref'][case['short']]), rel_err(got[LONG], case['ref'][LONG])
    print(f'r={r} implicit={implicit}: kernel {g_short:.3g} (short rows), {g_long:.3g} (long row)')
    assert int(failed) == 0
    assert not got[EMPTY_ROW].any()
    assert g_short <= 1e-5, g_short
    assert g_long <= max(1e-5, 4 * e_long), (g_long, e_long)
    assert tuple(X.shape) == (N_ROWS, r) and X.dtype == torch.float32


# ------------------------------------------------------------------ 2. layout
@pytest.mark.parametrize('r', [3, 65, 128])
def test_layout_padding_guards_and_skipped_rows(ops, r):
    from teamoflow_amd import _lib
    lib = _lib.get()
    case = make_case(r, True)
    want, _ = solve(ops, case)
    ids_np = np.array([5, LONG, EMPTY_ROW, 17, FULL_ROW, 5], dtype=np.int32)
    ids = torch.tensor(ids_np, device='cuda')
    named = np.zeros(N_ROWS, bool)
    named[ids_np] = True
    rowptr, col = torch.tensor(case['rowptr'], device='cuda'), torch.tensor(case['col'], device='cuda')
    w, t = torch.tensor(case['w'], device='cuda'), torch.tensor(case['t'], device='cuda')
    ld = _lib.padded_ld(r) + 4
    for poison in POISONS:
        Y, _ = embed(torch.tensor(case['Y']), ld, row_step=2, poison=poison)          # padding columns and every other row poisoned
        G0, _ = embed(torch.tensor(case['G0']), r + 3, poison=poison)
        X, buffer = embed(torch.full((N_ROWS, r), -7.0), ld, poison=-12345.0)
        buffer[GUARD:GUARD + N_ROWS, r:] = -9.0                                      # padding columns of X: written as zeros where a row is solved
        before = buffer.clone()
        n_failed = torch.zeros(1, dtype=torch.int32, device='cuda')
        _lib.check(lib.tmf_als_solve_rows_f32(_lib.ptr(Y), N_OTHER, r, Y.stride(0), _lib.ptr(G0), G0.stride(0), _lib.ptr(rowptr),
                                              _lib.ptr(col), _lib.ptr(w), _lib.ptr(t), KERNEL_REG, _lib.ptr(ids), ids.numel(),
                                              _lib.ptr(X), ld, _lib.ptr(n_failed), _lib.stream_ptr()), lib)
        torch.cuda.synchronize()
        assert int(n_failed) == 0
        rows = buffer[GUARD:GUARD + N_ROWS]
        named_t = torch.tensor(named, device='cuda')
        assert torch.equal(rows[named_t][:, :r], want[named_t]), poison                # the bits of the plain launch
        assert not rows[named_t][:, r:].any(), poison                                  # padding exactly zero
        assert torch.equal(rows[~named_t], before[GUARD:GUARD + N_ROWS][~named_t])    # rows not named: untouched
        assert torch.equal(buffer[:GUARD], before[:GUARD]) and torch.equal(buffer[GUARD + N_ROWS:], before[GUARD + N_ROWS:])


# ------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize('implicit', [True, False])
@pytest.mark.parametrize('r', [3, 64, 128])
def test_bits_do_not_depend_on_the_launch(ops, r, implicit):
    case = make_case(r, implicit)
    X1, _ = solve(ops, case)
    X2, _ = solve(ops, case)
    assert torch.equal(X1, X2)
    ids = [LONG, 0, 11, LONG, 3, 0, N_ROWS - 1, 20, 11]
    X3, failed = solve(ops, case, ids=ids)
    named = torch.zeros(N_ROWS, dtype=torch.bool, device='cuda')
    named[torch.tensor(ids, device='cuda')] = True
    assert int(failed) == 0
    assert torch.equal(X3[named], X1[named]) and not X3[~named].any()


# ------------------------------------------------------------------ 4. the Gram matrix
@pytest.mark.parametrize('n', [1, 5, 257, 5000])
@pytest.mark.parametrize('r', WIDTHS)
def test_gram(ops, r, n):
    rng = np.random.default_rng(7 * r + n)
    T = rng.standard_normal((n, r)).astype(np.float32)
    view, _ = embed(torch.tensor(T), 132, poison=float('nan'))
    G = ops.gram(view)
    ref = T.astype(np.float64).T @ T.astype(np.float64)
    assert tuple(G.shape) == (r, r) and rel_err(G.cpu().numpy(), ref) <= 1e-5
    assert torch.equal(G, G.T)
    assert torch.equal(G, ops.gram(view)) and torch.equal(G, ops.gram(torch.tensor(T)))


# ------------------------------------------------------------------ 5. a matrix that is not positive definite
@pytest.mark.parametrize('implicit', [True, False])
@pytest.mark.parametrize('r', [4, 128])
def test_indefinite_row_fails_alone(ops, r, implicit):
    """w = -100 on every entry of the row that holds every column: A = G0 + reg I - 100 Y^T Y is indefinite.  The kernel meets a
    pivot <= 0, writes zeros and counts the row - handled by contract, nothing faults."""
    case = dict(make_case(r, implicit))
    others = [i for i in range(N_ROWS) if i != FULL_ROW]
    want, _ = solve(ops, case, ids=others)
    w = case['w'].copy()
    w[case['rowptr'][FULL_ROW]:case['rowptr'][FULL_ROW + 1]] = -100.0
    case['w'] = w
    X, failed = solve(ops, case)
    assert int(failed) == 1
    assert not X[FULL_ROW].any()
    keep = torch.tensor(others, device='cuda')
    assert torch.equal(X[keep], want[keep])


# ------------------------------------------------------------------ 6. argument errors
def test_argument_errors_launch_nothing(ops):
    from teamoflow_amd import _lib
    lib = _lib.get()
    r = 8
    case = make_case(r, False)
    Y = torch.zeros(N_OTHER + 1, 8, device='cuda')
    rowptr, col = torch.tensor(case['rowptr'], device='cuda'), torch.tensor(case['col'], device='cuda')
    w, t = torch.tensor(case['w'], device='cuda'), torch.tensor(case['t'], device='cuda')
    X = torch.full((N_ROWS, 8), -3.0, device='cuda')
    n_failed = torch.zeros(1, dtype=torch.int32, device='cuda')

    def call(r=r, reg=0.5, y=Y.data_ptr(), ldx=8, q=N_ROWS):
        return lib.tmf_als_solve_rows_f32(ctypes.c_void_p(y), N_OTHER, r, 8, None, 0, _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(w),
                                          _lib.ptr(t), reg, None, q, _lib.ptr(X), ldx, _lib.ptr(n_failed), _lib.stream_ptr())
    for bad in (dict(reg=0.0), dict(reg=float('nan')), dict(r=0), dict(r=129), dict(y=Y.data_ptr() + 4), dict(ldx=7)):
        assert call(**bad) == -1, bad   # TMF_E_INVALID
    assert call(q=0) == 0
    torch.cuda.synchronize()
    assert bool((X == -3.0).all()) and int(n_failed) == 0
    for bad in (dict(reg=0.0), dict(reg=float('nan'))):
        with pytest.raises(ValueError):
            ops.als_solve_rows(Y[:N_OTHER], rowptr, col, w, t, **bad)
    with pytest.raises(IndexError):
        ops.als_solve_rows(Y[:5], rowptr, col, w, t, 0.5)             # columns beyond the table
    with pytest.raises(IndexError):
        ops.als_solve_rows(Y[:N_OTHER], rowptr, col, w, t, 0.5, ids=[N_ROWS])
    with pytest.raises(ValueError):
        ops.als_solve_rows(torch.zeros(N_OTHER, 129), rowptr, col, w, t, 0.5)


# ------------------------------------------------------------------ 7. the API
@pytest.mark.parametrize('implicit', [True, False])
def test_fit_als_matches_the_oracle_on_the_gpu(implicit):
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    idx, val = make_data()
    model, U0, V0 = make_model()
    model.fit_als(EPOCHS, eye(M), eye(N), SparseInteractions(idx, val, (M, N)), reg=REG, alpha=ALPHA, implicit=implicit)
    ref = als_ref(U0, V0, idx, val, EPOCHS, REG, ALPHA, implicit)
    assert model.user_embedding.is_cuda
    eu = rel_err(model.user_embedding.cpu().numpy(), ref['U'][-1])
    ev = rel_err(model.item_embedding.cpu().numpy(), ref['V'][-1])
    el = rel_err(model.loss_history_, ref['loss'])
    print(f'fit_als implicit={implicit}: U {eu:.3g}, V {ev:.3g}, loss {el:.3g}')
    assert eu <= 1e-5 and ev <= 1e-5 and el <= 1e-5, (eu, ev, el)


BIG_M, BIG_N = 300, 257
# The teacher-forced half-steps solve up to 128 components from about 26 entries per row, and every table is the previous solve's
# output.  With values in [-2, 5] and reg = 0.1 those tables grow until the systems have condition numbers of 1e3 - 1e4, where plain
# fp32 (the NumPy oracle in fp32) is itself 7e-5 to 6e-4 from fp64 in explicit mode.  The values are therefore scaled to [-0.2, 0.5]
# and the ridge is the kernel test's 0.5 - data terms and ridge of the same order: the fp32 oracle is then <= 1.2e-6 on all four cases
# (measured on the CPU), which the test asserts (<= 2.5e-6) before it judges the kernel.
TF_REG, TF_SCALE = 0.5, 0.1


def big_data(seed):
    rng = np.random.default_rng(seed)
    idx = np.argwhere(rng.random((BIG_M, BIG_N)) < 0.1)
    val = rng.integers(-2, 6, len(idx)).astype(np.float32)
    return idx, val


@pytest.mark.parametrize('implicit', [True, False])
@pytest.mark.parametrize('r', [32, 128])
def test_teacher_forced_half_steps_through_ids(ops, r, implicit):
    """Every half-step of the oracle starts from the GPU's own previous table, so the bound is on one half-step (Gram included)."""
    from teamoflow_amd import _engine
    idx, val = big_data(r)
    val = (val * TF_SCALE).astype(np.float32)
    rng = np.random.default_rng(r + 1)
    plan = _engine.InteractionPlan(torch.tensor(idx, device='cuda'), torch.tensor(val, device='cuda'), BIG_M, BIG_N, user_chunks=1)
    V = torch.tensor((rng.standard_normal((BIG_N, r)) / np.sqrt(r)).astype(np.float32), device='cuda')
    sides = ((plan.rowptr_u, plan.col_u, plan.val_u, BIG_M, (0, 1)), (plan.rowptr_i, plan.row_i, plan.val_i, BIG_N, (1, 0)))
    worst = 0.0
    for half in range(4):
        rowptr, col, a, n_rows, (rc, cc) = sides[half % 2]
        w, t, _ = (torch.tensor(x, device='cuda') for x in entry_terms_ref(a.cpu().numpy(), ALPHA, implicit, np.float32))
        ids = torch.tensor(rng.permutation(n_rows), device='cuda')
        X, failed = ops.als_solve_rows(V, rowptr, col, w, t, TF_REG, G0=ops.gram(V) if implicit else None, ids=ids)
        assert int(failed) == 0
        Vn = V.cpu().numpy()
        want = half_step_ref(Vn.astype(np.float64), idx[:, rc], idx[:, cc], val, n_rows, TF_REG, ALPHA, implicit)
        err32 = rel_err(half_step_ref(Vn, idx[:, rc], idx[:, cc], val, n_rows, TF_REG, ALPHA, implicit, dtype=np.float32), want)
        assert err32 <= 2.5e-6, (half, err32)
        err = rel_err(X.cpu().numpy(), want)
        worst = max(worst, err)
        assert err <= 1e-5, (half, err)
        V = X
    print(f'teacher-forced r={r} implicit={implicit}: worst half-step {worst:.3g}')


@pytest.fixture(scope='module')
def big_model():
    """(model, oracle, train): r = 32, 15 epochs, implicit - shared by the tests below and left unchanged."""
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    idx, val = big_data(2)
    model, U0, V0 = make_model(r=32, seed=3, m=BIG_M, n=BIG_N)
    train = SparseInteractions(idx, val, (BIG_M, BIG_N))
    model.fit_als(15, eye(BIG_M), eye(BIG_N), train, reg=REG, alpha=ALPHA)
    return model, als_ref(U0, V0, idx, val, 15, REG, ALPHA, True), train


def test_objective_never_rises(big_model):
    model, ref, _ = big_model
    L = np.array(model.loss_history_)
    print('loss history', L, 'oracle', ref['loss'])
    assert len(L) == 15 and np.all(np.diff(L) <= 1e-6 * L[0]), np.diff(L) / L[0]
    assert rel_err(L, ref['loss']) <= 1e-5


def decided_positions(S, k, excluded=None):
    """(oracle ids [q, k], decided [q, k]) by the per-position rule over fp64 scores S [q, n]."""
    R = S.copy()
    if excluded is not None:
        R[excluded] = -np.inf
    scale = float(np.abs(S).max())
    order = np.argsort(-R, axis=1, kind='stable')
    top = np.take_along_axis(R, order[:, :k + 1], 1)
    assert np.isfinite(top).all()
    wide = (top[:, :-1] - top[:, 1:]) > 2e-5 * scale
    decided = np.ones((S.shape[0], k), bool)
    decided[:, 1:] &= wide[:, :k - 1]
    decided &= wide[:, :k]
    return order[:, :k], decided


def test_fold_in_users_and_its_top_items(ops, big_model):
    from teamoflow_amd.mf.sparse import SparseInteractions
    model, _, _ = big_model
    rng = np.random.default_rng(11)
    idx = np.argwhere(rng.random((10, BIG_N)) < 0.1)
    val = rng.integers(-2, 6, len(idx)).astype(np.float32)
    before = model.item_embedding.clone()
    X = model.fold_in_users(SparseInteractions(idx, val, (10, BIG_N)), reg=REG, alpha=ALPHA)
    V = model.item_embedding.cpu().numpy().astype(np.float64)
    assert rel_err(X.cpu().numpy(), half_step_ref(V, idx[:, 0], idx[:, 1], val, 10, REG, ALPHA, True)) <= 1e-5
    assert torch.equal(model.item_embedding, before)
    top = ops.predict_topk(X, model.item_embedding, 10).cpu().numpy()
    want, decided = decided_positions(X.cpu().numpy().astype(np.float64) @ V.T, 10)
    assert (top[decided] == want[decided]).all()
    assert 1.0 - decided.all(axis=1).mean() <= 0.10


def test_rankings_agree_with_a_model_holding_the_oracles_tables(big_model):
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    model, ref, train = big_model
    other = MatrixFactorization(32)
    other.user_embedding = torch.tensor(ref['U'][-1].astype(np.float32), device='cuda')
    other.item_embedding = torch.tensor(ref['V'][-1].astype(np.float32), device='cuda')
    U, V = ref['U'][-1], ref['V'][-1]
    excluded = np.zeros((BIG_M, BIG_N), bool)
    seen = (train.values != 0).cpu().numpy()   # exclude= leaves out the stored entries with a value != 0 (_ops.build_exclusion)
    excluded[train.indices[:, 0].cpu().numpy()[seen], train.indices[:, 1].cpu().numpy()[seen]] = True
    want, decided = decided_positions(U @ V.T, 10, excluded)
    for m_ in (model, other):
        top = m_.retrieve_user_recs(k=10, exclude=train)
        assert (top[decided] == want[decided]).all()
    assert 1.0 - decided.all(axis=1).mean() <= 0.10
    Vn = V / np.maximum(np.linalg.norm(V, axis=1, keepdims=True), 1e-300)
    C = Vn @ Vn.T
    own = np.eye(BIG_N, dtype=bool)
    want, decided = decided_positions(C, 10, own)
    for m_ in (model, other):
        ids, sims = m_.similar_items(k=10)
        assert (ids[decided] == want[decided]).all()
        if m_ is other:   # its table is the oracle's: a reported similarity is that pair's fp64 cosine to 1e-5
            assert np.abs(sims - np.take_along_axis(C, ids.astype(np.int64), 1)).max() <= 1e-5
    assert 1.0 - decided.all(axis=1).mean() <= 0.10


def test_a_csr_without_entries_gives_zeros(ops):
    """q > 0 rows and no stored entry at all: every row is a row without entries."""
    Y = torch.randn(N_OTHER, 8, device='cuda')
    empty = torch.zeros(0)
    for G0 in (None, ops.gram(Y)):
        X, failed = ops.als_solve_rows(Y, torch.zeros(6, dtype=torch.int64), empty.int(), empty, empty, 0.5, G0=G0)
        assert tuple(X.shape) == (5, 8) and not X.any() and int(failed) == 0
