"""tmf_als_cg_rows_f32 / tmf_gram_wide_f32 and fit_als(solver='cg') on the GPU, against the NumPy fp64 oracle (als_cg_ref.py).

The cases are test_gpu_als.py's (make_case: 40 rows against 257 - an empty row, a one-entry row, a row holding every column, a
3000-entry row with repeated columns, the rest at 10 % density; reg 0.5, alpha 2.0) with a random starting table x0 scaled by 1/sqrt(r).
Bounds.  A solved row is compared norm-wise (conftest.rel_err) with the fp64 oracle of the SAME iteration (the same cg_steps from the
same x0) at the project bound 1e-5; every test first asserts that the oracle run in fp32 is within 2.5e-6 of fp64 on the case, which
leaves plain fp32 arithmetic a factor 4.  The long row is bounded by max(1e-5, 4 x its own fp32-oracle error): the factor covers a
summation order other than NumPy's over 3000 terms.  cg_steps = 8 is not used at r >= 192 for these bounds: the fp32 oracle itself
reaches 9.8e-6 there.  Rankings follow test_gpu_als.decided_positions."""
import numpy as np
import pytest
import torch

from als_cg_ref import als_cg_ref, cg_half_step_ref, cg_rows_ref
from als_ref import als_ref, entry_terms_ref
from conftest import rel_err
from test_als_cpu import ALPHA, REG, make_model
from test_gpu_als import (BIG_M, BIG_N, EMPTY_ROW, FULL_ROW, KERNEL_REG, LONG, N_OTHER, N_ROWS, TF_REG, TF_SCALE, big_data, decided_positions,
                          make_case)
from test_gpu_strided_views import GUARD, POISONS, embed

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 4, 63, 64, 65, 127, 128, 129, 192, 255, 256]


@pytest.fixture(scope='module')
def ops():
    from teamoflow_amd import _lib, _ops
    _lib.get()
    return _ops


def cg_case(r, implicit):
    """make_case(r, implicit) with x0 [N_ROWS, r] fp32 added - cached; refs(steps) adds the oracle's results per cg_steps."""
    key = (r, implicit)
    if key not in cg_case.cache:
        case = dict(make_case(r, implicit))
        rng = np.random.default_rng(77 + 2 * r + implicit)
        case['x0'] = (rng.standard_normal((N_ROWS, r)) / np.sqrt(r)).astype(np.float32)
        case['cg'] = {}
        cg_case.cache[key] = case
    return cg_case.cache[key]


cg_case.cache = {}


def refs(case, steps, x0=True):
    """(fp64 oracle [N_ROWS, r], fp32 oracle's rel_err on the short rows, on the long row) for cg_steps = steps - cached."""
    key = (steps, x0)
    if key not in case['cg']:
        args = (case['Y'], case['G0'], case['rowptr'], case['col'], case['w'], case['t'], KERNEL_REG, case['x0'] if x0 else None, steps)
        ref, ref32 = cg_rows_ref(*args), cg_rows_ref(*args, dtype=np.float32)
        short = case['short']
        case['cg'][key] = (ref, rel_err(ref32[short], ref[short]), rel_err(ref32[LONG], ref[LONG]))
    return case['cg'][key]


def solve(ops, case, steps, x0=True, **kw):
    return ops.als_cg_rows(torch.tensor(case['Y']), torch.tensor(case['rowptr']), torch.tensor(case['col']), torch.tensor(case['w']),
                           torch.tensor(case['t']), KERNEL_REG, G0=None if case['G0'] is None else torch.tensor(case['G0']),
                           x0=torch.tensor(case['x0']) if x0 is True else x0, cg_steps=steps, **kw)


# ------------------------------------------------------------------ 1. the kernel against fp64
@pytest.mark.parametrize('steps', [1, 3])
@pytest.mark.parametrize('implicit', [True, False])
@pytest.mark.parametrize('r', WIDTHS)
def test_cg_rows_against_fp64(ops, r, implicit, steps):
    case = cg_case(r, implicit)
    ref, e_short, e_long = refs(case, steps)
    print(f'r={r} implicit={implicit} steps={steps}: fp32 oracle {e_short:.3g} (short rows), {e_long:.3g} (long row)')
    assert e_short <= 2.5e-6, e_short
    X, failed = solve(ops, case, steps)
    got = X.cpu().numpy()
    g_short, g_long = rel_err(got[case['short']], ref[case['short']]), rel_err(got[LONG], ref[LONG])
    print(f'r={r} implicit={implicit} steps={steps}: kernel {g_short:.3g} (short rows), {g_long:.3g} (long row)')
    assert int(failed) == 0
    assert not got[EMPTY_ROW].any()
    assert g_short <= 1e-5, g_short
    assert g_long <= max(1e-5, 4 * e_long), (g_long, e_long)
    assert tuple(X.shape) == (N_ROWS, r) and X.dtype == torch.float32


# ------------------------------------------------------------------ 2. the stop rule
@pytest.mark.parametrize('implicit', [True, False])
@pytest.mark.parametrize('r', [1, 3, 4])
def test_more_steps_than_dimensions_stop_cleanly(ops, r, implicit):
    case = cg_case(r, implicit)
    ref, e_short, _ = refs(case, 8)
    assert e_short <= 2.5e-6, e_short
    X, failed = solve(ops, case, 8)
    got = X.cpu().numpy()
    assert np.isfinite(got).all() and int(failed) == 0
    assert rel_err(got[case['short']], ref[case['short']]) <= 1e-5
    X2, failed = solve(ops, case, 8, x0=X.clone())
    assert bool(torch.isfinite(X2).all()) and int(failed) == 0
    assert rel_err(X2.cpu().numpy(), got.astype(np.float64)) < 1e-5


# ------------------------------------------------------------------ 3. layout
@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('r', [3, 65, 128, 129, 256])
def test_layout_padding_guards_and_skipped_rows(ops, r, in_place):
    from teamoflow_amd import _lib
    lib = _lib.get()
    case = cg_case(r, True)
    want, _ = solve(ops, case, 3)
    ids_np = np.array([5, LONG, EMPTY_ROW, 17, FULL_ROW], dtype=np.int32)
    ids = torch.tensor(ids_np, device='cuda')
    named = np.zeros(N_ROWS, bool)
    named[ids_np] = True
    named_t = torch.tensor(named, device='cuda')
    rowptr, col = torch.tensor(case['rowptr'], device='cuda'), torch.tensor(case['col'], device='cuda')
    w, t = torch.tensor(case['w'], device='cuda'), torch.tensor(case['t'], device='cuda')
    ld = _lib.padded_ld(r) + 4
    for poison in POISONS:
        Y, _ = embed(torch.tensor(case['Y']), ld, row_step=2, poison=poison)          # padding columns and every other row poisoned
        G0, _ = embed(torch.tensor(case['G0']), r + 3, poison=poison)
        if in_place:   # X holds x0; its padding columns are overwritten with zeros where a row is solved
            X, buffer = embed(torch.tensor(case['x0']), ld, poison=-12345.0)
            X0, ldx0 = X, ld
        else:
            X, buffer = embed(torch.full((N_ROWS, r), -7.0), ld, poison=-12345.0)
            X0, _ = embed(torch.tensor(case['x0']), ld + 4, row_step=2, poison=poison)
            ldx0 = X0.stride(0)
        buffer[GUARD:GUARD + N_ROWS, r:] = -9.0
        before = buffer.clone()
        n_failed = torch.zeros(1, dtype=torch.int32, device='cuda')
        _lib.check(lib.tmf_als_cg_rows_f32(_lib.ptr(Y), N_OTHER, r, Y.stride(0), _lib.ptr(G0), G0.stride(0), _lib.ptr(rowptr),
                                           _lib.ptr(col), _lib.ptr(w), _lib.ptr(t), KERNEL_REG, _lib.ptr(ids), ids.numel(),
                                           _lib.ptr(X0), ldx0, _lib.ptr(X), ld, 3, _lib.ptr(n_failed), _lib.stream_ptr()), lib)
        torch.cuda.synchronize()
        assert int(n_failed) == 0
        rows = buffer[GUARD:GUARD + N_ROWS]
        assert torch.equal(rows[named_t][:, :r], want[named_t]), poison                # the bits of the plain launch
        assert not rows[named_t][:, r:].any(), poison                                  # padding exactly zero
        assert torch.equal(rows[~named_t], before[GUARD:GUARD + N_ROWS][~named_t])    # rows not named: untouched
        assert torch.equal(buffer[:GUARD], before[:GUARD]) and torch.equal(buffer[GUARD + N_ROWS:], before[GUARD + N_ROWS:])


# ------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize('implicit', [True, False])
@pytest.mark.parametrize('r', [3, 64, 128, 256])
def test_bits_do_not_depend_on_the_launch(ops, r, implicit):
    case = cg_case(r, implicit)
    X1, _ = solve(ops, case, 3)
    X2, _ = solve(ops, case, 3)
    assert torch.equal(X1, X2)
    perm = np.random.default_rng(r).permutation(N_ROWS)
    X3, failed = solve(ops, case, 3, ids=perm)
    assert int(failed) == 0 and torch.equal(X3, X1)
    ids = [LONG, 0, 11, 3, N_ROWS - 1, 20, FULL_ROW, 1, 30]   # nine rows: other neighbours in the batch
    X4, failed = solve(ops, case, 3, ids=ids)
    named = torch.zeros(N_ROWS, dtype=torch.bool, device='cuda')
    named[torch.tensor(ids, device='cuda')] = True
    assert int(failed) == 0
    assert torch.equal(X4[named], X1[named]) and not X4[~named].any()


# ------------------------------------------------------------------ 5. a matrix that is not positive definite
@pytest.mark.parametrize('implicit', [True, False])
@pytest.mark.parametrize('r', [4, 128])
def test_indefinite_row_fails_alone(ops, r, implicit):
    """w = -100 on every entry of the row that holds every column: p^T A p <= 0 on the first step.  The kernel writes zeros and counts
    the row - handled by contract, nothing faults."""
    case = dict(cg_case(r, implicit))
    others = [i for i in range(N_ROWS) if i != FULL_ROW]
    want, _ = solve(ops, case, 3, ids=others)
    w = case['w'].copy()
    w[case['rowptr'][FULL_ROW]:case['rowptr'][FULL_ROW + 1]] = -100.0
    case['w'] = w
    X, failed = solve(ops, case, 3)
    assert int(failed) == 1
    assert not X[FULL_ROW].any()
    keep = torch.tensor(others, device='cuda')
    assert torch.equal(X[keep], want[keep])


# ------------------------------------------------------------------ 6. the wide Gram matrix
@pytest.mark.parametrize('n', [1, 257, 5000])
@pytest.mark.parametrize('r', [129, 192, 255, 256])
def test_gram_wide(ops, r, n):
    rng = np.random.default_rng(7 * r + n)
    T = rng.standard_normal((n, r)).astype(np.float32)
    view, _ = embed(torch.tensor(T), 260, poison=float('nan'))
    G = ops.gram(view)
    ref = T.astype(np.float64).T @ T.astype(np.float64)
    assert tuple(G.shape) == (r, r) and rel_err(G.cpu().numpy(), ref) <= 1e-5
    assert torch.equal(G, G.T)
    assert torch.equal(G, ops.gram(view)) and torch.equal(G, ops.gram(torch.tensor(T)))


def test_gram_at_128_is_still_the_narrow_entry_point(ops):
    from teamoflow_amd import _lib
    lib = _lib.get()
    T = torch.randn(5000, 128, device='cuda')
    G = torch.empty(128, 128, device='cuda')
    ws = torch.empty(lib.tmf_gram_workspace_bytes(5000, 128), dtype=torch.uint8, device='cuda')
    _lib.check(lib.tmf_gram_f32(_lib.ptr(T), 5000, 128, 128, _lib.ptr(G), 128, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), lib)
    assert torch.equal(ops.gram(T), G)


# ------------------------------------------------------------------ 7. teacher-forced half-steps through fit's path
@pytest.mark.parametrize('implicit', [True, False])
@pytest.mark.parametrize('r', [32, 128, 256])
def test_teacher_forced_half_steps_in_place(ops, r, implicit):
    """Every half-step of the oracle starts from the GPU's own previous tables, so the bound is on one half-step (Gram included); the
    GPU runs in place with permuted ids, as fit does."""
    from teamoflow_amd import _engine, _lib
    idx, val = big_data(r)
    val = (val * TF_SCALE).astype(np.float32)
    rng = np.random.default_rng(r + 1)
    plan = _engine.InteractionPlan(torch.tensor(idx, device='cuda'), torch.tensor(val, device='cuda'), BIG_M, BIG_N, user_chunks=1)
    ld = _lib.padded_ld(r)
    tables = [torch.zeros(BIG_M, ld, device='cuda')[:, :r], torch.zeros(BIG_N, ld, device='cuda')[:, :r]]
    for T in tables:
        T.copy_(torch.tensor((rng.standard_normal(tuple(T.shape)) / np.sqrt(r)).astype(np.float32)))
    sides = ((plan.rowptr_u, plan.col_u, plan.val_u, BIG_M, (0, 1)), (plan.rowptr_i, plan.row_i, plan.val_i, BIG_N, (1, 0)))
    worst = 0.0
    for half in range(4):
        rowptr, col, a, n_rows, (rc, cc) = sides[half % 2]
        X, Y = tables[half % 2], tables[1 - half % 2]
        w, t, _ = (torch.tensor(x, device='cuda') for x in entry_terms_ref(a.cpu().numpy(), ALPHA, implicit, np.float32))
        ids = torch.tensor(rng.permutation(n_rows), device='cuda')
        Xn, Yn = X.cpu().numpy(), Y.cpu().numpy()
        want = cg_half_step_ref(Yn.astype(np.float64), Xn, idx[:, rc], idx[:, cc], val, n_rows, TF_REG, ALPHA, implicit, 3)
        err32 = rel_err(cg_half_step_ref(Yn, Xn, idx[:, rc], idx[:, cc], val, n_rows, TF_REG, ALPHA, implicit, 3, dtype=np.float32), want)
        assert err32 <= 2.5e-6, (half, err32)
        out, failed = ops.als_cg_rows(Y, rowptr, col, w, t, TF_REG, G0=ops.gram(Y) if implicit else None, ids=ids, x0=X, out=X, cg_steps=3)
        assert int(failed) == 0 and out.data_ptr() == X.data_ptr()
        err = rel_err(X.cpu().numpy(), want)
        worst = max(worst, err)
        assert err <= 1e-5, (half, err)
    print(f'teacher-forced r={r} implicit={implicit}: worst half-step {worst:.3g}')


# ------------------------------------------------------------------ 8. the API
@pytest.mark.parametrize('implicit', [True, False])
def test_fit_als_cg_on_the_gpu(implicit):
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    idx, val = big_data(2)
    model, U0, V0 = make_model(r=32, seed=3, m=BIG_M, n=BIG_N)
    train = SparseInteractions(idx, val, (BIG_M, BIG_N))
    model.fit_als(15, eye(BIG_M), eye(BIG_N), train, reg=REG, alpha=ALPHA, implicit=implicit, solver='cg', cg_steps=3)
    assert model.user_embedding.is_cuda
    ref = als_cg_ref(U0, V0, idx, val, 15, REG, ALPHA, implicit, 3)
    L = np.array(model.loss_history_)
    print(f'implicit={implicit}: loss history {L}, oracle {ref["loss"]}')
    assert len(L) == 15 and rel_err(L, ref['loss']) <= 1e-5
    assert np.all(np.diff(L) <= 1e-6 * L[0]), np.diff(L) / L[0]
    if not implicit:
        return   # 15 sweeps of 3 steps are not converged in explicit mode (the fp64 oracles: 1.15 x the exact sweeps' loss): no claim
    exact = als_ref(U0, V0, idx, val, 15, REG, ALPHA, True)
    assert L[14] <= 1.01 * exact['loss'][14], (L[14], exact['loss'][14])
    # the rankings of the fitted model against its own tables in fp64
    U, V = model.user_embedding.cpu().numpy().astype(np.float64), model.item_embedding.cpu().numpy().astype(np.float64)
    excluded = np.zeros((BIG_M, BIG_N), bool)
    excluded[idx[val != 0, 0], idx[val != 0, 1]] = True
    want, decided = decided_positions(U @ V.T, 10, excluded)
    top = model.retrieve_user_recs(k=10, exclude=train)
    assert (top[decided] == want[decided]).all()
    assert 1.0 - decided.all(axis=1).mean() <= 0.10


# ------------------------------------------------------------------ 9. a CSR without entries
def test_a_csr_without_entries_gives_zeros(ops):
    """q > 0 rows and no stored entry at all: every row is a row without entries, whatever x0 holds."""
    Y = torch.randn(N_OTHER, 8, device='cuda')
    empty = torch.zeros(0)
    for G0 in (None, ops.gram(Y)):
        for x0 in (None, torch.randn(5, 8, device='cuda')):
            X, failed = ops.als_cg_rows(Y, torch.zeros(6, dtype=torch.int64), empty.int(), empty, empty, 0.5, G0=G0, x0=x0)
            assert tuple(X.shape) == (5, 8) and not X.any() and int(failed) == 0


def test_argument_errors(ops):
    case = cg_case(4, False)
    r = case['Y'].shape[1]
    args = (torch.tensor(case['Y']), torch.tensor(case['rowptr']), torch.tensor(case['col']), torch.tensor(case['w']), torch.tensor(case['t']))
    for bad in (dict(cg_steps=0), dict(cg_steps=33), dict(x0=torch.zeros(N_ROWS, r + 1))):
        with pytest.raises(ValueError):
            ops.als_cg_rows(*args, 0.5, **bad)
    with pytest.raises(ValueError):
        ops.als_cg_rows(torch.zeros(N_OTHER, 257), *args[1:], 0.5)
    X = torch.zeros(N_ROWS, 4 * ((r + 3) // 4), device='cuda')[:, :r]
    with pytest.raises(ValueError):
        ops.als_cg_rows(*args, 0.5, x0=X, out=X, ids=[1, 2, 1])   # in place and a row named twice
