"""Alternating least squares where the suite runs without a GPU: the fp64 oracle's own properties, fit_als / fold_in_users /
fold_in_items against it (the chunked torch half-step without a GPU, the HIP kernel with one - the same bound), the conventions
(empty rows, duplicates, stored zeros), every refusal, save / load, and the C ABI's argument checks, which return before any launch."""
import os
import re

import numpy as np
import pytest
import torch

from als_ref import als_ref, csr_ref, entry_terms_ref, grad_u_ref, half_step_ref, objective_ref, solve_rows_ref
from conftest import ROOT, rel_err

M, N, R, EPOCHS, REG, ALPHA = 100, 50, 5, 5, 0.1, 2.0
EMPTY_USER, EMPTY_ITEM = 7, 3


def make_data(seed=0, m=M, n=N, density=0.1):
    """Integer values in [-2, 5] (zeros and negatives among them) at the given density, one duplicated pair, one user and one item
    without entries."""
    rng = np.random.default_rng(seed)
    mask = rng.random((m, n)) < density
    mask[EMPTY_USER, :] = False
    mask[:, EMPTY_ITEM] = False
    idx = np.argwhere(mask)
    val = rng.integers(-2, 6, len(idx)).astype(np.float32)
    idx = np.concatenate([idx, idx[:1]])            # a duplicate of the first pair, with another value
    val = np.concatenate([val, np.float32([3.0])])
    perm = rng.permutation(len(idx))                # COO order is the caller's
    return idx[perm], val[perm]


def make_model(r=R, seed=1, m=M, n=N):
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    rng = np.random.default_rng(seed)
    U0 = (rng.standard_normal((m, r)) / np.sqrt(r)).astype(np.float32)
    V0 = (rng.standard_normal((n, r)) / np.sqrt(r)).astype(np.float32)
    model = MatrixFactorization(r, user_weight_graph=FixedInitializer(U0), item_weight_graph=FixedInitializer(V0))
    model.verbose = False
    return model, U0, V0


@pytest.fixture(scope='module')
def fitted():
    """{implicit: (model, ref, idx, val)}: one fit and one oracle run per mode, shared and left unchanged."""
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    out = {}
    idx, val = make_data()
    for implicit in (True, False):
        model, U0, V0 = make_model()
        model.fit_als(EPOCHS, eye(M), eye(N), SparseInteractions(idx, val, (M, N)), reg=REG, alpha=ALPHA, implicit=implicit)
        out[implicit] = (model, als_ref(U0, V0, idx, val, EPOCHS, REG, ALPHA, implicit), idx, val)
    return out


# ------------------------------------------------------------------ the oracle
@pytest.mark.parametrize('implicit', [True, False])
def test_oracle_objective_never_rises_and_half_step_is_stationary(implicit):
    idx, val = make_data(seed=3)
    _, U0, V0 = make_model(seed=4)
    ref = als_ref(U0, V0, idx, val, 15, REG, ALPHA, implicit)
    L = ref['loss']
    assert np.all(np.diff(L) <= 1e-12 * abs(L[0])), L
    # after a user half-step from V the gradient of L with respect to U vanishes
    V = ref['V'][3]
    U = half_step_ref(V, idx[:, 0], idx[:, 1], val, M, REG, ALPHA, implicit)
    g, scale = grad_u_ref(U, V, idx, val, REG, ALPHA, implicit)
    assert np.abs(g).max() <= 1e-10 * scale, (np.abs(g).max(), scale)


# ------------------------------------------------------------------ fit_als
@pytest.mark.parametrize('implicit', [True, False])
def test_fit_als_matches_the_oracle(fitted, implicit):
    model, ref, _, _ = fitted[implicit]
    eu = rel_err(model.user_embedding.cpu().numpy(), ref['U'][-1])
    ev = rel_err(model.item_embedding.cpu().numpy(), ref['V'][-1])
    el = rel_err(model.loss_history_, ref['loss'])
    print(f'implicit={implicit}: U {eu:.3g}, V {ev:.3g}, loss {el:.3g}')
    assert len(model.loss_history_) == EPOCHS
    assert eu <= 1e-5 and ev <= 1e-5 and el <= 1e-5, (eu, ev, el)
    assert model.user_embedding.dtype == torch.float32 and tuple(model.user_embedding.shape) == (M, R)
    assert model.user_trainable[0] is model.user_embedding and model.item_trainable[0] is model.item_embedding
    assert model.fit_seconds_ > 0 and model.plan_seconds_ > 0


@pytest.mark.parametrize('implicit', [True, False])
def test_rows_without_entries_are_zero(fitted, implicit):
    model, _, idx, _ = fitted[implicit]
    assert EMPTY_USER not in idx[:, 0] and EMPTY_ITEM not in idx[:, 1]
    assert not model.user_embedding[EMPTY_USER].any() and not model.item_embedding[EMPTY_ITEM].any()
    assert bool(model.user_embedding[0].any()) and bool(model.item_embedding[0].any())


@pytest.mark.parametrize('implicit', [True, False])
def test_duplicate_entries_add_up(fitted, implicit):
    """Two stored values on one pair count as two entries: the same as ONE entry carrying the sums of their w and t."""
    from teamoflow_amd.mf.sparse import SparseInteractions
    model, _, _, _ = fitted[implicit]
    V = model.item_embedding.cpu().numpy().astype(np.float64)
    idx = np.array([[0, 4], [0, 9], [0, 4], [1, 9]])
    val = np.float32([2.0, 1.0, 5.0, -1.0])
    got = model.fold_in_users(SparseInteractions(idx, val, (2, N)), reg=REG, alpha=ALPHA, implicit=implicit).cpu().numpy()
    w, t, _ = entry_terms_ref(val, ALPHA, implicit)
    merged_w, merged_t = np.array([w[0] + w[2], w[1], w[3]]), np.array([t[0] + t[2], t[1], t[3]])
    want = solve_rows_ref(V, V.T @ V if implicit else None, np.array([0, 2, 3]), np.array([4, 9, 9]), merged_w, merged_t, REG)
    assert rel_err(got, want) <= 1e-5


def test_stored_zero_changes_nothing_in_implicit_mode(fitted):
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    base, _, idx, val = fitted[True]
    rng = np.random.default_rng(5)
    extra = np.stack([rng.integers(0, M, 40), rng.integers(0, N, 40)], axis=1)   # the empty user and item may get one too
    model, _, _ = make_model()
    model.fit_als(EPOCHS, eye(M), eye(N), SparseInteractions(np.concatenate([idx, extra]), np.concatenate([val, np.zeros(40, np.float32)]),
                                                             (M, N)), reg=REG, alpha=ALPHA, implicit=True)
    # w = t = 0: the entry adds exact zeros to A and b; only the order of the other terms may differ (a few fp32 roundings)
    assert rel_err(model.user_embedding.cpu().numpy(), base.user_embedding.cpu().numpy()) <= 1e-6
    assert rel_err(model.item_embedding.cpu().numpy(), base.item_embedding.cpu().numpy()) <= 1e-6
    assert rel_err(model.loss_history_, base.loss_history_) <= 1e-6


# ------------------------------------------------------------------ fold-in
@pytest.mark.parametrize('implicit', [True, False])
def test_fold_in_is_the_oracles_half_step_and_leaves_the_model_alone(fitted, implicit):
    from teamoflow_amd.mf.sparse import SparseInteractions
    model, ref, idx, val = fitted[implicit]
    U_before, V_before = model.user_embedding.clone(), model.item_embedding.clone()
    trainable, history = model.user_trainable, list(model.loss_history_)
    V = model.item_embedding.cpu().numpy().astype(np.float64)
    U = model.user_embedding.cpu().numpy().astype(np.float64)
    got_u = model.fold_in_users(SparseInteractions(idx, val, (M, N)), reg=REG, alpha=ALPHA, implicit=implicit)
    got_v = model.fold_in_items(SparseInteractions(idx[:, ::-1].copy(), val, (N, M)), reg=REG, alpha=ALPHA, implicit=implicit)
    assert got_u.dtype == torch.float32 and tuple(got_u.shape) == (M, R) and tuple(got_v.shape) == (N, R)
    assert rel_err(got_u.cpu().numpy(), half_step_ref(V, idx[:, 0], idx[:, 1], val, M, REG, ALPHA, implicit)) <= 1e-5
    assert rel_err(got_v.cpu().numpy(), half_step_ref(U, idx[:, 1], idx[:, 0], val, N, REG, ALPHA, implicit)) <= 1e-5
    assert torch.equal(model.user_embedding, U_before) and torch.equal(model.item_embedding, V_before)
    assert model.user_trainable is trainable and model.loss_history_ == history
    with pytest.raises(ValueError):
        model.fold_in_users(SparseInteractions(idx, val, (M, N + 1)))


def test_fold_in_upcasts_a_bf16_table(fitted):
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions
    base, _, idx, val = fitted[True]
    model = MatrixFactorization(R)
    model.factor_dtype = torch.bfloat16
    model.item_embedding = base.item_embedding.to(torch.bfloat16)
    model.user_embedding = base.user_embedding.to(torch.bfloat16)
    got = model.fold_in_users(SparseInteractions(idx, val, (M, N)), reg=REG, alpha=ALPHA)
    V = model.item_embedding.float().cpu().numpy().astype(np.float64)
    assert got.dtype == torch.float32
    assert rel_err(got.cpu().numpy(), half_step_ref(V, idx[:, 0], idx[:, 1], val, M, REG, ALPHA, True)) <= 1e-5


# ------------------------------------------------------------------ refusals
class CountingInitializer:
    def __init__(self):
        self.calls = 0

    def initialize_weights(self, n_features, n_components):
        self.calls += 1
        return torch.zeros(n_features, n_components)


def refused(exc, setup=None, features=None, **kw):
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    idx, val = make_data()
    init = CountingInitializer()
    model = MatrixFactorization(kw.pop('n_components', R), user_weight_graph=init, item_weight_graph=init, **kw.pop('ctor', {}))
    sentinel = object()
    model.user_trainable = sentinel
    if setup:
        setup(model)
    uf, itf = features or (eye(M), eye(N))
    with pytest.raises(exc):
        model.fit_als(2, uf, itf, SparseInteractions(idx, val, (M, N)), **kw)
    assert model.user_trainable is sentinel and init.calls == 0
    return model


@pytest.mark.parametrize('kw', [dict(reg=0.0), dict(reg=-1.0), dict(reg=float('nan')), dict(reg=float('inf')),
                                dict(alpha=-1.0), dict(alpha=float('nan')), dict(alpha=float('inf'))])
def test_bad_reg_and_alpha_raise_value_error(kw):
    refused(ValueError, **kw)


@pytest.mark.parametrize('name, value', [('factor_dtype', torch.bfloat16), ('batch_users', 16), ('shard_items', 2),
                                         ('data_parallel', 'force'), ('user_alpha', 0.1), ('item_alpha', 0.1)])
def test_unbuilt_settings_raise_before_any_weight_is_drawn(name, value):
    refused(NotImplementedError, setup=lambda model: setattr(model, name, value))


def test_unbuilt_widths_and_sides_raise_before_any_weight_is_drawn():
    from teamoflow_amd.mf.embedding_graphs import BiasedLinearEmbedding, ReLUEmbedding
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseFeatures, SparseInteractions, eye
    refused(NotImplementedError, n_components=129)
    refused(NotImplementedError, ctor=dict(user_repr_graph=BiasedLinearEmbedding()))
    refused(NotImplementedError, ctor=dict(item_repr_graph=ReLUEmbedding()))
    F = SparseFeatures(np.stack([np.arange(M), np.arange(M)], 1), np.ones(M, np.float32), (M, M))
    refused(NotImplementedError, features=(F, eye(N)))
    refused(NotImplementedError, features=(eye(M), torch.ones(N, N)))   # dense, but not the identity
    wide = MatrixFactorization(129)
    wide.item_embedding = torch.zeros(N, 129)
    wide.user_embedding = torch.zeros(M, 129)
    for call in (wide.fold_in_users, wide.fold_in_items):
        with pytest.raises(NotImplementedError):
            call(SparseInteractions(np.array([[0, 1]]), np.float32([1.0]), (1, N)))
    with pytest.raises(ValueError):
        MatrixFactorization(R).fold_in_users(SparseInteractions(np.array([[0, 1]]), np.float32([1.0]), (1, N)))   # nothing fitted


def test_dense_identity_features_are_accepted(fitted):
    from teamoflow_amd.mf.sparse import SparseInteractions
    base, _, idx, val = fitted[True]
    model, _, _ = make_model()
    model.fit_als(EPOCHS, torch.eye(M), np.eye(N, dtype=np.float32), SparseInteractions(idx, val, (M, N)), reg=REG, alpha=ALPHA)
    assert torch.equal(model.user_embedding, base.user_embedding) and model.loss_history_ == base.loss_history_


# ------------------------------------------------------------------ what a fit leaves
def test_save_and_load_round_trip(fitted, tmp_path):
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    model, _, _, _ = fitted[True]
    path = str(tmp_path / 'als.pt')
    model.save(path)
    back = MatrixFactorization.load(path)
    assert torch.equal(back.user_embedding.cpu(), model.user_embedding.cpu())
    assert torch.equal(back.item_embedding.cpu(), model.item_embedding.cpu())
    assert back.loss_history_ == model.loss_history_ and back.n_components == R


@pytest.mark.gpu
def test_rankings_run_on_an_als_model(fitted):
    """retrieve_user_recs and similar_items read user_embedding / item_embedding as after fit (they need the engine: a GPU test)."""
    from teamoflow_amd.mf.sparse import SparseInteractions
    model, _, idx, val = fitted[True]
    train = SparseInteractions(idx, val, (M, N))
    top = model.retrieve_user_recs(k=10, exclude=train)
    ids, sims = model.similar_items(k=5)
    assert top.shape == (M, 10) and ids.shape == (N, 5) and np.isfinite(sims).all()
    seen = np.zeros((M, N), bool)
    seen[idx[val != 0, 0], idx[val != 0, 1]] = True
    assert not seen[np.arange(M)[:, None], top].any()   # nothing seen is recommended
    assert (ids != np.arange(N)[:, None]).all()          # an item is not its own neighbour


def test_no_interactions_give_zero_rows(fitted):
    """A row without entries gets x = 0 - also when NO row has any: an empty fold-in and a fit on an empty table."""
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    model, _, _, _ = fitted[True]
    none = SparseInteractions(np.zeros((0, 2), np.int64), np.zeros(0, np.float32), (4, N))
    for implicit in (True, False):
        X = model.fold_in_users(none, reg=REG, alpha=ALPHA, implicit=implicit)
        assert tuple(X.shape) == (4, R) and X.dtype == torch.float32 and not X.any()
    empty, _, _ = make_model()
    empty.fit_als(2, eye(M), eye(N), SparseInteractions(np.zeros((0, 2), np.int64), np.zeros(0, np.float32), (M, N)), reg=REG)
    assert not empty.user_embedding.any() and not empty.item_embedding.any() and empty.loss_history_ == [0.0, 0.0]
    assert tuple(empty.user_embedding.shape) == (M, R) and tuple(empty.item_embedding.shape) == (N, R)


def test_cpu_half_step_takes_a_row_longer_than_a_chunk():
    """solve_rows_torch with a chunk budget far below one row's entries: the long row goes through a matrix product, no
    per-entry outer products, and agrees with the oracle like the others."""
    from teamoflow_amd import _als
    rng = np.random.default_rng(9)
    r, n = 6, 40
    Y = (rng.standard_normal((n, r)) / np.sqrt(r)).astype(np.float32)
    counts = np.array([3, 500, 0, 7])
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    col = rng.integers(0, n, counts.sum())
    w, t = rng.random(counts.sum()).astype(np.float32), rng.standard_normal(counts.sum()).astype(np.float32)
    G0 = (Y.T @ Y).astype(np.float32)
    X, failed = _als.solve_rows_torch(torch.tensor(Y), torch.tensor(rowptr), torch.tensor(col), torch.tensor(w), torch.tensor(t), 0.5,
                                      G0=torch.tensor(G0), max_floats=20 * r * r)
    assert failed == 0 and not X[2].any()
    assert rel_err(X.numpy(), solve_rows_ref(Y, G0, rowptr, col, w, t, 0.5)) <= 1e-5


# ------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_bound_and_built():
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    declared = set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    lib = _lib.load_library()
    for name, n_args in (('tmf_gram_workspace_bytes', 2), ('tmf_gram_f32', 9), ('tmf_als_solve_rows_f32', 17)):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert 'KNOWN LIMIT' in header
    make = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS :=.*\btmf_als\.hip\b', make, re.M)
    assert lib.tmf_gram_workspace_bytes(5000, 128) >= 128 * 128 * 4 and lib.tmf_gram_workspace_bytes(10, 129) == 0


def test_argument_checks_return_before_any_launch():
    """Null pointers throughout: a call that got as far as a launch would fail differently (or crash)."""
    from teamoflow_amd import _lib
    lib = _lib.load_library()

    def solve(r=8, ldy=8, ldx=8, reg=0.5, q=5, ldg=0):
        return lib.tmf_als_solve_rows_f32(None, 10, r, ldy, None, ldg, None, None, None, None, reg, None, q, None, ldx, None, None)
    for bad in (dict(r=0), dict(r=129, ldy=132, ldx=132), dict(reg=0.0), dict(reg=-1.0), dict(reg=float('nan')), dict(reg=float('inf')),
                dict(ldy=4), dict(ldy=10), dict(ldx=7), dict(q=-1)):
        assert solve(**bad) == -1, bad   # TMF_E_INVALID
    assert solve(q=0) == 0               # nothing to do: no launch
    assert solve() == -1 and b'required' in lib.tmf_last_error()   # in range, but no tables
    assert lib.tmf_gram_f32(None, 10, 0, 8, None, 8, None, 0, None) == -1
    assert lib.tmf_gram_f32(None, 10, 129, 132, None, 132, None, 0, None) == -1
    assert lib.tmf_gram_f32(None, 10, 8, 4, None, 8, None, 0, None) == -1
    assert lib.tmf_gram_f32(None, 10, 8, 8, None, 8, None, 0, None) == -1   # no G
