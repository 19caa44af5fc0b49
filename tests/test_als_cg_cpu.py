"""The conjugate-gradient form of alternating least squares where the suite runs without a GPU: the fp64 oracle's own properties
(als_cg_ref.py), fit_als / fold_in_users with solver='cg' against it (solve_rows_cg_torch without a GPU, the HIP kernel with one - the
same bounds), the warm start, every refusal, and the C ABI's argument checks, which return before any launch.

Bounds.  Loss histories agree with the fp64 oracle to the project bound 1e-5.  Tables are bounded by max(1e-5, 4 x the distance of the
oracle run in fp32 from the oracle in fp64 on the same case): a truncated iteration does not damp rounding differences the way an exact
solve does, and the factor covers a summation order other than NumPy's; the fp32 oracle's distance is computed here, from the oracle
alone."""
import numpy as np
import pytest
import torch

from als_cg_ref import als_cg_ref, cg_half_step_ref
from als_ref import half_step_ref
from conftest import rel_err
from test_als_cpu import ALPHA, EPOCHS, M, N, R, REG, CountingInitializer, make_data, make_model

CG_STEPS = 3


def fit_cg(implicit, seed=1, solver='cg', cg_steps=CG_STEPS, **kw):
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    idx, val = make_data()
    model, U0, V0 = make_model(seed=seed)
    model.fit_als(EPOCHS, eye(M), eye(N), SparseInteractions(idx, val, (M, N)), reg=REG, alpha=ALPHA, implicit=implicit, solver=solver,
                  cg_steps=cg_steps, **kw)
    return model, U0, V0, idx, val


@pytest.fixture(scope='module')
def fitted():
    """{implicit: (model, U0, V0, idx, val)}: one fit per mode, shared and left unchanged."""
    return {implicit: fit_cg(implicit) for implicit in (True, False)}


# ------------------------------------------------------------------ the oracle
@pytest.mark.parametrize('implicit', [True, False])
def test_oracle_with_as_many_steps_as_dimensions_is_the_exact_half_step(implicit):
    idx, val = make_data(seed=3)
    _, U0, V0 = make_model(seed=4)
    want = half_step_ref(V0, idx[:, 0], idx[:, 1], val, M, REG, ALPHA, implicit)
    rng = np.random.default_rng(8)
    for X0 in (None, U0, rng.standard_normal((M, R))):
        for steps in (R, R + 3):
            got = cg_half_step_ref(V0, X0, idx[:, 0], idx[:, 1], val, M, REG, ALPHA, implicit, steps)
            assert rel_err(got, want) <= 1e-10, (steps, rel_err(got, want))


@pytest.mark.parametrize('implicit', [True, False])
def test_oracle_objective_never_rises(implicit):
    idx, val = make_data(seed=3)
    _, U0, V0 = make_model(seed=4)
    L = als_cg_ref(U0, V0, idx, val, 15, REG, ALPHA, implicit, CG_STEPS)['loss']
    assert np.all(np.diff(L) <= 1e-12 * abs(L[0])), L


# ------------------------------------------------------------------ fit_als
@pytest.mark.parametrize('implicit', [True, False])
def test_fit_als_cg_matches_the_oracle(fitted, implicit):
    model, U0, V0, idx, val = fitted[implicit]
    ref = als_cg_ref(U0, V0, idx, val, EPOCHS, REG, ALPHA, implicit, CG_STEPS)
    ref32 = als_cg_ref(U0, V0, idx, val, EPOCHS, REG, ALPHA, implicit, CG_STEPS, dtype=np.float32)
    bound_u = max(1e-5, 4 * rel_err(ref32['U'][-1], ref['U'][-1]))
    bound_v = max(1e-5, 4 * rel_err(ref32['V'][-1], ref['V'][-1]))
    eu = rel_err(model.user_embedding.cpu().numpy(), ref['U'][-1])
    ev = rel_err(model.item_embedding.cpu().numpy(), ref['V'][-1])
    el = rel_err(model.loss_history_, ref['loss'])
    print(f'implicit={implicit}: U {eu:.3g} (bound {bound_u:.3g}), V {ev:.3g} (bound {bound_v:.3g}), loss {el:.3g}')
    assert len(model.loss_history_) == EPOCHS
    assert el <= 1e-5, el
    assert eu <= bound_u and ev <= bound_v, (eu, bound_u, ev, bound_v)
    assert model.user_embedding.dtype == torch.float32 and tuple(model.user_embedding.shape) == (M, R)
    assert model.user_trainable[0] is model.user_embedding and model.item_trainable[0] is model.item_embedding


@pytest.mark.parametrize('implicit', [True, False])
def test_the_warm_start_is_real(implicit):
    """Two fits that differ only in U0: different tables under 'cg' (the first user half-step starts from U0), identical ones under
    'cholesky' (it replaces U0)."""
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    idx, val = make_data()
    _, U0_a, V0 = make_model(seed=1)
    _, U0_b, _ = make_model(seed=2)   # make_model draws U0 and V0 from one generator: both fits take the first one's V0
    assert not np.array_equal(U0_a, U0_b)
    tables = {}
    for solver in ('cg', 'cholesky'):
        for name, U0 in (('a', U0_a), ('b', U0_b)):
            model = MatrixFactorization(R, user_weight_graph=FixedInitializer(U0), item_weight_graph=FixedInitializer(V0))
            model.verbose = False
            model.fit_als(2, eye(M), eye(N), SparseInteractions(idx, val, (M, N)), reg=REG, alpha=ALPHA, implicit=implicit, solver=solver,
                          cg_steps=CG_STEPS)
            tables[solver, name] = (model.user_embedding.clone(), model.item_embedding.clone())
    assert not torch.equal(tables['cg', 'a'][0], tables['cg', 'b'][0]) and not torch.equal(tables['cg', 'a'][1], tables['cg', 'b'][1])
    assert torch.equal(tables['cholesky', 'a'][0], tables['cholesky', 'b'][0])
    assert torch.equal(tables['cholesky', 'a'][1], tables['cholesky', 'b'][1])


# ------------------------------------------------------------------ fold-in
# fp32 conjugate gradients with exactly as many steps as dimensions have no spare step to make up for the conjugacy that rounding
# loses: on the fit's own data (values in [-2, 5], reg = 0.1) the ORACLE run in fp32 is 2.6e-5 (implicit) and 8.0e-5 (explicit) from
# the exact fold-in after R = 5 steps, and 5.6e-7 / 8.6e-7 after R + 1 (measured on the CPU, the oracle alone).  The fold-in case is
# therefore conditioned like the teacher-forced GPU half-steps - values scaled to [-0.2, 0.5] - with a ridge of 1.0, where the fp32
# oracle after R steps is 1.6e-7 / 1.3e-6; the test asserts that (<= 2.5e-6) before it judges fold_in_users at the project bound.
FOLD_REG, FOLD_SCALE = 1.0, 0.1


@pytest.mark.parametrize('implicit', [True, False])
def test_fold_in_with_as_many_steps_as_dimensions_is_the_exact_fold_in(fitted, implicit):
    from teamoflow_amd.mf.sparse import SparseInteractions
    model, _, _, idx, val = fitted[implicit]
    val = (val * FOLD_SCALE).astype(np.float32)
    U_before, V_before = model.user_embedding.clone(), model.item_embedding.clone()
    trainable, history = model.user_trainable, list(model.loss_history_)
    V, U = model.item_embedding.cpu().numpy(), model.user_embedding.cpu().numpy()
    kw = dict(reg=FOLD_REG, alpha=ALPHA, implicit=implicit)
    data = SparseInteractions(idx, val, (M, N))
    want = half_step_ref(V.astype(np.float64), idx[:, 0], idx[:, 1], val, M, FOLD_REG, ALPHA, implicit)
    err32 = rel_err(cg_half_step_ref(V, None, idx[:, 0], idx[:, 1], val, M, FOLD_REG, ALPHA, implicit, R, dtype=np.float32), want)
    assert err32 <= 2.5e-6, err32
    exact = model.fold_in_users(data, **kw)
    got = model.fold_in_users(data, solver='cg', cg_steps=R, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (M, R)
    e = rel_err(got.cpu().numpy(), exact.cpu().numpy().astype(np.float64))
    print(f'implicit={implicit}: fp32 oracle {err32:.3g} from the exact fold-in, fold_in_users(cg) {e:.3g} from the Cholesky fold-in')
    assert e <= 1e-5, e
    # the items' side with steps to spare (2 R): converged, whatever rounding did to the first R
    items = SparseInteractions(idx[:, ::-1].copy(), val, (N, M))
    want_v = half_step_ref(U.astype(np.float64), idx[:, 1], idx[:, 0], val, N, FOLD_REG, ALPHA, implicit)
    err32 = rel_err(cg_half_step_ref(U, None, idx[:, 1], idx[:, 0], val, N, FOLD_REG, ALPHA, implicit, 2 * R, dtype=np.float32), want_v)
    assert err32 <= 2.5e-6, err32
    got_v = model.fold_in_items(items, solver='cg', cg_steps=2 * R, **kw)
    assert tuple(got_v.shape) == (N, R) and rel_err(got_v.cpu().numpy(), want_v) <= 1e-5
    assert torch.equal(model.user_embedding, U_before) and torch.equal(model.item_embedding, V_before)
    assert model.user_trainable is trainable and model.loss_history_ == history


# ------------------------------------------------------------------ refusals
def refused(exc, setup=None, **kw):
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    idx, val = make_data()
    init = CountingInitializer()
    model = MatrixFactorization(kw.pop('n_components', R), user_weight_graph=init, item_weight_graph=init)
    sentinel = object()
    model.user_trainable = sentinel
    if setup:
        setup(model)
    with pytest.raises(exc):
        model.fit_als(2, eye(M), eye(N), SparseInteractions(idx, val, (M, N)), **kw)
    assert model.user_trainable is sentinel and init.calls == 0
    return model


@pytest.mark.parametrize('kw', [dict(solver='qr'), dict(cg_steps=0), dict(cg_steps=33), dict(cg_steps=2.5), dict(cg_steps=None),
                                dict(solver='cg', cg_steps=0), dict(solver='cg', cg_steps=33), dict(solver='cg', cg_steps=2.5),
                                dict(solver='cg', cg_steps=None)])
def test_bad_solver_and_steps_raise_value_error(kw):
    refused(ValueError, **kw)


def test_fold_in_checks_solver_and_steps(fitted):
    from teamoflow_amd.mf.sparse import SparseInteractions
    model = fitted[True][0]
    one = SparseInteractions(np.array([[0, 1]]), np.float32([1.0]), (1, N))
    for kw in (dict(solver='qr'), dict(cg_steps=0), dict(solver='cg', cg_steps=33), dict(cg_steps=2.5), dict(solver='cg', cg_steps=None)):
        with pytest.raises(ValueError):
            model.fold_in_users(one, **kw)


def test_widths_the_cg_form_takes_and_refuses():
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    refused(NotImplementedError, n_components=257, solver='cg')
    wide = MatrixFactorization(257)
    wide.item_embedding, wide.user_embedding = torch.zeros(N, 257), torch.zeros(M, 257)
    for call in (wide.fold_in_users, wide.fold_in_items):
        with pytest.raises(NotImplementedError):
            call(SparseInteractions(np.array([[0, 1]]), np.float32([1.0]), (1, N)), solver='cg')
    m, n = 20, 15
    idx, val = make_data(seed=6, m=m, n=n, density=0.3)
    model, _, _ = make_model(r=129, seed=7, m=m, n=n)
    model.fit_als(2, eye(m), eye(n), SparseInteractions(idx, val, (m, n)), reg=REG, alpha=ALPHA, solver='cg')
    assert tuple(model.user_embedding.shape) == (m, 129) and len(model.loss_history_) == 2
    assert bool(torch.isfinite(model.user_embedding).all()) and bool(model.item_embedding.any())
    assert model.loss_history_[1] <= model.loss_history_[0]


@pytest.mark.parametrize('name, value', [('factor_dtype', torch.bfloat16), ('batch_users', 16), ('shard_items', 2),
                                         ('data_parallel', 'force'), ('user_alpha', 0.1), ('item_alpha', 0.1)])
def test_unbuilt_settings_raise_before_any_weight_is_drawn_with_cg(name, value):
    refused(NotImplementedError, setup=lambda model: setattr(model, name, value), solver='cg')


# ------------------------------------------------------------------ the C ABI
@pytest.fixture(scope='module')
def lib():
    from teamoflow_amd import _lib
    return _lib.load_library()


def test_entry_points_are_declared_bound_and_built(lib):
    import os
    import re

    from conftest import ROOT
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    declared = set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    for name, n_args in (('tmf_gram_wide_workspace_bytes', 2), ('tmf_gram_wide_f32', 9), ('tmf_als_cg_rows_f32', 20)):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == n_args
    make = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS :=.*\btmf_als_cg\.hip\b', make, re.M)
    assert lib.tmf_gram_wide_workspace_bytes(5000, 256) >= 256 * 256 * 4 and lib.tmf_gram_wide_workspace_bytes(10, 257) == 0


def test_argument_checks_return_before_any_launch(lib):
    """Null pointers throughout: a call that got as far as a launch would fail differently (or crash)."""
    import ctypes

    def solve(r=8, ldy=8, ldx=8, reg=0.5, q=5, steps=3, y=None):
        return lib.tmf_als_cg_rows_f32(y, 10, r, ldy, None, 0, None, None, None, None, reg, None, q, None, 0, None, ldx, steps, None, None)
    for bad in (dict(r=0), dict(r=257, ldy=260, ldx=260), dict(steps=0), dict(steps=33), dict(reg=0.0), dict(reg=-1.0),
                dict(reg=float('nan')), dict(reg=float('inf')), dict(ldy=4), dict(ldy=10), dict(ldx=4), dict(ldx=10), dict(q=-1)):
        assert solve(**bad) == -1, bad   # TMF_E_INVALID
    assert solve(q=0) == 0               # nothing to do: no launch
    assert solve(r=256, ldy=256, ldx=256, q=0) == 0
    assert solve() == -1 and b'required' in lib.tmf_last_error()   # in range, but no tables
    # every pointer present but Y misaligned: refused for the alignment (nothing is dereferenced on the host)
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = ctypes.c_void_p(base)
    rc = lib.tmf_als_cg_rows_f32(ctypes.c_void_p(base + 4), 10, 8, 8, None, 0, p, p, p, p, 0.5, None, 5, None, 0, p, 8, 3, p, None)
    assert rc == -1 and b'aligned' in lib.tmf_last_error()
    assert lib.tmf_gram_wide_f32(None, 10, 0, 8, None, 8, None, 0, None) == -1
    assert lib.tmf_gram_wide_f32(None, 10, 257, 260, None, 260, None, 0, None) == -1
    assert lib.tmf_gram_wide_f32(None, 10, 8, 4, None, 8, None, 0, None) == -1
    assert lib.tmf_gram_wide_f32(None, 10, 8, 8, None, 8, None, 0, None) == -1   # no G
    assert lib.tmf_gram_f32(None, 10, 129, 132, None, 132, None, 0, None) == -1   # the narrow entry keeps its range
