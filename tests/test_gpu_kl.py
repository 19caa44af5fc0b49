"""KLDivergenceLoss on the sparse HIP engine (tmf_kl_moments / tmf_kl_coeffs / tmf_kl_pass, _engine.epoch_kl) against
oracle.dense_ref.fit_dense_plugins(..., 'kl', dtype=float64) - the reference loop on the dense [m, n] scores, fine at these sizes.
Every problem is test_kl_cpu.kl_problem's unless a test builds the row lengths it is about: first loss ~ 0.5, both classes
populated, stored zeros among the values."""
import numpy as np
import pytest
import torch

from conftest import assert_step, rel_err, step_bounds
from test_kl_cpu import kl_closed_form, kl_moments, kl_oracle, kl_problem

pytestmark = pytest.mark.gpu
LR = 0.05


@pytest.fixture(scope='module')
def tm():
    from teamoflow_amd import _engine, _lib
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import KLDivergenceLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    lib = _lib.get()

    class NS:
        pass
    ns = NS()
    ns.lib, ns.L, ns.E, ns.MF, ns.Fixed, ns.KL, ns.Sparse, ns.eye = lib, _lib, _engine, MatrixFactorization, FixedInitializer, \
        KLDivergenceLoss, SparseInteractions, eye
    return ns


def fit_kl(tm, U0, V0, idx, val, epochs, lr=LR, **attrs):
    m, n = U0.shape[0], V0.shape[0]
    model = tm.MF(U0.shape[1], loss_graph=tm.KL(), user_weight_graph=tm.Fixed(U0), item_weight_graph=tm.Fixed(V0))
    model.verbose = False
    for k, v in attrs.items():
        setattr(model, k, v)
    model.fit(epochs, tm.eye(m), tm.eye(n), tm.Sparse(idx, val, (m, n)), lr=lr)
    return model


def tables(model):
    return model.user_embedding.float().cpu().numpy(), model.item_embedding.float().cpu().numpy()


def check_one_step(tm, U0, V0, idx, val, what=''):
    model = fit_kl(tm, U0, V0, idx, val, 1)
    ref = kl_oracle(U0, V0, idx, val, 1, LR)
    assert rel_err(model.loss_history_[0], ref['loss'][0]) < 1e-5, what
    U1, V1 = tables(model)
    assert_step(U1, U0, ref['first_grads'][0][0], LR, what=f'{what} U')
    assert_step(V1, V0, ref['first_grads'][1][0], LR, what=f'{what} V')
    return model


@pytest.mark.parametrize('r', [1, 3, 7, 16, 33, 64, 100, 128, 200, 256, 300, 512])
def test_every_row_geometry_one_step(tm, r):
    idx, val, U0, V0 = kl_problem(r, r=r)
    check_one_step(tm, U0, V0, idx, val, f'r={r}')


def test_raw_moments_and_gradient_through_the_c_abi(tm):
    """The three kernels called directly: the per-segment moments reduced on the host against NumPy fp64 on the same tables, and
    the raw gradient (TMF_EPI_GRAD on both sides) against the oracle's."""
    L, lib, r = tm.L, tm.lib, 24
    idx, val, U0, V0 = kl_problem(24, r=r)
    m, n = U0.shape[0], V0.shape[0]
    dev = torch.device('cuda')
    plan = tm.E.InteractionPlan(torch.as_tensor(idx, device=dev), torch.as_tensor(val, device=dev), m, n)
    st = tm.E.TrainState(U0, V0, plan, r, kl=True)
    s, P = L.stream_ptr(), L.ptr
    L.check(lib.tmf_kl_moments_f32(plan.seg_u.cstruct(), P(plan.col_u), P(plan.val_u), P(st.U), P(st.V), P(st.kl_part), r, s), lib)
    t = st.kl_part.cpu().numpy().sum(0)
    got = (t[0], t[1], t[2] / t[0], t[3] / t[1], t[4] / t[0] - (t[2] / t[0]) ** 2, t[5] / t[1] - (t[3] / t[1]) ** 2)
    p = np.einsum('kr,kr->k', U0.astype(np.float64)[idx[:, 0]], V0.astype(np.float64)[idx[:, 1]])
    want = kl_moments(p, val)
    assert got[0] == want[0] and got[1] == want[1]
    for a, b, name in zip(got[2:], want[2:], ('mu+', 'mu-', 'v+', 'v-')):
        assert abs(a - b) <= 1e-5 * abs(b), (name, a, b)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    L.check(lib.tmf_kl_coeffs(P(st.kl_part), plan.seg_u.nseg, P(loss), P(st.kl_coef), s), lib)
    gU, gV = torch.zeros_like(st.U), torch.zeros_like(st.V)
    adam = tm.E.adam_constants(LR)
    L.check(lib.tmf_kl_pass_f32(plan.seg_u.cstruct(), P(plan.col_u), P(plan.val_u), P(st.U), P(st.V), P(gU), P(st.slab), P(st.kl_coef),
                                r, L.EPI_GRAD, adam, s), lib)
    L.check(lib.tmf_kl_pass_f32(plan.seg_i.cstruct(), P(plan.row_i), P(plan.val_i), P(st.V), P(st.U), P(gV), P(st.slab), P(st.kl_coef),
                                r, L.EPI_GRAD, adam, s), lib)
    ref = kl_oracle(U0, V0, idx, val, 1, LR)
    assert rel_err(float(loss), ref['loss'][0]) < 1e-5
    assert rel_err(gU[:, :r].cpu().numpy(), ref['first_grads'][0][0]) < 1e-5
    assert rel_err(gV[:, :r].cpu().numpy(), ref['first_grads'][1][0]) < 1e-5


def test_rows_cut_into_segments(tm):
    """User 0 stores all 5000 items (5 segments of 1024), user 1 exactly 1024 (one full segment), user 2 1025 (two): the partial
    rows of users 0 and 2 go through the slab and tmf_combine_rows, and so do the moments of their segments."""
    rng = np.random.default_rng(5)
    m, n, r = 6, 5000, 32
    rows = [np.arange(n), rng.choice(n, 1024, replace=False), rng.choice(n, 1025, replace=False), rng.choice(n, 40, replace=False),
            rng.choice(n, 3, replace=False), np.arange(0)]
    idx = np.concatenate([np.stack([np.full(c.size, u), np.sort(c)], 1) for u, c in enumerate(rows)])
    val = rng.integers(-5, 6, idx.shape[0]).astype(np.float32)
    U0 = (rng.standard_normal((m, r)) * 0.3).astype(np.float32)
    V0 = (rng.standard_normal((n, r)) * 0.3).astype(np.float32)
    model = check_one_step(tm, U0, V0, idx, val, 'segmented')
    assert model._state.plan.seg_u.n_long == 2 and model._state.plan.seg_u.nseg == 5 + 1 + 2 + 3


def test_more_segments_than_one_round_of_the_reduction(tm):
    """4500 users of 1-3 entries: the coefficient kernel's 1024 threads each take several strided shares of the 4500 x 6
    moments (two full rounds of 6 x 1024 pairs and a ragged third), and the passes run thousands of workgroups."""
    rng = np.random.default_rng(11)
    m, n, r = 4500, 7, 3
    deg = rng.integers(1, 4, m)
    idx = np.concatenate([np.stack([np.full(d, u), np.sort(rng.choice(n, d, replace=False))], 1) for u, d in enumerate(deg)])
    val = rng.integers(-5, 6, idx.shape[0]).astype(np.float32)
    U0 = (rng.standard_normal((m, r)) * 0.3).astype(np.float32)
    V0 = (rng.standard_normal((n, r)) * 0.3).astype(np.float32)
    model = check_one_step(tm, U0, V0, idx, val, 'many segments')
    assert model._state.plan.seg_u.nseg == m and model._state.plan.seg_i.n_long == n


def test_user_blocked_item_lists(tm, monkeypatch):
    monkeypatch.setenv('TMF_USER_CHUNKS', '4')
    idx, val, U0, V0 = kl_problem(32, r=32)
    model = check_one_step(tm, U0, V0, idx, val, 'TMF_USER_CHUNKS=4')
    assert model._state.plan.seg_i.row_mod == V0.shape[0] and model._state.plan.user_chunks == 4


def test_untouched_rows_and_input_order(tm):
    idx, val, U0, V0 = kl_problem(4, r=12)
    keep = (idx[:, 0] != 7) & (idx[:, 1] != 11)           # user 7 and item 11 store nothing
    idx, val = idx[keep], val[keep]
    model = check_one_step(tm, U0, V0, idx, val, 'empty rows')
    U1, V1 = tables(model)
    assert np.array_equal(U1[7], U0[7]) and np.array_equal(V1[11], V0[11])
    # a shuffled list with duplicate pairs: every stored entry counts on its own, as in the oracle's gather of the same list
    rng = np.random.default_rng(9)
    dup = rng.choice(idx.shape[0], 60, replace=False)
    idx2 = np.concatenate([idx, idx[dup]])
    val2 = np.concatenate([val, rng.integers(-5, 6, 60).astype(np.float32)])
    order = rng.permutation(idx2.shape[0])
    check_one_step(tm, U0, V0, idx2[order], val2[order], 'shuffled with duplicates')


def test_trajectory(tm):
    idx, val, U0, V0 = kl_problem(6, m=70, n=45, r=5)
    model = fit_kl(tm, U0, V0, idx, val, 12)
    ref = kl_oracle(U0, V0, idx, val, 12, LR)['loss']
    h = model.loss_history_
    assert rel_err(h[:3], ref[:3]) < 1e-5 and rel_err(h, ref) < 1e-3   # near-sign Adam steps amplify rounding over the epochs


def test_graph_replay_equals_eager(tm, monkeypatch):
    idx, val, U0, V0 = kl_problem(7, r=12)
    for epochs in (10, 13):                               # 10 = one replay; 13 = one replay of 12 and an eager epoch
        monkeypatch.delenv('TMF_NO_GRAPH', raising=False)
        a, b = fit_kl(tm, U0, V0, idx, val, epochs), fit_kl(tm, U0, V0, idx, val, epochs)
        monkeypatch.setenv('TMF_NO_GRAPH', '1')
        c = fit_kl(tm, U0, V0, idx, val, epochs)
        for other in (b, c):
            assert a.loss_history_ == other.loss_history_ and len(a.loss_history_) == epochs
            assert torch.equal(a.user_embedding, other.user_embedding) and torch.equal(a.item_embedding, other.item_embedding)
        assert np.isfinite(a.loss_history_).all()


def _bf16(x):
    return torch.tensor(np.asarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


@pytest.mark.parametrize('r', [5, 100, 300])
def test_bf16_storage_one_step(tm, r):
    """bf16 factor storage / fp32 arithmetic: against the oracle on the bf16-rounded tables; the new rows must lie in the step
    interval rounded to bf16 (tests/test_gpu_parity.py::test_bf16_storage_one_step)."""
    idx, val, U0, V0 = kl_problem(100 + r, r=r)
    U0, V0 = _bf16(U0), _bf16(V0)
    model = fit_kl(tm, U0, V0, idx, val, 1, factor_dtype=torch.bfloat16)
    assert model.user_embedding.dtype == torch.bfloat16
    ref = kl_oracle(U0, V0, idx, val, 1, LR)
    assert abs(model.loss_history_[0] - ref['loss'][0]) <= 1e-5 * abs(ref['loss'][0])
    for got, W0, g in zip(tables(model), (U0, V0), (ref['first_grads'][0][0], ref['first_grads'][1][0])):
        lo, hi = step_bounds(W0, g, LR)
        got = got.astype(np.float64)
        assert (got >= _bf16(lo) - 1e-12).all() and (got <= _bf16(hi) + 1e-12).all(), r


def test_opt_in_persistent_adam(tm):
    """optimizer='adam': the first step is the default's bit for bit; later steps follow Keras Adam with carried moments,
    evaluated in NumPy from the closed form (test_kl_cpu pins it to the oracle)."""
    idx, val, U0, V0 = kl_problem(8, r=12)
    a1, f1 = fit_kl(tm, U0, V0, idx, val, 1, optimizer='adam'), fit_kl(tm, U0, V0, idx, val, 1)
    assert torch.equal(a1.user_embedding, f1.user_embedding) and torch.equal(a1.item_embedding, f1.item_embedding)
    assert a1.loss_history_ == f1.loss_history_
    got = fit_kl(tm, U0, V0, idx, val, 4, optimizer='adam')
    U, V = U0.astype(np.float64), V0.astype(np.float64)
    mU, vU, mV, vV = (np.zeros_like(x) for x in (U, U, V, V))
    ref = []
    for t in range(1, 5):
        loss, gU, gV, _ = kl_closed_form(U, V, idx, val)
        ref.append(loss)
        alpha = LR * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        mU += (gU - mU) * 0.1
        vU += (gU ** 2 - vU) * 0.001
        mV += (gV - mV) * 0.1
        vV += (gV ** 2 - vV) * 0.001
        U = U - alpha * mU / (np.sqrt(vU) + 1e-7)
        V = V - alpha * mV / (np.sqrt(vV) + 1e-7)
    assert rel_err(got.loss_history_, ref) < 1e-4


def test_dispatch(tm, monkeypatch):
    """KL over indicator features trains on the engine (on the parent commit this fit went through _fit_generic); everything the
    engine has no KL form for keeps the generic path."""
    idx, val, U0, V0 = kl_problem(9, r=6)
    m, n = U0.shape[0], V0.shape[0]

    def refuse(self, *a, **k):
        raise AssertionError('_fit_generic was called')
    monkeypatch.setattr(tm.MF, '_fit_generic', refuse)
    model = fit_kl(tm, U0, V0, idx, val, 2)
    assert model.user_embedding.is_cuda and len(model.loss_history_) == 2 and hasattr(model, '_state')

    calls = []
    monkeypatch.setattr(tm.MF, '_fit_generic', lambda self, *a, **k: calls.append(type(self.loss_graph).__name__))

    class MyKL(tm.KL):
        pass

    def model_with(loss=None, **attrs):
        mf = tm.MF(6, loss_graph=loss or tm.KL(), user_weight_graph=tm.Fixed(U0), item_weight_graph=tm.Fixed(V0))
        mf.verbose = False
        for k, v in attrs.items():
            setattr(mf, k, v)
        return mf
    inter = tm.Sparse(idx, val, (m, n))
    rng = np.random.default_rng(0)
    Fu = torch.tensor((np.eye(m) + 0.05 * rng.random((m, m))).astype(np.float32), device='cuda')
    model_with().fit(1, Fu, tm.eye(n), inter, lr=LR)                                   # dense non-identity features
    model_with(MyKL()).fit(1, tm.eye(m), tm.eye(n), inter, lr=LR)                      # a subclass of the loss
    model_with(batch_users=8).fit(1, tm.eye(m), tm.eye(n), inter, lr=LR)
    model_with().fit(1, tm.eye(m), tm.eye(n), tm.Sparse(idx, np.abs(val) + 1.0, (m, n)), lr=LR)   # only positive values
    assert calls == ['KLDivergenceLoss', 'MyKL', 'KLDivergenceLoss', 'KLDivergenceLoss']
