"""sampling_correction='logq' on the sparse HIP engine: tmf_softmax_pairs_offset and tmf_slot_offsets alone, then
SampledSoftmaxLoss fits on tables drawn by popularity through the public API, against the NumPy fp64 closed form of
tests/test_logq_cpu.py - which that file pins to the plug-in's own get_loss on sp - l[R] and whose fp32 restatement it shows to meet
the tolerances used here on the same inputs: rel_err < 1e-5 for delta, D and the loss, the sum identity at 1e-5, and
assert_step(rtol=1e-5) for the tables after one step (tests/test_gpu_softmax.py's tolerances)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_step, rel_err, step_bounds
from test_bpr_cpu import LR, bpr_problem, kernel_case
from test_logq_cpu import LOGQ_MAGNITUDES, OFFSET_LOWS, exact_difference, log_expected_count_ref, logq_closed_form, logq_pairs_ref, \
    offset_case
from test_softmax_cpu import KERNEL_S, sum_identity_gaps

pytestmark = pytest.mark.gpu
NAN = float('nan')
M_USERS, N_ITEMS, POWER = 60, 400, 0.75
GEOMETRIES = [(1, 5), (7, 64), (33, 70), (128, 64), (256, 5)]        # (r, S)


@pytest.fixture(scope='module')
def tm():
    from teamoflow_amd import _engine, _lib, _ops
    from teamoflow_amd.mf import utils
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import SampledSoftmaxLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    lib = _lib.get()

    class NS:
        pass
    ns = NS()
    ns.lib, ns.L, ns.E, ns.ops, ns.utils, ns.MF, ns.Fixed, ns.SM, ns.Sparse, ns.eye = lib, _lib, _engine, _ops, utils, \
        MatrixFactorization, FixedInitializer, SampledSoftmaxLoss, SparseInteractions, eye
    return ns


@pytest.fixture
def engine_only(tm, monkeypatch):
    """_fit_generic refuses to run: a fit that passes ran on the engine."""
    def refuse(self, *a, **k):
        raise AssertionError('_fit_generic was called')
    monkeypatch.setattr(tm.MF, '_fit_generic', refuse)


# ------------------------------------------------------------------------------------------------------------------------
# the kernels alone
# ------------------------------------------------------------------------------------------------------------------------
def run_kernel(tm, rowptr, val, p, sp, off=None, order=None, c=1.0):
    """tmf_softmax_pairs_offset (off given) or tmf_softmax_pairs on host arrays, every output pre-filled with NaN ->
    (delta, D, loss_part) as NumPy.  A table without entries passes NULL for val, p and delta."""
    dev, P = torch.device('cuda'), tm.L.ptr
    m, S = sp.shape
    d_rowptr = torch.as_tensor(np.asarray(rowptr, np.int64), device=dev)
    d_val, d_p, d_sp = (torch.as_tensor(np.asarray(x, np.float32), device=dev).contiguous() for x in (val, p, sp))
    delta = torch.full((d_val.numel(),), NAN, device=dev)
    D = torch.full((m, S), NAN, device=dev)
    loss = torch.full((m,), NAN, device=dev)
    d_order = None if order is None else torch.as_tensor(np.asarray(order, np.int32), device=dev)
    entries = [P(x) if x.numel() else None for x in (d_val, d_p, delta)]
    sizes = (ctypes.c_int32(m), ctypes.c_int32(S), float(c))
    tail = (entries[2], P(D), P(loss), P(d_order), tm.L.stream_ptr())
    if off is None:
        rc = tm.lib.tmf_softmax_pairs(P(d_rowptr), entries[0], entries[1], P(d_sp), *sizes, *tail)
    else:
        d_off = torch.as_tensor(np.asarray(off, np.float32), device=dev).contiguous()
        assert d_off.shape == d_sp.shape
        rc = tm.lib.tmf_softmax_pairs_offset(P(d_rowptr), entries[0], entries[1], P(d_sp), P(d_off), *sizes, *tail)
    tm.L.check(rc, tm.lib)
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


def case_and_reference(S, low, scale=None):
    """offset_case(S, low) and its fp64 outputs on the exact difference, computed once and left unchanged."""
    key = (S, low, scale)
    if key not in _CASE_REFS:
        case = offset_case(S, low, scale=scale)
        ref = logq_pairs_ref(case[0], case[1], case[2], exact_difference(case[3], case[4]))
        for a in ref:
            a.setflags(write=False)
        _CASE_REFS[key] = case, ref
    return _CASE_REFS[key]


@pytest.mark.parametrize('low', OFFSET_LOWS)
@pytest.mark.parametrize('S', KERNEL_S)
def test_kernel_against_fp64(tm, S, low):
    """tests/test_gpu_softmax.py's 67 users and row lengths, with offsets uniform in [low, 0]."""
    case, ref = case_and_reference(S, low)
    rowptr, val = case[0], case[1]
    got = run_kernel(tm, *case)
    assert all(np.isfinite(g).all() for g in got)                     # no NaN left anywhere: every element was written
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    delta, D, loss = got
    worst = assert_sum_identity(rowptr, val, delta, D)
    print(f'[kernel] S={S} off in [{low:g}, 0]: delta {errs[0]:.3g} D {errs[1]:.3g} loss {errs[2]:.3g} identity {worst:.3g}')
    assert max(errs) < 1e-5, errs
    assert not delta[val <= 0].any() and (delta[val > 0] < 0).all()
    no_pos = np.array([not (val[rowptr[u]:rowptr[u + 1]] > 0).any() for u in range(67)])
    assert no_pos.sum() >= 12 and not D[no_pos].any() and not loss[no_pos].any() and (D[~no_pos] > 0).all()
    assert_bits(run_kernel(tm, *case), got)                                                          # a second call
    assert_bits(run_kernel(tm, *case, order=np.random.default_rng(S).permutation(67)), got)          # two permuted user orders
    assert_bits(run_kernel(tm, *case, order=np.arange(67)[::-1].copy()), got)


@pytest.mark.parametrize('S', KERNEL_S)
def test_offsets_of_zero_give_the_bits_of_the_plain_kernel(tm, S):
    case = kernel_case(S)
    for zero in (0.0, -0.0):
        assert_bits(run_kernel(tm, *case, off=np.full(case[3].shape, zero, np.float32)), run_kernel(tm, *case))
    # and the correction is not a no-op: other offsets, other outputs
    assert not np.array_equal(run_kernel(tm, *case, off=np.full(case[3].shape, -1.0, np.float32))[2], run_kernel(tm, *case)[2])


def test_kernel_at_the_magnitudes(tm):
    """Scores of magnitude 0, 1e-3 and 30 with both signs (tests/test_logq_cpu.py says why not 88 and 1e4), overall and user by user."""
    case, ref = case_and_reference(65, -12.0, LOGQ_MAGNITUDES)
    got = run_kernel(tm, *case)
    assert all(np.isfinite(g).all() for g in got)
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    print(f'[kernel] magnitudes: delta {errs[0]:.3g} D {errs[1]:.3g} loss {errs[2]:.3g}')
    assert max(errs) < 1e-5, errs
    assert_sum_identity(case[0], case[1], got[0], got[1])
    rowptr, val = case[0], case[1]
    for u in range(67):
        if (val[rowptr[u]:rowptr[u + 1]] > 0).any():
            assert rel_err(got[2][u], ref[2][u]) < 1e-5, (u, LOGQ_MAGNITUDES[u % len(LOGQ_MAGNITUDES)])


def test_non_finite_offsets_stay_inside_their_user(tm):
    """A NaN offset in one user and an infinite one in another: every other user's outputs keep their bits."""
    rowptr, val, p, sp, off = (x[:12] if x.ndim == 2 else x for x in offset_case(65, -12.0))
    rowptr = rowptr[:13]
    val, p = val[:rowptr[-1]], p[:rowptr[-1]]
    a, b = 5, 8                                                # 33 and 131 positives
    assert rowptr[a + 1] - rowptr[a] == 33 and rowptr[b + 1] - rowptr[b] == 131
    clean = run_kernel(tm, rowptr, val, p, sp, off)
    off2 = off.copy()
    off2[a, 20], off2[b, 64] = np.nan, -np.inf
    delta, D, loss = run_kernel(tm, rowptr, val, p, sp, off2)
    others = ~np.isin(np.arange(12), (a, b))
    ent = np.ones(val.shape[0], bool)
    ent[rowptr[a]:rowptr[a + 1]] = ent[rowptr[b]:rowptr[b + 1]] = False
    assert_bits((delta[ent], D[others], loss[others]), (clean[0][ent], clean[1][others], clean[2][others]))
    assert np.isfinite(delta[ent]).all() and np.isfinite(D[others]).all() and np.isfinite(loss[others]).all()
    assert not np.isfinite(loss[a]) and not np.isfinite(loss[b])        # nothing was silently dropped either
    off3 = off.copy()
    off3[a, 20] = np.inf                                       # an item that is never proposed: its slot takes no part
    got = run_kernel(tm, rowptr, val, p, sp, off3)
    assert all(np.isfinite(g).all() for g in got) and not got[1][a, 20] and (np.delete(got[1][a], 20) > 0).all()


def test_kernel_on_tables_without_users_or_entries(tm):
    empty = np.zeros(0, np.float32)
    got = run_kernel(tm, np.zeros(1, np.int64), empty, empty, np.zeros((0, 65), np.float32), np.zeros((0, 65), np.float32))
    assert [g.shape for g in got] == [(0,), (0, 65), (0,)]                                           # n_users = 0
    case = kernel_case(65, n_users=1)                                                                # one user, nothing stored
    assert case[0].tolist() == [0, 0]
    delta, D, loss = run_kernel(tm, *case, off=np.full((1, 65), NAN, np.float32))                    # its offsets are not read
    assert delta.shape == (0,) and not D.any() and not loss.any()
    rowptr, val, p, sp = kernel_case(65, n_users=3)                                                  # users with 0, 1 and 2 entries
    off = np.random.default_rng(3).uniform(-12.0, 0.0, sp.shape).astype(np.float32)
    got, ref = run_kernel(tm, rowptr, val, p, sp, off), logq_pairs_ref(rowptr, val, p, exact_difference(sp, off))
    assert max(rel_err(g, r) for g, r in zip(got, ref)) < 1e-5 and not got[1][0].any() and not got[2][0]


@pytest.mark.parametrize('shift', [0, 1], ids=['aligned', 'one element in'])
@pytest.mark.parametrize('shape', [(0, 7), (1, 1), (1, 3), (2, 2), (65, 7), (67, 1025)], ids=lambda s: 'x'.join(map(str, s)))
def test_slot_offsets(tm, shape, shift):
    """off[j] = ell[R[j]] at totals of 0, 1, 3, 4, 65 x 7 and 67 x 1025 - below one 16-byte piece, exactly one, whole pieces with
    and without a tail - on fresh allocations (16-byte aligned) and on views that start one element into their storage."""
    dev, n = torch.device('cuda'), N_ITEMS
    m, S = shape
    total = m * S
    rng = np.random.default_rng(total + shift)
    ell = torch.as_tensor(rng.uniform(-25.0, 0.0, n).astype(np.float32), device=dev)
    ids = rng.integers(0, n, total)
    if total >= 2:
        ids[0], ids[-1] = n - 1, 0                                      # both ends of the table are gathered
    R_store = torch.zeros(total + shift + 4, dtype=torch.int32, device=dev)
    off_store = torch.full((total + shift + 4,), NAN, device=dev)
    R, off = R_store[shift:shift + total], off_store[shift:shift + total]
    R.copy_(torch.as_tensor(ids, dtype=torch.int32))
    if total:
        assert (R.data_ptr() % 16 == 0) == (shift == 0) and (off.data_ptr() % 16 == 0) == (shift == 0)
    tm.L.check(tm.lib.tmf_slot_offsets(ell, n, R, m, S, off, tm.L.stream_ptr()), tm.lib)
    torch.cuda.synchronize()
    assert torch.equal(off, ell[R.long()])
    assert torch.isnan(off_store[:shift]).all() and torch.isnan(off_store[shift + total:]).all()     # nothing outside the table


# ------------------------------------------------------------------------------------------------------------------------
# one step through the public API
# ------------------------------------------------------------------------------------------------------------------------
def fit_logq(tm, p, epochs, U0=None, V0=None, loss=None, correction='logq', sampling='popularity', **attrs):
    U0, V0 = (p['U0'] if U0 is None else U0), (p['V0'] if V0 is None else V0)
    model = tm.MF(p['r'], loss_graph=loss or tm.SM(), user_weight_graph=tm.Fixed(U0), item_weight_graph=tm.Fixed(V0), n_users=p['m'],
                  n_items=p['n'], n_samples=p['S'])
    model.verbose, model.random_ind = False, torch.as_tensor(p['R'])
    model.negative_sampling, model.sampling_power, model.sampling_correction = sampling, POWER, correction
    for k, v in attrs.items():
        setattr(model, k, v)
    return refit(tm, model, p, epochs)


def refit(tm, model, p, epochs):
    model.fit(epochs, tm.eye(p['m']), tm.eye(p['n']), tm.Sparse(p['idx'], p['val'], (p['m'], p['n'])), lr=LR)
    return model


def host(t):
    return t.detach().float().cpu().numpy()


def same_fit(a, b):
    return a.loss_history_ == b.loss_history_ and torch.equal(a.user_embedding, b.user_embedding) \
        and torch.equal(a.item_embedding, b.item_embedding)


def weights_of(tm, p):
    return tm.utils.popularity_weights(torch.as_tensor(np.bincount(p['idx'][p['val'] > 0, 1], minlength=p['n'])), POWER)


_REFS = {}


def problem_and_reference(tm, seed, r, S, sample_seed=0, tables=None):
    """(problem, q, the table of round 0, l as the fit subtracts it, loss mean, gU, gV, gb): the fp64 closed form of a shape on the table
    the sampler draws for it, computed once and left unchanged.  tables: (U0, V0) other than the problem's."""
    key = (seed, r, S, sample_seed, tables is not None)
    if key not in _REFS:
        p = bpr_problem(seed, M_USERS, N_ITEMS, r, S)
        q = weights_of(tm, p)
        R = tm.ops.sample_negatives(N_ITEMS, M_USERS, S, seed=sample_seed, device='cuda', weights=q).cpu().numpy()
        ell = log_expected_count_ref(q.numpy(), S).astype(np.float32)           # what the fit subtracts: fp32 values
        U0, V0 = (p['U0'], p['V0']) if tables is None else tables
        loss, delta, D, gU, gV = logq_closed_form(U0, V0, p['idx'], p['val'], R, ell.astype(np.float64))
        # of a scalar item bias at zero: the sum of D over the slots that hold the item and of delta over its positives
        gb = np.bincount(R.reshape(-1), weights=D.reshape(-1), minlength=N_ITEMS) \
            + np.bincount(p['idx'][:, 1], weights=delta, minlength=N_ITEMS)
        for a in (R, ell, gU, gV, gb):
            a.setflags(write=False)
        _REFS[key] = (p, q, R, ell, loss / int((p['val'] > 0).sum()), gU, gV, gb)
    return _REFS[key]


def test_the_counts_pass_the_admission_rule_at_every_sample_count(tm):
    """4 H <= 3 T with H the sum of the S heaviest weights (utils.weighted_cum), for the problems of every geometry below."""
    for seed, r, S in [(r, r, S) for r, S in GEOMETRIES] + [(133, 33, 64), (9, 33, 20), (64, 64, 5)]:
        q = weights_of(tm, bpr_problem(seed, M_USERS, N_ITEMS, r, S)).numpy()
        assert (q >= 1).all() and 4 * int(np.sort(q)[-S:].sum()) <= 3 * int(q.sum()) and np.ptp(q) > 0
        tm.utils.weighted_cum(torch.as_tensor(q), N_ITEMS, S)                     # and the package agrees


def check_one_step(tm, seed, r, S, what='', tables=None, check_tables=True, **attrs):
    p, q, R, ell, loss, gU, gV, gb = problem_and_reference(tm, seed, r, S, tables=tables)
    kw = {} if tables is None else dict(U0=tables[0], V0=tables[1])
    model = fit_logq(tm, p, 1, **kw, **attrs)
    st = model._state
    assert st.wplan.sliced and st.plan.n_pos == int((p['val'] > 0).sum()), 'the fit did not take the sliced user pass'
    assert np.array_equal(st.wplan.R_model.cpu().numpy(), R), 'not the table of round 0'
    got = model.sample_log_q_
    assert got.dtype == torch.float32 and got.shape == (N_ITEMS,) and torch.equal(got.cpu(), tm.utils.log_expected_count(q, S))
    assert np.array_equal(got.cpu().numpy(), ell) and (ell < 0).all() and np.ptp(ell) > 0.5
    assert st.wplan.off is not None and torch.equal(st.wplan.off, got.to('cuda')[st.wplan.R.long()])
    assert [name for name, _ in st.wplan.prepared] == ['slot_offsets']
    err = rel_err(model.loss_history_[0], loss)
    print(f'[one step] {what}: loss {err:.3g}')
    assert err < 1e-5, what                                                    # the mean over the positives
    if check_tables:
        U0, V0 = (p['U0'], p['V0']) if tables is None else tables
        assert_step(host(model.user_embedding), U0, gU, LR, rtol=1e-5, what=f'{what} U')
        assert_step(host(model.item_embedding), V0, gV, LR, rtol=1e-5, what=f'{what} V')
        for row in (p['empty_user'], p['nonpos_user']):
            assert np.array_equal(host(model.user_embedding)[row], U0[row])    # a zero gradient: the row keeps its bits
    return model


@pytest.mark.parametrize('r,S', GEOMETRIES)
def test_every_row_geometry_one_step(tm, engine_only, r, S):
    check_one_step(tm, r, r, S, f'r={r} S={S}')


@pytest.mark.parametrize('env', [{'TMF_ITEM_SLICES': '3'}, {'TMF_ROW_STATIONARY': '1'}, {'TMF_SCORES6': '1'}, {'TMF_ROWS4': '1'}],
                         ids=lambda e: '='.join(*e.items()))
def test_the_forms_of_the_user_and_item_pass_one_step(tm, engine_only, monkeypatch, env):
    """Everything around the pair step in its other forms (tests/test_gpu_softmax.py): the offsets follow the plan's slot order in
    each of them."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = 128
    st = check_one_step(tm, 128, r, 64, str(env))._state
    if 'TMF_ITEM_SLICES' in env:
        assert st.wplan.n_slices == 3
    if 'TMF_ROW_STATIONARY' in env:
        assert st.row_stationary == bool(tm.lib.tmf_wmrb_gradu4_supported(r, 0))
    if 'TMF_SCORES6' in env:
        assert (st.wplan.s6 is not None) == bool(tm.lib.tmf_wmrb_scores6_supported(r, 0, N_ITEMS))
    if 'TMF_ROWS4' in env:
        assert st.wplan.rows4 == bool(tm.lib.tmf_wsum_rows4_rows_per_group(r, 0))


def test_scalar_item_bias_one_step(tm, engine_only):
    """The bias starts at zero and its add pass runs first, in place: the logit is sp + b - l, the tables step as without it, and the
    bias steps by the sum of D over the slots of an item plus delta over its positives."""
    gb = problem_and_reference(tm, 128, 128, 64)[-1]
    model = check_one_step(tm, 128, 128, 64, 'scalar_item_bias', scalar_item_bias=True)
    assert model._state.ib is not None
    assert_step(host(model.item_bias_), np.zeros(N_ITEMS), gb, LR, rtol=1e-5, what='item bias')


def _bf16(x):
    return torch.tensor(np.asarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def test_bf16_storage_one_step(tm, engine_only):
    """bf16 factor storage / fp32 arithmetic: against the closed form on the bf16-rounded tables; the new rows must lie in the step
    interval rounded to bf16 (tests/test_gpu_softmax.py::test_bf16_storage_one_step, its tolerances)."""
    p = bpr_problem(133, M_USERS, N_ITEMS, 33, 64)
    U0, V0 = _bf16(p['U0']), _bf16(p['V0'])
    _, _, _, _, _, gU, gV, _ = problem_and_reference(tm, 133, 33, 64, tables=(U0, V0))
    model = check_one_step(tm, 133, 33, 64, 'bf16', tables=(U0, V0), check_tables=False, factor_dtype=torch.bfloat16)
    assert model.user_embedding.dtype == torch.bfloat16
    for got, W0, g in zip((host(model.user_embedding), host(model.item_embedding)), (U0, V0), (gU, gV)):
        lo, hi = step_bounds(W0, g, LR)
        got = got.astype(np.float64)
        assert (got >= _bf16(lo) - 1e-12).all() and (got <= _bf16(hi) + 1e-12).all()


def test_opt_in_persistent_adam_one_step(tm, engine_only):
    """optimizer='adam': the first step is the closed form's and the default's bit for bit."""
    a = check_one_step(tm, 7, 7, 64, "optimizer='adam'", optimizer='adam')
    assert same_fit(a, check_one_step(tm, 7, 7, 64, 'fresh_adam'))


# ------------------------------------------------------------------------------------------------------------------------
# resampling, replay, the uniform sampler, no leakage, the spans
# ------------------------------------------------------------------------------------------------------------------------
def test_resample_every_is_three_one_epoch_fits(tm, engine_only):
    """resample_every=1 over three epochs = three one-epoch fits on the tables of rounds 0, 1 and 2, each from the tables the one
    before left: bit for bit (tests/test_gpu_resample.py's construction).  Offsets left from an earlier round would show here."""
    p, seed = bpr_problem(4, 200, 150, 16, 32), 21
    whole = fit_logq(tm, p, 3, resample_every=1, sample_seed=seed)
    assert whole.resample_rounds_ == 3 and torch.equal(torch.as_tensor(whole.random_ind), torch.as_tensor(p['R']))
    w = whole._state.wplan
    q = weights_of(tm, p)
    assert torch.equal(w.R_model, tm.ops.sample_negatives(150, 200, 32, seed=seed + 2, device='cuda', weights=q))
    assert torch.equal(w.off, whole.sample_log_q_.to('cuda')[w.R.long()]) and [name for name, _ in w.prepared] == ['slot_offsets']
    chain = fit_logq(tm, p, 1, sample_seed=seed)
    history = list(chain.loss_history_)
    for j in (1, 2):
        U, V = host(chain.user_embedding).copy(), host(chain.item_embedding).copy()
        chain.user_weight_graph, chain.item_weight_graph, chain.sample_seed = tm.Fixed(U), tm.Fixed(V), seed + j
        refit(tm, chain, p, 1)
        assert chain.resample_rounds_ == 1
        history += chain.loss_history_
    assert whole.loss_history_ == history
    assert torch.equal(whole.user_embedding, chain.user_embedding) and torch.equal(whole.item_embedding, chain.item_embedding)
    static = fit_logq(tm, p, 3, sample_seed=seed)
    assert static.loss_history_[0] == whole.loss_history_[0] and static.loss_history_[1:] != whole.loss_history_[1:]


def test_graph_replay_gives_the_launched_bits(tm, engine_only, monkeypatch):
    """Ten epochs as one replay of a ten-epoch hipGraph (the offsets are built before the capture), then launched one by one."""
    p = bpr_problem(6, 200, 150, 16, 32)
    monkeypatch.delenv('TMF_NO_GRAPH', raising=False)
    a = fit_logq(tm, p, 10)
    monkeypatch.setenv('TMF_NO_GRAPH', '1')
    b = fit_logq(tm, p, 10)
    assert a.graph_epochs_ == 10 and b.graph_epochs_ == 0 and len(a.loss_history_) == 10
    assert same_fit(a, b) and a.loss_history_[-1] < a.loss_history_[0]
    assert not same_fit(a, fit_logq(tm, p, 10, correction='none'))


def test_under_uniform_tables_the_fit_is_catalog_scale(tm, engine_only):
    """l is the constant log(S / n_items): catalog_scale's c and the plain kernel, bit for bit, and no table of offsets."""
    p = bpr_problem(64, M_USERS, N_ITEMS, 64, 5)
    logq = fit_logq(tm, p, 3, sampling='uniform')
    scaled = fit_logq(tm, p, 3, sampling='uniform', correction='none', loss=tm.SM(catalog_scale=True))
    assert same_fit(logq, scaled) and logq.sample_log_q_ is None
    assert logq._state.wplan.off is None and logq._state.wplan.prepared == []
    assert not same_fit(logq, fit_logq(tm, p, 3, sampling='uniform', correction='none'))
    fresh = [fit_logq(tm, p, 3, sampling='uniform', resample_every=1, sample_seed=3, **kw)
             for kw in (dict(), dict(correction='none', loss=tm.SM(True)))]
    assert same_fit(*fresh) and not same_fit(fresh[0], logq)


def test_a_later_fit_without_the_setting_equals_a_fresh_one(tm, engine_only):
    p = bpr_problem(9, M_USERS, N_ITEMS, 33, 20)
    alone = fit_logq(tm, p, 3, correction='none')
    model = fit_logq(tm, p, 3)
    assert not same_fit(model, alone) and model.sample_log_q_ is not None
    model.sampling_correction = 'none'
    refit(tm, model, p, 3)
    assert same_fit(model, alone) and model.sample_log_q_ is None and model._state.wplan.off is None
    del model.sampling_correction                                              # and a model that never had the attribute
    assert same_fit(refit(tm, model, p, 3), alone)


@pytest.mark.parametrize('biased', [False, True], ids=['plain', 'scalar_item_bias'])
def test_the_spans_of_an_epoch(tm, engine_only, biased):
    """One launch of the pair step under its usual name; an item_bias_add pass only where the model has a bias."""
    p = bpr_problem(9, M_USERS, N_ITEMS, 33, 20)
    st = fit_logq(tm, p, 1, scalar_item_bias=biased)._state
    prof, out = tm.E.KernelTimer(), torch.zeros(1, dtype=torch.float64, device='cuda')
    tm.E.epoch_sides(st, tm.E.adam_constants(LR), out, 'softmax', 1.0, prof)
    torch.cuda.synchronize()
    assert len(prof.spans['softmax_pairs']) == 1 and ('item_bias_add' in prof.spans) == biased
    assert not any('offset' in name for name in prof.spans) and float(out) > 0
