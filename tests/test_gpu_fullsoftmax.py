"""FullSoftmaxLoss on the sparse HIP engine (csrc/tmf_fullsoftmax.hip, _engine.epoch_full_softmax) against the NumPy fp64 closed form
of tests/test_fullsoftmax_cpu.py, which that file pins to the plug-in's own get_loss and whose fp32 restatement it shows to meet the
tolerances used here on the same inputs: rel_err < 1e-5 for lse, the swept sums, the loss and the raw gradients,
assert_step(rtol=1e-5) for the tables after one step.  Kernel outputs are pre-filled with NaN and followed by a poisoned guard zone
that must keep its bits; the padding columns of every table are NaN."""
import numpy as np
import pytest
import torch

from conftest import assert_step, rel_err
from test_bpr_cpu import LR, bpr_problem
from test_fullsoftmax_cpu import KERNEL_SHAPES, fresh_adam_fp64, fullsoftmax_closed_form, times_six

pytestmark = pytest.mark.gpu
NAN = float('nan')
GUARD, GUARD_BITS = 192, 0x7fc0beef   # floats behind every kernel output, and what they hold (a NaN with a payload)


@pytest.fixture(scope='module')
def tm():
    from teamoflow_amd import _engine, _lib
    from teamoflow_amd.mf import embedding_graphs as EG
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import FullSoftmaxLoss, WMRBLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseFeatures, SparseInteractions, eye, hstack_identity
    lib = _lib.get()

    class NS:
        pass
    ns = NS()
    ns.lib, ns.L, ns.E, ns.EG, ns.MF, ns.Fixed, ns.FS, ns.WMRB, ns.Sparse, ns.SF, ns.eye, ns.hstack = lib, _lib, _engine, EG, \
        MatrixFactorization, FixedInitializer, FullSoftmaxLoss, WMRBLoss, SparseInteractions, SparseFeatures, eye, hstack_identity
    return ns


@pytest.fixture
def engine_only(tm, monkeypatch):
    """_fit_generic refuses to run: a fit that passes ran on the engine."""
    def refuse(self, *a, **k):
        raise AssertionError('_fit_generic was called')
    monkeypatch.setattr(tm.MF, '_fit_generic', refuse)


def host(t):
    return t.detach().float().cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------
# the kernels alone
# ------------------------------------------------------------------------------------------------------------------------
def device_table(tm, W, pad=NAN):
    """[rows, ld(r)] fp32 on the device, the padding columns poisoned: they are never used, whatever they hold."""
    rows, r = W.shape
    T = torch.full((rows, tm.L.padded_ld(r)), pad, dtype=torch.float32, device='cuda')
    T[:, :r] = torch.as_tensor(np.asarray(W, np.float32))
    return T


def guarded(n_floats, fill=NAN):
    """A flat fp32 buffer of n_floats (filled) + the guard zone."""
    buf = torch.full((n_floats + GUARD,), fill, dtype=torch.float32, device='cuda')
    buf.view(torch.int32)[n_floats:] = GUARD_BITS
    return buf


def guard_intact(buf, n_floats):
    return bool((buf.view(torch.int32)[n_floats:] == GUARD_BITS).all())


def run_lse(tm, A, B):
    m, r = A.shape
    dA, dB = device_table(tm, A), device_table(tm, B)
    out = guarded(m)
    tm.L.check(tm.lib.tmf_fsm_lse_f32(tm.L.ptr(dA), tm.L.ptr(dB), m, B.shape[0], r, dA.shape[1], dB.shape[1], tm.L.ptr(out),
                                      tm.L.stream_ptr()), tm.lib)
    torch.cuda.synchronize()
    assert guard_intact(out, m), 'lse wrote past its m rows'
    return out[:m].cpu().numpy()


def lse_fp64(A, B):
    s = np.asarray(A, np.float64) @ np.asarray(B, np.float64).T
    mx = s.max(axis=1, keepdims=True)
    return mx[:, 0] + np.log(np.exp(s - mx).sum(axis=1))


def tables(seed, m, n, r, scale=0.3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((m, r)) * scale).astype(np.float32), (rng.standard_normal((n, r)) * scale).astype(np.float32)


@pytest.mark.parametrize('shape', KERNEL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_lse_against_fp64(tm, shape):
    """One row and one item; partial row and item tiles; K no multiple of 4 or of 32; rows at their padded ld; more than one
    workgroup and eight item tiles.  A second call gives the same bits."""
    m, n, r = shape
    A, B = tables(sum(shape), m, n, r, scale=1.0 if r < 8 else 0.3)
    got, ref = run_lse(tm, A, B), lse_fp64(A, B)
    assert np.isfinite(got).all()                                             # every row was written
    err = rel_err(got, ref)
    print(f'[lse] {shape}: {err:.3g}')
    assert err < 1e-5
    assert np.array_equal(bits(run_lse(tm, A, B)), bits(got))


def test_lse_above_the_overflow_of_exp(tm):
    """Both tables scaled by 6: the largest |score| is 94.6, exp of which is not an fp32 number - a running maximum keeps lse finite."""
    p = times_six()
    got, ref = run_lse(tm, p['U0'], p['V0']), lse_fp64(p['U0'], p['V0'])
    assert np.isfinite(got).all() and ref.max() > 88.73
    print(f'[lse] x6: {rel_err(got, ref):.3g}, largest lse {ref.max():.4g}')
    assert rel_err(got, ref) < 1e-5


def test_lse_a_nan_row_stays_inside_its_user(tm):
    A, B = tables(3, 300, 257, 33)
    clean = run_lse(tm, A, B)
    A2 = A.copy()
    A2[137, 20] = np.nan
    got = run_lse(tm, A2, B)
    others = np.arange(300) != 137
    assert np.array_equal(bits(got[others]), bits(clean[others])) and np.isnan(got[137])


def run_wsum(tm, A, B, lse, w, user_is_a, G0):
    """tmf_fsm_wsum_f32 on top of G0 [ma, r] (padded to ld with NaN columns, followed by the guard zone) -> G [ma, r]."""
    ma, r = A.shape
    dA, dB = device_table(tm, A), device_table(tm, B)
    ld = dA.shape[1]
    buf = guarded(ma * ld)
    G = buf[:ma * ld].view(ma, ld)
    G[:, :r] = torch.as_tensor(np.asarray(G0, np.float32))
    d_lse, d_w = (torch.as_tensor(np.asarray(x, np.float32), device='cuda') for x in (lse, w))
    tm.L.check(tm.lib.tmf_fsm_wsum_f32(tm.L.ptr(dA), tm.L.ptr(dB), ma, B.shape[0], r, ld, dB.shape[1], tm.L.ptr(d_lse), tm.L.ptr(d_w),
                                       int(user_is_a), tm.L.ptr(G), ld, tm.L.stream_ptr()), tm.lib)
    torch.cuda.synchronize()
    assert guard_intact(buf, ma * ld), 'wsum wrote past G'
    assert bool(torch.isnan(G[:, r:]).all()), 'wsum wrote padding columns of G'
    return G[:, :r].cpu().numpy()


def wsum_fp64(A, B, lse, w, user_is_a, G0):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    s = A @ B.T
    lse, w = np.asarray(lse, np.float64), np.asarray(w, np.float64)
    P = w[:, None] * np.exp(s - lse[:, None]) if user_is_a else w[None, :] * np.exp(s - lse[None, :])
    return np.asarray(G0, np.float64) + P @ B


_WSUM_CASES = {}


def wsum_case(shape, user_is_a):
    """Users x items = shape[:2]; the stationary table is the users' (user_is_a) or the items'.  lse is the users' true log-partition
    rounded to fp32, w their number of positives (0 .. 5, a fifth of them 0), G0 random.  The fp64 result is computed once."""
    key = (shape, user_is_a)
    if key not in _WSUM_CASES:
        m, n, r = shape
        U, V = tables(sum(shape) + 1, m, n, r, scale=1.0 if r < 8 else 0.3)
        rng = np.random.default_rng(sum(shape))
        lse = lse_fp64(U, V).astype(np.float32)
        w = rng.integers(0, 6, m).astype(np.float32) * (rng.random(m) > 0.2)
        w[0], w[m - 1] = 0.0, 3.0                                             # one user alone: w = 3
        A, B = (U, V) if user_is_a else (V, U)
        G0 = (rng.standard_normal(A.shape) * 0.01).astype(np.float32)
        ref = wsum_fp64(A, B, lse, w, user_is_a, G0)
        ref.setflags(write=False)
        _WSUM_CASES[key] = (A, B, lse, w, G0, ref)
    return _WSUM_CASES[key]


@pytest.mark.parametrize('user_is_a', [1, 0], ids=['users-stationary', 'items-stationary'])
@pytest.mark.parametrize('shape', KERNEL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_wsum_against_fp64(tm, shape, user_is_a):
    A, B, lse, w, G0, ref = wsum_case(shape, user_is_a)
    got = run_wsum(tm, A, B, lse, w, user_is_a, G0)
    assert np.isfinite(got).all()
    err = rel_err(got, ref)
    print(f'[wsum] {shape} user_is_a={user_is_a}: {err:.3g}; |sum| up to {np.abs(ref - G0).max():.3g} on |G0| up to {np.abs(G0).max():.3g}')
    assert err < 1e-5                                                         # the sums, added onto what G held
    if user_is_a:                                                             # stationary users with w = 0: not written at all
        assert np.array_equal(bits(got[w == 0]), bits(G0[w == 0])) and ((w == 0).any() or shape[0] == 1)
        assert not (bits(got[w != 0]) == bits(G0[w != 0])).all(axis=1).any()
    else:                                                                     # swept users with w = 0: as if they were not there
        keep = w != 0
        if keep.any():
            ref2 = wsum_fp64(A, B[keep], lse[keep], w[keep], 0, G0)
            assert rel_err(got, ref2) < 1e-5
        bad_lse = np.where(keep, lse, np.float32(NAN))                        # whatever their lse holds
        assert np.array_equal(bits(run_wsum(tm, A, B, bad_lse, w, 0, G0)), bits(got))
    assert np.array_equal(bits(run_wsum(tm, A, B, lse, w, user_is_a, G0)), bits(got))      # a second call


def test_wsum_above_the_overflow_of_exp(tm):
    """Both tables scaled by 6 (scores up to 94.6), lse as tmf_fsm_lse_f32 gives it - what an epoch feeds the sweep - against fp64
    with the exact lse.  An fp32 score of that size is only good to its ulp, 7.6e-6, and exp(s - lse) carries that absolute error as a
    relative one: it is the normalisation by an lse formed from the SAME fp32 scores (both kernels add a score's products in one
    order) that takes it out again, as it does in torch's fp32 (tests/test_fullsoftmax_cpu.py: 2.5e-6 on this input)."""
    p = times_six()
    U, V = p['U0'], p['V0']
    lse, exact = run_lse(tm, U, V), lse_fp64(U, V)
    w = np.bincount(p['idx'][p['val'] > 0, 0], minlength=U.shape[0]).astype(np.float32)
    for user_is_a, (A, B) in ((1, (U, V)), (0, (V, U))):
        G0 = np.zeros(A.shape, np.float32)
        got, ref = run_wsum(tm, A, B, lse, w, user_is_a, G0), wsum_fp64(A, B, exact, w, user_is_a, G0)
        print(f'[wsum] x6 user_is_a={user_is_a}: {rel_err(got, ref):.3g}')
        assert np.isfinite(got).all() and rel_err(got, ref) < 1e-5


@pytest.mark.parametrize('r', [128, 33])
def test_swept_table_past_32_bit_byte_offsets(tm, r):
    """The swept table at a leading dimension of 2^20 floats: 1030 rows span 4.3 GB, so byte offsets into it no longer fit 32 bits and
    the kernels leave the buffer loads for 64-bit addresses (r = 128: the branch-free loads of lse; r = 33: the guarded ones).  Only
    the rows' first r floats are ever written or read; the allocation is not initialised."""
    m, n, ldb = 130, 1030, 1 << 20
    assert n * ldb * 4 > 2 ** 32
    A, B = tables(r, m, n, r)
    dA = device_table(tm, A)
    big = torch.empty(n * ldb, dtype=torch.float32, device='cuda').view(n, ldb)
    big[:, :r] = torch.as_tensor(B)
    big[:, r:tm.L.padded_ld(r)] = NAN
    out = guarded(m)
    tm.L.check(tm.lib.tmf_fsm_lse_f32(tm.L.ptr(dA), tm.L.ptr(big), m, n, r, dA.shape[1], ldb, tm.L.ptr(out), tm.L.stream_ptr()), tm.lib)
    torch.cuda.synchronize()
    ref = lse_fp64(A, B)
    assert guard_intact(out, m) and rel_err(out[:m].cpu().numpy(), ref) < 1e-5
    w = np.random.default_rng(r).integers(0, 6, m).astype(np.float32)
    ld = dA.shape[1]
    buf = guarded(m * ld, 0.0)
    G = buf[:m * ld].view(m, ld)
    d_w = torch.as_tensor(w, device='cuda')
    tm.L.check(tm.lib.tmf_fsm_wsum_f32(tm.L.ptr(dA), tm.L.ptr(big), m, n, r, ld, ldb, tm.L.ptr(out), tm.L.ptr(d_w), 1, tm.L.ptr(G), ld,
                                       tm.L.stream_ptr()), tm.lib)
    torch.cuda.synchronize()
    assert guard_intact(buf, m * ld) and not G[:, r:].any()
    assert rel_err(G[:, :r].cpu().numpy(), wsum_fp64(A, B, ref, w, 1, np.zeros((m, r)))) < 1e-5
    del big


def raw_gradients(tm, p):
    """One epoch under TMF_EPI_GRAD on both sides -> (loss sum, G_U, G_V) of the state's kernels, the tables untouched."""
    dev = torch.device('cuda')
    idx, val = torch.as_tensor(p['idx'], device=dev), torch.as_tensor(p['val'], device=dev)
    plan = tm.E.InteractionPlan(idx, val, p['m'], p['n'], csc=True)
    st = tm.E.TrainState(p['U0'], p['V0'], plan, p['r'], full_softmax=True)
    gU, gV = torch.full_like(st.U, NAN), torch.full_like(st.V, NAN)
    out = torch.zeros(1, dtype=torch.float64, device=dev)
    U_before = st.U.clone()
    tm.E.run_epoch(st, tm.E.adam_constants(LR), out, 'full_softmax', 0.0, tm.L.EPI_GRAD, gV, None, tm.L.EPI_GRAD, gU)
    torch.cuda.synchronize()
    assert torch.equal(st.U, U_before)
    r = p['r']
    assert not gU[:, r:].any() and not gV[:, r:].any()                       # the padding columns of a gradient table are zeros
    return float(out), host(gU[:, :r]), host(gV[:, :r]), st


def test_the_partition_identity(tm):
    """One column of V set to 1.0: G_U[u, col] = n_u sum_i pi_ui - n_u = 0, to 1e-5 n_u for every user - columns >= n leaking into the
    ragged last tile (257 = 2 x 128 + 1 items) would show here."""
    p = dict(bpr_problem(33, 300, 257, 33, 8))
    p['V0'] = p['V0'].copy()
    col = 17
    p['V0'][:, col] = 1.0
    _, gU, _, st = raw_gradients(tm, p)
    n_u = host(st.fsm_w)
    assert np.array_equal(n_u, np.bincount(p['idx'][p['val'] > 0, 0], minlength=300)) and n_u.max() > 50
    gap = np.abs(gU[:, col])
    print(f'[identity] worst |G_U[u, col]| / n_u = {(gap[n_u > 0] / n_u[n_u > 0]).max():.3g}')
    assert (gap <= 1e-5 * n_u).all()


def test_raw_gradients_against_fp64(tm):
    """Both gradient tables as the sides, L2 and persistent Adam receive them (TMF_EPI_GRAD), and the loss sum."""
    p = bpr_problem(33, 300, 257, 33, 8)
    loss, gU, gV = fullsoftmax_closed_form(p['U0'], p['V0'], p['idx'], p['val'])
    got_loss, aU, aV, _ = raw_gradients(tm, p)
    errs = rel_err(got_loss, loss), rel_err(aU, gU), rel_err(aV, gV)
    print(f'[raw gradients] loss {errs[0]:.3g} gU {errs[1]:.3g} gV {errs[2]:.3g}')
    assert max(errs) < 1e-5
    assert not aU[p['empty_user']].any() and not aU[p['nonpos_user']].any() and aV[p['empty_item']].any()


def test_rows_cut_into_segments(tm):
    """2500 users, 40 items, every user stores item 3 (a list of 2500 entries: three segments of the item pass) and a few others."""
    rng = np.random.default_rng(11)
    m, n, r = 2500, 40, 8
    mask = rng.random((m, n)) < 0.05
    mask[:, 3] = True
    idx = np.argwhere(mask)
    val = rng.choice(np.array([-1, 0, 1, 2], np.float32), idx.shape[0], p=[.1, .1, .4, .4])
    U0, V0 = tables(12, m, n, r)
    p = dict(idx=idx, val=val, U0=U0, V0=V0, m=m, n=n, r=r)
    loss, gU, gV = fullsoftmax_closed_form(U0, V0, idx, val)
    got_loss, aU, aV, st = raw_gradients(tm, p)
    assert st.plan.seg_i.n_long >= 1
    assert max(rel_err(got_loss, loss), rel_err(aU, gU), rel_err(aV, gV)) < 1e-5


# ------------------------------------------------------------------------------------------------------------------------
# one step through the public API
# ------------------------------------------------------------------------------------------------------------------------
def fit_full(tm, p, epochs, U0=None, V0=None, loss=None, lr=LR, item_features=None, r=None, **attrs):
    U0, V0 = (p['U0'] if U0 is None else U0), (p['V0'] if V0 is None else V0)
    graphs = {k: attrs.pop(k) for k in ('user_repr_graph', 'item_repr_graph') if k in attrs}
    model = tm.MF(r or p['r'], loss_graph=loss or tm.FS(), user_weight_graph=tm.Fixed(U0), item_weight_graph=tm.Fixed(V0), n_users=p['m'],
                  n_items=p['n'], n_samples=p['S'], **graphs)
    model.verbose = False
    for k, v in attrs.items():
        setattr(model, k, v)
    model.fit(epochs, tm.eye(p['m']), tm.eye(p['n']) if item_features is None else item_features,
              tm.Sparse(p['idx'], p['val'], (p['m'], p['n'])), lr=lr)
    return model


_REFS = {}


def problem_and_reference(seed, m, n, r):
    """(problem, loss mean, gU, gV): the fp64 closed form of a shape, computed once and left unchanged."""
    key = (seed, m, n, r)
    if key not in _REFS:
        p = bpr_problem(seed, m, n, r, 8)
        loss, gU, gV = fullsoftmax_closed_form(p['U0'], p['V0'], p['idx'], p['val'])
        for a in (gU, gV):
            a.setflags(write=False)
        _REFS[key] = (p, loss / int((p['val'] > 0).sum()), gU, gV)
    return _REFS[key]


@pytest.mark.parametrize('m,n,r', [(60, 40, 1), (60, 40, 7), (60, 40, 33), (60, 40, 64), (60, 40, 128), (300, 257, 33)])
def test_every_row_geometry_one_step(tm, engine_only, m, n, r):
    p, loss, gU, gV = problem_and_reference(r, m, n, r)
    model = fit_full(tm, p, 1)
    st = model._state
    assert st.wplan is None and model.random_ind is None and model.resample_rounds_ == 0 and st.plan.n_pos == int((p['val'] > 0).sum())
    err = rel_err(model.loss_history_[0], loss)
    print(f'[one step] {m}x{n} r={r}: loss {err:.3g}')
    assert err < 1e-5                                                         # the mean over the positives
    assert_step(host(model.user_embedding), p['U0'], gU, LR, rtol=1e-5, what=f'r={r} U')
    assert_step(host(model.item_embedding), p['V0'], gV, LR, rtol=1e-5, what=f'r={r} V')
    for row in (p['empty_user'], p['nonpos_user']):                           # n_u = 0: the row keeps its bits
        assert np.array_equal(host(model.user_embedding)[row], p['U0'][row])
    assert not np.array_equal(host(model.item_embedding)[p['empty_item']], p['V0'][p['empty_item']])   # dense: every item row moves


def test_opt_in_persistent_adam(tm, engine_only):
    """optimizer='adam': the first step is the default's bit for bit; later steps follow Keras Adam with carried moments, evaluated
    in NumPy on the closed-form gradients (tests/test_gpu_softmax.py's statement and tolerance), over three epochs."""
    p = bpr_problem(8, 60, 40, 12, 20)
    a1, f1 = fit_full(tm, p, 1, optimizer='adam'), fit_full(tm, p, 1)
    assert torch.equal(a1.user_embedding, f1.user_embedding) and torch.equal(a1.item_embedding, f1.item_embedding)
    assert a1.loss_history_ == f1.loss_history_
    got = fit_full(tm, p, 3, optimizer='adam')
    U, V = p['U0'].astype(np.float64), p['V0'].astype(np.float64)
    mU, vU, mV, vV = (np.zeros_like(x) for x in (U, U, V, V))
    ref, n_pos = [], int((p['val'] > 0).sum())
    for t in range(1, 4):
        loss, gU, gV = fullsoftmax_closed_form(U, V, p['idx'], p['val'])
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


@pytest.mark.parametrize('alphas', [(2.0, 0.0), (0.3, 0.7)], ids=str)
def test_l2_one_step(tm, engine_only, alphas):
    """user_alpha / item_alpha: the closed-form data gradient + 2 alpha W0 (tests/test_gpu_l2.py's statement and tolerance); the
    unpenalised side is the unregularised fit's bit for bit, and loss_history_ stays the data term."""
    from test_gpu_l2 import assert_l2_step
    p, loss, gU, gV = problem_and_reference(33, 60, 40, 33)
    plain = fit_full(tm, p, 1)
    model = fit_full(tm, p, 1, user_alpha=alphas[0], item_alpha=alphas[1])
    assert model._state.l2 == [np.float32(2 * a) for a in alphas] and model.loss_history_ == plain.loss_history_
    for side, got, ref, W0, g, alpha in (('U', model.user_embedding, plain.user_embedding, p['U0'], gU, alphas[0]),
                                         ('V', model.item_embedding, plain.item_embedding, p['V0'], gV, alphas[1])):
        if alpha == 0:
            assert torch.equal(got, ref), f'{alphas} {side}: the unpenalised side differs from an unregularised fit'
        else:
            assert_l2_step(host(got), W0, g, alpha, f'l2 full softmax {alphas} {side}')
            assert not torch.equal(got, ref)


def test_biased_user_side_one_step(tm, engine_only):
    """A bias starts at zero, so the effective tables are the weights and their gradients the closed form's; the user bias moves
    by the column sums of G_U."""
    p, loss, gU, gV = problem_and_reference(1033, 60, 40, 33)
    model = fit_full(tm, p, 1, user_repr_graph=tm.EG.BiasedLinearEmbedding())
    st = model._state
    assert st.bias_u is not None and st.bias_v is None and st.wplan is None
    assert rel_err(model.loss_history_[0], loss) < 1e-5
    assert_step(host(model.item_embedding), p['V0'], gV, LR, rtol=1e-5, what='biased user side: V')
    assert len(model.user_trainable) == 2 and model.user_trainable[1] is model.user_linear_bias
    assert_step(host(model.user_trainable[0]), p['U0'], gU, LR, rtol=1e-5, what='biased user side: user weights')
    slack = 1e-5 * np.abs(gU).sum(axis=0, keepdims=True)
    from test_gpu_features import assert_step_with_slack
    assert_step_with_slack(host(model.user_linear_bias), np.zeros((1, 33)), gU.sum(axis=0, keepdims=True), slack, LR, 'the user bias')
    assert torch.equal(model.user_embedding, model.user_trainable[0] + model.user_linear_bias.detach())


def test_item_side_over_sparse_features_one_step(tm, engine_only):
    """F = [I | tags] (hstack_identity): E = F W, dL/dW = F^T dL/dE with dL/dE the closed form on (U, E); every row's gradient
    agrees to 1e-5, so feature f's sum may be off by 1e-5 sum_i |x_if| |dL/dE[i]| (tests/test_gpu_features.py)."""
    from test_gpu_features import assert_step_with_slack
    m, n, r, T = 60, 40, 33, 6
    p = bpr_problem(2033, m, n, r, 8)
    rng = np.random.default_rng(5)
    tag_idx = np.argwhere(rng.random((n, T)) < 0.3)
    tag_val = rng.choice(np.array([1.0, 0.5, -0.25, 2.0], np.float32), tag_idx.shape[0])
    F = tm.hstack(n, tm.SF(tag_idx, tag_val, (n, T)))
    F_dense = np.zeros((n, n + T))
    F_dense[np.arange(n), np.arange(n)] = 1.0
    F_dense[tag_idx[:, 0], n + tag_idx[:, 1]] = tag_val
    W0 = (rng.standard_normal((n + T, r)) * 0.3).astype(np.float32)
    model = fit_full(tm, p, 1, V0=W0, item_features=F)
    E0 = F_dense @ W0.astype(np.float64)
    loss, gU, gE = fullsoftmax_closed_form(p['U0'], E0, p['idx'], p['val'])
    st = model._state
    assert st.feat_v is not None and st.feat_u is None and st.wplan is None
    assert rel_err(model.loss_history_[0], loss / int((p['val'] > 0).sum())) < 1e-5
    assert_step(host(model.user_embedding), p['U0'], gU, LR, rtol=1e-5, what='user table')
    slack = 1e-5 * np.abs(F_dense).T @ np.abs(gE)
    assert_step_with_slack(host(model.item_trainable[0]), W0, F_dense.T @ gE, slack, LR, 'full softmax item weights over sparse features')
    assert model.item_embedding.shape == (n, r) and torch.equal(model.item_embedding, model.embed_items(F))


# ------------------------------------------------------------------------------------------------------------------------
# trajectory, replay, no leakage, refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_trajectory_and_graph_replay(tm, engine_only, monkeypatch):
    """200 x 150, r = 16: ten epochs - one replay of a ten-epoch hipGraph - against ten closed-form steps in fp64, epoch by epoch, every
    loss within 1e-5 and below the one before.  TMF_NO_GRAPH=1 gives the same bits and the same history."""
    p = bpr_problem(6, 200, 150, 16, 32)
    n_pos = int((p['val'] > 0).sum())
    U, V, ref = p['U0'].astype(np.float64), p['V0'].astype(np.float64), []
    for _ in range(10):
        loss, gU, gV = fullsoftmax_closed_form(U, V, p['idx'], p['val'])
        ref.append(loss / n_pos)
        U, V = fresh_adam_fp64(U, gU, LR), fresh_adam_fp64(V, gV, LR)
    monkeypatch.delenv('TMF_NO_GRAPH', raising=False)
    from teamoflow_amd.mf import matrix_factorization as M
    assert 200 * 150 + p['idx'].shape[0] <= M.GRAPH_MAX_WORK                  # small enough for the captured form
    a = fit_full(tm, p, 10)
    monkeypatch.setenv('TMF_NO_GRAPH', '1')
    b = fit_full(tm, p, 10)
    assert a.loss_history_ == b.loss_history_ and len(a.loss_history_) == 10
    assert torch.equal(a.user_embedding, b.user_embedding) and torch.equal(a.item_embedding, b.item_embedding)
    errs = [abs(h - r) / r for h, r in zip(a.loss_history_, ref)]
    print(f'[trajectory] per epoch: {" ".join(f"{e:.2g}" for e in errs)}')
    assert max(errs) < 1e-5 and all(y < x for x, y in zip(a.loss_history_, a.loss_history_[1:]))
    odd = fit_full(tm, p, 3)                                                  # an odd number of epochs: the same two buffers all the same
    assert odd.loss_history_ == a.loss_history_[:3]


def test_a_full_softmax_fit_leaves_nothing_behind_for_wmrb(tm, engine_only):
    p = bpr_problem(9, 60, 40, 33, 20)

    def wmrb_fit(model):
        model.loss_graph, model.random_ind = tm.WMRB(), torch.as_tensor(p['R'])
        model.fit(3, tm.eye(p['m']), tm.eye(p['n']), tm.Sparse(p['idx'], p['val'], (p['m'], p['n'])), lr=LR)
        return model
    alone = fit_full(tm, p, 3, loss=tm.WMRB(), random_ind=torch.as_tensor(p['R']))
    model = fit_full(tm, p, 3)
    full_history, full_U = list(model.loss_history_), model.user_embedding.clone()
    wmrb_fit(model)                                                           # then a WMRB fit on the same model
    assert model.loss_history_ == alone.loss_history_ and alone.loss_history_ != full_history
    assert torch.equal(model.user_embedding, alone.user_embedding) and torch.equal(model.item_embedding, alone.item_embedding)
    assert not torch.equal(alone.user_embedding, full_U)


def test_refusals_on_the_gpu(tm, engine_only):
    limit = tm.E.FULL_SOFTMAX_MAX_COMPONENTS
    assert limit == tm.lib.tmf_fsm_max_components()
    p = bpr_problem(15, 12, 9, limit + 1, 4)
    with pytest.raises(NotImplementedError, match=f'n_components={limit + 1} > {limit}'):
        fit_full(tm, p, 1)
    p = bpr_problem(15, 12, 9, 4, 4)
    with pytest.raises(NotImplementedError, match='factor_dtype'):
        fit_full(tm, p, 1, factor_dtype=torch.bfloat16)
    for setting in (dict(batch_users=8), dict(shard_items=2), dict(data_parallel='force')):
        with pytest.raises(NotImplementedError, match=next(iter(setting))):
            fit_full(tm, p, 1, **setting)
