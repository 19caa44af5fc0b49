"""L2 regularisation (model.user_alpha / model.item_alpha) on the MI355X: the four regularised table steps through the C ABI, bit for
bit, and regularised fits on the engine against fp64 references "closed-form data gradient + 2 alpha W0".

What "bit for bit" is measured against.  The steps compute g' = fl(g + fl(l2 w)) and hand g' to the op sequence of the function they
extend.  g' is restated here in NumPy float32 (one product, one sum, each rounded to nearest).  The rest of the sequence cannot be
restated bit for bit on a host: the kernels' square root is the hardware's v_sqrt_f32, accurate to 1 ulp and not correctly rounded
(tests/test_gpu_biased.py::assert_fresh_adam_mirror), and the persistent-Adam kernel is compiled with contracted multiply-adds.  So
every regularised step is compared, bit for bit, with the EXISTING step kernel applied to the NumPy g' - everything this feature adds
is on the NumPy side of that comparison - and, for the fresh-Adam steps, with the full NumPy float32 mirror within the bound the
existing test derives for that square root (the bf16 mirror ends in round-to-nearest-even).  Measured on an MI355X at 70 001 x 33
(4 480 064 stored elements): 120 889 (l2 = 0.25) and 125 423 (l2 = 3.0) fp32 results differ from the whole-step NumPy mirror, every
one within that bound; 3 do after the bf16 rounding; none differs from the existing kernel applied to the NumPy g'."""
import gc

import numpy as np
import pytest
import torch

from conftest import assert_step, rel_err, step_bounds
from test_biased_cpu import LR, biased_oracle, biased_problem
from test_bpr_cpu import bpr_closed_form, bpr_problem
from test_features_cpu import UNUSED, featured_problem
from test_features_cpu import _model as featured_model
from test_gpu_features import assert_step_with_slack, embedding_gradients
from test_l2_cpu import ALPHAS, TRAJECTORY_EPOCHS, TRAJECTORY_LR, l2_trajectory
from test_logistic_cpu import logistic_closed_form, logistic_problem

pytestmark = pytest.mark.gpu
NAN = float('nan')


@pytest.fixture(scope='module')
def tm():
    from teamoflow_amd import _engine, _lib
    from teamoflow_amd.mf import embedding_graphs as EG
    from teamoflow_amd.mf import loss_graphs as LG
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseFeatures, SparseInteractions, eye
    lib = _lib.get()

    class NS:
        pass
    ns = NS()
    ns.lib, ns.L, ns.E, ns.EG, ns.LG, ns.MF, ns.Fixed, ns.Sparse, ns.SF, ns.eye = lib, _lib, _engine, EG, LG, MatrixFactorization, \
        FixedInitializer, SparseInteractions, SparseFeatures, eye
    return ns


@pytest.fixture
def engine_only(tm, monkeypatch):
    """_fit_generic refuses to run: a fit that passes ran on the engine."""
    def refuse(self, *a, **k):
        raise AssertionError('_fit_generic was called')
    monkeypatch.setattr(tm.MF, '_fit_generic', refuse)


def host(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype is torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------------------
# the kernels through the C ABI
# ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (3, 33), (257, 128), (5, 300), (70001, 33)]   # the last: ld 64 -> more than 4096 x 256 float4, a second grid-stride trip
L2S = [0.25, 3.0]


def table(seed, rows, r, ld, scale=1.0, pad=0.0):
    """[rows, ld] fp32 on the device: normal values of magnitude ``scale`` with every eleventh element an exact zero, the padding
    columns ``pad``."""
    gen = torch.Generator(device='cuda').manual_seed(seed)
    t = torch.randn(rows, ld, generator=gen, device='cuda', dtype=torch.float32) * scale
    t.view(-1)[5::11] = 0.0
    t[:, r:] = pad
    return t


def l2_grad_numpy(G, W, l2):
    """g' = fl(g + fl(l2 w)) in NumPy float32: two operations, each rounded to nearest once.  W: fp32 or bf16 (widened exactly)."""
    g, w = G.cpu().numpy(), W.float().cpu().numpy()
    prod = np.float32(l2) * w
    out = g + prod
    assert prod.dtype == np.float32 and out.dtype == np.float32
    return torch.from_numpy(out).to(G.device)


def fresh_adam_numpy(w, g, lr=LR):
    """(w1, q): the fresh-Adam op sequence in NumPy float32 (tests/test_gpu_biased.py::assert_fresh_adam_mirror) and its quotient."""
    from oracle import dense_ref as D
    alpha, omb1, omb2, eps = D.adam_fresh_constants(lr)
    q = ((g * omb1) * alpha) / (np.sqrt((g * g) * omb2) + eps)
    w1 = w - q
    assert q.dtype == np.float32 and w1.dtype == np.float32
    return w1, q


def to_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).float().numpy()   # round-to-nearest-even


def assert_numpy_mirror(got, W0, Gp, bf16, what):
    """The whole step restated in NumPy float32 from g': within 2^-23 (3 |q| + |w1|) of the kernel (the 1-ulp square root; the bound
    of assert_fresh_adam_mirror); a bf16 result lies between the round-to-nearest-even values of the two ends of that interval."""
    w0, gp, got = W0.float().cpu().numpy(), Gp.cpu().numpy(), got.float().cpu().numpy()
    w1, q = fresh_adam_numpy(w0, gp)
    tol = 2.0 ** -23 * (3.0 * np.abs(q.astype(np.float64)) + np.abs(w1.astype(np.float64)))
    if bf16:
        lo, hi = to_bf16((w1 - tol).astype(np.float32)), to_bf16((w1 + tol).astype(np.float32))
        differ = int((got != to_bf16(w1)).sum())
        ok = (got >= lo) & (got <= hi)
    else:
        differ = int((got != w1).sum())
        ok = np.abs(got.astype(np.float64) - w1.astype(np.float64)) <= tol
    print(f'[mirror] {what}: {differ} of {got.size} elements differ from the NumPy float32 mirror')
    assert ok.all(), (what, int((~ok).sum()))


@pytest.mark.parametrize('l2', L2S)
@pytest.mark.parametrize('rows,r', SHAPES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_fresh_rows_l2(tm, dtype, rows, r, l2):
    L, lib, P, s = tm.L, tm.lib, tm.L.ptr, tm.L.stream_ptr()
    bf16 = dtype is torch.bfloat16
    ld = L.padded_ld(r, dtype)
    sfx = '_bf16' if bf16 else '_f32'
    adam = tm.E.adam_constants(LR)
    W0 = table(3 * rows + r, rows, r, ld, 0.3).to(dtype)
    G = table(5 * rows + r, rows, r, ld, 2.0)
    G0 = G.clone()
    Gp = l2_grad_numpy(G, W0, l2)
    W, W_ref = W0.clone(), W0.clone()
    L.check(getattr(lib, 'tmf_adam_fresh_rows_l2' + sfx)(P(W), P(G), rows, r, adam, l2, s), lib)
    L.check(getattr(lib, 'tmf_adam_fresh_rows' + sfx)(P(W_ref), P(Gp), rows, r, adam, s), lib)      # the existing step on NumPy's g'
    torch.cuda.synchronize()
    what = f'fresh_rows_l2{sfx} {rows}x{r} l2={l2}'
    assert same_bits(W, W_ref), what
    assert same_bits(G, G0), f'{what}: the gradient is only read'
    assert not W[:, r:].any(), f'{what}: padding columns'
    assert not same_bits(W, W0)
    assert_numpy_mirror(W, W0, Gp, bf16, what)
    # l2 = 0: the existing function's bits
    Z, Z_ref = W0.clone(), W0.clone()
    L.check(getattr(lib, 'tmf_adam_fresh_rows_l2' + sfx)(P(Z), P(G), rows, r, adam, 0.0, s), lib)
    L.check(getattr(lib, 'tmf_adam_fresh_rows' + sfx)(P(Z_ref), P(G), rows, r, adam, s), lib)
    torch.cuda.synchronize()
    assert same_bits(Z, Z_ref), f'{what}: l2 = 0'


@pytest.mark.parametrize('l2', L2S)
@pytest.mark.parametrize('rows,r', SHAPES)
def test_state_rows_l2(tm, rows, r, l2):
    """Two successive steps (the second with non-zero moments and the step-2 scalars): each equals tmf_adam_state_rows_f32 on the
    NumPy g' of the table it started from, tables and moments; the first also the fresh step on g'."""
    L, lib, P, s = tm.L, tm.lib, tm.L.ptr, tm.L.stream_ptr()
    ld = L.padded_ld(r)
    W0 = table(7 * rows + r, rows, r, ld, 0.3)
    what = f'state_rows_l2 {rows}x{r} l2={l2}'
    got = [W0.clone(), torch.zeros_like(W0), torch.zeros_like(W0)]
    ref = [W0.clone(), torch.zeros_like(W0), torch.zeros_like(W0)]
    for step in (1, 2):
        a = lib.tmf_adam_step(LR, step)
        G = table(11 * rows + r + step, rows, r, ld, 2.0)
        G0, W_before = G.clone(), got[0].clone()
        Gp = l2_grad_numpy(G, W_before, l2)
        L.check(lib.tmf_adam_state_rows_l2_f32(P(got[0]), P(G), P(got[1]), P(got[2]), rows, r, a, l2, s), lib)
        L.check(lib.tmf_adam_state_rows_f32(P(ref[0]), P(Gp), P(ref[1]), P(ref[2]), rows, r, a, s), lib)
        torch.cuda.synchronize()
        for x, y, name in zip(got, ref, ('W', 'M', 'V')):
            assert same_bits(x, y), f'{what} step {step}: {name}'
            assert not x[:, r:].any(), f'{what} step {step}: padding columns of {name}'
        assert same_bits(G, G0), f'{what}: the gradient is only read'
        if step == 1:
            F = W_before.clone()
            L.check(lib.tmf_adam_fresh_rows_l2_f32(P(F), P(G), rows, r, tm.E.adam_constants(LR), l2, s), lib)
            torch.cuda.synchronize()
            assert same_bits(got[0], F), f'{what}: step 1 with zero moments is the fresh step'
            assert_numpy_mirror(got[0], W_before, Gp, False, what)
    # l2 = 0, two successive steps: the existing function's bits
    z = [W0.clone(), torch.zeros_like(W0), torch.zeros_like(W0)]
    zr = [W0.clone(), torch.zeros_like(W0), torch.zeros_like(W0)]
    for step in (1, 2):
        a = lib.tmf_adam_step(LR, step)
        G = table(11 * rows + r + step, rows, r, ld, 2.0)
        L.check(lib.tmf_adam_state_rows_l2_f32(P(z[0]), P(G), P(z[1]), P(z[2]), rows, r, a, 0.0, s), lib)
        L.check(lib.tmf_adam_state_rows_f32(P(zr[0]), P(G), P(zr[1]), P(zr[2]), rows, r, a, s), lib)
    torch.cuda.synchronize()
    assert all(same_bits(x, y) for x, y in zip(z, zr)), f'{what}: l2 = 0'


@pytest.mark.parametrize('l2', L2S)
@pytest.mark.parametrize('rows,r', SHAPES)
def test_bias_rows_l2(tm, rows, r, l2):
    """tmf_adam_bias_rows_l2_f32: W as the fresh step on the NumPy g' (g' from the RAW weight), E = fl(W + b), the padding columns
    of W and E zeros whatever W, G and b held there (NaN here)."""
    L, lib, P, s = tm.L, tm.lib, tm.L.ptr, tm.L.stream_ptr()
    ld = L.padded_ld(r)
    adam = tm.E.adam_constants(LR)
    W0 = table(13 * rows + r, rows, r, ld, 0.3, pad=NAN)
    G = table(17 * rows + r, rows, r, ld, 2.0, pad=NAN)
    b = table(19 * rows + r, 1, r, ld, 0.1, pad=NAN)
    G0 = G.clone()
    what = f'bias_rows_l2 {rows}x{r} l2={l2}'
    clean = lambda t: torch.where(torch.isnan(t), torch.zeros_like(t), t)   # noqa: E731
    Gp = l2_grad_numpy(clean(G), clean(W0), l2)
    W, E = W0.clone(), torch.full_like(W0, NAN)
    L.check(lib.tmf_adam_bias_rows_l2_f32(P(W), P(G), P(b), P(E), rows, r, adam, l2, s), lib)
    W_ref, E_ref = clean(W0), torch.full_like(W0, NAN)
    L.check(lib.tmf_adam_bias_rows_f32(P(W_ref), P(Gp), P(b), P(E_ref), rows, r, adam, s), lib)   # the existing step on NumPy's g'
    F = clean(W0)
    L.check(lib.tmf_adam_fresh_rows_l2_f32(P(F), P(clean(G)), rows, r, adam, l2, s), lib)
    torch.cuda.synchronize()
    assert same_bits(W, W_ref) and same_bits(E, E_ref), what
    assert same_bits(W, F), f'{what}: the weights take the plain regularised step'
    assert not W[:, r:].any() and not E[:, r:].any(), f'{what}: padding columns'
    assert torch.equal(E[:, :r], W[:, :r] + b[0, :r]), f'{what}: E = fl(W + b)'
    assert same_bits(G[:, :r], G0[:, :r]) and bool(torch.isnan(G[:, r:]).all()) if r < ld else same_bits(G, G0), f'{what}: G is only read'
    assert_numpy_mirror(W[:, :r], clean(W0)[:, :r], Gp[:, :r], False, what)
    Z, EZ, Zr, EZr = W0.clone(), torch.full_like(W0, NAN), W0.clone(), torch.full_like(W0, NAN)
    L.check(lib.tmf_adam_bias_rows_l2_f32(P(Z), P(G), P(b), P(EZ), rows, r, adam, 0.0, s), lib)
    L.check(lib.tmf_adam_bias_rows_f32(P(Zr), P(G), P(b), P(EZr), rows, r, adam, s), lib)
    torch.cuda.synchronize()
    assert same_bits(Z, Zr) and same_bits(EZ, EZr), f'{what}: l2 = 0'


def test_table_past_32_bit_byte_offsets(tm):
    """8,400,000 x 128 fp32 = 4.3e9 bytes: slices at the start, across byte offset 2^32 and at the end against the existing step on
    the g' of copies of those slices (taken before the in-place update).  A 32-bit offset would fold the tail onto the head."""
    L, lib, P, s = tm.L, tm.lib, tm.L.ptr, tm.L.stream_ptr()
    rows, r, l2 = 8_400_000, 128, 0.25
    assert rows * r * 4 > 2 ** 32
    adam = tm.E.adam_constants(LR)
    gen = torch.Generator(device='cuda').manual_seed(9)
    W = torch.randn(rows, r, generator=gen, device='cuda') * 0.3
    G = torch.randn(rows, r, generator=gen, device='cuda') * 2.0
    cross = 2 ** 32 // (4 * r)                                    # the row that starts at byte offset 2^32
    blocks = [(0, 2048), (cross - 1024, cross + 1024), (rows - 2048, rows)]
    want = []
    for lo, hi in blocks:
        w = W[lo:hi].clone()
        gp = l2_grad_numpy(G[lo:hi].clone(), w, l2)
        L.check(lib.tmf_adam_fresh_rows_f32(P(w), P(gp), hi - lo, r, adam, s), lib)
        want.append(w)
    g_head = G[:2048].clone()
    L.check(lib.tmf_adam_fresh_rows_l2_f32(P(W), P(G), rows, r, adam, l2, s), lib)
    torch.cuda.synchronize()
    for (lo, hi), w in zip(blocks, want):
        assert same_bits(W[lo:hi], w), (lo, hi)
    assert same_bits(G[:2048], g_head)
    del W, G, want
    gc.collect()
    torch.cuda.empty_cache()


def test_bad_arguments_leave_the_table_untouched(tm):
    L, lib, P, s = tm.L, tm.lib, tm.L.ptr, tm.L.stream_ptr()
    adam = tm.E.adam_constants(LR)
    rows, r = 9, 33
    for name, sfx_dtype in (('tmf_adam_fresh_rows_l2_f32', torch.float32), ('tmf_adam_fresh_rows_l2_bf16', torch.bfloat16),
                            ('tmf_adam_state_rows_l2_f32', torch.float32), ('tmf_adam_bias_rows_l2_f32', torch.float32)):
        ld = L.padded_ld(r, sfx_dtype)
        W0 = table(23, rows, r, ld, 0.3).to(sfx_dtype)
        W, G = W0.clone(), table(29, rows, r, ld, 2.0)
        extra = {'tmf_adam_state_rows_l2_f32': [torch.zeros(rows, ld, device='cuda'), torch.zeros(rows, ld, device='cuda')],
                 'tmf_adam_bias_rows_l2_f32': [torch.zeros(ld, device='cuda'), torch.zeros(rows, ld, device='cuda')]}.get(name, [])
        extra0 = [x.clone() for x in extra]
        fn = getattr(lib, name)
        tabs = [W, G] + extra
        cases = [([P(t) for t in tabs], r, -0.5), ([P(t) for t in tabs], r, NAN), ([P(t) for t in tabs], r, float('inf')),
                 ([P(t) for t in tabs], 0, 0.25), ([P(t) for t in tabs], 1025, 0.25), ([P(t) for t in tabs], -3, 0.25)]
        cases += [([None if k == j else P(t) for k, t in enumerate(tabs)], r, 0.25) for j in range(len(tabs))]   # a null table
        for ptrs, rr, l2 in cases:
            assert fn(*ptrs, rows, rr, adam, l2, s) == -1, (name, rr, l2)                                       # TMF_E_INVALID
            assert lib.tmf_last_error()
        torch.cuda.synchronize()
        assert same_bits(W, W0) and all(same_bits(x, y) for x, y in zip(extra, extra0)), name


# ------------------------------------------------------------------------------------------------------------------------
# fits, engine only
# ------------------------------------------------------------------------------------------------------------------------
LOSSES = ('mse', 'wmrb', 'kl', 'logistic', 'bpr')
M, N, S = 300, 200, 64


def problem(loss, r):
    """(p, fp64 data loss mean, gU, gV) of the 300 x 200 problem of ``loss``.  The data gradient comes from the oracle (MSE, WMRB,
    KL) or the closed forms (Logistic, BPR).  WMRB: tables ~ N(0, 0.1^2), the scale of a fit's start, and a table of S = 64
    negatives; the reference must then hold no hinge term within fp32 reach of the kink (oracle.sparse_ref.wmrb_slack), so that its
    gradient is determined to the tolerance it is compared at."""
    seed = 4000 + r
    if loss == 'logistic':
        p = logistic_problem(seed, M, N, r, zeros=True)
        data, gU, gV, _ = logistic_closed_form(p['U0'], p['V0'], p['idx'], p['val'], False)
        return p, data / p['idx'].shape[0], gU, gV
    if loss == 'bpr':
        p = bpr_problem(seed, M, N, r, S)
        p['loss'] = 'bpr'
        data, _, _, gU, gV = bpr_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
        return p, data / int((p['val'] > 0).sum()), gU, gV
    p = biased_problem(seed, M, N, r, loss)
    if loss == 'wmrb':
        from oracle import sparse_ref as SR
        p['U0'], p['V0'], p['R'], p['S'] = p['U0'] / 3, p['V0'] / 3, np.ascontiguousarray(p['R'][:, :S]), S
        sl = SR.wmrb_slack(p['U0'].astype(np.float64), p['V0'].astype(np.float64), p['idx'], p['val'].astype(np.float64),
                           p['R'].astype(np.int64), N, S)
        assert sl['pairs'] == 0, 'the WMRB problem has hinge terms on the kink: its reference gradient is not determined'
    ref = biased_oracle(p, ('linear', 'linear'), 1)
    return p, ref['loss'][0], ref['first_grads'][0][0], ref['first_grads'][1][0]


@pytest.fixture(scope='module')
def problems():
    cache = {}

    def get(loss, r):
        if (loss, r) not in cache:
            cache[loss, r] = problem(loss, r)
        return cache[loss, r]
    return get


@pytest.fixture(scope='module')
def plain_fits(tm, problems):
    """The unregularised one-step fit of every (loss, r), run once and shared by the alpha pairs."""
    cache = {}

    def get(loss, r):
        if (loss, r) not in cache:
            p = problems(loss, r)[0]
            cache[loss, r] = fit(tm, new_model(tm, p), p, 1)
        return cache[loss, r]
    return get


def new_model(tm, p, **attrs):
    kw = dict(user_weight_graph=tm.Fixed(p['U0']), item_weight_graph=tm.Fixed(p['V0']))
    for k in ('user_repr_graph', 'item_repr_graph'):
        if k in attrs:
            kw[k] = attrs.pop(k)
    loss = p['loss']
    if loss in ('wmrb', 'bpr'):
        kw.update(loss_graph=tm.LG.WMRBLoss() if loss == 'wmrb' else tm.LG.BPRLoss(), n_users=p['m'], n_items=p['n'], n_samples=p['S'])
    elif loss == 'kl':
        kw.update(loss_graph=tm.LG.KLDivergenceLoss())
    elif loss == 'logistic':
        kw.update(loss_graph=tm.LG.LogisticLoss())
    model = tm.MF(p['U0'].shape[1], **kw)
    model.verbose = False
    if loss in ('wmrb', 'bpr'):
        model.random_ind = torch.as_tensor(p['R'])
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


def fit(tm, model, p, epochs, lr=LR, user_features=None, item_features=None):
    m, n = (p['m'], p['n']) if 'm' in p else (p['U0'].shape[0], p['V0'].shape[0])
    model.fit(epochs, tm.eye(m) if user_features is None else user_features, tm.eye(n) if item_features is None else item_features,
              tm.Sparse(p['idx'], p['val'], (m, n)), lr=lr)
    return model


def assert_l2_step(W_new, W0, g_data, alpha, what, lr=LR, extra_slack=None):
    """assert_step against g_data + 2 alpha W0 at rtol 1e-5 with the per-element slack 1e-5 (|g_data| + 2 alpha |W0|) - what the two
    terms may lose to cancellation.  The slack is logged (report_slack) and at most 1 % of the elements may need it."""
    W64, g_data = np.asarray(W0, np.float64), np.asarray(g_data, np.float64)
    g_ref = g_data + 2 * alpha * W64
    slack = 1e-5 * (np.abs(g_data) + 2 * alpha * np.abs(W64))
    if extra_slack is not None:
        slack = slack + extra_slack
    assert_step_with_slack(W_new, W64, g_ref, slack, lr, what)
    lo, hi = step_bounds(W64, g_ref, lr, 1e-5)
    need = int(((W_new < lo) | (W_new > hi)).sum())
    assert need <= 0.01 * g_ref.size, f'{what}: {need} of {g_ref.size} elements needed the slack'


@pytest.mark.parametrize('alphas', ALPHAS, ids=str)
@pytest.mark.parametrize('r', [33, 128])
@pytest.mark.parametrize('loss', LOSSES)
def test_one_step(tm, engine_only, problems, plain_fits, loss, r, alphas):
    p, data_loss, gU, gV = problems(loss, r)
    plain = plain_fits(loss, r)
    model = fit(tm, new_model(tm, p, user_alpha=alphas[0], item_alpha=alphas[1]), p, 1)
    what = f'{loss} r={r} alphas={alphas}'
    assert hasattr(model, '_state') and model._state.l2 == [np.float32(2 * a) for a in alphas], what
    assert model.loss_history_ == plain.loss_history_, f'{what}: loss_history_ is the data term'
    assert rel_err(model.loss_history_[0], data_loss) < 1e-5, what
    for side, got, ref, W0, g, alpha in (('U', model.user_embedding, plain.user_embedding, p['U0'], gU, alphas[0]),
                                         ('V', model.item_embedding, plain.item_embedding, p['V0'], gV, alphas[1])):
        if alpha == 0:
            assert same_bits(got, ref), f'{what} {side}: the unpenalised side differs from an unregularised fit'
        else:
            assert_l2_step(host(got), W0, g, alpha, f'l2 {what} {side}')
            assert not got[:, :].equal(ref)


def _bf16(x):
    return torch.tensor(np.asarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


@pytest.mark.parametrize('r', [8, 33, 128])
def test_bf16_storage_one_step(tm, engine_only, r):
    """bf16 factor storage / fp32 arithmetic: against the closed form + 2 alpha W0 on the bf16-rounded tables; the new rows must lie
    in the step interval rounded to bf16 (tests/test_gpu_logistic.py::test_bf16_storage_one_step)."""
    p = logistic_problem(100 + r, 60, 40, r, zeros=True)
    p['U0'], p['V0'] = _bf16(p['U0']), _bf16(p['V0'])
    loss, gU, gV, _ = logistic_closed_form(p['U0'], p['V0'], p['idx'], p['val'], False)
    plain = fit(tm, new_model(tm, p, factor_dtype=torch.bfloat16), p, 1)
    for alphas in ALPHAS:
        model = fit(tm, new_model(tm, p, factor_dtype=torch.bfloat16, user_alpha=alphas[0], item_alpha=alphas[1]), p, 1)
        assert model.user_embedding.dtype == torch.bfloat16 and hasattr(model, '_state')
        assert model.loss_history_ == plain.loss_history_ and rel_err(model.loss_history_[0], loss / p['idx'].shape[0]) < 1e-5
        for got, ref, W0, g, alpha in ((model.user_embedding, plain.user_embedding, p['U0'], gU, alphas[0]),
                                       (model.item_embedding, plain.item_embedding, p['V0'], gV, alphas[1])):
            if alpha == 0:
                assert same_bits(got, ref), (r, alphas)
                continue
            lo, hi = step_bounds(W0, g + 2 * alpha * W0.astype(np.float64), LR)
            got = host(got).astype(np.float64)
            assert (got >= _bf16(lo) - 1e-12).all() and (got <= _bf16(hi) + 1e-12).all(), (r, alphas)


@pytest.mark.parametrize('alphas', ALPHAS, ids=str)
@pytest.mark.parametrize('loss', ['mse', 'logistic'])
def test_biased_sides_one_step(tm, engine_only, loss, alphas):
    """Both sides biased (the biases start at zero, so E0 = W0): the weights step by g + 2 alpha W0, the bias - never penalised -
    equals an unregularised fit's bit for bit."""
    r = 33
    p = logistic_problem(1000 + r, 60, 40, r, zeros=True) if loss == 'logistic' else biased_problem(1000 + r, 60, 40, r, 'mse')
    if loss == 'logistic':
        _, gU, gV, _ = logistic_closed_form(p['U0'], p['V0'], p['idx'], p['val'], False)
    else:
        ref = biased_oracle(p, ('linear', 'linear'), 1)
        gU, gV = ref['first_grads'][0][0], ref['first_grads'][1][0]
    graphs = lambda: dict(user_repr_graph=tm.EG.BiasedLinearEmbedding(), item_repr_graph=tm.EG.BiasedLinearEmbedding())   # noqa: E731
    plain = fit(tm, new_model(tm, p, **graphs()), p, 1)
    model = fit(tm, new_model(tm, p, user_alpha=alphas[0], item_alpha=alphas[1], **graphs()), p, 1)
    st = model._state
    assert st.bias_u is not None and st.bias_v is not None and (st.bias_u.l2, st.bias_v.l2) == tuple(np.float32(2 * a) for a in alphas)
    assert model.loss_history_ == plain.loss_history_
    for side, W0, g, alpha in (('user', p['U0'], gU, alphas[0]), ('item', p['V0'], gV, alphas[1])):
        (W, b), (Wp, bp) = getattr(model, side + '_trainable'), getattr(plain, side + '_trainable')
        assert same_bits(b.detach(), bp.detach()), f'{loss} {alphas} {side}: the bias'
        assert torch.equal(getattr(model, side + '_embedding'), W + b.detach())
        if alpha == 0:
            assert same_bits(W, Wp)
        else:
            assert_l2_step(host(W), W0, g, alpha, f'l2 biased {loss} {alphas} {side} weights')


@pytest.mark.parametrize('alphas', ALPHAS, ids=str)
@pytest.mark.parametrize('featured', [('user',), ('user', 'item')], ids='+'.join)
def test_sides_over_sparse_features_one_step(tm, engine_only, featured, alphas):
    """Hybrid features [I | tags]: dL/dW = F^T dL/dE + 2 alpha W0.  The tag column no row carries has no data gradient: without a
    penalty it stays, with one it moves by the penalty step alone."""
    m, n, r = 60, 40, 33
    p = featured_problem(2000 + r, m, n, r, 'mse', 'hybrid')
    G = embedding_gradients(p, featured)
    feats = lambda: (tm.SF(*p['Fu']), tm.SF(*p['Fv']) if 'item' in featured else None)   # noqa: E731

    def run(**attrs):
        model = featured_model(p, featured)
        for k, v in attrs.items():
            setattr(model, k, v)
        uf, vf = feats()
        return fit(tm, model, p, 1, user_features=uf, item_features=vf)
    plain, model = run(), run(user_alpha=alphas[0], item_alpha=alphas[1])
    assert hasattr(model, '_state') and model._state.feat_u is not None and model.loss_history_ == plain.loss_history_
    for s, name, rows, G_ref, alpha in (('u', 'user', m, G[0], alphas[0]), ('v', 'item', n, G[1], alphas[1])):
        got, ref = getattr(model, name + '_trainable')[0], getattr(plain, name + '_trainable')[0]
        what = f'l2 featured {"+".join(featured)} {alphas} {name}'
        if alpha == 0:
            assert same_bits(got, ref), what
            continue
        if name not in featured:
            assert_l2_step(host(got), p['V0'], G_ref, alpha, what + ' table')
            continue
        W0, Fd = p['W' + s + '0'], p['F' + s + '_dense']
        # every row's gradient agrees to 1e-5 -> feature f's sum may be off by 1e-5 sum_i |x_if| |G_ref[i]| (tests/test_gpu_features.py)
        assert_l2_step(host(got), W0, Fd.T @ G_ref, alpha, what + ' weights', extra_slack=1e-5 * np.abs(Fd).T @ np.abs(G_ref))
        unused = rows + UNUSED
        assert not Fd[:, unused].any() and np.array_equal(host(ref)[unused], W0[unused])          # no row carries it: no data gradient
        assert_step(host(got)[unused], W0[unused], 2 * alpha * W0[unused].astype(np.float64), LR, rtol=1e-5, what=what + ' unused feature')
        assert (np.abs(host(got)[unused]) < np.abs(W0[unused])).all() or (np.abs(W0[unused]) < LR).any()
        emb, embed = getattr(model, name + '_embedding'), getattr(model, 'embed_' + name + 's')
        assert torch.equal(emb, embed(tm.SF(*p['F' + s]))), what + ': embedding != embed(F)'


@pytest.mark.parametrize('alphas', [(2.0, 2.0), (0.3, 0.7), (0.0, 2.0)], ids=str)
@pytest.mark.parametrize('seed', [6, 7, 8])
def test_trajectory(tm, engine_only, seed, alphas):
    p = logistic_problem(seed, 70, 45, 5, zeros=True)
    ref, _, _ = l2_trajectory(p['U0'], p['V0'], p['idx'], p['val'], alphas)
    model = fit(tm, new_model(tm, p, user_alpha=alphas[0], item_alpha=alphas[1]), p, TRAJECTORY_EPOCHS, lr=TRAJECTORY_LR)
    h = model.loss_history_
    print(f'[trajectory] seed={seed} alphas={alphas}: first three {rel_err(h[:3], ref[:3]):.3g}, all {rel_err(h, ref):.3g}')
    assert hasattr(model, '_state') and len(h) == TRAJECTORY_EPOCHS
    assert rel_err(h[:3], ref[:3]) < 1e-5 and rel_err(h, ref) < 1e-3
    if alphas == (2.0, 2.0):
        plain = fit(tm, new_model(tm, p), p, TRAJECTORY_EPOCHS, lr=TRAJECTORY_LR)
        assert torch.linalg.norm(model.user_embedding) < torch.linalg.norm(plain.user_embedding)
        assert torch.linalg.norm(model.item_embedding) < torch.linalg.norm(plain.item_embedding)
        assert h[-1] > plain.loss_history_[-1]


@pytest.mark.parametrize('alphas', [(0.5, 0.0), (0.3, 0.7)], ids=str)
@pytest.mark.parametrize('kind', ['plain', 'biased', 'featured'])
def test_graph_replay_equals_eager_and_fits_repeat(tm, engine_only, monkeypatch, kind, alphas):
    if kind == 'featured':
        p = featured_problem(21, 45, 30, 12, 'mse', 'hybrid')

        def run(epochs):
            model = featured_model(p, ('user',))
            model.user_alpha, model.item_alpha = alphas
            return fit(tm, model, p, epochs, user_features=tm.SF(*p['Fu']))
    else:
        p = logistic_problem(7, 60, 40, 12, zeros=True)
        graphs = (lambda: dict(user_repr_graph=tm.EG.BiasedLinearEmbedding())) if kind == 'biased' else dict

        def run(epochs):
            return fit(tm, new_model(tm, p, user_alpha=alphas[0], item_alpha=alphas[1], **graphs()), p, epochs)
    for epochs in (10, 13):                               # 10 = one replay; 13 = one replay of 12 and an eager epoch
        monkeypatch.delenv('TMF_NO_GRAPH', raising=False)
        a, b = run(epochs), run(epochs)
        monkeypatch.setenv('TMF_NO_GRAPH', '1')
        c = run(epochs)
        for other in (b, c):
            assert a.loss_history_ == other.loss_history_ and len(a.loss_history_) == epochs
            for x, y in zip([a.user_embedding, a.item_embedding] + a.user_trainable + a.item_trainable,
                            [other.user_embedding, other.item_embedding] + other.user_trainable + other.item_trainable):
                assert same_bits(x.detach(), y.detach())
        assert np.isfinite(a.loss_history_).all() and hasattr(a, '_state')


@pytest.mark.parametrize('alphas', ALPHAS, ids=str)
def test_opt_in_persistent_adam(tm, engine_only, alphas):
    """optimizer='adam': the first step is the fresh-Adam regularised fit's bit for bit; five steps follow Keras Adam on
    g' = g + 2 alpha W in NumPy fp64 (test_gpu_logistic.test_opt_in_persistent_adam's tolerances)."""
    p = logistic_problem(8, 60, 40, 12)
    kw = dict(user_alpha=alphas[0], item_alpha=alphas[1])
    a1, f1 = fit(tm, new_model(tm, p, optimizer='adam', **kw), p, 1), fit(tm, new_model(tm, p, **kw), p, 1)
    assert same_bits(a1.user_embedding, f1.user_embedding) and same_bits(a1.item_embedding, f1.item_embedding)
    assert a1.loss_history_ == f1.loss_history_
    got = fit(tm, new_model(tm, p, optimizer='adam', **kw), p, 5)
    U, V = p['U0'].astype(np.float64), p['V0'].astype(np.float64)
    mU, vU, mV, vV = (np.zeros_like(x) for x in (U, U, V, V))
    ref = []
    for t in range(1, 6):
        loss, gU, gV, _ = logistic_closed_form(U, V, p['idx'], p['val'], False)
        gU, gV = gU + 2 * alphas[0] * U, gV + 2 * alphas[1] * V
        ref.append(loss / p['idx'].shape[0])
        alpha = LR * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        mU += (gU - mU) * 0.1
        vU += (gU ** 2 - vU) * 0.001
        mV += (gV - mV) * 0.1
        vV += (gV ** 2 - vV) * 0.001
        U = U - alpha * mU / (np.sqrt(vU) + 1e-7)
        V = V - alpha * mV / (np.sqrt(vV) + 1e-7)
    assert rel_err(got.loss_history_, ref) < 1e-4
    assert np.abs(host(got.user_embedding) - U).max() < 1e-3 and np.abs(host(got.item_embedding) - V).max() < 1e-3
    plain = fit(tm, new_model(tm, p, optimizer='adam'), p, 5)
    assert not torch.equal(plain.user_embedding, got.user_embedding) or not torch.equal(plain.item_embedding, got.item_embedding)


def test_a_relu_side_on_the_engine_is_refused(tm):
    p = logistic_problem(9, 12, 9, 2)
    model = new_model(tm, p, user_repr_graph=tm.EG.ReLUEmbedding(), relu_engine=True, item_alpha=0.5)
    with pytest.raises(NotImplementedError, match='relu_engine'):
        fit(tm, model, p, 1)
