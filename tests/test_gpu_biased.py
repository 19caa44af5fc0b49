"""BiasedLinearEmbedding over indicator features on the sparse HIP engine (tmf_bias_colsum_f32 / tmf_bias_adam_f32 /
tmf_adam_bias_rows_f32, _engine.BiasSide / epoch_sides) against oracle.dense_ref.fit_dense_plugins - the reference loop on the dense
[m, n] scores, fine at these sizes.  The problems are test_biased_cpu.biased_problem's; that file also shows, on the reference
alone, that the tolerances used here hold for the fp32 oracle itself and why no test looks at a WMRB item bias: it cancels
analytically, so the reference steps it on rounding noise.  A whole WMRB fit therefore compares the raw item weights, the loss
trajectory and the per-user rankings (invariant to that bias), never the bias or the item embedding that carries it."""
import gc

import numpy as np
import pytest
import torch

from conftest import assert_step, rel_err
from test_biased_cpu import LR, SIDES, assert_bias_step, biased_oracle, biased_problem

pytestmark = pytest.mark.gpu
GUARD = 3
SENTINEL = 12345.0
LOSSES = ('mse', 'wmrb', 'kl')


@pytest.fixture(scope='module')
def tm():
    from teamoflow_amd import _engine, _lib
    from teamoflow_amd.mf import embedding_graphs as EG
    from teamoflow_amd.mf import loss_graphs as LG
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    lib = _lib.get()

    class NS:
        pass
    ns = NS()
    ns.lib, ns.L, ns.E, ns.MF, ns.Fixed, ns.EG, ns.LG, ns.Sparse, ns.eye = lib, _lib, _engine, MatrixFactorization, FixedInitializer, \
        EG, LG, SparseInteractions, eye
    return ns


def new_model(tm, p, sides, **attrs):
    graph = {'biased': tm.EG.BiasedLinearEmbedding, 'linear': tm.EG.LinearEmbedding}
    kw = dict(user_repr_graph=attrs.pop('user_graph', None) or graph[sides[0]](),
              item_repr_graph=attrs.pop('item_graph', None) or graph[sides[1]](),
              user_weight_graph=tm.Fixed(p['U0']), item_weight_graph=tm.Fixed(p['V0']))
    if p['loss'] == 'wmrb':
        kw.update(loss_graph=tm.LG.WMRBLoss(), n_users=p['m'], n_items=p['n'], n_samples=p['S'])
    elif p['loss'] == 'kl':
        kw.update(loss_graph=tm.LG.KLDivergenceLoss())
    model = tm.MF(p['r'], **kw)
    model.verbose = False
    if p['loss'] == 'wmrb':
        model.random_ind = torch.as_tensor(p['R'])
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


def fit(tm, model, p, epochs, lr=LR, user_features=None, item_features=None):
    model.fit(epochs, tm.eye(p['m']) if user_features is None else user_features,
              tm.eye(p['n']) if item_features is None else item_features, tm.Sparse(p['idx'], p['val'], (p['m'], p['n'])), lr=lr)
    return model


def host(t):
    return t.detach().float().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------
# one step against the fp64 oracle
# ------------------------------------------------------------------------------------------------------------------------
ONE_STEP = [('mse', r) for r in (1, 3, 7, 33, 64, 100, 128, 200, 300)] + [(loss, r) for loss in ('wmrb', 'kl') for r in (3, 33, 128)]


@pytest.mark.parametrize('sides', SIDES, ids=['-'.join(s) for s in SIDES])
@pytest.mark.parametrize('loss,r', ONE_STEP)
def test_one_step(tm, loss, r, sides):
    p = biased_problem(1000 + r, 60, 40, r, loss)
    ref = biased_oracle(p, sides, 1)
    model = fit(tm, new_model(tm, p, sides), p, 1)
    what = f'{loss} r={r} {sides}'
    assert hasattr(model, '_state'), 'the fit did not run on the engine'
    assert rel_err(model.loss_history_[0], ref['loss'][0]) < 1e-5, what
    zero = np.zeros((1, r))
    for side, kind, W0, got, emb, kept, grads, empty in (
            ('user', sides[0], p['U0'], model.user_trainable, model.user_embedding, model.user_linear_bias, ref['first_grads'][0],
             p['empty_user']),
            ('item', sides[1], p['V0'], model.item_trainable, model.item_embedding, model.item_linear_bias, ref['first_grads'][1],
             None if loss == 'wmrb' else p['empty_item'])):       # WMRB samples the item without interactions as a negative
        assert emb.is_cuda and emb.shape == W0.shape
        assert_step(host(got[0]), W0, grads[0], LR, what=f'{what} {side} weights')
        if kind == 'biased':
            assert len(got) == 2 and got[1] is kept and kept.shape == (1, r) and kept.is_cuda
            assert kept.is_leaf and kept.requires_grad
            if not (loss == 'wmrb' and side == 'item'):
                assert_bias_step(host(kept), zero, grads[1], grads[0], LR, f'{what} {side} bias')
            assert torch.equal(emb, got[0] + kept.detach()), f'{what} {side}: embedding != fl(weights + bias)'
            b_new = host(kept)
        else:
            assert len(got) == 1 and kept is None and torch.equal(emb, got[0])
            b_new = np.zeros((1, r), np.float32)
        if empty is not None:   # a row no interaction touches: its weights do not move, its embedding follows the bias
            assert np.array_equal(host(got[0])[empty], W0[empty]), f'{what} {side}'
            assert np.array_equal(host(emb)[empty], W0[empty] + b_new[0]), f'{what} {side}'


# ------------------------------------------------------------------------------------------------------------------------
# the kernels through the C ABI (no leading dimension in it: contiguous operands between guard rows that must stay untouched)
# ------------------------------------------------------------------------------------------------------------------------
def guarded(rows, ld, dtype, fill, src=None):
    buf = torch.full((rows + 2 * GUARD, ld), fill, dtype=dtype, device='cuda')
    view = buf[GUARD:GUARD + rows]
    if src is not None:
        view.copy_(src)
    return view, buf


def guards_intact(buf, fill):
    g = torch.cat([buf[:GUARD], buf[buf.shape[0] - GUARD:]])
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


def random_table(seed, rows, r, ld, pad):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    t = torch.randn(rows, ld, generator=gen, device='cuda', dtype=torch.float32)
    t[:, r:] = pad
    return t


def run_colsum(tm, G, r):
    """-> (colsum [ld] fp64, part [P, ld] fp64), guards checked."""
    n_rows, ld = G.shape
    P = tm.lib.tmf_bias_colsum_part_rows(n_rows)
    part, part_buf = guarded(P, ld, torch.float64, SENTINEL)
    out, out_buf = guarded(1, ld, torch.float64, SENTINEL)
    tm.L.check(tm.lib.tmf_bias_colsum_f32(tm.L.ptr(G) if n_rows else None, n_rows, r, tm.L.ptr(part), P, tm.L.ptr(out),
                                          tm.L.stream_ptr()), tm.lib)
    torch.cuda.synchronize()
    assert guards_intact(part_buf, SENTINEL) and guards_intact(out_buf, SENTINEL)
    return out[0].clone(), part.clone()


@pytest.mark.parametrize('r', [1, 3, 33, 128, 300])
@pytest.mark.parametrize('n_rows', [0, 1, 63, 64, 65, 1000, 70001])
def test_colsum_against_numpy(tm, n_rows, r):
    ld = tm.L.padded_ld(r)
    G = random_table(n_rows * 1000 + r, n_rows, r, ld, float('nan'))
    got, part = run_colsum(tm, G, r)
    Gh = G[:, :r].cpu().numpy().astype(np.float64)
    ref = Gh.sum(0)
    bound = n_rows * 2.0 ** -53 * np.abs(Gh).sum(0)      # the worst case of any fp64 summation order
    got_h = got.cpu().numpy()
    assert (np.abs(got_h[:r] - ref) <= bound).all(), (n_rows, r, float(np.abs(got_h[:r] - ref).max()))
    assert not got_h[r:].any()                            # NaN in the padding columns of G never reaches the result
    again, part2 = run_colsum(tm, G, r)
    assert torch.equal(got, again) and torch.equal(part[:, :r], part2[:, :r])


def assert_fresh_adam_mirror(got, w0, g, what):
    """The one-step formula of oracle.dense_ref.adam_fresh_step, w - (g (1-b1) alpha) / (sqrt(g g (1-b2)) + eps), evaluated on the host
    in fp32 with every operation rounded to nearest (NumPy float32 scalars of adam_fresh_constants), against the kernel's result.
    Not bit for bit: the kernels' multiply, add and divide are correctly rounded, but their square root is the hardware's
    v_sqrt_f32, which is accurate to 1 ulp.  With s the square root, d = s + eps, q = n / d and w1 = w - q: s is off by at most
    1 ulp <= 2^-23 s, so d by at most 2^-23 d plus one rounding to a neighbouring value (2 x 2^-23 d), q by that plus one rounding
    (3 x 2^-23 |q|), and w1 by that plus one rounding of w1 itself:  |got - mirror| <= 2^-23 (3 |q| + |w1|)."""
    from oracle import dense_ref as D
    alpha, omb1, omb2, eps = D.adam_fresh_constants(LR)
    w0, g, got = (np.asarray(x.detach().cpu().numpy(), np.float32) for x in (w0, g, got))
    q = ((g * omb1) * alpha) / (np.sqrt((g * g) * omb2) + eps)
    w1 = w0 - q
    assert q.dtype == np.float32 and w1.dtype == np.float32
    tol = 2.0 ** -23 * (3.0 * np.abs(q.astype(np.float64)) + np.abs(w1.astype(np.float64)))
    d = np.abs(got.astype(np.float64) - w1.astype(np.float64))
    print(f'[mirror] {what}: {int((got != w1).sum())} of {got.size} elements differ from the host mirror, worst {float((d / np.maximum(tol, 1e-300)).max()):.3g} of the bound')
    assert (d <= tol).all(), (what, float((d / np.maximum(tol, 1e-300)).max()))


@pytest.mark.parametrize('r', [1, 3, 33, 128, 300])
@pytest.mark.parametrize('n_rows', [1, 65, 1000])
def test_bias_step_and_row_update_against_the_host_mirror(tm, n_rows, r):
    """tmf_bias_adam_f32 and tmf_adam_bias_rows_f32 against the host mirror of the fresh-Adam arithmetic (assert_fresh_adam_mirror),
    bit for bit against tmf_adam_fresh_rows_f32 on the same inputs and against fl(W + b)."""
    L, lib, P, s = tm.L, tm.lib, tm.L.ptr, tm.L.stream_ptr()
    ld = L.padded_ld(r)
    nan = float('nan')
    adam = tm.E.adam_constants(LR)
    W0 = random_table(7 * n_rows + r, n_rows, r, ld, 0.0)
    G, G_buf = guarded(n_rows, ld, torch.float32, nan, random_table(11 * n_rows + r, n_rows, r, ld, nan))
    b0 = random_table(13 * n_rows + r, 1, r, ld, 0.0) * 0.1
    colsum, part = run_colsum(tm, G, r)
    # ---- bias step ----
    b, b_buf = guarded(1, ld, torch.float32, nan, b0)
    g_out, g_buf = guarded(1, ld, torch.float32, nan)
    L.check(lib.tmf_bias_adam_f32(P(part), part.shape[0], P(b), P(g_out), r, adam, s), lib)
    torch.cuda.synchronize()
    assert guards_intact(b_buf, nan) and guards_intact(g_buf, nan)
    g_b = colsum.to(torch.float32)                        # the fp64 sums rounded once
    assert torch.equal(g_out[0], g_b) and not g_out[0, r:].any() and not b[0, r:].any()
    assert_fresh_adam_mirror(b[0, :r], b0[0, :r], g_b[:r], f'bias step n_rows={n_rows} r={r}')
    # ---- row update ----
    W, W_buf = guarded(n_rows, ld, torch.float32, nan, W0)
    E, E_buf = guarded(n_rows, ld, torch.float32, nan)
    L.check(lib.tmf_adam_bias_rows_f32(P(W), P(G), P(b), P(E), n_rows, r, adam, s), lib)
    W_ref, G_clean = W0.clone(), G.clone()
    G_clean[:, r:] = 0.0
    L.check(lib.tmf_adam_fresh_rows_f32(P(W_ref), P(G_clean), n_rows, r, adam, s), lib)
    torch.cuda.synchronize()
    assert guards_intact(W_buf, nan) and guards_intact(E_buf, nan) and guards_intact(G_buf, nan)
    assert torch.equal(W, W_ref) and not W[:, r:].any()
    assert_fresh_adam_mirror(W[:, :r], W0[:, :r], G[:, :r], f'row update n_rows={n_rows} r={r}')
    assert torch.equal(E[:, :r], W[:, :r] + b[0, :r]) and not E[:, r:].any()
    assert torch.equal(G[:, :r], G_clean[:, :r]) and bool(torch.isnan(G[:, r:]).all())      # the gradient is only read


def test_tables_past_32_bit_offsets(tm):
    """n_rows x ld just above 2^31 elements (r = 512): the column sum against torch.sum(dtype=float64) and the row update against
    torch ops on the device, block by block; a 32-bit offset would fold the last rows onto the first."""
    L, lib, P, s = tm.L, tm.lib, tm.L.ptr, tm.L.stream_ptr()
    r = ld = 512
    n_rows = 2 ** 22 + 5
    assert n_rows * ld > 2 ** 31
    adam = tm.E.adam_constants(LR)
    gen = torch.Generator(device='cuda').manual_seed(5)
    G = torch.randn(n_rows, ld, generator=gen, device='cuda')
    colsum, _ = run_colsum(tm, G, r)
    ref = torch.sum(G, 0, dtype=torch.float64)
    bound = n_rows * 2.0 ** -53 * torch.sum(G.abs(), 0, dtype=torch.float64)
    assert bool(((colsum - ref).abs() <= bound).all())
    tail = torch.sum(G[2 ** 22:], 0, dtype=torch.float64)                     # the rows past 2^31 elements count
    assert bool((tail.abs() > bound).any())
    W = torch.randn(n_rows, ld, generator=gen, device='cuda')
    b = torch.randn(ld, generator=gen, device='cuda') * 0.1
    E = torch.empty_like(W)
    # the reference of a few blocks of rows, taken before the in-place update: the first rows, the rows around 2^31 elements, the last
    a = adam
    blocks = [(0, 4096), (2 ** 21, 2 ** 21 + 4096), (2 ** 22 - 2048, n_rows)]
    want = []
    for lo, hi in blocks:
        g, w = G[lo:hi], W[lo:hi]
        w1 = w - ((g * a.one_minus_b1) * a.alpha) / (torch.sqrt((g * g) * a.one_minus_b2) + a.eps)
        want.append((w1, w1 + b))
    L.check(lib.tmf_adam_bias_rows_f32(P(W), P(G), P(b), P(E), n_rows, r, adam, s), lib)
    torch.cuda.synchronize()
    for (lo, hi), (w1, e1) in zip(blocks, want):
        # fp32 rounding of the update itself (conftest.step_bounds' allowance): 1e-6 relative to max(|w|, lr)
        tol = 1e-6 * torch.clamp(w1.abs(), min=LR)
        assert bool(((W[lo:hi] - w1).abs() <= tol).all()), (lo, hi)
        assert torch.equal(E[lo:hi], W[lo:hi] + b), (lo, hi)
    del G, W, E, want, ref
    gc.collect()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------
# whole fits
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss', LOSSES)
def test_trajectory(tm, loss):
    """40 epochs, both sides biased, against the fp32 oracle with the existing plug-in test's bounds (near-sign steps
    amplify rounding over the epochs, an element moves by at most lr per epoch)."""
    epochs = 40
    p = biased_problem(77, 50, 35, 8, loss)
    ref = biased_oracle(p, SIDES[0], epochs, dtype=torch.float32)
    model = fit(tm, new_model(tm, p, SIDES[0]), p, epochs)
    h = model.loss_history_
    print(f'[trajectory] {loss}: first three {rel_err(h[:3], ref["loss"][:3]):.3g}, all {rel_err(h, ref["loss"]):.3g}')
    assert rel_err(h[:3], ref['loss'][:3]) < 1e-5 and rel_err(h, ref['loss']) < 1e-3
    assert np.abs(host(model.user_trainable[0]) - ref['user_vars'][0]).max() <= LR * epochs * 0.5
    assert np.abs(host(model.item_trainable[0]) - ref['item_vars'][0]).max() <= LR * epochs * 0.5
    pred = model.predict().cpu().numpy()
    assert np.array_equal(model.retrieve_user_recs(k=7), np.argsort(-pred, axis=1, kind='stable')[:, :7])


@pytest.mark.parametrize('sides', SIDES, ids=['-'.join(s) for s in SIDES])
@pytest.mark.parametrize('loss', LOSSES)
def test_graph_replay_equals_eager(tm, monkeypatch, loss, sides):
    p = biased_problem(21, 45, 30, 12, loss)
    monkeypatch.delenv('TMF_NO_GRAPH', raising=False)
    a = fit(tm, new_model(tm, p, sides), p, 8)
    monkeypatch.setenv('TMF_NO_GRAPH', '1')
    b = fit(tm, new_model(tm, p, sides), p, 8)
    assert a.loss_history_ == b.loss_history_ and len(a.loss_history_) == 8 and np.isfinite(a.loss_history_).all()
    for x, y in zip([a.user_embedding, a.item_embedding] + a.user_trainable + a.item_trainable,
                    [b.user_embedding, b.item_embedding] + b.user_trainable + b.item_trainable):
        assert torch.equal(x, y)


@pytest.mark.parametrize('loss', LOSSES)
def test_bias_is_carried_into_the_next_fit(tm, loss):
    """As in the reference, the bias stays on the model: a second engine fit re-initialises the weights and starts from the first
    fit's bias.  Its first loss is the unbiased loss on E = W0 + b (test_biased_cpu pins that closed form), and its first bias
    step starts at b."""
    p = biased_problem(31, 60, 40, 7, loss)
    model = fit(tm, new_model(tm, p, SIDES[0]), p, 3)
    bu, bv = host(model.user_linear_bias).astype(np.float64), host(model.item_linear_bias).astype(np.float64)
    assert np.abs(bu).min() > 0
    ref = biased_oracle(p, ('linear', 'linear'), 1, U0=p['U0'] + bu, V0=p['V0'] + bv)
    fit(tm, model, p, 1)
    assert rel_err(model.loss_history_[0], ref['loss'][0]) < 1e-5
    gU, gV = ref['first_grads'][0][0], ref['first_grads'][1][0]
    assert_step(host(model.user_trainable[0]), p['U0'], gU, LR, what=f'{loss} second fit U')
    assert_bias_step(host(model.user_linear_bias), bu, gU.sum(0), gU, LR, f'{loss} second fit user bias')
    if loss != 'wmrb':
        assert_bias_step(host(model.item_linear_bias), bv, gV.sum(0), gV, LR, f'{loss} second fit item bias')


def test_engine_fit_then_generic_fit(tm):
    """The bias an engine fit leaves is a leaf that requires grad: a later fit over dense non-identity features lands in
    _fit_generic, which differentiates with respect to it."""
    p = biased_problem(41, 40, 30, 6, 'mse')
    model = fit(tm, new_model(tm, p, SIDES[0]), p, 2)
    kept = model.user_linear_bias.detach().clone()
    rng = np.random.default_rng(0)
    Fu = torch.tensor((np.eye(40) + 0.05 * rng.random((40, 40))).astype(np.float32), device='cuda')
    fit(tm, model, p, 2, user_features=Fu)
    assert len(model.loss_history_) == 2 and np.isfinite(model.loss_history_).all()
    assert model.user_linear_bias.shape == (1, 6) and not torch.equal(model.user_linear_bias.detach(), kept)
    fit(tm, model, p, 2)                                   # and back on the engine, from the generic fit's bias
    assert np.isfinite(model.loss_history_).all()


# ------------------------------------------------------------------------------------------------------------------------
# dispatch
# ------------------------------------------------------------------------------------------------------------------------
def test_biased_fits_run_on_the_engine(tm, monkeypatch):
    """On the parent commit every one of these fits went through _fit_generic."""
    def refuse(self, *a, **k):
        raise AssertionError('_fit_generic was called')
    monkeypatch.setattr(tm.MF, '_fit_generic', refuse)
    for loss in LOSSES:
        p = biased_problem(51, 30, 20, 5, loss)
        for sides in SIDES:
            model = fit(tm, new_model(tm, p, sides), p, 2)
            assert hasattr(model, '_state') and len(model.loss_history_) == 2 and model.user_embedding.is_cuda
            assert (model._state.bias_u is not None) == (sides[0] == 'biased')
            assert (model._state.bias_v is not None) == (sides[1] == 'biased')


def test_everything_else_with_a_bias_stays_generic(tm, monkeypatch):
    from teamoflow_amd.mf.initializer_graphs import NormalInitializer
    calls = []
    monkeypatch.setattr(tm.MF, '_fit_generic', lambda self, *a, **k: calls.append(1))
    p = biased_problem(52, 30, 20, 5, 'mse')

    class Mine(tm.EG.BiasedLinearEmbedding):
        pass
    rng = np.random.default_rng(0)
    Fu = torch.tensor((np.eye(30) + 0.05 * rng.random((30, 30))).astype(np.float32), device='cuda')
    cases = [(dict(user_graph=Mine()), None), ({}, Fu), (dict(factor_dtype=torch.bfloat16), None), (dict(optimizer='adam'), None),
             (dict(batch_users=8), None),
             (dict(item_graph=tm.EG.ReLUEmbedding(), item_weight_graph=NormalInitializer()), None)]   # ReLU weights are [5 r, r]
    for i, (attrs, features) in enumerate(cases):
        fit(tm, new_model(tm, p, SIDES[0], **attrs), p, 1, user_features=features)
        assert len(calls) == i + 1, (i, attrs)


# ------------------------------------------------------------------------------------------------------------------------
# scale: no dense table anywhere
# ------------------------------------------------------------------------------------------------------------------------
def test_large_biased_fit_allocates_no_dense_table(tm):
    """100 000 users x 2 000 items, 1e6 interactions: the generic path would build eye(100 000) as a 40 GB matrix and 800 MB of
    scores; the engine fit stays below 2 GB."""
    m, n, r, per_user = 100_000, 2_000, 16, 10
    rng = np.random.default_rng(0)
    users = np.repeat(np.arange(m), per_user)
    items = (users * 7 + np.tile(np.arange(per_user), m) * 199) % n       # ten distinct items per user
    idx = np.stack([users, items], 1)
    val = rng.integers(1, 6, idx.shape[0]).astype(np.float32)
    p = dict(idx=idx, val=val, m=m, n=n, r=r, loss='mse', R=None, S=0,
             U0=(rng.standard_normal((m, r)) * 0.3).astype(np.float32), V0=(rng.standard_normal((n, r)) * 0.3).astype(np.float32))
    model = new_model(tm, p, SIDES[0])
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fit(tm, model, p, 3)
    peak = torch.cuda.max_memory_allocated()
    print(f'[scale] peak allocated {peak / 1e6:.0f} MB')
    assert peak < 2e9
    assert hasattr(model, '_state') and model.user_embedding.shape == (m, r)
    h = model.loss_history_
    assert len(h) == 3 and h[2] < h[1] < h[0]
