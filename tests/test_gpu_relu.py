"""ReLUEmbedding on the sparse HIP engine (csrc/tmf_relu.hip, _engine.ReLUSide / epoch_sides; opt-in through ``relu_engine``): the
four kernels through the C ABI against fp64 NumPy, and fits against oracle.dense_ref.fit_dense_plugins with 'relu' sides - the
reference loop on dense features and the dense [m, n] scores, fine at these sizes.  The problems are test_relu_cpu.relu_problem's;
that file also shows, on the reference alone, that the tolerances used here hold for the fp32 oracle itself, that the hidden units
of these problems sit far enough from the kink for fp32 and fp64 to agree on the mask, and why only MSE is followed for 40 epochs."""
import gc

import numpy as np
import pytest
import torch

from conftest import assert_step, rel_err, report_slack, step_bounds
from test_biased_cpu import LR
from test_features_cpu import UNUSED
from test_gpu_biased import guarded, guards_intact
from test_relu_cpu import BOTH, LAYOUTS, LOSSES, SIDE_IDS, SIDES, kink_margin, relu_features, relu_model, relu_oracle, relu_problem

pytestmark = pytest.mark.gpu
NAN = float('nan')
U = 2.0 ** -24


@pytest.fixture(scope='module')
def tm():
    from teamoflow_amd import _engine, _lib
    from teamoflow_amd.mf import embedding_graphs as EG
    from teamoflow_amd.mf import loss_graphs as LG
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseFeatures, SparseInteractions, eye
    lib = _lib.get()

    class NS:
        pass
    ns = NS()
    ns.lib, ns.L, ns.E, ns.MF, ns.EG, ns.LG, ns.SF, ns.Sparse, ns.eye = lib, _lib, _engine, MatrixFactorization, EG, LG, SparseFeatures, \
        SparseInteractions, eye
    return ns


def host(t):
    return t.detach().float().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------
# the kernels through the C ABI
# ------------------------------------------------------------------------------------------------------------------------
ROWS = (0, 1, 127, 128, 129, 300)
RANKS = (1, 3, 33, 128, 204)             # aux = 5 r: 5 .. 1020 (the widest row); K a multiple of neither 16 nor 4 among them
MODES = ('mix', 'off', 'on')


def kernel_case(tm, rows, r, mode, seed=0):
    """Operands of one (rows, r, hidden units) case: Z and b on a grid of 1/16 (fl(z + b) is then exact, so every non-zero
    |z + b| is at least 1/16 and the mask is the same in fp32 and fp64 - asserted), G and W ~ N(0, 1); the padding columns of
    every input hold NaN.  Host copies in fp32 beside the device tables (between NaN guard rows)."""
    aux = 5 * r
    rng = np.random.default_rng(1000 * rows + 10 * r + MODES.index(mode) + seed)
    ldz, ldw = tm.L.padded_ld(aux), tm.L.padded_ld(r)
    Z = (np.round(rng.standard_normal((rows, aux)) * 16) / 16).astype(np.float32)
    b = (np.round(rng.standard_normal(aux) * 16) / 16).astype(np.float32)
    if mode == 'off':
        Z, b = -np.abs(Z) - 1, -np.abs(b)
    elif mode == 'on':
        Z, b = np.abs(Z) + 1, np.abs(b)
    if mode == 'mix' and rows:
        Z[0, 0] = -b[0]                                                  # a unit exactly on the kink: off
    G = rng.standard_normal((rows, r)).astype(np.float32)
    W = rng.standard_normal((aux, r)).astype(np.float32)
    s = Z + b[None, :]                                                   # fp32: the kernels' fl(z + b)
    nz = s != 0
    assert (np.abs(s[nz]) > 10 * U * (np.abs(Z) + np.abs(b)[None, :])[nz]).all()   # 10 x the bound of the one addition
    assert np.array_equal(s.astype(np.float64), Z.astype(np.float64) + b.astype(np.float64)[None, :])
    on = s > 0
    if mode == 'mix' and rows >= 127:
        assert on.any() and (~on).any() and s[0, 0] == 0
    assert mode != 'off' or not on.any()
    assert mode != 'on' or on.all()
    c = dict(rows=rows, r=r, aux=aux, ldz=ldz, ldw=ldw, Z=Z, b=b, G=G, W=W, on=on, H=np.maximum(s, 0).astype(np.float64))

    def table(x, n_rows, width, ld):
        t = torch.full((n_rows, ld), NAN, dtype=torch.float32)
        t[:, :width] = torch.from_numpy(np.ascontiguousarray(x).reshape(n_rows, width))
        return guarded(n_rows, ld, torch.float32, NAN, t.cuda())
    c['tZ'], c['tZ_buf'] = table(Z, rows, aux, ldz)
    c['tb'], c['tb_buf'] = table(b, 1, aux, ldz)
    c['tG'], c['tG_buf'] = table(G, rows, r, ldw)
    c['tW'], c['tW_buf'] = table(W, aux, r, ldw)
    return c


@pytest.fixture(scope='module')
def cases(tm):
    cache = {}

    def get(rows, r, mode):
        if (rows, r, mode) not in cache:
            cache[rows, r, mode] = kernel_case(tm, rows, r, mode)
        return cache[rows, r, mode]
    return get


def inputs_untouched(c):
    for name, width in (('Z', c['aux']), ('b', c['aux']), ('G', c['r']), ('W', c['r'])):
        t = c['t' + name]
        if not np.array_equal(host(t[:, :width]).reshape(c[name].shape), c[name]) or not bool(torch.isnan(t[:, width:]).all()):
            return False
        if not guards_intact(c['t' + name + '_buf'], NAN):
            return False
    return True


def run_embed(tm, c):
    P = tm.L.ptr
    E, E_buf = guarded(c['rows'], c['ldw'], torch.float32, NAN)
    tm.L.check(tm.lib.tmf_relu_embed_f32(P(c['tZ']), P(c['tb']), P(c['tW']), P(E), c['rows'], c['aux'], c['r'], tm.L.stream_ptr()), tm.lib)
    torch.cuda.synchronize()
    assert guards_intact(E_buf, NAN)
    return E


def run_dhidden(tm, c):
    P = tm.L.ptr
    dZ, dZ_buf = guarded(c['rows'], c['ldz'], torch.float32, NAN)
    tm.L.check(tm.lib.tmf_relu_dhidden_f32(P(c['tG']), P(c['tW']), P(c['tZ']), P(c['tb']), P(dZ), c['rows'], c['aux'], c['r'],
                                           tm.L.stream_ptr()), tm.lib)
    torch.cuda.synchronize()
    assert guards_intact(dZ_buf, NAN)
    return dZ


def run_dweights(tm, c):
    """-> (part [P, aux, ldw], P)"""
    P = tm.L.ptr
    n_parts = int(tm.lib.tmf_relu_part_rows(c['rows']))
    part, part_buf = guarded(n_parts * c['aux'], c['ldw'], torch.float32, NAN)
    tm.L.check(tm.lib.tmf_relu_dweights_f32(P(c['tZ']), P(c['tb']), P(c['tG']), P(part), n_parts, c['rows'], c['aux'], c['r'],
                                            tm.L.stream_ptr()), tm.lib)
    torch.cuda.synchronize()
    assert guards_intact(part_buf, NAN)
    return part.view(n_parts, c['aux'], c['ldw']), n_parts


def within(got, ref, mag, K, what):
    """|got - ref| <= (K + 2) 2^-24 mag elementwise: the worst case of any fp32 summation order of K rounded products."""
    err, bound = np.abs(got.astype(np.float64) - ref), (K + 2) * U * mag
    print(f'[relu kernel] {what}: worst {float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0:.3g} of the bound')
    assert (err <= bound).all(), what


@pytest.mark.parametrize('r', RANKS)
@pytest.mark.parametrize('rows', ROWS)
def test_embed_against_numpy(tm, cases, rows, r):
    for mode in MODES:
        c = cases(rows, r, mode)
        E = run_embed(tm, c)
        W = c['W'].astype(np.float64)
        within(host(E[:, :r]), c['H'] @ W, c['H'] @ np.abs(W), c['aux'], f'embed rows={rows} r={r} {mode}')
        assert E.shape == (rows, c['ldw']) and not E[:, r:].any()            # padding columns are exactly 0, whatever W holds there
        if mode == 'off':
            assert not E.any()
        assert inputs_untouched(c)
        assert torch.equal(E, run_embed(tm, c))


@pytest.mark.parametrize('r', RANKS)
@pytest.mark.parametrize('rows', ROWS)
def test_dhidden_against_numpy(tm, cases, rows, r):
    for mode in MODES:
        c = cases(rows, r, mode)
        dZ = run_dhidden(tm, c)
        G, W, aux = c['G'].astype(np.float64), c['W'].astype(np.float64), c['aux']
        got = host(dZ[:, :aux])
        within(got, (G @ W.T) * c['on'], np.abs(G) @ np.abs(W).T * c['on'], r, f'dhidden rows={rows} r={r} {mode}')
        assert (got[~c['on']] == 0).all()                                    # exactly 0 where the unit is off
        assert dZ.shape == (rows, c['ldz']) and not dZ[:, aux:].any()        # the list pass gathers whole rows of it
        if mode == 'on' and rows:
            assert np.count_nonzero(got) == got.size
        assert inputs_untouched(c)
        assert torch.equal(dZ, run_dhidden(tm, c))


def part_edge(tm):
    """The largest row count of a single part (tmf_relu_part_rows' block size for small tables)."""
    return next(n for n in range(1, 100000) if tm.lib.tmf_relu_part_rows(n) == 2) - 1


def check_weights_step(tm, c, what):
    L, lib, P, s = tm.L, tm.lib, tm.L.ptr, tm.L.stream_ptr()
    rows, r, aux, ldw = c['rows'], c['r'], c['aux'], c['ldw']
    part, n_parts = run_dweights(tm, c)
    H, G = c['H'], c['G'].astype(np.float64)
    edge = part_edge(tm)
    assert n_parts == -(-rows // edge)
    for p in range(n_parts):                                                 # every part against its block of rows
        blk = slice(p * edge, min((p + 1) * edge, rows))
        within(host(part[p, :, :r]), H[blk].T @ G[blk], np.abs(H[blk]).T @ np.abs(G[blk]), blk.stop - blk.start, f'{what} part {p}')
    assert not part[:, :, r:].any()
    again, _ = run_dweights(tm, c)
    assert torch.equal(part, again)
    # the step: g = sum of the parts in order, W_out = fresh_adam(W_old, g); W_old is only read, its padding holds NaN
    adam = tm.E.adam_constants(LR)
    outs = []
    for _ in range(2):
        W_out, W_buf = guarded(aux, ldw, torch.float32, NAN)
        g_out, g_buf = guarded(aux, ldw, torch.float32, NAN)
        L.check(lib.tmf_relu_adam_weights_f32(P(part) if n_parts else None, n_parts, P(c['tW']), P(W_out), P(g_out), aux, r, adam, s), lib)
        torch.cuda.synchronize()
        assert guards_intact(W_buf, NAN) and guards_intact(g_buf, NAN)
        outs.append((W_out, g_out))
    (W_out, g_out), (W_2, g_2) = outs
    assert torch.equal(W_out, W_2) and torch.equal(g_out, g_2)
    within(host(g_out[:, :r]), H.T @ G, np.abs(H).T @ np.abs(G), rows, f'{what} sum')
    assert not g_out[:, r:].any() and not W_out[:, r:].any()
    want = torch.zeros(aux, ldw, device='cuda')
    want[:, :r] = torch.from_numpy(c['W']).cuda()
    L.check(lib.tmf_adam_fresh_rows_f32(P(want), P(g_out.contiguous()), aux, r, adam, s), lib)
    no_g, _ = guarded(aux, ldw, torch.float32, NAN)                          # g_out = NULL: the same step
    L.check(lib.tmf_relu_adam_weights_f32(P(part) if n_parts else None, n_parts, P(c['tW']), P(no_g), None, aux, r, adam, s), lib)
    torch.cuda.synchronize()
    assert torch.equal(W_out, want) and torch.equal(no_g, W_out)
    if rows == 0 or not c['on'].any():                                       # no rows, or no unit on: W_out = W_old
        assert not g_out.any() and np.array_equal(host(W_out[:, :r]), c['W'])
    assert inputs_untouched(c)


@pytest.mark.parametrize('r', RANKS)
@pytest.mark.parametrize('rows', ROWS)
def test_dweights_and_the_weights_step_against_numpy(tm, cases, rows, r):
    for mode in MODES:
        check_weights_step(tm, cases(rows, r, mode), f'dweights rows={rows} r={r} {mode}')


@pytest.mark.parametrize('r', [3, 33])
@pytest.mark.parametrize('offset', [-1, 0, 1, 'three parts'])
def test_dweights_around_a_part_boundary(tm, offset, r):
    edge = part_edge(tm)
    rows = 2 * edge + 5 if offset == 'three parts' else edge + offset
    c = kernel_case(tm, rows, r, 'mix', seed=7)
    assert int(tm.lib.tmf_relu_part_rows(rows)) == {-1: 1, 0: 1, 1: 2, 'three parts': 3}[offset]
    check_weights_step(tm, c, f'dweights rows={rows} r={r}')


# ------------------------------------------------------------------------------------------------------------------------
# fits
# ------------------------------------------------------------------------------------------------------------------------
def fit(tm, model, p, relu, epochs, lr=LR):
    uf, vf = relu_features(p, relu)
    model.fit(epochs, uf, vf, tm.Sparse(p['idx'], p['val'], (p['m'], p['n'])), lr=lr)
    return model


def forward64(F, Wr, b, W):
    """fp64 (Z, H, E) of one ReLU side."""
    Z = np.asarray(F, np.float64) @ np.asarray(Wr, np.float64)
    H = np.maximum(Z + np.asarray(b, np.float64).reshape(1, -1), 0)
    return Z, H, H @ np.asarray(W, np.float64)


def embedding_gradients(p, relu, loss_fn=None):
    """fp64 dL/dE of the first epoch for both sides: the oracle over identity features started from the effective tables
    E0 = relu(F relu_w0) W0 of the ReLU sides."""
    from oracle import dense_ref as D
    E0 = [forward64(p['relu_F' + s + '_dense'], p['relu_Wr' + s], 0.0, p['relu_W' + s])[2] if name in relu else p[t0]
          for s, name, t0 in (('u', 'user', 'U0'), ('v', 'item', 'V0'))]
    if loss_fn is not None:
        return loss_fn(E0[0], E0[1])
    ref = D.fit_dense_plugins(E0[0], E0[1], p['idx'], p['val'], p['loss'], 1, LR, np.eye(p['m']), np.eye(p['n']), random_ind=p['R'],
                              n_items=p['n'], n_samples=p['S'], dtype=torch.float64)
    return ref['first_grads'][0][0], ref['first_grads'][1][0]


def assert_step_with_slack(W_new, W0, g_ref, slack, lr, what):
    """assert_step with a per-element slack on the gradient; at most 1 % of the elements may need it (the fp32 reference needs
    none, test_relu_cpu); logs how many did and the largest share of the slack they used."""
    W_new, W0, g_ref = (np.asarray(x, np.float64) for x in (W_new, W0, g_ref))
    assert W_new.shape == W0.shape == g_ref.shape, what

    def outside(t):
        lo, hi = step_bounds(W0, g_ref, lr, 1e-5, t * slack)
        return (W_new < lo) | (W_new > hi)
    need = outside(0.0)
    lo_t, hi_t = np.zeros_like(W_new), np.ones_like(W_new)
    for _ in range(30):
        mid = 0.5 * (lo_t + hi_t)
        out = outside(mid)
        lo_t, hi_t = np.where(out, mid, lo_t), np.where(out, hi_t, mid)
    report_slack(check=what, n_elements=int(W_new.size), n_needed_slack=int(need.sum()),
                 max_consumed=float(hi_t[need].max()) if need.any() else 0.0)
    assert_step(W_new, W0, g_ref, lr, rtol=1e-5, what=what, slack=slack)
    assert need.sum() <= 0.01 * W_new.size, f'{what}: {int(need.sum())} of {W_new.size} elements needed the slack'


def check_relu_side(tm, p, s, name, rows, r, model, grads, G_ref, what):
    """One ReLU side after one step from (W0, relu_w0, 0): the three variables inside their step intervals, what the fit leaves
    on the model, and the embedding against the variables it left."""
    aux = 5 * r
    trainable = (model.user_trainable, model.item_trainable)[name == 'item']
    emb = (model.user_embedding, model.item_embedding)[name == 'item']
    kept_w, kept_b = ((model.user_relu_weight, model.user_relu_bias), (model.item_relu_weight, model.item_relu_bias))[name == 'item']
    F, W0, Wr0 = p['relu_F' + s + '_dense'], p['relu_W' + s], p['relu_Wr' + s]
    assert [tuple(t.shape) for t in trainable] == [(aux, r), (F.shape[1], aux), (1, aux)], what
    assert emb.is_cuda and emb.shape == (rows, r) and all(t.is_cuda for t in trainable)
    assert kept_w is trainable[1] and kept_b is trainable[2] and kept_w.requires_grad and kept_b.requires_grad
    assert kept_w.is_leaf and kept_b.is_leaf
    # a 1e-5 error of every row of G = dL/dE, pushed through dW = H^T G, dZ = (G W^T) . mask, db = colsum(dZ), dWr = F^T dZ
    Z0, H0, _ = forward64(F, Wr0, 0.0, W0)
    smallest, bound, ratio = kink_margin(F, Wr0)
    assert ratio > 10, f'{what}: a pre-activation within 10 x its summation bound of the kink ({smallest:.3g}, {bound:.3g})'
    aG = np.abs(G_ref)
    dZ_slack = 1e-5 * (aG @ np.abs(W0.astype(np.float64)).T) * (Z0 > 0)
    slacks = (1e-5 * np.abs(H0).T @ aG, np.abs(F).T @ dZ_slack, dZ_slack.sum(0, keepdims=True))
    starts = (W0, Wr0, np.zeros((1, aux)))
    for var, got, w0, g, slack in zip(('W', 'relu_weight', 'relu_bias'), trainable, starts, grads, slacks):
        assert_step_with_slack(host(got), w0, g, slack, LR, f'{what} {name} {var}')
    if p['relu_layout'] != 'eye':
        off = rows if p['relu_layout'] == 'hybrid' else 0
        assert np.array_equal(host(kept_w)[off + UNUSED], Wr0[off + UNUSED]), f'{what} {name}: a feature no row carries moved'
        embed = (model.embed_users, model.embed_items)[name == 'item']
        assert torch.equal(emb, embed(tm.SF(*p['F' + s]))), f'{what} {name}: embedding != embed(F)'
    # the embedding against relu(F Wr + b) W in fp64 from the variables the fit left: the pre-activation within its product bound
    # (n_i + 2) u sum |x w|, one more rounding for the addition of b - the ReLU passes that error on at most unchanged -, then
    # the product bound (aux + 2) u sum h |w| of the second product on top of the error it inherits
    W1, Wr1, b1 = (host(t).astype(np.float64) for t in trainable)
    Z1, H1, E1 = forward64(F, Wr1, b1, W1)
    dH = ((F != 0).sum(1, keepdims=True) + 2) * U * (np.abs(F) @ np.abs(Wr1)) + U * (np.abs(Z1) + np.abs(b1))
    bound = dH @ np.abs(W1) + (aux + 2) * U * ((H1 + dH) @ np.abs(W1))
    assert (np.abs(host(emb).astype(np.float64) - E1) <= bound).all(), f'{what} {name}: embedding != relu(F Wr + b) W'


ONE_STEP = [(loss, r) for loss in LOSSES for r in (3, 33, 128)]


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('relu', SIDES, ids=SIDE_IDS)
@pytest.mark.parametrize('loss,r', ONE_STEP)
def test_one_step(tm, loss, r, relu, layout):
    m, n = 60, 40
    p = relu_problem(3000 + r, m, n, r, loss, layout)
    ref = relu_oracle(p, relu, 1)
    G = embedding_gradients(p, relu)
    model = fit(tm, relu_model(p, relu), p, relu, 1)
    what = f'{loss} r={r} {"+".join(relu)} {layout}'
    assert hasattr(model, '_state'), 'the fit did not run on the engine'
    assert rel_err(model.loss_history_[0], ref['loss'][0]) < 1e-5, what
    for s, name, rows, grads, G_ref in (('u', 'user', m, ref['first_grads'][0], G[0]), ('v', 'item', n, ref['first_grads'][1], G[1])):
        if name in relu:
            check_relu_side(tm, p, s, name, rows, r, model, grads, G_ref, what)
        else:
            got, emb = (model.user_trainable, model.user_embedding) if name == 'user' else (model.item_trainable, model.item_embedding)
            assert len(got) == 1 and torch.equal(emb, got[0])
            assert_step(host(got[0]), p[s.upper() + '0'], grads[0], LR, what=f'{what} {name} table')


def logistic_autograd(p, relu, weighted):
    """LogisticLoss restated in float64 torch: -> (loss sum, gradients of the variables of both sides, dL/dE of both sides)."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)   # noqa: E731
    idx, val = torch.tensor(p['idx']), torch.tensor(p['val'].astype(np.float64))
    sides = []
    for s, name, t0 in (('u', 'user', 'U0'), ('v', 'item', 'V0')):
        if name in relu:
            vs = [t(p['relu_W' + s]), t(p['relu_Wr' + s]), t(np.zeros((1, 5 * p['r'])))]
            E = torch.relu(torch.tensor(p['relu_F' + s + '_dense']) @ vs[1] + vs[2]) @ vs[0]
        else:
            vs = [t(p[t0])]
            E = vs[0] * 1.0
        E.retain_grad()
        sides.append((vs, E))
    (uv, Eu), (iv, Ev) = sides
    score = (Eu[idx[:, 0]] * Ev[idx[:, 1]]).sum(1)
    y = torch.where(val > 0, 1.0, -1.0).to(torch.float64)
    w = val.abs() if weighted else torch.ones_like(val)
    loss = (w * torch.nn.functional.softplus(-y * score)).sum()
    loss.backward()
    return float(loss), [v.grad.numpy() for v in uv], [v.grad.numpy() for v in iv], (Eu.grad.numpy(), Ev.grad.numpy())


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('relu', SIDES, ids=SIDE_IDS)
def test_one_step_logistic(tm, relu, layout, weighted):
    m, n, r = 60, 40, 33
    p = relu_problem(3000 + r, m, n, r, 'kl', layout)                        # signed values: both classes
    p['loss'] = 'logistic'
    loss, gu, gv, G = logistic_autograd(p, relu, weighted)
    model = fit(tm, relu_model(p, relu, loss_graph=tm.LG.LogisticLoss(weighted=weighted)), p, relu, 1)
    what = f'logistic weighted={weighted} {"+".join(relu)} {layout}'
    assert hasattr(model, '_state') and rel_err(model.loss_history_[0], loss / len(p['val'])) < 1e-5, what
    for s, name, rows, grads, G_ref in (('u', 'user', m, gu, G[0]), ('v', 'item', n, gv, G[1])):
        if name in relu:
            check_relu_side(tm, p, s, name, rows, r, model, grads, G_ref, what)
        else:
            got = model.user_trainable if name == 'user' else model.item_trainable
            assert_step(host(got[0]), p[s.upper() + '0'], grads[0], LR, what=f'{what} {name} table')


@pytest.mark.parametrize('loss', LOSSES)
def test_trajectory(tm, loss):
    """Both sides hybrid ReLU against the fp32 oracle: 3 epochs to 1e-5 and 10 to 1e-3 for every loss, 40 to 1e-3 for MSE only
    (test_relu_cpu: beyond that the reference's own fp32 and fp64 runs drift apart for WMRB and KL)."""
    epochs = 40 if loss == 'mse' else 10
    p = relu_problem(77, 50, 35, 8, loss, 'hybrid', item_everywhere=False)
    ref = relu_oracle(p, BOTH, epochs, dtype=torch.float32)
    model = fit(tm, relu_model(p, BOTH), p, BOTH, epochs)
    h = model.loss_history_
    first, ten, whole = rel_err(h[:3], ref['loss'][:3]), rel_err(h[:10], ref['loss'][:10]), rel_err(h, ref['loss'])
    print(f'[relu trajectory] {loss}: 3 epochs {first:.3g}, 10 epochs {ten:.3g}, {epochs} epochs {whole:.3g}')
    assert hasattr(model, '_state') and len(h) == epochs
    assert first < 1e-5 and ten < 1e-3 and whole < 1e-3
    pred = model.predict().cpu().numpy()
    assert np.array_equal(model.retrieve_user_recs(k=7), np.argsort(-pred, axis=1, kind='stable')[:, :7])


def everything(model):
    return [model.user_embedding, model.item_embedding] + model.user_trainable + model.item_trainable


@pytest.mark.parametrize('relu', SIDES, ids=SIDE_IDS)
@pytest.mark.parametrize('loss', LOSSES)
def test_graph_replay_equals_eager_and_fits_repeat(tm, monkeypatch, loss, relu):
    p = relu_problem(21, 45, 30, 12, loss, 'hybrid')
    monkeypatch.delenv('TMF_NO_GRAPH', raising=False)
    a = fit(tm, relu_model(p, relu), p, relu, 8)
    monkeypatch.setenv('TMF_NO_GRAPH', '1')
    b = fit(tm, relu_model(p, relu), p, relu, 8)
    c = fit(tm, relu_model(p, relu), p, relu, 8)
    assert len(a.loss_history_) == 8 and np.isfinite(a.loss_history_).all() and hasattr(a, '_state')
    for other in (b, c):   # graph against eager, eager against eager
        assert a.loss_history_ == other.loss_history_
        assert all(torch.equal(x, y) for x, y in zip(everything(a), everything(other)))


# ------------------------------------------------------------------------------------------------------------------------
# dispatch
# ------------------------------------------------------------------------------------------------------------------------
def test_relu_fits_run_on_the_engine(tm, monkeypatch):
    """Every combination of test_one_step with _fit_generic refusing to run.  Without the engine form of a ReLU side every one of
    these fits calls it."""
    def refuse(self, *a, **k):
        raise AssertionError('_fit_generic was called')
    monkeypatch.setattr(tm.MF, '_fit_generic', refuse)
    for loss, r in ONE_STEP:
        for layout in LAYOUTS:
            p = relu_problem(51, 30, 20, r, loss, layout)
            for relu in SIDES:
                model = fit(tm, relu_model(p, relu), p, relu, 2)
                assert hasattr(model, '_state') and len(model.loss_history_) == 2 and model.user_embedding.is_cuda
                assert (model._state.relu_u is not None) == ('user' in relu) and (model._state.relu_v is not None) == ('item' in relu)
                assert model._state.feat_u is None and model._state.feat_v is None
                assert len(model.user_trainable) == (3 if 'user' in relu else 1)
                assert len(model.item_trainable) == (3 if 'item' in relu else 1)


def test_a_relu_side_beside_a_featured_and_a_biased_side(tm, monkeypatch):
    """The other engine sides keep their own steps beside a ReLU side: the state holds both kinds and the fit lowers the loss."""
    monkeypatch.setattr(tm.MF, '_fit_generic', lambda self, *a, **k: pytest.fail('_fit_generic was called'))
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    p = relu_problem(55, 30, 20, 5, 'mse', 'hybrid')
    inter = tm.Sparse(p['idx'], p['val'], (30, 20))
    a = relu_model(p, ('user',), item_weight_graph=FixedInitializer(p['Wv0']))            # item side: LinearEmbedding over [I | tags]
    a.fit(4, tm.SF(*p['Fu']), tm.SF(*p['Fv']), inter, lr=LR)
    assert a._state.relu_u is not None and a._state.feat_v is not None and a.item_trainable[0].shape == p['Wv0'].shape
    b = relu_model(p, ('item',), user_repr_graph=tm.EG.BiasedLinearEmbedding())
    b.fit(4, tm.eye(30), tm.SF(*p['Fv']), inter, lr=LR)
    assert b._state.relu_v is not None and b._state.bias_u is not None and b.user_linear_bias.shape == (1, 5)
    for model in (a, b):
        h = model.loss_history_
        assert np.isfinite(h).all() and h[3] < h[0]


def test_everything_else_stays_generic(tm, monkeypatch):
    """Each setting the engine has no ReLU form for calls _fit_generic exactly once although relu_engine is set - and so does the
    default, relu_engine = False."""
    calls = []
    monkeypatch.setattr(tm.MF, '_fit_generic', lambda self, epochs, uf, vf, *a, **k: calls.append((uf, vf)))
    p = relu_problem(52, 30, 20, 5, 'mse', 'hybrid')

    class Mine(tm.EG.ReLUEmbedding):
        pass

    class MyLoss(tm.LG.MSELoss):
        pass
    Fu = tm.SF(*p['Fu'])
    none = tm.SF(np.zeros((0, 2)), np.zeros(0), Fu.shape)
    cases = [dict(relu_engine=False), dict(user_repr_graph=Mine()), dict(loss_graph=MyLoss()), dict(factor_dtype=torch.bfloat16),
             dict(optimizer='adam'), dict(batch_users=8), dict(shard_items=2), dict(data_parallel='force'),
             dict(features=Fu.to_dense()), dict(features=none)]
    for i, attrs in enumerate(cases):
        graphs = {k: attrs.pop(k) for k in list(attrs) if k.endswith('_graph')}
        uf = attrs.pop('features', Fu)
        model = relu_model(p, ('user',), **graphs)
        for k, v in attrs.items():
            setattr(model, k, v)
        model.fit(1, uf, tm.eye(p['n']), tm.Sparse(p['idx'], p['val'], (p['m'], p['n'])), lr=LR)
        assert len(calls) == i + 1, (i, graphs, attrs)
        assert torch.is_tensor(calls[-1][0]) and not calls[-1][0].is_sparse           # SparseFeatures arrive as their dense form
    # an aux width beyond a table row: 5 r > 1024
    from teamoflow_amd.mf.initializer_graphs import NormalInitializer
    wide = tm.MF(205, user_repr_graph=tm.EG.ReLUEmbedding(), user_weight_graph=NormalInitializer(), item_weight_graph=NormalInitializer())
    wide.relu_engine, wide.verbose = True, False
    wide.fit(1, tm.eye(p['m']), tm.eye(p['n']), tm.Sparse(p['idx'], p['val'], (p['m'], p['n'])), lr=LR)
    assert len(calls) == len(cases) + 1


def test_span_names_of_a_relu_epoch(tm):
    """The KernelTimer spans tools/time_relu_c4.py reads, as an exact set."""
    p = relu_problem(54, 30, 20, 16, 'mse', 'hybrid')
    dev = torch.device('cuda')
    plan = tm.E.InteractionPlan(torch.tensor(p['idx'], device=dev), torch.tensor(p['val'], device=dev), 30, 20, csc=True)
    adam, loss = tm.E.adam_constants(LR), torch.zeros(1, dtype=torch.float64, device=dev)
    names = ('relu_dweights', 'relu_dhidden', 'relu_adam_weights', 'relu_bias_colsum', 'relu_bias_adam', 'relu_feat_backward',
             'relu_feat_forward', 'relu_embed')
    user = dict(F=tm.SF(*p['Fu']), Wr0=p['relu_Wru'], b0=np.zeros(80, np.float32))
    item = dict(F=None, Wr0=np.eye(20, 80, dtype=np.float32), b0=np.zeros(80, np.float32))   # indicator features: the identity lists
    for kw, want in ((dict(user_relu=user, item_relu=item), {side + x for side in ('user_', 'item_') for x in names}),
                     (dict(item_relu=item, user_bias=torch.zeros(16)),
                      {'item_' + x for x in names} | {'user_bias_colsum', 'user_bias_adam', 'user_adam_bias_rows'})):
        st = tm.E.TrainState(p['relu_Wu'] if 'user_relu' in kw else p['U0'], p['relu_Wv'], plan, 16, **kw)
        prof = tm.E.KernelTimer()
        tm.E.epoch_sides(st, adam, loss, 'mse', prof=prof)
        torch.cuda.synchronize()
        assert set(prof.spans) == want | {'mse_user_pass', 'mse_item_pass'}
        assert all(b is not None for spans in prof.spans.values() for _, b in spans) and float(loss) > 0


def test_a_second_fit_starts_from_the_kept_hidden_variables(tm):
    """fit() re-initialises the output weights and continues from relu_weight / relu_bias, as the reference does (:115-146): the
    second fit of a model is the first fit of a fresh model given what the first one kept."""
    p = relu_problem(56, 30, 20, 5, 'mse', 'hybrid')
    a = fit(tm, relu_model(p, BOTH), p, BOTH, 2)
    kept = [t.detach().clone() for t in (a.user_relu_weight, a.user_relu_bias, a.item_relu_weight, a.item_relu_bias)]
    first = [t.detach().clone() for t in everything(a)]
    assert not torch.equal(kept[0], torch.tensor(p['relu_Wru'], device='cuda')) and bool(kept[1].any())
    fit(tm, a, p, BOTH, 2)
    b = relu_model(p, BOTH)
    b.user_relu_weight, b.user_relu_bias, b.item_relu_weight, b.item_relu_bias = kept
    fit(tm, b, p, BOTH, 2)
    assert a.loss_history_ == b.loss_history_ and all(torch.equal(x, y) for x, y in zip(everything(a), everything(b)))
    assert not torch.equal(everything(a)[0], first[0])                         # and not the first fit over again
    with pytest.raises(ValueError, match='relu_weight'):                       # kept variables of another shape
        c = relu_model(p, BOTH)
        c.user_relu_weight = kept[0][:, :7]
        fit(tm, c, p, BOTH, 1)


def test_large_relu_fit_allocates_no_dense_table(tm):
    """100 000 users x 2 000 items, 1e6 interactions, a ReLU user side over eye(): the generic path would multiply a 40 GB identity
    and differentiate through 800 MB of scores; the engine fit stays below 2 GB.  The loss falls over the fit, not epoch by epoch:
    from hidden weights ~ N(0, 1), as get_repr draws them, the first sign-like Adam steps of all 80 units of a row add up."""
    m, n, r, per_user = 100_000, 2_000, 16, 10
    rng = np.random.default_rng(0)
    users = np.repeat(np.arange(m), per_user)
    items = (users * 7 + np.tile(np.arange(per_user), m) * 199) % n       # ten distinct items per user
    idx = np.stack([users, items], 1)
    val = rng.integers(1, 6, idx.shape[0]).astype(np.float32)
    model = tm.MF(r, user_repr_graph=tm.EG.ReLUEmbedding())
    model.relu_engine, model.verbose = True, False
    torch.manual_seed(0)
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    model.fit(3, tm.eye(m), tm.eye(n), tm.Sparse(idx, val, (m, n)), lr=LR)
    peak = torch.cuda.max_memory_allocated()
    h = model.loss_history_
    print(f'[relu scale] peak allocated {peak / 1e6:.0f} MB, loss {h}')
    assert peak < 2e9
    assert hasattr(model, '_state') and model.user_embedding.shape == (m, r)
    assert [tuple(t.shape) for t in model.user_trainable] == [(5 * r, r), (m, 5 * r), (1, 5 * r)]
    assert len(h) == 3 and np.isfinite(h).all() and h[2] < h[0]
