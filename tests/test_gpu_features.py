"""LinearEmbedding over SparseFeatures on the sparse HIP engine (tmf_feat_pass_f32, _engine.FeatureSide / epoch_sides) against
NumPy through the C ABI and against oracle.dense_ref.fit_dense_plugins over F.to_dense() - the reference loop on dense features
and the dense [m, n] scores, fine at these sizes.  The problems are test_features_cpu.featured_problem's; that file also shows,
on the reference alone, that the tolerances used here hold for the fp32 oracle itself, why whole trajectories use the hybrid
layout only and why no trajectory problem has an everywhere-feature on the item side."""
import gc

import numpy as np
import pytest
import torch

from conftest import assert_step, rel_err, report_slack, step_bounds
from test_biased_cpu import LR
from test_features_cpu import BOTH, LAYOUTS, LOSSES, UNUSED, _model, featured_oracle, featured_problem
from test_gpu_biased import guarded, guards_intact, host, random_table

pytestmark = pytest.mark.gpu
NAN = float('nan')
SIDES = (('user',), ('item',), BOTH)
SIDE_IDS = ['user', 'item', 'both']


@pytest.fixture(scope='module')
def tm():
    from teamoflow_amd import _engine, _lib
    from teamoflow_amd.mf import embedding_graphs as EG
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseFeatures, SparseInteractions, eye, hstack_identity
    lib = _lib.get()

    class NS:
        pass
    ns = NS()
    ns.lib, ns.L, ns.E, ns.MF, ns.EG, ns.SF, ns.Sparse, ns.eye, ns.hstack = lib, _lib, _engine, MatrixFactorization, EG, SparseFeatures, \
        SparseInteractions, eye, hstack_identity
    return ns


# ------------------------------------------------------------------------------------------------------------------------
# the kernel through the C ABI
# ------------------------------------------------------------------------------------------------------------------------
LISTS = ('no rows', 'one entry', 'short rows', 'long row', 'chunk 4')


def make_lists(kind, seed, n_table):
    """(lens per list row, chunk) of the list shapes the kernel can go wrong on, then ids in [0, n_table) and values (explicit
    zeros among them) -> (lens, ids int32, vals fp32, chunk)."""
    rng = np.random.default_rng(seed)
    chunk = 1024
    if kind == 'no rows':
        lens = np.zeros(0, np.int64)
    elif kind == 'one entry':
        lens = np.array([1])
    elif kind == 'short rows':
        lens = rng.integers(0, 6, 65)
        lens[7] = 0                                 # an empty list
    elif kind == 'long row':
        lens = rng.integers(0, 6, 1000)
        lens[0], lens[500] = 0, 2 * chunk + 7       # three segments: slab slots and tmf_combine_rows_f32
    else:
        chunk = 4
        lens = rng.integers(0, 14, 65)              # up to four segments per row
        lens[3], lens[64] = 0, 13
    nnz = int(lens.sum())
    ids = rng.integers(0, n_table, nnz).astype(np.int32)
    vals = rng.choice(np.array([1.0, 0.5, -0.25, 2.0, 0.0, -1.5], np.float32), nnz)
    return lens, ids, vals, chunk


def run_feat(tm, seg, ids, vals, T, r, epi, X_old=None):
    """One tmf_feat_pass_f32 + the combine of its multi-segment rows into fresh guarded buffers -> X_out (a view between NaN guard
    rows, checked)."""
    L, lib, P, s = tm.L, tm.lib, tm.L.ptr, tm.L.stream_ptr()
    ld = L.padded_ld(r)
    adam = tm.E.adam_constants(LR)
    out, out_buf = guarded(seg.rows, ld, torch.float32, NAN)
    slab, slab_buf = guarded(max(seg.n_slab, 1), ld, torch.float32, NAN)
    L.check(lib.tmf_feat_pass_f32(seg.cstruct(), P(ids), P(vals), P(T), P(X_old), P(out), P(slab), r, epi, adam, s), lib)
    tm.E._row_pass_finish(lib, seg, slab, X_old, out, r, epi, adam, s)
    torch.cuda.synchronize()
    assert guards_intact(out_buf, NAN) and guards_intact(slab_buf, NAN)
    return out


def product_bound(lens, ids, vals, Th):
    """(fp64 sums [rows, r], elementwise bound): (n_i + 2) 2^-24 sum_k |val_k T[id_k]| - the worst case of any fp32 summation order of
    n_i rounded products."""
    rows = np.repeat(np.arange(lens.size), lens)
    terms = vals.astype(np.float64)[:, None] * Th[ids]
    ref, mag = np.zeros((lens.size, Th.shape[1])), np.zeros((lens.size, Th.shape[1]))
    np.add.at(ref, rows, terms)
    np.add.at(mag, rows, np.abs(terms))
    return ref, (lens[:, None] + 2) * 2.0 ** -24 * mag


@pytest.fixture(scope='module')
def feat_cases(tm):
    """The operands of a (lists, r) case, built once and shared by the GRAD and the ADAM test: they are only read."""
    cache = {}

    def get(kind, r):
        if (kind, r) not in cache:
            n_table, ld = 50, tm.L.padded_ld(r)
            lens, ids, vals, chunk = make_lists(kind, 100 * LISTS.index(kind) + r, n_table)
            rowptr = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device='cuda')
            seg = tm.E.SegmentTable(rowptr, chunk)
            T, T_buf = guarded(n_table, ld, torch.float32, NAN, random_table(31 * r + len(kind), n_table, r, ld, 0.0))
            cache[kind, r] = dict(lens=lens, ids_h=ids, vals_h=vals, seg=seg, T=T, T_buf=T_buf, ld=ld,
                                  ids=torch.tensor(ids, device='cuda'), vals=torch.tensor(vals, device='cuda'))
        return cache[kind, r]
    return get


@pytest.mark.parametrize('r', [1, 3, 33, 128, 300])
@pytest.mark.parametrize('kind', LISTS)
def test_feat_pass_grad_against_numpy(tm, feat_cases, kind, r):
    c = feat_cases(kind, r)
    seg, lens = c['seg'], c['lens']
    if kind == 'long row':
        assert seg.n_long == 1 and seg.n_slab == 3
    if kind == 'chunk 4':
        assert seg.n_long > 10 and seg.chunk == 4
    before = [c[k].clone() for k in ('ids', 'vals', 'T')]
    out = run_feat(tm, seg, c['ids'], c['vals'], c['T'], r, tm.L.EPI_GRAD)
    assert out.shape == (lens.size, c['ld'])
    ref, bound = product_bound(lens, c['ids_h'], c['vals_h'], c['T'][:, :r].cpu().numpy().astype(np.float64))
    got = out[:, :r].cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    print(f'[feat grad] {kind} r={r}: worst {float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0:.3g} of the bound')
    assert (err <= bound).all(), (kind, r)
    assert not out[:, r:].any()                                          # padding columns are exactly 0
    assert not out[torch.tensor(lens == 0, device='cuda')].any()         # an empty list gives a zero row
    assert all(torch.equal(a, c[k]) for a, k in zip(before, ('ids', 'vals', 'T'))) and guards_intact(c['T_buf'], NAN)   # only read
    again = run_feat(tm, seg, c['ids'], c['vals'], c['T'], r, tm.L.EPI_GRAD)
    assert torch.equal(out, again)


@pytest.mark.parametrize('r', [1, 3, 33, 128, 300])
@pytest.mark.parametrize('kind', LISTS)
def test_feat_pass_adam_is_the_row_update_of_its_sums(tm, feat_cases, kind, r):
    """TMF_EPI_ADAM = tmf_adam_fresh_rows_f32 applied to X_old with the TMF_EPI_GRAD output of the same lists: the same adam_fresh
    device function on the same sums, bit for bit."""
    L, lib, P = tm.L, tm.lib, tm.L.ptr
    c = feat_cases(kind, r)
    seg, lens, ld = c['seg'], c['lens'], c['ld']
    rows = lens.size
    X0 = random_table(17 * r + rows, rows, r, ld, 0.0)
    X_old, old_buf = guarded(rows, ld, torch.float32, NAN, X0)
    g = run_feat(tm, seg, c['ids'], c['vals'], c['T'], r, L.EPI_GRAD)
    got = run_feat(tm, seg, c['ids'], c['vals'], c['T'], r, L.EPI_ADAM, X_old=X_old)
    want = X0.clone()
    L.check(lib.tmf_adam_fresh_rows_f32(P(want), P(g.contiguous()), rows, r, tm.E.adam_constants(LR), L.stream_ptr()), lib)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(X_old, X0) and guards_intact(old_buf, NAN)        # X_old is only read
    empty = torch.tensor(lens == 0, device='cuda')
    assert torch.equal(got[empty], X0[empty])                            # a feature without entries keeps its weights exactly
    if rows and kind != 'one entry':
        assert not torch.equal(got, X0)


def test_table_past_32_bit_offsets(tm):
    """T of 2^22 + 5 rows x 512 floats (> 2^31 elements): lists that gather rows on both sides of element 2^31, against torch on
    the device; a 32-bit offset would fold the last rows onto the first."""
    r = ld = 512
    n_table = 2 ** 22 + 5
    assert n_table * ld > 2 ** 31
    gen = torch.Generator(device='cuda').manual_seed(9)
    T = torch.randn(n_table, ld, generator=gen, device='cuda')
    rng = np.random.default_rng(9)
    lens = rng.integers(1, 7, 300)
    lens[5] = 2 * 1024 + 7
    nnz = int(lens.sum())
    low, high = rng.integers(0, 4096, nnz), rng.integers(2 ** 22 - 2048, n_table, nnz)
    ids_h = np.where(rng.random(nnz) < 0.5, low, high).astype(np.int32)
    ids_h[:4] = [0, n_table - 1, 2 ** 22 - 1, 2 ** 22]                   # the ends, and the two rows around element 2^31
    vals_h = rng.choice(np.array([1.0, 0.5, -0.25, 2.0], np.float32), nnz)
    ids, vals = torch.tensor(ids_h, device='cuda'), torch.tensor(vals_h, device='cuda')
    rowptr = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device='cuda')
    seg = tm.E.SegmentTable(rowptr)
    out = run_feat(tm, seg, ids, vals, T, r, tm.L.EPI_GRAD)
    row_of = torch.repeat_interleave(torch.arange(300, device='cuda'), torch.tensor(lens, device='cuda'))
    n_i = torch.tensor(lens, device='cuda', dtype=torch.float64)[:, None]
    ref = torch.zeros(300, ld, dtype=torch.float64, device='cuda')
    mag = torch.zeros(300, ld, dtype=torch.float64, device='cuda')
    for lo in range(0, nnz, 1024):                                       # block by block: the gathered rows in fp64
        sl = slice(lo, min(lo + 1024, nnz))
        terms = vals[sl].double()[:, None] * T[ids[sl].long()].double()
        ref.index_add_(0, row_of[sl], terms)
        mag.index_add_(0, row_of[sl], terms.abs())
    assert bool(((out.double() - ref).abs() <= (n_i + 2) * 2.0 ** -24 * mag).all())
    assert bool((T[2 ** 22:].abs().sum() > 0)) and (ids_h >= 2 ** 22).any()
    del T, ref, mag, out
    gc.collect()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------
# fits
# ------------------------------------------------------------------------------------------------------------------------
def features_of(tm, p, featured):
    """(user_features, item_features) of a fit: SparseFeatures on the featured sides, the identity on the others."""
    return (tm.SF(*p['Fu']) if 'user' in featured else tm.eye(p['m']), tm.SF(*p['Fv']) if 'item' in featured else tm.eye(p['n']))


def fit(tm, model, p, featured, epochs, lr=LR):
    uf, vf = features_of(tm, p, featured)
    model.fit(epochs, uf, vf, tm.Sparse(p['idx'], p['val'], (p['m'], p['n'])), lr=lr)
    return model


def assert_step_with_slack(W_new, W0, g_ref, slack, lr, what):
    """assert_step with a per-element slack on the gradient; logs how many elements needed the slack and the largest share of it
    they used (the smallest t for which the element lies in the interval widened by t * slack, by bisection)."""
    W_new, W0, g_ref = (np.asarray(x, np.float64) for x in (W_new, W0, g_ref))
    assert_step(W_new, W0, g_ref, lr, rtol=1e-5, what=what, slack=slack)

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


def embedding_gradients(p, featured):
    """fp64 dL/dE of the first epoch for both sides: the oracle over identity features started from the effective tables
    E0 = F W0 of the featured sides."""
    from oracle import dense_ref as D
    E0 = [p['F' + s + '_dense'] @ p['W' + s + '0'].astype(np.float64) if name in featured else p[t0]
          for s, name, t0 in (('u', 'user', 'U0'), ('v', 'item', 'V0'))]
    ref = D.fit_dense_plugins(E0[0], E0[1], p['idx'], p['val'], p['loss'], 1, LR, np.eye(p['m']), np.eye(p['n']), random_ind=p['R'],
                              n_items=p['n'], n_samples=p['S'], dtype=torch.float64)
    return ref['first_grads'][0][0], ref['first_grads'][1][0]


ONE_STEP = [(loss, r) for loss in LOSSES for r in (3, 33, 128)] + [('mse', r) for r in (1, 7, 64, 100, 200, 300)]


def entry_bound(entries, W):
    """(fp64 F W, elementwise bound (nnz_row + 2) 2^-24 sum |x W|) of COO entries against weights W [n_features, r] (fp64)."""
    idx, val, shape = entries
    lens = np.bincount(idx[:, 0], minlength=shape[0])
    order = np.argsort(idx[:, 0], kind='stable')
    return product_bound(lens, idx[order, 1], val[order], W)


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('featured', SIDES, ids=SIDE_IDS)
@pytest.mark.parametrize('loss,r', ONE_STEP)
def test_one_step(tm, loss, r, featured, layout):
    m, n = 60, 40
    p = featured_problem(2000 + r, m, n, r, loss, layout)
    ref = featured_oracle(p, featured, 1)
    G = embedding_gradients(p, featured)
    model = fit(tm, _model(p, featured), p, featured, 1)
    what = f'{loss} r={r} {"+".join(featured)} {layout}'
    assert hasattr(model, '_state'), 'the fit did not run on the engine'
    assert rel_err(model.loss_history_[0], ref['loss'][0]) < 1e-5, what
    for s, name, rows, got, emb, embed, g_ref, G_ref in (
            ('u', 'user', m, model.user_trainable, model.user_embedding, model.embed_users, ref['first_grads'][0][0], G[0]),
            ('v', 'item', n, model.item_trainable, model.item_embedding, model.embed_items, ref['first_grads'][1][0], G[1])):
        assert len(got) == 1 and emb.is_cuda and emb.shape == (rows, r), f'{what} {name}'
        if name not in featured:
            assert torch.equal(emb, got[0])
            assert_step(host(got[0]), p[s.upper() + '0'], g_ref, LR, what=f'{what} {name} table')
            continue
        W0, F = p['W' + s + '0'], tm.SF(*p['F' + s])
        assert got[0].is_cuda and got[0].shape == W0.shape
        # every row's gradient agrees to 1e-5 -> feature f's sum may be off by 1e-5 sum_i |x_if| |G_ref[i]|
        slack = 1e-5 * np.abs(p['F' + s + '_dense']).T @ np.abs(G_ref)
        assert_step_with_slack(host(got[0]), W0, g_ref, slack, LR, f'{what} {name} weights')
        off = rows if layout == 'hybrid' else 0
        assert np.array_equal(host(got[0])[off + UNUSED], W0[off + UNUSED]), f'{what} {name}: a feature no row carries moved'
        assert torch.equal(emb, embed(F)), f'{what} {name}: embedding != embed(F)'
        prod, bound = entry_bound(p['F' + s], host(got[0]).astype(np.float64))
        assert (np.abs(host(emb).astype(np.float64) - prod) <= bound).all(), f'{what} {name}: embedding != F W'
        if layout == 'pure':
            assert not emb[p['tags_' + s]['bare']].any(), f'{what} {name}: a row without features has a non-zero embedding'


@pytest.mark.parametrize('loss', LOSSES)
def test_trajectory(tm, loss):
    """40 epochs, both sides hybrid, against the fp32 oracle with test_gpu_biased.test_trajectory's bounds."""
    epochs = 40
    p = featured_problem(77, 50, 35, 8, loss, 'hybrid', item_everywhere=False)
    ref = featured_oracle(p, BOTH, epochs, dtype=torch.float32)
    model = fit(tm, _model(p, BOTH), p, BOTH, epochs)
    h = model.loss_history_
    du = np.abs(host(model.user_trainable[0]) - ref['user_vars'][0]).max()
    dv = np.abs(host(model.item_trainable[0]) - ref['item_vars'][0]).max()
    print(f'[trajectory] {loss}: first three {rel_err(h[:3], ref["loss"][:3]):.3g}, all {rel_err(h, ref["loss"]):.3g}, weights {du:.3g} / {dv:.3g}')
    assert hasattr(model, '_state')
    assert rel_err(h[:3], ref['loss'][:3]) < 1e-5 and rel_err(h, ref['loss']) < 1e-3
    assert du <= LR * epochs * 0.5 and dv <= LR * epochs * 0.5
    pred = model.predict().cpu().numpy()
    assert np.array_equal(model.retrieve_user_recs(k=7), np.argsort(-pred, axis=1, kind='stable')[:, :7])


@pytest.mark.parametrize('featured', SIDES, ids=SIDE_IDS)
@pytest.mark.parametrize('loss', LOSSES)
def test_graph_replay_equals_eager_and_fits_repeat(tm, monkeypatch, loss, featured):
    p = featured_problem(21, 45, 30, 12, loss, 'hybrid')
    monkeypatch.delenv('TMF_NO_GRAPH', raising=False)
    a = fit(tm, _model(p, featured), p, featured, 8)
    monkeypatch.setenv('TMF_NO_GRAPH', '1')
    b = fit(tm, _model(p, featured), p, featured, 8)
    c = fit(tm, _model(p, featured), p, featured, 8)
    assert len(a.loss_history_) == 8 and np.isfinite(a.loss_history_).all() and hasattr(a, '_state')
    for other in (b, c):   # graph against eager, eager against eager
        assert a.loss_history_ == other.loss_history_
        for x, y in zip([a.user_embedding, a.item_embedding] + a.user_trainable + a.item_trainable,
                        [other.user_embedding, other.item_embedding] + other.user_trainable + other.item_trainable):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------------------
# dispatch
# ------------------------------------------------------------------------------------------------------------------------
def test_featured_fits_run_on_the_engine(tm, monkeypatch):
    """Every combination of test_one_step with _fit_generic refusing to run.  Without the engine path for SparseFeatures every
    one of these fits calls it."""
    def refuse(self, *a, **k):
        raise AssertionError('_fit_generic was called')
    monkeypatch.setattr(tm.MF, '_fit_generic', refuse)
    for loss, r in ONE_STEP:
        for layout in LAYOUTS:
            p = featured_problem(51, 30, 20, r, loss, layout)
            for featured in SIDES:
                model = fit(tm, _model(p, featured), p, featured, 2)
                assert hasattr(model, '_state') and len(model.loss_history_) == 2 and model.user_embedding.is_cuda
                assert (model._state.feat_u is not None) == ('user' in featured)
                assert (model._state.feat_v is not None) == ('item' in featured)
                assert model.user_trainable[0].shape == ((p['Wu0'] if 'user' in featured else p['U0']).shape)


def test_everything_else_over_sparse_features_stays_generic(tm, monkeypatch):
    """Each setting the engine has no featured form for calls _fit_generic exactly once, with the dense feature matrix."""
    from teamoflow_amd.mf.initializer_graphs import NormalInitializer
    calls = []
    monkeypatch.setattr(tm.MF, '_fit_generic', lambda self, epochs, uf, vf, *a, **k: calls.append((uf, vf)))
    p = featured_problem(52, 30, 20, 5, 'mse', 'hybrid')

    class Mine(tm.EG.LinearEmbedding):
        pass
    cases = [dict(user_repr_graph=tm.EG.BiasedLinearEmbedding()), dict(user_repr_graph=Mine()),
             dict(user_repr_graph=tm.EG.ReLUEmbedding(), user_weight_graph=NormalInitializer()),   # ReLU weights are [5 r, r]
             dict(factor_dtype=torch.bfloat16), dict(optimizer='adam'), dict(batch_users=8), dict(shard_items=2),
             dict(data_parallel='force')]
    Fu = tm.SF(*p['Fu'])
    for i, attrs in enumerate(cases):
        graphs = {k: attrs.pop(k) for k in list(attrs) if k.endswith('_graph')}
        model = _model(p, ('user',), **graphs)
        for k, v in attrs.items():
            setattr(model, k, v)
        model.fit(1, Fu, tm.eye(p['n']), tm.Sparse(p['idx'], p['val'], (p['m'], p['n'])), lr=LR)
        assert len(calls) == i + 1, (i, graphs, attrs)
        uf, vf = calls[-1]
        assert torch.is_tensor(uf) and not uf.is_sparse and torch.equal(uf.cpu(), Fu.to_dense().cpu()), (i, graphs, attrs)
        assert not torch.is_tensor(vf)                                   # the identity side is handed over as it came
    # KLDivergenceLoss over a table with an empty class: the engine declines, the generic path keeps the reference's NaN
    q = featured_problem(53, 30, 20, 5, 'kl', 'hybrid')
    q['val'] = np.abs(q['val'])
    _model(q, ('user',)).fit(1, tm.SF(*q['Fu']), tm.eye(q['n']), tm.Sparse(q['idx'], q['val'], (q['m'], q['n'])), lr=LR)
    assert len(calls) == len(cases) + 1 and torch.is_tensor(calls[-1][0])


def test_span_names_of_a_featured_epoch(tm):
    """The KernelTimer spans tools/time_features_c4.py reads, as an exact set; a biased indicator side beside a featured one."""
    p = featured_problem(54, 30, 20, 16, 'mse', 'hybrid')
    dev = torch.device('cuda')
    plan = tm.E.InteractionPlan(torch.tensor(p['idx'], device=dev), torch.tensor(p['val'], device=dev), 30, 20, csc=True)
    adam, loss = tm.E.adam_constants(LR), torch.zeros(1, dtype=torch.float64, device=dev)
    feat = {side + name for side in ('user_', 'item_') for name in ('feat_backward', 'feat_forward')}
    for kw, names in ((dict(user_feat=tm.SF(*p['Fu']), item_feat=tm.SF(*p['Fv'])), feat),
                      (dict(item_feat=tm.SF(*p['Fv']), user_bias=torch.zeros(16)),
                       {'item_feat_backward', 'item_feat_forward', 'user_bias_colsum', 'user_bias_adam', 'user_adam_bias_rows'})):
        st = tm.E.TrainState(p['U0'] if 'user_bias' in kw else p['Wu0'], p['Wv0'], plan, 16, **kw)
        prof = tm.E.KernelTimer()
        tm.E.epoch_sides(st, adam, loss, 'mse', prof=prof)
        torch.cuda.synchronize()
        assert set(prof.spans) == names | {'mse_user_pass', 'mse_item_pass'}
        assert all(b is not None for spans in prof.spans.values() for _, b in spans) and float(loss) > 0


# ------------------------------------------------------------------------------------------------------------------------
# cold start and scale
# ------------------------------------------------------------------------------------------------------------------------
def test_cold_start_items(tm):
    """embed_items on rows the fit has not seen: F_new W for the trained weights, through the forward kernel."""
    p = featured_problem(61, 40, 30, 7, 'mse', 'pure')
    model = fit(tm, _model(p, ('item',)), p, ('item',), 3)
    rng = np.random.default_rng(61)
    n_features = p['Fv'][2][1]
    idx = np.stack([rng.integers(0, 9, 40), rng.integers(0, n_features, 40)], 1)     # 9 new rows, row 8 possibly empty, duplicates
    idx = idx[idx[:, 0] != 8]
    val = rng.choice(np.array([1.0, 0.5, -0.25, 2.0], np.float32), idx.shape[0])
    F_new = tm.SF(idx, val, (9, n_features))
    got = model.embed_items(F_new)
    assert got.is_cuda and got.shape == (9, 7)
    W = host(model.item_trainable[0]).astype(np.float64)
    prod, bound = entry_bound((idx, val, (9, n_features)), W)
    assert np.allclose(prod, F_new.to_dense().cpu().numpy().astype(np.float64) @ W, rtol=0, atol=1e-12)
    assert (np.abs(host(got).astype(np.float64) - prod) <= bound).all() and not got[8].any()
    with pytest.raises(ValueError, match='SparseFeatures'):
        model.embed_users(F_new)
    with pytest.raises(ValueError, match='columns'):
        model.embed_items(tm.SF([[0, 0]], [1.0], (1, n_features + 1)))


def test_large_featured_fit_allocates_no_dense_table(tm):
    """200 000 users as [I | 3 tags of 50] x 2 000 items as [I | 4 tags of 30], 2e6 interactions: the dense user features alone
    would be 160 GB; the engine fit stays below 2 GB."""
    m, n, r, per_user = 200_000, 2_000, 16, 10
    rng = np.random.default_rng(0)
    users = np.repeat(np.arange(m), per_user)
    items = (users * 7 + np.tile(np.arange(per_user), m) * 199) % n       # ten distinct items per user
    idx = np.stack([users, items], 1)
    val = rng.integers(1, 6, idx.shape[0]).astype(np.float32)

    def tags(rows, per_row, n_tags):
        t = np.stack([np.repeat(np.arange(rows), per_row), rng.integers(0, n_tags, rows * per_row)], 1)
        return tm.hstack(rows, tm.SF(t, np.ones(t.shape[0], np.float32), (rows, n_tags)))
    Fu, Fv = tags(m, 3, 50), tags(n, 4, 30)
    assert Fu.shape == (m, m + 50) and Fv.shape == (n, n + 30)
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    model = tm.MF(r, user_weight_graph=FixedInitializer((rng.standard_normal((m + 50, r)) * 0.3).astype(np.float32)),
                  item_weight_graph=FixedInitializer((rng.standard_normal((n + 30, r)) * 0.3).astype(np.float32)))
    model.verbose = False
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    model.fit(3, Fu, Fv, tm.Sparse(idx, val, (m, n)), lr=LR)
    peak = torch.cuda.max_memory_allocated()
    print(f'[scale] peak allocated {peak / 1e6:.0f} MB')
    assert peak < 2e9
    assert hasattr(model, '_state') and model.user_embedding.shape == (m, r) and model.user_trainable[0].shape == (m + 50, r)
    h = model.loss_history_
    assert len(h) == 3 and h[2] < h[1] < h[0]
