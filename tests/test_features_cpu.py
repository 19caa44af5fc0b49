"""CPU side of SparseFeatures on the sparse HIP engine (no GPU): the problem generator of tests/test_gpu_features.py, the
container, the dispatch without a GPU, the C ABI of tmf_feat_pass_f32 (declared, bound, built, argument checks that fail before
anything is launched), and the statements the GPU tolerances rest on, checked on the reference alone
(oracle.dense_ref.fit_dense_plugins over F.to_dense(), fp32 against fp64):

  * one step: every weight table of the fp32 oracle lies inside conftest.assert_step's interval at rtol = 1e-5 and the loss agrees
    to 1e-5 - three losses, two shapes, both layouts ([I | tags] = hybrid, tags only = pure);
  * 40 epochs, hybrid layout: the loss agrees to 1e-5 over the first three epochs and to 1e-3 over all, the weights to
    lr * epochs * 0.5.  The pure layout (a dozen weight rows that every interaction moves) is held to one step and three epochs;
  * with WMRB an item feature that every item carries with the same value cancels like the item bias (test_biased_cpu): the
    generator's everywhere-feature carries varying values and skips the tagless row, and no trajectory problem has one on the item side.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_step, rel_err
from test_biased_cpu import LR, biased_problem

N_TAGS = 10
UNUSED, EVERYWHERE = N_TAGS, N_TAGS + 1          # tag columns: a feature no row carries, a feature every row with tags carries
N_TAG_COLUMNS = N_TAGS + 2
TAG_VALUES = np.array([1.0, 0.5, -0.25, 2.0], np.float32)
LAYOUTS = ('hybrid', 'pure')
LOSSES = ('mse', 'wmrb', 'kl')


def tag_entries(rng, rows, everywhere=True):
    """COO entries of a [rows, N_TAG_COLUMNS] tag matrix in shuffled order: 0 - 3 distinct random tags per row out of N_TAGS with
    values from TAG_VALUES, row ``bare`` without any entry, column UNUSED without any, column EVERYWHERE on every other row
    (``everywhere``), one (row, tag) pair twice and one explicit zero.  -> (indices [nnz, 2], values, dict of the special places)."""
    bare = rows // 4
    idx, val = [], []
    for i in range(rows):
        if i == bare:
            continue
        for t in rng.choice(N_TAGS, rng.integers(0, 4), replace=False):
            idx.append((i, int(t)))
            val.append(rng.choice(TAG_VALUES))
        if everywhere:
            idx.append((i, EVERYWHERE))
            val.append(rng.choice(TAG_VALUES))
    dup = idx[len(idx) // 2]
    idx.append(dup)                                # a duplicate: the two values add up
    val.append(np.float32(0.5))
    zero = (rows - 1, int(rng.integers(0, N_TAGS)))
    while zero in idx:
        zero = (rows - 1, (zero[1] + 1) % N_TAGS)
    idx.append(zero)                               # an explicit zero: kept, multiplies like any value
    val.append(np.float32(0.0))
    order = rng.permutation(len(idx))
    return np.asarray(idx, np.int64)[order], np.asarray(val, np.float32)[order], dict(bare=bare, dup=dup, zero=zero)


def layout_entries(layout, rows, tags):
    """(indices, values, shape) of [I | tags] (hybrid) or of the tags alone (pure)."""
    idx, val, _ = tags
    if layout == 'pure':
        return idx, val, (rows, N_TAG_COLUMNS)
    own = np.arange(rows, dtype=np.int64)
    return (np.concatenate([np.stack([own, own], 1), idx + np.array([0, rows])]), np.concatenate([np.ones(rows, np.float32), val]),
            (rows, rows + N_TAG_COLUMNS))


def dense_of(entries):
    idx, val, shape = entries
    A = np.zeros(shape, np.float64)
    np.add.at(A, (idx[:, 0], idx[:, 1]), val.astype(np.float64))
    return A


def featured_problem(seed, m, n, r, loss, layout, item_everywhere=True):
    """test_biased_cpu.biased_problem plus, per side, the entries of its feature matrix in ``layout`` (p['Fu'], p['Fv']: indices,
    values, shape), their dense fp64 forms (p['Fu_dense'], ..), starting weights [n_features, r] ~ N(0, 0.3^2) (p['Wu0'], p['Wv0'])
    and the special places of the tag matrices (p['tags_u'], p['tags_v']).  p['U0'] / p['V0'] stay the [rows, r] tables of a side
    trained over identity features."""
    p = biased_problem(seed, m, n, r, loss)
    rng = np.random.default_rng(seed + 7919)
    for side, rows, everywhere in (('u', m, True), ('v', n, item_everywhere)):
        tags = tag_entries(rng, rows, everywhere)
        entries = layout_entries(layout, rows, tags)
        p['F' + side], p['F' + side + '_dense'], p['tags_' + side] = entries, dense_of(entries), tags[2]
        p['W' + side + '0'] = (rng.standard_normal((entries[2][1], r)) * 0.3).astype(np.float32)
    p['layout'] = layout
    return p


def featured_oracle(p, featured, epochs, lr=LR, dtype=torch.float64):
    """fit_dense_plugins with the dense feature matrix on the sides named in ``featured`` ('user', 'item') and the identity on
    the others."""
    from oracle import dense_ref as D
    fu, fi = 'user' in featured, 'item' in featured
    return D.fit_dense_plugins(p['Wu0'] if fu else p['U0'], p['Wv0'] if fi else p['V0'], p['idx'], p['val'], p['loss'], epochs, lr,
                               p['Fu_dense'] if fu else np.eye(p['m']), p['Fv_dense'] if fi else np.eye(p['n']), random_ind=p['R'],
                               n_items=p['n'], n_samples=p['S'], dtype=dtype)


BOTH = ('user', 'item')


# ------------------------------------------------------------------------------------------------------------------------
# the generator and the container
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', LAYOUTS)
def test_problem_generator(layout):
    p = featured_problem(5, 60, 40, 7, 'mse', layout)
    for side, rows in (('u', 60), ('v', 40)):
        (idx, val, shape), A, tags = p['F' + side], p['F' + side + '_dense'], p['tags_' + side]
        off = rows if layout == 'hybrid' else 0
        assert shape == (rows, off + N_TAG_COLUMNS) and p['W' + side + '0'].shape == (shape[1], 7)
        T = A[:, off:]
        pairs = [tuple(x) for x in idx.tolist()]
        assert len(pairs) - len(set(pairs)) == 1                               # one duplicated pair, summed by the dense form
        dup = (tags['dup'][0], tags['dup'][1] + off)
        assert pairs.count(dup) == 2 and A[dup] == val[[i for i, q in enumerate(pairs) if q == dup]].astype(np.float64).sum()
        zero = (tags['zero'][0], tags['zero'][1] + off)
        assert val[pairs.index(zero)] == 0.0 and A[zero] == 0.0                # an explicit zero
        assert not T[tags['bare']].any() and not T[:, UNUSED].any()            # a row without tags, a feature no row carries
        assert (np.delete(T[:, EVERYWHERE], tags['bare']) != 0).all()          # a feature every other row carries
        per_row = (T[:, :N_TAGS] != 0).sum(1)
        assert per_row.max() <= 4 and set(per_row) >= {0, 1, 2, 3}
        assert set(np.unique(val)) <= set(TAG_VALUES) | {0.0}
        if layout == 'hybrid':
            assert np.array_equal(A[:, :rows], np.eye(rows))
    q = featured_problem(5, 60, 40, 7, 'wmrb', 'hybrid', item_everywhere=False)
    assert not q['Fv_dense'][:, 40 + EVERYWHERE].any() and q['Fu_dense'][:, 60 + EVERYWHERE].any()


def test_container():
    from teamoflow_amd.mf.sparse import SparseFeatures, hstack_identity
    import teamoflow.mf as alias
    assert alias.SparseFeatures is SparseFeatures and alias.hstack_identity is hstack_identity
    idx, val, shape = featured_problem(9, 30, 20, 4, 'mse', 'pure')['Fu']
    F = SparseFeatures(idx, val, shape, device='cpu')
    assert F.shape == shape and F.nnz == len(val) and F.device == torch.device('cpu') and F.to('cpu').nnz == F.nnz
    assert F.indices.dtype == torch.int64 and F.values.dtype == torch.float32 and (F.values == 0).sum() == 1   # the zero is kept
    D = F.to_dense()
    assert D.dtype == torch.float32 and np.array_equal(D.numpy(), dense_of((idx, val, shape)).astype(np.float32))   # duplicates add up
    back = SparseFeatures.from_dense(D, device='cpu')
    assert back.nnz == int((D != 0).sum()) and torch.equal(back.to_dense(), D)
    assert torch.equal(SparseFeatures.from_dense(D.numpy(), device='cpu').to_dense(), D)
    sp = pytest.importorskip('scipy.sparse')
    coo = sp.coo_matrix((val, (idx[:, 0], idx[:, 1])), shape=shape)
    S = SparseFeatures.from_scipy(coo, device='cpu')
    assert S.nnz == F.nnz and torch.equal(S.to_dense(), D)                     # explicit zero and duplicate included
    assert torch.equal(SparseFeatures.from_scipy(coo.tocsr(), device='cpu').to_dense(), D)
    H = hstack_identity(30, F)
    assert H.shape == (30, 30 + shape[1]) and H.nnz == 30 + F.nnz
    assert torch.equal(H.to_dense(), torch.cat([torch.eye(30), D], 1))
    with pytest.raises(ValueError):
        hstack_identity(31, F)
    for bad in ([[30, 0]], [[0, shape[1]]], [[-1, 0]], [[0, -1]]):
        with pytest.raises(IndexError):
            SparseFeatures(bad, [1.0], shape, device='cpu')
    with pytest.raises(ValueError):
        SparseFeatures([[0, 0], [1, 1]], [1.0], shape, device='cpu')
    with pytest.raises(ValueError):
        SparseFeatures([[0, 0]], [1.0], (4, 2 ** 31), device='cpu')
    empty = SparseFeatures(np.zeros((0, 2)), np.zeros(0), (3, 5), device='cpu')
    assert empty.nnz == 0 and not empty.to_dense().any()


# ------------------------------------------------------------------------------------------------------------------------
# dispatch without a GPU
# ------------------------------------------------------------------------------------------------------------------------
def _model(p, featured, **graphs):
    from teamoflow_amd.mf import loss_graphs as LG
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    kw = dict(user_weight_graph=FixedInitializer(p['Wu0'] if 'user' in featured else p['U0']),
              item_weight_graph=FixedInitializer(p['Wv0'] if 'item' in featured else p['V0']))
    kw.update(graphs)
    if p['loss'] == 'wmrb':
        kw.update(loss_graph=LG.WMRBLoss(), n_users=p['m'], n_items=p['n'], n_samples=p['S'])
    elif p['loss'] == 'kl':
        kw.update(loss_graph=LG.KLDivergenceLoss())
    model = MatrixFactorization(p['r'], **kw)
    model.verbose = False
    if p['loss'] == 'wmrb':
        model.random_ind = torch.as_tensor(p['R'])
    return model


@pytest.mark.parametrize('loss', LOSSES)
def test_fit_without_a_gpu_equals_the_dense_features_fit(monkeypatch, loss):
    """No GPU: SparseFeatures reaches _fit_generic as F.to_dense(), so the fit is, bit for bit, the fit with that matrix."""
    from teamoflow_amd.mf.sparse import SparseFeatures, SparseInteractions, eye
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    p = featured_problem(13, 30, 20, 5, loss, 'hybrid')
    inter = SparseInteractions(p['idx'], p['val'], (30, 20))
    Fu, Fv = SparseFeatures(*p['Fu']), SparseFeatures(*p['Fv'])
    for featured, feats in ((BOTH, (Fu, Fv)), (('user',), (Fu, eye(20))), (('item',), (eye(30), Fv))):
        a, b = _model(p, featured), _model(p, featured)
        a.fit(3, feats[0], feats[1], inter, lr=LR)
        b.fit(3, *(f.to_dense() if isinstance(f, SparseFeatures) else f for f in feats), inter, lr=LR)
        assert not hasattr(a, '_state') and a.loss_history_ == b.loss_history_ and len(a.loss_history_) == 3
        assert torch.equal(a.user_embedding, b.user_embedding) and torch.equal(a.item_embedding, b.item_embedding)
        assert torch.equal(a.user_trainable[0], b.user_trainable[0]) and torch.equal(a.item_trainable[0], b.item_trainable[0])
        if 'user' in featured:   # cold start after a generic fit: the dense definition
            assert a.user_trainable[0].shape == p['Wu0'].shape
            assert torch.equal(a.embed_users(Fu), a.user_embedding)
        else:
            with pytest.raises(ValueError, match='SparseFeatures'):
                a.embed_users(Fu)
        with pytest.raises(ValueError, match='columns'):
            (a.embed_users if 'user' in featured else a.embed_items)(SparseFeatures([[0, 0]], [1.0], (1, 3)))


def test_dispatch_predicate(monkeypatch):
    """A side over SparseFeatures is an engine side under the conditions a biased side is (one predicate), and only as exactly
    LinearEmbedding; what exists today does not change."""
    from teamoflow_amd.mf.embedding_graphs import BiasedLinearEmbedding, LinearEmbedding, ReLUEmbedding
    from teamoflow_amd.mf.loss_graphs import KLDivergenceLoss, LossGraph, MSELoss, WMRBLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseFeatures, eye

    class Mine(LinearEmbedding):
        pass

    class MyLoss(MSELoss):
        pass
    assert issubclass(MyLoss, LossGraph)
    F6, F7 = SparseFeatures([[0, 1], [5, 2]], [1.0, 2.0], (6, 3), device='cpu'), SparseFeatures([[6, 0]], [1.0], (7, 9), device='cpu')
    none = SparseFeatures(np.zeros((0, 2)), np.zeros(0), (6, 3), device='cpu')

    def model(u=LinearEmbedding, i=LinearEmbedding, loss=None, **attrs):
        mf = MatrixFactorization(4, user_repr_graph=u(), item_repr_graph=i(), **({'loss_graph': loss} if loss else {}))
        for k, v in attrs.items():
            setattr(mf, k, v)
        return mf
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    assert model()._route(F6, eye(7)) == 'generic' and model()._route(eye(6), F7) == 'generic' and model()._route(F6, F7) == 'generic'
    assert model()._route(eye(6), eye(7)) == 'engine'
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    for loss in (None, WMRBLoss(), KLDivergenceLoss()):
        assert model(loss=loss)._route(F6, eye(7)) == 'engine' and model(loss=loss)._route(eye(6), F7) == 'engine'
        assert model(loss=loss)._route(F6, F7) == 'engine'
        assert model(u=BiasedLinearEmbedding, loss=loss)._route(eye(6), F7) == 'engine'      # a biased indicator side beside a featured one
    assert model(loss=MyLoss())._route(F6, F7) == 'generic'
    for kind in (BiasedLinearEmbedding, ReLUEmbedding, Mine):
        assert model(u=kind)._route(F6, eye(7)) == 'generic' and model(i=kind)._route(eye(6), F7) == 'generic', kind
    assert model()._route(none, eye(7)) == 'generic'                                      # nothing to multiply: the generic zeros
    for name, value in (('batch_users', 8), ('shard_items', 2), ('data_parallel', 'force'), ('factor_dtype', torch.bfloat16),
                        ('optimizer', 'adam')):
        assert model(**{name: value})._route(F6, eye(7)) == 'generic', name
        assert model(**{name: value})._route(eye(6), F7) == 'generic', name
        assert model(**{name: value})._route(eye(6), eye(7)) == 'engine', name
        assert (model(u=BiasedLinearEmbedding, **{name: value})._route(eye(6), eye(7))
                == model(**{name: value})._route(F6, eye(7)) == 'generic'), name   # one row of ROUTES for both
    # dense and torch-sparse inputs keep the generic path, as before
    dense = torch.eye(6)[:, :3].contiguous()
    assert model()._route(dense, eye(7)) == 'generic' and model()._route(dense.to_sparse(), eye(7)) == 'generic'


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_built_and_listed():
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    declared = set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    lib = _lib.load_library()
    assert 'tmf_feat_pass_f32' in declared and 'tmf_feat_pass_f32' in _lib.SIGNATURES and hasattr(lib, 'tmf_feat_pass_f32')
    make = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS :=.*\btmf_feat\.hip\b', make, re.M)


def test_argument_checks_fail_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail differently (or crash); these return first."""
    from teamoflow_amd import _lib
    lib = _lib.load_library()
    adam = lib.tmf_adam_fresh(0.05)
    i64, i32 = (ctypes.c_int64 * 2)(0, 1), (ctypes.c_int32 * 1)(0)
    slab = (ctypes.c_int32 * 1)(-1)
    host = (ctypes.c_double * 8)()              # stands for any non-null table / list / buffer: never dereferenced
    H = ctypes.cast(host, ctypes.c_void_p)

    def seg(nseg, chunk=1024):
        return ctypes.byref(_lib.Segments(ctypes.addressof(i64), ctypes.addressof(i32), ctypes.addressof(i32), ctypes.addressof(slab),
                                          nseg, chunk, 0))

    def failed(rc, word):
        return rc != 0 and word in lib.tmf_last_error().decode()
    feat = lib.tmf_feat_pass_f32
    G, A = _lib.EPI_GRAD, _lib.EPI_ADAM
    assert feat(seg(0), None, None, None, None, None, None, 24, 7, adam, None) == 0                 # nothing to do
    assert failed(feat(seg(1), H, H, None, H, H, H, 24, G, adam, None), 'null table')                # T
    assert failed(feat(seg(1), H, H, H, H, None, H, 24, G, adam, None), 'null table')                # X_out
    assert failed(feat(seg(1), H, H, H, None, H, H, 24, A, adam, None), 'null table')                # X_old under ADAM
    assert failed(feat(seg(1), None, H, H, H, H, H, 24, G, adam, None), 'entry list')
    assert failed(feat(seg(1), H, None, H, H, H, H, 24, G, adam, None), 'entry list')
    for epi in (2, -1, 7):
        assert failed(feat(seg(1), H, H, H, H, H, H, 24, epi, adam, None), f'bad epilogue {epi}')
    assert failed(feat(None, H, H, H, H, H, H, 24, G, adam, None), 'segments')
    assert failed(feat(seg(1, chunk=0), H, H, H, H, H, H, 24, G, adam, None), 'segments')
    assert feat(seg(1), H, H, H, H, H, H, 5000, G, adam, None) != 0 and 'n_components' in lib.tmf_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------------
# what the GPU tolerances rest on: the fp32 reference against the fp64 reference
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('shape', [(60, 40, 7), (300, 90, 33)])
@pytest.mark.parametrize('loss', LOSSES)
def test_fp32_oracle_step_lies_inside_the_intervals(loss, shape, layout):
    p = featured_problem(sum(shape), *shape, loss, layout)
    ref64, ref32 = featured_oracle(p, BOTH, 1), featured_oracle(p, BOTH, 1, dtype=torch.float32)
    what = f'{loss} {shape} {layout} fp32 oracle'
    d = rel_err(ref32['loss'][0], ref64['loss'][0])
    print(f'[oracle step] {what}: loss differs by {d:.3g}')
    assert d < 1e-5, what
    (gU,), (gV,) = ref64['first_grads']
    assert gU.shape == p['Wu0'].shape and gV.shape == p['Wv0'].shape
    assert_step(ref32['user_vars'][0], p['Wu0'], gU, LR, what=what + ' W_u')
    assert_step(ref32['item_vars'][0], p['Wv0'], gV, LR, what=what + ' W_v')
    off_u, off_v = (shape[0], shape[1]) if layout == 'hybrid' else (0, 0)
    assert not gU[off_u + UNUSED].any() and not gV[off_v + UNUSED].any()          # a feature no row carries has no gradient
    assert np.array_equal(ref32['user_vars'][0][off_u + UNUSED], p['Wu0'][off_u + UNUSED])
    if layout == 'pure':
        assert not ref64['user_embedding'][p['tags_u']['bare']].any()             # a row without features embeds to zero


@pytest.mark.parametrize('loss', LOSSES)
def test_fp32_oracle_trajectory_hybrid(loss):
    epochs = 40
    p = featured_problem(77, 50, 35, 8, loss, 'hybrid', item_everywhere=False)
    ref64, ref32 = featured_oracle(p, BOTH, epochs), featured_oracle(p, BOTH, epochs, dtype=torch.float32)
    first, whole = rel_err(ref32['loss'][:3], ref64['loss'][:3]), rel_err(ref32['loss'], ref64['loss'])
    du = np.abs(ref32['user_vars'][0] - ref64['user_vars'][0]).max()
    dv = np.abs(ref32['item_vars'][0] - ref64['item_vars'][0]).max()
    print(f'[oracle trajectory] {loss}: first three {first:.3g}, all {whole:.3g}, weights {du:.3g} / {dv:.3g}')
    assert first < 1e-5 and whole < 1e-3
    assert du <= LR * epochs * 0.5 and dv <= LR * epochs * 0.5


@pytest.mark.parametrize('loss', LOSSES)
def test_fp32_oracle_first_three_epochs_pure(loss):
    p = featured_problem(78, 50, 35, 8, loss, 'pure')
    ref64, ref32 = featured_oracle(p, BOTH, 3), featured_oracle(p, BOTH, 3, dtype=torch.float32)
    assert rel_err(ref32['loss'], ref64['loss']) < 1e-5
