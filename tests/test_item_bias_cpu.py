"""CPU side of the scalar item bias (scalar_item_bias / item_bias_; no GPU): off is off, the generic loop's step against the fp64
reference (tests/item_bias_ref.py), the refusals and the route table, save / load, the chunk tables of tmf_item_bias_grad and the
augmented tables every ranking call goes through."""
import importlib.util
import json
import os
import string

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, assert_step, rel_err
from item_bias_ref import biased_reference
from test_bpr_cpu import bpr_problem

LR = 0.05
PROBLEM = (11, 30, 20, 4, 6)   # seed, users, items, r, S


def _parts():
    from teamoflow_amd.mf import loss_graphs as L
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye

    class PluginBPR(L.BPRLoss):        # a subclass is a plug-in loss: the generic loop on every machine, fed the samples
        pass

    class PluginSquares(L.LossGraph):   # a loss of the dense [m, n] matrix
        def get_loss(self, tf_interactions, predictions, tf_sample_predictions=None, tf_prediction_serial=None, n_items=None,
                     n_samples=None):
            idx = tf_interactions.indices
            return torch.square(tf_interactions.values.to(predictions.dtype) - predictions[idx[:, 0], idx[:, 1]])
    return L, FixedInitializer, MatrixFactorization, SparseInteractions, eye, PluginBPR, PluginSquares


def _model(p, loss, init=None, **attrs):
    L, Fixed, MF, Sparse, eye, _, _ = _parts()
    model = MF(p['r'], loss_graph=loss, user_weight_graph=init or Fixed(p['U0']), item_weight_graph=init or Fixed(p['V0']),
               n_users=p['m'], n_items=p['n'], n_samples=p['S'])
    model.verbose, model.random_ind = False, torch.as_tensor(p['R'])
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


def _fit(p, loss, epochs, **attrs):
    _, _, _, Sparse, eye, _, _ = _parts()
    model = _model(p, loss, **attrs)
    model.fit(epochs, eye(p['m']), eye(p['n']), Sparse(p['idx'], p['val'], (p['m'], p['n'])), lr=LR)
    return model


def host(t):
    return t.detach().float().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------
# off is off
# ------------------------------------------------------------------------------------------------------------------------
def test_off_is_a_model_that_never_had_the_setting(tmp_path):
    _, _, MF, _, _, PluginBPR, _ = _parts()
    p = bpr_problem(*PROBLEM)
    off = _fit(p, PluginBPR(), 3)
    assert off.scalar_item_bias is False and off.item_bias_ is None
    bare = _model(p, PluginBPR())
    del bare.scalar_item_bias, bare.item_bias_
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    bare.fit(3, eye(p['m']), eye(p['n']), SparseInteractions(p['idx'], p['val'], (p['m'], p['n'])), lr=LR)
    assert torch.equal(off.user_embedding, bare.user_embedding) and torch.equal(off.item_embedding, bare.item_embedding)
    assert off.loss_history_ == bare.loss_history_ and bare.item_bias_ is None
    # the file of a model without the setting has no word of it; both states come back
    del bare.item_bias_
    builtin = _parts()[0].BPRLoss()   # a file stores built-in plug-ins as plain data
    off.loss_graph = bare.loss_graph = builtin
    off.save(tmp_path / 'off.pt')
    bare.save(tmp_path / 'bare.pt')
    blob_off, blob_bare = (torch.load(tmp_path / f, weights_only=True) for f in ('off.pt', 'bare.pt'))
    assert sorted(blob_off) == sorted(blob_bare) and 'scalar_item_bias' not in blob_off and 'item_bias' not in blob_off
    back = MF.load(tmp_path / 'off.pt', device='cpu')
    assert back.scalar_item_bias is False and back.item_bias_ is None
    on = _fit(p, PluginBPR(), 2, scalar_item_bias=True)
    on.loss_graph = builtin
    on.save(tmp_path / 'on.pt')
    back = MF.load(tmp_path / 'on.pt', device='cpu')
    assert back.scalar_item_bias is True and torch.equal(back.item_bias_, on.item_bias_.cpu()) and back.item_bias_.dtype == torch.float32
    assert torch.equal(back.item_embedding, on.item_embedding.cpu())


# ------------------------------------------------------------------------------------------------------------------------
# the generic loop
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['samples', 'dense'])
def test_generic_loop_steps_the_bias_with_the_tables(kind):
    _, _, _, _, _, PluginBPR, PluginSquares = _parts()
    p = bpr_problem(*PROBLEM)
    loss = PluginBPR() if kind == 'samples' else PluginSquares()
    ref = biased_reference(loss, p['U0'], p['V0'], np.zeros(p['n']), p['idx'], p['val'], p['R'], p['n'], p['S'], feeds=kind)
    assert np.abs(ref['gb']).max() > 0.1
    one = _fit(p, loss, 1, scalar_item_bias=True)
    assert one.item_bias_.shape == (p['n'],) and one.item_bias_.dtype == torch.float32
    assert rel_err(one.loss_history_[0], ref['loss_sum'] / ref['n_terms']) < 1e-5
    assert_step(host(one.user_embedding), p['U0'], ref['gU'], LR, what=f'{kind} U')
    assert_step(host(one.item_embedding), p['V0'], ref['gV'], LR, what=f'{kind} V')
    assert_step(host(one.item_bias_), np.zeros(p['n']), ref['gb'], LR, what=f'{kind} b')
    # the bias changes the fit: the same epochs without it end elsewhere
    three, plain = _fit(p, loss, 3, scalar_item_bias=True), _fit(p, loss, 3)
    assert three.loss_history_[0] == plain.loss_history_[0] and three.loss_history_[1:] != plain.loss_history_[1:]
    # an item that is nobody's entry and nobody's sample keeps b = 0.0 exactly
    b = host(three.item_bias_)
    assert b[p['empty_item']] == 0.0 and np.count_nonzero(b) >= p['n'] - 2
    # the score of the model is U V^T + b: the tables every ranking call shares
    from teamoflow_amd.mf.matrix_factorization import augmented_tables
    Ua, Va, fused = augmented_tables(three.user_embedding, three.item_embedding, three.item_bias_)
    want = host(three.user_embedding).astype(np.float64) @ host(three.item_embedding).astype(np.float64).T + b[None, :]
    assert fused and rel_err(host(Ua) @ host(Va).T, want) < 1e-6
    again = _fit(p, loss, 3, scalar_item_bias=True)   # every fit starts the bias from zeros
    assert torch.equal(again.item_bias_, three.item_bias_)


# ------------------------------------------------------------------------------------------------------------------------
# the refusals
# ------------------------------------------------------------------------------------------------------------------------
class _Spy:
    def __init__(self):
        self.calls = 0

    def initialize_weights(self, n_features, n_components):
        self.calls += 1
        return torch.zeros(n_features, n_components)


def _refused():
    L = _parts()[0]
    yield 'batch_users', L.BPRLoss(), dict(batch_users=8)
    yield 'shard_items', L.BPRLoss(), dict(shard_items=2)
    yield 'data_parallel', L.BPRLoss(), dict(data_parallel=True)
    yield 'data_parallel', L.WMRBLoss(), dict(data_parallel='force')
    yield 'factor_dtype', L.WARPLoss(), dict(factor_dtype=torch.bfloat16)
    yield 'factor_dtype', L.WMRBLoss(), dict(factor_dtype=torch.bfloat16)
    for loss in (L.MSELoss(), L.KLDivergenceLoss(), L.LogisticLoss(), L.LogisticLoss(weighted=True), L.FullSoftmaxLoss()):
        yield type(loss).__name__, loss, {}


def test_every_refusal_names_the_setting_before_a_weight_is_drawn():
    _, _, _, Sparse, eye, _, _ = _parts()
    p = bpr_problem(*PROBLEM)
    inter = Sparse(p['idx'], p['val'], (p['m'], p['n']))
    for named, loss, attrs in _refused():
        spy = _Spy()
        model = _model(p, loss, init=spy, scalar_item_bias=True, **attrs)
        with pytest.raises(NotImplementedError, match=r'scalar_item_bias=True with ' + named) as e:
            model.fit(1, eye(p['m']), eye(p['n']), inter, lr=LR)
        assert 'back to its default' in str(e.value) and spy.calls == 0, (named, attrs)
    for bad in (1, 0, 'yes', None, 1.0):
        spy = _Spy()
        model = _model(p, _parts()[0].BPRLoss(), init=spy, scalar_item_bias=bad)
        with pytest.raises(ValueError, match='scalar_item_bias'):
            model.fit(1, eye(p['m']), eye(p['n']), inter, lr=LR)
        assert spy.calls == 0


def test_the_table_of_the_refusals():
    from teamoflow_amd import _engine
    from teamoflow_amd.mf import matrix_factorization as M
    row = M.ITEM_BIAS_ROUTES['item_bias']
    assert list(row) == list(M._SETTINGS) and set(row.values()) == {'ok', 'refuse'}
    assert [s for s, a in row.items() if a == 'refuse'] == ['batch_users', 'shard_items', 'data_parallel set', 'data_parallel active', 'bf16']
    assert set(M.ITEM_BIAS_FAMILIES) == {rec.family for rec in _engine.LOSSES.values()}
    assert [f for f, a in M.ITEM_BIAS_FAMILIES.items() if a == 'ok'] == ['table']
    with open(os.path.join(ROOT, 'DESIGN.md')) as f:
        design = f.read()
    head = ['feature \\ setting'] + list(M._SETTINGS)
    printed = '\n'.join('| ' + ' | '.join(cells) + ' |' for cells in (head, ['---'] * len(head), ['`item_bias`'] + list(row.values())))
    assert '\n\n' + printed + '\n\n' in design, 'DESIGN.md, "What trains where", should print:\n' + printed


@pytest.mark.parametrize('state', ['False', 'absent'])
def test_every_recorded_route_is_unchanged_without_the_setting(state, monkeypatch):
    spec = importlib.util.spec_from_file_location('make_golden_ib', os.path.join(GOLDEN, 'make_golden.py'))
    make_golden = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make_golden)
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    if state == 'absent':
        init = MatrixFactorization.__init__

        def bare(self, *a, **k):
            init(self, *a, **k)
            del self.scalar_item_bias, self.item_bias_
        monkeypatch.setattr(MatrixFactorization, '__init__', bare)
    with open(os.path.join(GOLDEN, 'fit_routes.json')) as f:
        doc = json.load(f)
    texts = doc['outcomes']
    recorded = {kind: {key: [texts[string.ascii_letters.index(ch)] for ch in rows] for key, rows in doc[kind].items()}
                for kind in ('fit', 'als')}
    assert make_golden.fit_route_outcomes() == recorded


# ------------------------------------------------------------------------------------------------------------------------
# the chunk tables of tmf_item_bias_grad and the augmented tables
# ------------------------------------------------------------------------------------------------------------------------
def test_chunk_tables_list_every_further_chunk_by_item_block_and_chunk():
    from teamoflow_amd import _engine
    n, C, chunk = 3, 2, 4
    lens = torch.tensor([0, 13, 4, 9, 5, 0])            # list rows (block 0: items 0..2, block 1: items 0..2)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    xrow, xchunk, xptr, n_extra = _engine.item_bias_chunks(rowptr, n, chunk)
    assert n_extra == 6 and xrow.dtype == xchunk.dtype == torch.int32 and xptr.dtype == torch.int64
    assert list(zip(xrow.tolist(), xchunk.tolist())) == [(3, 1), (3, 2), (1, 1), (1, 2), (1, 3), (4, 1)]
    assert xptr.tolist() == [0, 2, 6, 6]
    xrow, xchunk, xptr, n_extra = _engine.item_bias_chunks(rowptr, n, 16)
    assert n_extra == 0 and xrow.numel() == 0 and xptr.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize('r', [1, 3, 4, 127, 128, 255, 256])
def test_augmented_tables(r):
    from teamoflow_amd.mf.matrix_factorization import augmented_tables
    g = torch.Generator().manual_seed(r)
    U, V, b = torch.randn(5, r, generator=g), torch.randn(7, r, generator=g), torch.randn(7, generator=g)
    Ua, Va, fused = augmented_tables(U, V, b)
    assert fused == (r != 256)
    for T, rows in ((Ua, 5), (Va, 7)):
        assert tuple(T.shape) == (rows, r + 1) and T.dtype == torch.float32 and T.stride(1) == 1
        assert T.stride(0) % 4 == 0 and T.stride(0) >= r + 1 and T.data_ptr() % 16 == 0
    assert torch.equal(Ua[:, :r], U) and torch.equal(Va[:, :r], V) and torch.equal(Va[:, r], b) and bool((Ua[:, r] == 1.0).all())
    want = U.double() @ V.double().T + b.double()[None, :]
    assert rel_err((Ua.double() @ Va.double().T).numpy(), want.numpy()) < 1e-14
