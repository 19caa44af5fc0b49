"""CPU side of similar_items / similar_users (no GPU): the fp64 oracle's known answers, the C ABI of tmf_unit_rows_* (declared, bound,
built; its argument checks with null pointers, which return before any launch) and the model-level refusals, all of which run
before the engine is touched."""
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from similar_ref import similar_ref, similarities, unit_rows_ref

NEW_ENTRY_POINTS = ('tmf_unit_rows_f32', 'tmf_unit_rows_bf16')


# ------------------------------------------------------------------ the oracle
def test_oracle_duplicates_come_out_in_id_order():
    T = np.array([[1.0, 0.0], [0.0, 2.0], [3.0, 0.0], [1.0, 1.0], [0.5, 0.0]])
    ids, vals, S = similar_ref(T, 3)
    assert ids[0].tolist() == [2, 4, 3] and ids[2].tolist() == [0, 4, 3] and ids[4].tolist() == [0, 2, 3]   # cosine 1 twice: ids ascending
    assert np.allclose(vals[0], [1.0, 1.0, np.sqrt(0.5)]) and S.shape == (5, 5)
    assert ids[1].tolist() == [3, 0, 2]   # 0, 2 and 4 tie at cosine 0
    ids, vals, _ = similar_ref(T, 2, include_self=True)
    assert ids[:, 0].tolist() == [0, 1, 0, 3, 0] and np.allclose(vals[:, 0], 1.0)   # rows 0, 2, 4 are one direction: the lowest id first
    ids, vals, _ = similar_ref(T, 2, ids=[4, 4, 1], metric='dot')
    assert ids.tolist() == [[2, 0], [2, 0], [3, 0]] and vals.tolist() == [[1.5, 0.5], [1.5, 0.5], [2.0, 0.0]]
    ids, _, _ = similar_ref(T, 1, queries=T[[3]])
    assert ids.tolist() == [[3]]   # nothing is excluded for queries


def test_oracle_zero_row_has_cosine_zero_with_everything():
    T = np.array([[1.0, 2.0], [0.0, 0.0], [-1.0, 0.5], [4.0, 4.0]])
    unit, norms = unit_rows_ref(T)
    assert not unit[1].any() and norms[1] == 0 and np.allclose(norms, [np.sqrt(5), 0, np.sqrt(1.25), np.sqrt(32)])
    S = similarities(T)
    assert not S[1].any() and not S[:, 1].any() and np.isfinite(S).all()
    ids, vals, _ = similar_ref(T, 3)
    assert ids[1].tolist() == [0, 2, 3] and not vals[1].any()   # the lowest ids other than itself
    big, small = unit_rows_ref(np.array([[3e300, 4e300], [3e-300, 4e-300]]))
    assert np.allclose(big, [[0.6, 0.8], [0.6, 0.8]]) and np.allclose(small, [5e300, 5e-300], rtol=1e-12)


# ------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_bound_and_built():
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    declared = set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    lib = _lib.load_library()
    for name in NEW_ENTRY_POINTS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == 10
    assert 'non-finite' in header   # the header says what is outside the contract
    make = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS :=.*\btmf_unit\.hip\b', make, re.M)
    assert lib.tmf_version() == _lib.MIN_LIB_VERSION == 203


@pytest.mark.parametrize('name', NEW_ENTRY_POINTS)
def test_argument_checks_return_before_any_launch(name):
    """Null pointers throughout: a call that got as far as a launch would fail differently (or crash)."""
    from teamoflow_amd import _lib
    lib = _lib.load_library()
    fn = getattr(lib, name)
    per16 = 8 if name.endswith('bf16') else 4

    def call(r, ldt, ldo, q=5, n_rows=10):
        return fn(None, n_rows, r, ldt, None, q, None, ldo, None, None)
    assert call(0, 8, 8) != 0                       # r = 0
    assert call(1025, 1032, 1032) != 0              # r = 1025
    assert call(8, 8, 10) != 0                      # ldo % 4 != 0
    assert call(16, 8, 16) != 0                     # ldt < r
    assert call(8, 8, 4) != 0                       # ldo < r
    assert call(8, 8 + per16 // 2, 8) != 0          # rows that are not 16-byte aligned
    assert call(8, 8, 8, q=-1) != 0
    assert call(8, 8, 8, q=5) != 0                  # in range, but no table
    assert b'required' in lib.tmf_last_error()
    assert call(8, 8, 8, q=11) != 0                 # ids == NULL: q <= n_rows
    assert call(8, 8, 8, q=0) == 0                  # nothing to do: no launch
    assert call(1024, 1024, 1024, q=0, n_rows=0) == 0


# ------------------------------------------------------------------ the model's refusals
@pytest.fixture()
def model():
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    g = torch.Generator().manual_seed(0)
    m = MatrixFactorization(4)
    m.user_embedding, m.item_embedding = torch.randn(6, 4, generator=g), torch.randn(9, 4, generator=g)
    return m


def test_model_refusals_need_no_engine(model, monkeypatch):
    from teamoflow_amd import _lib

    def no_engine():
        raise AssertionError('the engine was asked for before the arguments were checked')
    monkeypatch.setattr(_lib, 'get', no_engine)
    for call, n in ((model.similar_items, 9), (model.similar_users, 6)):
        with pytest.raises(ValueError, match='metric'):
            call(metric='euclid')
        with pytest.raises(ValueError, match=rf'\[1, {n - 1}\]'):
            call(k=0)
        with pytest.raises(ValueError, match=rf'\[1, {n - 1}\]'):
            call(k=n)                                   # a row never returns itself: at most n - 1
        with pytest.raises(ValueError, match=rf'\[1, {n}\]'):
            call(k=n + 1, include_self=True)
        with pytest.raises(ValueError, match=rf'\[1, {n}\]'):
            call(k=n + 1, queries=torch.zeros(2, 4))
        with pytest.raises(IndexError):
            call(-1)
        with pytest.raises(IndexError):
            call(n)
        with pytest.raises(IndexError):
            call([0, n, 1])
        with pytest.raises(IndexError):
            call(np.array([2, -1]))
        with pytest.raises(ValueError, match='not both'):
            call([0, 1], queries=torch.zeros(2, 4))
        with pytest.raises(ValueError, match='queries'):
            call(queries=torch.zeros(2, 5))             # another width
        with pytest.raises(ValueError, match='queries'):
            call(queries=np.zeros(4, np.float32))       # not [q, r]
    # what passes the checks reaches the engine (and only then)
    for kw in (dict(k=8), dict(k=9, include_self=True), dict(items=[3, 3, 0], k=1), dict(queries=np.zeros((2, 4), np.float32), k=9)):
        with pytest.raises(AssertionError, match='engine'):
            model.similar_items(**kw)


def test_item_sharded_fit_is_refused(model):
    model._sharded_epoch = types.SimpleNamespace(world=2)
    for call in (model.similar_items, model.similar_users):
        with pytest.raises(NotImplementedError, match='sharded'):
            call(k=2)
    model._sharded_epoch = types.SimpleNamespace(world=1)   # one rank holds every row
    with pytest.raises(ValueError, match='metric'):
        model.similar_items(metric='l2')
