"""CPU side of the sparse DCG path (no GPU): the graded test-table CSR (order, duplicate sums, zero drop, gains), the discounts, the
argument checks of dcg_at_k / idcg_at_k / ndcg_at_k that run before anything is launched, and the C ABI of tmf_dcg_idcg_f32."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_graded_csr_sorts_sums_duplicates_and_drops_zeros():
    from teamoflow_amd import _ops
    from teamoflow_amd.mf.sparse import SparseInteractions
    idx = np.array([[2, 3], [0, 5], [2, 3], [0, 1], [1, 4], [1, 4], [3, 0], [3, 2], [0, 5], [0, 5]])
    val = np.array([1.0, 2.0, 0.5, -1.0, 1.0, -1.0, 3.0, 0.0, 0.25, 0.25], np.float32)
    A = SparseInteractions(idx, val, (5, 6), device='cpu')
    t = _ops.graded_csr(A, 5, 6)
    assert t.rowptr.tolist() == [0, 2, 2, 3, 4, 4]            # (1, 4) sums to 0 and (3, 2) is 0: dropped; user 4 has nothing
    assert t.cols.tolist() == [1, 5, 3, 0]
    assert t.cols.dtype == torch.int32 and t.gain.dtype == torch.float32 and t.rowptr.dtype == torch.int64
    a = torch.tensor([-1.0, 2.5, 1.5, 3.0])
    assert torch.equal(t.gain, torch.pow(2.0, a) - 1.0)
    assert t.stored().tolist() == [2, 0, 1, 1, 0]
    d = _ops.graded_csr(A.to_dense(), 5, 6)                  # the dense form of the same table
    for x, y in ((t.rowptr, d.rowptr), (t.cols, d.cols), (t.gain, d.gain)):
        assert torch.equal(x, y)


@pytest.mark.parametrize('seed', range(4))
def test_graded_csr_matches_to_dense(seed):
    from teamoflow_amd import _ops
    from teamoflow_amd.mf.sparse import SparseInteractions
    rng = np.random.default_rng(seed)
    m, n, nnz = 17, 29, 300
    idx = np.stack([rng.integers(0, m, nnz), rng.integers(0, n, nnz)], 1)   # many duplicates, any order
    val = rng.choice(np.array([-2, -1, -0.5, 0, 0.5, 1, 2, 3], np.float32), nnz)
    A = SparseInteractions(idx, val, (m, n), device='cpu')
    D = A.to_dense()
    t = _ops.graded_csr(A, m, n)
    want = torch.nonzero(D)
    P = int(t.rowptr[-1])
    assert t.cols.numel() == max(P, 1)
    got = torch.stack([_ops._csr_rows(t.rowptr), t.cols[:P].long()], 1)
    assert torch.equal(got, want)
    assert torch.equal(t.gain[:P], torch.pow(2.0, D[want[:, 0], want[:, 1]]) - 1.0)


def test_graded_csr_empty_table():
    from teamoflow_amd import _ops
    t = _ops.graded_csr(torch.zeros(4, 3), 4, 3)
    assert t.rowptr.tolist() == [0] * 5 and t.cols.numel() == 1 and t.gain.numel() == 1


def test_discounts_are_the_dense_expression():
    from teamoflow_amd import _ops
    k = 70
    d = _ops.dcg_discounts(k, torch.device('cpu'))
    want = torch.log1p(torch.arange(1, 301, dtype=torch.float32)) / float(np.log(np.float32(2.0)))
    assert torch.equal(d, want[:k])


def cpu_model(m, n, r=4):
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    model = MatrixFactorization(r)
    model.user_embedding, model.item_embedding = torch.zeros(m, r), torch.zeros(n, r)
    return model


def test_argument_errors_before_launch():
    """Raised on CPU tables (no GPU needed): every check runs before the engine is touched."""
    from teamoflow_amd.mf.sparse import SparseInteractions
    m, n = 6, 9
    model = cpu_model(m, n)
    A = SparseInteractions(np.array([[0, 1], [0, 2], [3, 8], [5, 0], [5, 0]]), np.array([1.0, 2.0, 1.0, -1.0, 3.0], np.float32), (m, n),
                           device='cpu')
    ex = np.zeros((m, n), np.float32)
    ex[0, 2] = ex[5, 0] = ex[4, 4] = 1.0
    for fn in (model.dcg_at_k, model.idcg_at_k, model.ndcg_at_k):
        with pytest.raises(ValueError, match=r'^2 \(user, item\) pairs'):
            fn(A, 3, exclude=torch.as_tensor(ex))
        with pytest.raises(ValueError, match=r'^2 \(user, item\) pairs'):
            fn(A.to_dense(), 3, exclude=SparseInteractions(np.argwhere(ex), np.ones(3, np.float32), (m, n), device='cpu'))
        with pytest.raises(IndexError):
            fn(SparseInteractions(np.array([[0, 9]]), np.array([1.0], np.float32), (m, n), device='cpu'), 3)
        with pytest.raises(IndexError):
            fn(SparseInteractions(np.array([[-1, 0]]), np.array([1.0], np.float32), (m, n), device='cpu'), 3)
        with pytest.raises(IndexError):
            fn(A, 3, exclude=SparseInteractions(np.array([[6, 0]]), np.array([1.0], np.float32), (7, 9), device='cpu'))
        with pytest.raises(ValueError):
            fn(SparseInteractions(np.array([[0, 1]]), np.array([1.0], np.float32), (m, n + 1), device='cpu'), 3)
        with pytest.raises(ValueError):
            fn(torch.ones(m, n - 1), 3, exclude=torch.as_tensor(ex))
        with pytest.raises(ValueError):
            fn(A, 0)
        with pytest.raises(ValueError):
            fn(A, -2, exclude=torch.as_tensor(ex))
    # a test entry whose values sum to 0 is no entry, so it cannot clash with an exclusion
    B = SparseInteractions(np.array([[0, 2], [0, 2], [1, 1]]), np.array([1.0, -1.0, 2.0], np.float32), (m, n), device='cpu')
    ex2 = np.zeros((m, n), np.float32)
    ex2[0, 2] = 1.0
    from teamoflow_amd import _ops
    t = _ops.graded_csr(B, m, n)
    assert _ops.overlap_count(t, _ops.build_exclusion(torch.as_tensor(ex2), m, n), m, n) == 0


def test_item_sharded_fit_is_refused():
    from teamoflow_amd.mf.sparse import SparseInteractions

    class Epoch:
        world = 2

    model = cpu_model(4, 5)
    model._sharded_epoch = Epoch()
    A = SparseInteractions(np.array([[0, 1]]), np.array([1.0], np.float32), (4, 5), device='cpu')
    for fn in (model.dcg_at_k, model.idcg_at_k, model.ndcg_at_k):
        with pytest.raises(NotImplementedError):
            fn(A, 3)


def test_entry_point_is_declared_bound_and_built():
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    assert 'tmf_dcg_idcg_f32' in set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    assert 'tmf_dcg_idcg_f32' in _lib.SIGNATURES
    make = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS :=.*\btmf_ndcg\.hip\b', make, re.M)
    lib = _lib.load_library()
    assert hasattr(lib, 'tmf_dcg_idcg_f32')
    assert lib.tmf_version() == _lib.MIN_LIB_VERSION
    # argument checks of the entry point itself (no launch: they fail first, or there is nothing to do)
    assert lib.tmf_dcg_idcg_f32(None, None, None, 4, 10, None, 0, 0, None, None, None, None, None) != 0     # k < 1
    assert lib.tmf_dcg_idcg_f32(None, None, None, 0, 10, None, 0, 5, None, None, None, None, None) == 0     # m = 0
    assert lib.tmf_dcg_idcg_f32(None, None, None, 4, 10, None, 0, 5, None, None, None, None, None) == 0     # no output asked
