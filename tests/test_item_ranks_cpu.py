"""CPU side of the full-catalog ranks (no GPU): AUC / reciprocal rank from ranks against brute-force pair counting, the virtual rows of
the rank kernels, the argument checks that run before anything is launched, and the C ABI of the new entry points."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

NEW_ENTRY_POINTS = ('tmf_pair_scores_f32', 'tmf_pair_scores_split', 'tmf_item_ranks_f32_supported', 'tmf_item_ranks_split_supported',
                    'tmf_item_ranks_split_workspace_bytes', 'tmf_item_ranks_f32', 'tmf_item_ranks_split', 'tmf_rank_count_rows_f32')


def brute_force(scores, pos, excl):
    """Per user: ranks of the positives (order value desc, index asc over the eligible items), AUC by counting (positive, negative)
    pairs, 1 / (1 + best rank)."""
    m, n = scores.shape
    ids = np.arange(n)
    ranks, auc, rr = [], np.full(m, np.nan), np.full(m, 1.0 / (1 + n))
    for u in range(m):
        s, elig = scores[u], ~excl[u]
        P = np.nonzero(pos[u])[0]
        N = np.nonzero(elig & ~pos[u])[0]
        rk = [int(np.count_nonzero(elig & ((s > s[i]) | ((s == s[i]) & (ids < i))))) for i in P]
        ranks += rk
        if P.size:
            rr[u] = 1.0 / (1 + min(rk))
            ordered = sum(int(np.count_nonzero((s[N] > s[i]) | ((s[N] == s[i]) & (N < i)))) for i in P)
            auc[u] = 1.0 if N.size == 0 else 1.0 - ordered / (P.size * N.size)
    return np.array(ranks, np.int64), auc, rr


@pytest.mark.parametrize('seed', range(6))
def test_auc_and_reciprocal_rank_from_ranks(seed):
    from teamoflow_amd import _ops
    rng = np.random.default_rng(seed)
    m, n = 23, 37
    scores = rng.integers(-4, 5, (m, n)).astype(np.float64)   # many ties
    pos = rng.random((m, n)) < rng.uniform(0.05, 0.5)
    excl = (rng.random((m, n)) < 0.2) & ~pos
    pos[0] = False                      # P = 0
    pos[1] = True                       # N = 0 (nothing excluded)
    excl[1] = False
    pos[2] = False
    pos[2, 4] = True                    # N = 0: everything else excluded
    excl[2] = True
    excl[2, 4] = False
    ranks, auc, rr = brute_force(scores, pos, excl)
    rowptr = torch.zeros(m + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.as_tensor(pos.sum(axis=1)), 0)
    got_auc, counts = _ops.auc_from_ranks(rowptr, torch.as_tensor(ranks), n, torch.as_tensor(excl.sum(axis=1)))
    got_rr, _ = _ops.reciprocal_rank_from_ranks(rowptr, torch.as_tensor(ranks), n)
    has = pos.any(axis=1)
    assert np.array_equal(counts.numpy(), pos.sum(axis=1))
    assert got_auc.dtype == torch.float32 and got_rr.dtype == torch.float32
    np.testing.assert_allclose(got_auc.numpy()[has], auc[has], rtol=0, atol=1e-7)
    assert np.isnan(got_auc.numpy()[~has]).all()
    assert got_auc[1] == 1.0 and got_auc[2] == 1.0
    np.testing.assert_allclose(got_rr.numpy(), rr, rtol=1e-7)


@pytest.mark.parametrize('P', [0, 1, 16, 17, 1000])
def test_virtual_rows(P):
    from teamoflow_amd import _ops
    pc = _ops.RANK_ROW_PAIRS
    counts = torch.tensor([3, P, 0, P, 1], dtype=torch.int64)
    rowptr = torch.zeros(6, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(counts, 0)
    user, begin, count = _ops.virtual_rows(rowptr)
    assert user.dtype == torch.int32 and begin.dtype == torch.int64 and count.dtype == torch.int32
    want = []
    for u, c in enumerate(counts.tolist()):
        for b in range(0, c, pc):
            want.append((u, int(rowptr[u]) + b, min(pc, c - b)))
    assert list(zip(user.tolist(), begin.tolist(), count.tolist())) == want
    assert (count >= 1).all() and (count <= pc).all()
    per_user = torch.bincount(user.long(), minlength=5)
    assert per_user.tolist() == [(c + pc - 1) // pc for c in counts.tolist()]


def test_overlap_and_range_errors_before_launch():
    """Raised on CPU tables (no GPU needed): the checks run before the engine is touched."""
    from teamoflow_amd import _ops
    from teamoflow_amd.mf.sparse import SparseInteractions
    U, V = torch.zeros(6, 4), torch.zeros(9, 4)
    A = SparseInteractions(np.array([[0, 1], [0, 2], [3, 8], [5, 0], [5, 0]]), np.array([1.0, 2.0, 1.0, 1.0, 1.0], np.float32), (6, 9))
    ex = np.zeros((6, 9), np.float32)
    ex[0, 2] = ex[5, 0] = ex[4, 4] = 1.0
    with pytest.raises(ValueError, match=r'^2 \(user, item\) pairs'):
        _ops.item_ranks(U, V, A, exclude=torch.as_tensor(ex))
    with pytest.raises(IndexError):
        _ops.item_ranks(U, V, SparseInteractions(np.array([[0, 9]]), np.array([1.0], np.float32), (6, 10)))
    with pytest.raises(IndexError):
        _ops.item_ranks(U, V, A, exclude=SparseInteractions(np.array([[6, 0]]), np.array([1.0], np.float32), (7, 9)))
    with pytest.raises(ValueError):
        _ops.item_ranks(U, V, torch.ones(5, 9))   # a dense table of the wrong shape
    # entries <= 0 are not positives (recall_at_k's "relevant"), so they cannot clash with an exclusion
    B = SparseInteractions(np.array([[0, 2], [1, 1]]), np.array([0.0, -1.0], np.float32), (6, 9))
    pos = _ops.positive_pairs(B, 6, 9)
    assert int(pos.rowptr[-1]) == 0
    assert _ops.overlap_count(pos, _ops.build_exclusion(torch.as_tensor(ex), 6, 9), 6, 9) == 0


def test_positive_pairs_and_overlap_count():
    from teamoflow_amd import _ops
    rng = np.random.default_rng(1)
    D = rng.integers(-1, 3, (7, 11)).astype(np.float32)
    pos = _ops.positive_pairs(torch.as_tensor(D), 7, 11)
    want = np.argwhere(D > 0)
    P = int(pos.rowptr[-1])
    got = np.stack([_ops._csr_rows(pos.rowptr).numpy(), pos.cols[:P].numpy()], 1)
    assert np.array_equal(got, want)
    ex = (rng.random((7, 11)) < 0.3)
    ec = _ops.build_exclusion(torch.as_tensor(ex), 7, 11)
    assert _ops.overlap_count(pos, ec, 7, 11) == int(np.count_nonzero(ex & (D > 0)))
    assert _ops.exclusion_counts(ec, 7, 11).tolist() == ex.sum(axis=1).tolist()


def test_new_entry_points_are_declared_and_bound():
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    declared = set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    assert re.search(r'#define TMF_RANK_ROW_PAIRS (\d+)', header).group(1) == '16'
    from teamoflow_amd import _ops
    assert _ops.RANK_ROW_PAIRS == 16
    lib = _lib.load_library()
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert lib.tmf_version() == _lib.MIN_LIB_VERSION
    assert lib.tmf_item_ranks_split_supported(256) == 1 and lib.tmf_item_ranks_split_supported(257) == 0
    assert lib.tmf_item_ranks_f32_supported(1) == 1 and lib.tmf_item_ranks_f32_supported(300) == 0
    assert lib.tmf_item_ranks_split_workspace_bytes(1000, 100) == lib.tmf_predict_topk_split_workspace_bytes(1000, 100)
    assert lib.tmf_item_ranks_split_workspace_bytes(1000, 300) == 0
