"""CPU tests of the exclusion CSR (_ops.build_exclusion: sorted, de-duplicated rows, zero values dropped, ids checked) and of the
argument checks in front of the ranking calls with ``exclude=``."""
import numpy as np
import pytest
import torch


def csr_rows(ex):
    rp, cols = ex.rowptr.numpy(), ex.cols.numpy()
    return [cols[rp[u]:rp[u + 1]].tolist() for u in range(ex.n_users)]


def test_sparse_input_is_sorted_deduplicated_and_drops_zeros():
    from teamoflow_amd._ops import build_exclusion
    from teamoflow_amd.mf.sparse import SparseInteractions
    idx = [[2, 7], [0, 3], [0, 1], [2, 0], [0, 3], [1, 4], [2, 7], [3, 2]]
    val = [1.0, 2.0, 1.0, -1.0, 1.0, 0.0, 5.0, 0.0]
    ex = build_exclusion(SparseInteractions(idx, val, (4, 8), device='cpu'), 4, 8)
    assert csr_rows(ex) == [[1, 3], [], [0, 7], []]
    assert ex.rowptr.dtype == torch.int64 and ex.cols.dtype == torch.int32
    assert ex.rowptr.tolist() == [0, 2, 2, 4, 4]


def test_dense_input_and_equivalence_with_sparse():
    from teamoflow_amd._ops import build_exclusion
    from teamoflow_amd.mf.sparse import SparseInteractions
    rng = np.random.default_rng(0)
    A = (rng.random((30, 50)) < 0.2) * rng.integers(-2, 3, (30, 50))
    a = build_exclusion(torch.tensor(A), 30, 50)
    b = build_exclusion(A, 30, 50)   # NumPy works too
    c = build_exclusion(SparseInteractions.from_dense(A, device='cpu'), 30, 50)
    want = [np.nonzero(A[u])[0].tolist() for u in range(30)]
    assert csr_rows(a) == csr_rows(b) == csr_rows(c) == want


def test_empty_exclusion():
    from teamoflow_amd._ops import build_exclusion
    ex = build_exclusion(torch.zeros(3, 5), 3, 5)
    assert ex.rowptr.tolist() == [0, 0, 0, 0] and csr_rows(ex) == [[], [], []]
    assert ex.cols.numel() >= 1   # a valid pointer for the kernels


@pytest.mark.parametrize('bad', [[[0, 5]], [[0, -1]], [[3, 0]], [[-1, 2]]])
def test_out_of_range_ids_raise_index_error(bad):
    from teamoflow_amd._ops import build_exclusion
    from teamoflow_amd.mf.sparse import SparseInteractions
    with pytest.raises(IndexError):
        build_exclusion(SparseInteractions(bad, [1.0], (3, 5), device='cpu'), 3, 5)


def test_dense_table_wider_than_the_catalog():
    from teamoflow_amd._ops import build_exclusion
    A = torch.zeros(2, 7)
    build_exclusion(A, 2, 5)        # zeros past the catalog are not pairs
    A[1, 6] = 1.0
    with pytest.raises(IndexError):
        build_exclusion(A, 2, 5)
    with pytest.raises(ValueError):
        build_exclusion(torch.ones(5), 1, 5)


def test_views_shift_users_and_items():
    from teamoflow_amd._ops import build_exclusion
    A = torch.zeros(4, 6)
    A[2, 3] = 1
    ex = build_exclusion(A, 4, 6)
    v = ex.shifted(2, 4).shifted(1, -1)
    assert (v.user_base, v.item_base) == (3, 3) and v.rowptr is ex.rowptr
    assert build_exclusion(ex.shifted(1), 3, 2) is not None   # a window: its own item count, users must fit
    with pytest.raises(IndexError):
        build_exclusion(ex.shifted(2), 3, 6)


def test_exclude_is_keyword_only_on_the_public_api():
    import inspect
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    for name in ('recall_at_k', 'precision_at_k', 'f1_at_k', 'retrieve_user_recs'):
        p = inspect.signature(getattr(MatrixFactorization, name)).parameters['exclude']
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, name
    from teamoflow_amd import _ops, dist
    for fn in (_ops.predict_topk, _ops.topk_stable, dist.sharded_top_items):
        assert inspect.signature(fn).parameters['exclude'].default is None


@pytest.mark.parametrize('shuffled', [False, True])
@pytest.mark.parametrize('filled', [False, True])
def test_hits_and_relevant_on_a_sparse_table(shuffled, filled):
    """The one body of _hits_and_relevant over a SparseInteractions test table on CPU tensors, the ranking replaced by a fixed
    list: full lists (no exclusion) and lists with -1 in trailing slots (one row entirely -1), for a row-major table (the
    already-sorted shortcut) and a shuffled one with duplicates (of negative entries) and explicit zeros, against a NumPy count over
    the dense form."""
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions
    rng = np.random.default_rng(5)
    m, n, k = 9, 14, 5
    D = ((rng.random((m, n)) < 0.35) * rng.integers(-2, 4, (m, n))).astype(np.float32)
    D[4] = 0                                            # a user without entries
    D[2, 0], D[6, 0], D[7, 0] = 2, -1, 3                # item 0 stands in for the -1 slots of these rows: only the mask keeps it from counting
    idx = np.argwhere(D != 0)
    val = D[idx[:, 0], idx[:, 1]]
    if shuffled:
        zeros = np.argwhere(D == 0)[::7]                # explicit zeros: stored, but neither hits nor relevant
        neg = idx[val < 0]                              # duplicates of negative entries: hits, never relevant ("relevant" counts the
        assert len(neg) > 3 and len(zeros) > 3          # STORED entries > 0, so a repeated positive would count once per copy)
        idx = np.concatenate([idx, neg, neg[::2], zeros])
        val = np.concatenate([val, D[neg[:, 0], neg[:, 1]], D[neg[::2, 0], neg[::2, 1]], np.zeros(len(zeros), np.float32)])
        perm = rng.permutation(len(idx))
        idx, val = idx[perm], val[perm]
    A = SparseInteractions(idx, val, (m, n), device='cpu')
    assert np.array_equal(A.to_dense().numpy() != 0, D != 0) and np.array_equal(A.to_dense().numpy() > 0, D > 0)
    top = np.stack([rng.permutation(n)[:k] for _ in range(m)]).astype(np.int32)
    exclude = None
    if filled:
        top[2, 3:] = -1
        top[6, 1:] = -1
        top[7, :] = -1                                  # a user with no eligible item at all
        exclude = torch.zeros(m, n)                     # any exclusion: the ranking is the fixed list
    model = MatrixFactorization(4)
    model.user_embedding, model.item_embedding = torch.zeros(m, 4), torch.zeros(n, 4)
    seen = []
    model._top_items = lambda k_, clamp, users=None, exclude=None: (seen.append((k_, clamp, exclude)), torch.tensor(top))[1]
    hits, relevant = model._hits_and_relevant(A, k, exclude=exclude)
    assert seen == [(k, True, exclude)]
    want_hits = [sum(1 for j in top[u] if j >= 0 and D[u, j] != 0) for u in range(m)]
    assert hits.dtype == torch.float32 and relevant.dtype == torch.float32
    assert hits.tolist() == want_hits
    assert relevant.tolist() == (D > 0).sum(axis=1).tolist()
    assert filled or sum(want_hits) > 0                 # the lists do meet the table
    if filled:
        assert all(D[u, 0] != 0 and 0 not in top[u] for u in (2, 6, 7))   # every fill slot points at a stored non-zero
        assert hits[7] == 0 and relevant[7] == (D[7] > 0).sum()
