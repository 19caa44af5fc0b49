"""Sparse, exclude-aware dcg_at_k / idcg_at_k / ndcg_at_k (top-k of the fused kernels + tmf_dcg_idcg_f32): the sparse path against the
dense full-sort path and oracle.dense_ref on tables whose fp32 scores are exact; exclude= against an fp64 NumPy oracle; DCG against
the retrieve_user_recs lists on every arithmetic; IDCG of heavy rows against a NumPy sort with the same fp32 sums; determinism, errors
and the C4 shape."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from teamoflow_amd import _lib, _ops
    _lib.get()
    return _ops


def model_of(U, V, arithmetic=None):
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    model = MatrixFactorization(U.shape[1])
    model.user_embedding, model.item_embedding = U.cuda(), V.cuda()
    if arithmetic is not None:
        model.predict_arithmetic = arithmetic
    return model


def dyadic_tables(m, n, r, seed):
    """Factors in multiples of 1/4 with |x| <= 1: every fp32 score is exact, and exact ties are common."""
    rng = np.random.default_rng(seed)
    return (torch.as_tensor(rng.integers(-4, 5, (m, r)).astype(np.float32) / 4),
            torch.as_tensor(rng.integers(-4, 5, (n, r)).astype(np.float32) / 4))


GRADES = np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 5.0], np.float32)


def graded_table(m, n, seed, density=0.05):
    """Dense graded table (negatives included): users 0-2 have no entries, users 3-4 only negative ones, user 5 has entries on more
    than 64 items."""
    rng = np.random.default_rng(seed)
    D = np.where(rng.random((m, n)) < density, rng.choice(GRADES, (m, n)), 0.0).astype(np.float32)
    D[:3] = 0.0
    D[3:5] = np.where(rng.random((2, n)) < 0.1, -rng.choice([0.5, 1.0, 2.0], (2, n)), 0.0)
    D[5, rng.choice(n, min(n, 100), replace=False)] = rng.choice(GRADES, min(n, 100))
    return D


def sparse_with_duplicates(D, seed):
    """SparseInteractions whose to_dense() is D: some entries split into two exact halves, some (user, item) pairs stored as +1 and -1
    (summing to 0, i.e. no entry), in shuffled order."""
    from teamoflow_amd.mf.sparse import SparseInteractions
    rng = np.random.default_rng(seed)
    idx = np.argwhere(D != 0)
    val = D[idx[:, 0], idx[:, 1]]
    split = rng.random(len(idx)) < 0.3
    zeros = np.argwhere(D == 0)
    zeros = zeros[rng.choice(len(zeros), min(len(zeros), 40), replace=False)]
    all_idx = np.concatenate([idx, idx[split], zeros, zeros])
    all_val = np.concatenate([np.where(split, val / 2, val), val[split] / 2, np.ones(len(zeros)), -np.ones(len(zeros))]).astype(np.float32)
    perm = rng.permutation(len(all_idx))
    A = SparseInteractions(all_idx[perm], all_val[perm], D.shape)
    assert torch.equal(A.to_dense().cpu(), torch.as_tensor(D))
    return A


def oracle(S, D, excl, k):
    """fp64 DCG / IDCG: eligible items ranked by (value desc, id asc), gains 2^a - 1, discounts log2(j + 2), zeros of eligible items."""
    m, n = S.shape
    kk = min(k, n)
    disc = np.log2(np.arange(kk) + 2.0)
    G = np.power(2.0, D.astype(np.float64)) - 1.0
    dcg, idcg = np.zeros(m), np.zeros(m)
    for u in range(m):
        ids = np.nonzero(~excl[u])[0]
        top = ids[np.lexsort((ids, -S[u, ids]))][:kk]
        dcg[u] = (G[u, top] / disc[:top.size]).sum()
        g = np.sort(G[u, ids])[::-1][:kk]
        idcg[u] = (g / disc[:g.size]).sum()
    return dcg, idcg


def close(got, want, rtol=1e-6, atol=1e-6):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    np.testing.assert_allclose(got.astype(np.float64), np.asarray(want, np.float64), rtol=rtol, atol=atol)


@pytest.mark.parametrize('k', [1, 10, 64, 65, 300])
def test_sparse_path_equals_dense_path(ops, k):
    from oracle import dense_ref as DR
    m, n, r = 150, 300, 16
    U, V = dyadic_tables(m, n, r, seed=k)
    D = graded_table(m, n, seed=k)
    A = sparse_with_duplicates(D, seed=k)
    model = model_of(U, V)
    Dd = torch.as_tensor(D).cuda()
    for name in ('dcg_at_k', 'idcg_at_k'):
        dense = getattr(model, name)(Dd, k)
        sparse = getattr(model, name)(A, k)
        assert sparse.dtype == torch.float32 and sparse.device == Dd.device and sparse.shape == (m,)
        close(sparse, dense.cpu().numpy())
    close(model.dcg_at_k(A, k), DR.dcg_at_k_dense(U.numpy(), V.numpy(), D, k))
    close(model.idcg_at_k(A, k), DR.dcg_at_k_dense(U.numpy(), V.numpy(), D, k, ideal=True))
    for preserve in (False, True):
        dense = model.ndcg_at_k(Dd, k, preserve_rows=preserve).cpu().numpy()
        sparse = model.ndcg_at_k(A, k, preserve_rows=preserve).cpu().numpy()
        assert sparse.shape == dense.shape
        assert np.array_equal(np.isnan(sparse), np.isnan(dense)) and np.array_equal(np.isinf(sparse), np.isinf(dense))
        fin = np.isfinite(dense)
        close(sparse[fin], dense[fin])
        ref = DR.ndcg_at_k_dense(U.numpy(), V.numpy(), D, k, preserve_rows=preserve)
        close(sparse[fin], ref[fin])
    S = U.double().numpy() @ V.double().numpy().T
    dcg, idcg = oracle(S, D, np.zeros_like(D, dtype=bool), k)
    close(model.dcg_at_k(A, k), dcg)
    close(model.idcg_at_k(A, k), idcg)


def excl_set(D, seed, crowd=()):
    """Random exclusions that never hit a test entry; users in `crowd` keep only a few eligible items (fewer than k)."""
    rng = np.random.default_rng(seed)
    n = D.shape[1]
    ex = (rng.random(D.shape) < 0.2) & (D == 0)
    for u in crowd:
        ex[u] = D[u] == 0
        keep = rng.choice(np.nonzero(D[u] == 0)[0], 3, replace=False)
        ex[u, keep] = False
    assert not (ex & (D != 0)).any()
    return ex


@pytest.mark.parametrize('k', [1, 10, 40, 64, 65, 100])
@pytest.mark.parametrize('form', ['sparse', 'dense'])
def test_exclude_against_fp64_oracle(ops, k, form):
    from teamoflow_amd.mf.sparse import SparseInteractions
    m, n, r = 130, 257, 24
    U, V = dyadic_tables(m, n, r, seed=100 + k)
    D = graded_table(m, n, seed=200 + k, density=0.04)
    D[7] = 0.0
    D[7, :5] = [3.0, -1.0, 0.5, 2.0, 1.0]
    D[8] = 0.0
    D[8, 10:14] = [-1.0, -2.0, -0.5, -1.0]   # only negative gains, few eligible items: the negatives enter the ideal list
    ex = excl_set(D, seed=k, crowd=(7, 8, 9))
    S = U.double().numpy() @ V.double().numpy().T
    want_dcg, want_idcg = oracle(S, D, ex, k)
    model = model_of(U, V)
    if form == 'sparse':
        A, E = sparse_with_duplicates(D, seed=k), SparseInteractions(np.argwhere(ex), np.ones(int(ex.sum()), np.float32), ex.shape)
    else:
        A, E = torch.as_tensor(D).cuda(), torch.as_tensor(ex.astype(np.float32)).cuda()
    close(model.dcg_at_k(A, k, exclude=E), want_dcg)
    close(model.idcg_at_k(A, k, exclude=E), want_idcg)
    has = (D != 0).any(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        want = want_dcg / want_idcg
    got = model.ndcg_at_k(A, k, exclude=E).cpu().numpy()
    assert got.shape == (int(has.sum()),)
    fin = np.isfinite(want[has])
    close(got[fin], want[has][fin], rtol=1e-5)
    got_p = model.ndcg_at_k(A, k, preserve_rows=True, exclude=E).cpu().numpy()
    assert (got_p[~has] == 0).all()
    fin = np.isfinite(want)
    close(got_p[fin], want[fin], rtol=1e-5)
    # the crowded users have fewer eligible items than most k: their lists end in -1
    top = model.retrieve_user_recs(k=min(k, n), exclude=E)
    for u in (7, 8, 9):
        assert int((top[u] >= 0).sum()) == min(k, int((~ex[u]).sum()))


def dcg_from_lists(top, D, den):
    """float64 DCG from ranked lists (-1 = empty) with gains 2^a - 1."""
    G = np.power(2.0, D.astype(np.float64)) - 1.0
    valid = top >= 0
    g = np.where(valid, np.take_along_axis(G, np.where(valid, top, 0), 1), 0.0)
    return (g / den[None, :top.shape[1]]).sum(axis=1)


@pytest.mark.parametrize('arithmetic', ['fp32', 'split', 'half2', 'bf16'])
@pytest.mark.parametrize('k', [10, 32])
def test_dcg_follows_retrieve_user_recs_on_every_arithmetic(ops, arithmetic, k):
    from teamoflow_amd.mf.sparse import SparseInteractions
    m, n, r = 400, 3001, 64
    g = torch.Generator().manual_seed(k)
    U, V = torch.randn(m, r, generator=g), torch.randn(n, r, generator=g) * 0.3
    rng = np.random.default_rng(k)
    S = U.double().numpy() @ V.double().numpy().T
    best = np.argsort(-S, axis=1, kind='stable')[:, :40]
    D = np.where(rng.random((m, n)) < 0.01, rng.choice(GRADES, (m, n)), 0.0).astype(np.float32)
    for u in range(m):
        D[u, best[u, rng.choice(40, 6, replace=False)]] = rng.choice(GRADES[3:], 6)
    ex = (rng.random((m, n)) < 0.05) & (D == 0)
    A = SparseInteractions.from_dense(D)
    E = SparseInteractions(np.argwhere(ex), np.ones(int(ex.sum()), np.float32), ex.shape)
    if arithmetic == 'bf16':
        model = model_of(U.bfloat16(), V.bfloat16())
    else:
        model = model_of(U, V, arithmetic)
    den = np.log1p(np.arange(1, k + 1, dtype=np.float32)).astype(np.float64) / np.log(np.float32(2.0))
    for E_ in (None, E):
        top = model.retrieve_user_recs(k=k, exclude=E_)
        want = dcg_from_lists(top, D, den)
        close(model.dcg_at_k(A, k, exclude=E_), want, rtol=2e-6)
        assert np.count_nonzero(want) > m // 2


def row_idcg_fp32(gains, z, k, den):
    """IDCG of one row exactly as the kernel sums it: the k largest of gains + z zeros, fp32 terms, fp32 sum in slot order."""
    vals = np.concatenate([gains.astype(np.float32), np.zeros(int(min(z, k)), np.float32)])
    top = -np.sort(-vals, kind='stable')[:k]
    terms = top / den[:top.size]
    return np.cumsum(terms, dtype=np.float32)[-1] if top.size else np.float32(0)


@pytest.mark.parametrize('k', [10, 300, 2500])
def test_heavy_rows_idcg_equals_full_sort(ops, k):
    """User 1 stores 2^20 items, user 3 every item; integer grades (ties everywhere, also across the kernel's 1024-slot rounds) and
    a share of negative ones; with and without exclusions (the implicit zeros shrink)."""
    from teamoflow_amd.mf.sparse import SparseInteractions
    rng = np.random.default_rng(k)
    m, n, r = 6, (1 << 20) + 3000, 8
    heavy = {1: np.sort(rng.choice(n, 1 << 20, replace=False)), 3: np.arange(n)}
    rows, cols, vals = [], [], []
    for u, it in heavy.items():
        rows.append(np.full(it.size, u))
        cols.append(it)
        vals.append(rng.choice(np.array([-3, -2, -1, 1, 2, 3, 4, 5, 6], np.float32), it.size,
                               p=[.05, .05, .1, .4, .2, .1, .05, .03, .02]))
    cont = np.sort(rng.choice(n, 5000, replace=False))   # user 5: continuous grades, half of them negative
    rows.append(np.full(cont.size, 5))
    cols.append(cont)
    vals.append((rng.standard_normal(cont.size) * 2).astype(np.float32))
    rows.append(np.array([0, 0, 2, 4]))
    cols.append(np.array([5, 9, 7, 11]))
    vals.append(np.array([2.0, -1.0, 3.0, 1.0], np.float32))
    idx = np.stack([np.concatenate(rows), np.concatenate(cols)], 1)
    val = np.concatenate(vals)
    A = SparseInteractions(idx, val, (m, n))
    U = torch.randn(m, r)
    V = torch.randn(n, r)
    model = model_of(U, V)
    den = ops.dcg_discounts(k, torch.device('cuda')).cpu().numpy()
    ex_cols = np.setdiff1d(rng.choice(n, 5000, replace=False), heavy[1])   # excluded for user 1 only: never one of its test items
    E = SparseInteractions(np.stack([np.ones(ex_cols.size, np.int64), ex_cols], 1), np.ones(ex_cols.size, np.float32), (m, n))
    tab = ops.graded_csr(A, m, n, device=torch.device('cuda'))   # the gains as the device computes them (2^a - 1)
    rp, gains = tab.rowptr.cpu().numpy(), tab.gain.cpu().numpy()
    assert rp[2] - rp[1] == 1 << 20 and rp[4] - rp[3] == n
    for E_ in (None, E):
        got = model.idcg_at_k(A, k, exclude=E_).cpu().numpy()
        for u in range(m):
            g = gains[rp[u]:rp[u + 1]]
            z = n - g.size - (ex_cols.size if (E_ is not None and u == 1) else 0)
            want = row_idcg_fp32(g, z, min(k, n), den)
            assert got[u] == want, (u, got[u], want)
    assert got[3] > 0 and got[1] > 0


def test_repeated_calls_are_bit_identical(ops):
    from teamoflow_amd.mf.sparse import SparseInteractions
    m, n, r = 300, 5000, 32
    g = torch.Generator().manual_seed(3)
    U, V = torch.randn(m, r, generator=g), torch.randn(n, r, generator=g)
    rng = np.random.default_rng(3)
    D = np.where(rng.random((m, n)) < 0.02, rng.standard_normal((m, n)) * 2, 0.0).astype(np.float32)
    D[4, :3000] = rng.standard_normal(3000).astype(np.float32)   # a long row of distinct continuous gains
    A = SparseInteractions.from_dense(D)
    ex = (rng.random((m, n)) < 0.1) & (D == 0)
    E = torch.as_tensor(ex.astype(np.float32))
    model = model_of(U, V)
    for k in (10, 100):
        first = [model.ndcg_at_k(A, k, preserve_rows=True, exclude=E), model.dcg_at_k(A, k), model.idcg_at_k(A, k, exclude=E)]
        for _ in range(3):
            again = [model.ndcg_at_k(A, k, preserve_rows=True, exclude=E), model.dcg_at_k(A, k), model.idcg_at_k(A, k, exclude=E)]
            for x, y in zip(first, again):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_errors(ops):
    from teamoflow_amd.mf.sparse import SparseInteractions
    m, n = 10, 20
    U, V = dyadic_tables(m, n, 4, seed=1)
    model = model_of(U, V)
    A = SparseInteractions(np.array([[0, 1], [3, 4], [3, 5]]), np.array([1.0, 2.0, 3.0], np.float32), (m, n))
    ex = np.zeros((m, n), np.float32)
    ex[3, 4] = ex[3, 5] = ex[1, 1] = 1.0
    for fn in (model.dcg_at_k, model.idcg_at_k, model.ndcg_at_k):
        with pytest.raises(ValueError, match=r'^2 \(user, item\) pairs'):
            fn(A, 5, exclude=torch.as_tensor(ex))
        with pytest.raises(IndexError):
            fn(SparseInteractions(np.array([[0, 20]]), np.array([1.0], np.float32), (m, n)), 5)
        with pytest.raises(IndexError):
            fn(A, 5, exclude=SparseInteractions(np.array([[10, 0]]), np.array([1.0], np.float32), (m, n)))
        with pytest.raises(ValueError):
            fn(SparseInteractions(np.array([[0, 1]]), np.array([1.0], np.float32), (m, n + 1)), 5)
        with pytest.raises(ValueError):
            fn(torch.ones(m - 1, n), 5, exclude=torch.as_tensor(ex))
        with pytest.raises(ValueError):
            fn(A, 0)
    # k beyond the catalog: the reference's [:, :k] slice, i.e. k = n
    assert torch.equal(model.dcg_at_k(A, 50), model.dcg_at_k(A, n))


def test_c4_shape(ops):
    """1M users x 100K items, r = 128: 10 graded held-out items per user (values 1-5, 3 of the user's 20 best), ~1e8 excluded pairs,
    ndcg_at_k(k = 10) on the default arithmetic.  256 sampled users against the fp64 oracle where the top-11 eligible scores are
    separated by more than 1e-5 (tests/test_gpu_fullsize.py's rule); peak memory far below the 400 GB of a dense score matrix."""
    from teamoflow_amd.mf.sparse import SparseInteractions
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(13)
    m, n, r, k, per, held = 1_000_000, 100_000, 128, 10, 100, 10
    U = torch.randn(m, r, device=dev, generator=g) * 0.1
    V = torch.randn(n, r, device=dev, generator=g) * 0.1
    best = ops.predict_topk(U, V, 20, arithmetic='fp32').long()
    hp = torch.cat([best[:, :3], torch.randint(0, n, (m, held - 3), device=dev, generator=g)], 1)
    users = torch.arange(m, device=dev)
    grades = torch.randint(1, 6, (m * held,), device=dev, generator=g).float()
    A = SparseInteractions(torch.stack([users.repeat_interleave(held), hp.reshape(-1)], 1), grades, (m, n), device=dev)
    xi = torch.cat([best[:, 5:15], torch.randint(0, n, (m, per - 10), device=dev, generator=g)], 1).reshape(-1)
    keys = torch.unique(users.repeat_interleave(per) * n + xi)
    keys = keys[~torch.isin(keys, users.repeat_interleave(held) * n + hp.reshape(-1))]
    ex = ops.build_exclusion(SparseInteractions(torch.stack([keys // n, keys % n], 1), torch.ones(keys.numel(), device=dev), (m, n),
                                                device=dev), m, n)
    del best, xi, keys
    assert int(ex.cols.numel()) > 9e7
    model = model_of(U, V)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ndcg = model.ndcg_at_k(A, k, preserve_rows=True, exclude=ex)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    assert peak < 16 * 2 ** 30, peak
    assert ndcg.shape == (m,) and bool(torch.isfinite(ndcg).all())
    assert 0 < float(ndcg.mean()) < 1
    sample = torch.randperm(m, device=dev, generator=g)[:256].sort()[0]
    S = (U[sample].double() @ V.double().T).cpu().numpy()
    Dd = torch.zeros(256, n, device=dev)
    rows = torch.searchsorted(sample, users.repeat_interleave(held))
    hit = sample[rows.clamp(max=255)] == users.repeat_interleave(held)
    Dd.index_put_((rows[hit], hp.reshape(-1)[hit]), grades[hit], accumulate=True)
    Dd = Dd.cpu().numpy()
    rp, cols = ex.rowptr.cpu().numpy(), ex.cols.cpu().numpy()
    got = ndcg[sample].cpu().numpy()
    checked = 0
    for row, u in enumerate(sample.cpu().numpy()):
        elig = np.ones(n, bool)
        elig[cols[rp[u]:rp[u + 1]]] = False
        s = np.where(elig, S[row], -np.inf)
        top = np.argsort(-s, kind='stable')[:k + 1]
        v = s[top]
        if not ((v[:-1] - v[1:]) / max(abs(v[0]), 1e-30) > 1e-5).all():
            continue
        dcg, idcg = oracle(S[row:row + 1], Dd[row:row + 1], ~elig[None, :], k)
        assert abs(got[row] - dcg[0] / idcg[0]) <= 2e-6, (u, got[row], dcg[0] / idcg[0])
        checked += 1
    assert checked > 64, checked
