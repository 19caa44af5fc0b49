"""Full-catalog ranks of held-out pairs (_ops.item_ranks, MatrixFactorization.item_ranks / auc_score / reciprocal_rank): every form
(fused fp32 MFMA, fused three bf16 planes, the non-fused score blocks, bf16 tables) against a NumPy fp64 oracle that counts, for each
positive, the eligible items ordered before it (value desc, index asc); the invariant rank < k <=> membership in the fused top-k of the
same arithmetic; the fused fp32 ranks against the non-fused ones; the metrics; the C4 shape."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from teamoflow_amd import _lib, _ops
    _lib.get()
    return _ops


def oracle_ranks(U, V, pos, excl):
    """fp64 rank of every positive (row-major order of np.argwhere(pos)) among the items with excl == False."""
    S = np.asarray(U, np.float64) @ np.asarray(V, np.float64).T
    n = S.shape[1]
    out = []
    ids = np.arange(n)
    for u, i in np.argwhere(pos):
        s, e = S[u], ~excl[u]
        above = (s > s[i]) | ((s == s[i]) & (ids < i))
        out.append(int(np.count_nonzero(above & e)))
    return np.array(out, np.int64)


def int_tables(m, n, r, seed, lo=-3, hi=4):
    """Small-integer factors: every arithmetic is exact and ties are many."""
    rng = np.random.default_rng(seed)
    return rng.integers(lo, hi, (m, r)).astype(np.float32), rng.integers(lo, hi, (n, r)).astype(np.float32)


def edge_sets(m, n, seed):
    """Positives and exclusions of every awkward kind: random pairs; tile borders 63/64, 127/128, item 0 and n - 1; a user with
    1000 positives, one whose every item is a positive, one with all but one item excluded (its only positive on that item),
    users without positives."""
    rng = np.random.default_rng(seed)
    pos = rng.random((m, n)) < 0.03
    for c in (0, 63, 64, 127, 128, n - 1):
        pos[3::5, c] = True
    pos[4] = False
    pos[4, rng.choice(n, 1000, replace=False)] = True   # 1000 positives: 63 virtual rows
    pos[5] = True                                       # every item
    pos[6] = False
    pos[6, n // 3] = True
    pos[7:12] = False                                   # no positives
    pos[m - 1] = False
    excl = (rng.random((m, n)) < 0.08) & ~pos
    excl[5] = False
    excl[6] = True
    excl[6, n // 3] = False                             # all but one item excluded
    excl[8] = rng.random(n) < 0.5                       # exclusions of a user without positives
    return pos, excl


def dense(mask):
    return torch.as_tensor(mask.astype(np.float32))


def run(ops, U, V, pos, excl, arithmetic):
    return ops.item_ranks(U, V, dense(pos), exclude=None if excl is None else dense(excl), arithmetic=arithmetic).cpu().numpy()


@pytest.mark.parametrize('arithmetic,r', [('fp32', 30), ('fp32', 128), ('fp32', 200), ('split', 32), ('split', 128), ('split', 256),
                                          ('split', 30), ('fp32', 300), ('bf16', 50)])
@pytest.mark.parametrize('with_excl', [False, True])
def test_exact_ranks_on_integer_tables(ops, arithmetic, r, with_excl):
    m, n = 141, 1061   # m not a multiple of 128, n ragged against 128- and 64-item tiles
    Un, Vn = int_tables(m, n, r, seed=r + 7)
    pos, excl = edge_sets(m, n, seed=r)
    want = oracle_ranks(Un, Vn, pos, excl if with_excl else np.zeros_like(excl))
    U, V = torch.as_tensor(Un).cuda(), torch.as_tensor(Vn).cuda()
    if arithmetic == 'bf16':
        U, V, arithmetic = U.bfloat16(), V.bfloat16(), 'auto'
    got = run(ops, U, V, pos, excl if with_excl else None, arithmetic)
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f'{bad.size} of {want.size} ranks differ, first at pair {np.argwhere(pos)[bad[0]]}: {got[bad[0]]} vs {want[bad[0]]}'


def gauss_sets(m, n, U, V, seed):
    """Positives: random pairs plus some of each user's 60 best items (so that ranks below every k occur); exclusions: random
    pairs plus other best items of every second user, never a positive."""
    rng = np.random.default_rng(seed)
    S = U.astype(np.float64) @ V.T.astype(np.float64)
    best = np.argsort(-S, axis=1, kind='stable')[:, :60]
    pos = rng.random((m, n)) < 0.01
    excl = rng.random((m, n)) < 0.05
    for u in range(m):
        pick = rng.choice(60, 12, replace=False)
        pos[u, best[u, pick[:6]]] = True
        if u % 2 == 0:
            excl[u, best[u, pick[6:]]] = True
    excl &= ~pos
    return pos, excl


@pytest.mark.parametrize('arithmetic,r', [('fp32', 64), ('fp32', 100), ('split', 64), ('split', 128), ('split', 256)])
@pytest.mark.parametrize('with_excl', [False, True])
def test_invariant_rank_below_k_iff_in_topk(ops, arithmetic, r, with_excl):
    m, n = 300, 5003
    g = torch.Generator().manual_seed(r)
    U, V = torch.randn(m, r, generator=g), torch.randn(n, r, generator=g) * 0.3
    pos, excl = gauss_sets(m, n, U.numpy(), V.numpy(), seed=r)
    Ud, Vd = U.cuda(), V.cuda()
    ex = dense(excl) if with_excl else None
    ranks = ops.item_ranks(Ud, Vd, dense(pos), exclude=ex, arithmetic=arithmetic).cpu().numpy()
    pairs = np.argwhere(pos)
    for k in ((1, 10, 40, 64) if arithmetic == 'fp32' else (1, 10, 40)):
        top = ops.predict_topk(Ud, Vd, k, arithmetic=arithmetic, exclude=ex).cpu().numpy()
        member = (top[pairs[:, 0]] == pairs[:, 1][:, None]).any(axis=1)
        bad = np.nonzero(member != (ranks < k))[0]
        assert bad.size == 0, f'k={k}: {bad.size} pairs break the invariant, first {pairs[bad[0]]} rank {ranks[bad[0]]}'
        assert member.any() and not member.all()


@pytest.mark.parametrize('r', [40, 128, 256])
def test_fused_fp32_equals_non_fused(ops, r):
    m, n = 260, 4099
    g = torch.Generator().manual_seed(100 + r)
    U, V = torch.randn(m, r, generator=g), torch.randn(n, r, generator=g)
    pos, excl = gauss_sets(m, n, U.numpy(), V.numpy(), seed=r)
    Ud, Vd = U.cuda(), V.cuda()
    for ex in (None, dense(excl)):
        fused = ops.item_ranks(Ud, Vd, dense(pos), exclude=ex, arithmetic='fp32')
        # 'half2' has no fused rank form: it scores blocks with tmf_predict_gemm_f32 and counts them (the non-fused path)
        blocks = ops.item_ranks(Ud, Vd, dense(pos), exclude=ex, arithmetic='half2')
        assert torch.equal(fused, blocks)


def test_nan_and_inf_scores(ops):
    """A NaN item is never counted above anyone; a NaN positive ranks behind every non-NaN eligible item."""
    m, n, r = 40, 700, 8
    Un, Vn = int_tables(m, n, r, seed=3)
    Vn[[5, 130, 699]] = np.nan
    Vn[7] = np.inf * np.sign(Vn[7] + 0.5)
    pos = np.zeros((m, n), bool)
    pos[:, [5, 9, 64, 300]] = True
    S = Un.astype(np.float64) @ Vn.T.astype(np.float64)
    elig = ~np.isnan(S)
    want = []
    for u, i in np.argwhere(pos):
        s = S[u]
        if np.isnan(s[i]):
            want.append(int(np.count_nonzero(elig[u])) - 0)
        else:
            ids = np.arange(n)
            want.append(int(np.count_nonzero(elig[u] & ((s > s[i]) | ((s == s[i]) & (ids < i))))))
    U, V = torch.as_tensor(Un).cuda(), torch.as_tensor(Vn).cuda()
    for arithmetic in ('fp32', 'half2'):
        got = ops.item_ranks(U, V, dense(pos), arithmetic=arithmetic).cpu().numpy()
        assert np.array_equal(got, np.array(want)), arithmetic


def c1_model():
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    from oracle import datagen as G
    np.random.seed(0)
    m, n, r = 100, 50, 5
    idx, val, shape, _ = G.generate_random_interaction(m, n, density=0.05)
    model = MatrixFactorization(r, user_weight_graph=FixedInitializer(G.normal_init(m, r, 1)),
                                item_weight_graph=FixedInitializer(G.normal_init(n, r, 2)))
    model.verbose = False
    model.fit(10, eye(m), eye(n), SparseInteractions(idx, val, shape), lr=1e-2)
    return model


def test_auc_and_reciprocal_rank_against_oracle():
    from teamoflow_amd.mf.sparse import SparseInteractions
    model = c1_model()
    m, n = 100, 50
    rng = np.random.default_rng(5)
    pos = rng.random((m, n)) < 0.1
    pos[:7] = False
    pos[7] = True                      # N = 0: AUC 1
    excl = (rng.random((m, n)) < 0.2) & ~pos
    S = model.user_embedding.double().cpu().numpy() @ model.item_embedding.double().cpu().numpy().T
    ids = np.arange(n)
    want_auc, want_rr = np.zeros(m), np.zeros(m)
    for u in range(m):
        P = np.nonzero(pos[u])[0]
        N = np.nonzero(~pos[u] & ~excl[u])[0]
        if P.size == 0:
            continue
        rk = [np.count_nonzero(~excl[u] & ((S[u] > S[u, i]) | ((S[u] == S[u, i]) & (ids < i)))) for i in P]
        want_rr[u] = 1.0 / (1 + min(rk))
        if N.size == 0:
            want_auc[u] = 1.0
            continue
        beat = sum(int(np.count_nonzero((S[u, N] > S[u, i]) | ((S[u, N] == S[u, i]) & (N < i)))) for i in P)
        want_auc[u] = 1.0 - beat / (P.size * N.size)
    has = pos.any(axis=1)
    idx = np.argwhere(pos)
    A = SparseInteractions(idx, np.ones(len(idx), np.float32), (m, n))
    ex = SparseInteractions(np.argwhere(excl), np.ones(int(excl.sum()), np.float32), (m, n))
    auc = model.auc_score(A, exclude=ex).cpu().numpy()
    rr = model.reciprocal_rank(A, exclude=ex).cpu().numpy()
    assert auc.dtype == np.float32 and auc.shape == (int(has.sum()),)
    np.testing.assert_allclose(auc, want_auc[has], rtol=0, atol=1e-6)
    np.testing.assert_allclose(rr, want_rr[has], rtol=0, atol=1e-6)
    auc_p = model.auc_score(torch.as_tensor(pos.astype(np.float32)), preserve_rows=True, exclude=ex).cpu().numpy()
    rr_p = model.reciprocal_rank(A, preserve_rows=True, exclude=ex).cpu().numpy()
    np.testing.assert_allclose(auc_p, np.where(has, want_auc, 0.0), rtol=0, atol=1e-6)
    np.testing.assert_allclose(rr_p, np.where(has, want_rr, 0.0), rtol=0, atol=1e-6)
    got_idx, got_rank = model.item_ranks(A, exclude=ex)
    assert got_idx.dtype == torch.int64 and got_rank.dtype == torch.int64
    assert np.array_equal(got_idx.cpu().numpy(), idx)
    clash = excl.copy()
    clash[idx[0][0], idx[0][1]] = True
    clash[idx[5][0], idx[5][1]] = True
    with pytest.raises(ValueError, match='2 '):
        model.auc_score(A, exclude=torch.as_tensor(clash.astype(np.float32)))


def test_c4_shape(ops):
    """1M users x 100K items, r = 128, 10 held-out items per user, ~1e8 excluded pairs, default arithmetic: the invariant for
    k = 10 on every user; 256 sampled users against fp64 wherever no eligible item lies within 1e-5 of the positive's score
    (relative to the larger of |score| and the user's mean |score|)."""
    from teamoflow_amd.mf.sparse import SparseInteractions
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(11)
    m, n, r, k, per, held = 1_000_000, 100_000, 128, 10, 100, 10
    U = torch.randn(m, r, device=dev, generator=g) * 0.1
    V = torch.randn(n, r, device=dev, generator=g) * 0.1
    best = ops.predict_topk(U, V, 20, arithmetic='fp32').long()
    # held-out: 3 of the user's 20 best, 7 random; excluded: 10 other best ones + 90 random, never a held-out pair
    hp = torch.cat([best[:, :3], torch.randint(0, n, (m, held - 3), device=dev, generator=g)], 1)
    users = torch.arange(m, device=dev)
    A = SparseInteractions(torch.stack([users.repeat_interleave(held), hp.reshape(-1)], 1), torch.ones(m * held, device=dev), (m, n),
                           device=dev)
    pos = ops.positive_pairs(A, m, n)
    xi = torch.cat([best[:, 5:15], torch.randint(0, n, (m, per - 10), device=dev, generator=g)], 1).reshape(-1)
    xu = users.repeat_interleave(per)
    keys = torch.unique(xu * n + xi)
    pk = ops._csr_rows(pos.rowptr) * n + pos.cols[:int(pos.rowptr[-1])].long()
    keys = keys[~torch.isin(keys, pk)]
    ex = ops.build_exclusion(SparseInteractions(torch.stack([keys // n, keys % n], 1), torch.ones(keys.numel(), device=dev), (m, n),
                                                device=dev), m, n)
    del best, hp, xi, xu, keys, pk
    assert int(ex.cols.numel()) > 9e7
    ranks = ops.item_ranks(U, V, A, exclude=ex).long()
    top = ops.predict_topk(U, V, k, exclude=ex).long()
    pu, pi = ops._csr_rows(pos.rowptr), pos.cols[:ranks.numel()].long()
    member = (top[pu] == pi[:, None]).any(dim=1)
    bad = int((member != (ranks < k)).sum())
    assert bad == 0, f'{bad} of {ranks.numel()} pairs break the invariant'
    assert 0 < int(member.sum()) < ranks.numel()
    sample = torch.randperm(m, device=dev, generator=g)[:256].sort()[0]
    S = (U[sample].double() @ V.double().T).cpu().numpy()
    rp, cols = ex.rowptr.cpu().numpy(), ex.cols.cpu().numpy()
    prp, pcols, rk = pos.rowptr.cpu().numpy(), pos.cols.cpu().numpy(), ranks.cpu().numpy()
    ids = np.arange(n)
    checked = 0
    for row, u in enumerate(sample.cpu().numpy()):
        s = S[row]
        elig = np.ones(n, bool)
        elig[cols[rp[u]:rp[u + 1]]] = False
        scale = np.abs(s).mean()
        for p in range(prp[u], prp[u + 1]):
            i = pcols[p]
            near = elig & (np.abs(s - s[i]) <= 1e-5 * max(abs(s[i]), scale)) & (ids != i)
            if near.any():
                continue
            want = int(np.count_nonzero(elig & (s > s[i])))
            assert rk[p] == want, (u, i, rk[p], want)
            checked += 1
    assert checked > 1000   # of 2560: the others have an eligible item within the window
