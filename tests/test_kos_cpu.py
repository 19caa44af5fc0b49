"""CPU side of KOSWARPLoss (no GPU): the NumPy fp64 reference of the weights (kos_weights_ref: counts by comparing every two
positives of a user, B from its sum with math.comb) and of the weighted pair step (kos_pairs_ref: omega times warp_pairs_ref's
terms), which tests/test_gpu_kos.py imports; the weights against an exhaustive enumeration of every draw in exact fractions; their
sum, their invariance under the storage order; the plug-in's get_loss against the reference; the class surface, save / load, the
dispatch and its refusals; the C ABI of tmf_kos_weights and tmf_warp_pairs_kos (declared, bound, built, argument checks); and the
statement the GPU file's fits rest on: every one-step problem is *decided* - no first-violator choice (test_warp_cpu.decidedness)
and no order of two positives of one user (order_decidedness) is within fp32 reach of flipping."""
import itertools
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_step, rel_err
from test_warp_cpu import GENERIC_PROBLEM, GEOMETRY_PROBLEMS, LR, _scores, bf16_round, decidedness, warp_pairs_ref, warp_problem

KOS_CAP = 2048                                    # csrc/tmf_kos.hip: KCAP (the positives of a row the LDS holds at once)
K, N = 5, 10                                      # KOSWARPLoss's defaults


# ------------------------------------------------------------------------------------------------------------------------
# the reference: shares no code with the package
# ------------------------------------------------------------------------------------------------------------------------
def kos_B(c, P, k, n):
    """B(c / P) in fp64 for n' = min(n, P), k' = min(k, n'): sum_{i < k'} C(n', i) q^i (1 - q)^(n' - i)."""
    n_ = min(n, P)
    k_ = min(k, n_)
    q, r = c / P, (P - c) / P
    return sum(math.comb(n_, i) * q ** i * r ** (n_ - i) for i in range(k_))


def kos_weights_ref(rowptr, val, p, k, n):
    """tmf_kos_weights on given scores: omega [nnz] in fp64.  The scores are compared in the dtype they come in; a NaN orders below
    -inf and ties with the other NaNs; 0 for a stored value <= 0."""
    rowptr, val, p = np.asarray(rowptr, np.int64), np.asarray(val, np.float64), np.asarray(p)
    omega = np.zeros(val.shape[0])
    for u in range(rowptr.shape[0] - 1):
        ks = np.arange(rowptr[u], rowptr[u + 1])[val[rowptr[u]:rowptr[u + 1]] > 0]
        P = ks.size
        if P == 0:
            continue
        x, nan = p[ks], np.isnan(p[ks])
        with np.errstate(invalid='ignore'):
            above = (x[None, :] > x[:, None]) | (~nan[None, :] & nan[:, None])        # [j, i]: p_i > p_j
            equal = (x[None, :] == x[:, None]) | (nan[None, :] & nan[:, None])
        a, t = above.sum(1), equal.sum(1)
        memo = {}
        for j, (aj, tj) in enumerate(zip(a.tolist(), t.tolist())):
            for c in (aj, aj + tj):
                if c not in memo:
                    memo[c] = kos_B(c, P, k, n)
            omega[ks[j]] = max((memo[aj] - memo[aj + tj]) / tj, 0.0)
    return omega


def kos_pairs_ref(rowptr, val, p, sp, n_items, omega, decide=np.float32):
    """tmf_warp_pairs_kos on given scores and weights: (delta [nnz], D [m, S], loss_part [m], first [nnz]) - warp_pairs_ref's first
    violators and weights, every term times omega[k]; values in fp64."""
    rowptr, val, omega = np.asarray(rowptr, np.int64), np.asarray(val, np.float64), np.asarray(omega, np.float64)
    pd, spd = np.asarray(p, decide).astype(np.float64), np.asarray(sp, decide).astype(np.float64)
    first = warp_pairs_ref(rowptr, val, p, sp, n_items, decide=decide)[3]
    m, S = spd.shape
    delta, D, loss = np.zeros(val.shape[0]), np.zeros((m, S)), np.zeros(m)
    with np.errstate(invalid='ignore', over='ignore'):
        for u in range(m):
            for k in range(rowptr[u], rowptr[u + 1]):
                if first[k] >= 0:
                    w = omega[k] * float(np.log(max(1, (int(n_items) - 1) // (int(first[k]) + 1))))
                    if w > 0:
                        delta[k] = -w
                        D[u, first[k]] += w
                        loss[u] += w * (1.0 - pd[k] + spd[u, first[k]])
    return delta, D, loss, first


def kos_closed_form(U0, V0, idx, val, R, k=K, n=N):
    """One KOSWARPLoss epoch in fp64 (decisions and ranks in fp64 too: the dtype of the scores) - test_warp_cpu.warp_closed_form with
    the weights.  -> (loss sum over the positives, delta [nnz], D [m, S] in R's order, gU, gV)."""
    U, V, u, i, rowptr, p, sp = _scores(U0, V0, idx, R)
    R = np.asarray(R, np.int64)
    m, S = R.shape
    omega = kos_weights_ref(rowptr, val, p, k, n)
    delta, D, loss, _ = kos_pairs_ref(rowptr, val, p, sp, V.shape[0], omega, decide=np.float64)
    gU = np.einsum('us,usr->ur', D, V[R])
    np.add.at(gU, u, delta[:, None] * V[i])
    gV = np.zeros_like(V)
    np.add.at(gV, R.reshape(-1), (D[:, :, None] * U[:, None, :]).reshape(m * S, -1))
    np.add.at(gV, i, delta[:, None] * U[u])
    return loss.sum(), delta, D, gU, gV


def order_decidedness(U0, V0, idx, val):
    """The smallest difference between the scores of two positives of one user (inf where no user has two).  Above twice the bound b
    of test_warp_cpu.decidedness - what an fp32 evaluation of either score may be off by - no fp32 evaluation can order two positives
    otherwise than fp64 does, or tie them."""
    U, V = np.asarray(U0, np.float64), np.asarray(V0, np.float64)
    idx, val = np.asarray(idx, np.int64), np.asarray(val)
    p = np.einsum('kr,kr->k', U[idx[:, 0]], V[idx[:, 1]])
    gap = np.inf
    for u in np.unique(idx[:, 0]):
        mine = np.sort(p[(idx[:, 0] == u) & (val > 0)])
        if mine.size > 1:
            gap = min(gap, float(np.diff(mine).min()))
    return gap


def assert_decided(U0, V0, idx, val, R, what=''):
    g_min, b = decidedness(U0, V0, idx, val, R)
    gap = order_decidedness(U0, V0, idx, val)
    print(f'[decided] {what}: smallest violator gap {g_min:.3g}, smallest gap between two positives {gap:.3g}, fp32 reach {b:.3g}')
    assert g_min > b and gap > 2 * b, (what, g_min, gap, b)


# (seed, m, n, r, S) of every one-step problem tests/test_gpu_kos.py runs through fit(), at KOS_DENSITY: all decided - first violators
# and the order of every user's positives (asserted below and there).  About 10 positives per user: k' = 5 of n' = 10 for many
# users, n' or both clamped for the others.
KOS_DENSITY = 0.05
KOS_GEOMETRY = {(1, 5): (2, 60, 240, 1, 5), (7, 64): (7, 60, 240, 7, 64), (33, 70): (33, 60, 240, 33, 70), (64, 5): (65, 60, 240, 64, 5),
                (128, 64): (129, 60, 240, 128, 64), (200, 70): (200, 60, 240, 200, 70), (256, 5): (258, 60, 240, 256, 5)}
KOS_BF16 = (133, 60, 240, 33, 64)
KOS_ADAM = (8, 60, 240, 12, 20)
KOS_BIASED = (1033, 60, 240, 33, 64)
KOS_FEATURES = (2033, 60, 240, 33, 64)
KOS_L2 = (3033, 60, 240, 33, 64)
KOS_REPLAY = (2006, 200, 150, 16, 32)
KOS_ONE_STEP = list(KOS_GEOMETRY.values()) + [KOS_ADAM, KOS_BIASED, KOS_L2, KOS_REPLAY]


def kos_problem(problem):
    seed, m, n, r, S = problem
    return warp_problem(seed, m, n, r, S, density=KOS_DENSITY)


def kos_features_problem():
    """test_warp_cpu.features_problem on the sparser table: (problem, tag_idx, tag_val, F_dense, W0), E = F W0."""
    p = kos_problem(KOS_FEATURES)
    n, r, T = p['n'], p['r'], 6
    rng = np.random.default_rng(5)
    tag_idx = np.argwhere(rng.random((n, T)) < 0.3)
    tag_val = rng.choice(np.array([1.0, 0.5, -0.25, 2.0], np.float32), tag_idx.shape[0])
    F_dense = np.zeros((n, n + T))
    F_dense[np.arange(n), np.arange(n)] = 1.0
    F_dense[tag_idx[:, 0], n + tag_idx[:, 1]] = tag_val
    W0 = (rng.standard_normal((n + T, r)) * np.sqrt(1.5) / r ** 0.25 / 1.5).astype(np.float32)
    return p, tag_idx, tag_val, F_dense, W0


def single_positive_problem(seed=4, m=60, n=240, r=33, S=64):
    """Every user stores exactly one positive (and a few values <= 0): omega is exactly 1, KOSWARPLoss(1, 1) is WARPLoss."""
    p = warp_problem(seed, m, n, r, S, density=0.05)
    keep = np.ones(p['val'].shape[0], bool)
    seen = set()
    for j, ((u, _), a) in enumerate(zip(p['idx'], p['val'])):
        if a > 0:
            keep[j] = u not in seen
            seen.add(int(u))
    p['idx'], p['val'] = p['idx'][keep], p['val'][keep]
    return p


# ------------------------------------------------------------------------------------------------------------------------
# the weights
# ------------------------------------------------------------------------------------------------------------------------
def enumerated_weights(scores, k, n):
    """omega of one user's positives as exact fractions: every one of the P^n' draws with replacement, the k'-th best score of the
    draw, its probability shared equally by the entries that have that score."""
    P = len(scores)
    n_ = min(n, P)
    k_ = min(k, n_)
    out = [Fraction(0)] * P
    for draw in itertools.product(range(P), repeat=n_):
        v = sorted((scores[j] for j in draw), reverse=True)[k_ - 1]
        block = [j for j in range(P) if scores[j] == v]
        for j in block:
            out[j] += Fraction(1, P ** n_ * len(block))
    return out


ENUMERATED_ROWS = ([3.0], [1.0, 2.0], [2.0, 2.0], [0.5, 1.5, 1.0], [1.0, 1.0, 0.0], [0.0, 1.0, 1.0], [7.0, 7.0, 7.0],
                   [4.0, 3.0, 2.0, 1.0], [2.0, 2.0, 1.0, 0.0], [2.0, 1.0, 1.0, 0.0], [0.0, 1.0, 2.0, 0.0], [5.0, 1.0, 1.0, 1.0],
                   [1.0, 1.0, 1.0, 0.0], [3.0, 3.0, 1.0, 1.0])


def test_weights_against_every_draw_enumerated():
    """P <= 4, n <= 5 and every k <= n, tie blocks of 2 and 3 at the top, in the middle and at the end: 1e-14 of the exact fraction."""
    worst = 0.0
    for scores in ENUMERATED_ROWS:
        P = len(scores)
        for n in range(1, 6):
            for k in range(1, n + 1):
                exact = enumerated_weights(scores, k, n)
                assert sum(exact) == 1
                got = kos_weights_ref([0, P], np.ones(P), np.array(scores, np.float32), k, n)
                worst = max(worst, max(abs(g - float(e)) for g, e in zip(got, exact)))
    print(f'[enumerated] largest deviation {worst:.3g}')
    assert worst <= 1e-14


@pytest.mark.parametrize('k,n', [(5, 10), (1, 1), (10, 10), (1, 64), (64, 64), (3, 7)])
def test_weights_sum_to_one(k, n):
    """P = 1 .. 200 with ties (scores from a small set): P < k clamps k', k <= P < n clamps n' alone."""
    rng = np.random.default_rng(k * 100 + n)
    for P in range(1, 201):
        p = rng.integers(0, max(2, P // 2), P).astype(np.float32)
        omega = kos_weights_ref([0, P], np.ones(P), p, k, n)
        assert abs(omega.sum() - 1.0) <= 1e-12 and (omega >= 0).all(), (P, omega.sum())
    assert kos_weights_ref([0, 3], np.ones(3), [1.0, 2.0, 3.0], 5, 10).tolist() == pytest.approx([1 - (2 / 3) ** 3, (2 / 3) ** 3 - (1 / 3) ** 3, (1 / 3) ** 3], abs=1e-15)
    # P = 7, k = 5, n = 10: n' = 7 alone is clamped; the best positive is the 5th best of 7 draws only if at least 5 draws hit it
    top = kos_weights_ref([0, 7], np.ones(7), np.arange(7.0), 5, 10)[6]
    assert top == pytest.approx(sum(math.comb(7, i) * (1 / 7) ** i * (6 / 7) ** (7 - i) for i in range(5, 8)), abs=1e-15)


def test_weights_do_not_depend_on_the_storage_order():
    rng = np.random.default_rng(3)
    P = 40
    val = rng.choice(np.array([-1.0, 0.0, 1.0, 2.0]), P, p=[.1, .1, .4, .4])
    p = rng.integers(0, 12, P).astype(np.float32)
    p[[3, 17]] = np.nan
    p[5], p[6] = np.inf, -np.inf
    omega = kos_weights_ref([0, P], val, p, K, N)
    for seed in range(5):
        perm = np.random.default_rng(seed).permutation(P)
        assert np.abs(kos_weights_ref([0, P], val[perm], p[perm], K, N) - omega[perm]).max() <= 1e-15
    assert not omega[val <= 0].any() and abs(omega.sum() - 1) < 1e-12


def test_infinite_and_nan_scores_in_the_ranking():
    """+inf is the best, -inf below every number, a NaN below -inf and tied with the other NaNs; all count in P."""
    nan, inf = float('nan'), float('inf')
    p = np.array([nan, 1.0, -inf, inf, nan, 0.0], np.float32)
    omega = kos_weights_ref([0, 6], np.ones(6), p, 1, 1)
    assert omega.tolist() == pytest.approx([1 / 6] * 6, abs=1e-16)
    omega = kos_weights_ref([0, 6], np.ones(6), p, 2, 2)                     # the lower of two draws
    B = [kos_B(c, 6, 2, 2) for c in range(7)]
    assert omega.tolist() == pytest.approx([(B[4] - B[6]) / 2, B[1] - B[2], B[3] - B[4], B[0] - B[1], (B[4] - B[6]) / 2, B[2] - B[3]], abs=1e-16)
    assert kos_weights_ref([0, 2], np.ones(2), np.array([0.0, -0.0], np.float32), 1, 2).tolist() == [0.5, 0.5]    # -0 == +0: one tie block


# ------------------------------------------------------------------------------------------------------------------------
# the plug-in
# ------------------------------------------------------------------------------------------------------------------------
def _get_loss(U, V, idx, val, R, loss, dtype=torch.float64):
    """(per-positive losses, dL/dU, dL/dV) of a loss graph's get_loss fed as _fit_generic feeds it, by autograd."""
    from teamoflow_amd.mf.sparse import SparseInteractions
    U, V = (torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in (U, V))
    inter = SparseInteractions(idx, val, (U.shape[0], V.shape[0]), device='cpu')
    pred = U @ V.T
    out = loss.get_loss(tf_interactions=inter, tf_sample_predictions=torch.gather(pred, 1, torch.as_tensor(R, dtype=torch.int64)),
                        tf_prediction_serial=pred[inter.indices[:, 0], inter.indices[:, 1]], predictions=None,
                        n_items=V.shape[0], n_samples=R.shape[1])
    gU, gV = torch.autograd.grad(out.sum(), (U, V))
    return out.detach().numpy(), gU.numpy(), gV.numpy()


def test_class_surface():
    import inspect
    import teamoflow.mf.loss_graphs as alias
    from teamoflow_amd.mf import loss_graphs as LG
    from teamoflow_amd.mf import matrix_factorization as M
    Kos = LG.KOSWARPLoss
    assert alias.KOSWARPLoss is Kos and issubclass(Kos, LG.LossGraph) and not issubclass(Kos, LG.WARPLoss)
    assert inspect.signature(Kos.get_loss) == inspect.signature(LG.WARPLoss.get_loss)
    assert (Kos().k, Kos().n) == (5, 10) and (Kos(2, 7).k, Kos(n=7, k=2).n) == (2, 7)
    assert Kos in M.ENGINE_LOSSES and Kos in M.TABLE_LOSSES and Kos in M.PAIR_STEP_LOSSES
    assert "warp-kos" in Kos.__doc__ and 'B(q)' in Kos.__doc__


@pytest.mark.parametrize('k,n', [(0, 5), (6, 5), (1, 65), (65, 65), (-1, 3), (2.0, 4), (2, 4.0), (True, 4), ('2', 4), (None, 3)])
def test_constructor_refuses(k, n):
    from teamoflow_amd.mf.loss_graphs import KOSWARPLoss
    with pytest.raises(ValueError, match='KOSWARPLoss'):
        KOSWARPLoss(k, n)


def test_constructor_accepts_the_corners():
    from teamoflow_amd.mf.loss_graphs import KOSWARPLoss
    for k, n in ((1, 1), (1, 64), (64, 64)):
        assert (KOSWARPLoss(k, n).k, KOSWARPLoss(k, n).n) == (k, n)


@pytest.mark.parametrize('r,S', list(GEOMETRY_PROBLEMS))
def test_get_loss_is_the_reference(r, S):
    """fp64, the shapes of test_warp_cpu.GEOMETRY_PROBLEMS (about 58 positives per user) and (k, n) = (5, 10): 1e-12."""
    from teamoflow_amd.mf.loss_graphs import KOSWARPLoss
    p = warp_problem(*GEOMETRY_PROBLEMS[(r, S)])
    loss, delta, D, gU, gV = kos_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    out, aU, aV = _get_loss(p['U0'], p['V0'], p['idx'], p['val'], p['R'], KOSWARPLoss())
    assert out.shape == (int((p['val'] > 0).sum()),) and out.dtype == np.float64
    _, _, _, _, rowptr, pk, sp = _scores(p['U0'], p['V0'], p['idx'], p['R'])
    omega = kos_weights_ref(rowptr, p['val'], pk, K, N)
    pos = p['val'] > 0
    terms = -delta[pos] * (1.0 - pk[pos] + np.take_along_axis(sp[p['idx'][pos, 0]], np.maximum(
        warp_pairs_ref(rowptr, p['val'], pk, sp, p['n'], decide=np.float64)[3][pos], 0)[:, None], 1)[:, 0])
    assert rel_err(out, terms) < 1e-12 and rel_err(out.sum(), loss) < 1e-12 and rel_err(aU, gU) < 1e-12 and rel_err(aV, gV) < 1e-12
    assert loss > 0 and (D > 0).any() and not gU[p['empty_user']].any() and not gU[p['nonpos_user']].any()
    sums = np.bincount(p['idx'][:, 0], weights=omega, minlength=p['m'])
    has = np.bincount(p['idx'][pos, 0], minlength=p['m']) > 0
    assert np.abs(sums[has] - 1).max() < 1e-12 and not sums[~has].any()


def test_k_and_n_of_one_give_the_per_user_mean_of_warp():
    from teamoflow_amd.mf.loss_graphs import KOSWARPLoss, WARPLoss
    p = warp_problem(12, 33, 47, 5, 12)
    kos, _, _ = _get_loss(p['U0'], p['V0'], p['idx'], p['val'], p['R'], KOSWARPLoss(1, 1))
    warp, _, _ = _get_loss(p['U0'], p['V0'], p['idx'], p['val'], p['R'], WARPLoss())
    users = p['idx'][p['val'] > 0, 0]
    P = np.bincount(users, minlength=p['m'])[users]
    assert P.max() > 5 and rel_err(kos, warp / P) < 1e-12 and warp.sum() > 0


def test_get_loss_with_infinite_and_nan_scores():
    """The ranking of test_infinite_and_nan_scores_in_the_ranking through the plug-in; a NaN positive's WARP term is zero anyway, and
    nothing next to it becomes NaN."""
    from teamoflow_amd.mf.loss_graphs import KOSWARPLoss
    from teamoflow_amd.mf.sparse import SparseInteractions
    nan, inf = float('nan'), float('inf')
    idx = np.array([[0, j] for j in range(6)] + [[1, 0]])
    inter = SparseInteractions(idx, np.ones(7), (2, 6), device='cpu')
    pos = torch.tensor([nan, 1.0, -inf, inf, nan, 0.0, 0.25], dtype=torch.float64)
    sp = torch.tensor([[0.5, nan, 2.0], [-inf, nan, 0.5]], dtype=torch.float64)
    users = inter.indices[:, 0]
    omega = KOSWARPLoss(2, 2).weights(users, pos, 2).numpy()
    ref = kos_weights_ref([0, 6, 7], np.ones(7), pos.numpy(), 2, 2)
    assert np.abs(omega - ref).max() < 1e-15 and omega[6] == 1.0
    out = KOSWARPLoss(2, 2).get_loss(tf_interactions=inter, tf_sample_predictions=sp, tf_prediction_serial=pos, n_items=100, n_samples=3)
    want = kos_pairs_ref([0, 6, 7], np.ones(7), pos.numpy(), sp.numpy(), 100, ref, decide=np.float64)
    assert not torch.isnan(out).any() and out[0] == 0 and out[4] == 0 and out[3] == 0
    assert out[6].item() == pytest.approx(np.log(33.0) * (1 - 0.25 + 0.5), rel=1e-15)
    assert np.bincount([0] * 6 + [1], weights=out.numpy()).tolist() == pytest.approx(want[2].tolist(), rel=1e-13)


# ------------------------------------------------------------------------------------------------------------------------
# what the GPU file's fits rest on
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('problem', KOS_ONE_STEP, ids=lambda s: 'x'.join(map(str, s)))
def test_one_step_problems_are_decided(problem):
    p = kos_problem(problem)
    assert_decided(p['U0'], p['V0'], p['idx'], p['val'], p['R'], str(problem))
    users = p['idx'][p['val'] > 0, 0]
    P = np.bincount(users, minlength=p['m'])
    assert (P > N).any() and ((P > 0) & (P < K)).any(), 'users with more than n and with fewer than k positives'
    assert kos_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])[0] > 0


def test_the_bf16_the_featured_and_the_single_positive_problem_are_decided():
    p = kos_problem(KOS_BF16)
    assert_decided(bf16_round(p['U0']), bf16_round(p['V0']), p['idx'], p['val'], p['R'], 'bf16')
    p, _, _, F_dense, W0 = kos_features_problem()
    assert_decided(p['U0'], F_dense @ W0.astype(np.float64), p['idx'], p['val'], p['R'], 'features')
    p = single_positive_problem()
    P = np.bincount(p['idx'][p['val'] > 0, 0], minlength=p['m'])
    assert set(P.tolist()) == {0, 1} and P.sum() > 40 and (p['val'] <= 0).any()
    g_min, b = decidedness(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    assert g_min > b


def test_order_decidedness_sees_two_positives_within_reach():
    U0, V0 = np.array([[1.0, 0.5]]), np.array([[2.0, 0.0], [2.0 + 1e-9, 0.0], [0.0, 1.0]])
    assert abs(order_decidedness(U0, V0, np.array([[0, 0], [0, 1], [0, 2]]), np.array([1.0, 1.0, 1.0])) - 1e-9) < 1e-12
    assert order_decidedness(U0, V0, np.array([[0, 0], [0, 1], [0, 2]]), np.array([1.0, 0.0, 1.0])) == 1.5    # the close one is no positive
    assert order_decidedness(U0, V0, np.array([[0, 0]]), np.array([1.0])) == np.inf


# ------------------------------------------------------------------------------------------------------------------------
# the model without a GPU
# ------------------------------------------------------------------------------------------------------------------------
def _model(p, loss=None, table=True, **attrs):
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import KOSWARPLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    model = MatrixFactorization(p['r'], loss_graph=loss or KOSWARPLoss(), user_weight_graph=FixedInitializer(p['U0']),
                                item_weight_graph=FixedInitializer(p['V0']), n_users=p['m'], n_items=p['n'], n_samples=p['S'])
    model.verbose = False
    if table:
        model.random_ind = torch.as_tensor(p['R'])
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


def _fit(model, p, epochs):
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    model.fit(epochs, eye(p['m']), eye(p['n']), SparseInteractions(p['idx'], p['val'], (p['m'], p['n']), device='cpu'), lr=LR)
    return model


def test_generic_fit_without_a_gpu(monkeypatch):
    """test_warp_cpu.GENERIC_PROBLEM through _fit_generic: the first loss is the closed form's mean over the positives (WARPLoss's
    reduction and denominator), one step moves the tables as the closed-form gradients say, and 20 epochs end below where they began."""
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    p = warp_problem(*GENERIC_PROBLEM)
    assert_decided(p['U0'], p['V0'], p['idx'], p['val'], p['R'], 'generic')
    model = _fit(_model(p), p, 20)
    h = model.loss_history_
    assert not hasattr(model, '_state') and len(h) == 20 and h[-1] < h[0], h
    loss, _, _, gU, gV = kos_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    assert rel_err(h[0], loss / int((p['val'] > 0).sum())) < 1e-5
    one = _fit(_model(p), p, 1)
    assert_step(one.user_embedding.detach().numpy(), p['U0'], gU, LR, rtol=1e-5, what='U')
    assert_step(one.item_embedding.detach().numpy(), p['V0'], gV, LR, rtol=1e-5, what='V')


def test_no_sample_table(monkeypatch):
    from teamoflow_amd.mf.matrix_factorization import SampleTableMissing
    p = warp_problem(15, 12, 9, 4, 4)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(SampleTableMissing, match='KOSWARPLoss'):
        _fit(_model(p, table=False), p, 1)


def test_loss_name_and_dispatch(monkeypatch):
    from teamoflow_amd import _engine
    from teamoflow_amd.mf import loss_graphs as LG
    from teamoflow_amd.mf.sparse import eye

    class MyKOS(LG.KOSWARPLoss):
        pass
    assert _engine.loss_name(LG.KOSWARPLoss()) == 'warp_kos' and 'warp_kos' in _engine.PAIR_LOSSES and 'warp_kos' in _engine.SLICED_ONLY
    with pytest.raises(TypeError, match='KOSWARPLoss'):
        _engine.loss_name(MyKOS())
    p = warp_problem(16, 12, 9, 4, 4)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    for settings in ({}, dict(factor_dtype=torch.bfloat16), dict(optimizer='adam'), dict(user_alpha=0.1), dict(resample_every=1)):
        assert _model(p, **settings)._route(eye(12), eye(9)) == 'engine', settings
    assert _model(p, loss=MyKOS())._route(eye(12), eye(9)) == 'generic'
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    assert _model(p)._route(eye(12), eye(9)) == 'generic'


def test_a_kos_epoch_needs_a_sliced_plan():
    from teamoflow_amd import _engine

    class Plan:
        sliced = False

    class State:
        wplan = Plan()
        plan = r = None
    with pytest.raises(ValueError, match="'warp_kos' on a state without a sliced WmrbPlan"):
        _engine.run_epoch(State(), None, None, 'warp_kos', (5, 10))
    with pytest.raises(ValueError, match='pairs=warp_kos needs the sliced user pass'):
        _engine.epoch_wmrb(State(), None, (5, 10), None, pairs='warp_kos')


@pytest.mark.parametrize('setting', [('batch_users', 8), ('shard_items', 2), ('data_parallel', True), ('data_parallel', 'force')],
                         ids=lambda s: f'{s[0]}={s[1]}')
@pytest.mark.parametrize('gpu', [False, True], ids=['cpu', 'gpu'])
def test_unbuilt_forms_are_refused_before_anything_is_built(monkeypatch, setting, gpu):
    from teamoflow_amd import _engine
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    p = warp_problem(17, 12, 9, 4, 4)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: gpu)
    for name in ('_fit_sparse', '_fit_generic'):
        monkeypatch.setattr(MatrixFactorization, name, lambda self, *a, **k: pytest.fail('a fit was started'))
    monkeypatch.setattr(_engine, 'InteractionPlan', lambda *a, **k: pytest.fail('a plan was built'))
    monkeypatch.setattr(FixedInitializer, 'initialize_weights', lambda self, *a, **k: pytest.fail('a weight was drawn'))
    with pytest.raises(NotImplementedError, match=f'KOSWARPLoss with {setting[0]}'):
        _fit(_model(p, **{setting[0]: setting[1]}), p, 1)


def test_save_and_load(tmp_path, monkeypatch):
    from teamoflow_amd.mf.loss_graphs import KOSWARPLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    p = warp_problem(18, 12, 9, 4, 4)
    model = _fit(_model(p, loss=KOSWARPLoss(2, 7)), p, 2)
    path = str(tmp_path / 'model.pt')
    model.save(path)
    back = MatrixFactorization.load(path, device='cpu')
    assert type(back.loss_graph) is KOSWARPLoss and (back.loss_graph.k, back.loss_graph.n) == (2, 7)
    assert back.loss_history_ == model.loss_history_ and torch.equal(back.user_embedding, model.user_embedding.detach())
    again = _fit(back, p, 2)                                            # a loaded model trains again, through the same path
    assert again.loss_history_ == model.loss_history_
    assert _fit(_model(p, loss=KOSWARPLoss(5, 10)), p, 2).loss_history_ != model.loss_history_       # k and n matter


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_built():
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    declared = set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    lib = _lib.load_library()
    for name in ('tmf_kos_weights', 'tmf_warp_pairs_kos'):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES['tmf_kos_weights'][1]) == 9
    assert len(_lib.SIGNATURES['tmf_warp_pairs_kos'][1]) == len(_lib.SIGNATURES['tmf_warp_pairs_ranked'][1]) + 1     # and omega
    assert _lib.HEADER.constants['TMF_VERSION'] == 203
    make = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS :=.*\btmf_kos\.hip\b', make, re.M)
    source = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'tmf_kos.hip')).read()
    assert re.search(rf'\bKCAP = {KOS_CAP};', source)


def test_argument_checks_fail_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail differently; these return first."""
    import ctypes
    from teamoflow_amd import _lib
    lib = _lib.load_library()
    host = (ctypes.c_double * 8)()              # stands for any non-null buffer: never dereferenced
    H, i32 = ctypes.cast(host, ctypes.c_void_p), ctypes.c_int32
    assert lib.tmf_kos_weights(None, None, None, i32(0), i32(5), i32(10), None, None, None) == 0          # no users: nothing to do
    for args in ((None, H, H, i32(3), i32(5), i32(10), H), (H, H, H, i32(-1), i32(5), i32(10), H), (H, H, H, i32(3), i32(0), i32(10), H),
                 (H, H, H, i32(3), i32(11), i32(10), H), (H, H, H, i32(3), i32(5), i32(65), H), (H, H, H, i32(0), i32(5), i32(65), H)):
        assert lib.tmf_kos_weights(*args, None, None) == -1 and 'tmf_kos_weights' in lib.tmf_last_error().decode()
    assert lib.tmf_warp_pairs_kos(None, None, None, None, None, None, i32(0), i32(8), i32(9), None, None, None, None, None) == 0
    for args in ((None, H, H, H, H, H, i32(3), i32(8), i32(9), H, H, H), (H, H, H, None, H, H, i32(3), i32(8), i32(9), H, H, H),
                 (H, H, H, H, H, None, i32(3), i32(8), i32(9), H, H, H), (H, H, H, H, None, None, i32(3), i32(8), i32(9), H, H, H),
                 (H, H, H, H, H, H, i32(3), i32(8), i32(9), H, None, H), (H, H, H, H, H, H, i32(3), i32(0), i32(9), H, H, H),
                 (H, H, H, H, H, H, i32(-1), i32(8), i32(9), H, H, H), (H, H, H, H, H, H, i32(3), i32(8), i32(0), H, H, H),
                 (H, H, H, H, H, H, i32(3), i32(65537), i32(9), H, H, H)):
        assert lib.tmf_warp_pairs_kos(*args, None, None) == -1 and 'tmf_warp_pairs_kos' in lib.tmf_last_error().decode()
