"""CPU side of WARPLoss (no GPU): the NumPy reference the GPU tests compare the engine with (a linear scan per positive, values in
fp64), the problem generators both files use, the statements the GPU checks rest on - the prefix-maximum search finds the linear
scan's index, fp32 in the kernel's order of additions meets the value tolerance, and every one-step problem is *decided* (no
first-violator choice within fp32 reach of flipping) -, the plug-in's get_loss, a fit through the generic loop, the dispatch and its
refusals, save / load, and the C ABI of tmf_warp_pairs (declared, bound, built)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_step, rel_err

LR = 0.05
WARP_CHUNK, WARP_CAP = 64, 4096                 # csrc/tmf_warp.hip: WCHUNK, WCAP (the samples of a row the LDS form holds at once)


# ------------------------------------------------------------------------------------------------------------------------
# the reference: shares no code with the package
# ------------------------------------------------------------------------------------------------------------------------
def warp_pairs_ref(rowptr, val, p, sp, n_items, decide=np.float32):
    """tmf_warp_pairs on given scores: (delta [nnz], D [m, S], loss_part [m], first [nnz]).  One linear scan of the user's row per
    positive, in table order.  The decisions are made in ``decide`` exactly as defined - t = decide(p) - decide(1), sample s
    violates when decide(sp[u, s]) > t, strictly, NaN never -, the values are fp64.  first[k] is the first violator's index, -1
    where there is none or the stored value is <= 0."""
    rowptr, val = np.asarray(rowptr, np.int64), np.asarray(val, np.float64)
    pd, spd = np.asarray(p, decide), np.asarray(sp, decide)
    m, S = spd.shape
    delta, D, loss = np.zeros(val.shape[0]), np.zeros((m, S)), np.zeros(m)
    first = np.full(val.shape[0], -1, np.int64)
    one = decide(1)
    with np.errstate(invalid='ignore', over='ignore'):
        for u in range(m):
            for k in range(rowptr[u], rowptr[u + 1]):
                if not val[k] > 0:
                    continue
                t = decide(pd[k] - one)
                for s in np.flatnonzero(spd[u] > t)[:1]:              # the first sample above the threshold, if any
                    first[k] = s
                    n_trials = int(s) + 1
                    w = float(np.log(max(1, (int(n_items) - 1) // n_trials)))
                    if w > 0:
                        delta[k] = -w
                        D[u, s] += w
                        loss[u] += w * (1.0 - float(pd[k]) + float(spd[u, s]))
    return delta, D, loss, first


def _scores(U0, V0, idx, R):
    U, V = np.asarray(U0, np.float64), np.asarray(V0, np.float64)
    idx, R = np.asarray(idx, np.int64), np.asarray(R, np.int64)
    u, i = idx[:, 0], idx[:, 1]
    assert (np.diff(u * V.shape[0] + i) >= 0).all(), 'row-major pairs'
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=R.shape[0]))])
    return U, V, u, i, rowptr, np.einsum('kr,kr->k', U[u], V[i]), np.einsum('ur,usr->us', U, V[R])


def warp_closed_form(U0, V0, idx, val, R):
    """One WARPLoss epoch in fp64 (decisions in fp64 too: the dtype of the scores).  idx: row-major (user, item) pairs (the CSR
    order), R [m, S] the negative table, n_items = the rows of V0.
    -> (loss sum over the positives, delta [nnz], D [m, S] in R's order, gU, gV)."""
    U, V, u, i, rowptr, p, sp = _scores(U0, V0, idx, R)
    R = np.asarray(R, np.int64)
    m, S = R.shape
    delta, D, loss, _ = warp_pairs_ref(rowptr, val, p, sp, V.shape[0], decide=np.float64)
    gU = np.einsum('us,usr->ur', D, V[R])
    np.add.at(gU, u, delta[:, None] * V[i])
    gV = np.zeros_like(V)
    np.add.at(gV, R.reshape(-1), (D[:, :, None] * U[:, None, :]).reshape(m * S, -1))
    np.add.at(gV, i, delta[:, None] * U[u])
    return loss.sum(), delta, D, gU, gV


def warp_problem(seed, m, n, r, S, density=0.3):
    """bpr_problem's layout (tests/test_bpr_cpu.py): row-major COO pairs without duplicates; values from {-2, -1, 0, 1 .. 5}; user
    ``empty_user`` stores nothing, user ``nonpos_user`` only values <= 0; item ``empty_item`` is stored by nobody; an [m, S]
    negative table whose first column is one of the user's positives where it has one (negatives that coincide with positives
    are not filtered).  The tables are ~ N(0, 1.5 / sqrt(r)): a score has standard deviation 1.5 at every r, so that the margin
    of 1 neither always nor never holds and first violators spread over the row."""
    rng = np.random.default_rng(seed)
    mask = rng.random((m, n)) < density
    empty_user, nonpos_user, empty_item = m // 3, m // 2, n // 2
    mask[empty_user, :] = False
    mask[:, empty_item] = False
    idx = np.argwhere(mask)
    val = rng.choice(np.array([-2, -1, 0, 1, 2, 3, 4, 5], np.float32), idx.shape[0], p=[.06, .06, .08, .16, .16, .16, .16, .16])
    val[idx[:, 0] == nonpos_user] = -np.abs(val[idx[:, 0] == nonpos_user])
    R = rng.integers(0, n, (m, S))
    R[R == empty_item] = (empty_item + 1) % n      # the empty item's row moves only if somebody samples it: keep it still
    hits = 0
    for u in range(m):
        mine = idx[(idx[:, 0] == u) & (val > 0), 1]
        if mine.size:
            R[u, 0] = mine[rng.integers(mine.size)]
            hits += 1
    scale = np.sqrt(1.5) / r ** 0.25
    U0 = (rng.standard_normal((m, r)) * scale).astype(np.float32)
    V0 = (rng.standard_normal((n, r)) * scale).astype(np.float32)
    return dict(idx=idx, val=val, U0=U0, V0=V0, R=R.astype(np.int32), S=S, m=m, n=n, r=r, empty_user=empty_user, nonpos_user=nonpos_user,
                empty_item=empty_item, hits=hits)


def decidedness(U0, V0, idx, val, R):
    """(g_min, b) of a problem.  g_min: the smallest |sp[u, s] - t_k| over every comparison the definition makes - for each
    positive the samples up to and including its first violator, or the whole row where it has none.  b: the largest
    2 (r + 2) 2^-24 sum_i |u_i| |v_i| over the two dot products of any such comparison - what an fp32 evaluation of either score
    may be off by.  g_min > b: no fp32 evaluation can choose another first violator than fp64 does."""
    U, V, u, i, rowptr, p, sp = _scores(U0, V0, idx, R)
    R = np.asarray(R, np.int64)
    eps = 2.0 * (U.shape[1] + 2) * 2.0 ** -24
    b_p = eps * np.einsum('kr,kr->k', np.abs(U[u]), np.abs(V[i]))
    b_sp = eps * np.einsum('ur,usr->us', np.abs(U), np.abs(V[R]))
    g_min, b = np.inf, 0.0
    for k in np.flatnonzero(np.asarray(val) > 0):
        t = p[k] - 1.0
        above = np.flatnonzero(sp[u[k]] > t)
        upto = (above[0] + 1) if above.size else sp.shape[1]
        g_min = min(g_min, float(np.abs(sp[u[k], :upto] - t).min()))
        b = max(b, float(b_p[k]), float(b_sp[u[k], :upto].max()))
    return g_min, b


# (seed, m, n, r, S) of every one-step problem tests/test_gpu_warp.py runs through fit(): all decided (asserted below and there).
# 60 x 240: n >= 4 S at S = 5, so the weights log(floor(239 / N)) take several values; 60 x 40 with S = 64: n <= S, violators
# with N > n - 1 get w = 0.
GEOMETRY_PROBLEMS = {(1, 5): (2001, 60, 240, 1, 5), (7, 64): (7, 60, 240, 7, 64), (33, 70): (33, 60, 240, 33, 70), (64, 5): (64, 60, 240, 64, 5),
                     (128, 64): (128, 60, 240, 128, 64), (200, 70): (200, 60, 240, 200, 70), (256, 5): (2256, 60, 240, 256, 5)}
SMALL_CATALOG_PROBLEM = (2040, 60, 40, 33, 64)
BF16_PROBLEM = (133, 60, 240, 33, 64)
ADAM_PROBLEM = (8, 60, 240, 12, 20)
BIASED_PROBLEM = (1033, 60, 240, 33, 64)
FEATURES_PROBLEM = (2033, 60, 240, 33, 64)
L2_PROBLEM = (3033, 60, 240, 33, 64)
REPLAY_PROBLEM = (2006, 200, 150, 16, 32)
ONE_STEP_PROBLEMS = list(GEOMETRY_PROBLEMS.values()) + [SMALL_CATALOG_PROBLEM, ADAM_PROBLEM, BIASED_PROBLEM, L2_PROBLEM, REPLAY_PROBLEM]


def bf16_round(x):
    return torch.tensor(np.asarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def features_problem():
    """The item side over F = [I | tags] (hstack_identity): (problem, tag_idx, tag_val, F_dense, W0) - the embedding is E = F W0."""
    seed, m, n, r, S = FEATURES_PROBLEM
    T = 6
    p = warp_problem(seed, m, n, r, S)
    rng = np.random.default_rng(5)
    tag_idx = np.argwhere(rng.random((n, T)) < 0.3)
    tag_val = rng.choice(np.array([1.0, 0.5, -0.25, 2.0], np.float32), tag_idx.shape[0])
    F_dense = np.zeros((n, n + T))
    F_dense[np.arange(n), np.arange(n)] = 1.0
    F_dense[tag_idx[:, 0], n + tag_idx[:, 1]] = tag_val
    W0 = (rng.standard_normal((n + T, r)) * np.sqrt(1.5) / r ** 0.25 / 1.5).astype(np.float32)
    return p, tag_idx, tag_val, F_dense, W0


# the row lengths every kernel case holds: nothing, one, two, around half a chunk, a chunk of 64 and one more, two chunks + 3,
# only values <= 0 (5) and mixed signs (40) - tests/test_bpr_cpu.py's KERNEL_DEGREES
KERNEL_DEGREES = (0, 1, 2, 31, 32, 33, WARP_CHUNK, WARP_CHUNK + 1, 2 * WARP_CHUNK + 3, 5, 40)
KERNEL_S = (1, 63, 64, 65, 511, 512, 513, 1100, WARP_CAP + 5)
KERNEL_RANDOM_USERS = 33


def kernel_n_items(S):
    return 50 * S + 7        # floor((n - 1) / N) >= 50 for every N <= S: every violator has a weight, and the weights differ


def kernel_case(S, n_users=None, seed=0):
    """Synthetic inputs of tmf_warp_pairs -> (rowptr, val, p, sp, notes).  The first KERNEL_RANDOM_USERS users (or ``n_users`` of them
    and nothing else): user q has KERNEL_DEGREES[q % 11] stored entries - all positive but for the users with 5 (only values <= 0)
    and 40 (mixed signs, zeros among them) -, sp ~ N(0, 1) and p ~ N(2.5, 1), so that first violators spread over the row.  Then
    constructed rows, named in ``notes`` (name -> user):
      first@s   three positives whose first violator is exactly s, for s in 0, 63, 64, 65, S - 1 where S allows
      none      no violator anywhere
      equal     one positive with t = 1.5 exactly, sp == 1.5 at one place (not a violator) and 1.5 + 1 ulp at a later one (S >= 2)
      same      64 positives that all resolve to one s*
      distinct  min(64, S) positives that resolve to as many distinct s*, in shuffled lane order."""
    rng = np.random.default_rng(1000 * S + seed)
    f = np.float32
    rows, notes = [], {}                                     # (val, p, sp) per user
    for q in range(KERNEL_RANDOM_USERS if n_users is None else n_users):
        deg = KERNEL_DEGREES[q % len(KERNEL_DEGREES)]
        val = rng.integers(1, 6, deg).astype(f)
        if deg == 5:
            val = rng.choice(np.array([0, -1, -3], f), 5)
        elif deg == 40:
            val = rng.choice(np.array([-2, 0, 1, 4], f), 40)
        rows.append((val, (2.5 + rng.standard_normal(deg)).astype(f), rng.standard_normal(S).astype(f)))
    if n_users is None:
        def low(k):
            return (-3.0 * rng.random(k)).astype(f)                                   # in (-3, 0]: below every threshold used here
        for s in sorted({0, 63, 64, 65, S - 1}):
            if s < S:
                sp = np.concatenate([low(s), [f(10.0)], (3 * rng.standard_normal(S - s - 1)).astype(f)])
                notes[f'first@{s}'] = len(rows)
                rows.append((np.array([1, 0, 3, 5], f), np.array([2.0, 9.0, 2.5, 3.0], f), sp))
        notes['none'] = len(rows)
        rows.append((np.array([2, 4, 1], f), np.array([2.25, 2.5, 3.0], f), low(S)))
        if S >= 2:
            a, b = min(S // 3, S - 2), S - 1
            sp = low(S)
            sp[a], sp[b] = f(1.5), np.nextafter(f(1.5), f(2))
            notes['equal'] = len(rows)
            rows.append((np.array([1], f), np.array([2.5], f), sp))
        j = min(S - 1, 37)
        sp = np.concatenate([low(j), [f(5.0)], rng.standard_normal(S - j - 1).astype(f)])
        notes['same'] = len(rows)
        rows.append((np.ones(64, f), (2.0 + rng.random(64)).astype(f), sp))
        k = min(64, S)
        sp = np.concatenate([0.25 * np.arange(k), 8 * rng.standard_normal(S - k)]).astype(f)
        notes['distinct'] = len(rows)
        rows.append((np.ones(k, f), (0.25 * rng.permutation(k) - 0.125 + 1.0).astype(f), sp))   # t_k = 0.25 j - 0.125: s* = j
    rowptr = np.concatenate([[0], np.cumsum([v.shape[0] for v, _, _ in rows])]).astype(np.int64)
    val, p = (np.concatenate([row[i] for row in rows]).astype(f) if rows else np.zeros(0, f) for i in (0, 1))
    sp = np.stack([row[2] for row in rows]) if rows else np.zeros((0, S), f)
    return rowptr, val, p, sp, notes


def prefix_max_search(rowptr, val, p, sp):
    """first [nnz] as the kernel finds it: the inclusive prefix maximum of the row (NaN skipped), then a binary search for the
    first place where it is above t."""
    rowptr, val, p, sp = np.asarray(rowptr, np.int64), np.asarray(val, np.float32), np.asarray(p, np.float32), np.asarray(sp, np.float32)
    first = np.full(val.shape[0], -1, np.int64)
    for u in range(sp.shape[0]):
        M = np.maximum.accumulate(np.where(np.isnan(sp[u]), np.float32(-np.inf), sp[u]))
        for k in range(rowptr[u], rowptr[u + 1]):
            t = np.float32(p[k] - np.float32(1))
            if val[k] > 0 and not np.isnan(t):
                at = int(np.searchsorted(M, t, side='right'))       # M[at - 1] <= t < M[at]
                first[k] = at if at < M.shape[0] else -1
    return first


def _butterfly(v):
    """sum over 64 lanes as `for off in 32, 16, .., 1: v += shfl_xor(v, off)` leaves it in every lane, in v's dtype."""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[lanes ^ off]).astype(v.dtype)
    return v


def warp_pairs_fp32_kernel_order(rowptr, val, p, sp, n_items):
    """tmf_warp_pairs restated in NumPy fp32 with its order of additions: lane = place of the entry in its chunk of 64 stored
    entries; w = fp32 log of the fp32 quotient; within a chunk the distinct s* are taken in the order of their lowest lane, the w
    of the lanes that share one are added by the xor butterfly (zeros elsewhere; a single lane as it is) and the sum is added to
    D[u, s*]; chunks in ascending order.  The loss: w (sp[s*] - (p - 1)) in fp64 into the lane's accumulator, a butterfly at the end."""
    f = np.float32
    rowptr, val, p, sp = np.asarray(rowptr, np.int64), np.asarray(val, f), np.asarray(p, f), np.asarray(sp, f)
    m, S = sp.shape
    first = prefix_max_search(rowptr, val, p, sp)
    delta, D, loss = np.zeros(val.shape[0], f), np.zeros((m, S), f), np.zeros(m, f)
    for u in range(m):
        lacc = np.zeros(64, np.float64)
        for g0 in range(0, S, WARP_CAP):                             # segments outermost, as the kernel walks a long row
            for cb in range(rowptr[u], rowptr[u + 1], WARP_CHUNK):
                ks = np.arange(cb, min(cb + WARP_CHUNK, rowptr[u + 1]))
                w, sstar = np.zeros(64, f), np.full(64, -1, np.int64)
                for lane, k in enumerate(ks):
                    if g0 <= first[k] < g0 + WARP_CAP:
                        q = (int(n_items) - 1) // (int(first[k]) + 1)
                        w[lane] = np.log(f(q)) if q > 1 else f(0)
                        if w[lane] > 0:
                            sstar[lane] = first[k]
                            delta[k] = -w[lane]
                            lacc[lane] += np.float64(w[lane]) * (np.float64(sp[u, first[k]]) - (np.float64(p[k]) - 1.0))
                pending = sstar >= 0
                while pending.any():
                    leader = int(np.flatnonzero(pending)[0])
                    members = pending & (sstar == sstar[leader])
                    v = np.where(members, w, f(0)).astype(f)
                    D[u, sstar[leader]] = f(D[u, sstar[leader]] + (_butterfly(v)[leader] if members.sum() > 1 else v[leader]))
                    pending &= ~members
        loss[u] = f(_butterfly(lacc)[0])
    return delta, D, loss, first


# ------------------------------------------------------------------------------------------------------------------------
# the generators and the reference
# ------------------------------------------------------------------------------------------------------------------------
def _first_violators(p):
    """first [nnz] of a problem, in fp64."""
    _, _, _, _, rowptr, pk, sp = _scores(p['U0'], p['V0'], p['idx'], p['R'])
    return warp_pairs_ref(rowptr, p['val'], pk, sp, p['n'], decide=np.float64)[3]


def test_problem_generator():
    p = warp_problem(3, 60, 40, 7, 20)
    idx, val, R = p['idx'], p['val'], p['R']
    assert len({(int(u), int(i)) for u, i in idx}) == idx.shape[0] > 400 and (np.diff(idx[:, 0] * 40 + idx[:, 1]) > 0).all()
    assert (val > 0).any() and (val < 0).any() and (val == 0).any()
    assert p['empty_user'] not in idx[:, 0] and p['empty_item'] not in idx[:, 1] and p['empty_item'] not in R
    mine = idx[:, 0] == p['nonpos_user']
    assert mine.sum() >= 3 and (val[mine] <= 0).all()
    assert R.shape == (60, 20) and R.min() >= 0 and R.max() < 40 and p['hits'] >= 50
    pos = {(int(u), int(i)) for (u, i), a in zip(idx, val) if a > 0}
    assert sum((u, int(R[u, 0])) in pos for u in range(60)) == p['hits']
    for r in (1, 16, 256):                                           # a score has standard deviation about 1.5 at every r
        q = warp_problem(5, 60, 240, r, 5)
        sd = (q['U0'].astype(np.float64) @ q['V0'].astype(np.float64).T).std()
        assert 1.2 < sd < 1.8, (r, sd)


@pytest.mark.parametrize('problem', ONE_STEP_PROBLEMS + [BF16_PROBLEM], ids=lambda s: 'x'.join(map(str, s)))
def test_first_violators_spread_over_the_rows(problem):
    """Every shape the GPU file uses really searches: at least a quarter of the positives need a second trial, some go past the
    first 64 samples where the row is longer than that, and at least one finds no violator at all."""
    seed, m, n, r, S = problem
    p = warp_problem(seed, m, n, r, S)
    first = _first_violators(p)[p['val'] > 0]
    trials = np.where(first < 0, S + 1, first + 1)
    print(f'[spread] {problem}: N >= 2: {(trials >= 2).mean():.2f}, N > 64: {int(((first >= 64)).sum())}, none: {int((first < 0).sum())}')
    assert (trials >= 2).mean() >= 0.25 and (first < 0).any()
    if S > 64:
        assert (first >= 64).any()
    if n <= S:
        assert (first + 1 > n - 1).any(), 'violators with N > n - 1: weight 0'
    if n >= 4 * S:
        _, delta, _, _, _ = warp_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
        assert np.unique(delta[delta < 0]).size >= min(S, 3)


def test_kernel_cases_hold_what_they_promise():
    for S in KERNEL_S:
        rowptr, val, p, sp, notes = kernel_case(S)
        deg = np.diff(rowptr)
        assert set(KERNEL_DEGREES) <= set(deg[:KERNEL_RANDOM_USERS].tolist()) and sp.shape == (rowptr.shape[0] - 1, S)
        first = warp_pairs_ref(rowptr, val, p, sp, kernel_n_items(S))[3]
        rows = {name: first[rowptr[u]:rowptr[u + 1]][val[rowptr[u]:rowptr[u + 1]] > 0] for name, u in notes.items()}
        for s in (0, 63, 64, 65, S - 1):
            if s < S:
                assert rows[f'first@{s}'].tolist() == [s, s, s]
        assert (rows['none'] == -1).all() and rows['none'].size == 3
        if S >= 2:
            assert rows['equal'].tolist() == [S - 1] and sp[notes['equal'], min(S // 3, S - 2)] == np.float32(1.5)
        assert rows['same'].size == 64 and np.unique(rows['same']).tolist() == [min(S - 1, 37)]
        assert sorted(rows['distinct'].tolist()) == list(range(min(64, S))) and rows['distinct'].tolist() != list(range(min(64, S))) or S == 1
        rnd = first[:rowptr[KERNEL_RANDOM_USERS]][val[:rowptr[KERNEL_RANDOM_USERS]] > 0]
        if S >= 63:                                                  # the random rows: spread over the row, and some without a violator
            assert (rnd >= 8).mean() > 0.1 and (rnd < 0).any() and np.unique(rnd).size > 20
        if S > WARP_CAP:
            assert (rnd >= WARP_CAP).any() or (first >= WARP_CAP).sum() >= 3


def test_closed_form_on_a_problem_small_enough_to_write_out():
    """One user, two positives and a stored zero, three negatives, five items: every number by hand."""
    U0 = np.array([[1.0, 0.0]])
    V0 = np.array([[2.0, 0.0], [0.0, 1.0], [0.25, 3.0], [0.5, 0.5], [1.5, -1.0]])      # scores of the user: 2, 0, 0.25, 0.5, 1.5
    idx, val, R = np.array([[0, 0], [0, 1], [0, 2]]), np.array([1.0, 0.0, 3.0]), np.array([[3, 1, 4]])   # sp = 0.5, 0, 1.5
    loss, delta, D, gU, gV = warp_closed_form(U0, V0, idx, val, R)
    # positive 0: p = 2, t = 1: 0.5 and 0 do not violate, 1.5 does: N = 3, w = log(floor(4 / 3)) = log 1 = 0 - nothing
    # positive 2: p = 0.25, t = -0.75: 0.5 violates at once: N = 1, w = log 4, loss = log 4 (1 - 0.25 + 0.5)
    w = np.log(4.0)
    assert rel_err(loss, w * 1.25) < 1e-15
    assert np.array_equal(delta, [0.0, 0.0, -w]) and np.array_equal(D, [[w, 0.0, 0.0]])
    assert rel_err(gU, [w * V0[3] - w * V0[2]]) < 1e-15
    assert rel_err(gV, [0 * U0[0], 0 * U0[0], -w * U0[0], w * U0[0], 0 * U0[0]]) < 1e-15
    # with 9 items positive 0 counts too: w = log(floor(8 / 3)) = log 2 against the third sample, positive 2 gets log 8
    V9 = np.concatenate([V0, np.zeros((4, 2))])
    loss, delta, D, _, _ = warp_closed_form(U0, V9, idx, val, R)
    assert rel_err(loss, np.log(2.0) * (1 - 2 + 1.5) + np.log(8.0) * 1.25) < 1e-15
    assert np.array_equal(delta, [-np.log(2.0), 0.0, -np.log(8.0)]) and np.array_equal(D, [[np.log(8.0), 0.0, np.log(2.0)]])
    _, _, _, first = warp_pairs_ref([0, 3], val, [2.0, 0.0, 0.25], [[0.5, 0.0, 1.5]], 9)
    assert first.tolist() == [2, -1, 0]


def test_the_comparison_is_strict_and_made_against_the_rounded_threshold():
    one, up = np.float32(1.5), np.nextafter(np.float32(1.5), np.float32(2))
    assert warp_pairs_ref([0, 1], [1.0], [2.5], [[one, one]], 100)[3].tolist() == [-1]           # sp == t: not a violator
    assert warp_pairs_ref([0, 1], [1.0], [2.5], [[one, up]], 100)[3].tolist() == [1]
    # p = 1 + 2^-24 + 2^-47 rounds to 1 + 2^-23 in fp32: there t = 2^-23 and the sample 2^-24 + 2^-46 (exact in fp32) is below
    # it; in fp64 t = 2^-24 + 2^-47 and the same sample is above it - the threshold is rounded once, in the dtype of the scores
    p, s = 1.0 + 2.0 ** -24 + 2.0 ** -47, 2.0 ** -24 + 2.0 ** -46
    assert warp_pairs_ref([0, 1], [1.0], [p], [[s]], 100, decide=np.float64)[3].tolist() == [0]
    assert warp_pairs_ref([0, 1], [1.0], [p], [[s]], 100)[3].tolist() == [-1]
    nan = float('nan')
    assert warp_pairs_ref([0, 2], [1.0, 1.0], [nan, 2.5], [[nan, 9.0]], 100)[3].tolist() == [-1, 1]   # NaN never violates


def _get_loss(U, V, idx, val, R, dtype=torch.float64):
    """(per-positive losses, dL/dU, dL/dV) of WARPLoss.get_loss fed as _fit_generic feeds it, by autograd."""
    from teamoflow_amd.mf.loss_graphs import WARPLoss
    from teamoflow_amd.mf.sparse import SparseInteractions
    U, V = (torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in (U, V))
    inter = SparseInteractions(idx, val, (U.shape[0], V.shape[0]), device='cpu')
    pred = U @ V.T
    out = WARPLoss().get_loss(tf_interactions=inter, tf_sample_predictions=torch.gather(pred, 1, torch.as_tensor(R, dtype=torch.int64)),
                              tf_prediction_serial=pred[inter.indices[:, 0], inter.indices[:, 1]], predictions=None,
                              n_items=V.shape[0], n_samples=R.shape[1])
    gU, gV = torch.autograd.grad(out.sum(), (U, V))
    return out.detach().numpy(), gU.numpy(), gV.numpy()


def test_class_surface():
    import inspect
    import teamoflow.mf.loss_graphs as alias
    from teamoflow_amd.mf import loss_graphs as LG
    assert alias.WARPLoss is LG.WARPLoss and issubclass(LG.WARPLoss, LG.LossGraph)
    assert not issubclass(LG.WARPLoss, (LG.WMRBLoss, LG.BPRLoss))
    assert inspect.signature(LG.WARPLoss.get_loss) == inspect.signature(LG.BPRLoss.get_loss)


@pytest.mark.parametrize('shape', [(33, 47, 5, 12), (60, 40, 7, 1), (20, 15, 3, 40)], ids=lambda s: 'x'.join(map(str, s)))
def test_get_loss_is_the_closed_form(shape):
    m, n, r, S = shape
    p = warp_problem(11 + S, m, n, r, S)
    loss, delta, D, gU, gV = warp_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    out, aU, aV = _get_loss(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    assert out.shape == (int((p['val'] > 0).sum()),) and out.dtype == np.float64
    assert rel_err(out.sum(), loss) < 1e-12 and rel_err(aU, gU) < 1e-12 and rel_err(aV, gV) < 1e-12
    assert loss > 0 and (D > 0).any()
    assert not gU[p['empty_user']].any() and not gU[p['nonpos_user']].any() and not gV[p['empty_item']].any()
    assert not delta[p['val'] <= 0].any() and (delta[p['val'] > 0] <= 0).all() and not D[p['nonpos_user']].any()
    assert ((D > 0).sum(1) <= np.bincount(p['idx'][p['val'] > 0, 0], minlength=m)).all()      # at most one entry of D per positive


def test_get_loss_with_infinite_and_nan_scores():
    """No violator next to an infinite or NaN sample: the loss of that positive is 0, not NaN."""
    from teamoflow_amd.mf.loss_graphs import WARPLoss
    from teamoflow_amd.mf.sparse import SparseInteractions
    inter = SparseInteractions(np.array([[0, 0], [0, 1]]), np.array([1.0, 2.0]), (1, 3), device='cpu')
    sp = torch.tensor([[-np.inf, np.nan, 0.5]], dtype=torch.float64)
    out = WARPLoss().get_loss(tf_interactions=inter, tf_sample_predictions=sp, tf_prediction_serial=torch.tensor([9.0, 1.0], dtype=torch.float64),
                              n_items=100, n_samples=3)
    assert out.tolist() == pytest.approx([0.0, float(np.log(33.0)) * (1 - 1.0 + 0.5)], rel=1e-15)


# ------------------------------------------------------------------------------------------------------------------------
# what the GPU file's checks rest on
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', KERNEL_S)
def test_prefix_maximum_search_is_the_linear_scan(S):
    rowptr, val, p, sp, _ = kernel_case(S)
    assert np.array_equal(prefix_max_search(rowptr, val, p, sp), warp_pairs_ref(rowptr, val, p, sp, kernel_n_items(S))[3])
    sp2, p2 = sp.copy(), p.copy()                                    # and with NaN and infinite samples and scores in the way
    rng = np.random.default_rng(S)
    sp2[rng.random(sp.shape) < 0.05] = np.nan
    sp2[rng.random(sp.shape) < 0.01] = np.inf
    sp2[rng.random(sp.shape) < 0.02] = -np.inf
    p2[rng.random(p.shape) < 0.05] = np.nan
    assert np.array_equal(prefix_max_search(rowptr, val, p2, sp2), warp_pairs_ref(rowptr, val, p2, sp2, kernel_n_items(S))[3])


@pytest.mark.parametrize('S', KERNEL_S)
def test_fp32_in_the_kernels_order_meets_the_gpu_tolerance(S):
    """What tests/test_gpu_warp.py asks of the kernel - the reference's first violators exactly, rel_err < 1e-5 for delta, D and
    the loss on kernel_case(S) - is reachable: fp32 arithmetic in the kernel's order of additions gets there on the same inputs."""
    rowptr, val, p, sp, _ = kernel_case(S)
    for n_items in (kernel_n_items(S), max(S, 2)):
        ref, got = warp_pairs_ref(rowptr, val, p, sp, n_items), warp_pairs_fp32_kernel_order(rowptr, val, p, sp, n_items)
        errs = [rel_err(g, r) for g, r in zip(got[:3], ref[:3])]
        print(f'[fp32, kernel order] S={S} n_items={n_items}: delta {errs[0]:.3g} D {errs[1]:.3g} loss {errs[2]:.3g}')
        assert np.array_equal(got[3], ref[3])
        assert max(errs) < 1e-5 and all(g.dtype == np.float32 and np.isfinite(g).all() for g in got[:3])
        assert np.array_equal(got[1] != 0, ref[1] != 0)


@pytest.mark.parametrize('problem', ONE_STEP_PROBLEMS, ids=lambda s: 'x'.join(map(str, s)))
def test_one_step_problems_are_decided(problem):
    seed, m, n, r, S = problem
    p = warp_problem(seed, m, n, r, S)
    g_min, b = decidedness(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    print(f'[decided] {problem}: smallest gap {g_min:.3g}, fp32 reach {b:.3g}')
    assert g_min > b


def test_the_bf16_and_the_featured_problem_are_decided():
    seed, m, n, r, S = BF16_PROBLEM
    p = warp_problem(seed, m, n, r, S)
    g_min, b = decidedness(bf16_round(p['U0']), bf16_round(p['V0']), p['idx'], p['val'], p['R'])
    assert g_min > b, (g_min, b)
    p, _, _, F_dense, W0 = features_problem()
    g_min, b = decidedness(p['U0'], F_dense @ W0.astype(np.float64), p['idx'], p['val'], p['R'])
    assert g_min > b, (g_min, b)


def test_decidedness_sees_a_gap_within_reach():
    """A problem with one comparison 1e-9 from its threshold is not decided, whatever the rest looks like."""
    U0, V0 = np.array([[1.0, 0.5]]), np.array([[2.0, 0.0], [1.0 + 1e-9, 0.0], [0.0, 1.0]])
    idx, val = np.array([[0, 0]]), np.array([1.0])
    g_min, b = decidedness(U0, V0, idx, val, np.array([[2, 1]]))
    assert abs(g_min - 1e-9) < 1e-12 and b > 2e-7 > g_min
    g_min, b = decidedness(U0, V0, idx, val, np.array([[2, 2]]))           # sp = 0.5 twice, t = 1: gap 0.5
    assert g_min == 0.5 > b


# ------------------------------------------------------------------------------------------------------------------------
# the model without a GPU
# ------------------------------------------------------------------------------------------------------------------------
def _model(p, loss=None, table=True, **attrs):
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import WARPLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    model = MatrixFactorization(p['r'], loss_graph=loss or WARPLoss(), user_weight_graph=FixedInitializer(p['U0']),
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


GENERIC_PROBLEM = (2014, 30, 20, 4, 8)


def test_generic_fit_without_a_gpu(monkeypatch):
    """30 x 20, r = 4, S = 8 through _fit_generic on a decided problem: the first loss is the closed form's mean over the
    positives, one step moves the tables as the closed-form gradients say, and 20 epochs end below where they began (the
    objective is discontinuous: a single epoch may rise, so nothing is asked of consecutive epochs)."""
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    p = warp_problem(*GENERIC_PROBLEM)
    g_min, b = decidedness(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    assert g_min > b
    model = _fit(_model(p), p, 20)
    h = model.loss_history_
    assert not hasattr(model, '_state') and len(h) == 20 and h[-1] < h[0], h
    loss, _, _, gU, gV = warp_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    assert rel_err(h[0], loss / int((p['val'] > 0).sum())) < 1e-5
    one = _fit(_model(p), p, 1)
    assert_step(one.user_embedding.detach().numpy(), p['U0'], gU, LR, rtol=1e-5, what='U')
    assert_step(one.item_embedding.detach().numpy(), p['V0'], gV, LR, rtol=1e-5, what='V')


def test_no_sample_table(monkeypatch):
    from teamoflow_amd.mf.matrix_factorization import SampleTableMissing
    p = warp_problem(15, 12, 9, 4, 4)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(SampleTableMissing, match='WARPLoss'):
        _fit(_model(p, table=False), p, 1)


def test_loss_name_and_dispatch(monkeypatch):
    from teamoflow_amd import _engine
    from teamoflow_amd.mf import loss_graphs as LG
    from teamoflow_amd.mf.sparse import eye

    class MyWARP(LG.WARPLoss):
        pass
    assert _engine.loss_name(LG.WARPLoss()) == 'warp' and 'warp' in _engine.PAIR_LOSSES and 'bpr' in _engine.PAIR_LOSSES
    with pytest.raises(TypeError, match='WARPLoss'):
        _engine.loss_name(MyWARP())
    p = warp_problem(16, 12, 9, 4, 4)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    for settings in ({}, dict(factor_dtype=torch.bfloat16), dict(optimizer='adam')):
        assert _model(p, **settings)._route(eye(12), eye(9)) == 'engine', settings
    assert _model(p, loss=MyWARP())._route(eye(12), eye(9)) == 'generic'
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    assert _model(p)._route(eye(12), eye(9)) == 'generic'


def test_a_warp_epoch_needs_a_sliced_plan():
    """The one-kernel user pass has the hinge built in: a state without a sliced plan is refused, never run as WMRB."""
    from teamoflow_amd import _engine

    class Plan:
        sliced = False

    class State:
        wplan = Plan()
        plan = r = None
    with pytest.raises(ValueError, match="'warp' on a state without a sliced WmrbPlan"):
        _engine.run_epoch(State(), None, None, 'warp')
    with pytest.raises(ValueError, match='pairs=warp needs the sliced user pass'):
        _engine.epoch_wmrb(State(), None, 0.0, None, pairs='warp')


def test_the_plan_keeps_the_table_order_of_the_samples():
    """The sliced pass sorts every user's negatives by item; WARP tries them in the table's order.  sample_rank() maps a place of
    the plan's row to its place in the model's row - also past 32767 samples, where 16 bits only hold it unsigned."""
    from teamoflow_amd import _engine
    for n, S in ((40, 64), (70000, 40000)):
        m = 3
        R = torch.randint(0, n, (m, S), generator=torch.Generator().manual_seed(S)).to(torch.int32)
        idx = torch.tensor([[0, 1], [2, 0]])
        plan = _engine.InteractionPlan(idx, torch.tensor([1.0, 2.0]), m, n)
        w = _engine.WmrbPlan(plan, R, item_slices=2, n_components=8, sliced=True, item_lists=False)
        rank = w.sample_rank()
        assert rank.dtype == torch.int16 and rank.shape == (m, S) and w.sample_rank() is rank
        table_index = torch.from_numpy(rank.numpy().view(np.uint16).astype(np.int64))
        assert torch.equal(torch.sort(table_index, dim=1)[0], torch.arange(S).expand(m, S))          # a permutation of every row
        assert torch.equal(torch.gather(R, 1, table_index), w.R) and (w.R[:, 1:] >= w.R[:, :-1]).all()
    flat = _engine.WmrbPlan(plan, R[:, :5].contiguous(), n_components=8, sliced=False, item_lists=False)
    assert flat.sample_rank().tolist() == [list(range(5))] * 3


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
    with pytest.raises(NotImplementedError, match=f'WARPLoss with {setting[0]}'):
        _fit(_model(p, **{setting[0]: setting[1]}), p, 1)


def test_save_and_load(tmp_path, monkeypatch):
    from teamoflow_amd.mf.loss_graphs import WARPLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    p = warp_problem(18, 12, 9, 4, 4)
    model = _fit(_model(p), p, 2)
    path = str(tmp_path / 'model.pt')
    model.save(path)
    back = MatrixFactorization.load(path, device='cpu')
    assert type(back.loss_graph) is WARPLoss and back.loss_history_ == model.loss_history_
    assert torch.equal(back.user_embedding, model.user_embedding.detach()) and torch.equal(back.random_ind.cpu(), model.random_ind)
    again = _fit(back, p, 2)                                            # a loaded model trains again, through the same path
    assert again.loss_history_ == model.loss_history_


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_built():
    from teamoflow_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tmf.h')).read()
    declared = set(re.findall(r'\b(tmf_[a-z0-9_]+)\s*\(', header))
    lib = _lib.load_library()
    for name in ('tmf_warp_pairs', 'tmf_warp_pairs_ranked'):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    # tmf_bpr_pairs's arguments and n_items; the ranked form: and the ranks
    assert len(_lib.SIGNATURES['tmf_warp_pairs'][1]) == len(_lib.SIGNATURES['tmf_bpr_pairs'][1]) + 1
    assert len(_lib.SIGNATURES['tmf_warp_pairs_ranked'][1]) == len(_lib.SIGNATURES['tmf_warp_pairs'][1]) + 1
    make = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS :=.*\btmf_warp\.hip\b', make, re.M)
    source = open(os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'tmf_warp.hip')).read()
    assert re.search(rf'\bWCAP = {WARP_CAP};', source) and re.search(rf'\bWCHUNK = {WARP_CHUNK};', source)


def test_argument_checks_fail_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail differently; these return first."""
    import ctypes
    from teamoflow_amd import _lib
    lib = _lib.load_library()
    host = (ctypes.c_double * 8)()              # stands for any non-null buffer: never dereferenced
    H, i32 = ctypes.cast(host, ctypes.c_void_p), ctypes.c_int32
    assert lib.tmf_warp_pairs(None, None, None, None, i32(0), i32(8), i32(9), None, None, None, None, None) == 0     # no users: nothing to do
    for args in ((None, H, H, H, i32(3), i32(8), i32(9), H, H, H), (H, H, H, None, i32(3), i32(8), i32(9), H, H, H),
                 (H, H, H, H, i32(3), i32(8), i32(9), H, None, H), (H, H, H, H, i32(3), i32(0), i32(9), H, H, H),
                 (H, H, H, H, i32(-1), i32(8), i32(9), H, H, H), (H, H, H, H, i32(3), i32(8), i32(0), H, H, H)):
        assert lib.tmf_warp_pairs(*args, None, None) == -1 and 'warp_pairs' in lib.tmf_last_error().decode()
        assert lib.tmf_warp_pairs_ranked(*args[:4], H, *args[4:], None, None) == -1 and 'warp_pairs_ranked' in lib.tmf_last_error().decode()
    assert lib.tmf_warp_pairs_ranked(None, None, None, None, None, i32(0), i32(8), i32(9), None, None, None, None, None) == 0
    assert lib.tmf_warp_pairs_ranked(H, H, H, H, None, i32(3), i32(8), i32(9), H, H, H, None, None) == -1          # no ranks
    assert lib.tmf_warp_pairs_ranked(H, H, H, H, H, i32(3), i32(65537), i32(9), H, H, H, None, None) == -1         # ranks are 16 bits
