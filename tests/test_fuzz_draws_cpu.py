"""The random problems of tests/test_gpu_fuzz_scores7.py (draw_s7: WMRB epochs whose scores come from the item-run kernel
tmf_wmrb_scores7 / tmf_wmrb_scores7_fill_f32 under random forms of every other pass) and of tests/test_gpu_fuzz_pairs.py (draw_pairs:
BPR, WARP and the sampled softmax on scores3 / scores6 / scores7 under the same random forms) - and, without a GPU, what those files
rest on: over the default seed range the draws reach every value they promise, the Scores7Plan of every draw_s7 problem passes the
brute-force invariants of tests/test_scores7_cpu.py and tests/test_scores7_fill_cpu.py, every WARP problem is decided (no
first-violator choice within fp32 reach of flipping), and fp32 arithmetic in the pair kernels' order of additions meets, on every
draw_pairs problem, the tolerances the GPU file asks of the engine."""
import os

import numpy as np
import pytest
import torch

from conftest import assert_step, rel_err
from teamoflow_amd._engine import SWITCHES
from test_bpr_cpu import bpr_closed_form, bpr_pairs_fp32_kernel_order, bpr_problem, fresh_adam_fp32
from test_softmax_cpu import softmax_closed_form, softmax_pairs_fp32_kernel_order, sum_identity_gaps
from test_warp_cpu import decidedness, warp_closed_form, warp_pairs_fp32_kernel_order, warp_problem

N_SEEDS = int(os.environ.get('TMF_FUZZ_SEEDS', '24'))
DEFAULT_SEEDS = 24
LR = 0.05

# every variable that chooses a form of a pass: a test clears them all before it sets its own
FORM_KEYS = tuple(k for k, (_, form) in SWITCHES.items() if form)   # declared once, beside their one reader

S7_R = (65, 72, 96, 100, 127, 128)                    # the widths tmf_wmrb_scores7 exists for: both ends, pad columns, none
S7_SLOTS = (1, 3, 4, 64, 100, 512, None)              # TMF_S7_SLOTS; None = unset (the library's buffer)
S7_SLICE_BYTES = (512, 37 * 512, 300 * 512, None)     # TMF_S7_SLICE_BYTES: one row per slice, 37 rows, 300 rows, unset (one slice here)
S7_BORDER_M = (1, 4, 255, 256, 257, 511, 512, 513)    # users around the borders of the groups of 256

PAIR_KINDS = ('bpr', 'warp', 'softmax', 'softmax_scaled')
PAIR_R = (16, 32, 64, 100, 128, 160, 256)
PAIR_R_S7 = (100, 128)                                # those of PAIR_R for which tmf_wmrb_scores7_supported answers 1
MAX_STORED = 3600                                     # ~ 2900 of them positive

# The problem seeds of the WARP draws: walk_warp_seeds(30) - candidates 0, 1, 2 ... in ascending order, a candidate is kept when
# its problem is decided (test_warp_cpu.decidedness: g_min > b).  test_the_warp_seeds_are_the_walk repeats the walk and counts
# the candidates it rejected: 7 of 37.
WARP_SEEDS = (0, 1, 2, 5, 6, 7, 8, 9, 11, 12, 13, 14, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 28, 29, 30, 31, 32, 33, 34, 36)


def _lib_and_engine():
    import __graft_entry__ as ge
    from teamoflow_amd import _engine as E, _lib
    ge.build()
    return _lib.load_library(), E


@pytest.fixture(scope='module', autouse=True)
def built():
    """The library is built before any test of this file draws (the GPU files that import the draws run on a built tree)."""
    _lib_and_engine()


@pytest.fixture(autouse=True)
def no_ambient_forms(monkeypatch):
    """No form variable of the caller's environment reaches a plan built here: Scores7Plan reads TMF_S7_SLOTS and
    TMF_S7_SLICE_BYTES before its arguments."""
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)


def _common_forms(rng, env):
    """The forms of the gather kernels and the item pass, as test_gpu_fuzz_forms.draw draws them."""
    env['TMF_ITEM_SLICES'] = str(int(rng.integers(1, 10)))
    env['TMF_USER_CHUNKS'] = str(int(rng.integers(1, 7)))
    env['TMF_ROWS4'] = str(int(rng.integers(0, 2)))
    env['TMF_ROWS5'] = str(int(rng.integers(0, 2)))
    if rng.integers(0, 2):
        env['TMF_ROWS5_TARGET'] = str(int(rng.choice([1, 2, 5, 20, 1000])))
    env['TMF_ROW_STATIONARY'] = str(int(rng.integers(0, 2)))
    if rng.integers(0, 3) == 0:
        env['TMF_SLICE_XCD'] = str(int(rng.integers(0, 2)))


def _s7_forms(rng, env, slice_bytes, slots):
    for name, v in (('TMF_S7_SLICE_BYTES', slice_bytes), ('TMF_S7_SLOTS', slots)):
        if v is not None:
            env[name] = str(v)
    env['TMF_S7_FILL'] = str(int(rng.integers(0, 2)))


def draw_s7(seed):
    """A WMRB problem with the patterns of test_gpu_fuzz_forms.draw - n <= 32 S, a popular item and a heavy user every fourth seed,
    permuted COO every fifth, a popular negative that repeats an id inside a row every fourth - and, every third seed, every user's
    first sample replaced by one of its own positives: that (user, item) pair sits in one item run twice, as interaction and as
    negative.  fp32; the width, the slots and the slice size walk through their lists so that a range of 24 seeds holds each;
    m around a group border every third seed.  -> (m, n, r, S, idx, val, R, U, V, dtype, env) as draw returns it."""
    rng = np.random.default_rng(66000 + seed)
    r = S7_R[seed % len(S7_R)]
    slots = S7_SLOTS[seed % len(S7_SLOTS)]
    slice_bytes = S7_SLICE_BYTES[(seed + seed // 4) % len(S7_SLICE_BYTES)]
    m = S7_BORDER_M[(seed // 3) % len(S7_BORDER_M)] if seed % 3 == 0 else int(rng.integers(1, 701))
    n = int(rng.integers(3, 900))
    S = int(rng.integers(1, min(n, 48) + 1))
    n = max(3, min(n, 32 * S))   # c = n / S multiplies every rounding of a score (the tolerance of test_gpu_fuzz_forms)
    S = min(S, n)
    nnz = int(rng.integers(1, 6 * m + 2))
    u, j = rng.integers(0, m, nnz), rng.integers(0, n, nnz)
    if seed % 4 == 1:                                            # a popular item (a long list) and a heavy user
        u = np.concatenate([u, np.arange(m), np.zeros(min(n, 300), np.int64)])
        j = np.concatenate([j, np.full(m, int(rng.integers(0, n))), np.arange(min(n, 300))])
    key = np.unique(u.astype(np.int64) * n + j)
    if seed % 5 == 0:
        key = rng.permutation(key)                               # the engine must not rely on row-major order
    idx = np.stack([key // n, key % n], 1)
    val = rng.integers(-1, 6, len(key)).astype(np.float32)
    if not (val > 0).any():
        val[0] = 1.0
    R = np.stack([rng.choice(n, S, replace=False) for _ in range(m)]).astype(np.int32)
    if seed % 4 == 3:
        R[::2, 0] = n - 1                                        # a popular NEGATIVE (may repeat an id within a row: allowed)
    if seed % 3 == 1:                                            # a positive of the user among its own negatives
        for a in range(m):
            mine = idx[(idx[:, 0] == a) & (val > 0), 1]
            if mine.size:
                R[a, 0] = mine[rng.integers(mine.size)]
    U = (rng.standard_normal((m, r)) * 0.3).astype(np.float32)
    V = (rng.standard_normal((n, r)) * 0.3).astype(np.float32)
    env = {'TMF_FORCE_SLICED': '1', 'TMF_SCORES5': '0', 'TMF_SCORES6': '0', 'TMF_SCORES7': '1'}
    _common_forms(rng, env)
    _s7_forms(rng, env, slice_bytes, slots)
    return m, n, r, S, idx, val, R, U, V, torch.float32, env


def _s7_args(env):
    """(slice_bytes, slots, item_slices) of a drawn environment, for a Scores7Plan built without the environment."""
    return (int(env['TMF_S7_SLICE_BYTES']) if 'TMF_S7_SLICE_BYTES' in env else None,
            int(env['TMF_S7_SLOTS']) if 'TMF_S7_SLOTS' in env else None, int(env['TMF_ITEM_SLICES']))


def _pair_problem(kind, problem_seed, r):
    """m 3 .. 600, n 40 .. 700, S 1 .. 48, at most ~MAX_STORED stored pairs; the generators of the pair losses' own tests: ids repeat
    inside a row of R, every user's first sample is one of its positives, one user stores nothing, one only values <= 0, one item
    is stored and sampled by nobody."""
    rng = np.random.default_rng(88000 + problem_seed)
    m, n, S = int(rng.integers(3, 601)), int(rng.integers(40, 701)), int(rng.integers(1, 49))
    make = warp_problem if kind == 'warp' else bpr_problem
    return make(problem_seed, m, n, r, S, density=min(0.3, MAX_STORED / (m * n)))


def draw_pairs(seed, warp_seed=None):
    """kind k = seed % 4 of PAIR_KINDS; round i = seed // 4.  Every third round is a scores7 round: r walks through the widths the
    kernel exists for (PAIR_R_S7[(i + k) % 2]) and the scores form is scores7; in the other rounds r walks through all of PAIR_R
    (PAIR_R[(4 i + k) % 7]: a range of 24 seeds holds each) and the form is drawn from scores3, scores6 and scores7 where the library
    supports them at that r.  A WARP problem is drawn from WARP_SEEDS[i] (``warp_seed`` instead: the walk that
    chose the tuple), any other from the seed itself.  The forms of the other passes as draw_s7 draws them.  ``permute``: the engine
    gets the COO pairs in a permuted order (``order``); the closed forms always take idx / val as they are, row-major.
    -> dict(kind, c, p = the problem, form, env, permute, order)."""
    from teamoflow_amd import _lib
    lib = _lib.load_library()
    k, i = seed % 4, seed // 4
    kind = PAIR_KINDS[k]
    if kind == 'warp':
        i %= len(WARP_SEEDS) if warp_seed is None else 1 << 30       # a soak past the tuple walks it again, under other forms
        problem_seed = WARP_SEEDS[i] if warp_seed is None else warp_seed
    else:
        problem_seed = seed
    s7_turn = i % 3 == 0
    p = _pair_problem(kind, problem_seed, PAIR_R_S7[(i + k) % len(PAIR_R_S7)] if s7_turn else PAIR_R[(4 * i + k) % len(PAIR_R)])
    m, n, r, S = p['m'], p['n'], p['r'], p['S']
    rng = np.random.default_rng(89000 + seed)
    env = {'TMF_FORCE_SLICED': '1', 'TMF_SCORES5': '0'}
    _common_forms(rng, env)
    forms = ['s3'] + ['s6'] * bool(lib.tmf_wmrb_scores6_supported(r, 0, n)) + ['s7'] * bool(lib.tmf_wmrb_scores7_supported(r, 0, n))
    form = 's7' if s7_turn else str(rng.choice(forms))
    assert form in forms
    env['TMF_SCORES6'], env['TMF_SCORES7'] = str(int(form == 's6')), str(int(form == 's7'))
    if form == 's6' and rng.integers(0, 2):
        env['TMF_S6_SLICE_BYTES'] = str(int(rng.choice([512, 4096, 50000, 1 << 20])))
    if form == 's7':
        _s7_forms(rng, env, S7_SLICE_BYTES[int(rng.integers(0, len(S7_SLICE_BYTES)))], S7_SLOTS[int(rng.integers(0, len(S7_SLOTS)))])
    permute = bool((i + seed) % 2)
    order = rng.permutation(len(p['val'])) if permute else np.arange(len(p['val']))
    c = n / S if kind == 'softmax_scaled' else 1.0
    return dict(kind=kind, c=c, p=p, form=form, env=env, permute=permute, order=order, seed=seed)


def dyadic_pair_seed(t):
    """The draw_pairs seed of case t of the dyadic test of tests/test_gpu_fuzz_pairs.py: kind t % 4; the first four cases are
    scores7 rounds, one per kind; the later ones walk through the rounds.  WARP draws from its own seeds."""
    k, j = t % 4, 0 if t < 4 else t - 3
    return 4 * j + 1 if k == 1 else 7008 + 4 * j + k             # 7008 / 4 is a multiple of 3: round j of either is a scores7 round with j


def closed_form(d):
    """(loss sum, delta, D in the table's order, gU, gV) of a draw_pairs problem in fp64, on the tables as given."""
    p, kind = d['p'], d['kind']
    if kind == 'bpr':
        return bpr_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    if kind == 'warp':
        return warp_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    return softmax_closed_form(p['U0'], p['V0'], p['idx'], p['val'], p['R'], d['c'])


def walk_warp_seeds(count):
    """-> (the first ``count`` decided candidates, candidates rejected on the way): candidate c is tried as the problem of round
    i = the number kept so far."""
    kept, rejected, c = [], 0, 0
    while len(kept) < count:
        p = draw_pairs(4 * len(kept) + 1, warp_seed=c)['p']
        g_min, b = decidedness(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
        if g_min > b:
            kept.append(c)
        else:
            rejected += 1
        c += 1
    return tuple(kept), rejected


# ------------------------------------------------------------------------------------------------------------------------
# what the draws promise
# ------------------------------------------------------------------------------------------------------------------------
def _seeds():
    return range(max(N_SEEDS, DEFAULT_SEEDS))


def test_draw_s7_reaches_every_value_it_lists():
    lib, E = _lib_and_engine()
    UG, cap = lib.tmf_wmrb_scores7_users_per_group(), lib.tmf_wmrb_scores7_slots()
    seen = dict(r=set(), slots=set(), slice_bytes=set(), fill=set(), m=set())
    groups_and_slices = over_slots = repeated_pair = 0
    for seed in _seeds():
        m, n, r, S, idx, val, R, U, V, dtype, env = draw_s7(seed)
        assert dtype is torch.float32 and n <= 32 * S and 1 <= S <= n and U.shape == (m, r) and V.shape == (n, r) and R.shape == (m, S)
        assert (env['TMF_FORCE_SLICED'], env['TMF_SCORES5'], env['TMF_SCORES6'], env['TMF_SCORES7']) == ('1', '0', '0', '1')
        assert set(env) <= set(FORM_KEYS) and len(np.unique(idx[:, 0] * n + idx[:, 1])) == len(val) and (val > 0).any()
        slice_bytes, slots, _ = _s7_args(env)
        seen['r'].add(r), seen['slots'].add(slots), seen['slice_bytes'].add(slice_bytes), seen['fill'].add(env['TMF_S7_FILL']), seen['m'].add(m)
        # the geometry Scores7Plan derives from these (asserted against the plan itself in the invariants test below)
        ns = max(1, -(-n * 512 // slice_bytes)) if slice_bytes else 1
        width = -(-n // ns)
        ns, ng = -(-n // width), -(-m // UG)
        groups_and_slices += ng > 1 and ns > 1
        per_chunk = np.zeros((m, ns), np.int64)                  # entries of every (user, slice): a chunk holds those of its group's users
        np.add.at(per_chunk, (idx[:, 0], idx[:, 1] // width), 1)
        np.add.at(per_chunk, (np.repeat(np.arange(m), S), R.reshape(-1) // width), 1)
        over_slots += per_chunk.max() > (slots or cap)
        stored = set((idx[:, 0] * n + idx[:, 1]).tolist())
        repeated_pair += any(int(a) * n + int(R[a, 0]) in stored for a in range(m)) and seed % 3 == 1
    assert seen['r'] == set(S7_R) and seen['slots'] == set(S7_SLOTS) and seen['slice_bytes'] == set(S7_SLICE_BYTES), seen
    assert seen['fill'] == {'0', '1'} and set(S7_BORDER_M) <= seen['m'], seen
    assert any(x % UG and x > UG for x in seen['m']) and any(x < UG for x in seen['m'])
    assert groups_and_slices >= 1 and over_slots >= 1 and repeated_pair >= 1, (groups_and_slices, over_slots, repeated_pair)


def test_draw_pairs_reaches_every_kind_on_every_scores_form():
    lib, _ = _lib_and_engine()
    UG = lib.tmf_wmrb_scores7_users_per_group()
    on_s7, forms, rs, rs_s7, permuted, groups_and_slices = {k: 0 for k in PAIR_KINDS}, set(), set(), set(), set(), 0
    assert all(lib.tmf_wmrb_scores7_supported(r, 0, 700) == (r in PAIR_R_S7) for r in PAIR_R)
    for seed in _seeds():
        d = draw_pairs(seed)
        p = d['p']
        assert d['kind'] == PAIR_KINDS[seed % 4] and set(d['env']) <= set(FORM_KEYS)
        assert 3 <= p['m'] <= 600 and 40 <= p['n'] <= 700 and 1 <= p['S'] <= 48 and p['r'] in PAIR_R
        assert len(p['val']) <= 1.15 * MAX_STORED and (np.diff(p['idx'][:, 0] * p['n'] + p['idx'][:, 1]) > 0).all()
        assert d['c'] == (p['n'] / p['S'] if d['kind'] == 'softmax_scaled' else 1.0)
        if d['form'] == 's7':
            assert lib.tmf_wmrb_scores7_supported(p['r'], 0, p['n']) == 1
            on_s7[d['kind']] += 1
            rs_s7.add(p['r'])
            slice_bytes = int(d['env'].get('TMF_S7_SLICE_BYTES', 0))
            width = -(-p['n'] // -(-p['n'] * 512 // slice_bytes)) if slice_bytes else p['n']
            groups_and_slices += p['m'] > UG and width < p['n']          # several user groups and several scores7 slices at once
        forms.add(d['form']), rs.add(p['r']), permuted.add((d['kind'], d['permute']))
        assert sorted(d['order'].tolist()) == list(range(len(p['val']))) and d['permute'] == (d['order'].tolist() != list(range(len(p['val']))))
    assert min(on_s7.values()) >= 2 and forms == {'s3', 's6', 's7'}, (on_s7, forms)
    for t in range(6):                                           # the dyadic test's default cases: every kind on scores7 among them
        d = draw_pairs(dyadic_pair_seed(t))
        assert d['kind'] == PAIR_KINDS[t % 4] and (d['form'] == 's7' or t >= 4), (t, d['form'])
    assert permuted == {(k, f) for k in PAIR_KINDS for f in (False, True)}, permuted
    assert rs == set(PAIR_R) and rs_s7 >= set(PAIR_R_S7) and groups_and_slices >= 1, (rs, rs_s7, groups_and_slices)


# ------------------------------------------------------------------------------------------------------------------------
# the plans of the draw_s7 problems
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(N_SEEDS))
def test_scores7_plan_of_every_draw(seed):
    """Scores7Plan on CPU tensors, through the brute force of tests/test_scores7_cpu.py; after order_by_fill through that of
    tests/test_scores7_fill_cpu.py."""
    from test_scores7_cpu import check_streams
    from test_scores7_fill_cpu import _check_fill
    lib, E = _lib_and_engine()
    m, n, r, S, idx, val, R, U, V, dtype, env = draw_s7(seed)
    slice_bytes, slots, item_slices = _s7_args(env)
    problem = (torch.tensor(idx), torch.tensor(val), torch.tensor(R))
    s7 = check_streams(E, lib, m, n, S, problem, r=r, slice_bytes=slice_bytes, slots=slots, item_slices=item_slices)
    assert s7.n_groups == -(-m // 256) and s7.width == -(-n // max(1, -(-n * 512 // slice_bytes) if slice_bytes else 1))
    _check_fill(E, lib, m, n, S, None, None, slots=slots, problem=problem, r=r, slice_bytes=slice_bytes, item_slices=item_slices)


@pytest.mark.parametrize('value,slots', [('0', 1), ('-5', 1), ('1', 1), ('6144', 6144), ('6145', 6144), ('1000000', 6144)])
def test_scores7_slots_are_clamped_to_what_the_kernel_holds(monkeypatch, value, slots):
    """include/tmf.h: a sub-chunk fills at most tmf_wmrb_scores7_slots() slots of the LDS buffer - the pad slot sits right behind
    them - and holds at least one entry."""
    lib, E = _lib_and_engine()
    assert lib.tmf_wmrb_scores7_slots() == 6144
    m, n, r, S, idx, val, R, U, V, dtype, env = draw_s7(1)
    plan = E.InteractionPlan(torch.tensor(idx), torch.tensor(val), m, n)
    wplan = E.WmrbPlan(plan, torch.tensor(R), item_slices=2, n_components=r, sliced=True)
    monkeypatch.setenv('TMF_S7_SLOTS', value)
    s7 = E.Scores7Plan(plan, wplan, r, torch.float32)
    assert s7.slots == slots and int(torch.diff(s7.sub_place).max()) <= slots


@pytest.mark.parametrize('value', ['0', '-512', '1', '511'])
def test_scores7_slices_hold_at_least_one_row(monkeypatch, value):
    """A slice is a range of whole rows of V: a slice size below one row (zero and negative sizes included) gives slices of one row."""
    lib, E = _lib_and_engine()
    m, n, r, S, idx, val, R, U, V, dtype, env = draw_s7(1)
    plan = E.InteractionPlan(torch.tensor(idx), torch.tensor(val), m, n)
    wplan = E.WmrbPlan(plan, torch.tensor(R), item_slices=2, n_components=r, sliced=True)
    monkeypatch.setenv('TMF_S7_SLICE_BYTES', value)
    s7 = E.Scores7Plan(plan, wplan, r, torch.float32)
    assert s7.width == 1 and s7.n_slices == n and s7.chunk_sub.numel() == n * s7.n_groups + 1


# ------------------------------------------------------------------------------------------------------------------------
# WARP: every problem is decided
# ------------------------------------------------------------------------------------------------------------------------
def test_the_warp_seeds_are_the_walk():
    kept, rejected = walk_warp_seeds(len(WARP_SEEDS))
    print(f'[warp seeds] {kept}: {rejected} of {len(kept) + rejected} candidates rejected')
    assert kept == WARP_SEEDS and len(WARP_SEEDS) % 3 == 0 and 4 * len(WARP_SEEDS) >= 100
    assert 3 * rejected <= len(kept) + rejected


@pytest.mark.parametrize('seed', [s for s in range(N_SEEDS) if s % 4 == 1])
def test_every_warp_draw_is_decided(seed):
    p = draw_pairs(seed)['p']
    g_min, b = decidedness(p['U0'], p['V0'], p['idx'], p['val'], p['R'])
    print(f"[decided] seed {seed}: {p['m']} x {p['n']} x {p['r']}, S = {p['S']}: smallest gap {g_min:.3g}, fp32 reach {b:.3g}")
    assert g_min > b


# ------------------------------------------------------------------------------------------------------------------------
# the tolerances of tests/test_gpu_fuzz_pairs.py are reachable in fp32
# ------------------------------------------------------------------------------------------------------------------------
def fp32_restatement(d):
    """(loss sum, delta, D, gU, gV, first violators or None) from fp32 scores of the fp32 tables through the pair kernel's
    arithmetic in its order of additions; the gradients summed in fp64 from those fp32 weights."""
    p, kind = d['p'], d['kind']
    m, n, r = p['m'], p['n'], p['r']
    u, i, R = p['idx'][:, 0], p['idx'][:, 1], p['R'].astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=m))])
    pk = np.einsum('kr,kr->k', p['U0'][u], p['V0'][i]).astype(np.float32)             # fp32 scores of fp32 tables
    sp = np.einsum('ur,usr->us', p['U0'], p['V0'][R]).astype(np.float32)
    first = None
    if kind == 'bpr':
        delta, D, lp = bpr_pairs_fp32_kernel_order(rowptr, p['val'], pk, sp)
    elif kind == 'warp':
        delta, D, lp, first = warp_pairs_fp32_kernel_order(rowptr, p['val'], pk, sp, n)
    else:
        delta, D, lp = softmax_pairs_fp32_kernel_order(rowptr, p['val'], pk, sp, d['c'])
    assert all(x.dtype == np.float32 and np.isfinite(x).all() for x in (delta, D, lp))
    delta, D, lp = (x.astype(np.float64) for x in (delta, D, lp))
    gU = np.einsum('us,usr->ur', D, p['V0'][R].astype(np.float64))
    np.add.at(gU, u, delta[:, None] * p['V0'][i])
    gV = np.zeros((n, r))
    np.add.at(gV, R.reshape(-1), (D[:, :, None] * p['U0'][:, None, :]).reshape(m * p['S'], -1))
    np.add.at(gV, i, delta[:, None] * p['U0'][u])
    return lp.sum(), delta, D, gU, gV, rowptr


@pytest.mark.parametrize('seed', range(N_SEEDS))
def test_fp32_in_the_kernels_order_meets_the_gpu_tolerances_on_every_draw(seed):
    d = draw_pairs(seed)
    p = d['p']
    loss, delta, D, gU, gV = closed_form(d)
    l32, d32, D32, aU, aV, rowptr = fp32_restatement(d)
    errs = dict(loss=rel_err(l32, loss), delta=rel_err(d32, delta), D=rel_err(D32, D), gU=rel_err(aU, gU), gV=rel_err(aV, gV))
    print(f"[fp32, kernel order] seed {seed} {d['kind']} {p['m']} x {p['n']} x {p['r']} S={p['S']} c={d['c']:.3g}: "
          + ' '.join(f'{k} {v:.3g}' for k, v in errs.items()))
    assert max(errs.values()) < 1e-5, errs
    if d['kind'] == 'warp':
        assert np.array_equal(D32 != 0, D != 0) and np.array_equal(d32 != 0, delta != 0)
    if d['kind'].startswith('softmax'):
        assert all(gap <= 1e-5 * size for gap, size in sum_identity_gaps(rowptr, p['val'], d32, D32))
    assert_step(fresh_adam_fp32(p['U0'], aU, LR), p['U0'], gU, LR, rtol=1e-5, what=f'seed {seed} U')
    assert_step(fresh_adam_fp32(p['V0'], aV, LR), p['V0'], gV, LR, rtol=1e-5, what=f'seed {seed} V')


# ------------------------------------------------------------------------------------------------------------------------
# the draws of tests/test_gpu_fuzz_bias.py: the five table losses from a non-zero scalar item bias
# ------------------------------------------------------------------------------------------------------------------------
BIAS_KINDS = ('wmrb', 'bpr', 'warp', 'warp_kos', 'softmax')          # the names of the table losses in _engine.LOSSES
BIAS_CLASSES = dict(wmrb='WMRBLoss', bpr='BPRLoss', warp='WARPLoss', warp_kos='KOSWARPLoss', softmax='SampledSoftmaxLoss')
BIAS_KINKED = ('wmrb', 'warp', 'warp_kos')                            # a hinge, a first violator, an order statistic: decided problems only
BIAS_DEFAULT_SEEDS = 25
N_BIAS_SEEDS = int(os.environ.get('TMF_FUZZ_SEEDS', str(BIAS_DEFAULT_SEEDS)))
BIAS_CANDIDATES = 1000                                                # the problem seeds of draw ``seed``: 1000 seed, 1000 seed + 1, ...
UNROLL_BORDER = 192                                                   # k_item_bias_partial enters its unrolled loop above 3 * 64 entries of a chunk
# The largest rel_err of loss, gU, gV, gb of the reference's own computation run in float32 against its float64 run, over the 25
# default draws, for the two kinds without a kernel-order restatement (test_fp32_meets_the_bias_tolerances_on_every_draw prints
# every figure and holds them to these): measured 2.42095e-5 and 1.07509e-6, written here rounded UP in the fourth digit.  WMRB's weight c / (1 + c M) moves by up to c^2 times the rounding of a score, and the
# draws reach c = n / S = 191 (seed 15: 574 items, 3 samples): no fp32 evaluation of the scores gets its gradients to 1e-5.
BIAS_FP32_REF_ERR = dict(wmrb=2.421e-5, warp_kos=1.076e-6)
# rel_err of loss, gU, gV and gb against tests/item_bias_ref.py that the GPU file asks of every kind: 1e-5 where fp32 arithmetic
# reaches it on every default draw, else four times the largest fp32-reference error above (WMRB: 4 x 2.421e-5 = 9.684e-5)
BIAS_RTOL = dict(wmrb=4 * BIAS_FP32_REF_ERR['wmrb'], bpr=1e-5, warp=1e-5, warp_kos=1e-5, softmax=1e-5)
_BIAS_DRAWS, _BIAS_REFS = {}, {}


def _bias_problem(i, problem_seed, r):
    """_pair_problem's size ranges through bpr_problem, and b0 ~ 0.3 N(0, 1).  A long-list round (i even): 400 .. 600 users, S >= 4,
    and one item that is not empty_item in the columns 1 .. min(S - 1, 1 + i % 4) of every row of R (column 0 keeps the user's own
    positive): its list row holds every user of a block once, or three times."""
    rng = np.random.default_rng(91000 + problem_seed)
    m, n, S = int(rng.integers(3, 601)), int(rng.integers(40, 701)), int(rng.integers(1, 49))
    long_lists = i % 2 == 0
    if long_lists:
        m, S = int(rng.integers(400, 601)), max(S, 4)
    p = bpr_problem(problem_seed, m, n, r, S, density=min(0.3, MAX_STORED / (m * n)))
    p['long_item'] = None
    if long_lists:
        p['long_item'] = (p['empty_item'] + 1 + int(rng.integers(0, n - 1))) % n
        p['R'][:, 1:min(S - 1, 1 + i % 4) + 1] = p['long_item']
    b0 = (0.3 * rng.standard_normal(n)).astype(np.float32)
    assert b0[p['empty_item']] != 0 and p['long_item'] != p['empty_item']
    return p, b0


def bias_loss(kind):
    """The loss object of a kind, with the defaults of its class (KOSWARPLoss: k = 5 of n = 10; SampledSoftmaxLoss: c = 1)."""
    from teamoflow_amd.mf import loss_graphs
    return getattr(loss_graphs, BIAS_CLASSES[kind])()


def draw_bias(seed):
    """kind k = seed % 5 of BIAS_KINDS; round i = seed // 5.

    Width and scores form: a walk, not a draw, so that 25 seeds hold every kind on every form.
      - Every third round is a scores7 round, r = PAIR_R_S7[(i + k) % 2].
      - The other rounds, counted j = 0, 1, 2 ..: r = PAIR_R[(k + 2 j + 6) % 7].  Three of them give every kind one width at which
        scores6 exists and two at which only scores3 does; 25 seeds hold every width.
      - Their form is scores6 where it exists, else scores3 (in a soak, every second run of three such rounds takes scores3).
    The other passes: as draw_s7 draws them; the COO order is permuted every second draw.

    Long lists: even rounds are long-list rounds (_bias_problem).
      - i % 4 == 0: one column and TMF_USER_CHUNKS = 1.  The item's list row holds every user once: past the unrolled loop's border.
      - i % 4 == 2: three columns.  Every second kind gets TMF_USER_CHUNKS = 1: a list row of 1200 entries or more, further chunks
        at ITEM_BIAS_CHUNK.  The other kinds keep their drawn blocks: several list rows past the border.

    Decided problems: a kinked kind walks the problem seeds 1000 seed, 1000 seed + 1, .. and keeps the first whose biased fp64
    scores satisfy item_bias_ref.margins_decided; ``rejected`` counts the candidates it passed over.

    -> dict(kind, name, loss, c, p, b0, R, form, env, permute, order, long_lists, rejected, seed), computed once and left unchanged."""
    if seed in _BIAS_DRAWS:
        return _BIAS_DRAWS[seed]
    import types
    from item_bias_ref import margins_decided
    from teamoflow_amd import _engine as E, _lib
    lib = _lib.load_library()
    k, i = seed % 5, seed // 5
    kind = BIAS_KINDS[k]
    s7_turn = i % 3 == 0
    j = i - i // 3 - 1                                                      # the rounds that are no scores7 rounds, counted
    r = PAIR_R_S7[(i + k) % len(PAIR_R_S7)] if s7_turn else PAIR_R[(k + 2 * j + 6) % len(PAIR_R)]
    for rejected in range(BIAS_CANDIDATES):
        p, b0 = _bias_problem(i, BIAS_CANDIDATES * seed + rejected, r)
        if kind not in BIAS_KINKED:
            break
        scores = p['U0'].astype(np.float64) @ p['V0'].astype(np.float64).T + b0.astype(np.float64)[None, :]
        if margins_decided(scores, p['idx'], p['val'], p['R']):
            break
    else:
        raise AssertionError(f'no decided problem for draw_bias({seed})')
    m, n, S = p['m'], p['n'], p['S']
    rng = np.random.default_rng(92000 + seed)
    env = {'TMF_FORCE_SLICED': '1', 'TMF_SCORES5': '0'}
    _common_forms(rng, env)
    long_lists = i % 2 == 0
    if long_lists and (i % 4 == 0 or k % 2 == 0):
        env['TMF_USER_CHUNKS'] = '1'
    assert not s7_turn or lib.tmf_wmrb_scores7_supported(r, 0, n)
    plain = ['s3'] + ['s6'] * bool(lib.tmf_wmrb_scores6_supported(r, 0, n))
    form = 's7' if s7_turn else plain[(j // 3 + 1) % len(plain)]
    env['TMF_SCORES6'], env['TMF_SCORES7'] = str(int(form == 's6')), str(int(form == 's7'))
    if form == 's6' and rng.integers(0, 2):
        env['TMF_S6_SLICE_BYTES'] = str(int(rng.choice([512, 4096, 50000, 1 << 20])))
    if form == 's7':
        _s7_forms(rng, env, S7_SLICE_BYTES[int(rng.integers(0, len(S7_SLICE_BYTES)))], S7_SLOTS[int(rng.integers(0, len(S7_SLOTS)))])
    permute = bool((i + seed) % 2)
    order = rng.permutation(len(p['val'])) if permute else np.arange(len(p['val']))
    loss = bias_loss(kind)
    c = E.LOSSES[kind].param(types.SimpleNamespace(n_items=n, n_samples=S, loss_graph=loss))
    for a in (p['R'], p['U0'], p['V0'], b0, order):
        a.setflags(write=False)
    _BIAS_DRAWS[seed] = dict(kind=kind, name=kind, loss=loss, c=c, p=p, b0=b0, R=p['R'], form=form, env=env, permute=permute, order=order,
                             long_lists=long_lists, rejected=rejected, seed=seed)
    return _BIAS_DRAWS[seed]


def bias_reference(d, dtype=torch.float64):
    """item_bias_ref.biased_reference of a draw (fp64 autograd of the model's own get_loss over U V^T + b; dtype=torch.float32: the
    same computation in fp32), computed once per draw and left unchanged."""
    from item_bias_ref import biased_reference
    key = (d['seed'], dtype)
    if key not in _BIAS_REFS:
        p = d['p']
        _BIAS_REFS[key] = biased_reference(d['loss'], p['U0'], p['V0'], d['b0'], p['idx'], p['val'], p['R'], p['n'], p['S'], dtype=dtype)
    return _BIAS_REFS[key]


def bias_plan_lens(d, E):
    """(lengths of the list rows [C n], n_extra at ITEM_BIAS_CHUNK) of a draw's plan, built on CPU tensors with the draw's own user blocks."""
    p = d['p']
    C = int(d['env']['TMF_USER_CHUNKS'])
    plan = E.InteractionPlan(torch.tensor(p['idx'][d['order']]), torch.tensor(p['val'][d['order']]), p['m'], p['n'])
    wplan = E.WmrbPlan(plan, torch.tensor(p['R']), user_chunks=C, item_slices=int(d['env']['TMF_ITEM_SLICES']), n_components=p['r'], sliced=True)
    assert wplan.user_chunks == C and wplan.rowptr_e.numel() == C * p['n'] + 1
    lens = (wplan.rowptr_e[1:] - wplan.rowptr_e[:-1]).numpy()
    return lens, E.item_bias_chunks(wplan.rowptr_e, p['n'], E.ITEM_BIAS_CHUNK)[3]


def _bias_seeds():
    return range(max(N_BIAS_SEEDS, BIAS_DEFAULT_SEEDS))


def test_draw_bias_reaches_what_it_promises():
    lib, E = _lib_and_engine()
    assert set(BIAS_KINDS) == {name for name, rec in E.LOSSES.items() if rec.table}
    forms, exist, long_kinds, over_border, extra, rs, permuted = {}, {}, set(), set(), {}, set(), set()
    kept = rejected = 0
    for seed in _bias_seeds():
        d = draw_bias(seed)
        p, kind, i = d['p'], d['kind'], seed // 5
        m, n, r, S = p['m'], p['n'], p['r'], p['S']
        assert kind == d['name'] == BIAS_KINDS[seed % 5] and set(d['env']) <= set(FORM_KEYS) and type(d['loss']).__name__ == BIAS_CLASSES[kind]
        assert 3 <= m <= 600 and 40 <= n <= 700 and 1 <= S <= 48 and r in PAIR_R and d['b0'].shape == (n,) and d['b0'].dtype == np.float32
        assert len(p['val']) <= 1.15 * MAX_STORED and (np.diff(p['idx'][:, 0] * n + p['idx'][:, 1]) > 0).all()
        assert d['b0'][p['empty_item']] != 0 and not (p['R'] == p['empty_item']).any() and not (p['idx'][:, 1] == p['empty_item']).any()
        assert sorted(d['order'].tolist()) == list(range(len(p['val']))) and d['permute'] == (d['order'].tolist() != list(range(len(p['val']))))
        assert d['long_lists'] == (i % 2 == 0) and (d['form'] == 's7') == (i % 3 == 0)
        forms.setdefault(kind, set()).add(d['form'])
        exist.setdefault(kind, set()).update(['s3'] + ['s6'] * bool(lib.tmf_wmrb_scores6_supported(r, 0, n))
                                             + ['s7'] * bool(lib.tmf_wmrb_scores7_supported(r, 0, n)))
        rs.add(r), permuted.add(d['permute'])
        if kind in BIAS_KINKED:                                  # only these problems were tested for decidedness: the others count for nothing
            kept, rejected = kept + 1, rejected + d['rejected']
        assert d['rejected'] == 0 or kind in BIAS_KINKED
        lens, n_extra = bias_plan_lens(d, E)
        if d['long_lists']:
            cols = min(S - 1, 1 + i % 4)
            assert 400 <= m <= 600 and S >= 4 and (p['R'][:, 1:cols + 1] == p['long_item']).all() and p['long_item'] != p['empty_item']
            assert d['env']['TMF_USER_CHUNKS'] == '1' or (i % 4 and seed % 5 % 2)
            has = p['idx'][:, 0][p['val'] > 0]
            assert all(p['R'][u, 0] in p['idx'][(p['idx'][:, 0] == u) & (p['val'] > 0), 1] for u in np.unique(has)[:50])
            long_kinds.add(kind)
        if lens.max() > UNROLL_BORDER:
            over_border.add(kind)
        if n_extra:
            extra.setdefault(kind, []).append((seed, int(lens.max()), n_extra))
    print(f'[bias draws] forms {forms}; lists past {UNROLL_BORDER}: {sorted(over_border)}; n_extra > 0: {extra}; '
          f'{rejected} of {kept + rejected} candidates of the kinked kinds rejected')
    assert forms == exist and all(f == {'s3', 's6', 's7'} for f in forms.values()), (forms, exist)
    assert long_kinds == set(BIAS_KINDS) and over_border == set(BIAS_KINDS), (long_kinds, over_border)
    assert len(extra) >= 2, extra                                # n_extra > 0 at ITEM_BIAS_CHUNK in draws of two kinds or more
    assert rs == set(PAIR_R) and permuted == {False, True}
    assert kept == sum(BIAS_KINDS[s % 5] in BIAS_KINKED for s in _bias_seeds())
    assert 3 * rejected <= kept + rejected                       # the rule of test_the_warp_seeds_are_the_walk


@pytest.mark.parametrize('seed', [s for s in range(N_BIAS_SEEDS) if BIAS_KINDS[s % 5] in BIAS_KINKED])
def test_every_kinked_bias_draw_is_decided(seed):
    from item_bias_ref import margins_decided
    d = draw_bias(seed)
    p = d['p']
    assert margins_decided(bias_reference(d)['scores'], p['idx'], p['val'], p['R'])


def bias_errors(d, ref, loss, gU, gV, gb):
    """rel_err of the four quantities against the reference - and, in a long-list round, of gb over the items but the long one
    (gb_rest): that item's gradient, a sum of 400 .. 1800 weights, is max |gb| and would hide an error in any other item."""
    errs = dict(loss=rel_err(loss, ref['loss_sum']), gU=rel_err(gU, ref['gU']), gV=rel_err(gV, ref['gV']), gb=rel_err(gb, ref['gb']))
    if d['p']['long_item'] is not None:
        rest = np.arange(d['p']['n']) != d['p']['long_item']
        errs['gb_rest'] = rel_err(np.asarray(gb)[rest], ref['gb'][rest])
    return errs


def bias_fp32_restatement(d):
    """(loss sum, gU, gV, gb) of a bpr / warp / softmax draw from fp32 scores of the fp32 tables plus one fp32 add of b0, through the
    pair kernel's arithmetic in its order of additions; the gradients summed in fp64 from those fp32 weights."""
    p, kind = d['p'], d['kind']
    m, n, r = p['m'], p['n'], p['r']
    u, i, R = p['idx'][:, 0], p['idx'][:, 1], p['R'].astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=m))])
    pk = np.einsum('kr,kr->k', p['U0'][u], p['V0'][i]).astype(np.float32) + d['b0'][i]
    sp = np.einsum('ur,usr->us', p['U0'], p['V0'][R]).astype(np.float32) + d['b0'][R]
    assert pk.dtype == np.float32 and sp.dtype == np.float32
    if kind == 'bpr':
        delta, D, lp = bpr_pairs_fp32_kernel_order(rowptr, p['val'], pk, sp)
    elif kind == 'warp':
        delta, D, lp, _ = warp_pairs_fp32_kernel_order(rowptr, p['val'], pk, sp, n)
    else:
        delta, D, lp = softmax_pairs_fp32_kernel_order(rowptr, p['val'], pk, sp, d['c'])
    assert all(x.dtype == np.float32 and np.isfinite(x).all() for x in (delta, D, lp))
    delta, D, lp = (x.astype(np.float64) for x in (delta, D, lp))
    gU = np.einsum('us,usr->ur', D, p['V0'][R].astype(np.float64))
    np.add.at(gU, u, delta[:, None] * p['V0'][i])
    gV = np.zeros((n, r))
    np.add.at(gV, R.reshape(-1), (D[:, :, None] * p['U0'][:, None, :]).reshape(m * p['S'], -1))
    np.add.at(gV, i, delta[:, None] * p['U0'][u])
    gb = np.zeros(n)
    np.add.at(gb, R.reshape(-1), D.reshape(-1))
    np.add.at(gb, i, delta)
    return lp.sum(), gU, gV, gb


@pytest.mark.parametrize('seed', range(N_BIAS_SEEDS))
def test_fp32_meets_the_bias_tolerances_on_every_draw(seed):
    """What tests/test_gpu_fuzz_bias.py asks of the engine, BIAS_RTOL, is reachable in fp32: bpr, warp and softmax through the pair
    kernels' restatements on fp32 scores with an fp32 add of b0; wmrb and warp_kos, which have no restatement, through the
    reference's own computation in float32.  Largest fp32-reference error over the 25 default draws: warp_kos 1.07509e-6 (gU,
    seed 8) - below 1e-5, so 1e-5 -; wmrb 2.42095e-5 (gU, seed 15; gb 2.31e-5) - above it, so WMRB's tolerance is four times that
    figure rounded up to 2.421e-5: 9.684e-5.  In a long-list round gb is also held to the tolerance over the items but the long
    one (bias_errors: gb_rest)."""
    d = draw_bias(seed)
    p, kind = d['p'], d['kind']
    ref = bias_reference(d)
    if kind in ('bpr', 'warp', 'softmax'):
        loss, gU, gV, gb = bias_fp32_restatement(d)
    else:
        low = bias_reference(d, torch.float32)
        loss, gU, gV, gb = low['loss_sum'], low['gU'], low['gV'], low['gb']
    errs = bias_errors(d, ref, loss, gU, gV, gb)
    print(f"[fp32 bias] seed {seed} {kind} {p['m']} x {p['n']} x {p['r']} S={p['S']} {d['form']}: "
          + ' '.join(f'{k} {v:.6g}' for k, v in errs.items()))
    assert np.abs(ref['gb']).max() > 1e-3 and ref['gb'][p['empty_item']] == 0
    assert max(errs.values()) < BIAS_RTOL[kind], errs
    if kind in BIAS_FP32_REF_ERR and seed < BIAS_DEFAULT_SEEDS:      # the figures the tolerances were derived from still hold
        assert max(errs.values()) <= BIAS_FP32_REF_ERR[kind] and (BIAS_FP32_REF_ERR[kind] < 1e-5) == (BIAS_RTOL[kind] == 1e-5), errs
    assert_step(fresh_adam_fp32(d['b0'], gb, LR), d['b0'], ref['gb'], LR, rtol=BIAS_RTOL[kind], what=f'seed {seed} b')
