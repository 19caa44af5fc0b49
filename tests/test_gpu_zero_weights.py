"""Entries of weight 0 in the WMRB gradient gathers.  k_wmrb_gradu3 (+ finish) and k_wsum_pass / k_wsum_pass_pg (+ combine) drop the
entries whose weight is exactly 0 while they stage a list (stage_nonzero, tmf_common.h) and gather only the rows that are left:

  * hand-made weights on small plans, integer-valued tables and weights (every sum exact in fp32): the raw gradient equals a NumPy
    fp64 evaluation EXACTLY for every zero pattern - none, all, a whole staging tile of zeros before a tile of non-zeros, zeros at a
    tile's end, 4k / 4k + 1 / 1 survivors, alternating, -0.f;
  * poisoned rows: the same with every row that only zero-weight entries point at (V for gradU, U for the item pass) filled with NaN
    and Inf - bit-equal to the unpoisoned run and finite, so such a row never reaches an accumulator, not even multiplied by 0;
  * two runs of every case are bit-identical;
  * one random (non-dyadic) epoch per storage type against oracle.sparse_c.wmrb_epoch with the tolerances and the boundary slack of
    tests/test_gpu_configs.py, from tables that leave at least a fifth of the hinge terms inactive (asserted).

Forms: gradU as one launch over all slices, one launch per slice and one per round of slices; the item pass with one wave and with
one lane group per segment (TMF_WSUM_PER_GROUP), 1 and 3 user blocks; fp32 r = 128 and r = 40, bf16 r = 256; 37 and 700 users (no
multiples of 16); S = 96 in 3 slices; S = 700 in 2 slices (a visit of ~350 entries exceeds the 256-entry staging tile); one item held
by all 700 users and sampled by all of them (a list of 1,400 entries: two segments, each longer than the item pass's tile)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_close_with_slack, assert_step

pytestmark = pytest.mark.gpu

FORM_KEYS = ('TMF_ROWS4', 'TMF_ROWS5', 'TMF_SCORES5', 'TMF_SCORES6', 'TMF_ROW_STATIONARY', 'TMF_ITEM_SLICES', 'TMF_USER_CHUNKS',
             'TMF_FORCE_SLICED', 'TMF_FORCE_FUSED', 'TMF_SLICE_XCD', 'TMF_WSUM_PER_GROUP', 'TMF_WSUM_XCD_RUN', 'TMF_PART_BUDGET')

# (users, items, r, bf16, S, slices)
SHAPES = {'37x300_r40_S96x3': (37, 300, 40, False, 96, 3),
          '700x1500_r128_S700x2': (700, 1500, 128, False, 700, 2),
          '700x1500_r256bf16_S700x2': (700, 1500, 256, True, 700, 2),
          '700x300_r128_S96x3': (700, 300, 128, False, 96, 3)}
PATTERNS = ('none', 'all', 'tile_then', 'tile_end', 'keep_8', 'keep_9', 'keep_1', 'alternate', 'neg_zero')


@pytest.fixture(scope='module')
def eng():
    from teamoflow_amd import _engine, _lib
    _lib.get()
    return _engine


def lanes_per_row(r, bf16):
    lanes, G = -(-r // (8 if bf16 else 4)), 1
    while G < lanes:
        G <<= 1
    return G


def zero_mask(pattern, pos, length, tile):
    """Which positions of a list of `length` entries get weight 0 (pos: int array of positions, tile: the kernel's staging tile)."""
    if pattern in ('none',):
        return np.zeros(len(pos), bool)
    if pattern == 'all':
        return np.ones(len(pos), bool)
    if pattern == 'tile_then':      # a whole tile of zeros, then non-zeros
        return pos < tile
    if pattern == 'tile_end':       # zeros only at the end of every tile and at the end of the list
        return (pos % tile >= tile - 5) | (pos >= length - 3)
    if pattern.startswith('keep_'):  # exactly k survivors, spread over the list (k = 8: 4k, 9: 4k + 1, 1)
        k = min(int(pattern[5:]), length)
        keep = np.unique(np.linspace(0, length - 1, k).astype(np.int64)) if k > 1 else np.array([length // 2])
        return ~np.isin(pos, keep)
    return pos % 2 == 1              # alternate, neg_zero


def problem(name):
    """Interactions and negatives whose lists have a KNOWN order, so that a pattern over list positions is a set of items (gradU:
    a user's negatives are walked in ascending item order) or of users (item pass: an item's list is its positives, then the
    users that sampled it, each by ascending user).  Even users sample the item set A, odd users the set B; both hold item 0."""
    m, n, r, bf16, S, ns = SHAPES[name]
    rng = np.random.default_rng(len(name) * 1000 + m)
    others = rng.permutation(np.arange(1, n))
    A = np.sort(np.concatenate([[0], others[:S - 1]]))
    B = np.sort(np.concatenate([[0], others[S - 1:2 * (S - 1)]])) if n >= 2 * S else A
    R = np.stack([rng.permutation(A if u % 2 == 0 else B) for u in range(m)]).astype(np.int32)   # model order: any
    u = np.concatenate([np.arange(m), rng.integers(0, m, 5 * m)])           # item 0 is held by every user
    j = np.concatenate([np.zeros(m, np.int64), rng.integers(0, n, 5 * m)])
    key = np.unique(u.astype(np.int64) * n + j)
    idx = np.stack([key // n, key % n], 1)
    val = rng.integers(1, 6, len(key)).astype(np.float32)
    U = rng.integers(-3, 4, (m, r)).astype(np.float32)
    V = rng.integers(-3, 4, (n, r)).astype(np.float32)
    return dict(m=m, n=n, r=r, bf16=bf16, S=S, ns=ns, A=A, B=B, R=R, idx=idx, val=val, U=U, V=V, rng=rng)


_built = {}


def built(eng, monkeypatch, name, chunks):
    """Plan, WMRB plan and state of a shape, built once per (shape, user blocks) and shared by the tests (they only write the weights
    and their own output buffers, and restore the tables they poison)."""
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    p = problem(name)
    for k, v in (('TMF_FORCE_SLICED', '1'), ('TMF_ITEM_SLICES', str(p['ns'])), ('TMF_USER_CHUNKS', str(chunks)), ('TMF_ROWS4', '0'),
                 ('TMF_ROW_STATIONARY', '0'), ('TMF_SCORES5', '0'), ('TMF_SCORES6', '0')):
        monkeypatch.setenv(k, v)
    if (name, chunks) not in _built:
        dev = 'cuda'
        dtype = torch.bfloat16 if p['bf16'] else torch.float32
        plan = eng.InteractionPlan(torch.tensor(p['idx'], device=dev), torch.tensor(p['val'], device=dev), p['m'], p['n'])
        wplan = eng.wmrb_plan_for(plan, torch.tensor(p['R'], device=dev), p['r'], dtype)
        st = eng.TrainState(torch.tensor(p['U'], device=dev), torch.tensor(p['V'], device=dev), plan, p['r'], wplan, dtype=dtype)
        assert wplan.sliced and wplan.n_slices == p['ns'] and wplan.user_chunks == chunks and not wplan.rows4 and wplan.seg_e is not None
        p.update(plan=plan, wplan=wplan, st=st, Rs=wplan.R.cpu().numpy().astype(np.int64), col=plan.col_u.cpu().numpy().astype(np.int64),
                 user_of=plan.user_of.cpu().numpy().astype(np.int64))
        _built[(name, chunks)] = p
    return _built[(name, chunks)]


def dense_weights(p, D, delta):
    """W[u, j] = sum of the weights of user u's entries at item j (fp64): gU = W V, gV = W^T U."""
    W = np.zeros((p['m'], p['n']))
    np.add.at(W, (np.repeat(np.arange(p['m']), p['S']), p['Rs'].reshape(-1)), D.reshape(-1).astype(np.float64))
    np.add.at(W, (p['user_of'], p['col']), delta.astype(np.float64))
    return W


def set_weights(p, D, delta):
    w = p['wplan']
    w.D.copy_(torch.tensor(D, device='cuda'))
    w.delta.copy_(torch.tensor(delta, device='cuda'))


def nonzero_ints(rng, shape):
    x = rng.integers(1, 5, shape).astype(np.float32)
    return x * rng.choice(np.float32([-1, 1]), shape)


def gradu(eng, p, launches):
    """tmf_wmrb_gradu3 + tmf_wmrb_finish with the raw-gradient epilogue -> gU [m, ld] (fp32)."""
    from teamoflow_amd import _lib
    lib, st, w = _lib.get(), p['st'], p['wplan']
    layers = {0: w.n_slices, 1: 1, 3: min(8, w.n_slices)}[launches]
    part = torch.full((layers * p['m'], st.ld), 5.0, device='cuda')
    gU = torch.full((p['m'], st.ld), 7.0, device='cuda')
    s, adam = _lib.stream_ptr(), eng.adam_constants(0.1)
    _lib.check(getattr(lib, 'tmf_wmrb_gradu3' + st.sfx)(w.lists(p['plan']), _lib.ptr(w.D), _lib.ptr(w.delta), _lib.ptr(st.V), _lib.ptr(part),
                                                        launches, p['r'], s), lib)
    _lib.check(getattr(lib, 'tmf_wmrb_finish' + st.sfx)(_lib.ptr(part), ctypes.c_int32(layers), ctypes.c_int32(p['m']), _lib.ptr(st.U),
                                                        _lib.ptr(gU), p['r'], _lib.EPI_GRAD, adam, s), lib)
    torch.cuda.synchronize()
    return gU


def item_pass(eng, p):
    """tmf_wsum_pass + tmf_combine_rows with the raw-gradient epilogue -> gV [n, ld] (fp32)."""
    from teamoflow_amd import _lib
    lib, st, w = _lib.get(), p['st'], p['wplan']
    gV = torch.full((p['n'], st.ld), 7.0, device='cuda')
    st.slab.fill_(5.0)
    s, adam = _lib.stream_ptr(), eng.adam_constants(0.1)
    _lib.check(getattr(lib, 'tmf_wsum_pass' + st.sfx)(w.seg_e.cstruct(), _lib.ptr(w.ent_row), _lib.ptr(w.ent_w), _lib.ptr(w.wbuf), _lib.ptr(st.U),
                                                      _lib.ptr(st.V), _lib.ptr(gV), _lib.ptr(st.slab), p['r'], _lib.EPI_GRAD, adam, s), lib)
    eng._row_pass_finish(lib, w.seg_e, st.slab, st.V, gV, p['r'], _lib.EPI_GRAD, adam, s, st.sfx)
    torch.cuda.synchronize()
    return gV


def poison(table, rows):
    """NaN, +Inf and -Inf over the rows `rows` of a device table (all its columns); returns the rows' former contents."""
    rows_t = torch.tensor(rows, device='cuda', dtype=torch.int64)
    saved = table[rows_t].clone()
    bad = torch.tensor([float('nan'), float('inf'), float('-inf')], device='cuda').to(table.dtype)
    table[rows_t] = bad[torch.arange(table.shape[1], device='cuda') % 3][None, :].expand(len(rows), -1)
    return rows_t, saved


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('name', list(SHAPES))
def test_gradu_drops_zero_weight_entries(eng, monkeypatch, name):
    p = built(eng, monkeypatch, name, 1)
    m, n, S, ns, rng = p['m'], p['n'], p['S'], p['ns'], p['rng']
    tile = 8 * lanes_per_row(p['r'], p['bf16'])
    width = -(-n // ns)
    if S == 700:
        assert max(int((p['A'] // width == sl).sum()) for sl in range(ns)) > tile   # a visit longer than the staging tile
    for pattern in PATTERNS:
        # zero items: the pattern over the positions of A (and of B) inside every slice - the order gradU walks them in
        zero_item = np.zeros(n, bool)
        for items in (p['A'], p['B']):
            for sl in range(ns):
                part = items[items // width == sl]
                zero_item[part[zero_mask(pattern, np.arange(len(part)), len(part), tile)]] = True
        if pattern == 'all':
            zero_item[:] = True
        zero_val = np.float32(-0.0) if pattern == 'neg_zero' else np.float32(0.0)
        D = np.where(zero_item[p['Rs']], zero_val, nonzero_ints(rng, (m, S)))
        delta = np.where(zero_item[p['col']], zero_val, nonzero_ints(rng, len(p['col'])))
        set_weights(p, D, delta)
        want = dense_weights(p, D, delta) @ p['V'].astype(np.float64)
        assert np.abs(want).max() < 2 ** 24   # every partial sum is an integer fp32 holds exactly
        if pattern == 'all':
            assert not want.any()
        # rows that only zero-weight entries point at (every entry of a zero item has weight 0)
        referenced = np.zeros(n, bool)
        referenced[p['Rs'].reshape(-1)] = True
        referenced[p['col']] = True
        bad_rows = np.flatnonzero(zero_item & referenced)
        assert (pattern == 'none') == (len(bad_rows) == 0), pattern
        for launches in (0, 1, 3):
            what = (name, pattern, launches)
            g = gradu(eng, p, launches)
            assert np.array_equal(g[:, :p['r']].double().cpu().numpy(), want), what
            assert not bool(g[:, p['r']:].any()), what
            assert same_bits(g, gradu(eng, p, launches)), what          # two runs: the same bits
            if len(bad_rows):
                rows_t, saved = poison(p['st'].V, bad_rows)
                try:
                    gp = gradu(eng, p, launches)
                finally:
                    p['st'].V[rows_t] = saved
                assert bool(torch.isfinite(gp).all()) and same_bits(gp, g), what


@pytest.mark.parametrize('per_group', ['0', '1'])
@pytest.mark.parametrize('chunks', [1, 3])
@pytest.mark.parametrize('name', list(SHAPES))
def test_item_pass_drops_zero_weight_entries(eng, monkeypatch, name, chunks, per_group):
    p = built(eng, monkeypatch, name, chunks)
    monkeypatch.setenv('TMF_WSUM_PER_GROUP', per_group)
    m, n, S, rng, w = p['m'], p['n'], p['S'], p['rng'], p['wplan']
    G = lanes_per_row(p['r'], p['bf16'])
    tile = 512 // (64 // G) if per_group == '1' else 512
    rowptr = w.rowptr_e.cpu().numpy()
    longest = int(np.diff(rowptr).max())
    if m == 700 and chunks == 1:
        assert longest == 2 * m and longest > 1024 > tile      # item 0: every user holds it and samples it - two segments
        assert w.seg_e.n_long >= 1
    for pattern in PATTERNS:
        # zero users: the pattern over the users of a block in ascending order - the order every list of the block holds them in
        upc = -(-m // chunks)
        zero_user = np.zeros(m, bool)
        for b in range(chunks):
            users = np.arange(b * upc, min(m, (b + 1) * upc))
            zero_user[users[zero_mask(pattern, np.arange(len(users)), len(users), tile)]] = True
        zero_val = np.float32(-0.0) if pattern == 'neg_zero' else np.float32(0.0)
        D = np.where(zero_user[:, None], zero_val, nonzero_ints(rng, (m, S)))
        delta = np.where(zero_user[p['user_of']], zero_val, nonzero_ints(rng, len(p['col'])))
        set_weights(p, D, delta)
        want = dense_weights(p, D, delta).T @ p['U'].astype(np.float64)
        assert np.abs(want).max() < 2 ** 24
        if pattern == 'all':
            assert not want.any()
        bad_rows = np.flatnonzero(zero_user)
        what = (name, chunks, per_group, pattern)
        g = item_pass(eng, p)
        assert np.array_equal(g[:, :p['r']].double().cpu().numpy(), want), what
        assert not bool(g[:, p['r']:].any()), what
        assert same_bits(g, item_pass(eng, p)), what
        if len(bad_rows):
            rows_t, saved = poison(p['st'].U, bad_rows)
            try:
                gp = item_pass(eng, p)
            finally:
                p['st'].U[rows_t] = saved
            assert bool(torch.isfinite(gp).all()) and same_bits(gp, g), what


@pytest.mark.parametrize('bf16', [False, True])
def test_random_epoch_with_inactive_hinge_terms(eng, monkeypatch, bf16):
    """A whole epoch (scores -> hinge -> gradU + finish, item pass + combine) on random tables against the C oracle: D, delta, the
    loss and both updated tables, with the tolerances and the boundary slack of tests/test_gpu_configs.py.  The tables separate
    positives from negatives well enough that at least a fifth of the hinge terms is inactive - D and delta hold exact zeros that
    the two gather kernels drop."""
    from oracle import sparse_c as C
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (('TMF_FORCE_SLICED', '1'), ('TMF_ITEM_SLICES', '3'), ('TMF_USER_CHUNKS', '3'), ('TMF_ROWS4', '0'),
                 ('TMF_ROW_STATIONARY', '0'), ('TMF_WSUM_PER_GROUP', '1')):
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(5)
    m, n, S = 700, 600, 96
    r = 256 if bf16 else 128
    dtype = torch.bfloat16 if bf16 else torch.float32
    u, j = rng.integers(0, m, 6 * m), rng.integers(0, n, 6 * m)
    key = np.unique(u.astype(np.int64) * n + j)
    idx = np.stack([key // n, key % n], 1)
    val = rng.integers(1, 6, len(key)).astype(np.float32)
    R = np.stack([rng.choice(n, S, replace=False) for _ in range(m)]).astype(np.int32)
    # every item an even user holds leans towards that user's row: their positives score ~1.6, their negatives ~0 +- 0.3, so
    # nearly all hinge terms 1 - p_k + sp[u, s] of the even users are inactive and those of the odd users active
    U = (rng.standard_normal((m, r)) * (2.0 / np.sqrt(r))).astype(np.float32)
    V = (rng.standard_normal((n, r)) * (0.5 / np.sqrt(r))).astype(np.float32)
    for uu, jj in idx[idx[:, 0] % 2 == 0]:
        V[jj] += 0.8 * U[uu] / np.linalg.norm(U[uu])
    dev = 'cuda'
    plan = eng.InteractionPlan(torch.tensor(idx, device=dev), torch.tensor(val, device=dev), m, n)
    wplan = eng.wmrb_plan_for(plan, torch.tensor(R, device=dev), r, dtype)
    st = eng.TrainState(torch.tensor(U, device=dev), torch.tensor(V, device=dev), plan, r, wplan, dtype=dtype)
    assert wplan.sliced and wplan.n_slices == 3 and wplan.user_chunks == 3 and not wplan.rows4 and not st.row_stationary
    Us, Vs = st.U[:, :r].float().cpu().numpy(), st.V[:, :r].float().cpu().numpy()   # the tables as stored (bf16: rounded)
    lr = 0.05
    cplan = C.Plan(idx, val, m, n, R)
    _, _, mean, t = C.wmrb_epoch(Us, Vs, cplan, n, S, lr)
    sl = C.wmrb_boundary_slack(Us, Vs, cplan, n, S)
    U64, V64 = Us.astype(np.float64), Vs.astype(np.float64)
    x = 1.0 - np.einsum('kc,kc->k', U64[idx[:, 0]], V64[idx[:, 1]])[:, None] + np.einsum('uc,usc->us', U64, V64[R])[idx[:, 0]]
    inactive = float((x < 0).mean())          # share of the hinge terms (positive k, sample s) that are inactive
    zero_D, zero_delta = float((t['D'] == 0).mean()), float((t['delta'] == 0).mean())
    print(f'inactive hinge terms {inactive:.3f}; exact zeros in D {zero_D:.3f}, in delta {zero_delta:.3f}; boundary pairs {sl["pairs"]}')
    assert inactive >= 0.2 and zero_D >= 0.2, (inactive, zero_D, zero_delta)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    eng.epoch_wmrb(st, eng.adam_constants(lr), n / S, loss)
    torch.cuda.synchronize()
    n_pos = int((val > 0).sum())
    assert abs(float(loss) / n_pos - mean) <= 1e-5 * abs(mean)
    got_D = wplan.D_in_model_order().cpu().numpy()
    assert float((got_D == 0).mean()) >= 0.2
    assert_close_with_slack(got_D, t['D'], sl['D'], what='D')
    assert_close_with_slack(wplan.delta.cpu().numpy(), t['delta'], sl['delta'], what='delta')
    if not bf16:   # the updated tables inside the step interval (bf16 tables round the step: the gradients above are the check)
        assert_step(st.U_nxt[:, :r].cpu().numpy(), Us, t['gU'], lr, what='U', slack=sl['gU'])
        assert_step(st.V_nxt[:, :r].cpu().numpy(), Vs, t['gV'], lr, what='V', slack=sl['gV'])
    else:
        gU = torch.full((m, st.ld), 7.0, device=dev)
        gV = torch.full((n, st.ld), 7.0, device=dev)
        from teamoflow_amd import _lib
        eng.epoch_wmrb(st, eng.adam_constants(lr), n / S, loss.zero_(), item_epi=_lib.EPI_GRAD, item_out=gV, user_epi=_lib.EPI_GRAD,
                       user_out=gU)
        torch.cuda.synchronize()
        assert_close_with_slack(gU[:, :r].cpu().numpy(), t['gU'], sl['gU'], what='gU')
        assert_close_with_slack(gV[:, :r].cpu().numpy(), t['gV'], sl['gV'], what='gV')
