"""The scalar item bias on the GPU (scalar_item_bias / item_bias_): tmf_item_bias_add and tmf_item_bias_grad alone, one engine epoch
of every table loss from a non-zero bias in every form of the passes, fits through the public API, and every ranking call on the
augmented tables.  The fp64 reference is tests/item_bias_ref.py: autograd of the model's own get_loss over U V^T + b."""
import types

import numpy as np
import pytest
import torch

from conftest import assert_step, rel_err
from item_bias_ref import biased_reference, margins_decided, ulp32
from test_bpr_cpu import bpr_problem

pytestmark = pytest.mark.gpu
LR = 0.05
NAN = float('nan')
SHAPES = ((40, 23, 16, 8), (33, 50, 128, 37))   # m, n, r, S
KINKED = ('wmrb', 'warp', 'warp_kos')             # losses with a hinge, a first violator or an order statistic: decided problems only


@pytest.fixture(scope='module')
def tm():
    from teamoflow_amd import _engine, _lib, _ops
    from teamoflow_amd.mf import embedding_graphs as EG, loss_graphs as LG
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseFeatures, SparseInteractions, eye, hstack_identity
    ns = types.SimpleNamespace(lib=_lib.get(), L=_lib, E=_engine, ops=_ops, EG=EG, LG=LG, MF=MatrixFactorization, Fixed=FixedInitializer,
                               Sparse=SparseInteractions, SF=SparseFeatures, eye=eye, hstack=hstack_identity)
    ns.losses = {'wmrb': LG.WMRBLoss, 'bpr': LG.BPRLoss, 'warp': LG.WARPLoss, 'warp_kos': LG.KOSWARPLoss, 'softmax': LG.SampledSoftmaxLoss}
    assert set(ns.losses) == {name for name, rec in _engine.LOSSES.items() if rec.table}
    return ns


@pytest.fixture
def engine_only(tm, monkeypatch):
    """_fit_generic refuses to run: a fit that passes ran on the engine."""
    def refuse(self, *a, **k):
        raise AssertionError('_fit_generic was called')
    monkeypatch.setattr(tm.MF, '_fit_generic', refuse)


def host(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def dev(x, dtype):
    return torch.as_tensor(np.asarray(x), dtype=dtype).cuda().contiguous()


# ------------------------------------------------------------------------------------------------------------------------
# tmf_item_bias_add alone: one add per score, so bit-exact against torch
# ------------------------------------------------------------------------------------------------------------------------
def run_add(tm, b, R, sp, col, pk, pad=4):
    """The kernel on sp / pk that sit inside larger buffers of poisoned guard words (``pad`` floats before, 4 behind)."""
    m, S = R.shape
    guard = -7.25e33
    bufs = []
    for x in (sp.reshape(-1), pk):
        buf = torch.full((pad + x.numel() + 4,), guard, device='cuda')
        buf[pad:pad + x.numel()] = x
        bufs.append(buf)
    d_sp, d_pk = bufs[0][pad:pad + m * S], bufs[1][pad:pad + pk.numel()]
    tm.L.check(tm.lib.tmf_item_bias_add(b, b.numel(), R, m, S, d_sp if m * S else None, col if pk.numel() else None, pk.numel(),
                                        d_pk if pk.numel() else None, tm.L.stream_ptr()), tm.lib)
    torch.cuda.synchronize()
    for buf, x in zip(bufs, (sp.reshape(-1), pk)):
        assert bool((buf[:pad] == guard).all()) and bool((buf[pad + x.numel():] == guard).all())
    return d_sp.view(m, S).clone(), d_pk.clone()


def same_scores(got, want):
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(bits(got)[~nan], bits(want)[~nan])


@pytest.mark.parametrize('pad', [4, 1], ids=['aligned', 'unaligned'])
@pytest.mark.parametrize('m,S,n', [(3, 5, 7), (17, 37, 9), (5, 1024, 2000), (2, 4, 1)])
def test_add_is_one_add_per_score(tm, m, S, n, pad):
    g = torch.Generator().manual_seed(m * S + n)
    b = torch.randn(n, generator=g).cuda()
    R = torch.randint(0, n, (m, S), generator=g, dtype=torch.int32).cuda()
    sp = torch.randn(m, S, generator=g).cuda()
    deg = torch.randint(0, 4, (m,), generator=g)
    deg[0] = 0                                             # a user without positives
    nnz = int(deg.sum())
    col = torch.randint(0, n, (nnz,), generator=g, dtype=torch.int32).cuda()
    pk = torch.randn(nnz, generator=g).cuda()
    got_sp, got_pk = run_add(tm, b, R, sp, col, pk, pad)
    assert torch.equal(bits(got_sp), bits(sp + b[R.long()])) and torch.equal(bits(got_pk), bits(pk + b[col.long()]))
    # +-inf and NaN in one slot reach the scores of that item and no other
    for bad in (float('inf'), -float('inf'), NAN):
        b2 = b.clone()
        b2[n // 2] = bad
        got_sp, got_pk = run_add(tm, b2, R, sp, col, pk, pad)
        assert same_scores(got_sp, sp + b2[R.long()]) and same_scores(got_pk, pk + b2[col.long()])
        assert torch.equal(~torch.isfinite(got_sp), R == n // 2) and torch.equal(~torch.isfinite(got_pk), col == n // 2)


IB_ADD_BLOCKS, IB_THREADS = 16384, 256   # kIbAddBlocks and kIbThreads of csrc/tmf_itembias.hip: one pass of the add's grid-stride loops


@pytest.mark.parametrize('pad', [4, 1], ids=['aligned', 'unaligned'])
def test_add_past_one_pass_of_the_grid(tm, pad):
    """4100 x 4100 scores and 16384 * 256 + 300 interactions: every grid-stride loop of the kernel takes a second trip (the float4
    pieces and the interactions one pass and a bit, the scalar form of the unaligned table more than four)."""
    m = S = 4100
    n, nnz, one_pass = 1000, IB_ADD_BLOCKS * IB_THREADS + 300, IB_ADD_BLOCKS * IB_THREADS
    assert m * S // 4 > one_pass and m * S > 4 * one_pass and nnz > one_pass
    g = torch.Generator(device='cuda').manual_seed(4100 + pad)
    b = torch.randn(n, generator=g, device='cuda')
    R = torch.randint(0, n, (m, S), generator=g, dtype=torch.int32, device='cuda')
    sp = torch.randn(m, S, generator=g, device='cuda')
    col = torch.randint(0, n, (nnz,), generator=g, dtype=torch.int32, device='cuda')
    pk = torch.randn(nnz, generator=g, device='cuda')
    want_sp, want_pk = sp + b[R.long()], pk + b[col.long()]
    got_sp, got_pk = run_add(tm, b, R, sp, col, pk, pad)
    assert torch.equal(bits(got_sp), bits(want_sp)) and torch.equal(bits(got_pk), bits(want_pk))


def test_add_on_tables_without_users_samples_or_entries(tm):
    b = torch.randn(5).cuda()
    empty_i, empty_f = torch.zeros(0, dtype=torch.int32).cuda(), torch.zeros(0).cuda()
    R, sp = torch.randint(0, 5, (3, 4), dtype=torch.int32).cuda(), torch.randn(3, 4).cuda()
    got_sp, got_pk = run_add(tm, b, R, sp, empty_i, empty_f)                      # nnz = 0
    assert torch.equal(got_sp, sp + b[R.long()]) and got_pk.numel() == 0
    col, pk = torch.randint(0, 5, (6,), dtype=torch.int32).cuda(), torch.randn(6).cuda()
    for m, S in ((0, 4), (3, 0)):                                                 # m = 0, S = 0
        got_sp, got_pk = run_add(tm, b, torch.zeros(m, S, dtype=torch.int32).cuda(), torch.zeros(m, S).cuda(), col, pk)
        assert torch.equal(got_pk, pk + b[col.long()])
    s = tm.L.stream_ptr()
    assert tm.lib.tmf_item_bias_add(None, 0, None, 0, 0, None, None, 0, None, s) == 0          # nothing at all: TMF_OK
    assert tm.lib.tmf_item_bias_add(None, 5, R, 3, 4, sp, None, 0, None, s) < 0                # a null bias table
    assert tm.lib.tmf_item_bias_add(b, 5, None, 3, 4, sp, None, 0, None, s) < 0
    assert tm.lib.tmf_item_bias_add(b, 5, R, 3, 4, sp, None, 6, pk, s) < 0
    assert tm.lib.tmf_item_bias_add(b, 5, R, -1, 4, sp, None, 0, None, s) < 0


# ------------------------------------------------------------------------------------------------------------------------
# tmf_item_bias_grad alone
# ------------------------------------------------------------------------------------------------------------------------
def run_grad(tm, rowptr, n, C, ent_w, wbuf, chunk, epi, b_old=None, lr=LR, stream=None):
    """-> b_out [n] (NaN-prefilled), with the workspace between poisoned guard words that must stay."""
    xrow, xchunk, xptr, n_extra = tm.E.item_bias_chunks(rowptr, n, chunk)
    words = tm.lib.tmf_item_bias_grad_workspace_bytes(n, C, n_extra) // 8
    assert words == n * C + n_extra
    guard = -3.5e300
    buf = torch.full((16 + words + 16,), guard, dtype=torch.float64, device='cuda')
    ws = buf[16:16 + words]
    out = torch.full((n,), NAN, device='cuda')
    adam = tm.E.adam_constants(lr)

    def call():
        tm.L.check(tm.lib.tmf_item_bias_grad(rowptr, n, C, ent_w, wbuf, chunk, xrow, xchunk, xptr, n_extra, b_old, out, epi, adam,
                                             ws, words * 8, tm.L.stream_ptr()), tm.lib)
    if stream is None:
        call()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            call()
        torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    assert bool((buf[:16] == guard).all()) and bool((buf[16 + words:] == guard).all())
    return out, n_extra


def hand_lists(C, chunk=4, n=7):
    """Lists of 7 items in C user blocks: item 0 without entries, item 1 with a list row of 3 chunks + 1 entry, item 2 with large
    weights of both signs that cancel to near zero, the others a few entries; behind the last list row a row of entries whose
    weights are NaN (the stored values <= 0 of a plan: never read)."""
    rng = np.random.default_rng(100 + C)
    lens = rng.integers(1, 7, (C, n))
    lens[:, 0] = 0
    lens[0, 1] = 3 * chunk + 1
    lens[:, 2] = 0
    lens[C - 1, 2] = 6
    lens = lens.reshape(-1)
    E_lists, tail = int(lens.sum()), 5
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    E = E_lists + tail
    ent_w = rng.permutation(E).astype(np.int32)            # entry id of every list entry, the NaN row's behind the lists
    wbuf = rng.standard_normal(E).astype(np.float32)
    wbuf[ent_w[E_lists:]] = np.nan
    row2 = (C - 1) * n + 2
    wbuf[ent_w[rowptr[row2]:rowptr[row2 + 1]]] = np.array([3.0e6, -3.0e6, 1.5e-3, 7.25e5, -7.25e5, -1.0e-3], np.float32)
    item = np.tile(np.arange(n), C)
    G, A = np.zeros(n), np.zeros(n)
    for row in range(C * n):
        w = wbuf[ent_w[rowptr[row]:rowptr[row + 1]]].astype(np.float64)
        G[item[row]] += w.sum()
        A[item[row]] += np.abs(w).sum()
    return rowptr, ent_w, wbuf, G, A


@pytest.mark.parametrize('C', [1, 3])
def test_grad_on_hand_built_lists(tm, C):
    n, chunk = 7, 4
    rowptr, ent_w, wbuf, G, A = hand_lists(C, chunk, n)
    d_rowptr, d_ent, d_w = dev(rowptr, torch.int64), dev(ent_w, torch.int32), dev(wbuf, torch.float32)
    g, n_extra = run_grad(tm, d_rowptr, n, C, d_ent, d_w, chunk, tm.L.EPI_GRAD)
    assert n_extra >= 3
    got = host(g).astype(np.float64)
    assert np.isfinite(got).all() and got[0] == 0.0 and abs(G[2]) < 1.0
    assert (np.abs(got - G) <= ulp32(G) + 1e-12 * A).all(), (got, G)
    for other in (run_grad(tm, d_rowptr, n, C, d_ent, d_w, chunk, tm.L.EPI_GRAD)[0],                               # twice
                  run_grad(tm, d_rowptr, n, C, d_ent, d_w, chunk, tm.L.EPI_GRAD, stream=torch.cuda.Stream())[0]):  # a stream of its own
        assert torch.equal(bits(other), bits(g))
    # another chunk length is another (fixed) order of the same sums: within the same bound
    g16, none = run_grad(tm, d_rowptr, n, C, d_ent, d_w, 16, tm.L.EPI_GRAD)
    assert none == 0 and (np.abs(host(g16).astype(np.float64) - G) <= ulp32(G) + 1e-12 * A).all()
    # TMF_EPI_ADAM = tmf_adam_fresh_rows_f32 on the TMF_EPI_GRAD output, bit for bit; an item without entries keeps its bias
    b_old = torch.randn(n, generator=torch.Generator().manual_seed(C)).cuda()
    stepped, _ = run_grad(tm, d_rowptr, n, C, d_ent, d_w, chunk, tm.L.EPI_ADAM, b_old=b_old)
    W, Gp = torch.zeros(8, device='cuda'), torch.zeros(8, device='cuda')
    W[:n], Gp[:n] = b_old, g
    tm.L.check(tm.lib.tmf_adam_fresh_rows_f32(W, Gp, 2, 4, tm.E.adam_constants(LR), tm.L.stream_ptr()), tm.lib)
    torch.cuda.synchronize()
    assert torch.equal(bits(stepped), bits(W[:n])) and torch.equal(bits(stepped[:1]), bits(b_old[:1]))
    assert not torch.equal(stepped[1:], b_old[1:])


# list-row lengths around every border of k_item_bias_partial: the lanes of a wave (64), the first trip of the unrolled loop (a chunk
# of more than 3 * 64 = 192 entries) and its later trips (256, 448), the chunk lengths 256 and 1024 and their multiples
LENS = (0, 1, 63, 64, 65, 192, 193, 255, 256, 257, 448, 449, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 200)
CANCELLING = np.array([3.0e6, -3.0e6, 1.5e-3, 7.25e5, -7.25e5, -1.0e-3], np.float32)   # hand_lists' item 2


def border_lists(C):
    """One item per length of LENS; block c gives item i the length LENS[(i + c) % len(LENS)].  ent_w a permutation, weights N(0, 1)
    but for item 10 (448 entries in block 0: two trips of the unrolled loop and a tail), whose entries repeat CANCELLING and
    end in terms of 1e-3; the row behind the lists NaN.  -> rowptr, ent_w, wbuf, lens [C, n], G, A (fp64 sums per item)."""
    n = len(LENS)
    rng = np.random.default_rng(700 + C)
    lens = np.array([[LENS[(i + c) % n] for i in range(n)] for c in range(C)], np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens.reshape(-1))]).astype(np.int64)
    E_lists, tail = int(rowptr[-1]), 5
    E = E_lists + tail
    ent_w = rng.permutation(E).astype(np.int32)
    wbuf = rng.standard_normal(E).astype(np.float32)
    wbuf[ent_w[E_lists:]] = np.nan
    for c in range(C):
        row = c * n + 10
        k = int(lens[c, 10])
        w = np.tile(CANCELLING, k // 6 + 1)[:k]
        w[k - k % 6:] = (1e-3 * rng.standard_normal(k % 6)).astype(np.float32)
        wbuf[ent_w[rowptr[row]:rowptr[row + 1]]] = w
    G, A = np.zeros(n), np.zeros(n)
    for row in range(C * n):
        w = wbuf[ent_w[rowptr[row]:rowptr[row + 1]]].astype(np.float64)
        G[row % n] += w.sum()
        A[row % n] += np.abs(w).sum()
    return rowptr, ent_w, wbuf, lens, G, A


def grad_in_kernel_order(rowptr, ent_w, wbuf, n, C, chunk):
    """tmf_item_bias_grad restated in NumPy in the order its header promises: lane l of a chunk's wave adds the entries l, l + 64, ..
    in ascending order in fp64 from 0.0; the butterfly acc += acc[lane ^ off], off = 32 .. 1; an item adds chunk 0 of its blocks
    0 .. C - 1, then its further chunks in (block, chunk) order; one rounding to fp32."""
    lanes = np.arange(64)

    def chunk_sum(row, c):
        beg = rowptr[row] + c * chunk
        w = wbuf[ent_w[beg:min(beg + chunk, rowptr[row + 1])]].astype(np.float64)
        acc = np.zeros(64)
        for j in range(0, w.size, 64):
            acc[:w[j:j + 64].size] += w[j:j + 64]
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[lanes ^ off]
        return acc[0]
    out = np.zeros(n, np.float32)
    for i in range(n):
        acc = 0.0
        for blk in range(C):
            acc += chunk_sum(blk * n + i, 0)
        for blk in range(C):
            row = blk * n + i
            for c in range(1, -(-int(rowptr[row + 1] - rowptr[row]) // chunk)):
                acc += chunk_sum(row, c)
        out[i] = np.float32(acc)
    return out


@pytest.mark.parametrize('chunk', [256, 1024])
@pytest.mark.parametrize('C', [1, 3])
def test_grad_at_the_borders_of_its_loops(tm, C, chunk):
    """Every trip count of the unrolled loop and of its tail, chunks that end on and beside a border, further chunks at the length the
    engine uses.  Against the fp64 sum within the file's bound (a lost or repeated N(0, 1) entry misses it by about 1) and, bit for
    bit, against the order of additions the kernel's header states: fp64 additions in a fixed order, no fast-math."""
    n = len(LENS)
    rowptr, ent_w, wbuf, lens, G, A = border_lists(C)
    d_rowptr, d_ent, d_w = dev(rowptr, torch.int64), dev(ent_w, torch.int32), dev(wbuf, torch.float32)
    g, n_extra = run_grad(tm, d_rowptr, n, C, d_ent, d_w, chunk, tm.L.EPI_GRAD)
    assert n_extra == int(np.maximum(-(-lens // chunk) - 1, 0).sum()) and n_extra > 0
    assert int(lens.max()) > 3 * chunk and (lens > 192).any(axis=0).sum() >= n - 6      # further chunks; most items enter the unrolled loop
    got = host(g).astype(np.float64)
    assert np.isfinite(got).all() and abs(G[10]) < 1.0 and A[10] > 1e8
    if C == 1:
        assert got[0] == 0.0
    miss = np.abs(got - G) - (ulp32(G) + 1e-12 * A)
    print(f'[item bias] borders C={C} chunk={chunk}: n_extra {n_extra}, worst |got - G| - bound {miss.max():.3g}')
    assert (miss <= 0).all(), (got, G)
    want = grad_in_kernel_order(rowptr, ent_w, wbuf, n, C, chunk)
    assert np.array_equal(host(g).view(np.int32), want.view(np.int32)), (host(g), want)
    for other in (run_grad(tm, d_rowptr, n, C, d_ent, d_w, chunk, tm.L.EPI_GRAD)[0],                               # twice
                  run_grad(tm, d_rowptr, n, C, d_ent, d_w, chunk, tm.L.EPI_GRAD, stream=torch.cuda.Stream())[0]):  # a stream of its own
        assert torch.equal(bits(other), bits(g))
    # TMF_EPI_ADAM = tmf_adam_fresh_rows_f32 on the TMF_EPI_GRAD output, bit for bit
    b_old = torch.randn(n, generator=torch.Generator().manual_seed(C)).cuda()
    stepped, _ = run_grad(tm, d_rowptr, n, C, d_ent, d_w, chunk, tm.L.EPI_ADAM, b_old=b_old)
    rows = -(-n // 4)
    W, Gp = torch.zeros(4 * rows, device='cuda'), torch.zeros(4 * rows, device='cuda')
    W[:n], Gp[:n] = b_old, g
    tm.L.check(tm.lib.tmf_adam_fresh_rows_f32(W, Gp, rows, 4, tm.E.adam_constants(LR), tm.L.stream_ptr()), tm.lib)
    torch.cuda.synchronize()
    assert torch.equal(bits(stepped), bits(W[:n])) and not torch.equal(stepped[1:], b_old[1:])
    if C == 1:
        assert torch.equal(bits(stepped[:1]), bits(b_old[:1]))                          # an item without entries keeps its bias


def test_grad_on_the_lists_of_a_real_plan(tm):
    """12 x 7 with stored values <= 0: their weights (NaN here) sit in the row behind the lists, which is never read."""
    p = bpr_problem(4, 12, 7, 4, 5)
    m, n, S = p['m'], p['n'], p['S']
    assert (p['val'] <= 0).sum() >= 3
    plan = tm.E.InteractionPlan(dev(p['idx'], torch.int64), dev(p['val'], torch.float32), m, n, csc=False)
    for C in (1, 3):
        wplan = tm.E.WmrbPlan(plan, dev(p['R'], torch.int32), user_chunks=C, item_slices=1, n_components=4, sliced=True)
        nnz = plan.nnz
        rng = np.random.default_rng(C)
        w = rng.standard_normal(nnz + m * S).astype(np.float32)
        val, col, Rs = host(plan.val_u), plan.col_u.cpu().numpy(), wplan.R.cpu().numpy()
        w[:nnz][val <= 0] = np.nan
        wplan.wbuf.copy_(torch.as_tensor(w))
        G, A = np.zeros(n), np.zeros(n)
        for arr, ids in ((w[:nnz][val > 0], col[val > 0]), (w[nnz:], Rs.reshape(-1))):
            np.add.at(G, ids, arr.astype(np.float64))
            np.add.at(A, ids, np.abs(arr.astype(np.float64)))
        for chunk in (4, 1024):
            g, _ = run_grad(tm, wplan.rowptr_e, n, C, wplan.ent_w, wplan.wbuf, chunk, tm.L.EPI_GRAD)
            got = host(g).astype(np.float64)
            assert (np.abs(got - G) <= ulp32(G) + 1e-12 * A).all(), (C, chunk, got, G)
            assert got[p['empty_item']] == 0.0


# ------------------------------------------------------------------------------------------------------------------------
# the engine: one epoch from a non-zero bias
# ------------------------------------------------------------------------------------------------------------------------
_CASES = {}


def engine_case(tm, name, shape, zero_bias=False):
    """(problem, b0, loss object, fp64 reference) of one (loss, shape), computed once and left unchanged.  For the losses with a kink
    the first seed whose margins and positive order are decided at the biased scores."""
    key = (name, shape, zero_bias)
    if key not in _CASES:
        m, n, r, S = shape
        loss = tm.losses[name]()
        for seed in range(300, 340):
            p = bpr_problem(seed, m, n, r, S)
            b0 = np.zeros(n, np.float32) if zero_bias else (np.random.default_rng(seed).standard_normal(n) * 0.3).astype(np.float32)
            ref = biased_reference(loss, p['U0'], p['V0'], b0, p['idx'], p['val'], p['R'], n, S)
            if name not in KINKED or margins_decided(ref['scores'], p['idx'], p['val'], p['R']):
                break
        else:
            raise AssertionError(f'no decided problem for {key}')
        _CASES[key] = (p, b0, loss, ref)
    return _CASES[key]


def engine_state(tm, p, name, loss, b0, U0=None, V0=None, R=None):
    m, n, r, S = p['m'], p['n'], p['r'], p['S']
    rec = tm.E.LOSSES[name]
    plan = tm.E.InteractionPlan(dev(p['idx'], torch.int64), dev(p['val'], torch.float32), m, n, **rec.plan_form())
    table = tm.E.checked_negatives(p['R'] if R is None else R, m, n, 'cuda')
    wplan = tm.E.wmrb_plan_for(plan, table, r, force_sliced=True)
    rec.prepare(wplan, plan)
    st = tm.E.TrainState(p['U0'] if U0 is None else U0, p['V0'] if V0 is None else V0, plan, r, wplan, item_scalar_bias=b0)
    c = rec.param(types.SimpleNamespace(n_items=n, n_samples=S, loss_graph=loss))
    return st, c


def engine_epoch(tm, p, name, loss, b0, lr=LR, prof=None, **kw):
    st, c = engine_state(tm, p, name, loss, b0, **kw)
    out = torch.zeros(1, dtype=torch.float64, device='cuda')
    tm.E.epoch_sides(st, tm.E.adam_constants(lr), out, name, c, prof)
    torch.cuda.synchronize()
    return st, float(out)


FORMS = [{}, {'TMF_SCORES6': '1'}, {'TMF_SCORES7': '1'}, {'TMF_ROW_STATIONARY': '1'}, {'TMF_ROWS4': '1'}]


@pytest.mark.parametrize('env', FORMS, ids=lambda e: '='.join(*e.items()) if e else 'default')
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('name', ['wmrb', 'bpr', 'warp', 'warp_kos', 'softmax'])
def test_one_epoch_from_a_nonzero_bias(tm, monkeypatch, name, shape, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, b0, loss, ref = engine_case(tm, name, shape)
    assert np.abs(ref['gb']).max() > 1e-3 and np.abs(b0).max() > 0.3
    st, loss_sum = engine_epoch(tm, p, name, loss, b0)
    r = p['r']
    assert st.wplan.sliced and st.ib is not None
    if 'TMF_ROWS4' in env:
        assert st.wplan.rows4 == bool(tm.lib.tmf_wsum_rows4_rows_per_group(r, 0)) and (not st.wplan.rows4 or st.wplan.seg_e is None)
    if 'TMF_ROW_STATIONARY' in env:
        assert st.row_stationary == bool(tm.lib.tmf_wmrb_gradu4_supported(r, 0))
    if 'TMF_SCORES6' in env:
        assert (st.wplan.s6 is not None) == bool(tm.lib.tmf_wmrb_scores6_supported(r, 0, p['n']))
    err = rel_err(loss_sum, ref['loss_sum'])
    print(f'[item bias] {name} {shape} {env}: loss {err:.3g}')
    assert err < 1e-5
    what = f'{name} {shape} {env}'
    assert_step(host(st.U[:, :r]), p['U0'], ref['gU'], LR, what=what + ' U')
    assert_step(host(st.V[:, :r]), p['V0'], ref['gV'], LR, what=what + ' V')
    assert_step(host(st.ib.value), b0, ref['gb'], LR, what=what + ' b')
    assert host(st.ib.value)[p['empty_item']] == b0[p['empty_item']]     # nobody's entry, nobody's sample: the bias keeps its bits
    assert not bool(st.ib.b[p['n']:].any())                              # the padding of the vector stays zero


@pytest.mark.parametrize('name', ['wmrb', 'bpr', 'warp', 'warp_kos', 'softmax'])
def test_a_zero_bias_leaves_the_tables_of_a_state_without_one(tm, name):
    p, b0, loss, _ = engine_case(tm, name, SHAPES[0], zero_bias=True)
    with_b, loss_b = engine_epoch(tm, p, name, loss, b0)
    without, loss_0 = engine_epoch(tm, p, name, loss, None)
    assert without.ib is None and loss_b == loss_0
    assert torch.equal(bits(with_b.U), bits(without.U)) and torch.equal(bits(with_b.V), bits(without.V))
    assert bool(with_b.ib.value.abs().max() > 0)


def test_the_spans_of_the_bias_passes(tm):
    p, b0, loss, _ = engine_case(tm, 'bpr', SHAPES[0])
    prof = tm.E.KernelTimer()
    engine_epoch(tm, p, 'bpr', loss, b0, prof=prof)
    order = list(prof.spans)
    assert order.index('wmrb_scores') < order.index('item_bias_add') < order.index('bpr_pairs') < order.index('item_bias_grad')
    assert prof.mean_ms('item_bias_add') > 0 and prof.mean_ms('item_bias_grad') > 0
    prof = tm.E.KernelTimer()
    engine_epoch(tm, p, 'bpr', loss, None, prof=prof)
    assert 'item_bias_add' not in prof.spans and 'item_bias_grad' not in prof.spans


# ------------------------------------------------------------------------------------------------------------------------
# through the public API
# ------------------------------------------------------------------------------------------------------------------------
def fit(tm, p, epochs, loss=None, U0=None, V0=None, lr=LR, item_features=None, bias=True, **attrs):
    graphs = {k: attrs.pop(k) for k in ('user_repr_graph', 'item_repr_graph') if k in attrs}
    model = tm.MF(p['r'], loss_graph=loss or tm.LG.BPRLoss(), user_weight_graph=tm.Fixed(p['U0'] if U0 is None else U0),
                  item_weight_graph=tm.Fixed(p['V0'] if V0 is None else V0), n_users=p['m'], n_items=p['n'], n_samples=p['S'], **graphs)
    model.verbose, model.random_ind, model.scalar_item_bias = False, torch.as_tensor(p['R']), bias
    for k, v in attrs.items():
        setattr(model, k, v)
    model.fit(epochs, tm.eye(p['m']), tm.eye(p['n']) if item_features is None else item_features,
              tm.Sparse(p['idx'], p['val'], (p['m'], p['n'])), lr=lr)
    return model


MODEL_PROBLEM = (77, 60, 40, 12, 20)


def test_the_second_epoch_steps_from_what_the_first_left(tm, engine_only):
    p = bpr_problem(*MODEL_PROBLEM)
    one, two = fit(tm, p, 1), fit(tm, p, 2)
    assert one._state.ib is not None and one.item_bias_.shape == (p['n'],) and one.item_bias_.dtype == torch.float32
    assert one.item_bias_.device == one.item_embedding.device and two.loss_history_[0] == one.loss_history_[0]
    U1, V1, b1 = host(one.user_embedding), host(one.item_embedding), host(one.item_bias_)
    first = biased_reference(tm.LG.BPRLoss(), p['U0'], p['V0'], np.zeros(p['n']), p['idx'], p['val'], p['R'], p['n'], p['S'])
    assert_step(b1, np.zeros(p['n']), first['gb'], LR, what='first epoch b')
    ref = biased_reference(tm.LG.BPRLoss(), U1, V1, b1, p['idx'], p['val'], p['R'], p['n'], p['S'])
    assert rel_err(two.loss_history_[1], ref['loss_sum'] / ref['n_terms']) < 1e-5
    assert_step(host(two.user_embedding), U1, ref['gU'], LR, what='second epoch U')
    assert_step(host(two.item_embedding), V1, ref['gV'], LR, what='second epoch V')
    assert_step(host(two.item_bias_), b1, ref['gb'], LR, what='second epoch b')
    plain = fit(tm, p, 2, bias=False)
    assert plain.item_bias_ is None and plain._state.ib is None and plain.loss_history_[0] == two.loss_history_[0]
    assert plain.loss_history_[1] != two.loss_history_[1]


def test_wmrb_with_the_bias_takes_the_sliced_plan(tm, engine_only):
    p, _, loss, _ = engine_case(tm, 'wmrb', SHAPES[0], zero_bias=True)
    ref = biased_reference(loss, p['U0'], p['V0'], np.zeros(p['n']), p['idx'], p['val'], p['R'], p['n'], p['S'])
    on, off = fit(tm, p, 1, loss=tm.LG.WMRBLoss()), fit(tm, p, 1, loss=tm.LG.WMRBLoss(), bias=False)
    assert on._state.wplan.sliced and not off._state.wplan.sliced
    assert rel_err(on.loss_history_[0], ref['loss_sum'] / ref['n_terms']) < 1e-5
    assert_step(host(on.item_bias_), np.zeros(p['n']), ref['gb'], LR, what='wmrb b')
    assert_step(host(on.user_embedding), p['U0'], ref['gU'], LR, what='wmrb U')


def test_opt_in_persistent_adam(tm, engine_only):
    """optimizer='adam' over 3 epochs against the fp64 Adam recursion on U, V and b (tests/test_gpu_bpr.py's tolerance)."""
    p = bpr_problem(*MODEL_PROBLEM)
    got = fit(tm, p, 3, optimizer='adam')
    X = [p['U0'].astype(np.float64), p['V0'].astype(np.float64), np.zeros(p['n'])]
    M, V2 = [np.zeros_like(x) for x in X], [np.zeros_like(x) for x in X]
    history = []
    for t in range(1, 4):
        ref = biased_reference(tm.LG.BPRLoss(), X[0], X[1], X[2], p['idx'], p['val'], p['R'], p['n'], p['S'])
        history.append(ref['loss_sum'] / ref['n_terms'])
        alpha = LR * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        for i, g in enumerate((ref['gU'], ref['gV'], ref['gb'])):
            M[i] += (g - M[i]) * 0.1
            V2[i] += (g ** 2 - V2[i]) * 0.001
            X[i] = X[i] - alpha * M[i] / (np.sqrt(V2[i]) + 1e-7)
    assert rel_err(got.loss_history_, history) < 1e-4
    for have, want in zip((got.user_embedding, got.item_embedding, got.item_bias_), X):
        assert np.abs(host(have) - want).max() < 1e-3
    assert np.abs(X[2]).max() > 0.05
    first = fit(tm, p, 1, optimizer='adam'), fit(tm, p, 1)
    assert torch.equal(first[0].item_bias_, first[1].item_bias_) and torch.equal(first[0].user_embedding, first[1].user_embedding)


def test_graph_replay(tm, engine_only, monkeypatch):
    p = bpr_problem(*MODEL_PROBLEM)
    monkeypatch.delenv('TMF_NO_GRAPH', raising=False)
    a = fit(tm, p, 8)
    monkeypatch.setenv('TMF_NO_GRAPH', '1')
    b = fit(tm, p, 8)
    assert a.graph_epochs_ == 8 and b.graph_epochs_ == 0 and a.loss_history_ == b.loss_history_
    for x, y in ((a.user_embedding, b.user_embedding), (a.item_embedding, b.item_embedding), (a.item_bias_, b.item_bias_)):
        assert torch.equal(bits(x), bits(y))
    assert a.loss_history_[-1] < a.loss_history_[0]


def test_resampling_every_epoch_is_three_chained_engine_epochs(tm, engine_only):
    p, seed = bpr_problem(*MODEL_PROBLEM), 21
    whole = fit(tm, p, 3, resample_every=1, sample_seed=seed)
    assert whole.resample_rounds_ == 3 and bool(whole.item_bias_.abs().max() > 0)
    U, V, b, history = p['U0'], p['V0'], np.zeros(p['n'], np.float32), []
    n_pos = int((p['val'] > 0).sum())
    for j in range(3):
        R = p['R'] if j == 0 else tm.ops.sample_negatives(p['n'], p['m'], p['S'], seed=seed + j, device='cuda').cpu().numpy()
        st, loss_sum = engine_epoch(tm, p, 'bpr', tm.LG.BPRLoss(), b, U0=U, V0=V, R=R)
        U, V, b = host(st.U[:, :p['r']]), host(st.V[:, :p['r']]), host(st.ib.value)
        history.append(loss_sum / n_pos)
    assert whole.loss_history_ == history
    assert np.array_equal(host(whole.user_embedding), U) and np.array_equal(host(whole.item_embedding), V)
    assert np.array_equal(host(whole.item_bias_), b)


def test_sides_and_the_bias_one_step(tm, engine_only):
    """A biased item side and an item side over SparseFeatures: the bias passes never see the tables."""
    from test_gpu_features import assert_step_with_slack
    p = bpr_problem(1033, 60, 40, 33, 64)
    n, r = p['n'], p['r']
    ref = biased_reference(tm.LG.BPRLoss(), p['U0'], p['V0'], np.zeros(n), p['idx'], p['val'], p['R'], n, p['S'])
    model = fit(tm, p, 1, item_repr_graph=tm.EG.BiasedLinearEmbedding())
    assert model._state.bias_v is not None and model._state.ib is not None
    assert rel_err(model.loss_history_[0], ref['loss_sum'] / ref['n_terms']) < 1e-5
    assert_step(host(model.user_embedding), p['U0'], ref['gU'], LR, what='biased side U')
    assert_step(host(model.item_trainable[0]), p['V0'], ref['gV'], LR, what='biased side item weights')
    assert_step(host(model.item_bias_), np.zeros(n), ref['gb'], LR, what='biased side b')
    rng = np.random.default_rng(5)
    T = 6
    tag_idx = np.argwhere(rng.random((n, T)) < 0.3)
    tag_val = rng.choice(np.array([1.0, 0.5, -0.25, 2.0], np.float32), tag_idx.shape[0])
    F = tm.hstack(n, tm.SF(tag_idx, tag_val, (n, T)))
    F_dense = np.zeros((n, n + T))
    F_dense[np.arange(n), np.arange(n)] = 1.0
    F_dense[tag_idx[:, 0], n + tag_idx[:, 1]] = tag_val
    W0 = (rng.standard_normal((n + T, r)) * 0.3).astype(np.float32)
    E0 = F_dense @ W0.astype(np.float64)
    ref = biased_reference(tm.LG.BPRLoss(), p['U0'], E0, np.zeros(n), p['idx'], p['val'], p['R'], n, p['S'])
    model = fit(tm, p, 1, V0=W0, item_features=F)
    assert model._state.feat_v is not None and model._state.ib is not None
    assert rel_err(model.loss_history_[0], ref['loss_sum'] / ref['n_terms']) < 1e-5
    assert_step(host(model.user_embedding), p['U0'], ref['gU'], LR, what='features U')
    assert_step(host(model.item_bias_), np.zeros(n), ref['gb'], LR, what='features b')
    slack = 1e-5 * np.abs(F_dense).T @ np.abs(ref['gV'])
    assert_step_with_slack(host(model.item_trainable[0]), W0, F_dense.T @ ref['gV'], slack, LR, 'item weights over sparse features')


def test_the_bias_is_never_penalised(tm, engine_only):
    alpha = 0.01
    p = bpr_problem(*MODEL_PROBLEM)
    ref = biased_reference(tm.LG.BPRLoss(), p['U0'], p['V0'], np.zeros(p['n']), p['idx'], p['val'], p['R'], p['n'], p['S'])
    model = fit(tm, p, 1, user_alpha=alpha, item_alpha=alpha)
    assert model._state.l2 == [np.float32(2 * alpha)] * 2
    assert_step(host(model.user_embedding), p['U0'], ref['gU'] + 2 * alpha * p['U0'].astype(np.float64), LR, what='l2 U')
    assert_step(host(model.item_embedding), p['V0'], ref['gV'] + 2 * alpha * p['V0'].astype(np.float64), LR, what='l2 V')
    assert_step(host(model.item_bias_), np.zeros(p['n']), ref['gb'], LR, what='l2 b')
    assert torch.equal(model.item_bias_, fit(tm, p, 1).item_bias_)        # the unpenalised gradient's step, bit for bit


def test_the_generic_loop_on_the_gpu_and_predict(tm):
    """A plug-in loss trains its bias in the generic loop; predict() is U V^T + b."""
    class PluginBPR(tm.LG.BPRLoss):
        pass
    p = bpr_problem(*MODEL_PROBLEM)
    model = fit(tm, p, 3, loss=PluginBPR())
    assert getattr(model, '_state', None) is None and model.item_bias_ is not None
    want = host(model.user_embedding).astype(np.float64) @ host(model.item_embedding).astype(np.float64).T + host(model.item_bias_)[None, :]
    assert rel_err(host(model.predict()), want) < 1e-6
    engine = fit(tm, p, 1)
    assert rel_err(engine.loss_history_[0], model.loss_history_[0]) < 1e-5


# ------------------------------------------------------------------------------------------------------------------------
# ranking on the augmented tables
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ranked(tm):
    """A trained 64 x 300 model, r = 16, whose bias reorders the top of at least half the users; items 7 and 9 made exact ties
    (equal factors, equal bias); a held-out table and an exclusion table that do not overlap."""
    p = bpr_problem(5, 64, 300, 16, 32, density=0.05)
    model = fit(tm, p, 6, lr=0.2)
    with torch.no_grad():
        model.item_embedding[9] = model.item_embedding[7]
        model.item_bias_[9] = model.item_bias_[7]
    rng = np.random.default_rng(9)
    mask = rng.random((64, 300))
    test = np.argwhere(mask < 0.03)
    excl = np.argwhere(mask > 0.9)
    gains = rng.integers(1, 4, test.shape[0]).astype(np.float32)
    A = tm.Sparse(test, gains, (64, 300))
    X = tm.Sparse(excl, np.ones(excl.shape[0], np.float32), (64, 300))
    dense = np.zeros((64, 300), np.float32)
    dense[test[:, 0], test[:, 1]] = gains
    return model, A, X, test, excl, dense


def dense_ranking(P, k, excl=None):
    P = np.array(P, np.float64)
    if excl is not None:
        P[excl[:, 0], excl[:, 1]] = -np.inf
    order = np.argsort(-P, axis=1, kind='stable')
    return order[:, :k]


def test_the_bias_reorders_the_lists(tm, ranked):
    model = ranked[0]
    with_b = model.retrieve_user_recs(k=10)
    bias, model.item_bias_ = model.item_bias_, None
    try:
        without = model.retrieve_user_recs(k=10)
        plain = host(model.predict())
    finally:
        model.item_bias_ = bias
    changed = int((with_b != without).any(axis=1).sum())
    print(f'[item bias] top-10 lists changed by the bias: {changed} of 64 users')
    assert changed >= 32
    assert rel_err(host(model.predict()), plain.astype(np.float64) + host(bias)[None, :]) < 1e-6


@pytest.mark.parametrize('arithmetic', ['fp32', 'split', 'auto'])
def test_rankings_are_those_of_the_dense_scores(tm, ranked, arithmetic):
    model, A, X, test, excl, dense = ranked
    model.predict_arithmetic = arithmetic
    try:
        P = model.predict()
        for ex_table, ex_pairs in ((None, None), (X, excl)):
            top = model.retrieve_user_recs(k=10, exclude=ex_table)
            ex = None if ex_table is None else model._exclusion(ex_table)
            assert np.array_equal(top, tm.ops.topk_stable(P.clone(), 10, exclude=ex).cpu().numpy())
            Pn = host(P)
            assert np.array_equal(top, dense_ranking(Pn, 10, ex_pairs))
            # exact ties created through b: the lower id first
            for row in top:
                if 9 in row:
                    assert 7 in row and list(row).index(7) + 1 == list(row).index(9)
            # item_ranks / recall / auc from the dense scores
            D = np.array(Pn, np.float64)
            if ex_pairs is not None:
                D[ex_pairs[:, 0], ex_pairs[:, 1]] = -np.inf
            pairs, ranks = model.item_ranks(A, exclude=ex_table)
            pairs, ranks = pairs.cpu().numpy(), ranks.cpu().numpy()
            assert np.array_equal(pairs, test[np.lexsort((test[:, 1], test[:, 0]))])
            ids = np.arange(300)
            want = np.array([int(((D[u] > D[u, i]) | ((D[u] == D[u, i]) & (ids < i))).sum()) for u, i in pairs])
            assert np.array_equal(ranks, want)
            relevant = np.bincount(test[:, 0], minlength=64)
            hits = np.array([np.isin(top[u], test[test[:, 0] == u, 1]).sum() for u in range(64)])
            recall = host(model.recall_at_k(A, k=10, preserve_rows=True, exclude=ex_table))
            assert np.allclose(recall, np.where(relevant > 0, hits / np.maximum(relevant, 1), 0.0), rtol=1e-6, atol=0)
            n_excl = np.zeros(64) if ex_pairs is None else np.bincount(ex_pairs[:, 0], minlength=64)
            auc = host(model.auc_score(A, preserve_rows=True, exclude=ex_table))
            for u in range(64):
                r_u = np.sort(want[pairs[:, 0] == u])
                if r_u.size:
                    N = 300 - n_excl[u] - r_u.size
                    assert abs(auc[u] - (1 - (r_u - np.arange(r_u.size)).sum() / (r_u.size * N))) < 1e-6
        # ndcg: the sparse path (top-k of the fused kernels) against the reference's full sort of predict()
        sparse_path = host(model.ndcg_at_k(A, k=10, preserve_rows=True))
        dense_path = host(model.ndcg_at_k(torch.as_tensor(dense), k=10, preserve_rows=True))
        assert np.allclose(sparse_path, dense_path, rtol=1e-5, atol=1e-7)
    finally:
        model.predict_arithmetic = None


def test_a_model_of_256_components_ranks_through_the_general_path(tm):
    rank_a_wide_model(tm, 256, fused=False)


@pytest.mark.parametrize('r', [127, 128, 255])
def test_models_up_to_the_widest_fused_tables_rank_with_a_bias(tm, r):
    """[U | 1], [V | b] of 128, 129 and 256 columns: the last width of the 128-column kernels, the first past it, and the widest the
    fused ranking kernels take (_ops.FUSED_MAX_R)."""
    assert r + 1 <= tm.ops.FUSED_MAX_R == 256
    rank_a_wide_model(tm, r, fused=True)


def rank_a_wide_model(tm, r, fused):
    g = torch.Generator().manual_seed(3)
    model = tm.MF(r, n_users=40, n_items=90)
    model.user_embedding = (torch.randn(40, r, generator=g) * 0.1).cuda()
    model.item_embedding = (torch.randn(90, r, generator=g) * 0.1).cuda()
    model.item_embedding[11] = model.item_embedding[4]
    model.item_bias_ = torch.randn(90, generator=g).cuda()
    model.item_bias_[11] = model.item_bias_[4]
    Ua, Va, says = model._score_tables()
    assert says is fused and Ua.shape == (40, r + 1) and Va.shape == (90, r + 1)
    P = model.predict()
    want = host(model.user_embedding).astype(np.float64) @ host(model.item_embedding).astype(np.float64).T + host(model.item_bias_)[None, :]
    assert rel_err(host(P), want) < 1e-6
    for arithmetic in (None, 'fp32', 'split'):
        model.predict_arithmetic = arithmetic
        top = model.retrieve_user_recs(k=10)
        assert np.array_equal(top, tm.ops.topk_stable(P.clone(), 10).cpu().numpy()) and np.array_equal(top, dense_ranking(host(P), 10))
        for row in top:
            if 11 in row:
                assert list(row).index(4) + 1 == list(row).index(11)
        test = np.argwhere(np.random.default_rng(1).random((40, 90)) < 0.05)
        pairs, ranks = model.item_ranks(tm.Sparse(test, np.ones(test.shape[0], np.float32), (40, 90)))
        D, ids = host(P).astype(np.float64), np.arange(90)
        want_r = [int(((D[u] > D[u, i]) | ((D[u] == D[u, i]) & (ids < i))).sum()) for u, i in pairs.cpu().numpy()]
        assert ranks.cpu().tolist() == want_r
