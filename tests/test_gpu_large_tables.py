"""Kernels on tables past the 32-bit offset limits.  Several hot kernels reach V through 32-bit byte offsets while the table is
below 4 GB and switch to a 64-bit form above it:
  k_predict_topk (fp32)        MODE 2 (buffer descriptor, 32-bit voffset) while (n + 4*FBN) * ldb * 4 < 2^32, else MODE 1
  k_predict_topk_bf16          MODE 2 while (n + 4*HBN) * ldb * 2 < 2^32, else MODE 0
  tmf_wmrb_scores3             lean walk (load_raw32 / row_byte_off) while n_items * row_bytes < 2^32, else the general form
  tmf_wmrb_scores6 / scores5   only while n_items * row_bytes < 2^32; the engine falls back to scores3 beyond
Every size below comes from the launch condition it targets, with an assert that restates it: the largest table of the 32-bit
form, the smallest of the 64-bit form, and one with real rows past byte 2^32.

Data that exposes a wrong offset: integer factors (exact in fp32, in the bf16 / fp16 planes and in bf16 storage); rows around
byte 2^31 and 2^32, the last row and the first row of the ragged last tile are "beacons": 3 * sign(U[u]) for one user u, which
outscores every other row for u.  Past 4 GB, row j and row j - 2^32 / B (what an offset truncated to 32 bits reads) are beacons
of different users.  Rankings are compared id for id and value for value with a chunked fp64 torch product + stable sort
(oracle.dense_ref.tf_top_k_chunked); training with the fp64 closed form (oracle.sparse_ref) and across the kernel forms."""
import types

import numpy as np
import pytest
import torch

from conftest import assert_step
from test_gpu_c5shard import assert_step_bf16, check_user as check_user_bf16
from test_gpu_fullsize import check_user_against_oracle, independent_item_gradient

pytestmark = pytest.mark.gpu

GB = 1 << 30
TWO31, TWO32 = 1 << 31, 1 << 32
FBN = HBN = 128   # item tile of k_predict_topk / k_predict_topk_bf16 (tmf_predict.hip)
DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    from teamoflow_amd import _lib, _ops
    _lib.get()
    return _ops


def need(nbytes):
    """Skip (the machines are shared) unless `nbytes` of device memory are free."""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f'needs {nbytes / 1e9:.1f} GB of free device memory, {free / 1e9:.1f} GB free')
    torch.cuda.reset_peak_memory_stats()


def release(what=None):
    torch.cuda.synchronize()
    if what:
        print(f'[large tables] {what}: peak {torch.cuda.max_memory_allocated() / 1e9:.1f} GB allocated')
    torch.cuda.empty_cache()


def fp32_mode2(n, ldb):
    return (n + 4 * FBN) * ldb * 4 < TWO32


def bf16_mode2(n, ldb):
    return (n + 4 * HBN) * ldb * 2 < TWO32


def named_rows(n, row_bytes, tile):
    """The rows on either side of byte 2^31 and 2^32 (where the table reaches them), n - 1, the first row of the last tile; and the
    alias pairs (j past byte 2^32, j - 2^32 / row_bytes) for three such j."""
    rows = []
    for edge in (TWO31, TWO32):
        j = -(-edge // row_bytes)
        if j < n:
            rows += [j - 1, j]
    rows += [n - 1, (n - 1) // tile * tile]
    aliases = []
    hi = -(-TWO32 // row_bytes)
    if hi < n:
        assert TWO32 % row_bytes == 0
        step = TWO32 // row_bytes
        aliases = [(j, j - step) for j in (hi, (hi + n) // 2, n - 1)]
    return sorted(set(rows)), aliases


def beacon_table(n, r, m, dtype, tile, seed):
    """U [m, r] in {-2..2} (no zero row), V [n, r] in {-1, 0, 1} made on the device; about 12 beacon rows per user in windows
    around the named and alias rows, owners assigned round-robin, the high row of an alias pair never owned by its partner's user."""
    row_bytes = r * (2 if dtype is torch.bfloat16 else 4)
    named, aliases = named_rows(n, row_bytes, tile)
    anchors = sorted(set(named) | {a for p in aliases for a in p})
    w = 12 * m // len(anchors)
    while True:   # windows wide enough for about 12 beacons per user (windows at the end of the table overlap)
        rows = torch.unique(torch.cat([torch.arange(max(0, a - w // 2), min(n, a + w // 2 + 1)) for a in anchors]))
        if rows.numel() >= 12 * m:
            break
        w += w // 2
    owner = torch.arange(rows.numel()) % m
    if aliases:   # j past byte 2^32 and j - 2^32 / B: beacons of different users
        step = TWO32 // row_bytes
        pos = {int(x): i for i, x in enumerate(rows.tolist())}
        for i, x in enumerate(rows.tolist()):
            if x >= step and (x - step) in pos and owner[i] == owner[pos[x - step]]:
                owner[i] = (owner[i] + 1) % m
        for j, a in aliases:
            assert owner[pos[j]] != owner[pos[a]]
    g = torch.Generator(device=DEV).manual_seed(seed)
    U = torch.randint(-2, 3, (m, r), generator=g, device=DEV, dtype=torch.float32)
    U[U.abs().sum(1) == 0, 0] = 1
    V = torch.randint(-1, 2, (n, r), generator=g, device=DEV, dtype=torch.int8).to(dtype)
    rows_d, owner_d = rows.to(DEV), owner.to(DEV)
    V[rows_d] = (3 * torch.sign(U[owner_d])).to(dtype)
    beacons = [rows[owner == u] for u in range(m)]
    return dict(U=U.to(dtype), V=V, named=named, aliases=aliases, beacons=beacons, rows=rows, owner=owner, n=n, r=r, m=m)


def reference(t, k, **kw):
    from oracle import dense_ref as D
    return D.tf_top_k_chunked(t['U'], t['V'], k, **kw)


def check(got, want, k, what):
    gv, gi = got
    wv, wi = want
    wi, wv = wi[:, :k], wv[:, :k]
    bad = (gi.long() != wi).any(1)
    assert not bool(bad.any()), f'{what}: wrong ids in {int(bad.sum())} of {bad.numel()} rows, first {int(bad.nonzero()[0])}'
    assert torch.equal(gv.double(), wv), f'{what}: values differ'


def check_beacons(t, ref_i):
    """The data does what it is meant to: each user's best rows are its beacons, in ascending id."""
    for u in (0, t['m'] // 2, t['m'] - 1):
        b = t['beacons'][u]
        assert torch.equal(ref_i[u, :b.numel()].cpu(), b), u


FP32_TABLES = {  # id: (n, r, 32-bit form wanted)
    'fp32_r128_last_mode2': (8_388_095, 128, True),
    'fp32_r128_first_mode1': (8_388_096, 128, False),
    'fp32_r128_past_4gb': (9_000_000, 128, False),
    'fp32_r256_first_mode1': (4_193_792, 256, False),
}


@pytest.mark.parametrize('case', list(FP32_TABLES))
def test_fp32_ranking_at_the_offset_edges(ops, case):
    n, r, mode2 = FP32_TABLES[case]
    assert fp32_mode2(n, r) == mode2
    if case == 'fp32_r128_last_mode2':     # the largest MODE 2 table: its last row ends within 256 KB + one row of byte 2^32
        assert not fp32_mode2(n + 1, r) and TWO32 - n * r * 4 <= 256 * 1024 + r * 4
    elif case == 'fp32_r128_past_4gb':     # MODE 1 with real rows past byte 2^32
        assert (n - 1) * r * 4 >= TWO32 + GB // 4
    else:                                  # the smallest MODE 1 table: below 4 GB, the 4 * FBN prefetch margin decides
        assert fp32_mode2(n - 1, r) and n * r * 4 < TWO32
    past = n * r * 4 > TWO32
    m = 300
    split_ws = ops._lib.get().tmf_predict_topk_split_workspace_bytes(n, r)
    need(n * r * 4 + split_ws + 12 * GB)
    t = beacon_table(n, r, m, torch.float32, FBN, seed=n + r)
    U, V = t['U'], t['V']
    want = reference(t, 50)
    check_beacons(t, want[1])
    assert bool((want[0][:, 49] > 0).all())   # every listed score is positive: the clamped ranking is the same list
    for k in (10, 20, 50):
        check(ops.predict_topk(U, V, k, return_values=True, arithmetic='fp32'), want, k, f'{case} fp32 k={k}')
    check(ops.predict_topk(U, V, 20, clamp_negatives=True, return_values=True, arithmetic='fp32'), want, 20, f'{case} fp32 clamp')
    for arith in ('split', 'half2'):
        for k in (10, 30):
            check(ops.predict_topk(U, V, k, clamp_negatives=k == 30, return_values=True, arithmetic=arith), want, k, f'{case} {arith} k={k}')
    release()
    if past:
        # each user's first beacon and one alias row left out: the EXCL instances at ids past 2^23
        hi = torch.tensor([a for p in t['aliases'] for a in p])
        rows = torch.cat([torch.arange(m), torch.arange(m)])
        cols = torch.cat([torch.stack([b[0] for b in t['beacons']]), hi[torch.arange(m) % hi.numel()]])
        ex = ops.build_exclusion(types.SimpleNamespace(indices=torch.stack([rows, cols], 1).to(DEV), values=torch.ones(2 * m, device=DEV)), m, n)
        wx = reference(t, 20, excluded=(rows.to(DEV), cols.to(DEV)))
        check(ops.predict_topk(U, V, 20, return_values=True, arithmetic='fp32', exclude=ex), wx, 20, f'{case} fp32 exclude')
        check(ops.predict_topk(U, V, 10, return_values=True, arithmetic='split', exclude=ex), wx, 10, f'{case} split exclude')
        check(ops.predict_topk(U, V, 10, return_values=True, arithmetic='half2', exclude=ex), wx, 10, f'{case} half2 exclude')
        release()
        # the non-fused path: predict_gemm + topk_stable over score blocks
        from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
        model = MatrixFactorization(r)
        model.user_embedding, model.item_embedding = U[m - 130:], V
        from oracle import dense_ref as D
        w100 = D.tf_top_k_chunked(U[m - 130:], V, 100)[1].cpu().numpy()
        got = model.retrieve_user_recs(k=100)
        assert np.array_equal(got, w100)
        assert np.array_equal(model.retrieve_user_recs(user=129, k=100), w100[129])
    del t, U, V, want
    release(case)


BF16_TABLES = {  # id: (n, 32-bit form wanted), r = 256
    'bf16_r256_last_mode2': (8_388_095, True),
    'bf16_r256_first_mode0': (8_388_096, False),
    'bf16_r256_past_4gb': (9_000_000, False),
}


@pytest.mark.parametrize('case', list(BF16_TABLES))
def test_bf16_ranking_at_the_offset_edges(ops, case):
    n, mode2 = BF16_TABLES[case]
    r, m = 256, 300
    assert bf16_mode2(n, r) == mode2
    if mode2:                              # the largest MODE 2 table
        assert not bf16_mode2(n + 1, r)
    elif n == 8_388_096:                   # the smallest MODE 0 table (below 4 GB: the 4 * HBN prefetch margin decides)
        assert bf16_mode2(n - 1, r) and n * r * 2 < TWO32
    else:                                  # MODE 0 with real rows past byte 2^32
        assert (n - 1) * r * 2 >= TWO32 + GB // 4
    past = n * r * 2 > TWO32
    need(n * r * 2 + n * r * 4 + 12 * GB)   # the bf16 table and the fp32 copy the k > 32 path makes
    t = beacon_table(n, r, m, torch.bfloat16, HBN, seed=n + 7)
    U, V = t['U'], t['V']
    want = reference(t, 50)
    check_beacons(t, want[1])
    for k in (10, 32, 50):   # 50: the fp32 kernel on the exact fp32 copy of the table (8.6 GB past 4 GB)
        check(ops.predict_topk(U, V, k, clamp_negatives=k == 32, return_values=True), want, k, f'{case} k={k}')
    release()
    if past:
        hi = torch.tensor([a for p in t['aliases'] for a in p])
        rows = torch.cat([torch.arange(m), torch.arange(m)])
        cols = torch.cat([torch.stack([b[0] for b in t['beacons']]), hi[torch.arange(m) % hi.numel()]])
        ex = ops.build_exclusion(types.SimpleNamespace(indices=torch.stack([rows, cols], 1).to(DEV), values=torch.ones(2 * m, device=DEV)), m, n)
        wx = reference(t, 50, excluded=(rows.to(DEV), cols.to(DEV)))
        check(ops.predict_topk(U, V, 10, return_values=True, exclude=ex), wx, 10, f'{case} exclude k=10')
        check(ops.predict_topk(U, V, 50, return_values=True, exclude=ex), wx, 50, f'{case} exclude k=50')
    del t, U, V, want
    release(case)


def test_user_table_past_2_31_elements(ops):
    """17M users x 128 fp32 = 8.7 GB: more than 2^31 elements of U.  The rows of the first users, those around element 2^31 and
    byte 2^32 of U, and the last 256 users, all three arithmetics, against the fp64 product of those rows."""
    m, n, r = 17_000_000, 4096, 128
    assert m * r > TWO31
    need(m * r * 4 + m * 50 * 8 + 6 * GB)
    g = torch.Generator(device=DEV).manual_seed(17)
    U = torch.randint(-2, 3, (m, r), generator=g, device=DEV, dtype=torch.float32)
    V = torch.randint(-1, 2, (n, r), generator=g, device=DEV, dtype=torch.float32)
    probe = torch.cat([torch.arange(8), torch.arange(TWO32 // (4 * r) - 4, TWO32 // (4 * r) + 4),
                       torch.arange(TWO31 // r - 4, TWO31 // r + 4), torch.arange(m - 256, m)]).to(DEV)
    from oracle import dense_ref as D
    want = D.tf_top_k_chunked(U[probe], V, 50)
    for arith, ks in (('fp32', (10, 50)), ('split', (10, 30)), ('half2', (10, 30))):
        for k in ks:
            v, i = ops.predict_topk(U, V, k, return_values=True, arithmetic=arith)
            check((v[probe], i[probe]), want, k, f'many users {arith} k={k}')
            del v, i
            release()
    del U, V
    release('17M users')


# ---------------------------------------------------------------------------------------------------------------------------
# training: WMRB epochs on item tables at the 4 GB edge (512-byte rows) and past it
# ---------------------------------------------------------------------------------------------------------------------------
WMRB_LAST = (1 << 23) - 1     # the largest table scores6, scores5 and the lean scores3 walk accept at 512-byte rows
WMRB_PAST = 9_000_000


def wmrb_problem(n, r, dtype, dyadic, seed, m=4096, S=256):
    """m users, S negatives each drawn uniformly, ~20 positives per user drawn uniformly plus one on a named row; the first two
    negatives of every user forced onto the named and alias rows."""
    from teamoflow_amd.mf.utils import random_sampler_device
    row_bytes = r * (2 if dtype is torch.bfloat16 else 4)
    named, aliases = named_rows(n, row_bytes, 128)
    special = torch.tensor(sorted(set(named) | {a for p in aliases for a in p}), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    u = torch.cat([torch.randint(0, m, (20 * m,), generator=g, device=DEV), torch.arange(m, device=DEV)])
    j = torch.cat([torch.randint(0, n, (20 * m,), generator=g, device=DEV), special[torch.arange(m, device=DEV) % special.numel()]])
    key = torch.unique(u * n + j)
    idx = torch.stack([key // n, key % n], 1)
    val = torch.randint(1, 6, (key.numel(),), generator=g, device=DEV).float()
    R = random_sampler_device(n, m, S, seed=seed, device=DEV)
    R[:, 0] = special[torch.arange(m, device=DEV) % special.numel()].to(R.dtype)
    R[:, 1] = special[(torch.arange(m, device=DEV) * 7 + 3) % special.numel()].to(R.dtype)
    if dyadic:   # multiples of 1/8: every product and every partial sum is exact in fp32 and in bf16 storage
        U = torch.randint(-8, 9, (m, r), generator=g, device=DEV, dtype=torch.float32) / 8
        V = torch.randint(-8, 9, (n, r), generator=g, device=DEV, dtype=torch.float32) / 8
    else:
        U = torch.randn(m, r, generator=g, device=DEV) * 0.3
        V = torch.randn(n, r, generator=g, device=DEV) * 0.3
    if dtype is torch.bfloat16:
        U, V = U.to(torch.bfloat16), V.to(torch.bfloat16)
    return dict(idx=idx, val=val, R=R, U0=U, V0=V, m=m, n=n, r=r, S=S, special=special.tolist(), lr=0.05, dtype=dtype)


def wmrb_epoch(eng, monkeypatch, p, form):
    """One epoch through the named form of the scores kernel: 'lean' (scores3, 32-bit walk), 'general' (scores3, 64-bit),
    's6', 's5'.  -> dict of the engine objects and the epoch's outputs."""
    from teamoflow_amd import _lib
    monkeypatch.setenv('TMF_SCORES5', '1' if form == 's5' else '0')
    monkeypatch.setenv('TMF_SCORES6', '1' if form in ('s6', 'asked_s6') else '0')
    monkeypatch.setenv('TMF_LEAN', '0' if form == 'general' else '1')
    m, n, r, S, dtype = p['m'], p['n'], p['r'], p['S'], p['dtype']
    plan = eng.InteractionPlan(p['idx'], p['val'], m, n)
    wplan = eng.WmrbPlan(plan, p['R'], item_slices=eng.default_item_slices(n, _lib.padded_ld(r, dtype), elem_size=2 if dtype is torch.bfloat16 else 4), n_components=r, sliced=True)
    st = eng.TrainState(p['U0'].float(), p['V0'].float(), plan, r, wplan, dtype=dtype)
    if form != 'asked_s6':   # asked_s6: TMF_SCORES6=1, the engine decides
        assert (wplan.s6 is not None) == (form == 's6') and (wplan.s5 is not None) == (form == 's5'), form
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    eng.epoch_wmrb(st, eng.adam_constants(p['lr']), n / S, loss)
    torch.cuda.synchronize()
    return dict(st=st, plan=plan, wplan=wplan, loss=float(loss), D_model=wplan.D_in_model_order())


def wmrb_need(n, r, dtype):
    es = 2 if dtype is torch.bfloat16 else 4
    return 4 * n * r * es + n * r * 4 + 8 * GB   # input, V, V_nxt, the copy kept for comparison, fp32 staging


@pytest.fixture(scope='module')
def eng():
    from teamoflow_amd import _engine, _lib
    _lib.get()
    return _engine


@pytest.mark.parametrize('r,dtype', [(128, torch.float32), (256, torch.bfloat16)], ids=['fp32_r128', 'bf16_r256'])
def test_wmrb_forms_bit_identical_at_the_last_32bit_table(eng, monkeypatch, r, dtype):
    """n_items = 2^23 - 1 at 512-byte rows: the last row ends at byte 2^32 - 1.  Dyadic tables: lean scores3, general scores3
    (64-bit addressing), scores6 and scores5 give the same bits in sp, pk, D, delta, loss, U_nxt and V_nxt."""
    from teamoflow_amd import _lib
    n = WMRB_LAST
    lib = _lib.load_library()
    row_bytes = _lib.padded_ld(r, dtype) * (2 if dtype is torch.bfloat16 else 4)
    assert n * row_bytes < TWO32 <= (n + 1) * row_bytes
    bf = int(dtype is torch.bfloat16)
    assert lib.tmf_wmrb_scores6_supported(r, bf, n) == 1 and lib.tmf_wmrb_scores5_supported(r, bf, n) == 1
    need(wmrb_need(n, r, dtype))
    p = wmrb_problem(n, r, dtype, dyadic=True, seed=23 + r)
    base = None
    for form in ('general', 'lean', 's6', 's5'):
        e = wmrb_epoch(eng, monkeypatch, p, form)
        st, w = e['st'], e['wplan']
        out = dict(sp=st.sp.clone(), pk=st.pk.clone(), D=w.D.clone(), delta=w.delta.clone(),
                   U=st.U_nxt.clone(), loss=e['loss'])
        if base is None:
            base, V1 = out, st.V_nxt.clone()
        else:
            for key in ('sp', 'pk', 'D', 'delta', 'U'):
                assert torch.equal(out[key], base[key]), (form, key)
            assert out['loss'] == base['loss'], form
            assert torch.equal(st.V_nxt, V1), (form, 'V_nxt')
        del e, st, w, out
        release()
    del base, V1, p
    release(f'wmrb forms {dtype}')


def check_wmrb_against_fp64(p, e, r, what):
    """sp / pk of every user against an fp64 product; D, delta, loss and the new row of sampled users (those whose positives and
    negatives sit on the named and alias rows among them) against the closed form; the new rows of the named and alias items
    against an fp64 resummation of their entry sets."""
    st, plan, w = e['st'], e['plan'], e['wplan']
    m, S = p['m'], p['S']
    U64 = st.U[:m, :r].double()
    sp_ref = torch.empty(m, S, dtype=torch.float64, device=DEV)
    Rs = w.R.long()   # sp is in the plan's (R-sorted) order
    for b in range(0, m, 512):
        sp_ref[b:b + 512] = torch.einsum('ur,usr->us', U64[b:b + 512], st.V[Rs[b:b + 512], :r].double())
    assert float((st.sp.double() - sp_ref).abs().max()) <= 1e-5 * float(sp_ref.abs().max()), what
    pk_ref = (st.U[plan.user_of.long(), :r].double() * st.V[plan.col_u.long(), :r].double()).sum(1)
    assert float((st.pk[:plan.nnz].double() - pk_ref).abs().max()) <= 1e-5 * float(pk_ref.abs().max()), what
    ctx = dict(st=st, plan=plan, wplan=w, R=p['R'], U0=p['U0'], V0=p['V0'], n=p['n'], S=S, r=r, D_model=e['D_model'], lr=p['lr'])
    bf16 = p['dtype'] is torch.bfloat16
    special = set(p['special'])
    users = [0, 1, 2, m - 1] + [u for u in range(3, 40) if int(p['R'][u, 0]) in special][:4]
    for u in users:
        (check_user_bf16 if bf16 else check_user_against_oracle)(ctx, u)
    for j in p['special']:
        g, _ = independent_item_gradient(j, p['R'], e['D_model'], plan, w.delta, st.U, r)
        (assert_step_bf16 if bf16 else assert_step)(st.V_nxt[j, :r].float().cpu().numpy()[None], p['V0'][j:j + 1].float().cpu().numpy(),
                                                    g[None], p['lr'], what=f'{what}: item {j}')


@pytest.mark.parametrize('r,dtype', [(128, torch.float32), (256, torch.bfloat16)], ids=['fp32_r128', 'bf16_r256'])
@pytest.mark.parametrize('n', [WMRB_LAST, WMRB_PAST], ids=['last_32bit', 'past_4gb'])
def test_wmrb_epoch_against_fp64_at_and_past_4gb(eng, monkeypatch, n, r, dtype):
    """Gaussian tables.  At 2^23 - 1 items: scores6 (the form the dyadic test pins the others to).  At 9M items (rows past byte
    2^32): TMF_SCORES6=1 cannot force scores6 (the numbers are checked first, then which form ran), scores6 and scores5 refuse
    the table, and scores3's general form answers."""
    from teamoflow_amd import _lib
    lib = _lib.load_library()
    bf = int(dtype is torch.bfloat16)
    row_bytes = _lib.padded_ld(r, dtype) * (2 if bf else 4)
    past = n * row_bytes > TWO32
    assert past == (n == WMRB_PAST) and (past or (n + 1) * row_bytes == TWO32)
    need(wmrb_need(n, r, dtype))
    p = wmrb_problem(n, r, dtype, dyadic=False, seed=n + r)
    e = wmrb_epoch(eng, monkeypatch, p, 'asked_s6' if past else 's6')
    check_wmrb_against_fp64(p, e, r, f'n={n} {dtype}')
    assert (e['wplan'].s6 is None) == past and e['wplan'].s5 is None
    assert eng.scores_form_of(e['plan'], e['wplan'], r, dtype) == (('scores3', False) if past else ('scores6', True))
    assert lib.tmf_wmrb_scores6_supported(r, bf, n) == (0 if past else 1)
    assert lib.tmf_wmrb_scores5_supported(r, bf, n) == (0 if past else 1)
    del e, p
    release(f'wmrb n={n} {dtype}')


def test_mse_epoch_with_more_than_2_31_user_elements(eng):
    """MSE epoch on 17M users x 128 fp32 (more than 2^31 elements of U), 100K items: sampled users - the first ones, those around
    element 2^31 and byte 2^32 of U, the last 10 - against oracle.sparse_ref.mse_epoch on their compact sub-problem."""
    from oracle import sparse_ref as SR
    m, n, r, lr = 17_000_000, 100_000, 128, 0.05
    assert m * r > TWO31
    need(3 * m * r * 4 + 6 * GB)
    g = torch.Generator(device=DEV).manual_seed(99)
    users = [0, 1, TWO32 // (4 * r) - 1, TWO32 // (4 * r), TWO31 // r - 1, TWO31 // r] + list(range(m - 10, m))
    u = torch.cat([torch.randint(0, m, (4_000_000,), generator=g, device=DEV), torch.tensor(users, device=DEV).repeat_interleave(8)])
    j = torch.randint(0, n, (u.numel(),), generator=g, device=DEV)
    key = torch.unique(u * n + j)
    idx = torch.stack([key // n, key % n], 1)
    val = torch.randint(1, 6, (key.numel(),), generator=g, device=DEV).float()
    U0 = torch.randn(m, r, generator=g, device=DEV) * 0.3
    V0 = torch.randn(n, r, generator=g, device=DEV) * 0.3
    plan = eng.InteractionPlan(idx, val, m, n)
    st = eng.TrainState(U0, V0, plan, r)
    U_probe = U0[torch.tensor(users, device=DEV)].double().cpu().numpy()
    del U0
    release()
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    eng.epoch_mse(st, eng.adam_constants(lr), loss)
    torch.cuda.synchronize()
    rp = plan.rowptr_u
    for q, uu in enumerate(users):
        b, e = int(rp[uu]), int(rp[uu + 1])
        cols = plan.col_u[b:e].long()
        items, inv = torch.unique(cols, return_inverse=True)
        Vc = V0[items].double().cpu().numpy()
        ic = np.stack([np.zeros(e - b, np.int64), inv.cpu().numpy()], 1)
        _, _, _, t = SR.mse_epoch(U_probe[q:q + 1], Vc, ic, plan.val_u[b:e].double().cpu().numpy(), lr)
        assert e > b
        assert_step(st.U_nxt[uu, :r].cpu().numpy()[None], U_probe[q:q + 1], t['gU'], lr, what=f'mse user {uu}')
    del st, plan
    release('mse 17M users')
