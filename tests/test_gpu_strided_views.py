"""The ranking entry points on operands that are VIEWS: row pitches other than the minimal one (lda != ldb), rows that skip, storage
offsets, and poison - NaN in one run, 2^60 in the next (k_absmax skips non-finite values, so a NaN read there would go unseen) - in
every column [r, ld), every skipped row and the guard rows around the tables.  The contract (include/tmf.h): A[u, :r] . B[:, :r]^T
is what gets ranked, whatever the pitches; outputs and workspaces are written inside their stated extents only.

Part A goes through the Python API (predict_topk in its four forms, predict_gemm, topk_stable, item_ranks, dcg_idcg), with
small-integer factors: every score is an integer below 2^12, so the fp32 MFMA, three bf16 planes, two fp16 planes and bf16 storage
are all exact, ties are plentiful and every comparison is torch.equal / np.array_equal against the fp64 oracle AND against the same
call on compact clones.  Every layout called a view is asserted to reach the kernel uncopied (_ops._operand keeps its pointer).

Part B calls the C ABI with ctypes: out_idx, out_val and a workspace of exactly the queried size sit inside a byte arena between
64 KiB bands of 0xA5 that must come back unchanged (the eight tmf_predict_topk_* and tmf_topk_stable_f32 with its radix workspace).
tmf_item_ranks_split's workspace is not covered here; its inputs are covered by Part A."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import sparse_ref
from test_gpu_item_ranks import edge_sets, int_tables, oracle_ranks

pytestmark = pytest.mark.gpu

M, N = 261, 1061   # ragged against 128- and 256-user and 128-item tiles
POISONS = (float('nan'), 2.0 ** 60)   # 2^60 is finite and bf16-exact
# r % 4 != 0 (MODE 0 tails) | % 4 == 0, % 8 != 0 | % 8 == 0, no chunk multiple | whole chunks, all four NCH classes
WIDTHS = [3, 30, 65, 130, 36, 100, 40, 200, 32, 128, 256]
FORMS = ['fp32', 'split', 'half2', 'bf16']
GUARD = 3


@pytest.fixture(scope='module')
def ops():
    from teamoflow_amd import _lib, _ops
    _lib.get()
    return _ops


def roundup(x, q):
    return (x + q - 1) // q * q


def embed(t, ld, guard_rows=GUARD, row_step=1, poison=float('nan')):
    """t [rows, r] inside a [2 * guard_rows + row_step * rows, ld] buffer of `poison`: row i of t is buffer row
    guard_rows + row_step * i, columns [0, r).  -> (view, buffer)."""
    rows, r = t.shape
    buffer = torch.full((2 * guard_rows + row_step * rows, ld), poison, dtype=t.dtype, device='cuda')
    view = buffer[guard_rows:guard_rows + row_step * rows:row_step, :r]
    view.copy_(t)
    return view, buffer


def unaligned(t, ld, poison):
    """t in columns [1, r + 1) of a poisoned buffer: rows that start 4 (bf16: 2) bytes off a 16-byte boundary."""
    view, buffer = embed(torch.cat([t[:, :1], t], 1), ld, poison=poison)
    buffer[:, 0] = poison
    return view[:, 1:]


def assert_view(ops, v, per16):
    """The host passes this tensor straight to the kernel: had it copied, the test would test nothing."""
    kept, rows, r, ld = ops._operand(v, per16)
    assert kept.data_ptr() == v.data_ptr() and ld == v.stride(0) and (rows, r) == tuple(v.shape)


def layouts(ops, U, V, per16, poison, which=('L1', 'L2', 'L3', 'L4')):
    """(name, A, B) of the compact device tables U [m, r], V [n, r] in every layout; the buffers live as long as the views."""
    r = U.shape[1]
    base = roundup(r, per16)
    lda, ldb = base + 3 * per16, base + 5 * per16
    for name in which:
        if name == 'L1':     # tight: the minimal pitch, the next row's data replaced by guard rows only at the ends
            A, B = embed(U, base, poison=poison)[0], embed(V, base, poison=poison)[0]
        elif name == 'L2':   # wide: lda != ldb
            A, B = embed(U, lda, poison=poison)[0], embed(V, ldb, poison=poison)[0]
        elif name == 'L3':   # skip: the rows in between are poison
            A, B = embed(U, lda, row_step=2, poison=poison)[0], embed(V, ldb, row_step=3, poison=poison)[0]
        else:                # L4, unaligned: one element into the row - the host must copy (and zero pad), the result is unchanged
            A, B = unaligned(U, base + per16, poison), unaligned(V, base + per16, poison)
            for t in (A, B):
                assert ops._operand(t, per16)[0].data_ptr() != t.data_ptr()
            yield name, A, B
            continue
        assert_view(ops, A, per16)
        assert_view(ops, B, per16)
        assert A.stride(0) >= r and B.stride(0) >= r and A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0
        yield name, A, B


def device_tables(Un, Vn, bf16):
    U, V = torch.as_tensor(Un).cuda(), torch.as_tensor(Vn).cuda()
    return (U.bfloat16(), V.bfloat16(), 8) if bf16 else (U, V, 4)


def exclusion_mask(m, n, ks, seed):
    """A random 8 % of the pairs; for every k of ks one user with all but k - 2 items excluded (the -1 / -inf slots)."""
    rng = np.random.default_rng(seed)
    mask = rng.random((m, n)) < 0.08
    for u, k in enumerate(ks):
        if u < m and k >= 2:
            mask[u] = True
            mask[u, rng.choice(n, k - 2, replace=False)] = False
    return mask


class TopkOracle:
    """fp64 U @ V.T ranked by oracle.sparse_ref.topk_stable, once per (exclusion, clamp); any k slices it."""

    def __init__(self, Un, Vn, mask, kmax):
        self.S = np.asarray(Un, np.float64) @ np.asarray(Vn, np.float64).T
        self.mask, self.kmax, self.memo = mask, kmax, {}

    def lists(self, k, excl, clamp):
        if (excl, clamp) not in self.memo:
            S = np.where(self.S > 0, self.S, 0.0) if clamp else self.S.copy()
            if excl:
                S[self.mask] = -np.inf   # every eligible score is a finite integer: the excluded ones sort behind them all
            ids = sparse_ref.topk_stable(S, self.kmax).astype(np.int64)
            vals = np.take_along_axis(S, ids, 1)
            ids[np.isneginf(vals)] = -1
            self.memo[excl, clamp] = (torch.as_tensor(vals.astype(np.float32)).cuda(), torch.as_tensor(ids.astype(np.int32)).cuda())
        vals, ids = self.memo[excl, clamp]
        return vals[:, :k].contiguous(), ids[:, :k].contiguous()


def check_predict_topk(ops, Un, Vn, form, ks, which, seed, clamps=(False, True), special=None):
    """Every (layout, poison, k, exclusion, clamp) of one (form, tables): oracle == compact call == call on the views."""
    bf16 = form == 'bf16'
    arithmetic = 'auto' if bf16 else form
    U, V, per16 = device_tables(Un, Vn, bf16)
    m, n = U.shape[0], V.shape[0]
    mask = exclusion_mask(m, n, ks, seed)
    ex = ops.build_exclusion(torch.as_tensor(mask).cuda(), m, n)
    orc = TopkOracle(Un, Vn, mask, max(ks))
    fewer = 0
    for k in ks:
        for excl in (False, True):
            for clamp in clamps:
                kw = dict(clamp_negatives=clamp, return_values=True, arithmetic=arithmetic, exclude=ex if excl else None)
                want_v, want_i = orc.lists(k, excl, clamp)
                fewer += int((want_i < 0).sum())
                ref_v, ref_i = ops.predict_topk(U.clone(), V.clone(), k, **kw)
                assert torch.equal(ref_i, want_i) and torch.equal(ref_v, want_v), (form, k, excl, clamp, 'compact')
                for poison in POISONS:
                    for name, A, B in (special(poison) if special else layouts(ops, U, V, per16, poison, which)):
                        got_v, got_i = ops.predict_topk(A, B, k, **kw)
                        what = (form, name, poison, k, excl, clamp)
                        assert torch.equal(got_i, want_i), what
                        assert torch.equal(got_v, want_v), what
                        assert torch.equal(got_i, ref_i) and torch.equal(got_v, ref_v), what
    assert fewer > 0   # the -1 / -inf slots occurred


def topk_ks(form):
    return (10, 20, 40) if form in ('fp32', 'split') else (10, 20, 32)   # fp32 / split: the pending, insertion and merge candidate paths


# ------------------------------------------------------------------ Part A: inputs, through the Python API
@pytest.mark.parametrize('r', WIDTHS)
@pytest.mark.parametrize('form', FORMS)
def test_predict_topk_on_views(ops, form, r):
    Un, Vn = int_tables(M, N, r, seed=r + 11)
    check_predict_topk(ops, Un, Vn, form, topk_ks(form), ('L1', 'L2', 'L3', 'L4'), seed=r)


@pytest.mark.parametrize('r', [30, 128])
@pytest.mark.parametrize('form', ['split', 'half2'])
def test_predict_topk_wide_views_with_warm_up_pass(ops, form, r):
    """256 item tiles and more: the plane kernels' warm-up pass reads the planes too."""
    Un, Vn = int_tables(M, 33001, r, seed=r + 5)
    check_predict_topk(ops, Un, Vn, form, (10,), ('L2',), seed=r, clamps=(False,))


def far_ldb(n, elem_size, per16):
    """The smallest aligned pitch with (n + 512) * ldb * elem_size >= 2^32: 32-bit byte offsets into the item table no longer do."""
    ldb = roundup(-(-2 ** 32 // ((n + 512) * elem_size)), per16)
    assert (n + 512) * ldb * elem_size >= 2 ** 32 > (n + 512) * (ldb - per16) * elem_size
    return ldb


@pytest.mark.parametrize('r', [36, 128])
@pytest.mark.parametrize('form', ['fp32', 'split', 'bf16', 'ranks_fp32'])
def test_far_pitch_takes_the_kernels_off_32_bit_offsets(ops, form, r):
    """L5: 129 item rows ~6.7 MB apart (under 1 GB of backing store) - the fp32 kernels go to MODE 1 (r % 4 == 0), the bf16 kernel
    off MODE 2, without a 4 GB table."""
    n = 129
    Un, Vn = int_tables(M, n, r, seed=r + 3)
    bf16 = form == 'bf16'
    U, V, per16 = device_tables(Un, Vn, bf16)
    ldb = far_ldb(n, 2 if bf16 else 4, per16)
    lda = roundup(r, per16) + 3 * per16

    def special(poison):
        A, B = embed(U, lda, poison=poison)[0], embed(V, ldb, guard_rows=1, poison=poison)[0]
        assert_view(ops, A, per16)
        assert_view(ops, B, per16)
        assert B.stride(0) == ldb
        yield 'L5', A, B

    if form != 'ranks_fp32':
        check_predict_topk(ops, Un, Vn, form, topk_ks(form), None, seed=r, special=special)
        return
    rng = np.random.default_rng(r)
    pos = rng.random((M, n)) < 0.1
    pos[5] = True                                    # every item: seven virtual rows
    pos[7:12] = False                                # no positives
    excl = (rng.random((M, n)) < 0.08) & ~pos
    for ex in (None, excl):
        want = oracle_ranks(Un, Vn, pos, np.zeros_like(excl) if ex is None else ex)
        ref = run_ranks(ops, U.clone(), V.clone(), pos, ex, 'fp32')
        assert np.array_equal(ref, want)
        for poison in POISONS:
            for _, A, B in special(poison):
                assert np.array_equal(run_ranks(ops, A, B, pos, ex, 'fp32'), want), (poison, ex is not None)


@pytest.mark.parametrize('r', WIDTHS)
def test_predict_gemm_on_views_into_a_view(ops, r):
    """A, B views; C a [m, n] view with ldc = n + 7 inside a sentinel-filled buffer: C is the fp64 product exactly and every byte
    of the buffer outside it is unchanged."""
    Un, Vn = int_tables(M, N, r, seed=r + 17)
    U, V, per16 = device_tables(Un, Vn, False)
    want = torch.as_tensor((Un.astype(np.float64) @ Vn.astype(np.float64).T).astype(np.float32)).cuda()
    assert torch.equal(ops.predict_gemm(U.clone(), V.clone()), want)
    inside = torch.zeros(M + 2 * GUARD, N + 7, dtype=torch.bool, device='cuda')
    inside[GUARD:GUARD + M, :N] = True
    for poison in POISONS:
        for name, A, B in layouts(ops, U, V, per16, poison):
            out, buffer = embed(torch.full((M, N), -5.0), N + 7, poison=-12345.0)
            before = buffer.clone()
            got = ops.predict_gemm(A, B, out=out)
            assert got.data_ptr() == out.data_ptr() and out.stride(0) == N + 7
            assert torch.equal(out, want), (name, poison)
            assert torch.equal(buffer.view(torch.int32)[~inside], before.view(torch.int32)[~inside]), (name, poison)


def test_predict_gemm_rejects_an_out_it_cannot_write(ops):
    U, V = torch.ones(5, 8, device='cuda'), torch.ones(9, 8, device='cuda')
    ok = torch.empty(5, 9, device='cuda')
    assert ops.predict_gemm(U, V, out=ok) is ok
    assert ops.predict_gemm(U, V, out=torch.empty(5, 16, device='cuda')[:, :9]).shape == (5, 9)
    bad = [torch.empty(5, 9),                                       # not on the device
           torch.empty(5, 9, device='cuda', dtype=torch.float64),   # not float32
           torch.empty(5, 9, device='cuda', dtype=torch.bfloat16),
           torch.empty(9, 5, device='cuda'),                        # not [m, n]
           torch.empty(5, 10, device='cuda'),
           torch.empty(45, device='cuda'),
           torch.empty(9, 5, device='cuda').T,                      # column stride != 1
           torch.empty(5, 18, device='cuda')[:, ::2],
           torch.empty(9, device='cuda').expand(5, 9),              # row stride 0 < n: the rows overlap
           torch.empty(64, device='cuda').as_strided((5, 9), (8, 1))]
    for out in bad:
        with pytest.raises(ValueError, match='out'):
            ops.predict_gemm(U, V, out=out)
    with pytest.raises(ValueError, match='out'):
        ops.predict_gemm(U, V, out=np.empty((5, 9), np.float32))


@pytest.mark.parametrize('cols,k', [(7, 7), (129, 10), (1000, 64), (1000, 300), (16385, 65), (16385, 300)])
def test_topk_stable_on_views(ops, cols, k):
    """x a [37, cols] view with ldx in {cols + 1, cols + 4, 2 * cols} (rows 16-byte aligned or not); the last two shapes take the
    radix-sort workspace path.  exclude=..., overwrite=True works on the view itself: outside it the buffer stays bit-identical,
    inside the only changes are the clamp and -inf on excluded entries."""
    rows = 37
    rng = np.random.default_rng(cols + k)
    xn = rng.integers(-40, 41, (rows, cols)).astype(np.float32)   # ties, zeros and negatives
    mask = exclusion_mask(rows, cols, (k,), seed=cols)
    ex = ops.build_exclusion(torch.as_tensor(mask).cuda(), rows, cols)
    x = torch.as_tensor(xn).cuda()
    maskd = torch.as_tensor(mask).cuda()
    want = {}
    for clamp in (False, True):
        xc = np.where(xn > 0, xn, np.float32(0)) if clamp else xn
        for excl in (False, True):
            xe = np.where(mask, -np.inf, xc).astype(np.float32) if excl else xc
            ids = sparse_ref.topk_stable(xe.astype(np.float64), k).astype(np.int64)
            vals = np.take_along_axis(xe, ids, 1)
            ids[np.isneginf(vals)] = -1
            want[clamp, excl] = (torch.as_tensor(vals).cuda(), torch.as_tensor(ids.astype(np.int32)).cuda(), torch.as_tensor(xe).cuda())
    assert int((want[False, True][1] < 0).sum()) >= 2   # the row with k - 2 eligible entries
    for clamp in (False, True):
        for excl in (False, True):
            want_v, want_i, want_x = want[clamp, excl]
            kw = dict(clamp_negatives=clamp, return_values=True)
            if excl:
                kw.update(exclude=ex, overwrite=True)
            ref_v, ref_i = ops.topk_stable(x.clone(), k, **kw)
            assert torch.equal(ref_i, want_i) and torch.equal(ref_v, want_v), (clamp, excl, 'compact')
            for ldx in (cols + 1, cols + 4, 2 * cols):
                for poison in POISONS:
                    view, buffer = embed(x, ldx, poison=poison)
                    before = buffer.clone()
                    got_v, got_i = ops.topk_stable(view, k, **kw)
                    what = (clamp, excl, ldx, poison)
                    assert torch.equal(got_i, want_i) and torch.equal(got_v, want_v), what
                    inside = torch.zeros(buffer.shape, dtype=torch.bool, device='cuda')
                    inside[GUARD:GUARD + rows, :cols] = True
                    assert torch.equal(buffer.view(torch.int32)[~inside], before.view(torch.int32)[~inside]), what
                    if excl:   # tmf_topk_stable_exclude_f32 worked on the view: the clamp in place, -inf on the excluded entries
                        assert torch.equal(view, want_x), what
                        assert bool(torch.isneginf(view[maskd]).all())
                    else:      # without exclude x is only read
                        assert torch.equal(view, x), what


def run_ranks(ops, U, V, pos, excl, arithmetic):
    dense = lambda mask: torch.as_tensor(mask.astype(np.float32))   # noqa: E731
    return ops.item_ranks(U, V, dense(pos), exclude=None if excl is None else dense(excl), arithmetic=arithmetic).cpu().numpy()


@pytest.mark.parametrize('r', WIDTHS)
@pytest.mark.parametrize('form', FORMS)
def test_item_ranks_on_views(ops, form, r):
    """'fp32' / 'split': the fused rank kernels and tmf_pair_scores_*; 'half2': score blocks of tmf_predict_gemm_f32 on the views
    and tmf_rank_count_rows_f32; bf16 views (the host casts their rows to fp32 per block)."""
    Un, Vn = int_tables(M, N, r, seed=r + 7)
    pos, excl = edge_sets(M, N, seed=r)
    bf16 = form == 'bf16'
    U, V, per16 = device_tables(Un, Vn, bf16)
    arithmetic = 'auto' if bf16 else form
    for ex in (None, excl):
        want = oracle_ranks(Un, Vn, pos, np.zeros_like(excl) if ex is None else ex)
        ref = run_ranks(ops, U.clone(), V.clone(), pos, ex, arithmetic)
        assert np.array_equal(ref, want), (form, ex is not None, 'compact')
        for poison in POISONS:
            for name, A, B in layouts(ops, U, V, per16, poison, ('L1', 'L2', 'L3')):
                got = run_ranks(ops, A, B, pos, ex, arithmetic)
                assert np.array_equal(got, want), (form, name, poison, ex is not None)


@pytest.mark.parametrize('k', [1, 10, 40])
def test_dcg_of_a_strided_list(ops, k):
    """top a [m, k] view of an int32 buffer with ldt = k + 5 whose other columns (and guard rows) hold 0x7fffffff and -7."""
    rng = np.random.default_rng(1000 + k)   # not the stream of the exclusion mask: graded items must stay eligible
    Un, Vn = int_tables(M, N, 30, seed=k)
    graded = (rng.random((M, N)) < 0.05) * rng.integers(1, 5, (M, N))
    table = ops.graded_csr(torch.as_tensor(graded.astype(np.float32)).cuda(), M, N)
    mask = exclusion_mask(M, N, (k,), seed=k)   # a user with -1 slots
    top = ops.predict_topk(torch.as_tensor(Un).cuda(), torch.as_tensor(Vn).cuda(), k, exclude=torch.as_tensor(mask).cuda())
    assert top.dtype == torch.int32 and top.is_contiguous() and (k < 2 or int((top < 0).sum()) == 2)
    want, want_idcg = ops.dcg_idcg(table, top, k)
    assert float(want.max()) > 0
    view, buffer = embed(top, k + 5, poison=0x7fffffff)
    buffer[:, 1::2] = -7
    view.copy_(top)
    before = buffer.clone()
    pads = buffer[:, k:]
    assert view.stride(0) == k + 5 and int((pads == -7).sum()) > 0 and int((pads == 0x7fffffff).sum()) > 0
    got, got_idcg = ops.dcg_idcg(table, view, k)
    assert torch.equal(got, want) and torch.equal(got_idcg, want_idcg)
    assert torch.equal(buffer, before)


# ------------------------------------------------------------------ Part B: outputs and workspaces, through the C ABI
BAND = 64 << 10


class Arena:
    """Regions of exact byte sizes inside one uint8 buffer of 0xA5, each starting 16-byte aligned with at least 64 KiB of 0xA5 on
    both sides."""

    def __init__(self, sizes):
        self.spans, at = [], BAND
        for size in sizes:
            self.spans.append((at, int(size)))
            at = roundup(at + int(size), 16) + BAND
        self.buf = torch.full((at,), 0xA5, dtype=torch.uint8, device='cuda')
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self, i):
        return ctypes.c_void_p(self.buf.data_ptr() + self.spans[i][0])

    def region(self, i, dtype, shape):
        at, size = self.spans[i]
        return self.buf[at:at + size].view(dtype).view(shape)

    def assert_bands_unchanged(self, what):
        rest = self.buf.clone()
        for at, size in self.spans:
            rest[at:at + size] = 0xA5
        assert bool((rest == 0xA5).all()), what


ENTRY_POINTS = [(form, excl) for form in ('f32', 'bf16', 'split', 'half2') for excl in (False, True)]


@pytest.mark.parametrize('m,n,r,k', [(261, 1061, 30, 10), (261, 1061, 128, 32), (1, 129, 256, 1), (129, 128, 65, 20)])
@pytest.mark.parametrize('form,excl', ENTRY_POINTS)
def test_predict_topk_writes_inside_its_extents(ops, form, excl, m, n, r, k):
    from teamoflow_amd import _lib
    lib = _lib.get()
    Un, Vn = int_tables(m, n, r, seed=m + r)
    U, V, per16 = device_tables(Un, Vn, form == 'bf16')
    A, _, _, lda = ops._operand(embed(U, roundup(r, per16) + per16, poison=2.0 ** 60)[0], per16)
    B, _, _, ldb = ops._operand(embed(V, roundup(r, per16) + 2 * per16, poison=2.0 ** 60)[0], per16)
    mask = exclusion_mask(m, n, (0, k) if m > 1 else (), seed=k)   # m > 1: user 1 has k - 2 eligible items
    ex = ops.build_exclusion(torch.as_tensor(mask).cuda(), m, n)
    want_v, want_i = TopkOracle(Un, Vn, mask, k).lists(k, excl, False)
    name = {'f32': 'tmf_predict_topk_%sf32', 'bf16': 'tmf_predict_topk_%sbf16', 'split': 'tmf_predict_topk_split_%sf32',
            'half2': 'tmf_predict_topk_half2_%sf32'}[form] % ('exclude_' if excl else '')
    ws_bytes = {'split': lib.tmf_predict_topk_split_workspace_bytes, 'half2': lib.tmf_predict_topk_half2_workspace_bytes}
    sizes = [4 * m * k, 4 * m * k]
    if form in ws_bytes:
        sizes.append(ws_bytes[form](n, r))
        assert sizes[2] > 0
    arena = Arena(sizes)
    args = [_lib.ptr(A), _lib.ptr(B), m, n, r, lda, ldb, k, 0]
    if excl:
        args.append(ctypes.byref(ex.struct(m)))
    args += [arena.ptr(0), arena.ptr(1)]
    if form in ws_bytes:
        args += [arena.ptr(2), sizes[2]]
    _lib.check(getattr(lib, name)(*args, _lib.stream_ptr()), lib)
    torch.cuda.synchronize()
    arena.assert_bands_unchanged(name)
    assert torch.equal(arena.region(0, torch.int32, (m, k)), want_i), name
    assert torch.equal(arena.region(1, torch.float32, (m, k)), want_v), name


def test_topk_stable_radix_path_writes_inside_its_extents(ops):
    from teamoflow_amd import _lib
    lib = _lib.get()
    rows, cols, k = 37, 16385, 300
    xn = np.random.default_rng(1).integers(-40, 41, (rows, cols)).astype(np.float32)
    x = torch.as_tensor(xn).cuda()
    need = lib.tmf_topk_workspace_bytes(rows, cols, k)
    assert need > 0   # the segmented radix sort
    arena = Arena([4 * rows * k, 4 * rows * k, need])
    _lib.check(lib.tmf_topk_stable_f32(_lib.ptr(x), rows, cols, cols, k, 0, arena.ptr(0), arena.ptr(1), arena.ptr(2), need,
                                       _lib.stream_ptr()), lib)
    torch.cuda.synchronize()
    arena.assert_bands_unchanged('tmf_topk_stable_f32')
    ids = sparse_ref.topk_stable(xn.astype(np.float64), k)
    assert np.array_equal(arena.region(0, torch.int32, (rows, k)).cpu().numpy(), ids)
    assert np.array_equal(arena.region(1, torch.float32, (rows, k)).cpu().numpy(), np.take_along_axis(xn, ids, 1))
    assert torch.equal(x, torch.as_tensor(xn).cuda())


def test_rank_count_rows_on_a_strided_score_block(ops):
    """tmf_rank_count_rows_f32 takes ldx too, and the host only ever hands it compact blocks: here X is a [m, n] view with
    ldx in {n + 1, n + 4, 2 n} inside a poisoned buffer.  With an exclusion the excluded entries of X become NaN in place -
    nothing else inside the view changes and nothing at all outside it."""
    from teamoflow_amd import _lib
    lib = _lib.get()
    Un, Vn = int_tables(M, N, 30, seed=41)
    pos, excl = edge_sets(M, N, seed=41)
    S = torch.as_tensor((Un.astype(np.float64) @ Vn.astype(np.float64).T).astype(np.float32)).cuda()
    pairs = ops.positive_pairs(torch.as_tensor(pos.astype(np.float32)).cuda(), M, N)
    vu, vb, vc = ops.virtual_rows(pairs.rowptr)
    rows = ops._rank_rows(vu, vb, vc)
    for mask in (None, excl):
        want = oracle_ranks(Un, Vn, pos, np.zeros_like(excl) if mask is None else mask)
        ex = None if mask is None else ops.build_exclusion(torch.as_tensor(mask).cuda(), M, N)
        maskd = torch.as_tensor(np.zeros_like(excl) if mask is None else mask).cuda()
        for ldx in (N + 1, N + 4, 2 * N):
            for poison in POISONS:
                X, buffer = embed(S, ldx, poison=poison)
                before = buffer.clone()
                ranks = torch.zeros(want.size, dtype=torch.int32, device='cuda')
                _lib.check(lib.tmf_rank_count_rows_f32(_lib.ptr(X), M, N, ldx, 0, ctypes.byref(rows), _lib.ptr(pairs.cols),
                                                       None if ex is None else ctypes.byref(ex.struct(M)), _lib.ptr(ranks),
                                                       _lib.stream_ptr()), lib)
                torch.cuda.synchronize()
                what = (mask is not None, ldx, poison)
                assert np.array_equal(ranks.cpu().numpy(), want), what
                inside = torch.zeros(buffer.shape, dtype=torch.bool, device='cuda')
                inside[GUARD:GUARD + M, :N] = True
                assert torch.equal(buffer.view(torch.int32)[~inside], before.view(torch.int32)[~inside]), what
                assert bool(torch.isnan(X[maskd]).all()) and torch.equal(X[~maskd], S[~maskd]), what
