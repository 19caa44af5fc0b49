"""Tensor-level wrappers over the predict / ranking entry points of libtmf.so."""
import ctypes
import os

import numpy as np
import torch

from . import _lib


def _cuda(t, dtype=None):
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    _lib.get()  # raises EngineUnavailable without a GPU: there is no CPU path
    if not t.is_cuda:
        t = t.cuda()
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t


def _operand(t, per16=4):
    """[rows, r] tensor -> (tensor kept alive, rows, r, ld) with 16-byte aligned rows: ld a multiple of per16, the elements per
    16 bytes (4: the tensor as fp32, 8: a bf16 tensor)."""
    dtype = torch.float32 if per16 == 4 else torch.bfloat16
    t = _cuda(t, dtype).detach()
    rows, r = t.shape
    ok = t.stride(1) == 1 and t.stride(0) % per16 == 0 and t.stride(0) >= r and t.data_ptr() % 16 == 0
    if not ok:
        ld = (r + per16 - 1) // per16 * per16
        p = torch.zeros(rows, ld, dtype=dtype, device=t.device)
        p[:, :r] = t
        t = p[:, :r]
    return t, rows, r, t.stride(0)


def predict_gemm(user_embedding, item_embedding, out=None):
    """user_embedding [m, r] @ item_embedding [n, r]^T -> [m, n] fp32 (exact-fp32 MFMA)."""
    lib = _lib.get()
    A, m, r, lda = _operand(user_embedding)
    B, n, rb, ldb = _operand(item_embedding)
    if r != rb:
        raise ValueError(f'embedding widths differ: {r} vs {rb}')
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=A.device)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (m, n)
              and out.stride(1) == 1 and out.stride(0) >= n):
        # out.stride(0) is the ldc the kernel writes with: anything else would be written past its rows or as another type
        raise ValueError(f'out must be a CUDA float32 [{m}, {n}] tensor with unit column stride and a row stride >= {n}, got '
                         + (f'{out.dtype} {tuple(out.shape)} on {out.device}, strides {tuple(out.stride())}' if torch.is_tensor(out)
                            else type(out).__name__))
    _lib.check(lib.tmf_predict_gemm_f32(A, B, out, m, n, r, lda, ldb, out.stride(0),
                                        _lib.stream_ptr()), lib)
    return out


class Exclusion:
    """Already-seen (user, item) pairs as a CSR on the device: row u's excluded item ids are cols[rowptr[u]:rowptr[u + 1]],
    ascending and distinct (build_exclusion).  ``user_base`` / ``item_base`` select a block of users / a window of the catalog
    without copying: row 0 of the view is user ``user_base``, and item id ``item_base`` is column 0 of the table being ranked."""

    def __init__(self, rowptr, cols, n_users, n_items, user_base=0, item_base=0):
        self.rowptr, self.cols = rowptr, cols
        self.n_users, self.n_items = int(n_users), int(n_items)
        self.user_base, self.item_base = int(user_base), int(item_base)

    def shifted(self, users=0, items=0):
        """The view whose row 0 is user ``user_base + users`` and whose column 0 is item ``item_base + items``."""
        return Exclusion(self.rowptr, self.cols, self.n_users, self.n_items, self.user_base + int(users), self.item_base + int(items))

    def struct(self, rows):
        """tmf_exclusion for `rows` users from this view's row 0."""
        if self.user_base < 0 or self.user_base + rows > self.n_users:
            raise IndexError(f'exclusion covers users [0, {self.n_users}), asked for [{self.user_base}, {self.user_base + rows})')
        return _lib.Exclusion(self.rowptr.data_ptr() + 8 * self.user_base, self.cols.data_ptr(), self.item_base)


def _decode_table(A, what, device=None, shape=None, keep=None):
    """(u, i, val, stated shape) of a table of (user, item) entries: a SparseInteractions-like object (indices / values, optional
    dense_shape: the stated shape, else None) or a dense [rows, cols] table (torch or NumPy; its non-zeros; ``shape``: what it must
    be), moved to ``device`` when one is given.  keep: 'nonzero' or 'positive' - only the ids of the entries with such a value are
    wanted (val is None); None: every entry with its value."""
    if not torch.is_tensor(A) and hasattr(A, 'indices') and hasattr(A, 'values'):
        idx, val = torch.as_tensor(A.indices), torch.as_tensor(A.values)
        if device is not None:
            idx, val = idx.to(device), val.to(device)
        idx, val = idx.to(torch.int64).reshape(-1, 2), val.reshape(-1)
        # column first, mask second: masked ROW selection of a [nnz, 2] tensor is unreliable beyond ~6e7 rows on this
        # PyTorch-ROCm build (tools/torch_row_index_probe.py)
        u, i = idx[:, 0], idx[:, 1]
        if keep is not None:
            mask = val > 0 if keep == 'positive' else val != 0
            u, i, val = u[mask], i[mask], None
        stated = getattr(A, 'dense_shape', None)
        return u, i, val, None if stated is None else (int(stated[0]), int(stated[1]))
    D = A if torch.is_tensor(A) else torch.as_tensor(np.asarray(A))
    if device is not None:
        D = D.to(device)
    if D.dim() != 2 or (shape is not None and tuple(D.shape) != shape):
        raise ValueError(f'a dense table of {what} must be {"2-D" if shape is None else list(shape)}, got shape {tuple(D.shape)}')
    nz = torch.nonzero(D > 0 if keep == 'positive' else D)   # the non-zeros of D itself: no [rows, cols] mask for them
    u, i = nz[:, 0], nz[:, 1]
    return u, i, D[u, i] if keep is None else None, None


def _check_ids(u, i, n_users, n_items, what):
    if u.numel():
        if int(u.min()) < 0 or int(u.max()) >= n_users:
            raise IndexError(f'{what} user id out of range [0, {n_users})')
        if int(i.min()) < 0 or int(i.max()) >= n_items:
            raise IndexError(f'{what} item id out of range [0, {n_items})')


def _pairs_csr(u, i, n_users, n_items):
    """Exclusion (CSR: rows sorted and de-duplicated) of (user, item) pairs whose ids are in range."""
    dev = u.device
    keys = torch.unique(u * n_items + i)   # sorted and distinct: row-major (user, item) order
    rows = torch.div(keys, n_items, rounding_mode='floor') if n_items else keys
    rowptr = torch.zeros(n_users + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(rows, minlength=n_users), 0, out=rowptr[1:])
    cols = (keys - rows * n_items).to(torch.int32)
    if cols.numel() == 0:
        cols = torch.zeros(1, dtype=torch.int32, device=dev)   # a valid pointer for the kernels; rowptr says there is nothing
    return Exclusion(rowptr, cols, n_users, n_items)


def build_exclusion(exclude, n_users, n_items, device=None):
    """CSR of the pairs to leave out of a ranking.  ``exclude``: an Exclusion (returned as it is), SparseInteractions or an object
    with indices / values / dense_shape (every stored entry with a value != 0 is a pair), or a dense [rows, cols] table (every
    non-zero is a pair).  Duplicates are allowed; each row is sorted and de-duplicated.  A user id outside [0, n_users) or an
    item id outside [0, n_items) raises IndexError.  Built with torch sort / bincount / cumsum on ``device`` (default: where the
    input is)."""
    if isinstance(exclude, Exclusion):   # a view: its ids outside [item_base, item_base + n_items) are ignored by the kernels
        if exclude.user_base < 0 or exclude.user_base + n_users > exclude.n_users:
            raise IndexError(f'exclusion covers users [0, {exclude.n_users}), asked for [{exclude.user_base}, '
                             f'{exclude.user_base + n_users})')
        return exclude
    n_users, n_items = int(n_users), int(n_items)
    u, i, _, _ = _decode_table(exclude, 'exclusions', device, keep='nonzero')
    _check_ids(u, i, n_users, n_items, 'excluded')
    return _pairs_csr(u, i, n_users, n_items)


def _exclusion_on(ex, device):
    if ex.rowptr.device != device:
        ex = Exclusion(ex.rowptr.to(device), ex.cols.to(device), ex.n_users, ex.n_items, ex.user_base, ex.item_base)
    return ex


def merge_lists(vals, ids, k):
    """The k best of per-window lists laid side by side in catalog order (each sorted value desc, index asc; -1 / -inf fill entries
    at their ends): a stable sort by value keeps equal values in ascending item order, and the fill entries go behind every item."""
    v, pos = torch.sort(vals, dim=1, descending=True, stable=True)
    i = torch.gather(ids, 1, pos)
    order = torch.argsort((i < 0).to(torch.int8), dim=1, stable=True)
    return torch.gather(v, 1, order)[:, :k], torch.gather(i, 1, order)[:, :k]


def merge_windows(vals, ids, k, fill, return_values=True):
    """(values, ids) of the k best of per-window top lists laid side by side in catalog order, so that equal values keep ascending
    item order.  fill: the lists may hold -1 / -inf fill entries (rankings with an exclusion) -> merge_lists; without them one
    stable top-k over the candidates (the window values carry their clamp already), its values only when asked for."""
    if fill:
        return merge_lists(vals, ids, k)
    out = topk_stable(vals, k, return_values=return_values)
    v, pos = out if return_values else (None, out)
    return v, torch.gather(ids, 1, pos.long())


FUSED_MAX_K, FUSED_MAX_K_BF16, FUSED_MAX_R, FUSED_MAX_R_BF16 = 64, 32, 256, 256
SPLIT_MIN_SCORES = 1 << 26   # arithmetic='auto' takes the three-plane bf16 split from this many scores (m * n) on: below, the pass that
                             # splits the item table and its workspace are not worth it and the fp32 MFMA kernel answers
SORT_MAX_ELEMS = 1 << 29   # elements ranked per call of the wide-row path (2 GB of keys + 2 GB of ids, twice)


def fused_topk_supported(user_embedding, item_embedding, k):
    """Whether predict_topk ranks these tables without materialising scores: k <= 64, width <= 256 (bf16 tables beyond the bf16 kernel's
    k <= 32 go through the fp32 fused kernel on exact fp32 copies: predict_topk)."""
    bf16 = user_embedding.dtype == torch.bfloat16 and item_embedding.dtype == torch.bfloat16
    return k <= FUSED_MAX_K and user_embedding.shape[1] <= (FUSED_MAX_R_BF16 if bf16 else FUSED_MAX_R)


BF16_UPCAST_WINDOWS = 8       # item windows of the same path when the fp32 copy of the whole item table does not fit
BF16_UPCAST_USERS = 1 << 18   # users per call when bf16 tables are ranked through the fp32 kernel (bounds the fp32 copy of their rows)


PREDICT_ARITHMETIC = os.environ.get('TMF_PREDICT_ARITHMETIC', 'auto')   # 'auto' | 'fp32' | 'split' | 'half2'


SPLIT_MAX_K = 40    # two 4-wave workgroups' lists fit a CU's LDS beside their pending buffers up to k = 40 (tmf_predict_split.hip)
SPLIT_MAX_R = 256   # the three-plane kernel: 96 A registers per lane at r = 128, 192 at r = 256 (eight waves per workgroup, two per SIMD)


def split_topk_supported(r, k):
    return 1 <= r <= SPLIT_MAX_R and 1 <= k <= SPLIT_MAX_K


def half2_topk_supported(r, k):
    return 1 <= r <= 256 and 1 <= k <= 32


HALF2_MAX_ROW_RANGE = 2.0 ** 12   # largest / smallest item-row magnitude up to which the opt-in two-plane fp16 kernel keeps 22 bits


def half2_range_ok(item_rows):
    """The fp16 planes of the item table share ONE power-of-two scale: rows whose largest magnitude is within 2^12 of the
    table's keep 22 bits of their dominant factors (the second plane stays in fp16's normal range); beyond that the three
    bf16 planes ('split': no range limit) are the safe choice.  One small reduction and a host read."""
    row_max = item_rows.abs().amax(dim=1)
    top = row_max.max()
    low = torch.where(row_max > 0, row_max, top).min()
    top, low = float(top), float(low)
    return top == 0.0 or (top < float('inf') and low > 0 and top / low <= HALF2_MAX_ROW_RANGE)


def _upcast_table(B):
    """Exact fp32 copy of a bf16 item table (twice its size; torch.OutOfMemoryError when it does not fit)."""
    return B.float()


def predict_topk(user_embedding, item_embedding, k, clamp_negatives=False, return_values=False, arithmetic=None, exclude=None):
    """Top-k item ids (int32) of user_embedding @ item_embedding^T per user, fused (no [m, n] matrix).
    fp32 tables: 'fp32' = fp32 MFMA (k <= 64, width <= 256, bit-equal to an fmaf chain); 'split' = the bf16 matrix cores with ALL
    24 significand bits of every factor (three exact bf16 planes per factor, six plane products each exact in the fp32
    accumulator; ~1.9x the rate of the fp32 kernel, errors against fp64 at or below its; width <= 256 - 1.55x the fp32 kernel at 256: 171 against 110 TF -, k <= 40).
    'auto' (the default) takes 'split' where it applies and the job has SPLIT_MIN_SCORES scores or more, else 'fp32' - both keep
    the reference's fp32 operands whole (tf.matmul on fp32, matrix_factorization.py:236-248, 424-438).
    'half2' is an OPT-IN approximation, never chosen by 'auto': two fp16 planes under power-of-two scales = 22 bits of every
    factor, three products, ~2.9x; one scale for the whole item table, so check half2_range_ok(item_embedding) first.
    Scores BEYOND the fp32 range: the fp32 kernel returns +-inf like tf.matmul; the plane kernels may form +inf - inf = NaN between
    plane products of opposite sign, and a NaN score is never ranked (the ids returned are those of the finite scores).
    bf16 tables (both operands): bf16 MFMA with fp32 accumulation, k <= 32, width <= 256; 32 < k <= 64: the fp32 kernel on exact fp32 copies.
    See topk_stable(predict_gemm(...)) for the general case.
    exclude: pairs to leave out (build_exclusion: an Exclusion, SparseInteractions or a dense table, rows = these users, columns =
    these items unless an Exclusion view says otherwise); a user with fewer than k eligible items gets id -1 / value -inf in the
    trailing slots.  None runs the calls without exclusion."""
    lib = _lib.get()
    arithmetic = arithmetic or PREDICT_ARITHMETIC
    if arithmetic not in ('auto', 'fp32', 'split', 'half2'):
        raise ValueError(f"arithmetic={arithmetic!r}: expected 'auto', 'fp32', 'split' or 'half2'")
    bf16 = torch.is_tensor(user_embedding) and torch.is_tensor(item_embedding) and \
        user_embedding.dtype == torch.bfloat16 and item_embedding.dtype == torch.bfloat16
    A, m, r, lda = _operand(user_embedding, 8 if bf16 else 4)
    B, n, rb, ldb = _operand(item_embedding, 8 if bf16 else 4)
    if r != rb:
        raise ValueError(f'embedding widths differ: {r} vs {rb}')
    k = int(k)
    if not 1 <= k <= n:
        raise ValueError(f'k={k} must be in [1, {n}]')
    ex = None if exclude is None else _exclusion_on(build_exclusion(exclude, m, n), A.device)
    if bf16 and FUSED_MAX_K_BF16 < k <= FUSED_MAX_K:
        # The bf16 kernel keeps 256 users' lists in LDS: k <= 32.  Beyond it the fp32 fused kernel (k <= 64) ranks exact fp32
        # copies of the rows - a bf16 x bf16 product is exact in fp32 either way, the fp32 sums differ in order only.
        # Costs a transient fp32 copy of the item table (twice its size); when that does not fit the catalog is ranked in windows
        # of rows (a copy of one window at a time) and the per-window lists are merged (merge_windows).
        if m == 0:
            idx = torch.empty(0, k, dtype=torch.int32, device=A.device)
            return (torch.empty(0, k, dtype=torch.float32, device=A.device), idx) if return_values else idx
        try:
            windows = [(0, _upcast_table(B))]
        except torch.OutOfMemoryError:
            step = max(k, -(-n // BF16_UPCAST_WINDOWS))
            windows = [(c0, None) for c0 in range(0, n, step)]
            if n - windows[-1][0] < k:   # a last window narrower than k joins the one before it
                windows.pop()
        out_i, out_v = [], []
        for b in range(0, m, BF16_UPCAST_USERS):
            Au = A[b:b + BF16_UPCAST_USERS].float()
            cand_v, cand_i = [], []
            for w, (c0, Bf) in enumerate(windows):
                c1 = windows[w + 1][0] if w + 1 < len(windows) else n
                v_, i_ = predict_topk(Au, Bf if Bf is not None else B[c0:c1].float(), k, clamp_negatives=clamp_negatives,
                                      return_values=True, arithmetic='fp32',
                                      exclude=None if ex is None else ex.shifted(b, c0))
                cand_v.append(v_)
                cand_i.append(i_ + c0 if ex is None else torch.where(i_ >= 0, i_ + c0, i_))
            v_, i_ = cand_v[0], cand_i[0]
            if len(windows) > 1:
                v_, i_ = merge_windows(torch.cat(cand_v, dim=1), torch.cat(cand_i, dim=1), k, fill=ex is not None)
            out_v.append(v_)
            out_i.append(i_)
        idx = torch.cat(out_i) if len(out_i) > 1 else out_i[0]
        return ((torch.cat(out_v) if len(out_v) > 1 else out_v[0]), idx) if return_values else idx
    idx = torch.empty(m, k, dtype=torch.int32, device=A.device)
    vals = torch.empty(m, k, dtype=torch.float32, device=A.device) if return_values else None

    def launch(form, ws=None):
        """tmf_predict_topk_<form>, or its _exclude twin with the exclusion struct; the plane forms take their workspace."""
        name = {'f32': 'tmf_predict_topk_%sf32', 'bf16': 'tmf_predict_topk_%sbf16', 'split': 'tmf_predict_topk_split_%sf32',
                'half2': 'tmf_predict_topk_half2_%sf32'}[form] % ('' if ex is None else 'exclude_')
        args = [A, B, m, n, r, lda, ldb, k, int(bool(clamp_negatives))]
        if ex is not None:
            args.append(ctypes.byref(ex.struct(m)))
        args += [idx, vals]
        if ws is not None:
            args += [ws, ws.numel()]
        _lib.check(getattr(lib, name)(*args, _lib.stream_ptr()), lib)   # looked up per call: tests wrap the entry points of lib
        return (vals, idx) if return_values else idx

    if bf16:
        return launch('bf16')
    if (arithmetic == 'split' and not split_topk_supported(r, k)) or (arithmetic == 'half2' and not half2_topk_supported(r, k)):
        raise ValueError(f"the plane kernels support widths <= 256 and k <= {SPLIT_MAX_K} ('split') / 32 ('half2') (got {r}, {k})")
    planes_optional = arithmetic == 'auto'   # 'auto' may fall back to the fp32 kernel (it needs no workspace) when memory is short
    if arithmetic == 'auto':
        # 32 < k <= 40 on tables of width <= 32: the fp32 kernel is the faster one (262144 x 100000, r = 32, k = 40: 43.9 against 38.1 TF;
        # r = 64: 65 against 69, r = 96: 65 against 86, r = 128: 86 against 113, r = 256: 100 against 127)
        planes = split_topk_supported(r, k) and not (k > 32 and r <= 32)
        arithmetic = 'split' if m * n >= SPLIT_MIN_SCORES and planes else 'fp32'
    if arithmetic in ('half2', 'split'):
        size = lib.tmf_predict_topk_half2_workspace_bytes if arithmetic == 'half2' else lib.tmf_predict_topk_split_workspace_bytes
        try:
            ws = torch.empty(size(n, r), dtype=torch.uint8, device=A.device)
        except torch.OutOfMemoryError:
            if not planes_optional:
                raise
            ws = None   # the planes of the item table (1.5x its size) do not fit: the fp32 MFMA kernel ranks without them
        if ws is not None:
            return launch(arithmetic, ws)
    return launch('f32')


def topk_stable(x, k, clamp_negatives=False, return_values=False, exclude=None, overwrite=False):
    """Row-wise top-k indices (int32) ordered like tf.math.top_k: value desc, ties -> lower index.
    exclude: pairs to leave out (build_exclusion; rows = the rows of x, columns = its columns unless an Exclusion view says
    otherwise): trailing slots past a row's eligible items hold -1 / -inf.  The ranking then works on x itself when ``overwrite``
    (the clamp and -inf for excluded entries are written into it), on a copy otherwise.  Without exclude x is only read."""
    lib = _lib.get()
    x = _cuda(x, torch.float32)
    squeeze = x.dim() == 1
    if squeeze:
        x = x[None, :]
    if x.stride(1) != 1:
        x = x.contiguous()
    elif exclude is not None and not overwrite:
        x = x.clone()
    rows, cols = x.shape
    k = int(k)
    if not 1 <= k <= cols:
        raise ValueError(f'k={k} must be in [1, {cols}]')  # tf.math.top_k raises for k > last dim
    ex = None if exclude is None else _exclusion_on(build_exclusion(exclude, rows, cols), x.device)
    run = lib.tmf_topk_stable_f32 if ex is None else lib.tmf_topk_stable_exclude_f32
    idx = torch.empty(rows, k, dtype=torch.int32, device=x.device)
    vals = torch.empty(rows, k, dtype=torch.float32, device=x.device) if return_values else None
    # large k over wide rows goes through a segmented radix sort with a workspace: a bounded number of rows per call
    step = rows if lib.tmf_topk_workspace_bytes(1, cols, k) == 0 else max(1, SORT_MAX_ELEMS // cols)
    ws = None
    for b in range(0, rows, step):
        e = min(b + step, rows)
        need = lib.tmf_topk_workspace_bytes(e - b, cols, k)
        if need and (ws is None or ws.numel() < need):
            ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        args = [x[b:e], e - b, cols, x.stride(0), k, int(bool(clamp_negatives))]
        if ex is not None:
            args.append(ctypes.byref(ex.shifted(b).struct(e - b)))
        _lib.check(run(*args, idx[b:e], vals[b:e] if return_values else None, ws,
                       ws.numel() if ws is not None else 0, _lib.stream_ptr()), lib)
    if squeeze:
        idx = idx[0]
        vals = vals[0] if return_values else None
    return (vals, idx) if return_values else idx


def gather_rows_cols(x, idx):
    """out[i, c] = x[i, idx[i, c]]."""
    lib = _lib.get()
    x = _cuda(x, torch.float32).contiguous()
    idx = _cuda(idx, torch.int64).contiguous()
    rows, cols = x.shape
    if idx.shape[0] != rows:
        raise ValueError('index_arr must have the same number of rows as input_arr')
    k = idx.shape[1]
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= cols):
        raise IndexError('column index out of range')
    out = torch.empty(rows, k, dtype=torch.float32, device=x.device)
    _lib.check(lib.tmf_gather_rows_cols_f32(x, idx, out, rows, cols, k,
                                            _lib.stream_ptr()), lib)
    return out


# ---- nearest neighbours inside one side (tmf_unit_rows_* + the fused top-k: implicit's similar_items / similar_users) ----
SIMILAR_BLOCK_BYTES = 2 << 30   # score block of the non-fused path (k > 64 or r > 256): MatrixFactorization._user_blocks' budget


def _row_ids(ids, n_rows, what='row'):
    """ids (an int sequence, array or tensor; any order, repeats allowed) as a flat int32 tensor where it is, every id checked
    against [0, n_rows): IndexError - no library needed."""
    ids = torch.as_tensor(ids).reshape(-1)
    if ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
        raise TypeError(f'{what} ids must be integers, got {ids.dtype}')
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n_rows):
        raise IndexError(f'{what} id out of range [0, {n_rows})')
    return ids.to(torch.int32).contiguous()


def _table_2d(t, what):
    t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
    if t.dim() != 2:
        raise ValueError(f'{what} must be 2-D [rows, r], got shape {tuple(t.shape)}')
    return t


def unit_rows(table, ids=None, return_norms=False):
    """Unit rows of table [n, r] (fp32 or bf16, any layout) in one launch of tmf_unit_rows_*: row j of the result is
    table[ids[j]] / ||table[ids[j]]|| (ids=None: every row in order), always fp32 - the [q, r] view of a [q, padded_ld(r)] buffer
    whose other columns are zero.  Right for every finite row whatever its scale; a zero row stays zero (norm 0); the same row
    content gives the same bits wherever it stands.  ids out of range raise IndexError.  return_norms: also the Euclidean norms
    (float32 [q])."""
    table = _table_2d(table, 'table')
    n, r = table.shape
    if ids is not None:
        ids = _row_ids(ids, n)
    lib = _lib.get()
    bf16 = table.dtype == torch.bfloat16
    T, n, r, ldt = _operand(table, 8 if bf16 else 4)
    ids = None if ids is None else ids.to(T.device)
    q = n if ids is None else ids.numel()
    ldo = _lib.padded_ld(r)
    out = torch.empty(q, ldo, dtype=torch.float32, device=T.device)
    norms = torch.empty(q, dtype=torch.float32, device=T.device) if return_norms else None
    run = lib.tmf_unit_rows_bf16 if bf16 else lib.tmf_unit_rows_f32
    _lib.check(run(T, n, r, ldt, ids, q, out, ldo, norms, _lib.stream_ptr()), lib)
    return (out[:, :r], norms) if return_norms else out[:, :r]


def similar_rows(table, k, *, ids=None, queries=None, metric='cosine', include_self=False, arithmetic=None, block_bytes=None):
    """The k rows of table [n, r] nearest to each query row -> (ids int32 [q, k], values float32 [q, k]), value descending, ties by
    ascending id.  The query rows are table[ids] (ids=None: every row), or ``queries`` [q, r] (embeddings of rows the table does
    not hold).  metric 'cosine' ranks unit_rows of both sides (a zero row has cosine 0 with everything), 'dot' the raw rows.
    Unless include_self is set or queries are given, query j never returns ids[j] (the exclusion CSR with one entry per row), so
    k <= n - 1 then and k <= n otherwise: ValueError beyond; ids out of range: IndexError.  All checks run before the library is
    touched.
    One fused predict_topk call where fused_topk_supported holds (arithmetic as there; a form whose kernel does not take this
    (r, k) - 'split' beyond k = 40, 'half2' beyond 32 - is answered by the fp32 MFMA kernel); otherwise blocks of at most
    block_bytes of scores (tmf_predict_gemm_f32 + tmf_topk_stable_*): no [q, n] matrix is ever whole in memory."""
    if metric not in ('cosine', 'dot'):
        raise ValueError(f"metric={metric!r}: expected 'cosine' or 'dot'")
    if ids is not None and queries is not None:
        raise ValueError('give ids (rows of the table) or queries (embeddings), not both')
    table = _table_2d(table, 'table')
    n, r = table.shape
    if queries is not None:
        queries = _table_2d(queries, 'queries')
        if queries.shape[1] != r:
            raise ValueError(f'queries are {queries.shape[1]} wide, the table {r}')
    if ids is not None:
        ids = _row_ids(ids, n)
    drop_self = queries is None and not include_self
    k, limit = int(k), n - 1 if drop_self else n
    if not 1 <= k <= limit:
        raise ValueError(f'k={k} must be in [1, {limit}]' + (f': {n} rows, and a row never returns itself' if drop_self else ''))
    arithmetic = arithmetic or PREDICT_ARITHMETIC
    if arithmetic not in ('auto', 'fp32', 'split', 'half2'):
        raise ValueError(f"arithmetic={arithmetic!r}: expected 'auto', 'fp32', 'split' or 'half2'")
    T = _cuda(table).detach()
    dev = T.device
    ids = None if ids is None else ids.to(dev)
    q = queries.shape[0] if queries is not None else n if ids is None else ids.numel()
    if q == 0:
        return torch.empty(0, k, dtype=torch.int32, device=dev), torch.empty(0, k, dtype=torch.float32, device=dev)
    if metric == 'cosine':
        B = unit_rows(T)
        A = unit_rows(queries) if queries is not None else B if ids is None else unit_rows(T, ids)
    else:
        B = T
        A = _cuda(queries).detach() if queries is not None else T if ids is None else T[ids.long()]
    ex = None
    if drop_self:   # row j leaves out ids[j]: one sorted entry per row, nothing to sort
        cols = torch.arange(n, dtype=torch.int32, device=dev) if ids is None else ids
        ex = Exclusion(torch.arange(q + 1, dtype=torch.int64, device=dev), cols, q, n)
    if fused_topk_supported(A, B, k):
        both_bf16 = A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16
        if not both_bf16 and ((arithmetic == 'split' and not split_topk_supported(r, k))
                              or (arithmetic == 'half2' and not half2_topk_supported(r, k))):
            arithmetic = 'fp32'
        vals, idx = predict_topk(A, B, k, return_values=True, arithmetic=arithmetic, exclude=ex)
        return idx, vals
    Bf = B if B.dtype == torch.float32 else B.float()
    budget = SIMILAR_BLOCK_BYTES if block_bytes is None else int(block_bytes)
    step = max(1, min(q, budget // (4 * n)))
    out_i, out_v = [], []
    for b in range(0, q, step):
        scores = predict_gemm(A[b:b + step], Bf)
        v_, i_ = topk_stable(scores, k, return_values=True, exclude=None if ex is None else ex.shifted(b), overwrite=True)
        out_v.append(v_)
        out_i.append(i_)
    return (torch.cat(out_i), torch.cat(out_v)) if len(out_i) > 1 else (out_i[0], out_v[0])


# ---- full-catalog ranks of held-out pairs (tmf_item_ranks_*: LightFM's predict_rank / auc_score / reciprocal_rank) ----
RANK_ROW_PAIRS = 16          # include/tmf.h TMF_RANK_ROW_PAIRS: positives per virtual row of the rank kernels
RANK_BLOCK_BYTES = 1 << 30   # score block of the non-fused path (tmf_predict_gemm_f32 + tmf_rank_count_rows_f32)


def positive_pairs(A, n_users, n_items, device=None):
    """CSR (an Exclusion: sorted, de-duplicated, range-checked) of the held-out positives: the entries of A with a value > 0 -
    recall_at_k's "relevant".  A: SparseInteractions (or indices / values / dense_shape) or a dense [n_users, n_items] table."""
    n_users, n_items = int(n_users), int(n_items)
    u, i, _, _ = _decode_table(A, 'positives', device, shape=(n_users, n_items), keep='positive')
    _check_ids(u, i, n_users, n_items, 'positive')
    return _pairs_csr(u, i, n_users, n_items)


def _csr_rows(rowptr):
    """Row of every entry of a CSR (int64)."""
    m = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(m, device=rowptr.device), rowptr[1:] - rowptr[:-1])


def _exclusion_view_pairs(ex, m, n):
    """(rows, local item ids) of an Exclusion view for m users x n items: ids outside the window are dropped (as the kernels do)."""
    rp = ex.rowptr[ex.user_base:ex.user_base + m + 1]
    lo, hi = int(rp[0]), int(rp[-1])
    cols = ex.cols[lo:hi].to(torch.int64) - ex.item_base
    rows = _csr_rows(rp - lo)
    keep = (cols >= 0) & (cols < n)
    return rows[keep], cols[keep]


def exclusion_counts(ex, m, n):
    """Distinct excluded items of each of the m users inside the n-item catalog (int64 [m])."""
    rows, _ = _exclusion_view_pairs(ex, m, n)
    return torch.bincount(rows, minlength=m)


def overlap_count(pos, ex, m, n):
    """Number of (user, item) pairs that are both positives and excluded: the two sorted key lists merged by searchsorted."""
    P = int(pos.rowptr[-1])
    er, ec = _exclusion_view_pairs(ex, m, n)
    if P == 0 or er.numel() == 0:
        return 0
    kp = _csr_rows(pos.rowptr) * n + pos.cols[:P].to(torch.int64)
    ke = (er * n + ec).to(kp.device)
    at = torch.clamp(torch.searchsorted(ke, kp), max=ke.numel() - 1)
    return int((ke[at] == kp).sum())


def virtual_rows(rowptr, pairs_per_row=RANK_ROW_PAIRS):
    """The rank kernels' rows: a user with P > 0 positives becomes ceil(P / pairs_per_row) rows of at most pairs_per_row of them
    (same user, consecutive CSR ranges), users in ascending order; users without positives get none.
    Returns (user int32, begin int64, count int32)."""
    counts = rowptr[1:] - rowptr[:-1]
    nv = (counts + pairs_per_row - 1) // pairs_per_row
    users = torch.repeat_interleave(torch.arange(counts.numel(), device=rowptr.device), nv)
    first = torch.cumsum(nv, 0) - nv
    part = torch.arange(users.numel(), device=rowptr.device) - first[users]
    begin = rowptr[users] + pairs_per_row * part
    count = torch.clamp(counts[users] - pairs_per_row * part, max=pairs_per_row)
    return users.to(torch.int32), begin.to(torch.int64), count.to(torch.int32)


def _rank_rows(vu, vb, vc, lo=0, hi=None):
    hi = vu.numel() if hi is None else hi
    return _lib.RankRows(vu.data_ptr() + 4 * lo, vb.data_ptr() + 8 * lo, vc.data_ptr() + 4 * lo, hi - lo)


def item_ranks(user_embedding, item_embedding, positives, exclude=None, arithmetic=None, return_pairs=False):
    """Full-catalog rank of every held-out positive: int32 [P] in the order of the positives' CSR (positive_pairs: row-major,
    ascending).  rank(u, i) = the number of ELIGIBLE items j != i (not excluded; other positives count) that the fused top-k's
    order (value desc, index asc) puts before i - 0 is the top.  Scores are the raw u.v (no clamp); an item whose score is NaN is
    never counted above anyone, a positive whose own score is NaN gets the number of its user's non-NaN eligible items (itself
    excluded).  No [m, n] score matrix is built.
    positives: SparseInteractions or a dense table (entries > 0; duplicates count once).  exclude: as predict_topk; a pair that is
    both positive and excluded raises ValueError (checked on the device before any launch), ids out of range IndexError.
    arithmetic: 'fp32' (fp32 MFMA) or 'split' (three bf16 planes, r <= 256) run the fused GEMM + count (tmf_item_ranks_*) with the
    pair scores of the same form (tmf_pair_scores_*); 'auto' takes 'split' where r <= 256, the scores computed (virtual rows x n)
    reach SPLIT_MIN_SCORES and the item planes fit, else 'fp32'.  'half2', bf16 tables and r > 256 score blocks of users with
    tmf_predict_gemm_f32 (bf16 rows cast to fp32 per block: the products are exact) and count with tmf_rank_count_rows_f32.
    Under the same arithmetic and exclusion, rank < k holds exactly when the item is in predict_topk(..., k) - claimed for the
    'fp32' and 'split' forms, whose pair scores are bit for bit those of their tiles.
    return_pairs: also the CSR -> (rowptr int64 [m + 1], cols int32, ranks)."""
    arithmetic = arithmetic or PREDICT_ARITHMETIC
    if arithmetic not in ('auto', 'fp32', 'split', 'half2'):
        raise ValueError(f"arithmetic={arithmetic!r}: expected 'auto', 'fp32', 'split' or 'half2'")
    (m, r), (n, rb) = tuple(user_embedding.shape), tuple(item_embedding.shape)
    if r != rb:
        raise ValueError(f'embedding widths differ: {r} vs {rb}')
    # the pairs are checked where the tables are, before anything is launched
    home = user_embedding.device if torch.is_tensor(user_embedding) else torch.device('cpu')
    pos = positive_pairs(positives, m, n, device=home)
    ex = None if exclude is None else build_exclusion(exclude, m, n, device=home)
    if ex is not None:
        both = overlap_count(pos, ex, m, n)
        if both:
            raise ValueError(f'{both} (user, item) pairs are both positives and excluded: a held-out pair cannot be left out of '
                             f'its own ranking')
    lib = _lib.get()
    U = _cuda(user_embedding).detach()
    V = _cuda(item_embedding).detach()
    dev = U.device
    pos = _exclusion_on(pos, dev)
    ex = None if ex is None else _exclusion_on(ex, dev)
    P = int(pos.rowptr[-1])
    ranks = torch.zeros(P, dtype=torch.int32, device=dev)
    out = (pos.rowptr, pos.cols, ranks) if return_pairs else ranks
    if P == 0:
        return out
    if arithmetic == 'split' and not lib.tmf_item_ranks_split_supported(r):
        raise ValueError(f"arithmetic='split' ranks widths <= 256 (got {r})")
    vu, vb, vc = virtual_rows(pos.rowptr)
    bf16 = U.dtype == torch.bfloat16 and V.dtype == torch.bfloat16
    fused = not bf16 and arithmetic != 'half2' and lib.tmf_item_ranks_f32_supported(r)
    if not fused:
        _item_ranks_blocks(lib, U, V, pos, ex, vu, vb, vc, ranks)
        return out
    A, _, _, lda = _operand(U)
    B, _, _, ldb = _operand(V)
    ws = None
    if arithmetic in ('auto', 'split'):
        if arithmetic == 'split' or vu.numel() * n >= SPLIT_MIN_SCORES:
            need = lib.tmf_item_ranks_split_workspace_bytes(n, r)
            try:
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
            except torch.OutOfMemoryError:
                if arithmetic == 'split':
                    raise
    pair_user = _csr_rows(pos.rowptr).to(torch.int32)
    scores = torch.empty(P, dtype=torch.float32, device=dev)
    pair_fn = lib.tmf_pair_scores_f32 if ws is None else lib.tmf_pair_scores_split
    _lib.check(pair_fn(A, B, r, lda, ldb, pair_user, pos.cols, P, scores,
                       _lib.stream_ptr()), lib)
    rows = _rank_rows(vu, vb, vc)
    exs = None if ex is None else ctypes.byref(ex.struct(m))
    if ws is None:
        _lib.check(lib.tmf_item_ranks_f32(A, B, n, r, lda, ldb, ctypes.byref(rows), pos.cols,
                                          scores, exs, ranks, _lib.stream_ptr()), lib)
    else:
        _lib.check(lib.tmf_item_ranks_split(A, B, n, r, lda, ldb, ctypes.byref(rows), pos.cols,
                                            scores, exs, ranks, ws, ws.numel(), _lib.stream_ptr()), lib)
    return out


def _item_ranks_blocks(lib, U, V, pos, ex, vu, vb, vc, ranks):
    """The non-fused path: fp32 score blocks of users (tmf_predict_gemm_f32), counted by tmf_rank_count_rows_f32; blocks without a
    positive are not scored."""
    m, n = U.shape[0], V.shape[0]
    Vf = V if V.dtype == torch.float32 else V.float()
    step = max(1, min(m, RANK_BLOCK_BYTES // (4 * max(n, 1))))
    bounds = torch.arange(0, m + step, step, device=vu.device).clamp_(max=m)
    cut = torch.searchsorted(vu, bounds.to(torch.int32)).tolist()
    bounds = bounds.tolist()
    exs = None if ex is None else ctypes.byref(ex.struct(m))
    for blk in range(len(bounds) - 1):
        b, e, lo, hi = bounds[blk], bounds[blk + 1], cut[blk], cut[blk + 1]
        if hi <= lo or e <= b:
            continue
        X = predict_gemm(U[b:e].float(), Vf)
        rows = _rank_rows(vu, vb, vc, lo, hi)
        _lib.check(lib.tmf_rank_count_rows_f32(X, e - b, n, X.stride(0), b, ctypes.byref(rows), pos.cols, exs,
                                               ranks, _lib.stream_ptr()), lib)


def auc_from_ranks(rowptr, ranks, n_items, excluded=None):
    """Per-user AUC from the positives' ranks (CSR order; item_ranks): P positives, N = n_items - excluded - P negatives; with the
    user's ranks sorted r_0 < ... < r_{P-1}, r_t - t negatives rank above the t-th positive, AUC = 1 - sum_t (r_t - t) / (P N) in
    fp64, 1.0 where N = 0 (NaN where P = 0).  Returns (auc float32 [m], P int64 [m])."""
    m = rowptr.numel() - 1
    counts = rowptr[1:] - rowptr[:-1]
    users = _csr_rows(rowptr)
    ranks = ranks.to(device=rowptr.device, dtype=torch.int64)
    srt = torch.sort(users * (n_items + 1) + ranks)[0] - users * (n_items + 1)   # ranks ascending inside each user
    t = torch.arange(users.numel(), device=users.device) - rowptr[users]
    above = torch.zeros(m, dtype=torch.float64, device=users.device).index_add_(0, users, (srt - t).to(torch.float64))
    excluded = torch.zeros_like(counts) if excluded is None else excluded.to(counts.device)
    neg = (n_items - excluded - counts).to(torch.float64)
    auc = 1.0 - above / (counts.to(torch.float64) * neg)
    auc = torch.where((neg == 0) & (counts > 0), torch.ones_like(auc), auc)
    return auc.to(torch.float32), counts


class GradedTable:
    """A graded test table as a CSR (graded_csr): row u's item ids are cols[rowptr[u]:rowptr[u + 1]] (ascending, distinct), their
    gains 2^a - 1 in gain; cols / gain hold at least one element (valid pointers for the kernel)."""

    def __init__(self, rowptr, cols, gain, n_users, n_items):
        self.rowptr, self.cols, self.gain = rowptr, cols, gain
        self.n_users, self.n_items = int(n_users), int(n_items)

    def stored(self):
        """Stored (non-zero) entries of every user (int64 [m]): the rows ndcg_at_k keeps without preserve_rows."""
        return self.rowptr[1:] - self.rowptr[:-1]


def graded_csr(A, n_users, n_items, device=None):
    """The graded test table of dcg_at_k / idcg_at_k / ndcg_at_k: every entry of A with its value a, duplicates summed (as
    SparseInteractions.to_dense does, in input order), entries whose sum is 0 dropped, gain = 2^a - 1 computed with the dense path's
    expression (torch.pow(2.0, a) - 1.0) where the table is.  A: SparseInteractions (or indices / values / dense_shape) or a dense
    [n_users, n_items] table.  A dense_shape or a dense shape other than (n_users, n_items) raises ValueError, an id out of range
    IndexError.  On the device the rows are ordered by tmf_csr_build; CPU tables (argument checks, tests) by a stable torch sort."""
    n_users, n_items = int(n_users), int(n_items)
    u, i, val, stated = _decode_table(A, 'test entries', device, shape=(n_users, n_items))
    if stated is not None and stated != (n_users, n_items):
        raise ValueError(f'the test table is {stated}, the model ranks [{n_users}, {n_items}]')
    u, i, val = u.contiguous(), i.contiguous(), val.to(torch.float32).contiguous()
    if u.numel() != val.numel():
        raise ValueError('indices and values disagree on the number of entries')
    nnz = u.numel()
    _check_ids(u, i, n_users, n_items, 'test')
    dev = u.device
    if dev.type == 'cuda' and 0 < nnz < 2 ** 31:
        lib = _lib.get()
        rowptr = torch.empty(n_users + 1, dtype=torch.int64, device=dev)
        cols = torch.empty(nnz, dtype=torch.int32, device=dev)
        vals = torch.empty(nnz, dtype=torch.float32, device=dev)
        rows = torch.empty(nnz, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.tmf_csr_build_workspace_bytes(nnz), dtype=torch.uint8, device=dev)
        pairs = torch.stack([u, i], 1)
        _lib.check(lib.tmf_csr_build(pairs, val, nnz, n_users, n_items, rowptr, cols,
                                     vals, rows, ws, ws.numel(), _lib.stream_ptr()), lib)
        del ws, pairs
    else:
        key = u * n_items + i
        perm = torch.sort(key, stable=True)[1]
        rows, cols, vals, rowptr = u[perm], i[perm].to(torch.int32), val[perm], None
    if nnz > 1:
        key = rows.to(torch.int64) * n_items + cols.to(torch.int64)
        first = torch.ones(nnz, dtype=torch.bool, device=dev)
        torch.ne(key[1:], key[:-1], out=first[1:])
        del key
        if not bool(first.all()):   # duplicates: adjacent, in input order
            starts = torch.nonzero(first).flatten()
            lengths = torch.diff(starts, append=torch.tensor([nnz], device=dev))
            vals = torch.segment_reduce(vals, 'sum', lengths=lengths)
            rows, cols, rowptr = rows[starts], cols[starts], None
    keep = vals != 0
    if not bool(keep.all()):
        rows, cols, vals, rowptr = rows[keep], cols[keep], vals[keep], None
    if rowptr is None:
        rowptr = torch.zeros(n_users + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(rows.to(torch.int64), minlength=n_users), 0, out=rowptr[1:])
    gain = torch.pow(2.0, vals) - 1.0
    if cols.numel() == 0:
        cols = torch.zeros(1, dtype=torch.int32, device=dev)
        gain = torch.zeros(1, dtype=torch.float32, device=dev)
    return GradedTable(rowptr, cols.contiguous(), gain.contiguous(), n_users, n_items)


def dcg_discounts(k, device):
    """log1p(j + 1) / log(2) for slots j = 0 .. k - 1: the expression of MatrixFactorization._dcg_terms, so that every term
    gain / discount is the dense path's term bit for bit."""
    order = torch.arange(1, k + 1, dtype=torch.float32, device=device)
    return torch.log1p(order) / float(np.log(np.float32(2.0)))


def dcg_idcg(table, top, k, n_zero=None, want_dcg=True, want_idcg=True):
    """Per-user DCG@k from the ranked lists top (int32 [m, >= k], -1 = empty slot) and IDCG@k of the graded table (GradedTable)
    with n_zero[u] zero gains beside the stored ones (None: every unstored item) - one launch of tmf_dcg_idcg_f32.
    Returns (dcg, idcg) float32 [m] on the device (None for what was not asked)."""
    lib = _lib.get()
    m, n, k = table.n_users, table.n_items, int(k)
    if k < 1:
        raise ValueError(f'k={k} must be >= 1')
    rowptr, cols, gain = (_cuda(table.rowptr, torch.int64).contiguous(), _cuda(table.cols, torch.int32).contiguous(),
                          _cuda(table.gain, torch.float32).contiguous())
    dev = rowptr.device
    den = dcg_discounts(k, dev)
    dcg = torch.empty(m, dtype=torch.float32, device=dev) if want_dcg else None
    idcg = torch.empty(m, dtype=torch.float32, device=dev) if want_idcg else None
    ldt = 0
    if want_dcg:
        top = _cuda(top, torch.int32)
        if top.dim() != 2 or top.shape[0] != m or top.shape[1] < k or top.stride(1) != 1:
            raise ValueError(f'top must be [{m}, >= {k}] int32 with unit column stride, got {tuple(top.shape)}')
        ldt = top.stride(0)
    nz = None if n_zero is None else _cuda(n_zero, torch.int64).contiguous()
    _lib.check(lib.tmf_dcg_idcg_f32(rowptr, cols, gain, m, n, top if want_dcg else None, ldt, k,
                                    den, nz, dcg, idcg, _lib.stream_ptr()), lib)
    return dcg, idcg


def reciprocal_rank_from_ranks(rowptr, ranks, n_items):
    """Per-user 1 / (1 + min rank) of the positives (CSR order), float32 (1 / (1 + n_items) where P = 0).  Returns (rr, P)."""
    m = rowptr.numel() - 1
    counts = rowptr[1:] - rowptr[:-1]
    best = torch.full((m,), int(n_items), dtype=torch.int64, device=rowptr.device)
    best = best.scatter_reduce(0, _csr_rows(rowptr), ranks.to(device=rowptr.device, dtype=torch.int64), reduce='amin')
    return (1.0 / (1.0 + best.to(torch.float64))).to(torch.float32), counts


# ---- alternating least squares (tmf_gram_f32 + tmf_als_solve_rows_f32 / tmf_als_cg_rows_f32: implicit's ALS and recalculate_user) ----
ALS_MAX_COMPONENTS = 128      # include/tmf.h: the per-row factorisation holds the packed triangle of an r x r matrix in LDS
ALS_CG_MAX_COMPONENTS = 256   # include/tmf.h: the conjugate-gradient form never forms the matrix
ALS_CG_MAX_STEPS = 32
ALS_CG_BATCH, ALS_CG_LONG_ROW = 32, 1024   # tmf_als_cg.hip: rows per workgroup, and the entries from which a whole workgroup walks a row


def _als_reg(reg):
    reg = float(reg)
    if not 0.0 < reg <= float(np.finfo(np.float32).max):   # NaN fails both comparisons
        raise ValueError(f'reg={reg!r}: the ALS regulariser must be finite and > 0')
    return reg


def gram(table):
    """table^T table of a [n, r] fp32 table (any layout), r <= 256 -> [r, r] float32.  Fixed summation order: exactly symmetric, and
    bit-identical from run to run (tmf_gram_f32; tmf_gram_wide_f32 for r > 128 only, so the bits at r <= 128 are tmf_gram_f32's)."""
    table = _table_2d(table, 'table')
    if not 1 <= table.shape[1] <= ALS_CG_MAX_COMPONENTS:
        raise ValueError(f'gram: width {table.shape[1]} outside [1, {ALS_CG_MAX_COMPONENTS}]')
    lib = _lib.get()
    T, n, r, ldt = _operand(table)
    G = torch.empty(r, r, dtype=torch.float32, device=T.device)
    size, run = ((lib.tmf_gram_workspace_bytes, lib.tmf_gram_f32) if r <= ALS_MAX_COMPONENTS
                 else (lib.tmf_gram_wide_workspace_bytes, lib.tmf_gram_wide_f32))
    ws = torch.empty(size(n, r), dtype=torch.uint8, device=T.device)
    _lib.check(run(T, n, r, ldt, G, r, ws, ws.numel(), _lib.stream_ptr()), lib)
    return G


def _als_row_operands(what, max_r, Y, rowptr, col, w, t, reg, G0, ids, out, n_failed, check):
    """The checks and device operands als_solve_rows and als_cg_rows share -> dict(reg, Y, n_other, r, ldy, g0, ldg, rowptr, col, w, t,
    ids, q, out, ldx, n_failed, n_rows)."""
    reg = _als_reg(reg)
    Y = _table_2d(Y, 'Y')
    n_other, r = Y.shape
    if not 1 <= r <= max_r:
        raise ValueError(f'{what}: width {r} outside [1, {max_r}]')
    rowptr = torch.as_tensor(rowptr).reshape(-1)
    n_rows = rowptr.numel() - 1
    if n_rows < 0:
        raise ValueError('rowptr must hold at least one offset')
    col, w, t = (torch.as_tensor(x).reshape(-1) for x in (col, w, t))
    if not (col.numel() == w.numel() == t.numel()):
        raise ValueError(f'col, w and t disagree on the number of entries: {col.numel()}, {w.numel()}, {t.numel()}')
    if check:
        col = _row_ids(col, n_other, 'column')
        if int(rowptr[0]) != 0 or int(rowptr[-1]) != col.numel() or (n_rows and bool((rowptr[1:] < rowptr[:-1]).any())):
            raise ValueError('rowptr is not a CSR row pointer over the entries given')
    if ids is not None:
        ids = _row_ids(ids, n_rows) if check else torch.as_tensor(ids).reshape(-1)
    Yt, _, _, ldy = _operand(Y)
    dev = Yt.device
    rowptr = _cuda(rowptr, torch.int64).contiguous()
    col, w, t = _cuda(col, torch.int32).contiguous(), _cuda(w, torch.float32).contiguous(), _cuda(t, torch.float32).contiguous()
    ids = None if ids is None else _cuda(ids, torch.int32).contiguous()
    if col.numel() == 0:   # no stored entry at all: every row is empty and gets zeros; the library wants valid pointers all the same
        col, w, t = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    g0, ldg = None, 0
    if G0 is not None:
        g0 = _cuda(_table_2d(G0, 'G0'), torch.float32).contiguous()
        if tuple(g0.shape) != (r, r):
            raise ValueError(f'G0 must be [{r}, {r}], got {tuple(g0.shape)}')
        ldg = r
    if out is None:
        out = torch.zeros(n_rows, _lib.padded_ld(r), dtype=torch.float32, device=dev)[:, :r]
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n_rows, r)
              and (n_rows == 0 or (out.stride(1) == 1 and out.stride(0) >= r)) and out.data_ptr() % 16 == 0):
        raise ValueError(f'out must be a CUDA float32 [{n_rows}, {r}] view with unit column stride, a row stride >= {r} and a 16-byte '
                         f'aligned base')
    if n_failed is None:
        n_failed = torch.zeros(1, dtype=torch.int32, device=dev)
    q = n_rows if ids is None else ids.numel()
    ldx = max(out.stride(0), r)   # a view of at most one row may state any stride
    return dict(reg=reg, Y=Yt, n_other=n_other, r=r, ldy=ldy, g0=g0, ldg=ldg, rowptr=rowptr, col=col, w=w, t=t, ids=ids, q=q, out=out,
                ldx=ldx, n_failed=n_failed, n_rows=n_rows)


def als_solve_rows(Y, rowptr, col, w, t, reg, G0=None, ids=None, out=None, n_failed=None, check=True):
    """One ALS half-step (tmf_als_solve_rows_f32): for the rows of the CSR (rowptr int64 [n_rows + 1], col: row ids of Y, w / t the
    per-entry weights and targets) the solutions of (G0 + reg I + sum w y y^T) x = sum t y -> (X, n_failed).  X is the [n_rows, r]
    view of a [n_rows, padded_ld(r)] table: ``out`` (such a view, written in place) or a fresh one of zeros.  ids: only these rows
    are solved (any order, repeats allowed) and the others keep what X held.  n_failed: int32 [1] on the device, counting the rows
    whose matrix was not positive definite (their x is zeros); pass the previous call's to keep counting.  check=False skips the id
    and CSR checks (a caller that has made them once)."""
    o = _als_row_operands('als_solve_rows', ALS_MAX_COMPONENTS, Y, rowptr, col, w, t, reg, G0, ids, out, n_failed, check)
    lib = _lib.get()
    _lib.check(lib.tmf_als_solve_rows_f32(o['Y'], o['n_other'], o['r'], o['ldy'], o['g0'], o['ldg'],
                                          o['rowptr'], o['col'], o['w'], o['t'], o['reg'],
                                          o['ids'], o['q'], o['out'], o['ldx'], o['n_failed'],
                                          _lib.stream_ptr()), lib)
    return o['out'], o['n_failed']


def als_cg_rows(Y, rowptr, col, w, t, reg, G0=None, ids=None, x0=None, out=None, n_failed=None, cg_steps=3, check=True):
    """als_solve_rows by ``cg_steps`` conjugate-gradient steps per row instead of a factorisation (tmf_als_cg_rows_f32; _als.py states
    the iteration), for widths up to 256.  x0: the [n_rows, r] float32 starting values (None: zeros) - a table of its own, or ``out``
    itself (in place), which needs ids that name no row twice (checked with check=True).  A row fails (x = 0, n_failed += 1) where
    p^T A p is not a positive finite number."""
    cg_steps = int(cg_steps)
    if not 1 <= cg_steps <= ALS_CG_MAX_STEPS:
        raise ValueError(f'als_cg_rows: cg_steps={cg_steps} outside [1, {ALS_CG_MAX_STEPS}]')
    o = _als_row_operands('als_cg_rows', ALS_CG_MAX_COMPONENTS, Y, rowptr, col, w, t, reg, G0, ids, out, n_failed, check)
    lib = _lib.get()
    r, n_rows, X = o['r'], o['n_rows'], o['out']
    ldx = o['ldx']
    if ldx % 4:
        raise ValueError(f'als_cg_rows: the row stride of out ({ldx}) must be a multiple of 4')
    x0t, ldx0 = None, 0
    if x0 is not None:
        if not (torch.is_tensor(x0) and tuple(x0.shape) == (n_rows, r)):
            raise ValueError(f'x0 must be a [{n_rows}, {r}] tensor')
        in_place = x0.is_cuda and x0.dtype == torch.float32 and x0.data_ptr() == X.data_ptr() and (n_rows <= 1 or x0.stride() == X.stride())
        if in_place:
            if check and o['ids'] is not None and torch.unique(o['ids']).numel() != o['ids'].numel():
                raise ValueError('als_cg_rows: in place (x0 is out) ids must not name a row twice')
            x0t, ldx0 = X, ldx
        else:
            x0t, _, _, ldx0 = _operand(_table_2d(x0, 'x0'))
            if n_rows and _overlap(x0t, n_rows, ldx0, X, ldx):
                raise ValueError('als_cg_rows: x0 and out overlap without being the same view')
    _lib.check(lib.tmf_als_cg_rows_f32(o['Y'], o['n_other'], r, o['ldy'], o['g0'], o['ldg'], o['rowptr'],
                                       o['col'], o['w'], o['t'], o['reg'], o['ids'], o['q'],
                                       x0t, ldx0, X, ldx, cg_steps, o['n_failed'], _lib.stream_ptr()), lib)
    return X, o['n_failed']


def _overlap(a, n_rows, lda, b, ldb):
    """Whether the byte ranges of two float32 row tables of n_rows rows intersect."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + 4 * n_rows * ldb and b0 < a0 + 4 * n_rows * lda


def pair_scores(A, B, pair_a, pair_b):
    """out[p] = <A[pair_a[p]], B[pair_b[p]]> as float32 (tmf_pair_scores_f32; ids int32 on the device, checked by the caller)."""
    lib = _lib.get()
    At, _, r, lda = _operand(A)
    Bt, _, _, ldb = _operand(B)
    out = torch.empty(pair_a.numel(), dtype=torch.float32, device=At.device)
    if pair_a.numel():
        _lib.check(lib.tmf_pair_scores_f32(At, Bt, r, lda, ldb, pair_a, pair_b, pair_a.numel(),
                                           out, _lib.stream_ptr()), lib)
    return out


def sample_negatives(n_items, n_users, n_samples, seed=0, device=None, user_offset=0, out=None, weights=None):
    """int32 [n_users, n_samples]: rows user_offset .. user_offset + n_users of the negative table of ``seed`` - exactly the table
    mf.utils.random_sampler_device draws (its definition), by one launch of tmf_sample_rows where the kernel takes the shape
    (tmf_sample_rows_supported: 2 n_samples <= n_items, n_samples within its LDS bound) and the device is a GPU, and by the torch
    function otherwise (most of the catalog per row, longer rows, the CPU): the same bits either way.  out: a contiguous int32
    [n_users, n_samples] tensor on the device to draw into.
    weights (int64 [n_items], None = uniform): the weighted table random_sampler_device(weights=...) defines - item i drawn with
    probability weights[i] / sum(weights) (utils.popularity_weights makes them; utils.weighted_cum states what is admitted and
    raises otherwise) - by tmf_sample_rows_weighted where tmf_sample_rows_weighted_supported holds on a GPU, else by the torch
    function: the same bits either way."""
    if weights is not None:
        return _sample_negatives_weighted(n_items, n_users, n_samples, seed, device, user_offset, out, weights)
    from .mf.sparse import default_device
    from .mf.utils import random_sampler_device
    n_items, n_users, n_samples, seed, user_offset = int(n_items), int(n_users), int(n_samples), int(seed), int(user_offset)
    device = default_device() if device is None else torch.device(device)
    if out is not None and not (torch.is_tensor(out) and out.dtype == torch.int32 and tuple(out.shape) == (n_users, n_samples)
                                and out.is_contiguous() and out.device.type == device.type):
        raise ValueError(f'out must be a contiguous int32 [{n_users}, {n_samples}] tensor on {device}')
    if n_samples > n_items:
        raise ValueError("Cannot take a larger sample than population when 'replace=False'")
    if n_users < 0 or user_offset < 0:
        raise ValueError(f'n_users={n_users}, user_offset={user_offset}: negative')
    native = device.type == 'cuda' and 0 < n_items < 2 ** 31 and n_samples < 2 ** 31 and \
        _lib.load_library().tmf_sample_rows_supported(n_items, n_samples)
    if not native:
        R = random_sampler_device(n_items, n_users, n_samples, seed=seed, device=device, user_offset=user_offset)
        if out is None:
            return R
        out.copy_(R)
        return out
    lib = _lib.get()
    seed = (seed + 2 ** 63) % 2 ** 64 - 2 ** 63   # the low 64 bits, as the torch function's wrapping arithmetic sees the seed
    with torch.cuda.device(out.device if out is not None else device):
        R = torch.empty(n_users, n_samples, dtype=torch.int32, device=device) if out is None else out
        failed = torch.zeros(1, dtype=torch.int32, device=R.device)
        _lib.check(lib.tmf_sample_rows(n_items, n_users, n_samples, seed, user_offset, R, failed, _lib.stream_ptr()),
                   lib)
        if n_users and int(failed):
            raise RuntimeError('could not draw distinct samples')
    return R


def _sample_negatives_weighted(n_items, n_users, n_samples, seed, device, user_offset, out, weights):
    """sample_negatives(weights=...)."""
    from .mf.sparse import default_device
    from .mf.utils import random_sampler_device, weighted_cum
    n_items, n_users, n_samples, seed, user_offset = int(n_items), int(n_users), int(n_samples), int(seed), int(user_offset)
    device = default_device() if device is None else torch.device(device)
    if out is not None and not (torch.is_tensor(out) and out.dtype == torch.int32 and tuple(out.shape) == (n_users, n_samples)
                                and out.is_contiguous() and out.device.type == device.type):
        raise ValueError(f'out must be a contiguous int32 [{n_users}, {n_samples}] tensor on {device}')
    if n_users < 0 or user_offset < 0:
        raise ValueError(f'n_users={n_users}, user_offset={user_offset}: negative')
    cum = weighted_cum(weights, n_items, n_samples)   # length, sign, dtype, total and the admission rule: before anything is drawn
    native = device.type == 'cuda' and n_items < 2 ** 31 and 0 < n_samples < 2 ** 31 and \
        _lib.load_library().tmf_sample_rows_weighted_supported(n_items, n_samples)
    if not native:
        R = random_sampler_device(n_items, n_users, n_samples, seed=seed, device=device, user_offset=user_offset, weights=weights)
        if out is None:
            return R
        out.copy_(R)
        return out
    lib = _lib.get()
    seed = (seed + 2 ** 63) % 2 ** 64 - 2 ** 63   # the low 64 bits, as the torch function's wrapping arithmetic sees the seed
    with torch.cuda.device(out.device if out is not None else device):
        R = torch.empty(n_users, n_samples, dtype=torch.int32, device=device) if out is None else out
        cum = cum.to(R.device)
        failed = torch.zeros(1, dtype=torch.int32, device=R.device)
        _lib.check(lib.tmf_sample_rows_weighted(cum, n_items, n_users, n_samples, seed, user_offset, R, failed, _lib.stream_ptr()),
                   lib)
        if n_users and int(failed):
            raise RuntimeError('could not draw distinct samples')
    return R
