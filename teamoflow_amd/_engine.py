"""Host side of the sparse training path: index structures built once per ``fit`` and the per-epoch
launch sequence.  Everything numeric runs in libtmf.so (HIP); torch is used for device memory,
streams and the one-off index preparation (sort / bincount / cumsum).

What replaces what (reference paths under /root/reference/src/teamoflow/mf/): the epoch functions at the end of this file replace
matrix_factorization.py:130-176 with one loss of loss_graphs.py each - LOSSES, the table behind them, is the ONE place that says what
every loss the engine trains is made of - and epoch_sides the same loop with plug-in sides: any of those losses, then the step of
every side that is an object (TrainState.sides: PlainL2Side, BiasSide, FeatureSide, ReLUSide <- embedding_graphs.py:30-87).
"""
import collections
import ctypes
import dataclasses
import os

import torch

from . import _lib

# Every environment switch this file reads: name -> (meaning, whether it selects a kernel form: the tests clear those before they
# set their own).  switch() below is the ONE reader and refuses a name that is not declared here; README's "Tunables" names them all.
SWITCHES = {
    'TMF_PART_BUDGET': ('bytes of gradU slice partials kept as one layer per slice (read once, at import)', False),
    'TMF_SLAB_BUDGET': ('bytes of partial rows the WMRB item pass may use', False),
    'TMF_USER_CHUNKS': ('user blocks of the item passes', True),
    'TMF_ITEM_SLICES': ('item slices of the sliced WMRB user pass', True),
    'TMF_SLICE_XCD': ('0 | 1: every XCD its own item slice', True),
    'TMF_FORCE_SLICED': ('1: the sliced WMRB user pass whatever the shape', True),
    'TMF_FORCE_FUSED': ('1: the one-kernel WMRB user pass where it fits', True),
    'TMF_ROWS4': ('0 | 1: the row-stationary item pass (tmf_wsum_rows5)', True),
    'TMF_ROWS5': ('0: the unbalanced row-stationary item pass (tmf_wsum_rows4)', True),
    'TMF_ROWS5_TARGET': ('list entries per part of a cut row of tmf_wsum_rows5', True),
    'TMF_ROWS4_PER_LAUNCH': ('rows per launch of the row-stationary item pass', True),
    'TMF_HINGE_ORDER': ('0: the hinge kernel takes the users in their natural order', True),
    'TMF_ROW_STATIONARY': ('0 | 1: the row-stationary gradU (tmf_wmrb_gradu4)', True),
    'TMF_G4_USERS': ('users per launch of tmf_wmrb_gradu4', True),
    'TMF_SCORES7': ('0 | 1: the item-run scores kernel (tmf_wmrb_scores7)', True),
    'TMF_S7_SLICE_BYTES': ('bytes of V rows per slice of tmf_wmrb_scores7', True),
    'TMF_S7_SLOTS': ('slots of a sub-chunk of tmf_wmrb_scores7', True),
    'TMF_S7_FILL': ('0: its steps stay in item order (tmf_wmrb_scores7_f32)', True),
    'TMF_S7_BUILD': ('device | torch: who builds the streams of tmf_wmrb_scores7', True),
    'TMF_SCORES6': ('0 | 1: the flat-stream scores kernel (tmf_wmrb_scores6)', True),
    'TMF_S6_SLICE_BYTES': ('bytes of V rows per slice of tmf_wmrb_scores6', True),
    'TMF_SCORES5': ('1: the row-stationary scores kernel (tmf_wmrb_scores5), opt-in only', True),
    'TMF_S5_SLICE_BYTES': ('bytes of V rows per slice of the stream of tmf_wmrb_scores5', True),
    'TMF_S5_PACE': ('0: its workgroups run freely', True),
    'TMF_S5_PACE_EVERY': ('slices between two rendezvous of its workgroups', True),
    'TMF_S5_LAG': ('windows a workgroup of tmf_wmrb_scores5 may run ahead of its peers', True),
    'TMF_S5_WGS': ('workgroups per launch of tmf_wmrb_scores5', True),
}


def switch(name, default=None):
    """The value of a declared switch (SWITCHES) in the environment, else ``default``."""
    if name not in SWITCHES:
        raise KeyError(f'{name} is not declared in _engine.SWITCHES')
    return os.environ.get(name, default)


DEFAULT_CHUNK = 1024  # list entries per segment (heavy rows are cut into several segments)
# bytes of gradU slice partials kept as one layer per slice (one launch); above it a single layer is summed in place by
# per-slice launches (C4: 6.6 GB of layers, 0.8 ms faster than in place; the config-5 shard would need 82 GB and sums in place)
PART_BUDGET = int(switch('TMF_PART_BUDGET', 8 << 30))


def row_bytes(n_components, dtype=torch.float32):
    """Bytes of one factor-table row as stored (padded to the row geometry, _lib.padded_ld)."""
    return _lib.padded_ld(n_components, dtype) * (2 if dtype is torch.bfloat16 else 4)


def _excl_cumsum(x):
    out = torch.zeros(x.numel() + 1, dtype=torch.int64, device=x.device)
    torch.cumsum(x, 0, out=out[1:])
    return out


def take_interactions(indices, values, keep, user_offset=0, item_offset=0):
    """(indices[keep] - offsets, values[keep]) of a COO list, selected COLUMN BY COLUMN.  Row-indexing a [nnz, 2] int64 device
    tensor with a mask (or index_select) returns wrong rows beyond ~6e7 rows on this PyTorch-ROCm build
    (tools/torch_row_index_probe.py: wrong from 7e7 rows on, 1-D masked selects stay correct) - and C4 has 1e8."""
    u = indices[:, 0][keep] - user_offset
    j = indices[:, 1][keep] - item_offset
    return torch.stack([u, j], dim=1), values[keep]


def stable_order(keys, n_rows):
    """(perm, rowptr): stable order of int keys in [0, n_rows) and the row pointers of the sorted list.
    Device tensors go through libtmf (tmf_stable_order_i32: rocPRIM radix sort + binary-search row pointers);
    CPU tensors (host-logic tests) through torch."""
    n = keys.numel()
    if keys.is_cuda and n < 2 ** 31 and n_rows < 2 ** 31:
        lib = _lib.get()
        k32 = keys.to(torch.int32).contiguous()
        perm = torch.empty(n, dtype=torch.int64, device=keys.device)
        rowptr = torch.empty(n_rows + 1, dtype=torch.int64, device=keys.device)
        ws = torch.empty(lib.tmf_stable_order_workspace_bytes(n), dtype=torch.uint8, device=keys.device)
        _lib.check(lib.tmf_stable_order_i32(k32, n, n_rows, perm, None, rowptr, ws,
                                            ws.numel(), _lib.stream_ptr()), lib)
        return perm, rowptr
    perm = torch.sort(keys, stable=True)[1]
    return perm, _excl_cumsum(torch.bincount(keys.to(torch.int64), minlength=n_rows))


class SegmentTable:
    """Rows of one side cut into segments of <= chunk entries (see include/tmf.h, tmf_segments).

    ``out_row`` (optional, int64 [rows]) maps every list row to the table row its partial sums belong
    to (several list rows per table row: the user-chunked WMRB item lists).  Then EVERY segment gets a
    slab slot, slots are numbered table-row-major, and all ``n_out`` table rows are finished by
    tmf_combine_rows."""

    def __init__(self, rowptr, chunk=DEFAULT_CHUNK, out_row=None, n_out=None, row_mod=0):
        rows = rowptr.numel() - 1
        nch, seg_row, seg_chunk = self._cut(rowptr[1:] - rowptr[:-1], chunk)
        if out_row is None:
            multi = nch > 1
            slab_beg = _excl_cumsum(nch * multi)
            seg_slab = torch.where(multi[seg_row], slab_beg[seg_row] + seg_chunk, torch.full_like(seg_chunk, -1))
            long_rows = torch.nonzero(multi).flatten()
            self.n_slab = int(slab_beg[-1])
            self.long_slab_beg = torch.cat([slab_beg[long_rows], slab_beg[-1:]]).contiguous()
        else:
            seg_slab, long_rows = self._slots_by_out_row(out_row[seg_row], n_out)
        self._set(rows, chunk, row_mod, rowptr.contiguous(), seg_row, seg_chunk, seg_slab, long_rows)

    @staticmethod
    def _cut(lens, chunk):
        """(segments per row, row of every segment, its chunk index): rows of ``lens`` entries cut into segments of <= chunk."""
        nch = torch.clamp((lens + (chunk - 1)) // chunk, min=1)
        nseg = int(nch.sum())
        seg_row = torch.repeat_interleave(torch.arange(lens.numel(), device=lens.device), nch, output_size=nseg)
        return nch, seg_row, torch.arange(nseg, device=lens.device) - _excl_cumsum(nch)[seg_row]

    def _slots_by_out_row(self, seg_out, n_out):
        """Every segment a slab slot, numbered output-row-major with the list order kept inside a row; all n_out rows are
        'long'.  seg_out: output row of every segment.  -> (seg_slab, long_rows); sets n_slab and long_slab_beg."""
        nseg = seg_out.numel()
        seg_slab = torch.empty(nseg, dtype=torch.int64, device=seg_out.device)
        seg_slab[torch.sort(seg_out, stable=True)[1]] = torch.arange(nseg, device=seg_out.device)
        self.n_slab = nseg
        self.long_slab_beg = _excl_cumsum(torch.bincount(seg_out, minlength=n_out))
        return seg_slab, torch.arange(n_out, device=seg_out.device)

    def _set(self, rows, chunk, row_mod, rowptr, seg_row, seg_chunk, seg_slab, long_rows):
        self.rows, self.chunk, self.nseg, self.row_mod = int(rows), int(chunk), int(seg_row.numel()), int(row_mod)
        self.rowptr = rowptr
        self.seg_row = seg_row.to(torch.int32)
        self.seg_chunk = seg_chunk.to(torch.int32)
        self.seg_slab = seg_slab.to(torch.int32)
        self.long_rows = long_rows.to(torch.int32)
        self.n_long = int(long_rows.numel())
        self._c = None

    @classmethod
    def of_rows(cls, rowptr, rows, out_row, n_out, chunk=DEFAULT_CHUNK):
        """Segments of a SUBSET of the list rows of ``rowptr`` (int64 ids ``rows``, any order), every one with a slab slot;
        ``out_row[i]`` in [0, n_out) is the output row the partial sums of list row ``rows[i]`` belong to.  One window of
        an item-row-sharded pass: the lists of the window's items, output rows relative to the window."""
        self = cls.__new__(cls)
        _, sel, seg_chunk = cls._cut(rowptr[rows + 1] - rowptr[rows], chunk)
        seg_slab, long_rows = self._slots_by_out_row(out_row[sel], n_out)
        self._set(rows.numel(), chunk, 0, rowptr, rows[sel], seg_chunk, seg_slab, long_rows)
        return self

    def cstruct(self):
        if self._c is None:
            self._c = _lib.Segments(self.rowptr.data_ptr(), self.seg_row.data_ptr(), self.seg_chunk.data_ptr(),
                                    self.seg_slab.data_ptr(), self.nseg, self.chunk, self.row_mod)
        return ctypes.byref(self._c)


class InteractionPlan:
    """CSR-by-user and CSC-by-item views of the interactions (values duplicated in both orders).  Inside a user the
    interactions are in ascending item order - the row-major order tf.sparse.SparseTensor is specified in - whatever
    order the caller's COO list has (duplicates keep their input order)."""

    def __init__(self, indices, values, n_users, n_items, chunk=DEFAULT_CHUNK, user_chunks=1, csc=True):
        dev = indices.device
        u = indices[:, 0].contiguous()
        j = indices[:, 1].contiguous()
        nnz = u.numel()
        if nnz:
            lo_u, hi_u, lo_j, hi_j = int(u.min()), int(u.max()), int(j.min()), int(j.max())
            if lo_u < 0 or hi_u >= n_users or lo_j < 0 or hi_j >= n_items:
                raise IndexError(f'interaction indices outside dense_shape: users [{lo_u}, {hi_u}] of {n_users}, '
                                 f'items [{lo_j}, {hi_j}] of {n_items}')
        values = values.to(torch.float32).contiguous()
        self.nnz, self.n_users, self.n_items = nnz, n_users, n_items
        if indices.is_cuda and nnz < 2 ** 31:
            # native: one stable sort on user * n_items + item, row pointers, column / value gather (tmf_csr_build)
            lib = _lib.get()
            idx64 = indices.to(torch.int64).contiguous()
            self.rowptr_u = torch.empty(n_users + 1, dtype=torch.int64, device=dev)
            self.col_u = torch.empty(nnz, dtype=torch.int32, device=dev)
            self.val_u = torch.empty(nnz, dtype=torch.float32, device=dev)
            self.user_of = torch.empty(nnz, dtype=torch.int32, device=dev)
            ws = torch.empty(lib.tmf_csr_build_workspace_bytes(nnz), dtype=torch.uint8, device=dev)
            _lib.check(lib.tmf_csr_build(idx64, values, nnz, n_users, n_items, self.rowptr_u,
                                         self.col_u, self.val_u, self.user_of, ws,
                                         ws.numel(), _lib.stream_ptr()), lib)
            del ws, idx64
        else:
            key = u.to(torch.int64) * n_items + j.to(torch.int64)
            if nnz > 1 and not bool((key[1:] >= key[:-1]).all()):
                perm = torch.sort(key, stable=True)[1]
                u, j, values = u[perm], j[perm], values[perm]
            self.rowptr_u = _excl_cumsum(torch.bincount(u, minlength=n_users))
            self.col_u = j.to(torch.int32)
            self.val_u = values.contiguous()
            self.user_of = u.to(torch.int32)
        self.seg_u = SegmentTable(self.rowptr_u, chunk)
        # CSC by item (only the MSE item pass reads it); with user_chunks = C > 1 by (user block, item), blocks
        # outermost, so that the U rows gathered at any time come from one cache-sized block of users
        C = max(1, int(user_chunks))
        self.user_chunks = C
        self.seg_i = self.rowptr_i = self.row_i = self.val_i = None
        if csc:
            if C > 1:
                upc = -(-n_users // C)
                key = (self.user_of.to(torch.int64) // upc) * n_items + self.col_u.to(torch.int64)
            else:
                key = self.col_u
            perm_c, self.rowptr_i = stable_order(key, C * n_items)
            self.row_i = self.user_of[perm_c].contiguous()
            self.val_i = self.val_u[perm_c].contiguous()
            if C > 1:
                out_row = torch.arange(C * n_items, device=dev) % n_items
                self.seg_i = SegmentTable(self.rowptr_i, chunk, out_row=out_row, n_out=n_items, row_mod=n_items)
            else:
                self.seg_i = SegmentTable(self.rowptr_i, chunk)
        self.n_pos = int((self.val_u > 0).sum())

    @property
    def user_ids(self):
        """int64 user of every CSR entry (tests, multi-GPU bookkeeping)."""
        return self.user_of.to(torch.int64)


def _slab_budget():
    """Bytes of per-(user block, item) partial rows the item pass may use: TMF_SLAB_BUDGET, else a quarter of the card's
    memory capped at 64 GB (config-5 shard, 1M items: 8 blocks 118 ms, 33 -> 106, 67 -> 90; C4 needs 8.3 GB either way)."""
    env = switch('TMF_SLAB_BUDGET')
    if env:
        return int(env)
    total = torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory if torch.cuda.is_available() else 32 << 30
    return int(min(64 << 30, total // 4))


def default_user_chunks(n_users, ld, target_bytes=3 << 20, n_items=None):
    """Number of user blocks the WMRB item lists are cut into so that the U rows the lists of one block
    gather (n_users / chunks * ld * 4 bytes, most of one XCD L2) stay cache-resident while that block is processed.
    Measured at C4 (1M users, 512-byte rows), item pass ms: 48 blocks 69.7, 64 -> 60.4, 96 -> 45.2, 123 -> 35.8,
    160 -> 33.8, 256 -> 33.7 (profiles/r01_user_chunk_sweep.txt; with non-temporal partial-row stores)."""
    env = switch('TMF_USER_CHUNKS')
    if env:
        return max(1, int(env))
    c = -(-n_users * ld * 4 // target_bytes)
    if n_items:  # every (block, item) list owns at least one fp32 partial row: keep that slab within budget
        c = min(c, max(1, _slab_budget() // (n_items * ld * 4)))
    return int(min(max(c, 1), 256)) if c > 1 else 1


def mse_user_chunks():
    """User blocks for the MSE item pass (CSC by (user block, item)).  Off by default: MSE lists are short (81M
    entries over 100K items at C4 against 1.1e9 for WMRB), so splitting them buys nothing - item pass 5.73 ms with
    1 block, 5.49 with 32, 8.57 with 123.  TMF_USER_CHUNKS forces a value (tests)."""
    env = switch('TMF_USER_CHUNKS')
    return max(1, int(env)) if env else 1


def default_item_slices(n_items, ld, n_samples=None, target_bytes=4 << 20, elem_size=4):
    """Number of item slices of the sliced WMRB user pass; 1 = the fused single-kernel pass.

    The sliced pass keeps every user's negatives sorted by item and walks the catalog in ~4 MB slices
    (slice-major grid) so that V rows are gathered from the XCD L2s instead of the Infinity Cache; the ids
    (and D) of a (user, slice) range are staged in LDS so a row gather depends on an LDS read only.
    At C4 (profiles/r01_sliced_user_pass.txt): scores 33.6 ms + hinge 25.5 ms + gradU 24.9 ms + finish = 86 ms
    against 134 ms for the fused kernel, which is bound by the Infinity-Cache gather rate.  Used when the V table
    is larger than two slices; small catalogs are L2-resident anyway and keep the fused kernel."""
    env = switch('TMF_ITEM_SLICES')
    if env:
        return max(1, int(env))
    # slices of ~4 MB of V rows in the table's OWN storage type (bf16 rows are half as long: C4 bf16 7 slices 65.4 ms, 13 68.0)
    if n_items * ld * elem_size <= 2 * target_bytes:
        return 1
    return int(min(-(-n_items * ld * elem_size // target_bytes), 64))


def slices_xcd_major(n_slices):
    """Block order of the slice kernels (tmf_slice_lists.xcd_major): every XCD its own slice (eight resident at a time) or all
    of them the same one.  TMF_SLICE_XCD = 0 | 1 forces it (the library reads the same variable)."""
    env = switch('TMF_SLICE_XCD')
    if env in ('0', '1'):
        return env == '1'
    return XCD_MAJOR_DEFAULT and n_slices >= 8


XCD_MAJOR_DEFAULT = False
SLICED_MIN_HINGE_TERMS = 1 << 16   # positives x negatives per user from which the O((S + P) log P) hinge step pays
SLICED_MIN_SCORES = 1 << 21        # n_users x n_samples below which the epoch is launch-bound and one fused kernel wins


def choose_wmrb_user_pass(n_users, n_items, ld, n_samples, n_positives, n_components, elem_size=4):
    """(item_slices, sliced) for a WMRB fit.  Large catalogs: the sliced pass with ~4 MB slices (default_item_slices).
    Small catalogs (V in the L2s, scores in LDS) default to the one-kernel pass, whose hinge step costs P_u x S terms per
    user - at the MovieLens-1M shape (C3: 6040 x 3706, S = 1853, 165 positives per user) that is 3e5 terms per user and
    the sliced pass with its O((S + P) log P) hinge kernel is faster although the catalog needs no slicing: 0.37 ms
    against 0.61 ms per user pass, item pass 0.20 against 0.26 (sorted negatives) - profiles/r02_hinge_rewrite.txt item 11.
    The slice count then only provides workgroups (the kernels also shrink their user groups, tmf_wmrb.hip)."""
    ns = default_item_slices(n_items, ld, elem_size=elem_size)
    if ns > 1 or not fused_user_pass_fits(n_samples, n_components) or switch('TMF_FORCE_SLICED') == '1':
        return ns, True
    if switch('TMF_ITEM_SLICES') or switch('TMF_FORCE_FUSED') == '1':
        return ns, False
    if (n_positives / max(n_users, 1)) * n_samples >= SLICED_MIN_HINGE_TERMS and n_users * n_samples >= SLICED_MIN_SCORES:
        groups = -(-n_users // 16)
        # slices: enough workgroups for a small user count, and no slice larger than one XCD L2 once the pass is sliced anyway
        return int(max(min(max(round(1400 / groups), 1), 8), -(-n_items * ld * elem_size // (4 << 20)))), True
    return 1, False


def rows4_wanted(n_components, dtype=torch.float32, plan=None, R=None, n_users=None, n_items=None):
    """Which form the WMRB item pass takes: False = lists -> partial rows -> combine (tmf_wsum_pass + tmf_combine_rows: every
    (user block, item) list writes one fp32 partial row into the slab), True = the ROW-STATIONARY form (lane groups own output rows,
    keep their sums in registers and walk the user blocks; no slab, no combine - tmf_wsum_rows5, balanced over virtual rows so that
    popular items are cut into parts, VirtualRows below).  Needs rows of at least 16 lanes.

    Default: row-stationary exactly when the slab form cannot block the users for the L2s - its slab (user blocks x items x fp32
    row) would exceed the budget at ~4 MB blocks, so the blocks grow (config-5 shard: 64 blocks of 10 MB, L2 hit rate 0.43, 128 GB
    of slab traffic per epoch; profiles/r05_c5_shard.txt).  Where the slab fits (C4: 163 blocks, 8.3 GB) the slab form stays:
    register-resident rows halve the waves per CU there (68 ms against 33, profiles/r03_c5_experiments.txt item 5).
    TMF_ROWS4 = 1 | 0 forces the choice."""
    env = switch('TMF_ROWS4')
    if env == '0':
        return False
    if not _lib.load_library().tmf_wsum_rows4_rows_per_group(int(n_components), int(dtype is torch.bfloat16)):
        return False
    if env == '1':
        return True
    if plan is not None:
        n_users = plan.n_users if n_users is None else n_users
        n_items = plan.n_items if n_items is None else n_items
    if not n_users or not n_items:
        return False
    blocks_wanted = -(-int(n_users) * row_bytes(n_components, dtype) // ROWS5_BLOCK_BYTES)   # user blocks of ~4 MB of rows as stored
    # one fp32 partial row per (block, item)
    blocks_slab_allows = max(1, _slab_budget() // (int(n_items) * _lib.padded_ld(n_components, dtype) * 4))
    return blocks_wanted > 2 * blocks_slab_allows


ROWS5_TARGET_OVER_MEDIAN = 1.15
ROWS5_BLOCK_BYTES = 4 << 20   # user blocks of the row-stationary item pass (config-5 shard: 160 blocks of 4 MB 80.6 ms, 305 blocks 86.5)


def rows5_user_chunks(n_users, n_components, dtype=torch.float32):
    """User blocks of the row-stationary item pass: ~4 MB of U rows as stored, at most 256 (TMF_USER_CHUNKS overrides)."""
    env = switch('TMF_USER_CHUNKS')
    if env:
        return max(1, int(env))
    return int(min(max(1, -(-int(n_users) * row_bytes(n_components, dtype) // ROWS5_BLOCK_BYTES)), 256))


class VirtualRows:
    """Work units of tmf_wsum_rows5 (include/tmf.h): output row i with cnt_i list entries (all user blocks together) is cut into
    P_i = ceil(cnt_i / target) parts, target = 1.15 x the median, at least the mean (TMF_ROWS5_TARGET overrides): the ordinary rows
    stay whole, the popular ones become parts of about the bulk's size, and a lane group's K consecutive virtual rows carry about K x mean entries
    whatever the popularity of its items.  Cut rows get consecutive slab slots (part order) and are finished by tmf_combine_rows."""

    def __init__(self, rowptr_e, n_blocks, n_rows, target=None):
        dev = rowptr_e.device
        lens = (rowptr_e[1:] - rowptr_e[:-1]).view(n_blocks, n_rows).sum(0)                       # entries of every output row
        mean = float(lens.to(torch.float64).mean()) if n_rows else 0.0
        median = float(lens.to(torch.float64).median()) if n_rows else 0.0
        env = switch('TMF_ROWS5_TARGET')
        # just above the bulk of the rows: the ordinary rows stay whole (a cut row costs a slab slot and a second pass over it), whatever
        # lies above is cut to about the bulk's size.  Config-5 shard (median 1,300, mean 1,405 entries per item), item pass ms by
        # target: 500: 103   700: 96   1000: 95   1200: 100 (every row cut in two)   1500: 81   2100: 93   4000: 170
        self.target = int(env) if env else (int(target) if target else max(1, int(max(ROWS5_TARGET_OVER_MEDIAN * median, mean)) + 1))
        parts = torch.clamp((lens + (self.target - 1)) // self.target, min=1)
        first = _excl_cumsum(parts)                                                               # first virtual row of every row
        nv = int(first[-1])
        item = torch.repeat_interleave(torch.arange(n_rows, device=dev), parts, output_size=nv)
        part = torch.arange(nv, device=dev) - first[item]
        multi = parts > 1
        slab_beg = _excl_cumsum(parts * multi)
        slot = torch.where(multi[item], slab_beg[item] + part, torch.full_like(part, -1))
        i32 = torch.int32
        self.n_vrows, self.n_slab = nv, int(slab_beg[-1])
        self.item = torch.cat([item, torch.tensor([n_rows], device=dev)]).to(i32).contiguous()   # + the sentinel (n_rows, 0, 1)
        self.part = torch.cat([part, torch.zeros(1, dtype=part.dtype, device=dev)]).to(i32).contiguous()
        self.nparts = torch.cat([parts[item], torch.ones(1, dtype=parts.dtype, device=dev)]).to(i32).contiguous()
        self.slot = slot.to(i32).contiguous()
        long_rows = torch.nonzero(multi).flatten()
        self.long_rows = long_rows.to(i32).contiguous()
        self.long_slab_beg = torch.cat([slab_beg[long_rows], slab_beg[-1:]]).contiguous()
        self.n_long = int(long_rows.numel())
        self.max_parts = int(parts.max()) if n_rows else 0


def fused_user_pass_fits(n_samples, n_components):
    """The one-kernel user pass keeps a user's scores and D in LDS; above ~13K negatives they do not fit and the sliced
    pass (no such limit) takes over whatever the catalog size."""
    return bool(_lib.load_library().tmf_wmrb_user_pass_fits(int(n_samples), min(int(n_components), 1024)))


HINGE_CHUNK = 255   # interactions the hinge kernel ranks per pass (csrc/tmf_hinge.hip: HCHUNK)


def hinge_user_order(rowptr_u):
    """Order in which the hinge kernel's waves take the users: by passes over their interactions (ceil(degree / 255)),
    most first, users of equal cost in their natural order (the bulk - one pass - keeps streaming its rows in sequence).
    None when no user needs a second pass.  Speed only (tmf_wmrb_hinge2_ordered)."""
    if switch('TMF_HINGE_ORDER', '1') == '0':
        return None
    deg = rowptr_u[1:] - rowptr_u[:-1]
    passes = (deg + (HINGE_CHUNK - 1)) // HINGE_CHUNK
    if passes.numel() == 0 or int(passes.max()) <= 1:
        return None
    return torch.argsort(passes, descending=True, stable=True).to(torch.int32)


class WmrbPlan:
    """Index structures of a WMRB fit, built once from the interactions and the static negative table.

    Item side: per-(user block, item) entry lists - the item's positives followed by the (user, sample) pairs whose
    negative is the item; list row = block * n_items + item, blocks of ceil(n_users / user_chunks) users outermost, so
    the waves running at any moment gather U rows of ONE cache-sized block of users.  Entry ids: k < nnz = interaction k
    of the CSR, nnz + u * S + s = negative s of user u; ``ent_row[e]`` = user of list entry e.
    Weights: ``wbuf = [delta (nnz) | D (m * S)]`` indexed by entry id; the user pass writes it and the item pass gathers
    through ``ent_w`` (entry id of every list entry).
    Sliced pass (``sliced``): ``R`` holds every user's negatives in ascending item order, ``slice_off`` / ``pos_off`` the first
    negative / interaction of every item slice."""

    def __init__(self, plan, R, chunk=DEFAULT_CHUNK, user_chunks=1, item_slices=1, n_components=128, sliced=None, item_lists=True,
                 xcd_major=None, rows4=False):
        dev = R.device
        m, S = R.shape
        nnz, n = plan.nnz, plan.n_items
        self.S, self.n_slices = S, max(1, int(item_slices))
        self.xcd_major = slices_xcd_major(self.n_slices) if xcd_major is None else bool(xcd_major)
        self.sliced = bool(sliced) if sliced is not None else (self.n_slices > 1 or not fused_user_pass_fits(S, n_components))
        C = self.user_chunks = max(1, int(user_chunks))
        E = nnz + m * S
        if E >= 2 ** 31:
            raise ValueError(f'interactions + n_users * n_samples = {E} >= 2^31 on one GPU: split the users over more GPUs')
        self.R_model = R  # the caller's table (model order): only D_in_model_order() reads it
        native = R.is_cuda
        lib = _lib.get() if native else None
        self.slice_off = self.pos_off = None
        if self.sliced:
            # every user's negatives in ascending item order (the order of s is immaterial to the loss); D is
            # produced in this order - D_in_model_order() maps it back
            ns = self.n_slices
            if native:
                Rs = torch.empty_like(R)
                ws = torch.empty(lib.tmf_sort_samples_workspace_bytes(m, S), dtype=torch.uint8, device=dev)
                _lib.check(lib.tmf_sort_samples(R, m, S, n, Rs, ws, ws.numel(),
                                                _lib.stream_ptr()), lib)
                del ws
                self.slice_off = torch.empty(m, ns + 1, dtype=torch.int32, device=dev)
                self.pos_off = torch.empty(m, ns + 1, dtype=torch.int32, device=dev)
                _lib.check(lib.tmf_slice_offsets(Rs, None, S, m, n, ns, self.slice_off,
                                                 _lib.stream_ptr()), lib)
                _lib.check(lib.tmf_slice_offsets(plan.col_u, plan.rowptr_u, 0, m, n, ns,
                                                 self.pos_off, _lib.stream_ptr()), lib)
            else:
                Rs = torch.sort(R.to(torch.int64), dim=1, stable=True)[0].to(torch.int32).contiguous()
                width = -(-n // ns)
                bnd = torch.arange(ns + 1, dtype=torch.int64) * width
                self.slice_off = torch.searchsorted(Rs.to(torch.int64), bnd[None, :].expand(m, -1).contiguous()).to(torch.int32)
                self.slice_off[:, -1] = S
                key = plan.user_of.to(torch.int64) * (ns * width + 1) + plan.col_u.to(torch.int64)  # ascending (CSR order)
                q = torch.arange(m, dtype=torch.int64)[:, None] * (ns * width + 1) + bnd[None, :]
                self.pos_off = (torch.searchsorted(key, q.reshape(-1)).reshape(m, ns + 1) - plan.rowptr_u[:-1, None]).to(torch.int32)
                self.pos_off[:, -1] = (plan.rowptr_u[1:] - plan.rowptr_u[:-1]).to(torch.int32)
            R = Rs
        self.R = R.contiguous()
        # ---- item-side entry lists ----
        self.ent_row = torch.empty(E, dtype=torch.int32, device=dev)
        rowptr = torch.empty(C * n + 2, dtype=torch.int64, device=dev)
        if native:
            ent_id = torch.empty(E, dtype=torch.int32, device=dev)
            ws = torch.empty(lib.tmf_wmrb_entry_lists_workspace_bytes(nnz, m, S), dtype=torch.uint8, device=dev)
            _lib.check(lib.tmf_wmrb_entry_lists(plan.user_of, plan.col_u, plan.val_u, nnz,
                                                self.R, m, S, n, C, self.ent_row,
                                                ent_id, rowptr, ws, ws.numel(),
                                                _lib.stream_ptr()), lib)
            del ws
        else:
            upc = max(1, -(-m // C))
            ku = plan.user_of.to(torch.int64)
            kp = torch.where(plan.val_u > 0, (ku // upc) * n + plan.col_u.to(torch.int64), torch.full_like(ku, C * n))
            ks = (torch.arange(m, dtype=torch.int64) // upc).repeat_interleave(S) * n + self.R.reshape(-1).to(torch.int64)
            keys = torch.cat([kp, ks])
            ent_id = torch.sort(keys, stable=True)[1]
            rowptr = _excl_cumsum(torch.bincount(keys, minlength=C * n + 1))
            owner = torch.cat([ku, torch.arange(m, dtype=torch.int64).repeat_interleave(S)])  # user of every entry id
            self.ent_row = owner[ent_id].to(torch.int32)
            ent_id = ent_id.to(torch.int32)
        self.rowptr_e = rowptr[:C * n + 1].contiguous()  # the row behind them holds the stored values <= 0: never read
        self.ent_w = ent_id
        self.rows4 = bool(rows4)
        # the row-stationary item pass walks VIRTUAL rows (popular items cut into parts); TMF_ROWS5=0: the plain form (tmf_wsum_rows4)
        self.vrows = VirtualRows(self.rowptr_e, C, n) if self.rows4 and switch('TMF_ROWS5', '1') != '0' else None
        if not item_lists or self.rows4:
            self.seg_e = None   # the caller cuts the lists into windows itself (SegmentTable.of_rows) / row-stationary item pass
        elif C > 1:
            out_row = torch.arange(C * n, device=dev) % n
            self.seg_e = SegmentTable(self.rowptr_e, chunk, out_row=out_row, n_out=n)
        else:
            self.seg_e = SegmentTable(self.rowptr_e, chunk)
        self.wbuf = torch.zeros(E, dtype=torch.float32, device=dev)
        self.delta = self.wbuf[:nnz]
        self.hinge_order = hinge_user_order(plan.rowptr_u)
        self.D = self.wbuf[nnz:].view(m, S)
        self._lists = None
        self.s5 = self.s6 = self.s7 = None   # Scores5Plan / Scores6Plan / Scores7Plan: the adopting TrainState fills at most one (scores_form)
        self.row_stationary = None   # wmrb_plan_for's answer to row_stationary_wanted (it sized the slices by it); None: a hand-built plan
        self.route = None   # wmrb_plan_for's keyword arguments where it built this plan: TrainState.set_negatives builds the next one alike
        self.prepared = []   # (method, arguments) of what was built on this plan for its loss - sample_rank, kos_omega, slot_offsets: set_negatives calls them on the next plan
        self.off = None      # slot_offsets(): the logQ offsets of this table, in the order of R / sp / D (None: an uncorrected fit)

    def release(self):
        """Drops every index structure (entry lists, sorted table, weights, score streams, slice lists, ranks) whoever still holds the
        plan object: TrainState.set_negatives frees the old plan before it builds the next."""
        for name in list(vars(self)):
            setattr(self, name, None)

    def lists(self, plan):
        """tmf_slice_lists of the sliced pass (kept alive with the plan)."""
        if self._lists is None:
            m, S = self.R.shape
            self._lists = _lib.SliceLists(self.R.data_ptr(), self.slice_off.data_ptr(), plan.rowptr_u.data_ptr(),
                                          plan.col_u.data_ptr(), self.pos_off.data_ptr(), m, S, self.n_slices, 0, 0, 0,
                                          (_lib.SLICE_XCD_MAJOR if self.xcd_major else 0) | _lib.SLICE_N_ITEMS_STATED, int(plan.n_items))
        return ctypes.byref(self._lists)

    def window_lists(self, plan, slice_begin, slice_count, item_base):
        """tmf_slice_lists restricted to slices [slice_begin, +slice_count); the V pointer of the call then holds the rows
        from item_base on (item-row-sharded V).  The caller keeps the returned struct alive."""
        m, S = self.R.shape
        return _lib.SliceLists(self.R.data_ptr(), self.slice_off.data_ptr(), plan.rowptr_u.data_ptr(), plan.col_u.data_ptr(),
                               self.pos_off.data_ptr(), m, S, self.n_slices, slice_begin, slice_count, item_base,
                               _lib.SLICE_N_ITEMS_STATED, int(plan.n_items))

    def sample_rank(self):
        """rank[u, pos] = the place in the model's random_ind row of the negative at place pos of the plan's row (16 bits, stored as
        int16; the identity where the plan keeps the model's order).  WARPLoss tries a user's samples in table order: the one
        consumer.  Built on first use, in blocks of users, and kept with the plan.  Samples of the same item may swap their
        places: they have the same score and their weights meet in the same row of V."""
        if getattr(self, '_rank', None) is None:
            m, S = self.R_model.shape
            if S > 65536:
                raise ValueError(f'n_samples={S}: the sample ranks of a WARPLoss fit are 16 bits (n_samples <= 65536)')
            rank = torch.empty(m, S, dtype=torch.int16, device=self.R_model.device)
            for b in range(0, m, 1 << 16):
                rows = self.R_model[b:b + (1 << 16)]
                if self.sliced:
                    rank[b:b + (1 << 16)] = torch.sort(rows, dim=1, stable=True)[1].to(torch.int16)   # wraps: the kernel reads unsigned
                else:
                    rank[b:b + (1 << 16)] = torch.arange(S, device=rows.device).to(torch.int16)[None, :]
            self._rank = rank
            self.prepared.append(('sample_rank', ()))
        return self._rank

    def kos_omega(self, nnz):
        """The weights of a KOSWARPLoss fit: fp32, one slot per stored interaction (tmf_kos_weights fills it, tmf_warp_pairs_kos reads
        it).  Allocated on first use - only this loss has it - and kept with the plan: the same buffer every epoch."""
        if getattr(self, 'omega', None) is None:
            self.omega = torch.empty(nnz, dtype=torch.float32, device=self.R.device)
            self.prepared.append(('kos_omega', (nnz,)))
        return self.omega

    def slot_offsets(self, ell):
        """The offsets of a SampledSoftmaxLoss fit under sampling_correction='logq': off[u, s] = ell[R[u, s]], fp32 [n_users, n_samples]
        in the plan's slot order (the order of sp and D), ell fp32 [n_items] on the plan's device (utils.log_expected_count).  Built
        once per table by tmf_slot_offsets - the pair step then reads it as a coalesced stream instead of gathering from ell every
        epoch - and kept with the plan; noted in ``prepared`` with ell, so TrainState.set_negatives builds it again for the next
        table and no epoch allocates."""
        if self.off is None:
            m, S = self.R.shape
            ell = ell.to(device=self.R.device, dtype=torch.float32).contiguous()
            n = (self.rowptr_e.numel() - 1) // self.user_chunks   # the plan's n_items: R's ids were checked against it
            if ell.numel() != n:
                raise ValueError(f'slot_offsets: {ell.numel()} offsets for {n} items')
            if self.R.is_cuda:
                lib = _lib.get()
                self.off = torch.empty(m, S, dtype=torch.float32, device=self.R.device)
                _lib.check(lib.tmf_slot_offsets(ell, n, self.R, m, S, self.off, _lib.stream_ptr()), lib)
            else:
                self.off = ell[self.R.to(torch.int64)]
            self.prepared.append(('slot_offsets', (ell,)))
        return self.off

    def D_in_model_order(self):
        """D[u, s] indexed like the model's random_ind (the sliced pass keeps every user's negatives sorted by item)."""
        if not self.sliced:
            return self.D
        perm = torch.sort(self.R_model.to(torch.int64), dim=1, stable=True)[1]
        out = torch.empty_like(self.D)
        out.scatter_(1, perm, self.D)
        return out


def row_stationary_wanted(n_users, n_items, n_samples, nnz, n_components, dtype=torch.float32, sliced=True):
    """Whether gradU runs row-stationary (tmf_wmrb_gradu4: lane groups own users, keep their gradient rows in registers and walk
    all slices; no partial rows, no finish kernel).  TMF_ROW_STATIONARY = 1 | 0 forces it; default: where the visits are short
    (short_visits) and the kernel exists for the geometry."""
    env = switch('TMF_ROW_STATIONARY')
    if env == '0' or not sliced:
        return False
    if not _lib.load_library().tmf_wmrb_gradu4_supported(int(n_components), int(dtype is torch.bfloat16)):
        return False
    return env == '1' or short_visits(n_users, n_items, n_samples, nnz, n_components, dtype)


def wmrb_plan_for(plan, R, n_components, dtype=torch.float32, n_items=None, force_sliced=False):
    """The WmrbPlan a fit builds for (plan, R): the user-pass form (choose_wmrb_user_pass), the item-pass form (rows4_wanted) and the
    user blocks that go with it - ONE place for MatrixFactorization._fit_sparse, dist.fit_data_parallel and bench.py.
    n_items: the catalog size for the slice geometry when the plan's table is padded (multi-GPU: rows padded to the world size).
    force_sliced: the sliced user pass whatever the shape (BPRLoss, WARPLoss: the one-kernel pass has the hinge built in); the slice count
    stays the one the shape gets."""
    m = plan.n_users
    n = plan.n_items if n_items is None else n_items
    ns, sliced = choose_wmrb_user_pass(m, n, _lib.padded_ld(n_components, dtype), int(R.shape[1]), plan.n_pos, n_components,
                                       elem_size=2 if dtype is torch.bfloat16 else 4)
    sliced = sliced or bool(force_sliced)
    # short visits (config-5 shard): the row-stationary gradU with its own slice size, unless the environment decides
    # (TMF_ROW_STATIONARY = 0 | 1, TMF_ITEM_SLICES)
    rs = row_stationary_wanted(m, n, int(R.shape[1]), plan.nnz, n_components, dtype, sliced)
    if rs and not switch('TMF_ITEM_SLICES'):
        ns = int(max(1, -(-n * row_bytes(n_components, dtype) // GRADU4_SLICE_BYTES)))
    rows4 = rows4_wanted(n_components, dtype, plan, R)
    C = rows5_user_chunks(m, n_components, dtype) if rows4 else default_user_chunks(m, _lib.padded_ld(n_components), n_items=plan.n_items)
    wplan = WmrbPlan(plan, R, user_chunks=C, item_slices=ns, n_components=n_components, sliced=sliced, rows4=rows4)
    wplan.route, wplan.row_stationary = dict(n_items=n_items, force_sliced=bool(force_sliced)), rs
    return wplan


def short_visits(n_users, n_items, n_samples, nnz, n_components, dtype=torch.float32):
    """Whether a (user, ~4 MB slice of V) visit of the sliced user pass is only a handful of rows - S x slice bytes / table bytes
    (+ the user's interactions in the slice): 9 at the config-5 shard (1M items x 512 bytes), 88 at C4.  Short visits are what
    tmf_wmrb_scores3 / gradu3 pay their per-visit round trips, their row of U and their partial row for; such shapes take the flat
    streams (tmf_wmrb_scores6) and the row-stationary gradU (tmf_wmrb_gradu4) instead."""
    table = n_items * row_bytes(n_components, dtype)
    if table < 8 * VISIT_SLICE_BYTES:   # short because the catalog is cut fine, not because a user has few negatives (tiny S)
        return False
    return (n_samples + nnz / max(n_users, 1)) * VISIT_SLICE_BYTES / table <= SCORES6_MAX_VISIT


SCORES6_SLICE_BYTES = 6 << 20   # slices of the flat-stream scores kernel, whatever the slice count of the other kernels.  Config-5 shard, scores ms
                                # by slice size: 2 MB 70.3   3 MB 59.6   4 MB 55.4   5 MB 53.9   6 MB 52.9   7 MB 53.8   8 MB 56.9 (scores3, 8 MB: 59.5)
VISIT_SLICE_BYTES = 4 << 20     # the slice size a visit's length is judged at (short_visits)
GRADU4_SLICE_BYTES = 3200000    # 3.2 MB slices for the row-stationary gradU: config-5 shard 160 slices 74.8 ms (128: 77.4, 192: 75.8, 256: 82.2;
                                # gradu3 + finish at 64 slices: 82.3)
SCORES6_MAX_VISIT = 24          # rows of a (user, 4 MB slice) visit up to which visits are too short for scores3 (config-5 shard: 9; C4: 86)
SCORES6_DEFAULT = True          # config-5 shard: 55.4 ms against 59.5 for scores3, fabric traffic 183 GB against 446 (profiles/r05_c5_shard.txt)


class _ScoreStreams:
    """What Scores5Plan and Scores6Plan share: ONE stable radix sort (stable_order) puts every (user, item) pair whose score the epoch
    needs - interaction k of the CSR (score -> p[k], place ~k) and negative (u, pos) of the item-sorted table (score -> sp[u, pos],
    place u * S + pos) - in key order; inside a key the interactions come first, then the negatives, each by user and item.  An id
    packs (user % users_per_owner) << 24 | item.  A stream = keys_per_stream consecutive keys, padded to whole steps of 8 entries
    with its last id (a valid user, a resident row) and the PAD place."""

    PAD = -2 ** 31

    def ready(self):
        """Nothing is left to build behind the constructor (Scores7Plan.ready)."""

    def _build(self, plan, wplan, users_per_owner, key_of, n_keys, keys_per_stream=1):
        """key_of(owner = user // users_per_owner, item) -> int32 key in [0, n_keys).  Sets ids, outs, n_entries, n_padded;
        -> (first padded entry of every stream, first sorted entry of every key)."""
        dev, i32, UO = plan.col_u.device, torch.int32, users_per_owner
        m, S = wplan.R.shape
        nnz = plan.nnz
        E = nnz + m * S
        uo = plan.user_of                                                  # int32 [nnz]
        rows = torch.arange(m, device=dev, dtype=i32)
        keys = torch.empty(E, dtype=i32, device=dev)
        keys[:nnz] = key_of(uo // UO, plan.col_u)
        keys[nnz:].view(m, S).copy_(key_of((rows // UO)[:, None], wplan.R))
        perm, rowptr = stable_order(keys, n_keys)
        del keys
        packed = torch.empty(E, dtype=i32, device=dev)
        packed[:nnz] = ((uo % UO) << 24) | plan.col_u
        packed[nnz:].view(m, S).copy_(((rows % UO) << 24)[:, None] | wplan.R)
        ids_sorted = packed[perm]
        del packed
        outs = torch.empty(E, dtype=i32, device=dev)
        outs[:nnz] = -1 - torch.arange(nnz, device=dev, dtype=i32)         # ~k: the score of interaction k goes to p[k]
        outs[nnz:] = torch.arange(m * S, device=dev, dtype=i32)            # u * S + pos: to sp[u, pos]
        outs_sorted = outs[perm]
        del outs, perm
        ptr = rowptr[::keys_per_stream].contiguous()
        cnt = ptr[1:] - ptr[:-1]
        ptr8 = _excl_cumsum((cnt + 7) // 8 * 8)
        E8 = int(ptr8[-1])
        self.ids = torch.empty(E8 + 8, dtype=i32, device=dev)
        self.outs = torch.full((E8 + 8,), self.PAD, dtype=i32, device=dev)
        self.ids[E8:] = 0
        step = 1 << 27
        for q0 in range(0, E8, step):
            q = torch.arange(q0, min(q0 + step, E8), device=dev, dtype=torch.int64)
            st = torch.searchsorted(ptr8, q, right=True) - 1
            r = q - ptr8[st]
            c = cnt[st]
            src = ptr[st] + torch.minimum(r, c - 1)
            self.ids[q0:q0 + q.numel()] = ids_sorted[src]
            self.outs[q0:q0 + q.numel()] = torch.where(r < c, outs_sorted[src], torch.full_like(src, self.PAD).to(i32))
            del q, st, r, c, src
        self.n_entries, self.n_padded = E, E8
        return ptr8, rowptr


class Scores6Plan(_ScoreStreams):
    """Entry stream of tmf_wmrb_scores6 (include/tmf.h), built once per fit from the sliced plan (_ScoreStreams): keyed by chunk =
    slice * n_groups + user group, so the scores of a user's visit are neighbours in the stream AND in sp / p; every chunk is a
    stream of its own."""

    def __init__(self, plan, wplan, n_components, dtype=torch.float32, slice_bytes=None):
        lib = _lib.load_library()   # the builder itself needs no GPU (tests/test_host_cpu.py runs it on CPU tensors)
        self.key = (int(n_components), dtype)
        UG = int(lib.tmf_wmrb_scores6_users_per_group())
        n = plan.n_items
        self.n_groups = ng = -(-wplan.R.shape[0] // UG)
        slice_bytes = int(switch('TMF_S6_SLICE_BYTES', slice_bytes or SCORES6_SLICE_BYTES))
        ns = int(min(max(1, -(-n * row_bytes(n_components, dtype) // slice_bytes)), max(1, (2 ** 31 - 1) // max(ng, 1))))
        width = -(-n // ns)
        self.n_slices = ns = -(-n // width)
        self.chunk_ptr, _ = self._build(plan, wplan, UG, lambda grp, item: (item // width) * ng + grp, ns * ng)

    def scores(self, lib, st):
        """One workgroup per (slice, group of 32 users) chunk, the group's rows in LDS."""
        return getattr(lib, 'tmf_wmrb_scores6' + st.sfx)(self.ids, self.outs, self.chunk_ptr, self.n_groups, self.n_slices, st.plan.n_users,
                                                         st.plan.n_items, st.U, st.V, st.sp, st.pk, st.r, _lib.stream_ptr())


SCORES7_SLICE_BYTES = 4 << 20   # slices of the item-run scores kernel (TMF_S7_SLICE_BYTES)
SCORES7_MIN_SHARE = 1.5         # expected entries per distinct row of a group from which sharing the row load pays (C4: 2.9; config-5 shard: 0.29)
# Scores7Plan.order_by_fill: a step costs STEP + SLOT * fill when a wave's range of a sub-chunk is cut (one row load and the record
# per step; four LDS reads, the products and the reduction per slot).  The unrolled loops of fill 4 / 3 / 2 / 1 issue 110 / 85 / 62 /
# 38 VALU and 16 / 12 / 8 / 4 LDS reads per wave-round of 8 steps against 64 CU clocks of row bytes: 3 + 2 fill = 11 / 9 / 7 / 5 sits
# between the VALU ratio and the flat row cost.  C4 figures: profiles/scores7_fill_c4.json
SCORES7_COST_STEP, SCORES7_COST_SLOT = 3, 2
SCORES7_FILL = True             # the default of TMF_S7_FILL


def scores7_fill_wanted():
    """Whether a TrainState that adopts a Scores7Plan puts its steps into fill order (Scores7Plan.order_by_fill) and runs
    tmf_wmrb_scores7_fill_f32.  TMF_S7_FILL = 0 | 1 forces the choice; 0 leaves the plan in item order for tmf_wmrb_scores7_f32."""
    return switch('TMF_S7_FILL', '1' if SCORES7_FILL else '0') != '0'


def scores7_sub_wave(cnt, W):
    """sub_wave [n_sub, W + 1] int32 of Scores7Plan.order_by_fill from the class counts cnt [n_sub, 4] int64 (steps of fill 4, 3, 2, 1)
    alone, in integers - both builders of the plan come through here."""
    K, dev, i64 = cnt.shape[1], cnt.device, torch.int64
    n_sub = cnt.shape[0]
    # wave w of W takes the steps between the points where the running cost passes w / W of the sub-chunk's; the running cost is
    # piecewise linear in the step (one slope per class), so the points come from the class counts alone - in integers
    zero = torch.zeros(n_sub, 1, dtype=i64, device=dev)
    slope = torch.tensor([SCORES7_COST_STEP + SCORES7_COST_SLOT * f for f in range(K, 0, -1)], dtype=i64, device=dev)
    step_edge = torch.cat([zero, torch.cumsum(cnt, 1)], 1)             # [n_sub, K + 1] first step of every class
    cost_edge = torch.cat([zero, torch.cumsum(cnt * slope, 1)], 1) * W
    target = cost_edge[:, K:] // W * torch.arange(1, W, device=dev, dtype=i64)       # [n_sub, W - 1], in units of 1 / W
    cls = (target[:, :, None] >= cost_edge[:, None, 1:K]).sum(2)                     # the class the point falls in
    cut = torch.gather(step_edge, 1, cls) + (target - torch.gather(cost_edge, 1, cls)) // (W * slope[cls])
    cut = torch.minimum((cut + 4) // 8 * 8, step_edge[:, K:])
    return torch.cat([zero, cut, step_edge[:, K:]], 1).to(torch.int32).contiguous()


class Scores7Plan:
    """Streams of tmf_wmrb_scores7 (include/tmf.h), built once per fit from the sliced plan; the builder needs no GPU.
    Every (user, item) pair whose score the epoch needs - interaction k of the CSR (place ~k) and negative (u, pos) of the item-sorted
    table (place u * S + pos) - is an ENTRY.  chunk = slice * n_groups + user group; the entries of a chunk, by (item, local user),
    are cut every `slots` entries into SUB-CHUNKS (so a sub-chunk is an item range of its chunk; neighbours may share their border
    item).  Inside a sub-chunk a run of entries with one item is cut into STEPS of up to K users; a slot is an entry's rank in its
    sub-chunk by (local user, place order): the slots of a user are consecutive and so are their addresses in sp / p.
      steps [n_steps, 4] int32   item | K 8-bit local users | K 16-bit slots; pads: the step's first user, slot = pad_slot
      place [n_entries] int32    sub-chunk after sub-chunk, slot order
      sub_step, sub_place [n_sub + 1] int64; chunk_sub [n_slices * n_groups + 1] int32
    builder='torch': the global sorts of __init__ (any device).  builder='device': the same bits from the chunk-local kernels of
    csrc/tmf_s7plan.hip (GPU tensors); steps and place are then written when first read or by order_by_fill().  None: TMF_S7_BUILD,
    else 'device' on a GPU."""

    K = 4

    def __init__(self, plan, wplan, n_components, dtype=torch.float32, slice_bytes=None, slots=None, builder=None):
        lib = _lib.load_library()
        self.key = (int(n_components), dtype)
        dev, i32, i64, K = plan.col_u.device, torch.int32, torch.int64, self.K
        self.users_per_group = UG = int(lib.tmf_wmrb_scores7_users_per_group())
        self.pad_slot = cap = int(lib.tmf_wmrb_scores7_slots())
        self.slots = SL = max(1, min(cap, int(switch('TMF_S7_SLOTS', slots or cap))))
        m, S = wplan.R.shape
        n, nnz = plan.n_items, plan.nnz
        E = nnz + m * S
        self.n_groups = ng = -(-m // UG)
        # a slice is a range of whole rows: a size below one row (0 and negative values of TMF_S7_SLICE_BYTES included) means one row
        slice_bytes = max(1, int(switch('TMF_S7_SLICE_BYTES', slice_bytes or SCORES7_SLICE_BYTES)))
        ns = int(min(max(1, -(-n * row_bytes(n_components, dtype) // slice_bytes)), max(1, (2 ** 31 - 1) // max(ng, 1))))
        self.width = width = -(-n // ns)
        self.n_slices = ns = -(-n // width)
        nc = ns * ng
        # builder: 'device' = the chunk-local kernels of csrc/tmf_s7plan.hip (GPU tensors, the shapes the scores kernel itself takes),
        # 'torch' = the global sorts below (any device; the oracle of the kernels).  None: TMF_S7_BUILD, else 'device' where it exists
        fits = n < 2 ** 24 and nnz < 2 ** 31 and m * S < 2 ** 31 and hasattr(lib, 'tmf_s7plan_chunks')   # (TMF_LIB_OLDER: an A/B library without them)
        builder = builder or switch('TMF_S7_BUILD') or ('device' if dev.type == 'cuda' and fits else 'torch')
        if builder not in ('device', 'torch'):
            raise ValueError(f"Scores7Plan: builder={builder!r} is neither 'device' nor 'torch'")
        if builder == 'device':
            if dev.type != 'cuda':
                raise ValueError(f"Scores7Plan: builder='device' needs the plan on a GPU, not on {dev} (builder='torch' runs anywhere)")
            self.n_entries = E
            return self._build_device(plan, wplan)
        ar = torch.arange(E, device=dev, dtype=i64)
        # entries in place order: e < nnz is interaction e, e >= nnz is negative e - nnz = u * S + pos
        user = torch.cat([plan.user_of.to(i64), torch.arange(m, device=dev, dtype=i64).repeat_interleave(S)])
        item = torch.cat([plan.col_u.to(i64), wplan.R.reshape(-1).to(i64)])
        lu = (user % UG).to(i32)
        chunk = (item // width) * ng + user // UG
        del user
        ordA = torch.sort((chunk * width + item % width) * UG + lu, stable=True)[1]   # entries by (chunk, item, local user)
        chunkA = chunk[ordA]
        cnt_c = torch.bincount(chunk, minlength=nc)
        del chunk
        chunk_sub = _excl_cumsum((cnt_c + SL - 1) // SL)
        subA = chunk_sub[chunkA] + (ar - _excl_cumsum(cnt_c)[chunkA]) // SL           # the sub-chunk of every entry, ascending
        del chunkA, cnt_c
        self.n_sub = n_sub = int(chunk_sub[-1])
        self.chunk_sub = chunk_sub.to(i32)
        self.sub_place = sub_place = _excl_cumsum(torch.bincount(subA, minlength=n_sub))
        # slots: a stable sort of the entries in place order by (sub-chunk, local user)
        sub_e = torch.empty(E, dtype=i64, device=dev)
        sub_e[ordA] = subA
        ordB = torch.sort(sub_e * UG + lu, stable=True)[1]
        place_e = torch.cat([-1 - torch.arange(nnz, device=dev, dtype=i32), torch.arange(m * S, device=dev, dtype=i32)])
        self.place = place_e[ordB]
        del place_e
        slot_e = torch.empty(E, dtype=i32, device=dev)
        slot_e[ordB] = (ar - sub_place[sub_e[ordB]]).to(i32)
        del sub_e, ordB
        slotA, itemA, luA = slot_e[ordA], item[ordA].to(i32), lu[ordA]
        del slot_e, item, lu, ordA
        # steps: runs of one item inside a sub-chunk, cut every K entries
        new_run = torch.ones(E, dtype=torch.bool, device=dev)
        if E > 1:
            new_run[1:] = (subA[1:] != subA[:-1]) | (itemA[1:] != itemA[:-1])
        run_start = torch.nonzero(new_run).flatten()
        run_of = torch.cumsum(new_run, 0) - 1
        del new_run
        run_len = torch.diff(run_start, append=torch.tensor([E], device=dev, dtype=i64))
        run_steps = (run_len + K - 1) // K
        del run_len
        run_step0 = _excl_cumsum(run_steps)
        self.n_steps = n_steps = int(run_step0[-1])
        sub_steps = torch.zeros(n_sub, dtype=i64, device=dev)
        sub_steps.scatter_add_(0, subA[run_start], run_steps)
        self.sub_step = _excl_cumsum(sub_steps)
        del subA, sub_steps, run_steps
        pos = ar - run_start[run_of]
        del ar, run_start
        stepA = run_step0[run_of] + pos // K
        k = pos % K
        del pos, run_of, run_step0
        users = torch.zeros(n_steps, K, dtype=i64, device=dev)
        slot4 = torch.full((n_steps, K), cap, dtype=i64, device=dev)
        first = k == 0
        users[stepA[first]] = luA[first].to(i64)[:, None]          # pads repeat the step's first user: a resident row
        users[stepA, k] = luA.to(i64)
        slot4[stepA, k] = slotA.to(i64)
        steps = torch.zeros(n_steps + 1, 4, dtype=i32, device=dev)  # one record behind the last: 16-byte loads never leave the buffer
        steps[stepA[first], 0] = itemA[first]
        del first, stepA, k, luA, slotA, itemA
        w = users[:, 0] | (users[:, 1] << 8) | (users[:, 2] << 16) | (users[:, 3] << 24)
        steps[:n_steps, 1] = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(i32)
        steps[:n_steps, 2] = (slot4[:, 0] | (slot4[:, 1] << 16)).to(i32)
        steps[:n_steps, 3] = (slot4[:, 2] | (slot4[:, 3] << 16)).to(i32)
        self.steps = steps
        self.n_entries = E

    def _s7plan_call(self, fn, *tail):
        rowptr, col, R, chunk_ent = self._dev[:4]
        m, S = R.shape
        _lib.check(fn(rowptr, col, R, col.numel(), m, S, self._n_items, self.width, self.slots, chunk_ent, self.chunk_sub, *tail,
                      _lib.stream_ptr()))

    def _build_device(self, plan, wplan):
        """The same streams from tmf_s7plan_chunks / _subs / _streams (include/tmf.h): a workgroup per sub-chunk finds its borders in
        the users' sorted lists, nothing of length E or n_steps is sorted.  Two device-to-host reads: n_sub and n_steps.  Holds on to
        rowptr_u, col_u and R until order_by_fill() has run (or for good, where it never does)."""
        lib = _lib.get()
        dev, i32, i64 = plan.col_u.device, torch.int32, torch.int64
        R = wplan.R.contiguous()
        nc = self.n_slices * self.n_groups
        self._n_items = plan.n_items
        chunk_ent = torch.empty(nc + 1, dtype=i64, device=dev)
        self.chunk_sub = torch.empty(nc + 1, dtype=i32, device=dev)
        self._dev = (plan.rowptr_u, plan.col_u, R, chunk_ent, None)
        ws = torch.empty(lib.tmf_s7plan_workspace_bytes(nc), dtype=torch.uint8, device=dev)
        self._s7plan_call(lambda *a: lib.tmf_s7plan_chunks(*a[:-1], ws, ws.numel(), a[-1]))
        self.n_sub = n_sub = int(self.chunk_sub[-1])
        sub_fill = torch.empty(n_sub, 4, dtype=i32, device=dev)
        self.sub_place = torch.empty(n_sub + 1, dtype=i64, device=dev)
        self.sub_step = torch.empty(n_sub + 1, dtype=i64, device=dev)
        ws = torch.empty(lib.tmf_s7plan_workspace_bytes(n_sub), dtype=torch.uint8, device=dev)
        self._s7plan_call(lib.tmf_s7plan_subs, n_sub, sub_fill, self.sub_place, self.sub_step, ws, ws.numel())
        self.n_steps = int(self.sub_step[-1])
        self._dev = self._dev[:4] + (sub_fill,)
        # steps and place are written when they are first asked for (_streams): a state that wants fill order (the default) calls
        # order_by_fill() first, and the item-ordered steps, 7 GB at C4, are then never written at all

    def _streams(self, fill_order):
        """The third call, into fresh buffers: the steps in the order asked for and, where they are not there yet, the places."""
        dev = self.chunk_sub.device
        self._steps = None
        steps = torch.empty(self.n_steps + 1, 4, dtype=torch.int32, device=dev)
        place = torch.empty(self.n_entries, dtype=torch.int32, device=dev) if self._place is None else None
        self._s7plan_call(_lib.get().tmf_s7plan_streams, self.n_sub, self.sub_step, self.n_steps, int(fill_order), steps, place)
        self._steps = steps
        if place is not None:
            self._place = place

    # steps / place: plain attributes of a torch-built plan; a device-built plan writes them on first use
    _steps = _place = None

    @property
    def steps(self):
        if self._steps is None and self._dev is not None:
            self._streams(False)
        return self._steps

    @steps.setter
    def steps(self, value):
        self._steps = value

    @property
    def place(self):
        if self._place is None and self._dev is not None:
            self._streams(False)
        return self._place

    @place.setter
    def place(self, value):
        self._place = value

    _dev = None                  # a device-built plan in item order: (rowptr_u, col_u, R, chunk_ent, sub_fill) for order_by_fill
    sub_wave = sub_fill = None   # the tables of tmf_wmrb_scores7_fill_f32: order_by_fill() builds them

    def ready(self):
        """What an adopting state asks before the first launch, inside its out-of-memory fallback: the steps in fill order where that
        is wanted (a plan that has its tables stays as it is); a device-built plan writes its streams here at the latest."""
        if scores7_fill_wanted():
            self.order_by_fill()
        self.steps

    def order_by_fill(self):
        """The second step of the plan, for tmf_wmrb_scores7_fill_f32 (include/tmf.h): the step records of every sub-chunk, stably, into
        descending FILL (= slots that are no pads), so the kernel runs each class with a loop that computes its slots only and a pad
        slot costs nothing.  A sub-chunk keeps its steps, its slots and its places: place / sub_place / sub_step / chunk_sub do not
        change, and inside a class the steps still ascend by (item, local user).
          sub_fill [n_sub, 4] int32          steps of fill 4, 3, 2, 1
          sub_wave [n_sub, waves + 1] int32  first step (counted from the sub-chunk's first) of every wave's contiguous range, cut for
                                             equal cost SCORES7_COST_STEP + SCORES7_COST_SLOT * fill per step, at multiples of 8 steps
                                             (a wave-round reads 8 records = 128 contiguous bytes)
        A second call changes nothing.  -> self"""
        if self.sub_wave is not None:
            return self
        W = int(_lib.load_library().tmf_wmrb_scores7_waves())
        if self._dev is not None:   # built on the device: the kernel writes the steps in fill order; places that are there stay
            self._streams(True)
            self.sub_fill = self._dev[4]
            self.sub_wave = scores7_sub_wave(self.sub_fill.to(torch.int64), W)
            self._dev = None
            return self
        K, cap, n_steps, n_sub = self.K, self.pad_slot, self.n_steps, self.n_sub
        dev, i32, i64 = self.steps.device, torch.int32, torch.int64
        rec = self.steps[:n_steps]
        fill = torch.zeros(n_steps, dtype=i64, device=dev)
        for word in (rec[:, 2], rec[:, 3]):
            fill += ((word & 0xffff) != cap).to(i64) + (((word >> 16) & 0xffff) != cap).to(i64)
        # the sub-chunk of every step (no sub-chunk is empty): a mark at every first step but the very first, summed up - with the
        # sorts, gathers and sums the constructor runs at this size (4.4e8 steps at C4), nothing else
        sub_of = torch.zeros(n_steps, dtype=i64, device=dev)
        if n_sub > 1:
            sub_of.scatter_add_(0, self.sub_step[1:n_sub], torch.ones(n_sub - 1, dtype=i64, device=dev))
        sub_of = torch.cumsum(sub_of, 0)
        key = sub_of * K + (K - fill)
        del fill, sub_of
        order = torch.sort(key, stable=True)[1]
        cnt = torch.bincount(key, minlength=K * n_sub).view(n_sub, K)      # steps of fill 4, 3, 2, 1
        del key
        steps = torch.zeros_like(self.steps)                               # with the record behind the last
        old64, new64 = self.steps.view(i64), steps.view(i64)               # a record = two 64-bit words, gathered one after the other
        for half in range(2):
            new64[:n_steps, half] = old64[:n_steps, half][order]
        del order, rec, old64, new64
        self.steps = steps
        self.sub_fill = cnt.to(i32).contiguous()
        self.sub_wave = scores7_sub_wave(cnt, W)
        return self

    def scores(self, lib, st):
        """One workgroup per (slice, group of 256 users) chunk, the group's rows in LDS, one load of a V row per run; a plan in fill
        order (order_by_fill) runs the kernel whose pad slots cost no work."""
        head = (self.steps, self.place, self.sub_step, self.sub_place, self.chunk_sub)
        tail = (self.n_groups, self.n_slices, st.plan.n_users, st.plan.n_items, st.U, st.V, st.sp, st.pk, st.r, _lib.stream_ptr())
        if self.sub_wave is None:
            return lib.tmf_wmrb_scores7_f32(*head, *tail)
        return lib.tmf_wmrb_scores7_fill_f32(*head, self.sub_wave, self.sub_fill, *tail)


class Scores5Plan(_ScoreStreams):
    """Entry streams of tmf_wmrb_scores5 (include/tmf.h), built once per fit from the sliced plan (_ScoreStreams): keyed by
    (workgroup = u // 256, slice = item // width); a workgroup's slices together are its stream.
    The slices only order the stream (the kernel never sees them), so they are fine: ~512 KB of V rows each."""

    def __init__(self, plan, wplan, n_components, dtype=torch.float32, slice_bytes=None):
        lib = _lib.load_library()   # like Scores6Plan: the builder itself needs no GPU
        dev = plan.col_u.device
        self.key = (int(n_components), dtype)   # what the streams were built for (the slice width follows the row bytes)
        UB = int(lib.tmf_wmrb_scores5_users_per_workgroup())
        n = plan.n_items
        self.n_wg = n_wg = -(-wplan.R.shape[0] // UB)
        slice_bytes = int(switch('TMF_S5_SLICE_BYTES', slice_bytes or (512 << 10)))
        ns = int(min(max(1, -(-n * row_bytes(n_components, dtype) // slice_bytes)), 4096, max(1, (2 ** 31 - 1) // max(n_wg, 1))))
        width = -(-n // ns)
        self.n_slices = ns
        i32 = torch.int32
        self.wg_ptr, rowptr = self._build(plan, wplan, UB, lambda wg, item: wg * ns + item // width, n_wg * ns, keys_per_stream=ns)
        wg_ptr8, wg_ptr = self.wg_ptr, rowptr[::ns]                         # [n_wg + 1] first padded / sorted entry of every workgroup
        # pacing: the workgroups of a launch meet every `pace_every` slices (tmf.h: window w may start when the peers have
        # completed window w - lag - 1; lag 0 = a barrier per window) and run freely in between - equal work per slice keeps them
        # within a slice or two of each other over such a stretch, a rendezvous per slice would cost more than a slice takes.
        # Window 0 is empty: passing it is the start line (every workgroup has its rows in LDS).  wstart = first step (8 entries)
        # of every window in every workgroup's stream; the padding sits behind a workgroup's last entry, so offsets inside a
        # workgroup are those of the sorted list
        # at most kS5MaxWindows (4096) windows: their first steps sit in LDS - a smaller request is widened, never an error
        every = max(1, int(switch('TMF_S5_PACE_EVERY', 32)), -(-ns // 4000))
        firsts = list(range(0, ns, every))
        off = rowptr[:n_wg * ns].view(n_wg, ns)[:, firsts] - wg_ptr[:-1, None]
        self.n_windows = nwin = len(firsts) + 1
        self.wstart = torch.zeros(n_wg, nwin + 1, dtype=i32, device=dev)
        self.wstart[:, 1:nwin] = ((off + 7) // 8).to(i32)
        self.wstart[:, nwin] = ((wg_ptr8[1:] - wg_ptr8[:-1]) // 8).to(i32)
        self.lag = int(switch('TMF_S5_LAG', 0))
        self.wgs_per_launch = int(switch('TMF_S5_WGS', 0))
        self.paced = switch('TMF_S5_PACE', '1') != '0' and ns > 1
        nb = lib.tmf_wmrb_scores5_workspace_bytes(n_wg, nwin, self.wgs_per_launch) if self.paced else 0
        self.sync = torch.zeros(max(nb // 4, 1), dtype=i32, device=dev)

    def scores(self, lib, st):
        """Workgroups own 256 users (rows in LDS) and walk one flat stream of (user, item) pairs."""
        return getattr(lib, 'tmf_wmrb_scores5' + st.sfx)(
            self.ids, self.outs, self.wg_ptr, self.n_wg, st.plan.n_users, st.plan.n_items, st.U, st.V, st.sp, st.pk, st.r,
            self.wgs_per_launch, self.wstart if self.paced else None, self.n_windows, self.lag, self.sync if self.paced else None,
            self.sync.numel() * 4, _lib.stream_ptr())


# A stream form of the sliced user pass's scores kernel, a row of SCORES_FORMS: the kernel tmf_wmrb_<name>; its switch (0: never, 1:
# forced, where `open` holds and the kernel exists); the library's query (n_components, bf16, n_items) -> 0 | 1; the plan class, built
# by the adopting TrainState into WmrbPlan.<slot>; open(q): what even a forced choice needs; default(q): the choice where the switch
# is not set (q: a ScoresQuery, the arguments of scores_form by name)
ScoresForm = collections.namedtuple('ScoresForm', 'name switch supported plan slot open default')
ScoresQuery = collections.namedtuple('ScoresQuery', 'n_users n_items n_samples nnz n_components dtype item_lists')


def _scores7_default(q):
    """Where the catalog is far beyond one slice and a group of UG users meets every row of a slice SCORES7_MIN_SHARE times or more;
    TMF_SCORES5=1 / TMF_SCORES6=1 win over it."""
    if switch('TMF_SCORES5') == '1' or switch('TMF_SCORES6') == '1' or q.n_items * row_bytes(q.n_components, q.dtype) < 8 * VISIT_SLICE_BYTES:
        return False
    UG = int(_lib.load_library().tmf_wmrb_scores7_users_per_group())
    return UG * (q.n_samples + q.nnz / max(q.n_users, 1)) / q.n_items >= SCORES7_MIN_SHARE


# In precedence order: the first row that is chosen runs, and when none is, tmf_wmrb_scores3 - one visit per (user, slice).
SCORES_FORMS = (
    # item runs: a group of 256 users' rows in LDS, one load of a row of V for all of them that need it.  fp32 rows of 65..128
    # components, fewer than 2^24 items, a table below 4 GB.  The default at C4 (2.9 entries per row of a group; config-5 shard: 0.29)
    ScoresForm('scores7', 'TMF_SCORES7', 'tmf_wmrb_scores7_supported', Scores7Plan, 's7', lambda q: True, _scores7_default),
    # flat streams on the slice-major grid.  Rows of 32 lanes, fewer than 2^24 items, a table below 4 GB.  The default where the visits
    # of scores3 are short (SCORES6_MAX_VISIT: the config-5 shard); TMF_SCORES5=1 wins even over TMF_SCORES6=1
    ScoresForm('scores6', 'TMF_SCORES6', 'tmf_wmrb_scores6_supported', Scores6Plan, 's6', lambda q: switch('TMF_SCORES5') != '1',
               lambda q: SCORES6_DEFAULT and short_visits(q.n_users, q.n_items, q.n_samples, q.nnz, q.n_components, q.dtype)),
    # row-stationary: workgroups own 256 users and walk one flat stream ordered by item.  Same geometries as scores6, and a plan with
    # item lists.  OPT-IN, never the default: built for the config-5 shard and measured there at 68 - 124 ms against 63 ms for scores3,
    # whatever the pacing (profiles/r04_scores5_experiment.txt)
    ScoresForm('scores5', 'TMF_SCORES5', 'tmf_wmrb_scores5_supported', Scores5Plan, 's5', lambda q: q.item_lists, lambda q: False),
)


def scores_form(n_users, n_items, n_samples, nnz, n_components, dtype=torch.float32, sliced=True, on_gpu=True, item_lists=True,
                after=None):
    """(name, forced): the kernel that computes the scores of the sliced user pass - the first row of SCORES_FORMS (behind the row
    ``after``, where one is named: that form's streams did not fit) that is chosen, else 'scores3' - and whether its switch forced it.
    Every stream form needs the sliced pass, the plan on the GPU and int32 places (n_users n_samples, nnz < 2^31)."""
    rows = SCORES_FORMS[[f.name for f in SCORES_FORMS].index(after) + 1:] if after else SCORES_FORMS
    if sliced and on_gpu and n_users * n_samples < 2 ** 31 and nnz < 2 ** 31:
        q, lib = ScoresQuery(n_users, n_items, n_samples, nnz, n_components, dtype, item_lists), _lib.load_library()
        for f in rows:
            forced = switch(f.switch) == '1'
            if switch(f.switch) != '0' and f.open(q) and getattr(lib, f.supported)(int(n_components), int(dtype is torch.bfloat16), int(n_items)) \
                    and (forced or f.default(q)):
                return f.name, forced
    return 'scores3', False


def scores_form_of(plan, wplan, n_components, dtype=torch.float32, after=None):
    """scores_form of a state over (plan, wplan): what TrainState._adopt_wplan asks."""
    if wplan is None:
        return 'scores3', False
    m, S = wplan.R.shape
    return scores_form(m, plan.n_items, S, plan.nnz, n_components, dtype, wplan.sliced, plan.col_u.is_cuda, wplan.seg_e is not None, after=after)


ITEM_BIAS_CHUNK = DEFAULT_CHUNK   # list entries one wave of tmf_item_bias_grad sums (longer list rows are cut into several chunks)


def item_bias_chunks(rowptr_e, n_items, chunk=ITEM_BIAS_CHUNK):
    """The chunks c >= 1 of the entry lists ``rowptr_e`` (list row = block * n_items + item) as tmf_item_bias_grad takes them (chunk 0
    of every list row needs no table): -> (xrow, xchunk int32 [n_extra], xptr int64 [n_items + 1], n_extra), ordered by (item, block,
    chunk).  Built once per plan with torch, on the lists' device."""
    dev = rowptr_e.device
    lens = rowptr_e[1:] - rowptr_e[:-1]
    extra = torch.clamp((lens + (chunk - 1)) // chunk - 1, min=0)
    rows = torch.nonzero(extra).flatten()                       # the list rows longer than a chunk, ascending: block-major
    rows = rows[torch.sort(rows % n_items, stable=True)[1]]     # by item, an item's blocks in their order
    cnt = extra[rows]
    n_extra = int(cnt.sum())
    xrow = torch.repeat_interleave(rows, cnt, output_size=n_extra)
    first = _excl_cumsum(cnt)[:-1]
    xchunk = torch.arange(n_extra, device=dev) - torch.repeat_interleave(first, cnt, output_size=n_extra) + 1
    per_item = torch.zeros(n_items, dtype=torch.int64, device=dev).index_add_(0, rows % n_items, cnt)
    return xrow.to(torch.int32).contiguous(), xchunk.to(torch.int32).contiguous(), _excl_cumsum(per_item), n_extra


class ItemScalarBias:
    """The scalar item bias of a table-family state (scores U[u] . V[i] + b[i]; csrc/tmf_itembias.hip): ``b`` and its second buffer
    ``b_nxt`` - the stepped bias under TMF_EPI_ADAM (TrainState.swap exchanges them), the raw gradient under TMF_EPI_GRAD (``epi``:
    persistent Adam steps b in place from it) -, both fp32 [n_items rounded up to 4] with zeros behind n_items, so that the vector
    is also a padded [rows, 4] table for the table steps; and, per WmrbPlan (``adopt``), the chunk tables and the fp64 workspace of
    tmf_item_bias_grad.  The passes read everything else (R, rowptr_e, ent_w, wbuf) from the state's plan when they launch."""

    def __init__(self, b0, n_items, dev):
        b0 = torch.as_tensor(b0).detach().to(device=dev, dtype=torch.float32).reshape(-1)
        if b0.numel() != n_items:
            raise ValueError(f'item_scalar_bias of {b0.numel()} elements for {n_items} items')
        self.n, self.chunk, self.epi = int(n_items), ITEM_BIAS_CHUNK, _lib.EPI_ADAM
        self.b = torch.zeros(max(-(-self.n // 4) * 4, 4), dtype=torch.float32, device=dev)
        self.b[:self.n] = b0
        self.b_nxt = torch.zeros_like(self.b)

    def adopt(self, wplan):
        lib = _lib.load_library()
        self.xrow = self.xchunk = self.xptr = self.ws = None   # the old plan's, before the next ones are built
        self.xrow, self.xchunk, self.xptr, self.n_extra = item_bias_chunks(wplan.rowptr_e, self.n, self.chunk)
        nb = lib.tmf_item_bias_grad_workspace_bytes(self.n, wplan.user_chunks, self.n_extra)
        self.ws = torch.empty(max(nb // 8, 1), dtype=torch.float64, device=self.b.device)

    @property
    def value(self):
        return self.b[:self.n]


class TrainState:
    """Double-buffered factor tables [rows, ld] and the scratch the passes need.
    ``V_tables`` = (V, V_nxt) already padded: several states (the user batches of a mini-batch fit) step the SAME item table;
    ``scratch`` = a dict shared by such states: the per-step buffers are allocated once at the largest size any of them needs
    (``share_scratch``) instead of once per state."""

    def __init__(self, U0, V0, plan, n_components, wplan=None, dtype=torch.float32, V_tables=None, scratch=None, kl=False,
                 user_bias=None, item_bias=None, user_feat=None, item_feat=None, user_relu=None, item_relu=None, full_softmax=False,
                 item_scalar_bias=None):
        dev = plan.col_u.device
        # the scalar item bias b0 [n_items] (None: today's state): everything it needs is allocated here and in set_negatives
        self.ib = None
        if item_scalar_bias is not None:
            if wplan is None or not wplan.sliced or dtype is not torch.float32 or V_tables is not None or scratch is not None:
                raise ValueError('item_scalar_bias needs a sliced WmrbPlan (wmrb_plan_for(force_sliced=True)) and float32 factor '
                                 'tables and scratch of its own')
            self.ib = ItemScalarBias(item_scalar_bias, plan.n_items, dev)
        if full_softmax:   # epoch_full_softmax: every user's log-partition (rewritten each epoch) and its number of positives, as fp32
            if dtype is not torch.float32 or int(n_components) > FULL_SOFTMAX_MAX_COMPONENTS or plan.seg_i is None or V_tables is not None:
                raise ValueError(f'the full softmax needs float32 tables of its own with n_components <= {FULL_SOFTMAX_MAX_COMPONENTS} '
                                 f'and a plan with csc=True')
            self.fsm_lse = torch.zeros(max(plan.n_users, 1), dtype=torch.float32, device=dev)
            self.fsm_w = torch.bincount(plan.user_of[plan.val_u > 0].to(torch.int64), minlength=max(plan.n_users, 1)).to(torch.float32)
        if kl:   # epoch_kl: the per-segment fp64 moments of the user side and the six coefficients tmf_kl_coeffs derives from them
            self.kl_part = torch.zeros(max(plan.seg_u.nseg, 1), 6, dtype=torch.float64, device=dev)
            self.kl_coef = torch.zeros(6, dtype=torch.float64, device=dev)
        self.r = int(n_components)
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError('factor tables are stored as float32 or bfloat16')
        self.dtype = dtype
        self.sfx = '_bf16' if dtype is torch.bfloat16 else '_f32'
        self.ld = _lib.padded_ld(self.r, dtype)
        sided = [x for x in (user_bias, item_bias, user_feat, item_feat, user_relu, item_relu) if x is not None]
        if sided and (dtype is not torch.float32 or V_tables is not None):
            raise ValueError('a biased side, a side over sparse features or a ReLU side needs float32 factor tables of its own')
        if (user_bias is not None and user_feat is not None) or (item_bias is not None and item_feat is not None):
            raise ValueError('a side over sparse features has no bias form')
        if (user_relu is not None and (user_bias is not None or user_feat is not None)) or \
                (item_relu is not None and (item_bias is not None or item_feat is not None)):
            raise ValueError('a ReLU side carries its own features and bias (user_relu / item_relu: dict(F=, Wr0=, b0=))')
        # a biased side (BiasSide): U / V is its effective table E = W + b, rebuilt in place every epoch - no second buffer.
        # A side over sparse features (FeatureSide): U0 / V0 are its weights [n_features, r] and U / V is E = F W, likewise
        # A ReLU side (ReLUSide): U0 / V0 are its output weights [aux, r] and U / V is E = relu(F Wr + b) W, likewise
        self.feat_u = None if user_feat is None else FeatureSide(user_feat, self._pad(U0, dev), self.r, plan.n_users)
        self.relu_u = None if user_relu is None else ReLUSide(self._pad(U0, dev), self.r, plan.n_users, **user_relu)
        own_u = user_feat is None and user_relu is None   # the table is the variable itself
        self.U = self._pad(U0, dev) if own_u else torch.zeros(plan.n_users, self.ld, dtype=torch.float32, device=dev)
        self.bias_u = None if user_bias is None else BiasSide(self.U, user_bias, self.r)
        self.U_nxt = torch.empty_like(self.U) if user_bias is None and own_u else None
        self.feat_v = None if item_feat is None else FeatureSide(item_feat, self._pad(V0, dev), self.r, plan.n_items)
        self.relu_v = None if item_relu is None else ReLUSide(self._pad(V0, dev), self.r, plan.n_items, **item_relu)
        own_v = item_feat is None and item_relu is None
        if V_tables is None:
            self.V = self._pad(V0, dev) if own_v else torch.zeros(plan.n_items, self.ld, dtype=torch.float32, device=dev)
            self.V_nxt = torch.empty_like(self.V) if item_bias is None and own_v else None
        else:
            self.V, self.V_nxt = V_tables
        self.bias_v = None if item_bias is None else BiasSide(self.V, item_bias, self.r)
        self.plan, self.wplan = plan, wplan
        # (user, item): the side object that steps the table after the passes - None = a plain unpenalised side, stepped by the passes'
        # own fused fresh-Adam epilogue into the second buffer (set_l2 puts a PlainL2Side there) - and l2 = 2 alpha of the side
        self.sides = [self.relu_u or self.feat_u or self.bias_u, self.relu_v or self.feat_v or self.bias_v]
        self.l2 = [0.0, 0.0]
        # slab floats whatever the negative table: the interaction lists and the sides' lists; the list passes of a ReLU side run at
        # width aux, so the one slab holds rows of max(ld(r), ld(aux)) floats
        self._slab_fixed = max([max(plan.seg_u.n_slab, plan.seg_i.n_slab if plan.seg_i else 0,
                                    *(f.n_slab for f in (self.feat_u, self.feat_v) if f is not None), 1) * self.ld]
                               + [f.n_slab * f.ld_aux for f in (self.relu_u, self.relu_v) if f is not None])
        need = dict(slab=self._slab_fixed, loss_part=max(plan.seg_u.nseg, plan.n_users, 1))
        need.update(self._adopt_wplan())
        self._need = need
        self._bufs = None   # the scratch buffers where they are this state's own: set_negatives may replace one
        if scratch is None:
            bufs = {k: torch.zeros(v, dtype=torch.float32, device=dev) if k == 'loss_part'
                    else torch.empty(v, dtype=torch.float32, device=dev) for k, v in need.items()}
            self._bind(bufs)
            if V_tables is None:
                self._bufs = bufs
        else:
            scratch.setdefault('states', []).append(self)
        for side, E in ((self.feat_u, self.U), (self.feat_v, self.V)):   # the initial E = F W0 (the slab is bound by now)
            if side is not None:
                feature_forward(side.plan, side.W, E, self.slab, self.r)
        for side, E in ((self.relu_u, self.U), (self.relu_v, self.V)):   # likewise E = relu(F Wr0 + b0) W0
            if side is not None:
                relu_forward(side, E, self.slab)

    def _adopt_wplan(self):
        """Everything the state derives from its WmrbPlan (``self.wplan``; None: nothing): the form of gradU, the one stream plan the
        sliced pass's scores kernel wants (scores_form), the launch sizes and sync words of the row-stationary passes.  -> the scratch
        sizes that depend on the plan
        (``slab`` always; ``sp`` / ``pk`` / ``part`` of the sliced pass).  __init__ and set_negatives both come through here."""
        plan, wplan, dtype, dev = self.plan, self.wplan, self.dtype, self.plan.col_u.device
        need = dict(slab=max(self._slab_fixed,
                             (wplan.seg_e.n_slab if wplan is not None and wplan.seg_e is not None else 0) * self.ld,
                             (wplan.vrows.n_slab if wplan is not None and wplan.vrows is not None else 0) * self.ld))
        self.row_stationary = False
        if wplan is not None and wplan.sliced:
            m, S = wplan.R.shape
            self.row_stationary = wplan.row_stationary   # decided once, where the slices were sized for it (wmrb_plan_for)
            if self.row_stationary is None:
                self.row_stationary = row_stationary_wanted(m, plan.n_items, S, plan.nnz, self.r, dtype)
            self.users_per_launch = int(switch('TMF_G4_USERS', 32768))
            if self.row_stationary:
                nb = _lib.load_library().tmf_wmrb_gradu4_workspace_bytes(m, wplan.n_slices, self.users_per_launch)
                self.g4_sync = torch.zeros(max(nb // 4, 1), dtype=torch.int32, device=dev)
            # gradU partials: one layer per slice, or (above PART_BUDGET bytes) a single layer summed by per-slice launches -
            # eight layers summed by per-round launches when the slices are walked XCD-major
            ns = wplan.n_slices
            if ns * m * self.ld * 4 <= PART_BUDGET:
                self.part_layers, self.gradu_launches = ns, 0          # one launch, a layer per slice
            elif wplan.xcd_major:
                self.part_layers, self.gradu_launches = min(8, ns), 3  # a launch per round of eight slices
            else:
                self.part_layers, self.gradu_launches = 1, 1           # a launch per slice
            need.update(sp=m * S, pk=max(plan.nnz, 1), part=self.part_layers * max(m, 1) * self.ld)
            name, forced = scores_form_of(plan, wplan, self.r, dtype)
            while True:   # the ONE stream plan the answer names; every other slot is emptied
                form = next((f for f in SCORES_FORMS if f.name == name), None)
                for f in SCORES_FORMS:
                    if f is not form:
                        setattr(wplan, f.slot, None)
                try:
                    if form is not None:
                        have = getattr(wplan, form.slot)
                        if have is None or have.key != (self.r, dtype):
                            setattr(wplan, form.slot, form.plan(plan, wplan, self.r, dtype))
                        getattr(wplan, form.slot).ready()
                    break
                except torch.OutOfMemoryError:
                    # a default form whose streams (~10 bytes per entry) do not fit leaves the pass to the rows below it
                    if forced:
                        raise
                    name, forced = scores_form_of(plan, wplan, self.r, dtype, after=name)
        if wplan is not None and wplan.rows4:
            L = _lib.load_library()
            per_group = L.tmf_wsum_rows4_rows_per_group(self.r, int(dtype is torch.bfloat16))
            if not per_group:
                raise ValueError('the row-stationary item pass needs rows of at least 16 lanes')
            cus = torch.cuda.get_device_properties(dev).multi_processor_count if torch.cuda.is_available() else 256
            self.rows4_per_launch = int(switch('TMF_ROWS4_PER_LAUNCH', 2 * cus * per_group))   # two workgroups per CU resident
            n_work = wplan.vrows.n_vrows if wplan.vrows is not None else plan.n_items
            nb = L.tmf_wsum_rows4_workspace_bytes(n_work, wplan.user_chunks, self.rows4_per_launch)
            self.rows4_sync = torch.zeros(max(nb // 4, 1), dtype=torch.int32, device=dev)
        if self.ib is not None:
            self.ib.adopt(wplan)
        return need

    def set_negatives(self, R):
        """Another negative table (int32 [n_users, n_samples], the shape of the one it replaces) for a live state: the WmrbPlan is
        rebuilt by the route that built it (wmrb_plan_for, same force_sliced), with whatever was built on the old one for its loss
        (WmrbPlan.prepared: the sample ranks, the omega buffer - by Loss.prepare, by hand or by an epoch; no epoch after this call
        allocates) and everything derived from it again by _adopt_wplan.  The tables, the side objects, l2, the gradient tables and
        moments of persistent Adam and the InteractionPlan are not touched.  The old plan - its entry lists, score streams, slice
        lists and ranks - is dropped BEFORE the new one is built, so the peak stays that of building the state.  The scalar item bias
        carries over like the tables; its passes read R, rowptr_e, ent_w and wbuf from the plan the state holds when they launch, and
        its chunk tables and workspace are built again for the new lists.  ``sp`` / ``pk`` /
        ``part`` keep their sizes (m, S and nnz do not change); the slab grows when the new lists need more, and the sync words are
        allocated and zeroed again.  A graph captured over this state holds the old plan's pointers: capture after, not across."""
        if self._bufs is None:
            raise NotImplementedError('set_negatives on a state that shares its scratch (scratch= / V_tables=: the mini-batch fit) is '
                                      'not built')
        old = self.wplan
        if old is None or old.route is None:
            raise ValueError('set_negatives needs a state whose WmrbPlan was built by wmrb_plan_for')
        R = torch.as_tensor(R).to(device=self.plan.col_u.device, dtype=torch.int32).contiguous()
        if tuple(R.shape) != tuple(old.R_model.shape):
            raise ValueError(f'the new table has shape {tuple(R.shape)}, the one it replaces {tuple(old.R_model.shape)}')
        route, prepared = old.route, old.prepared
        self.wplan = None
        self.sp = self.pk = self.part = None
        for name in ('g4_sync', 'rows4_sync'):
            self.__dict__.pop(name, None)
        old.release()
        del old
        self.wplan = wmrb_plan_for(self.plan, R, self.r, self.dtype, **route)
        for build, args in prepared:
            getattr(self.wplan, build)(*args)
        need = dict(self._need)
        need.update(self._adopt_wplan())
        if need['slab'] > self._bufs['slab'].numel():
            self._bufs['slab'] = None
            self.slab = None
            self._bufs['slab'] = torch.empty(need['slab'], dtype=torch.float32, device=R.device)
        self._need = need
        self._bind(self._bufs)

    def _bind(self, bufs):
        """Views of the (possibly shared, larger) flat fp32 scratch buffers in this state's shapes."""
        need = self._need
        self.slab = bufs['slab'][:need['slab']].view(-1, self.ld)
        self.loss_part = bufs['loss_part'][:need['loss_part']]
        if 'sp' in need:
            m, S = self.wplan.R.shape
            self.sp = bufs['sp'][:need['sp']].view(m, S)               # sampled scores, R-sorted order
            self.pk = bufs['pk'][:need['pk']]                          # scores of the interactions, CSR order
            self.part = bufs['part'][:need['part']].view(-1, self.ld)

    def _pad(self, W, dev):
        W = torch.as_tensor(W).detach().to(device=dev, dtype=torch.float32)
        out = torch.zeros(W.shape[0], self.ld, dtype=self.dtype, device=dev)
        out[:, :self.r] = W  # bf16: round-to-nearest-even, like the kernels' stores
        return out

    def set_l2(self, user_alpha=0.0, item_alpha=0.0):
        """L2 regularisation alpha ||W||_F^2 of either side's weight matrix (0 = none: nothing changes for that side).  A penalised
        side steps from g' = g + l2 w, l2 = 2 alpha in fp32, by the _l2 twin of its table step; for that it emits its raw gradient
        (TMF_EPI_GRAD) where it ran the fused fresh-Adam epilogue.  A plain side becomes a PlainL2Side: a gradient table in its second
        buffer's place and a step in place (no swap); what a structured side changes is its own set_l2."""
        for k, alpha in enumerate((user_alpha, item_alpha)):
            l2 = ctypes.c_float(2.0 * float(alpha)).value
            if not (0.0 <= l2 < float('inf')):
                raise ValueError(f'alpha={alpha!r} of the {("user", "item")[k]} side is negative or not finite')
            if l2 == 0.0:
                continue
            for side in self.sides:   # a ReLU side refuses it for the side opposite too
                if isinstance(side, ReLUSide):
                    side.set_l2(l2)
            if self.sides[k] is None:
                nxt = ('U_nxt', 'V_nxt')[k]
                if getattr(self, nxt) is None:
                    raise NotImplementedError('L2 regularisation of a table that several states step is not built')
                setattr(self, nxt, None)   # stepped in place from now on: the gradient table takes the second buffer's place
                self.sides[k] = PlainL2Side((self.U, self.V)[k], self.r, self.sfx)
            self.sides[k].set_l2(l2)
            self.l2[k] = l2

    def swap(self):
        if self.U_nxt is not None:
            self.U, self.U_nxt = self.U_nxt, self.U
        if self.V_nxt is not None:
            self.V, self.V_nxt = self.V_nxt, self.V
        if self.ib is not None and self.ib.epi == _lib.EPI_ADAM:
            self.ib.b, self.ib.b_nxt = self.ib.b_nxt, self.ib.b


class BiasSide:
    """One BiasedLinearEmbedding side over indicator features (embedding_graphs.py:41-58): the raw weights W [rows, ld] - kept as
    a table of their own, the reference computes fl(W + b) afresh every epoch -, the bias b [ld] (zeros beyond r), the gradient
    table G the passes fill under TMF_EPI_GRAD, g_b [ld] (the last bias gradient) and the fp64 partial column sums.  ``E`` is the
    TrainState table of the side: it holds the padded W0 on entry and W0 + b0 afterwards."""

    def __init__(self, E, b0, r):
        lib = _lib.get()
        rows, ld = E.shape
        b0 = torch.as_tensor(b0).detach().to(device=E.device, dtype=torch.float32).reshape(-1)
        if b0.numel() != r:
            raise ValueError(f'linear bias of {b0.numel()} elements for n_components={r}')
        self.r = int(r)
        self.l2 = 0.0   # TrainState.set_l2
        self.W = E.clone()
        self.b = torch.zeros(ld, dtype=torch.float32, device=E.device)
        self.b[:r] = b0
        E[:, :r] += self.b[:r]
        self.g_b = torch.zeros(ld, dtype=torch.float32, device=E.device)
        self.G = torch.empty_like(E)
        self.part_rows = int(lib.tmf_bias_colsum_part_rows(rows))
        self.part = torch.empty(self.part_rows, ld, dtype=torch.float64, device=E.device)

    def set_l2(self, l2):
        self.l2 = l2

    def step(self, E, slab, adam, prof=None, tag=''):
        """From the gradient table G (filled by this epoch's pass): column sums -> bias step -> row update, which also rebuilds
        E = W + b in place.  Stream-ordered, nothing allocated, no host scalars: graph-capturable."""
        lib, s = _lib.get(), _lib.stream_ptr()
        rows = E.shape[0]
        _timed(prof, tag + 'bias_colsum', lambda: lib.tmf_bias_colsum_f32(self.G, rows, self.r, self.part, self.part_rows, None, s))
        _timed(prof, tag + 'bias_adam', lambda: lib.tmf_bias_adam_f32(self.part, self.part_rows, self.b, self.g_b, self.r, adam, s))
        if self.l2:   # the weights are penalised, the bias never: its step above saw the raw gradient
            _timed(prof, tag + 'adam_bias_rows_l2', lambda: lib.tmf_adam_bias_rows_l2_f32(self.W, self.G, self.b, E, rows,
                                                                                          self.r, adam, self.l2, s))
            return
        _timed(prof, tag + 'adam_bias_rows', lambda: lib.tmf_adam_bias_rows_f32(self.W, self.G, self.b, E, rows, self.r, adam, s))


class PlainL2Side:
    """A plain side whose table is penalised (TrainState.set_l2): the gradient table G [rows, ld] the passes fill under TMF_EPI_GRAD
    in the second buffer's place, and l2 = 2 alpha in fp32.  The TrainState table of the side is the variable itself."""

    def __init__(self, W, r, sfx):
        self.r, self.sfx, self.l2 = int(r), sfx, 0.0
        self.G = torch.empty(W.shape[0], W.shape[1], dtype=torch.float32, device=W.device)

    def set_l2(self, l2):
        self.l2 = l2

    def step(self, E, slab, adam, prof=None, tag=''):
        """E = fresh-Adam(E, G + l2 E) in place.  Stream-ordered, no host scalars: graph-capturable."""
        lib, s = _lib.get(), _lib.stream_ptr()
        step = getattr(lib, 'tmf_adam_fresh_rows_l2' + self.sfx)
        _timed(prof, tag + 'adam_rows_l2', lambda: step(E, self.G, E.shape[0], self.r, adam, self.l2, s))


class FeatureSide:
    """One LinearEmbedding side over sparse features F [rows, n_features] (embedding_graphs.py:30-38): the list views of F - an
    InteractionPlan over its entries, CSR by row for E = F W and CSC by feature for dW = F^T G, heavy lists cut into segments -,
    the weights W [n_features, ld] with their second buffer and the gradient table G [rows, ld] the passes fill under
    TMF_EPI_GRAD.  The TrainState table of the side is the effective table E, rebuilt every epoch.
    F: anything with .indices [nnz, 2] (row, feature), .values [nnz] and .shape (mf.sparse.SparseFeatures); W0: padded weights."""

    def __init__(self, F, W0, r, n_rows, chunk=DEFAULT_CHUNK):
        rows, n_features = (int(d) for d in F.shape)
        if rows != n_rows or tuple(W0.shape[:1]) != (n_features,):
            raise ValueError(f'features of shape {(rows, n_features)} for {n_rows} rows and weights of {W0.shape[0]} rows')
        dev = W0.device
        self.r = int(r)
        self.plan = InteractionPlan(F.indices.to(dev), F.values.to(dev), rows, n_features, chunk=chunk, csc=True)
        self.n_slab = max(self.plan.seg_u.n_slab, self.plan.seg_i.n_slab)
        self.W, self.W_nxt = W0, torch.empty_like(W0)
        self.G = torch.empty(rows, W0.shape[1], dtype=torch.float32, device=dev)
        self.l2, self.GW = 0.0, None   # set_l2: l2 > 0 = the weights step in place from GW [n_features, ld] (no W_nxt)

    def set_l2(self, l2):
        self.l2, self.GW, self.W_nxt = l2, torch.empty_like(self.W), None

    def step(self, E, slab, adam, prof=None, tag=''):
        """The step of the weights from G (filled by this epoch's pass), then the rebuilt E = F W."""
        _timed(prof, tag + 'feat_backward', lambda: self._backward(slab, adam))
        _timed(prof, tag + 'feat_forward', lambda: feature_forward(self.plan, self.W, E, slab, self.r))

    def _backward(self, slab, adam):
        """W_nxt[f] = fresh_adam(W[f], sum_i x_if G[i]) over the CSC lists (a feature no row carries keeps its weights), then the swap.
        With penalised weights (l2 > 0): the sums as a table of their own, then the regularised step in place and no swap."""
        lib, s, p = _lib.get(), _lib.stream_ptr(), self.plan
        if self.l2:
            # penalised weights: dW = F^T G into GW (a feature no row carries gets a zero row), then W = fresh-Adam(W, dW + l2 W) in
            # place over EVERY feature - one no row carries decays, its penalty gradient is not zero
            _lib.check(lib.tmf_feat_pass_f32(p.seg_i.cstruct(), p.row_i, p.val_i, self.G, None, self.GW, slab,
                                             self.r, _lib.EPI_GRAD, adam, s), lib)
            _row_pass_finish(lib, p.seg_i, slab, None, self.GW, self.r, _lib.EPI_GRAD, adam, s)
            _lib.check(lib.tmf_adam_fresh_rows_l2_f32(self.W, self.GW, self.W.shape[0], self.r, adam, self.l2, s), lib)
            return
        _lib.check(lib.tmf_feat_pass_f32(p.seg_i.cstruct(), p.row_i, p.val_i, self.G, self.W, self.W_nxt, slab,
                                         self.r, _lib.EPI_ADAM, adam, s), lib)
        _row_pass_finish(lib, p.seg_i, slab, self.W, self.W_nxt, self.r, _lib.EPI_ADAM, adam, s)
        self.W, self.W_nxt = self.W_nxt, self.W


def feature_forward(plan, W, E, slab, r):
    """E = F W over the CSR lists of ``plan`` (every row of E is written; a row without entries becomes zeros)."""
    lib, s = _lib.get(), _lib.stream_ptr()
    adam = lib.tmf_adam_fresh(0.0)   # unused by the GRAD epilogue
    _lib.check(lib.tmf_feat_pass_f32(plan.seg_u.cstruct(), plan.col_u, plan.val_u, W, None, E, slab, r,
                                     _lib.EPI_GRAD, adam, s), lib)
    _row_pass_finish(lib, plan.seg_u, slab, None, E, r, _lib.EPI_GRAD, adam, s)


def embed_features(F, W, r, chunk=DEFAULT_CHUNK):
    """F W [rows, ld] for padded weights W [n_features, ld] on the GPU: the forward pass over a plan built for F alone."""
    if F.nnz == 0:
        return torch.zeros(int(F.shape[0]), W.shape[1], dtype=torch.float32, device=W.device)
    plan = InteractionPlan(F.indices.to(W.device), F.values.to(W.device), int(F.shape[0]), int(F.shape[1]), chunk=chunk, csc=False)
    E = torch.empty(plan.n_users, W.shape[1], dtype=torch.float32, device=W.device)
    slab = torch.empty(max(plan.seg_u.n_slab, 1), W.shape[1], dtype=torch.float32, device=W.device)
    feature_forward(plan, W, E, slab, r)
    return E


class ReLUSide:
    """One ReLUEmbedding side (embedding_graphs.py:61-87), E = relu(F Wr + b) W with the hidden width aux = 5 r: a FeatureSide-like
    plan over the entries of F (CSR by row for Z = F Wr, CSC by feature for dWr = F^T dZ) - indicator features are the identity
    lists, one entry per row, no dense matrix -, the hidden weights Wr [n_features, ld(aux)] and the output weights W [aux, ld(r)],
    each with its second buffer, the hidden bias b [ld(aux)], the pre-activations Z and their gradient dZ [rows, ld(aux)], the
    gradient table G [rows, ld(r)] the passes fill under TMF_EPI_GRAD, and the partial sums of the W and b steps.  The hidden
    values are never stored.  The TrainState table of the side is the effective table E, rebuilt every epoch.
    W0: padded output weights; F: None (indicator features) or anything FeatureSide takes; Wr0 [n_features, aux]; b0 [aux]."""

    def __init__(self, W0, r, n_rows, F=None, Wr0=None, b0=None, chunk=DEFAULT_CHUNK):
        lib, dev = _lib.load_library(), W0.device
        self.r, self.aux, self.rows = int(r), int(W0.shape[0]), int(n_rows)
        self.ld_aux = _lib.padded_ld(self.aux)
        if F is None:
            own = torch.arange(self.rows, dtype=torch.int64, device=dev)
            indices, values, n_features = torch.stack([own, own], 1), torch.ones(self.rows, dtype=torch.float32, device=dev), self.rows
        else:
            rows, n_features = (int(d) for d in F.shape)
            if rows != self.rows:
                raise ValueError(f'features of shape {(rows, n_features)} for {n_rows} rows')
            indices, values = F.indices.to(dev), F.values.to(dev)
        self.n_features = n_features
        Wr0 = torch.as_tensor(Wr0).detach().to(device=dev, dtype=torch.float32)
        b0 = torch.as_tensor(b0).detach().to(device=dev, dtype=torch.float32).reshape(-1)
        if tuple(Wr0.shape) != (n_features, self.aux) or b0.numel() != self.aux:
            raise ValueError(f'relu_weight of shape {tuple(Wr0.shape)} and relu_bias of {b0.numel()} elements for {n_features} '
                             f'features and aux width {self.aux}')
        self.plan = InteractionPlan(indices, values, self.rows, n_features, chunk=chunk, csc=True)
        self.n_slab = max(self.plan.seg_u.n_slab, self.plan.seg_i.n_slab)
        f32 = dict(dtype=torch.float32, device=dev)
        self.W, self.W_nxt = W0, torch.empty_like(W0)
        self.Wr = torch.zeros(n_features, self.ld_aux, **f32)
        self.Wr[:, :self.aux] = Wr0
        self.Wr_nxt = torch.empty_like(self.Wr)
        self.b = torch.zeros(self.ld_aux, **f32)
        self.b[:self.aux] = b0
        self.g_b = torch.zeros(self.ld_aux, **f32)
        self.Z = torch.empty(self.rows, self.ld_aux, **f32)
        self.dZ = torch.empty(self.rows, self.ld_aux, **f32)
        self.G = torch.empty(self.rows, W0.shape[1], **f32)
        self.part_rows = int(lib.tmf_relu_part_rows(self.rows))
        self.part = torch.empty(max(self.part_rows, 1), self.aux, W0.shape[1], **f32)
        self.bias_part_rows = int(lib.tmf_bias_colsum_part_rows(self.rows))
        self.bias_part = torch.empty(self.bias_part_rows, self.ld_aux, dtype=torch.float64, device=dev)

    def set_l2(self, l2):
        raise NotImplementedError('L2 regularisation next to a ReLU side on the engine is not built')

    def step(self, E, slab, adam, prof=None, tag=''):
        """From the gradient table G (filled by this epoch's pass).  Every read of the pre-update W and b comes before their steps:
        the partials of dW = H^T G and dZ = (G W^T) . mask first, then W, then b from the column sums of dZ, then Wr from F^T dZ
        over the CSC lists (a feature no row carries keeps its weights); last the rebuilt Z = F Wr and E = relu(Z + b) W.
        Stream-ordered, nothing allocated, no host scalars, no atomics: graph-capturable and bit-reproducible."""
        lib, s, p = _lib.get(), _lib.stream_ptr(), self.plan
        rows, aux, r = self.rows, self.aux, self.r
        _timed(prof, tag + 'relu_dweights', lambda: lib.tmf_relu_dweights_f32(self.Z, self.b, self.G, self.part,
                                                                              self.part_rows, rows, aux, r, s))
        _timed(prof, tag + 'relu_dhidden', lambda: lib.tmf_relu_dhidden_f32(self.G, self.W, self.Z, self.b, self.dZ,
                                                                            rows, aux, r, s))
        _timed(prof, tag + 'relu_adam_weights', lambda: lib.tmf_relu_adam_weights_f32(self.part, self.part_rows, self.W,
                                                                                      self.W_nxt, None, aux, r, adam, s))
        self.W, self.W_nxt = self.W_nxt, self.W
        _timed(prof, tag + 'relu_bias_colsum', lambda: lib.tmf_bias_colsum_f32(self.dZ, rows, aux, self.bias_part,
                                                                               self.bias_part_rows, None, s))
        _timed(prof, tag + 'relu_bias_adam', lambda: lib.tmf_bias_adam_f32(self.bias_part, self.bias_part_rows, self.b,
                                                                           self.g_b, aux, adam, s))

        def hidden_backward():
            _lib.check(lib.tmf_feat_pass_f32(p.seg_i.cstruct(), p.row_i, p.val_i, self.dZ, self.Wr, self.Wr_nxt,
                                             slab, aux, _lib.EPI_ADAM, adam, s), lib)
            _row_pass_finish(lib, p.seg_i, slab, self.Wr, self.Wr_nxt, aux, _lib.EPI_ADAM, adam, s)
            self.Wr, self.Wr_nxt = self.Wr_nxt, self.Wr
        _timed(prof, tag + 'relu_feat_backward', hidden_backward)
        relu_forward(self, E, slab, prof, tag)


def relu_forward(side, E, slab, prof=None, tag=''):
    """E = relu(F Wr + b) W from the side's current variables: the pre-activations over the CSR lists, then tmf_relu_embed_f32."""
    lib, s = _lib.get(), _lib.stream_ptr()
    _timed(prof, tag + 'relu_feat_forward', lambda: feature_forward(side.plan, side.Wr, side.Z, slab, side.aux))
    _timed(prof, tag + 'relu_embed', lambda: lib.tmf_relu_embed_f32(side.Z, side.b, side.W, E, side.rows, side.aux,
                                                                    side.r, s))


def embed_relu(F, side, chunk=DEFAULT_CHUNK):
    """relu(F Wr + b) W [rows, ld] for the variables of a trained ReLUSide on the GPU: the two forward kernels over a plan built for
    F alone - for the rows the fit saw, bit for bit the table it left."""
    lib, s = _lib.get(), _lib.stream_ptr()
    rows, dev = int(F.shape[0]), side.W.device
    Z = embed_features(F, side.Wr, side.aux, chunk)
    E = torch.empty(rows, side.W.shape[1], dtype=torch.float32, device=dev)
    _lib.check(lib.tmf_relu_embed_f32(Z, side.b, side.W, E, rows, side.aux, side.r, s), lib)
    return E


def epoch_sides(st, adam, loss_out, loss='mse', c=0.0, prof=None):
    """One epoch of a state, whatever its sides (TrainState.sides): the loss's own epoch on the effective tables, every side that is
    an object emitting its raw gradient into its G (TMF_EPI_GRAD) where a plain unpenalised one keeps the fused fresh-Adam epilogue
    into its second buffer; then, user side first, the step of every such side (both passes have read the pre-update tables by
    then) and the swap of the others.
    Stream-ordered, nothing allocated, no host reads, no atomics: graph-capturable and bit-reproducible."""
    (ue, uo), (ie, io) = [(_lib.EPI_ADAM, None) if side is None else (_lib.EPI_GRAD, side.G) for side in st.sides]
    run_epoch(st, adam, loss_out, loss, c, ie, io, prof, ue, uo)
    for side, E, tag in zip(st.sides, (st.U, st.V), ('user_', 'item_')):
        if side is not None:
            side.step(E, st.slab, adam, prof, tag)
    st.swap()


def share_scratch(scratch, dev):
    """Allocate the per-step buffers of the states registered in ``scratch`` once, at the largest size any of them needs."""
    states = scratch.get('states', [])
    sizes = {}
    for st in states:
        for k, v in st._need.items():
            sizes[k] = max(sizes.get(k, 0), v)
    bufs = {k: torch.zeros(v, dtype=torch.float32, device=dev) for k, v in sizes.items()}
    for st in states:
        st._bind(bufs)
    return bufs


class KernelTimer:
    """HIP-event brackets around named launches on the current stream (bench.py uses it to get the
    dominant kernel's own duration inside the timed region)."""

    def __init__(self):
        self.spans = {}

    def start(self, name):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.spans.setdefault(name, []).append([ev, None])

    def stop(self, name):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.spans[name][-1][1] = ev

    def mean_ms(self, name):
        v = [a.elapsed_time(b) for a, b in self.spans.get(name, []) if b is not None]
        return sum(v) / len(v) if v else float('nan')


def _timed(prof, name, call):
    """call() as the span ``name`` of ``prof`` (a KernelTimer, or None).  A launch returns its code, which is checked here; a
    sequence of launches that checks its own returns None."""
    if prof:
        prof.start(name)
    rc = call()
    if rc is not None:
        _lib.check(rc)
    if prof:
        prof.stop(name)


FULL_SOFTMAX_MAX_COMPONENTS = 128   # tmf_fsm_max_components: the widest table csrc/tmf_fullsoftmax.hip sweeps (fp32 only)


def loss_name(loss_graph):
    """The LOSSES name of a fit's loss, for exactly the built-in loss classes (not their subclasses: what a subclass computes is its
    own business, and the generic path's).  Anything else raises - no loss trains as another one because a test fell through."""
    for rec in LOSSES.values():
        if rec.cls is type(loss_graph) and (rec.weighted is None or rec.weighted == bool(loss_graph.weighted)):
            return rec.name
    raise TypeError(f'{type(loss_graph).__name__} is not a loss the HIP engine trains '
                    f'({", ".join(dict.fromkeys(rec.kind for rec in LOSSES.values()))})')


def form_loss(model, form, optimizer_text):
    """loss_name at the door of a fit that is a form of its own (``form``: 'mini-batch', 'multi-GPU'): such a fit steps by the
    reference's fresh Adam only (ValueError(optimizer_text)) and has no loss whose moments are global (KLDivergenceLoss)."""
    if getattr(model, 'optimizer', 'fresh_adam') != 'fresh_adam':
        raise ValueError(optimizer_text)
    loss = loss_name(model.loss_graph)
    if LOSSES[loss].global_moments:
        raise ValueError(f'{LOSSES[loss].kind} has no {form} form (its moments are global)')
    return loss


def checked_negatives(random_ind, n_rows, n_items, device, rows=None):
    """The negative table as a WmrbPlan reads it - int32, contiguous, on ``device`` - once it is [n_rows, n_samples] (ValueError) with
    ids in [0, n_items) (IndexError).  rows = (b, e): only that block of rows is moved and range-checked (a rank's users)."""
    R = torch.as_tensor(random_ind)
    if R.dim() != 2 or R.shape[0] != n_rows:
        raise ValueError(f'random_ind has shape {tuple(R.shape)}, expected [{n_rows}, n_samples]')
    if rows is not None:
        R = R[rows[0]:rows[1]]
    R = R.to(device=device, dtype=torch.int32).contiguous()
    if R.numel() and (int(R.min()) < 0 or int(R.max()) >= n_items):
        raise IndexError('random_ind holds item ids outside [0, n_items)')
    return R


def run_epoch(st, adam, loss_out, loss, c=0.0, item_epi=_lib.EPI_ADAM, item_out=None, prof=None, user_epi=_lib.EPI_ADAM,
              user_out=None):
    """One epoch of ``loss`` - a name of LOSSES, c = what its record's ``param`` gives for the model - on the state's tables: the ONE
    place that maps a loss to its epoch.  The other arguments as in epoch_mse.  A sliced-only loss is an epoch only of a state whose
    WmrbPlan is sliced (wmrb_plan_for(force_sliced=True)), a 'catalog' loss only of one built with full_softmax=True.  On any other
    state they are refused like a name nobody knows - never run as WMRB."""
    rec = LOSSES.get(loss)
    unsliced = rec is not None and rec.sliced_only and not getattr(getattr(st, 'wplan', None), 'sliced', False)
    unswept = rec is not None and rec.family == 'catalog' and getattr(st, 'fsm_lse', None) is None
    if rec is None or unsliced or unswept:
        raise ValueError(f'run_epoch: unknown loss {loss!r}' + ' on a state without a sliced WmrbPlan' * unsliced
                         + ' on a state built without full_softmax=True' * unswept)
    tail = (item_epi, item_out, prof, user_epi, user_out)
    if rec.table:
        return rec.epoch(st, adam, c, loss_out, *tail, pairs=rec.pairs)
    rec.epoch(st, adam, loss_out, *(() if rec.weighted is None else (rec.weighted,)), *tail)


def _row_pass_finish(lib, seg, slab, X_old, X_out, r, epi, adam, stream, sfx='_f32'):
    if seg.n_long:
        _lib.check(getattr(lib, 'tmf_combine_rows' + sfx)(seg.long_rows, seg.long_slab_beg, seg.n_long,
                                            slab, X_old, X_out, r, epi, adam, stream), lib)


def _list_passes(st, adam, entry, span, user_slot, item_slot, tail, loss_out, item_epi, item_out, prof, user_epi, user_out):
    """The two list passes of the pointwise losses, both reading the pre-update tables: the user pass over the CSR lists, then the
    item pass over the CSC lists, each finished by tmf_combine_rows for the cut rows.  entry: the pass's entry point (+ the
    state's type suffix); span: prefix of the two span names; user_slot / item_slot: what the pass gets in its loss_part argument
    (None: nothing to write); tail: its arguments behind ``adam``; loss_out: where the user pass's per-segment loss sums (the
    state's loss_part) are added up, None = they are not."""
    lib, p, r, s = _lib.get(), st.plan, st.r, _lib.stream_ptr()
    run = getattr(lib, entry + st.sfx)
    U_out = st.U_nxt if user_out is None else user_out
    _timed(prof, span + '_user_pass', lambda: run(p.seg_u.cstruct(), p.col_u, p.val_u, st.U, st.V, U_out, st.slab,
                                                  user_slot, r, user_epi, adam, *tail, s))
    _row_pass_finish(lib, p.seg_u, st.slab, st.U, U_out, r, user_epi, adam, s, st.sfx)
    if loss_out is not None:
        _lib.check(lib.tmf_sum_f32(st.loss_part, p.seg_u.nseg, loss_out, s), lib)
    V_out = st.V_nxt if item_out is None else item_out
    _timed(prof, span + '_item_pass', lambda: run(p.seg_i.cstruct(), p.row_i, p.val_i, st.V, st.U, V_out, st.slab,
                                                  item_slot, r, item_epi, adam, *tail, s))
    _row_pass_finish(lib, p.seg_i, st.slab, st.V, V_out, r, item_epi, adam, s, st.sfx)


def epoch_mse(st, adam, loss_out, item_epi=_lib.EPI_ADAM, item_out=None, prof=None, user_epi=_lib.EPI_ADAM, user_out=None):
    """One MSE epoch: user pass (+loss), item pass; both read the pre-update tables.
    loss_out: 1-element fp64 device tensor receiving sum_k (a_k - p_k)^2.
    item_epi / user_epi = EPI_GRAD write the raw fp32 gradient into item_out / user_out instead of the updated table
    (multi-GPU; optimisers other than the reference's)."""
    _list_passes(st, adam, 'tmf_mse_pass', 'mse', st.loss_part, None, (), loss_out, item_epi, item_out, prof, user_epi, user_out)


def epoch_logistic(st, adam, loss_out, weighted=False, item_epi=_lib.EPI_ADAM, item_out=None, prof=None, user_epi=_lib.EPI_ADAM,
                   user_out=None):
    """One LogisticLoss epoch: epoch_mse with tmf_logistic_pass in place of tmf_mse_pass - user pass (+loss), item pass (no
    loss, no logarithm); both read the pre-update tables.  loss_out receives sum_k w_k log(1 + exp(-y_k p_k)), y_k = +1 where the
    stored value is > 0, else -1, w_k = |value| if ``weighted`` else 1.  item_epi / user_epi as in epoch_mse."""
    _list_passes(st, adam, 'tmf_logistic_pass', 'logistic', st.loss_part, None, (int(bool(weighted)),), loss_out, item_epi, item_out,
                 prof, user_epi, user_out)


def epoch_kl(st, adam, loss_out, item_epi=_lib.EPI_ADAM, item_out=None, prof=None, user_epi=_lib.EPI_ADAM, user_out=None):
    """One KLDivergenceLoss epoch (st built with kl=True): moments of the stored scores -> loss and coefficients -> user pass ->
    item pass; everything reads the pre-update tables and nothing comes back to the host.
    loss_out: 1-element fp64 device tensor receiving the epoch's loss (a scalar).  item_epi / user_epi as in epoch_mse."""
    lib, p, r = _lib.get(), st.plan, st.r
    s = _lib.stream_ptr()
    _timed(prof, 'kl_moments', lambda: getattr(lib, 'tmf_kl_moments' + st.sfx)(
        p.seg_u.cstruct(), p.col_u, p.val_u, st.U, st.V, st.kl_part, r, s))
    _timed(prof, 'kl_coeffs', lambda: lib.tmf_kl_coeffs(st.kl_part, p.seg_u.nseg, loss_out, st.kl_coef, s))
    _list_passes(st, adam, 'tmf_kl_pass', 'kl', st.kl_coef, st.kl_coef, (), None, item_epi, item_out, prof, user_epi, user_out)


def epoch_full_softmax(st, adam, loss_out, item_epi=_lib.EPI_ADAM, item_out=None, prof=None, user_epi=_lib.EPI_ADAM, user_out=None):
    """One FullSoftmaxLoss epoch (st built with full_softmax=True; csrc/tmf_fullsoftmax.hip): lse of every user over the whole catalog
    -> the positives' term of both gradients over the interaction lists (the user pass also sums lse_u - p_k: the loss) -> the two
    sweeps that add n_u pi_ui V[i] to G_U and n_u pi_ui U[u] to G_V -> the steps.  Everything reads the pre-update tables.
    loss_out: 1-element fp64 device tensor receiving sum over positives of (lse_u - p_k).
    Both sides always form their raw gradient table.  item_epi / user_epi = EPI_GRAD: that table is item_out / user_out and nothing is
    stepped here (the sides, L2, persistent Adam).  EPI_ADAM: the gradient takes the second buffer's place, the table steps in place from
    it (tmf_adam_fresh_rows_f32) and the two names change hands, so that the caller's swap() leaves the stepped table in U / V as after
    any other epoch - the same two buffers every epoch, whatever the number of epochs captured.
    Stream-ordered, nothing allocated, no host reads, no atomics: graph-capturable and bit-reproducible."""
    lib, p, r, s = _lib.get(), st.plan, st.r, _lib.stream_ptr()
    m, n, ld = p.n_users, p.n_items, st.ld
    for epi, out, nxt in ((user_epi, user_out, st.U_nxt), (item_epi, item_out, st.V_nxt)):
        if epi not in (_lib.EPI_ADAM, _lib.EPI_GRAD) or (epi == _lib.EPI_ADAM) != (out is None) or (out is None and nxt is None):
            raise ValueError('epoch_full_softmax: EPI_GRAD with the gradient table to fill, or EPI_ADAM without one on a side that has '
                             'its second buffer')
    G_U = st.U_nxt if user_out is None else user_out
    G_V = st.V_nxt if item_out is None else item_out
    _timed(prof, 'fsm_lse', lambda: lib.tmf_fsm_lse_f32(st.U, st.V, m, n, r, ld, ld, st.fsm_lse, s))
    _timed(prof, 'fsm_user_pass', lambda: lib.tmf_fsm_pos_pass_f32(p.seg_u.cstruct(), p.col_u, p.val_u, st.U, st.V, G_U,
                                                                   st.slab, st.fsm_lse, st.loss_part, r, s))
    _row_pass_finish(lib, p.seg_u, st.slab, st.U, G_U, r, _lib.EPI_GRAD, adam, s)
    _lib.check(lib.tmf_sum_f32(st.loss_part, p.seg_u.nseg, loss_out, s), lib)
    _timed(prof, 'fsm_item_pass', lambda: lib.tmf_fsm_pos_pass_f32(p.seg_i.cstruct(), p.row_i, p.val_i, st.V, st.U, G_V,
                                                                   st.slab, None, None, r, s))
    _row_pass_finish(lib, p.seg_i, st.slab, st.V, G_V, r, _lib.EPI_GRAD, adam, s)
    _timed(prof, 'fsm_wsum_user', lambda: lib.tmf_fsm_wsum_f32(st.U, st.V, m, n, r, ld, ld, st.fsm_lse, st.fsm_w, 1, G_U,
                                                               G_U.shape[1], s))
    _timed(prof, 'fsm_wsum_item', lambda: lib.tmf_fsm_wsum_f32(st.V, st.U, n, m, r, ld, ld, st.fsm_lse, st.fsm_w, 0, G_V,
                                                               G_V.shape[1], s))
    if user_epi == _lib.EPI_ADAM:
        _timed(prof, 'fsm_user_step', lambda: lib.tmf_adam_fresh_rows_f32(st.U, G_U, m, r, adam, s))
        st.U, st.U_nxt = st.U_nxt, st.U
    if item_epi == _lib.EPI_ADAM:
        _timed(prof, 'fsm_item_step', lambda: lib.tmf_adam_fresh_rows_f32(st.V, G_V, n, r, adam, s))
        st.V, st.V_nxt = st.V_nxt, st.V


# The pair steps of the sliced user pass: from the scores just computed - pk of the interactions, sp of the negatives, in the plan's order
# (every user's negatives sorted by item) - to the weights delta / D in the same layout and every user's loss in loss_part, whose sum over
# the positives epoch_wmrb leaves in loss_out.  step(lib, st, c, prof, head, tail): c = the loss's parameter (LOSSES), head = (rowptr_u,
# val_u, pk, sp) and tail = (delta, D, loss_part, hinge_order, stream) open and close every launch.
def hinge_pairs(lib, st, c, prof, head, tail):
    """WMRBLoss (csrc/tmf_hinge.hip), c = n_items / n_samples: log(1 + M_k) per positive.  The step the one-kernel user pass has built in."""
    _timed(prof, 'wmrb_hinge', lambda: lib.tmf_wmrb_hinge2_ordered(*head, st.plan.n_users, st.wplan.S, c, *tail))


def bpr_pairs(lib, st, c, prof, head, tail):
    """BPRLoss (csrc/tmf_bpr.hip), the hinge kernel's arguments but c: mean_s softplus(sp[u, s] - p_k) per positive."""
    _timed(prof, 'bpr_pairs', lambda: lib.tmf_bpr_pairs(*head, st.plan.n_users, st.wplan.S, *tail))


def warp_pairs(lib, st, c, prof, head, tail):
    """WARPLoss (csrc/tmf_warp.hip), c unused: w_k (1 - p_k + sp[u, s*_k]) per positive, s*_k its first violator.  Takes the plan's
    n_items (the weight's rank estimate) and WmrbPlan.sample_rank(): the losses of this kind depend on the order of a user's samples
    and try them in the model's table order, whatever order the plan keeps them in."""
    p, rank = st.plan, st.wplan.sample_rank()
    _timed(prof, 'warp_pairs', lambda: lib.tmf_warp_pairs_ranked(*head, rank, p.n_users, st.wplan.S, p.n_items, *tail))


def kos_pairs(lib, st, c, prof, head, tail):
    """KOSWARPLoss, c = (k, n): two steps.  tmf_kos_weights (csrc/tmf_kos.hip) ranks every user's positives by pk and leaves in
    WmrbPlan.kos_omega() the probability omega_k that the k-th best of n draws from them is this one; tmf_warp_pairs_kos is the ranked
    WARP step with those weights: omega_k w_k (1 - p_k + sp[u, s*_k]) per positive."""
    p, w = st.plan, st.wplan
    rank, omega = w.sample_rank(), w.kos_omega(p.nnz)
    _timed(prof, 'kos_weights', lambda: lib.tmf_kos_weights(p.rowptr_u, p.val_u, st.pk, p.n_users, *c, omega, w.hinge_order,
                                                            _lib.stream_ptr()))
    _timed(prof, 'warp_pairs', lambda: lib.tmf_warp_pairs_kos(*head, rank, omega, p.n_users, w.S, p.n_items, *tail))


def softmax_pairs(lib, st, c, prof, head, tail):
    """SampledSoftmaxLoss (csrc/tmf_softmax.hip), the hinge kernel's arguments, c = 1 or n_items / n_samples:
    -log(exp(p_k) / (exp(p_k) + c sum_s exp(sp[u, s]))) per positive.  No dependence on the order of a user's samples.
    A plan with logQ offsets (WmrbPlan.slot_offsets: sampling_correction='logq' on tables drawn by popularity) takes the same step on
    sp - off, with c = 1: the form is chosen from the state, as the bias passes are from st.ib."""
    off = st.wplan.off
    if off is not None:
        _timed(prof, 'softmax_pairs', lambda: lib.tmf_softmax_pairs_offset(*head, off, st.plan.n_users, st.wplan.S, 1.0, *tail))
        return
    _timed(prof, 'softmax_pairs', lambda: lib.tmf_softmax_pairs(*head, st.plan.n_users, st.wplan.S, c, *tail))


def _wmrb_user_pass_sliced(lib, st, adam, c, prof=None, user_epi=_lib.EPI_ADAM, U_out=None, pairs='hinge'):
    """Sliced user pass: scores -> the pair step PAIRS[pairs] -> gradU (+ weights into entry order) -> finish (csrc/tmf_wmrb.hip).
    A state with a scalar item bias (TrainState.ib) adds b to the scores behind the scores kernel and takes b's gradient and step
    behind the pair step (csrc/tmf_itembias.hip); without one, not a launch more."""
    p, w, r = st.plan, st.wplan, st.r
    m, s = p.n_users, _lib.stream_ptr()
    lists = w.lists(p)
    stream = w.s7 or w.s6 or w.s5   # the state's one stream plan (TrainState._adopt_wplan), else a visit per (user, slice)
    _timed(prof, 'wmrb_scores', (lambda: stream.scores(lib, st)) if stream is not None else
           lambda: getattr(lib, 'tmf_wmrb_scores3' + st.sfx)(lists, st.U, st.V, st.sp, st.pk, r, s))
    ib = st.ib
    if ib is not None:   # the scalar item bias, into the scores before any pair step reads them (tmf_kos_weights ranks positives by pk)
        _timed(prof, 'item_bias_add', lambda: lib.tmf_item_bias_add(ib.b, p.n_items, w.R, m, w.S, st.sp, p.col_u, p.nnz, st.pk, s))
    PAIRS[pairs].pair_step(lib, st, c, prof, (p.rowptr_u, p.val_u, st.pk, st.sp), (w.delta, w.D, st.loss_part, w.hinge_order, s))
    if ib is not None:   # its gradient: every item the sum of the weights of its list entries, and the step (or, EPI_GRAD, the gradient)
        _timed(prof, 'item_bias_grad', lambda: lib.tmf_item_bias_grad(
            w.rowptr_e, p.n_items, w.user_chunks, w.ent_w, w.wbuf, ib.chunk, ib.xrow, ib.xchunk, ib.xptr, ib.n_extra,
            ib.b, ib.b_nxt, ib.epi, adam, ib.ws, ib.ws.numel() * 8, s))
    if st.row_stationary:
        # gradU + finish in one row-stationary kernel (lane groups own users and walk the slices; no partial rows)
        _timed(prof, 'wmrb_gradu', lambda: getattr(lib, 'tmf_wmrb_gradu4' + st.sfx)(
            lists, w.D, w.delta, st.V, st.U, st.U_nxt if U_out is None else U_out,
            r, user_epi, adam, st.users_per_launch, st.g4_sync, st.g4_sync.numel() * 4, s))
        return
    _timed(prof, 'wmrb_gradu', lambda: getattr(lib, 'tmf_wmrb_gradu3' + st.sfx)(
        lists, w.D, w.delta, st.V, st.part,
        st.gradu_launches, r, s))
    _timed(prof, 'wmrb_finish', lambda: getattr(lib, 'tmf_wmrb_finish' + st.sfx)(st.part, st.part_layers, m,
                                                                          st.U, st.U_nxt if U_out is None else U_out,
                                                                          r, user_epi, adam, s))


def epoch_wmrb(st, adam, c, loss_out, item_epi=_lib.EPI_ADAM, item_out=None, prof=None, user_epi=_lib.EPI_ADAM, user_out=None,
               pairs='hinge'):
    """One epoch of a loss over the static negative table: the same scores, gathers and item pass around the pair step ``pairs`` (a key of
    PAIRS; 'hinge' = one WMRB epoch), c = that loss's parameter.  loss_out receives the sum over positives of what the pair step's
    function states.  Every pair step but the hinge exists only on a sliced plan.  item_epi / user_epi as in epoch_mse."""
    if pairs not in PAIRS:
        raise ValueError(f'epoch_wmrb: pairs={pairs!r} ({", ".join(list(PAIRS)[:-1])} or {list(PAIRS)[-1]})')
    if PAIRS[pairs].sliced_only and not st.wplan.sliced:
        raise ValueError(f'epoch_wmrb: pairs={pairs} needs the sliced user pass (wmrb_plan_for(force_sliced=True))')
    lib, p, w, r = _lib.get(), st.plan, st.wplan, st.r
    s = _lib.stream_ptr()
    if w.sliced:
        _timed(prof, 'wmrb_user_pass', lambda: _wmrb_user_pass_sliced(lib, st, adam, c, prof, user_epi, user_out, pairs))
    else:
        _timed(prof, 'wmrb_user_pass', lambda: getattr(lib, 'tmf_wmrb_user_pass' + st.sfx)(
            p.rowptr_u, p.col_u, p.val_u, w.R, p.n_users, w.S, c, st.U, st.V,
            st.U_nxt if user_out is None else user_out, w.delta, w.D, st.loss_part, None,
            r, user_epi, adam, s))
    _lib.check(lib.tmf_sum_f32(st.loss_part, p.n_users, loss_out, s), lib)
    V_out = st.V_nxt if item_out is None else item_out
    v = w.vrows
    if not w.rows4:
        _timed(prof, 'wmrb_item_pass', lambda: getattr(lib, 'tmf_wsum_pass' + st.sfx)(
            w.seg_e.cstruct(), w.ent_row, w.ent_w, w.wbuf, st.U, st.V, V_out,
            st.slab, r, item_epi, adam, s))
        _timed(prof, 'wmrb_combine', lambda: _row_pass_finish(lib, w.seg_e, st.slab, st.V, V_out, r, item_epi, adam, s, st.sfx))
    elif v is not None:
        # row-stationary item pass: lane groups own (virtual) rows and walk the user blocks; no slab but for the parts of cut rows
        _timed(prof, 'wmrb_item_pass', lambda: getattr(lib, 'tmf_wsum_rows5' + st.sfx)(
            w.rowptr_e, p.n_items, w.user_chunks, w.ent_row, w.ent_w, w.wbuf, st.U,
            st.V, V_out, st.slab, v.item, v.part, v.nparts, v.slot,
            v.n_vrows, r, item_epi, adam, st.rows4_per_launch, st.rows4_sync, st.rows4_sync.numel() * 4, s))
        if v.n_long:   # the cut rows: their parts' slab slots summed in part order (VirtualRows has a SegmentTable's long-row fields)
            _timed(prof, 'wmrb_combine', lambda: _row_pass_finish(lib, v, st.slab, st.V, V_out, r, item_epi, adam, s, st.sfx))
    else:
        _timed(prof, 'wmrb_item_pass', lambda: getattr(lib, 'tmf_wsum_rows4' + st.sfx)(
            w.rowptr_e, p.n_items, w.user_chunks, w.ent_row, w.ent_w, w.wbuf, st.U,
            st.V, V_out, r, item_epi, adam, st.rows4_per_launch, st.rows4_sync,
            st.rows4_sync.numel() * 4, s))


def no_param(model):
    return 0.0


def catalog_ratio(model):
    return model.n_items / model.n_samples   # the constructor ints, true division (the reference's matrix_factorization.py:167)


def softmax_scale(model):
    return catalog_ratio(model) if model.loss_graph.catalog_scale else 1.0


def kos_k_n(model):
    return model.loss_graph.k, model.loss_graph.n


@dataclasses.dataclass(frozen=True)
class Loss:
    """What one loss the engine trains is made of: a row of LOSSES, which DESIGN.md ("What a loss is made of") prints.  Every dispatch on a
    loss - here, in mf/matrix_factorization.py and in the forms (_minibatch.py, _windowed.py, dist.py) - reads these fields."""
    name: str                  # what run_epoch and the forms know it by
    kind: str                  # its class in mf.loss_graphs, matched by exact type (``cls``): a subclass is not an engine loss
    family: str                # 'list': two passes over the interaction lists | 'table': the static negative table (WmrbPlan; sp / pk /
    #                            delta / D) | 'catalog': every item of the catalog for every user
    epoch: object              # its epoch function (run_epoch calls it; the table family shares epoch_wmrb, told apart by ``pairs``)
    prose: str
    weighted: object = None    # the ``weighted`` of the LogisticLoss it stands for; None: the class has one record
    pair_step: object = None   # family 'table': its step of the sliced user pass ...
    sliced_only: bool = False  # ... which is then the only user pass it has: the one-kernel pass has the hinge built in
    ranked: bool = False       # the pair step tries a user's samples in the model's table order: WmrbPlan.sample_rank()
    plan_needs: tuple = ()     # the WmrbPlan methods (of nnz) that build what else the pair step reads
    param: object = no_param   # model -> what travels in the slot ``c`` of run_epoch and epoch_wmrb
    flag: str = None           # the TrainState keyword the epoch needs set
    global_moments: bool = False   # the loss is a function of moments over ALL interactions: no mini-batch or multi-GPU form, and
    #                            no fit at all where a class of the interactions is empty
    denom: str = 'nnz'         # loss_history_ = an epoch's loss sum / plan.nnz | plan.n_pos | 1 (the loss is one scalar)
    route: str = None          # the ROUTES row (mf/matrix_factorization.py) a fit of it answers by
    feeds: str = 'dense'       # what _fit_generic hands get_loss, of this class and its subclasses: 'samples' (sample and serial
    #                            predictions) | 'serial' | 'dense' (the [n_users, n_items] matrix)

    @property
    def cls(self):   # looked up when asked for: mf imports this module
        from .mf import loss_graphs
        return getattr(loss_graphs, self.kind)

    @property
    def table(self):
        return self.family == 'table'

    @property
    def hinge(self):
        """The one loss of the table family that every user pass and every form of a fit has (the others: SLICED_ONLY)."""
        return self.table and not self.sliced_only

    @property
    def pairs(self):
        """Its value of epoch_wmrb's ``pairs`` (None outside the table family)."""
        return 'hinge' if self.hinge else self.name if self.table else None

    def plan_form(self):
        """The InteractionPlan keywords of a fit: the table family reads no CSC lists; the others may block theirs by users."""
        return dict(user_chunks=1 if self.table else mse_user_chunks(), csc=not self.table)

    def prepare(self, wplan, plan):
        """Builds on ``wplan`` what the pair step reads beside the table - now, before any epoch runs or is captured.  The plan notes
        what was built on it (WmrbPlan.prepared), and TrainState.set_negatives builds the same on the plan of the next table."""
        if self.ranked:
            wplan.sample_rank()
        for build in self.plan_needs:
            getattr(wplan, build)(plan.nnz)

    def denominator(self, plan):
        return 1 if self.denom == '1' else getattr(plan, self.denom)

    def work(self, plan, wplan):
        """Scores per epoch: what _fit_sparse weighs against GRAPH_MAX_WORK (the catalog family forms every score, five times)."""
        return plan.nnz + (plan.n_users * wplan.S if self.table else 0) + (plan.n_users * plan.n_items if self.family == 'catalog' else 0)


_TABLE = dict(denom='n_pos', feeds='samples')
_PAIR = dict(_TABLE, sliced_only=True, route='pair')
LOSSES = {rec.name: rec for rec in (
    Loss('mse', 'MSELoss', 'list', epoch_mse, 'squared error of every stored interaction'),
    Loss('wmrb', 'WMRBLoss', 'table', epoch_wmrb, 'log of one plus the scaled hinge sum of a positive against the sampled negatives',
         pair_step=hinge_pairs, param=catalog_ratio, **_TABLE),
    Loss('kl', 'KLDivergenceLoss', 'list', epoch_kl, 'KL divergence between the score distributions of the two classes: one scalar',
         flag='kl', global_moments=True, denom='1', route='kl', feeds='serial'),
    Loss('logistic', 'LogisticLoss', 'list', epoch_logistic, 'log(1 + exp(-y p)) of every stored interaction, y the sign of its value',
         weighted=False, route='logistic'),
    Loss('logistic_w', 'LogisticLoss', 'list', epoch_logistic, 'the same, weighted by |value|', weighted=True, route='logistic'),
    Loss('bpr', 'BPRLoss', 'table', epoch_wmrb, 'mean softplus of sampled negative minus positive', pair_step=bpr_pairs, **_PAIR),
    Loss('warp', 'WARPLoss', 'table', epoch_wmrb, 'rank-weighted hinge against the first violating sample, in table order',
         pair_step=warp_pairs, ranked=True, **_PAIR),
    Loss('warp_kos', 'KOSWARPLoss', 'table', epoch_wmrb, 'WARP with every positive weighted as the k-th best of n draws',
         pair_step=kos_pairs, ranked=True, plan_needs=('kos_omega',), param=kos_k_n, **_PAIR),
    Loss('softmax', 'SampledSoftmaxLoss', 'table', epoch_wmrb, 'softmax of a positive over itself and the sampled negatives',
         pair_step=softmax_pairs, param=softmax_scale, **_PAIR),
    Loss('full_softmax', 'FullSoftmaxLoss', 'catalog', epoch_full_softmax, 'softmax of a positive over the whole catalog',
         flag='full_softmax', denom='n_pos', route='pair'),   # answers by the row 'pair' without being a pair step
)}
PAIRS = {rec.pairs: rec for rec in LOSSES.values() if rec.table}   # epoch_wmrb's pairs= -> the record whose pair step it runs
LOGISTIC_LOSSES = tuple(name for name, rec in LOSSES.items() if rec.weighted is not None)
SLICED_ONLY = tuple(name for name, rec in LOSSES.items() if rec.sliced_only)
PAIR_LOSSES = tuple(name for name, rec in LOSSES.items() if rec.table)


def adam_constants(lr):
    return _lib.load_library().tmf_adam_fresh(float(lr))
