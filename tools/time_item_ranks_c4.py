"""Cost of the full-catalog rank pass at the C4 shape (1M users x 100K items, r = 128): 10 held-out positives per user (3 of the user's
20 best items, 7 random) and ~1e8 excluded pairs (10 other best items + 90 random per user), as in tools/time_exclude_c4.py.  In one
process: _ops.item_ranks under 'auto' and 'fp32' next to the fused top-10 with the same exclusion and arithmetic, and where the rank
time goes - pair scores, the fused GEMM + count (the same kernel with a never-passing epilogue is not built, so the GEMM share is the
top-10's kernel time as the bound), host-side setup (CSR, overlap check, virtual rows).

    python tools/time_item_ranks_c4.py [--reps 5] [--out profiles/item_ranks_c4.json]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from teamoflow_amd import _lib, _ops
    from teamoflow_amd.mf.sparse import SparseInteractions
    lib = _lib.get()
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(7)
    m, n, r, k, per, held = 1_000_000, 100_000, 128, 10, 100, 10
    U = torch.randn(m, r, device=dev, generator=g) * 0.1
    V = torch.randn(n, r, device=dev, generator=g) * 0.1
    best = _ops.predict_topk(U, V, 20, arithmetic='fp32').long()
    users = torch.arange(m, device=dev)
    hp = torch.cat([best[:, :3], torch.randint(0, n, (m, held - 3), device=dev, generator=g)], 1).reshape(-1)
    A = SparseInteractions(torch.stack([users.repeat_interleave(held), hp], 1), torch.ones(m * held, device=dev), (m, n), device=dev)
    pos = _ops.positive_pairs(A, m, n)
    P = int(pos.rowptr[-1])
    xi = torch.cat([best[:, 5:15], torch.randint(0, n, (m, per - 10), device=dev, generator=g)], 1).reshape(-1)
    keys = torch.unique(users.repeat_interleave(per) * n + xi)
    keys = keys[~torch.isin(keys, _ops._csr_rows(pos.rowptr) * n + pos.cols[:P].long())]
    ex = _ops.build_exclusion(SparseInteractions(torch.stack([keys // n, keys % n], 1), torch.ones(keys.numel(), device=dev), (m, n),
                                                 device=dev), m, n)
    del best, hp, xi, keys
    res = dict(shape=dict(m=m, n=n, r=r, k=k), positives=P, excluded_pairs=int(ex.cols.numel()), device=torch.cuda.get_device_name(0),
               reps=args.reps)

    def timed(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    def median(x):
        x = sorted(x)
        return x[len(x) // 2]

    # the pieces of one call, timed alone on the prepared arguments
    vu, vb, vc = _ops.virtual_rows(pos.rowptr)
    pair_user = _ops._csr_rows(pos.rowptr).to(torch.int32)
    scores = torch.empty(P, dtype=torch.float32, device=dev)
    ranks = torch.empty(P, dtype=torch.int32, device=dev)
    rows = _ops._rank_rows(vu, vb, vc)
    ws = torch.empty(lib.tmf_item_ranks_split_workspace_bytes(n, r), dtype=torch.uint8, device=dev)
    exs = ctypes.byref(ex.struct(m))
    P_ = _lib.ptr
    pieces = {
        'fp32': (lambda: _lib.check(lib.tmf_pair_scores_f32(P_(U), P_(V), r, r, r, P_(pair_user), P_(pos.cols), P, P_(scores), _lib.stream_ptr())),
                 lambda: _lib.check(lib.tmf_item_ranks_f32(P_(U), P_(V), n, r, r, r, ctypes.byref(rows), P_(pos.cols), P_(scores), exs,
                                                           P_(ranks), _lib.stream_ptr()))),
        'split': (lambda: _lib.check(lib.tmf_pair_scores_split(P_(U), P_(V), r, r, r, P_(pair_user), P_(pos.cols), P, P_(scores), _lib.stream_ptr())),
                  lambda: _lib.check(lib.tmf_item_ranks_split(P_(U), P_(V), n, r, r, r, ctypes.byref(rows), P_(pos.cols), P_(scores), exs,
                                                              P_(ranks), P_(ws), ws.numel(), _lib.stream_ptr()))),
    }
    for arith in ('auto', 'fp32'):
        form = 'split' if arith == 'auto' else 'fp32'
        rank = lambda: _ops.item_ranks(U, V, A, exclude=ex, arithmetic=arith)
        top = lambda: _ops.predict_topk(U, V, k, arithmetic=arith, exclude=ex)
        rank(), top()   # warm-up (code objects, LDS grants)
        tr, tt, tp, tk = [], [], [], []
        for _ in range(args.reps):
            tr.append(timed(rank)[0])
            tt.append(timed(top)[0])
            tp.append(timed(pieces[form][0])[0])
            tk.append(timed(pieces[form][1])[0])
        mr, mt = median(tr), median(tt)
        res[arith] = dict(form=form, ms_ranks=mr, ms_top10_exclude=mt, ratio=mr / mt, ms_pair_scores=median(tp), ms_rank_kernel=median(tk),
                          ms_setup=mr - median(tp) - median(tk), ms_ranks_all=tr, ms_top10_all=tt)
        print(arith, json.dumps(res[arith]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
