"""Cost of the sparse, exclude-aware ndcg_at_k at the C4 shape (1M users x 100K items, r = 128): 10 graded held-out items per user
(values 1-5; 3 of them from the user's 20 best, 7 random) and ~1e8 excluded pairs (10 other best items + 90 random per user), as in
tools/time_item_ranks_c4.py, plus one user storing 2^20 test entries (its IDCG is radix-selected by a workgroup).  In one process:
ndcg_at_k(test, k=10, exclude=train) under 'auto' and 'fp32' next to the fused top-10 with the same exclusion and arithmetic, and
where the time goes - the top-10, the DCG/IDCG kernel (tmf_dcg_idcg_f32 alone on the prepared arguments), host-side setup (the
test table's CSR, the overlap check, the per-user zero counts).

    python tools/time_ndcg_c4.py [--reps 5] [--out profiles/ndcg_c4.json]
"""
import argparse
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
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions
    lib = _lib.get()
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(7)
    m, n, r, k, per, held, heavy = 1_000_000, 100_000, 128, 10, 100, 10, 1 << 20
    U = torch.randn(m, r, device=dev, generator=g) * 0.1
    V = torch.randn(n, r, device=dev, generator=g) * 0.1
    best = _ops.predict_topk(U, V, 20, arithmetic='fp32').long()
    users = torch.arange(m, device=dev)
    hp = torch.cat([best[:, :3], torch.randint(0, n, (m, held - 3), device=dev, generator=g)], 1).reshape(-1)
    hu = users.repeat_interleave(held)
    # user 0: 2^20 stored entries (ids repeat over the catalog; duplicates are summed, as to_dense does)
    hu = torch.cat([hu, torch.zeros(heavy, dtype=torch.int64, device=dev)])
    hp = torch.cat([hp, torch.arange(heavy, device=dev) % n])
    grades = torch.randint(1, 6, (hu.numel(),), device=dev, generator=g).float()
    A = SparseInteractions(torch.stack([hu, hp], 1), grades, (m, n), device=dev)
    xi = torch.cat([best[:, 5:15], torch.randint(0, n, (m, per - 10), device=dev, generator=g)], 1).reshape(-1)
    keys = torch.unique(users.repeat_interleave(per) * n + xi)
    keys = keys[~torch.isin(keys, torch.unique(hu * n + hp))]
    ex = _ops.build_exclusion(SparseInteractions(torch.stack([keys // n, keys % n], 1), torch.ones(keys.numel(), device=dev), (m, n),
                                                 device=dev), m, n)
    del best, xi, keys
    model = MatrixFactorization(r)
    model.user_embedding, model.item_embedding = U, V
    res = dict(shape=dict(m=m, n=n, r=r, k=k), test_entries=int(A.nnz), heavy_user_entries=heavy, excluded_pairs=int(ex.cols.numel()),
               device=torch.cuda.get_device_name(0), reps=args.reps)

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

    # the kernel alone, on the prepared arguments of one call
    table, kk, ex_, n_zero = model._dcg_setup(A, k, ex)
    top = _ops.predict_topk(U, V, k, exclude=ex)
    den = _ops.dcg_discounts(kk, dev)
    dcg = torch.empty(m, device=dev)
    idcg = torch.empty(m, device=dev)
    P_ = _lib.ptr

    def kernel():
        _lib.check(lib.tmf_dcg_idcg_f32(P_(table.rowptr), P_(table.cols), P_(table.gain), m, n, P_(top), k, k, P_(den), P_(n_zero),
                                        P_(dcg), P_(idcg), _lib.stream_ptr()), lib)

    kernel()
    tk = [timed(kernel)[0] for _ in range(args.reps)]
    ts = [timed(lambda: model._dcg_setup(A, k, ex))[0] for _ in range(args.reps)]
    res['ms_kernel'], res['ms_setup'] = median(tk), median(ts)
    res['ms_kernel_all'], res['ms_setup_all'] = tk, ts
    for arith in ('auto', 'fp32'):
        model.predict_arithmetic = arith
        ndcg = lambda: model.ndcg_at_k(A, k, exclude=ex)
        topk = lambda: _ops.predict_topk(U, V, k, arithmetic=arith, exclude=ex)
        ndcg(), topk()   # warm-up (code objects, LDS grants)
        tn, tt = [], []
        for _ in range(args.reps):
            tn.append(timed(ndcg)[0])
            tt.append(timed(topk)[0])
        mn, mt = median(tn), median(tt)
        res[arith] = dict(ms_ndcg=mn, ms_top10_exclude=mt, ratio=mn / mt, ms_other=mn - mt - res['ms_kernel'] - res['ms_setup'],
                          ms_ndcg_all=tn, ms_top10_all=tt)
        print(arith, json.dumps(res[arith]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
