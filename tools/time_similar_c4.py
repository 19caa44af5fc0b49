"""Cost of similar_items / similar_users at the C4 shape (100K items, 1M users, r = 128, k = 10, self excluded), against the same
ranking on the PARENT commit's library:

    yardstick = predict_topk(V, V, 10, return_values=True, exclude=<one entry per row: itself>)     (parent library)
    similar_items() over all 100K items <= yardstick x 1.10, under 'auto' and under 'fp32'

What similar_items adds to that ranking is the normalisation: tmf_unit_rows_f32 over the table (~0.1 GB moved beside a ~2.6 TF
product).  1.10 is the pool-spread margin of the other time_*_c4.py tools.  If the bound is missed the record says so; the bound is
not tuned.  Also measured with this library: tmf_unit_rows_f32 alone on a 1M x 128 table, as GB/s of its byte count
(n ldt 4 read, n ldo 4 + 4 n written), and similar_users for 100K query users against the 1M-user table.

A library is chosen when the package is imported, so every measurement is a child process of its own (this process never opens
the GPU); this library's run and the parent's alternate, --rounds times; medians over the rounds.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/libtmf_parent.so
    python tools/time_similar_c4.py --parent-lib libtmf_parent.so [--out profiles/similar_c4.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MARGIN = 1.10   # pool spread (tools/time_l2_c4.py's)
ARITHMETICS = ('auto', 'fp32')


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def timed(torch, run, reps, warmup):
    """ms of every one of `reps` calls (device events around each, a synchronise after it), after `warmup` calls."""
    for _ in range(warmup):
        run()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def child(args):
    import torch

    from teamoflow_amd import _lib, _ops
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    lib = _lib.get()
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(7)
    n, m, r, k = args.items, args.users, args.r, args.k
    V = torch.randn(n, r, device=dev, generator=g) * 0.1
    res = dict(device=torch.cuda.get_device_name(0), library=os.path.basename(_lib.LIB_PATH), version=lib.tmf_version())
    if args.child == 'parent':
        ex = _ops.Exclusion(torch.arange(n + 1, dtype=torch.int64, device=dev), torch.arange(n, dtype=torch.int32, device=dev), n, n)
        for arith in ARITHMETICS:
            t = timed(torch, lambda: _ops.predict_topk(V, V, k, return_values=True, arithmetic=arith, exclude=ex), args.reps, args.warmup)
            res[arith] = dict(ms_topk=median(t), ms_topk_all=t)
        print(json.dumps(res), flush=True)
        return
    model = MatrixFactorization(r)
    model.item_embedding = V
    model.user_embedding = V[:1]
    for arith in ARITHMETICS:
        model.predict_arithmetic = arith
        t = timed(torch, lambda: model.similar_items(k=k), args.reps, args.warmup)
        res[arith] = dict(ms_similar_items=median(t), ms_similar_items_all=t)
    # the kernel alone
    U = torch.randn(m, r, device=dev, generator=g) * 0.1
    T, rows, _, ldt = _ops._operand(U)
    ldo = _lib.padded_ld(r)
    out = torch.empty(rows, ldo, device=dev)
    norms = torch.empty(rows, device=dev)
    t = timed(torch, lambda: _lib.check(lib.tmf_unit_rows_f32(_lib.ptr(T), rows, r, ldt, None, rows, _lib.ptr(out), ldo, _lib.ptr(norms),
                                                             _lib.stream_ptr()), lib), 4 * args.reps, args.warmup)
    moved = rows * ldt * 4 + rows * ldo * 4 + 4 * rows
    res['unit_rows'] = dict(rows=rows, r=r, bytes=moved, ms=median(t), gb_per_s=moved / (median(t) * 1e-3) / 1e9, ms_all=t)
    del out, norms
    model.user_embedding = U
    model.predict_arithmetic = None
    ids = torch.randperm(m, device=dev, generator=g)[:args.query_users]
    t = timed(torch, lambda: model.similar_users(ids, k=k), max(1, args.reps // 2), 1)
    res['similar_users'] = dict(queries=int(ids.numel()), table_rows=m, ms=median(t), ms_all=t)
    print(json.dumps(res), flush=True)


def run_child(args, which, env_extra):
    """One measurement in a fresh process under its own time limit; any failure ends the whole run (nothing more is started)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', which, '--users', str(args.users), '--items', str(args.items),
           '--r', str(args.r), '--k', str(args.k), '--reps', str(args.reps), '--warmup', str(args.warmup),
           '--query-users', str(args.query_users)]
    print(f'[time_similar_c4] {which} {env_extra}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=dict(os.environ, **env_extra), stdout=subprocess.PIPE, timeout=args.limit)
    if p.returncode != 0:
        raise SystemExit(f'{which} run failed with exit status {p.returncode}')
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help='libtmf.so built from the parent commit (the yardstick)')
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--reps', type=int, default=6)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--query-users', type=int, default=100_000)
    ap.add_argument('--r', type=int, default=128)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--limit', type=int, default=300, help='seconds one child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', choices=['this', 'parent'], default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit('--parent-lib: the library of the parent commit is the yardstick of this measurement; build it first')
    parent_env = dict(TMF_LIB=os.path.abspath(args.parent_lib), TMF_LIB_OLDER='1')
    rounds = []
    for _ in range(args.rounds):
        rounds.append(dict(this=run_child(args, 'this', {}), parent=run_child(args, 'parent', parent_env)))
    first = rounds[0]['this']
    res = dict(shape=dict(n=args.items, m=args.users, r=args.r, k=args.k), device=first['device'], reps=args.reps, warmup=args.warmup,
               margin=MARGIN)
    for arith in ARITHMETICS:
        ms = median([x['this'][arith]['ms_similar_items'] for x in rounds])
        ref = median([x['parent'][arith]['ms_topk'] for x in rounds])
        res[arith] = dict(ms_similar_items=ms, ms_parent_topk=ref, ratio=ms / ref, within_bound=bool(ms <= ref * MARGIN))
    res['within_bound'] = all(res[a]['within_bound'] for a in ARITHMETICS)
    res['unit_rows'] = dict(first['unit_rows'], ms=median([x['this']['unit_rows']['ms'] for x in rounds]),
                            gb_per_s=median([x['this']['unit_rows']['gb_per_s'] for x in rounds]))
    res['similar_users'] = dict(first['similar_users'], ms=median([x['this']['similar_users']['ms'] for x in rounds]))
    res['rounds'] = rounds
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
