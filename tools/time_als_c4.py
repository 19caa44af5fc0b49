"""Cost of one implicit ALS epoch at the C4 shape (1M users x 100K items, r = 128, 1.0e8 interactions; bench.gen_interactions), each
piece between device events: the two Gram matrices, the two solves (tmf_als_solve_rows_f32 over users, then over items), the
objective, and the whole epoch.  Each solve's time is set against the flop model of DESIGN.md:

    flops(solve) = sum over solved rows of  K r (r + 1)  [lower triangle of the normal matrix]  +  r^3 / 3 + 2 r^2  [Cholesky + solves]

as a fraction of the 157.3 TF fp32 peak.  There is no pass / fail bound: nothing was measured before.  --items-dist uniform measures the
same counts without the power-law items, whose longest rows (a popular item is rated by most users) each serialise one workgroup.

    python tools/time_als_c4.py                                                   # writes profiles/als_c4.json
    python tools/time_als_c4.py --items-dist uniform --out profiles/als_c4_uniform.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_FP32_TF = 157.3


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def timed(torch, run, reps, warmup):
    """ms of every one of `reps` calls (device events around each), after `warmup` calls."""
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


def solve_flops(rowptr, r):
    counts = (rowptr[1:] - rowptr[:-1]).double()
    solved = float((counts > 0).sum())
    return float(counts.sum()) * r * (r + 1), solved * (r ** 3 / 3 + 2 * r * r), float(counts.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--nnz', type=int, default=100_000_000)
    ap.add_argument('--r', type=int, default=128)
    ap.add_argument('--items-dist', default='zipf', choices=['zipf', 'uniform'])
    ap.add_argument('--reg', type=float, default=0.01)
    ap.add_argument('--alpha', type=float, default=1.0)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'als_c4.json'))
    args = ap.parse_args()

    import torch

    import bench
    from teamoflow_amd import _als, _engine, _lib, _ops
    lib = _lib.get()
    dev = torch.device('cuda', 0)
    m, n, r = args.users, args.items, args.r
    idx, val = bench.gen_interactions(m, n, args.nnz, args.items_dist, 1234, dev)
    plan = _engine.InteractionPlan(idx, val, m, n, user_chunks=1, csc=True)
    del idx, val
    ld = _lib.padded_ld(r)
    U = torch.zeros(m, ld, device=dev)[:, :r]
    V = torch.zeros(n, ld, device=dev)[:, :r]
    V.copy_(bench.init_table(n, r, 2, dev))
    w_u, t_u, c0 = _als.entry_terms(plan.val_u, args.alpha, True)
    w_i, t_i, _ = _als.entry_terms(plan.val_i, args.alpha, True)
    n_failed = torch.zeros(1, dtype=torch.int32, device=dev)
    G = {}

    def gram_v():
        G['v'] = _ops.gram(V)

    def gram_u():
        G['u'] = _ops.gram(U)

    def solve_users():
        _ops.als_solve_rows(V, plan.rowptr_u, plan.col_u, w_u, t_u, args.reg, G0=G['v'], out=U, n_failed=n_failed, check=False)

    def solve_items():
        _ops.als_solve_rows(U, plan.rowptr_i, plan.row_i, w_i, t_i, args.reg, G0=G['u'], out=V, n_failed=n_failed, check=False)

    def objective():
        return _als.objective(U, V, plan.user_of, plan.col_u, w_u, t_u, c0, args.reg, True)

    def epoch():
        gram_v()
        solve_users()
        gram_u()
        solve_items()
        objective()

    res = dict(shape=dict(m=m, n=n, r=r, nnz=plan.nnz, items=args.items_dist), device=torch.cuda.get_device_name(0),
               version=lib.tmf_version(), reps=args.reps, warmup=args.warmup, reg=args.reg, alpha=args.alpha, peak_fp32_tf=PEAK_FP32_TF)
    epoch()   # one sweep first: every piece is then timed on tables a sweep has produced
    res['loss_after_first_epoch'] = float(objective())
    for name, run in (('gram_v', gram_v), ('solve_users', solve_users), ('gram_u', gram_u), ('solve_items', solve_items),
                      ('objective', objective), ('epoch', epoch)):
        t = timed(torch, run, args.reps, args.warmup)
        res[name] = dict(ms=median(t), ms_all=t)
        print(f'[time_als_c4] {name}: {median(t):.2f} ms', file=sys.stderr, flush=True)
    res['loss_after_timing'] = float(objective())
    res['n_failed'] = int(n_failed)
    for name, rowptr in (('solve_users', plan.rowptr_u), ('solve_items', plan.rowptr_i)):
        acc, fac, longest = solve_flops(rowptr, r)
        tf = (acc + fac) / (res[name]['ms'] * 1e-3) / 1e12
        res[name].update(flops_accumulate=acc, flops_factorise=fac, longest_row=longest, tf=tf, fraction_of_peak=tf / PEAK_FP32_TF)
    total = sum(res[k]['flops_accumulate'] + res[k]['flops_factorise'] for k in ('solve_users', 'solve_items'))
    res['model_ms_at_peak'] = total / (PEAK_FP32_TF * 1e12) * 1e3
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
