"""Cost of one implicit ALS epoch at the C4 shape (1M users x 100K items, r = 128, 1.0e8 interactions; bench.gen_interactions), each
piece between device events: the two Gram matrices, the two solves (tmf_als_solve_rows_f32 over users, then over items), the
objective, and the whole epoch.  Each solve's time is set against the flop model of DESIGN.md:

    flops(solve) = sum over solved rows of  K r (r + 1)  [lower triangle of the normal matrix]  +  r^3 / 3 + 2 r^2  [Cholesky + solves]

as a fraction of the 157.3 TF fp32 peak.  There is no pass / fail bound: nothing was measured before.  --items-dist uniform measures the
same counts without the power-law items, whose longest rows (a popular item is rated by most users) each serialise one workgroup.

    python tools/time_als_c4.py                                                   # writes profiles/als_c4.json
    python tools/time_als_c4.py --items-dist uniform --out profiles/als_c4_uniform.json

--solver cg times the conjugate-gradient half-steps (tmf_als_cg_rows_f32, --cg-steps steps from the tables' current values, in place,
heavy rows first - what fit_als(solver='cg') launches) against the flop model  (s + 1) (2 r^2 + 4 K r)  per solved row, and sets each
solve against the YARDSTICK: the Cholesky solve of the same side by the PARENT commit's library (--parent-lib, loaded by a child process
through TMF_LIB / TMF_LIB_OLDER) on the same plan.  The condition has no margin: each CG solve takes less time than the parent's
Cholesky solve of that side.  Every piece is timed inside whole epochs (device events around it), because a CG half-step repeated on
unchanged tables converges and stops early.  r > 128 has no yardstick (the parent refuses it): a first measurement.

    python tools/time_als_c4.py --solver cg --parent-lib /path/to/parent/libtmf.so                       # profiles/als_cg_c4.json
    python tools/time_als_c4.py --solver cg --parent-lib ... --items-dist uniform                        # profiles/als_cg_c4_uniform.json
    python tools/time_als_c4.py --solver cg --r 256 --out profiles/als_cg_c4_r256.json
"""
import argparse
import json
import os
import subprocess
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


def cg_flops(rowptr, r, steps):
    counts = (rowptr[1:] - rowptr[:-1]).double()
    solved = float((counts > 0).sum())
    return (steps + 1) * (2.0 * r * r * solved + 4.0 * r * float(counts.sum())), float(counts.max())


def timed_epochs(torch, pieces, reps, warmup):
    """{name: [ms per epoch]} of the pieces run in order as whole epochs (device events around each piece), after `warmup` epochs."""
    out = {name: [] for name, _ in pieces}
    out['epoch'] = []
    for e in range(warmup + reps):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(pieces) + 1)]
        torch.cuda.synchronize()
        marks[0].record()
        for k, (_, run) in enumerate(pieces):
            run()
            marks[k + 1].record()
        torch.cuda.synchronize()
        if e >= warmup:
            for k, (name, _) in enumerate(pieces):
                out[name].append(marks[k].elapsed_time(marks[k + 1]))
            out['epoch'].append(marks[0].elapsed_time(marks[-1]))
    return out


def measure_epochs(args, solver):
    """The in-epoch timing of --solver cg, and of the parent's Cholesky solves on the same plan (solver='cholesky', the child)."""
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
    if solver == 'cg':
        U.copy_(bench.init_table(m, r, 3, dev))   # the first user half-step starts from it
        order_u, order_i = _als.heavy_first(plan.rowptr_u), _als.heavy_first(plan.rowptr_i)

        def solve_users():
            _ops.als_cg_rows(V, plan.rowptr_u, plan.col_u, w_u, t_u, args.reg, G0=G['v'], ids=order_u, x0=U, out=U, n_failed=n_failed,
                             cg_steps=args.cg_steps, check=False)

        def solve_items():
            _ops.als_cg_rows(U, plan.rowptr_i, plan.row_i, w_i, t_i, args.reg, G0=G['u'], ids=order_i, x0=V, out=V, n_failed=n_failed,
                             cg_steps=args.cg_steps, check=False)
    else:
        def solve_users():
            _ops.als_solve_rows(V, plan.rowptr_u, plan.col_u, w_u, t_u, args.reg, G0=G['v'], out=U, n_failed=n_failed, check=False)

        def solve_items():
            _ops.als_solve_rows(U, plan.rowptr_i, plan.row_i, w_i, t_i, args.reg, G0=G['u'], out=V, n_failed=n_failed, check=False)

    def objective():
        return _als.objective(U, V, plan.user_of, plan.col_u, w_u, t_u, c0, args.reg, True)

    pieces = [('gram_v', lambda: G.__setitem__('v', _ops.gram(V))), ('solve_users', solve_users),
              ('gram_u', lambda: G.__setitem__('u', _ops.gram(U))), ('solve_items', solve_items)]
    if solver == 'cg':
        pieces.append(('objective', objective))
    res = dict(shape=dict(m=m, n=n, r=r, nnz=plan.nnz, items=args.items_dist), device=torch.cuda.get_device_name(0), solver=solver,
               library=os.path.basename(_lib.LIB_PATH), version=lib.tmf_version(), reps=args.reps, warmup=args.warmup, reg=args.reg,
               alpha=args.alpha, peak_fp32_tf=PEAK_FP32_TF)
    t = timed_epochs(torch, pieces, args.reps, args.warmup)
    for name, ms in t.items():
        res[name] = dict(ms=median(ms), ms_all=ms)
        print(f'[time_als_c4] {solver} {name}: {median(ms):.2f} ms', file=sys.stderr, flush=True)
    res['loss_after_timing'] = float(objective())
    res['n_failed'] = int(n_failed)
    if solver == 'cg':
        res['cg_steps'] = args.cg_steps
        for name, rowptr in (('solve_users', plan.rowptr_u), ('solve_items', plan.rowptr_i)):
            flops, longest = cg_flops(rowptr, r, args.cg_steps)
            tf = flops / (res[name]['ms'] * 1e-3) / 1e12
            res[name].update(flops=flops, longest_row=longest, tf=tf, fraction_of_peak=tf / PEAK_FP32_TF)
    return res


def main_cg(args):
    if args.child:
        print(json.dumps(measure_epochs(args, 'cholesky')), flush=True)
        return
    parent = None
    if args.r <= 128:
        if not args.parent_lib or not os.path.exists(args.parent_lib):
            raise SystemExit('--parent-lib: the library of the parent commit is the yardstick of this measurement; build it first')
        cmd = [sys.executable, os.path.abspath(__file__), '--solver', 'cg', '--child', '--users', str(args.users), '--items', str(args.items),
               '--nnz', str(args.nnz), '--r', str(args.r), '--items-dist', args.items_dist, '--reg', str(args.reg), '--alpha', str(args.alpha),
               '--reps', str(args.reps), '--warmup', str(args.warmup)]
        env = dict(os.environ, TMF_LIB=os.path.abspath(args.parent_lib), TMF_LIB_OLDER='1')
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=args.limit)   # before this process opens the GPU
        if p.returncode != 0:
            raise SystemExit(f'the parent run failed with exit status {p.returncode}')   # nothing more is started
        parent = json.loads(p.stdout.decode().strip().splitlines()[-1])
    res = measure_epochs(args, 'cg')
    if parent is not None:
        res['parent'] = parent
        res['condition'] = {}
        for name in ('solve_users', 'solve_items'):
            cg_ms, parent_ms = res[name]['ms'], parent[name]['ms']
            res['condition'][name] = dict(cg_ms=cg_ms, parent_cholesky_ms=parent_ms, ratio=cg_ms / parent_ms, met=bool(cg_ms < parent_ms))
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, 'profiles', 'als_cg_c4.json' if args.items_dist == 'zipf' else 'als_cg_c4_uniform.json')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write(line + '\n')


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
    ap.add_argument('--solver', default='cholesky', choices=['cholesky', 'cg'])
    ap.add_argument('--cg-steps', type=int, default=3)
    ap.add_argument('--parent-lib', default=None, help='--solver cg: libtmf.so built from the parent commit (the yardstick)')
    ap.add_argument('--limit', type=int, default=420, help='--solver cg: seconds the parent run may take')
    ap.add_argument('--child', action='store_true', help='internal: the parent run of --solver cg')
    ap.add_argument('--out', default=None, help='default: profiles/als_c4.json (cholesky), profiles/als_cg_c4[_uniform].json (cg)')
    args = ap.parse_args()
    if args.solver == 'cg':
        return main_cg(args)
    args.out = args.out or os.path.join(ROOT, 'profiles', 'als_c4.json')

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
