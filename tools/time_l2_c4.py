"""Cost of an L2-regularised MSE epoch (user_alpha, item_alpha > 0) on the sparse engine at the C4 shape (1M users x 100K items,
r = 128, ~1e8 interactions of bench.py's generator), against its yardstick from the PARENT commit's library on the same plan:

    yardstick = MSE epoch (parent) + tmf_adam_fresh_rows_f32 over the U table (parent) + the same over the V table (parent)
    regularised epoch <= yardstick x 1.10

In the regularised sequence a pass writes the raw gradient G where its fused epilogue wrote the stepped table - the same bytes -
and the added step kernel (tmf_adam_fresh_rows_l2_f32) has exactly tmf_adam_fresh_rows_f32's traffic: read W and G, write W.  1.10
is the pool-spread margin of the other time_*_c4.py tools.  If the bound is missed the record says so, with the per-kernel split;
the bound is not tuned.

A library is chosen when the package is imported, so every measurement is a child process of its own (this process never opens
the GPU); the regularised run and the parent's run alternate, --rounds times; medians over the rounds.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/libtmf_parent.so
    python tools/time_l2_c4.py --parent-lib libtmf_parent.so [--out profiles/l2_c4.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MARGIN = 1.10   # pool spread (tools/time_kl_c4.py's)


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def c4_problem(args, dev):
    import torch

    import bench
    idx, val = bench.gen_interactions(args.users, args.items, args.nnz, 'zipf', 1234, dev)
    g = torch.Generator(device=dev).manual_seed(5)
    U0 = torch.randn(args.users, args.r, device=dev, generator=g) * 0.1
    V0 = torch.randn(args.items, args.r, device=dev, generator=g) * 0.1
    return idx, val, U0, V0


def timed(torch, run, reps, warmup):
    """ms per call over `reps` calls between two device events, after `warmup` calls."""
    for e in range(warmup):
        run(e)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for e in range(reps):
        run(e)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def child(args):
    import torch

    from teamoflow_amd import _engine, _lib
    lib = _lib.get()
    dev = torch.device('cuda', 0)
    idx, val, U0, V0 = c4_problem(args, dev)
    plan = _engine.InteractionPlan(idx, val, args.users, args.items, user_chunks=_engine.mse_user_chunks(), csc=True)
    del idx, val
    adam = _engine.adam_constants(0.01)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    res = dict(nnz=plan.nnz, device=torch.cuda.get_device_name(0), library=os.path.basename(_lib.LIB_PATH), version=lib.tmf_version())
    st = _engine.TrainState(U0, V0, plan, args.r)

    def mse(e, prof=None):
        _engine.epoch_mse(st, adam, loss, prof=prof)
        st.swap()
    res['mse_epoch_ms'] = timed(torch, mse, args.epochs, args.warmup)
    prof = _engine.KernelTimer()
    for e in range(args.epochs):
        mse(e, prof)
    torch.cuda.synchronize()
    res['mse_passes_ms'] = {k: prof.mean_ms(k) for k in ('mse_user_pass', 'mse_item_pass')}
    if args.child == 'parent':
        # the existing step kernel alone, over each table, from the raw gradients of one epoch
        gU, gV = torch.empty_like(st.U), torch.empty_like(st.V)
        _engine.epoch_mse(st, adam, loss, _lib.EPI_GRAD, gV, None, _lib.EPI_GRAD, gU)
        for name, W, G in (('adam_rows_user_ms', st.U, gU), ('adam_rows_item_ms', st.V, gV)):
            res[name] = timed(torch, lambda e: _lib.check(lib.tmf_adam_fresh_rows_f32(_lib.ptr(W), _lib.ptr(G), W.shape[0], args.r, adam,
                                                                                      _lib.stream_ptr()), lib), args.epochs, args.warmup)
    else:
        del st
        st = _engine.TrainState(U0, V0, plan, args.r)
        st.set_l2(args.alpha, args.alpha)

        def l2(e, prof=None):
            _engine.epoch_sides(st, adam, loss, 'mse', prof=prof)
        res['l2_epoch_ms'] = timed(torch, l2, args.epochs, args.warmup)
        res['l2_loss_after'] = float(loss)
        prof = _engine.KernelTimer()
        for e in range(args.epochs):
            l2(e, prof)
        torch.cuda.synchronize()
        res['l2_kernels_ms'] = {k: prof.mean_ms(k) for k in ('mse_user_pass', 'mse_item_pass', 'user_adam_rows_l2', 'item_adam_rows_l2')}
    print(json.dumps(res), flush=True)


def run_child(args, which, env_extra):
    """One measurement in a fresh process under its own time limit; any failure ends the whole run (nothing more is started)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', which, '--users', str(args.users), '--items', str(args.items),
           '--r', str(args.r), '--nnz', str(args.nnz), '--epochs', str(args.epochs), '--warmup', str(args.warmup), '--alpha', str(args.alpha)]
    print(f'[time_l2_c4] {which} {env_extra}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=dict(os.environ, **env_extra), stdout=subprocess.PIPE, timeout=args.limit)
    if p.returncode != 0:
        raise SystemExit(f'{which} run failed with exit status {p.returncode}')
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help='libtmf.so built from the parent commit (the yardstick)')
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--epochs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--r', type=int, default=128)
    ap.add_argument('--nnz', type=int, default=100_000_000)
    ap.add_argument('--alpha', type=float, default=0.01, help='user_alpha = item_alpha of the regularised run')
    ap.add_argument('--limit', type=int, default=420, help='seconds one child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', choices=['l2', 'parent'], default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit('--parent-lib: the library of the parent commit is the yardstick of this measurement; build it first')
    if not args.alpha > 0:
        raise SystemExit('--alpha must be > 0: both sides of the measured epoch are penalised')
    parent_env = dict(TMF_LIB=os.path.abspath(args.parent_lib), TMF_LIB_OLDER='1')
    rounds = []
    for _ in range(args.rounds):
        rounds.append(dict(l2=run_child(args, 'l2', {}), parent=run_child(args, 'parent', parent_env)))
    first = rounds[0]['l2']
    l2_ms = median([x['l2']['l2_epoch_ms'] for x in rounds])
    parent = {k: median([x['parent'][k] for x in rounds]) for k in ('mse_epoch_ms', 'adam_rows_user_ms', 'adam_rows_item_ms')}
    yardstick = sum(parent.values())
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r), nnz=first['nnz'], device=first['device'], epochs=args.epochs,
               warmup=args.warmup, alpha=args.alpha, l2_epoch_ms=l2_ms,
               l2_kernels_ms={k: median([x['l2']['l2_kernels_ms'][k] for x in rounds]) for k in first['l2_kernels_ms']},
               mse_epoch_ms_this_library=median([x['l2']['mse_epoch_ms'] for x in rounds]), parent=parent,
               parent_mse_passes_ms={k: median([x['parent']['mse_passes_ms'][k] for x in rounds]) for k in first['mse_passes_ms']},
               yardstick_ms=yardstick, margin=MARGIN, bound_ms=yardstick * MARGIN, ratio_to_yardstick=l2_ms / yardstick,
               ratio_to_parent_mse_epoch=l2_ms / parent['mse_epoch_ms'], within_bound=bool(l2_ms <= yardstick * MARGIN), rounds=rounds)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
