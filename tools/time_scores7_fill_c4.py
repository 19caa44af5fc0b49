"""The scores kernel of the sliced WMRB user pass at the C4 shape of bench.py (1M users x 100K items, r = 128, S = 1024, fp32,
~1e8 interactions): steps classed by fill (tmf_wmrb_scores7_fill_f32, Scores7Plan.order_by_fill) against the item-ordered plan, on the
SAME problem and the same box, with two libraries alternated through TMF_LIB:

    parent   --parent-lib (built from the commit before; TMF_LIB_OLDER=1, TMF_S7_FILL=0: it has no fill entry point)
    fill     --lib, TMF_S7_FILL=1
    item     --lib, TMF_S7_FILL=0: the same kernel without the tables - what templating the loop cost by itself

Every measurement is a child process of its own (this process never opens the GPU); the three alternate, --rounds times each.
Reported: medians and max - min spreads of the `wmrb_scores` time and of the epoch, and the build time of the second plan step.
The rule (not tuned): the change is a gain if the median scores time AND the median epoch each improve on the parent by more than
the sum of the two spreads.

    python tools/time_scores7_fill_c4.py --parent-lib /path/to/parent/libtmf.so [--rounds 5] [--out profiles/scores7_fill_c4.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def child(args):
    import torch

    import bench
    from teamoflow_amd import _engine, _lib
    _lib.get()
    dev = torch.device('cuda', 0)
    ns = argparse.Namespace(item_dist='zipf', lr=0.1)
    wl = bench.Workload(ns, args.users, args.items, args.nnz, args.r, args.samples, 'wmrb', 'f32', 0, 1, dev)
    s7 = wl.wplan.s7
    t0 = time.perf_counter()
    elapsed, _, prof, loss_buf = bench.run_steps(wl, args.epochs, args.warmup)
    res = dict(fill=s7 is not None and s7.sub_wave is not None, lib=_lib.LIB_PATH, device=torch.cuda.get_device_name(0),
               epoch_ms=elapsed / args.epochs * 1e3, loss_last=float(loss_buf[args.warmup + args.epochs - 1]),
               kernels_ms={k: prof.mean_ms(k) for k in ('wmrb_scores', 'wmrb_hinge', 'wmrb_gradu', 'wmrb_item_pass')},
               run_seconds=time.perf_counter() - t0)
    if res['fill'] and args.time_build:   # the two steps of the plan once more, timed apart
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        again = _engine.Scores7Plan(wl.plan, wl.wplan, args.r, torch.float32)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        again.order_by_fill()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        fill = s7.sub_fill.sum(0).double()
        res['build'] = dict(streams_seconds=t1 - t0, order_by_fill_seconds=t2 - t1, n_steps=s7.n_steps, n_sub=s7.n_sub, n_entries=s7.n_entries,
                            steps_of_fill_4_3_2_1=[int(x) for x in fill.tolist()],
                            sub_wave_bytes=s7.sub_wave.numel() * 4, sub_fill_bytes=s7.sub_fill.numel() * 4)
    print(json.dumps(res), flush=True)


def run_child(args, mode, time_build=False):
    """One measurement in a fresh process under its own time limit; any failure ends the whole run (nothing more is started)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--users', str(args.users), '--items', str(args.items), '--r', str(args.r),
           '--nnz', str(args.nnz), '--samples', str(args.samples), '--epochs', str(args.epochs), '--warmup', str(args.warmup)]
    env = dict(os.environ, TMF_S7_FILL='1' if mode == 'fill' else '0')
    env.pop('TMF_LIB_OLDER', None)
    if mode == 'parent':
        env.update(TMF_LIB=os.path.abspath(args.parent_lib), TMF_LIB_OLDER='1')
    elif args.lib:
        env.update(TMF_LIB=os.path.abspath(args.lib))
    else:
        env.pop('TMF_LIB', None)
    if time_build:
        cmd.append('--time-build')
    print(f'[time_scores7_fill_c4] {mode}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=args.limit)
    if p.returncode != 0:
        raise SystemExit(f'{mode} run failed with exit status {p.returncode}')
    res = json.loads(p.stdout.decode().strip().splitlines()[-1])
    if res['fill'] != (mode == 'fill'):
        raise SystemExit(f'{mode}: the run used the other form')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help="libtmf.so built from the parent commit")
    ap.add_argument('--lib', default=None, help='libtmf.so of this tree (default: the in-tree build)')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--epochs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--r', type=int, default=128)
    ap.add_argument('--nnz', type=int, default=100_000_000)
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--limit', type=int, default=300, help='seconds one child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--time-build', action='store_true')
    args = ap.parse_args()
    if args.child:
        return child(args)
    modes = (['parent'] if args.parent_lib else []) + ['fill', 'item']
    rounds = []
    for i in range(args.rounds):
        rounds.append({mode: run_child(args, mode, time_build=(mode == 'fill' and i == 0)) for mode in modes})
        print(f'[time_scores7_fill_c4] round {i}: ' + ', '.join(
            f"{mode} scores {r['kernels_ms']['wmrb_scores']:.2f} epoch {r['epoch_ms']:.2f}" for mode, r in rounds[-1].items()),
            file=sys.stderr, flush=True)
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r, S=args.samples), device=rounds[0]['fill']['device'], epochs=args.epochs,
               warmup=args.warmup, n_rounds=args.rounds, build=rounds[0]['fill'].get('build'),
               rule='gain if the median improves on the parent by more than the sum of the two max - min spreads, for scores AND epoch')
    base = 'parent' if args.parent_lib else 'item'
    for what, pick in (('scores_ms', lambda x: x['kernels_ms']['wmrb_scores']), ('epoch_ms', lambda x: x['epoch_ms'])):
        col = {mode: [pick(x[mode]) for x in rounds] for mode in modes}
        res[what] = {mode: dict(median=median(v), spread=max(v) - min(v), runs=v) for mode, v in col.items()}
        gain = median(col[base]) - median(col['fill'])
        noise = max(col[base]) - min(col[base]) + max(col['fill']) - min(col['fill'])
        res[what].update(against=base, gain=gain, sum_of_spreads=noise, passes=bool(gain > noise))
    res['same_loss'] = len({x[mode]['loss_last'] for x in rounds for mode in modes}) == 1
    res['rounds'] = rounds
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
