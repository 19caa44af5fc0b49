"""The scores kernel of the sliced WMRB user pass at the C4 shape of bench.py (1M users x 100K items, r = 128, S = 1024, fp32,
~1e8 interactions): item runs (tmf_wmrb_scores7, TMF_SCORES7=1) against per-(user, slice) visits (tmf_wmrb_scores3, TMF_SCORES7=0)
on the SAME problem, the same library and the same box.

The kernel form is chosen when the training state is built, so every measurement is a child process of its own (this process never
opens the GPU); the two forms alternate, --rounds times each.  Reported: the median `wmrb_scores` time and the median epoch of either
form, and the min-max spread of the scores3 runs.  The pass condition (not tuned):

    median scores7 < median scores3 - 3 x (max - min of the scores3 runs)        the same for the epoch

    python tools/time_scores7_c4.py [--rounds 5] [--out profiles/scores7_c4.json]
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
    from teamoflow_amd import _lib
    _lib.get()
    dev = torch.device('cuda', 0)
    ns = argparse.Namespace(item_dist='zipf', lr=0.1)
    wl = bench.Workload(ns, args.users, args.items, args.nnz, args.r, args.samples, 'wmrb', 'f32', 0, 1, dev)
    s7 = wl.wplan.s7
    t0 = time.perf_counter()
    elapsed, _, prof, loss_buf = bench.run_steps(wl, args.epochs, args.warmup)
    res = dict(scores7=s7 is not None, nnz=wl.nnz, device=torch.cuda.get_device_name(0), prep_seconds=wl.prep_seconds,
               epoch_ms=elapsed / args.epochs * 1e3, loss_last=float(loss_buf[args.warmup + args.epochs - 1]),
               kernels_ms={k: prof.mean_ms(k) for k in ('wmrb_scores', 'wmrb_hinge', 'wmrb_gradu', 'wmrb_item_pass')},
               run_seconds=time.perf_counter() - t0)
    if s7 is not None:
        res['streams'] = dict(users_per_group=s7.users_per_group, slots=s7.slots, n_slices=s7.n_slices, n_sub=s7.n_sub, n_steps=s7.n_steps,
                              n_entries=s7.n_entries, entries_per_step=s7.n_entries / max(s7.n_steps, 1),
                              steps_bytes=s7.steps.numel() * 4, place_bytes=s7.place.numel() * 4)
    print(json.dumps(res), flush=True)


def run_child(args, s7):
    """One measurement in a fresh process under its own time limit; any failure ends the whole run (nothing more is started)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--users', str(args.users), '--items', str(args.items), '--r', str(args.r),
           '--nnz', str(args.nnz), '--samples', str(args.samples), '--epochs', str(args.epochs), '--warmup', str(args.warmup)]
    print(f'[time_scores7_c4] TMF_SCORES7={s7}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=dict(os.environ, TMF_SCORES7=str(s7)), stdout=subprocess.PIPE, timeout=args.limit)
    if p.returncode != 0:
        raise SystemExit(f'TMF_SCORES7={s7} run failed with exit status {p.returncode}')
    res = json.loads(p.stdout.decode().strip().splitlines()[-1])
    if res['scores7'] != bool(s7):
        raise SystemExit(f'TMF_SCORES7={s7}: the run used the other kernel')
    return res


def main():
    ap = argparse.ArgumentParser()
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
    args = ap.parse_args()
    if args.child:
        return child(args)
    rounds = []
    for _ in range(args.rounds):
        rounds.append({'scores3': run_child(args, 0), 'scores7': run_child(args, 1)})
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r, S=args.samples), nnz=rounds[0]['scores3']['nnz'],
               device=rounds[0]['scores3']['device'], epochs=args.epochs, warmup=args.warmup, n_rounds=args.rounds,
               streams=rounds[0]['scores7'].get('streams'))
    for what, pick in (('scores_ms', lambda x: x['kernels_ms']['wmrb_scores']), ('epoch_ms', lambda x: x['epoch_ms'])):
        a, b = [pick(x['scores3']) for x in rounds], [pick(x['scores7']) for x in rounds]
        spread = max(a) - min(a)
        res[what] = dict(scores3_median=median(a), scores7_median=median(b), scores3_spread=spread, scores7_spread=max(b) - min(b),
                         gain=median(a) - median(b), passes=bool(median(a) - median(b) > 3 * spread))
    res['rounds'] = rounds
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
