"""Cost of WARPLoss on the sparse engine at the C4 shape (1M users x 100K items, r = 128, S = 1024, ~1e8 positives of bench.py's
generator and negative table), beside the WMRB hinge kernel and the WMRB epoch of the PARENT commit's library on the same plan.

The pair step.  tmf_warp_pairs_ranked (the form the engine calls: sp and D in the plan's item-sorted order, 16-bit ranks beside
them) and tmf_warp_pairs (the same rows taken as if they were in table order: the hinge kernel's bytes exactly - sp read once, D
written once) against tmf_wmrb_hinge2_ordered of the parent's library, loaded as a second handle into the same process, so that
all three run on the same rowptr, val, pk, sp and user order: launches alternate, warm-up first, medians over ``--reps`` launches
between device events.  Twice: with sp / pk of one scores pass over freshly initialised tables, and of a scores pass after ten
WARP epochs (first violators move deeper as training goes).  The bound is on the engine's form: warp <= 1.10 x hinge.
The epoch.  Ten WARP epochs between two device events, then per-kernel times through _engine.KernelTimer, beside the same of the
parent library's WMRB epoch (a child process of its own: a library is chosen when the package is imported).  No bound; recorded
next to them: the share of D entries that are not zero, which is what the gathers behind the pair step have left to do.
Every measurement is a child process under its own time limit (this process never opens the GPU); nothing is started after one fails.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/libtmf_parent.so
    python tools/time_warp_c4.py --parent-lib libtmf_parent.so [--out profiles/warp_c4.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
MARGIN = 1.10
SPANS = ('wmrb_scores', 'warp_pairs', 'wmrb_hinge', 'wmrb_gradu', 'wmrb_finish', 'wmrb_user_pass', 'wmrb_item_pass', 'wmrb_combine')


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def c4_state(args, torch, dev, force_sliced=False):
    import bench
    from teamoflow_amd import _engine
    from teamoflow_amd.mf.utils import random_sampler_device
    m, n, r, S = args.users, args.items, args.r, args.samples
    idx, val = bench.gen_interactions(m, n, args.nnz, 'zipf', 0, dev)
    U0, V0 = bench.init_table(m, r, 11, dev), bench.init_table(n, r, 7, dev)
    plan = _engine.InteractionPlan(idx, val, m, n, user_chunks=1, csc=False)
    del idx, val
    R = random_sampler_device(n, m, S, seed=100, device=dev)
    wplan = _engine.wmrb_plan_for(plan, R, r, force_sliced=force_sliced)   # at C4 the catalog is sliced whatever the loss
    assert wplan.sliced, 'this shape would take the one-kernel user pass under WMRB: not the same plan'
    return plan, wplan, _engine.TrainState(U0, V0, plan, r, wplan)


def child_warp(args):
    import torch

    from teamoflow_amd import _engine, _lib
    from time_logistic_c4 import timed_epochs
    lib = _lib.get()
    dev = torch.device('cuda', 0)
    m, n, S = args.users, args.items, args.samples
    plan, w, st = c4_state(args, torch, dev, force_sliced=True)
    rank = w.sample_rank()
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))                 # a second handle: only its hinge kernel is called
    parent.tmf_wmrb_hinge2_ordered.restype, parent.tmf_wmrb_hinge2_ordered.argtypes = _lib.SIGNATURES['tmf_wmrb_hinge2_ordered']
    adam = _engine.adam_constants(args.lr)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    P, i32, s = _lib.ptr, ctypes.c_int32, _lib.stream_ptr()
    common = (P(plan.rowptr_u), P(plan.val_u), P(st.pk), P(st.sp))
    outs = (P(w.delta), P(w.D), P(st.loss_part), P(w.hinge_order), s)
    launches = dict(
        warp_ranked=lambda: lib.tmf_warp_pairs_ranked(*common, P(rank), i32(m), i32(S), i32(n), *outs),
        warp_table_order=lambda: lib.tmf_warp_pairs(*common, i32(m), i32(S), i32(n), *outs),
        hinge_parent=lambda: parent.tmf_wmrb_hinge2_ordered(*common, i32(m), i32(S), n / S, *outs),
        hinge_this=lambda: lib.tmf_wmrb_hinge2_ordered(*common, i32(m), i32(S), n / S, *outs))

    def pair_step():
        """sp / pk of the state's tables by one epoch that is not swapped in, then the launches in turn."""
        _engine.epoch_wmrb(st, adam, 0.0, loss, pairs='warp')
        torch.cuda.synchronize()
        pos = plan.val_u > 0
        out = dict(loss=float(loss) / plan.n_pos, D_nonzero_share=float((w.D != 0).float().mean()),
                   positives_with_a_weight=float((w.delta[pos] < 0).float().mean()),
                   D_nonzero_per_user=float((w.D != 0).sum()) / m)
        times = {k: [] for k in launches}
        for rep in range(args.warmup + args.reps):
            for k, call in launches.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                _lib.check(call())
                b.record()
                b.synchronize()
                if rep >= args.warmup:
                    times[k].append(a.elapsed_time(b))
        out['ms'] = {k: median(v) for k, v in times.items()}
        out['ms_min_max'] = {k: [min(v), max(v)] for k, v in times.items()}
        return out

    props = torch.cuda.get_device_properties(0)
    res = dict(nnz=plan.nnz, n_pos=plan.n_pos, S=S, n_slices=w.n_slices, device=torch.cuda.get_device_name(0),
               compute_units=props.multi_processor_count, library=os.path.basename(_lib.LIB_PATH),
               bytes_sp_and_D=8 * m * S, bytes_rank=2 * m * S)
    res['pair_step_fresh'] = pair_step()

    def run(e, prof=None):
        _engine.epoch_wmrb(st, adam, 0.0, loss, prof=prof, pairs='warp')
        st.swap()
    res['warp_epoch_ms'] = timed_epochs(torch, run, args.epochs, 0)        # the pair step above has warmed every kernel
    res['warp_loss_after'] = float(loss) / plan.n_pos
    res['pair_step_trained'] = dict(pair_step(), epochs_before=args.epochs)
    prof = _engine.KernelTimer()
    for e in range(args.prof_epochs):
        run(e, prof)
    torch.cuda.synchronize()
    res['warp_kernels_ms'] = {k: prof.mean_ms(k) for k in SPANS if k in prof.spans}
    res['D_nonzero_share_at_the_end'] = float((w.D != 0).float().mean())
    print(json.dumps(res), flush=True)


def child_wmrb(args):
    import torch

    from teamoflow_amd import _engine, _lib
    from time_logistic_c4 import timed_epochs
    _lib.get()
    dev = torch.device('cuda', 0)
    plan, w, st = c4_state(args, torch, dev)
    adam = _engine.adam_constants(args.lr)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)

    def run(e, prof=None):
        _engine.epoch_wmrb(st, adam, args.items / args.samples, loss, prof=prof)
        st.swap()
    res = dict(library=os.path.basename(_lib.LIB_PATH), wmrb_epoch_ms=timed_epochs(torch, run, args.epochs, 1))
    prof = _engine.KernelTimer()
    for e in range(args.prof_epochs):
        run(e, prof)
    torch.cuda.synchronize()
    res['wmrb_kernels_ms'] = {k: prof.mean_ms(k) for k in SPANS if k in prof.spans}
    res['D_nonzero_share_at_the_end'] = float((w.D != 0).float().mean())
    print(json.dumps(res), flush=True)


def run_child(args, child, env_extra, limit):
    """One measurement in a fresh process under its own time limit; any failure ends the whole run (nothing more is started)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', child, '--parent-lib', os.path.abspath(args.parent_lib)]
    for k in ('users', 'items', 'r', 'nnz', 'samples', 'epochs', 'prof_epochs', 'warmup', 'reps', 'lr'):
        cmd += ['--' + k.replace('_', '-'), str(getattr(args, k))]
    print(f'[time_warp_c4] {child} {env_extra}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=dict(os.environ, **env_extra), stdout=subprocess.PIPE, timeout=limit)
    if p.returncode != 0:
        raise SystemExit(f'{child} run failed with exit status {p.returncode}')
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help='libtmf.so built from the parent commit: its hinge kernel and its WMRB epoch are the yardsticks')
    ap.add_argument('--epochs', type=int, default=10, help='WARP epochs between the two pair-step measurements (timed)')
    ap.add_argument('--prof-epochs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3, help='untimed launches of every pair kernel')
    ap.add_argument('--reps', type=int, default=15, help='timed launches of every pair kernel')
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--r', type=int, default=128)
    ap.add_argument('--nnz', type=int, default=100_000_000)
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--lr', type=float, default=0.05)
    ap.add_argument('--limit', type=int, default=420, help='seconds one child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', choices=['warp', 'wmrb'], default=None)
    args = ap.parse_args()
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit('--parent-lib: the library of the parent commit holds the yardsticks of this measurement; build it first')
    if args.child:
        return child_warp(args) if args.child == 'warp' else child_wmrb(args)
    warp = run_child(args, 'warp', {}, args.limit)
    parent = run_child(args, 'wmrb', dict(TMF_LIB=os.path.abspath(args.parent_lib), TMF_LIB_OLDER='1'), args.limit)
    verdicts = {}
    for state in ('pair_step_fresh', 'pair_step_trained'):
        ms = warp[state]['ms']
        verdicts[state] = dict(ratio_ranked=ms['warp_ranked'] / ms['hinge_parent'], ratio_table_order=ms['warp_table_order'] / ms['hinge_parent'],
                               bound=MARGIN, met=bool(ms['warp_ranked'] <= MARGIN * ms['hinge_parent']))
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r, S=args.samples), lr=args.lr, epochs=args.epochs, reps=args.reps,
               warmup=args.warmup, margin=MARGIN, pair_step=verdicts, warp=warp, parent=parent,
               epoch_ratio=warp['warp_epoch_ms'] / parent['wmrb_epoch_ms'])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
