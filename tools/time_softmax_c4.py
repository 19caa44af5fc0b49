"""Cost of SampledSoftmaxLoss on the sparse engine at the C4 shape (1M users x 100K items, r = 128, S = 1024, ~1e8 positives of bench.py's
generator and negative table), against the WMRB hinge kernel and the WMRB epoch of the PARENT commit's library on the same plan,
tables and user order; the parent's BPR epoch is recorded beside them (the comparison that motivates the loss; no bound).

The pair step.  tmf_softmax_pairs against tmf_wmrb_hinge2_ordered of the parent's library, loaded as a second handle into the same
process, so that both run on the same rowptr, val, pk, sp and user order: launches alternate, warm-up first, medians over ``--reps``
launches between device events.  Twice: with sp / pk of one scores pass over freshly initialised tables, and of a scores pass after
``--epochs`` softmax epochs.  Both kernels move the same 2 x 4 m S bytes.  Bound: softmax <= 1.10 x hinge.
The epoch.  ``--epochs`` softmax epochs (c = n_items / n_samples) between two device events, then per-kernel times through
_engine.KernelTimer, beside the same of the parent library's WMRB epoch and BPR epoch (child processes of their own: a library is
chosen when the package is imported).  Bound: softmax epoch <= 1.10 x WMRB epoch (D is dense here where WMRB's is not).
Every measurement is a child process under its own time limit (this process never opens the GPU); nothing is started after one fails.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/libtmf_parent.so
    python tools/time_softmax_c4.py --parent-lib libtmf_parent.so [--out profiles/softmax_c4.json]
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
SPANS = ('wmrb_scores', 'softmax_pairs', 'bpr_pairs', 'wmrb_hinge', 'wmrb_gradu', 'wmrb_finish', 'wmrb_user_pass', 'wmrb_item_pass',
         'wmrb_combine')


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def child_softmax(args):
    import torch

    from teamoflow_amd import _engine, _lib
    from time_logistic_c4 import timed_epochs
    from time_warp_c4 import c4_state
    lib = _lib.get()
    dev = torch.device('cuda', 0)
    m, n, S = args.users, args.items, args.samples
    plan, w, st = c4_state(args, torch, dev, force_sliced=True)
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))                 # a second handle: only its hinge kernel is called
    parent.tmf_wmrb_hinge2_ordered.restype, parent.tmf_wmrb_hinge2_ordered.argtypes = _lib.SIGNATURES['tmf_wmrb_hinge2_ordered']
    adam = _engine.adam_constants(args.lr)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    P, i32, s, c = _lib.ptr, ctypes.c_int32, _lib.stream_ptr(), n / S
    common = (P(plan.rowptr_u), P(plan.val_u), P(st.pk), P(st.sp), i32(m), i32(S), c)
    outs = (P(w.delta), P(w.D), P(st.loss_part), P(w.hinge_order), s)
    launches = dict(softmax=lambda: lib.tmf_softmax_pairs(*common, *outs),
                    hinge_parent=lambda: parent.tmf_wmrb_hinge2_ordered(*common, *outs),
                    hinge_this=lambda: lib.tmf_wmrb_hinge2_ordered(*common, *outs))

    def pair_step():
        """sp / pk of the state's tables by one epoch that is not swapped in, then the launches in turn."""
        _engine.epoch_wmrb(st, adam, c, loss, pairs='softmax')
        torch.cuda.synchronize()
        out = dict(loss=float(loss) / plan.n_pos, D_nonzero_share=float((w.D != 0).float().mean()))
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
        out['softmax_GB_per_s'] = 8e-6 * m * S / out['ms']['softmax']
        return out

    props = torch.cuda.get_device_properties(0)
    res = dict(nnz=plan.nnz, n_pos=plan.n_pos, S=S, c=c, n_slices=w.n_slices, device=torch.cuda.get_device_name(0),
               compute_units=props.multi_processor_count, library=os.path.basename(_lib.LIB_PATH), bytes_sp_and_D=8 * m * S)
    res['pair_step_fresh'] = pair_step()

    def run(e, prof=None):
        _engine.epoch_wmrb(st, adam, c, loss, prof=prof, pairs='softmax')
        st.swap()
    res['softmax_epoch_ms'] = timed_epochs(torch, run, args.epochs, 0)     # the pair step above has warmed every kernel
    res['softmax_loss_after'] = float(loss) / plan.n_pos
    res['pair_step_trained'] = dict(pair_step(), epochs_before=args.epochs)
    prof = _engine.KernelTimer()
    for e in range(args.prof_epochs):
        run(e, prof)
    torch.cuda.synchronize()
    res['softmax_kernels_ms'] = {k: prof.mean_ms(k) for k in SPANS if k in prof.spans}
    print(json.dumps(res), flush=True)


def child_parent_epoch(args, pairs):
    """The WMRB (pairs='hinge') or BPR epoch of the library this process was started with (TMF_LIB: the parent's)."""
    import torch

    from teamoflow_amd import _engine, _lib
    from time_logistic_c4 import timed_epochs
    from time_warp_c4 import c4_state
    _lib.get()
    dev = torch.device('cuda', 0)
    plan, w, st = c4_state(args, torch, dev, force_sliced=pairs != 'hinge')
    adam = _engine.adam_constants(args.lr)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)

    def run(e, prof=None):
        _engine.epoch_wmrb(st, adam, args.items / args.samples, loss, prof=prof, pairs=pairs)
        st.swap()
    name = 'wmrb' if pairs == 'hinge' else pairs
    res = {'library': os.path.basename(_lib.LIB_PATH), name + '_epoch_ms': timed_epochs(torch, run, args.epochs, 1)}
    prof = _engine.KernelTimer()
    for e in range(args.prof_epochs):
        run(e, prof)
    torch.cuda.synchronize()
    res[name + '_kernels_ms'] = {k: prof.mean_ms(k) for k in SPANS if k in prof.spans}
    res['D_nonzero_share_at_the_end'] = float((w.D != 0).float().mean())
    print(json.dumps(res), flush=True)


def run_child(args, child, env_extra, limit):
    """One measurement in a fresh process under its own time limit; any failure ends the whole run (nothing more is started)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', child, '--parent-lib', os.path.abspath(args.parent_lib)]
    for k in ('users', 'items', 'r', 'nnz', 'samples', 'epochs', 'prof_epochs', 'warmup', 'reps', 'lr'):
        cmd += ['--' + k.replace('_', '-'), str(getattr(args, k))]
    print(f'[time_softmax_c4] {child} {env_extra}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=dict(os.environ, **env_extra), stdout=subprocess.PIPE, timeout=limit)
    if p.returncode != 0:
        raise SystemExit(f'{child} run failed with exit status {p.returncode}')
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help='libtmf.so built from the parent commit: its hinge kernel and its WMRB epoch are the yardsticks')
    ap.add_argument('--epochs', type=int, default=10, help='epochs between the two pair-step measurements (timed)')
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
    ap.add_argument('--child', choices=['softmax', 'wmrb', 'bpr'], default=None)
    args = ap.parse_args()
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit('--parent-lib: the library of the parent commit holds the yardsticks of this measurement; build it first')
    if args.child:
        return child_softmax(args) if args.child == 'softmax' else child_parent_epoch(args, 'hinge' if args.child == 'wmrb' else 'bpr')
    softmax = run_child(args, 'softmax', {}, args.limit)
    older = dict(TMF_LIB=os.path.abspath(args.parent_lib), TMF_LIB_OLDER='1')
    parent = run_child(args, 'wmrb', older, args.limit)
    parent.update({k: v for k, v in run_child(args, 'bpr', older, args.limit).items() if k.startswith('bpr_')})
    verdicts = {}
    for state in ('pair_step_fresh', 'pair_step_trained'):
        ms = softmax[state]['ms']
        verdicts[state] = dict(ratio=ms['softmax'] / ms['hinge_parent'], bound=MARGIN, met=bool(ms['softmax'] <= MARGIN * ms['hinge_parent']))
    ratio = softmax['softmax_epoch_ms'] / parent['wmrb_epoch_ms']
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r, S=args.samples), lr=args.lr, epochs=args.epochs, reps=args.reps,
               warmup=args.warmup, margin=MARGIN, pair_step=verdicts, epoch=dict(ratio=ratio, bound=MARGIN, met=bool(ratio <= MARGIN)),
               epoch_ratio_to_bpr=softmax['softmax_epoch_ms'] / parent['bpr_epoch_ms'], softmax=softmax, parent=parent)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
