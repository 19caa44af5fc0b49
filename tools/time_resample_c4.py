"""What resampling the negative table costs and buys at the C4 shape (1M users x 100K items, r = 128, S = 1024, ~1e8 positives of
bench.py's generator).

(a) sampler.  tmf_sample_rows (through _ops.sample_negatives) against utils.random_sampler_device, the torch program it restates
    and the yardstick (unchanged from the parent commit), both drawing the [1M, 1024] table of one seed on the device: the kernel
    as the median of ``--reps`` launches between device events after a warm-up, the torch function once between synchronisations
    after a small warm-up call.  The bound: the kernel is faster.  The two tables are compared (torch.equal).
(b) one re-plan, split.  TrainState.set_negatives at C4 under WARPLoss, every part between synchronisations: the draw, WmrbPlan
    (sort, slice offsets, entry lists), the scores plan the state wants (Scores7Plan at C4: its constructor - on the device the two
    counting calls - and order_by_fill, where a device-built plan writes its streams), sample_rank, and the rest (freeing the old
    plan, sync words, rebinding).
(c) epoch time.  The WARP and BPR epoch on the static table, with this library and with the PARENT commit's (a child process of
    its own: a library is chosen when the package is imported), and the mean epoch of a fit that re-plans every epoch and every
    fifth.  No bound.
(d) quality.  bench.py's zipf problem at a mid shape, a tenth of the interactions held out: recall@10 with exclude=train of a
    WARPLoss fit on the static table against resample_every = 1 after the same number of epochs.  Recorded, no pass / fail.
Every measurement is a child process under its own time limit (this process never opens the GPU); nothing is started after one fails.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/libtmf_parent.so
    python tools/time_resample_c4.py --parent-lib libtmf_parent.so [--out profiles/resample_c4.json]
"""
import argparse
import json
import os
import subprocess
import sys
import timeit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
HBM_GBPS = 8000.0   # MI355X peak, for the kernel's floor: the table it writes


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def child_sampler(args):
    import torch

    from teamoflow_amd import _lib, _ops
    from teamoflow_amd.mf.utils import random_sampler_device
    _lib.get()
    dev = torch.device('cuda', 0)
    m, n, S = args.users, args.items, args.samples
    out = torch.empty(m, S, dtype=torch.int32, device=dev)
    times = []
    for rep in range(args.warmup + args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _ops.sample_negatives(n, m, S, seed=100, device=dev, out=out)
        b.record()
        b.synchronize()
        if rep >= args.warmup:
            times.append(a.elapsed_time(b))
    random_sampler_device(n, 4096, S, seed=100, device=dev)   # torch's sort and hash kernels loaded before the clock starts
    torch.cuda.synchronize()
    t0 = timeit.default_timer()
    want = random_sampler_device(n, m, S, seed=100, device=dev)
    torch.cuda.synchronize()
    torch_ms = (timeit.default_timer() - t0) * 1e3
    kernel_ms = median(times)
    floor_ms = 4.0 * m * S / (HBM_GBPS * 1e9) * 1e3
    print(json.dumps(dict(kernel_ms=kernel_ms, kernel_ms_min_max=[min(times), max(times)], torch_ms=torch_ms, ratio=torch_ms / kernel_ms,
                          faster=bool(kernel_ms < torch_ms), same_table=bool(torch.equal(out, want)), bytes_written=4 * m * S,
                          floor_ms_at_peak_hbm=floor_ms, kernel_over_floor=kernel_ms / floor_ms,
                          device=torch.cuda.get_device_name(0), library=os.path.basename(_lib.LIB_PATH))), flush=True)


def c4_problem(args, torch, dev):
    import bench
    from teamoflow_amd import _engine
    m, n, r = args.users, args.items, args.r
    idx, val = bench.gen_interactions(m, n, args.nnz, 'zipf', 0, dev)
    plan = _engine.InteractionPlan(idx, val, m, n, user_chunks=1, csc=False)
    return plan, bench.init_table(m, r, 11, dev), bench.init_table(n, r, 7, dev)


def child_epochs(args):
    """(b) and (c) with the library the environment names.  With the parent's library only the static epochs are run."""
    import torch

    from teamoflow_amd import _engine, _lib, _ops
    from teamoflow_amd.mf.utils import random_sampler_device
    from time_logistic_c4 import timed_epochs
    _lib.get()
    dev = torch.device('cuda', 0)
    m, n, r, S = args.users, args.items, args.r, args.samples
    plan, U0, V0 = c4_problem(args, torch, dev)
    adam = _engine.adam_constants(args.lr)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    res = dict(library=os.path.basename(_lib.LIB_PATH), nnz=plan.nnz, parent=bool(args.static_only))
    spans = {}

    def timed(name, fn):   # a method wrapped so that its calls are timed between synchronisations
        def wrapper(*a, **k):
            torch.cuda.synchronize()
            t0 = timeit.default_timer()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            spans.setdefault(name, []).append((timeit.default_timer() - t0) * 1e3)
            return out
        return wrapper

    for pairs in ('warp', 'bpr'):
        R = random_sampler_device(n, m, S, seed=100, device=dev)
        wplan = _engine.wmrb_plan_for(plan, R, r, force_sliced=True)
        if pairs == 'warp':
            wplan.sample_rank()
        st = _engine.TrainState(U0, V0, plan, r, wplan)
        del R, wplan

        def run(e):
            _engine.epoch_wmrb(st, adam, 0.0, loss, pairs=pairs)
            st.swap()
        out = dict(static_epoch_ms=timed_epochs(torch, run, args.epochs, 1), scores7=st.wplan.s7 is not None, n_slices=st.wplan.n_slices)
        if not args.static_only:
            if pairs == 'warp':   # (b): the parts of one re-plan
                spans.clear()
                saved = (_engine.WmrbPlan.__init__, _engine.Scores7Plan.__init__, _engine.Scores6Plan.__init__, _engine.WmrbPlan.sample_rank,
                         _engine.Scores7Plan.order_by_fill)
                _engine.WmrbPlan.__init__ = timed('wmrb_plan', saved[0])
                _engine.Scores7Plan.__init__ = timed('scores7_plan', saved[1])
                _engine.Scores6Plan.__init__ = timed('scores6_plan', saved[2])
                _engine.WmrbPlan.sample_rank = timed('sample_rank', saved[3])
                _engine.Scores7Plan.order_by_fill = timed('scores7_order_by_fill', saved[4])
                draw = timed('draw', lambda j: _ops.sample_negatives(n, m, S, seed=100 + j, device=dev))
                rebind = timed('set_negatives', st.set_negatives)
                for j in (1, 2):
                    rebind(draw(j))
                (_engine.WmrbPlan.__init__, _engine.Scores7Plan.__init__, _engine.Scores6Plan.__init__, _engine.WmrbPlan.sample_rank,
                 _engine.Scores7Plan.order_by_fill) = saved
                split = {k: median(v) for k, v in spans.items()}
                split['rest_free_sync_rebind'] = split['set_negatives'] - sum(v for k, v in split.items() if k not in ('draw', 'set_negatives'))
                split['replan_total'] = split['draw'] + split['set_negatives']
                out['replan_split_ms'] = split
            for every, epochs in ((1, 3), (5, 10)):   # (c): the mean epoch of a fit in its steady state, one re-plan per `every` epochs
                torch.cuda.synchronize()
                t0 = timeit.default_timer()
                for e in range(epochs):
                    if e % every == 0:
                        st.set_negatives(_ops.sample_negatives(n, m, S, seed=200 + 16 * every + e // every, device=dev))
                    run(e)
                torch.cuda.synchronize()
                out[f'resample_every_{every}_epoch_ms'] = (timeit.default_timer() - t0) * 1e3 / epochs
        out['D_nonzero_share_at_the_end'] = float((st.wplan.D != 0).float().mean())
        res[pairs] = out
        del st
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


def child_quality(args):
    import torch

    import bench
    from teamoflow_amd import _lib
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import WARPLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    from teamoflow_amd.mf.utils import random_sampler_device
    _lib.get()
    dev = torch.device('cuda', 0)
    m, n, r, S, nnz = args.q_users, args.q_items, args.q_r, args.q_samples, args.q_nnz
    idx, val = bench.gen_interactions(m, n, nnz, 'zipf', 0, dev)
    held = torch.rand(val.numel(), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) < 0.1
    train = SparseInteractions(torch.stack([idx[:, 0][~held], idx[:, 1][~held]], 1), val[~held], (m, n))
    test = SparseInteractions(torch.stack([idx[:, 0][held], idx[:, 1][held]], 1), val[held], (m, n))
    U0, V0 = bench.init_table(m, r, 11, dev), bench.init_table(n, r, 7, dev)
    R = random_sampler_device(n, m, S, seed=100, device=dev)
    res = dict(shape=dict(m=m, n=n, r=r, S=S, nnz_train=int((~held).sum()), nnz_test=int(held.sum())), epochs=args.q_epochs, lr=args.q_lr,
               k=10, runs={})
    for name, every in (('static', 0), ('resample_every_1', 1), ('resample_every_5', 5)):
        model = MatrixFactorization(r, loss_graph=WARPLoss(), user_weight_graph=FixedInitializer(U0), item_weight_graph=FixedInitializer(V0),
                                    n_users=m, n_items=n, n_samples=S)
        model.verbose, model.random_ind, model.resample_every = False, R, every
        model.fit(args.q_epochs, eye(m), eye(n), train, lr=args.q_lr)
        st = model._state
        res['runs'][name] = dict(recall_at_10=float(model.recall_at_k(test, k=10, exclude=train).mean()),
                                 recall_at_10_train=float(model.recall_at_k(train, k=10).mean()),
                                 loss_first_last=[model.loss_history_[0], model.loss_history_[-1]],
                                 D_nonzero_share_at_the_end=float((st.wplan.D != 0).float().mean()),
                                 fit_seconds=model.fit_seconds_, resample_seconds=model.resample_seconds_, rounds=model.resample_rounds_)
    print(json.dumps(res), flush=True)


def run_child(args, child, env_extra, limit, extra=()):
    """One measurement in a fresh process under its own time limit; any failure ends the whole run (nothing more is started)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', child, *extra]
    for k in ('users', 'items', 'r', 'nnz', 'samples', 'epochs', 'warmup', 'reps', 'lr', 'q_users', 'q_items', 'q_r', 'q_nnz', 'q_samples',
              'q_epochs', 'q_lr'):
        cmd += ['--' + k.replace('_', '-'), str(getattr(args, k))]
    print(f'[time_resample_c4] {child} {env_extra}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=dict(os.environ, **env_extra), stdout=subprocess.PIPE, timeout=limit)
    if p.returncode != 0:
        raise SystemExit(f'{child} run failed with exit status {p.returncode}')
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help='libtmf.so built from the parent commit: its static WARP and BPR epochs are the yardsticks of (c)')
    ap.add_argument('--epochs', type=int, default=5, help='timed epochs on the static table')
    ap.add_argument('--warmup', type=int, default=2, help='untimed launches of the sampler kernel')
    ap.add_argument('--reps', type=int, default=7, help='timed launches of the sampler kernel')
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--r', type=int, default=128)
    ap.add_argument('--nnz', type=int, default=100_000_000)
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--lr', type=float, default=0.05)
    ap.add_argument('--q-users', type=int, default=50_000)
    ap.add_argument('--q-items', type=int, default=20_000)
    ap.add_argument('--q-r', type=int, default=64)
    ap.add_argument('--q-nnz', type=int, default=2_500_000)
    ap.add_argument('--q-samples', type=int, default=256)
    ap.add_argument('--q-epochs', type=int, default=30)
    ap.add_argument('--q-lr', type=float, default=0.05)
    ap.add_argument('--limit', type=int, default=420, help='seconds one child process may take')
    ap.add_argument('--only', default='sampler,epochs,parent,quality', help='which measurements to run')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', choices=['sampler', 'epochs', 'quality'], default=None)
    ap.add_argument('--static-only', action='store_true')
    args = ap.parse_args()
    if args.child:
        return dict(sampler=child_sampler, epochs=child_epochs, quality=child_quality)[args.child](args)
    only = args.only.split(',')
    if 'parent' in only and (not args.parent_lib or not os.path.exists(args.parent_lib)):
        raise SystemExit('--parent-lib: the library of the parent commit holds the yardsticks of (c); build it first')
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r, S=args.samples), lr=args.lr, epochs=args.epochs, reps=args.reps)
    if 'sampler' in only:
        res['sampler'] = run_child(args, 'sampler', {}, args.limit)
    if 'epochs' in only:
        res['this'] = run_child(args, 'epochs', {}, args.limit)
    if 'parent' in only:
        res['parent'] = run_child(args, 'epochs', dict(TMF_LIB=os.path.abspath(args.parent_lib), TMF_LIB_OLDER='1'), args.limit, ['--static-only'])
    if 'quality' in only:
        res['quality'] = run_child(args, 'quality', {}, args.limit)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
