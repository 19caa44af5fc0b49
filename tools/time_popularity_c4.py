"""What popularity-weighted negative sampling costs and buys (negative_sampling='popularity'; tmf_sample_rows_weighted).

(a) sampler.  tmf_sample_rows_weighted (through _ops.sample_negatives(weights=q)) at the C4 shape - 1M users x 100K items, S = 1024 -
    on the popularity of bench.py's zipf problem under power 0.75, against utils.random_sampler_device(weights=q), the torch program
    it restates, in the same process: the kernel as the median of ``--reps`` launches between device events after a warm-up, the
    torch function once between synchronisations after a small warm-up call.  The bound: the kernel is faster, and the two tables
    are torch.equal.  Recorded beside it, without a bound: the uniform kernel tmf_sample_rows at the same shape, with this library
    and (``--parent-lib``) with the parent commit's, and the redraw rounds the table took (the definition restated with a counter).
    ``--also-lib NAME=PATH`` repeats (a) with another build of the library (an experiment kept as a patch under profiles/).
(b) one re-plan.  TrainState.set_negatives at C4 under WARPLoss with a uniform table and with a popularity table, every part between
    synchronisations: the draw, WmrbPlan, Scores7Plan (constructor and order_by_fill), sample_rank; and the WARP epoch on either
    table.  No bound.
(c) quality.  bench.py's zipf problem at the shape of profiles/resample_c4.json (50K x 20K, r = 64, S = 256, 30 epochs, lr 0.05), a
    tenth of the interactions held out: recall@10 with exclude=train for BPRLoss and WARPLoss, static table and resample_every = 1,
    uniform against power 0.5 / 0.75 / 1.0 (a power the admission rule refuses is recorded as refused), with and without
    scalar_item_bias.  Recorded, no pass / fail.
Every measurement is a child process under its own time limit (this process never opens the GPU); nothing is started after one fails.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/libtmf_parent.so
    python tools/time_popularity_c4.py --parent-lib libtmf_parent.so [--out profiles/popularity_c4.json]
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


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def popularity(torch, idx, val, n, power):
    """The weights a fit under negative_sampling='popularity' draws with: MatrixFactorization._popularity_weights."""
    from teamoflow_amd.mf.utils import popularity_weights
    return popularity_weights(torch.bincount(idx[:, 1][val > 0].to(torch.int64), minlength=n).cpu(), power)


def redraw_rounds(torch, n, m, S, seed, q, dev, block=32768):
    """Redraw rounds the weighted table of ``seed`` takes: the definition's loop restated with a counter, block by block."""
    from teamoflow_amd.mf.utils import counter_hash, hash_below, weighted_item
    cum = torch.cumsum(q, 0).to(dev)
    total = int(cum[-1])
    pos = torch.arange(S, device=dev, dtype=torch.int64)[None, :]
    worst = 0
    for r0 in range(0, m, block):
        u = torch.arange(r0, min(m, r0 + block), device=dev, dtype=torch.int64)[:, None]
        blk = torch.sort(weighted_item(hash_below(counter_hash(seed, u, pos, 2), total), cum), dim=1)[0]
        for rnd in range(3, 259):
            dup = torch.zeros_like(blk, dtype=torch.bool)
            dup[:, 1:] = blk[:, 1:] == blk[:, :-1]
            if not bool(dup.any()):
                break
            blk = torch.sort(torch.where(dup, weighted_item(hash_below(counter_hash(seed, u, pos, rnd), total), cum), blk), dim=1)[0]
        worst = max(worst, rnd - 3)
    return worst


def time_draws(torch, draw, warmup, reps):
    times = []
    for rep in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        draw()
        b.record()
        b.synchronize()
        if rep >= warmup:
            times.append(a.elapsed_time(b))
    return dict(ms=median(times), ms_min_max=[min(times), max(times)])


def child_sampler(args):
    import torch

    import bench
    from teamoflow_amd import _lib, _ops
    from teamoflow_amd.mf.utils import random_sampler_device
    _lib.get()
    dev = torch.device('cuda', 0)
    m, n, S = args.users, args.items, args.samples
    out = torch.empty(m, S, dtype=torch.int32, device=dev)
    res = dict(device=torch.cuda.get_device_name(0), library=os.path.basename(_lib.LIB_PATH))
    res['uniform_kernel'] = time_draws(torch, lambda: _ops.sample_negatives(n, m, S, seed=100, device=dev, out=out), args.warmup, args.reps)
    if args.uniform_only:   # the parent's library: it has no weighted kernel
        return print(json.dumps(res), flush=True)
    idx, val = bench.gen_interactions(m, n, args.nnz, 'zipf', 0, dev)
    q = popularity(torch, idx, val, n, args.power)
    del idx, val
    heavy, total = int(torch.topk(q, S)[0].sum()), int(q.sum())
    res.update(power=args.power, total_weight=total, top_S_mass=heavy / total, weight_min_max=[int(q.min()), int(q.max())])
    res['weighted_kernel'] = time_draws(torch, lambda: _ops.sample_negatives(n, m, S, seed=100, device=dev, out=out, weights=q),
                                        args.warmup, args.reps)
    random_sampler_device(n, 4096, S, seed=100, device=dev, weights=q)   # torch's sort and search kernels loaded before the clock starts
    torch.cuda.synchronize()
    t0 = timeit.default_timer()
    want = random_sampler_device(n, m, S, seed=100, device=dev, weights=q)
    torch.cuda.synchronize()
    torch_ms = (timeit.default_timer() - t0) * 1e3
    kernel_ms = res['weighted_kernel']['ms']
    res.update(torch_ms=torch_ms, ratio=torch_ms / kernel_ms, faster=bool(kernel_ms < torch_ms), same_table=bool(torch.equal(out, want)),
               weighted_over_uniform=kernel_ms / res['uniform_kernel']['ms'])
    del want
    res['redraw_rounds'] = redraw_rounds(torch, n, m, S, 100, q, dev)
    print(json.dumps(res), flush=True)


def child_replan(args):
    import torch

    import bench
    from teamoflow_amd import _engine, _lib, _ops
    from time_logistic_c4 import timed_epochs
    _lib.get()
    dev = torch.device('cuda', 0)
    m, n, r, S = args.users, args.items, args.r, args.samples
    idx, val = bench.gen_interactions(m, n, args.nnz, 'zipf', 0, dev)
    q = popularity(torch, idx, val, n, args.power)
    plan = _engine.InteractionPlan(idx, val, m, n, user_chunks=1, csc=False)
    del idx, val
    U0, V0 = bench.init_table(m, r, 11, dev), bench.init_table(n, r, 7, dev)
    adam = _engine.adam_constants(args.lr)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    res = dict(library=os.path.basename(_lib.LIB_PATH), nnz=plan.nnz, power=args.power)
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

    wplan = _engine.wmrb_plan_for(plan, _ops.sample_negatives(n, m, S, seed=100, device=dev), r, force_sliced=True)
    wplan.sample_rank()
    st = _engine.TrainState(U0, V0, plan, r, wplan)
    del wplan

    def run(e):
        _engine.epoch_wmrb(st, adam, 0.0, loss, pairs='warp')
        st.swap()
    res['warp_epoch_ms_before_any_replan'] = timed_epochs(torch, run, args.epochs, 1)   # as tools/time_resample_c4.py: epochs first
    saved = (_engine.WmrbPlan.__init__, _engine.Scores7Plan.__init__, _engine.WmrbPlan.sample_rank, _engine.Scores7Plan.order_by_fill)
    _engine.WmrbPlan.__init__ = timed('wmrb_plan', saved[0])
    _engine.Scores7Plan.__init__ = timed('scores7_plan', saved[1])
    _engine.WmrbPlan.sample_rank = timed('sample_rank', saved[2])
    _engine.Scores7Plan.order_by_fill = timed('scores7_order_by_fill', saved[3])
    rebind = timed('set_negatives', st.set_negatives)
    for name, weights in (('uniform', None), ('popularity', q)):
        spans.clear()
        kw = {} if weights is None else dict(weights=weights)
        draw = timed('draw', lambda j: _ops.sample_negatives(n, m, S, seed=100 + j, device=dev, **kw))
        for j in (1, 2, 3):
            rebind(draw(j))
        split = {k: median(v) for k, v in spans.items()}
        split['set_negatives_each'] = spans['set_negatives']
        split['replan_total'] = split['draw'] + split['set_negatives']
        items = st.wplan.R_model.reshape(-1).to(torch.int64)
        res[name] = dict(replan_split_ms=split, scores7=st.wplan.s7 is not None, n_slices=st.wplan.n_slices,
                         longest_item_list=int(torch.bincount(items, minlength=n).max()),
                         warp_epoch_ms=timed_epochs(torch, run, args.epochs, 1))
        del items
    print(json.dumps(res), flush=True)


def child_quality(args):
    import torch

    import bench
    from teamoflow_amd import _lib
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import BPRLoss, WARPLoss
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
               k=10, top_S_mass={}, runs={})
    for power in (0.5, 0.75, 1.0):
        q = popularity(torch, train.indices, train.values, n, power)
        res['top_S_mass'][str(power)] = int(torch.topk(q, S)[0].sum()) / int(q.sum())
    for loss in (BPRLoss, WARPLoss):
        for every in (0, 1):
            for power in (None, 0.5, 0.75, 1.0):
                for bias in (False, True):
                    model = MatrixFactorization(r, loss_graph=loss(), user_weight_graph=FixedInitializer(U0),
                                                item_weight_graph=FixedInitializer(V0), n_users=m, n_items=n, n_samples=S)
                    model.verbose, model.random_ind, model.resample_every, model.scalar_item_bias = False, R, every, bias
                    if power is not None:
                        model.negative_sampling, model.sampling_power = 'popularity', power
                    name = (f'{loss.__name__} {"resample_every_1" if every else "static"} '
                            f'{"uniform" if power is None else f"power_{power}"} {"bias" if bias else "no_bias"}')
                    try:
                        model.fit(args.q_epochs, eye(m), eye(n), train, lr=args.q_lr)
                    except ValueError as e:   # the admission rule
                        res['runs'][name] = dict(refused=str(e))
                        continue
                    res['runs'][name] = dict(recall_at_10=float(model.recall_at_k(test, k=10, exclude=train).mean()),
                                             recall_at_10_train=float(model.recall_at_k(train, k=10).mean()),
                                             loss_first_last=[model.loss_history_[0], model.loss_history_[-1]],
                                             fit_seconds=model.fit_seconds_, plan_seconds=model.plan_seconds_,
                                             resample_seconds=model.resample_seconds_, rounds=model.resample_rounds_)
    print(json.dumps(res), flush=True)


def run_child(args, child, env_extra, limit, extra=()):
    """One measurement in a fresh process under its own time limit; any failure ends the whole run (nothing more is started)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', child, *extra]
    for k in ('users', 'items', 'r', 'nnz', 'samples', 'power', 'epochs', 'warmup', 'reps', 'lr', 'q_users', 'q_items', 'q_r', 'q_nnz',
              'q_samples', 'q_epochs', 'q_lr'):
        cmd += ['--' + k.replace('_', '-'), str(getattr(args, k))]
    print(f'[time_popularity_c4] {child} {env_extra}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=dict(os.environ, **env_extra), stdout=subprocess.PIPE, timeout=limit)
    if p.returncode != 0:
        raise SystemExit(f'{child} run failed with exit status {p.returncode}')
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help='libtmf.so built from the parent commit: its uniform sampler is recorded beside (a)')
    ap.add_argument('--also-lib', action='append', default=[], metavar='NAME=PATH',
                    help='(a) again with another build of libtmf.so (an experiment such as profiles/popularity_guide_table_experiment.patch), recorded as sampler_NAME')
    ap.add_argument('--epochs', type=int, default=3, help='timed WARP epochs on either table')
    ap.add_argument('--warmup', type=int, default=2, help='untimed launches of a sampler kernel')
    ap.add_argument('--reps', type=int, default=7, help='timed launches of a sampler kernel')
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--r', type=int, default=128)
    ap.add_argument('--nnz', type=int, default=100_000_000)
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--power', type=float, default=0.75)
    ap.add_argument('--lr', type=float, default=0.05)
    ap.add_argument('--q-users', type=int, default=50_000)
    ap.add_argument('--q-items', type=int, default=20_000)
    ap.add_argument('--q-r', type=int, default=64)
    ap.add_argument('--q-nnz', type=int, default=2_500_000)
    ap.add_argument('--q-samples', type=int, default=256)
    ap.add_argument('--q-epochs', type=int, default=30)
    ap.add_argument('--q-lr', type=float, default=0.05)
    ap.add_argument('--limit', type=int, default=420, help='seconds one child process may take')
    ap.add_argument('--only', default='sampler,parent,replan,quality', help='which measurements to run')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', choices=['sampler', 'replan', 'quality'], default=None)
    ap.add_argument('--uniform-only', action='store_true')
    args = ap.parse_args()
    if args.child:
        return dict(sampler=child_sampler, replan=child_replan, quality=child_quality)[args.child](args)
    only = args.only.split(',')
    if 'parent' in only and (not args.parent_lib or not os.path.exists(args.parent_lib)):
        raise SystemExit("--parent-lib: the library of the parent commit holds the uniform sampler recorded beside (a); build it first "
                         "(or leave 'parent' out of --only)")
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r, S=args.samples), power=args.power, lr=args.lr, epochs=args.epochs, reps=args.reps)
    if 'sampler' in only:
        res['sampler'] = run_child(args, 'sampler', {}, args.limit)
    if 'parent' in only:
        res['parent_uniform_sampler'] = run_child(args, 'sampler', dict(TMF_LIB=os.path.abspath(args.parent_lib), TMF_LIB_OLDER='1'), args.limit,
                                                  ['--uniform-only'])
    for spec in args.also_lib:
        name, path = spec.split('=', 1)
        res['sampler_' + name] = run_child(args, 'sampler', dict(TMF_LIB=os.path.abspath(path)), args.limit)
    if 'replan' in only:
        res['replan'] = run_child(args, 'replan', {}, args.limit)
    if 'quality' in only:
        res['quality'] = run_child(args, 'quality', {}, args.limit)
    if args.out and os.path.exists(args.out) and set(only) != {'sampler', 'parent', 'replan', 'quality'}:
        with open(args.out) as f:   # a partial run replaces its own parts of the file
            res = dict(json.load(f), **res)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
