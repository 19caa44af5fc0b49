"""What the logQ correction of SampledSoftmaxLoss costs and buys (sampling_correction='logq'; tmf_softmax_pairs_offset,
tmf_slot_offsets), at the C4 shape: 1M users x 100K items, r = 128, S = 1024, ~1e8 positives of bench.py's zipf generator, the
negative table drawn by popularity at power 0.75 and l = utils.log_expected_count of those weights.  Every bound is reported as met
or missed, never adjusted.

(a) pair.  On one popularity plan, with sp / pk of one scores pass, launches alternating, warm-up first, medians over ``--reps``
    launches between device events, the PARENT commit's library loaded as a second handle into the same process:
      offset       tmf_softmax_pairs_offset (c = 1)           bound: <= 1.65 x parent_plain (byte model 12.3 GB / 8.2 GB = 1.5, + 10 %)
      parent_plain the parent's tmf_softmax_pairs (c = 1)     the yardstick
      plain        this library's tmf_softmax_pairs           torch.equal outputs; its median inside [min, max] of the parent's runs
      unfused      the parent's tmf_item_bias_add with b = -l on a copy of sp, then its tmf_softmax_pairs: record only; its loss
                   agrees with the offset kernel's to 1e-5 (the add rounds once, like the kernel's subtraction)
      slot_offsets tmf_slot_offsets alone: first measurement, no bound, beside tmf_item_bias_add's 5.78 ms
(b) epoch.  The softmax epoch on that plan with the offsets and without, epochs alternating and not swapped in (both see the same
    tables); the uncorrected epoch runs the PARENT's pair kernel (its handle stands in for tmf_softmax_pairs; every other kernel of
    the epoch is this library's, whose sources the change does not touch).  Bound: the difference <= 1.10 x (offset - parent_plain
    of (a)) + the spread (max - min) of the parent's epochs.  One re-plan (TrainState.set_negatives) with and without the offsets.
(c) quality, record only.  The shape of profiles/resample_c4.json (50K x 20K, r = 64, S = 256, 30 epochs, lr 0.05), a tenth of the
    interactions held out, recall@10 with the training pairs excluded, SampledSoftmaxLoss on a static table and with
    resample_every = 1: uniform, uniform + catalog_scale, popularity at 0.5 / 0.75 / 1.0 each with and without 'logq'.
Every measurement is a child process under its own time limit (this process never opens the GPU); nothing is started after one fails.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/libtmf_parent.so
    python tools/time_logq_c4.py --parent-lib libtmf_parent.so [--only pair,epoch,quality] [--out profiles/logq_c4.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import timeit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
PAIR_BOUND, MARGIN = 1.65, 1.10


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def popularity_state(args, torch, dev):
    """(plan, TrainState on the popularity table of seed 100, q, l on the device): the plan a 'popularity' fit builds at C4."""
    import bench
    from teamoflow_amd import _engine, _ops
    from teamoflow_amd.mf.utils import log_expected_count
    from time_popularity_c4 import popularity
    m, n, r, S = args.users, args.items, args.r, args.samples
    idx, val = bench.gen_interactions(m, n, args.nnz, 'zipf', 0, dev)
    q = popularity(torch, idx, val, n, args.power)
    plan = _engine.InteractionPlan(idx, val, m, n, user_chunks=1, csc=False)
    del idx, val
    U0, V0 = bench.init_table(m, r, 11, dev), bench.init_table(n, r, 7, dev)
    R = _ops.sample_negatives(n, m, S, seed=100, device=dev, weights=q)
    wplan = _engine.wmrb_plan_for(plan, R, r, force_sliced=True)
    return plan, _engine.TrainState(U0, V0, plan, r, wplan), q, log_expected_count(q, S).to(dev)


def parent_handle(args, names):
    from teamoflow_amd import _lib
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    for name in names:
        fn = getattr(parent, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return parent


def child_pair(args):
    import torch

    from teamoflow_amd import _engine, _lib
    lib = _lib.get()
    dev = torch.device('cuda', 0)
    m, n, S = args.users, args.items, args.samples
    plan, st, q, ell = popularity_state(args, torch, dev)
    w = st.wplan
    parent = parent_handle(args, ('tmf_softmax_pairs', 'tmf_item_bias_add'))
    adam = _engine.adam_constants(args.lr)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    _engine.epoch_wmrb(st, adam, 1.0, loss, pairs='softmax')               # sp / pk of the state's tables; not swapped in
    torch.cuda.synchronize()
    off = w.slot_offsets(ell)
    neg_ell = (-ell).contiguous()
    sp_copy = torch.empty_like(st.sp)
    P, i32, i64, s = _lib.ptr, ctypes.c_int32, ctypes.c_int64, _lib.stream_ptr()
    head = (P(plan.rowptr_u), P(plan.val_u), P(st.pk))
    sizes = (i32(m), i32(S), 1.0)
    outs = (P(w.delta), P(w.D), P(st.loss_part), P(w.hinge_order), s)

    def unfused():
        sp_copy.copy_(st.sp)   # the add is in place: its input is restored first, outside the events
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(parent.tmf_item_bias_add(P(neg_ell), i32(n), P(w.R), i64(m), i32(S), P(sp_copy), None, i64(0), None, s))
        _lib.check(parent.tmf_softmax_pairs(*head, P(sp_copy), *sizes, *outs))
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def between_events(call):
        def run():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(call())
            b.record()
            b.synchronize()
            return a.elapsed_time(b)
        return run
    off_probe = torch.empty_like(off)
    launches = dict(offset=between_events(lambda: lib.tmf_softmax_pairs_offset(*head, P(st.sp), P(off), *sizes, *outs)),
                    parent_plain=between_events(lambda: parent.tmf_softmax_pairs(*head, P(st.sp), *sizes, *outs)),
                    plain=between_events(lambda: lib.tmf_softmax_pairs(*head, P(st.sp), *sizes, *outs)),
                    unfused=unfused,
                    slot_offsets=between_events(lambda: lib.tmf_slot_offsets(P(ell), i32(n), P(w.R), i64(m), i32(S), P(off_probe), s)))
    times, sums, kept = {k: [] for k in launches}, {}, {}
    for rep in range(args.warmup + args.reps):
        for k, run in launches.items():
            ms = run()
            if rep >= args.warmup:
                times[k].append(ms)
            if rep == 0 and k != 'slot_offsets':
                sums[k] = float(st.loss_part.double().sum()) / plan.n_pos
                if k in ('plain', 'parent_plain'):
                    kept[k] = (w.delta.clone(), w.D.clone(), st.loss_part.clone())
    ms = {k: median(v) for k, v in times.items()}
    spread = {k: [min(v), max(v)] for k, v in times.items()}
    res = dict(device=torch.cuda.get_device_name(0), library=os.path.basename(_lib.LIB_PATH), nnz=plan.nnz, n_pos=plan.n_pos, S=S,
               power=args.power, n_slices=w.n_slices, ms=ms, ms_min_max=spread, loss=sums,
               offset_GB_per_s=12e-6 * m * S / ms['offset'], plain_GB_per_s=8e-6 * m * S / ms['parent_plain'],
               slot_offsets_same_table=bool(torch.equal(off_probe, off)), item_bias_add_ms_recorded=5.78)
    res['offset_over_parent_plain'] = dict(ratio=ms['offset'] / ms['parent_plain'], bound=PAIR_BOUND,
                                           met=bool(ms['offset'] <= PAIR_BOUND * ms['parent_plain']))
    res['unfused'] = dict(ms=ms['unfused'], over_offset=ms['unfused'] / ms['offset'],
                          loss_rel_diff=abs(sums['unfused'] - sums['offset']) / abs(sums['offset']),
                          loss_agrees_to_1e_5=bool(abs(sums['unfused'] - sums['offset']) <= 1e-5 * abs(sums['offset'])))
    lo, hi = spread['parent_plain']
    res['plain_against_parent'] = dict(same_outputs=all(bool(torch.equal(a, b)) for a, b in zip(kept['plain'], kept['parent_plain'])),
                                       ms=ms['plain'], parent_min_max=[lo, hi], inside_parent_spread=bool(lo <= ms['plain'] <= hi))
    print(json.dumps(res), flush=True)


def child_epoch(args):
    import torch

    from teamoflow_amd import _engine, _lib
    lib = _lib.get()
    dev = torch.device('cuda', 0)
    plan, st, q, ell = popularity_state(args, torch, dev)
    parent = parent_handle(args, ('tmf_softmax_pairs',))
    adam = _engine.adam_constants(args.lr)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    off = st.wplan.slot_offsets(ell)

    class ParentPairs:   # the library with the parent's plain pair kernel in its place
        def __getattr__(self, name):
            return getattr(parent if name == 'tmf_softmax_pairs' else lib, name)
    shim = ParentPairs()

    def whole_epoch(corrected):
        """The epoch function itself between events; the uncorrected one through the shim in _lib's place."""
        st.wplan.off = off if corrected else None
        saved = _lib.get
        _lib.get = (lambda: lib) if corrected else (lambda: shim)
        try:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _engine.epoch_wmrb(st, adam, 1.0, loss, pairs='softmax')       # not swapped in: every epoch sees the same tables
            b.record()
            b.synchronize()
        finally:
            _lib.get = saved
        return a.elapsed_time(b), float(loss) / plan.n_pos
    times, losses = dict(corrected=[], parent=[]), {}
    for rep in range(args.warmup + args.epochs):
        for name, corrected in (('corrected', True), ('parent', False)):
            ms, l = whole_epoch(corrected)
            losses[name] = l
            if rep >= args.warmup:
                times[name].append(ms)
    ms = {k: median(v) for k, v in times.items()}
    res = dict(library=os.path.basename(_lib.LIB_PATH), epoch_ms=ms, epoch_ms_min_max={k: [min(v), max(v)] for k, v in times.items()},
               loss=losses, difference_ms=ms['corrected'] - ms['parent'],
               parent_spread_ms=max(times['parent']) - min(times['parent']))
    st.wplan.off = off
    prof = _engine.KernelTimer()
    for e in range(args.prof_epochs):
        _engine.epoch_wmrb(st, adam, 1.0, loss, prof=prof, pairs='softmax')
    torch.cuda.synchronize()
    res['corrected_kernels_ms'] = {k: prof.mean_ms(k) for k in prof.spans}
    # one re-plan with the offsets (the plan notes them: set_negatives builds them again) and one without
    from teamoflow_amd import _ops
    replan = {}
    for name, j in (('with_offsets', 1), ('without_offsets', 2)):
        if name == 'without_offsets':
            st.wplan.off, st.wplan.prepared = None, []
        R = _ops.sample_negatives(args.items, args.users, args.samples, seed=100 + j, device=dev, weights=q)
        torch.cuda.synchronize()
        t0 = timeit.default_timer()
        st.set_negatives(R)
        torch.cuda.synchronize()
        replan[name] = dict(set_negatives_ms=(timeit.default_timer() - t0) * 1e3, has_offsets=st.wplan.off is not None)
    res['replan'] = replan
    print(json.dumps(res), flush=True)


def child_quality(args):
    import torch

    import bench
    from teamoflow_amd import _lib
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import SampledSoftmaxLoss
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
    cases = [('uniform', None, False, 'none'), ('uniform catalog_scale', None, True, 'none')]
    for power in (0.5, 0.75, 1.0):
        cases += [(f'power_{power}', power, False, 'none'), (f'power_{power} logq', power, False, 'logq')]
    for every in (0, 1):
        for label, power, scale, correction in cases:
            model = MatrixFactorization(r, loss_graph=SampledSoftmaxLoss(scale), user_weight_graph=FixedInitializer(U0),
                                        item_weight_graph=FixedInitializer(V0), n_users=m, n_items=n, n_samples=S)
            model.verbose, model.random_ind, model.resample_every, model.sampling_correction = False, R, every, correction
            if power is not None:
                model.negative_sampling, model.sampling_power = 'popularity', power
            name = f'{"resample_every_1" if every else "static"} {label}'
            try:
                model.fit(args.q_epochs, eye(m), eye(n), train, lr=args.q_lr)
            except ValueError as e:   # the admission rule
                res['runs'][name] = dict(refused=str(e))
                continue
            res['runs'][name] = dict(recall_at_10=float(model.recall_at_k(test, k=10, exclude=train).mean()),
                                     recall_at_10_train=float(model.recall_at_k(train, k=10).mean()),
                                     loss_first_last=[model.loss_history_[0], model.loss_history_[-1]],
                                     fit_seconds=model.fit_seconds_, resample_seconds=model.resample_seconds_,
                                     rounds=model.resample_rounds_)
    print(json.dumps(res), flush=True)


def run_child(args, child, limit):
    """One measurement in a fresh process under its own time limit; any failure ends the whole run (nothing more is started)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', child]
    if args.parent_lib:
        cmd += ['--parent-lib', os.path.abspath(args.parent_lib)]
    for k in ('users', 'items', 'r', 'nnz', 'samples', 'power', 'epochs', 'prof_epochs', 'warmup', 'reps', 'lr', 'q_users', 'q_items',
              'q_r', 'q_nnz', 'q_samples', 'q_epochs', 'q_lr'):
        cmd += ['--' + k.replace('_', '-'), str(getattr(args, k))]
    print(f'[time_logq_c4] {child}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=limit)
    if p.returncode != 0:
        raise SystemExit(f'{child} run failed with exit status {p.returncode}')
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help='libtmf.so built from the parent commit: its pair kernel and its add pass are the yardsticks')
    ap.add_argument('--epochs', type=int, default=7, help='timed epochs of either form, alternating')
    ap.add_argument('--prof-epochs', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2, help='untimed launches of every kernel / epochs of either form')
    ap.add_argument('--reps', type=int, default=15, help='timed launches of every kernel')
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
    ap.add_argument('--only', default='pair,epoch,quality', help='which measurements to run')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', choices=['pair', 'epoch', 'quality'], default=None)
    args = ap.parse_args()
    if args.child:
        return dict(pair=child_pair, epoch=child_epoch, quality=child_quality)[args.child](args)
    only = args.only.split(',')
    if {'pair', 'epoch'} & set(only) and (not args.parent_lib or not os.path.exists(args.parent_lib)):
        raise SystemExit("--parent-lib: the library of the parent commit holds the yardsticks of (a) and (b); build it first (or run "
                         "--only quality)")
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r, S=args.samples), power=args.power, lr=args.lr, epochs=args.epochs,
               reps=args.reps, warmup=args.warmup)
    for name in ('pair', 'epoch', 'quality'):
        if name in only:
            res[name] = run_child(args, name, args.limit)
    if args.out and os.path.exists(args.out) and set(only) != {'pair', 'epoch', 'quality'}:
        with open(args.out) as f:   # a partial run replaces its own parts of the file
            res = dict(json.load(f), **res)
    if 'pair' in res and 'epoch' in res:   # the epoch's bound needs the kernels' difference of (a)
        ms, ep = res['pair']['ms'], res['epoch']
        allowed = MARGIN * (ms['offset'] - ms['parent_plain']) + ep['parent_spread_ms']
        res['epoch_bound'] = dict(difference_ms=ep['difference_ms'], allowed_ms=allowed, met=bool(ep['difference_ms'] <= allowed))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
