"""Cost and quality of FullSoftmaxLoss (csrc/tmf_fullsoftmax.hip) on the sparse engine.

The kernels at C4 (1M users x 100K items, r = 128, bench.py's zipf interactions and tables).  tmf_fsm_lse_f32 against
tmf_predict_topk_f32 (k = 10) of the PARENT commit's library, loaded as a second handle into the same process so that both sweep the
same tables: launches alternate, warm-up first, medians over ``--reps`` launches between device events.  Bound: lse <= 1.10 x top-k,
the margin of a kernel that shares its yardstick's loop.  tmf_fsm_wsum_f32 in both orientations against 2 x that yardstick (two
products per tile): first measurement, no bound.  Then ``--epochs`` whole epochs between two device events and per-kernel times
through _engine.KernelTimer, beside the recorded epochs of the sampled losses (profiles/softmax_c4.json, profiles/resample_c4.json).
The epoch at a MovieLens-20M-like shape (138K x 27K, r = 128, 2e7 interactions): first measurement, no bound.
Quality at the shape of profiles/resample_c4.json (50K x 20K, r = 64, 2.2M training interactions, 30 epochs, lr 0.05): held-out
recall@10 with the training pairs excluded and the fit's seconds, beside the recorded figures of WARP on a static and a resampled table.
Every measurement is a child process under its own time limit (this process never opens the GPU); nothing is started after one fails;
at most 16 threads.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/build/libtmf_parent.so
    python tools/time_fullsoftmax_c4.py --parent-lib build/libtmf_parent.so [--out profiles/fullsoftmax_c4.json]
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
THREADS = 16
SPANS = ('fsm_lse', 'fsm_user_pass', 'fsm_item_pass', 'fsm_wsum_user', 'fsm_wsum_item', 'fsm_user_step', 'fsm_item_step')


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def full_state(args, torch, dev, m, n, r, nnz):
    import bench
    from teamoflow_amd import _engine
    idx, val = bench.gen_interactions(m, n, nnz, 'zipf', 0, dev)
    plan = _engine.InteractionPlan(idx, val, m, n, csc=True)
    del idx, val
    return plan, _engine.TrainState(bench.init_table(m, r, 11, dev), bench.init_table(n, r, 7, dev), plan, r, full_softmax=True)


def epoch_times(args, torch, st, plan):
    from teamoflow_amd import _engine
    from time_logistic_c4 import timed_epochs
    adam = _engine.adam_constants(args.lr)
    loss = torch.zeros(1, dtype=torch.float64, device=st.U.device)

    def run(e, prof=None):
        _engine.epoch_sides(st, adam, loss, 'full_softmax', 0.0, prof)
    res = dict(epoch_ms=timed_epochs(torch, run, args.epochs, 1), loss_after=float(loss) / max(plan.n_pos, 1))
    prof = _engine.KernelTimer()
    for e in range(args.prof_epochs):
        run(e, prof)
    torch.cuda.synchronize()
    res['kernels_ms'] = {k: prof.mean_ms(k) for k in SPANS if k in prof.spans}
    return res


def child_c4(args):
    import torch

    from teamoflow_amd import _lib
    torch.set_num_threads(THREADS)
    lib = _lib.get()
    dev = torch.device('cuda', 0)
    m, n, r = args.users, args.items, args.r
    plan, st = full_state(args, torch, dev, m, n, r, args.nnz)
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))                 # a second handle: only its fused top-k is called
    parent.tmf_predict_topk_f32.restype, parent.tmf_predict_topk_f32.argtypes = _lib.SIGNATURES['tmf_predict_topk_f32']
    P, s, ld = _lib.ptr, _lib.stream_ptr(), st.ld
    top = torch.empty(m, 10, dtype=torch.int32, device=dev)
    gU, gV = torch.zeros_like(st.U), torch.zeros_like(st.V)
    launches = dict(
        lse=lambda: lib.tmf_fsm_lse_f32(P(st.U), P(st.V), m, n, r, ld, ld, P(st.fsm_lse), s),
        topk_parent=lambda: parent.tmf_predict_topk_f32(P(st.U), P(st.V), m, n, r, ld, ld, 10, 0, P(top), None, s),
        wsum_users_stationary=lambda: lib.tmf_fsm_wsum_f32(P(st.U), P(st.V), m, n, r, ld, ld, P(st.fsm_lse), P(st.fsm_w), 1, P(gU), ld, s),
        wsum_items_stationary=lambda: lib.tmf_fsm_wsum_f32(P(st.V), P(st.U), n, m, r, ld, ld, P(st.fsm_lse), P(st.fsm_w), 0, P(gV), ld, s))
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
    ms = {k: median(v) for k, v in times.items()}
    tflop = 2e-12 * m * n * r
    props = torch.cuda.get_device_properties(0)
    res = dict(nnz=plan.nnz, n_pos=plan.n_pos, device=torch.cuda.get_device_name(0), compute_units=props.multi_processor_count,
               library=os.path.basename(_lib.LIB_PATH), users_with_a_positive=int((st.fsm_w > 0).sum()), ms=ms,
               ms_min_max={k: [min(v), max(v)] for k, v in times.items()}, tflop_per_product=tflop,
               tflops=dict(lse=tflop / ms['lse'] * 1e3, topk_parent=tflop / ms['topk_parent'] * 1e3,
                           wsum_users_stationary=2 * tflop / ms['wsum_users_stationary'] * 1e3,
                           wsum_items_stationary=2 * tflop / ms['wsum_items_stationary'] * 1e3))
    del gU, gV, top
    res['epoch'] = epoch_times(args, torch, st, plan)
    print(json.dumps(res), flush=True)


def child_ml20m(args):
    import torch

    from teamoflow_amd import _lib
    torch.set_num_threads(THREADS)
    _lib.get()
    dev = torch.device('cuda', 0)
    m, n, r, nnz = 138_000, 27_000, 128, 20_000_000
    plan, st = full_state(args, torch, dev, m, n, r, nnz)
    res = dict(shape=dict(m=m, n=n, r=r), nnz=plan.nnz, n_pos=plan.n_pos, flop_model_ms_at_120_tf=5 * 2e-12 * m * n * r / 120 * 1e3)
    res.update(epoch_times(args, torch, st, plan))
    print(json.dumps(res), flush=True)


def child_quality(args):
    import torch

    import bench
    from teamoflow_amd import _lib
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import FullSoftmaxLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    torch.set_num_threads(THREADS)
    _lib.get()
    dev = torch.device('cuda', 0)
    m, n, r, nnz = args.q_users, args.q_items, args.q_r, args.q_nnz
    idx, val = bench.gen_interactions(m, n, nnz, 'zipf', 0, dev)                      # the split of tools/time_resample_c4.py
    held = torch.rand(val.numel(), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) < 0.1
    train = SparseInteractions(torch.stack([idx[:, 0][~held], idx[:, 1][~held]], 1), val[~held], (m, n))
    test = SparseInteractions(torch.stack([idx[:, 0][held], idx[:, 1][held]], 1), val[held], (m, n))
    U0, V0 = bench.init_table(m, r, 11, dev), bench.init_table(n, r, 7, dev)
    model = MatrixFactorization(r, loss_graph=FullSoftmaxLoss(), user_weight_graph=FixedInitializer(U0), item_weight_graph=FixedInitializer(V0),
                                n_users=m, n_items=n)
    model.verbose = False
    model.fit(args.q_epochs, eye(m), eye(n), train, lr=args.q_lr)
    res = dict(shape=dict(m=m, n=n, r=r, nnz_train=int((~held).sum()), nnz_test=int(held.sum())), epochs=args.q_epochs, lr=args.q_lr, k=10,
               recall_at_10=float(model.recall_at_k(test, k=10, exclude=train).mean()),
               recall_at_10_train=float(model.recall_at_k(train, k=10).mean()),
               loss_first_last=[model.loss_history_[0], model.loss_history_[-1]], fit_seconds=model.fit_seconds_,
               plan_seconds=model.plan_seconds_, rounds=model.resample_rounds_)
    print(json.dumps(res), flush=True)


def run_child(args, child, limit):
    """One measurement in a fresh process under its own time limit; any failure ends the whole run (nothing more is started)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', child, '--parent-lib', os.path.abspath(args.parent_lib)]
    for k in ('users', 'items', 'r', 'nnz', 'epochs', 'prof_epochs', 'warmup', 'reps', 'lr', 'q_users', 'q_items', 'q_r', 'q_nnz', 'q_epochs',
              'q_lr'):
        cmd += ['--' + k.replace('_', '-'), str(getattr(args, k))]
    print(f'[time_fullsoftmax_c4] {child}', file=sys.stderr, flush=True)
    env = dict(os.environ, OMP_NUM_THREADS=str(min(THREADS, int(os.environ.get('OMP_NUM_THREADS', THREADS)))))
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=limit)
    if p.returncode != 0:
        raise SystemExit(f'{child} run failed with exit status {p.returncode}')
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def recorded(name, *path):
    """A figure an earlier measurement left in profiles/ (None when the file or the field is not there)."""
    try:
        d = json.loads(open(os.path.join(ROOT, 'profiles', name)).read().strip().splitlines()[-1])
        for k in path:
            d = d[k]
        return d
    except (OSError, KeyError, ValueError, IndexError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help='libtmf.so built from the parent commit: its fused fp32 top-k is the yardstick')
    ap.add_argument('--epochs', type=int, default=3, help='timed epochs')
    ap.add_argument('--prof-epochs', type=int, default=2)
    ap.add_argument('--warmup', type=int, default=1, help='untimed launches of every kernel')
    ap.add_argument('--reps', type=int, default=5, help='timed launches of every kernel')
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--r', type=int, default=128)
    ap.add_argument('--nnz', type=int, default=100_000_000)
    ap.add_argument('--lr', type=float, default=0.05)
    ap.add_argument('--q-users', type=int, default=50_000)
    ap.add_argument('--q-items', type=int, default=20_000)
    ap.add_argument('--q-r', type=int, default=64)
    ap.add_argument('--q-nnz', type=int, default=2_500_000)
    ap.add_argument('--q-epochs', type=int, default=30)
    ap.add_argument('--q-lr', type=float, default=0.05)
    ap.add_argument('--limit', type=int, default=420, help='seconds one child process may take')
    ap.add_argument('--only', default='c4,ml20m,quality', help='which measurements to run')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', choices=['c4', 'ml20m', 'quality'], default=None)
    args = ap.parse_args()
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit('--parent-lib: the library of the parent commit holds the yardstick of this measurement; build it first')
    if args.child:
        return dict(c4=child_c4, ml20m=child_ml20m, quality=child_quality)[args.child](args)
    only = args.only.split(',')
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r), lr=args.lr, epochs=args.epochs, reps=args.reps, warmup=args.warmup,
               margin=MARGIN)
    if 'c4' in only:
        c4 = run_child(args, 'c4', args.limit)
        ms = c4['ms']
        res['c4'] = c4
        res['lse'] = dict(ratio=ms['lse'] / ms['topk_parent'], bound=MARGIN, met=bool(ms['lse'] <= MARGIN * ms['topk_parent']))
        res['wsum_ratio_to_two_products'] = {k: ms[k] / (2 * ms['topk_parent']) for k in ('wsum_users_stationary', 'wsum_items_stationary')}
        res['c4_epochs_ms'] = dict(full_softmax=c4['epoch']['epoch_ms'],
                                   wmrb_recorded=recorded('softmax_c4.json', 'parent', 'wmrb_epoch_ms'),
                                   sampled_softmax_recorded=recorded('softmax_c4.json', 'softmax', 'softmax_epoch_ms'),
                                   warp_resample_every_1_recorded=recorded('resample_c4.json', 'this', 'warp', 'resample_every_1_epoch_ms'))
    if 'ml20m' in only:
        res['ml20m'] = run_child(args, 'ml20m', args.limit)
    if 'quality' in only:
        res['quality'] = run_child(args, 'quality', args.limit)
        res['quality']['warp_recorded'] = {k: recorded('resample_c4.json', 'quality', 'runs', k, 'recall_at_10')
                                           for k in ('static', 'resample_every_1', 'resample_every_5')}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
