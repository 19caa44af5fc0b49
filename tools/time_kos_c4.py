"""Cost of KOSWARPLoss on the sparse engine at the C4 shape (1M users x 100K items, r = 128, S = 1024, ~1e8 positives of bench.py's
generator and negative table), beside the ranked WARP pair step and the WARP epoch of the PARENT commit's library on the same plan.

The weights.  tmf_kos_weights alone on the state's rowptr, val and pk: the median of ``--reps`` launches between device events after
a warm-up, its rate against the bytes it must move (rowptr, val and p read, omega written), the longest user row, and the sum of
the weights per user.  A first measurement: no bound.
The pair step.  tmf_warp_pairs_kos (with ranks, the form the engine calls) against tmf_warp_pairs_ranked of the parent's library,
loaded as a second handle into the same process, on the same rowptr, val, pk, sp, rank and user order: launches alternate.  Bound:
kos <= 1.10 x ranked.
Both twice: with sp / pk of one scores pass over freshly initialised tables, and after ten KOS epochs.
Single rows.  tmf_kos_weights on tables of one user with 100 ... 100 000 positives (random scores), one wave each: what a row of
that length costs by itself, the segmented path (more than 2048 positives) included.
The epoch.  Ten KOS epochs between two device events and per-kernel times through _engine.KernelTimer, beside the parent library's
WARP epoch (a child process of its own: a library is chosen when the package is imported).  Bound: kos epoch <= 1.10 x (parent's
WARP epoch + tmf_kos_weights alone).
Quality (no bound).  tools/time_resample_c4.py's mid shape, a tenth of the interactions held out: recall@10 with exclude=train of
KOSWARPLoss(5, 10) on the static table and with resample_every = 1.
Every measurement is a child process under its own time limit (this process never opens the GPU); nothing is started after one fails.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/libtmf_parent.so
    python tools/time_kos_c4.py --parent-lib libtmf_parent.so [--out profiles/kos_c4.json]
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
SPANS = ('wmrb_scores', 'kos_weights', 'warp_pairs', 'wmrb_gradu', 'wmrb_finish', 'wmrb_user_pass', 'wmrb_item_pass', 'wmrb_combine')


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def child_kos(args):
    import torch

    from teamoflow_amd import _engine, _lib
    from time_logistic_c4 import timed_epochs
    from time_warp_c4 import c4_state
    lib = _lib.get()
    dev = torch.device('cuda', 0)
    m, n, S, kn = args.users, args.items, args.samples, (args.k, args.n)
    plan, w, st = c4_state(args, torch, dev, force_sliced=True)
    rank, omega = w.sample_rank(), w.kos_omega(plan.nnz)
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))                 # a second handle: only its ranked WARP step is called
    parent.tmf_warp_pairs_ranked.restype, parent.tmf_warp_pairs_ranked.argtypes = _lib.SIGNATURES['tmf_warp_pairs_ranked']
    adam = _engine.adam_constants(args.lr)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    P, i32, s = _lib.ptr, ctypes.c_int32, _lib.stream_ptr()
    common = (P(plan.rowptr_u), P(plan.val_u), P(st.pk), P(st.sp))
    outs = (i32(m), i32(S), i32(n), P(w.delta), P(w.D), P(st.loss_part), P(w.hinge_order), s)
    launches = dict(
        kos_weights=lambda: lib.tmf_kos_weights(*common[:3], i32(m), i32(kn[0]), i32(kn[1]), P(omega), P(w.hinge_order), s),
        warp_pairs_kos=lambda: lib.tmf_warp_pairs_kos(*common, P(rank), P(omega), *outs),
        warp_ranked_parent=lambda: parent.tmf_warp_pairs_ranked(*common, P(rank), *outs),
        warp_ranked_this=lambda: lib.tmf_warp_pairs_ranked(*common, P(rank), *outs))
    pos = plan.val_u > 0
    rows = torch.diff(plan.rowptr_u)
    positives = torch.zeros(m, dtype=torch.int64, device=dev).index_add_(0, plan.user_of.to(torch.int64), pos.to(torch.int64))
    model_bytes = 8 * (m + 1) + 12 * plan.nnz                              # rowptr, val and p read, omega written

    def pair_step():
        """sp / pk of the state's tables by one epoch that is not swapped in, then the launches in turn."""
        _engine.epoch_wmrb(st, adam, kn, loss, pairs='warp_kos')
        torch.cuda.synchronize()
        sums = torch.zeros(m, dtype=torch.float64, device=dev).index_add_(0, plan.user_of.to(torch.int64), omega.double())
        out = dict(loss=float(loss) / plan.n_pos, D_nonzero_share=float((w.D != 0).float().mean()),
                   positives_with_a_weight=float((w.delta[pos] < 0).float().mean()),
                   omega_sum_max_dev=float((sums[positives > 0] - 1).abs().max()), omega_zero_share_of_positives=float((omega[pos] == 0).float().mean()))
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
        out['kos_weights_gbps_against_the_byte_model'] = model_bytes / out['ms']['kos_weights'] / 1e6
        return out

    props = torch.cuda.get_device_properties(0)
    res = dict(nnz=plan.nnz, n_pos=plan.n_pos, S=S, k=kn[0], n=kn[1], n_slices=w.n_slices, device=torch.cuda.get_device_name(0),
               compute_units=props.multi_processor_count, library=os.path.basename(_lib.LIB_PATH), kos_weights_model_bytes=model_bytes,
               longest_row_entries=int(rows.max()), longest_row_positives=int(positives.max()),
               rows_over_one_segment=int((positives > 2048).sum()), mean_positives=float(positives.double().mean()))
    res['pair_step_fresh'] = pair_step()

    def run(e, prof=None):
        _engine.epoch_wmrb(st, adam, kn, loss, prof=prof, pairs='warp_kos')
        st.swap()
    res['kos_epoch_ms'] = timed_epochs(torch, run, args.epochs, 0)         # the pair step above has warmed every kernel
    res['kos_loss_after'] = float(loss) / plan.n_pos
    res['pair_step_trained'] = dict(pair_step(), epochs_before=args.epochs)
    prof = _engine.KernelTimer()
    for e in range(args.prof_epochs):
        run(e, prof)
    torch.cuda.synchronize()
    res['kos_kernels_ms'] = {k: prof.mean_ms(k) for k in SPANS if k in prof.spans}
    res['D_nonzero_share_at_the_end'] = float((w.D != 0).float().mean())
    print(json.dumps(res), flush=True)


def child_rows(args):
    """One user with P positives, the kernel's one wave alone on the device: ms per launch."""
    import torch

    from teamoflow_amd import _lib
    lib = _lib.get()
    dev = torch.device('cuda', 0)
    P_, i32, s = _lib.ptr, ctypes.c_int32, _lib.stream_ptr()
    res = {}
    for P in (100, 2048, 2049, 2650, 4096, 16384, 100_000):
        rowptr = torch.tensor([0, P], dtype=torch.int64, device=dev)
        val = torch.ones(P, device=dev)
        p = torch.randn(P, device=dev, generator=torch.Generator(device=dev).manual_seed(P))
        omega = torch.full((P,), float('nan'), device=dev)
        times = []
        for rep in range(args.warmup + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(lib.tmf_kos_weights(P_(rowptr), P_(val), P_(p), i32(1), i32(args.k), i32(args.n), P_(omega), None, s))
            b.record()
            b.synchronize()
            if rep >= args.warmup:
                times.append(a.elapsed_time(b))
        res[str(P)] = dict(ms=median(times), ms_min_max=[min(times), max(times)], segments=-(-P // 2048), omega_sum=float(omega.double().sum()))
    print(json.dumps(res), flush=True)


def child_warp(args):
    """The WARP epoch of the library the environment names (the parent's) on the same plan."""
    import torch

    from teamoflow_amd import _engine, _lib
    from time_logistic_c4 import timed_epochs
    from time_warp_c4 import c4_state
    _lib.get()
    dev = torch.device('cuda', 0)
    plan, w, st = c4_state(args, torch, dev, force_sliced=True)
    w.sample_rank()
    adam = _engine.adam_constants(args.lr)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)

    def run(e, prof=None):
        _engine.epoch_wmrb(st, adam, 0.0, loss, prof=prof, pairs='warp')
        st.swap()
    res = dict(library=os.path.basename(_lib.LIB_PATH), warp_epoch_ms=timed_epochs(torch, run, args.epochs, 1))
    prof = _engine.KernelTimer()
    for e in range(args.prof_epochs):
        run(e, prof)
    torch.cuda.synchronize()
    res['warp_kernels_ms'] = {k: prof.mean_ms(k) for k in SPANS if k in prof.spans}
    res['D_nonzero_share_at_the_end'] = float((w.D != 0).float().mean())
    print(json.dumps(res), flush=True)


def child_quality(args):
    import torch

    import bench
    from teamoflow_amd import _lib
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import KOSWARPLoss
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
               k_at=10, kos=[args.k, args.n], runs={})
    for name, every in (('static', 0), ('resample_every_1', 1)):
        model = MatrixFactorization(r, loss_graph=KOSWARPLoss(args.k, args.n), user_weight_graph=FixedInitializer(U0),
                                    item_weight_graph=FixedInitializer(V0), n_users=m, n_items=n, n_samples=S)
        model.verbose, model.random_ind, model.resample_every = False, R, every
        model.fit(args.q_epochs, eye(m), eye(n), train, lr=args.q_lr)
        res['runs'][name] = dict(recall_at_10=float(model.recall_at_k(test, k=10, exclude=train).mean()),
                                 recall_at_10_train=float(model.recall_at_k(train, k=10).mean()),
                                 loss_first_last=[model.loss_history_[0], model.loss_history_[-1]],
                                 fit_seconds=model.fit_seconds_, resample_seconds=model.resample_seconds_, rounds=model.resample_rounds_)
    print(json.dumps(res), flush=True)


def run_child(args, child, env_extra, limit):
    """One measurement in a fresh process under its own time limit; any failure ends the whole run (nothing more is started)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', child, '--parent-lib', os.path.abspath(args.parent_lib)]
    for k in ('users', 'items', 'r', 'nnz', 'samples', 'epochs', 'prof_epochs', 'warmup', 'reps', 'lr', 'k', 'n', 'q_users', 'q_items', 'q_r',
              'q_nnz', 'q_samples', 'q_epochs', 'q_lr'):
        cmd += ['--' + k.replace('_', '-'), str(getattr(args, k))]
    print(f'[time_kos_c4] {child} {env_extra}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=dict(os.environ, **env_extra), stdout=subprocess.PIPE, timeout=limit)
    if p.returncode != 0:
        raise SystemExit(f'{child} run failed with exit status {p.returncode}')
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help='libtmf.so built from the parent commit: its ranked WARP step and its WARP epoch are the yardsticks')
    ap.add_argument('--epochs', type=int, default=10, help='KOS epochs between the two pair-step measurements (timed)')
    ap.add_argument('--prof-epochs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3, help='untimed launches of every kernel')
    ap.add_argument('--reps', type=int, default=15, help='timed launches of every kernel')
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--r', type=int, default=128)
    ap.add_argument('--nnz', type=int, default=100_000_000)
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--lr', type=float, default=0.05)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--n', type=int, default=10)
    ap.add_argument('--q-users', type=int, default=50_000)
    ap.add_argument('--q-items', type=int, default=20_000)
    ap.add_argument('--q-r', type=int, default=64)
    ap.add_argument('--q-nnz', type=int, default=2_500_000)
    ap.add_argument('--q-samples', type=int, default=256)
    ap.add_argument('--q-epochs', type=int, default=30)
    ap.add_argument('--q-lr', type=float, default=0.05)
    ap.add_argument('--limit', type=int, default=420, help='seconds one child process may take')
    ap.add_argument('--only', default='kos,parent,quality,rows', help='which measurements to run')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', choices=['kos', 'warp', 'quality', 'rows'], default=None)
    args = ap.parse_args()
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit('--parent-lib: the library of the parent commit holds the yardsticks of this measurement; build it first')
    if args.child:
        return dict(kos=child_kos, warp=child_warp, quality=child_quality, rows=child_rows)[args.child](args)
    only = args.only.split(',')
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r, S=args.samples), kos=[args.k, args.n], lr=args.lr, epochs=args.epochs,
               reps=args.reps, warmup=args.warmup, margin=MARGIN)
    if 'kos' in only:
        kos = res['kos_run'] = run_child(args, 'kos', {}, args.limit)
        res['pair_step'] = {}
        for state in ('pair_step_fresh', 'pair_step_trained'):
            ms = kos[state]['ms']
            res['pair_step'][state] = dict(ratio=ms['warp_pairs_kos'] / ms['warp_ranked_parent'], bound=MARGIN,
                                           met=bool(ms['warp_pairs_kos'] <= MARGIN * ms['warp_ranked_parent']),
                                           kos_weights_over_ranked_parent=ms['kos_weights'] / ms['warp_ranked_parent'])
    if 'parent' in only:
        res['parent'] = run_child(args, 'warp', dict(TMF_LIB=os.path.abspath(args.parent_lib), TMF_LIB_OLDER='1'), args.limit)
    if 'kos' in only and 'parent' in only:
        allowed = MARGIN * (res['parent']['warp_epoch_ms'] + res['kos_run']['pair_step_trained']['ms']['kos_weights'])
        res['epoch'] = dict(kos_epoch_ms=res['kos_run']['kos_epoch_ms'], parent_warp_epoch_ms=res['parent']['warp_epoch_ms'],
                            bound_ms=allowed, met=bool(res['kos_run']['kos_epoch_ms'] <= allowed))
    if 'quality' in only:
        res['quality'] = run_child(args, 'quality', {}, args.limit)
    if 'rows' in only:
        res['single_rows'] = run_child(args, 'rows', {}, args.limit)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
