"""Cost and effect of the scalar item bias (scalar_item_bias; csrc/tmf_itembias.hip) at the C4 shape (1M users x 100K items, r = 128,
S = 1024, ~1e8 positives of bench.py's generator and negative table), against the PARENT commit's library on the same plan, tables
and weights.  The parent's library is loaded as a second handle into the measuring process and takes the engine's place launch by
launch (``use``), so that its kernels and epochs alternate with this library's on the same buffers; every figure is a median over
``--reps`` runs between device events after ``--warmup`` untimed ones.

(a) tmf_item_bias_add alone against the parent's tmf_softmax_pairs on the same sp (8.19 GB streamed against 12.3 GB):
    bound 1.5 x 1.25 x that time.
(b) tmf_item_bias_grad alone, on the weights a WMRB epoch leaves, against the parent's item pass (tmf_wsum_pass + combine, or
    tmf_wsum_rows5, whichever the plan runs) on the same plan and weights: bound 0.5 x that time.
(c) The epoch of WMRB, WARP and sampled softmax: the parent's, this library's with the bias off and with it on, in turn.  Bound: on -
    parent <= 1.10 x ((a) + (b) alone); off within the spread of the parent's own runs.
(d) predict_topk(k = 10) over all users on the augmented width 129 against width 128, 'split' and 'fp32' (no bound; the ranking
    kernels are the parent's, unchanged).
(e) Quality at 50K x 20K zipf, r = 64, S = 256, 30 epochs, lr 0.05, training pairs excluded: held-out recall@10 of WARP and BPR with
    and without the bias, on the static table and with resample_every = 1 (no bound).
Every measurement is a child process under its own time limit (this process never opens the GPU); nothing is started after one fails.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/libtmf_parent.so
    python tools/time_item_bias_c4.py --parent-lib libtmf_parent.so [--out profiles/item_bias_c4.json]
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
ADD_BOUND, GRAD_BOUND, EPOCH_MARGIN = 1.5 * 1.25, 0.5, 1.10


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def stats(v):
    return dict(ms=median(v), min=min(v), max=max(v))


def child_c4(args):
    import torch

    from teamoflow_amd import _engine, _lib, _ops
    from teamoflow_amd.mf.matrix_factorization import augmented_tables
    from time_warp_c4 import c4_state
    this = _lib.get()
    dev = torch.device('cuda', 0)
    m, n, r, S = args.users, args.items, args.r, args.samples
    plan, w, st = c4_state(args, torch, dev, force_sliced=True)
    w.sample_rank()
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    for name, (res, argtypes) in _lib.SIGNATURES.items():       # the parent lacks what this commit adds: those are never called on it
        if hasattr(parent, name):
            getattr(parent, name).restype, getattr(parent, name).argtypes = res, argtypes

    def use(lib):
        _lib._lib = lib                                          # what _lib.get() hands the engine from now on
    ib = _engine.ItemScalarBias(torch.randn(n, device=dev) * 1e-3, n, dev)
    ib.adopt(w)
    ib.epi = _lib.EPI_GRAD                                       # alone: the gradient, the bias stays
    adam = _engine.adam_constants(args.lr)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    s, c = _lib.stream_ptr(), n / S

    def timed(calls, reps=args.reps, warmup=args.warmup):
        times = {k: [] for k in calls}
        for rep in range(warmup + reps):
            for k, call in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                b.synchronize()
                if rep >= warmup:
                    times[k].append(a.elapsed_time(b))
        return {k: stats(v) for k, v in times.items()}

    props = torch.cuda.get_device_properties(0)
    res = dict(nnz=plan.nnz, n_pos=plan.n_pos, S=S, n_slices=w.n_slices, user_chunks=w.user_chunks, rows4=w.rows4,
               device=torch.cuda.get_device_name(0), compute_units=props.multi_processor_count, n_extra_chunks=ib.n_extra,
               longest_item_list=int((w.rowptr_e[1:] - w.rowptr_e[:-1]).view(w.user_chunks, n).sum(0).max()),
               bias_workspace_bytes=ib.ws.numel() * 8, bytes_add=12 * m * S + 12 * plan.nnz)
    # ---- the weights a WMRB epoch leaves ----
    use(this)
    _engine.epoch_wmrb(st, adam, c, loss, pairs='hinge')
    torch.cuda.synchronize()
    res['D_nonzero_share'] = float((w.D != 0).float().mean())

    def item_pass(lib):
        V_out, v = st.V_nxt, w.vrows
        if not w.rows4:
            _lib.check(lib.tmf_wsum_pass_f32(w.seg_e.cstruct(), w.ent_row, w.ent_w, w.wbuf, st.U, st.V, V_out, st.slab, r, _lib.EPI_ADAM, adam, s))
            _engine._row_pass_finish(lib, w.seg_e, st.slab, st.V, V_out, r, _lib.EPI_ADAM, adam, s)
        else:
            _lib.check(lib.tmf_wsum_rows5_f32(w.rowptr_e, n, w.user_chunks, w.ent_row, w.ent_w, w.wbuf, st.U, st.V, V_out, st.slab, v.item,
                                              v.part, v.nparts, v.slot, v.n_vrows, r, _lib.EPI_ADAM, adam, st.rows4_per_launch, st.rows4_sync,
                                              st.rows4_sync.numel() * 4, s))
            if v.n_long:
                _engine._row_pass_finish(lib, v, st.slab, st.V, V_out, r, _lib.EPI_ADAM, adam, s)
    res['grad_alone'] = timed(dict(
        item_bias_grad=lambda: _lib.check(this.tmf_item_bias_grad(w.rowptr_e, n, w.user_chunks, w.ent_w, w.wbuf, ib.chunk, ib.xrow, ib.xchunk,
                                                                  ib.xptr, ib.n_extra, ib.b, ib.b_nxt, ib.epi, adam, ib.ws, ib.ws.numel() * 8, s)),
        item_pass_parent=lambda: item_pass(parent), item_pass_this=lambda: item_pass(this)))
    head = (plan.rowptr_u, plan.val_u, st.pk, st.sp, m, S, c)
    tail = (w.delta, w.D, st.loss_part, w.hinge_order, s)
    res['add_alone'] = timed(dict(
        item_bias_add=lambda: _lib.check(this.tmf_item_bias_add(ib.b, n, w.R, m, S, st.sp, plan.col_u, plan.nnz, st.pk, s)),
        softmax_pairs_parent=lambda: _lib.check(parent.tmf_softmax_pairs(*head, *tail))))
    res['add_GB_per_s'] = 1e-6 * res['bytes_add'] / res['add_alone']['item_bias_add']['ms']
    # ---- the epochs: the parent's, this library's without the bias, this library's with it, in turn ----
    ib.epi = _lib.EPI_ADAM
    res['epochs'] = {}
    for name, pairs, cc in (('wmrb', 'hinge', c), ('warp', 'warp', 0.0), ('softmax', 'softmax', c)):
        def epoch(lib, bias):
            use(lib)
            st.ib = ib if bias else None
            _engine.epoch_wmrb(st, adam, cc, loss, pairs=pairs)
            st.swap()
        res['epochs'][name] = timed(dict(parent=lambda: epoch(parent, False), bias_off=lambda: epoch(this, False),
                                         bias_on=lambda: epoch(this, True)), reps=args.epoch_reps, warmup=1)
        use(this)
        prof = _engine.KernelTimer()
        st.ib = ib
        for e in range(2):
            _engine.epoch_wmrb(st, adam, cc, loss, prof=prof, pairs=pairs)
            st.swap()
        torch.cuda.synchronize()
        res['epochs'][name]['kernels_ms'] = {k: prof.mean_ms(k) for k in prof.spans}
        res['epochs'][name]['loss_after'] = float(loss) / plan.n_pos
    st.ib = None
    res['bias_abs_max_after'] = float(ib.value.abs().max())
    # ---- ranking: width 129 against 128 ----
    U, V = st.U[:, :r], st.V[:, :r]
    res['ranking'] = {}
    for arithmetic in ('split', 'fp32'):
        Ua, Va, fused = augmented_tables(U, V, ib.value)
        assert fused
        res['ranking'][arithmetic] = timed(dict(
            width_128=lambda: _ops.predict_topk(U, V, 10, arithmetic=arithmetic),
            width_129=lambda: _ops.predict_topk(Ua, Va, 10, arithmetic=arithmetic),
            augment=lambda: augmented_tables(U, V, ib.value)), reps=3, warmup=1)
        del Ua, Va
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
               k=10, runs={})
    for loss in (WARPLoss, BPRLoss):
        for every in (0, 1):
            for bias in (False, True):
                model = MatrixFactorization(r, loss_graph=loss(), user_weight_graph=FixedInitializer(U0), item_weight_graph=FixedInitializer(V0),
                                            n_users=m, n_items=n, n_samples=S)
                model.verbose, model.random_ind, model.resample_every, model.scalar_item_bias = False, R, every, bias
                model.fit(args.q_epochs, eye(m), eye(n), train, lr=args.q_lr)
                run = dict(recall_at_10=float(model.recall_at_k(test, k=10, exclude=train).mean()),
                           recall_at_10_train=float(model.recall_at_k(train, k=10).mean()),
                           loss_first_last=[model.loss_history_[0], model.loss_history_[-1]], fit_seconds=model.fit_seconds_,
                           rounds=model.resample_rounds_)
                if bias:
                    b = model.item_bias_
                    pop = torch.bincount(train.indices[:, 1], minlength=n).float()
                    run.update(bias_min_max=[float(b.min()), float(b.max())],
                               bias_popularity_correlation=float(torch.corrcoef(torch.stack([b, torch.log1p(pop)]))[0, 1]))
                res['runs'][f'{loss.__name__} {"resample_every_1" if every else "static"} {"bias" if bias else "no_bias"}'] = run
    print(json.dumps(res), flush=True)


def run_child(args, child, limit):
    """One measurement in a fresh process under its own time limit; any failure ends the whole run (nothing more is started)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', child, '--parent-lib', os.path.abspath(args.parent_lib)]
    for k in ('users', 'items', 'r', 'nnz', 'samples', 'warmup', 'reps', 'epoch_reps', 'lr', 'q_users', 'q_items', 'q_r', 'q_nnz',
              'q_samples', 'q_epochs', 'q_lr'):
        cmd += ['--' + k.replace('_', '-'), str(getattr(args, k))]
    print(f'[time_item_bias_c4] {child}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=limit)
    if p.returncode != 0:
        raise SystemExit(f'{child} run failed with exit status {p.returncode}')
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help='libtmf.so built from the parent commit: its kernels and epochs are the yardsticks')
    ap.add_argument('--warmup', type=int, default=2, help='untimed launches of every kernel timed alone')
    ap.add_argument('--reps', type=int, default=9, help='timed launches of every kernel timed alone')
    ap.add_argument('--epoch-reps', type=int, default=7, help='timed epochs of every (loss, library, bias) in turn')
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
    ap.add_argument('--limit', type=int, default=480, help='seconds one child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', choices=['c4', 'quality'], default=None)
    args = ap.parse_args()
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit('--parent-lib: the library of the parent commit holds the yardsticks of this measurement; build it first')
    if args.child:
        return child_c4(args) if args.child == 'c4' else child_quality(args)
    c4 = run_child(args, 'c4', args.limit)
    quality = run_child(args, 'quality', args.limit)
    add, grad = c4['add_alone'], c4['grad_alone']
    alone = add['item_bias_add']['ms'] + grad['item_bias_grad']['ms']
    verdicts = dict(
        add=dict(ms=add['item_bias_add']['ms'], yardstick_ms=add['softmax_pairs_parent']['ms'], bound=ADD_BOUND,
                 ratio=add['item_bias_add']['ms'] / add['softmax_pairs_parent']['ms'],
                 met=bool(add['item_bias_add']['ms'] <= ADD_BOUND * add['softmax_pairs_parent']['ms'])),
        grad=dict(ms=grad['item_bias_grad']['ms'], yardstick_ms=grad['item_pass_parent']['ms'], bound=GRAD_BOUND,
                  ratio=grad['item_bias_grad']['ms'] / grad['item_pass_parent']['ms'],
                  met=bool(grad['item_bias_grad']['ms'] <= GRAD_BOUND * grad['item_pass_parent']['ms'])), epochs={})
    for name, e in c4['epochs'].items():
        band = e['parent']['max'] - e['parent']['min']
        verdicts['epochs'][name] = dict(
            on_minus_parent_ms=e['bias_on']['ms'] - e['parent']['ms'], bound_ms=EPOCH_MARGIN * alone,
            on_met=bool(e['bias_on']['ms'] - e['parent']['ms'] <= EPOCH_MARGIN * alone),
            off_minus_parent_ms=e['bias_off']['ms'] - e['parent']['ms'], parent_band_ms=band,
            off_met=bool(abs(e['bias_off']['ms'] - e['parent']['ms']) <= band))
    rank = {a: dict(ratio=t['width_129']['ms'] / t['width_128']['ms'], augment_ms=t['augment']['ms']) for a, t in c4['ranking'].items()}
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r, S=args.samples), lr=args.lr, reps=args.reps, epoch_reps=args.epoch_reps,
               warmup=args.warmup, verdicts=verdicts, ranking_width_129_over_128=rank, c4=c4, quality=quality)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
