"""Cost of an MSE epoch over hybrid SparseFeatures on the sparse engine at the C4 shape (1M users x 100K items, r = 128, ~1e8
interactions of bench.py's generator): users = [I | 4 tags of 500], items = [I | 8 tags of 2 000], against its yardstick, the MSE
epoch of the PARENT commit's library on the same interactions over identity features - the parent has no feature path, so that
is the cost a user compares with.  The four feature passes gather nnz_F * ld * 4 bytes and write rows * ld * 4 each (DESIGN.md
section 3); the expectation is  added time / parent epoch <= 1.5 x added bytes / bytes of the MSE epoch  (feature rows of ~5
entries are latency-bound, hence the margin).  Recorded, not gated.
A library is chosen when the package is imported, so every measurement is a child process of its own (this process never opens
the GPU); the hybrid run and the parent's MSE run alternate, --rounds times.  Each child warms up, then times --epochs epochs with
device events; the hybrid child also brackets the four feature passes (KernelTimer, a run of its own).  Second record: hybrid
features at the C2 shape (943 x 1682, 1e5 interactions) through the generic path on the dense matrices (what `fit` did for
SparseFeatures-shaped input before) against the engine.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/libtmf_parent.so
    python tools/time_features_c4.py --parent-lib libtmf_parent.so [--out profiles/features_c4.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MARGIN = 1.5
MSE_EPOCH_BYTES = 75e9   # what the MSE epoch moves at C4
SPANS = ('user_feat_backward', 'user_feat_forward', 'item_feat_backward', 'item_feat_forward')


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def timed_epochs(torch, run, epochs, warmup):
    """ms per epoch over `epochs` epochs between two device events, after `warmup` epochs."""
    for e in range(warmup):
        run(e)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for e in range(epochs):
        run(e)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / epochs


def hybrid(torch, rows, per_row, n_tags, seed, dev):
    """[I | per_row random tags of n_tags] as SparseFeatures (values 1)."""
    from teamoflow_amd.mf.sparse import SparseFeatures, hstack_identity
    g = torch.Generator(device=dev).manual_seed(seed)
    idx = torch.stack([torch.arange(rows, device=dev).repeat_interleave(per_row),
                       torch.randint(0, n_tags, (rows * per_row,), device=dev, generator=g)], 1)
    return hstack_identity(rows, SparseFeatures(idx, torch.ones(rows * per_row, device=dev), (rows, n_tags), device=dev))


def child_c4(args):
    import torch

    import bench
    from teamoflow_amd import _engine, _lib
    _lib.get()
    dev = torch.device('cuda', 0)
    idx, val = bench.gen_interactions(args.users, args.items, args.nnz, 'zipf', 1234, dev)
    plan = _engine.InteractionPlan(idx, val, args.users, args.items, user_chunks=_engine.mse_user_chunks(), csc=True)
    del idx, val
    g = torch.Generator(device=dev).manual_seed(5)
    adam = _engine.adam_constants(0.01)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    res = dict(nnz=plan.nnz, device=torch.cuda.get_device_name(0), library=os.path.basename(_lib.LIB_PATH))
    if args.child == 'hybrid':
        Fu, Fv = hybrid(torch, args.users, 4, 500, 7, dev), hybrid(torch, args.items, 8, 2000, 8, dev)
        Wu = torch.randn(Fu.shape[1], args.r, device=dev, generator=g) * 0.1
        Wv = torch.randn(Fv.shape[1], args.r, device=dev, generator=g) * 0.1
        st = _engine.TrainState(Wu, Wv, plan, args.r, user_feat=Fu, item_feat=Fv)
        ld = st.ld
        res.update(nnz_user_features=Fu.nnz, nnz_item_features=Fv.nnz, user_features=list(Fu.shape), item_features=list(Fv.shape),
                   # per pass: nnz_F rows gathered + the rows written (backward: the weights, read and written; forward: E)
                   feature_bytes=4 * ld * sum(2 * F.nnz + 2 * F.shape[1] + F.shape[0] for F in (Fu, Fv)))

        def epoch(e, prof=None):
            _engine.epoch_sides(st, adam, loss, 'mse', prof=prof)
        res['hybrid_epoch_ms'] = timed_epochs(torch, epoch, args.epochs, args.warmup)
        res['loss_after'] = float(loss)
        prof = _engine.KernelTimer()
        for e in range(args.epochs):
            epoch(e, prof)
        torch.cuda.synchronize()
        res['spans_ms'] = {k: prof.mean_ms(k) for k in SPANS + ('mse_user_pass', 'mse_item_pass')}
    else:
        U0 = torch.randn(args.users, args.r, device=dev, generator=g) * 0.1
        V0 = torch.randn(args.items, args.r, device=dev, generator=g) * 0.1
        st = _engine.TrainState(U0, V0, plan, args.r)

        def mse(e):
            _engine.epoch_mse(st, adam, loss)
            st.swap()
        res['mse_epoch_ms'] = timed_epochs(torch, mse, args.epochs, args.warmup)
    print(json.dumps(res), flush=True)


def child_c2(args):
    """Hybrid features at the MovieLens-100K shape through the generic path (dense matrices, autograd) and through the engine."""
    import numpy as np
    import torch

    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions
    rng = np.random.default_rng(0)
    m, n, r, nnz, epochs = 943, 1682, 128, 100_000, 100
    keys = rng.choice(m * n, nnz, replace=False)
    idx = np.stack([keys // n, keys % n], 1)
    val = rng.integers(1, 6, nnz).astype(np.float32)
    dev = torch.device('cuda', 0)
    Fu, Fv = hybrid(torch, m, 4, 50, 7, dev), hybrid(torch, n, 8, 200, 8, dev)
    U0 = (rng.standard_normal((Fu.shape[1], r)) * 0.1).astype(np.float32)
    V0 = (rng.standard_normal((Fv.shape[1], r)) * 0.1).astype(np.float32)
    res = dict(shape=dict(m=m, n=n, r=r), nnz=nnz, epochs=epochs, user_features=list(Fu.shape), item_features=list(Fv.shape))
    for name in ('generic', 'engine', 'generic', 'engine'):          # the second pair is the record: everything is warm
        model = MatrixFactorization(r, user_weight_graph=FixedInitializer(U0), item_weight_graph=FixedInitializer(V0))
        model.verbose = False
        if name == 'generic':
            model._route = lambda user_features, item_features: 'generic'
        model.fit(epochs, Fu, Fv, SparseInteractions(idx, val, (m, n)), lr=0.01)
        torch.cuda.synchronize()
        assert hasattr(model, '_state') == (name == 'engine')
        res[name + '_ms_per_epoch'] = 1e3 * model.fit_seconds_ / epochs
        res[name + '_loss_last'] = model.loss_history_[-1]
    res['speedup'] = res['generic_ms_per_epoch'] / res['engine_ms_per_epoch']
    print(json.dumps(res), flush=True)


def run_child(args, child, env_extra, limit):
    """One measurement in a fresh process under its own time limit; any failure ends the whole run (nothing more is started)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', child, '--users', str(args.users), '--items', str(args.items),
           '--r', str(args.r), '--nnz', str(args.nnz), '--epochs', str(args.epochs), '--warmup', str(args.warmup)]
    env = dict(os.environ, **env_extra)
    print(f'[time_features_c4] {child} {env_extra}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=limit)
    if p.returncode != 0:
        raise SystemExit(f'{child} run failed with exit status {p.returncode}')
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help="libtmf.so built from the parent commit (the yardstick's MSE epoch)")
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--epochs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--r', type=int, default=128)
    ap.add_argument('--nnz', type=int, default=100_000_000)
    ap.add_argument('--limit', type=int, default=420, help='seconds one child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', choices=['hybrid', 'mse', 'c2'], default=None)
    args = ap.parse_args()
    if args.child == 'c2':
        return child_c2(args)
    if args.child:
        return child_c4(args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit('--parent-lib: the library of the parent commit is the yardstick of this measurement; build it first')
    parent_env = dict(TMF_LIB=os.path.abspath(args.parent_lib), TMF_LIB_OLDER='1')
    rounds = []
    for _ in range(args.rounds):
        rounds.append(dict(hybrid=run_child(args, 'hybrid', {}, args.limit), parent=run_child(args, 'mse', parent_env, args.limit)))
    hybrid_ms = median([x['hybrid']['hybrid_epoch_ms'] for x in rounds])
    parent_ms = median([x['parent']['mse_epoch_ms'] for x in rounds])
    spans = {k: median([x['hybrid']['spans_ms'][k] for x in rounds]) for k in rounds[0]['hybrid']['spans_ms']}
    h0 = rounds[0]['hybrid']
    share = h0['feature_bytes'] / MSE_EPOCH_BYTES
    added = (hybrid_ms - parent_ms) / parent_ms
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r), nnz=h0['nnz'], device=h0['device'], epochs=args.epochs,
               warmup=args.warmup, user_features=h0['user_features'], item_features=h0['item_features'],
               nnz_user_features=h0['nnz_user_features'], nnz_item_features=h0['nnz_item_features'], hybrid_epoch_ms=hybrid_ms,
               spans_ms=spans, feature_spans_ms=sum(spans[k] for k in SPANS), mse_epoch_ms_parent=parent_ms,
               feature_bytes=h0['feature_bytes'], mse_epoch_bytes=MSE_EPOCH_BYTES, added_bytes_share=share, added_time_share=added,
               margin=MARGIN, within_expectation=bool(added <= MARGIN * share), rounds=rounds, c2=run_child(args, 'c2', {}, args.limit))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
