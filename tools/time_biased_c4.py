"""Cost of a BiasedLinearEmbedding epoch on the sparse engine at the C4 shape (1M users x 100K items, r = 128, ~1e8 interactions
of bench.py's generator), both sides biased, against its yardstick: the MSE epoch of the PARENT commit's library on the same plan
with LinearEmbedding.  A biased side adds five sweeps of its table to that epoch (the column sum reads G; the row update reads W
and G and writes W and E; the TMF_EPI_GRAD write replaces the fused table write), B = 5 x (user table + item table) bytes, so
    biased MSE epoch <= parent MSE epoch + 1.5 x B / 6.29 TB/s
(6.29 TB/s: the measured float4-copy rate of the card; 1.5: the row update is a two-read, two-write stream and six short
launches are added).
A library is chosen when the package is imported, so every measurement is a child process of its own (this process never opens
the GPU); the biased run and the parent's MSE run alternate, --rounds times.  Each child warms up, then times --epochs epochs with
device events; the biased child also brackets the three new kernels of each side (KernelTimer, a run of its own) and times the
unbiased MSE epoch of the current library.  Records without a bound: the WMRB epoch at C4, biased against unbiased (--wmrb), and
a biased WMRB model at the MovieLens-1M shape through the generic autograd path against the engine - what a user saw before and
sees now.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/libtmf_parent.so
    python tools/time_biased_c4.py --parent-lib libtmf_parent.so [--wmrb] [--out profiles/biased_c4.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.29e12   # bytes / s
MARGIN = 1.5
BIAS_SPANS = ('bias_colsum', 'bias_adam', 'adam_bias_rows')


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


def c4_problem(args, dev):
    import torch

    import bench
    idx, val = bench.gen_interactions(args.users, args.items, args.nnz, 'zipf', 1234, dev)
    g = torch.Generator(device=dev).manual_seed(5)
    U0 = torch.randn(args.users, args.r, device=dev, generator=g) * 0.1
    V0 = torch.randn(args.items, args.r, device=dev, generator=g) * 0.1
    return idx, val, U0, V0


def spans(prof, st):
    """ms and bytes/s of the three bias kernels of each side: the column sum reads the table once, the row update sweeps it four times."""
    out = {}
    for tag, E in (('user_', st.U), ('item_', st.V)):
        table = E.numel() * 4
        for name, sweeps in zip(BIAS_SPANS, (1, 0, 4)):
            ms = prof.mean_ms(tag + name)
            out[tag + name] = dict(ms=ms, bytes=sweeps * table, bytes_per_s=sweeps * table / (ms * 1e-3) if sweeps else None)
    return out


def child_mse(args):
    """'mse': the unbiased MSE epoch (the parent's library, TMF_LIB); 'biased': the biased epoch, its kernels, and the unbiased
    epoch of the current library."""
    import torch

    from teamoflow_amd import _engine, _lib
    _lib.get()
    dev = torch.device('cuda', 0)
    idx, val, U0, V0 = c4_problem(args, dev)
    plan = _engine.InteractionPlan(idx, val, args.users, args.items, user_chunks=_engine.mse_user_chunks(), csc=True)
    del idx, val
    adam = _engine.adam_constants(0.01)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    res = dict(nnz=plan.nnz, device=torch.cuda.get_device_name(0), library=os.path.basename(_lib.LIB_PATH))
    if args.child == 'biased':
        zero = torch.zeros(args.r)
        sb = _engine.TrainState(U0, V0, plan, args.r, user_bias=zero, item_bias=zero)
        res['biased_epoch_ms'] = timed_epochs(torch, lambda e: _engine.epoch_sides(sb, adam, loss, 'mse'), args.epochs, args.warmup)
        res['biased_loss_after'] = float(loss)
        prof = _engine.KernelTimer()
        for e in range(args.epochs):
            _engine.epoch_sides(sb, adam, loss, 'mse', prof=prof)
        torch.cuda.synchronize()
        res['bias_kernels'] = spans(prof, sb)
        res['biased_passes_ms'] = {k: prof.mean_ms(k) for k in ('mse_user_pass', 'mse_item_pass')}
        res['table_bytes'] = dict(user=sb.U.numel() * 4, item=sb.V.numel() * 4)
        del sb
    st = _engine.TrainState(U0, V0, plan, args.r)

    def mse(e, prof=None):
        _engine.epoch_mse(st, adam, loss, prof=prof)
        st.swap()
    res['mse_epoch_ms'] = timed_epochs(torch, mse, args.epochs, args.warmup)
    prof = _engine.KernelTimer()
    for e in range(args.epochs):
        mse(e, prof)
    torch.cuda.synchronize()
    res['mse_passes_ms'] = {k: prof.mean_ms(k) for k in ('mse_user_pass', 'mse_item_pass')}
    print(json.dumps(res), flush=True)


def child_wmrb(args):
    """The WMRB epoch at C4 (bench.py's negative table, S = 1024), unbiased and with both sides biased, on one plan."""
    import torch

    from teamoflow_amd import _engine, _lib
    from teamoflow_amd.mf.utils import random_sampler_device
    _lib.get()
    dev = torch.device('cuda', 0)
    idx, val, U0, V0 = c4_problem(args, dev)
    plan = _engine.InteractionPlan(idx, val, args.users, args.items, user_chunks=1, csc=False)
    del idx, val
    R = random_sampler_device(args.items, args.users, args.samples, seed=100, device=dev)
    wplan = _engine.wmrb_plan_for(plan, R, args.r)
    adam, c = _engine.adam_constants(0.1), args.items / args.samples
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    res = dict(nnz=plan.nnz, n_pos=plan.n_pos, samples=args.samples)
    st = _engine.TrainState(U0, V0, plan, args.r, wplan)

    def plain(e):
        _engine.epoch_wmrb(st, adam, c, loss)
        st.swap()
    res['wmrb_epoch_ms'] = timed_epochs(torch, plain, args.wmrb_epochs, 2)
    del st
    zero = torch.zeros(args.r)
    sb = _engine.TrainState(U0, V0, plan, args.r, wplan, user_bias=zero, item_bias=zero)
    res['wmrb_biased_epoch_ms'] = timed_epochs(torch, lambda e: _engine.epoch_sides(sb, adam, loss, 'wmrb', c), args.wmrb_epochs, 2)
    res['ratio'] = res['wmrb_biased_epoch_ms'] / res['wmrb_epoch_ms']
    print(json.dumps(res), flush=True)


def child_ml1m(args):
    """A biased WMRB model at the MovieLens-1M shape (6040 x 3706, 1e6 interactions, 5 components, n_items // 5 negatives, lr 0.1):
    the third model of examples/movielens_shape.py --biased, through the generic path (what `fit` did for this model before) and
    through the engine."""
    import numpy as np
    import torch

    from teamoflow_amd.mf.embedding_graphs import BiasedLinearEmbedding
    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import WMRBLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    rng = np.random.default_rng(0)
    m, n, r, nnz, epochs = 6040, 3706, 5, 1_000_000, 20
    S = n // 5
    keys = rng.choice(m * n, nnz, replace=False)
    idx = np.stack([keys // n, keys % n], 1)
    val = rng.integers(1, 6, nnz).astype(np.float32)
    U0 = (rng.standard_normal((m, r)) * 0.1).astype(np.float32)
    V0 = (rng.standard_normal((n, r)) * 0.1).astype(np.float32)
    R = torch.as_tensor(np.stack([rng.choice(n, S, replace=False) for _ in range(m)]))
    res = dict(shape=dict(m=m, n=n, r=r), nnz=nnz, epochs=epochs, loss='wmrb', samples=S)
    for name in ('generic', 'engine', 'generic', 'engine'):          # the second pair is the record: everything is warm
        model = MatrixFactorization(r, loss_graph=WMRBLoss(), user_repr_graph=BiasedLinearEmbedding(),
                                    item_repr_graph=BiasedLinearEmbedding(), n_users=m, n_items=n, n_samples=S,
                                    user_weight_graph=FixedInitializer(U0), item_weight_graph=FixedInitializer(V0))
        model.verbose, model.random_ind = False, R
        if name == 'generic':
            model._route = lambda user_features, item_features: 'generic'
        model.fit(epochs, eye(m), eye(n), SparseInteractions(idx, val, (m, n)), lr=0.1)
        torch.cuda.synchronize()
        res[name + '_ms_per_epoch'] = 1e3 * model.fit_seconds_ / epochs
        res[name + '_loss_last'] = model.loss_history_[-1]
    res['speedup'] = res['generic_ms_per_epoch'] / res['engine_ms_per_epoch']
    print(json.dumps(res), flush=True)


def run_child(args, child, env_extra, limit):
    """One measurement in a fresh process under its own time limit; any failure ends the whole run (nothing more is started)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', child, '--users', str(args.users), '--items', str(args.items),
           '--r', str(args.r), '--nnz', str(args.nnz), '--epochs', str(args.epochs), '--warmup', str(args.warmup),
           '--samples', str(args.samples), '--wmrb-epochs', str(args.wmrb_epochs)]
    env = dict(os.environ, **env_extra)
    print(f'[time_biased_c4] {child} {env_extra}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=limit)
    if p.returncode != 0:
        raise SystemExit(f'{child} run failed with exit status {p.returncode}')
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help="libtmf.so built from the parent commit (the yardstick's MSE epoch)")
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--epochs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--r', type=int, default=128)
    ap.add_argument('--nnz', type=int, default=100_000_000)
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--wmrb', action='store_true', help='also time the WMRB epoch at this shape, biased against unbiased')
    ap.add_argument('--wmrb-epochs', type=int, default=5)
    ap.add_argument('--limit', type=int, default=420, help='seconds one child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', choices=['biased', 'mse', 'wmrb', 'ml1m'], default=None)
    args = ap.parse_args()
    if args.child in ('biased', 'mse'):
        return child_mse(args)
    if args.child == 'wmrb':
        return child_wmrb(args)
    if args.child == 'ml1m':
        return child_ml1m(args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit('--parent-lib: the library of the parent commit is the yardstick of this measurement; build it first')
    parent_env = dict(TMF_LIB=os.path.abspath(args.parent_lib), TMF_LIB_OLDER='1')
    rounds = []
    for _ in range(args.rounds):
        rounds.append(dict(biased=run_child(args, 'biased', {}, args.limit), parent=run_child(args, 'mse', parent_env, args.limit)))
    biased_ms = median([x['biased']['biased_epoch_ms'] for x in rounds])
    parent_ms = median([x['parent']['mse_epoch_ms'] for x in rounds])
    tables = rounds[0]['biased']['table_bytes']
    extra_bytes = 5 * (tables['user'] + tables['item'])
    bound_ms = parent_ms + MARGIN * extra_bytes / COPY_RATE * 1e3
    kernels = {k: dict(ms=median([x['biased']['bias_kernels'][k]['ms'] for x in rounds]), bytes=v['bytes'])
               for k, v in rounds[0]['biased']['bias_kernels'].items()}
    for v in kernels.values():
        v['bytes_per_s'] = v['bytes'] / (v['ms'] * 1e-3) if v['bytes'] else None
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r), nnz=rounds[0]['biased']['nnz'], device=rounds[0]['biased']['device'],
               epochs=args.epochs, warmup=args.warmup, biased_epoch_ms=biased_ms, mse_epoch_ms_parent=parent_ms,
               mse_epoch_ms_this_library=median([x['biased']['mse_epoch_ms'] for x in rounds]), extra_bytes=extra_bytes,
               extra_ms=biased_ms - parent_ms, bound_ms=bound_ms, within_bound=bool(biased_ms <= bound_ms), bias_kernels=kernels,
               rounds=rounds, ml1m=run_child(args, 'ml1m', {}, args.limit))
    if args.wmrb:
        res['wmrb_c4'] = run_child(args, 'wmrb', {}, args.limit)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
