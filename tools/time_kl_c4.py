"""Cost of a KLDivergenceLoss epoch on the sparse engine at the C4 shape (1M users x 100K items, r = 128, ~1e8 interactions of
bench.py's generator with a random sign on every value), against its yardstick: the MSE epoch of the PARENT commit's library on the
same plan.  KL is the two MSE-shaped passes plus one pass that is the user pass without its table write, so the bound is
    KL epoch <= 1.5 x MSE epoch (parent) x 1.10.
A library is chosen when the package is imported, so every measurement is a child process of its own (this process never opens
the GPU); the KL run and the parent's MSE run alternate, --rounds times.  Each child warms up, then times --epochs epochs with
device events; the KL child also brackets the three passes and the coefficient kernel (KernelTimer, a run of its own) and times the
MSE epoch of the current library.  Second record, no bound: KL at the C2 shape (943 x 1682, 1e5 interactions) through the generic
autograd path against the engine - what a user saw before and sees now.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/libtmf_parent.so
    python tools/time_kl_c4.py --parent-lib libtmf_parent.so [--out profiles/kl_c4.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BOUND = 1.5 * 1.10


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def c4_problem(args, dev):
    import torch

    import bench
    idx, val = bench.gen_interactions(args.users, args.items, args.nnz, 'zipf', 1234, dev)
    g = torch.Generator(device=dev).manual_seed(5)
    val = val * (torch.randint(0, 2, val.shape, device=dev, generator=g) * 2 - 1).to(val.dtype)
    U0 = torch.randn(args.users, args.r, device=dev, generator=g) * 0.1
    V0 = torch.randn(args.items, args.r, device=dev, generator=g) * 0.1
    return idx, val, U0, V0


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


def child_c4(args):
    import torch

    from teamoflow_amd import _engine, _lib
    _lib.get()
    dev = torch.device('cuda', 0)
    idx, val, U0, V0 = c4_problem(args, dev)
    plan = _engine.InteractionPlan(idx, val, args.users, args.items, user_chunks=_engine.mse_user_chunks(), csc=True)
    del idx, val
    kl = args.child == 'kl'
    st = _engine.TrainState(U0, V0, plan, args.r, **(dict(kl=True) if kl else {}))
    adam = _engine.adam_constants(0.01)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    res = dict(nnz=plan.nnz, n_pos=plan.n_pos, segments_user=plan.seg_u.nseg, segments_item=plan.seg_i.nseg,
               device=torch.cuda.get_device_name(0), library=os.path.basename(_lib.LIB_PATH))

    def mse(e, prof=None):
        _engine.epoch_mse(st, adam, loss, prof=prof)
        st.swap()
    if kl:
        def kl_epoch(e, prof=None):
            _engine.epoch_kl(st, adam, loss, prof=prof)
            st.swap()
        res['kl_epoch_ms'] = timed_epochs(torch, kl_epoch, args.epochs, args.warmup)
        res['kl_loss_after'] = float(loss)
        prof = _engine.KernelTimer()
        for e in range(args.epochs):
            kl_epoch(e, prof)
        torch.cuda.synchronize()
        res['kl_passes_ms'] = {k: prof.mean_ms(k) for k in ('kl_moments', 'kl_coeffs', 'kl_user_pass', 'kl_item_pass')}
    res['mse_epoch_ms'] = timed_epochs(torch, mse, args.epochs, args.warmup)
    prof = _engine.KernelTimer()
    for e in range(args.epochs):
        mse(e, prof)
    torch.cuda.synchronize()
    res['mse_passes_ms'] = {k: prof.mean_ms(k) for k in ('mse_user_pass', 'mse_item_pass')}
    print(json.dumps(res), flush=True)


def child_c2(args):
    """KL at the MovieLens-100K shape through the generic path (what `fit` did for this model before) and through the engine."""
    import numpy as np
    import torch

    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import KLDivergenceLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    rng = np.random.default_rng(0)
    m, n, r, nnz, epochs = 943, 1682, 128, 100_000, 100
    keys = rng.choice(m * n, nnz, replace=False)
    idx = np.stack([keys // n, keys % n], 1)
    val = (rng.integers(1, 6, nnz) * rng.choice([-1, 1], nnz)).astype(np.float32)
    U0 = (rng.standard_normal((m, r)) * 0.1).astype(np.float32)
    V0 = (rng.standard_normal((n, r)) * 0.1).astype(np.float32)
    res = dict(shape=dict(m=m, n=n, r=r), nnz=nnz, epochs=epochs)
    for name in ('generic', 'engine', 'generic', 'engine'):          # the second pair is the record: everything is warm
        model = MatrixFactorization(r, loss_graph=KLDivergenceLoss(), user_weight_graph=FixedInitializer(U0),
                                    item_weight_graph=FixedInitializer(V0))
        model.verbose = False
        if name == 'generic':
            model._route = lambda user_features, item_features: 'generic'
        model.fit(epochs, eye(m), eye(n), SparseInteractions(idx, val, (m, n)), lr=0.01)
        torch.cuda.synchronize()
        res[name + '_ms_per_epoch'] = 1e3 * model.fit_seconds_ / epochs
        res[name + '_loss_last'] = model.loss_history_[-1]
    res['speedup'] = res['generic_ms_per_epoch'] / res['engine_ms_per_epoch']
    print(json.dumps(res), flush=True)


def run_child(args, child, env_extra, limit):
    """One measurement in a fresh process under its own time limit; any failure ends the whole run (nothing more is started)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', child, '--users', str(args.users), '--items', str(args.items),
           '--r', str(args.r), '--nnz', str(args.nnz), '--epochs', str(args.epochs), '--warmup', str(args.warmup)]
    env = dict(os.environ, **env_extra)
    print(f'[time_kl_c4] {child} {env_extra}', file=sys.stderr, flush=True)
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
    ap.add_argument('--child', choices=['kl', 'mse', 'c2'], default=None)
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
        rounds.append(dict(kl=run_child(args, 'kl', {}, args.limit), parent=run_child(args, 'mse', parent_env, args.limit)))
    kl_ms = median([x['kl']['kl_epoch_ms'] for x in rounds])
    parent_ms = median([x['parent']['mse_epoch_ms'] for x in rounds])
    passes = {k: median([x['kl']['kl_passes_ms'][k] for x in rounds]) for k in rounds[0]['kl']['kl_passes_ms']}
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r), nnz=rounds[0]['kl']['nnz'], n_pos=rounds[0]['kl']['n_pos'],
               device=rounds[0]['kl']['device'], epochs=args.epochs, warmup=args.warmup, kl_epoch_ms=kl_ms, kl_passes_ms=passes,
               mse_epoch_ms_this_library=median([x['kl']['mse_epoch_ms'] for x in rounds]), mse_epoch_ms_parent=parent_ms,
               ratio=kl_ms / parent_ms, bound=BOUND, within_bound=bool(kl_ms <= BOUND * parent_ms), rounds=rounds,
               c2=run_child(args, 'c2', {}, args.limit))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
