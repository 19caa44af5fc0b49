"""Cost of a ReLU user side on the sparse engine at the C4 shape (1M users x 100K items, r = 128, aux = 640, ~1e8 interactions of
bench.py's generator, MSE, indicator features), against yardsticks measured with the PARENT commit's library on the same machine:

 (a) each new GEMM against tmf_predict_gemm_f32 (parent) at the same (m, n, K):
        tmf_relu_embed_f32     (1M, 128, 640)   bound 1.15 x
        tmf_relu_dhidden_f32   (1M, 640, 128)   bound 1.15 x
        tmf_relu_dweights_f32 + tmf_relu_adam_weights_f32   (640, 128, 1M)   bound 1.30 x (it also writes and re-reads the partials)
 (b) the epoch against the sum of parent-measured parts, plus 10 %:
        the parent's MSE epoch on the same plan + those three GEMM times + the two tmf_feat_pass_f32 launches at width 640 over the
        identity lists, timed alone + the parent's tmf_adam_bias_rows_f32 on a [1M, 640] table once per sweep over a [1M, ld(aux)]
        table that none of those parts contains (DESIGN.md counts them: the mask read of Z in dhidden and the column sums of dZ).

A library is chosen when the package is imported, so every measurement is a child process of its own (this process never opens the
GPU).  Second record, no bound: a ReLU fit at the C2 shape (943 x 1682, 1e5 interactions), engine against the generic path.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/libtmf_parent.so
    python tools/time_relu_c4.py --parent-lib libtmf_parent.so [--out profiles/relu_c4.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GEMM_BOUNDS = dict(embed=1.15, dhidden=1.15, dweights=1.30)
EPOCH_MARGIN = 1.10
SWEEPS_OUTSIDE_PARTS = 2   # DESIGN.md, "ReLU sides": dhidden's read of Z for the mask, the column sums of dZ
SPANS = ('relu_dweights', 'relu_dhidden', 'relu_adam_weights', 'relu_bias_colsum', 'relu_bias_adam', 'relu_feat_backward',
         'relu_feat_forward', 'relu_embed')


def timed(torch, run, reps, warmup=2):
    """ms per call of run() between two device events."""
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def c4_plan(args, dev):
    import torch

    import bench
    from teamoflow_amd import _engine
    idx, val = bench.gen_interactions(args.users, args.items, args.nnz, 'zipf', 1234, dev)
    plan = _engine.InteractionPlan(idx, val, args.users, args.items, user_chunks=_engine.mse_user_chunks(), csc=True)
    g = torch.Generator(device=dev).manual_seed(5)
    V0 = torch.randn(args.items, args.r, device=dev, generator=g) * 0.1
    return plan, V0, g


def child_relu(args):
    """This library: the epoch with a ReLU user side, its spans, and the MSE epoch of a plain fit on the same plan."""
    import torch

    from teamoflow_amd import _engine, _lib
    _lib.get()
    dev = torch.device('cuda', 0)
    plan, V0, g = c4_plan(args, dev)
    aux = 5 * args.r
    adam, loss = _engine.adam_constants(0.01), torch.zeros(1, dtype=torch.float64, device=dev)
    W0 = torch.randn(aux, args.r, device=dev, generator=g) * 0.1
    st = _engine.TrainState(W0, V0, plan, args.r, user_relu=dict(F=None, Wr0=torch.randn(args.users, aux, device=dev, generator=g),
                                                                 b0=torch.zeros(aux, device=dev)))
    res = dict(nnz=plan.nnz, device=torch.cuda.get_device_name(0), library=os.path.basename(_lib.LIB_PATH),
               part_rows=st.relu_u.part_rows, ld_aux=st.relu_u.ld_aux)
    res['relu_epoch_ms'] = timed(torch, lambda: _engine.epoch_sides(st, adam, loss, 'mse'), args.epochs, args.warmup)
    res['relu_loss_after'] = float(loss)
    prof = _engine.KernelTimer()
    for _ in range(args.epochs):
        _engine.epoch_sides(st, adam, loss, 'mse', prof=prof)
    torch.cuda.synchronize()
    res['spans_ms'] = {k: prof.mean_ms(k) for k in ('mse_user_pass', 'mse_item_pass') + tuple('user_' + x for x in SPANS)}
    res['units_on'] = float(((st.relu_u.Z[:4096, :aux] + st.relu_u.b[:aux]) > 0).float().mean())
    del st
    torch.cuda.empty_cache()
    plain = _engine.TrainState(torch.randn(args.users, args.r, device=dev, generator=g) * 0.1, V0, plan, args.r)

    def mse():
        _engine.epoch_mse(plain, adam, loss)
        plain.swap()
    res['mse_epoch_ms'] = timed(torch, mse, args.epochs, args.warmup)
    print(json.dumps(res), flush=True)


def child_parent(args):
    """The parent's library: its MSE epoch on the same plan, tmf_predict_gemm_f32 at the three GEMM shapes, the two list passes at the
    hidden width over the identity lists, and tmf_adam_bias_rows_f32 on a [users, aux] table."""
    import torch

    from teamoflow_amd import _engine, _lib
    lib, P, s = _lib.get(), _lib.ptr, _lib.stream_ptr()
    dev = torch.device('cuda', 0)
    plan, V0, g = c4_plan(args, dev)
    m, r, aux = args.users, args.r, 5 * args.r
    ld_aux = _lib.padded_ld(aux)
    adam, loss = _engine.adam_constants(0.01), torch.zeros(1, dtype=torch.float64, device=dev)
    res = dict(nnz=plan.nnz, device=torch.cuda.get_device_name(0), library=os.path.basename(_lib.LIB_PATH))
    plain = _engine.TrainState(torch.randn(m, r, device=dev, generator=g) * 0.1, V0, plan, r)

    def mse():
        _engine.epoch_mse(plain, adam, loss)
        plain.swap()
    res['mse_epoch_ms'] = timed(torch, mse, args.epochs, args.warmup)
    del plain, plan
    torch.cuda.empty_cache()
    f32 = dict(dtype=torch.float32, device=dev)
    Z = torch.randn(m, ld_aux, generator=g, **f32)
    dZ, G, E = torch.empty(m, ld_aux, **f32), torch.randn(m, r, generator=g, **f32), torch.empty(m, r, **f32)
    W = torch.randn(aux, r, generator=g, **f32)
    Wt = W.t().contiguous()                                   # [r, aux]: both operands K-contiguous
    gemm = lib.tmf_predict_gemm_f32
    shapes = dict(embed=lambda: gemm(P(Z), P(Wt), P(E), m, r, aux, ld_aux, aux, r, s),
                  dhidden=lambda: gemm(P(G), P(W), P(dZ), m, aux, r, r, r, ld_aux, s))
    res['gemm_ms'] = {k: timed(torch, lambda f=f: _lib.check(f()), args.epochs, 2) for k, f in shapes.items()}
    Ht, Gt, C = torch.randn(aux, m, generator=g, **f32), G.t().contiguous(), torch.empty(aux, r, **f32)
    res['gemm_ms']['dweights'] = timed(torch, lambda: _lib.check(gemm(P(Ht), P(Gt), P(C), aux, r, m, m, m, r, s)), 3, 1)
    del Ht, Gt
    torch.cuda.empty_cache()
    # the list passes of the hidden layer over indicator features: one entry per row
    own = torch.arange(m, dtype=torch.int64, device=dev)
    ident = _engine.InteractionPlan(torch.stack([own, own], 1), torch.ones(m, **f32), m, m, csc=True)
    slab = torch.empty(max(ident.seg_u.n_slab, ident.seg_i.n_slab, 1), ld_aux, **f32)
    Wr, Wr_nxt = torch.randn(m, ld_aux, generator=g, **f32), torch.empty(m, ld_aux, **f32)

    def backward():
        _lib.check(lib.tmf_feat_pass_f32(ident.seg_i.cstruct(), P(ident.row_i), P(ident.val_i), P(Z), P(Wr), P(Wr_nxt), P(slab), aux,
                                         _lib.EPI_ADAM, adam, s), lib)
    res['feat_backward_ms'] = timed(torch, backward, args.epochs, 2)
    res['feat_forward_ms'] = timed(torch, lambda: _engine.feature_forward(ident, Wr, dZ, slab, aux), args.epochs, 2)
    b = torch.zeros(ld_aux, **f32)
    res['adam_bias_rows_ms'] = timed(torch, lambda: _lib.check(lib.tmf_adam_bias_rows_f32(P(Wr), P(Z), P(b), P(dZ), m, aux, adam, s)),
                                     args.epochs, 2)
    print(json.dumps(res), flush=True)


def child_c2(args):
    """A ReLU user side at the MovieLens-100K shape through the generic path (relu_engine off: what the parent does) and the engine."""
    import numpy as np
    import torch

    from teamoflow_amd.mf.embedding_graphs import ReLUEmbedding
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    rng = np.random.default_rng(0)
    m, n, r, nnz, epochs = 943, 1682, 128, 100_000, 50
    keys = rng.choice(m * n, nnz, replace=False)
    idx = np.stack([keys // n, keys % n], 1)
    val = rng.integers(1, 6, nnz).astype(np.float32)
    res = dict(shape=dict(m=m, n=n, r=r, aux=5 * r), nnz=nnz, epochs=epochs)
    for name in ('generic', 'engine', 'generic', 'engine'):          # the second pair is the record: everything is warm
        torch.manual_seed(0)
        model = MatrixFactorization(r, user_repr_graph=ReLUEmbedding())
        model.verbose, model.relu_engine = False, name == 'engine'
        model.fit(epochs, eye(m), eye(n), SparseInteractions(idx, val, (m, n)), lr=0.01)
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
    print(f'[time_relu_c4] {child} {env_extra}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=dict(os.environ, **env_extra), stdout=subprocess.PIPE, timeout=limit)
    if p.returncode != 0:
        raise SystemExit(f'{child} run failed with exit status {p.returncode}')
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help='libtmf.so built from the parent commit (the yardsticks)')
    ap.add_argument('--epochs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--r', type=int, default=128)
    ap.add_argument('--nnz', type=int, default=100_000_000)
    ap.add_argument('--limit', type=int, default=300, help='seconds one child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', choices=['relu', 'parent', 'c2'], default=None)
    args = ap.parse_args()
    if args.child:
        return dict(relu=child_relu, parent=child_parent, c2=child_c2)[args.child](args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit('--parent-lib: the library of the parent commit is the yardstick of this measurement; build it first')
    ours = run_child(args, 'relu', {}, args.limit)
    parent = run_child(args, 'parent', dict(TMF_LIB=os.path.abspath(args.parent_lib), TMF_LIB_OLDER='1'), args.limit)
    sp = ours['spans_ms']
    mine = dict(embed=sp['user_relu_embed'], dhidden=sp['user_relu_dhidden'], dweights=sp['user_relu_dweights'] + sp['user_relu_adam_weights'])
    gemms = {k: dict(ms=mine[k], parent_gemm_ms=parent['gemm_ms'][k], ratio=mine[k] / parent['gemm_ms'][k], bound=GEMM_BOUNDS[k],
                     within_bound=bool(mine[k] <= GEMM_BOUNDS[k] * parent['gemm_ms'][k])) for k in mine}
    parts = dict(mse_epoch_parent=parent['mse_epoch_ms'], gemms=sum(parent['gemm_ms'].values()),
                 feat_passes=parent['feat_backward_ms'] + parent['feat_forward_ms'],
                 sweeps=SWEEPS_OUTSIDE_PARTS * parent['adam_bias_rows_ms'])
    bound_ms = EPOCH_MARGIN * sum(parts.values())
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r, aux=5 * args.r, ld_aux=ours['ld_aux']), nnz=ours['nnz'], device=ours['device'],
               epochs=args.epochs, warmup=args.warmup, relu_epoch_ms=ours['relu_epoch_ms'], spans_ms=sp, gemms=gemms,
               epoch_parts_ms=parts, sweeps_outside_parts=SWEEPS_OUTSIDE_PARTS, epoch_margin=EPOCH_MARGIN, epoch_bound_ms=bound_ms,
               epoch_within_bound=bool(ours['relu_epoch_ms'] <= bound_ms), mse_epoch_ms_this_library=ours['mse_epoch_ms'],
               mse_epoch_ms_parent=parent['mse_epoch_ms'], this_library=ours, parent=parent, c2=run_child(args, 'c2', {}, args.limit))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
