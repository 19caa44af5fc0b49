"""Cost of a BPRLoss epoch on the sparse engine at the C4 shape (1M users x 100K items, r = 128, S = 1024, ~1e8 positives of bench.py's
generator and negative table), beside the WMRB epoch of the PARENT commit's library on the same plan and tables.  The two epochs differ
in one kernel: tmf_bpr_pairs stands where tmf_wmrb_hinge2_ordered stands, and evaluates every (positive, negative) pair - P x S of
them - where the hinge kernel sorts and scans.  The bound is on that kernel alone:

    bpr_pairs <= iterations x (CYCLES x plain + TRANS_CYCLES x transcendental instructions of one loop iteration)
                 / (SIMDs x clock) x 1.10

An iteration is one positive against one tile of 512 samples (8 per lane): iterations = sum over users of positives x ceil(S / 512).
The instructions are counted in the full-tile pair loop of k_bpr_pairs in the assembly hipcc emits for gfx950 (--count-only prints
them and needs no GPU; --counts FILE reads them back).  A SIMD issues a wave64 instruction of several resident waves every 2 cycles
and a transcendental one (v_exp_f32, v_rcp_f32, v_log_f32: quarter rate) every 8; 4 SIMDs per CU, the clock as the device reports it;
10 % for the launch ramp and the tail of the heaviest users.  The gather kernels around it are the parent's code on weights that are
never zero (the zero-weight compaction has nothing to remove): their times are reported beside the parent's, without a bound.
A library is chosen when the package is imported, so every measurement is a child process of its own under its own time limit (this
process never opens the GPU), and nothing further is started after one fails.  Second record, no bound: the C2 shape (943 x 1682,
1e5 interactions, S = 841) through the generic autograd path against the engine.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/libtmf_parent.so
    python tools/time_bpr_c4.py --parent-lib libtmf_parent.so [--out profiles/bpr_c4.json]
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
MARGIN = 1.10
CYCLES, TRANS_CYCLES = 2, 8        # SIMD cycles per wave64 instruction with several waves resident: plain / quarter-rate transcendental
TRANSCENDENTAL = ('v_exp_', 'v_log_', 'v_rcp_', 'v_rsq_', 'v_sqrt_', 'v_sin_', 'v_cos_')
TILE, PAIRS_PER_LANE = 512, 8      # csrc/tmf_bpr.hip: BTILE, BSPL
SPANS = ('wmrb_scores', 'bpr_pairs', 'wmrb_hinge', 'wmrb_gradu', 'wmrb_finish', 'wmrb_user_pass', 'wmrb_item_pass', 'wmrb_combine')


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def pair_loop_counts():
    """(instructions, transcendental ones) of one iteration of the full-tile pair loop of k_bpr_pairs: the shortest backward-branch
    loop that holds a tile's PAIRS_PER_LANE exponentials."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'tmf_bpr.s')
        subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-ffp-contract=on', '-S', '--cuda-device-only',
                        os.path.join(ROOT, 'teamoflow_amd', 'csrc', 'tmf_bpr.hip'), '-o', out], check=True, stderr=subprocess.DEVNULL)
        lines = open(out).read().split('\n')
    start = next(i for i, x in enumerate(lines) if re.match(r'^_ZN3tmf11k_bpr_pairs\w+:', x))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
    body = lines[start:end]
    labels = {m.group(1): i for i, x in enumerate(body) for m in [re.match(r'^(\.LBB\d+_\d+):', x)] if m}
    loops = []
    for i, x in enumerate(body):
        m = re.search(r'\bs_c?branch\w*\s+(?:\S+,\s*)?(\.LBB\d+_\d+)', x)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            seg = body[labels[m.group(1)]:i + 1]
            if sum('v_exp_f32' in s for s in seg) == PAIRS_PER_LANE:
                loops.append(seg)
    loop = min(loops, key=len)
    ops = [s.split()[0] for s in loop if s.strip() and not s.strip().startswith((';', '.')) and not s.rstrip().endswith(':')]
    trans = sum(op.startswith(TRANSCENDENTAL) for op in ops)
    return dict(instructions=len(ops), transcendental=trans, packed=sum(op.startswith('v_pk_') for op in ops),
                pairs_per_lane=PAIRS_PER_LANE)


def bound_ms(counts, iterations, simds, clock_khz):
    cycles = iterations * (CYCLES * (counts['instructions'] - counts['transcendental']) + TRANS_CYCLES * counts['transcendental'])
    return MARGIN * cycles / (simds * clock_khz)      # cycles / (SIMDs x kHz) = ms


# ------------------------------------------------------------------------------------------------------------------------
# the measurements (child processes)
# ------------------------------------------------------------------------------------------------------------------------
def child_c4(args):
    import torch

    import bench
    from teamoflow_amd import _engine, _lib
    from teamoflow_amd.mf.utils import random_sampler_device
    from time_logistic_c4 import device_clock_khz, timed_epochs
    lib = _lib.get()
    dev = torch.device('cuda', 0)
    m, n, r, S = args.users, args.items, args.r, args.samples
    idx, val = bench.gen_interactions(m, n, args.nnz, 'zipf', 0, dev)
    U0, V0 = bench.init_table(m, r, 11, dev), bench.init_table(n, r, 7, dev)
    plan = _engine.InteractionPlan(idx, val, m, n, user_chunks=1, csc=False)
    del idx, val
    R = random_sampler_device(n, m, S, seed=100, device=dev)
    # the same plan for both: at C4 the catalog is sliced whatever the loss (force_sliced changes nothing there)
    wplan = _engine.wmrb_plan_for(plan, R, r)
    assert wplan.sliced, 'this shape would take the one-kernel user pass under WMRB: not the same plan'
    st = _engine.TrainState(U0, V0, plan, r, wplan)
    adam = _engine.adam_constants(0.01)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    props = torch.cuda.get_device_properties(0)
    deg_pos = torch.zeros(m, dtype=torch.int64, device=dev).index_add_(0, plan.user_ids, (plan.val_u > 0).to(torch.int64))
    res = dict(nnz=plan.nnz, n_pos=plan.n_pos, S=S, n_slices=wplan.n_slices, pairs=int(plan.n_pos) * S,
               iterations=int(deg_pos.sum()) * (-(-S // TILE)), max_positives_of_a_user=int(deg_pos.max()),
               device=torch.cuda.get_device_name(0), compute_units=props.multi_processor_count,
               clock_khz=args.clock_khz or device_clock_khz(torch, lib), library=os.path.basename(_lib.LIB_PATH))
    del deg_pos
    name, kw = ('bpr', dict(pairs='bpr')) if args.child == 'bpr' else ('wmrb', {})

    def run(e, prof=None):
        _engine.epoch_wmrb(st, adam, n / S, loss, prof=prof, **kw)
        st.swap()
    res[name + '_epoch_ms'] = timed_epochs(torch, run, args.epochs, args.warmup)
    res[name + '_loss_after'] = float(loss) / plan.n_pos
    prof = _engine.KernelTimer()
    for e in range(args.epochs):
        run(e, prof)
    torch.cuda.synchronize()
    res[name + '_kernels_ms'] = {k: prof.mean_ms(k) for k in SPANS if k in prof.spans}
    print(json.dumps(res), flush=True)


def child_c2(args):
    """BPRLoss at the MovieLens-100K shape through the generic path (what a fit without the engine pays) and the engine."""
    import numpy as np
    import torch

    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import BPRLoss
    from teamoflow_amd.mf.matrix_factorization import MatrixFactorization
    from teamoflow_amd.mf.sparse import SparseInteractions, eye
    rng = np.random.default_rng(0)
    m, n, r, nnz, epochs = 943, 1682, 128, 100_000, 50
    S = n // 2
    keys = rng.choice(m * n, nnz, replace=False)
    idx = np.stack([keys // n, keys % n], 1)
    val = rng.integers(1, 6, nnz).astype(np.float32)
    U0 = (rng.standard_normal((m, r)) * 0.1).astype(np.float32)
    V0 = (rng.standard_normal((n, r)) * 0.1).astype(np.float32)
    R = torch.as_tensor(rng.integers(0, n, (m, S)).astype(np.int32))
    res = dict(shape=dict(m=m, n=n, r=r, S=S), nnz=nnz, epochs=epochs)
    for name in ('generic', 'engine', 'generic', 'engine'):          # the second pair is the record: everything is warm
        model = MatrixFactorization(r, loss_graph=BPRLoss(), user_weight_graph=FixedInitializer(U0), item_weight_graph=FixedInitializer(V0),
                                    n_users=m, n_items=n, n_samples=S)
        model.verbose, model.random_ind = False, R
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
           '--r', str(args.r), '--nnz', str(args.nnz), '--samples', str(args.samples), '--epochs', str(args.epochs),
           '--warmup', str(args.warmup), '--clock-khz', str(args.clock_khz)]
    env = dict(os.environ, **env_extra)
    print(f'[time_bpr_c4] {child} {env_extra}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=limit)
    if p.returncode != 0:
        raise SystemExit(f'{child} run failed with exit status {p.returncode}')
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help="libtmf.so built from the parent commit (its WMRB epoch stands beside the BPR epoch)")
    ap.add_argument('--count-only', action='store_true', help='print the counted instructions as JSON and stop (no GPU)')
    ap.add_argument('--counts', default=None, help='the JSON --count-only printed, instead of compiling again')
    ap.add_argument('--rounds', type=int, default=1)
    ap.add_argument('--epochs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--r', type=int, default=128)
    ap.add_argument('--nnz', type=int, default=100_000_000)
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--limit', type=int, default=420, help='seconds one child process may take')
    ap.add_argument('--clock-khz', type=int, default=0, help='engine clock for the bound; default: what the device reports')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', choices=['bpr', 'wmrb', 'c2'], default=None)
    args = ap.parse_args()
    if args.child == 'c2':
        return child_c2(args)
    if args.child:
        return child_c4(args)
    if args.count_only:
        print(json.dumps(pair_loop_counts()))
        return
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit('--parent-lib: the library of the parent commit runs the WMRB epoch this measurement stands beside; build it first')
    counts = json.load(open(args.counts)) if args.counts else pair_loop_counts()
    parent_env = dict(TMF_LIB=os.path.abspath(args.parent_lib), TMF_LIB_OLDER='1')
    rounds = []
    for _ in range(args.rounds):
        rounds.append(dict(bpr=run_child(args, 'bpr', {}, args.limit), parent=run_child(args, 'wmrb', parent_env, args.limit)))
    first = rounds[0]['bpr']
    kernels = {k: median([x['bpr']['bpr_kernels_ms'][k] for x in rounds]) for k in first['bpr_kernels_ms']}
    parent_kernels = {k: median([x['parent']['wmrb_kernels_ms'][k] for x in rounds]) for k in rounds[0]['parent']['wmrb_kernels_ms']}
    bound = bound_ms(counts, first['iterations'], 4 * first['compute_units'], first['clock_khz'])
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r, S=args.samples), nnz=first['nnz'], n_pos=first['n_pos'], pairs=first['pairs'],
               iterations=first['iterations'], max_positives_of_a_user=first['max_positives_of_a_user'], device=first['device'],
               compute_units=first['compute_units'], clock_khz=first['clock_khz'], epochs=args.epochs, warmup=args.warmup,
               counted_instructions=counts, cycles=dict(plain=CYCLES, transcendental=TRANS_CYCLES), margin=MARGIN,
               bpr_pairs_bound_ms=bound, bpr_pairs_ms=kernels['bpr_pairs'], bpr_pairs_within_bound=bool(kernels['bpr_pairs'] <= bound),
               bpr_epoch_ms=median([x['bpr']['bpr_epoch_ms'] for x in rounds]), bpr_kernels_ms=kernels,
               wmrb_epoch_ms_parent=median([x['parent']['wmrb_epoch_ms'] for x in rounds]), wmrb_kernels_ms_parent=parent_kernels,
               rounds=rounds, c2=run_child(args, 'c2', {}, args.limit))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
