"""Cost of a LogisticLoss epoch on the sparse engine at the C4 shape (1M users x 100K items, r = 128, ~1e8 interactions of
bench.py's generator with a random sign on every value), against its yardstick: the MSE epoch of the PARENT commit's library on the
same plan.  The logistic pass moves exactly the MSE pass's bytes; what it adds is VALU work per entry (one exp, one quotient, a few
selects, and log1p in the user pass), computed by all lanes of a lane group.  The bound allows for all of it staying unhidden:

    allowance = sum over the two passes of  iterations x (4 cycles x added VALU + 16 cycles x added transcendental instructions)
                / (SIMDs x clock)
    logistic epoch <= (MSE epoch (parent) + allowance) x 1.10

The added instructions are counted in the gather loop of the r = 128 fp32 instances (rows of 32 lanes, 2 lane groups x 4 entries in
flight = 8 entries per wave and iteration) of k_logistic_pass, with and without the loss, against k_mse_pass's - in the
assembly hipcc emits for gfx950 (--count-only prints them and needs no GPU; --counts FILE reads them back).  An iteration count is
sum over rows of ceil(entries / 8); SIMDs = 4 per CU and the clock as the device reports them.
A library is chosen when the package is imported, so every measurement is a child process of its own (this process never opens
the GPU); the logistic run and the parent's MSE run alternate, --rounds times.  Second record, no bound: the C2 shape
(943 x 1682, 1e5 interactions) through the generic autograd path against the engine.

    # the parent's library: git worktree add ../parent HEAD~1 && make -C ../parent/teamoflow_amd/csrc OUT=$PWD/libtmf_parent.so
    python tools/time_logistic_c4.py --parent-lib libtmf_parent.so [--out profiles/logistic_c4.json]
"""
import argparse
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MARGIN = 1.10                      # pool spread (tools/time_kl_c4.py's)
VALU_CYCLES, TRANS_CYCLES = 4, 16  # issue cycles of a wave64 VALU / transcendental instruction on one SIMD
TRANSCENDENTAL = ('v_exp_', 'v_log_', 'v_rcp_', 'v_rsq_', 'v_sqrt_', 'v_sin_', 'v_cos_')
ENTRIES_PER_ITERATION = 8          # r = 128 fp32: rows of 32 lanes -> 2 lane groups x 4 entries in flight


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


# ------------------------------------------------------------------------------------------------------------------------
# the added instructions, from the assembly
# ------------------------------------------------------------------------------------------------------------------------
def gather_loop_counts(asm_text, symbol_part):
    """(VALU, transcendental) instructions of the gather loop of the kernel whose symbol contains ``symbol_part``: the innermost
    backward-branch loop that holds the four row loads."""
    lines = asm_text.split('\n')
    start = next(i for i, x in enumerate(lines) if re.match(r'^_ZN3tmf\w+:', x) and symbol_part in x)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
    body = lines[start:end]
    labels = {m.group(1): i for i, x in enumerate(body) for m in [re.match(r'^(\.LBB\d+_\d+):', x)] if m}
    loops = []
    for i, x in enumerate(body):
        m = re.search(r'\bs_c?branch\w*\s+(?:\S+,\s*)?(\.LBB\d+_\d+)', x)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            seg = body[labels[m.group(1)]:i + 1]
            if sum('global_load_dwordx4' in s for s in seg) >= 4:
                loops.append(seg)
    loop = min(loops, key=len)
    ops = [s.split()[0] for s in loop if s.strip() and not s.strip().startswith((';', '.')) and not s.rstrip().endswith(':')]
    trans = sum(op.startswith(TRANSCENDENTAL) for op in ops)
    return sum(op.startswith('v_') for op in ops) - trans, trans


def count_added():
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    texts = {}
    with tempfile.TemporaryDirectory() as tmp:
        for src in ('tmf_logistic.hip', 'tmf_train.hip'):
            out = os.path.join(tmp, src + '.s')
            subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-ffp-contract=on', '-S', '--cuda-device-only',
                            os.path.join(ROOT, 'teamoflow_amd', 'csrc', src), '-o', out], check=True, stderr=subprocess.DEVNULL)
            texts[src] = open(out).read()
    mse = gather_loop_counts(texts['tmf_train.hip'], '10k_mse_passILi32ELi1EfE')
    user = gather_loop_counts(texts['tmf_logistic.hip'], '15k_logistic_passILi32ELi1EfLb1EE')
    item = gather_loop_counts(texts['tmf_logistic.hip'], '15k_logistic_passILi32ELi1EfLb0EE')
    return dict(mse_loop=dict(valu=mse[0], transcendental=mse[1]), user_loop=dict(valu=user[0], transcendental=user[1]),
                item_loop=dict(valu=item[0], transcendental=item[1]),
                added_user=dict(valu=user[0] - mse[0], transcendental=user[1] - mse[1]),
                added_item=dict(valu=item[0] - mse[0], transcendental=item[1] - mse[1]),
                entries_per_iteration=ENTRIES_PER_ITERATION)


def allowance_ms(counts, iters_user, iters_item, simds, clock_khz):
    cycles = sum(iters * (VALU_CYCLES * counts[k]['valu'] + TRANS_CYCLES * counts[k]['transcendental'])
                 for k, iters in (('added_user', iters_user), ('added_item', iters_item)))
    return cycles / (simds * clock_khz)      # cycles / (SIMDs x kHz) = ms


# ------------------------------------------------------------------------------------------------------------------------
# the measurements (child processes)
# ------------------------------------------------------------------------------------------------------------------------
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


def device_clock_khz(torch, lib, dev=0):
    """Peak engine clock in kHz: torch's device properties where they carry it, else hipDeviceAttributeClockRate (= 5) from the HIP
    runtime libtmf.so is linked against - the one torch has loaded (a symbol lookup on the library's handle reaches it)."""
    props = torch.cuda.get_device_properties(dev)
    if hasattr(props, 'clock_rate'):
        return int(props.clock_rate)
    v = ctypes.c_int(0)
    rc = lib.hipDeviceGetAttribute(ctypes.byref(v), 5, dev)
    if rc != 0 or v.value <= 0:
        raise SystemExit(f'hipDeviceGetAttribute(ClockRate) failed with {rc}: pass --clock-khz')
    return int(v.value)


def child_c4(args):
    import torch

    from teamoflow_amd import _engine, _lib
    lib = _lib.get()
    dev = torch.device('cuda', 0)
    clock_khz = args.clock_khz or device_clock_khz(torch, lib)
    idx, val, U0, V0 = c4_problem(args, dev)
    plan = _engine.InteractionPlan(idx, val, args.users, args.items, user_chunks=_engine.mse_user_chunks(), csc=True)
    del idx, val
    st = _engine.TrainState(U0, V0, plan, args.r)
    adam = _engine.adam_constants(0.01)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    props = torch.cuda.get_device_properties(0)
    E = ENTRIES_PER_ITERATION

    def iterations(rowptr):
        return int(((rowptr[1:] - rowptr[:-1] + (E - 1)) // E).sum())
    res = dict(nnz=plan.nnz, n_pos=plan.n_pos, segments_user=plan.seg_u.nseg, segments_item=plan.seg_i.nseg,
               iterations_user=iterations(plan.rowptr_u), iterations_item=iterations(plan.rowptr_i),
               device=torch.cuda.get_device_name(0), compute_units=props.multi_processor_count, clock_khz=clock_khz,
               library=os.path.basename(_lib.LIB_PATH))

    def epoch_of(name, **kw):
        def run(e, prof=None):
            getattr(_engine, name)(st, adam, loss, prof=prof, **kw)
            st.swap()
        return run
    runs = [('mse', epoch_of('epoch_mse'))]
    if args.child == 'logistic':
        runs = [('logistic', epoch_of('epoch_logistic')), ('logistic_w', epoch_of('epoch_logistic', weighted=True))] + runs
    for name, run in runs:
        res[name + '_epoch_ms'] = timed_epochs(torch, run, args.epochs, args.warmup)
        res[name + '_loss_after'] = float(loss)
        prof = _engine.KernelTimer()
        for e in range(args.epochs):
            run(e, prof)
        torch.cuda.synchronize()
        span = name.split('_')[0]
        res[name + '_passes_ms'] = {k: prof.mean_ms(k) for k in (span + '_user_pass', span + '_item_pass')}
    print(json.dumps(res), flush=True)


def child_c2(args):
    """LogisticLoss at the MovieLens-100K shape through the generic path (what a fit without the engine pays) and the engine."""
    import numpy as np
    import torch

    from teamoflow_amd.mf.initializer_graphs import FixedInitializer
    from teamoflow_amd.mf.loss_graphs import LogisticLoss
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
        model = MatrixFactorization(r, loss_graph=LogisticLoss(), user_weight_graph=FixedInitializer(U0),
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
           '--r', str(args.r), '--nnz', str(args.nnz), '--epochs', str(args.epochs), '--warmup', str(args.warmup), '--clock-khz', str(args.clock_khz)]
    env = dict(os.environ, **env_extra)
    print(f'[time_logistic_c4] {child} {env_extra}', file=sys.stderr, flush=True)
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=limit)
    if p.returncode != 0:
        raise SystemExit(f'{child} run failed with exit status {p.returncode}')
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help="libtmf.so built from the parent commit (the yardstick's MSE epoch)")
    ap.add_argument('--count-only', action='store_true', help='print the counted instructions as JSON and stop (no GPU)')
    ap.add_argument('--counts', default=None, help='the JSON --count-only printed, instead of compiling again')
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--epochs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--r', type=int, default=128)
    ap.add_argument('--nnz', type=int, default=100_000_000)
    ap.add_argument('--limit', type=int, default=420, help='seconds one child process may take')
    ap.add_argument('--clock-khz', type=int, default=0, help='engine clock for the allowance; default: what the device reports')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', choices=['logistic', 'mse', 'c2'], default=None)
    args = ap.parse_args()
    if args.child == 'c2':
        return child_c2(args)
    if args.child:
        return child_c4(args)
    if args.count_only:
        print(json.dumps(count_added()))
        return
    if args.r != 128:
        raise SystemExit('the allowance is counted in the r = 128 fp32 instances')
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit('--parent-lib: the library of the parent commit is the yardstick of this measurement; build it first')
    counts = json.load(open(args.counts)) if args.counts else count_added()
    parent_env = dict(TMF_LIB=os.path.abspath(args.parent_lib), TMF_LIB_OLDER='1')
    rounds = []
    for _ in range(args.rounds):
        rounds.append(dict(logistic=run_child(args, 'logistic', {}, args.limit), parent=run_child(args, 'mse', parent_env, args.limit)))
    first = rounds[0]['logistic']
    lg_ms = median([x['logistic']['logistic_epoch_ms'] for x in rounds])
    lgw_ms = median([x['logistic']['logistic_w_epoch_ms'] for x in rounds])
    parent_ms = median([x['parent']['mse_epoch_ms'] for x in rounds])
    allow = allowance_ms(counts, first['iterations_user'], first['iterations_item'], 4 * first['compute_units'], first['clock_khz'])
    bound_ms = (parent_ms + allow) * MARGIN
    passes = {k: median([x['logistic']['logistic_passes_ms'][k] for x in rounds]) for k in first['logistic_passes_ms']}
    res = dict(shape=dict(m=args.users, n=args.items, r=args.r), nnz=first['nnz'], n_pos=first['n_pos'], device=first['device'],
               compute_units=first['compute_units'], clock_khz=first['clock_khz'], epochs=args.epochs, warmup=args.warmup,
               counted_instructions=counts, iterations=dict(user=first['iterations_user'], item=first['iterations_item']),
               allowance_ms=allow, margin=MARGIN, bound_ms=bound_ms, bound=bound_ms / parent_ms,
               logistic_epoch_ms=lg_ms, logistic_weighted_epoch_ms=lgw_ms, logistic_passes_ms=passes,
               mse_epoch_ms_this_library=median([x['logistic']['mse_epoch_ms'] for x in rounds]), mse_epoch_ms_parent=parent_ms,
               ratio=lg_ms / parent_ms, within_bound=bool(lg_ms <= bound_ms), rounds=rounds, c2=run_child(args, 'c2', {}, args.limit))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
