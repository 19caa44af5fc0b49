"""The two builders of the item-run score streams (_engine.Scores7Plan: builder='device' = csrc/tmf_s7plan.hip, builder='torch' = the
global sorts, unchanged from the parent commit) at the C4 shape of bench.py (1M users x 100K items, r = 128, S = 1024, ~1e8
interactions of the zipf generator), in ONE process on one problem:

  1. both plans are built (constructor, then order_by_fill) and compared with torch.equal: steps in item order, then steps, place,
     sub_step, sub_place, chunk_sub, sub_fill and sub_wave in fill order.  Nothing is timed before this holds - it is also the only
     place where offsets beyond 4 GB (steps: 7 GB, place: 4.4 GB) are exercised, and the warm-up of both.
  2. constructor + order_by_fill of either builder, alternated --rounds times, each between synchronisations on a host clock, with
     its torch.cuda.max_memory_allocated peak above what was allocated before it started.
Conditions (no margin): the median device build is faster than the median torch build, and its highest peak is not above the torch
build's.  Recorded beside them: the ratio, the bytes the device build has to read and write (counted from the shapes: the counting
and the writing pass each read the ids of all entries once - col_u, R - the first writes the per-sub-chunk tables, the second place
and the steps), and that traffic over the measured time as a share of the HBM stream rate.  The kernels also bisect in the users'
lists and sort every sub-chunk in LDS, so this share says how far the build is from a pure stream, not how busy the memory was.

    python tools/time_scores7_plan_c4.py [--rounds 3] [--out profiles/scores7_plan_c4.json]
"""
import argparse
import json
import os
import sys
import timeit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GBPS = 8000.0   # MI355X peak
SEVEN = ('steps', 'place', 'sub_step', 'sub_place', 'chunk_sub', 'sub_fill', 'sub_wave')


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--r', type=int, default=128)
    ap.add_argument('--nnz', type=int, default=100_000_000)
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch

    import bench
    from teamoflow_amd import _engine, _lib
    from teamoflow_amd.mf.utils import random_sampler_device
    _lib.get()
    dev = torch.device('cuda', 0)
    m, n, r, S = args.users, args.items, args.r, args.samples
    idx, val = bench.gen_interactions(m, n, args.nnz, 'zipf', 0, dev)
    plan = _engine.InteractionPlan(idx, val, m, n, user_chunks=1, csc=False)
    del idx, val
    wplan = _engine.wmrb_plan_for(plan, random_sampler_device(n, m, S, seed=100, device=dev), r, force_sliced=True)

    def build(builder):
        return _engine.Scores7Plan(plan, wplan, r, torch.float32, builder=builder)

    # 1. the same bits, before any clock starts
    t, d = build('torch'), build('device')
    same = dict(steps_item_order=bool(torch.equal(t.steps, d.steps)))
    t.order_by_fill(), d.order_by_fill()
    same.update({name: bool(torch.equal(getattr(t, name), getattr(d, name))) for name in SEVEN})
    same['sizes'] = (t.n_steps, t.n_sub, t.n_entries) == (d.n_steps, d.n_sub, d.n_entries)
    sizes = dict(n_entries=d.n_entries, n_steps=d.n_steps, n_sub=d.n_sub, n_chunks=d.n_slices * d.n_groups, n_slices=d.n_slices,
                 width=d.width, slots=d.slots, nnz=plan.nnz, steps_bytes=d.steps.numel() * 4, place_bytes=d.place.numel() * 4)
    del t, d
    if not all(same.values()):
        raise SystemExit(f'the device build differs from the torch build: {same}')
    torch.cuda.empty_cache()

    # 2. the clock
    runs = dict(device=[], torch=[])
    for rnd in range(args.rounds):
        for builder in ('device', 'torch'):
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = timeit.default_timer()
            s7 = build(builder)
            torch.cuda.synchronize()
            t1 = timeit.default_timer()
            s7.order_by_fill()
            torch.cuda.synchronize()
            t2 = timeit.default_timer()
            runs[builder].append(dict(constructor_ms=(t1 - t0) * 1e3, order_by_fill_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3,
                                      peak_bytes_above_start=torch.cuda.max_memory_allocated() - before))
            del s7
            print(f'[time_scores7_plan_c4] round {rnd} {builder}: {runs[builder][-1]}', file=sys.stderr, flush=True)
    med = {b: median([x['total_ms'] for x in v]) for b, v in runs.items()}
    peak = {b: max(x['peak_bytes_above_start'] for x in v) for b, v in runs.items()}
    E, n_steps, n_sub, nc = sizes['n_entries'], sizes['n_steps'], sizes['n_sub'], sizes['n_chunks']
    rowptr = 8 * (m + 1)
    # the timed build = the three calls once each: order_by_fill() comes before anything reads the streams, so they are written once
    traffic = dict(chunks_pass=rowptr + 2 * 12 * (nc + 1),                           # bisections only; counts, chunk_ent, chunk_sub
                   subs_pass=4 * E + rowptr + 12 * nc + (16 + 8 + 8 + 8) * n_sub,     # ids; sub_fill, counts, sub_place, sub_step
                   streams_pass=4 * E + rowptr + 12 * nc + 8 * n_sub + 4 * E + 16 * (n_steps + 1))   # ids; place, steps
    total = sum(traffic.values())
    res = dict(shape=dict(m=m, n=n, r=r, S=S), device=torch.cuda.get_device_name(0), rounds=args.rounds, sizes=sizes, same_bits=same,
               median_total_ms=med, ratio_torch_over_device=med['torch'] / med['device'], peak_bytes_above_start=peak,
               conditions=dict(device_build_is_faster=bool(med['device'] < med['torch']),
                               device_peak_not_above_torch_peak=bool(peak['device'] <= peak['torch'])),
               device_build_bytes=dict(traffic, total=total, counted='from the shapes: what a build must read and write, not a counter'),
               device_build_gbps=total / (med['device'] * 1e-3) / 1e9,
               share_of_hbm_stream=total / (med['device'] * 1e-3) / 1e9 / HBM_GBPS, hbm_stream_gbps=HBM_GBPS, runs=runs)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    if not all(res['conditions'].values()):
        raise SystemExit(f"conditions not met: {res['conditions']}")


if __name__ == '__main__':
    main()
