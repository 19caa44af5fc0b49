"""Share of list entries whose weight is exactly 0 in the WMRB epochs bench.py times, at the C4 shape (1M users x 100K items,
r = 128, S = 1024, ~1e8 interactions, lr = 0.1, the benchmark's own generator, negative table and initial tables).

An inactive hinge term gives D[u, s] = 0 and a positive without an active sample gives delta_k = 0 (tmf_hinge.hip); gradU
(k_wmrb_gradu3) and the item pass (k_wsum_pass*) walk lists of (row, weight) entries, and an entry of weight 0 adds nothing.  After
every epoch this records the share of exact zeros (+0 or -0) in wplan.D, in wplan.delta and over both together - the entries of
gradU's lists are exactly D and delta - and over the item pass's lists (D and the delta of the positives with a value > 0, gathered
through ent_w).  The mean over the timed epochs (warmup + 1 .. epochs, bench.py's --warmup 5 --steps 20 by default) is the share of
those kernels' row loads whose result is multiplied by zero.

    python tools/zero_weight_share.py [--out profiles/zero_weights_c4.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def zero_share(x, chunk=1 << 27):
    """(exact zeros, elements) of a flat float tensor, counted in chunks (bounded transient memory)."""
    x = x.reshape(-1)
    zeros = 0
    for b in range(0, x.numel(), chunk):
        zeros += int((x[b:b + chunk] == 0).sum())
    return zeros, x.numel()


def gathered_zero_share(wbuf, ent_w, chunk=1 << 27):
    """(exact zeros, entries) of wbuf[ent_w]: the weights the item pass gathers, list entry by list entry."""
    zeros = 0
    for b in range(0, ent_w.numel(), chunk):
        zeros += int((wbuf[ent_w[b:b + chunk].long()] == 0).sum())
    return zeros, ent_w.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=5, help='epochs before the ones bench.py times (the mean is taken after them)')
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--rank', type=int, default=128, dest='r')
    ap.add_argument('--nnz', type=int, default=100_000_000)
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--lr', type=float, default=0.1)
    ap.add_argument('--item-dist', choices=['zipf', 'uniform'], default='zipf')
    ap.add_argument('--dtype', choices=['f32', 'bf16'], default='f32')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'zero_weights_c4.json'))
    args = ap.parse_args()

    import torch

    import bench
    from teamoflow_amd import _engine, _lib
    _lib.get()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    wl = bench.Workload(args, args.users, args.items, args.nnz, args.r, args.samples, 'wmrb', args.dtype, 0, 1, dev)
    st, w = wl.st, wl.wplan
    n_item_lists = int(w.rowptr_e[-1])   # entries of the item pass's lists (positives with a stored value <= 0 are in none)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    per_epoch = []
    for e in range(1, args.epochs + 1):
        _engine.epoch_wmrb(st, wl.adam, wl.c, loss)
        st.swap()
        torch.cuda.synchronize()
        zD, nD = zero_share(w.D)
        zd, nd = zero_share(w.delta)
        zi, ni = gathered_zero_share(w.wbuf, w.ent_w[:n_item_lists])
        per_epoch.append(dict(epoch=e, loss=float(loss), D_zero_share=zD / nD, delta_zero_share=zd / nd,
                              gradu_entries_zero_share=(zD + zd) / (nD + nd), item_pass_entries_zero_share=zi / ni))
        print(f'[zero_weight_share] epoch {e}: D {zD / nD:.4f}  delta {zd / nd:.4f}  gradU lists {(zD + zd) / (nD + nd):.4f}  '
              f'item-pass lists {zi / ni:.4f}', file=sys.stderr, flush=True)
    timed = per_epoch[args.warmup:]
    keys = ('D_zero_share', 'delta_zero_share', 'gradu_entries_zero_share', 'item_pass_entries_zero_share')
    res = dict(shape=dict(m=wl.m, n=wl.n, r=args.r, S=args.samples), nnz=wl.nnz, lr=args.lr, dtype=args.dtype, epochs=args.epochs,
               device=torch.cuda.get_device_name(0), D_elements=int(w.D.numel()), delta_elements=int(w.delta.numel()),
               item_pass_entries=n_item_lists, n_slices=w.n_slices, user_chunks=w.user_chunks,
               timed_epochs=[args.warmup + 1, args.epochs],
               mean_over_timed_epochs={k: sum(x[k] for x in timed) / len(timed) for k in keys},
               per_epoch=per_epoch)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
