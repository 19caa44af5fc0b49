"""Child process of tests/test_gpu_split_8waves.py, started with TMF_SPLIT_WAVES=8 (read once per process by the library): every
plane-kernel instance that variable makes the dispatcher choose - bf16 planes <4,2,1|2,8>, <2,4,2|4,8>, fp16 planes <4,2,1|2|4,8> -
with and without exclusion, at k <= 16, 17..22 and 23..32 (34 for the bf16 planes), with clamping, on catalogs long enough for the
warm-up pass (>= 256 tiles), against torch's fp64 product and stable sort on the same device.  Small integer factors: every plane
product and every sum is exact, so ids and values must match bit for bit.  k = 35..40 (bf16 planes): the 8-wave lists do not fit
the LDS beside the ring, so these calls go to the 4-wave instances and must still be right.  Prints one line per case; exit
status 0 only if all of them pass."""
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

from oracle import dense_ref as D  # noqa: E402
from teamoflow_amd import _lib, _ops  # noqa: E402


def main():
    assert os.environ.get('TMF_SPLIT_WAVES') == '8'
    _lib.get()
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(8)
    m, n = 300, 40000                                  # 40000 items: 313 tiles of 128, 625 of 64
    cases = 0
    for arith, ks in (('split', (10, 20, 30, 34, 40)), ('half2', (10, 20, 32))):
        for r in (32, 64, 100, 256):                   # planes of width 32, 64, 128, 256
            U = torch.randint(-2, 3, (m, r), generator=g, device=dev, dtype=torch.float32)
            V = torch.randint(-2, 3, (n, r), generator=g, device=dev, dtype=torch.float32)
            # exclusion: each user's 40 best items under the fp64 product (the ones a wrong skip would let through) and random pairs
            top = D.tf_top_k_chunked(U, V, 40)[1]
            rows = torch.cat([torch.arange(m, device=dev).repeat_interleave(40), torch.randint(0, m, (2000,), generator=g, device=dev)])
            cols = torch.cat([top.reshape(-1), torch.randint(0, n, (2000,), generator=g, device=dev)])
            ex = _ops.build_exclusion(torch.sparse_coo_tensor(torch.stack([rows, cols]), torch.ones_like(rows, dtype=torch.float32),
                                                              (m, n)).coalesce().to_dense(), m, n)
            for k in ks:
                for excl in (False, True):
                    clamp = (k + excl) % 2 == 1
                    want_v, want_i = D.tf_top_k_chunked(U, V, k, clamp=clamp, excluded=(rows, cols) if excl else None)
                    got_v, got_i = _ops.predict_topk(U, V, k, clamp_negatives=clamp, return_values=True, arithmetic=arith,
                                                     exclude=ex if excl else None)
                    ok = torch.equal(got_i.long(), want_i) and torch.equal(got_v.double(), want_v)
                    bad = int((got_i.long() != want_i).any(1).sum())
                    print(f'{arith} r={r} k={k} clamp={clamp} exclude={excl}: {"ok" if ok else f"WRONG lists in {bad} of {m} rows"}',
                          flush=True)
                    assert ok, (arith, r, k, clamp, excl)
                    cases += 1
    print(f'8-wave plane kernels: {cases} cases ok')


if __name__ == '__main__':
    main()
