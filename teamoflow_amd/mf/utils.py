"""Helpers of /root/reference/src/teamoflow/mf/utils.py on torch tensors."""
import numpy as np
import torch
from scipy import sparse as sp

from .. import _ops
from .sparse import SparseInteractions, default_device


def random_sampler(n_items, n_users, n_samples, replace=False):
    """utils.py:8-22.  One ``np.random.choice`` per user from the GLOBAL NumPy RNG, so the same
    ``np.random.seed`` gives the table the reference would draw.  int64 [n_users, n_samples]."""
    items_per_user = [np.random.choice(a=n_items, size=n_samples, replace=replace) for _ in range(n_users)]
    return torch.as_tensor(np.array(items_per_user), dtype=torch.int64).to(default_device())


def _i64(x):
    """Python int -> the int64 value with the same low 64 bits (torch integer arithmetic wraps)."""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= (1 << 63) else x


def _srl(x, s):
    """Logical right shift of an int64 tensor (torch's >> is arithmetic)."""
    return (x >> s) & ((1 << (64 - s)) - 1)


def _mix64(x):
    """splitmix64's finaliser on an int64 tensor: a bijection of the 64-bit words with full avalanche."""
    x = (x ^ _srl(x, 30)) * _i64(0xBF58476D1CE4E5B9)
    x = (x ^ _srl(x, 27)) * _i64(0x94D049BB133111EB)
    return x ^ _srl(x, 31)


def _affine(x, mul, add):
    """x * mul + add in wrapping 64-bit arithmetic, for an int or an int64 tensor x."""
    if torch.is_tensor(x):
        return x * _i64(mul) + _i64(add)
    return torch.tensor(_i64(int(x) * mul + add), dtype=torch.int64)


def counter_hash(seed, a, b=0, c=0):
    """Counter-based random words: a 64-bit hash of (seed, a, b, c), each an int or a broadcastable int64 tensor.  Stateless,
    so the word of (a, b, c) does not depend on which other words are drawn with it - a rank that draws only its own
    users' rows gets exactly the rows of the whole table."""
    h = _mix64(_affine(a, 1, (2 * int(seed) + 1) * 0x9E3779B97F4A7C15))
    k = _affine(b, 0xD6E8FEB86659FD93, 0xA0761D6478BD642F)
    h = _mix64(h ^ k.to(h.device))
    k = _affine(c, 0xE7037ED1A0B428DB, 0x8EBC6AF09C88C6E3)
    return _mix64(h ^ k.to(h.device))


def hash_below(h, n):
    """Random words -> integers in [0, n) (53 random bits; the modulo bias is below n / 2^53)."""
    return _srl(h, 11) % int(n)


def hash_unit(h):
    """Random words -> float64 in (0, 1)."""
    return (_srl(h, 11).to(torch.float64) + 0.5) * (2.0 ** -53)


WEIGHT_TOTAL_MAX = 1 << 33   # the total of the integer weights of a weighted table stays below this
WEIGHTED_FAIL_ROUND = 259    # redraws of a weighted table run in rounds 3 .. 258


def popularity_weights(item_counts, power):
    """int64 [n_items] on the CPU: the integer weights q of popularity-weighted negative sampling (word2vec's unigram^0.75,
    implicit's BPR), for ``random_sampler_device(weights=q)`` / ``_ops.sample_negatives(weights=q)``.  item_counts: the number of
    training interactions of every item (>= 0); power: finite and >= 0 (ValueError otherwise).
    w_i = (c_i + 1)^power and q_i = max(1, floor(w_i / sum(w) * 2^31)), computed ON THE HOST in float64 whatever device the counts
    are on, so a CPU fit and a GPU fit draw the same tables.  Every q_i >= 1 (each item can be drawn), q is monotone in the
    counts and sum(q) <= 2^31 + n_items.  power = 0 gives equal weights: uniform in DISTRIBUTION, not the bits of the unweighted
    sampler (those are the bits of weights that are all 1)."""
    try:
        power = float(power)
    except (TypeError, ValueError):
        raise ValueError(f'power={power!r} is not a number') from None
    if not (np.isfinite(power) and power >= 0.0):
        raise ValueError(f'power={power!r}: the sampling power must be finite and >= 0')
    c = torch.as_tensor(item_counts).detach().cpu().numpy().astype(np.float64).reshape(-1)
    if c.size == 0 or not np.all(np.isfinite(c)) or c.min() < 0:
        raise ValueError('item_counts must be a non-empty vector of finite counts >= 0')
    w = (c + 1.0) ** power
    q = np.maximum(1.0, np.floor(w / w.sum() * float(1 << 31)))
    return torch.from_numpy(q.astype(np.int64))


def log_expected_count(q, n_samples):
    """float32 [n_items] on the CPU: l_i = log(min(1, S q_i / T)), T = sum(q) - what sampling_correction='logq' subtracts from the
    sampled logit of item i under a table of S = n_samples columns drawn with the weights q (any non-negative numbers, not all zero;
    ``popularity_weights`` makes the ones a fit uses).  S q_i / T is the WITH-REPLACEMENT expected count of item i among the S draws
    of a row, clamped at the one appearance a row of distinct items can hold.  It is not the exact inclusion probability of the
    rejection sampler, which redraws repeated items and so proposes light items a little more often than this says.  0.0 where
    q_i = 0: that item is never drawn, so the value is never read.  Computed ON THE HOST in float64 whatever device q is on, like
    popularity_weights, and rounded to float32 once: a CPU fit and a GPU fit subtract the same numbers.  Equal weights give the one
    value float32(log(S / n_items)) (0.0 once S >= n_items)."""
    S = int(n_samples)
    w = torch.as_tensor(q).detach().cpu().numpy().astype(np.float64).reshape(-1)
    if S < 1:
        raise ValueError(f'n_samples={n_samples!r}: at least one sample')
    if w.size == 0 or not np.all(np.isfinite(w)) or w.min() < 0 or not w.sum() > 0:
        raise ValueError('q must be a non-empty vector of finite weights >= 0 with a positive total')
    count = np.minimum(1.0, S * w / w.sum())
    ell = np.zeros_like(count)
    np.log(count, out=ell, where=count > 0)
    return torch.from_numpy(ell.astype(np.float32))


def weighted_cum(weights, n_items, n_samples):
    """The checked prefix sums of a weighted table: int64 [n_items] on the CPU, cum[i] = q_0 + ... + q_i.  weights: int64 [n_items],
    q_i >= 0, total T = sum(q) with 1 <= T < 2^33 (TypeError / ValueError otherwise).  The admission rule, in integers: with H the sum
    of the n_samples largest weights, 4 H <= 3 T - a row holds fewer than n_samples distinct items while it is redrawn, they hold at
    most H of the mass, so every redraw lands outside them with probability >= 1/4 (the uniform sampler's 2 S <= n_items says the
    same with 1/2).  ValueError otherwise, before anything is drawn."""
    n_items, n_samples = int(n_items), int(n_samples)
    if not torch.is_tensor(weights) or weights.dtype != torch.int64:
        raise TypeError('weights must be an int64 tensor (utils.popularity_weights makes one)')
    if weights.dim() != 1 or weights.numel() != n_items:
        raise ValueError(f'weights has shape {tuple(weights.shape)}, expected [{n_items}]')
    q = weights.detach().cpu()
    if n_items == 0 or int(q.min()) < 0:
        raise ValueError('weights must be >= 0 (and there must be an item)')
    if int(q.max()) >= WEIGHT_TOTAL_MAX:   # before the sums: they must not wrap
        raise ValueError(f'weights: a weight of {int(q.max())}; the total must lie in [1, 2^33)')
    cum = torch.cumsum(q, 0)
    total = int(cum[-1])
    if not 1 <= total < WEIGHT_TOTAL_MAX:
        raise ValueError(f'weights: their total is {total}; it must lie in [1, 2^33)')
    if n_samples > n_items:
        raise ValueError("Cannot take a larger sample than population when 'replace=False'")
    heavy = int(torch.topk(q, n_samples)[0].sum()) if n_samples > 0 else 0
    if 4 * heavy > 3 * total:
        raise ValueError(f'weighted sampling of {n_samples} distinct items: the {n_samples} heaviest items hold {heavy} of the total '
                         f'weight {total}, more than 3/4 - a row could not be completed in bounded time.  Use a smaller power or '
                         f'fewer samples')
    return cum


def weighted_item(x, cum):
    """The item of the integers x in [0, T): the first i with cum[i] > x.  An item of weight 0 is never the answer."""
    return torch.searchsorted(cum, x, right=True)


def random_sampler_device(n_items, n_users, n_samples, seed=0, device=None, rows_per_block=32768, user_offset=0, weights=None):
    """Extension for tables too large for the host loop above (1M users x 1024 samples): distinct
    items per user drawn on the device.  Not the NumPy stream - use ``random_sampler`` for parity.
    The row of user u is a function of (seed, u) alone (counter_hash): ``user_offset=b`` returns rows b .. b + n_users of
    the table, so the ranks of a user-partitioned job each draw their own block of ONE table.
    weights (int64 [n_items], None = uniform, the function as it always was): every draw takes item i with probability q_i / T
    instead - x = (h >> 11) mod T of the same random words, item = weighted_item(x, cum) -, the rest is the rejection branch with
    redraw rounds 3 .. 258.  weighted_cum states what weights are admitted (ValueError otherwise: there is no weighted permutation
    branch).  The row of user u is then a function of (seed, u, weights) alone; weights that are all 1 give the uniform table."""
    if weights is not None:
        return _weighted_sampler_device(n_items, n_users, n_samples, seed, device, rows_per_block, user_offset, weights)
    if n_samples > n_items:
        raise ValueError("Cannot take a larger sample than population when 'replace=False'")
    device = default_device() if device is None else torch.device(device)
    out = torch.empty(n_users, n_samples, dtype=torch.int32, device=device)
    if 2 * n_samples > n_items:
        # most of the catalog per row: rejection would take coupon-collector time - the first n_samples entries of a random
        # permutation instead (argsort of per-(user, item) keys), in blocks of at most 2^25 keys
        step = max(1, (1 << 25) // n_items)
        items = torch.arange(n_items, device=device, dtype=torch.int64)[None, :]
        for r0 in range(0, n_users, step):
            rows = min(step, n_users - r0)
            u = torch.arange(user_offset + r0, user_offset + r0 + rows, device=device, dtype=torch.int64)[:, None]
            keys = _srl(counter_hash(seed, u, items, 1), 1)
            out[r0:r0 + rows] = torch.argsort(keys, dim=1, stable=True)[:, :n_samples].to(torch.int32)
        return out
    rows_per_block = max(1, min(rows_per_block, (1 << 25) // n_samples))
    pos = torch.arange(n_samples, device=device, dtype=torch.int64)[None, :]
    for r0 in range(0, n_users, rows_per_block):
        rows = min(rows_per_block, n_users - r0)
        u = torch.arange(user_offset + r0, user_offset + r0 + rows, device=device, dtype=torch.int64)[:, None]
        # every row is kept sorted between rounds and a repeated item is redrawn from (user, position, round): what happens
        # to a row never depends on the other rows of the block (a row without repeats is a fixed point of a round)
        blk = torch.sort(hash_below(counter_hash(seed, u, pos, 2), n_items), dim=1)[0]
        for rnd in range(3, 67):
            dup = torch.zeros_like(blk, dtype=torch.bool)
            dup[:, 1:] = blk[:, 1:] == blk[:, :-1]
            if not bool(dup.any()):
                break
            blk = torch.sort(torch.where(dup, hash_below(counter_hash(seed, u, pos, rnd), n_items), blk), dim=1)[0]
        else:
            raise RuntimeError('could not draw distinct samples')
        shuffle = torch.argsort(_srl(counter_hash(seed, u, pos, 0), 1), dim=1, stable=True)
        out[r0:r0 + rows] = torch.gather(blk, 1, shuffle).to(torch.int32)
    return out


def _weighted_sampler_device(n_items, n_users, n_samples, seed, device, rows_per_block, user_offset, weights):
    """random_sampler_device(weights=...): its rejection branch with weighted_item for hash_below.  The definition of the weighted
    table (tmf_sample_rows_weighted restates it)."""
    cum = weighted_cum(weights, n_items, n_samples)
    total = int(cum[-1])
    device = default_device() if device is None else torch.device(device)
    cum = cum.to(device)
    out = torch.empty(n_users, n_samples, dtype=torch.int32, device=device)
    if n_samples == 0:
        return out
    rows_per_block = max(1, min(rows_per_block, (1 << 25) // n_samples))
    pos = torch.arange(n_samples, device=device, dtype=torch.int64)[None, :]
    for r0 in range(0, n_users, rows_per_block):
        rows = min(rows_per_block, n_users - r0)
        u = torch.arange(user_offset + r0, user_offset + r0 + rows, device=device, dtype=torch.int64)[:, None]
        blk = torch.sort(weighted_item(hash_below(counter_hash(seed, u, pos, 2), total), cum), dim=1)[0]
        for rnd in range(3, WEIGHTED_FAIL_ROUND + 1):
            dup = torch.zeros_like(blk, dtype=torch.bool)
            dup[:, 1:] = blk[:, 1:] == blk[:, :-1]
            if not bool(dup.any()):
                break
            if rnd == WEIGHTED_FAIL_ROUND:
                raise RuntimeError('could not draw distinct samples')
            blk = torch.sort(torch.where(dup, weighted_item(hash_below(counter_hash(seed, u, pos, rnd), total), cum), blk), dim=1)[0]
        shuffle = torch.argsort(_srl(counter_hash(seed, u, pos, 0), 1), dim=1, stable=True)
        out[r0:r0 + rows] = torch.gather(blk, 1, shuffle).to(torch.int32)
    return out


def generate_random_interaction(n_users, n_items, min_val=0.0, max_val=5.0, density=0.50):
    """utils.py:25-59: scipy.sparse.random -> affine rescale -> round -> (sparse, dense) pair."""
    p = sp.random(n_users, n_items, density=density)
    p = (max_val - min_val) * p + min_val * p.ceil()
    random_arr = np.round(p.toarray())
    interactions = SparseInteractions.from_scipy(sp.csr_matrix(random_arr))
    A = torch.as_tensor(random_arr, dtype=torch.float32).to(default_device())
    return interactions, A


def gather_matrix_indices(input_arr, index_arr):
    """utils.py:62-105: out[i, c] = input_arr[i, index_arr[i, c]] (torch.gather along dim 1)."""
    return _ops.gather_rows_cols(input_arr, index_arr)
