"""The fp64 reference of the scalar item bias tests: torch autograd in float64 of the model's own ``loss_graph.get_loss`` over
U V^T + b, fed as MatrixFactorization._fit_generic feeds it.  Shares no code with the engine.  Not a test module."""
import numpy as np
import torch


def biased_reference(loss_graph, U, V, b, idx, val, R, n_items, n_samples, feeds='samples', dtype=torch.float64):
    """One epoch's loss and gradients at (U, V, b) in float64.  idx: row-major (user, item) pairs, val their stored values, R [m, S]
    the negative table in the model's order (None for a loss that reads none).  feeds: what get_loss is handed ('samples': sample and
    serial predictions, 'dense': the [m, n] matrix).  dtype: torch.float32 runs the same computation in fp32 - the error of that run
    against the float64 one is what fp32 arithmetic costs this loss (tests/test_fuzz_draws_cpu.py derives a tolerance from it).
    -> dict(loss_sum, n_terms, gU, gV, gb, scores) of NumPy float64."""
    from teamoflow_amd.mf.sparse import SparseInteractions
    U, V, b = (torch.tensor(np.asarray(x, np.float64), dtype=dtype, requires_grad=True) for x in (U, V, b))
    idx = torch.as_tensor(np.asarray(idx, np.int64))
    inter = SparseInteractions(idx, torch.as_tensor(np.asarray(val, np.float32)), (U.shape[0], V.shape[0]), device='cpu')
    predictions = U @ V.T + b[None, :]
    samples = serial = None
    if feeds == 'samples':
        samples = torch.gather(predictions, 1, torch.as_tensor(np.asarray(R, np.int64)))
        serial = predictions[idx[:, 0], idx[:, 1]]
    loss = loss_graph.get_loss(tf_interactions=inter, tf_sample_predictions=samples, tf_prediction_serial=serial,
                               predictions=predictions if feeds == 'dense' else None, n_items=n_items, n_samples=n_samples)
    gU, gV, gb = torch.autograd.grad(loss.sum(), (U, V, b), allow_unused=True)
    out = dict(loss_sum=float(loss.detach().double().sum()), n_terms=int(loss.numel()), scores=predictions.detach().double().numpy())
    for name, g, like in (('gU', gU, U), ('gV', gV, V), ('gb', gb, b)):
        g = torch.zeros_like(like) if g is None else g
        out[name] = g.detach().double().numpy().copy()
        out[name].setflags(write=False)
    return out


def margins_decided(scores, idx, val, R, gap=5e-6):
    """Whether a hinge / first-violator / order-statistic loss is decided on these scores however fp32 rounds them: no margin
    1 - p_k + sp[u, s] of a positive within ``gap`` of the kink, and no two distinct positives of a user within ``gap`` of each other.
    gap: fifty times the rounding error an fp32 dot product of 128 terms of this size can have (~1e-7)."""
    scores, idx, R = np.asarray(scores, np.float64), np.asarray(idx, np.int64), np.asarray(R, np.int64)
    pos = np.asarray(val) > 0
    u, i = idx[pos, 0], idx[pos, 1]
    p = scores[u, i]
    sp = np.take_along_axis(scores, R, 1)[u]
    if np.abs(1.0 - p[:, None] + sp).min(initial=1.0) <= gap:
        return False
    for q in np.unique(u):
        mine = np.sort(p[u == q])
        if mine.size > 1 and np.diff(mine).min() <= gap:
            return False
    return True


def ulp32(x):
    """The spacing of float32 at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)
