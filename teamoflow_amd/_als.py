"""Alternating least squares (an extension: implicit's flagship method, Hu, Koren and Volinsky) over the engine's interaction plans.

One row of either side, with stored entries k (column j_k, value a_k) and the other side's table Y, gets the exact minimiser x of its
part of the objective:

    A x = b,   A = G0 + reg I + sum_k w_k y_k y_k^T,   b = sum_k t_k y_k,   y_k = Y[j_k]

implicit:  G0 = Y^T Y, w_k = alpha |a_k|, t_k = (1 + w_k) [a_k > 0]   (confidence 1 + alpha |a|, preference 1 for a stored value > 0
           and 0 for everything else: a stored 0 changes nothing, a stored negative value is a confident zero)
explicit:  no G0, w_k = 1, t_k = a_k                                  (least squares over the stored entries only)

Duplicates of a pair add up; a row without entries gets x = 0.  Both half-steps minimise, and loss_history_ records (s_k the score of
entry k's pair)

    L = <U^T U, V^T V> [implicit] + sum_k (w_k s_k^2 - 2 t_k s_k + c0_k) + reg (||U||_F^2 + ||V||_F^2),   c0_k = t_k | a_k^2

With a GPU the half-step is tmf_gram_f32 + tmf_als_solve_rows_f32 (one workgroup per row: fp32 MFMA normal matrix, Cholesky in
registers and LDS).  Without one, solve_rows_torch restates the formulas with torch.linalg.cholesky_ex / cholesky_solve in fp32 over
chunks of rows - the form LogisticLoss and BPRLoss have where there is no GPU.  L is summed in fp64 where the tables are, from the
per-entry scores (tmf_pair_scores_f32, or chunks of entries) and two r x r Gram matrices: no [m, n] and no [nnz, r] temporary.

solver='cg' (implicit's use_cg, for n_components up to 256) replaces the exact solve by cg_steps steps of conjugate gradients from the
row's current value x0 (zeros for a fold-in).  A is never formed:  A v = G0 v + reg v + sum_k w_k (y_k . v) y_k.  THE ITERATION, fp32,
every sum in a fixed order (tmf_als_cg_rows_f32 on a GPU, solve_rows_cg_torch without one, tests/als_cg_ref.py in NumPy):

    x = x0      res = b - A x      p = res      rs = res . res      stop = max(1e-14 (b . b), 1e-30)
    repeat cg_steps times:
        if rs <= stop: finished      (fp32 cannot lower the residual further; also covers rs == 0)
        Ap = A p;  pAp = p . Ap
        if pAp is not a positive finite number: the row FAILS (x = 0, n_failed += 1), as an indefinite matrix does under Cholesky
        a = rs / pAp;  x += a p;  res -= a Ap;  rs' = res . res;  p = res + (rs' / rs) p;  rs = rs'

A row without entries gets x = 0 whatever x0 was.  A row's result depends on its entries, Y, G0, reg, x0 and cg_steps only.
"""
import timeit

import numpy as np
import torch

from . import _engine, _lib, _ops

MAX_COMPONENTS = _ops.ALS_MAX_COMPONENTS
CG_MAX_COMPONENTS = _ops.ALS_CG_MAX_COMPONENTS
CG_MAX_STEPS = _ops.ALS_CG_MAX_STEPS
SOLVERS = ('cholesky', 'cg')
CG_CHUNK_ENTRIES = 1 << 20    # entries a chunk of rows may hold in solve_rows_cg_torch ([entries, r] gathered rows)
CPU_CHUNK_FLOATS = 1 << 24    # floats of per-entry outer products a chunk of rows may hold (solve_rows_torch)
OBJECTIVE_CHUNK = 1 << 18     # rows / entries per fp64 chunk of the objective


def check_hyper(reg, alpha):
    """(reg, alpha) as floats: reg finite and > 0, alpha finite and >= 0, else ValueError."""
    reg = _ops._als_reg(reg)
    try:
        alpha = float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f'alpha={alpha!r} is not a number') from None
    if not 0.0 <= alpha <= float(np.finfo(np.float32).max):   # NaN fails both comparisons
        raise ValueError(f'alpha={alpha!r}: the confidence scale must be finite and >= 0')
    return reg, alpha


def check_solver(solver, cg_steps):
    """(solver, cg_steps): solver 'cholesky' or 'cg', cg_steps an int in [1, 32] (checked for either solver), else ValueError."""
    if solver not in SOLVERS:
        raise ValueError(f"solver={solver!r}: 'cholesky' or 'cg'")
    if isinstance(cg_steps, bool) or not isinstance(cg_steps, (int, np.integer)) or not 1 <= int(cg_steps) <= CG_MAX_STEPS:
        raise ValueError(f'cg_steps={cg_steps!r}: an int in [1, {CG_MAX_STEPS}]')
    return solver, int(cg_steps)


def entry_terms(values, alpha, implicit):
    """(w, t, c0) of the stored values, float32."""
    a = values.to(torch.float32)
    if implicit:
        w = a.abs() * float(alpha)
        t = (1.0 + w) * (a > 0).to(torch.float32)
        return w, t, t
    return torch.ones_like(a), a, a * a


def solve_rows_torch(Y, rowptr, col, w, t, reg, G0=None, max_floats=CPU_CHUNK_FLOATS):
    """The half-step in torch, fp32, where the operands are: -> (X [n_rows, r], number of rows that were not positive definite).
    Rows are taken in chunks whose per-entry outer products fit max_floats; a single row beyond that is summed by matrix products."""
    Y = Y.detach().to(torch.float32)
    dev, r = Y.device, Y.shape[1]
    n_rows = rowptr.numel() - 1
    X = torch.zeros(n_rows, r, dtype=torch.float32, device=dev)
    base = float(reg) * torch.eye(r, dtype=torch.float32, device=dev)
    if G0 is not None:
        base = G0.to(torch.float32) + base
    counts = rowptr[1:] - rowptr[:-1]
    limit = max(1, int(max_floats) // (r * r))   # entries, and rows, per chunk
    failed, a = 0, 0
    while a < n_rows:
        e0 = int(rowptr[a])
        b = int(torch.searchsorted(rowptr, torch.tensor(e0 + limit, device=dev), right=True)) - 1
        b = max(a + 1, min(b, n_rows, a + limit))
        e1 = int(rowptr[b])
        Yg = Y[col[e0:e1].long()] if e1 - e0 <= limit else None
        A = base.expand(b - a, r, r).clone()
        if Yg is None:
            # one row with more entries than a chunk may hold as outer products: its normal matrix as matrix products over pieces
            # of its entries, [limit, r] at a time
            rhs = torch.zeros(1, r, dtype=torch.float32, device=dev)
            for p0 in range(e0, e1, limit):
                piece = Y[col[p0:min(p0 + limit, e1)].long()]
                A[0] += (w[p0:p0 + piece.shape[0], None] * piece).T @ piece
                rhs[0] += piece.T @ t[p0:p0 + piece.shape[0]]
        else:
            local = torch.repeat_interleave(torch.arange(b - a, device=dev), counts[a:b])
            A.index_add_(0, local, (w[e0:e1, None] * Yg)[:, :, None] * Yg[:, None, :])
            rhs = torch.zeros(b - a, r, dtype=torch.float32, device=dev).index_add_(0, local, t[e0:e1, None] * Yg)
        L, info = torch.linalg.cholesky_ex(A)
        bad = info != 0
        if bool(bad.any()):
            L[bad] = torch.eye(r, dtype=torch.float32, device=dev)
        x = torch.cholesky_solve(rhs[:, :, None], L)[:, :, 0]
        x[bad | (counts[a:b] == 0)] = 0.0
        X[a:b] = x
        failed += int(bad.sum())
        a = b
    return X, failed


def solve_rows_cg_torch(Y, rowptr, col, w, t, reg, G0=None, x0=None, cg_steps=3, max_entries=CG_CHUNK_ENTRIES):
    """The iteration of the module docstring in torch, fp32, vectorised over chunks of rows -> (X [n_rows, r], rows that failed).
    Per application one index_add_ over the chunk's entries and one P @ (G0 + reg I): no [rows, r, r] temporary."""
    Y = Y.detach().to(torch.float32)
    dev, r = Y.device, Y.shape[1]
    n_rows = rowptr.numel() - 1
    X = torch.zeros(n_rows, r, dtype=torch.float32, device=dev)
    base = float(reg) * torch.eye(r, dtype=torch.float32, device=dev)
    if G0 is not None:
        base = G0.to(torch.float32) + base
    counts = rowptr[1:] - rowptr[:-1]
    fmax = float(np.finfo(np.float32).max)
    failed, a = 0, 0
    while a < n_rows:
        e0 = int(rowptr[a])
        b = int(torch.searchsorted(rowptr, torch.tensor(e0 + int(max_entries), device=dev), right=True)) - 1
        b = max(a + 1, min(b, n_rows))
        e1 = int(rowptr[b])
        Yg = Y[col[e0:e1].long()]
        local = torch.repeat_interleave(torch.arange(b - a, device=dev), counts[a:b])
        wk = w[e0:e1].to(torch.float32)

        def apply(P):
            s = wk * (Yg * P[local]).sum(1)
            return (P @ base).index_add_(0, local, s[:, None] * Yg)

        rhs = torch.zeros(b - a, r, dtype=torch.float32, device=dev).index_add_(0, local, t[e0:e1, None].to(torch.float32) * Yg)
        x = torch.zeros_like(rhs) if x0 is None else x0[a:b].detach().to(device=dev, dtype=torch.float32).clone()
        res = rhs - apply(x)
        p = res.clone()
        rs = (res * res).sum(1)
        stop = torch.clamp(1e-14 * (rhs * rhs).sum(1), min=1e-30)
        active = counts[a:b] > 0
        bad = torch.zeros_like(active)
        for _ in range(int(cg_steps)):
            active = active & ~(rs <= stop)
            if not bool(active.any()):
                break
            p = torch.where(active[:, None], p, torch.zeros_like(p))
            Ap = apply(p)
            pAp = (p * Ap).sum(1)
            fails = active & ~((pAp > 0) & (pAp <= fmax))
            bad |= fails
            active = active & ~fails
            step = torch.where(active, rs / torch.where(active, pAp, torch.ones_like(pAp)), torch.zeros_like(rs))
            x = x + step[:, None] * p
            res = res - step[:, None] * Ap
            rs_new = torch.where(active, (res * res).sum(1), rs)
            beta = torch.where(active, rs_new / torch.where(active, rs, torch.ones_like(rs)), torch.zeros_like(rs))
            p = res + beta[:, None] * p
            rs = rs_new
        x[bad | (counts[a:b] == 0)] = 0.0
        X[a:b] = x
        failed += int(bad.sum())
        a = b
    return X, failed


def half_step(Y, rowptr, col, w, t, reg, implicit, out=None, n_failed=None, solver='cholesky', cg_steps=3, x0=None, ids=None):
    """Every row of the CSR solved against Y [n_other, r] -> (X [n_rows, r], n_failed int32 [1]); out / n_failed as
    _ops.als_solve_rows.  The ids and the CSR come from an InteractionPlan, which has checked them.  solver='cg': cg_steps steps
    from x0 (None: zeros; ``out`` itself: in place); ids (the GPU's launch order: every row once, heavy rows first) changes no result."""
    if Y.is_cuda:
        G0 = _ops.gram(Y) if implicit else None
        if solver == 'cg':
            return _ops.als_cg_rows(Y, rowptr, col, w, t, reg, G0=G0, ids=ids, x0=x0, out=out, n_failed=n_failed, cg_steps=cg_steps,
                                    check=False)
        return _ops.als_solve_rows(Y, rowptr, col, w, t, reg, G0=G0, out=out, n_failed=n_failed, check=False)
    Yf = Y.detach().to(torch.float32)
    G0 = Yf.T @ Yf if implicit else None
    if solver == 'cg':
        X, failed = solve_rows_cg_torch(Yf, rowptr, col, w, t, reg, G0=G0, x0=x0, cg_steps=cg_steps)
    else:
        X, failed = solve_rows_torch(Yf, rowptr, col, w, t, reg, G0=G0)
    if out is not None:
        out.copy_(X)
        X = out
    if n_failed is None:
        n_failed = torch.zeros(1, dtype=torch.int32, device=Y.device)
    n_failed += failed
    return X, n_failed


def _gram64(T):
    G = torch.zeros(T.shape[1], T.shape[1], dtype=torch.float64, device=T.device)
    for a in range(0, T.shape[0], OBJECTIVE_CHUNK):
        c = T[a:a + OBJECTIVE_CHUNK].to(torch.float64)
        G += c.T @ c
    return G


def objective(U, V, rows, cols, w, t, c0, reg, implicit):
    """L of the module docstring as a 0-dim float64 tensor where the tables are.  rows / cols: int32 user and item of every entry."""
    if U.is_cuda:
        s = _ops.pair_scores(U, V, rows, cols).to(torch.float64)
        L = (w.to(torch.float64) * s * s - 2.0 * t.to(torch.float64) * s + c0.to(torch.float64)).sum()
    else:
        L = torch.zeros((), dtype=torch.float64, device=U.device)
        for a in range(0, rows.numel(), OBJECTIVE_CHUNK):
            e = slice(a, a + OBJECTIVE_CHUNK)
            s = (U[rows[e].long()].to(torch.float64) * V[cols[e].long()].to(torch.float64)).sum(1)
            L = L + (w[e].to(torch.float64) * s * s - 2.0 * t[e].to(torch.float64) * s + c0[e].to(torch.float64)).sum()
    L = L + float(reg) * (torch.linalg.vector_norm(U, dtype=torch.float64) ** 2 + torch.linalg.vector_norm(V, dtype=torch.float64) ** 2)
    if implicit:
        L = L + (_gram64(U) * _gram64(V)).sum()
    return L


def heavy_first(rowptr):
    """The launch order of the CG kernel's rows (int32; None without a GPU, where nothing is launched): by falling number of entries
    (stable), so that rows of similar length share a 32-row batch - except the rows the kernel walks with a whole workgroup, one
    after the other (_ops.ALS_CG_LONG_ROW entries or more), which are dealt round-robin over the batches, heaviest first, instead of
    filling the first batches on their own.  The order changes no result."""
    if not rowptr.is_cuda:
        return None
    counts = rowptr[1:] - rowptr[:-1]
    q, batch = counts.numel(), _ops.ALS_CG_BATCH
    order = torch.argsort(counts, descending=True, stable=True)
    n_long, full = int((counts >= _ops.ALS_CG_LONG_ROW).sum()), q // batch
    if 0 < n_long <= full * batch:
        k = torch.arange(n_long, device=order.device)
        at = (k % full) * batch + k // full            # long row k: batch k mod full, slot k div full
        free = torch.ones(q, dtype=torch.bool, device=order.device)
        free[at] = False
        dealt = torch.empty_like(order)
        dealt[at] = order[:n_long]
        dealt[free.nonzero().flatten()] = order[n_long:]   # the others keep their order in the slots that are left
        order = dealt
    return order.to(torch.int32)


def fit(model, epochs, n_users, n_items, interactions, U0, V0, reg, alpha, implicit, solver='cholesky', cg_steps=3):
    """The epoch loop of MatrixFactorization.fit_als: users from V, items from U, L after both.  Leaves the padded fp32 tables on
    the model as a fit does.  solver='cg': each half-step starts from the side's current table, in place."""
    dev = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')   # mf.sparse.default_device
    t_plan = timeit.default_timer()
    if interactions.device != dev:
        interactions = interactions.to(dev)
    r = model.n_components
    if interactions.nnz == 0:   # every row is a row without entries: x = 0 on both sides, L = 0
        ld = _lib.padded_ld(r)
        model.plan_seconds_ = model.fit_seconds_ = timeit.default_timer() - t_plan
        model.loss_history_ = [0.0] * epochs
        return (torch.zeros(n_users, ld, dtype=torch.float32, device=dev)[:, :r],
                torch.zeros(n_items, ld, dtype=torch.float32, device=dev)[:, :r])
    plan = _engine.InteractionPlan(interactions.indices, interactions.values, n_users, n_items, user_chunks=1, csc=True)
    ld = _lib.padded_ld(r)
    U = torch.zeros(n_users, ld, dtype=torch.float32, device=dev)
    V = torch.zeros(n_items, ld, dtype=torch.float32, device=dev)
    U[:, :r] = U0.detach().to(device=dev, dtype=torch.float32)
    V[:, :r] = V0.detach().to(device=dev, dtype=torch.float32)
    Uv, Vv = U[:, :r], V[:, :r]
    w_u, t_u, c0 = entry_terms(plan.val_u, alpha, implicit)
    w_i, t_i, _ = entry_terms(plan.val_i, alpha, implicit)
    n_failed = torch.zeros(1, dtype=torch.int32, device=dev)
    losses = torch.zeros(max(epochs, 1), dtype=torch.float64, device=dev)
    cg = solver == 'cg'
    kw_u = dict(solver=solver, cg_steps=cg_steps, x0=Uv, ids=heavy_first(plan.rowptr_u)) if cg else {}
    kw_i = dict(solver=solver, cg_steps=cg_steps, x0=Vv, ids=heavy_first(plan.rowptr_i)) if cg else {}
    if dev.type == 'cuda':
        torch.cuda.synchronize(dev)
    t0 = timeit.default_timer()
    model.plan_seconds_ = t0 - t_plan
    for epoch in range(epochs):
        half_step(Vv, plan.rowptr_u, plan.col_u, w_u, t_u, reg, implicit, out=Uv, n_failed=n_failed, **kw_u)
        half_step(Uv, plan.rowptr_i, plan.row_i, w_i, t_i, reg, implicit, out=Vv, n_failed=n_failed, **kw_i)
        losses[epoch] = objective(Uv, Vv, plan.user_of, plan.col_u, w_u, t_u, c0, reg, implicit)
        if model.verbose and (epoch + 1) % 25 == 0:
            model._report(epoch, float(losses[epoch]), timeit.default_timer() - t0)
    if dev.type == 'cuda':
        torch.cuda.synchronize(dev)
    model.fit_seconds_ = timeit.default_timer() - t0
    failed = int(n_failed)   # read once, after the last epoch
    if failed:
        raise FloatingPointError(f'fit_als: {failed} row solves met a matrix that was not positive definite (their rows were set to '
                                 f'zero); the tables hold non-finite values or reg is too small for them')
    model.loss_history_ = losses[:epochs].cpu().tolist()
    return Uv, Vv


def fold_in(Y, interactions, reg, alpha, implicit, solver='cholesky', cg_steps=3):
    """The rows of ``interactions`` [n_new, n_other] embedded against the fitted table Y [n_other, r]: fp32 [n_new, r] (solver='cg':
    cg_steps steps from zeros)."""
    n_new, n_other = interactions.shape
    if n_other != Y.shape[0]:
        raise ValueError(f'interactions have {n_other} columns, the fitted table {Y.shape[0]} rows')
    dev = Y.device
    if interactions.nnz == 0:   # rows without entries get x = 0
        return torch.zeros(n_new, Y.shape[1], dtype=torch.float32, device=dev)
    if interactions.device != dev:
        interactions = interactions.to(dev)
    plan = _engine.InteractionPlan(interactions.indices, interactions.values, n_new, n_other, csc=False)
    w, t, _ = entry_terms(plan.val_u, alpha, implicit)
    X, n_failed = half_step(Y.detach().to(torch.float32), plan.rowptr_u, plan.col_u, w, t, reg, implicit, solver=solver,
                            cg_steps=cg_steps, ids=heavy_first(plan.rowptr_u) if solver == 'cg' else None)
    failed = int(n_failed)
    if failed:
        raise FloatingPointError(f'fold-in: {failed} row solves met a matrix that was not positive definite')
    return X
