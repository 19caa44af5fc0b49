"""NumPy oracle of alternating least squares (teamoflow_amd/_als.py states the formulas), fp64 by default.

One row with stored entries k (column j_k, weight w_k, target t_k) against the other side's table Y:
    A x = b,  A = G0 + reg I + sum_k w_k y_k y_k^T,  b = sum_k t_k y_k
implicit: G0 = Y^T Y, w = alpha |a|, t = (1 + w) [a > 0];  explicit: no G0, w = 1, t = a.  A row without entries gets x = 0.
dtype=np.float32 runs the same statements in fp32 (how far plain fp32 arithmetic is from fp64 on a case)."""
import numpy as np


def entry_terms_ref(a, alpha, implicit, dtype=np.float64):
    a = np.asarray(a, dtype=dtype)
    if implicit:
        w = (dtype(alpha) * np.abs(a)).astype(dtype)
        t = ((1 + w) * (a > 0)).astype(dtype)
        return w, t, t
    return np.ones_like(a), a, (a * a).astype(dtype)


def csr_ref(rows, cols, vals, n_rows):
    """Entries sorted by row (stable: a row keeps the order its entries came in) -> (rowptr int64, cols, vals)."""
    rows = np.asarray(rows, dtype=np.int64)
    order = np.argsort(rows, kind='stable')
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_rows))]).astype(np.int64)
    return rowptr, np.asarray(cols)[order], np.asarray(vals)[order]


def solve_rows_ref(Y, G0, rowptr, col, w, t, reg, dtype=np.float64):
    """Every row of the CSR solved against Y -> X [n_rows, r] in ``dtype``.  A matrix that is not positive definite gives zeros."""
    Y = np.asarray(Y, dtype=dtype)
    w, t = np.asarray(w, dtype=dtype), np.asarray(t, dtype=dtype)
    r = Y.shape[1]
    n_rows = len(rowptr) - 1
    base = dtype(reg) * np.eye(r, dtype=dtype)
    if G0 is not None:
        base = (np.asarray(G0, dtype=dtype) + base).astype(dtype)
    X = np.zeros((n_rows, r), dtype=dtype)
    for i in range(n_rows):
        e = slice(int(rowptr[i]), int(rowptr[i + 1]))
        if e.stop <= e.start:
            continue
        Yg = Y[np.asarray(col[e], dtype=np.int64)]
        A = (base + (Yg * w[e, None]).T @ Yg).astype(dtype)
        b = (Yg.T @ t[e]).astype(dtype)
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            continue
        z = np.linalg.solve(L, b)
        X[i] = np.linalg.solve(L.T.copy(), z)
    return X


def objective_ref(U, V, indices, values, reg, alpha, implicit):
    """L = <U^T U, V^T V> [implicit] + sum_k (w s^2 - 2 t s + c0) + reg (||U||^2 + ||V||^2), fp64."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    indices = np.asarray(indices, dtype=np.int64).reshape(-1, 2)
    w, t, c0 = entry_terms_ref(values, alpha, implicit)
    s = (U[indices[:, 0]] * V[indices[:, 1]]).sum(1)
    L = float((w * s * s - 2 * t * s + c0).sum()) + reg * (float((U * U).sum()) + float((V * V).sum()))
    if implicit:
        L += float(((U.T @ U) * (V.T @ V)).sum())
    return L


def half_step_ref(Y, rows, cols, vals, n_rows, reg, alpha, implicit, dtype=np.float64):
    """The table of the ``rows`` side from Y, the table of the ``cols`` side."""
    rowptr, c, a = csr_ref(rows, cols, vals, n_rows)
    w, t, _ = entry_terms_ref(a, alpha, implicit, dtype)
    Yd = np.asarray(Y, dtype=dtype)
    return solve_rows_ref(Yd, (Yd.T @ Yd).astype(dtype) if implicit else None, rowptr, c, w, t, reg, dtype)


def als_ref(U0, V0, indices, values, epochs, reg, alpha, implicit, dtype=np.float64):
    """``epochs`` sweeps from (U0, V0) -> dict(U=[after every user half-step], V=[after every item half-step], loss=[L after every
    epoch, fp64]).  U0 only gives the number of users: the first half-step replaces it."""
    indices = np.asarray(indices, dtype=np.int64).reshape(-1, 2)
    values = np.asarray(values)
    m, n = np.asarray(U0).shape[0], np.asarray(V0).shape[0]
    V = np.asarray(V0, dtype=dtype)
    out = dict(U=[], V=[], loss=[])
    for _ in range(epochs):
        U = half_step_ref(V, indices[:, 0], indices[:, 1], values, m, reg, alpha, implicit, dtype)
        V = half_step_ref(U, indices[:, 1], indices[:, 0], values, n, reg, alpha, implicit, dtype)
        out['U'].append(U)
        out['V'].append(V)
        out['loss'].append(objective_ref(U, V, indices, values, reg, alpha, implicit))
    out['loss'] = np.array(out['loss'])
    return out


def grad_u_ref(U, V, indices, values, reg, alpha, implicit):
    """(dL/dU, the scale it is measured against: the largest |2 b| element), fp64."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    indices = np.asarray(indices, dtype=np.int64).reshape(-1, 2)
    w, t, _ = entry_terms_ref(values, alpha, implicit)
    s = (U[indices[:, 0]] * V[indices[:, 1]]).sum(1)
    g = 2 * reg * U
    if implicit:
        g = g + 2 * U @ (V.T @ V)
    np.add.at(g, indices[:, 0], 2 * (w * s - t)[:, None] * V[indices[:, 1]])
    b2 = np.zeros_like(U)
    np.add.at(b2, indices[:, 0], 2 * t[:, None] * V[indices[:, 1]])
    return g, float(np.abs(b2).max())
