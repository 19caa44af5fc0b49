"""NumPy oracle of the conjugate-gradient form of alternating least squares (teamoflow_amd/_als.py states the iteration), fp64 by
default; dtype=np.float32 runs the same statements in fp32, as als_ref.py does.

One row with stored entries k (column j_k, weight w_k, target t_k) against Y, never forming A:
    A v = G0 v + reg v + sum_k w_k (y_k . v) y_k,   b = sum_k t_k y_k
    x = x0, res = b - A x, p = res, rs = res . res, stop = max(1e-14 b . b, 1e-30); cg_steps times: finished if rs <= stop;
    Ap = A p, pAp = p . Ap (not a positive finite number: the row fails, x = 0); a = rs / pAp; x += a p; res -= a Ap;
    rs' = res . res; p = res + (rs' / rs) p; rs = rs'.
A row without entries gets x = 0 whatever x0 was."""
import numpy as np

from als_ref import csr_ref, entry_terms_ref, objective_ref


def cg_rows_ref(Y, G0, rowptr, col, w, t, reg, X0, cg_steps, dtype=np.float64):
    """Every row of the CSR by cg_steps steps from X0 (None: zeros) -> X [n_rows, r] in ``dtype``; a failed row is zeros."""
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
        Yg, wk = Y[np.asarray(col[e], dtype=np.int64)], w[e]

        def apply(v):
            return (base @ v + Yg.T @ (wk * (Yg @ v))).astype(dtype)

        b = (Yg.T @ t[e]).astype(dtype)
        x = np.zeros(r, dtype=dtype) if X0 is None else np.asarray(X0[i], dtype=dtype).copy()
        res = (b - apply(x)).astype(dtype)
        p = res.copy()
        rs = dtype(res @ res)
        stop = max(dtype(1e-14) * dtype(b @ b), dtype(1e-30))
        for _ in range(int(cg_steps)):
            if rs <= stop:
                break
            Ap = apply(p)
            pAp = dtype(p @ Ap)
            if not (pAp > 0 and np.isfinite(pAp)):
                x = np.zeros(r, dtype=dtype)
                break
            a = dtype(rs / pAp)
            x = (x + a * p).astype(dtype)
            res = (res - a * Ap).astype(dtype)
            rs_new = dtype(res @ res)
            p = (res + dtype(rs_new / rs) * p).astype(dtype)
            rs = rs_new
        X[i] = x
    return X


def cg_half_step_ref(Y, X0, rows, cols, vals, n_rows, reg, alpha, implicit, cg_steps, dtype=np.float64):
    """The table of the ``rows`` side from Y, the table of the ``cols`` side, starting from X0."""
    rowptr, c, a = csr_ref(rows, cols, vals, n_rows)
    w, t, _ = entry_terms_ref(a, alpha, implicit, dtype)
    Yd = np.asarray(Y, dtype=dtype)
    return cg_rows_ref(Yd, (Yd.T @ Yd).astype(dtype) if implicit else None, rowptr, c, w, t, reg, X0, cg_steps, dtype)


def als_cg_ref(U0, V0, indices, values, epochs, reg, alpha, implicit, cg_steps, dtype=np.float64):
    """``epochs`` sweeps from (U0, V0), every half-step from the side's current table -> what als_ref returns: dict(U=[after every
    user half-step], V=[after every item half-step], loss=[L after every epoch, fp64])."""
    indices = np.asarray(indices, dtype=np.int64).reshape(-1, 2)
    values = np.asarray(values)
    U, V = np.asarray(U0, dtype=dtype), np.asarray(V0, dtype=dtype)
    m, n = U.shape[0], V.shape[0]
    out = dict(U=[], V=[], loss=[])
    for _ in range(epochs):
        U = cg_half_step_ref(V, U, indices[:, 0], indices[:, 1], values, m, reg, alpha, implicit, cg_steps, dtype)
        V = cg_half_step_ref(U, V, indices[:, 1], indices[:, 0], values, n, reg, alpha, implicit, cg_steps, dtype)
        out['U'].append(U)
        out['V'].append(V)
        out['loss'].append(objective_ref(U, V, indices, values, reg, alpha, implicit))
    out['loss'] = np.array(out['loss'])
    return out
