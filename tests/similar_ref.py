"""fp64 oracle of similar_items / similar_users and of the unit rows behind them (NumPy only): normalise, multiply, stable sort by
(-value, id), drop self."""
import numpy as np


def unit_rows_ref(table, ids=None):
    """(unit rows, norms) of table[ids] in fp64; a zero row stays zero with norm 0.  Rows are scaled by their largest magnitude
    first, so neither 1e30 nor 1e-30 rows leave the fp64 range when squared."""
    T = np.asarray(table, np.float64)
    if ids is not None:
        T = T[np.asarray(ids, np.int64)]
    amax = np.abs(T).max(axis=1, keepdims=True) if T.shape[1] else np.zeros((T.shape[0], 1))
    safe = np.where(amax > 0, amax, 1.0)
    Y = T / safe
    nrm = np.sqrt((Y * Y).sum(axis=1, keepdims=True))
    unit = np.where(amax > 0, Y / np.where(nrm > 0, nrm, 1.0), 0.0)
    return unit, (nrm * amax)[:, 0]


def similarities(table, ids=None, queries=None, metric='cosine'):
    """fp64 [q, n] similarities of the query rows (table[ids], every row for ids=None, or ``queries``) with every row of table."""
    T = np.asarray(table, np.float64)
    Q = np.asarray(queries, np.float64) if queries is not None else T if ids is None else T[np.asarray(ids, np.int64)]
    if metric == 'cosine':
        return unit_rows_ref(Q)[0] @ unit_rows_ref(T)[0].T
    if metric == 'dot':
        return Q @ T.T
    raise ValueError(metric)


def similar_ref(table, k, ids=None, queries=None, metric='cosine', include_self=False):
    """(ids int64 [q, k], values fp64 [q, k], S fp64 [q, n]): per query the k best rows, value descending, ties by ascending id;
    query j never returns ids[j] unless include_self is set or queries are given (S keeps the self entries)."""
    S = similarities(table, ids, queries, metric)
    q, n = S.shape
    R = S.copy()
    if queries is None and not include_self:
        own = np.arange(n) if ids is None else np.asarray(ids, np.int64)
        R[np.arange(q), own] = -np.inf
    order = np.argsort(-R, axis=1, kind='stable')[:, :k]
    return order, np.take_along_axis(S, order, 1), S
