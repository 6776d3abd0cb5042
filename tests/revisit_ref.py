"""The definition of include/epcnet_revisits.h in numpy: the admissible prefix of every query and the answer assembled from ANY exact
k-nearest search ``search(database, queries, k) -> (dist (Q, k), idx (Q, k))`` called once per distinct prefix on ``database[:p]`` --
never from the entry under test.  The CPU tests pass ``brute_search`` (float64, well-separated data); the GPU tests pass the package's
``knn_search`` and compare bit patterns."""
import numpy as np


def prefix_counts(db_along, q_along, min_travel):
    """p_i = #{j : db_along[j] <= q_along[i] - min_travel}: one float64 subtraction, a float64 comparison."""
    db_along, q_along = np.asarray(db_along, np.float64), np.asarray(q_along, np.float64)
    return np.searchsorted(db_along, q_along - np.float64(min_travel), side="right").astype(np.int32)


def failed(db_along):
    """The whole-call failure: a non-finite entry, or a decrease anywhere."""
    db_along = np.asarray(db_along, np.float64)
    return bool((~np.isfinite(db_along)).any() or (np.diff(db_along) < 0).any())


def revisit_reference(search, database, db_along, queries, q_along, min_travel, k):
    """``(dist (Q, k) float32, idx (Q, k) int32, count (Q,) int32)``.  ``database`` and ``queries`` are only sliced (``database[:p]``) and
    indexed by an integer array (``queries[rows]``) and handed to ``search``, so they may live wherever ``search`` wants them."""
    q_along = np.asarray(q_along, np.float64)
    nq = len(q_along)
    dist = np.full((nq, k), np.inf, np.float32)
    idx = np.full((nq, k), -1, np.int32)
    count = np.full(nq, -1, np.int32)
    if failed(db_along):
        return dist, idx, count
    ok = np.isfinite(q_along)
    count[ok] = prefix_counts(db_along, q_along[ok], min_travel)
    for p in np.unique(count[count > 0]).tolist():
        rows = np.nonzero(count == p)[0]
        kk = min(k, p)
        d, i = search(database[:p], queries[rows], kk)
        dist[rows, :kk] = np.asarray(d, np.float32).reshape(len(rows), kk)
        idx[rows, :kk] = np.asarray(i, np.int32).reshape(len(rows), kk)
    return dist, idx, count


def brute_search(database, queries, k):
    """Exact k nearest in float64, ties to the lower index; a non-finite distance is never selected: (-1, +inf) in its place."""
    database, queries = np.asarray(database, np.float64), np.asarray(queries, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = ((queries[:, None, :] - database[None, :, :]) ** 2).sum(-1)
    d2 = np.where(np.isfinite(d2), d2, np.inf)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    d = np.take_along_axis(d2, order, axis=1)
    return np.sqrt(d).astype(np.float32), np.where(np.isfinite(d), order, -1).astype(np.int32)


def unit_rows(seed, rows, dim):
    """Seeded normal rows scaled to unit norm, float32."""
    x = np.random.default_rng([seed, rows, dim]).normal(size=(rows, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
