"""Host side of the cloud bank (no GPU): ``get_query_tuple_ids`` makes the draws of ``get_query_tuple`` -- the reference's tuple sampling,
utils/loading_pointclouds.py:102-168 -- as indices into the preloaded array: ``data[ids]`` are that function's arrays and ``random`` is
left in the identical state, so a seeded training run visits the same tuples whether it steps on arrays or on ids."""
import copy
import random

import numpy as np
import pytest

import helpers as H


def _dataset(T, n, seed=0):
    rng = np.random.default_rng(seed)
    data = rng.uniform(-1, 1, (T, n, 3)).astype(np.float32)
    queries = {}
    for i in range(T):
        queries[i] = {"query": "%d.bin" % i, "positives": [j for j in range(T) if j != i and abs(j - i) <= 2],
                      "negatives": [j for j in range(T) if abs(j - i) > 4]}
    return queries, data


def _both(key, queries, data, num_pos, num_neg, seed, **kw):
    LP = H.pkg("utils.loading_pointclouds")
    qa, qb = copy.deepcopy(queries), copy.deepcopy(queries)
    random.seed(seed)
    arrays = LP.get_query_tuple(key, qa[key], num_pos, num_neg, qa, data=data, **kw)
    state_a = random.getstate()
    random.seed(seed)
    ids = LP.get_query_tuple_ids(key, qb[key], num_pos, num_neg, qb, **kw)
    state_b = random.getstate()
    assert state_a == state_b                          # the same shuffles in the same order
    assert qa == qb                                    # ... which leave the query dict shuffled identically
    return arrays, ids


@pytest.mark.parametrize("other_neg", [False, True])
@pytest.mark.parametrize("hard", [[], [30, 12, 25]])
@pytest.mark.parametrize("seed", [0, 1, 7])
def test_ids_are_the_draws_of_get_query_tuple(other_neg, hard, seed):
    queries, data = _dataset(40, 16)
    for key in (0, 7, 20, 39):
        hard_neg = [h for h in hard if h in queries[key]["negatives"]]
        arrays, ids = _both(key, queries, data, 2, 6, seed, hard_neg=hard_neg, other_neg=other_neg)
        assert len(arrays) == len(ids) == (4 if other_neg else 3)
        assert ids[0] == key and np.array_equal(data[ids[0]], arrays[0])
        assert len(ids[1]) == 2 and np.array_equal(data[ids[1]], arrays[1])
        assert len(ids[2]) == 6 and np.array_equal(data[ids[2]], arrays[2])
        assert ids[2][:len(hard_neg)] == hard_neg       # hard negatives first (:121-128)
        if other_neg:
            assert len(ids[3]) == 1 and np.array_equal(data[ids[3][0]], arrays[3])


def test_no_possible_other_negative_is_an_empty_list():
    """Every cloud is a positive of the query or of one of its negatives: get_query_tuple returns an empty array (which the loop
    skips as "NO OTHER NEG", train.py:401), the id form an empty list -- after the same draws."""
    T = 8
    data = np.arange(T * 4 * 3, dtype=np.float32).reshape(T, 4, 3)
    queries = {i: {"query": "%d.bin" % i, "positives": [j for j in range(T) if j != i and (j < 4) == (i < 4)],
                   "negatives": [j for j in range(T) if (j < 4) != (i < 4)]} for i in range(T)}
    for i in range(T):
        queries[i]["positives"].append(i)          # (every key is somebody's positive: nothing is left over)
    arrays, ids = _both(1, queries, data, 2, 3, 3, other_neg=True)
    assert arrays[3].shape == (0,) and ids[3] == []
    assert np.array_equal(data[ids[1]], arrays[1]) and np.array_equal(data[ids[2]], arrays[2])


def test_bank_operators_refuse_cpu_tensors():
    """Like every operator of the package: no CPU fallback."""
    ops, L = H.pkg("ops"), H.pkg("lib")
    with pytest.raises(L.EpcNetError):
        ops.CloudBank(256, 4, "cpu")
