"""The numpy restatement of the tuple draw (tests/tuples_ref.py) against the package's own host rule, and the evenness of the fixed hash
of include/epcnet_poses.h.  No GPU: the relations are derived here by brute force, the twin of what ``query_dict_from_poses`` builds from the
device's radius lists (tests/test_gpu_pose_tuples.py holds that function to the same twin)."""
import random

import numpy as np
import pytest

import helpers as H
import tuples_ref as R

R_POS, R_NEG = 10.0, 50.0


def test_fixture_has_the_edges_and_collapses_in_float32():
    p = R.fixture_poses(300)
    dist = lambda a, b: float(np.sqrt(R.d2(p, p[a])[b]))
    assert [dist(0, 1), dist(2, 3), dist(4, 5), dist(6, 7)] == [10.0, 25.0, 50.0, 10.125]
    assert R.positives_mask(p, 0, 10.0)[1] and not R.positives_mask(p, 6, 10.0)[7]            # 10.0 is inside, 10.125 is not
    assert not R.negatives_mask(p, 4, 50.0)[5] and R.radius_lists(p[2:3], p, 25.0)[0].tolist() == [2, 3]   # 50.0 is no negative; 25.0 is truth
    assert (p[8] == p[9]).all() and (p[9] == p[10]).all() and R.pos_count(p, 10.0)[8:12].tolist() == [3, 3, 3, 3]
    assert R.pos_count(p, 10.0)[12:32].min() == 19                                           # the cluster: everybody's positive
    assert np.abs(p - [5735000.0, 620000.0]).max() < 4000 and (np.round((p - [5735000.0, 620000.0]) * 8) == (p - [5735000.0, 620000.0]) * 8).all()
    p32 = p.astype(np.float32).astype(np.float64)                                            # a float32 shortcut moves the relations
    assert (np.round(p32[:, 0] * 2) == p32[:, 0] * 2).all()          # (float32 northings: a 0.5 m lattice)
    assert (R.pos_count(p32, 10.0) != R.pos_count(p, 10.0)).any()


def test_sets_equal_the_host_rule():
    """Positives, negatives and eligible other negatives of tuples_ref are the sets ``get_query_tuple_ids`` draws from: set equality
    with the dict's lists and with the function's own ``set(QUERY_DICT.keys()) - set(neighbors)`` for the negatives IT chose, and
    membership of everything it returns -- 50 keys at T = 300."""
    LP = H.pkg("utils.loading_pointclouds")
    T, P, Nn = 300, 2, 14
    poses = R.fixture_poses(T)
    queries = R.brute_force_dict(poses, R_POS, R_NEG)
    random.seed(1)
    keys = [0, 1, 6, 8, 12, 31] + list(np.random.RandomState(0).permutation(np.arange(32, T))[:44])
    assert len(keys) == 50
    drawn_other = 0
    for key in keys:
        key = int(key)
        pos_mask, neg_mask = R.positives_mask(poses, key, R_POS), R.negatives_mask(poses, key, R_NEG)
        assert set(np.nonzero(pos_mask)[0]) == set(queries[key]["positives"])
        assert set(np.nonzero(neg_mask)[0]) == set(queries[key]["negatives"])
        if len(queries[key]["positives"]) < P:
            continue
        _, pos, neg, other = LP.get_query_tuple_ids(key, queries[key], P, Nn, queries, hard_neg=[], other_neg=True)
        assert all(pos_mask[c] for c in pos) and all(neg_mask[c] for c in neg)
        neighbors = list(queries[key]["positives"])
        for n in neg:
            neighbors.extend(queries[n]["positives"])
        eligible = R.eligible_other_mask(poses, key, neg, R_POS)
        assert set(np.nonzero(eligible)[0]) == set(queries.keys()) - set(neighbors)
        assert eligible[key]             # the reference's quirk: nobody is his own positive, so the key itself stays eligible
        assert len(other) == 1 and eligible[other[0]]
        drawn_other += 1
    assert drawn_other >= 40


def test_ref_sample_obeys_its_own_rules():
    """tuples_ref.sample on the fixture: slots, statuses and the hard-negative rule (order kept, -1 and repeats dropped)."""
    poses = R.fixture_poses(300)
    ids, status = R.sample(poses, [40, 0, -1, 300], R_POS, R_NEG, seed=3, step=7, P=2, Nn=6, hard=[[200, -1, 200, 150]] + [[-1] * 4] * 3)
    assert status.tolist() == [0, R.FEW_POSITIVES, R.BAD_KEY, R.BAD_KEY] and (ids[2:] == -1).all()
    assert ids[0, 0] == 40 and ids[0, 3:5].tolist() == [200, 150] and len(set(ids[0].tolist())) >= 9
    assert ids[1, 1] == 1 and ids[1, 2] == -1
    cand, st = R.candidates(poses, [40, -1], R_NEG, seed=3, step=7, C=64)
    assert st.tolist() == [0, R.BAD_KEY] and len(cand[0]) == 64 and (np.diff(cand[0]) > 0).all() and len(cand[1]) == 0
    assert R.negatives_mask(poses, 40, R_NEG)[cand[0]].all()


def test_the_fixed_hash_draws_evenly():
    """5-sigma bands of a fair draw (binomial: n p +- 5 sqrt(n p (1 - p))).  P = 2 of 8 positives over 4096 consecutive steps: every
    positive 1024 +- 139.  One other negative of 20 000 records over the same steps, in 16 id ranges: 256 +- 78 per range."""
    steps = np.arange(4096)
    key, seed = 1234, 0
    ids = np.array([1229, 1230, 1231, 1232, 1233, 1235, 1236, 1237], dtype=np.uint64)
    st = R.state(seed, steps, key, R.STREAM_POSITIVES)
    v = (R.mix(st[:, None] ^ ids[None, :]) << np.uint64(32)) | ids[None, :]
    picked = np.argsort(v, axis=1)[:, :2]
    counts = np.bincount(picked.reshape(-1), minlength=8)
    print("positives picked:", counts.tolist(), "worst deviation", int(np.abs(counts - 1024).max()))
    assert counts.sum() == 8192 and np.abs(counts - 1024).max() <= 139
    all_ids = np.arange(20000, dtype=np.uint64)
    bins = np.zeros(16, dtype=np.int64)
    st = R.state(seed, steps, key, R.STREAM_OTHER)
    for a in range(0, 4096, 128):
        v = (R.mix(st[a:a + 128, None] ^ all_ids[None, :]) << np.uint64(32)) | all_ids[None, :]
        bins += np.bincount(v.argmin(1) * 16 // 20000, minlength=16)
    print("other negative per id range:", bins.tolist(), "worst deviation", int(np.abs(bins - 256).max()))
    assert bins.sum() == 4096 and np.abs(bins - 256).max() <= 78


def test_second_header_is_bound_like_the_first():
    """include/epcnet_poses.h: its five entries are read by the same header reader, exported by the library, typed and callable through
    lib.run, and kept out of lib.EXPORTS / lib.LAUNCHING (what include/epcnet.h declares)."""
    import ctypes
    import os
    L = H.pkg("lib")
    text = open(os.path.join(H.ROOT, "include", "epcnet_poses.h")).read()
    functions, constants, status = L.parse_header(text, need_status=False)
    assert list(functions) == L.POSE_EXPORTS == ["epcnet_pose_radius_count", "epcnet_pose_radius_fill", "epcnet_pose_pos_count",
                                                 "epcnet_tuple_candidates", "epcnet_tuple_sample"] and status == {}
    assert not set(L.POSE_EXPORTS) & set(L.EXPORTS) and not set(L.POSE_EXPORTS) & set(L.LAUNCHING)
    assert constants["EPC_TUPLE_BAD_KEY"] == L.EPC_TUPLE_BAD_KEY == R.BAD_KEY and L.EPC_TUPLE_NO_OTHER == R.NO_OTHER
    assert (L.EPC_TUPLE_STREAM_POSITIVES, L.EPC_TUPLE_STREAM_CANDIDATES, L.EPC_TUPLE_STREAM_NEGATIVES, L.EPC_TUPLE_STREAM_OTHER) == (0, 1, 2, 3)
    for name, (ret, types, names) in functions.items():
        fn = getattr(L.lib(), name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(types) and names[-1] == "stream" and hasattr(L.run, name)
    seed_at = functions["epcnet_tuple_sample"][2].index("seed")
    assert L.lib().epcnet_tuple_sample.argtypes[seed_at] is ctypes.c_longlong
    # a refusal reaches the caller before anything is launched: no device is needed for it
    with pytest.raises(L.EpcNetError) as e:
        L.run.epcnet_pose_pos_count(None, 0, None, None, stream=0)
    assert e.value.status == L.EPC_EINVAL and "epcnet_pose_pos_count" in str(e.value)
