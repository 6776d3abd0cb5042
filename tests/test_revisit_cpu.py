"""The definition of include/epcnet_revisits.h as tests/revisit_ref.py restates it, without a device: causality, plateaus, the query's own
row at min_travel 0, the rows without an answer and the whole-call failures on well-separated data with a float64 brute-force search; the
sixth header's binding; and the entry's refusals, which launch nothing."""
import ctypes
import os

import numpy as np
import pytest
import torch

import helpers as H
import revisit_ref as R


def _well_separated(rows, dim=8):
    """Row i is e_(i % dim) * (1 + i): every pairwise distance differs from every other by far more than float32 resolves."""
    x = np.zeros((rows, dim), np.float32)
    x[np.arange(rows), np.arange(rows) % dim] = 1.0 + np.arange(rows)
    return x


def test_reference_is_causal_for_a_positive_min_travel():
    T, k = 40, 5
    db, along = _well_separated(T), np.arange(T) * 10.0
    dist, idx, count = R.revisit_reference(R.brute_search, db, along, db, along, 25.0, k)
    assert count.tolist() == [max(i - 2, 0) for i in range(T)]                 # along <= 10 i - 25: rows 0 .. i - 3
    for i in range(T):
        got = idx[i][idx[i] >= 0]
        assert (got < count[i]).all() and (got < i).all() and len(got) == min(k, count[i])
        assert np.isinf(dist[i, len(got):]).all() and (np.diff(dist[i, :len(got)]) >= 0).all()
        want = np.argsort(np.linalg.norm(db[:count[i]].astype(np.float64) - db[i], axis=1), kind="stable")[:k]
        assert got.tolist() == want.tolist()
    # every pair (i, j) is reported at most once, by its later member
    pairs = {(i, int(j)) for i in range(T) for j in idx[i] if j >= 0}
    assert not {(j, i) for i, j in pairs} & pairs


def test_reference_plateaus_move_the_prefix_by_the_run_length():
    along = np.array([0.0, 10.0, 10.0, 10.0, 10.0, 10.0, 20.0, 30.0, 30.0, 40.0])
    assert R.prefix_counts(along, along, 0.0).tolist() == [1, 6, 6, 6, 6, 6, 7, 9, 9, 10]
    assert R.prefix_counts(along, along, 10.0).tolist() == [0, 1, 1, 1, 1, 1, 6, 7, 7, 9]
    assert R.prefix_counts(along, along, 1e9).tolist() == [0] * 10
    db = _well_separated(10)
    _, idx, count = R.revisit_reference(R.brute_search, db, along, db, along, 10.0, 3)
    assert count.tolist() == [0, 1, 1, 1, 1, 1, 6, 7, 7, 9] and idx[0].tolist() == [-1] * 3 and idx[1].tolist() == [0, -1, -1]


def test_reference_min_travel_zero_admits_the_query_itself():
    T = 12
    db, along = _well_separated(T), np.arange(T) * 10.0
    dist, idx, count = R.revisit_reference(R.brute_search, db, along, db, along, 0.0, 2)
    assert count.tolist() == list(range(1, T + 1)) and idx[:, 0].tolist() == list(range(T)) and (dist[:, 0] == 0).all()
    # the subtraction is ONE float64 operation: 0.3 - 0.1 rounds below 0.2 + 2^-55, so a row at exactly fl(0.3 - 0.1) is admitted
    edge = np.float64(0.3) - np.float64(0.1)
    assert R.prefix_counts([edge], [0.3], 0.1).tolist() == [1] and R.prefix_counts([np.nextafter(edge, 1.0)], [0.3], 0.1).tolist() == [0]


def test_reference_rows_without_an_answer_and_whole_call_failures():
    T = 9
    db, along = _well_separated(T), np.arange(T) * 10.0
    q_along = np.array([np.nan, 35.0, np.inf, -np.inf, -5.0])
    dist, idx, count = R.revisit_reference(R.brute_search, db, along, db[:5], q_along, 0.0, 4)
    assert count.tolist() == [-1, 4, -1, -1, 0]
    assert (idx[[0, 2, 3, 4]] == -1).all() and np.isinf(dist[[0, 2, 3, 4]]).all() and (idx[1] >= 0).all()
    for bad in (np.r_[along[:-1], along[-2] - 1.0], np.r_[along[:4], np.nan, along[5:]], np.r_[along[:4], np.inf, along[5:]]):
        assert R.failed(bad)
        dist, idx, count = R.revisit_reference(R.brute_search, db, bad, db, along, 0.0, 4)
        assert (count == -1).all() and (idx == -1).all() and np.isinf(dist).all() and dist.dtype == np.float32
    assert not R.failed(along) and not R.failed(np.zeros(5)) and not R.failed(np.zeros(0))
    # a non-finite descriptor is never selected and selects nothing
    hurt = db.copy()
    hurt[2, 3] = np.nan
    _, idx, count = R.revisit_reference(R.brute_search, hurt, along, hurt, along, 0.0, 9)
    assert (idx[2] == -1).all() and not (idx == 2).any() and count.tolist() == list(range(1, T + 1))


def test_sixth_header_is_bound_like_the_others():
    L = H.pkg("lib")
    text = open(os.path.join(H.ROOT, "include", "epcnet_revisits.h")).read()
    assert L.REVISITS_HEADER_PATH == os.path.join(H.ROOT, "include", "epcnet_revisits.h")
    functions, constants, status = L.parse_header(text, need_status=False, scalars=L._REVISIT_SCALARS)
    assert list(functions) == L.REVISIT_EXPORTS == ["epcnet_revisit_workspace_bytes", "epcnet_revisit_search"]
    assert status == {} and constants == {}                                   # no new status constant: count == -1 is the flag
    with pytest.raises(ValueError):                                           # a `double` by value is this header's alone
        L.parse_header(text, need_status=False)
    for other in (L.EXPORTS, L.POSE_EXPORTS, L.SCAN_EXPORTS, L.SUBMAP_EXPORTS, L.STAMP_EXPORTS, L.LAUNCHING):
        assert not set(L.REVISIT_EXPORTS) & set(other)
    for name in L.REVISIT_EXPORTS:
        assert hasattr(L.lib(), name)
    size, search = L.lib().epcnet_revisit_workspace_bytes, L.lib().epcnet_revisit_search
    assert size.restype is ctypes.c_size_t and size.argtypes == [ctypes.c_int] * 3
    ret, types, names = functions["epcnet_revisit_search"]
    assert names == ["database", "db_along", "num_db", "queries", "q_along", "num_q", "dim", "min_travel", "k", "pass_queries", "idx", "dist",
                     "count", "workspace", "workspace_bytes", "stream"]
    assert ret == "int" and (types[-1], names[-1]) == ("void*", "stream") and search.restype is ctypes.c_int
    assert types[names.index("db_along")] == types[names.index("q_along")] == "double*" and types[names.index("min_travel")] == "double"
    assert types[names.index("database")] == types[names.index("dist")] == "float*" and types[names.index("count")] == "int32_t*"
    P, i = ctypes.c_void_p, ctypes.c_int
    assert search.argtypes == [P, P, i, P, P, i, i, ctypes.c_double, i, i, P, P, P, P, ctypes.c_size_t, P]
    assert hasattr(L.run, "epcnet_revisit_search") and not hasattr(L.run, "epcnet_revisit_workspace_bytes")
    assert L._POINTEES["double*"] is torch.float64
    # the checked call form refuses a float32 `along` before the library is reached, and takes a Python float for the double

    class Fake:
        def __init__(self, dtype):
            self.dtype, self.is_cuda = dtype, True

        def data_ptr(self):
            return 0x10000

    f32, f64, i32 = Fake(torch.float32), Fake(torch.float64), Fake(torch.int32)
    with pytest.raises(L.EpcNetError) as e:
        L.run.epcnet_revisit_search(f32, f32, 4, f32, f64, 4, 8, 1.0, 1, 0, i32, f32, i32, None, 0, stream=0)
    assert "argument 2" in str(e.value) and "db_along" in str(e.value) and "torch.float64" in str(e.value)
    with pytest.raises(L.EpcNetError) as e:                                   # everything typed right: the library refuses the null workspace
        L.run.epcnet_revisit_search(f32, f64, 4, f32, f64, 4, 8, 1, 1, 0, i32, f32, i32, None, 0, stream=0)
    assert e.value.status == L.EPC_EINVAL and "epcnet_revisit_search: null pointer" in str(e.value)


def test_size_query_answers_zero_for_what_the_entry_refuses():
    size = H.pkg("lib").lib().epcnet_revisit_workspace_bytes
    top = 1 << 22
    for good in ((300, 300, 0), (300, 300, 128), (0, 5, 0), (5, 0, 0), (0, 0, 0), (top, 1, 0), (1, top, top), (1000, 1000, 256)):
        assert size(*good) > 0 and size(*good) % 16 == 0, good
    for bad in ((-1, 5, 0), (5, -1, 0), (top + 1, 5, 0), (5, top + 1, 0), (5, 5, -128), (5, 5, 64), (5, 5, 129), (5, 5, 200), (5, 5, top + 128)):
        assert size(*bad) == 0, bad
    # the matrix of a pass: pass_queries rows of num_db floats, never more rows than queries
    assert size(1000, 300, 128) >= 128 * 1000 * 4 and size(1000, 300, 128) < 200 * 1000 * 4 <= size(1000, 300, 0)
    assert size(1000, 100, 128) < 128 * 1000 * 4
    assert size(top, top, 0) < (1 << 31) + (1 << 27)                          # 128 rows of 2^22 floats and the per-row words


def test_refusals_launch_nothing():
    """Every EPC_EINVAL and the EPC_ENOMEM are decided on the host before anything touches a device: the pointers here are made-up
    addresses that are never followed."""
    L = H.pkg("lib")
    lib = L.lib()
    A = 0x10000                                              # 16-byte aligned
    need = lib.epcnet_revisit_workspace_bytes(300, 200, 0)
    good = dict(database=A, db_along=2 * A, num_db=300, queries=3 * A, q_along=4 * A, num_q=200, dim=256, min_travel=100.0, k=5, pass_queries=0,
                idx=5 * A, dist=6 * A, count=7 * A, workspace=8 * A, workspace_bytes=need)
    order = list(good)
    top = 1 << 22
    bad = [dict(database=None), dict(db_along=None), dict(queries=None), dict(q_along=None), dict(idx=None), dict(dist=None), dict(count=None),
           dict(workspace=None), dict(database=A + 4), dict(queries=3 * A + 8), dict(workspace=8 * A + 8), dict(dim=0), dict(dim=-8), dict(dim=4),
           dict(dim=12), dict(k=0), dict(k=-1), dict(k=57), dict(num_db=-1), dict(num_db=top + 1), dict(num_q=-1), dict(num_q=top + 1),
           dict(pass_queries=-128), dict(pass_queries=64), dict(pass_queries=129), dict(pass_queries=top + 128), dict(min_travel=-1.0),
           dict(min_travel=float("nan")), dict(min_travel=float("inf")), dict(min_travel=-0.5)]
    for change in bad:
        a = dict(good, **change)
        assert lib.epcnet_revisit_search(*[a[k] for k in order], None) == L.EPC_EINVAL, change
        assert b"epcnet_revisit_search" in lib.epc_last_error()
    assert lib.epcnet_revisit_search(*[dict(good, workspace_bytes=need - 1)[k] for k in order], None) == L.EPC_ENOMEM
    assert lib.epcnet_revisit_search(*[dict(good, pass_queries=128, workspace_bytes=lib.epcnet_revisit_workspace_bytes(300, 200, 128) - 1)[k]
                                       for k in order], None) == L.EPC_ENOMEM
    assert lib.epcnet_revisit_search(*[dict(good, num_q=0)[k] for k in order], None) == L.EPC_OK          # no query: nothing to launch
    assert lib.epcnet_revisit_search(*[dict(good, num_q=0, workspace_bytes=0)[k] for k in order], None) == L.EPC_OK


def test_python_entry_refuses_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L, RT = H.pkg("lib"), H.pkg("retrieval")
    with pytest.raises(L.EpcNetError):
        RT.revisit_search(torch.zeros(4, 8), torch.zeros(4, dtype=torch.float64), 1.0)
    with pytest.raises(L.EpcNetError):
        RT.RevisitIndex(16, dim=8, min_travel=1.0)
