"""tests/sort_ref.py without a GPU: the Hilbert index against the curve's defining properties, the quantisation on the lattice clouds
(where the cells are known integers), the expected permutation against Python's sorted() over (index, j) tuples, and the occupancies
the GPU file's narrow-form cases are named after."""
import itertools

import numpy as np
import pytest

import sort_ref as S
from helpers import O


@pytest.mark.parametrize("bits", [1, 2, 3, 4])
def test_hilbert_index_is_a_face_adjacent_walk_of_the_cube(bits):
    side = 1 << bits
    cells = np.array(list(itertools.product(range(side), repeat=3)), dtype=np.int64)
    code = S.hilbert_index(cells, bits).astype(np.int64)
    assert np.array_equal(np.sort(code), np.arange(side ** 3))                     # a bijection onto 0 .. 8**bits - 1
    walk = cells[np.argsort(code)]
    assert np.array_equal(walk[0], [0, 0, 0])
    assert np.array_equal(np.abs(np.diff(walk, axis=0)).sum(1), np.ones(side ** 3 - 1, dtype=np.int64))   # one axis, one step


@pytest.mark.parametrize("b", [4, 7])
def test_hilbert_index_of_a_prefix_is_the_prefix_of_the_index(b):
    """What the kernel's 32-bit keys rely on (hilbert_index<7> of cells >> 3) and what makes a bucket a function of cells >> 6."""
    cells = np.random.RandomState(b).randint(0, 1024, size=(5000, 3))
    full = S.hilbert_index(cells, 10)
    assert np.array_equal(full >> np.uint64(3 * (10 - b)), S.hilbert_index(cells >> (10 - b), b))


def _specs():
    for n in S.ALL_SIZES:
        if n >= 2:
            yield "lattice-%d" % n, n, S.lattice_spec(n), None
    for n in S.WAVE_SIZES:
        yield "wave-%d" % n, n, S.wave_spec(n), None
    for n in S.OCCUPANCY_SIZES:
        for name, (m, _) in S.OCCUPANCY_CASES.items():
            yield "%s-%d" % (name, n), n, S.occupancy_spec(n, name), [m]
        yield "mixed-%d" % n, n, S.mixed_spec(n), [64, 65, 64]


@pytest.mark.parametrize("name,n,spec,occupancy", list(_specs()), ids=[s[0] for s in _specs()])
def test_lattice_clouds_quantise_to_their_cells(name, n, spec, occupancy):
    """Every lattice cloud of tests/test_gpu_sort_forms.py: the float32 quantisation returns the chosen integer cells, so the expected
    order is the integers' own; the occupancy cases hold what their names say; every other narrow cloud stays in the bucket sort."""
    clouds = S.clouds_of(spec)
    assert clouds.shape == (len(spec), n, 3) and clouds.dtype == np.float32
    for i, ((cells, _), cloud) in enumerate(zip(spec, clouds)):
        assert np.array_equal(S.cells_of(cloud), cells)
        key = S.hilbert_index(cells, 10)
        if S.NARROW_FROM <= n <= S.NARROW_TO:
            key = key >> np.uint64(10)
        assert np.array_equal(S.expected_perm(cloud), np.argsort(key, kind="stable"))
        if occupancy is not None:
            assert S.bucket_occupancy(cloud) == occupancy[i]
        elif S.NARROW_FROM <= n <= S.NARROW_TO:
            assert S.bucket_occupancy(cloud) <= S.BUCKET_MAX


def test_the_boundary_cases_straddle_the_kernels_limit():
    """The GPU file's '64' case is the fullest cloud the bucket sort keeps and its '65' case the emptiest one it gives up on."""
    assert S.OCCUPANCY_CASES["occ64"][0] == S.BUCKET_MAX == 64 and S.OCCUPANCY_CASES["occ65"][0] == S.BUCKET_MAX + 1 == 65
    for n in S.OCCUPANCY_SIZES:
        assert S.bucket_occupancy(S.clouds_of(S.occupancy_spec(n, "occ64"))[0]) == 64
        assert S.bucket_occupancy(S.clouds_of(S.occupancy_spec(n, "occ65"))[0]) == 65
        assert [S.bucket_occupancy(c) for c in S.clouds_of(S.mixed_spec(n))] == [64, 65, 64]


def test_the_clumped_float_clouds_leave_the_bucket_sort():
    """repeat30 / zeropad25 at 4096 points: a clump of equal points (1230 copies, 1024 zero rows) overfills one bucket, whose limit is
    64; a well-spread cloud does not."""
    assert S.bucket_occupancy(O.synthetic_clouds(1, 4096, 3, "repeat30")[0]) >= 1230
    assert S.bucket_occupancy(O.synthetic_clouds(1, 4096, 3, "zeropad25")[0]) >= 1024
    assert S.bucket_occupancy(O.synthetic_clouds(1, 4096, 3, "uniform")[0]) <= S.BUCKET_MAX


def test_bucket_is_a_function_of_the_cube():
    cells = np.random.RandomState(1).randint(0, 1024, size=(5000, 3))
    bucket = (S.hilbert_index(cells, 10) >> np.uint64(18)).astype(np.int64)
    cube = (cells >> 6) @ np.array([256, 16, 1])
    pairs = np.unique(np.stack([cube, bucket], 1), axis=0)
    assert len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


def _small_clouds():
    for kind, n, seed in (("uniform", 37, 0), ("dup", 64, 1), ("lidar", 200, 2), ("repeat30", 100, 3), ("zeros", 9, 4), ("lattice", 27, 5)):
        yield O.synthetic_clouds(1, n, seed, kind)[0]
    yield S.clouds_of(S.lattice_spec(33))[2]
    for n in (2049, 2100):                  # the narrow key (top 20 bits) on clouds small enough for sorted()
        yield O.synthetic_clouds(1, n, n, "dup")[0]
        yield S.clouds_of(S.occupancy_spec(n, "cell1500"))[0]


def test_expected_perm_is_pythons_sorted_over_index_and_position():
    for cloud in _small_clouds():
        n = len(cloud)
        index = [int(v) for v in S.hilbert_index(S.cells_of(cloud), 10)]
        if 2049 <= n <= 4096:
            index = [v >> 10 for v in index]
        want = [j for _, j in sorted((index[j], j) for j in range(n))]
        assert S.expected_perm(cloud).tolist() == want


def _odd_clouds():
    base = O.synthetic_clouds(1, 300, 8)[0]
    nan_row, inf_row, all_nan = base.copy(), base.copy(), np.full_like(base, np.nan)
    nan_row[17, 1] = np.nan
    inf_row[250, 0] = np.inf
    plane, line = base.copy(), base.copy()
    plane[:, 2] = 0.25
    line[:, 1:] = -1.5
    return {"nan": nan_row, "inf": inf_row, "all_nan": all_nan, "equal": np.full_like(base, 0.75), "plane": plane, "line": line}


def test_expected_perm_is_a_permutation_on_degenerate_and_non_finite_clouds():
    for name, cloud in _odd_clouds().items():
        perm = S.expected_perm(cloud)
        assert perm.dtype == np.int32 and np.array_equal(np.sort(perm), np.arange(len(cloud))), name
        assert S.cells_of(cloud).max() <= 1023
    odd = _odd_clouds()
    assert np.array_equal(S.expected_perm(odd["all_nan"]), np.arange(300)) and np.array_equal(S.expected_perm(odd["equal"]), np.arange(300))
    assert (S.cells_of(odd["plane"])[:, 2] == 0).all() and (S.cells_of(odd["line"])[:, 1:] == 0).all()
    # fminf / fmaxf skip the NaN: the box, and with it every other point's cell, is that of the finite coordinates; the NaN gives cell 0
    clean = odd["nan"].copy()
    clean[17, 1] = clean[:, 1][np.isfinite(clean[:, 1])].min()
    assert np.array_equal(S.cells_of(odd["nan"]), S.cells_of(clean))
    # an Inf makes the axis's extent infinite and its scale 0: the whole axis falls into cell 0
    assert (S.cells_of(odd["inf"])[:, 0] == 0).all() and S.cells_of(odd["inf"])[:, 1:].max() == 1023


def test_sorting_the_sorted_cloud_is_the_identity():
    clouds = list(_small_clouds()) + [c for k, c in _odd_clouds().items() if k not in ("nan", "all_nan")]
    clouds += [O.synthetic_clouds(1, n, 6, kind)[0] for kind in ("uniform", "repeat30") for n in (3000, 4096, 8192)]
    clouds += list(S.clouds_of(S.lattice_spec(4097)))
    for cloud in clouds:
        srt = cloud[S.expected_perm(cloud)]
        assert np.array_equal(S.expected_perm(srt), np.arange(len(cloud)))


def test_lattice_cloud_refuses_inexact_frames_and_missing_corners():
    with pytest.raises(AssertionError):
        S.lattice_cloud(S.CORNERS, 0.1, 10)            # 0.1 + c / 1024 is not a float32
    with pytest.raises(AssertionError):
        S.lattice_cloud(S.CORNERS, 1.0e6, 12)          # too few bits left below 2**-4 at 10**6
    with pytest.raises(AssertionError):
        S.lattice_cloud(np.array([[0, 0, 0], [1023, 1023, 1022]]), 0.0, 10)
