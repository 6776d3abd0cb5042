"""epc_morton_sort ALONE at every form of its kernel (epc-net_amd/csrc/sort.hip), against the exact order tests/sort_ref.py restates
(tests/test_sort_cpu.py checks that file without a GPU).  One kernel, five sorting forms, chosen from the point count and, in one
case, from the data:

  n 1 .. 2048      the plain bitonic network in LDS, 64-bit keys
  n 2049 .. 4096   32-bit keys (top 20 bits of the Hilbert index | 12-bit point index), two-level bucket sort ...
                   ... which gives up when a bucket holds more than 64 keys: bitonic_registers<4, unsigned>
  n 4097 .. 8192   bitonic_registers<8, u64>
  n 8193 .. 16384  bitonic_registers<16, u64>

Every comparison is exact and on whole arrays: perm == expected_perm(cloud), xyz_sorted bit for bit cloud[perm].  On the lattice
clouds (points origin + cells * 2**-k, both corner cells present) the quantisation is exact under any rounding, so the expected order
is a function of integers only; the float clouds go through the float32 restatement of the quantisation.  The outputs are filled with
bytes 0xFF before the call and have slack behind them that must still hold them afterwards."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
import sort_ref as S
import stage_ref as R
from helpers import O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; there is no CPU fallback"
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _launch(pc, dev, with_perm=True):
    """epc_morton_sort through the raw ABI on pc (B, n, 3) float32 into poisoned outputs -> (xyz_sorted, perm or None) as numpy; the
    slack behind both outputs must still be poisoned."""
    L = H.pkg("lib")
    nc, n, _ = pc.shape
    t = torch.from_numpy(np.ascontiguousarray(pc)).to(dev)
    out = R.Poisoned((nc, n, 3), torch.float32, dev)
    perm = R.Poisoned((nc, n), torch.int32, dev)
    L.check(L.lib().epc_morton_sort(t.data_ptr(), nc, n, out.t.data_ptr(), perm.t.data_ptr() if with_perm else None,
                                    L.current_stream()))
    torch.cuda.synchronize()
    assert out.untouched() and perm.untouched(), "the kernel wrote behind an output"
    if not with_perm:
        assert R.holds_poison(perm.t)
    return out.t.cpu().numpy(), (perm.t.cpu().numpy() if with_perm else None)


def _check(pc, dev):
    """The launch's perm is expected_perm of every cloud and xyz_sorted holds the bits of cloud[perm].  Returns (xyz_sorted, perm)."""
    srt, perm = _launch(pc, dev)
    want = np.stack([S.expected_perm(c) for c in pc])
    bad = [(b, int(np.argmax(perm[b] != want[b]))) for b in range(len(pc)) if not np.array_equal(perm[b], want[b])]
    assert np.array_equal(perm, want), "perm differs from the reference order: (cloud, first rank) %s" % bad
    assert np.array_equal(_bits(srt), _bits(np.take_along_axis(pc, want[:, :, None].astype(np.int64), 1)))
    return srt, perm


# ---- lattice clouds: the expected order is a function of integers only -------------------------------------------------------------------
@pytest.mark.parametrize("n", S.ALL_SIZES)
def test_lattice_clouds_at_every_form(dev, n):
    """Three clouds per launch, a different origin and scale each: the corner points first and last; at indices 1024 and n - 1 (thread
    0's second stride, the last wave; the other points off the box's faces); a quarter of the points in shared cells, so that ties fall
    to the index, with the corners in wave 1."""
    if n == 1:
        pc = np.array([[[0.5, -2.0, 3.0]], [[0.0, 0.0, 0.0]], [[-7.25, 1e-3, 1e6]]], dtype=np.float32)   # (one point is its own box)
        _, perm = _check(pc, dev)
        assert not perm.any()
        return
    _check(S.clouds_of(S.lattice_spec(n)), dev)


@pytest.mark.parametrize("n", S.WAVE_SIZES)
def test_box_reduction_sees_every_wave(dev, n):
    """16 clouds; cloud w's two corner points are in wave w, one of them in the threads' second stride."""
    _check(S.clouds_of(S.wave_spec(n)), dev)


# ---- the narrow form's data-dependent choice ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.OCCUPANCY_SIZES)
@pytest.mark.parametrize("name", list(S.OCCUPANCY_CASES))
def test_narrow_form_at_the_bucket_limit(dev, n, name):
    """The fullest bucket holds exactly 64 keys (the bucket sort keeps the cloud), exactly 65 (bitonic_registers<4> takes it), or
    1500 keys of one cell (tests/test_sort_cpu.py asserts these occupancies)."""
    _check(S.clouds_of(S.occupancy_spec(n, name)), dev)


@pytest.mark.parametrize("n", S.OCCUPANCY_SIZES)
def test_narrow_form_decides_per_cloud(dev, n):
    """Bucket sort, fallback, bucket sort in one launch."""
    _check(S.clouds_of(S.mixed_spec(n)), dev)


# ---- float clouds through the float32 restatement of the quantisation --------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 2048, 3000, 4096, 8192, 16384])
@pytest.mark.parametrize("kind", ["uniform", "lidar", "dup", "repeat30", "zeropad25", "zeros"])
def test_float_clouds(dev, kind, n):
    pc = O.synthetic_clouds(3, n, 21, kind)
    _, perm = _check(pc, dev)
    if kind == "zeros":
        assert np.array_equal(perm, np.tile(np.arange(n, dtype=np.int32), (3, 1)))


@pytest.mark.parametrize("n", [100, 4096, 8192])
def test_degenerate_boxes(dev, n):
    """All points equal (every key ties: the identity), one axis constant, two axes constant."""
    pc = O.synthetic_clouds(3, n, 5)
    pc[0] = np.float32([0.75, -1.5, 3.0])
    pc[1, :, 2] = 0.25
    pc[2, :, 1:] = -1.5
    _, perm = _check(pc, dev)
    assert np.array_equal(perm[0], np.arange(n))


@pytest.mark.parametrize("n", [96, 4096, 8192])
def test_non_finite_rows(dev, n):
    """One NaN coordinate, one +Inf coordinate, a cloud of NaNs: fminf / fmaxf skip a NaN, an infinite extent gives scale 0, a NaN
    cell index clamps to 0 -- in every case a permutation of 0 .. n-1 (the pipeline sends such clouds through this kernel before it
    flags them), and the one tests/sort_ref.py derives from those rules."""
    pc = O.synthetic_clouds(3, n, 13)
    pc[0, n // 3, 1] = np.nan
    pc[1, n - 7, 0] = np.inf
    pc[2] = np.nan
    _, perm = _check(pc, dev)
    assert np.array_equal(np.sort(perm, axis=1), np.tile(np.arange(n, dtype=np.int32), (3, 1)))
    assert np.array_equal(perm[2], np.arange(n))


# ---- the entry point's other arguments ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 4096, 8192])
def test_null_perm_gives_the_same_cloud(dev, n):
    pc = S.clouds_of(S.lattice_spec(n, seed=4))
    srt, _ = _check(pc, dev)
    alone, _ = _launch(pc, dev, with_perm=False)
    assert np.array_equal(_bits(alone), _bits(srt))


def _refused(dev, xyz, nc, n, out, perm):
    """The raw status of a call that must be refused; the outputs stay poisoned."""
    L = H.pkg("lib")
    rc = L.lib().epc_morton_sort(xyz, nc, n, out.t.data_ptr(), perm.t.data_ptr(), L.current_stream())
    torch.cuda.synchronize()
    assert R.holds_poison(out.t) and R.holds_poison(perm.t) and out.untouched() and perm.untouched()
    return rc


def test_zero_clouds_and_refusals_write_nothing(dev):
    L = H.pkg("lib")
    src = torch.from_numpy(O.synthetic_clouds(1, 16384, 0)).to(dev)
    out = R.Poisoned((1, 16384, 3), torch.float32, dev)
    perm = R.Poisoned((1, 16384), torch.int32, dev)
    assert _refused(dev, src.data_ptr(), 0, 4096, out, perm) == L.EPC_OK             # nothing to do is not an error
    assert _refused(dev, src.data_ptr(), 1, 0, out, perm) == L.EPC_EINVAL
    assert _refused(dev, src.data_ptr(), 1, 16385, out, perm) == L.EPC_EINVAL
    assert _refused(dev, None, 1, 4096, out, perm) == L.EPC_EINVAL
    assert _refused(dev, out.t.data_ptr(), 1, 4096, out, perm) == L.EPC_EINVAL     # xyz == xyz_sorted
    assert L.lib().epc_morton_sort(src.data_ptr(), 1, 4096, None, perm.t.data_ptr(), L.current_stream()) == L.EPC_EINVAL
    torch.cuda.synchronize()
    assert R.holds_poison(perm.t)


# ---- idempotence: on the device, and of the pipeline's own call of the sort --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _form_cloud(form):
    if form == "plain":
        return S.clouds_of(S.lattice_spec(2048, seed=8))
    if form == "bucket":
        return S.clouds_of(S.occupancy_spec(4096, "occ64", 2))
    if form == "fallback":
        return np.concatenate([S.clouds_of(S.occupancy_spec(4096, "occ65", 3)), O.synthetic_clouds(1, 4096, 2, "repeat30")])
    return O.synthetic_clouds(2, {"regs8": 8192, "regs16": 16384}[form], 9, "dup")


@pytest.mark.parametrize("form", ["plain", "bucket", "fallback", "regs8", "regs16"])
def test_sorting_the_sorted_cloud_returns_it(dev, form):
    srt, _ = _check(_form_cloud(form), dev)
    again, perm = _check(srt, dev)
    assert np.array_equal(_bits(again), _bits(srt))
    assert np.array_equal(perm, np.tile(np.arange(srt.shape[1], dtype=np.int32), (len(srt), 1)))


def test_the_pipelines_sort_is_this_sort(dev):
    """engine.forward sorts every cloud itself (the launch that also zeroes the pass's status words).  Sorting is idempotent, so the
    descriptors of x and of epc_morton_sort(x) are the same bits if and only if the pipeline's launch orders the points as the entry
    point tested above does.  And the status words are zeroed by that launch: after a pass that flagged a cloud, a clean pass reads 0."""
    L = H.pkg("lib")
    ops = H.pkg("ops")
    eng, _ = H.make_engine("epc-net-l", O.seeded_weights("epc-net-l", 0), dev)
    pc = O.synthetic_clouds(3, 256, 31)
    x = torch.from_numpy(pc).to(dev)
    srt = ops.morton_sort(x)
    want, _ = _check(pc, dev)
    assert np.array_equal(_bits(srt.cpu().numpy()), _bits(want)) and not torch.equal(srt, x)
    first = eng.forward(x).clone()
    assert eng.last_status(3) == [0, 0, 0] and bool(torch.isfinite(first).all())
    assert torch.equal(eng.forward(srt), first)
    bad = pc.copy()
    bad[1, 100, 2] = np.nan
    out = eng.forward(torch.from_numpy(bad).to(dev))
    assert eng.last_status(3) == [0, L.EPC_STATUS_NONFINITE_INPUT, 0] and bool(torch.isnan(out[1]).all())
    assert torch.equal(eng.forward(x), first) and eng.last_status(3) == [0, 0, 0]
