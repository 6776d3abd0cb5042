"""CPU tests of the raw-scan front end: the numpy restatement's known answers (tests/downsample_ref.py is the kernel's contract), the
binding derived for the two entry points, loud failure on CPU tensors."""
from ctypes import c_int, c_size_t, c_void_p

import numpy as np
import pytest
import torch

import downsample_ref as R
import helpers as H


def _kept_keys(out_sensor, lo, e, Rs):
    """Cell keys of an output in sensor units (normalize=False): q / 4096 per axis."""
    q = np.rint((out_sensor.astype(np.float64) - lo) / (float(e) / (Rs * 4096))).astype(np.int64)
    c = q >> 12
    return (c[:, 2] * 1024 + c[:, 1]) * 1024 + c[:, 0]


def test_lattice_every_cell_kept():
    out, status, info = R.grid_downsample_ref(R.lattice(8), 512)
    assert status == 0 and info == [512, 8, 512, 1]
    keys = _kept_keys(R.grid_downsample_ref(R.lattice(8), 512, normalize=False)[0], np.zeros(3), 7.0, 8)
    assert np.array_equal(keys, np.sort(np.unique(keys))) and keys.size == 512
    assert out.dtype == np.float32 and out.shape == (512, 3) and 1.0 - 2.0 ** -23 <= np.abs(out).max() <= 1.0
    assert abs(float(out.astype(np.float64).mean())) < 1e-3


def test_lattice_keeps_highest_counts_then_smallest_keys():
    p = R.lattice(8)
    out, status, info = R.grid_downsample_ref(p, 256, normalize=False)
    assert status == 0 and info[:3] == [512, 7, 343]
    # the grid of 7 cells over 8 lattice planes per axis: cell counts and keys from first principles
    u = R._u(p, p.min(0), np.float32(7.0), 7)
    keys, cnt = np.unique(R._keys(u), return_counts=True)
    assert keys.size == 343
    order = sorted(range(343), key=lambda i: (-cnt[i], keys[i]))[:256]
    assert info[3] == cnt[order[-1]]
    want = np.sort(keys[order])
    assert np.array_equal(_kept_keys(out, np.zeros(3), 7.0, 7), want)
    # every cell with more points than the last kept one is kept; of the cells tied with it, the smallest keys
    last = info[3]
    assert set(keys[cnt > last]) <= set(want)
    tied = keys[cnt == last]
    kept_tied = np.array(sorted(set(want) & set(tied)))
    assert np.array_equal(kept_tied, tied[:kept_tied.size])


def test_line_and_repeated_points():
    line = np.stack([np.linspace(0, 1, 3000), np.zeros(3000), np.zeros(3000)], 1)
    _, status, info = R.grid_downsample_ref(line, 256)
    assert status == 0 and info[1] == 256 and info[2] == 256
    pts = np.random.default_rng(0).uniform(-1, 1, (100, 3))
    out, status, info = R.grid_downsample_ref(np.tile(pts, (30, 1)), 256)
    assert out is None and status == 4 and info == [3000, 0, 0, 0]


@pytest.mark.parametrize("N,M", [(32, 40), (32, 200), (256, 1000), (256, 3000), (1024, 9000), (4096, 20000), (4096, 70000)])
def test_scenes_have_a_grid(N, M):
    out, status, info = R.grid_downsample_ref(R.scene(M, M), N)
    assert status == 0 and out.shape == (N, 3) and N <= info[2] <= 2 * N
    assert np.isfinite(out).all() and 1.0 - 2.0 ** -23 <= np.abs(out).max() <= 1.0     # d * fl(1 / max|d|): one ulp below 1 at most


def test_failures_of_the_restatement():
    assert R.grid_downsample_ref(R.scene(100, 1), 256)[1:] == (4, [100, 0, 0, 0])                 # fewer than N points
    assert R.grid_downsample_ref(np.zeros((0, 3)), 32)[1:] == (4, [0, 0, 0, 0])
    assert R.grid_downsample_ref(np.ones((300, 3)), 256)[1:] == (4, [300, 0, 0, 0])               # e == 0
    _, status, info = R.grid_downsample_ref(R.split_clusters(), 32)                                # D(R*) > 2N
    assert status == 4 and info[2] > 64 and info[1] > 0
    dirty = R.scene(1000, 3).copy()
    dirty[::10, 1] = np.nan
    assert R.grid_downsample_ref(dirty, 256)[2][0] == 900                                          # non-finite rows are dropped


def test_binding_of_the_two_entries():
    L = H.pkg("lib")
    P, i = c_void_p, c_int
    assert L.EPC_STATUS_NO_GRID == 4
    ws = L.lib().epc_grid_downsample_workspace_bytes
    assert ws.restype == c_size_t and list(ws.argtypes) == [i, i]
    fn = L.lib().epc_grid_downsample
    assert fn.restype == i and list(fn.argtypes) == [P, P, i, i, i, P, P, P, P, c_size_t, P] and len(fn.argtypes) == 11
    # 0 = unsupported n; host arithmetic only
    assert ws(4, 48) == 0 and ws(4, 8192) == 0 and ws(4, 0) == 0 and ws(4, 32) > 0 and ws(4, 4096) > 0
    assert ws(64, 4096) >= 64 * 4 * 4


def test_operators_refuse_cpu_tensors():
    ops = H.pkg("ops")
    E = H.pkg("lib").EpcNetError
    pts, off = torch.zeros((64, 3)), torch.tensor([0, 64], dtype=torch.int32)
    with pytest.raises(E):
        ops.grid_downsample(pts, off, 32)
    with pytest.raises(E):
        ops.grid_downsample(pts.double(), off, 32)
    with pytest.raises(E):
        ops.grid_downsample(pts, off.long(), 32)
    if not torch.cuda.is_available():
        with pytest.raises(E):
            ops.pack_scans([np.zeros((5, 3))])
