"""The hash-drawn augmentation of epc-net_amd/augment.py on the CPU: the package's ``augment_clouds`` and tables against the independent
restatement tests/augment_ref.py, bit for bit, and both against the formulas of the module's docstring on fixed inputs -- every figure
here is deterministic, none a flaky statistic."""
import math

import numpy as np
import pytest

import augment_ref as R
import helpers as H

A = H.pkg("augment")


def _cloud(n=4096, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (1, n, 3)).astype(np.float32)


def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def test_package_tables_are_the_restatement():
    for max_angle in (math.pi / 2, 0.3, 0.0, math.pi):
        assert np.array_equal(A.rotation_table(max_angle).view(np.uint32), R.rotation_table(max_angle).view(np.uint32))
    for sigma, clip in ((0.005, 0.05), (0.01, 0.02), (0.0, 0.05)):
        assert np.array_equal(A.jitter_table(sigma, clip).view(np.uint32), R.jitter_table(sigma, clip).view(np.uint32))
    assert A.TABLE == R.TABLE == 65536
    rot, jit = A.rotation_table(), A.jitter_table()
    assert rot.shape == (65536, 2) and rot.dtype == np.float32 and jit.shape == (65536,) and jit.dtype == np.float32
    assert rot.nbytes == 512 * 1024 and jit.nbytes == 256 * 1024             # 512 KB + 256 KB


@pytest.mark.parametrize("max_angle", [math.pi / 2, 0.3])
def test_rotation_table(max_angle):
    rot = A.rotation_table(max_angle).astype(np.float64)
    err = np.abs(rot[:, 0] ** 2 + rot[:, 1] ** 2 - 1.0).max()
    theta = np.arctan2(rot[:, 1], rot[:, 0])
    print("max |c^2 + s^2 - 1| = %.3e, max |theta| = %.6f of %.6f" % (err, np.abs(theta).max(), max_angle))
    assert err <= 3e-7
    assert np.abs(theta).max() < max_angle
    assert np.all(np.diff(theta) > 0) and abs(theta[0] + theta[-1]) < 1e-6     # ascending mid-points, symmetric about 0
    assert np.allclose(np.diff(theta), 2 * max_angle / R.TABLE, rtol=0, atol=1e-6)


def test_jitter_table():
    sigma, clip = 0.005, 0.05
    jit = A.jitter_table(sigma, clip)
    assert np.all(np.diff(jit) >= 0)                                             # non-decreasing
    assert np.array_equal(jit, -jit[::-1])                                       # antisymmetric
    assert np.abs(jit).max() <= clip
    std = float(jit.astype(np.float64).std())
    print("table std / sigma = %.6f, max |z| = %.3f sigma" % (std / sigma, np.abs(jit).max() / sigma))
    assert abs(std - sigma) <= 1e-3 * sigma
    # clip = 2 sigma: the share of entries AT +-clip is the two-sided normal tail beyond 2 sigma
    tight = A.jitter_table(sigma, 2 * sigma)
    at = float((np.abs(tight) == np.float32(2 * sigma)).mean())
    print("share at +-clip (clip = 2 sigma): %.5f" % at)
    assert abs(at - 0.0455) <= 0.001 and np.abs(tight).max() == np.float32(2 * sigma)
    assert np.all(np.diff(tight) >= 0) and np.array_equal(tight, -tight[::-1])


def test_state_is_the_headers_chain():
    """The seven-word chain spelled out with the mixer, for a seed and a step whose high words take part."""
    from tuples_ref import mix
    seed, step, lane, slot = (0x1234 << 32) | 0x9ABCDEF0, (1 << 32) + 5, 3, 17
    for stream in (R.STREAM_ROTATION, R.STREAM_JITTER):
        s = mix(0x9ABCDEF0)
        for w in (0x1234, 5, 1, lane, slot, stream):
            s = mix(np.uint64(int(s) ^ w))
        assert int(R.state(seed, step, lane, slot, stream)) == int(s)
    assert R.state(seed, step, lane, slot, 0) != R.state(seed, step, lane, slot, 1)
    assert R.state(seed, 5, lane, slot, 0) != R.state(seed, step, lane, slot, 0)             # the step's high word takes part
    assert R.state(seed & 0xFFFFFFFF, step, lane, slot, 0) != R.state(seed, step, lane, slot, 0)
    assert R.state(-1, 0, 0, 0, 0) == R.state(2 ** 64 - 1, 0, 0, 0, 0)                       # a negative seed = its 64-bit pattern


def test_jitter_draw():
    sigma = 0.005
    pc = _cloud()
    out = R.augment(pc, 7, None, R.jitter_table(), rotate=False, jitter=True, seed=0, lane=0)   # slot 0 ...
    idx = R.jitter_indices(0, 7, 0, 3, 4096)                                                     # ... and slot 3, from the indices
    assert idx.shape == (4096, 3) and idx.min() >= 0 and idx.max() < R.TABLE
    draws = R.jitter_table()[idx].astype(np.float64)
    print("slot 3, step 7: std / sigma = %.4f, mean / sigma = %.4f" % (draws.std() / sigma, draws.mean() / sigma))
    assert abs(draws.std() - sigma) <= 0.03 * sigma
    delta = out.astype(np.float64) - pc.astype(np.float64)
    assert np.abs(delta).max() <= 0.05 + 1e-7 and abs(delta.std() - sigma) <= 0.03 * sigma
    # coordinate a of point p uses 3 p + a: the flat order of the (n, 3) index array
    from tuples_ref import mix
    s = R.state(0, 7, 0, 3, R.STREAM_JITTER)
    assert idx[5, 2] == int(mix(np.uint64(int(s) ^ 17)) >> np.uint64(16))


def test_rotation_draw():
    pc = _cloud(seed=1)
    rot = R.rotation_table()
    out = R.augment(pc, 7, rot, None, rotate=True, jitter=False)
    assert np.array_equal(out[..., 2].view(np.uint32), pc[..., 2].view(np.uint32))             # z: the same bits
    n_in, n_out = np.linalg.norm(pc.astype(np.float64), axis=2), np.linalg.norm(out.astype(np.float64), axis=2)
    print("row norms: max relative change %.3e" % (np.abs(n_out - n_in) / n_in).max())
    assert (np.abs(n_out - n_in) / n_in).max() <= 2e-6
    # pc @ R of the reference's formula (utils/loading_pointclouds.py:80-86) with the drawn entry, in float64, rounded
    c, s = rot[R.rotation_index(0, 7, 0, 0)].astype(np.float64)
    want = pc[0].astype(np.float64) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    err = np.abs(out[0].astype(np.float64) - want.astype(np.float32).astype(np.float64))
    # One ulp per coordinate -- an ulp AT THE MAGNITUDE OF WHAT IS ADDED: the larger of the result and its two products.  The prescribed
    # arithmetic rounds each product once (half an ulp of the product each) before the sum, so where x c and y s cancel the result
    # keeps the products' rounding and no implementation of fl(fl(x c) + fl(y s)) stays within an ulp of the small RESULT: on this
    # input 446 of the 8192 rotated coordinates are further than that, the worst by 4830 of its own ulps; at the products'
    # magnitude the worst is 1.000.
    x, y = pc[0, :, 0].astype(np.float64), pc[0, :, 1].astype(np.float64)
    scale = np.stack([np.maximum(np.abs(x * c), np.abs(y * s)), np.maximum(np.abs(y * c), np.abs(x * s)), np.abs(want[:, 2])], 1)
    ulp = _ulp(np.maximum(np.abs(want), scale))
    print("rotation vs float64 pc @ R: worst error %.3f ulp" % (err / ulp).max())
    assert np.all(err <= ulp)
    assert not np.array_equal(out[..., :2], pc[..., :2])
    # max_angle = 0: c = 1, s = 0 exactly, and the formula returns x, y (x * 1 + y * 0)
    same = R.augment(pc, 7, R.rotation_table(0.0), None, rotate=True, jitter=False)
    assert np.array_equal(same, pc)


def test_slots_and_steps_differ_and_off_is_the_identity():
    pc = np.repeat(_cloud(256, seed=2), 2, 0)                                   # the same cloud in slots 0 and 1
    rot, jit = R.rotation_table(), R.jitter_table()
    for kw in (dict(rotate=True, jitter=False), dict(rotate=False, jitter=True), dict(rotate=True, jitter=True)):
        a0, a1 = R.augment(pc, 0, rot, jit, **kw), R.augment(pc, 1, rot, jit, **kw)
        assert not np.array_equal(a0[0], a0[1])                                 # slots 0 and 1 of one step
        assert not np.array_equal(a0[0], a1[0])                                 # steps 0 and 1 of one slot
        assert not np.array_equal(a0[0], R.augment(pc, 0, rot, jit, lane=1, **kw)[0])
        assert not np.array_equal(a0[0], R.augment(pc, 0, rot, jit, seed=1, **kw)[0])
        assert np.array_equal(a0, R.augment(pc, 0, rot, jit, **kw))             # the same bits every time
    off = R.augment(pc, 0, rot, jit, rotate=False, jitter=False)
    assert np.array_equal(off.view(np.uint32), pc.view(np.uint32))
    assert R.rotation_index(0, 0, 0, 0) != R.rotation_index(0, 0, 0, 1)


def test_rotation_indices_draw_evenly():
    """36 000 rotation indices (50 steps x 18 slots x 40 lanes) in 16 bins: chi-square on 15 degrees of freedom below its 99.9 %
    point 37.7 (a fixed hash on fixed inputs: the figure is one number, not a sample)."""
    idx = np.array([R.rotation_index(0, st, lane, t) for st in range(50) for t in range(18) for lane in range(40)])
    bins = np.bincount(idx * 16 // R.TABLE, minlength=16)
    chi2 = float(((bins - len(idx) / 16) ** 2 / (len(idx) / 16)).sum())
    print("rotation index chi-square (15 dof): %.1f" % chi2)
    assert bins.sum() == 36000 and chi2 < 37.7


def test_argument_checks():
    for call in (lambda: A.jitter_table(0.005, 0.0), lambda: A.jitter_table(0.005, -1.0), lambda: A.jitter_table(-0.001, 0.05),
                 lambda: A.jitter_table(float("nan"), 0.05), lambda: A.rotation_table(-0.1), lambda: A.rotation_table(3.2),
                 lambda: A.rotation_table(float("nan"))):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("n", [1, 7, 256])
def test_package_draw_is_the_restatement(n):
    """augment_clouds == augment_ref.augment, the same bits: every flag combination, lanes 0 and 1, step 0 and one past 2^32 (the high
    word takes part), a 64-bit seed, non-default tables with clip = 2 sigma (entries AT the clip), a zero-padded cloud and one with
    duplicated points among the five, and a cloud that occurs twice (two slots, two different augmentations)."""
    rng = np.random.default_rng(5)
    clouds = rng.uniform(-1, 1, (5, n, 3)).astype(np.float32)
    clouds[1, n // 2:] = 0.0
    clouds[2, n // 2:] = clouds[2, :n - n // 2]
    clouds[4] = clouds[0]
    for rotate, jitter in ((True, False), (False, True), (True, True)):
        for lane in (0, 1):
            for step in (0, 2 ** 32 + 5):
                got = A.augment_clouds(clouds, step, rotate=rotate, jitter=jitter, lane=lane)
                want = R.augment(clouds, step, R.rotation_table(), R.jitter_table(), rotate=rotate, jitter=jitter, lane=lane)
                assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, rotate, jitter, lane, step)
                assert not np.array_equal(got[0], got[4])
    kw = dict(seed=(0x1234 << 32) | 0x9ABCDEF0, lane=3)
    got = A.augment_clouds(clouds, 11, max_angle=0.7, sigma=0.01, clip=0.02, **kw)
    want = R.augment(clouds, 11, R.rotation_table(0.7), R.jitter_table(0.01, 0.02), **kw)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    tables = (A.rotation_table(0.7), A.jitter_table(0.01, 0.02))
    assert np.array_equal(A.augment_clouds(clouds, 11, tables=tables, **kw).view(np.uint32), want.view(np.uint32))
    off = A.augment_clouds(clouds, 3, rotate=False, jitter=False)
    assert np.array_equal(off.view(np.uint32), clouds.view(np.uint32)) and off is not clouds
    for bad in (clouds.astype(np.float64), clouds[0], clouds[:, :, :2]):
        with pytest.raises(ValueError):
            A.augment_clouds(bad, 0)
    with pytest.raises(ValueError):
        A.augment_clouds(clouds, 0, lane=-1)
