"""A second, independent numpy restatement of the augmentation draw that epc-net_amd/augment.py defines: the hash state (with the mixer of
tests/tuples_ref.py, not the package's), the two table formulas and the float32 arithmetic, each written the obvious way -- one
cloud at a time.  tests/test_augment_cpu.py holds the package's ``augment_clouds`` to it bit for bit, and both to the formulas."""
import functools
import math
from statistics import NormalDist

import numpy as np

from tuples_ref import M32, mix

TABLE = 65536
STREAM_ROTATION, STREAM_JITTER = 0, 1
ROTATE, JITTER = 1, 2


def rotation_table(max_angle=math.pi / 2):
    i = np.arange(TABLE, dtype=np.float64)
    theta = (2.0 * (i + 0.5) / TABLE - 1.0) * float(max_angle)
    return np.stack([np.cos(theta), np.sin(theta)], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def jitter_table(sigma=0.005, clip=0.05):
    """(Cached per argument pair and read-only: 65536 calls of the standard library's inverse take a few tenths of a second.)"""
    nd = NormalDist()
    z = np.array([nd.inv_cdf((i + 0.5) / TABLE) for i in range(TABLE)], dtype=np.float64)
    out = np.clip(float(sigma) * z, -float(clip), float(clip)).astype(np.float32)
    out.setflags(write=False)
    return out


def state(seed, step, lane, slot, stream):
    """s = mix((uint32)seed); s = mix(s ^ w) for w in (seed >> 32, (uint32)step, step >> 32, lane, slot, stream)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    s = mix(seed & 0xFFFFFFFF)
    for w in (seed >> 32, step & 0xFFFFFFFF, step >> 32, int(lane) & 0xFFFFFFFF, int(slot) & 0xFFFFFFFF, int(stream)):
        s = mix(s ^ np.uint64(w))
    return s


def rotation_index(seed, step, lane, slot):
    return int(mix(state(seed, step, lane, slot, STREAM_ROTATION) ^ np.uint64(0)) >> np.uint64(16))


def jitter_indices(seed, step, lane, slot, n):
    """(n, 3) table indices: coordinate a of point p uses mix(s_jit ^ (3 p + a)) >> 16."""
    k = (np.arange(3 * n, dtype=np.uint64) & M32).reshape(n, 3)
    return (mix(state(seed, step, lane, slot, STREAM_JITTER) ^ k) >> np.uint64(16)).astype(np.int64)


def augment(clouds, step, rot_table=None, jit_table=None, rotate=True, jitter=True, seed=0, lane=0):
    """``clouds`` (T, n, 3) float32 -> the augmented (T, n, 3) float32; slot t = the cloud's position in ``clouds``.  float32
    arithmetic, every operation rounded once (numpy never contracts)."""
    clouds = np.asarray(clouds)
    assert clouds.dtype == np.float32 and clouds.ndim == 3 and clouds.shape[2] == 3
    out = clouds.copy()
    n = clouds.shape[1]
    for t in range(clouds.shape[0]):
        if rotate:
            c, s = rot_table[rotation_index(seed, step, lane, t)]
            x, y = clouds[t, :, 0], clouds[t, :, 1]
            out[t, :, 0] = x * c + y * s
            out[t, :, 1] = y * c - x * s
        if jitter:
            out[t] = out[t] + jit_table[jitter_indices(seed, step, lane, t, n)]
    assert out.dtype == np.float32
    return out
