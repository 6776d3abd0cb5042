"""Rotation about z and jitter of training clouds from a FIXED HASH instead of numpy's random stream: pure numpy, importable without
a GPU or the library.

The reference ships ``rotate_point_cloud`` and ``jitter_point_cloud`` (utils/loading_pointclouds.py:67-100; this package mirrors them in
``utils.loading_pointclouds``) and draws from ``np.random``: a restored run does not continue the stream, and data-parallel ranks
seeded alike rotate alike.  ``augment_clouds`` below draws from a hash of (seed, step, lane, slot, point): the same bits on every
run, for any step in any order.  The definition is written so that a device kernel can restate it bit for bit -- everything
transcendental sits in two tables built once in float64 and rounded to float32, and the rest is 32-bit integer hashing and float32
arithmetic with every operation rounded once (numpy never contracts into an FMA).  tests/augment_ref.py is a second, independent
restatement; tests/test_augment_cpu.py holds both to the formulas.

The draw.
  mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16      (uint32; include/epcnet_poses.h's mixer)
  s = mix((uint32)seed);  for w in ((uint32)(seed >> 32), (uint32)step, (uint32)(step >> 32), lane, t, stream):  s = mix(s ^ w)
for slot t -- the cloud's position in the batch, NOT a record id: a cloud that occurs twice in a tuple is augmented twice, differently,
as in the reference's per-cloud loop -- the caller's word ``lane`` (a data-parallel rank) and stream 0 (rotation) or 1 (jitter).
  rotation table   TABLE pairs (float32 cos, float32 sin) of theta_i = (2 (i + 0.5) / TABLE - 1) max_angle; slot t uses the pair
                   mix(s_rot ^ 0) >> 16.  max_angle = pi / 2 is the reference's -90 .. 90 degrees (:79).
  jitter table     TABLE float32: clip(sigma Phi^-1((i + 0.5) / TABLE), -clip, clip), Phi^-1 from statistics.NormalDist; coordinate a
                   of point p uses the entry mix(s_jit ^ (3 p + a)) >> 16.  sigma = 0.005, clip = 0.05: :89.
  arithmetic       x' = fl(fl(x c) + fl(y s));  y' = fl(fl(y c) - fl(x s));  z' = z   (pc @ [[c, -s, 0], [s, c, 0], [0, 0, 1]], :80-86),
                   then v'' = fl(v' + jitter) per coordinate.  A part switched off is SKIPPED, not multiplied by an identity: with
                   both off the input bits come back."""
from __future__ import annotations

import functools
import math
from statistics import NormalDist

import numpy as np

TABLE = 65536          # entries per table (a 16-bit index: the top half of a 32-bit hash)
STREAM_ROTATION, STREAM_JITTER = 0, 1
_M32 = np.uint64(0xFFFFFFFF)


def rotation_table(max_angle: float = math.pi / 2) -> np.ndarray:
    """(TABLE, 2) float32: (cos, sin) of theta_i = (2 (i + 0.5) / TABLE - 1) max_angle -- the mid-points of TABLE equal parts of
    (-max_angle, max_angle), so |theta| < max_angle; the default is the reference's -90 .. 90 degrees (:79)."""
    max_angle = float(max_angle)
    if not 0.0 <= max_angle <= math.pi:
        raise ValueError("rotation_table: max_angle must lie in [0, pi], got %r" % max_angle)
    theta = (2.0 * (np.arange(TABLE, dtype=np.float64) + 0.5) / TABLE - 1.0) * max_angle
    return np.ascontiguousarray(np.stack([np.cos(theta), np.sin(theta)], 1).astype(np.float32))


@functools.lru_cache(maxsize=1)
def _unit_quantiles() -> np.ndarray:
    """Phi^-1((i + 0.5) / TABLE) in float64 by the standard library (65536 calls: a few tenths of a second, once per process)."""
    inv = NormalDist().inv_cdf
    z = np.array([inv((i + 0.5) / TABLE) for i in range(TABLE)], dtype=np.float64)
    z.setflags(write=False)
    return z


def jitter_table(sigma: float = 0.005, clip: float = 0.05) -> np.ndarray:
    """(TABLE,) float32: clip(sigma Phi^-1((i + 0.5) / TABLE), -clip, clip) -- the normal distribution's quantiles at the mid-points of
    TABLE equal parts of (0, 1): np.clip(sigma * randn, -clip, clip) of :89-98 with the uniform draw left to the hash."""
    sigma, clip = float(sigma), float(clip)
    if not clip > 0.0:
        raise ValueError("jitter_table: clip must be positive, got %r" % clip)
    if not sigma >= 0.0:
        raise ValueError("jitter_table: sigma must not be negative, got %r" % sigma)
    return np.ascontiguousarray(np.clip(sigma * _unit_quantiles(), -clip, clip).astype(np.float32))


def _mix(x: np.ndarray) -> np.ndarray:
    """The 32-bit mixer on uint32 values held in uint64 (masked after every product)."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def _state(seed: int, step: int, lane: int, slots: np.ndarray, stream: int) -> np.ndarray:
    """The hash state of every slot in front of the table draw, as uint64 holding uint32."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    s = _mix(np.uint64(seed & 0xFFFFFFFF))
    for w in (seed >> 32, step & 0xFFFFFFFF, step >> 32, int(lane) & 0xFFFFFFFF):
        s = _mix(s ^ np.uint64(w))
    return _mix(_mix(s ^ (slots.astype(np.uint64) & _M32)) ^ np.uint64(stream))


def augment_clouds(clouds: np.ndarray, step: int, rotate: bool = True, jitter: bool = True, max_angle: float = math.pi / 2,
                   sigma: float = 0.005, clip: float = 0.05, seed: int = 0, lane: int = 0, tables=None) -> np.ndarray:
    """The augmented copy of ``clouds`` (T, n, 3) float32 -- a training tuple in the order it is fed, slot t = cloud t -- for training
    step ``step`` (pass ``TrainStep.global_step``: a restored run then continues the same stream) and the caller's ``lane`` (the
    data-parallel rank, so that ranks do not rotate alike).  ``tables``: a ``(rotation_table(...), jitter_table(...))`` pair built
    once by a caller in a loop; built here from ``max_angle`` / ``sigma`` / ``clip`` otherwise."""
    clouds = np.asarray(clouds)
    if clouds.dtype != np.float32 or clouds.ndim != 3 or clouds.shape[2] != 3:
        raise ValueError("augment_clouds: clouds must be float32 (T, n, 3), got %s %s" % (clouds.dtype, clouds.shape))
    if not 0 <= int(lane) < 1 << 32:
        raise ValueError("augment_clouds: lane must fit an unsigned 32-bit word, got %r" % (lane,))
    rot, jit = tables if tables is not None else (rotation_table(max_angle) if rotate else None,
                                                  jitter_table(sigma, clip) if jitter else None)
    T, n = clouds.shape[:2]
    slots = np.arange(T)
    out = clouds.copy()
    if rotate:
        cs = rot[(_mix(_state(seed, step, lane, slots, STREAM_ROTATION)) >> np.uint64(16)).astype(np.int64)]      # (T, 2)
        c, s = cs[:, :1], cs[:, 1:]
        x, y = clouds[:, :, 0], clouds[:, :, 1]
        out[:, :, 0] = x * c + y * s
        out[:, :, 1] = y * c - x * s
    if jitter:
        k = (np.arange(3 * n, dtype=np.uint64) & _M32)[None, :]
        idx = _mix(_state(seed, step, lane, slots, STREAM_JITTER)[:, None] ^ k) >> np.uint64(16)
        out = out + jit[idx.astype(np.int64)].reshape(T, n, 3)
    assert out.dtype == np.float32
    return out
