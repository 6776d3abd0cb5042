"""numpy restatement of the pose relations and the tuple draw of include/epcnet_poses.h
(csrc/pose_tuples.hip): the hash, the three classifications and the selections, each written the obvious way -- a full argsort where the
kernels find a radix threshold.  The GPU tests hold the library to it bit for bit; tests/test_pose_tuples_cpu.py holds IT to the
package's own host rule (utils.loading_pointclouds.get_query_tuple_ids) and checks that the fixed hash draws evenly."""
import numpy as np

STREAM_POSITIVES, STREAM_CANDIDATES, STREAM_NEGATIVES, STREAM_OTHER = 0, 1, 2, 3
FEW_POSITIVES, FEW_NEGATIVES, NO_OTHER, BAD_KEY = 1, 2, 4, 8
M32 = np.uint64(0xFFFFFFFF)


def mix(x):
    """x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 on uint32 (held in uint64, masked)."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def state(seed, step, key, stream):
    """The hash state in front of the record id; ``step`` and ``key`` may be arrays (broadcast)."""
    seed = int(seed) & (2 ** 64 - 1)
    step = np.asarray(step).astype(np.int64).astype(np.uint64)
    key = np.asarray(key).astype(np.int64).astype(np.uint64) & M32
    s = mix(seed & 0xFFFFFFFF)
    for w in (np.uint64(seed >> 32), step & M32, step >> np.uint64(32), key, np.uint64(int(stream))):
        s = mix(s ^ w)
    return s


def values(seed, step, key, stream, ids):
    """(hash << 32) | id of the records ``ids`` (uint64): what every selection orders by."""
    ids = np.asarray(ids, dtype=np.uint64)
    return (mix(state(seed, step, key, stream) ^ ids) << np.uint64(32)) | ids


def d2(poses, p):
    """Squared distances of all ``poses`` to the pose ``p``: dx * dx + dy * dy in float64, every operation rounded once."""
    dx, dy = poses[:, 0] - p[0], poses[:, 1] - p[1]
    return dx * dx + dy * dy


def positives_mask(poses, key, r_pos):
    m = d2(poses, poses[key]) <= r_pos * r_pos
    m[key] = False
    return m


def negatives_mask(poses, key, r_neg):
    return d2(poses, poses[key]) > r_neg * r_neg


def eligible_other_mask(poses, key, negatives, r_pos):
    """A positive neither of the key nor of any chosen negative (nobody is his own positive: the key itself stays eligible)."""
    m = ~positives_mask(poses, key, r_pos)
    for n in negatives:
        if n >= 0:
            m &= ~positives_mask(poses, int(n), r_pos)
    return m


def radius_lists(query, db, r):
    return [np.nonzero(d2(db, q) <= r * r)[0] for q in query]


def radius_tables(query, db, r, width=None):
    """(padded (Q, width) int32 with -2, lens (Q,) int32, status): rows longer than ``width`` truncated, status 1."""
    lists = radius_lists(query, db, r)
    lens = np.array([len(x) for x in lists], dtype=np.int32)
    if width is None:
        width = max(int(lens.max()) if len(lists) else 0, 1)
    padded = np.full((len(lists), width), -2, dtype=np.int32)
    for i, x in enumerate(lists):
        padded[i, :min(len(x), width)] = x[:width]
    return padded, lens, int(bool((lens > width).any()))


def pos_count(poses, r_pos):
    return np.array([int(positives_mask(poses, i, r_pos).sum()) for i in range(len(poses))], dtype=np.int32)


def _smallest(ids, seed, step, key, stream, k):
    """The (at most) k records of ``ids`` with the smallest values, in that order."""
    ids = np.asarray(ids, dtype=np.int64)
    order = np.argsort(values(seed, step, key, stream, ids), kind="stable")
    return ids[order[:k]]


def candidates(poses, keys, r_neg, seed, step, C):
    """Per key the ascending ids of its min(C, #negatives) negatives with the smallest values of stream 1; status per key."""
    out, status = [], np.zeros(len(keys), dtype=np.int32)
    for b, key in enumerate(keys):
        if not 0 <= key < len(poses):
            out.append(np.zeros(0, dtype=np.int64))
            status[b] |= BAD_KEY
            continue
        negs = np.nonzero(negatives_mask(poses, key, r_neg))[0]
        out.append(np.sort(_smallest(negs, seed, step, key, STREAM_CANDIDATES, C)))
    return out, status


def sample(poses, keys, r_pos, r_neg, seed, step, P, Nn, hard=None):
    """ids (B, 1 + P + Nn + 1) int32 and status (B,) int32 of epcnet_tuple_sample."""
    T, W = len(poses), 1 + P + Nn + 1
    ids = np.full((len(keys), W), -1, dtype=np.int32)
    status = np.zeros(len(keys), dtype=np.int32)
    for b, key in enumerate(keys):
        if not 0 <= key < T:
            status[b] |= BAD_KEY
            continue
        ids[b, 0] = key
        pos = _smallest(np.nonzero(positives_mask(poses, key, r_pos))[0], seed, step, key, STREAM_POSITIVES, P)
        ids[b, 1:1 + len(pos)] = pos
        if len(pos) < P:
            status[b] |= FEW_POSITIVES
        negs = []
        for h in ([] if hard is None else hard[b]):
            if 0 <= h < T and h not in negs and len(negs) < Nn:
                negs.append(int(h))
        pool = np.nonzero(negatives_mask(poses, key, r_neg))[0]
        pool = pool[~np.isin(pool, negs)]
        negs += [int(c) for c in _smallest(pool, seed, step, key, STREAM_NEGATIVES, Nn - len(negs))]
        ids[b, 1 + P:1 + P + len(negs)] = negs
        if len(negs) < Nn:
            status[b] |= FEW_NEGATIVES
        other = _smallest(np.nonzero(eligible_other_mask(poses, key, negs, r_pos))[0], seed, step, key, STREAM_OTHER, 1)
        if len(other):
            ids[b, W - 1] = other[0]
        else:
            status[b] |= NO_OTHER
    return ids, status


def fixture_poses(T, seed=0):
    """Test poses on the 1/8 m lattice around (5 735 000, 620 000): every dx * dx + dy * dy is exact in float64 (so FMA contraction
    cannot matter), while float32 collapses them onto a 0.5 m lattice.  A loop trajectory with side clusters; the first records are
    placed by hand: pairs at exactly 10.0, 25.0 and 50.0 m (3-4-5 triangles), a pair at 10.125 m, duplicates, and a 20-record cluster
    inside 10 m far from everything else (records 12..31)."""
    rng = np.random.RandomState(seed)
    base = np.array([5735000.0, 620000.0])
    hand = [(0, 0), (48, 64),                # 0-1: 6 m, 8 m -> exactly 10.0 m
            (2400, 0), (2400 + 120, 160),    # 2-3: 15 m, 20 m -> exactly 25.0 m
            (4800, 0), (4800 + 240, 320),    # 4-5: 30 m, 40 m -> exactly 50.0 m
            (7200, 0), (7200 + 81, 0),       # 6-7: 10.125 m
            (9600, 0), (9600, 0), (9600, 0),  # 8-10: duplicates
            (9600 + 8, 0)]                   # 11: 1 m from the duplicates
    cluster = [(-24000 + int(a), -24000 + int(b)) for a, b in rng.randint(-28, 29, (20, 2))]   # 12..31: within 10 m of each other
    n_rest = T - len(hand) - len(cluster)
    t = np.linspace(0, 2 * np.pi, n_rest, endpoint=False)
    radius = min(16000.0, np.round(n_rest * 24 / (2 * np.pi)))          # records about 3 m apart along the loop (2.5 m at T = 5003)
    loop = np.stack([np.round(radius * np.cos(t)) + rng.randint(-16, 17, n_rest),
                     12000 + np.round(radius * np.sin(t)) + rng.randint(-16, 17, n_rest)], 1)
    ij = np.concatenate([np.array(hand + cluster, dtype=np.float64), loop.astype(np.float64)])[:T]
    return base + ij / 8.0


def brute_force_dict(poses, r_pos=10.0, r_neg=50.0):
    """generate_training_tuples_baseline.py:52-62 by brute force, without its shuffles: the reference-format training dict."""
    out = {}
    for i in range(len(poses)):
        d2 = ((poses - poses[i]) ** 2).sum(1)
        out[i] = {"query": "%d.bin" % i, "positives": [int(j) for j in np.nonzero(d2 <= r_pos ** 2)[0] if j != i],
                  "negatives": [int(j) for j in np.nonzero(~(d2 <= r_neg ** 2))[0]]}
    return out
