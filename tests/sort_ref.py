"""The spatial sort (epc-net_amd/csrc/sort.hip, epc_morton_sort) restated in numpy: the Hilbert index of integer cells, the kernel's
float32 quantisation of a cloud to cells, the permutation the kernel must return, and clouds whose cells are exact integers so that
the expected order involves no float rounding at all (tests/test_gpu_sort_forms.py; tests/test_sort_cpu.py checks this file without
a GPU).

The kernel's order: per cloud, the bounding box -> 10 bits per axis -> 30-bit Hilbert index; keys (index, original point index) are
sorted, so ties in the index fall to the lower original index.  For 2049 <= n <= 4096 points (npow2 == 4096) the keys keep only the
top 20 bits of the index; every other point count sorts the full 30 bits.  Which sorting network or bucket pass produced the order is
not visible in it: the keys are unique, so the order is one function of the cloud."""
import numpy as np

CELL_BITS = 10                     # bits per axis of the kernel's grid
CELL_MAX = (1 << CELL_BITS) - 1    # 1023
NARROW_FROM, NARROW_TO = 2049, 4096     # point counts whose keys keep the top 20 bits only (sort.hip: npow2 == 4096)
BUCKET_MAX = 64                    # sort.hip SORT_BUCKET_MAX: a fuller bucket sends the narrow form to bitonic_registers<4>
SORT_MAX_N = 16384


def hilbert_index(cells, bits):
    """Index along the 3-D Hilbert curve of the integer cells (m, 3), `bits` bits per axis (Skilling's transpose algorithm,
    "Programming the Hilbert curve", 2004); the first coordinate carries the most significant bit of every triple.  uint64 (m,)."""
    cells = np.asarray(cells)
    assert cells.ndim == 2 and cells.shape[1] == 3 and 1 <= bits <= 21
    X = [cells[:, d].astype(np.uint32).copy() for d in range(3)]
    top = 1 << (bits - 1)
    Q = top
    while Q > 1:
        P = np.uint32(Q - 1)
        for i in range(3):
            m = (X[i] & np.uint32(Q)) != 0
            X[0] = np.where(m, X[0] ^ P, X[0])
            t = np.where(~m, (X[0] ^ X[i]) & P, 0).astype(np.uint32)
            X[0] = X[0] ^ t
            X[i] = X[i] ^ t
        Q >>= 1
    X[1] = X[1] ^ X[0]
    X[2] = X[2] ^ X[1]
    t = np.zeros_like(X[0])
    Q = top
    while Q > 1:
        t = np.where((X[2] & np.uint32(Q)) != 0, t ^ np.uint32(Q - 1), t)
        Q >>= 1
    code = np.zeros(len(t), dtype=np.uint64)
    for bit in range(bits):
        for d in range(3):          # X[0] carries the most significant bit of every triple
            code |= (((X[d] ^ t) >> np.uint32(bit)) & np.uint32(1)).astype(np.uint64) << np.uint64(3 * bit + (2 - d))
    return code


def cells_of(cloud):
    """The kernel's quantisation of one cloud (n, 3) float32 to 10-bit cells, in float32 with one rounding per operation: the box by
    fminf / fmaxf (a NaN is skipped; a cloud of NaNs keeps +Inf / -Inf), scale = 1023 / ext where ext > 0 else 0, q = (v - lo) * scale,
    fmaxf(q, 0) then fminf(., 1023) -- NaN becomes 0 -- and truncation.  uint32 (n, 3)."""
    cloud = np.asarray(cloud)
    assert cloud.dtype == np.float32 and cloud.ndim == 2 and cloud.shape[1] == 3
    with np.errstate(all="ignore"):
        lo = np.fmin.reduce(cloud, axis=0, initial=np.float32(np.inf))
        hi = np.fmax.reduce(cloud, axis=0, initial=np.float32(-np.inf))
        ext = (hi - lo).astype(np.float32)
        pos = ext > 0
        scale = np.where(pos, np.float32(1023.0) / np.where(pos, ext, np.float32(1)), np.float32(0)).astype(np.float32)
        q = ((cloud - lo).astype(np.float32) * scale).astype(np.float32)
        q = np.fmin(np.fmax(q, np.float32(0)), np.float32(1023))
    assert q.dtype == np.float32
    return q.astype(np.uint32)


def sort_keys(cloud):
    """The Hilbert part of the kernel's keys for one cloud: the 30-bit index, or its top 20 bits at the narrow point counts."""
    n = len(cloud)
    code = hilbert_index(cells_of(cloud), CELL_BITS)
    return code >> np.uint64(10) if NARROW_FROM <= n <= NARROW_TO else code


def expected_perm(cloud):
    """The permutation epc_morton_sort must return for one cloud: a stable argsort by key, i.e. the total order of (key, j)."""
    return np.argsort(sort_keys(cloud), kind="stable").astype(np.int32)


def bucket_occupancy(cloud):
    """The fullest of the narrow form's 4096 buckets (the top 12 bits of the 30-bit index): above BUCKET_MAX the kernel leaves the
    bucket sort for bitonic_registers<4>."""
    code = hilbert_index(cells_of(cloud), CELL_BITS)
    return int(np.bincount((code >> np.uint64(18)).astype(np.int64), minlength=4096).max())


def lattice_cloud(cells, origin, k):
    """Points origin + cells * 2**-k in float32 for integer cells (n, 3) in 0..1023 that contain (0,0,0) and (1023,1023,1023).
    Every coordinate must be exact in float32 (asserted).  Then lo = origin, ext = 1023 * 2**-k, 1023 / ext = 2**k and
    (v - lo) * scale = the cell, each exactly and under any rounding mode: the expected order of such a cloud is a function of the
    integers alone."""
    cells = np.asarray(cells, dtype=np.int64)
    assert cells.ndim == 2 and cells.shape[1] == 3 and cells.min() >= 0 and cells.max() <= CELL_MAX
    assert (cells == 0).all(1).any() and (cells == CELL_MAX).all(1).any(), "both corner cells must be present"
    origin = np.broadcast_to(np.asarray(origin, dtype=np.float64), (3,))
    exact = origin[None, :] + cells.astype(np.float64) * 2.0 ** -k            # (exact in float64: few bits on either side)
    cloud = exact.astype(np.float32)
    assert np.array_equal(cloud.astype(np.float64), exact), "origin / k do not keep the coordinates exact in float32"
    return cloud


# ---- the lattice clouds of tests/test_gpu_sort_forms.py (built here so that tests/test_sort_cpu.py checks the very same ones) ---------
# (origin, k) pairs that keep every coordinate exact; a launch gives each of its clouds another one
FRAMES = [(0.0, 10), (-3.5, 7), (17.25, 12), (-0.5, 10)]
CORNERS = np.array([[0, 0, 0], [CELL_MAX] * 3], dtype=np.int64)


def _place(n, cells, at):
    """`cells` (n - 2, 3) with the two corner cells inserted at the indices at = (i0, i1) of the result (n, 3)."""
    i0, i1 = at
    assert i0 != i1 and 0 <= min(i0, i1) and max(i0, i1) < n and len(cells) == n - 2
    out = np.empty((n, 3), dtype=np.int64)
    rest = np.ones(n, dtype=bool)
    rest[[i0, i1]] = False
    out[rest] = cells
    out[i0], out[i1] = CORNERS[0], CORNERS[1]
    return out


def corner_slots(n, which):
    """Where the corner points sit.  'ends': first and last.  'stride': indices 1024 and n - 1 for n > 1025 -- thread 0's second
    stride and the last wave that holds a point -- else the last index and the middle one.  'wave1': indices 64 + 5 and, where it
    exists, 1024 + 64 + 7: both in wave 1, the first one the box reduction's serial pass adds to wave 0's value."""
    assert n >= 2
    if which == "ends":
        return 0, n - 1
    if which == "stride":
        if n > 1025:
            return 1024, n - 1
        return (n - 1, n // 2) if n - 1 != n // 2 else (1, 0)
    assert which == "wave1" and n > 71
    return 69, (1024 + 71 if n > 1024 + 71 else 70)


def random_lattice_cells(n, seed, which="ends", inner=0, tie_quarter=False):
    """n cells: the two corners at corner_slots(n, which), the others uniform over inner .. 1023 - inner (inner > 0 keeps them off the
    box's faces, so that a box computed without a corner point moves every cell).  tie_quarter: a quarter of the points take the cell
    of another point, wherever they sit, so that equal keys are ordered by the point index."""
    rng = np.random.RandomState(seed)
    body = rng.randint(inner, CELL_MAX + 1 - inner, size=(n - 2, 3)).astype(np.int64)
    if tie_quarter and n >= 6:
        m = n - 2
        dst = rng.permutation(m)[: max(n // 4, 1)]
        body[dst] = body[rng.randint(0, m, size=len(dst))]
    return _place(n, body, corner_slots(n, which))


def occupancy_cells(n, m, seed, one_cell=False):
    """n cells whose fullest bucket holds exactly m (2 <= m): m points inside ONE of the 4096 cubes cells >> 6 (a bucket is a function
    of cells >> 6 alone) -- in one cell of it when one_cell -- the rest in distinct other cubes, one point each, and the two corners in
    cubes of their own; shuffled."""
    rng = np.random.RandomState(seed)
    fill = n - m - 2
    assert m >= 2 and 0 <= fill <= 4093
    cube = np.array([5, 9, 3], dtype=np.int64)
    inside = rng.randint(0, 64, size=(1 if one_cell else m, 3))
    clump = cube * 64 + np.broadcast_to(inside, (m, 3))
    ids = np.arange(4096)
    ids = ids[(ids != 0) & (ids != 4095) & (ids != (cube[0] * 256 + cube[1] * 16 + cube[2]))]
    ids = rng.permutation(ids)[:fill]
    cubes = np.stack([ids >> 8, (ids >> 4) & 15, ids & 15], 1)
    filler = cubes * 64 + rng.randint(0, 64, size=(fill, 3))
    cells = np.concatenate([clump, filler, CORNERS], 0)
    return cells[rng.permutation(n)]


# A "spec" is a list of (cells, (origin, k)): what a launch's clouds are made of.  tests/test_sort_cpu.py checks every spec the GPU file
# uses (the quantisation returns the cells, the occupancies are the named ones); clouds_of() turns a spec into the (B, n, 3) input.
def clouds_of(spec):
    return np.stack([lattice_cloud(cells, *frame) for cells, frame in spec])


def lattice_spec(n, seed=0):
    """The three lattice clouds of one launch at n >= 3 points, a different frame each: corners at the ends; corners at 'stride' with
    the other cells off the faces; a quarter of the points in shared cells with the corners in wave 1 (n > 71, else at 'stride').
    n = 2: the two corners in both orders and again.  (n = 1 has no lattice cloud: one point is its own box.)"""
    assert n >= 2
    if n == 2:
        return [(CORNERS, FRAMES[0]), (CORNERS[::-1], FRAMES[1]), (CORNERS, FRAMES[2])]
    return [(random_lattice_cells(n, seed, "ends"), FRAMES[seed % 4]),
            (random_lattice_cells(n, seed + 1, "stride", inner=16), FRAMES[(seed + 1) % 4]),
            (random_lattice_cells(n, seed + 2, "wave1" if n > 71 else "stride", inner=16, tie_quarter=True), FRAMES[(seed + 2) % 4])]


def wave_spec(n):
    """16 clouds of n >= 2048 points: cloud w has both corners in wave w of the 1024-thread workgroup (indices 64 w + 5 and
    1024 + 64 w + 7, the second one in the threads' second stride), every other cell off the box's faces."""
    assert n >= 2048
    return [(_place(n, np.random.RandomState(100 + w).randint(16, 1008, size=(n - 2, 3)), (64 * w + 5, 1024 + 64 * w + 7)),
             FRAMES[w % 4]) for w in range(16)]


# the occupancy cases of the narrow form: name -> (fullest bucket, all of it in one cell)
OCCUPANCY_CASES = {"occ64": (64, False), "occ65": (65, False), "cell1500": (1500, True)}
OCCUPANCY_SIZES = (2049, 4095, 4096)


def occupancy_spec(n, name, frame=0):
    """One cloud of the named occupancy (a one-cloud spec)."""
    m, one_cell = OCCUPANCY_CASES[name]
    return [(occupancy_cells(n, m, seed=n + m + 100000 * frame, one_cell=one_cell), FRAMES[frame % 4])]


def mixed_spec(n):
    """Bucket sort, fallback, bucket sort in one launch: the decision is each workgroup's own."""
    return occupancy_spec(n, "occ64", 1) + occupancy_spec(n, "occ65", 2) + occupancy_spec(n, "occ64", 3)


# point counts per form of the kernel (sort.hip: the plain network in LDS; 32-bit keys, bucket sort or bitonic_registers<4>;
# bitonic_registers<8>; bitonic_registers<16>)
FORM_SIZES = {"plain": (1, 2, 3, 33, 1025, 2047, 2048), "narrow": (2049, 3000, 4095, 4096),
              "regs8": (4097, 8191, 8192), "regs16": (8193, 16383, 16384)}
ALL_SIZES = tuple(n for sizes in FORM_SIZES.values() for n in sizes)
WAVE_SIZES = (2048, 4096, 8192)
