"""A bit-level CPU emulation of the fp16 + MX-fp6 conv5 product of EPC_PRECISION_FAST (csrc/common.h at W5_SCALE, csrc/pack.hip
fold_pack_conv5_kernel(f16 = 1) + pack_conv5_lo6_kernel, csrc/conv5_vlad.hip c5_to_fp6 / c5_load_operands / c5_chunk_chain), in plain
numpy: float64 where the values are exact, float32 / uint32 bit operations where the device code rounds in f32, float16 where it
rounds to fp16.  tests/test_f16f6_ref_cpu.py checks it without a GPU, tests/test_gpu_f16f6_product.py holds the kernels to it.

  weight    w = W[k][col] * ((1 / sqrt(var + 1e-3)) * gamma) * 256 (f32, in that order); hi = fp16(w) -- of the f32-ROUNDED w, which
            is not always fp16 of the exact product: the pack forms lo from the hi it stored --; lo = w - hi (exact in f32);
            per (col, block of 32 k): e = block_exponent(max |lo|, -100, 20), lo6 = q6(fp16(lo * 2^-e)) * 2^e
            (pack_conv5_lo6_kernel hands the conversion an fp16 vector: lo * 2^-e is rounded to fp16 first -- 13 bits to 11 --, then
            to e2m3; the emulation takes both steps);
  bias      (b * inv + (beta - mean * inv)) * 256 in f32;
  input     per (row, block of 32 channels): e = block_exponent(max |x16|, -12, 14), x6 = q6(fp16(x16 * 2^-e)) * 2^e (the fp16
            product is exact unless it lands under 2^-14, far below e2m3's smallest step: rounded to fp16 here as there);
  product   acc = bias + sum_k x16 * hi + sum_blocks sum_k x6 * lo6 in float64, S = |bias| + sum |x16 * hi| + sum |x6 * lo6|.

MUTANTS are deliberately wrong variants of the emulation -- a dropped term, a scale byte of the neighbouring block, a reversed or
exchanged operand order, another rounding rule -- that the CPU test runs through the GPU tests' predicates: a predicate that cannot
tell a mutant from the emulation could not tell a kernel with that fault either."""
import functools

import numpy as np

from helpers import O

W5_SCALE = 256.0
FP6_MAX = 7.5
U32 = 2.0 ** -24          # float32 unit roundoff

# ---- e2m3 ------------------------------------------------------------------------------------------------------------------------------
# code = s eem mmm: e = 0: m / 8 (0 .. 0.875, step 0.125); e > 0: (1 + m / 8) * 2^(e - 1) (1 .. 1.875 step 0.125, 2 .. 3.75 step 0.25,
# 4 .. 7.5 step 0.5).  The magnitudes ascend with the 5-bit code, so a code's parity is its mantissa's.
MAGS = np.array([m / 8.0 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 1) for e in range(4) for m in range(8)], dtype=np.float64)
DECODE = np.concatenate([MAGS, -MAGS])          # 64 entries; code 32 is -0.0


def q6_codes(v, rtz=False):
    """e2m3 codes of v (any shape): round to nearest, ties to the even mantissa, saturating at +-7.5 (rtz: toward zero instead)."""
    v = np.asarray(v, dtype=np.float64)
    a = np.minimum(np.abs(v), FP6_MAX)
    lo = np.searchsorted(MAGS, a, side="right") - 1          # MAGS[lo] <= a
    hi = np.minimum(lo + 1, 31)
    if rtz:
        idx = lo
    else:
        dl, dh = a - MAGS[lo], MAGS[hi] - a                  # exact: dyadic values of a few bits
        idx = np.where((dh < dl) | ((dh == dl) & ((lo & 1) == 1)), hi, lo)
    return (idx | (np.signbit(v).astype(np.int64) << 5)).astype(np.uint8)


def q6(v, rtz=False):
    return DECODE[q6_codes(v, rtz)]


def block_exponent(m, lo_e, hi_e, round_up=True):
    """fp6_block_exponent (common.h) as the integer rule on the float32 bit pattern of float32(m) * float32(1 / 7.5): exponent field -
    127, + 1 if any mantissa bit is set, clamped to [lo_e, hi_e].  m = 0 gives lo_e.  (round_up = False: the mutant without the + 1.)"""
    p = np.ascontiguousarray(np.asarray(m, dtype=np.float32) * (np.float32(1.0) / np.float32(FP6_MAX)), dtype=np.float32)
    bits = p.view(np.uint32).astype(np.int64)
    e = ((bits >> 23) & 0xff) - 127
    if round_up:
        e = e + ((bits & 0x7fffff) != 0)
    return np.clip(e, lo_e, hi_e)


# ---- mutants -----------------------------------------------------------------------------------------------------------------------------
def mutants(cin):
    """Names of the wrong variants for a cin-channel product (blocks of 32 channels; the scale taken from block b + 1 / b - 1 wraps)."""
    nb = cin // 32
    return ["lo_dropped", "lo_block_dropped:0", "lo_block_dropped:%d" % (nb - 1), "w_scale_from:+1", "w_scale_from:-1",
            "x_scale_from:+1", "x_scale_from:-1", "x6_reversed", "w_halves_swapped", "fp6_rtz", "exponent_no_round_up"]


def _arg(mutant, name):
    return int(mutant.split(":")[1]) if mutant is not None and mutant.startswith(name + ":") else None


# ---- weight side -------------------------------------------------------------------------------------------------------------------------
def conv5_vars(w):
    """(W (cin, 1024), b, gamma, beta, mean, var) float32 of a weight dict's conv5."""
    mean, var = O.ema_names("fastdgcnn/conv5")
    W = np.asarray(w["fastdgcnn/conv5/weights"], dtype=np.float32)
    return (W.reshape(-1, 1024), w["fastdgcnn/conv5/biases"], w["fastdgcnn/conv5/bn/gamma"], w["fastdgcnn/conv5/bn/beta"], w[mean],
            w[var])


def fold_f32(w):
    """fold_pack_conv5_kernel(f16 = 1)'s expressions in numpy float32: (w (cin, 1024), bias (1024)), both scaled by 256."""
    W, b, gamma, beta, mean, var = (np.asarray(a, dtype=np.float32) for a in conv5_vars(w))
    inv = (np.float32(1.0) / np.sqrt(var + np.float32(1e-3))) * gamma
    return W * inv[None, :] * np.float32(W5_SCALE), (b * inv + (beta - mean * inv)) * np.float32(W5_SCALE)


def fold_f64(w):
    """The ideal folded weights W' * 256 and bias * 256 in float64 from the same float32 variables."""
    W, b, gamma, beta, mean, var = (np.asarray(a, dtype=np.float64) for a in conv5_vars(w))
    inv = gamma / np.sqrt(var + O.BN_EPS)
    return W * inv[None, :] * W5_SCALE, (b * inv + (beta - mean * inv)) * W5_SCALE


class Pack:
    """hi, lo, lo6 (cin, 1024) float64, the weight block exponents we (cin / 32, 1024) (as USED: a mutant may take a neighbour's) and
    bias (1024) float64."""

    def __init__(self, wf, bias, mutant=None):
        wf = np.asarray(wf, dtype=np.float32)
        cin = wf.shape[0]
        nb = cin // 32
        hi = wf.astype(np.float16).astype(np.float32)
        lo = wf - hi                                                     # exact in f32
        lob = lo.reshape(nb, 32, 1024)
        e = block_exponent(np.abs(lob).max(1), -100, 20, round_up=mutant != "exponent_no_round_up")
        q16 = (lob * np.exp2(-e).astype(np.float32)[:, None, :]).astype(np.float16)    # f32 product (exact), then fp16
        codes = q6_codes(q16.astype(np.float64), rtz=mutant == "fp6_rtz")
        d = _arg(mutant, "w_scale_from")
        if d is not None:
            e = np.roll(e, -d, axis=0)                                   # block b decodes with the scale of block b + d
        if mutant == "w_halves_swapped":                                 # blocks 2ks and 2ks + 1 (the lane halves of a k-step) exchanged
            codes = codes.reshape(nb // 2, 2, 32, 1024)[:, ::-1].reshape(nb, 32, 1024)
            e = e.reshape(nb // 2, 2, 1024)[:, ::-1].reshape(nb, 1024)
        lo6 = DECODE[codes] * np.exp2(e.astype(np.float64))[:, None, :]
        if mutant == "lo_dropped":
            lo6[:] = 0.0
        b = _arg(mutant, "lo_block_dropped")
        if b is not None:
            lo6[b] = 0.0
        self.cin, self.nb = cin, nb
        self.hi, self.lo, self.lo6, self.we = hi.astype(np.float64), lo.astype(np.float64), lo6.reshape(cin, 1024), e
        self.bias = np.asarray(bias, dtype=np.float64)


# ---- activation side ---------------------------------------------------------------------------------------------------------------------
def to_f16(x):
    """x rounded to fp16 (nearest even), as float64."""
    return np.asarray(x).astype(np.float16).astype(np.float64)


def rows_fp6(x16, mutant=None):
    """c5_to_fp6 on fp16-valued rows x16 (rows, cin) float64 -> (x6 (rows, cin) float64, xe (rows, cin / 32) exponents as used)."""
    rows, cin = x16.shape
    nb = cin // 32
    assert np.array_equal(to_f16(x16), x16), "the rows must hold fp16 values"
    xb = x16.reshape(rows, nb, 32)
    e = block_exponent(np.abs(xb).max(2), -12, 14, round_up=mutant != "exponent_no_round_up")
    q16 = (xb * np.exp2(-e.astype(np.float64))[:, :, None]).astype(np.float16)         # v * down in fp16
    codes = q6_codes(q16.astype(np.float64), rtz=mutant == "fp6_rtz")
    if mutant == "x6_reversed":
        codes = codes[:, :, ::-1]
    d = _arg(mutant, "x_scale_from")
    if d is not None:
        e = np.roll(e, -d, axis=1)
    return (DECODE[codes] * np.exp2(e.astype(np.float64))[:, :, None]).reshape(rows, cin), e


# ---- the product -------------------------------------------------------------------------------------------------------------------------
def emulate(x16, pack, mutant=None):
    """(acc, S) (rows, 1024) float64 of fp16-valued rows against a Pack built with the same mutant."""
    x6, _ = rows_fp6(x16, mutant)
    acc = pack.bias[None, :] + x16 @ pack.hi + x6 @ pack.lo6
    S = np.abs(pack.bias)[None, :] + np.abs(x16) @ np.abs(pack.hi) + np.abs(x6) @ np.abs(pack.lo6)
    return acc, S


def emulate_f32(x16, pack):
    """The same terms accumulated in numpy float32 -- a yardstick for what ANY float32 accumulation of them costs: from the bias, one
    rounded partial sum per lo block, then one (exact) hi product at a time."""
    x6, _ = rows_fp6(x16)
    acc = np.broadcast_to(pack.bias.astype(np.float32), (x16.shape[0], 1024)).copy()
    for b in range(pack.nb):
        k = slice(32 * b, 32 * b + 32)
        acc = acc + (x6[:, k] @ pack.lo6[k]).astype(np.float32)
    x32, hi32 = x16.astype(np.float32), pack.hi.astype(np.float32)
    for k in range(pack.cin):
        acc = acc + x32[:, k:k + 1] * hi32[k][None, :]                   # 11 x 11 bits: the product is exact
    assert acc.dtype == np.float32
    return acc.astype(np.float64)


def terms(x16, pack):
    """Every term of the sum, (rows, 1 + 2 cin, 1024) float64: the bias, x16 * hi, x6 * lo6 (for the exactness check of small families)."""
    x6, _ = rows_fp6(x16)
    return np.concatenate([np.broadcast_to(pack.bias, (x16.shape[0], 1, 1024)), x16[:, :, None] * pack.hi[None],
                           x6[:, :, None] * pack.lo6[None]], axis=1)


def lowest_bit(t):
    """The value of the lowest set bit of every float64 in t (inf for zeros)."""
    m, e = np.frexp(np.asarray(t, dtype=np.float64))
    mant = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = (mant & -mant).astype(np.float64)
    return np.where(mant == 0, np.inf, low * np.exp2((e - 53).astype(np.float64)))


# ---- stages ------------------------------------------------------------------------------------------------------------------------------
def pooled_of(acc, nc, n):
    """EPC-Net-L: max over the cloud's points of relu(acc), / 256 -> (nc, 1024)."""
    return np.maximum(acc, 0.0).reshape(nc, n, 1024).max(1) / W5_SCALE


def feat_of(acc):
    """EPC-Net: (feat16 = fp16(relu(acc) / 256) as float64, ss = sum (relu(acc) / 256)^2, rnorm = 1 / sqrt(max(ss, 1e-12)))."""
    f = np.maximum(acc, 0.0) / W5_SCALE
    ss = (f * f).sum(1)
    return to_f16(f), ss, 1.0 / np.sqrt(np.maximum(ss, 1e-12))


def half_ulp16(v):
    """Half an fp16 ulp at |v| (float64; subnormal spacing 2^-24 under 2^-14)."""
    _, e = np.frexp(np.abs(v))                                           # |v| = m 2^e, m in [0.5, 1)
    return np.exp2(np.maximum(e - 1, -14).astype(np.float64) - 11.0)


# ---- the GPU tests' predicates, as excesses in units of S ---------------------------------------------------------------------------------
# A predicate holds at tolerance T iff its excess is <= T.
def pooled_excess(got, acc, S, nc, n):
    """max over (cloud, channel) of |pooled - pooled_emul| / (max_points(S) / 256)."""
    return float((np.abs(got - pooled_of(acc, nc, n)) / (S.reshape(nc, n, 1024).max(1) / W5_SCALE)).max())


def feat_excess(got16, acc, S):
    """max over elements of (|feat16 - relu(acc) / 256| - half an fp16 ulp of the emulated value) / (S / 256)."""
    f = np.maximum(acc, 0.0) / W5_SCALE
    return float(((np.abs(got16 - f) - half_ulp16(f)) / (S / W5_SCALE)).max())


# ---- the random family ---------------------------------------------------------------------------------------------------------------------
# (arch, clouds, points): max-pool with workgroups that straddle clouds, with one-cloud workgroups; conv5 + assign
RANDOM_CASES = [("epc-net-l", 3, 96), ("epc-net-l", 2, 128), ("epc-net", 2, 96)]
CIN = {"epc-net-l": 128, "epc-net": 256}


@functools.lru_cache(maxsize=None)
def seeded(arch):
    return O.seeded_weights(arch, 1)


@functools.lru_cache(maxsize=None)
def seeded_pack(arch, mutant=None):
    return Pack(*fold_f32(seeded(arch)), mutant=mutant)


@functools.lru_cache(maxsize=None)
def random_rows(arch, nc, n):
    """stage_ref.rows_with_scales rounded to fp16, cloud b scaled by b + 1 -> (nc * n, cin) float64 of fp16 values."""
    import stage_ref as R
    x = R.rows_with_scales(np.random.RandomState(7000 + 10 * nc + n), nc * n, CIN[arch], cloud_scale=np.arange(1, nc + 1), n=n)
    x16 = to_f16(x)
    x16.setflags(write=False)
    return x16


@functools.lru_cache(maxsize=None)
def random_emulation(arch, nc, n):
    acc, S = emulate(random_rows(arch, nc, n), seeded_pack(arch))
    acc.setflags(write=False), S.setflags(write=False)
    return acc, S


@functools.lru_cache(maxsize=None)
def yardstick():
    """worst |float32-accumulated - exact| / S over the random cases."""
    worst = 0.0
    for arch, nc, n in RANDOM_CASES:
        acc, S = random_emulation(arch, nc, n)
        worst = max(worst, float((np.abs(emulate_f32(random_rows(arch, nc, n), seeded_pack(arch)) - acc) / S).max()))
    return worst


def t_rand():
    """The random family's tolerance in units of S: 8 x the yardstick (the matrix pipe adds in another order and may truncate; its own
    accumulation error has not been measured separately)."""
    return 8.0 * yardstick()


# ---- the exact family ----------------------------------------------------------------------------------------------------------------------
ZERO_LO_COL = 77          # the column whose lo parts are all zero (block exponent clamped at -100)


@functools.lru_cache(maxsize=None)
def exact_weights(arch):
    """seeded_weights(arch, 1) with a conv5 whose fold and split are exact: gamma = 2^g per column (g = -2 .. 2), EMA variance
    float32(0.999) (+ 1e-3f == 1.0f), mean = beta = bias = 0, W * gamma * 256 = +-(H + l): H even in [2050, 4094] (fp16's spacing
    there is 2, |l| < 1: hi = +-H), l a multiple of 1/8 with |l| <= 0.875 scaled per (column, block) by 1, 1/2 or 1/4 -- (column +
    block) % 3 halvings, so neighbouring blocks and neighbouring columns (lanes) carry different scale bytes; every group holds a
    +-0.875 (before scaling), which fixes its exponent at -3, -4, -5; column ZERO_LO_COL has l = 0."""
    cin = CIN[arch]
    nb = cin // 32
    rng = np.random.RandomState(cin)
    w = dict(seeded(arch))
    H = 2.0 * rng.randint(1025, 2048, size=(cin, 1024))
    l8 = rng.randint(-7, 8, size=(nb, 32, 1024)).astype(np.float64)
    pos = rng.randint(0, 32, size=(nb, 1024))
    bi, ci = np.meshgrid(np.arange(nb), np.arange(1024), indexing="ij")
    l8[bi, pos, ci] = np.where(rng.randint(0, 2, size=(nb, 1024)) == 1, 7.0, -7.0)
    halvings = (ci + bi) % 3
    l = (l8 / 8.0) * np.exp2(-halvings.astype(np.float64))[:, None, :]
    l[:, :, ZERO_LO_COL] = 0.0
    sign = np.where(rng.randint(0, 2, size=(cin, 1024)) == 1, 1.0, -1.0)
    wf = sign * (H + l.reshape(cin, 1024))
    g = np.exp2(((np.arange(1024) * 7) % 5 - 2).astype(np.float64))
    mean, var = O.ema_names("fastdgcnn/conv5")
    z = np.zeros(1024, dtype=np.float32)
    W = (wf / (W5_SCALE * g[None, :])).astype(np.float32)
    assert np.array_equal(W.astype(np.float64) * g[None, :] * W5_SCALE, wf)
    w.update({"fastdgcnn/conv5/weights": W.reshape(1, cin, 1024), "fastdgcnn/conv5/biases": z, "fastdgcnn/conv5/bn/gamma": g.astype(np.float32),
              "fastdgcnn/conv5/bn/beta": z, mean: z, var: np.full(1024, 0.999, dtype=np.float32)})
    return w


@functools.lru_cache(maxsize=None)
def exact_pack(arch, mutant=None):
    return Pack(*fold_f32(exact_weights(arch)), mutant=mutant)


def onehot_rows(cin):
    """The non-zero rows of the one-hot sweep, (2 cin, cin): row i < cin has +3 in channel i, row cin + i has -3."""
    return np.concatenate([3.0 * np.eye(cin), -3.0 * np.eye(cin)])


TIES = np.array([7.5, 4.25, 4.75, 5.25, 5.75, 6.25, 6.75, 7.25])      # the maximum, then e2m3's midpoints of [4, 7.5] at e = 0
NEXT_ABOVE_MAX = 7.5 + 2.0 ** -8                                          # the next fp16 above 7.5


@functools.lru_cache(maxsize=None)
def special_rows(cin, big=1024.0):
    """The tie and boundary rows, {name: row (cin,)} -- dyadic values, few enough and coarse enough that every partial sum against
    exact_weights is a float32 (test_f16f6_ref_cpu.py checks that).  `big`: the large value of the 1024-and-ones row; the others
    of its block scale with it."""
    nb = cin // 32
    rows = {}
    for b in range(nb):
        r = np.zeros(cin)
        r[32 * b + (3 * np.arange(8) + b) % 32] = TIES * np.where(np.arange(8) % 3 == 2, -1.0, 1.0)
        rows["ties:%d" % b] = r                      # rounding direction of the conversion, block b
    r = np.zeros(cin)
    r[32 + 4 * np.arange(5)] = [NEXT_ABOVE_MAX, 4.25, -4.75, 5.25, 5.75]
    rows["above_7.5"] = r                            # the exponent steps to 1; 4.25 / 2 = 2.125 is a midpoint again
    r = np.zeros(cin)
    r[64 + 3 * np.arange(7)] = np.arange(1, 8) * 2.0 ** -17 * np.array([1, -1, 1, 1, -1, 1, -1])
    rows["subnormals"] = r                           # fp16 subnormals only: the -12 clamp; x * 2^12 = j / 32, j = 1 .. 7
    r = np.zeros(cin)
    r[cin - 32:] = (1.0 + 0.25 * ((np.arange(32) % 3) - 1)) * np.where(np.arange(32) % 2 == 1, -1.0, 1.0) * (big / 1024.0)
    r[cin - 32 + 9] = -big
    rows["big_and_ones"] = r                         # e = 8 (big = 1024): the values near 1 fall under e2m3's smallest step
    for q in range(nb // 4):
        r = np.zeros(cin)
        for b in range(4 * q, 4 * q + 4):
            r[32 * b + (5 * b + 3) % 32] = (-1.0) ** b * 2.0 ** (2 * (b % 4) - 4)
        rows["block_scales:%d" % q] = r              # block b scaled by 2^(2 (b % 4) - 4): four distinct scale bytes in the row
    for r in rows.values():
        r.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def exact_rows(arch):
    """(names, rows (R, cin)) of the exact family: the one-hot sweep (+3 in channel k, then -3), the tie and boundary rows and their
    negatives (ReLU hides one sign of every sum).  Each row is row 0 of a cloud of 32 points whose other rows are zero.  EPC-Net's
    1024-and-ones row is scaled by 2^-6 (16 and values near 2^-6, e = 2): conv5_kernel's range guard flags a row with |feat|^2 >
    65504^2, which 1024 * 4094 / 256 per channel passes; the max-pool kernel has no guard and gets the row as it is."""
    cin = CIN[arch]
    special = special_rows(cin, 1024.0 if arch == "epc-net-l" else 16.0)
    names = ["onehot:%d" % k for k in range(cin)] + ["-onehot:%d" % k for k in range(cin)] + list(special) + ["-" + s for s in special]
    rows = np.concatenate([onehot_rows(cin), np.stack(list(special.values())), -np.stack(list(special.values()))])
    rows.setflags(write=False)
    return names, rows
