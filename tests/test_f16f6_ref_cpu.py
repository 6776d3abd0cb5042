"""tests/f16f6_ref.py -- the CPU emulation of the fp16 + MX-fp6 conv5 product that tests/test_gpu_f16f6_product.py holds the kernels to
-- is right and can tell: its quantiser and block-exponent rule against their definitions, the whole emulation against the ideal
float64 product, its exact family exact, and every deliberately wrong variant of it (f16f6_ref.mutants) caught by the predicates the
GPU tests apply.  No GPU.

Measured here (seeded_weights(., 1), rows_with_scales rounded to fp16; errors relative to S = |bias| + sum |x16 * hi| + sum |x6 * lo6|):
  emulation against the ideal product x16 . (W' * 256): worst 6.6e-6 (5.1e-6, 6.6e-6, 3.6e-6 on the three random cases) -- inside
      the 2^-15 = 3.1e-5 that csrc/common.h claims for the lo term's e2m3 rounding;
  yardstick (the same terms accumulated in float32): 1.27e-6, so T_rand = 8 x that = 1.01e-5;
  mutants on the random predicates, worst case of the three, in units of T_rand: lo dropped 8.7, lo of the first / last block
      dropped 5.9 / 5.8, weight scale of block b +- 1: 8.1 / 7.4, activation scale likewise 5.4 / 5.5, x6 reversed 14.8, halves of a
      k-step exchanged 11.8, exponent without the round-up 3.3, fp6 rounding toward zero 0.9.
The last two are too small for ANY bar relative to S that leaves the matrix pipe's accumulation room (toward-zero rounding moves a
product by at most half an e2m3 step of a 2^-11 correction: under 4.5e-5 of a single term, about 1e-5 of a sum): what pins them is
the exact family, where accumulation contributes nothing -- every partial sum is a float32 -- and one changed bit is a verdict."""
import numpy as np
import pytest

import f16f6_ref as F
import helpers  # noqa: F401  (puts the oracle on the path)

EMUL_VS_IDEAL = 6.6e-6       # measured (docstring); asserted with a 2x margin
# the mutants that the random family's max-pool cases must catch at >= 4 T_rand (at CIN = 256 one block is an eighth of the lo term:
# 3.3 T_rand when it is dropped); the exact family must catch ALL
RANDOM_CATCHES = ("lo_dropped", "lo_block_dropped", "w_scale_from", "x_scale_from", "x6_reversed", "w_halves_swapped")


# ---- quantiser ---------------------------------------------------------------------------------------------------------------------------
def test_e2m3_codes_round_trip_ties_go_to_even_and_saturate():
    assert F.DECODE.shape == (64,)
    want = ([0.125 * i for i in range(16)] + [2.0 + 0.25 * i for i in range(8)] + [4.0 + 0.5 * i for i in range(8)])
    assert F.MAGS.tolist() == want and F.MAGS[-1] == 7.5
    codes = np.arange(64, dtype=np.uint8)
    assert np.array_equal(F.q6_codes(F.DECODE), codes)                   # every code, -0.0 (code 32) included
    assert np.array_equal(F.q6_codes(F.DECODE, rtz=True), codes)
    z = F.q6(np.array([-0.0, 0.0]))
    assert np.signbit(z).tolist() == [True, False] and not z.any()
    # every midpoint between neighbouring magnitudes goes to the neighbour with the even mantissa, both signs
    mid = (F.MAGS[:-1] + F.MAGS[1:]) / 2
    even = np.where(np.arange(31) % 2 == 0, F.MAGS[:-1], F.MAGS[1:])
    assert np.array_equal(F.q6(mid), even) and np.array_equal(F.q6(-mid), -even)
    assert np.array_equal(F.q6_codes(mid) & 1, np.zeros(31, dtype=np.uint8))
    assert np.array_equal(F.q6(mid, rtz=True), F.MAGS[:-1])
    # just off a midpoint: to the nearer one
    assert np.array_equal(F.q6(mid + 2.0 ** -12), F.MAGS[1:]) and np.array_equal(F.q6(mid - 2.0 ** -12), F.MAGS[:-1])
    assert F.q6(np.array([7.75, 1e4, -7.75, -1e4, 7.5])).tolist() == [7.5, 7.5, -7.5, -7.5, 7.5]
    assert F.q6(np.array([1e4]), rtz=True).tolist() == [7.5]


# ---- block exponent ------------------------------------------------------------------------------------------------------------------------
def _search(m, lo_e, hi_e):
    """The smallest e with float32(m * (1 / 7.5f)) <= 2^e, clamped; also whether the clamp acted."""
    p = float(np.float32(m) * (np.float32(1.0) / np.float32(7.5)))
    e = next(e for e in range(-200, 200) if p <= 2.0 ** e)
    return min(max(e, lo_e), hi_e), not lo_e <= e <= hi_e


def test_block_exponent_integer_rule_against_a_search():
    ms = [0.0]
    for e in range(-12, 14):
        m = np.float16(7.5 * 2.0 ** e)
        assert float(m) == 7.5 * 2.0 ** e
        ms += [float(m), float(np.nextafter(m, np.float16(np.inf))), float(np.nextafter(m, np.float16(0)))]
    ms += [2.0 ** -24, 2.0 ** -15, 1023 * 2.0 ** -24, 65504.0, 1.0, 3.0, 0.875, 0.4375, 1e-35, 1e-41, 7.5 * 2.0 ** -100, 1e8, 7.5 * 2.0 ** 20]
    rng = np.random.RandomState(0)
    ms += (rng.randn(200).astype(np.float16).astype(np.float64) * 2.0 ** rng.randint(-10, 10, 200)).tolist()
    # lo parts as the pack sees them: f32 values of at most 13 significant bits
    ms += (rng.randint(1, 8192, 200) * 2.0 ** rng.randint(-30, 0, 200)).tolist()
    for lo_e, hi_e in ((-12, 14), (-100, 20)):
        for m in ms:
            m = abs(m)
            e = int(F.block_exponent(np.array([m]), lo_e, hi_e)[0])
            want, clamped = _search(m, lo_e, hi_e)
            assert e == want, (m, lo_e, hi_e, e, want)
            if not clamped:
                assert float(np.float32(m)) * 2.0 ** -e <= 7.5, (m, e)
                assert m == 0 or float(np.float32(m)) * 2.0 ** -e > 3.75, (m, e)
    assert F.block_exponent(np.array([0.0]), -12, 14)[0] == -12 and F.block_exponent(np.array([0.0]), -100, 20)[0] == -100
    assert F.block_exponent(np.array([2.0 ** -24]), -12, 14)[0] == -12 and F.block_exponent(np.array([1e8]), -100, 20)[0] == 20
    assert F.block_exponent(np.array([7.5]), -12, 14)[0] == 0 and F.block_exponent(np.array([F.NEXT_ABOVE_MAX]), -12, 14)[0] == 1
    assert F.block_exponent(np.array([65504.0]), -12, 14)[0] == 14
    # the mutant: no step up for a set mantissa bit
    assert F.block_exponent(np.array([3.0]), -12, 14)[0] == -1 and F.block_exponent(np.array([3.0]), -12, 14, round_up=False)[0] == -2


# ---- the emulation against the ideal product -------------------------------------------------------------------------------------------------
def test_emulation_against_the_ideal_product():
    """The emulated sum against x16 . (W' * 256) + bias * 256 in float64: what the weight representation (fp16 hi + e2m3 lo, fp6 inputs
    on the lo term) costs -- csrc/common.h's 2^-15 claim -- measured, printed and held to twice the measured figure."""
    worst = 0.0
    for arch, nc, n in F.RANDOM_CASES:
        x = F.random_rows(arch, nc, n)
        acc, S = F.random_emulation(arch, nc, n)
        W64, b64 = F.fold_f64(F.seeded(arch))
        err = float((np.abs(acc - (b64[None, :] + x @ W64)) / S).max())
        print("emulation against the ideal product, %s %d x %d: worst error / S %.3e" % (arch, nc, n, err))
        worst = max(worst, err)
    assert worst <= 2.0 ** -15
    assert worst <= 2 * EMUL_VS_IDEAL


def test_the_f32_fold_is_the_ideal_fold_to_f32_rounding():
    for arch in ("epc-net-l", "epc-net"):
        wf, bf = F.fold_f32(F.seeded(arch))
        W64, b64 = F.fold_f64(F.seeded(arch))
        assert wf.dtype == np.float32 and bf.dtype == np.float32
        assert float(np.abs(wf / W64 - 1.0).max()) <= 4 * 2.0 ** -24           # sqrt, divide, two multiplies
        assert float(np.abs(bf - b64).max()) <= 8 * 2.0 ** -24 * float(np.abs(b64).max() + 256.0)


def test_the_random_family_holds_weights_on_an_fp16_tie():
    """A folded weight whose f32 value lies exactly between two fp16 values is where a pack that rounds hi twice -- once for the hi
    fragment, once to form lo -- can take two different neighbours (it did: one rounded the f32 product, the other the exact one),
    leaving hi + lo an fp16 ulp off.  The random family must keep such weights, and such a pack must fail its predicates (on the GPU it
    did, at 1.3 .. 2.1 T_rand; the fixed kernels sit at 0.01 T_rand)."""
    T = F.t_rand()
    for arch, nc, n in F.RANDOM_CASES:
        p = F.seeded_pack(arch)
        tie = np.abs(p.lo) == 0.5 * np.spacing(np.abs(p.hi).astype(np.float16)).astype(np.float64)
        assert tie.sum() >= 8, (arch, int(tie.sum()))
        # the other neighbour as hi, lo left as it was
        bad = F.seeded_pack(arch)
        bad = type("P", (), dict(vars(bad)))()
        bad.hi = np.where(tie, p.hi + 2 * p.lo, p.hi)
        acc, S = F.random_emulation(arch, nc, n)
        macc, _ = F.emulate(F.random_rows(arch, nc, n), bad)
        excess = (F.pooled_excess(F.pooled_of(macc, nc, n), acc, S, nc, n) if arch == "epc-net-l" else
                  F.feat_excess(F.feat_of(macc)[0], acc, S))
        print("%s: %d weights on an fp16 tie; the other neighbour as hi: %.1f T_rand" % (arch, int(tie.sum()), excess / T))
        assert excess > T


# ---- separation ----------------------------------------------------------------------------------------------------------------------------
def _exact_outputs(arch, mutant=None):
    """What the GPU tests compare bit for bit on the exact family, from the (mutated) emulation: pooled (a cloud = one row and 31 zero
    rows: relu(acc) / 256) for EPC-Net-L, feat16 for EPC-Net."""
    _, rows = F.exact_rows(arch)
    acc, _ = F.emulate(rows, F.exact_pack(arch, mutant), mutant)
    return F.pooled_of(acc, rows.shape[0], 1) if arch == "epc-net-l" else F.feat_of(acc)[0]


def test_every_mutant_is_caught_by_the_gpu_tests_predicates():
    """T_rand from the yardstick; every mutant through the random family's predicates (an excess of >= 4 T_rand counts as caught: the
    kernels are allowed T_rand) and through the exact family's (one changed bit).  RANDOM_CATCHES must be caught by the random family,
    every mutant by the exact one; one that neither tells apart fails."""
    y, T = F.yardstick(), F.t_rand()
    print("yardstick %.3e  T_rand %.3e" % (y, T))
    assert T == 8 * y and 1e-7 < y < 1e-5
    for cin_arch in ("epc-net-l", "epc-net"):
        for m in F.mutants(F.CIN[cin_arch]):
            worst = 0.0
            for arch, nc, n in F.RANDOM_CASES:
                if arch != cin_arch:
                    continue
                acc, S = F.random_emulation(arch, nc, n)
                macc, _ = F.emulate(F.random_rows(arch, nc, n), F.seeded_pack(arch, m), m)
                if arch == "epc-net-l":
                    worst = max(worst, F.pooled_excess(F.pooled_of(macc, nc, n), acc, S, nc, n))
                else:
                    worst = max(worst, F.feat_excess(F.feat_of(macc)[0], acc, S))
            changed = float((_exact_outputs(cin_arch, m) != _exact_outputs(cin_arch)).mean())
            print("%-9s %-24s random: %5.1f T_rand   exact: %.4f of the outputs change" % (cin_arch, m, worst / T, changed))
            assert worst >= 4 * T or changed > 0, "%s %s: no predicate tells it from the emulation" % (cin_arch, m)
            if m.split(":")[0] in RANDOM_CATCHES and cin_arch == "epc-net-l":
                assert worst >= 4 * T, (cin_arch, m, worst / T)
    # the emulation itself passes its own predicates at zero
    acc, S = F.random_emulation(*F.RANDOM_CASES[0])
    assert F.pooled_excess(F.pooled_of(acc, 3, 96), acc, S, 3, 96) == 0.0
    acc, S = F.random_emulation(*F.RANDOM_CASES[2])
    assert F.feat_excess(F.feat_of(acc)[0], acc, S) <= 0.0
    # ... and the float32-accumulated yardstick passes them at T_rand
    a32 = F.emulate_f32(F.random_rows(*F.RANDOM_CASES[2]), F.seeded_pack("epc-net"))
    assert F.feat_excess(F.feat_of(a32)[0], acc, S) <= T


# ---- the exact family ------------------------------------------------------------------------------------------------------------------------
def test_exact_fold_facts():
    one = np.float32(0.999) + np.float32(1e-3)
    assert one == np.float32(1.0) and np.float32(1.0) / np.sqrt(one) == np.float32(1.0)


@pytest.mark.parametrize("arch", ["epc-net-l", "epc-net"])
def test_exact_family_is_exact_and_every_mutant_changes_a_bit(arch):
    cin = F.CIN[arch]
    nb = cin // 32
    p = F.exact_pack(arch)
    # the weights: hi = +-H, lo = +-l, lo6 == lo, zero bias; scale bytes differ between neighbouring blocks and columns
    assert np.array_equal(p.lo6, p.lo) and not p.bias.any()
    H = np.abs(p.hi)
    assert H.min() >= 2050 and H.max() <= 4094 and not (H % 2).any()
    assert np.abs(p.lo).max() == 0.875 and not ((p.lo * 32) % 1).any()
    assert not p.lo[:, F.ZERO_LO_COL].any() and (p.we[:, F.ZERO_LO_COL] == -100).all()
    cols = np.arange(1024) != F.ZERO_LO_COL
    we = p.we[:, cols]
    assert set(np.unique(we)) == {-3, -4, -5}
    assert np.array_equal(we, (-3 - (np.arange(1024)[None, cols] + np.arange(nb)[:, None]) % 3))
    assert (we[:-1] != we[1:]).all() and (we[:, :-1] != we[:, 1:]).all()
    if nb == 8:   # bytes 2 and 3 of a lane's scale dword (k-steps 2, 3; lane half h feeds block 2 ks + h) differ from each other and byte 0, 1
        for h in range(2):
            assert (we[4 + h] != we[6 + h]).all() and (we[h] != we[4 + h]).all() and (we[2 + h] != we[6 + h]).all()
    wf, _ = F.fold_f32(F.exact_weights(arch))
    assert np.array_equal(wf.astype(np.float64), p.hi + p.lo)
    # the rows: x6 exact where intended
    names, rows = F.exact_rows(arch)
    assert len(names) == rows.shape[0] and len(set(names)) == len(names)
    x6, xe = F.rows_fp6(rows)
    for i, name in enumerate(names):
        kind = name.lstrip("-").split(":")[0]
        if kind in ("onehot", "block_scales"):
            assert np.array_equal(x6[i], rows[i]), name
        elif kind == "big_and_ones":
            big = np.abs(rows[i]).max()
            assert np.array_equal(x6[i], np.where(np.abs(rows[i]) == big, rows[i], 0.0)), name
            assert big == (1024.0 if arch == "epc-net-l" else 16.0) and xe[i].max() == (8 if arch == "epc-net-l" else 2)
        elif kind == "ties":
            b = int(name.split(":")[1])
            assert xe[i, b] == 0 and (np.delete(xe[i], b) == -12).all()
            nz = rows[i] != 0
            assert nz.sum() == 8 and np.array_equal(np.sort(np.abs(x6[i, nz])), [4.0, 5.0, 5.0, 6.0, 6.0, 7.0, 7.0, 7.5])
            assert np.array_equal(np.sort(np.abs(F.rows_fp6(rows[i:i + 1], "fp6_rtz")[0][0, nz])), [4.0, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0, 7.5])
        elif kind == "above_7.5":
            assert xe[i, 1] == 1 and np.array_equal(np.sort(np.abs(x6[i, rows[i] != 0])), [4.0, 5.0, 5.0, 6.0, 7.5])
        elif kind == "subnormals":
            nz = rows[i] != 0
            assert (xe[i] == -12).all() and np.abs(rows[i]).max() < 2.0 ** -14
            assert np.array_equal(np.abs(x6[i, nz]) * 2.0 ** 12, [0.0, 0.0, 0.125, 0.125, 0.125, 0.25, 0.25])
        else:
            raise AssertionError(name)
    for q in range(nb // 4):
        i = names.index("block_scales:%d" % q)
        assert np.array_equal(xe[i, 4 * q:4 * q + 4], [-6, -4, -2, 0]) and (np.delete(xe[i], range(4 * q, 4 * q + 4)) == -12).all()
    # every term and every partial sum, in any order, is a float32: they are multiples of the row's coarsest common power of two,
    # and sum |terms| stays under 2^24 of those (the one-hot rows have one hi and one lo term: a sample of them is enough)
    special = [i for i, name in enumerate(names) if "onehot" not in name]
    for i in special + list(range(0, 2 * cin, 37)):
        t = F.terms(rows[i:i + 1], p)[0]
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t), names[i]
        ratio = float((np.abs(t).sum(0) / F.lowest_bit(t).min(0)).max())
        assert ratio < 2.0 ** 24, (names[i], ratio / 2.0 ** 24)
    acc, _ = F.emulate(rows, p)
    assert np.array_equal(acc.astype(np.float32).astype(np.float64), acc)
    assert np.array_equal(F.emulate_f32(rows[special], p), acc[special])          # one particular float32 order, for the record
    # the range guard of conv5_kernel (|feat row|^2 <= 65504^2) holds on every row of the EPC-Net family
    if arch == "epc-net":
        assert float(F.feat_of(acc)[1].max()) <= 0.5 * 65504.0 ** 2
    # each mutant changes at least one bit of what the GPU test compares
    base = _exact_outputs(arch)
    for m in F.mutants(cin):
        assert not np.array_equal(_exact_outputs(arch, m), base), m
