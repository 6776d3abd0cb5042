"""The fp16 + MX-fp6 conv5 product of EPC_PRECISION_FAST -- pack_conv5_lo6_kernel, c5_to_fp6 / c5_load_operands and the four
v_mfma_scale_f32_32x32x64_f8f6f4 steps of c5_chunk_chain, in conv5_max_f16_kernel<128> (EPC-Net-L) and conv5_kernel<256> (EPC-Net) --
against the bit-level CPU emulation of tests/f16f6_ref.py.  The stage tests' bars (1e-3 of the tensor maximum) are looser than the
whole lo term (1.3e-4 of S when it is dropped); here the two entry points run alone, as in tests/test_gpu_stage_forms.py, on

  a. an EXACT family, compared with torch.equal: folded weights +-(H + l) with hi = +-H and lo = +-l = lo6 exactly and block scale
     bytes that differ between neighbouring blocks and lanes (f16f6_ref.exact_weights); clouds of one non-zero row and 31 zero rows:
     +-3 in every single channel (every (k, column) of the pack: the six-dword layout, the [lane][ks] scale byte, op_sel, the
     64ks + 32h channel map, with k-steps 2 and 3 at CIN = 256), rows of e2m3 midpoints under a 7.5 (the conversion's rounding
     direction), the next fp16 above 7.5 (the exponent's boundary), fp16 subnormals (the -12 clamp), one large value among small ones,
     four block scales in one row.  tests/test_f16f6_ref_cpu.py shows that every partial sum of these, in any order, is a float32, so
     accumulation contributes nothing, and that every mutant of the emulation changes a bit of what is compared here;
  b. a RANDOM family at the emulation's yardstick: rows_with_scales rounded to fp16 against seeded_weights(., 1).  The fold is
     computed in numpy float32 with the kernel's expression; a one-ulp disagreement of a folded weight (a contracted multiply-add in
     the bias, a differently rounded divide) moves a sum by less than 2^-23 S = 1.2e-7 S for the weights and as much for the bias, under
     3e-7 S together: far below T_rand.  Predicates: |pooled - emulated| <= T_rand max_points(S) / 256 per (cloud, channel);
     |feat16 - relu(acc) / 256| <= half an fp16 ulp of the emulated value + T_rand S / 256 per element; nothing is exempted;
  c. epc_conv5_assign_fwd(cat_fp16 = 0), the f32-row loader that no other caller reaches: equal, output for output, to the
     cat_fp16 = 1 call on the same rows rounded to fp16, and the one-hot sweep of (a) through it.

Numbers (S = |bias| + sum |x16 * hi| + sum |x6 * lo6| per element; all in units of S):
  yardstick -- the same terms accumulated in numpy float32 -- 1.27e-6 over the random cases; T_rand = 8 x yardstick = 1.01e-5
      (computed by f16f6_ref.t_rand(), not written into a test);
  the emulation against the ideal float64 product x16 . (W' * 256): 6.6e-6 (tests/test_f16f6_ref_cpu.py);
  the kernels against the emulation, measured on an MI355X: conv5 + max-pool 9.4e-8 (3 x 96) and 6.6e-8 (2 x 128), conv5 + assign
      2.1e-8 beyond the fp16 half-ulp (2 x 96); the matrix pipe alone (weights with lo = 0, full f32 sums read through one-row
      clouds) 1.0e-7 -- it accumulates better than the float32 yardstick.
What these tests found: 1.3e-5 .. 2.1e-5 on the same three cases, from 9 of 131072 weights.  pack_conv5_lo6_kernel recomputed
fp16(w) to form lo, and hipcc fused that kernel's multiply into the conversion (v_fma_mixlo_f16: one rounding of the exact product)
while fold_pack_conv5_kernel converts the f32 product; where the f32 product is an fp16 tie the two took different neighbours and
hi + lo was a whole fp16 ulp off.  The pack now reads the stored hi back (csrc/pack.hip); tests/test_f16f6_ref_cpu.py keeps such
ties among the random family's weights."""
import functools

import numpy as np
import pytest
import torch

import f16f6_ref as F
import helpers as H
import stage_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; there is no CPU fallback"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _engine(arch, family, dev):
    w = F.exact_weights(arch) if family == "exact" else F.seeded(arch)
    eng, _ = H.make_engine(arch, w, dev, precision="fast")
    return eng


def _t(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(dev).to(dtype)


def _with_slack(a, dtype, dev, rows=8 * R.TILE):
    """The rows `a` as a device tensor of `dtype` with `rows` rows of zeros behind it (a kernel's inactive waves)."""
    buf = torch.zeros((a.shape[0] + rows, a.shape[1]), dtype=dtype, device=dev)
    buf[:a.shape[0]] = torch.from_numpy(np.array(a)).to(dev).to(dtype)
    return buf[:a.shape[0]]


def _clouds_of_one_row(rows):
    """(R, cin) -> (32 R, cin): every row as row 0 of a cloud of 32 points, the other 31 zero."""
    x = np.zeros((rows.shape[0], 32, rows.shape[1]))
    x[:, 0] = rows
    return x.reshape(-1, rows.shape[1])


def _maxpool(dev, family, x, nc, n, dtype=torch.float16):
    """epc_conv5_maxpool_f16_fwd alone on the rows x (nc * n, 128) -> pooled (nc, 1024) float32 tensor."""
    L = H.pkg("lib")
    eng = _engine("epc-net-l", family, dev)
    cfg, packed, off = R.stage_pack(L, eng, n)
    assert eng.resolved_precision == "fast"
    cat = _with_slack(x, dtype, dev)
    assert np.array_equal(cat.double().cpu().numpy(), x), "the rows are fp16 values"
    pooled = R.Poisoned((nc, 1024), torch.float32, dev, 1)
    L.check(L.lib().epc_conv5_maxpool_f16_fwd(cat.data_ptr(), 128, off(5), nc, n, pooled.t.data_ptr(), L.current_stream()))
    torch.cuda.synchronize()
    assert pooled.untouched(), "a write behind pooled"
    assert bool(torch.isfinite(pooled.t).all())
    return pooled.t


def _conv5_assign(dev, family, x, nc, n, cat_fp16):
    """epc_conv5_assign_fwd alone on the rows x (nc * n, 256), given as fp16 (cat_fp16 = 1) or f32 rows -> dict of its outputs
    (feat decoded to (M, 1024) float32 and the raw fragments)."""
    L = H.pkg("lib")
    eng = _engine("epc-net", family, dev)
    cfg, packed, off = R.stage_pack(L, eng, n)
    assert eng.resolved_precision == "fast"
    M, tiles = nc * n, nc * n // 32
    cat = _with_slack(x, torch.float16 if cat_fp16 else torch.float32, dev)
    featf = R.Poisoned((tiles, 32, 2, 64, 8), torch.float16, dev, 1)
    assignf = R.Poisoned((tiles, 2, 2, 64, 8), torch.float16, dev, 1)
    rnorm = R.Poisoned((M,), torch.float32, dev)
    assign = R.Poisoned((M, 64), torch.float32, dev)
    apart = R.Poisoned((tiles, 64), torch.float32, dev, 1)
    status = torch.zeros((nc,), dtype=torch.int32, device=dev)
    L.check(L.lib().epc_conv5_assign_fwd(cat.data_ptr(), 1 if cat_fp16 else 0, 256, off(5), M, n, featf.t.data_ptr(), rnorm.t.data_ptr(),
                                         assign.t.data_ptr(), assignf.t.data_ptr(), apart.t.data_ptr(), status.data_ptr(),
                                         L.current_stream()))
    torch.cuda.synchronize()
    out = dict(featf=featf.t, rnorm=rnorm.t, assign=assign.t, assignf=assignf.t, apart=apart.t)
    for name, p in (("featf", featf), ("assignf", assignf), ("rnorm", rnorm), ("assign", assign), ("apart", apart)):
        assert p.untouched(), "%s: a write behind the buffer" % name
        assert bool(torch.isfinite(out[name].float()).all()), "%s: not every element was written" % name
    assert int(status.abs().sum()) == 0
    out["feat"] = R.decode_feat_f16(featf.t, M)
    return out


# ---- a. the exact family -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_emulation(arch):
    names, rows = F.exact_rows(arch)
    acc, _ = F.emulate(rows, F.exact_pack(arch))
    return names, rows, acc


def _first_difference(got, want, names, per):
    bad = (got != want).nonzero()
    i, c = int(bad[0, 0]), int(bad[0, 1])
    return "%d values differ; first: %s column %d: %r, emulation %r" % (bad.shape[0], names[i // per], c, float(got[i, c]), float(want[i, c]))


def test_maxpool_on_the_exact_family_is_the_emulation_bit_for_bit(dev):
    """Every (k, column) of hi and lo6 through +-3 one-hot rows, the tie and boundary rows; a cloud's pooled row is
    relu(acc of its one row) / 256 (the zero rows contribute the zero bias)."""
    names, rows, acc = _exact_emulation("epc-net-l")
    nc = rows.shape[0]
    assert nc == 2 * 128 + 2 * 8
    pooled = _maxpool(dev, "exact", _clouds_of_one_row(rows), nc, 32)
    want = _t(F.pooled_of(acc, nc, 1), dev)
    assert want.double().cpu().numpy().tolist() == F.pooled_of(acc, nc, 1).tolist()      # float32 holds the emulation exactly
    assert torch.equal(pooled, want), _first_difference(pooled, want, names, 1)


def _check_feat_family(dev, out, names, rows, acc):
    nc = rows.shape[0]
    feat16, ss, rnorm = F.feat_of(acc)
    want = torch.zeros((nc, 32, 1024), dtype=torch.float32, device=dev)
    want[:, 0] = _t(feat16, dev)
    want = want.reshape(-1, 1024)
    assert torch.equal(out["feat"], want), _first_difference(out["feat"], want, names, 32)
    # rnorm: the kernel sums 1024 squares of exact values in float32 (in its own order): 1024 * 2^-24 relative on the sum, half of
    # that and two roundings on its inverse root -- inside 1024 * 2^-24.  The zero rows sit at the 1e-12 floor.
    rn = np.full((nc, 32), 1.0 / np.sqrt(1e-12))
    rn[:, 0] = rnorm
    err = float(np.abs(out["rnorm"].double().cpu().numpy() / rn.reshape(-1) - 1.0).max())
    print("rnorm against the emulation's sum of squares: %.3e (bound %.3e)" % (err, 1024 * F.U32))
    assert err <= 1024 * F.U32


def test_conv5_assign_on_the_exact_family_is_the_emulation_bit_for_bit(dev):
    """The same sweep at CIN = 256 -- k-steps 2 and 3 and bytes 2 and 3 of the scale dwords, which only this kernel has -- through the
    fp16 feat: decode_feat_f16(feat) == fp16(relu(acc)) / 256 bit for bit (an eleventh of the non-zero values change when lo is
    dropped: the fp16 store does not hide it), status 0, rnorm to the float32 bound of its sum."""
    names, rows, acc = _exact_emulation("epc-net")
    nc = rows.shape[0]
    assert nc == 2 * 256 + 2 * 13
    out = _conv5_assign(dev, "exact", _clouds_of_one_row(rows), nc, 32, cat_fp16=1)
    _check_feat_family(dev, out, names, rows, acc)


# ---- b. the random family ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc,n", [(3, 96), (2, 128)])
def test_maxpool_on_random_rows_at_the_emulations_yardstick(dev, nc, n):
    """3 x 96: workgroups of four tiles that straddle clouds (per-wave atomics); 2 x 128: one-cloud workgroups (maxima meet in LDS)."""
    assert ("epc-net-l", nc, n) in F.RANDOM_CASES
    x = F.random_rows("epc-net-l", nc, n)
    acc, S = F.random_emulation("epc-net-l", nc, n)
    T = F.t_rand()
    got = _maxpool(dev, "random", x, nc, n).double().cpu().numpy()
    excess = F.pooled_excess(got, acc, S, nc, n)
    print("conv5 + max-pool %d x %d: worst |pooled - emulation| / max_points(S) %.3e   yardstick %.3e   T_rand %.3e" % (
        nc, n, excess, F.yardstick(), T))
    assert excess <= T


def test_conv5_assign_on_random_rows_at_the_emulations_yardstick(dev):
    nc, n = 2, 96
    assert ("epc-net", nc, n) in F.RANDOM_CASES
    x = F.random_rows("epc-net", nc, n)
    acc, S = F.random_emulation("epc-net", nc, n)
    T = F.t_rand()
    got = _conv5_assign(dev, "random", x, nc, n, cat_fp16=1)["feat"].double().cpu().numpy()
    excess = F.feat_excess(got, acc, S)
    f = np.maximum(acc, 0.0) / F.W5_SCALE
    print("conv5 + assign %d x %d: worst (|feat16 - emulation| - half an fp16 ulp) / S %.3e   (|feat16 - fp16(emulation)| / S %.3e)   "
          "yardstick %.3e   T_rand %.3e" % (nc, n, excess, float((np.abs(got - F.to_f16(f)) / (S / F.W5_SCALE)).max()), F.yardstick(), T))
    assert excess <= T


# ---- c. the f32-row loader -----------------------------------------------------------------------------------------------------------------
OUTPUTS = ("featf", "rnorm", "assign", "assignf", "apart")


def test_conv5_assign_from_f32_rows_equals_the_fp16_row_call(dev):
    """launch_conv5<256, false>: f32 rows that are NOT fp16 values, rounded on load, with its own fp6 gather at 64ks + 32h + 4w8 --
    every output equal to the cat_fp16 = 1 call on the rows rounded to fp16 first."""
    nc, n = 2, 96
    x32 = R.rows_with_scales(np.random.RandomState(31), nc * n, 256, cloud_scale=np.arange(1, nc + 1), n=n)
    x16 = F.to_f16(x32)
    assert float((x16 != x32).mean()) > 0.99
    a = _conv5_assign(dev, "random", x32, nc, n, cat_fp16=0)
    b = _conv5_assign(dev, "random", x16, nc, n, cat_fp16=1)
    for name in OUTPUTS:
        assert torch.equal(a[name], b[name]), name


def test_conv5_assign_from_f32_rows_on_the_one_hot_sweep(dev):
    names, rows, acc = _exact_emulation("epc-net")
    k = 2 * 256
    out = _conv5_assign(dev, "exact", _clouds_of_one_row(rows[:k]), k, 32, cat_fp16=0)
    _check_feat_family(dev, out, names[:k], rows[:k], acc[:k])
