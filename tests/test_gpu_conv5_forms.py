"""The f32 conv5 + assignment kernel's two forms (epcnet_conv5_assign_f32_fwd_form, include/epcnet_forms.h) against each other, byte for
byte: form 0 is the kernel as it stood, form 1 what epc_conv5_assign_f32_fwd and the pipeline launch (streaming hints on the
once-touched bytes, packed bf16 conversions, one table base and a wave-uniform store base in the epilogue).  Nothing in form 1
changes an operand, a rounding or the order of a sum, so feat, rnorm, assign, the assignment fragments and the a_sum partials must
agree in every bit -- tests/test_gpu_stage_forms.py holds the shipped form against the float64 restatement.

Shapes, the smallest at which the changed code can go wrong:
  * 9 x 32: 9 tiles -- a second workgroup with one active and seven inactive waves: both vmcnt branches, early and late waves;
  * 3 x 96: an odd tile count;
  * 2 x 2304: 18 full workgroups -- every wave active, several workgroups per XCD;
  * 1 x 32: one active wave in the grid.
Inputs: rows whose scales span 2^12 (stage_ref.rows_with_scales), one all-zero row, one row with a NaN and one with an Inf: the ReLU
works on the bit pattern and must leave a NaN a NaN, so bytes are compared, not values.  Outputs are poisoned and allocated with
slack; the buffers are compared whole, so a write outside an output's extent shows as well."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
import stage_ref as R
from test_gpu_stage_forms import _engine, _with_slack

pytestmark = pytest.mark.gpu

SHAPES = [(9, 32), (3, 96), (2, 2304), (1, 32)]
NAMES = ("feat", "assign fragments", "rnorm", "assign", "apart")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; there is no CPU fallback"
    return torch.device("cuda:0")


def _special_rows(M):
    """(all-zero row, row with a NaN, row with an Inf): three different rows, in different tiles where there is more than one."""
    return 3, (M // 3) | 1, M - 5


@functools.lru_cache(maxsize=None)
def _case(nc, n):
    """(cat with slack behind it, the packed weights -- kept alive --, the address of the conv5 stage)."""
    dev = torch.device("cuda:0")
    L = H.pkg("lib")
    _, packed, off = R.stage_pack(L, _engine("epc-net", dev, "f32"), n)
    M = nc * n
    cat_np = R.rows_with_scales(np.random.RandomState(1000 * nc + n), M, 256, cloud_scale=np.arange(1, nc + 1), n=n)
    zero, nan, inf = _special_rows(M)
    assert len({zero, nan, inf}) == 3
    cat_np[zero] = 0.0
    cat_np[nan, 77] = np.nan
    cat_np[inf, 200] = np.inf
    scales = np.abs(cat_np[np.isfinite(cat_np).all(1)]).max(1)
    assert scales[scales > 0].max() / scales[scales > 0].min() >= 2.0 ** 8 or M == 32
    return _with_slack(cat_np, torch.float32, dev), packed, off(5)


def _launch(form, nc, n, with_assign=True):
    """One launch of the named form into poisoned buffers: the five Poisoned outputs in the order of NAMES."""
    L = H.pkg("lib")
    cat, _, pack5 = _case(nc, n)
    dev = cat.device
    M, tiles = nc * n, nc * n // 32
    featf = R.Poisoned((tiles, 32, 3, 64, 16), torch.uint8, dev, 1)
    assignf = R.Poisoned((tiles, 2, 2, 2, 64, 8), torch.bfloat16, dev, 1)
    rnorm = R.Poisoned((M,), torch.float32, dev)
    assign = R.Poisoned((M, 64), torch.float32, dev)
    apart = R.Poisoned((tiles, 64), torch.float32, dev, 1)
    L.check(L.lib().epcnet_conv5_assign_f32_fwd_form(cat.data_ptr(), 256, pack5, M, featf.t.data_ptr(), rnorm.t.data_ptr(),
                                                     assign.t.data_ptr() if with_assign else None, assignf.t.data_ptr(),
                                                     apart.t.data_ptr(), form, L.current_stream()))
    torch.cuda.synchronize()
    return featf, assignf, rnorm, assign, apart


def _assert_same_bytes(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        assert x.untouched() and y.untouched(), "%s: %s: a write behind the buffer" % (what, name)
        assert torch.equal(x.buf, y.buf), "%s: %s differs" % (what, name)


@pytest.mark.parametrize("with_assign", [True, False], ids=["assign", "noassign"])
@pytest.mark.parametrize("nc,n", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_conv5_forms_agree_byte_for_byte(dev, nc, n, with_assign):
    M = nc * n
    old, new = _launch(0, nc, n, with_assign), _launch(1, nc, n, with_assign)
    _assert_same_bytes(old, new, "form 0 against form 1")
    featf, assignf, rnorm, assign, apart = new
    if not with_assign:
        assert R.holds_poison(assign.t), "the optional assign copy was written without a pointer to it"
    # every element was written: rows and tiles without the NaN and the Inf are finite.  (What the two rows themselves become is the
    # matrix pipe's business -- its NaN carries a sign, which the bit-pattern ReLU keeps or clears -- and is pinned by the byte
    # comparison above: whatever form 0 leaves there, form 1 leaves too.)
    zero, nan, inf = _special_rows(M)
    plain = np.ones(M, dtype=bool)
    for r in (nan, inf):
        plain[r // 32 * 32:r // 32 * 32 + 32] = False       # rnorm, the assignment and apart mix a tile's points only through apart
    feat = R.decode_feat_b3(featf.t, M)
    rows_ok = torch.from_numpy(np.setdiff1d(np.arange(M), [nan, inf])).to(dev)
    assert bool(torch.isfinite(feat[rows_ok]).all()) and bool(torch.isfinite(rnorm.t[rows_ok]).all())
    tiles_ok = torch.from_numpy(np.nonzero(plain.reshape(-1, 32).all(1))[0]).to(dev)
    assert bool(torch.isfinite(apart.t[tiles_ok]).all())
    if with_assign:
        assert bool(torch.isfinite(assign.t[rows_ok]).all())
    # the all-zero row: feat = relu(bias), finite and the same whatever the row's neighbours are
    assert bool(torch.isfinite(feat[zero]).all()) and float(rnorm.t[zero]) > 0.0


def test_conv5_shipped_form_is_what_the_entry_launches_and_repeats(dev):
    """Form 1 twice, and epc_conv5_assign_f32_fwd itself: equal bytes (9 x 32: active and inactive, early and late waves)."""
    nc, n = 9, 32
    L = H.pkg("lib")
    first, second = _launch(1, nc, n), _launch(1, nc, n)
    _assert_same_bytes(first, second, "form 1 twice")
    cat, _, pack5 = _case(nc, n)
    M, tiles = nc * n, nc * n // 32
    featf = R.Poisoned((tiles, 32, 3, 64, 16), torch.uint8, dev, 1)
    assignf = R.Poisoned((tiles, 2, 2, 2, 64, 8), torch.bfloat16, dev, 1)
    rnorm = R.Poisoned((M,), torch.float32, dev)
    assign = R.Poisoned((M, 64), torch.float32, dev)
    apart = R.Poisoned((tiles, 64), torch.float32, dev, 1)
    L.check(L.lib().epc_conv5_assign_f32_fwd(cat.data_ptr(), 256, pack5, M, featf.t.data_ptr(), rnorm.t.data_ptr(), assign.t.data_ptr(),
                                             assignf.t.data_ptr(), apart.t.data_ptr(), L.current_stream()))
    torch.cuda.synchronize()
    _assert_same_bytes(first, (featf, assignf, rnorm, assign, apart), "form 1 against epc_conv5_assign_f32_fwd")


def test_conv5_form_entry_rejects_other_forms(dev):
    L = H.pkg("lib")
    cat, _, pack5 = _case(1, 32)
    outs = [R.Poisoned((1, 32, 3, 64, 16), torch.uint8, dev, 1), R.Poisoned((1, 2, 2, 2, 64, 8), torch.bfloat16, dev, 1),
            R.Poisoned((32,), torch.float32, dev), R.Poisoned((32, 64), torch.float32, dev), R.Poisoned((1, 64), torch.float32, dev)]
    featf, assignf, rnorm, assign, apart = outs
    for form in (-1, 2):
        rc = L.lib().epcnet_conv5_assign_f32_fwd_form(cat.data_ptr(), 256, pack5, 32, featf.t.data_ptr(), rnorm.t.data_ptr(),
                                                      assign.t.data_ptr(), assignf.t.data_ptr(), apart.t.data_ptr(), form,
                                                      L.current_stream())
        assert rc == L.EPC_EINVAL
    torch.cuda.synchronize()
    assert all(R.holds_poison(o.t) and o.untouched() for o in outs)
