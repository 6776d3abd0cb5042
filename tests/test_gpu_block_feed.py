"""The f32 ProxyConv block kernel's two forms (epcnet_block_fwd_form, include/epcnet_forms.h) against each other, bit for bit, and
against the float64 restatement of the block (tests/stage_ref.py) at the bar of tests/test_gpu_stage_forms.py.

Form 1 -- what epc_proxyconv_block_fwd launches -- decides per 32-point tile: a tile whose 32 lists all hold exactly 20 entries runs
the straight-line gather fed by the tile prologue (counts and lists in one coalesced load, lists parked in the staging tile),
every other tile the per-pass lookups, which are all of form 0.  test_gpu_stage_forms.py's clouds mix the list lengths inside every
pass, so no tile of theirs takes the new path; here a case's tiles are of ONE kind each:

  * uniform clouds: every count is 20 (every tile on the new path);
  * every point three times: the 20th entry falls inside a triple, counts of 21 and more up to the capacity (the tie loop);
  * the second half of the cloud zero-padded: more than 32 entries at distance 0 (the Kahan scan of the row) -- at 32 points a
    count cannot pass the capacity, and that cloud only checks the shape;
  * one launch whose clouds are of the three kinds at random, large enough that every wave of the persistent grid draws about
    three tiles: what the prologue left of the LAST tile (counts, lists, the parked rows) must not reach the present one.
    Which wave draws which tile is decided at run time, so the test cannot name the transitions it saw; with thousands of draws
    of three kinds every ordered pair of kinds follows each other in some wave.

Shapes: one tile (one wave busy), 3 x 96 (9 tiles, one workgroup), 2 x 160 (10 tiles, two tiles past a cloud boundary inside a
workgroup), and the smallest persistent one-workgroup-per-CU launch with a remainder; each with and without the next block's conv
and with 2-byte and 4-byte lists.  cat, x_next and the poison around them must be identical between the forms."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
import stage_ref as R
from helpers import O
from test_gpu_stage_forms import _engine, _f64, _rel, _weights, _with_slack, stage_tol

pytestmark = pytest.mark.gpu

SEED = 11
BLOCK = 1          # the first block: its pack holds conv2 as the next block's leading conv
OUT_OFF, CCAT = 64, 192
KINDS = ["uniform", "triples", "zeropad50"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; there is no CPU fallback"
    return torch.device("cuda:0")


def _clouds(nc, n, kind, seed=SEED):
    if kind == "triples":
        base = O.synthetic_clouds(nc, -(-n // 3), seed, "uniform")
        return np.ascontiguousarray(np.tile(base, (1, 3, 1))[:, :n])
    return O.synthetic_clouds(nc, n, seed, kind)


def _tile_kinds(cnt):
    """Per 32-point tile, from the kernel's own counts: 0 = every list holds 20 entries, 1 = some hold more and none overflows,
    2 = some overflow."""
    c = np.asarray(cnt).reshape(-1, R.TILE)
    return np.where((c > R.CAP).any(1), 2, np.where((c > 20).any(1), 1, 0))


def _launch(L, pack_addr, form, x, xyz, idx, u16, cnt, kth, knn, has_next):
    """epcnet_block_fwd_form (f32) alone, into poisoned buffers: R.launch_block with the form argument."""
    nc, n, _ = x.shape
    cat = R.Poisoned((nc * n, CCAT), torch.float32, x.device)
    nxt = R.Poisoned((nc * n, 64), torch.float32, x.device)
    lists = idx.clamp(0, 32767).to(torch.int16) if u16 else idx
    L.check(L.lib().epcnet_block_fwd_form(x.data_ptr(), None, xyz.data_ptr(), lists.data_ptr(), 1 if u16 else 0,
                                                 cnt.data_ptr(), kth.data_ptr(), R.CAP, pack_addr, has_next, nc, n, knn,
                                                 cat.t.data_ptr(), None, CCAT, OUT_OFF, nxt.t.data_ptr(), None, None, form,
                                                 L.current_stream()))
    torch.cuda.synchronize()
    return cat, nxt


@functools.lru_cache(maxsize=2)
def _case(nc, n, kind, ref_clouds=None):
    """The inputs of one (shape, kind) and its float64 reference (out, x_next) -- of the clouds `ref_clouds` (all when None) --
    computed once for the four (has_next, list format) launches."""
    dev = torch.device("cuda:0")
    L = H.pkg("lib")
    if isinstance(kind, str):
        pc = _clouds(nc, n, kind)
    else:                                    # a kind index per cloud
        per_kind = [_clouds(nc, n, k) for k in KINDS[:2] + ["zeropad75"]]
        pc = np.ascontiguousarray(np.stack([per_kind[k][c] for c, k in enumerate(kind)]))
    xyz = torch.from_numpy(pc).to(dev)
    idx, cnt, kth = R.knn_graph(L, xyz)
    torch.cuda.synchronize()
    x_np = R.rows_with_scales(np.random.RandomState(1000 + nc + n), nc * n, 64)
    x = _with_slack(x_np, torch.float32, dev).reshape(nc, n, 64)
    sel = np.arange(nc) if ref_clouds is None else np.asarray(ref_clouds)
    idx_c, cnt_c, kth_c = idx.cpu().numpy()[sel], cnt.cpu().numpy()[sel], kth.cpu().numpy()[sel]
    W = R.neighbour_sets(idx_c, cnt_c, O.neg_sq_dist(pc[sel]), kth_c)
    out_ref, nxt_ref = R.block_ref(R.state64(_weights("epc-net")), BLOCK, x_np.reshape(nc, n, 64)[sel].astype(np.float64), W, 20, True)
    return xyz, idx, cnt, kth, x, cnt.cpu().numpy(), sel, out_ref.reshape(-1, 64), nxt_ref.reshape(-1, 64)


@functools.lru_cache(maxsize=1)
def _pack():
    """(cfg, the packed weights -- kept alive here --, off(stage)) of one f32 EPC-Net engine: the block pack does not depend on the
    cloud size."""
    cfg, packed, off = R.stage_pack(H.pkg("lib"), _engine("epc-net", torch.device("cuda:0"), "f32"), 96)
    assert cfg.knn == 20
    return cfg, packed, off


def _check(dev, case, has_next, u16, what):
    xyz, idx, cnt, kth, x, cnt_c, sel, out_ref, nxt_ref = case
    nc, n, _ = x.shape
    L = H.pkg("lib")
    cfg, _, off = _pack()
    res = [_launch(L, off(BLOCK), form, x, xyz, idx, u16, cnt, kth, cfg.knn, has_next) for form in (0, 1)]
    (cat0, nxt0), (cat1, nxt1) = res
    rows = (sel[:, None] * n + np.arange(n)[None]).reshape(-1)
    for form, (cat, nxt) in enumerate(res):
        got = cat.t[:, OUT_OFF:OUT_OFF + 64]
        assert bool(torch.isfinite(got).all()), "form %d: rows of the concat slice were not written" % form
        e_out = _rel(got[rows], out_ref)
        e_nxt = _rel(nxt.t[rows], nxt_ref) if has_next else 0.0
        print("block form %d %s %d x %d has_next %d %s lists: out %.3e x_next %.3e" % (form, what, nc, n, has_next,
                                                                                      "2-byte" if u16 else "4-byte", e_out, e_nxt))
        assert e_out <= stage_tol(False) and e_nxt <= stage_tol(False)
        assert cat.untouched() and nxt.untouched(), "form %d: a write behind the last row" % form
        assert R.holds_poison(cat.t[:, :OUT_OFF]) and R.holds_poison(cat.t[:, OUT_OFF + 64:]), "form %d: a write outside the slice" % form
        if not has_next:
            assert R.holds_poison(nxt.t), "form %d: x_next written without has_next" % form
    # bit for bit, the poison included (buf = the tensor and its slack)
    assert torch.equal(cat0.buf, cat1.buf), "the forms' concat buffers differ"
    assert torch.equal(nxt0.buf, nxt1.buf), "the forms' x_next buffers differ"


def _shapes():
    return [(1, 32), (3, 96), (2, 160), ("persistent", 96)]


@pytest.mark.parametrize("u16", [True, False], ids=["u16", "i32"])
@pytest.mark.parametrize("has_next", [0, 1], ids=["last", "next"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", _shapes(), ids=["1x32", "3x96", "2x160", "persistent"])
def test_block_forms_agree_on_tiles_of_one_kind(dev, shape, kind, has_next, u16):
    nc, n = shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if nc == "persistent":
        nc = R.smallest_persistent_nc(cus, n)
        tiles = nc * n // R.TILE
        assert -(-tiles // R.BLK_WAVES) > cus and tiles % cus != 0
    else:
        assert -(-(nc * n // R.TILE) // R.BLK_WAVES) == 1, "one short workgroup"
    case = _case(nc, n, kind)
    tk = _tile_kinds(case[5])
    if kind == "uniform":
        # (an exact float32 tie at a 20th entry is possible in a uniform cloud, one point in 10^5: not an overflow, and rare)
        assert (tk == 0).mean() >= 0.99 and (tk != 2).all(), "uniform clouds with ties: not the straight-line path"
    elif kind == "triples":
        assert (tk == 1).all() and case[5].max() <= R.CAP
    elif n > R.CAP:
        assert (tk == 2).mean() >= 0.5 and case[5].max() >= n // 2
    _check(dev, case, has_next, u16, kind)


@pytest.mark.parametrize("u16", [True, False], ids=["u16", "i32"])
@pytest.mark.parametrize("has_next", [0, 1], ids=["last", "next"])
def test_block_forms_agree_when_a_wave_draws_tiles_of_every_kind(dev, has_next, u16):
    """36 tiles per CU and two more: the persistent launch, three draws per wave, clouds of two tiles each whose kind is drawn at
    random -- both tiles of a uniform cloud take the straight-line path, both of a tripled cloud the tie loop, and a cloud whose
    last 48 points are zero is an overflow tile after a tile that mixes overflowing and ordinary rows."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64
    nc = 18 * cus + 1
    kinds = tuple(int(k) for k in np.random.RandomState(SEED).randint(0, 3, size=nc))
    ref_clouds = tuple(int(c) for k in range(3) for c in np.nonzero(np.asarray(kinds) == k)[0][[0, 1, -1]])
    case = _case(nc, n, kinds, ref_clouds)
    tk = _tile_kinds(case[5]).reshape(nc, 2)
    want = np.asarray(kinds)
    assert (tk[want == 0] == 0).mean() >= 0.99 and (tk[want == 0] != 2).all()
    assert (tk[want == 1] == 1).all() and (tk[want == 2] == 2).all()
    assert min((want == k).mean() for k in range(3)) >= 0.25
    # (in tile order every ordered pair of kinds is adjacent many times; a wave's own order is the launch's business)
    seq = tk.reshape(-1)
    assert len({(int(a), int(b)) for a, b in zip(seq[:-1], seq[1:])}) == 9
    _check(dev, case, has_next, u16, "mixed")
