"""The references and decoders of tests/test_gpu_stage_forms.py, checked without a GPU: (a) the cloud sets of its block cases meet the
conditions the cases exist for, from O.knn_lists alone; (b) every float64 stage restatement of tests/stage_ref.py, fed the oracle's own
tap, reproduces the oracle's next tap; (c) every fragment decoder inverts a plain numpy encoder of the layout include/epcnet.h
describes."""
import numpy as np
import pytest
import torch

import helpers as H
import stage_ref as R
from helpers import O

BLOCK_SEED = 7      # the block cases' clouds: O.synthetic_clouds(nc, 96, BLOCK_SEED, "repeat30")


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [3, 50, R.smallest_persistent_nc(256)])
def test_block_clouds_hold_every_kind_of_list_in_mixed_passes(nc):
    """Each of the three kinds of row (20 entries, 21..32, overflowing) is at least 10 % of the rows, and at least a quarter of the 4-row
    (f32 kernel) and 8-row (fp16 kernel) passes mix overflowing and ordinary rows; for 3 clouds additionally every 32-point tile holds
    all three kinds."""
    pc = O.synthetic_clouds(nc, 96, BLOCK_SEED, "repeat30")
    if nc > 50:                                   # (the 256-CU persistent case: a slice from both ends and the middle)
        pc = pc[np.r_[0:16, nc // 2 - 8:nc // 2 + 8, nc - 16:nc]]
    _, lists = O.knn_lists(pc)
    cnt = np.array([[len(l) for l in cloud] for cloud in lists])
    assert cnt.min() == 20
    for group in (4, 8):
        plain, tail, ovf, mixed = R.list_kinds(cnt, group)
        print("%d clouds, %d-row passes: 20 entries %.2f, 21..32 %.2f, overflow %.2f, mixed passes %.2f (longest list %d)" % (
            nc, group, plain, tail, ovf, mixed, cnt.max()))
        assert min(plain, tail, ovf) >= 0.10 and mixed >= 0.25
    if nc == 3:
        t = cnt.reshape(-1, 32)
        assert ((t == 20).any(1) & ((t > 20) & (t <= 32)).any(1) & (t > 32).any(1)).all()


def test_smallest_persistent_cloud_count_on_256_cus():
    nc = R.smallest_persistent_nc(256)
    assert nc == 1025 and -(-(3 * nc) // 12) > 256 and (3 * nc) % 256 != 0      # 3075 tiles: 257 short workgroups; per 12, rem 3
    assert not (-(-(3 * (nc - 1)) // 12) > 256 and (3 * (nc - 1)) % 256 != 0)


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------
def _close(got, want, what):
    err = float(np.abs(got - want).max() / np.abs(want).max())
    assert err <= 1e-12, "%s: %.3e" % (what, err)


@pytest.fixture(scope="module")
def taps():
    out = {}
    for arch in ("epc-net", "epc-net-l"):
        pc = O.synthetic_clouds(3, 96, BLOCK_SEED, "repeat30")
        w = O.seeded_weights(arch, 1)
        ref, st = O.forward(pc[:, None], w, arch=arch, dtype=np.float64)
        out[arch] = (pc, w, ref.reshape(3, -1), st.taps)
    return out


def test_block_restatement_reproduces_the_oracle_taps(taps):
    """block_ref on the neighbour sets of neighbour_sets -- built here from the oracle's lists cut to 32 slots, as epc_knn_topk leaves
    them -- against the dense-mask oracle."""
    pc, w, _, tp = taps["epc-net"]
    kth, lists = O.knn_lists(pc)
    cnt = np.array([[len(l) for l in cloud] for cloud in lists], dtype=np.int32)
    idx = np.full((3, 96, R.CAP), -1, dtype=np.int32)          # slots past cnt are never read
    for b in range(3):
        for i, l in enumerate(lists[b]):
            idx[b, i, :min(len(l), R.CAP)] = l[:R.CAP]
    W = R.neighbour_sets(idx, cnt, O.neg_sq_dist(pc), kth)
    assert np.array_equal(W, O.pairwise_distance_mask(pc).astype(np.float64))
    st = R.state64(w)
    for b in (1, 4):
        out, nxt = R.block_ref(st, b, tp["fastdgcnn/conv%d" % b], W, 20, b < 4)
        _close(out, tp["block%d" % b], "block%d" % b)
        if b < 4:
            _close(nxt, tp["fastdgcnn/conv%d" % (b + 1)], "conv%d" % (b + 1))
        else:
            assert nxt is None


def test_conv5_aggregate_and_head_restatements_reproduce_the_oracle_taps(taps):
    _, w, ref, tp = taps["epc-net"]
    st = R.state64(w)
    cat = np.concatenate([tp["block%d" % b] for b in (1, 2, 3, 4)], axis=-1).reshape(-1, 256)
    feat, rnorm, assign, apart = R.conv5_assign_ref(st, cat, 96)
    _close(feat, tp["fastdgcnn/conv5"].reshape(-1, 1024), "conv5")
    _close(assign, tp["vlad_assign"], "assign")
    _close(rnorm, 1.0 / np.linalg.norm(feat, axis=1), "rnorm")
    _close(apart.reshape(3, 3, 64).sum(1), tp["vlad_assign"].reshape(3, 96, 64).sum(1), "apart")
    centres = st.w["VLAD/cluster_weights2"].reshape(1024, 64)
    V, colss = R.aggregate_ref((feat * rnorm[:, None]).reshape(3, 96, 1024), assign.reshape(3, 96, 64),
                               apart.reshape(3, 3, 64).sum(1), centres)
    _close(V, tp["vlad_raw"], "vlad")
    _close(colss.sum(1), (tp["vlad_raw"] ** 2).sum(1), "colss")
    _close(R.vlad_head_ref(st, tp["vlad_raw"], 4), ref, "descriptor")


@pytest.mark.parametrize("groups", [1, 16])
def test_head_restatement_for_other_group_counts(groups):
    """The oracle's whole G_VLAD on random features against vlad_head_ref on its vlad_raw tap, for the GROUPS the head dispatches on."""
    params = dict(H.PARAMS, GROUPS=groups)
    w = O.seeded_weights("epc-net", 2, params=params)
    st = R.state64(w)
    feats = O.l2_normalize(np.random.RandomState(0).randn(2 * 32, 1024), 1)
    want = O.l2_normalize(O.g_vlad_forward(st, feats, 32, groups, False), 1)
    _close(R.vlad_head_ref(st, st.taps["vlad_raw"], groups), want, "descriptor, GROUPS=%d" % groups)


def test_maxpool_and_fc_head_restatements_reproduce_the_oracle_taps(taps):
    _, w, ref, tp = taps["epc-net-l"]
    st = R.state64(w)
    cat = np.concatenate([tp["block1"], tp["block2"]], axis=-1).reshape(-1, 128)
    pooled = R.maxpool_ref(st, cat, 3, 96)
    _close(pooled, tp["maxpool"], "maxpool")
    _close(R.fc_head_ref(st, tp["maxpool"]), ref, "descriptor")


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------
# Plain encoders of include/epcnet.h's layouts: one assignment per index of the fragment, no reshapes shared with the decoders.
M = 96


def _lanes():
    l = np.arange(64)
    return l, l & 31, l >> 5


def test_fp16_feat_decoder_inverts_the_layout():
    """[tile g][chunk c][half s][lane l][q]: point 32g + (l&31), channel 32c + 16s + 8(q>>2) + 4(l>>5) + (q&3)."""
    feat = np.random.RandomState(1).randn(M, 1024).astype(np.float16)
    frag = np.zeros((M // 32, 32, 2, 64, 8), dtype=np.float16)
    l, j, h = _lanes()
    for g in range(M // 32):
        for c in range(32):
            for s in range(2):
                for q in range(8):
                    frag[g, c, s, :, q] = feat[32 * g + j, 32 * c + 16 * s + 8 * (q >> 2) + 4 * h + (q & 3)]
    got = R.decode_feat_f16(torch.from_numpy(frag), M).numpy()
    assert np.array_equal(got, feat.astype(np.float32))


def test_three_byte_feat_decoder_inverts_the_layout():
    """[tile g][chunk c][piece][lane l][16 bytes]; the lane's 48 bytes are 16 little-endian 3-byte values (the upper 24 bits of the
    float32); li = l & 15, q = l >> 4, value 4t + r (t = 2 g2 + p): point 32g + 16p + li, channel 32c + 16 g2 + 4q + r."""
    bits = np.random.RandomState(2).randn(M, 1024).astype(np.float32).view(np.uint32) & np.uint32(0xFFFFFF00)
    frag = np.zeros((M // 32, 32, 3, 64, 16), dtype=np.uint8)
    l = np.arange(64)
    li, q = l & 15, l >> 4
    for g in range(M // 32):
        for c in range(32):
            for g2 in range(2):
                for p in range(2):
                    for r in range(4):
                        v = 4 * (2 * g2 + p) + r
                        word = bits[32 * g + 16 * p + li, 32 * c + 16 * g2 + 4 * q + r]
                        for k in range(3):
                            byte = 3 * v + k                      # position among the lane's 48 bytes
                            frag[g, c, byte // 16, :, byte % 16] = (word >> np.uint32(8 * (k + 1))) & np.uint32(0xFF)
    got = R.decode_feat_b3(torch.from_numpy(frag), M).numpy()
    assert np.array_equal(got.view(np.uint32), bits)


def _assign():
    a = np.random.RandomState(3).dirichlet(np.full(64, 0.3), size=M)
    return a.astype(np.float32)


def test_fp16_assignment_decoder_inverts_the_layout():
    """[tile g][t][s][lane l][q] = fp16(assign * 2^14): cluster 32t + (l&31), point 32g + 16s + 8(l>>5) + q."""
    a = (_assign() * 16384.0).astype(np.float16)
    frag = np.zeros((M // 32, 2, 2, 64, 8), dtype=np.float16)
    l, j, h = _lanes()
    for g in range(M // 32):
        for t in range(2):
            for s in range(2):
                for q in range(8):
                    frag[g, t, s, :, q] = a[32 * g + 16 * s + 8 * h + q, 32 * t + j]
    got = R.decode_assign_f16(torch.from_numpy(frag), M).numpy()
    assert np.array_equal(got, a.astype(np.float32) / np.float32(16384.0))


def test_split_bf16_assignment_decoder_inverts_the_layout():
    """[tile g][t][s][part (hi, lo)][lane l][q] bf16, hi = bf16(a), lo = bf16(a - hi); indices as the fp16 form."""
    a = torch.from_numpy(_assign())
    hi = a.to(torch.bfloat16)
    lo = (a - hi.float()).to(torch.bfloat16)
    frag = torch.zeros((M // 32, 2, 2, 2, 64, 8), dtype=torch.bfloat16)
    l, j, h = (torch.from_numpy(v) for v in _lanes())
    for g in range(M // 32):
        for t in range(2):
            for s in range(2):
                for q in range(8):
                    frag[g, t, s, 0, :, q] = hi[32 * g + 16 * s + 8 * h + q, 32 * t + j]
                    frag[g, t, s, 1, :, q] = lo[32 * g + 16 * s + 8 * h + q, 32 * t + j]
    got = R.decode_assign_bf16x2(frag, M)
    assert torch.equal(got, hi.float() + lo.float())
    assert float((got - a).abs().max()) <= 2.0 ** -16
