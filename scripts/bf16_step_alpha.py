"""GPU box: the bf16 step's |alpha - 1| (tests/test_gpu_train_step.py: test_bf16_precision_step_matches_the_operand_rounded_oracle) at one
shape with the fused hidden projection and the fused VLAD tail switched on and off in turn.  The four settings compute the same arithmetic
up to float32 summation order (ops.HiddenProjection against ops.Linear's tile GEMMs, both with bf16 operands at these shapes; ops.HiddenTail
against the per-op tail: f32-accurate products, dWg rounded at B = 32 in both), so how far alpha moves between them is the part of it that
is summation-order noise.  Usage: python scripts/bf16_step_alpha.py [N_POINTS NNEG NQ]  (default 4096 12 2: 2 x 16 x 4096)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import helpers as H  # noqa: E402
import test_gpu_train_step as S  # noqa: E402

n, nneg, nq = (int(a) for a in (sys.argv[1:4] if len(sys.argv) >= 4 else (4096, 12, 2)))
ops = H.pkg("ops")
dev = torch.device("cuda:0")
for proj, tail in ((True, True), (False, True), (True, False), (False, False)):
    ops.HIDDEN_PROJ, ops.HIDDEN_TAIL = proj, tail
    print("=== fused hidden projection %s, fused tail %s" % (proj, tail), flush=True)
    try:
        S.test_bf16_precision_step_matches_the_operand_rounded_oracle(dev, n, nneg, nq, None)
        print("all bars held")
    except AssertionError as e:
        print("FAILED:", str(e)[:300])
    sys.stdout.flush()
