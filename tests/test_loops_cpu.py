"""CPU tests of where the loop-closing stack lives: loops.py defines it, retrieval re-exports it, and its entries refuse host tensors."""
import pytest
import torch

import helpers as H

NAMES = ("revisit_search", "RevisitIndex", "register_pairs", "yaw_seeds", "verify_revisits", "relax_trajectory", "close_loops")


def test_retrieval_re_exports_the_names_of_loops():
    RT, M = H.pkg("retrieval"), H.pkg("loops")
    for name in NAMES:
        assert getattr(RT, name) is getattr(M, name), name
        assert getattr(M, name).__module__ == M.__name__, name


def test_entries_refuse_host_tensors_with_or_without_a_device():
    """Without a device ``require_gpu`` refuses, with one the shared checker does: an EpcNetError that names the entry either way."""
    L, M = H.pkg("lib"), H.pkg("loops")
    f64 = torch.float64
    calls = {"revisit_search": lambda: M.revisit_search(torch.zeros(4, 8), torch.zeros(4, dtype=f64), 1.0),
             "register_pairs": lambda: M.register_pairs(torch.zeros(2, 32, 3), torch.zeros(1, 2, dtype=torch.int32)),
             "relax_trajectory": lambda: M.relax_trajectory(torch.zeros(2, 12, dtype=f64), torch.zeros(0, 2, dtype=torch.int32),
                                                            torch.zeros(0, 12, dtype=f64), torch.zeros(0, 2, dtype=f64))}
    for who, call in calls.items():
        with pytest.raises(L.EpcNetError) as e:
            call()
        assert torch.cuda.is_available() == str(e.value).split(": ", 1)[1].startswith(who + ":"), str(e.value)


def test_checker_words_its_refusals_alike_for_every_entry():
    """The order -- not a device tensor, then dtype or contiguity, then rank, last dimension or device -- on a stand-in that answers what
    the checker asks; every message begins with the entry's name and names the argument; float64 keeps its reason."""
    L, M = H.pkg("lib"), H.pkg("loops")

    class Fake(torch.Tensor):
        is_cuda = True

    def refusal(who, t, dtype, ndim, last=None):
        with pytest.raises(L.EpcNetError) as e:
            M._check(who, "x", t, dtype, ndim, None, last)
        text = str(e.value).split(": ", 1)[1]
        assert text.startswith(who + ": x must "), text
        return text

    for who, first in (("revisit_search", "descriptors"), ("register_pairs", "clouds"), ("relax_trajectory", "poses")):
        assert "live on a ROCm device" in refusal(who, torch.zeros(2, 12), torch.float64, 2)        # host, wrong dtype and all
        wrong = torch.zeros(2, 3).as_subclass(Fake)
        assert "contiguous torch.float64 tensor, got torch.float32" in refusal(who, wrong, torch.float64, 3, 12)
        assert "never converted" in refusal(who, wrong, torch.float64, 2)
        assert "never converted" not in refusal(who, wrong, torch.int32, 2)
        assert "2-d" not in refusal(who, wrong.t(), torch.float32, 3)                                # not contiguous comes before the rank
        assert refusal(who, wrong, torch.float32, 3).endswith("must be 3-d on the %s' device, got (2, 3)" % first)
        assert "2-d with a last dimension of 12" in refusal(who, wrong, torch.float32, 2, 12)
        M._check(who, "x", wrong, torch.float32, 2, None, 3)
