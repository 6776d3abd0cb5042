"""Every size query of the library on a fixed grid of arguments, one line per call: ``name(arguments) -> value``.

The queries are the functions the headers under include/ declare with a ``size_t`` result (workspace, scratch and partial-buffer sizes,
packed sizes and offsets).  Two builds of the library answer alike exactly when their outputs are the same text, so a change that is
meant to leave every workspace layout alone is checked by running this once per build and comparing:

    python scripts/size_queries.py > branch.txt
    EPCNET_LIB=/path/to/other/libepcnet_hip.so python scripts/size_queries.py > other.txt

``--digest`` prints the number of lines and the SHA-256 of the text instead.  Needs no GPU: the queries are host arithmetic.

Integer parameters take the cross product of ``VALUES`` (illegal combinations included: they answer 0); a query with an ``epc_cfg*``
takes both models x both precisions x ``GROUPS`` x ``POINTS`` (x ``CLOUDS``, x every stage index for the offset query)."""
import hashlib
import importlib
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
L = importlib.import_module("epc-net_amd.lib")

VALUES = (-1, 0, 1, 31, 32, 33, 95, 96, 97, 127, 128, 129, 255, 256, 257, 1000, 4096, 4608, 73728, 90112)
GROUPS = (1, 4, 16)
POINTS = (256, 4096)
CLOUDS = (1, 3, 64, 65, 256, 257)
STAGES = tuple(range(-1, 8))                        # 0 .. 6 are stages; -1 and 7 are refused


def configs():
    for arch, prec, groups, points in itertools.product((L.EPC_ARCH_EPC_NET, L.EPC_ARCH_EPC_NET_L),
                                                        (L.EPC_PRECISION_F32, L.EPC_PRECISION_FAST), GROUPS, POINTS):
        yield L.EpcCfg(arch=arch, num_points=points, input_dim=3, knn=20, cluster_size=64, output_dim=256, groups=groups,
                       micro_batch=0, precision=prec)


def lines():
    for functions in L._declared.values():
        for name, (ret, params, names) in functions.items():
            if ret != "size_t":
                continue
            fn = getattr(L.lib(), name)
            if params and params[0] == "epc_cfg*":
                rest = {"num_clouds": CLOUDS, "stage": STAGES}
                for cfg in configs():
                    shown = "arch=%d precision=%d groups=%d num_points=%d" % (cfg.arch, cfg.precision, cfg.groups, cfg.num_points)
                    for args in itertools.product(*(rest[n] for n in names[1:])):
                        yield "%s(%s) -> %d" % (name, ", ".join([shown] + [str(a) for a in args]), fn(cfg, *args))
            else:
                for args in itertools.product(*([VALUES] * len(params))):
                    yield "%s(%s) -> %d" % (name, ", ".join(str(a) for a in args), fn(*args))


if __name__ == "__main__":
    text = "".join(line + "\n" for line in lines())
    if "--digest" in sys.argv[1:]:
        print("%d lines, sha256 %s" % (text.count("\n"), hashlib.sha256(text.encode()).hexdigest()))
    else:
        sys.stdout.write(text)
