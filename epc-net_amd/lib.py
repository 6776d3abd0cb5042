"""ctypes binding of ``libepcnet_hip.so``, derived from ``include/epcnet.h`` at import.

The header is the one definition of the C boundary: ``parse_header`` reads every declaration, ``#define EPC_*`` and the
``epc_status`` enum out of it, and this module sets ``restype`` / ``argtypes`` of every entry point, the ``EPC_*`` module
attributes, ``STATUS_NAMES``, ``EXPORTS`` and the checked call form ``run`` of every entry point that takes a stream from the
result.  The further headers ``include/epcnet_*.h`` are read the same way, one row of the table ``_HEADERS`` each.  Anything the reader
does not understand, a name declared twice or a missing header is an exception at import, never a skipped line.  Only the three
structures are mirrored by hand (tests/test_host_cpu.py checks their layout against the compiler).

There is NO fallback: if the shared library has not been built (``python -c "import __graft_entry__ as g;
g.build()"`` or ``make -C epc-net_amd/csrc``) importing this module raises, and every op raises ``EpcNetError``
when the library reports a failure.  ``import torch`` happens first on purpose: the library's
``libamdhip64.so.7`` dependency then resolves to the HIP runtime torch already loaded, so device pointers and
streams are shared between torch (plumbing: allocation, streams, RCCL) and the kernels.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_void_p

import torch  # noqa: F401  (must precede CDLL, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
# EPCNET_LIB: load another build of the same library instead (how two builds are compared, e.g. scripts/ab_block.sh)
LIB_PATH = os.environ.get("EPCNET_LIB") or os.path.join(_HERE, "libepcnet_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "epcnet.h")

_SCALARS = {"int": c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong, "float": c_float,
            "size_t": ctypes.c_size_t, "int32_t": c_int32, "uint32_t": ctypes.c_uint32}
# what the headers whose row of _HEADERS says so pass by value besides: the reader of every other header goes on refusing a `double`
# parameter
_REVISIT_SCALARS = dict(_SCALARS, double=ctypes.c_double)
# the dtype a tensor must have where the header declares a typed pointee (``run``); any dtype goes at every other pointer
_POINTEES = {"float*": torch.float32, "double*": torch.float64, "int32_t*": torch.int32, "int*": torch.int32, "long*": torch.int64}


def parse_header(text: str, need_status: bool = True, scalars=_SCALARS):
    """``(functions, constants, status)`` of the text of include/epcnet.h (or, with ``need_status=False``, of a further header in the
    same grammar that declares no ``enum epc_status`` of its own and whose entries are named ``epcnet_*``: the rows of ``_HEADERS``):
    ``functions[name] = (return type, [parameter types], [parameter names])`` in header order, the types as C type names without
    ``const`` and spaces around ``*`` -- a key of ``scalars``, or any type with a ``*`` (``char*`` alone as a return type);
    ``constants``: every ``#define EPC_<NAME> <integer>``; ``status``: the members of ``enum epc_status``.  Raises ValueError on whatever
    it does not understand."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)         # extern "C" { and its }
    constants = {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(EPC_\w+)[ \t]+(.*?)[ \t]*$", text, flags=re.M)}
    enum = re.search(r"typedef\s+enum\s+epc_status\s*\{(.*?)\}", text, flags=re.S)
    if not enum and need_status:
        raise ValueError("epcnet.h: no enum epc_status")
    status = {n.strip(): int(v, 0) for n, v in (m.split("=") for m in enum.group(1).split(","))} if enum else {}
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r"typedef\s+(struct|enum)\s+\w+\s*(\{[^{}]*\})?\s*\w+\s*;", " ", text)

    def ctype(t):
        return re.sub(r"\s*\*\s*", "*", " ".join(re.sub(r"\bconst\b", " ", t).split()))

    functions = {}
    for decl in text.split(";"):
        if not decl.strip():
            continue
        m = re.fullmatch(r"\s*([\w\s*]+?)\b(epc(?:net)?_\w+)\s*\((.*)\)\s*", decl, flags=re.S)
        if not m or m.group(2) in functions:
            raise ValueError("epcnet.h: not a declaration, or a second one of its name: %r" % " ".join(decl.split()))
        ret, name, params, names = ctype(m.group(1)), m.group(2), [], []
        if ret not in scalars and ret != "char*":
            raise ValueError("epcnet.h: %s: unknown return type %r" % (name, ret))
        for p in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            pm = re.fullmatch(r"\s*(.*[\s*])(\w+)\s*", p, flags=re.S)              # the type, then the parameter's name
            if not pm or (ctype(pm.group(1)) not in scalars and "*" not in pm.group(1)):
                raise ValueError("epcnet.h: %s: unknown parameter type in %r" % (name, " ".join(p.split())))
            params.append(ctype(pm.group(1)))
            names.append(pm.group(2))
        functions[name] = (ret, params, names)
    return functions, constants, status


if not os.path.exists(HEADER_PATH):
    raise ImportError(
        "%s is missing: the binding is derived from the library's header (keep include/ beside the package).  "
        "There is no second copy of the declarations." % HEADER_PATH)
with open(HEADER_PATH) as _f:
    _functions, _constants, _status = parse_header(_f.read())
# The further headers, in the order they are bound: the same grammar and the same library, their entries bound and callable like the
# others but listed on their own -- EXPORTS stays what include/epcnet.h declares.  A new header is a new row: (the stem of
# include/epcnet_<stem>.h, the prefix of its list, whether a `double` may be passed by value, whether every entry must launch)
_HEADERS = (
    ("poses", "POSE", False, True),             # POSE_EXPORTS, POSES_HEADER_PATH: relations and tuples from poses
    ("scans", "SCAN", False, False),            # SCAN_EXPORTS, SCANS_HEADER_PATH: raw scans in front of the down-sampler
    ("submaps", "SUBMAP", False, False),        # SUBMAP_EXPORTS, SUBMAPS_HEADER_PATH: travel-length submaps from posed scans
    # STAMP_EXPORTS, STAMPS_HEADER_PATH: timestamped scans.  Its times are `long long*`, which _POINTEES does not know: ops checks them
    ("stamps", "STAMP", False, False),
    ("revisits", "REVISIT", True, False),       # REVISIT_EXPORTS, REVISITS_HEADER_PATH: `along` is `double*` (float64, _POINTEES)
    ("pairs", "PAIR", True, False),             # PAIR_EXPORTS, PAIRS_HEADER_PATH: its two status bits join the EPC_* constants
    ("trajectory", "TRAJECTORY", True, False),  # TRAJECTORY_EXPORTS, TRAJECTORY_HEADER_PATH: loop closing; one status bit more
    ("maps", "MAP", False, False),              # MAP_EXPORTS, MAPS_HEADER_PATH: corrected submaps fused into one voxel map
    ("surfels", "SURFEL", False, False),        # SURFEL_EXPORTS, SURFELS_HEADER_PATH: the map with a surfel per voxel
    ("localize", "LOCALIZE", False, False),     # LOCALIZE_EXPORTS, LOCALIZE_HEADER_PATH: scans localised against the surfel map
    ("forms", "FORM", False, False),            # FORM_EXPORTS, FORMS_HEADER_PATH: test / tuning entries that name a kernel's form
    ("growmap", "GROWMAP", False, False),       # GROWMAP_EXPORTS, GROWMAP_HEADER_PATH: the surfel map that grows across calls
    ("remap", "REMAP", False, False))           # REMAP_EXPORTS, REMAP_HEADER_PATH: rows taken out of that map, or re-posed in it


def _bind_header(text, header, doubles, declared, constants):
    """The functions of the further header ``header`` from its text; its constants join ``constants``.  A function that a header of
    ``declared`` (header -> functions) declares, or a constant that ``constants`` holds, is an ImportError that names ``header``."""
    functions, defines, _ = parse_header(text, need_status=False, scalars=_REVISIT_SCALARS if doubles else _SCALARS)
    if any(set(functions) & set(earlier) for earlier in declared.values()) or set(defines) & set(constants):
        raise ImportError("%s declares a name epcnet.h or an earlier header declares" % header)
    constants.update(defines)
    return functions


_declared = {"epcnet.h": _functions}            # header -> its functions, in the order bound: what argtypes and `run` are set from
for _stem, _prefix, _doubles, _ in _HEADERS:
    _header = "epcnet_%s.h" % _stem
    _path = os.path.join(os.path.dirname(HEADER_PATH), _header)
    if not os.path.exists(_path):
        raise ImportError("%s is missing: the binding of its entries is derived from it" % _path)
    with open(_path) as _f:
        _declared[_header] = _bind_header(_f.read(), _header, _doubles, _declared, _constants)
    globals().update({_stem.upper() + "_HEADER_PATH": _path, _prefix + "_EXPORTS": list(_declared[_header])})
globals().update(_constants, **_status)     # EPC_OK, EPC_EINVAL, EPC_KNN_CAP, EPC_PRECISION_FAST, EPC_NUM_STAGES ... as module attributes
# every symbol include/epcnet.h declares, in its order (tests check the library exports exactly these)
EXPORTS = list(_functions)
STATUS_NAMES = {v: n for n, v in _status.items()}
PRECISION_IDS = {"f32": _constants["EPC_PRECISION_F32"], "fast": _constants["EPC_PRECISION_FAST"]}
STAGE_NAMES = ["sort", "knn", "conv1", "block1", "block2", "block3", "block4", "conv5", "aggregate", "head"]
assert len(STAGE_NAMES) == _constants["EPC_NUM_STAGES"]


class EpcNetError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__("%s (%d): %s" % (STATUS_NAMES.get(status, "?"), status, message))
        self.status = status


class EpcCfg(ctypes.Structure):
    """``struct epc_cfg`` of include/epcnet.h."""
    _fields_ = [("arch", c_int32), ("num_points", c_int32), ("input_dim", c_int32), ("knn", c_int32),
                ("cluster_size", c_int32), ("output_dim", c_int32), ("groups", c_int32),
                ("micro_batch", c_int32), ("precision", c_int32)]


_P = c_void_p


class ChainFwdBlock(ctypes.Structure):
    """``struct epc_chain_fwd_block`` of include/epcnet.h."""
    _fields_ = [(n, _P) for n in ("gamma0", "beta0", "in_bias", "Wa", "ba", "gamma_a", "beta_a", "Wb", "bb", "gamma_b", "beta_b",
                                  "W0_next", "b0_next", "z0", "mean0", "var0", "mean_a", "var_a", "mean_b", "var_b",
                                  "d", "za", "zb", "z0_next")]


class ChainFwdArgs(ctypes.Structure):
    """``struct epc_chain_fwd_args`` of include/epcnet.h."""
    _fields_ = [("blk", ChainFwdBlock * _constants["EPC_CHAIN_MAX_BLOCKS"]), ("nblocks", c_int), ("xyz", _P), ("idx", _P), ("cnt", _P),
                ("kth", _P), ("cap", c_int), ("num_clouds", c_int), ("n", c_int), ("knn", c_int), ("cat", _P), ("cat_bf16", _P),
                ("eps", c_float), ("workspace", _P), ("spin_ticks", ctypes.c_longlong)]


if not os.path.exists(LIB_PATH):
    raise ImportError(
        "%s is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' or "
        "make -C epc-net_amd/csrc).  There is no CPU fallback." % LIB_PATH)

_lib = ctypes.CDLL(LIB_PATH)

# a pointer to a structure mirrored above keeps its type check; every other pointer is a void*
_POINTERS = {"epc_cfg*": POINTER(EpcCfg), "epc_chain_fwd_args*": POINTER(ChainFwdArgs)}
for _fs in _declared.values():
    for _name, (_ret, _params, _) in _fs.items():
        _fn = getattr(_lib, _name)  # AttributeError here = the built library is stale (rebuild it)
        _fn.restype = c_char_p if _ret == "char*" else _REVISIT_SCALARS[_ret]
        _fn.argtypes = [_REVISIT_SCALARS.get(_t) or _POINTERS.get(_t, c_void_p) for _t in _params]


def lib() -> ctypes.CDLL:
    return _lib


def check(status: int) -> None:
    if status != _status["EPC_OK"]:
        raise EpcNetError(status, (_lib.epc_last_error() or b"").decode("utf-8", "replace"))


def ptr(t) -> int:
    """Device pointer of a contiguous CUDA/HIP tensor (or None)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise EpcNetError(-1, "tensor must live on a ROCm device: the HIP path has no CPU fallback")
    if not t.is_contiguous():
        raise EpcNetError(-1, "tensor must be contiguous")
    return t.data_ptr()


def micro_batch_of(cfg: "EpcCfg", num_clouds: int) -> int:
    """Clouds per internal pass (mirrors micro_batch() of csrc/pipeline.hip)."""
    mb = cfg.micro_batch if cfg.micro_batch > 0 else (64 if cfg.arch == _constants["EPC_ARCH_EPC_NET"] else 256)
    return max(1, min(int(num_clouds), int(mb)))


def current_stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _converter(where: str, ctype: str):
    """What turns one Python argument of a launching entry point into what ctypes takes for a parameter of C type ``ctype``
    (``where`` names the function, the position and the parameter in a refusal).  Contiguity is the call site's business: the
    GEMMs take strided views with their strides, the chain writes column slices of the concat."""
    if "*" in ctype:
        dtype = _POINTEES.get(ctype)

        def pointer(a):
            if a is None:                   # a null pointer
                return None
            try:
                on_device = a.is_cuda
            except AttributeError:          # an int (a raw address) or a ctypes object (byref, a pointer array): ctypes' business
                return a
            if not on_device:
                raise EpcNetError(-1, "%s: tensor must live on a ROCm device: the HIP path has no CPU fallback" % where)
            if dtype is not None and a.dtype is not dtype:
                raise EpcNetError(-1, "%s: the header declares %s there, the tensor is %s" % (where, dtype, a.dtype))
            return a.data_ptr()
        return pointer
    cast = float if ctype in ("float", "double") else int

    def scalar(a):
        if type(a) is cast:
            return a
        if isinstance(a, torch.Tensor):
            raise TypeError("%s: a tensor where the header declares a scalar" % where)
        return cast(a)
    return scalar


def _launcher(name: str, fn, types, names):
    signature = "%s(%s)" % (name, ", ".join("%s %s" % tn for tn in zip(types, names)))
    converters = [_converter("%s: argument %d (%s %s)" % (name, i + 1, t, n), t) for i, (t, n) in enumerate(zip(types[:-1], names))]
    ok = _status["EPC_OK"]

    def launch(*args, stream=None):
        if len(args) != len(converters):
            raise TypeError("%s takes %d arguments and the stream, got %d" % (signature, len(converters), len(args)))
        status = fn(*[c(a) for c, a in zip(converters, args)], current_stream() if stream is None else stream)
        if status != ok:
            check(status)
    launch.__name__ = launch.__qualname__ = name
    launch.__doc__ = signature
    return launch


class run:
    """The checked call form of every LAUNCHING entry point -- one whose last parameter is ``void* stream`` -- by name:
    ``run.epc_col_sum(dy, rows, cout, db, ws, n)`` takes the header's arguments without the stream.  A tensor is legal at a pointer
    parameter only, must live on the device and have the dtype of a typed pointee (``_POINTEES``; anything goes at ``void*``); its
    address is passed, strides are the caller's.  None, an int address and ctypes objects pass unchanged, scalars through int() /
    float().  The stream is the current one (or ``stream=``), the returned status goes through ``check``.  Everything else --
    size queries, ``*_ok``, the forwards whose stream is not last -- is called on the raw handle ``lib()``."""


LAUNCHING = []                                  # what include/epcnet.h alone declares with a stream
_all_launch = {"epcnet_%s.h" % _stem for _stem, _, _, _every in _HEADERS if _every}
for _header, _fs in _declared.items():
    for _name, (_ret, _t, _pn) in _fs.items():
        if _t and (_t[-1], _pn[-1]) == ("void*", "stream"):
            assert _ret == "int", "%s takes a stream and does not return a status" % _name
            setattr(run, _name, staticmethod(_launcher(_name, getattr(_lib, _name), _t, _pn)))
            if _header == "epcnet.h":
                LAUNCHING.append(_name)
        else:
            assert _header not in _all_launch, "%s: every entry of %s takes a stream last" % (_name, _header)


def require_gpu() -> None:
    if not torch.cuda.is_available():
        raise EpcNetError(-3, "no ROCm device visible: the EPC-Net HIP path cannot run (no CPU fallback)")
