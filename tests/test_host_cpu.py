"""CPU tests of the host layer: C-ABI exports, naming contract, checkpoint reader, loud failure without a GPU."""
import importlib
import json
import os
import re
import shutil

import numpy as np
import pytest
import torch

import helpers as H
from helpers import O, ROOT

GOLD = os.path.join(ROOT, "tests", "golden")
TABLES = json.load(open(os.path.join(GOLD, "ckpt_tables.json")))


def test_library_exports_every_declared_symbol():
    L = H.pkg("lib")
    header = open(os.path.join(ROOT, "include", "epcnet.h")).read()
    declared = set(re.findall(r"\b(epc_[a-z0-9_]+)\s*\(", header))
    assert declared == set(L.EXPORTS), declared ^ set(L.EXPORTS)
    for name in declared:
        assert hasattr(L.lib(), name), name
    assert L.lib().epc_version() >= 100
    # ... and the prose may not name entry points that do not exist (the header spoke of an
    # `epc_net_forward_status`): every epc_* identifier in the header, comments included, and in the documents a binder reads, is an
    # exported symbol or one of the header's types
    types = {"epc_cfg", "epc_status", "epc_profile", "epc_chain_fwd_args", "epc_chain_fwd_block"}
    for doc in ("include/epcnet.h", "INTEGRATION.md", "DESIGN.md", "README.md", "epc-net_amd/lib.py", "epc-net_amd/engine.py"):
        text = open(os.path.join(ROOT, doc)).read()
        unknown = {n for n in re.findall(r"\bepc_[a-z0-9_]+\b", text) if n not in declared and n not in types}
        assert not unknown, "%s names entry points the library does not have: %s" % (doc, sorted(unknown))
    # the precision prose describes the arithmetic the kernels run (csrc/common.h split8_f16s, csrc/conv5_f32.hip)
    assert "split-fp16" in header and "3-byte" in header and "epc_net_forward_status" not in header


def test_built_library_defines_exactly_the_declared_symbols():
    """What DESIGN.md states: the header's declarations = the unmangled `T epc_*` symbols `nm -D` shows of the built library."""
    import subprocess
    L = H.pkg("lib")
    rocm_bin = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    nm = shutil.which("nm") or shutil.which("llvm-nm") or shutil.which("llvm-nm", path=rocm_bin)
    assert nm, "neither nm nor llvm-nm found"
    out = subprocess.run([nm, "-D", "--defined-only", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = re.findall(r"^[0-9a-f]+ T (epc_\w+)$", out, flags=re.M)
    assert len(defined) == len(set(defined)) == len(L.EXPORTS)
    assert set(defined) == set(L.EXPORTS), set(defined) ^ set(L.EXPORTS)


def test_binding_signatures_match_the_header():
    """restype / argtypes as lib.py derived them from include/epcnet.h, against expectations typed here from READING the header:
    one entry per class of type (a wrong width truncates silently: a c_int for the GEMM's `long` strides, a missing restype on a
    `size_t ..._bytes` function)."""
    from ctypes import POINTER, c_char_p, c_float, c_int, c_long, c_size_t, c_uint32, c_void_p
    L = H.pkg("lib")
    P, i, l, f = c_void_p, c_int, c_long, c_float
    want = {
        "epc_last_error": (c_char_p, []),                                             # const char* epc_last_error(void)
        "epc_crc32c": (c_uint32, [c_uint32, P, c_size_t]),
        "epc_gemm_f32": (i, [P, P, P, P, i, i, i, l, l, l, l, i, i, l, l, l, i, i, P]),   # sAm sAk sBk sBn .. bA bB bC are long
        "epc_sq_err_partial_floats": (c_size_t, [l]),
        "epc_net_forward": (i, [POINTER(L.EpcCfg), P, P, i, P, P, c_size_t, P]),
        "epc_hidden_tail_fwd": (i, [P, i, i, i, P, P, P, P, P, f, f, f, P, P, P, P, P, P, P, P, P, P]),   # eps, bessel1, bessel2
        "epc_chain_fwd_persist": (i, [POINTER(L.ChainFwdArgs), i, P]),
        "epc_chain_persist_workspace_bytes": (c_size_t, []),                          # (void)
        "epc_adam_multi": (i, [i, P, P, P, P, P, f, f, f, f, i, P, P]),               # float* const* w ... const long* n
    }
    for name, (restype, argtypes) in want.items():
        fn = getattr(L.lib(), name)
        assert fn.restype == restype, (name, fn.restype)
        assert list(fn.argtypes) == argtypes, (name, fn.argtypes)
    for name in L.EXPORTS:                                                            # nothing is left at ctypes' defaults
        assert getattr(L.lib(), name).argtypes is not None and getattr(L.lib(), name).restype is not None, name


def test_header_reader_refuses_what_it_does_not_understand():
    L = H.pkg("lib")
    enum = "typedef enum epc_status { EPC_OK = 0, EPC_EINVAL = -1 } epc_status;\n#define EPC_KNN_CAP 32 /* slots */\n"
    good = enum + "int epc_a(const float* x, long n, void* stream);\nsize_t epc_b(void); /* bytes */\n"
    functions, constants, status = L.parse_header(good)
    assert functions == {"epc_a": ("int", ["float*", "long", "void*"], ["x", "n", "stream"]), "epc_b": ("size_t", [], [])}
    names = L.parse_header(enum + "int epc_c(const epc_cfg *cfg, float* const* w, const int32_t*idx, void* stream, int lanes);\n")[0]
    assert names == {"epc_c": ("int", ["epc_cfg*", "float**", "int32_t*", "void*", "int"], ["cfg", "w", "idx", "stream", "lanes"])}
    assert list(functions) == ["epc_a", "epc_b"] and constants == {"EPC_KNN_CAP": 32} and status == {"EPC_OK": 0, "EPC_EINVAL": -1}
    for bad in (good.replace("long n", "double n"),                  # an unknown parameter type
                good.replace("long n", "long"),                      # a parameter without a name
                good.replace("size_t epc_b", "ssize_t epc_b"),       # an unknown return type
                good.replace("size_t epc_b", "stray size_t epc_b"),  # text between two declarations
                good.replace("size_t epc_b", "stray; size_t epc_b"),
                good + "int epc_a(int n);\n",                        # one name, two declarations
                good.replace("32", "(32)"),                          # a constant that is not an integer literal
                good + "}\n"):                                       # text after the last declaration
        with pytest.raises(ValueError):
            L.parse_header(bad)


def test_launching_set_is_the_headers_stream_last_functions():
    """lib.LAUNCHING / lib.run: exactly the declarations whose last parameter is `void* stream`, read here from the header's text with a
    pattern of the test's own."""
    L = H.pkg("lib")
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "epcnet.h")).read(), flags=re.S)
    want = re.findall(r"\b(epc_\w+)\s*\([^()]*\bvoid\s*\*\s*stream\s*\)\s*;", header)
    assert len(want) == 114 and set(want) == set(L.LAUNCHING) and len(L.LAUNCHING) == 114
    assert [n for n in L.EXPORTS if hasattr(L.run, n)] == L.LAUNCHING
    for name in ("epc_net_forward_overlapped", "epc_net_forward_profiled"):      # their stream is not the last parameter
        assert name in L.EXPORTS and name not in L.LAUNCHING
    functions = L.parse_header(open(os.path.join(ROOT, "include", "epcnet.h")).read())[0]
    assert len(functions) == 156
    assert all(functions[name][0] == "int" for name in L.LAUNCHING)              # a status; no size_t query is among them
    assert not [name for name, (ret, _, _) in functions.items() if ret == "size_t" and name in L.LAUNCHING]


def test_every_further_header_has_its_row_and_is_bound_whole():
    """lib._HEADERS against the files on disk -- a header added without a row fails here --, and what one loop makes of every row: the
    public lists and paths, non-default restype / argtypes, and `run` holding exactly the functions whose last parameter is
    `void* stream`."""
    import glob
    L = H.pkg("lib")
    on_disk = sorted(os.path.basename(p)[len("epcnet_"):-len(".h")] for p in glob.glob(os.path.join(ROOT, "include", "epcnet_*.h")))
    assert sorted(row[0] for row in L._HEADERS) == on_disk and list(L._declared) == ["epcnet.h"] + ["epcnet_%s.h" % row[0] for row in L._HEADERS]
    assert [row[0] for row in L._HEADERS if row[2]] == ["revisits", "pairs", "trajectory"]          # a `double` by value
    assert [row[0] for row in L._HEADERS if row[3]] == ["poses"]                                    # every entry launches
    launching = []
    for stem, prefix, doubles, every_launches in L._HEADERS:
        path = getattr(L, stem.upper() + "_HEADER_PATH")
        assert path == os.path.join(ROOT, "include", "epcnet_%s.h" % stem)
        functions = L.parse_header(open(path).read(), need_status=False, scalars=L._REVISIT_SCALARS if doubles else L._SCALARS)[0]
        assert functions == L._declared["epcnet_%s.h" % stem] and list(functions) == getattr(L, prefix + "_EXPORTS") and functions
        for name, (ret, types, names) in functions.items():
            fn = getattr(L.lib(), name)
            assert fn.restype is L._REVISIT_SCALARS[ret], name             # set, and to the header's type: ctypes' default is c_int
            assert fn.argtypes is not None and len(fn.argtypes) == len(types), name
            if types and (types[-1], names[-1]) == ("void*", "stream"):
                launching.append(name)
        assert not every_launches or [n for n in functions if n in launching] == list(functions)
    on_run = [n for n in vars(L.run) if not n.startswith("_")]
    assert sorted(on_run) == sorted(L.LAUNCHING + launching) and len(on_run) == len(set(on_run))


def test_a_name_declared_twice_is_an_import_error():
    """The loop's collision check (lib._bind_header) on copies of what it accumulated: binding any row's text a second time -- every
    function of it is declared already -- or a header that defines a constant again raises ImportError and names the header."""
    L = H.pkg("lib")
    for stem, _, doubles, _ in L._HEADERS:
        text = open(getattr(L, stem.upper() + "_HEADER_PATH")).read()
        declared, constants = dict(L._declared), dict(L._constants)
        with pytest.raises(ImportError) as e:
            L._bind_header(text, "epcnet_%s.h" % stem, doubles, declared, constants)
        assert "epcnet_%s.h" % stem in str(e.value) and constants == L._constants
        if not doubles:                                                      # ... and never by reading a `double` it should not
            continue
        with pytest.raises(ValueError):
            L._bind_header(text, "epcnet_%s.h" % stem, False, {}, {})
    fresh, constants = "int epcnet_fresh_entry(const float* x, int n, void* stream);\n", dict(L._constants)
    assert list(L._bind_header("#define EPC_FRESH 7\n" + fresh, "epcnet_fresh.h", False, dict(L._declared), constants)) == ["epcnet_fresh_entry"]
    assert constants["EPC_FRESH"] == 7 and "EPC_FRESH" not in L._constants
    for clash in ("#define EPC_KNN_CAP 32\n" + fresh, fresh.replace("epcnet_fresh_entry", "epc_version"),
                  fresh.replace("epcnet_fresh_entry", L.FORM_EXPORTS[-1])):
        with pytest.raises(ImportError):
            L._bind_header(clash, "epcnet_fresh.h", False, dict(L._declared), dict(L._constants))


class _FakeDeviceTensor:
    """What lib.run asks of a tensor argument, without a device."""

    def __init__(self, dtype, is_cuda=True):
        self.dtype, self.is_cuda, self.asked = dtype, is_cuda, 0

    def data_ptr(self):
        self.asked += 1
        return 0x1000


def test_checked_call_form_refuses_before_the_library_is_reached():
    """Every refusal names the function, the parameter's position and its header name, and happens before the C function runs: the
    library's last-error text stays what the call before left."""
    L = H.pkg("lib")
    functions = L.parse_header(open(os.path.join(ROOT, "include", "epcnet.h")).read())[0]
    _, types, names = functions["epc_col_moments"]
    assert types == ["float*", "int", "int", "float*", "float*", "void*", "size_t", "void*"] and names[-1] == "stream"
    # a status reaches the caller: epc_col_sum checks its pointers (EPC_CHECK_ARG, then colreduce_check) before its first HIP call
    with pytest.raises(L.EpcNetError) as e:
        L.run.epc_col_sum(None, 0, 0, None, None, 0, stream=0)
    assert e.value.status == L.EPC_EINVAL and "EPC_EINVAL" in str(e.value) and "epc_col_sum: null pointer" in str(e.value)
    mark = L.lib().epc_last_error()
    assert mark == b"epc_col_sum: null pointer"

    def refused(exc, position, *args):
        with pytest.raises(exc) as e:
            L.run.epc_col_moments(*args, stream=0)
        text = str(e.value)
        assert "epc_col_moments" in text and ("argument %d" % position) in text and names[position - 1] in text, text
        assert L.lib().epc_last_error() == mark                      # (reached, it would read "epc_col_moments: null pointer")
        return e.value

    err = refused(L.EpcNetError, 1, torch.zeros(4, 4), 4, 4, None, None, None, 0)         # a CPU tensor at `const float* x`
    assert err.status == -1 and "tensor must live on a ROCm device: the HIP path has no CPU fallback" in str(err)
    refused(TypeError, 2, None, torch.zeros(1), 4, None, None, None, 0)                   # a tensor at `int rows`
    for args in ((None, 4, 4, None, None, None), (None, 4, 4, None, None, None, 0, 0)):   # one short, one over (the stream is a keyword)
        with pytest.raises(TypeError) as e:
            L.run.epc_col_moments(*args, stream=0)
        assert "epc_col_moments" in str(e.value) and all(n in str(e.value) for n in names), str(e.value)
        assert L.lib().epc_last_error() == mark
    # dtypes, on a stand-in that answers is_cuda / dtype / data_ptr() (the conversion is the one the callable runs)
    f32, i32, bf16 = (_FakeDeviceTensor(d) for d in (torch.float32, torch.int32, torch.bfloat16))
    for bad in (i32, bf16):
        err = refused(L.EpcNetError, 1, bad, 4, 4, None, None, None, 0)                   # at `const float* x`
        assert str(bad.dtype) in str(err) and "torch.float32" in str(err) and bad.asked == 0
    assert functions["epc_neighbour_mean_fwd"][1][2] == "int32_t*" and functions["epc_neighbour_mean_fwd"][2][2] == "idx"
    with pytest.raises(L.EpcNetError) as e:                                               # float32 at `const int32_t* idx`
        L.run.epc_neighbour_mean_fwd(None, None, f32, None, None, 32, 1, 8, 4, None, stream=0)
    assert "epc_neighbour_mean_fwd" in str(e.value) and "argument 3" in str(e.value) and "idx" in str(e.value) and f32.asked == 0
    assert L.lib().epc_last_error() == mark
    # the same tensors pass at `void* workspace`: the call reaches the library, which refuses the null `x`
    for ok in (f32, i32, bf16):
        with pytest.raises(L.EpcNetError) as e:
            L.run.epc_col_moments(None, 4, 4, None, None, ok, 0, stream=0)
        assert e.value.status == L.EPC_EINVAL and "epc_col_moments: null pointer" in str(e.value) and ok.asked == 1
    with pytest.raises(L.EpcNetError) as e:                                               # float32 passes at `const float* x`
        L.run.epc_col_moments(f32, 4, 4, None, None, None, 0, stream=0)
    assert e.value.status == L.EPC_EINVAL and f32.asked == 2
    assert functions["epc_adam_multi"][1][5] == "long*"                                   # `const long* n` wants int64
    with pytest.raises(L.EpcNetError) as e:
        L.run.epc_adam_multi(0, None, None, None, None, i32, 0.0, 0.9, 0.999, 1e-8, 1, None, stream=0)
    assert "argument 6" in str(e.value) and "torch.int64" in str(e.value) and i32.asked == 1


def test_mirrored_struct_layouts_match_the_compiler(tmp_path):
    """EpcCfg, ChainFwdBlock and ChainFwdArgs of lib.py against sizeof / offsetof of include/epcnet.h's structs as gcc lays them out
    (a field name the header does not have fails to compile)."""
    import ctypes
    import subprocess
    L = H.pkg("lib")
    structs = (("epc_cfg", L.EpcCfg), ("epc_chain_fwd_block", L.ChainFwdBlock), ("epc_chain_fwd_args", L.ChainFwdArgs))
    lines = ['#include <stdio.h>', '#include "epcnet.h"', "int main(void) {"]
    for cname, cls in structs:
        lines.append('    printf("%%zu\\n", sizeof(%s));' % cname)
        lines += ['    printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (cname, f[0], cname, f[0]) for f in cls._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["    return 0;", "}", ""]))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o",
                        str(tmp_path / "layout")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    want = []
    for _, cls in structs:
        want.append("%d" % ctypes.sizeof(cls))
        want += ["%d %d" % (getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_]
    assert got == want + [""]
    assert len(L.ChainFwdBlock._fields_) == 24 and len(L.ChainFwdArgs._fields_) == 15      # every member of the header's structs is mirrored
    assert ctypes.sizeof(L.ChainFwdArgs) == (4 * 24 + 12) * 8                            # 96 block pointers + 12 eight-byte slots


def test_cfg_struct_layout_and_sizes():
    import ctypes
    L, E = H.pkg("lib"), H.pkg("engine")
    assert ctypes.sizeof(L.EpcCfg) == 36               # nine int32 fields (include/epcnet.h: epc_cfg, `precision` last)
    assert E.make_cfg("epc-net", 4096, H.PARAMS).precision == L.EPC_PRECISION_F32      # the package default: the reference's class
    assert E.make_cfg("epc-net", 4096, dict(H.PARAMS, PRECISION="fast")).precision == L.EPC_PRECISION_FAST
    with pytest.raises(ValueError):
        E.make_cfg("epc-net", 4096, dict(H.PARAMS, PRECISION="fp8"))
    f32 = E.make_cfg("epc-net", 4096, H.PARAMS, precision="f32")
    cfg = E.make_cfg("epc-net", 4096, H.PARAMS, precision="fast")
    # the f32-equivalent path keeps f32 tensors between its stages (and `feat` as 3-byte values against the fast path's fp16):
    # 1.6 x the workspace of the fp16 path
    ratio = L.lib().epc_net_workspace_bytes(ctypes.byref(f32), 64) / L.lib().epc_net_workspace_bytes(ctypes.byref(cfg), 64)
    assert 1.5 < ratio < 1.7
    assert L.lib().epc_net_packed_bytes(ctypes.byref(f32)) == L.lib().epc_net_packed_bytes(ctypes.byref(cfg))
    badp = E.make_cfg("epc-net", 4096, H.PARAMS)
    badp.precision = 7
    assert L.lib().epc_net_packed_bytes(ctypes.byref(badp)) == 0
    nbytes = L.lib().epc_net_packed_bytes(ctypes.byref(cfg))
    assert nbytes >= 4704832 * 4 - 4 * 10000          # folded weights: ~ the trainable matrices
    offs = [L.lib().epc_net_packed_offset(ctypes.byref(cfg), s) for s in range(7)]
    assert offs == sorted(offs) and offs[0] == 0 and all(o % 256 == 0 for o in offs)
    assert L.lib().epc_net_workspace_bytes(ctypes.byref(cfg), 64) > 64 * 4096 * 1024 * 2   # holds the fp16 conv5 map
    bad = E.make_cfg("epc-net", 4100, H.PARAMS)       # N not a multiple of 32
    assert L.lib().epc_net_packed_bytes(ctypes.byref(bad)) == 0


@pytest.mark.parametrize("arch,count", [("epc-net", 4704832), ("epc-net-l", 418880)])
def test_state_dict_equals_reference_checkpoint_names(arch, count):
    st = H.make_store(arch, O.seeded_weights(arch, 0), "cpu")
    ref = {e["name"]: tuple(e["shape"]) for e in TABLES[arch]["entries"]
           if not e["name"].endswith(("/Adam", "/Adam_1")) and e["name"] not in ("Variable", "beta1_power", "beta2_power")}
    assert {k: tuple(v.shape) for k, v in st.state_dict().items()} == ref
    assert st.num_trainable_params() == count


def test_reference_initialisers():
    V = H.pkg("variables")
    st = V.reset_default_store(device="cpu", seed=1)
    M = H.pkg("models.epc-net")
    with V.variable_scope("query_triplets"):
        M.declare_variables(H.PARAMS, 4096)
    w = st.vars["query_triplets/fastdgcnn/conv5/weights"]
    lim = (6.0 / (256 + 1024)) ** 0.5                                # xavier uniform, utils/tf_util.py:42
    assert float(w.abs().max()) <= lim and float(w.abs().max()) > 0.95 * lim
    assert float(st.vars["query_triplets/fastdgcnn/conv1/biases"].abs().max()) == 0.0
    assert float(st.vars["query_triplets/VLAD/bn/moving_variance"].min()) == 1.0
    h = st.vars["query_triplets/VLAD/hidden1_weights"]
    assert abs(float(h.std()) - 1 / 8.0) < 2e-3                      # N(0, 1/sqrt(cluster_size)), loupe.py:316


@pytest.mark.parametrize("tag,n", [("epc-net", 221), ("epc-net-l", 115), ("epc-net-l-d_student", 113),
                                   ("epc-net-l-d_teacher", 221)])
def test_tf_bundle_index_reader_on_reference_files(tag, n):
    tfb = H.pkg("tf_bundle")
    entries = tfb.read_index(os.path.join(GOLD, tag + ".ckpt.index"))
    assert len(entries) == n
    want = {e["name"]: (e["dtype"], tuple(e["shape"]), e["offset"], e["size"]) for e in TABLES[tag]["entries"]}
    got = {e.name: (e.dtype.name, e.shape, e.offset, e.size) for e in entries.values()}
    assert got == want


def test_checkpoint_round_trip_and_missing_payload(tmp_path):
    """Seeded weights written through the REFERENCE's index table load back into the store; a missing .data shard
    raises like evaluate.py:264-266 refuses to run."""
    tfb = H.pkg("tf_bundle")
    prefix = str(tmp_path / "model_epoch22_iter18101.ckpt")
    shutil.copyfile(os.path.join(GOLD, "epc-net.ckpt.index"), prefix + ".index")
    st = H.make_store("epc-net", O.seeded_weights("epc-net", 0, mode="init"), "cpu")
    with pytest.raises(FileNotFoundError):
        st.load_checkpoint(prefix)
    entries = tfb.read_index(prefix + ".index")
    w = O.seeded_weights("epc-net", 5)
    tensors = {}
    for name, e in entries.items():
        rel = name[len("query_triplets/"):] if name.startswith("query_triplets/") else None
        tensors[name] = w[rel] if rel in w else np.zeros(e.shape, dtype=e.dtype)
    tfb.write_checkpoint_payload(prefix, tensors)
    assert os.path.getsize(tfb.data_path_for(prefix)) == 56476940            # SURVEY.md 8c payload size
    # the index is the REFERENCE's: its entries carry the checksums of the trained weights, which this synthetic payload
    # cannot match -- the loader must notice (TensorFlow's BundleReader verifies them too), and load when told not to check
    with pytest.raises(ValueError, match="checksum"):
        st.load_checkpoint(prefix)
    unused = st.load_checkpoint(prefix, verify_crc=False)
    assert "beta1_power" in unused and any(u.endswith("/Adam") for u in unused)
    for k, v in w.items():
        assert np.array_equal(st.vars["query_triplets/" + k].numpy(), v)


def test_forward_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L, V = H.pkg("lib"), H.pkg("variables")
    V.reset_default_store(device="cpu", seed=0)
    M = H.pkg("models.epc-net")
    x = M.placeholder_inputs(1, 1, 64, 3)
    with V.variable_scope("query_triplets"), pytest.raises(L.EpcNetError):
        M.forward(x, False, params=H.PARAMS)


def test_submit_fails_loudly_without_gpu_and_micro_batch_mirror():
    """The throughput entry point has no CPU fallback either; lib.micro_batch_of mirrors micro_batch() of pipeline.hip
    (the workspace the library asks for is per pass, so it stops growing at the micro-batch)."""
    import ctypes
    L, E, V = H.pkg("lib"), H.pkg("engine"), H.pkg("variables")
    for arch, default in (("epc-net", 64), ("epc-net-l", 256)):
        cfg = E.make_cfg(arch, 4096, H.PARAMS)
        assert [L.micro_batch_of(cfg, n) for n in (1, default - 1, default, 10 * default)] == [1, default - 1, default, default]
        ws = [L.lib().epc_net_workspace_bytes(ctypes.byref(cfg), n) for n in (default - 1, default, 10 * default)]
        assert ws[0] < ws[1] == ws[2]
        cfg2 = E.make_cfg(arch, 4096, H.PARAMS, micro_batch=8)
        assert L.micro_batch_of(cfg2, 100) == 8 and L.micro_batch_of(cfg2, 3) == 3
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    st = V.reset_default_store(device="cpu", seed=0)
    eng = E.InferenceEngine("epc-net", H.PARAMS, st, in_flight=2)
    with pytest.raises(L.EpcNetError):
        eng.submit(torch.zeros(1, 64, 3))
    with pytest.raises(L.EpcNetError):
        eng.submit(torch.zeros(1, 64, 4))          # INPUT_DIM != 3 is rejected before any device work
    eng.drain()                                    # nothing submitted: a no-op


def test_forward_argument_errors():
    V = H.pkg("variables")
    V.reset_default_store(device="cpu", seed=0)
    M = H.pkg("models.epc-net")
    with pytest.raises(TypeError):
        M.forward(torch.zeros(1, 1, 64, 3), False)                        # params is required (epc-net.py:37)
    with pytest.raises(ValueError):
        M.forward(torch.zeros(1, 1, 64, 13), False, params=H.PARAMS)      # INPUT_DIM mismatch


def test_losses_match_oracle_and_reference_error_behaviour():
    M = H.pkg("models.epc-net")
    rng = np.random.RandomState(0)
    def unit(*s):
        a = rng.randn(*s); return a / np.linalg.norm(a, axis=-1, keepdims=True)
    q, pos, neg, oth = unit(3, 1, 256), unit(3, 2, 256), unit(3, 14, 256), unit(3, 1, 256)
    tq, tp, tn, to = (torch.from_numpy(a) for a in (q, pos, neg, oth))
    assert float(M.lazy_quadruplet_loss(tq, tp, tn, to, 0.5, 0.2)) == pytest.approx(O.lazy_quadruplet_loss(q, pos, neg, oth, 0.5, 0.2), rel=1e-12)
    assert float(M.quadruplet_loss(tq, tp, tn, to, 0.5, 0.2)) == pytest.approx(O.quadruplet_loss(q, pos, neg, oth, 0.5, 0.2), rel=1e-12)
    assert float(M.lazy_triplet_loss(tq, tp, tn, 0.5)) == pytest.approx(O.lazy_triplet_loss(q, pos, neg, 0.5), rel=1e-12)
    assert float(M.triplet_loss(tq, tp, tn, 0.5)) == pytest.approx(O.triplet_loss(q, pos, neg, 0.5), rel=1e-12)
    assert float(M.lazy_quadruplet_loss_sm(tq, tp, tn, to, 0.2)) == pytest.approx(O.lazy_quadruplet_loss_sm(q, pos, neg, oth, 0.2), rel=1e-12)
    with pytest.raises(NameError):                                         # models/epc-net.py:205 returns `soft_los`
        M.softmargin_loss(tq, tp, tn)
    with pytest.raises(NameError):
        M.quadruplet_loss_sm(tq, tp, tn, to, 0.2)
    L = importlib.import_module("epc-net_amd.models.epc-net-l")
    assert set(M.LOSS_NAMES) <= set(dir(L))                                # identical loss family in both files


def test_unused_reference_ops_are_named_not_silently_missing():
    tf_util = H.pkg("utils.tf_util")
    for name in ("conv2d", "conv3d", "dropout", "knn", "get_edge_feature", "pairwise_distance", "avg_pool2d"):
        with pytest.raises(NotImplementedError):
            getattr(tf_util, name)()


def test_plain_c_example_builds_against_the_header():
    """examples/epcnet_forward.c is a C99 program that uses the ABI without Python or torch: it must compile against
    include/epcnet.h and link against the built library (no GPU needed for that)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(root, "examples"), "clean"], check=True, capture_output=True)
    r = subprocess.run(["make", "-C", os.path.join(root, "examples")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(root, "examples", "epcnet_forward"))


def test_step_inputs_recognised_as_slices_of_one_buffer():
    """training._joined_along_dim1: the concat of train.py:252 is skipped only for the exact consecutive dim-1 slices."""
    import torch
    T = H.pkg("training")
    joined = torch.arange(2 * 18 * 5 * 3, dtype=torch.float32).reshape(2, 18, 5, 3)
    sizes = [1, 2, 14, 1]
    parts = torch.split(joined, sizes, 1)
    assert torch.equal(T._joined_along_dim1(parts), joined)
    assert T._joined_along_dim1(parts).data_ptr() == joined.data_ptr()
    assert T._joined_along_dim1((parts[0], parts[2], parts[1], parts[3])) is None          # wrong order
    assert torch.equal(T._joined_along_dim1(parts[:3]), joined[:, :17])                   # a prefix is still a slice run
    assert T._joined_along_dim1(tuple(p.clone() for p in parts)) is None                  # separate tensors
    t = torch.arange(18 * 5 * 3, dtype=torch.float32).reshape(18, 5, 3)                   # bench.py's tuples: t[None, a:b]
    q = (t[None, 0:1], t[None, 1:3], t[None, 3:17], t[None, 17:18])
    assert torch.equal(T._joined_along_dim1(q), t[None])
    assert T._joined_along_dim1((t[None, 0:1], t[None, 2:3])) is None                     # a gap
