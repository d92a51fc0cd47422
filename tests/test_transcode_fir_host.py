"""CPU: icw_transcode_files_fir is exported and mirrored in abi.py with the header's signature, refuses a
bad converter order or window parameter before it opens a file, and the setters the FIR converter now
serves keep the header's prototypes.

The ABI version: the entry point is an addition, and the suite's host tests pin ICW_ABI_VERSION to 2
(test_host.py, test_stream_graph_host.py), so the header and the library stay at the version they
agree on; this file checks that agreement, not a new number."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from in_cwave_amd import abi, graph
from in_cwave_amd import lib as L

from test_stream_graph_host import declaration

ROOT = Path(__file__).resolve().parents[1]


def c_type(arg):
    """ctypes type of one C parameter declaration of these entry points"""
    a = re.sub(r"\bconst\b", "", arg)
    stars = a.count("*")
    base = a.replace("*", " ").split()[0]
    if base == "icw_ctx":
        return C.c_void_p
    if base == "char" and stars == 2:
        return C.POINTER(C.c_char_p)
    t = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double, "icw_node": abi.Node,
         "icw_config": abi.Config, "icw_batch_opts": abi.BatchOpts, "icw_batch_stats": abi.BatchStats}[base]
    for _ in range(stars):
        t = C.POINTER(t)
    return t


def same(a, b):
    """two ctypes parameter types of one size and kind (abi.py writes int32_t as c_int, uint32_t as c_uint)"""
    if a is b:
        return True
    simple = (C.c_int, C.c_int32, C.c_uint, C.c_uint32)
    return a in simple and b in simple and C.sizeof(a) == C.sizeof(b) and (a(-1).value < 0) == (b(-1).value < 0)


@pytest.mark.parametrize("name", ["icw_transcode_files_fir", "icw_set_fir_hilbert", "icw_enable_stream_fir", "icw_set_stream_graph", "icw_set_stream_input"])
def test_prototypes_match_header(name):
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "in_cwave_amd" / "libicw.so")], capture_output=True,
                         text=True, check=True).stdout
    assert name in set(re.findall(r" T (\w+)", out)) and hasattr(L.load(), name)
    res, args = abi.SIGNATURES[name]
    want = [c_type(a) for a in declaration(name)]
    assert res is C.c_int and len(args) == len(want)
    assert all(same(x, y) for x, y in zip(args, want)), (name, args, want)


def test_abi_version_agrees():
    hdr = (ROOT / "include" / "icw.h").read_text()
    assert L.load().icw_abi_version() == int(re.search(r"#define ICW_ABI_VERSION (\d+)", hdr).group(1))
    assert callable(L.transcode_files_fir)


@pytest.mark.parametrize("k_M,k_beta", [(0, 8.0), (31, 8.0), (-2, 8.0), (abi.FIR_MAX_ORDER + 2, 8.0), (254, -1.0),
                                        (254, 1e3), (254, float("nan"))])
def test_bad_converter_is_refused_before_any_file(tmp_path, k_M, k_beta):
    src = tmp_path / "a.wav"
    src.write_bytes(b"not parsed: the converter's checks come first")
    dst = tmp_path / "out.wav"
    rc, st, status = L.transcode_files_fir(graph.default_config(48000), [graph.graph_shift_master()], [src], [dst], k_M, k_beta)
    assert rc == abi.EINVAL
    assert not dst.exists()
    assert st.n_files == 0 and st.n_groups == 0 and status == [abi.OK]      # stats and status untouched
