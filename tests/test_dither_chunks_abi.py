"""Host side of icw_last_dither_chunks, no GPU: the entry point in the header, the library and the binding,
parsed as the other ABI tests parse them, and the one chunk function the launcher and the host share.

The entry point is an addition, so ICW_ABI_VERSION stays 2 (tests/test_stream_cwave_abi.py has the rule)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from in_cwave_amd import abi
from in_cwave_amd import lib as L

from test_stream_graph_host import declaration
from test_transcode_fir_host import c_type, same

ROOT = Path(__file__).resolve().parents[1]
NAME = "icw_last_dither_chunks"


def test_prototype_matches_header_and_library():
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "in_cwave_amd" / "libicw.so")], capture_output=True,
                         text=True, check=True).stdout
    assert NAME in set(re.findall(r" T (\w+)", out)) and hasattr(L.load(), NAME)
    res, args = abi.SIGNATURES[NAME]
    want = [c_type(a) for a in declaration(NAME)]
    assert res is C.c_int and len(args) == len(want) == 2
    assert all(same(x, y) for x, y in zip(args, want)), (args, want)
    assert "int icw_last_dither_chunks(const icw_ctx *ctx, int *chunk_frames);" in (ROOT / "include" / "icw.h").read_text()


def test_null_context_is_refused_and_version_stays():
    lib = L.load()
    n = C.c_int(-7)
    assert lib.icw_last_dither_chunks(None, C.byref(n)) == abi.EINVAL and n.value == -7
    assert lib.icw_last_dither_chunks(None, None) == abi.EINVAL
    assert callable(L.Context.last_dither_chunks)
    hdr = (ROOT / "include" / "icw.h").read_text()
    assert lib.icw_abi_version() == int(re.search(r"#define ICW_ABI_VERSION (\d+)", hdr).group(1)) == 2


def test_launcher_and_host_share_one_chunk_function():
    """the chunk length is worked out in one inline function: the launcher cuts by it, the call plan
    reports it, and neither keeps an expression of its own"""
    src = ROOT / "in_cwave_amd" / "csrc"
    assert len(re.findall(r"\bint icw_dith_chunk_frames\(", (src / "icw_device.h").read_text())) == 1
    render = (src / "icw_render.hip").read_text()
    body = render[render.index("static hipError_t icw_launch_dither_t"):render.index('extern "C" hipError_t icw_launch_dither')]
    assert "icw_dith_chunk_frames(a->T, a->wcap, W)" in body and "wcap /" not in body
    host = (src / "icw_host.cpp").read_text()
    assert "icw_dith_chunk_frames(T, a3.wcap" in host and "wcap /" not in host
