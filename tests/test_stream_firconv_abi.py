"""Host side of per-stream FIR converters, no GPU: the two entry points in the header, the library and the
binding, parsed as the other ABI tests parse them.

The ABI version: both are additions, and the suite's host tests pin ICW_ABI_VERSION to 2 (test_host.py,
test_stream_graph_host.py and more), so the header and the library stay at the version they agree on; this
file checks that agreement, not a new number."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from in_cwave_amd import abi
from in_cwave_amd import lib as L

from test_stream_graph_host import declaration
from test_transcode_fir_host import c_type, same

ROOT = Path(__file__).resolve().parents[1]
PROTOS = {
    "icw_set_stream_fir": ("int icw_set_stream_fir(icw_ctx *ctx, int first, int count, int32_t k_M, double k_beta);", 5),
    "icw_stream_fir_count": ("int icw_stream_fir_count(const icw_ctx *ctx);", 1),
}


@pytest.mark.parametrize("name", list(PROTOS))
def test_prototype_matches_header_and_library(name):
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "in_cwave_amd" / "libicw.so")], capture_output=True,
                         text=True, check=True).stdout
    assert name in set(re.findall(r" T (\w+)", out)) and hasattr(L.load(), name)
    text, n_args = PROTOS[name]
    res, args = abi.SIGNATURES[name]
    want = [c_type(a) for a in declaration(name)]
    assert res is C.c_int and len(args) == len(want) == n_args
    assert all(same(x, y) for x, y in zip(args, want)), (args, want)
    assert text in (ROOT / "include" / "icw.h").read_text()


def test_null_context_is_refused():
    lib = L.load()
    assert lib.icw_set_stream_fir(None, 0, 1, 30, 8.0) == abi.EINVAL
    assert lib.icw_stream_fir_count(None) == abi.EINVAL


def test_context_helpers_and_version():
    assert callable(L.Context.set_stream_fir) and callable(L.Context.stream_fir_count)
    hdr = (ROOT / "include" / "icw.h").read_text()
    assert L.load().icw_abi_version() == int(re.search(r"#define ICW_ABI_VERSION (\d+)", hdr).group(1))


def test_reader_header_says_the_file_entry_points_keep_one_converter():
    text = (ROOT / "include" / "icw_reader.h").read_text()
    assert "icw_set_stream_fir" in text
