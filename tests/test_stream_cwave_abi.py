"""Host side of per-stream CWAVE inputs, no GPU: the new entry point and the file flag in the headers, the
library and the binding, parsed as the other ABI tests parse them.

The ABI version: icw_enable_stream_cwave is an addition, and the suite's host tests pin ICW_ABI_VERSION
to 2 (test_host.py, test_stream_graph_host.py and three more), so the header and the library stay at the
version they agree on; this file checks that agreement, not a new number."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

import pytest

from in_cwave_amd import abi
from in_cwave_amd import lib as L

from test_stream_graph_host import declaration
from test_transcode_fir_host import c_type, same

ROOT = Path(__file__).resolve().parents[1]


def test_prototype_matches_header_and_library():
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "in_cwave_amd" / "libicw.so")], capture_output=True,
                         text=True, check=True).stdout
    name = "icw_enable_stream_cwave"
    assert name in set(re.findall(r" T (\w+)", out)) and hasattr(L.load(), name)
    res, args = abi.SIGNATURES[name]
    want = [c_type(a) for a in declaration(name)]
    assert res is C.c_int and len(args) == len(want) == 2
    assert all(same(x, y) for x, y in zip(args, want)), (args, want)
    assert "int icw_enable_stream_cwave(icw_ctx *ctx, int on);" in (ROOT / "include" / "icw.h").read_text()


def test_null_context_is_refused():
    lib = L.load()
    assert lib.icw_enable_stream_cwave(None, 1) == abi.EINVAL
    assert lib.icw_enable_stream_cwave(None, 0) == abi.EINVAL


def test_flag_bits_agree_with_header():
    text = (ROOT / "include" / "icw_reader.h").read_text()
    bits = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+ICW_BATCH_(MERGE_\w+)\s+(\d+)", text)}
    assert bits == {"MERGE_INPUTS": abi.BATCH_MERGE_INPUTS, "MERGE_CWAVE": abi.BATCH_MERGE_CWAVE}
    assert abi.BATCH_MERGE_CWAVE == 2 and abi.BATCH_MERGE_INPUTS & abi.BATCH_MERGE_CWAVE == 0


@pytest.mark.parametrize("fn", [L.transcode_files, L.transcode_files_lists, L.transcode_files_fir, L.transcode_files_devices])
def test_helpers_take_merge_cwave(fn):
    p = inspect.signature(fn).parameters
    assert p["merge_cwave"].default is False and p["merge_inputs"].default is False


def test_context_helper_and_version():
    assert callable(L.Context.enable_stream_cwave)
    hdr = (ROOT / "include" / "icw.h").read_text()
    assert L.load().icw_abi_version() == int(re.search(r"#define ICW_ABI_VERSION (\d+)", hdr).group(1))


def test_no_file_accepted_with_the_flag(tmp_path):
    """the flag alone opens nothing: a missing file is its own refusal, no context, no device"""
    from in_cwave_amd import graph
    never = tmp_path / "never.wav"
    rc, st, status = L.transcode_files(graph.default_config(48000), graph.graph_shift_master(), [tmp_path / "none.cwave"],
                                       [never], merge_cwave=True)
    assert rc == abi.EINVAL and status == [abi.EINVAL] and st.n_groups == 0 and st.n_files == 0
