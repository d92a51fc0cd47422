"""Host only: the per-stream input entry points exist at every layer -- exported by libicw.so, declared
in the headers, mirrored in abi.py and wrapped in lib.py.  No device is touched."""
import ctypes as C
import inspect
import re
from pathlib import Path

from in_cwave_amd import abi
from in_cwave_amd import lib as L

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("icw_set_stream_input", "icw_stream_input_count", "icw_last_k0_timing")


def test_symbols_exported():
    lib = C.CDLL(str(L.LIB_PATH))
    for name in SYMBOLS:
        assert getattr(lib, name, None) is not None, name


def test_declared_in_header():
    text = (ROOT / "include" / "icw.h").read_text()
    assert re.search(r"int\s+icw_set_stream_input\s*\(\s*icw_ctx\s*\*\s*ctx,\s*int\s+first,\s*int\s+count,\s*"
                     r"uint32_t\s+sample_rate,\s*uint32_t\s+fmt,\s*uint32_t\s+channels\s*\)\s*;", text)
    assert re.search(r"int\s+icw_stream_input_count\s*\(\s*const\s+icw_ctx\s*\*\s*ctx\s*\)\s*;", text)


def test_abi_signatures():
    res, args = abi.SIGNATURES["icw_set_stream_input"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]
    res, args = abi.SIGNATURES["icw_stream_input_count"]
    assert res is C.c_int and args == [C.c_void_p]


def test_python_wrappers():
    sig = inspect.signature(L.Context.set_stream_input)
    assert list(sig.parameters) == ["self", "sample_rate", "fmt", "channels", "first", "count"]
    assert sig.parameters["first"].default == 0 and sig.parameters["count"].default is None
    assert callable(L.Context.stream_input_count)
    for fn in (L.transcode_files, L.transcode_files_lists, L.transcode_files_devices):
        assert inspect.signature(fn).parameters["merge_inputs"].default is False


def test_merge_flag():
    text = (ROOT / "include" / "icw_reader.h").read_text()
    m = re.search(r"#define\s+ICW_BATCH_MERGE_INPUTS\s+(\d+)", text)
    assert m and int(m.group(1)) == 1 and abi.BATCH_MERGE_INPUTS == 1
    # the flags word is the options' last member, its layout unchanged
    assert abi.BatchOpts._fields_[-1] == ("reserved_", C.c_int32) and C.sizeof(abi.BatchOpts) == 24
