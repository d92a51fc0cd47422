"""CPU: icw_enable_stream_bus is exported and mirrored in abi.py with the header's signature, the ABI version
stays 2, ICW_BATCH_MERGE_BUS is 4 on both sides, and the run cutting of the mixed serial graph kernel
(tests/native/bus_runs_host_check.cpp, built with AddressSanitizer and UBSan and run directly) holds."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from in_cwave_amd import abi
from in_cwave_amd import lib as L

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "in_cwave_amd" / "csrc"


def declaration(name):
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "icw.h").read_text(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, txt, flags=re.S)
    assert m, f"{name} is not declared in include/icw.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_exported_and_mirrored():
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "in_cwave_amd" / "libicw.so")], capture_output=True,
                         text=True, check=True).stdout
    assert "icw_enable_stream_bus" in set(re.findall(r" T (\w+)", out))
    lib = L.load()
    assert hasattr(lib, "icw_enable_stream_bus")
    assert declaration("icw_enable_stream_bus") == ["icw_ctx *ctx", "int on"]
    assert abi.SIGNATURES["icw_enable_stream_bus"] == (C.c_int, [C.c_void_p, C.c_int])
    assert callable(L.Context.enable_stream_bus)


def test_abi_version_stays_2():
    assert L.load().icw_abi_version() == 2
    assert "#define ICW_ABI_VERSION 2" in (ROOT / "include" / "icw.h").read_text()


def test_null_context_is_einval():
    lib = L.load()
    assert lib.icw_enable_stream_bus(None, 1) == abi.EINVAL
    assert lib.icw_enable_stream_bus(None, 0) == abi.EINVAL


def test_merge_bus_bit(tmp_path):
    (tmp_path / "v.c").write_text('#include <stdio.h>\n#include "icw_reader.h"\n'
                                  'int main(void) { printf("%d %d %d\\n", ICW_BATCH_MERGE_INPUTS, ICW_BATCH_MERGE_CWAVE, '
                                  'ICW_BATCH_MERGE_BUS); return 0; }\n')
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "v"), str(tmp_path / "v.c")], check=True)
    out = subprocess.run([str(tmp_path / "v")], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["1", "2", "4"]
    assert abi.BATCH_MERGE_BUS == 4
    assert abi.BATCH_MERGE_BUS & (abi.BATCH_MERGE_INPUTS | abi.BATCH_MERGE_CWAVE) == 0


def test_run_cutting(tmp_path):
    """the stand-alone check over icw_k4_cut_runs: every stream once, no wave with two runs, wg0 ascending, W"""
    exe = tmp_path / "bus_runs_host_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), str(ROOT / "tests" / "native" / "bus_runs_host_check.cpp"), str(CSRC / "icw_graph_compile.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "bus_runs_host_check: ok", r.stdout + r.stderr


def test_run_check_detects_a_shared_wave(tmp_path):
    """negative control: with runs packed to lanes instead of whole waves, the check must fail"""
    text = (CSRC / "icw_graph_compile.cpp").read_text()
    old = "        wg += (j - i + 63) / 64;\n"
    assert text.count(old) == 1
    (tmp_path / "icw_graph_compile.cpp").write_text(
        text.replace(old, "        wg += (j - i) / 64;\n").replace('"icw_graph_compile.h"', f'"{CSRC}/icw_graph_compile.h"')
        .replace('"icw_tables.inc"', f'"{CSRC}/icw_tables.inc"'))
    exe = tmp_path / "neg"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), str(ROOT / "tests" / "native" / "bus_runs_host_check.cpp"),
                    str(tmp_path / "icw_graph_compile.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 1 and "FAIL" in r.stderr, r.stdout + r.stderr
