"""CPU: the per-stream DSP-list entry points are exported, mirrored in abi.py with the header's
signatures, and leave the ABI version at 2; icw_graph_form sorts lists on the host alone."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from in_cwave_amd import abi, graph
from in_cwave_amd import lib as L

ROOT = Path(__file__).resolve().parents[1]
NEW = ("icw_set_stream_graph", "icw_clear_stream_bus_slot", "icw_stream_graph_count", "icw_transcode_files_lists")


def declaration(name):
    txt = "".join(h.read_text() for h in sorted((ROOT / "include").glob("*.h")))
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, txt, flags=re.S)
    assert m, f"{name} is not declared in include/"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def c_type(arg):
    """ctypes type of one C parameter declaration of these entry points"""
    a = re.sub(r"\bconst\b", "", arg)
    stars = a.count("*")
    base = a.replace("*", " ").split()[0]
    if base == "icw_ctx":
        return C.c_void_p
    if base == "char" and stars == 2:
        return C.POINTER(C.c_char_p)
    t = {"int": C.c_int, "icw_node": abi.Node, "icw_config": abi.Config, "icw_batch_opts": abi.BatchOpts,
         "icw_batch_stats": abi.BatchStats}[base]
    for _ in range(stars):
        t = C.POINTER(t)
    return t


def test_exported_and_mirrored():
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "in_cwave_amd" / "libicw.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    lib = L.load()
    for name in NEW + ("icw_graph_form",):
        assert name in exported and hasattr(lib, name)
        res, args = abi.SIGNATURES[name]
        assert res is C.c_int
        assert args == [c_type(a) for a in declaration(name)], name
    assert lib.icw_abi_version() == 2
    hdr = (ROOT / "include" / "icw.h").read_text()
    assert "#define ICW_ABI_VERSION 2" in hdr


def test_context_wrappers_exist():
    for m in ("set_stream_graph", "clear_stream_bus_slot", "stream_graph_count"):
        assert callable(getattr(L.Context, m))
    assert callable(L.transcode_files_lists)


def test_graph_form_needs_no_device():
    cfg = graph.default_config(48000)
    for nodes in (graph.graph_shift_master(), graph.graph_master_only(), graph.graph_pm_shift_mix()):
        assert L.graph_form(cfg, nodes) == 0
    for nodes in (graph.graph_pure_delay(), graph.graph_leaky_feedback(), graph.graph_feedback_pm_shift(),
                  graph.graph_long_chain()):
        assert L.graph_form(cfg, nodes) == 1
    # bypassed, only the Master runs: the register form whatever follows it
    assert L.graph_form(cfg, graph.graph_leaky_feedback(), bypass_list=1) == 0
    assert L.graph_form(cfg, [graph.shift()]) == abi.EGRAPH
    assert L.graph_form(cfg, [graph.master(), graph.master()]) == abi.EGRAPH
    assert L.load().icw_graph_form(C.byref(cfg), None, 1, 0) == abi.EINVAL
