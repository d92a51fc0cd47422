"""The per-stream setting table (in_cwave_amd/csrc/icw_stream_table.h) against a plain per-stream array, on
the host: tests/native/stream_table_check.cpp, built with AddressSanitizer and UBSan and run directly, drives
tables of 1, 2, 3 and 7 streams through random range assignments, colliding whole-table transforms and
resets, and checks after every operation each stream's value, that the entries are pairwise unequal, all
used and numbered in order of their first stream, the entry count, that a dropped candidate leaves the
table unchanged, and that runs() over the empty range, one stream, the whole table and random ranges tiles
the range with maximal runs of one entry each (exactly one for a one-entry table)."""
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
HEADER = HERE.parent / "in_cwave_amd" / "csrc" / "icw_stream_table.h"
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def build(src, exe):
    subprocess.run(["g++", *FLAGS, "-o", str(exe), str(src)], check=True)
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build(HERE / "native" / "stream_table_check.cpp", tmp_path_factory.mktemp("stream_table") / "stream_table_check")


@pytest.mark.parametrize("seed", ["1", "0x9E3779B97F4A7C15", "20240607"])
def test_table_matches_per_stream_model(checker, seed):
    r = subprocess.run([str(checker), "3000", seed], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("operations 12000 failures 0"), r.stdout


def test_header_compiles_alone(tmp_path):
    (tmp_path / "alone.cpp").write_text(f'#include "{HEADER}"\nint main() {{ return 0; }}\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", str(tmp_path / "alone.cpp")], check=True)


@pytest.mark.parametrize("what,old,new", [
    ("equal entries stay apart", "!same(ne[k], ents[(size_t)e])", "(true || same(ne[k], ents[(size_t)e]))"),
    ("survivors in the candidate's order, not by first stream", "        ents.swap(ne);",
     "        for (int32_t &e : of) e = (int32_t)ne.size() - 1 - e;\n        ents.assign(ne.rbegin(), ne.rend());"),
])
def test_checker_detects_broken_compaction(tmp_path, what, old, new):
    """negative controls: the same checker over a header whose compaction no longer merges equal entries, or
    no longer numbers the survivors by first stream, must fail"""
    checker_fails_on(tmp_path, what, old, new)


@pytest.mark.parametrize("what,old,new", [
    ("two neighbouring runs of different entries merged", "if (e == cur->e) {", "if (e == cur->e || i == 2) {"),
    ("one run split", "if (e == cur->e) {", "if (e == cur->e && i != 2) {"),
])
def test_checker_detects_broken_runs(tmp_path, what, old, new):
    """negative controls: the same checker over a header whose runs() takes stream 2 of a range into the run
    before it whatever its entry, or starts a new run there whatever its entry, must fail"""
    checker_fails_on(tmp_path, what, old, new)


def checker_fails_on(tmp_path, what, old, new):
    text = HEADER.read_text()
    assert text.count(old) == 1, what
    (tmp_path / "icw_stream_table.h").write_text(text.replace(old, new))
    src = (HERE / "native" / "stream_table_check.cpp").read_text()
    inc = '"../../in_cwave_amd/csrc/icw_stream_table.h"'
    assert src.count(inc) == 1
    (tmp_path / "neg.cpp").write_text(src.replace(inc, f'"{tmp_path}/icw_stream_table.h"'))
    exe = build(tmp_path / "neg.cpp", tmp_path / "neg")
    r = subprocess.run([str(exe), "300"], capture_output=True, text=True)
    assert r.returncode == 1 and "FAIL" in r.stdout, (what, r.stdout[-400:] + r.stderr[-400:])
