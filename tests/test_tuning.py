"""CPU test of the tuning record (in_cwave_amd/csrc/icw_tuning.h): a stand-alone program built with the
host compiler prints what icw_read_tuning() makes of the environment.  For each of the 25 ICW_* switches:
the default, accepted values, and (where a range exists) values just outside it, which leave the default.
The expected values below restate the parsing icw_create did before the record existed (strcmp against
one literal, or atoi / atof with a range), not the new reader's output.  The last test reads the record
twice in one process with ICW_DITH_PAR changed in between: each context sees its own environment (a
process-wide static once latched the first value)."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

SRC = r"""
#include <stdio.h>
#include "icw_tuning.h"
static void show(const IcwTuning &t)
{
    printf("k1_mode=%d render_row=%d serialize=%d cu_split=%d k1_wpc=%d k1_wg=%d k1_wg_env=%d fir_ramp=%.17g "
           "rest_cus=%d max_block=%d block_env=%d max_sets=%d zero_copy=%d spin_wait=%d first_block=%d "
           "first_block_env=%d taper=%.17g taper_min=%d dedup_ok=%d fill_drain=%d fir_fuse=%d chain_ok=%d "
           "stream1=%d s1_ovl=%d s1_stamps=%d k3r_spec=%d dith_par=%d fir_sig=%d\n",
           t.k1_mode, t.render_row, t.serialize, t.cu_split, t.k1_wpc, t.k1_wg, t.k1_wg_env, t.fir_ramp, t.rest_cus,
           t.max_block, t.block_env, t.max_sets, t.zero_copy, t.spin_wait, t.first_block, t.first_block_env, t.taper,
           t.taper_min, t.dedup_ok, t.fill_drain, t.fir_fuse, t.chain_ok, t.stream1, t.s1_ovl, t.s1_stamps,
           t.k3r_spec, t.dith_par, t.fir_sig);
}
int main(int argc, char **argv)
{
    show(icw_read_tuning());
    if (argc == 3) {                      /* NAME VALUE: set it and read again */
        setenv(argv[1], argv[2], 1);
        show(icw_read_tuning());
    }
    return 0;
}
"""

DEFAULTS = dict(k1_mode=-1, render_row=-1, serialize=0, cu_split=1, k1_wpc=2, k1_wg=1, k1_wg_env=0, fir_ramp=0.0,
                rest_cus=-1, max_block=16384, block_env=0, max_sets=2, zero_copy=1, spin_wait=1, first_block=4096,
                first_block_env=0, taper=-1.0, taper_min=1024, dedup_ok=1, fill_drain=1, fir_fuse=1, chain_ok=1,
                stream1=1, s1_ovl=1, s1_stamps=0, k3r_spec=1, dith_par=1, fir_sig=1)

# (switch, value, the fields it changes from DEFAULTS); {}: ignored, the default stays
CASES = [
    ("ICW_K1_MODE", "plain", dict(k1_mode=0)), ("ICW_K1_MODE", "row", dict(k1_mode=3)), ("ICW_K1_MODE", "lane", {}),
    ("ICW_RENDER", "serial", dict(render_row=0)), ("ICW_RENDER", "row", dict(render_row=1)), ("ICW_RENDER", "1", {}),
    ("ICW_SERIALIZE", "1", dict(serialize=1)), ("ICW_SERIALIZE", "0", {}), ("ICW_SERIALIZE", "2", {}),
    ("ICW_CU_SPLIT", "0", dict(cu_split=0)), ("ICW_CU_SPLIT", "1", {}), ("ICW_CU_SPLIT", "00", {}),
    ("ICW_K1_WPC", "1", dict(k1_wpc=1)), ("ICW_K1_WPC", "8", dict(k1_wpc=8)), ("ICW_K1_WPC", "9", {}),
    ("ICW_K1_WPC", "0", {}),
    ("ICW_K1_WG", "4", dict(k1_wg=4, k1_wg_env=1)), ("ICW_K1_WG", "1", dict(k1_wg=1, k1_wg_env=1)),
    ("ICW_K1_WG", "5", {}), ("ICW_K1_WG", "0", {}),
    ("ICW_FIR_RAMP", "2.5", dict(fir_ramp=2.5)), ("ICW_FIR_RAMP", "16", dict(fir_ramp=16.0)),
    ("ICW_FIR_RAMP", "1.0", {}), ("ICW_FIR_RAMP", "16.5", {}),
    ("ICW_REST_CUS", "0", dict(rest_cus=0)), ("ICW_REST_CUS", "8", dict(rest_cus=8)),
    ("ICW_REST_CUS", "160", dict(rest_cus=160)), ("ICW_REST_CUS", "4", {}), ("ICW_REST_CUS", "-8", {}),
    ("ICW_BLOCK", "256", dict(max_block=256, block_env=1)), ("ICW_BLOCK", "65536", dict(max_block=65536, block_env=1)),
    ("ICW_BLOCK", "255", {}), ("ICW_BLOCK", "65537", {}),
    ("ICW_SETS", "3", dict(max_sets=3)), ("ICW_SETS", "2", {}), ("ICW_SETS", "1", {}), ("ICW_SETS", "4", {}),
    ("ICW_ZEROCOPY", "0", dict(zero_copy=0)), ("ICW_ZEROCOPY", "1", {}),
    ("ICW_SPIN", "0", dict(spin_wait=0)), ("ICW_SPIN", "1", {}),
    ("ICW_FIRST_BLOCK", "0", dict(first_block=0, first_block_env=1)),
    ("ICW_FIRST_BLOCK", "2048", dict(first_block=2048, first_block_env=1)), ("ICW_FIRST_BLOCK", "-1", {}),
    ("ICW_TAPER", "0.5", dict(taper=0.5)), ("ICW_TAPER", "0", dict(taper=0.0)), ("ICW_TAPER", "1.0", {}),
    ("ICW_TAPER", "-0.5", {}),
    ("ICW_TAPER_MIN", "64", dict(taper_min=64)), ("ICW_TAPER_MIN", "63", {}),
    ("ICW_DEDUP", "0", dict(dedup_ok=0)), ("ICW_DEDUP", "1", {}),
    ("ICW_FILL_DRAIN", "0", dict(fill_drain=0)), ("ICW_FILL_DRAIN", "1", {}),
    ("ICW_FIR_FUSED", "0", dict(fir_fuse=0)), ("ICW_FIR_FUSED", "1", {}),
    ("ICW_CHAIN", "0", dict(chain_ok=0)), ("ICW_CHAIN", "1", {}),
    ("ICW_STREAM1", "0", dict(stream1=0)), ("ICW_STREAM1", "1", {}),
    ("ICW_S1_OVL", "0", dict(s1_ovl=0)), ("ICW_S1_OVL", "1", {}),
    ("ICW_S1_STAMPS", "1", dict(s1_stamps=1)), ("ICW_S1_STAMPS", "0", {}),
    # these three are numbers: off when atoi gives 0 (so "" and "00" too), on otherwise
    ("ICW_K3R_SPEC", "0", dict(k3r_spec=0)), ("ICW_K3R_SPEC", "", dict(k3r_spec=0)), ("ICW_K3R_SPEC", "1", {}),
    ("ICW_DITH_PAR", "0", dict(dith_par=0)), ("ICW_DITH_PAR", "00", dict(dith_par=0)), ("ICW_DITH_PAR", "2", {}),
    ("ICW_FIR_SIG", "0", dict(fir_sig=0)), ("ICW_FIR_SIG", "1", {}),
]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("tuning")
    (d / "t.cpp").write_text(SRC)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "in_cwave_amd" / "csrc"), "-o", str(d / "t"),
                    str(d / "t.cpp")], check=True)
    return d / "t"


def read(exe, env, *args):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("ICW_")}
    clean.update(env)
    out = subprocess.run([str(exe), *args], env=clean, capture_output=True, text=True, check=True).stdout
    return [{k: float(v) for k, v in (f.split("=") for f in ln.split())} for ln in out.splitlines()]


def test_covers_the_25_switches():
    assert len({c[0] for c in CASES}) == 25
    for name in {c[0] for c in CASES}:
        vals = [c for c in CASES if c[0] == name]
        assert any(c[2] for c in vals), name            # an accepted value


def test_defaults(exe):
    assert read(exe, {}) == [DEFAULTS]


@pytest.mark.parametrize("name,value,change", CASES, ids=["%s=%s" % (c[0], c[1]) for c in CASES])
def test_switch(exe, name, value, change):
    assert read(exe, {name: value}) == [dict(DEFAULTS, **change)]


def test_read_twice_in_one_process(exe):
    """the regression for the latched static: the second read sees the changed ICW_DITH_PAR"""
    a, b = read(exe, {"ICW_DITH_PAR": "1"}, "ICW_DITH_PAR", "0")
    assert (a["dith_par"], b["dith_par"]) == (1, 0)
    a, b = read(exe, {"ICW_DITH_PAR": "0"}, "ICW_DITH_PAR", "1")
    assert (a["dith_par"], b["dith_par"]) == (0, 1)
