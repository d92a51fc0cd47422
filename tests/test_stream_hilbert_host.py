"""CPU: the host-only side of per-stream Hilbert converters -- the two entry points are exported and bound,
and a NULL handle is ICW_EINVAL before anything touches a device."""
import re
import subprocess
from pathlib import Path

from in_cwave_amd import abi

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("icw_set_stream_hilbert", "icw_stream_hilbert_count")


def test_abi_symbols_present():
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "in_cwave_amd" / "libicw.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    hdr = (ROOT / "include" / "icw.h").read_text()
    for n in NAMES:
        assert n in exported and n in abi.SIGNATURES and re.search(r"^int %s\(" % n, hdr, flags=re.M), n


def test_null_handle_is_einval():
    from in_cwave_amd import lib as L
    l = L.load()
    assert l.icw_set_stream_hilbert(None, 0, 1, 1, 1, 1) == abi.EINVAL
    assert l.icw_stream_hilbert_count(None) == abi.EINVAL
