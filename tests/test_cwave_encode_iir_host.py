"""CPU tests of the IIR-Hilbert CWAVE encoder's host side: the ABI mirror of the two entry points and of
icw_cwave_enc_iir_opts, and the refusals that return before any device call -- no GPU call is made here."""
import ctypes as C

import numpy as np
import pytest

from in_cwave_amd import abi, synth
from in_cwave_amd import lib as L

import wavgen as W


def test_symbols_and_signatures():
    lib = L.load()
    for name in ("icw_encode_cwave_iir", "icw_cwave_encode_files_iir"):
        assert name in abi.SIGNATURES and hasattr(lib, name)
    # the same call shape as the FIR encoder's entry points
    assert abi.SIGNATURES["icw_encode_cwave_iir"] == abi.SIGNATURES["icw_encode_cwave"]
    res, args = abi.SIGNATURES["icw_cwave_encode_files_iir"]
    fres, fargs = abi.SIGNATURES["icw_cwave_encode_files"]
    assert res == fres and args[:3] == fargs[:3] and args[4:] == fargs[4:]
    assert args[3] == C.POINTER(abi.CwaveEncIirOpts)
    assert hasattr(L.Context, "encode_cwave_iir") and hasattr(L.Context, "encode_cwave_iir_device")
    assert lib.icw_abi_version() == 2                        # functions were only added


def test_options_struct_layout():
    """icw_cwave_enc_iir_opts (include/icw_reader.h): seven 4-byte fields, no padding"""
    o = abi.CwaveEncIirOpts
    names = ["hilbert_type", "iir_kahan", "iir_subnorm_reject", "cw_format", "block_frames", "device", "reserved_"]
    assert [f[0] for f in o._fields_] == names
    assert C.sizeof(o) == 28 and C.alignment(o) == 4
    assert [getattr(o, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 24]
    assert o.hilbert_type.size == o.cw_format.size == 4
    v = o(5, 1, 0, abi.FMT_CW_I16_F32, 4096, -1, 0)
    assert (v.hilbert_type, v.iir_kahan, v.iir_subnorm_reject, v.cw_format, v.block_frames, v.device) == \
        (5, 1, 0, abi.FMT_CW_I16_F32, 4096, -1)


def test_null_context_is_refused():
    lib = L.load()
    buf = np.zeros(64, np.uint8)
    for flags in (0, abi.F_DEVICE_PTRS):
        assert lib.icw_encode_cwave_iir(None, 0, 1, buf.ctypes.data, 64, buf.ctypes.data, 64, 4, abi.FMT_CW_F64,
                                        flags, None) == abi.EINVAL
    assert not buf.any()


@pytest.mark.parametrize("bad", [dict(hilbert_type=6), dict(hilbert_type=0xFFFFFFFF), dict(iir_kahan=2),
                                 dict(iir_kahan=-1), dict(iir_subnorm_reject=2), dict(cw_format=abi.FMT_I16),
                                 dict(cw_format=abi.FMT_CW_F32 + 1), dict(block_frames=-1)])
def test_files_bad_options_write_nothing(tmp_path, bad):
    src = W.write(tmp_path / "in.wav", synth.stream_pcm(0, 100, 48000), abi.FMT_I16, 2, 48000)
    dst = tmp_path / "never.cwave"
    rc, st, status, clipped = L.cwave_encode_files_iir([src], [dst], **bad)
    assert rc == abi.EINVAL and not dst.exists()
    assert st.n_files == 0 and st.n_groups == 0


def test_files_null_arguments(tmp_path):
    lib = L.load()
    o = abi.CwaveEncIirOpts(1, 1, 1, abi.FMT_CW_F64, 0, -1, 0)
    paths = (C.c_char_p * 1)(str(tmp_path / "x.wav").encode())
    assert lib.icw_cwave_encode_files_iir(paths, paths, 1, None, None, None, None) == abi.EINVAL
    assert lib.icw_cwave_encode_files_iir(None, paths, 1, C.byref(o), None, None, None) == abi.EINVAL
    assert lib.icw_cwave_encode_files_iir(paths, None, 1, C.byref(o), None, None, None) == abi.EINVAL
    assert lib.icw_cwave_encode_files_iir(paths, paths, -1, C.byref(o), None, None, None) == abi.EINVAL
    # no files: nothing to do, and no device is touched
    st = abi.BatchStats()
    assert lib.icw_cwave_encode_files_iir(None, None, 0, C.byref(o), C.byref(st), None, None) == abi.OK
    assert st.n_files == 0 and st.n_groups == 0
    assert not list(tmp_path.iterdir())
