"""CPU tests of the direct-FFT CWAVE encoder's host side: the ABI mirror, every refusal of
icw_encode_cwave_fft (each comes back before a device is touched -- this machine has none), the workspace
and pass queries, and the file layer's refusals.  No GPU call is made here."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from in_cwave_amd import abi, synth
from in_cwave_amd import lib as L

import wavgen as W

ROOT = Path(__file__).resolve().parents[1]
U64 = C.c_uint64


def u64(*v):
    return (U64 * max(1, len(v)))(*v)


def call(n_frames=(100,), fmt=abi.FMT_I16, channels=2, cw_format=abi.FMT_CW_F64, flags=0, opts=abi.FftEncOpts(-1, 0),
         inp=True, out=True, ioff=True, ooff=True, nfr=True, n=None):
    """icw_encode_cwave_fft on host buffers big enough for the tracks; returns (rc, out bytes, clipped)"""
    lib = L.load()
    n = len(n_frames) if n is None else n
    tot = int(sum(min(int(v), 1 << 16) for v in n_frames))
    src = np.full(tot * 16 + 16, 7, np.uint8)
    dst = np.zeros(tot * 32 + 16, np.uint8)
    clipped = u64(*([99] * len(n_frames)))
    offs = u64(*([0] * len(n_frames)))
    rc = lib.icw_encode_cwave_fft(src.ctypes.data if inp else None, offs if ioff else None,
                                  u64(*n_frames) if nfr else None, n, fmt, channels, dst.ctypes.data if out else None,
                                  offs if ooff else None, cw_format, clipped, flags,
                                  C.byref(opts) if opts is not None else None, None)
    return rc, dst, [clipped[i] for i in range(len(n_frames))]


def test_symbols_signatures_and_constants():
    lib = L.load()
    for name in ("icw_encode_cwave_fft", "icw_encode_cwave_fft_workspace", "icw_encode_cwave_fft_passes",
                 "icw_cwave_encode_files_fft"):
        assert name in abi.SIGNATURES and hasattr(lib, name)
    for name in ("encode_cwave_fft", "encode_cwave_fft_device", "cwave_encode_files_fft", "encode_cwave_fft_workspace",
                 "encode_cwave_fft_passes"):
        assert hasattr(L, name)
    hdr = (ROOT / "include" / "icw_cwave.h").read_text()
    assert int(re.search(r"#define ICW_FFT_MAX_LOG2 (\d+)", hdr).group(1)) == abi.FFT_MAX_LOG2 == 27
    assert C.sizeof(abi.FftEncOpts) == 8 and abi.FftEncOpts.max_pass_log2.offset == 4
    o = abi.CwaveEncFftOpts
    assert C.sizeof(o) == 16 and (o.cw_format.offset, o.device.offset, o.max_bytes.offset) == (0, 4, 8)
    assert lib.icw_abi_version() == 2                        # functions were only added
    # the headers no longer list the converter as missing
    for h in ("icw_cwave.h", "icw_reader.h"):
        assert "Not covered: the direct-FFT" not in (ROOT / "include" / h).read_text()


@pytest.mark.parametrize("bad", [
    dict(fmt=abi.FMT_CW_F64), dict(fmt=abi.FMT_CW_F32), dict(fmt=99), dict(channels=0),
    dict(cw_format=abi.FMT_F32), dict(cw_format=abi.FMT_CW_F32 + 1), dict(cw_format=0),
    dict(n_frames=(1,)), dict(n_frames=(0,)), dict(n_frames=(100, 1, 100)),
    dict(inp=False), dict(out=False), dict(ioff=False), dict(ooff=False), dict(nfr=False), dict(n=-1),
    dict(flags=abi.F_DEBUG_PRE), dict(flags=abi.F_TIMING), dict(flags=abi.F_DEVICE_PTRS | abi.F_DEBUG_INPUT), dict(flags=16),
    dict(opts=abi.FftEncOpts(-1, -1)), dict(opts=abi.FftEncOpts(-1, 1)),
    dict(n_frames=((1 << 27) + 1, 1)),                       # a bad track beside a long one: EINVAL comes first
])
def test_einval_without_a_device(bad):
    rc, dst, clipped = call(**bad)
    assert rc == abi.EINVAL
    assert not dst.any() and clipped == [99] * len(clipped)  # nothing ran, nothing was written


@pytest.mark.parametrize("n_frames", [((1 << 27) + 1,), (100, 1 << 28), (1 << 32,), ((1 << 32) + 5, 100), ((1 << 63),)])
@pytest.mark.parametrize("flags", [0, abi.F_DEVICE_PTRS])
def test_eunsupported_without_a_device(n_frames, flags):
    rc, dst, clipped = call(n_frames=n_frames, flags=flags)
    assert rc == abi.EUNSUPPORTED
    assert not dst.any() and clipped == [99] * len(clipped)


def test_passes_query():
    P = L.encode_cwave_fft_passes
    assert [P(n) for n in (2, 3, 128, 129, 1 << 14, (1 << 14) + 1, 1 << 20, 1 << 21, (1 << 21) + 1, 1 << 27)] == \
        [1, 1, 1, 2, 2, 3, 3, 3, 4, 4]
    assert [P(128, c) for c in (2, 3, 4, 7, 8, 100)] == [4, 3, 2, 1, 1, 1]
    assert [P(4096, c) for c in (4, 7, 0)] == [3, 2, 2]
    lib = L.load()
    assert lib.icw_encode_cwave_fft_passes(1, 0) == abi.EINVAL
    assert lib.icw_encode_cwave_fft_passes(100, 1) == abi.EINVAL
    assert lib.icw_encode_cwave_fft_passes(100, -3) == abi.EINVAL
    assert lib.icw_encode_cwave_fft_passes((1 << 27) + 1, 0) == abi.EUNSUPPORTED
    with pytest.raises(L.IcwError):
        P(1)


def test_workspace_query():
    Wk = L.encode_cwave_fft_workspace
    per = 40                                                 # bookkeeping bytes per track
    assert Wk([2]) == 16 * 2 + per
    assert Wk([3]) == 16 * 4 + per
    assert Wk([4096, 4097, 5000]) == 16 * (4096 + 8192 + 8192) + 3 * per
    assert Wk([1 << 20] * 256) == 256 * ((16 << 20) + per)
    assert Wk([1 << 27]) == (2 << 30) + per                  # 2 GiB of complex doubles per track of the largest P
    assert Wk([1 << 20], channels=1) == Wk([1 << 20], channels=2)
    assert Wk([]) == 0
    assert Wk([1]) == 0 and Wk([100, 1]) == 0 and Wk([(1 << 27) + 1]) == 0 and Wk([100], channels=0) == 0


# ------------------------------------------------------------------ files
def test_files_bad_options_write_nothing(tmp_path):
    src = W.write(tmp_path / "in.wav", synth.stream_pcm(0, 100, 48000), abi.FMT_I16, 2, 48000)
    dst = tmp_path / "never.cwave"
    for bad in (abi.FMT_I16, abi.FMT_CW_F32 + 1, 0):
        rc, st, status, clipped = L.cwave_encode_files_fft([src], [dst], cw_format=bad)
        assert rc == abi.EINVAL and not dst.exists()
        assert st.n_files == 0 and st.n_groups == 0


def test_files_null_arguments(tmp_path):
    lib = L.load()
    o = abi.CwaveEncFftOpts(abi.FMT_CW_F64, -1, 0)
    paths = (C.c_char_p * 1)(str(tmp_path / "x.wav").encode())
    assert lib.icw_cwave_encode_files_fft(paths, paths, 1, None, None, None, None) == abi.EINVAL
    assert lib.icw_cwave_encode_files_fft(None, paths, 1, C.byref(o), None, None, None) == abi.EINVAL
    assert lib.icw_cwave_encode_files_fft(paths, None, 1, C.byref(o), None, None, None) == abi.EINVAL
    assert lib.icw_cwave_encode_files_fft(paths, paths, -1, C.byref(o), None, None, None) == abi.EINVAL
    st = abi.BatchStats()
    assert lib.icw_cwave_encode_files_fft(None, None, 0, C.byref(o), C.byref(st), None, None) == abi.OK
    assert st.n_files == 0 and st.n_groups == 0
    assert not list(tmp_path.iterdir())


def test_files_refused_inputs_never_reach_a_device(tmp_path):
    """a CWAVE input, a WAV the parser refuses, fewer than 2 frames, a missing file: each gets ICW_EINVAL, no
    output file appears and no group is formed (so no device call is made)"""
    cw = tmp_path / "already.cwave"
    hdr = b"cPLXwAVE" + np.array([48, 2, 1, 2, 10, 48000, 0, 0], "<u4").tobytes() + np.float64(0.0).tobytes()
    cw.write_bytes(hdr + bytes(10 * 8))
    assert L.wav_parse_file(cw).fmt == abi.FMT_CW_I16
    broken = tmp_path / "broken.wav"
    broken.write_bytes(b"RIFF\0\0\0\0WAVEjunk")
    short = W.write(tmp_path / "short.wav", synth.stream_pcm(0, 1, 48000), abi.FMT_I16, 2, 48000)
    ins = [cw, broken, short, tmp_path / "missing.wav"]
    outs = [tmp_path / f"out_{i}.cwave" for i in range(len(ins))]
    rc, st, status, clipped = L.cwave_encode_files_fft(ins, outs)
    assert rc == abi.EINVAL and status == [abi.EINVAL] * 4 and clipped == [0] * 4
    assert st.n_files == 0 and st.n_groups == 0 and st.frames_in == 0 and st.frames_out == 0
    assert not any(o.exists() for o in outs)
