"""GPU: icw_cwave_encode_files / icw_cwave_encode_files_iir with ICW_ENC_MERGE_INPUTS -- every accepted file in
one context, each stream given its file's input -- against the same call with the flag 0 (one context per
(rate, format, channels) group).  The files written must be byte-identical, header and n_CRC32 included.

Eight WAV files of 2 000 - 5 000 frames over four shapes; block_frames 1 000 gives up to five blocks per file,
files that end inside different blocks (the per-block CRC lengths use each file's own frame size) and, beside
the 32-byte frames of the stereo files, mono rows whose 6-byte frames start off the 16-byte grid."""
import numpy as np
import pytest

from in_cwave_amd import abi, synth
from in_cwave_amd import lib as L

import wavgen as W

pytestmark = pytest.mark.gpu

SHAPES = [(abi.FMT_I16, 2, 44100), (abi.FMT_I24, 1, 48000), (abi.FMT_F32, 2, 96000), (abi.FMT_I16, 1, 48000)]
FRAMES = [2000, 3100, 4999, 2503, 5000, 2001, 3777, 4096]
BLOCK = 1000


@pytest.fixture(scope="module")
def wavs(tmp_path_factory):
    d = tmp_path_factory.mktemp("merged_wavs")
    files = []
    for i, n in enumerate(FRAMES):
        fmt, ch, fs = SHAPES[i % 4]
        sig = synth.stream_pcm(i, n, fs, channels=ch, fmt=abi.FMT_F32).view("<f4").astype(np.float64) * 2.5
        if fmt == abi.FMT_F32:                               # hot masters: the int16 formats clip
            data = sig.astype("<f4").view(np.uint8)
        elif fmt == abi.FMT_I16:
            data = np.clip(np.round(sig * 32767.0), -32768, 32767).astype("<i2").view(np.uint8)
        else:
            q = np.clip(np.round(sig * 8388607.0), -8388608, 8388607).astype("<i4")
            data = np.ascontiguousarray(q.view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)
        files.append(W.write(d / f"in_{i}.wav", data, fmt, ch, fs, kind="float" if fmt == abi.FMT_F32 else "pcm"))
    return files


def encode(kind, ins, outs, cw_format, merge, align=0):
    if kind == "iir":
        return L.cwave_encode_files_iir(ins, outs, 1, 1, 1, cw_format, block_frames=BLOCK, merge_inputs=merge)
    return L.cwave_encode_files(ins, outs, 30, 8.0, cw_format, align=align, block_frames=BLOCK, merge_inputs=merge)


@pytest.mark.parametrize("cw_format", [abi.FMT_CW_F64, abi.FMT_CW_I16_F32])
@pytest.mark.parametrize("kind,align", [("iir", 0), ("fir", 0), ("fir", 1)])
def test_merged_files_equal_grouped_files(icw, wavs, tmp_path, kind, align, cw_format):
    broken = tmp_path / "broken.wav"
    broken.write_bytes(b"RIFF\0\0\0\0WAVEjunk")
    ins = wavs[:3] + [broken] + wavs[3:]
    res = {}
    for merge in (False, True):
        outs = [tmp_path / f"{'m' if merge else 'g'}_{i}.cwave" for i in range(len(ins))]
        rc, st, status, clipped = encode(kind, ins, outs, cw_format, merge, align)
        assert rc == abi.EINVAL                              # the unreadable file's status; the rest completes
        assert status == [abi.OK] * 3 + [abi.EINVAL] + [abi.OK] * 5
        assert st.n_files == len(wavs) and st.frames_out == sum(FRAMES)
        res[merge] = (outs, st, clipped)
    assert res[False][1].n_groups == 4 and res[True][1].n_groups == 1
    assert res[False][2] == res[True][2]
    assert res[False][1].frames_in == res[True][1].frames_in
    if cw_format == abi.FMT_CW_I16_F32:
        assert sum(c > 0 for c in res[True][2]) >= 2         # hot masters: some files clip
    for i, (g, m) in enumerate(zip(res[False][0], res[True][0])):
        if i == 3:
            continue
        gb, mb = g.read_bytes(), m.read_bytes()
        assert gb == mb, f"file {i}: merged output differs from the grouped one"
        n = FRAMES[i if i < 3 else i - 1]
        fmt, ch, fs = SHAPES[(i if i < 3 else i - 1) % 4]
        assert len(mb) == 48 + n * L.cwave_frame_bytes(cw_format, ch)
        hdr = np.frombuffer(mb[:48], np.uint8)
        assert int(hdr[20:24].view("<u4")[0]) == ch and int(hdr[28:32].view("<u4")[0]) == fs
        crc, ok = L.cwave_check(np.frombuffer(mb, np.uint8).copy())
        assert ok == 1
