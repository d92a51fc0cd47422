"""GPU: the direct-FFT CWAVE encoder (icw_encode_cwave_fft, kernel KX `icw_fft_pass`; icw_cwave_encode_files_fft).

The converter's definition is the project's (include/icw_cwave.h), restated in long double by cwfft_ref.py
(pinned on the CPU by test_cwave_fft_ref.py):
  1. accuracy: I bit for bit the unpacked samples; max|Q - reference| <= max(4 e_np, 2^-52 log2(P) max|reference|),
     e_np = numpy.fft's float64 deviation from the same reference -- a bound from the reference side only;
  2. pass structure: the same check with the sub-transform capped so that a transform runs as one to six
     passes (among them blocks narrower than a tile before the last pass, and a one-stage pass), the pass count
     the plan reports, and equal bytes from two runs;
  3. every input format x mono / stereo / 3 channels; the lossy formats == cwenc_ref.frames of the F64 frames'
     I / Q, and the clip count;
  4. a track's bytes do not depend on the call's other tracks or on the pointer kind;
  5. sign and scale on a single-bin cosine;
  6. files: header, CRC, the reader, decode of the F64 file == oracle.Stream on the same frames, refusals.
Input: fixed seeds, int16 PCM uniform in +-30000.  Lengths: 2 and 3 (P = 2, 4: no twiddle is irrational), around
64 and 4096 (a power of two, one more, one less than a tile), 5000 and 40000 (two passes at the default cap;
40000 spans 32 workgroups per pass).
"""
import struct
import zlib

import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth
from in_cwave_amd import lib as L

import cwenc_ref
import cwfft_ref as R
import wavgen as W

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 50, 64, 65, 4096, 4097, 5000, 40000]
LOSSY = [abi.FMT_CW_I16, abi.FMT_CW_I16_F32, abi.FMT_CW_F32]


class Track:
    """a stereo int16 track of n frames with its long-double reference and tolerance per channel"""

    def __init__(self, n, seed):
        self.n = n
        self.raw = R.random_pcm16(np.random.default_rng(seed), n, 2)
        self.x = cwenc_ref.unpack(self.raw, abi.FMT_I16, 2)
        self.q = [R.hilbert_q(self.x[:, c]) for c in range(2)]
        self.tol = [R.tolerance(self.x[:, c], self.q[c]) for c in range(2)]


@pytest.fixture(scope="module")
def tracks():
    """computed once, shared by the tests, never modified"""
    return {n: Track(n, 1000 + n) for n in sorted(set(SIZES + [128, 1024, 2048, 32768]))}


def check_accuracy(t, frames, what=""):
    I, Q = cwenc_ref.iq_of_f64_frames(frames, 2)
    assert I.shape == (t.n, 2), what
    assert np.array_equal(I.view(np.uint64), t.x.view(np.uint64)), f"{what}: I is not the unpacked sample"
    for c in range(2):
        err = float(np.max(np.abs(Q[:, c].astype(np.longdouble) - t.q[c])))
        bound, e_np = t.tol[c]
        print(f"{what} N {t.n} P {R.pad_len(t.n)} ch {c}: err {err:.3e} e_np {e_np:.3e} bound {bound:.3e} "
              f"ratio to e_np {err / e_np if e_np else float('nan'):.2f}")
        assert err <= bound, f"{what} N {t.n} ch {c}: {err} > {bound} (e_np {e_np})"


# ------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("n", SIZES)
def test_accuracy(icw, tracks, n):
    t = tracks[n]
    (frames,), (clipped,) = L.encode_cwave_fft([t.raw], abi.FMT_I16, 2)
    assert frames.size == n * 32 and clipped == 0
    check_accuracy(t, frames, "default")


# ------------------------------------------------------------------ 2. pass structure
@pytest.mark.parametrize("n,cap,passes", [(128, 4, 2), (128, 7, 1), (128, 0, 1), (128, 3, 3), (128, 2, 4),
                                          (4096, 4, 3), (4096, 7, 2), (4096, 0, 2),
                                          (1024, 5, 2), (1024, 6, 2), (32768, 5, 3), (32768, 3, 5), (2048, 2, 6)])
def test_pass_structure(icw, tracks, n, cap, passes):
    t = tracks[n]
    assert L.encode_cwave_fft_passes(n, cap) == passes
    (a,), _ = L.encode_cwave_fft([t.raw], abi.FMT_I16, 2, max_pass_log2=cap)
    (b,), _ = L.encode_cwave_fft([t.raw], abi.FMT_I16, 2, max_pass_log2=cap)
    assert np.array_equal(a, b)                              # deterministic
    check_accuracy(t, a, f"cap {cap}")


# ------------------------------------------------------------------ 3. formats
def _pcm(fmt, ch, n, seed):
    rng = np.random.default_rng(seed)
    v = rng.integers(-30000, 30001, size=n * ch)
    if fmt == abi.FMT_U8:
        return ((v >> 8) + 128).astype(np.uint8)
    if fmt == abi.FMT_I16:
        return v.astype("<i2").view(np.uint8).copy()
    if fmt == abi.FMT_I24:
        w = (v * 256 + rng.integers(0, 256, size=v.size)).astype("<i4")
        return np.ascontiguousarray(w.view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)
    if fmt == abi.FMT_I32:
        return (v * 65536 + rng.integers(0, 65536, size=v.size)).astype("<i4").view(np.uint8).copy()
    return (v / 32768.0).astype("<f4").view(np.uint8).copy()


@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("fmt", [abi.FMT_U8, abi.FMT_I16, abi.FMT_I24, abi.FMT_I32, abi.FMT_F32])
def test_every_input_format(icw, fmt, ch):
    n = 1000
    raw = _pcm(fmt, ch, n, 50 + fmt * 4 + ch)
    x = cwenc_ref.unpack(raw, fmt, ch)                       # the first two channels
    nc = x.shape[1]
    (frames,), _ = L.encode_cwave_fft([raw], fmt, ch)
    assert frames.size == n * 16 * nc == n * L.cwave_frame_bytes(abi.FMT_CW_F64, ch)
    I, Q = cwenc_ref.iq_of_f64_frames(frames, nc)
    assert np.array_equal(I.view(np.uint64), x.view(np.uint64))
    for c in range(nc):
        q = R.hilbert_q(x[:, c])
        bound, e_np = R.tolerance(x[:, c], q)
        err = float(np.max(np.abs(Q[:, c].astype(np.longdouble) - q)))
        assert err <= bound, (c, err, bound, e_np)


@pytest.fixture(scope="module")
def loud(icw):
    """full-scale squares: the Hilbert pair of an edge overshoots int16.  (raw, F64 frames) per channel count"""
    res = {}
    for ch in (1, 2):
        k = np.arange(1000)
        cols = [np.where((k // (37 + 5 * c)) % 2 == 0, 32767, -32768) for c in range(ch)]
        raw = np.stack(cols, axis=1).astype("<i2").reshape(-1).view(np.uint8).copy()
        (f64,), (cl,) = L.encode_cwave_fft([raw], abi.FMT_I16, ch)
        assert cl == 0                                       # F64 frames clip nothing
        res[ch] = (raw, f64)
    return res


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("cw_format", LOSSY)
def test_lossy_formats_equal_the_restatement(icw, loud, cw_format, ch):
    raw, f64 = loud[ch]
    I, Q = cwenc_ref.iq_of_f64_frames(f64, ch)
    ref, clipped = cwenc_ref.frames(I, Q, cw_format)
    if cw_format == abi.FMT_CW_F32:
        clipped = 0
    elif cw_format == abi.FMT_CW_I16:
        assert clipped > 0                                   # Q overshoots; I16+F32 quantises I alone, which fits
    (got,), (cl,) = L.encode_cwave_fft([raw], abi.FMT_I16, ch, cw_format)
    assert np.array_equal(got, ref)
    assert cl == clipped


# ------------------------------------------------------------------ 4. batch independence, pointer kinds
@pytest.mark.parametrize("cw_format", [abi.FMT_CW_F64, abi.FMT_CW_I16_F32])
def test_batch_and_pointer_independence(icw, cw_format):
    import torch
    sizes = [2, 4097, 300, 40000]
    raws = [R.random_pcm16(np.random.default_rng(77 + i), n, 2) * 1 for i, n in enumerate(sizes)]
    fb = L.cwave_frame_bytes(cw_format, 2)
    together, clip_t = L.encode_cwave_fft(raws, abi.FMT_I16, 2, cw_format)
    for i, raw in enumerate(raws):
        (alone,), (cl,) = L.encode_cwave_fft([raw], abi.FMT_I16, 2, cw_format)
        assert alone.size == sizes[i] * fb
        assert np.array_equal(alone, together[i]), f"track {i}"
        assert cl == clip_t[i]
    # device pointers; the frames at odd offsets with gaps between the tracks
    d_in = torch.from_numpy(np.concatenate(raws)).cuda()
    ioff = np.concatenate([[0], np.cumsum([r.size for r in raws])])[:-1]
    ooff, o = [], 3
    for n in sizes:
        ooff.append(o)
        o += n * fb + 5
    d_out = torch.zeros(o + 16, dtype=torch.uint8, device="cuda")
    clip_d = L.encode_cwave_fft_device(d_in, ioff, sizes, abi.FMT_I16, 2, d_out, ooff, cw_format)
    got = d_out.cpu().numpy()
    covered = np.zeros(got.size, bool)
    for i, n in enumerate(sizes):
        assert np.array_equal(got[ooff[i]:ooff[i] + n * fb], together[i]), f"track {i}"
        covered[ooff[i]:ooff[i] + n * fb] = True
    assert not got[~covered].any()                           # nothing outside the frames
    assert clip_d == clip_t


# ------------------------------------------------------------------ 5. sign and scale
def test_cosine_gives_the_sine(icw):
    P, k, A = 4096, 37, 20000.0
    theta = 2 * R.PI * (np.asarray(np.arange(P) * k % P, dtype=np.longdouble) / P)
    raw = (A * np.cos(theta) / 32768).astype("<f4").view(np.uint8).copy()
    x = cwenc_ref.unpack(raw, abi.FMT_F32, 1)[:, 0]
    (frames,), _ = L.encode_cwave_fft([raw], abi.FMT_F32, 1)
    I, Q = cwenc_ref.iq_of_f64_frames(frames, 1)
    assert np.array_equal(I[:, 0].view(np.uint64), x.view(np.uint64))
    q = R.hilbert_q(x)
    bound, e_np = R.tolerance(x, q)
    assert float(np.max(np.abs(Q[:, 0].astype(np.longdouble) - q))) <= bound
    # the input is the cosine rounded to float32 (relative 2^-24): Q is the sine to that accuracy, +sin not -sin
    assert float(np.max(np.abs(Q[:, 0].astype(np.longdouble) - A * np.sin(theta)))) < A * 2.0 ** -24 * 12


# ------------------------------------------------------------------ 6. files
SPECS = [("a.wav", abi.FMT_I16, 2, 48000, 5000), ("b.wav", abi.FMT_F32, 1, 44100, 3001),
         ("c.rwave", abi.FMT_I24, 2, 96000, 2222)]


def _make_wavs(tmp_path):
    files = []
    for i, (name, fmt, ch, fs, n) in enumerate(SPECS):
        d = synth.stream_pcm(i, n, fs, channels=ch, fmt=fmt)
        W.write(tmp_path / name, d, fmt, ch, fs, kind="float" if fmt == abi.FMT_F32 else "pcm")
        files.append((tmp_path / name, fmt, ch, fs, n, d))
    return files


def _check_file(path, fmt_cw, ch, fs, n):
    img = np.frombuffer(path.read_bytes(), np.uint8)
    fb = abi.FMT_BYTES[fmt_cw] * ch
    info = L.wav_parse_file(path)
    assert (info.fmt, info.channels, info.sample_rate, info.frame_bytes, info.n_samples, info.data_offset,
            info.htype) == (fmt_cw, ch, fs, fb, n, 48, abi.HTYPE_CWAVE)
    magic, hsize, ver, hfmt, hch, hn, hrate, hM, hcrc, hbeta = struct.unpack("<8s6IiId", img[:48].tobytes())
    assert (magic, hsize, ver, hfmt, hch, hn, hrate, hM) == (b"cPLXwAVE", 48, 2, fmt_cw - abi.FMT_CW_F64, ch, n, fs, -1)
    assert img[40:48].tobytes() == struct.pack("<d", 0.0)
    data = img[48:]
    assert data.size == n * fb
    assert zlib.crc32(data.tobytes()) == hcrc
    assert L.cwave_check(img.copy()) == (hcrc, 1)
    return data.copy()


@pytest.mark.parametrize("cw_format", [abi.FMT_CW_F64, abi.FMT_CW_I16_F32])
def test_encode_files(tmp_path, icw, cw_format):
    files = _make_wavs(tmp_path)
    broken = tmp_path / "broken.wav"
    broken.write_bytes(b"RIFF\0\0\0\0WAVEjunk")
    ins = [files[0][0], broken, files[1][0], files[2][0]]
    outs = [tmp_path / f"out_{i}.cwave" for i in range(len(ins))]
    rc, st, status, clipped = L.cwave_encode_files_fft(ins, outs, cw_format)
    assert status == [abi.OK, abi.EINVAL, abi.OK, abi.OK] and rc == abi.EINVAL   # a refused file leaves the others done
    assert st.n_files == 3 and st.n_groups == 3
    assert st.frames_in == st.frames_out == sum(f[4] for f in files)
    assert not outs[1].exists() and clipped == [0] * 4
    for (path, fmt, ch, fs, n, d), out in zip(files, [outs[0], outs[2], outs[3]]):
        data = _check_file(out, cw_format, ch, fs, n)
        (ref,), _ = L.encode_cwave_fft([d], fmt, ch, cw_format)
        assert np.array_equal(data, ref), path.name


def test_files_group_by_format_not_rate_and_fit_max_bytes(tmp_path, icw):
    """three int16 stereo files of three rates are one group; a small max_bytes splits it into calls without
    changing a byte"""
    ins, outs, small = [], [], []
    for i, (fs, n) in enumerate([(44100, 700), (48000, 3000), (96000, 129)]):
        ins.append(W.write(tmp_path / f"r{i}.wav", synth.stream_pcm(i, n, fs), abi.FMT_I16, 2, fs))
        outs.append(tmp_path / f"r{i}.cwave")
        small.append(tmp_path / f"s{i}.cwave")
    rc, st, status, _ = L.cwave_encode_files_fft(ins, outs)
    assert rc == abi.OK and status == [abi.OK] * 3 and st.n_groups == 1 and st.n_files == 3
    rc, st, status, _ = L.cwave_encode_files_fft(ins, small, max_bytes=1)
    assert rc == abi.OK and status == [abi.OK] * 3 and st.n_groups == 1
    for a, b, fs in zip(outs, small, (44100, 48000, 96000)):
        assert a.read_bytes() == b.read_bytes()
        assert L.wav_parse_file(a).sample_rate == fs


def test_decode_of_the_file_equals_the_oracle(tmp_path, icw, oracle):
    """the F64 file through a context with ICW_FMT_CW_F64 input and Shift + Master == oracle.Stream fed the
    same file frames"""
    fs, n = 48000, 3000
    src = W.write(tmp_path / "in.wav", synth.stream_pcm(3, n, fs), abi.FMT_I16, 2, fs)
    dst = tmp_path / "in.cwave"
    rc, _, status, _ = L.cwave_encode_files_fft([src], [dst])
    assert rc == abi.OK and status == [abi.OK]
    data = _check_file(dst, abi.FMT_CW_F64, 2, fs, n)
    cfg = graph.default_config(fs, fmt=abi.FMT_CW_F64, channels=2)
    nodes = graph.graph_shift_master()
    ctx = L.Context(cfg, nodes, 1)
    out, _ = ctx.process(data[None, :], n)
    ctx.close()
    ref, _ = oracle.Stream(cfg, nodes).process(data, n)
    assert np.array_equal(out[0], ref)
