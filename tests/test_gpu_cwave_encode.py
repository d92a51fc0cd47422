"""GPU: the CWAVE encoder (icw_encode_cwave, kernel KFE `icw_fir_encode`; icw_cwave_encode_files).

The converter is the FIR Hilbert of icw_set_fir_hilbert; what the encoder writes is defined by this
project (include/icw_cwave.h), not by the reference, which ships no converter: parity is unpinned, like
the converter's own.  The pins here:
  a. ICW_FMT_CW_F64 frames bit-equal to the pure-Python restatement (tests/cwenc_ref.py, itself pinned to
     the oracle by tests/test_cwave_encode_ref.py);
  b. encode -> decode on a CWAVE context == the direct FIR call on the PCM: bytes, pre-render doubles, meters;
  c. the lossy formats == numpy's quantisation of the F64 frames, and the clip count;
  d. split calls and icw_get_state / icw_set_state == one call;  e. host / pinned / device pointers;
  f. argument checks;  g. files: header, CRC, data, the aligned mode, convert-then-play.
The kernel's tile is 2 048 frames: T = 2 * 2048 + 77 is three tiles with a partial last one.
"""
import struct
import zlib

import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth
from in_cwave_amd import lib as L

import cwenc_ref
import wavgen as W

pytestmark = pytest.mark.gpu

BETA = 8.0
T = 2 * 2048 + 77
S = 3
PCM = [abi.FMT_U8, abi.FMT_I16, abi.FMT_I24, abi.FMT_I32, abi.FMT_F32]
LOSSY = [abi.FMT_CW_I16, abi.FMT_CW_I16_F32, abi.FMT_CW_F32]


def fir_ctx(fmt, ch, k_M, n_streams=S, cfg=None, nodes=None, fs=48000):
    cfg = graph.default_config(fs, fmt=fmt, channels=ch) if cfg is None else cfg
    ctx = L.Context(cfg, graph.graph_shift_master() if nodes is None else nodes, n_streams)
    ctx.set_fir_hilbert(k_M, BETA)
    return ctx


def encode_once(raw, fmt, ch, k_M, cw_format, n=None):
    n = raw.shape[1] // (abi.FMT_BYTES[fmt] * ch) if n is None else n
    ctx = fir_ctx(fmt, ch, k_M, raw.shape[0])
    out = ctx.encode_cwave(raw, n, cw_format)
    clipped = [ctx.encode_clipped(s) for s in range(raw.shape[0])]
    ctx.close()
    return out, clipped


# ------------------------------------------------------------------ a. F64 bits vs the restatement
def test_f64_bits_equal_the_restatement(oracle, icw):
    n, k_M = 2048 + 77, 30
    raw = synth.batch_pcm(1, n, 48000)
    got, _ = encode_once(raw, abi.FMT_I16, 2, k_M, abi.FMT_CW_F64)
    ref, _ = cwenc_ref.encode(raw[0], abi.FMT_I16, 2, k_M, oracle.fir_taps(k_M, BETA))
    assert got.shape == (1, n * 32)
    bad = np.flatnonzero(got[0].view(np.uint64) != ref.view(np.uint64))
    assert bad.size == 0, f"{bad.size} of {n * 4} I/Q doubles differ, first at {bad[:5]}"


# ------------------------------------------------------------------ b. round trip
def _round_trip_cases():
    orders = [2, 30, 62, 254]
    cases = []
    for i, (fmt, ch) in enumerate((f, c) for f in PCM for c in (1, 2)):
        for j in range(3):                                   # three of the four orders, rotating
            cases.append((fmt, ch, orders[(i + j) % 4], (i + j) % 2 == 0))
    cases.append((abi.FMT_I16, 3, 62, True))
    return cases


@pytest.mark.parametrize("fmt,ch,k_M,tpdf16", _round_trip_cases())
def test_round_trip_equals_direct_fir(icw, fmt, ch, k_M, tpdf16):
    """path A: encode to F64, decode on a CW_F64 context; path B: the PCM through the FIR context"""
    nodes = graph.graph_shift_master()

    def config(f, c):
        cfg = graph.default_config(48000, fmt=f, channels=c, need24bits=not tpdf16)
        cfg.render.render_type = abi.RENDER_TPDF if tpdf16 else abi.RENDER_ROUND
        return cfg

    raw = synth.batch_pcm(S, T, 48000, channels=ch, fmt=fmt)
    enc = fir_ctx(fmt, ch, k_M, cfg=config(fmt, ch), nodes=nodes)
    frames = enc.encode_cwave(raw, T, abi.FMT_CW_F64)
    enc.close()
    nc = min(ch, 2)
    assert frames.shape == (S, T * 16 * nc)
    dec = L.Context(config(abi.FMT_CW_F64, nc), nodes, S)
    out_a, pre_a = dec.process(frames, T, want_pre=True)
    met_a = [dec.meters(s) for s in range(S)]
    dec.close()
    direct = fir_ctx(fmt, ch, k_M, cfg=config(fmt, ch), nodes=nodes)
    out_b, pre_b = direct.process(raw, T, want_pre=True)
    met_b = [direct.meters(s) for s in range(S)]
    direct.close()
    bad = np.flatnonzero(pre_a.view(np.uint64) != pre_b.view(np.uint64))
    assert bad.size == 0, f"{bad.size} pre-render doubles differ, first at {bad[:5]}"
    assert np.array_equal(out_a, out_b)
    assert met_a == met_b


# ------------------------------------------------------------------ c. lossy formats
def _ramp_i24():
    """stereo i24 ramps in steps of 128 (half an int16 LSB) and 384: every other Re is an exact .5"""
    rows = []
    for s in range(S):
        k = np.arange(T, dtype=np.int64)
        left = (128 * (k - 2000 + 7 * s)).astype("<i4")
        right = (384 * (k % 1501) - 200000 + 128 * s).astype("<i4")
        v = np.stack([left, right], axis=1).reshape(-1)
        rows.append(np.ascontiguousarray(v.view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1))
    return np.stack(rows), abi.FMT_I24


def _square_i16():
    """full-scale stereo i16 squares: the Hilbert transform of an edge overshoots full scale"""
    rows = []
    for s in range(S):
        k = np.arange(T)
        left = np.where((k // (37 + 5 * s)) % 2 == 0, 32767, -32768)
        right = np.where((k // (64 + s)) % 2 == 0, -32768, 32767)
        rows.append(np.stack([left, right], axis=1).astype("<i2").reshape(-1).view(np.uint8))
    return np.stack(rows), abi.FMT_I16


@pytest.mark.parametrize("cw_format", LOSSY)
@pytest.mark.parametrize("signal", ["ramp_i24", "square_i16"])
def test_lossy_formats_equal_numpy_quantisation(icw, signal, cw_format):
    raw, fmt = _ramp_i24() if signal == "ramp_i24" else _square_i16()
    k_M = 62
    f64, _ = encode_once(raw, fmt, 2, k_M, abi.FMT_CW_F64)
    ctx = fir_ctx(fmt, 2, k_M)
    got = ctx.encode_cwave(raw, T, cw_format)
    for s in range(S):
        I, Q = cwenc_ref.iq_of_f64_frames(f64[s], 2)
        ref, clipped = cwenc_ref.frames(I, Q, cw_format)
        assert np.array_equal(got[s], ref), f"stream {s}"
        if signal == "ramp_i24":
            assert np.count_nonzero(np.abs(I - np.trunc(I)) == 0.5) > T // 4      # the ties are there
        elif cw_format != abi.FMT_CW_F32:
            _, cq = cwenc_ref.quant_i16(Q)
            assert 0 < cq < Q.size                                                 # clipped and unclipped
        if cw_format == abi.FMT_CW_F32:
            clipped = 0
        assert ctx.encode_clipped(s) == clipped
        assert ctx.encode_clipped(s, reset=True) == clipped
        assert ctx.encode_clipped(s) == 0
    ctx.close()


def test_clip_count_accumulates_across_calls(icw):
    raw, fmt = _square_i16()
    ctx = fir_ctx(fmt, 2, 30)
    a = ctx.encode_cwave(raw, T, abi.FMT_CW_I16)
    one = [ctx.encode_clipped(s) for s in range(S)]
    ctx.encode_cwave(raw, T, abi.FMT_CW_I16)
    two = [ctx.encode_clipped(s) for s in range(S)]
    ctx.close()
    assert a.shape == (S, T * 8) and min(one) > 0 and all(t > o for t, o in zip(two, one))


# ------------------------------------------------------------------ d. carried state
def test_split_calls_and_state_transfer_equal_one_call(icw):
    k_M = 254
    raw = synth.batch_pcm(S, T, 48000)
    fsz, fb = 4, 32
    one, _ = encode_once(raw, abi.FMT_I16, 2, k_M, abi.FMT_CW_F64)

    ctx = fir_ctx(abi.FMT_I16, 2, k_M)
    parts, t = [], 0
    for n in [100, 1, 2047, T - 2148]:                       # the 254-frame history is longer than a call
        parts.append(ctx.encode_cwave(np.ascontiguousarray(raw[:, t * fsz:(t + n) * fsz]), n, abi.FMT_CW_F64))
        t += n
    assert [ctx.n_frame(s) for s in range(S)] == [0] * S     # the modulator's frame counter is not the encoder's
    ctx.close()
    assert np.array_equal(np.concatenate(parts, axis=1), one)

    h = T // 2
    first = fir_ctx(abi.FMT_I16, 2, k_M)
    a = first.encode_cwave(np.ascontiguousarray(raw[:, :h * fsz]), h, abi.FMT_CW_F64)
    blobs = [first.get_state(s) for s in range(S)]
    first.close()
    second = fir_ctx(abi.FMT_I16, 2, k_M)
    for s in range(S):
        second.set_state(s, blobs[s])
    b = second.encode_cwave(np.ascontiguousarray(raw[:, h * fsz:]), T - h, abi.FMT_CW_F64)
    second.close()
    assert a.shape[1] == h * fb
    assert np.array_equal(np.concatenate([a, b], axis=1), one)


def test_encode_leaves_the_decode_state_alone(icw):
    """a process call after an encode renders what it renders after a process call of the same frames
    whose output is thrown away, except for the state the encode must not touch: compare n_frame"""
    raw = synth.batch_pcm(S, 1000, 48000)
    ctx = fir_ctx(abi.FMT_I16, 2, 30)
    ctx.process(raw, 1000)
    before = [ctx.n_frame(s) for s in range(S)]
    ctx.encode_cwave(raw, 1000, abi.FMT_CW_I16)
    assert [ctx.n_frame(s) for s in range(S)] == before == [1000] * S
    ctx.close()


# ------------------------------------------------------------------ e. pointer paths
@pytest.mark.parametrize("cw_format", [abi.FMT_CW_I16_F32, abi.FMT_CW_F64])
def test_host_pinned_and_device_pointers_agree(icw, cw_format):
    import torch
    k_M = 62
    raw = synth.batch_pcm(S, T, 48000)
    fb = L.cwave_frame_bytes(cw_format, 2)
    ref, _ = encode_once(raw, abi.FMT_I16, 2, k_M, cw_format)

    ctx = fir_ctx(abi.FMT_I16, 2, k_M)
    pin_in, pin_out = L.host_array(raw.shape), L.host_array((S, T * fb))
    pin_in[:] = raw
    pin_out[:] = 0
    ctx.encode_cwave(pin_in, T, cw_format, out=pin_out)
    assert np.array_equal(np.asarray(pin_out), ref)
    ctx.close()

    # rows of T * fb bytes: 16-byte aligned for stream 0 only (the 12-byte frame), then a base 2 bytes off
    for shift in (0, 2):
        ctx = fir_ctx(abi.FMT_I16, 2, k_M)
        d_in = torch.from_numpy(raw.copy()).cuda()
        d_out = torch.zeros(S * T * fb + 16, dtype=torch.uint8, device="cuda")
        ctx.encode_cwave_device(d_in, raw.shape[1], d_out.data_ptr() + shift, T * fb, T, cw_format)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert np.array_equal(got[shift:shift + S * T * fb].reshape(S, T * fb), ref), f"shift {shift}"
        assert not got[:shift].any() and not got[shift + S * T * fb:].any()      # nothing outside the frames
        ctx.close()


# ------------------------------------------------------------------ f. argument checks
def test_argument_checks(icw):
    lib = L.load()
    raw = synth.batch_pcm(1, 256, 48000)
    out = np.zeros((1, 256 * 32), np.uint8)

    def call(ctx, cw_format=abi.FMT_CW_F64, flags=0, n=256):
        return lib.icw_encode_cwave(ctx.h, 0, 1, raw.ctypes.data, raw.shape[1], out.ctypes.data, out.shape[1], n,
                                    cw_format, flags, None)

    no_fir = L.Context(graph.default_config(48000), graph.graph_shift_master(), 1)
    assert call(no_fir) == abi.EINVAL
    for bad_order in (31, 4098, -2):                          # odd, oversized, negative: refused, so still no FIR
        assert lib.icw_set_fir_hilbert(no_fir.h, bad_order, BETA) == abi.EINVAL
        assert call(no_fir) == abi.EINVAL
    no_fir.close()

    cw = L.Context(graph.default_config(48000, fmt=abi.FMT_CW_I16), graph.graph_shift_master(), 1)
    cw.set_fir_hilbert(30, BETA)
    assert call(cw) == abi.EINVAL                             # already analytic
    cw.close()

    ctx = fir_ctx(abi.FMT_I16, 2, 30, 1)
    for bad_format in (abi.FMT_F32, abi.FMT_CW_F32 + 1, 0):
        assert call(ctx, cw_format=bad_format) == abi.EINVAL
    for bad_flags in (abi.F_DEBUG_PRE, abi.F_TIMING, abi.F_DEBUG_INPUT, 16):
        assert call(ctx, flags=bad_flags) == abi.EINVAL
    assert call(ctx, n=-1) == abi.EINVAL
    assert lib.icw_encode_cwave(ctx.h, 0, 2, raw.ctypes.data, raw.shape[1], out.ctypes.data, out.shape[1], 256,
                                abi.FMT_CW_F64, 0, None) == abi.EINVAL
    assert lib.icw_encode_cwave(ctx.h, 0, 1, raw.ctypes.data, 100, out.ctypes.data, out.shape[1], 256,
                                abi.FMT_CW_F64, 0, None) == abi.EINVAL
    assert not out.any()                                      # no kernel ran
    assert call(ctx) == abi.OK and out.any()                  # and the state was left fresh: equals a first call
    ref, _ = encode_once(raw, abi.FMT_I16, 2, 30, abi.FMT_CW_F64)
    assert np.array_equal(out, ref)
    ctx.close()
    assert [L.cwave_frame_bytes(f, 2) for f in abi.CW_FORMATS] == [32, 8, 12, 16]
    assert [L.cwave_frame_bytes(f, 1) for f in abi.CW_FORMATS] == [16, 4, 6, 8]
    assert L.cwave_frame_bytes(abi.FMT_CW_F64, 5) == 32
    assert L.cwave_frame_bytes(abi.FMT_I16, 2) == 0 and L.cwave_frame_bytes(abi.FMT_CW_F64, 0) == 0


# ------------------------------------------------------------------ g. files
SPECS = [("a.wav", abi.FMT_I16, 2, 48000, 70000), ("b.wav", abi.FMT_I16, 2, 48000, 33001),
         ("c.wav", abi.FMT_I16, 2, 48000, 1000), ("d.wav", abi.FMT_F32, 1, 44100, 40000),
         ("e.rwave", abi.FMT_F32, 1, 44100, 1333), ("f.wav", abi.FMT_U8, 2, 22050, 40000)]


def _make_wavs(tmp_path):
    files = []
    for i, (name, fmt, ch, fs, n) in enumerate(SPECS):
        d = synth.stream_pcm(i, n, fs, channels=ch, fmt=fmt)
        W.write(tmp_path / name, d, fmt, ch, fs, kind="ext" if i == 1 else ("float" if fmt == abi.FMT_F32 else "pcm"))
        files.append((tmp_path / name, fmt, ch, fs, n, d))
    return files


def _check_file(path, fmt_cw, ch, fs, n, k_M):
    img = np.frombuffer(path.read_bytes(), np.uint8)
    fb = abi.FMT_BYTES[fmt_cw] * ch
    info = L.wav_parse_file(path)
    assert (info.fmt, info.channels, info.sample_rate, info.frame_bytes, info.n_samples, info.data_offset,
            info.htype) == (fmt_cw, ch, fs, fb, n, 48, abi.HTYPE_CWAVE)
    magic, hsize, ver, hfmt, hch, hn, hrate, hM, hcrc, hbeta = struct.unpack("<8s6IiId", img[:48].tobytes())
    assert (magic, hsize, ver, hfmt, hch, hn, hrate, hM, hbeta) == (b"cPLXwAVE", 48, 2, fmt_cw - abi.FMT_CW_F64, ch, n,
                                                                   fs, k_M, BETA)
    data = img[48:]
    assert data.size == n * fb
    assert zlib.crc32(data.tobytes()) == hcrc
    assert L.cwave_check(img.copy()) == (hcrc, 1)
    return data.copy()


@pytest.mark.parametrize("cw_format", [abi.FMT_CW_F64, abi.FMT_CW_I16_F32])
def test_encode_files(tmp_path, icw, cw_format):
    from in_cwave_amd import cwave
    k_M = 62
    files = _make_wavs(tmp_path)
    cw_in = tmp_path / "g.cwave"
    cw_in.write_bytes(cwave.make_image(synth.stream_cwave(9, 5000, 48000, fmt=abi.FMT_CW_I16), abi.FMT_CW_I16, 2,
                                       48000).tobytes())
    broken = tmp_path / "broken.wav"
    broken.write_bytes(b"RIFF\0\0\0\0WAVEjunk")
    ins = [f[0] for f in files] + [cw_in, broken]
    outs = [tmp_path / f"out_{i}.cwave" for i in range(len(ins))]
    rc, st, status, clipped = L.cwave_encode_files(ins, outs, k_M, BETA, cw_format, block_frames=32768)
    assert status == [abi.OK] * len(files) + [abi.EINVAL, abi.EINVAL] and rc == abi.EINVAL
    assert st.n_files == len(files) and st.n_groups == 3
    assert st.frames_in == st.frames_out == sum(f[4] for f in files)
    for (path, fmt, ch, fs, n, d), out in zip(files, outs):
        data = _check_file(out, cw_format, ch, fs, n, k_M)
        ref, _ = encode_once(d[None, :], fmt, ch, k_M, cw_format)
        assert np.array_equal(data, ref[0]), path.name
    assert clipped == [0] * len(ins)
    assert not outs[-1].exists() and not outs[-2].exists()


def test_encode_files_aligned_and_refusals(tmp_path, icw):
    k_M, c = 254, 127
    files = _make_wavs(tmp_path)[2:]                          # 1000 .. 40000 frames, three groups
    one = tmp_path / "one.wav"                                # a single frame: the reader would refuse the result
    W.write(one, np.zeros(4, np.uint8), abi.FMT_I16, 2, 48000)
    ins = [f[0] for f in files] + [one]
    outs = [tmp_path / f"al_{i}.cwave" for i in range(len(ins))]
    rc, st, status, _ = L.cwave_encode_files(ins, outs, k_M, BETA, abi.FMT_CW_F32, align=1, block_frames=16384)
    assert status == [abi.OK] * len(files) + [abi.EINVAL] and rc == abi.EINVAL
    for (path, fmt, ch, fs, n, d), out in zip(files, outs):
        data = _check_file(out, abi.FMT_CW_F32, ch, fs, n, k_M)
        pad = np.full(c * abi.FMT_BYTES[fmt] * ch, 0x80 if fmt == abi.FMT_U8 else 0, np.uint8)
        ref, _ = encode_once(np.concatenate([d, pad])[None, :], fmt, ch, k_M, abi.FMT_CW_F32)
        assert np.array_equal(data, ref[0][c * 8 * ch:]), path.name
    for bad in (dict(k_M=31), dict(k_M=4098), dict(k_M=0), dict(k_M=30, cw_format=abi.FMT_I16), dict(k_M=30, align=2)):
        kw = dict(k_M=30, k_beta=BETA, cw_format=abi.FMT_CW_F64, align=0)
        kw.update(bad)
        rc, _, status, _ = L.cwave_encode_files(ins[:1], [tmp_path / "never.cwave"], **kw)
        assert rc == abi.EINVAL and not (tmp_path / "never.cwave").exists()


def test_convert_then_play(tmp_path, oracle, icw):
    """WAV -> CWAVE file (the encoder) -> icw_transcode_files (Hilbert bypassed) == the oracle's decode of
    the file's data"""
    n, fs = 30000, 48000
    src = tmp_path / "in.wav"
    W.write(src, synth.stream_pcm(3, n, fs), abi.FMT_I16, 2, fs)
    mid, dst = tmp_path / "mid.cwave", tmp_path / "out.wav"
    rc, _, status, _ = L.cwave_encode_files([src], [mid], 254, BETA, abi.FMT_CW_I16_F32, align=1)
    assert rc == abi.OK and status == [abi.OK]
    data = _check_file(mid, abi.FMT_CW_I16_F32, 2, fs, n, 254)
    cfg = graph.default_config(fs)
    nodes = graph.graph_shift_master()
    rc, _, status = L.transcode_files(cfg, nodes, [mid], [dst])
    assert rc == abi.OK and status == [abi.OK]
    ref_stream = oracle.Stream(graph.default_config(fs, fmt=abi.FMT_CW_I16_F32, channels=2), nodes)
    ref_stream.open(n)
    ref, _ = ref_stream.process(data, n)
    got = np.frombuffer(dst.read_bytes(), np.uint8)
    assert np.array_equal(got[44:], ref)
