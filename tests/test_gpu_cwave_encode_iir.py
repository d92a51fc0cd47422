"""GPU: the IIR-Hilbert CWAVE encoder (icw_encode_cwave_iir, packer KIP `icw_iq_pack`;
icw_cwave_encode_files_iir).

The converter is the reference's quadrature half-band IIR (hq_rp_process), which the project reproduces
bit for bit, so -- unlike the FIR encoder's -- these frames have a reference to be pinned to:
  a. ICW_FMT_CW_F64 frames bit-equal to oracle.hilbert_block per channel: six filter types x Kahan / baseline
     x reject on / off x both K1 kernels x stereo / mono, and every PCM format;
  b. encode -> decode on a CWAVE context == the direct call on the PCM: bytes, pre-render doubles, meters;
  c. the lossy formats == cwenc_ref.frames of the F64 frames' I / Q, and the clip count;
  d. split calls, launch blocks, icw_get_state / icw_set_state == one call; what an encode leaves alone;
     encode then process == process with the first frames dropped;
  e. host / pinned / device pointers;  f. argument checks;  g. files.
Shapes: K2's workgroup covers up to 4 tiles of 256 frames, the packer's 1 024 frames: T = 1024 + 256 + 77 is
two of either with a partial last tile; ICW_BLOCK=263 makes six launch blocks whose byte offsets 263 * FB are
not 16-byte aligned for FB = 4, 6, 12 and at whose edges K1 restarts.  Three streams: an ordinary one, one
that falls silent after 300 frames (the filters ring down through the `< 1.0` reject) and a quiet one (peak
below 1.0 on the 16-bit scale: its states are rejected from the first frame on).
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

T = 1024 + 256 + 77
S = 3
FS = 48000
LOSSY = [abi.FMT_CW_I16, abi.FMT_CW_I16_F32, abi.FMT_CW_F32]


def pcm(fmt, ch, n=T):
    """[S, n * frame bytes]: stream 0 ordinary, stream 1 silent from frame 300 on, stream 2 quiet"""
    raw = synth.batch_pcm(S, n, FS, channels=ch, fmt=fmt).copy()
    fsz = abi.FMT_BYTES[fmt] * ch
    zero = 0x80 if fmt == abi.FMT_U8 else 0
    raw[1, 300 * fsz:] = zero
    if fmt == abi.FMT_F32:
        v = raw[2].view("<f4")
        v *= np.float32(1e-5 / 0.6)                          # about -100 dBFS: below 1.0 on the 16-bit scale
        assert 0.0 < np.abs(v).max() * 32768.0 < 1.0
    else:
        raw[2, :] = zero
    return raw


def iir_ctx(fmt, ch, n_streams=S, htype=1, kahan=1, subn=1, cfg=None, nodes=None):
    if cfg is None:
        cfg = graph.default_config(FS, fmt=fmt, channels=ch, hilbert_type=htype)
        cfg.iir_kahan, cfg.iir_subnorm_reject = kahan, subn
    return L.Context(cfg, graph.graph_shift_master() if nodes is None else nodes, n_streams)


def encode_once(raw, fmt, ch, cw_format, n=None, **kw):
    n = raw.shape[1] // (abi.FMT_BYTES[fmt] * ch) if n is None else n
    ctx = iir_ctx(fmt, ch, raw.shape[0], **kw)
    out = ctx.encode_cwave_iir(raw, n, cw_format)
    clipped = [ctx.encode_clipped(s) for s in range(raw.shape[0])]
    ctx.close()
    return out, clipped


def oracle_frames(oracle, raw_row, fmt, ch, htype, kahan, subn):
    """the F64 frame bytes of one fresh stream: hq_rp_process per channel on the unpacked samples"""
    x = cwenc_ref.unpack(raw_row, fmt, ch)
    nc = x.shape[1]
    I, Q = np.zeros_like(x), np.zeros_like(x)
    for c in range(nc):
        I[:, c], Q[:, c] = oracle.hilbert_block(np.ascontiguousarray(x[:, c]), htype, kahan, subn)
    return cwenc_ref.frames(I, Q, abi.FMT_CW_F64)[0]


def assert_bits(got, ref, what=""):
    assert got.shape == ref.shape, what
    bad = np.flatnonzero(got.view(np.uint64) != ref.view(np.uint64))
    assert bad.size == 0, f"{what}: {bad.size} of {ref.size // 8} doubles differ, first at {bad[:5]}"


# ------------------------------------------------------------------ a. F64 bits vs the oracle
@pytest.fixture(params=["plain", "row"])
def k1_mode(request, monkeypatch):
    monkeypatch.setenv("ICW_K1_MODE", request.param)
    return request.param


@pytest.mark.parametrize("subn", [1, 0])
@pytest.mark.parametrize("kahan", [1, 0])
@pytest.mark.parametrize("htype", range(6))
def test_f64_bits_equal_the_oracle(oracle, icw, k1_mode, htype, kahan, subn):
    for ch in (2, 1):
        raw = pcm(abi.FMT_I16, ch)
        ctx = iir_ctx(abi.FMT_I16, ch, htype=htype, kahan=kahan, subn=subn)
        got = ctx.encode_cwave_iir(raw, T, abi.FMT_CW_F64)
        # the row kernel exists for Kahan sums with the reject only; otherwise the lane kernel runs
        want_k1 = abi.K1_ROW if (k1_mode == "row" and kahan and subn) else abi.K1_LANE
        assert ctx.last_k1_kernel() == want_k1
        sn = [ctx.meters(s)["desubnorm"] for s in range(S)]
        ctx.close()
        assert got.shape == (S, T * 16 * ch)
        for s in range(S):
            assert_bits(got[s], oracle_frames(oracle, raw[s], abi.FMT_I16, ch, htype, kahan, subn), f"ch {ch} stream {s}")
        if subn:
            assert sn[1] > 0 and sn[2] > 0                   # the ring-down and the quiet stream were rejected
        else:
            assert sn == [0] * S


@pytest.mark.parametrize("ch", [2, 1])
@pytest.mark.parametrize("fmt", [abi.FMT_U8, abi.FMT_I24, abi.FMT_I32, abi.FMT_F32])
def test_f64_bits_every_pcm_format(oracle, icw, k1_mode, fmt, ch):
    raw = pcm(fmt, ch)
    got, _ = encode_once(raw, fmt, ch, abi.FMT_CW_F64, htype=4)
    for s in range(S):
        assert_bits(got[s], oracle_frames(oracle, raw[s], fmt, ch, 4, 1, 1), f"stream {s}")


def test_three_channel_input_encodes_the_first_two(oracle, icw):
    raw = pcm(abi.FMT_I16, 3)
    got, _ = encode_once(raw, abi.FMT_I16, 3, abi.FMT_CW_F64)
    assert got.shape == (S, T * 32)
    assert_bits(got[0], oracle_frames(oracle, raw[0], abi.FMT_I16, 3, 1, 1, 1))


# ------------------------------------------------------------------ b. round trip
@pytest.mark.parametrize("ch", [2, 1])
@pytest.mark.parametrize("tpdf16", [False, True])
@pytest.mark.parametrize("gname", ["shift_master", "pm_shift_mix"])
def test_round_trip_equals_direct_call(icw, gname, tpdf16, ch):
    """A: encode to F64; B: decode A's frames on a fresh CW_F64 context; C: the PCM on a fresh context"""
    nodes = graph.graph_shift_master() if gname == "shift_master" else graph.graph_pm_shift_mix()

    def config(f, c):
        cfg = graph.default_config(FS, fmt=f, channels=c, need24bits=not tpdf16)
        cfg.render.render_type = abi.RENDER_TPDF if tpdf16 else abi.RENDER_ROUND
        return cfg

    raw = pcm(abi.FMT_I16, ch)
    a = L.Context(config(abi.FMT_I16, ch), nodes, S)
    frames = a.encode_cwave_iir(raw, T, abi.FMT_CW_F64)
    sn_a = [a.meters(s)["desubnorm"] for s in range(S)]
    a.close()
    assert frames.shape == (S, T * 16 * ch)
    b = L.Context(config(abi.FMT_CW_F64, ch), nodes, S)
    out_b, pre_b = b.process(frames, T, want_pre=True)
    met_b = [b.meters(s) for s in range(S)]
    b.close()
    c = L.Context(config(abi.FMT_I16, ch), nodes, S)
    out_c, pre_c = c.process(raw, T, want_pre=True)
    met_c = [c.meters(s) for s in range(S)]
    c.close()
    assert_bits(pre_b, pre_c, "pre-render")
    assert np.array_equal(out_b, out_c)
    assert [(m["clips"], m["peak_db"]) for m in met_b] == [(m["clips"], m["peak_db"]) for m in met_c]
    assert sn_a == [m["desubnorm"] for m in met_c] and sn_a[1] > 0


# ------------------------------------------------------------------ c. lossy formats
def _ramp_i24():
    """stereo i24 ramps in steps of 128 (half an int16 LSB) and 384"""
    rows = []
    for s in range(S):
        k = np.arange(T, dtype=np.int64)
        left = (128 * (k - 600 + 7 * s)).astype("<i4")
        right = (384 * (k % 501) - 60000 + 128 * s).astype("<i4")
        v = np.stack([left, right], axis=1).reshape(-1)
        rows.append(np.ascontiguousarray(v.view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1))
    return np.stack(rows), abi.FMT_I24


def _square_i16():
    """full-scale stereo i16 squares: the Hilbert pair of an edge overshoots full scale"""
    rows = []
    for s in range(S):
        k = np.arange(T)
        left = np.where((k // (37 + 5 * s)) % 2 == 0, 32767, -32768)
        right = np.where((k // (64 + s)) % 2 == 0, -32768, 32767)
        rows.append(np.stack([left, right], axis=1).astype("<i2").reshape(-1).view(np.uint8))
    return np.stack(rows), abi.FMT_I16


@pytest.fixture(scope="module")
def lossy_inputs(icw):
    """signal -> (raw, fmt, the F64 frames): computed once, shared by the formats"""
    res = {}
    for name, (raw, fmt) in (("ramp_i24", _ramp_i24()), ("square_i16", _square_i16())):
        f64, _ = encode_once(raw, fmt, 2, abi.FMT_CW_F64)
        res[name] = (raw, fmt, f64)
    return res


def test_lossy_inputs_hold_ties_and_saturations(lossy_inputs):
    """the ramp's samples are exact .5 on the 16-bit scale every other frame, and the square's Hilbert pair
    overshoots full scale"""
    raw, fmt, _ = lossy_inputs["ramp_i24"]
    x = cwenc_ref.unpack(raw[0], fmt, 2)
    assert np.count_nonzero(np.abs(x - np.trunc(x)) == 0.5) > T // 4
    raw, fmt, f64 = lossy_inputs["square_i16"]
    for s in range(S):
        I, Q = cwenc_ref.iq_of_f64_frames(f64[s], 2)
        clipped = cwenc_ref.quant_i16(I)[1] + cwenc_ref.quant_i16(Q)[1]
        assert 0 < clipped < I.size + Q.size                                   # clipped and unclipped


@pytest.mark.parametrize("cw_format", LOSSY)
@pytest.mark.parametrize("signal", ["ramp_i24", "square_i16"])
def test_lossy_formats_equal_the_restatement(icw, lossy_inputs, signal, cw_format, monkeypatch):
    raw, fmt, f64 = lossy_inputs[signal]
    if signal == "ramp_i24":
        monkeypatch.setenv("ICW_BLOCK", "263")               # block offsets 263 * FB: not 16-byte aligned
    ctx = iir_ctx(fmt, 2)
    got = ctx.encode_cwave_iir(raw, T, cw_format)
    for s in range(S):
        I, Q = cwenc_ref.iq_of_f64_frames(f64[s], 2)
        ref, clipped = cwenc_ref.frames(I, Q, cw_format)
        assert np.array_equal(got[s], ref), f"stream {s}"
        if cw_format == abi.FMT_CW_F32:
            clipped = 0
        elif signal == "square_i16":
            assert clipped > 0
        assert ctx.encode_clipped(s) == clipped
        assert ctx.encode_clipped(s, reset=True) == clipped
        assert ctx.encode_clipped(s) == 0
    ctx.close()


# ------------------------------------------------------------------ d. carried state
def test_split_calls_blocks_and_state_transfer_equal_one_call(icw, monkeypatch):
    raw = pcm(abi.FMT_I16, 2)
    fsz, fb = 4, 32
    one, _ = encode_once(raw, abi.FMT_I16, 2, abi.FMT_CW_F64)

    ctx = iir_ctx(abi.FMT_I16, 2)
    parts, t = [], 0
    for n in [101, 1, 602, T - 704]:                         # 101, 102, 704: the fs/4 phase is not 0 at a split
        parts.append(ctx.encode_cwave_iir(np.ascontiguousarray(raw[:, t * fsz:(t + n) * fsz]), n, abi.FMT_CW_F64))
        t += n
    sn_split = [ctx.meters(s)["desubnorm"] for s in range(S)]
    ctx.close()
    assert np.array_equal(np.concatenate(parts, axis=1), one)

    h = 677
    first = iir_ctx(abi.FMT_I16, 2)
    a = first.encode_cwave_iir(np.ascontiguousarray(raw[:, :h * fsz]), h, abi.FMT_CW_F64)
    blobs = [first.get_state(s) for s in range(S)]
    first.close()
    second = iir_ctx(abi.FMT_I16, 2)
    for s in range(S):
        second.set_state(s, blobs[s])
    b = second.encode_cwave_iir(np.ascontiguousarray(raw[:, h * fsz:]), T - h, abi.FMT_CW_F64)
    sn_moved = [second.meters(s)["desubnorm"] for s in range(S)]
    second.close()
    assert a.shape[1] == h * fb
    assert np.array_equal(np.concatenate([a, b], axis=1), one)

    monkeypatch.setenv("ICW_BLOCK", "263")                   # six launch blocks
    ctx = iir_ctx(abi.FMT_I16, 2)
    blocked = ctx.encode_cwave_iir(raw, T, abi.FMT_CW_F64)
    sn_blocked = [ctx.meters(s)["desubnorm"] for s in range(S)]
    ctx.close()
    assert np.array_equal(blocked, one)
    assert sn_split == sn_moved == sn_blocked and sn_blocked[1] > 0


@pytest.mark.parametrize("cw_format", abi.CW_FORMATS)
@pytest.mark.parametrize("ch", [2, 1])
def test_launch_blocks_every_frame_size(icw, cw_format, ch, monkeypatch):
    """263-frame launch blocks: FB = 4, 6, 12 put every block but the first off the 16-byte grid"""
    raw = pcm(abi.FMT_I16, ch)
    one, clip_one = encode_once(raw, abi.FMT_I16, ch, cw_format)
    monkeypatch.setenv("ICW_BLOCK", "263")
    blocked, clip_blocked = encode_once(raw, abi.FMT_I16, ch, cw_format)
    assert one.shape == (S, T * L.cwave_frame_bytes(cw_format, ch))
    assert np.array_equal(blocked, one) and clip_blocked == clip_one


def test_encode_leaves_the_rest_of_the_context_alone(icw):
    raw = pcm(abi.FMT_I16, 2, 1000)
    ctx = iir_ctx(abi.FMT_I16, 2)
    ctx.process(raw, 1000)
    before = ([ctx.n_frame(s) for s in range(S)], [ctx.meters(s) for s in range(S)])
    ctx.encode_cwave_iir(raw, 1000, abi.FMT_CW_I16)
    after = ([ctx.n_frame(s) for s in range(S)], [ctx.meters(s) for s in range(S)])
    ctx.close()
    assert after[0] == before[0] == [1000] * S
    assert [(m["clips"], m["peak_db"]) for m in after[1]] == [(m["clips"], m["peak_db"]) for m in before[1]]


@pytest.mark.parametrize("ch", [2, 1])
def test_process_after_encode_continues_the_converters(icw, ch):
    """Master-only graph, ROUND flat render: the output depends on the converters' state alone"""
    k = 531                                                  # not a multiple of 4
    nodes = graph.graph_master_only()
    raw = pcm(abi.FMT_I16, ch)
    fsz = 2 * ch
    whole = iir_ctx(abi.FMT_I16, ch, nodes=nodes)
    ref, ref_pre = whole.process(raw, T, want_pre=True)
    sn_ref = [whole.meters(s)["desubnorm"] for s in range(S)]
    whole.close()
    ctx = iir_ctx(abi.FMT_I16, ch, nodes=nodes)
    ctx.encode_cwave_iir(np.ascontiguousarray(raw[:, :k * fsz]), k, abi.FMT_CW_F32)
    out, pre = ctx.process(np.ascontiguousarray(raw[:, k * fsz:]), T - k, want_pre=True)
    sn = [ctx.meters(s)["desubnorm"] for s in range(S)]
    ctx.close()
    assert_bits(pre, np.ascontiguousarray(ref_pre[:, k:]), "pre-render")
    assert np.array_equal(out, ref[:, k * 4:])
    assert sn == sn_ref


# ------------------------------------------------------------------ e. pointer paths
@pytest.mark.parametrize("cw_format", [abi.FMT_CW_I16_F32, abi.FMT_CW_F64])
def test_host_pinned_and_device_pointers_agree(icw, cw_format):
    import torch
    raw = pcm(abi.FMT_I16, 2)
    fb = L.cwave_frame_bytes(cw_format, 2)
    ref, _ = encode_once(raw, abi.FMT_I16, 2, cw_format)

    ctx = iir_ctx(abi.FMT_I16, 2)
    pin_in, pin_out = L.host_array(raw.shape), L.host_array((S, T * fb))
    pin_in[:] = raw
    pin_out[:] = 0
    ctx.encode_cwave_iir(pin_in, T, cw_format, out=pin_out)
    assert np.array_equal(np.asarray(pin_out), ref)
    ctx.close()

    # (base shift, row stride): packed rows; a base 2 bytes off; an odd stride, so rows start at odd addresses
    for shift, stride in ((0, T * fb), (2, T * fb), (0, T * fb + 3)):
        ctx = iir_ctx(abi.FMT_I16, 2)
        d_in = torch.from_numpy(raw.copy()).cuda()
        d_out = torch.zeros(shift + S * stride + 16, dtype=torch.uint8, device="cuda")
        ctx.encode_cwave_iir_device(d_in, raw.shape[1], d_out.data_ptr() + shift, stride, T, cw_format)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        rows = got[shift:shift + S * stride].reshape(S, stride)
        assert np.array_equal(rows[:, :T * fb], ref), f"shift {shift} stride {stride}"
        # nothing outside the frames
        assert not got[:shift].any() and not rows[:, T * fb:].any() and not got[shift + S * stride:].any()
        ctx.close()


# ------------------------------------------------------------------ f. argument checks
def test_argument_checks(icw):
    lib = L.load()
    raw = synth.batch_pcm(1, 256, FS)
    out = np.zeros((1, 256 * 32), np.uint8)

    def call(ctx, cw_format=abi.FMT_CW_F64, flags=0, n=256, fn=lib.icw_encode_cwave_iir):
        return fn(ctx.h, 0, 1, raw.ctypes.data, raw.shape[1], out.ctypes.data, out.shape[1], n, cw_format, flags, None)

    cw = L.Context(graph.default_config(FS, fmt=abi.FMT_CW_I16), graph.graph_shift_master(), 1)
    assert call(cw) == abi.EINVAL                             # already analytic
    cw.close()

    fir = iir_ctx(abi.FMT_I16, 2, 1)
    fir.set_fir_hilbert(30, 8.0)
    assert call(fir) == abi.EINVAL                            # the FIR converter is on: icw_encode_cwave is the call
    fir.close()

    cfg = graph.default_config(FS)
    cfg.fp_check = 1
    fc = L.Context(cfg, graph.graph_shift_master(), 1)
    assert call(fc) == abi.EUNSUPPORTED
    fc.close()

    ctx = iir_ctx(abi.FMT_I16, 2, 1)
    assert call(ctx, fn=lib.icw_encode_cwave) == abi.EINVAL   # the FIR encoder still refuses an IIR context
    for bad_format in (abi.FMT_F32, abi.FMT_CW_F32 + 1, 0):
        assert call(ctx, cw_format=bad_format) == abi.EINVAL
    for bad_flags in (abi.F_DEBUG_PRE, abi.F_TIMING, abi.F_DEBUG_INPUT, 16, abi.F_DEVICE_PTRS | 2):
        assert call(ctx, flags=bad_flags) == abi.EINVAL
    assert call(ctx, n=-1) == abi.EINVAL
    args = (raw.ctypes.data, raw.shape[1], out.ctypes.data, out.shape[1], 256, abi.FMT_CW_F64, 0, None)
    assert lib.icw_encode_cwave_iir(ctx.h, 0, 2, *args) == abi.EINVAL             # range
    assert lib.icw_encode_cwave_iir(ctx.h, -1, 1, *args) == abi.EINVAL
    assert lib.icw_encode_cwave_iir(ctx.h, 0, 0, *args) == abi.EINVAL
    assert lib.icw_encode_cwave_iir(ctx.h, 0, 1, None, raw.shape[1], *args[2:]) == abi.EINVAL      # pointers
    assert lib.icw_encode_cwave_iir(ctx.h, 0, 1, raw.ctypes.data, raw.shape[1], None, *args[3:]) == abi.EINVAL
    assert lib.icw_encode_cwave_iir(ctx.h, 0, 1, raw.ctypes.data, 100, *args[2:]) == abi.EINVAL    # short strides
    assert lib.icw_encode_cwave_iir(ctx.h, 0, 1, raw.ctypes.data, raw.shape[1], out.ctypes.data, 256 * 32 - 1,
                                    *args[4:]) == abi.EINVAL
    assert not out.any()                                      # no kernel ran
    assert ctx.meters(0)["desubnorm"] == 0 and ctx.n_frame(0) == 0
    assert call(ctx) == abi.OK and out.any()                  # and the state was left fresh: equals a first call
    ref, _ = encode_once(raw, abi.FMT_I16, 2, abi.FMT_CW_F64)
    assert np.array_equal(out, ref)
    ctx.close()


# ------------------------------------------------------------------ g. files
SPECS = [("a.wav", abi.FMT_I16, 2, 48000, 5000), ("b.wav", abi.FMT_I16, 2, 48000, 1357),
         ("c.wav", abi.FMT_F32, 1, 44100, 3001), ("d.rwave", abi.FMT_I24, 2, 48000, 2222)]
HTYPE, KAHAN, SUBN = 2, 1, 1


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
    assert (magic, hsize, ver, hfmt, hch, hn, hrate, hM) == (b"cPLXwAVE", 48, 2, fmt_cw - abi.FMT_CW_F64, ch, n, fs, 0)
    assert img[40:48].tobytes() == struct.pack("<d", 0.0) and hbeta == 0.0
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
    ins = [f[0] for f in files[:2]] + [broken] + [f[0] for f in files[2:]]
    outs = [tmp_path / f"out_{i}.cwave" for i in range(len(ins))]
    rc, st, status, clipped = L.cwave_encode_files_iir(ins, outs, HTYPE, KAHAN, SUBN, cw_format, block_frames=1000)
    assert status == [abi.OK, abi.OK, abi.EINVAL, abi.OK, abi.OK] and rc == abi.EINVAL
    assert st.n_files == len(files) and st.n_groups == 3
    assert st.frames_in == st.frames_out == sum(f[4] for f in files)
    assert not outs[2].exists()
    good = [o for i, o in enumerate(outs) if i != 2]
    for (path, fmt, ch, fs, n, d), out in zip(files, good):
        data = _check_file(out, cw_format, ch, fs, n)
        cfg = graph.default_config(fs, fmt=fmt, channels=ch, hilbert_type=HTYPE)
        ref, _ = encode_once(d[None, :], fmt, ch, cw_format, cfg=cfg)
        assert np.array_equal(data, ref[0]), path.name
    assert clipped == [0] * len(ins)


def test_convert_then_play_equals_play(tmp_path, icw):
    """WAV -> CWAVE (F64) -> icw_transcode_files == icw_transcode_files of the WAV, byte for byte"""
    files = _make_wavs(tmp_path)
    ins = [f[0] for f in files]
    mids = [tmp_path / f"mid_{i}.cwave" for i in range(len(ins))]
    rc, _, status, _ = L.cwave_encode_files_iir(ins, mids, HTYPE, KAHAN, SUBN, abi.FMT_CW_F64)
    assert rc == abi.OK and status == [abi.OK] * len(ins)
    cfg = graph.default_config(48000, hilbert_type=HTYPE)
    cfg.iir_kahan, cfg.iir_subnorm_reject = KAHAN, SUBN
    nodes = graph.graph_shift_master()
    direct = [tmp_path / f"direct_{i}.wav" for i in range(len(ins))]
    played = [tmp_path / f"played_{i}.wav" for i in range(len(ins))]
    rc, _, status = L.transcode_files(cfg, nodes, ins, direct)
    assert rc == abi.OK and status == [abi.OK] * len(ins)
    rc, _, status = L.transcode_files(cfg, nodes, mids, played)
    assert rc == abi.OK and status == [abi.OK] * len(ins)
    for d, p, f in zip(direct, played, files):
        a, b = d.read_bytes(), p.read_bytes()
        assert len(a) == 44 + f[4] * 4 and a == b, f[0].name


def test_encode_files_bad_options_write_nothing(tmp_path, icw):
    files = _make_wavs(tmp_path)[:1]
    never = tmp_path / "never.cwave"
    for bad in (dict(hilbert_type=6), dict(iir_kahan=2), dict(iir_subnorm_reject=-1), dict(cw_format=abi.FMT_I16),
                dict(cw_format=abi.FMT_CW_F32 + 1), dict(block_frames=-1)):
        rc, _, _, _ = L.cwave_encode_files_iir([files[0][0]], [never], **bad)
        assert rc == abi.EINVAL and not never.exists(), bad
