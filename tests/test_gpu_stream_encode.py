"""GPU: the CWAVE encoders over streams with different inputs (icw_enable_stream_encode; the per-stream
kernels icw_iq_pack_mixed and icw_fir_encode_mixed).

The reference of every comparison is the path that existed before: for each stream a fresh ONE-input
context of one stream (opt-in off) driven through the same sequence of calls.  The mixed context must write,
per stream, exactly those bytes and count exactly those clipped samples -- nothing here has a tolerance.
The one-input path is itself pinned to the oracle by tests/test_gpu_cwave_encode_iir.py and
tests/test_gpu_cwave_encode.py; for ICW_FMT_CW_F64 the mixed context's frames are compared with the oracle
directly as well (hilbert_block per channel; the FIR restatement cwenc_ref.encode with the oracle's taps at
k_M 30 -- its exact-fraction FMA is too slow for 254 taps over these lengths, where the one-input contexts
stand in).

Shapes: KFE's tile is 2 048 frames and KIP's 1 024.  Every call's output rows start at frame 0, so calls of 1,
37, 1 023, 2 500 and 1 025 frames give partial tiles, more than one tile (tile starts at frames 0, 1 024 and
2 048 of a row) and, through s * out_stride, row starts on and off the 16-byte grid; the state carries from
call to call.  The block offset -- the per-stream kernels place a tile at frame t0 + tt of the stream's row at
the stream's own FB, and KFE reads its input from t0 at the stream's own frame size -- needs a call of several
launch blocks: test_launch_blocks runs the same calls with ICW_BLOCK=263, which starts tiles at frames 263 k
of a row, odd k included: the mono 6-byte frame then starts 1 578 k bytes into its row, off the dword grid
for odd k (the funnel path with two bytes of shift), and FB = 4, 8, 12 off the 16-byte grid.
Six streams cover the five PCM formats, mono and stereo, three rates.  The input is synth.stream_pcm's
signal 8 dB up and saturated like a hot master, so the int16 formats clip.
"""
import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth
from in_cwave_amd import lib as L

import cwenc_ref

pytestmark = pytest.mark.gpu

INPUTS6 = [(44100, abi.FMT_I16, 2), (48000, abi.FMT_I24, 1), (96000, abi.FMT_F32, 2), (48000, abi.FMT_U8, 1),
           (48000, abi.FMT_I32, 2), (44100, abi.FMT_I16, 1)]
CALLS = [1, 37, 1023, 2500, 1025]
BETA = 8.0


def loud_pcm(s, n, rate, ch, fmt):
    """synth.stream_pcm's signal of stream s, 8 dB up (peaks near 1.25 of full scale), in fmt: the integer
    formats saturate as stream_pcm saturates them, float keeps the overshoot"""
    sig = synth.stream_pcm(s, n, rate, channels=ch, fmt=abi.FMT_F32).view("<f4").astype(np.float64) * 2.5
    if fmt == abi.FMT_F32:
        return sig.astype("<f4").view(np.uint8)
    if fmt == abi.FMT_I16:
        return np.clip(np.round(sig * 32767.0), -32768, 32767).astype("<i2").view(np.uint8)
    if fmt == abi.FMT_I24:
        q = np.clip(np.round(sig * 8388607.0), -8388608, 8388607).astype("<i4")
        return np.ascontiguousarray(q.view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)
    if fmt == abi.FMT_I32:
        return np.clip(np.round(sig * 2147483647.0), -2147483648, 2147483647).astype("<i4").view(np.uint8)
    return np.clip(np.round(sig * 127.0) + 128, 0, 255).astype(np.uint8)


def fsz_of(inp):
    return abi.FMT_BYTES[inp[1]] * inp[2]


def make_ctx(inputs, enc, opt_in, htype=1, kahan=1, subn=1, k_M=30, nodes=None, via_stream_input=True):
    """a context whose stream s has inputs[s]; enc "iir" or "fir" (the converter on, k_M)"""
    rate, fmt, ch = inputs[0]
    cfg = graph.default_config(rate, fmt=fmt, channels=ch, hilbert_type=htype)
    cfg.iir_kahan, cfg.iir_subnorm_reject = kahan, subn
    ctx = L.Context(cfg, graph.graph_shift_master() if nodes is None else nodes, len(inputs))
    if opt_in:
        ctx.enable_stream_encode()
    if enc == "fir":
        if opt_in:
            ctx.enable_stream_fir()
        ctx.set_fir_hilbert(k_M, BETA)
    if via_stream_input:
        for s, (r, f, c) in enumerate(inputs):
            ctx.set_stream_input(r, f, c, s, 1)
    return ctx


def rows_of(inputs, raws, t, n, first=0, count=None):
    count = len(inputs) - first if count is None else count
    wide = max(fsz_of(inputs[first + i]) for i in range(count))
    rows = np.zeros((count, n * wide), np.uint8)
    for i in range(count):
        f = fsz_of(inputs[first + i])
        rows[i, :n * f] = raws[first + i][t * f:(t + n) * f]
    return rows


def encode_call(ctx, enc, rows, n, cw_format, first=0, count=None, device=False):
    """one encode call; returns every stream's own bytes [n * FB_s], and checks that a narrower stream's row
    is written no further than its frames"""
    count = ctx.n_streams - first if count is None else count
    fbs = ctx.encode_frame_bytes(cw_format, first, count)
    wide = max(fbs)
    if device:
        import torch
        d_in = torch.from_numpy(rows).cuda()
        d_out = torch.zeros((count, n * wide), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        fn = ctx.encode_cwave_iir_device if enc == "iir" else ctx.encode_cwave_device
        fn(d_in, rows.shape[1], d_out, n * wide, n, cw_format, first=first, count=count)
        ctx.synchronize()
        out = d_out.cpu().numpy()
    else:
        fn = ctx.encode_cwave_iir if enc == "iir" else ctx.encode_cwave
        out = fn(rows, n, cw_format, first=first, count=count)
    assert out.shape == (count, n * wide)
    for i, fb in enumerate(fbs):
        assert not out[i, n * fb:].any(), f"stream {first + i}: bytes past its {n} frames of {fb}"
    return [out[i, :n * fb].copy() for i, fb in enumerate(fbs)]


_SINGLE = {}


def single(enc, inp, s, n_total, calls, cw_format, **kw):
    """(bytes of every call, clipped) of stream s alone on a fresh one-input context, opt-in off -- the path
    as it was; computed once per configuration and shared"""
    key = (enc, inp, s, n_total, tuple(calls), cw_format, tuple(sorted(kw.items())))
    if key not in _SINGLE:
        raw = loud_pcm(s, n_total, inp[0], inp[2], inp[1])
        ctx = make_ctx([inp], enc, False, via_stream_input=False, **kw)
        assert ctx.stream_input_count() == 1
        parts, t = [], 0
        for n in calls:
            parts.append(encode_call(ctx, enc, rows_of([inp], [raw], t, n), n, cw_format)[0])
            t += n
        _SINGLE[key] = (parts, ctx.encode_clipped(0))
        ctx.close()
    return _SINGLE[key]


def run_mixed(enc, inputs, calls, cw_format, device=False, **kw):
    """the mixed context over the same calls: per stream (bytes of every call, clipped)"""
    n_total = sum(calls)
    raws = [loud_pcm(s, n_total, r, c, f) for s, (r, f, c) in enumerate(inputs)]
    ctx = make_ctx(inputs, enc, True, **kw)
    assert ctx.stream_input_count() == len(set(inputs))
    parts, t = [[] for _ in inputs], 0
    for n in calls:
        got = encode_call(ctx, enc, rows_of(inputs, raws, t, n), n, cw_format, device=device)
        for s in range(len(inputs)):
            parts[s].append(got[s])
        t += n
    clipped = [ctx.encode_clipped(s) for s in range(len(inputs))]
    k1 = ctx.last_k1_kernel() if enc == "iir" else None
    ctx.close()
    return raws, parts, clipped, k1


def assert_equal_singles(enc, inputs, calls, cw_format, parts, clipped, **kw):
    n_total = sum(calls)
    for s, inp in enumerate(inputs):
        ref_parts, ref_clip = single(enc, inp, s, n_total, calls, cw_format, **kw)
        for k, n in enumerate(calls):
            assert np.array_equal(parts[s][k], ref_parts[k]), f"stream {s} {inp}: call {k} of {n} frames differs"
        assert clipped[s] == ref_clip, f"stream {s} {inp}: clipped"


# ------------------------------------------------------------------ 1. the IIR encoder, mixed inputs
IIR_CASES = {"t1_kahan_reject": dict(htype=1, kahan=1, subn=1), "t4_baseline": dict(htype=4, kahan=0, subn=0)}


@pytest.mark.parametrize("case", list(IIR_CASES))
@pytest.mark.parametrize("cw_format", abi.CW_FORMATS)
def test_iir_mixed_inputs(icw, oracle, cw_format, case):
    kw = IIR_CASES[case]
    raws, parts, clipped, _ = run_mixed("iir", INPUTS6, CALLS, cw_format, **kw)
    assert_equal_singles("iir", INPUTS6, CALLS, cw_format, parts, clipped, **kw)
    if cw_format in (abi.FMT_CW_I16, abi.FMT_CW_I16_F32):
        assert all(c > 0 for c in clipped), clipped          # the input is loud enough
    else:
        assert cw_format == abi.FMT_CW_F64 or clipped == [0] * len(INPUTS6)
    if cw_format == abi.FMT_CW_F64:
        # as tests/test_gpu_cwave_encode_iir.py compares them: hq_rp_process per channel on the unpacked samples
        for s, (rate, fmt, ch) in enumerate(INPUTS6):
            x = cwenc_ref.unpack(raws[s], fmt, ch)
            I, Q = np.zeros_like(x), np.zeros_like(x)
            for c in range(x.shape[1]):
                I[:, c], Q[:, c] = oracle.hilbert_block(np.ascontiguousarray(x[:, c]), kw["htype"], kw["kahan"], kw["subn"])
            ref = cwenc_ref.frames(I, Q, abi.FMT_CW_F64)[0]
            got = np.concatenate(parts[s])
            bad = np.flatnonzero(got.view(np.uint64) != ref.view(np.uint64))
            assert bad.size == 0, f"stream {s}: {bad.size} doubles differ from the oracle, first at {bad[:5]}"


@pytest.mark.parametrize("mode", ["plain", "row"])
def test_iir_mixed_inputs_both_recurrence_kernels(icw, mode, monkeypatch):
    """existing tests force ICW_K1_MODE at context creation: either K1 feeds K2's per-stream instances and the
    per-stream KIP"""
    monkeypatch.setenv("ICW_K1_MODE", mode)
    _, parts, clipped, k1 = run_mixed("iir", INPUTS6, CALLS, abi.FMT_CW_I16_F32)
    assert k1 == (abi.K1_ROW if mode == "row" else abi.K1_LANE)
    assert_equal_singles("iir", INPUTS6, CALLS, abi.FMT_CW_I16_F32, parts, clipped)


# ------------------------------------------------------------------ 2. the FIR encoder
@pytest.mark.parametrize("k_M", [30, 254])
@pytest.mark.parametrize("cw_format", abi.CW_FORMATS)
def test_fir_mixed_inputs(icw, oracle, cw_format, k_M):
    raws, parts, clipped, _ = run_mixed("fir", INPUTS6, CALLS, cw_format, k_M=k_M)
    assert_equal_singles("fir", INPUTS6, CALLS, cw_format, parts, clipped, k_M=k_M)
    if cw_format in (abi.FMT_CW_I16, abi.FMT_CW_I16_F32):
        # I is the saturated input itself here: only the float stream's I and the Hilbert pairs of hard
        # saturations overshoot, so some streams clip and some do not
        assert sum(c > 0 for c in clipped) >= 2, clipped
    if cw_format == abi.FMT_CW_F64 and k_M == 30:
        g = oracle.fir_taps(k_M, BETA)
        for s, (rate, fmt, ch) in enumerate(INPUTS6):
            ref, _ = cwenc_ref.encode(raws[s], fmt, ch, k_M, g)
            got = np.concatenate(parts[s])
            bad = np.flatnonzero(got.view(np.uint64) != ref.view(np.uint64))
            assert bad.size == 0, f"stream {s}: {bad.size} doubles differ from the restatement, first at {bad[:5]}"


# ------------------------------------------------------------------ 3. mono dedup
@pytest.mark.parametrize("cw_format", [abi.FMT_CW_F64, abi.FMT_CW_I16_F32])
def test_all_mono_call_then_a_stereo_stream(icw, cw_format):
    """three mono streams (left = right known: K1 runs the left chains only), then a call that adds a stereo
    stream, which ends the shortcut for the call but leaves the mono streams' identity"""
    inputs = [(44100, abi.FMT_I16, 1), (48000, abi.FMT_F32, 1), (96000, abi.FMT_I24, 1), (48000, abi.FMT_I16, 2)]
    n1, n2 = 1300, 700
    raws = [loud_pcm(s, n1 + n2, r, c, f) for s, (r, f, c) in enumerate(inputs)]
    ctx = make_ctx(inputs, "iir", True)
    a = encode_call(ctx, "iir", rows_of(inputs, raws, 0, n1, 0, 3), n1, cw_format, 0, 3)
    # the stereo stream's own track starts with this call: its frames 0 .. n2
    raws4 = raws[:3] + [np.concatenate([np.zeros(n1 * 4, np.uint8), raws[3][:n2 * 4]])]
    b = encode_call(ctx, "iir", rows_of(inputs, raws4, n1, n2), n2, cw_format)
    c = encode_call(ctx, "iir", rows_of(inputs, raws, n1 + n2 - 300, 300, 0, 3), 300, cw_format, 0, 3)
    clipped = [ctx.encode_clipped(s) for s in range(4)]
    ctx.close()
    for s in range(3):
        # the third call repeats the last 300 frames of the input: any input will do, the state carries on
        raw = np.concatenate([raws[s], raws[s][(n1 + n2 - 300) * fsz_of(inputs[s]):]])
        one = make_ctx([inputs[s]], "iir", False, via_stream_input=False)
        t = 0
        for k, (n, got) in enumerate(((n1, a[s]), (n2, b[s]), (300, c[s]))):
            ref = encode_call(one, "iir", rows_of([inputs[s]], [raw], t, n), n, cw_format)[0]
            assert np.array_equal(got, ref), f"mono stream {s}, call {k}"
            t += n
        assert one.encode_clipped(0) == clipped[s]
        one.close()
    one = make_ctx([inputs[3]], "iir", False, via_stream_input=False)
    ref = encode_call(one, "iir", rows_of([inputs[3]], [raws[3]], 0, n2), n2, cw_format)[0]
    assert np.array_equal(b[3], ref) and one.encode_clipped(0) == clipped[3]
    one.close()


# ------------------------------------------------------------------ 4. one input through the opt-in
@pytest.mark.parametrize("enc", ["iir", "fir"])
def test_one_input_through_the_opt_in(icw, enc):
    inputs = [(48000, abi.FMT_I24, 2)] * 3
    n = 2500
    raws = [loud_pcm(s, n, *[inputs[s][0], inputs[s][2], inputs[s][1]]) for s in range(3)]
    res = []
    for opt_in in (False, True):
        ctx = make_ctx(inputs, enc, opt_in, via_stream_input=opt_in)
        assert ctx.stream_input_count() == 1
        res.append((encode_call(ctx, enc, rows_of(inputs, raws, 0, n), n, abi.FMT_CW_I16_F32),
                    [ctx.encode_clipped(s) for s in range(3)]))
        ctx.close()
    for s in range(3):
        assert np.array_equal(res[0][0][s], res[1][0][s])
    assert res[0][1] == res[1][1]


# ------------------------------------------------------------------ 5. encode and process calls interleaved
def test_encode_process_encode(icw, oracle):
    """Master-only list, ROUND render: what a process call renders depends on the converters' state alone, so
    oracle.Stream fed the encoded frames first renders the same bytes"""
    inputs = INPUTS6[:4]
    n = 700
    nodes = graph.graph_master_only()
    raws = [loud_pcm(s, 3 * n, r, c, f) for s, (r, f, c) in enumerate(inputs)]

    def drive(ctx, ins, rws):
        a = encode_call(ctx, "iir", rows_of(ins, rws, 0, n), n, abi.FMT_CW_F64)
        out, _ = ctx.process(rows_of(ins, rws, n, n), n)
        b = encode_call(ctx, "iir", rows_of(ins, rws, 2 * n, n), n, abi.FMT_CW_F64)
        return a, out, b

    ctx = make_ctx(inputs, "iir", True, nodes=nodes)
    a, out, b = drive(ctx, inputs, raws)
    ctx.close()
    for s, (rate, fmt, ch) in enumerate(inputs):
        one = make_ctx([inputs[s]], "iir", False, nodes=nodes, via_stream_input=False)
        ra, rout, rb = drive(one, [inputs[s]], [raws[s]])
        one.close()
        assert np.array_equal(a[s], ra[0]) and np.array_equal(b[s], rb[0]), f"stream {s}: encoded bytes"
        assert np.array_equal(out[s], rout[0]), f"stream {s}: rendered bytes"
        st = oracle.Stream(graph.default_config(rate, fmt=fmt, channels=ch, hilbert_type=1), nodes)
        f = fsz_of(inputs[s])
        st.process(raws[s][:n * f], n)
        ro, _ = st.process(raws[s][n * f:2 * n * f], n)
        assert np.array_equal(out[s], ro), f"stream {s}: rendered bytes against the oracle"


# ------------------------------------------------------------------ 6. device pointers
@pytest.mark.parametrize("enc", ["iir", "fir"])
def test_device_pointers(icw, enc):
    kw = dict(k_M=254) if enc == "fir" else {}
    _, parts, clipped, _ = run_mixed(enc, INPUTS6, CALLS, abi.FMT_CW_I16_F32, device=True, **kw)
    assert_equal_singles(enc, INPUTS6, CALLS, abi.FMT_CW_I16_F32, parts, clipped, **kw)


# ------------------------------------------------------------------ 6b. launch blocks: the block offset
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("cw_format", [abi.FMT_CW_I16_F32, abi.FMT_CW_F64])
@pytest.mark.parametrize("enc", ["iir", "fir"])
def test_launch_blocks(icw, enc, cw_format, device, monkeypatch):
    """263-frame launch blocks (read at context creation): the 2 500-frame call is ten of them, so the per-stream
    kernels run with block offsets t0 = 263 k and place their tiles, and KFE reads its input, at t0 times the
    stream's own frame size.  The one-input contexts they are compared with are created before the setting, so
    they run every call as one launch block."""
    kw = dict(k_M=254) if enc == "fir" else {}
    for s, inp in enumerate(INPUTS6):                        # the references first, outside the block setting
        single(enc, inp, s, sum(CALLS), CALLS, cw_format, **kw)
    monkeypatch.setenv("ICW_BLOCK", "263")
    _, parts, clipped, _ = run_mixed(enc, INPUTS6, CALLS, cw_format, device=device, **kw)
    assert_equal_singles(enc, INPUTS6, CALLS, cw_format, parts, clipped, **kw)


# ------------------------------------------------------------------ 7. refusals, each changing nothing
def _raw_call(ctx, enc, rows, in_stride, out, out_stride, n, cw_format):
    fn = ctx._lib.icw_encode_cwave_iir if enc == "iir" else ctx._lib.icw_encode_cwave
    return fn(ctx.h, 0, ctx.n_streams, rows.ctypes.data, in_stride, out.ctypes.data, out_stride, n, cw_format, 0, None)


@pytest.mark.parametrize("enc", ["iir", "fir"])
def test_refusals_change_nothing(icw, enc):
    inputs = INPUTS6[:3]
    n, cw_format = 600, abi.FMT_CW_I16_F32
    raws = [loud_pcm(s, 2 * n, r, c, f) for s, (r, f, c) in enumerate(inputs)]
    rows = rows_of(inputs, raws, 0, n)
    wide_in, wide_out = rows.shape[1], n * 12
    out = np.zeros((3, wide_out), np.uint8)

    ctx = make_ctx(inputs, enc, True)
    # the opt-in off again, the count above 1
    ctx.enable_stream_encode(False)
    assert _raw_call(ctx, enc, rows, wide_in, out, wide_out, n, cw_format) == abi.EUNSUPPORTED and not out.any()
    ctx.enable_stream_encode(False)                          # nothing to undo: ICW_OK
    ctx.enable_stream_encode()
    # a stride that holds the mono streams' frames but not the widest stream's
    assert _raw_call(ctx, enc, rows, wide_in, out, wide_out - 1, n, cw_format) == abi.EINVAL and not out.any()
    assert _raw_call(ctx, enc, rows, wide_in - 1, out, wide_out, n, cw_format) == abi.EINVAL and not out.any()
    import torch
    d_in, d_out = torch.from_numpy(rows).cuda(), torch.zeros((3, wide_out), dtype=torch.uint8, device="cuda")
    fn = ctx._lib.icw_encode_cwave_iir if enc == "iir" else ctx._lib.icw_encode_cwave
    for i_s, o_s in ((wide_in, wide_out - 1), (wide_in - 1, wide_out)):
        assert fn(ctx.h, 0, 3, d_in.data_ptr(), i_s, d_out.data_ptr(), o_s, n, cw_format, abi.F_DEVICE_PTRS, None) == abi.EINVAL
    ctx.synchronize()
    assert not d_out.cpu().numpy().any()
    assert [ctx.encode_clipped(s) for s in range(3)] == [0, 0, 0] and ctx.stream_input_count() == 3
    # a good call after them is the fresh streams' first call
    got = encode_call(ctx, enc, rows, n, cw_format)
    clipped = [ctx.encode_clipped(s) for s in range(3)]
    ctx.close()
    for s in range(3):
        ref_parts, ref_clip = single(enc, inputs[s], s, 2 * n, [n], cw_format)
        assert np.array_equal(got[s], ref_parts[0]) and clipped[s] == ref_clip


def test_fp_check_stays_refused_for_the_iir_encoder(icw):
    inputs = INPUTS6[:2]
    cfg = graph.default_config(44100, fmt=abi.FMT_I16, channels=2)
    cfg.fp_check = 1
    ctx = L.Context(cfg, graph.graph_shift_master(), 2)
    ctx.enable_stream_encode()
    for s, (r, f, c) in enumerate(inputs):
        ctx.set_stream_input(r, f, c, s, 1)
    rows = rows_of(inputs, [loud_pcm(s, 100, r, c, f) for s, (r, f, c) in enumerate(inputs)], 0, 100)
    out = np.zeros((2, 100 * 32), np.uint8)
    assert _raw_call(ctx, "iir", rows, rows.shape[1], out, out.shape[1], 100, abi.FMT_CW_F64) == abi.EUNSUPPORTED
    assert not out.any() and ctx.encode_clipped(0) == 0
    ctx.close()


def test_fir_encoder_needs_the_converter_beside_differing_inputs(icw):
    """icw_enable_stream_encode does not stand in for icw_enable_stream_fir: without it the converter cannot be
    on beside differing inputs (the setter's ICW_EUNSUPPORTED, as ever), and icw_encode_cwave returns the
    ICW_EINVAL of a context without a converter"""
    inputs = INPUTS6[:2]
    ctx = make_ctx(inputs, "iir", True)
    assert ctx._lib.icw_set_fir_hilbert(ctx.h, 30, BETA) == abi.EUNSUPPORTED
    rows = rows_of(inputs, [loud_pcm(s, 100, r, c, f) for s, (r, f, c) in enumerate(inputs)], 0, 100)
    out = np.zeros((2, 100 * 32), np.uint8)
    assert _raw_call(ctx, "fir", rows, rows.shape[1], out, out.shape[1], 100, abi.FMT_CW_F64) == abi.EINVAL
    assert not out.any() and ctx.stream_input_count() == 2
    # the IIR encoder serves the same context
    got = encode_call(ctx, "iir", rows, 100, abi.FMT_CW_F64)
    ctx.close()
    for s in range(2):
        ref_parts, _ = single("iir", inputs[s], s, 100, [100], abi.FMT_CW_F64)
        assert np.array_equal(got[s], ref_parts[0])
