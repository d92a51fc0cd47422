"""GPU: per-stream CWAVE inputs in one context (icw_enable_stream_cwave, then icw_set_stream_input with the
four CWAVE frame formats) against the oracle -- one oracle.Stream per GPU stream, each with its own rate,
frame format and channels.  A call over differing CWAVE inputs launches no K0: the output kernel reads the
file frames itself.  Every comparison is bit for bit: rendered bytes, pre-render doubles, clips, peaks,
de-subnorm counts and the frame counter.  Nothing here has a tolerance."""

import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth

from tests.streamrig import StreamRig, bits, copy_cfg, shift_list

pytestmark = pytest.mark.gpu

CW = (abi.FMT_CW_F64, abi.FMT_CW_I16, abi.FMT_CW_I16_F32, abi.FMT_CW_F32)
RATES = (8000, 44100, 48000, 96000, 192000)
# four formats x mono / stereo, the rates dealt so that neighbours differ and every rate is used
INPUTS8 = [(RATES[(2 * k + ch) % 5], fmt, ch + 1) for k, fmt in enumerate(CW) for ch in range(2)]


signal = StreamRig.signal


class CwRig(StreamRig):
    """the rig on a context that asked for per-stream CWAVE inputs: CWAVE streams get synth.stream_cwave's
    analytic signal, real ones synth.stream_pcm's"""

    def __init__(self, icw, oracle, cfg, inputs, lists, n_total):
        super().__init__(icw, oracle, cfg, n_total, inputs=inputs, lists=lists, cwave=True)

    def device_step(self, n, stride, first=0, count=None):
        """one device-pointer call with the given in_stride over frames [t, t + n); returns (bytes, pre)"""
        import torch
        ctx, count = self.ctx, len(self.sts) - first if count is None else count
        rows = self.rows(n, first, count)
        wide = np.zeros((count, stride), np.uint8)
        wide[:, :rows.shape[1]] = rows
        osz = 2 * ctx.render_size
        d_in = torch.from_numpy(wide.reshape(-1)).cuda()
        d_out = torch.zeros((count, n * osz), dtype=torch.uint8, device="cuda")
        d_pre = torch.zeros((count, n, 2), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc = ctx._lib.icw_process_streams(ctx.h, first, count, d_in.data_ptr(), stride, d_out.data_ptr(), n * osz, n,
                                          abi.F_DEVICE_PTRS | abi.F_DEBUG_PRE, d_pre.data_ptr(), None)
        assert rc == abi.OK, rc
        ctx.synchronize()
        return d_out.cpu().numpy(), d_pre.cpu().numpy()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", ["shift_scaled", "c4_unscaled"])
def test_matrix(icw, oracle, case, device):
    """eight streams, four CWAVE formats x mono / stereo at five rates, in one context: calls of 2 500 frames
    (K2 workgroups of 1 024 frames, the last tile partial), 577 and 1"""
    cfg = graph.default_config(48000)
    nodes = graph.graph_shift_master()
    if case == "c4_unscaled":
        cfg.frmod_scaled = 0
        nodes = graph.graph_pm_shift_mix()
    rig = CwRig(icw, oracle, cfg, INPUTS8, [nodes] * 8, 2500 + 577 + 1)
    assert rig.ctx.stream_input_count() == 8
    for n in (2500, 577, 1):
        rig.step(n, device=device, what=case)
    rig.check(case)
    rig.close()


def test_alignment(icw, oracle):
    """device pointers: a stride of the widest row + 2 puts every odd stream's row off its pair's alignment
    (the byte form); a stride rounded up to 16 keeps every 16-, 8- and 4-byte pair aligned (the typed
    loads).  Both give the oracle's bytes, so the same bytes.  The mono CW_I16_F32 stream (6-byte frames)
    is in the set"""
    cfg = graph.default_config(48000)
    assert any(fmt == abi.FMT_CW_I16_F32 and ch == 1 for _, fmt, ch in INPUTS8)
    n = 1500
    outs = []
    for how in ("byte form", "typed loads"):
        rig = CwRig(icw, oracle, cfg, INPUTS8, [graph.graph_shift_master()] * 8, n)
        wide = n * max(rig.fsz(s) for s in range(8))
        stride = wide + 2 if how == "byte form" else (wide + 15) & ~15
        out, pre = rig.device_step(n, stride)
        for s in range(8):
            ro, rp = rig.sts[s].process(rig.raw[s], n, want_pre=True)
            assert np.array_equal(bits(pre[s]), bits(rp)), (how, s, rig.inputs[s])
            assert np.array_equal(out[s], ro), (how, s, rig.inputs[s])
        rig.check(how)
        rig.close()
        outs.append(out)
    assert np.array_equal(outs[0], outs[1])


def test_launch_blocks(icw, oracle, monkeypatch):
    """one call over several launch blocks (ICW_BLOCK at its smallest, 256 frames; a block that is no
    multiple of the tile too): the skipped K0 leaves no event wait behind, host and device pointers"""
    cfg = graph.default_config(48000)
    for block in ("256", "263"):
        monkeypatch.setenv("ICW_BLOCK", block)
        rig = CwRig(icw, oracle, cfg, INPUTS8[:5], [graph.graph_shift_master()] * 5, 2100)
        rig.step(1100, what="blocks " + block)
        rig.step(1000, device=True, what="blocks " + block)
        rig.check("blocks " + block)
        rig.close()


def test_fades_and_tail(icw, oracle):
    """icw_stream_open with 5 ms fades and a sec_align tail on two CWAVE streams of different rates: the
    fade scales all four values at each stream's own rate, and each track runs to the end of its own tail"""
    cfg = graph.default_config(48000)
    inputs = [(1500, abi.FMT_CW_I16, 2), (2000, abi.FMT_CW_F32, 1)]
    rig = CwRig(icw, oracle, cfg, inputs, [graph.graph_shift_master()] * 2, 1000)
    totals = []
    for s in range(2):
        rig.ctx.stream_open(s, 1000, 5, 5, 1)
        totals.append(1000 + rig.sts[s].open(1000, 5, 5, 1))
        rig.raw[s] = np.concatenate([rig.raw[s], np.zeros((totals[s] - 1000) * rig.fsz(s), np.uint8)])
    assert totals == [1500, 2000]
    blob = [abi.StateBlob.from_buffer_copy(rig.ctx.get_state(s)) for s in range(2)]
    assert [(b.n_fade_in, b.n_fade_out) for b in blob] == [(7, 7), (10, 10)]
    rig.step(1500, what="tracks")
    rig.step(500, first=1, count=1, what="the longer tail")
    rig.check("fades")
    rig.close()


def test_counter_wrap(icw, oracle):
    """two CWAVE streams at different rates, each within 100 frames of its own rate x 1 000 wrap"""
    cfg = graph.default_config(48000)
    inputs = [(8000, abi.FMT_CW_I16, 2), (44100, abi.FMT_CW_F64, 1)]
    rig = CwRig(icw, oracle, cfg, inputs, [graph.graph_shift_master()] * 2, 300)
    for s, (rate, _, _) in enumerate(inputs):
        nf = rate * abi.HZ_SCALE - 60 - 17 * s
        blob = abi.StateBlob.from_buffer_copy(rig.ctx.get_state(s))
        blob.n_frame = nf
        rig.ctx.set_state(s, bytes(blob))
        rig.sts[s].set_n_frame(nf)
    rig.step(300, what="wrap")
    assert [rig.ctx.n_frame(s) for s in range(2)] == [240, 240 - 17]
    rig.check("wrap")
    rig.close()


def test_per_stream_lists_and_slabs(icw, oracle):
    """six CWAVE streams at one counter, two each on (list A, 44 100), (list A, 48 000), (list B, 48 000),
    the formats mixed: a rotation slab shared across rates, or across lists, gives wrong bytes"""
    cfg = graph.default_config(48000)
    a, b = shift_list(2.0), shift_list(3.5)
    inputs = [(44100, abi.FMT_CW_I16, 2), (44100, abi.FMT_CW_F64, 1), (48000, abi.FMT_CW_F32, 2), (48000, abi.FMT_CW_I16_F32, 2),
              (48000, abi.FMT_CW_I16, 1), (48000, abi.FMT_CW_F64, 2)]
    rig = CwRig(icw, oracle, cfg, inputs, [a, a, a, a, b, b], 1300)
    assert rig.ctx.stream_input_count() == 6 and rig.ctx.stream_graph_count() == 2
    rig.step(1100, what="slabs")
    rig.step(200, what="slabs")
    rig.check("slabs")
    rig.close()


PATHS = {
    "bus_form": dict(nodes=graph.graph_feedback_pm_shift),
    "tpdf_flat": dict(nodes=graph.graph_shift_master, render=(abi.RENDER_TPDF, abi.NSHAPE_FLAT)),
    "tpdf_mew44_24": dict(nodes=graph.graph_shift_master, need24bits=1, render=(abi.RENDER_TPDF, abi.NSHAPE_MEW44)),
    "fp_check": dict(nodes=graph.graph_shift_master, fp_check=1),
}


@pytest.mark.parametrize("case", sorted(PATHS))
def test_other_paths(icw, oracle, case):
    """a bus-form list with PM and Shift inside a feedback loop at two rates (K4), TPDF + flat (the
    frame-parallel dither), TPDF + MEW44 24-bit (the serial render), an FP_CHECK context with its census"""
    kw = dict(PATHS[case])
    nodes, render = kw.pop("nodes")(), kw.pop("render", None)
    cfg = copy_cfg(graph.default_config(48000), **kw)
    if render:
        cfg.render.render_type, cfg.render.nshape_type = render
    inputs = [(44100, abi.FMT_CW_I16, 2), (96000, abi.FMT_CW_F32, 1), (44100, abi.FMT_CW_F64, 2)]
    if case == "bus_form":
        assert icw.graph_form(cfg, nodes) == 1
    rig = CwRig(icw, oracle, cfg, inputs, [nodes] * 3, 1150)
    assert rig.ctx.stream_input_count() == 3
    rig.step(700, what=case)
    rig.step(450, what=case)
    rig.check(case, census=bool(cfg.fp_check))
    rig.close()


def test_two_kinds_in_one_context(icw, oracle):
    """two real and two CWAVE streams: calls over [0, 2) and [2, 4) match the oracle, a call over [0, 4)
    is refused and changes nothing; stream 1 then plays WAV -> CWAVE -> WAV, and its third call continues
    the converter's rings and phase from the first (the oracle's Stream does the same)"""
    cfg = graph.default_config(48000)
    inputs = [(44100, abi.FMT_I16, 2), (48000, abi.FMT_F32, 1), (96000, abi.FMT_CW_I16, 2), (44100, abi.FMT_CW_F64, 1)]
    rig = CwRig(icw, oracle, cfg, inputs, [graph.graph_shift_master()] * 4, 2000)
    ctx, lib = rig.ctx, rig.ctx._lib
    assert ctx.stream_input_count() == 4

    def halves(n, what):
        rig.step(n, first=0, count=2, what=what + " real")
        rig.step(n, first=2, count=2, what=what + " cwave")

    halves(301, "first")
    rows = rig.rows(64, 0, 4)
    out = np.zeros((4, 64 * 4), np.uint8)
    assert lib.icw_process_streams(ctx.h, 0, 4, rows.ctypes.data, rows.strides[0], out.ctypes.data, out.strides[0], 64, 0,
                                   None, None) == abi.EUNSUPPORTED
    assert lib.icw_process_batch(ctx.h, rows.ctypes.data, rows.strides[0], out.ctypes.data, out.strides[0], 64, 0, None,
                                 None) == abi.EUNSUPPORTED
    halves(200, "after the refusal")
    # stream 1: WAV -> CWAVE -> WAV.  Its signal is regenerated for each frame format, from the same frame on
    wav = rig.inputs[1]
    rig.set_input(1, 48000, abi.FMT_CW_F32, 2)
    rig.raw[1] = signal(11, 2000, 48000, abi.FMT_CW_F32, 2)
    rig.step(250, first=1, count=3, what="stream 1 on CWAVE")
    rig.step(250, first=0, count=1, what="stream 0 alone")
    rig.set_input(1, *wav)
    rig.raw[1] = signal(1, 2000, *wav)
    halves(300, "stream 1 on WAV again")
    # the CWAVE call left the converter alone: the phase counts the 801 WAV frames only (the rings are in
    # the bytes just compared: the oracle's Stream went WAV -> CWAVE -> WAV with one converter too)
    blob = abi.StateBlob.from_buffer_copy(rig.ctx.get_state(1))
    assert list(blob.hq_phase) == [(301 + 200 + 300) % 4] * 2
    rig.check("two kinds")
    rig.close()


def test_collapse(icw, oracle):
    """every stream given one CWAVE input: a one-input context (today's K0 + K2) whose outputs are those of
    a context created with that input; icw_set_input to a real format and back"""
    cfg = graph.default_config(48000)
    nodes = graph.graph_shift_master()
    one = (44100, abi.FMT_CW_I16_F32, 2)
    raw = synth.batch_pcm(3, 800, one[0], channels=one[2], fmt=one[1])
    fresh = icw.Context(copy_cfg(cfg, sample_rate=one[0], in_format=one[1], in_channels=one[2]), nodes, 3)
    want, want_pre = fresh.process(raw, 800, want_pre=True)
    fresh.close()
    ctx = icw.Context(copy_cfg(cfg), nodes, 3)
    ctx.enable_stream_cwave()
    for s, (rate, fmt, ch) in enumerate(INPUTS8[:3]):
        ctx.set_stream_input(rate, fmt, ch, s, 1)
    assert ctx.stream_input_count() == 3
    ctx.set_stream_input(*one)
    assert ctx.stream_input_count() == 1
    ctx.enable_stream_cwave(False)                      # one input, context-wide: nothing per stream is CWAVE
    ctx.enable_stream_cwave()
    got, got_pre = ctx.process(raw, 800, want_pre=True)
    assert np.array_equal(bits(got_pre), bits(want_pre)) and np.array_equal(got, want)
    ctx.close()
    # a context created on CWAVE input takes per-stream inputs with the opt-in; set_input to a real format
    # and back to CWAVE leaves one-input contexts that match the oracle
    ctx = icw.Context(copy_cfg(cfg, sample_rate=one[0], in_format=one[1], in_channels=one[2]), nodes, 3)
    ctx.enable_stream_cwave()
    ctx.set_stream_input(48000, abi.FMT_CW_F64, 1, 1, 1)
    assert ctx.stream_input_count() == 2
    sts = [oracle.Stream(copy_cfg(cfg), nodes) for _ in range(3)]
    for rate, fmt, ch in ((48000, abi.FMT_I16, 2), one):
        ctx.set_input(rate, fmt, ch)
        assert ctx.stream_input_count() == 1
        raw = synth.batch_pcm(3, 400, rate, channels=ch, fmt=fmt)
        got, got_pre = ctx.process(raw, 400, want_pre=True)
        for s in range(3):
            sts[s].set_input(rate, fmt, ch)
            ro, rp = sts[s].process(raw[s], 400, want_pre=True)
            assert np.array_equal(bits(got_pre[s]), bits(rp)) and np.array_equal(got[s], ro), (fmt, s)
    ctx.close()


def test_refusals_change_nothing(icw, oracle):
    cfg = graph.default_config(48000)
    nodes = graph.graph_shift_master()
    # without the opt-in: every refusal of today
    ctx = icw.Context(copy_cfg(cfg), nodes, 2)
    for fmt in CW:
        assert ctx._lib.icw_set_stream_input(ctx.h, 0, 1, 48000, fmt, 2) == abi.EUNSUPPORTED
    assert ctx.stream_input_count() == 1
    ctx.close()
    ctx = icw.Context(copy_cfg(cfg, in_format=abi.FMT_CW_F64), nodes, 2)
    assert ctx._lib.icw_set_stream_input(ctx.h, 0, 1, 48000, abi.FMT_I16, 2) == abi.EUNSUPPORTED
    assert ctx._lib.icw_set_stream_input(ctx.h, 0, 1, 44100, abi.FMT_CW_I16, 2) == abi.EUNSUPPORTED
    assert ctx.stream_input_count() == 1
    ctx.close()
    assert icw.load().icw_enable_stream_cwave(None, 1) == abi.EINVAL
    assert icw.load().icw_enable_stream_cwave(None, 0) == abi.EINVAL

    # with it
    inputs = [(44100, abi.FMT_CW_I16, 2), (96000, abi.FMT_CW_F32, 1)]
    rig = CwRig(icw, oracle, cfg, inputs, [nodes] * 2, 3000)
    ctx, lib = rig.ctx, rig.ctx._lib

    def still_the_same(what):
        assert ctx.stream_input_count() == 2, what
        rig.step(250, what=what)

    assert lib.icw_set_fir_hilbert(ctx.h, 64, 8.0) == abi.EUNSUPPORTED
    ctx.enable_stream_fir()
    assert lib.icw_set_fir_hilbert(ctx.h, 64, 8.0) == abi.EUNSUPPORTED
    still_the_same("set_fir_hilbert beside per-stream CWAVE inputs")
    assert lib.icw_enable_stream_cwave(ctx.h, 0) == abi.EUNSUPPORTED
    rig.set_input(0, 48000, abi.FMT_CW_F64, 2)           # still on: the setter takes a CWAVE format
    rig.raw[0] = signal(0, 3000, *rig.inputs[0])
    still_the_same("turning the opt-in off with CWAVE streams")
    for first, count in ((-1, 1), (0, 0), (1, 2), (2, 1), (0, 3)):
        assert lib.icw_set_stream_input(ctx.h, first, count, 48000, abi.FMT_CW_I16, 2) == abi.EINVAL
    for rate, fmt, ch in ((0, abi.FMT_CW_I16, 2), (abi.MAX_FS_SRC + 1, abi.FMT_CW_I16, 2), (48000, abi.FMT_CW_I16, 0), (48000, 9, 2)):
        assert lib.icw_set_stream_input(ctx.h, 0, 1, rate, fmt, ch) == abi.EINVAL
    still_the_same("bad arguments")
    n = 64
    rows = rig.rows(n, 0, 2)
    out = np.zeros((2, n * 4), np.uint8)
    assert rows.shape[1] == n * 32
    for stride in (n * 32 - 1, n * 8):                 # the narrow stream's frames fit, the widest's do not
        assert lib.icw_process_streams(ctx.h, 0, 2, rows.ctypes.data, stride, out.ctypes.data, out.strides[0], n, 0, None,
                                       None) == abi.EINVAL
    x = np.zeros((2, n, 2))
    assert lib.icw_process_streams(ctx.h, 0, 2, rows.ctypes.data, rows.strides[0], out.ctypes.data, out.strides[0], n,
                                   abi.F_DEBUG_INPUT, x.ctypes.data, None) == abi.EUNSUPPORTED
    enc = np.zeros((2, n * 32), np.uint8)
    ctx.enable_stream_encode()
    for fn in (lib.icw_encode_cwave, lib.icw_encode_cwave_iir):
        assert fn(ctx.h, 0, 2, rows.ctypes.data, rows.strides[0], enc.ctypes.data, enc.strides[0], n, abi.FMT_CW_F64, 0,
                  None) == abi.EINVAL
    still_the_same("stride, debug hook, encoders")
    rig.check("refusals")
    rig.close()

    # the converter on: no CWAVE format through the setter, opt-ins or not
    ctx = icw.Context(copy_cfg(cfg), nodes, 2)
    ctx.enable_stream_cwave()
    ctx.enable_stream_fir()
    ctx.set_fir_hilbert(64, 8.0)
    assert ctx._lib.icw_set_stream_input(ctx.h, 0, 1, 44100, abi.FMT_CW_I16, 2) == abi.EUNSUPPORTED
    assert ctx.stream_input_count() == 1
    raw = synth.batch_pcm(2, 300, 48000)
    got, pre = ctx.process(raw, 300, want_pre=True)
    for s in range(2):
        st = oracle.Stream(copy_cfg(cfg), nodes)
        st.set_fir(64, 8.0)
        ro, rp = st.process(raw[s], 300, want_pre=True)
        assert np.array_equal(bits(pre[s]), bits(rp)) and np.array_equal(got[s], ro)
    ctx.close()
