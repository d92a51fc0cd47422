"""GPU: per-stream renders in one context (icw_set_stream_render, icw_stream_render_count,
icw_stream_render_size) against the oracle -- one oracle.Stream per GPU stream, each with its own
set_render / set_outbits.  Every comparison is bit for bit: rendered bytes, pre-render doubles, clips,
peak dB bits, de-subnorm counts and the frame counter.  Nothing here has a tolerance."""

import ctypes as C

import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth
from tests.streamrig import NS_FIR20, StreamRig, bits, copy_cfg, entry

pytestmark = pytest.mark.gpu

FS = 48000


R16_ROUND = entry()
R24_TPDF_MEW = entry(abi.RENDER_TPDF, abi.NSHAPE_MEW44, True)
R16_TPDF = entry(abi.RENDER_TPDF)
R24_ROUND = entry(b24=True)
R16_GAUSS_FIR20 = entry(abi.RENDER_GAUSS, NS_FIR20, dth=1.5)
R24_STPDF_RISER = entry(abi.RENDER_STPDF, b24=True, quantz=abi.QUANTZ_MID_RISER, sb16=14, sb24=20)
# runs of length 1 and 2, serial and frame-parallel neighbours, 4- and 6-byte rows side by side
ENTRIES7 = [R16_ROUND, R24_TPDF_MEW, R16_TPDF, R16_TPDF, R24_ROUND, R16_GAUSS_FIR20, R24_STPDF_RISER]
SERIAL7 = [False, True, False, False, False, True, False]


def loud_list(fr=2.0):
    """Shift + Master, the Master loud enough that the -12 dBFS test tones clip"""
    return [graph.master(inputs=("A",), gain=3.0), graph.shift(inputs=("in",), out="A", fr=fr)]


def render_rig(icw, oracle, cfg, entries, n_total, lists=None, **kw):
    """a context whose stream s renders with entries[s] (None: the context's own) and runs the loud list, or
    lists[s]; a call's output rows get one byte more than the widest frames need (an odd out_stride) unless
    the call says pad=0"""
    return StreamRig(icw, oracle, cfg, n_total, renders=entries, lists=lists or [loud_list()] * len(entries), pad=1, **kw)


def matrix(icw, oracle, device, what):
    cfg = graph.default_config(FS)
    rig = render_rig(icw, oracle, cfg, ENTRIES7, 577 + 2049 + 20)
    assert rig.ctx.stream_render_count() == 6
    assert rig.ctx.render_size == 3 and [rig.ctx.stream_render_size(s) for s in range(7)] == [2, 3, 2, 2, 3, 2, 3]
    for n in (577, 2049, 20):
        rig.step(n, device=device, what=what)
    rig.check(what)
    assert sum(sum(st.meters()["clips"]) for st in rig.sts) > 0, "the input was meant to clip"
    assert all(sum(st.meters()["clips"]) > 0 for st in rig.sts)
    rig.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_matrix(icw, oracle, device):
    """seven streams, six entries: three calls of 577, 2 049 and 20 frames (odd, not a multiple of K3c's
    20-sample block, and exactly one block), host and device pointers, an odd out_stride"""
    matrix(icw, oracle, device, "matrix")


def test_matrix_small_blocks(icw, oracle, monkeypatch):
    """the same with 256-frame launch blocks: a call spans several blocks and both scratch sets"""
    monkeypatch.setenv("ICW_BLOCK", "256")
    matrix(icw, oracle, True, "matrix, ICW_BLOCK=256")


@pytest.mark.parametrize("kernel", ["serial", "row"])
def test_both_serial_kernels(icw, oracle, monkeypatch, kernel):
    """ICW_RENDER=serial|row: the serial runs through K3b (a lane per channel, time-major dither rows) and
    through K3c (a row per channel, generator-major rows); a new context per setting"""
    monkeypatch.setenv("ICW_RENDER", kernel)
    monkeypatch.setenv("ICW_BLOCK", "512")
    matrix(icw, oracle, False, f"ICW_RENDER={kernel}")


def test_subset_and_one_stream_calls(icw, oracle, monkeypatch):
    """icw_process_streams over a range inside one run, over ranges straddling runs and over one stream.  A
    uniform call launches what a one-render context with that entry launches: the one-stream call over a
    ROUND stream is K5's case -- the same K1 kernel and launch counts as on a one-render context, and the
    same bytes"""
    monkeypatch.setenv("ICW_K1_MODE", "row")
    monkeypatch.setenv("ICW_STREAM1", "1")
    cfg = graph.default_config(FS)
    rig = render_rig(icw, oracle, cfg, ENTRIES7, 4000)
    rig.step(300, what="whole batch")
    rig.step(700, first=2, count=2, what="inside one run")
    rig.step(301, first=1, count=4, what="serial, a run of two, frame-parallel")
    rig.step(259, first=4, count=3, what="frame-parallel, serial, frame-parallel")
    rig.step(100, first=5, count=1, what="one serial stream")
    out = rig.step(576, first=4, count=1, timing=True, pad=0, what="one ROUND stream")
    k1, (_, launches) = rig.ctx.last_k1_kernel(), rig.ctx.last_timing()
    rig.step(333, what="whole batch again")
    rig.check("subsets")
    rig.close()
    # the same stream in a one-render context: the same calls, then the one-stream call
    one = render_rig(icw, oracle, copy_cfg(cfg, need24bits=1, render=R24_ROUND[0]), [None] * 7, 4000)
    assert one.ctx.stream_render_count() == 1
    one.t[4] = 300 + 301 + 259
    ref = one.sts[4]
    ref.process(one.raw[4][:one.t[4] * 4], one.t[4])
    rows = np.zeros((7, one.t[4] * 4), np.uint8)
    rows[4] = one.raw[4][:one.t[4] * 4]
    one.ctx.process(rows, one.t[4])
    want = one.step(576, first=4, count=1, timing=True, pad=0, what="one-render context")
    assert (one.ctx.last_k1_kernel(), one.ctx.last_timing()[1]) == (k1, launches) == (abi.K1_ROW, (1, 1))
    assert np.array_equal(out, want)
    one.close()


def test_count_one_is_todays_path(icw, oracle, monkeypatch):
    """one entry given to every stream through icw_set_stream_render is a one-render context: the bytes and
    the launch counts of a context set through icw_set_render + icw_set_outbits"""
    monkeypatch.setenv("ICW_BLOCK", "256")
    cfg = graph.default_config(FS)
    res = []
    for how in ("stream", "context", "stream by stream"):
        rig = render_rig(icw, oracle, cfg, [None] * 4, 1500)
        r, b24 = R24_TPDF_MEW
        if how == "stream":
            rig.set_render(0, R24_TPDF_MEW, count=4)
        elif how == "stream by stream":
            for s in (2, 0, 3, 1):
                rig.set_render(s, R24_TPDF_MEW)
        else:
            rig.ctx.set_render(r)
            rig.ctx.set_outbits(b24)
            for s, st in enumerate(rig.sts):
                st.set_render(r)
                st.set_outbits(b24)
                rig.osz[s] = 6
        assert rig.ctx.stream_render_count() == 1 and rig.ctx.render_size == 3, how
        out = rig.step(1100, timing=True, pad=0, what=how)
        res.append((out, rig.ctx.last_timing()[1], rig.ctx.last_dither_chunks()))
        rig.check(how)
        rig.close()
    for out, launches, chunks in res[1:]:
        assert np.array_equal(out, res[0][0]) and launches == res[0][1] and chunks == res[0][2]
    assert res[0][1][0] > 1


def test_context_wide_setters_on_a_mixed_context(icw, oracle):
    """icw_set_render on a mixed context gives every stream the new setting, keeps each stream's depth and
    restarts the shaping; icw_set_outbits gives every stream the new depth and keeps its setting"""
    cfg = graph.default_config(FS)
    rig = render_rig(icw, oracle, cfg, ENTRIES7, 3000)
    rig.step(500, what="mixed")
    r, _ = entry(abi.RENDER_RPDF, abi.NSHAPE_FW44, dth=0.75)
    rig.ctx.set_render(r)
    for st in rig.sts:
        st.set_render(r)
    assert rig.ctx.stream_render_count() == 2 and rig.ctx.render_size == 3
    rig.step(611, what="after icw_set_render")
    rig.set_render(3, R16_TPDF)
    rig.set_render(6, R24_STPDF_RISER)
    assert rig.ctx.stream_render_count() == 4
    rig.ctx.set_outbits(0)
    for s, st in enumerate(rig.sts):
        st.set_outbits(0)
        rig.osz[s] = 4
    assert rig.ctx.stream_render_count() == 3 and rig.ctx.render_size == 2
    rig.step(450, what="after icw_set_outbits")
    rig.ctx.set_render(r)
    for st in rig.sts:
        st.set_render(r)
    assert rig.ctx.stream_render_count() == 1
    rig.step(300, what="one render again")
    rig.check("context-wide setters")
    rig.close()


def test_edits_between_calls(icw, oracle):
    """one stream's entry changed mid-track twice, ROUND -> TPDF + MEW44 -> 24-bit ROUND, on a context created
    ROUND + flat (the render state is created by the first edit): its shaping restarts, its MT19937 words go
    on, its peak folds against the old bound, and its neighbours carry on untouched"""
    cfg = graph.default_config(FS)
    rig = render_rig(icw, oracle, cfg, [None] * 3, 3000)
    assert abi.StateBlob.from_buffer_copy(rig.ctx.get_state(1)).has_render == 0
    rig.step(700, what="ROUND")
    rig.set_render(1, entry(abi.RENDER_TPDF, abi.NSHAPE_MEW44))
    assert rig.ctx.stream_render_count() == 2
    assert abi.StateBlob.from_buffer_copy(rig.ctx.get_state(1)).has_render == 1
    rig.step(650, what="TPDF + MEW44")
    rig.check("after the first edit")
    rig.set_render(1, entry(abi.RENDER_TPDF, abi.NSHAPE_MEW44))          # unchanged: the shaping restarts all the same
    rig.step(333, what="the same entry again")
    rig.set_render(1, R24_ROUND)
    rig.step(500, what="24-bit ROUND")
    rig.check("after the second edit")
    rig.set_render(1, (abi.RenderCfg.from_buffer_copy(bytes(cfg.render)), False))     # its neighbours' render
    assert rig.ctx.stream_render_count() == 1
    rig.step(200, what="one render again")
    rig.check("edits")
    rig.close()


@pytest.mark.parametrize("kind", ["real", "cwave"])
def test_with_per_stream_lists_and_inputs(icw, oracle, kind):
    """four streams with different inputs, different Shift lists and different renders in one context"""
    cfg = graph.default_config(FS)
    if kind == "real":
        inputs = [(44100, abi.FMT_I16, 2), (96000, abi.FMT_F32, 1), (48000, abi.FMT_I24, 2), (8000, abi.FMT_U8, 1)]
    else:
        cfg.in_format = abi.FMT_CW_F64
        inputs = [(44100, abi.FMT_CW_F64, 2), (96000, abi.FMT_CW_I16, 1), (48000, abi.FMT_CW_F32, 2), (48000, abi.FMT_CW_I16_F32, 2)]
    lists = [loud_list(fr) for fr in (2.0, -3.5, 7.25, 0.5)]
    entries = [R24_TPDF_MEW, R16_TPDF, R16_ROUND, R24_STPDF_RISER]
    rig = render_rig(icw, oracle, cfg, entries, 1200, lists=lists, inputs=inputs, cwave=kind == "cwave")
    assert (rig.ctx.stream_render_count(), rig.ctx.stream_graph_count(), rig.ctx.stream_input_count()) == (4, 4, 4)
    rig.step(700, what=kind)
    rig.step(500, device=True, what=kind)
    rig.check(kind)
    rig.close()


@pytest.mark.parametrize("which", ["serial", "frame-parallel"])
def test_forced_dither_rejects(icw, oracle, which):
    """a rejected dsopen pair planted through the state blob in one stream of a run of two: zeroed raw MT
    words temper to 0 and force the rejection (mt_jrnd.c:245-256), so K3f redoes that generator alone"""
    cfg = graph.default_config(FS)
    e = R24_TPDF_MEW if which == "serial" else R16_TPDF
    rig = render_rig(icw, oracle, cfg, [R16_ROUND, e, e, R24_ROUND], 3000)
    rig.step(700, what="before")
    blob = abi.StateBlob.from_buffer_copy(rig.ctx.get_state(2))
    assert blob.has_render == 1
    for ch in range(2):
        w = np.frombuffer(bytes(blob.mt[ch]), dtype=np.uint32).copy()
        i0 = blob.mt_idx[ch]
        start = min(i0 + 5, 623)
        w[start:min(start + 6, 624)] = 0
        if i0 + 5 >= 624:
            w[:6] = 0
        C.memmove(C.addressof(blob.mt[ch]), w.ctypes.data, 624 * 4)
        rig.sts[2].set_mt(ch, w, i0)
    rig.ctx.set_state(2, bytes(blob))
    rig.step(2300, what="planted")
    rig.check(which)
    rig.close()


def test_refusals_change_nothing(icw, oracle):
    cfg = graph.default_config(FS)
    rig = render_rig(icw, oracle, cfg, [R16_TPDF, R24_TPDF_MEW, R16_ROUND], 6000)
    ctx, lib = rig.ctx, rig.ctx._lib
    r, _ = R16_ROUND

    def still_the_same(what):
        assert ctx.stream_render_count() == 3, what
        assert [ctx.stream_render_size(s) for s in range(3)] == [2, 3, 2], what
        rig.step(250, what=what)

    # bad arguments
    for first, count in ((-1, 1), (0, 0), (1, 3), (3, 1), (0, 4)):
        assert lib.icw_set_stream_render(ctx.h, first, count, C.byref(r), 0) == abi.EINVAL
    assert lib.icw_set_stream_render(ctx.h, 0, 1, None, 0) == abi.EINVAL
    for field, v in (("sign_bits16", 1), ("sign_bits16", 17), ("sign_bits24", 25), ("quantz_type", 2), ("render_type", 5)):
        bad = abi.RenderCfg.from_buffer_copy(bytes(r))
        setattr(bad, field, v)
        assert lib.icw_set_stream_render(ctx.h, 0, 1, C.byref(bad), 0) == abi.EINVAL, field
    assert lib.icw_stream_render_size(ctx.h, 3) == abi.EINVAL and lib.icw_stream_render_size(ctx.h, -1) == abi.EINVAL
    still_the_same("bad arguments")
    # while the count is above 1: the FIR converter, a bus-form list
    assert lib.icw_set_fir_hilbert(ctx.h, 64, 8.0) == abi.EUNSUPPORTED
    still_the_same("icw_set_fir_hilbert")
    bus = graph.graph_feedback_pm_shift()
    assert icw.graph_form(cfg, bus) == 1
    acc = C.c_int()
    assert lib.icw_set_graph(ctx.h, graph.node_array(bus), len(bus), 0, C.byref(acc)) == abi.EUNSUPPORTED
    still_the_same("icw_set_graph with a bus-form list")
    # out_stride_bytes must hold n_frames frames of every stream of the call, device pointers included
    n = 64
    rows = rig.rows(n, 0, 3)
    out = np.zeros((3, n * 6), np.uint8)
    for stride in (n * 4, n * 6 - 1):
        assert lib.icw_process_streams(ctx.h, 0, 3, rows.ctypes.data, rows.shape[1], out.ctypes.data, stride, n, 0, None,
                                       None) == abi.EINVAL
        assert lib.icw_process_streams(ctx.h, 0, 3, rows.ctypes.data, rows.shape[1], out.ctypes.data, stride, n,
                                       abi.F_DEVICE_PTRS, None, None) == abi.EINVAL
    assert not out.any()
    still_the_same("out_stride too small for the widest stream")
    rig.check("refusals")
    rig.close()

    # the call that would raise the count above 1: the FIR converter on, FP_CHECK, a bus-form list in force
    def refused(ctx, sts, raw, what, fir=None):
        assert ctx._lib.icw_set_stream_render(ctx.h, 0, 1, C.byref(R24_TPDF_MEW[0]), 1) == abi.EUNSUPPORTED, what
        assert ctx.stream_render_count() == 1 and ctx.stream_render_size(0) == 2, what
        got, pre = ctx.process(raw, 300, want_pre=True)
        for s, st in enumerate(sts):
            ro, rp = st.process(raw[s], 300, want_pre=True)
            assert np.array_equal(bits(pre[s]), bits(rp)) and np.array_equal(got[s], ro), what
        # one entry for every stream keeps the count at 1 and is served
        ctx.set_stream_render(*R24_ROUND)
        assert ctx.stream_render_count() == 1 and ctx.render_size == 3, what
        ctx.close()

    raw = synth.batch_pcm(2, 300, FS)
    nodes = graph.graph_shift_master()
    ctx = icw.Context(copy_cfg(cfg), nodes, 2)
    ctx.set_fir_hilbert(64, 8.0)
    sts = [oracle.Stream(copy_cfg(cfg), nodes) for _ in range(2)]
    for st in sts:
        st.set_fir(64, 8.0)
    refused(ctx, sts, raw, "FIR converter on")
    fc = copy_cfg(cfg, fp_check=1)
    refused(icw.Context(copy_cfg(fc), nodes, 2), [oracle.Stream(copy_cfg(fc), nodes) for _ in range(2)], raw, "FP_CHECK")
    refused(icw.Context(copy_cfg(cfg), bus, 2), [oracle.Stream(copy_cfg(cfg), bus) for _ in range(2)], raw, "bus-form list")
