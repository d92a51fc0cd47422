"""GPU: per-stream inputs in one context (icw_set_stream_input, icw_stream_input_count) against the
oracle -- one oracle.Stream per GPU stream, each with its own rate, sample format and channels.
Every comparison is bit for bit: rendered bytes, pre-render doubles, clips, peaks, de-subnorm counts
and the frame counter.  Nothing here has a tolerance."""

import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth
from tests.streamrig import StreamRig, bits, copy_cfg, shift_list

pytestmark = pytest.mark.gpu

FORMATS = (abi.FMT_U8, abi.FMT_I16, abi.FMT_I24, abi.FMT_I32, abi.FMT_F32)
RATES = (8000, 44100, 48000, 96000, 192000)
# five formats x mono / stereo, the rates dealt so that neighbours differ and every rate is used twice
INPUTS10 = [(RATES[(2 * k + ch) % 5], fmt, ch + 1) for k, fmt in enumerate(FORMATS) for ch in range(2)]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", ["shift_scaled", "c4_unscaled"])
def test_matrix(icw, oracle, case, device):
    """ten streams, five formats x mono / stereo at five rates, in one context: calls of 2 500 frames
    (K2 workgroups of 1 024), 577 and 1"""
    cfg = graph.default_config(48000)
    nodes = graph.graph_shift_master()
    if case == "c4_unscaled":
        cfg.frmod_scaled = 0
        nodes = graph.graph_pm_shift_mix()
    rig = StreamRig(icw, oracle, cfg, 2500 + 577 + 1, inputs=INPUTS10, lists=[nodes] * 10)
    assert rig.ctx.stream_input_count() == 10
    for n in (2500, 577, 1):
        rig.step(n, device=device, what=case, wrapper=not device)      # host: through lib.Context.process
    rig.check(case)
    rig.close()


def test_rotation_table_keyed_by_list_and_rate(icw, oracle):
    """six streams at one counter, two each on (list A, 44 100), (list A, 48 000), (list B, 48 000): a
    slab shared across rates, or across lists, gives wrong bytes"""
    cfg = graph.default_config(48000)
    a, b = shift_list(2.0), shift_list(3.5)
    inputs = [(44100, abi.FMT_I16, 2)] * 2 + [(48000, abi.FMT_I16, 2)] * 4
    rig = StreamRig(icw, oracle, cfg, 1300, inputs=inputs, lists=[a, a, a, a, b, b])
    assert rig.ctx.stream_input_count() == 2 and rig.ctx.stream_graph_count() == 2
    rig.step(1100, what="slabs")
    rig.step(200, what="slabs")
    # one list, two rates: the one-entry program table
    rig.check("slabs")
    rig.close()
    rig = StreamRig(icw, oracle, cfg, 700, inputs=inputs[:4], lists=[a] * 4)
    assert rig.ctx.stream_input_count() == 2 and rig.ctx.stream_graph_count() == 1
    rig.step(700, what="one list, two rates")
    rig.check("one list, two rates")
    rig.close()


def test_counter_wrap(icw, oracle):
    """two streams at different rates, each within 100 frames of its own rate x 1 000 wrap"""
    cfg = graph.default_config(48000)
    inputs = [(8000, abi.FMT_I16, 2), (44100, abi.FMT_F32, 1)]
    rig = StreamRig(icw, oracle, cfg, 300, inputs=inputs)
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


def test_fades_and_tail(icw, oracle):
    """icw_stream_open with 5 ms fades and a sec_align tail on two streams of different rates: the fades
    take each stream's own rate, and each track runs to the end of its own tail"""
    cfg = graph.default_config(48000)
    inputs = [(1500, abi.FMT_I16, 2), (2000, abi.FMT_I24, 1)]
    rig = StreamRig(icw, oracle, cfg, 1000, inputs=inputs)
    totals = []
    for s, (rate, fmt, ch) in enumerate(inputs):
        rig.ctx.stream_open(s, 1000, 5, 5, 1)
        totals.append(1000 + rig.sts[s].open(1000, 5, 5, 1))
        # the virtual zero tail (the reader's): the format's zero sample after the track's frames
        rig.raw[s] = np.concatenate([rig.raw[s], np.zeros((totals[s] - 1000) * rig.fsz(s), np.uint8)])
    assert totals == [1500, 2000]
    blob = [abi.StateBlob.from_buffer_copy(rig.ctx.get_state(s)) for s in range(2)]
    assert [(b.n_fade_in, b.n_fade_out) for b in blob] == [(7, 7), (10, 10)]
    rig.step(1500, what="tracks")
    rig.step(500, first=1, count=1, what="the longer tail")
    rig.check("fades")
    rig.close()


def test_mono_bookkeeping(icw, oracle):
    """an all-mono call of mixed formats and rates (K1 on the left chains only), a mono + stereo call,
    and one stream switched mono -> stereo -> mono between calls"""
    cfg = graph.default_config(48000)
    mono = [(44100, abi.FMT_I16, 1), (48000, abi.FMT_F32, 1), (96000, abi.FMT_I24, 1), (8000, abi.FMT_U8, 1)]
    rig = StreamRig(icw, oracle, cfg, 2000, inputs=mono)
    rig.step(600, what="all mono")
    rig.step(300, what="all mono")
    # stream 2 becomes stereo: its signal is regenerated for the new frame, from the same frame on
    def switch(s, ch):
        rate, fmt, _ = rig.inputs[s]
        rig.set_input(s, rate, fmt, ch)
        rig.raw[s] = synth.stream_pcm(s + 10 * ch, 2000, rate, channels=ch, fmt=fmt)
    switch(2, 2)
    assert rig.ctx.stream_input_count() == 4
    rig.step(400, what="mono + stereo")
    switch(2, 1)
    rig.step(400, what="mono again")
    rig.step(300, what="mono again")
    rig.check("mono")
    rig.close()


PATHS = {
    "bus_form": dict(nodes=graph.graph_feedback_pm_shift),
    "tpdf_mew44_24": dict(nodes=graph.graph_shift_master, need24bits=1, render=(abi.RENDER_TPDF, abi.NSHAPE_MEW44)),
    "fp_check": dict(nodes=graph.graph_shift_master, fp_check=1),
}


@pytest.mark.parametrize("case", sorted(PATHS))
def test_other_paths(icw, oracle, case):
    """a bus-form list with PM and Shift inside a feedback loop at two rates (K4), TPDF + MEW44 24-bit
    (the serial render), an FP_CHECK context"""
    kw = dict(PATHS[case])
    nodes, render = kw.pop("nodes")(), kw.pop("render", None)
    cfg = copy_cfg(graph.default_config(48000), **kw)
    if render:
        cfg.render.render_type, cfg.render.nshape_type = render
    inputs = [(44100, abi.FMT_I16, 2), (96000, abi.FMT_F32, 1), (44100, abi.FMT_I32, 2)]
    if case == "bus_form":
        assert icw.graph_form(cfg, nodes) == 1
    rig = StreamRig(icw, oracle, cfg, 1150, inputs=inputs, nodes=nodes)
    assert rig.ctx.stream_input_count() == 3
    rig.step(700, what=case)
    rig.step(450, what=case)
    rig.check(case, census=bool(cfg.fp_check))
    rig.close()


def test_collapse(icw, oracle):
    """icw_set_input on a mixed context, and one input given to every stream through
    icw_set_stream_input, both leave a one-input context whose outputs are a fresh uniform context's"""
    cfg = graph.default_config(48000)
    nodes = graph.graph_shift_master()
    mixed = [(44100, abi.FMT_I16, 2), (96000, abi.FMT_F32, 1), (8000, abi.FMT_U8, 2)]
    one = (44100, abi.FMT_I24, 2)
    raw = synth.batch_pcm(3, 800, one[0], channels=one[2], fmt=one[1])
    fresh = icw.Context(copy_cfg(cfg, sample_rate=one[0], in_format=one[1], in_channels=one[2]), nodes, 3)
    want, want_pre = fresh.process(raw, 800, want_pre=True)
    fresh.close()
    for how in ("set_input", "set_stream_input", "stream by stream"):
        ctx = icw.Context(copy_cfg(cfg), nodes, 3)
        for s, (rate, fmt, ch) in enumerate(mixed):
            ctx.set_stream_input(rate, fmt, ch, s, 1)
        assert ctx.stream_input_count() == 3
        if how == "set_input":
            ctx.set_input(*one)
        elif how == "set_stream_input":
            ctx.set_stream_input(*one)
        else:
            for s in range(3):
                ctx.set_stream_input(*one, first=s, count=1)
        assert ctx.stream_input_count() == 1, how
        got, got_pre = ctx.process(raw, 800, want_pre=True)
        assert np.array_equal(bits(got_pre), bits(want_pre)) and np.array_equal(got, want), how
        ctx.close()


def test_refusals_change_nothing(icw, oracle):
    cfg = graph.default_config(48000)
    nodes = graph.graph_shift_master()
    inputs = [(44100, abi.FMT_I16, 2), (96000, abi.FMT_F32, 1)]
    rig = StreamRig(icw, oracle, cfg, 3000, inputs=inputs, nodes=nodes)
    ctx, lib = rig.ctx, rig.ctx._lib

    def still_the_same(what):
        assert ctx.stream_input_count() == 2, what
        rig.step(250, what=what)

    # a CWAVE format
    for fmt in (abi.FMT_CW_F64, abi.FMT_CW_I16, abi.FMT_CW_I16_F32, abi.FMT_CW_F32):
        assert lib.icw_set_stream_input(ctx.h, 0, 1, 48000, fmt, 2) == abi.EUNSUPPORTED
    still_the_same("CWAVE format")
    # while the count is above 1: the FIR converter, the encoders, the input debug hook
    assert lib.icw_set_fir_hilbert(ctx.h, 64, 8.0) == abi.EUNSUPPORTED
    still_the_same("set_fir_hilbert")
    n = 64
    rows = rig.rows(n, 0, 2)
    enc = np.zeros((2, n * 32), np.uint8)
    for fn in (lib.icw_encode_cwave, lib.icw_encode_cwave_iir):
        assert fn(ctx.h, 0, 2, rows.ctypes.data, rows.strides[0], enc.ctypes.data, enc.strides[0], n, abi.FMT_CW_F64, 0,
                  None) == abi.EUNSUPPORTED
    still_the_same("encoders")
    out = np.zeros((2, n * 4), np.uint8)
    x = np.zeros((2, n, 2))
    assert lib.icw_process_streams(ctx.h, 0, 2, rows.ctypes.data, rows.strides[0], out.ctypes.data, out.strides[0], n,
                                   abi.F_DEBUG_INPUT, x.ctypes.data, None) == abi.EUNSUPPORTED
    still_the_same("ICW_F_DEBUG_INPUT")
    # bad arguments
    for first, count in ((-1, 1), (0, 0), (1, 2), (2, 1), (0, 3)):
        assert lib.icw_set_stream_input(ctx.h, first, count, 48000, abi.FMT_I16, 2) == abi.EINVAL
    for rate, fmt, ch in ((0, abi.FMT_I16, 2), (abi.MAX_FS_SRC + 1, abi.FMT_I16, 2), (48000, abi.FMT_I16, 0), (48000, 9, 2)):
        assert lib.icw_set_stream_input(ctx.h, 0, 1, rate, fmt, ch) == abi.EINVAL
    still_the_same("bad arguments")
    # a stride that holds the narrow stream's frames (4 bytes) but not the widest's... here both are 4
    # bytes wide, so make stream 1 the wide one first: 8 bytes per frame
    rig.set_input(1, 96000, abi.FMT_F32, 2)
    rig.raw[1] = synth.stream_pcm(1, 3000, 96000, channels=2, fmt=abi.FMT_F32)
    rows = rig.rows(n, 0, 2)
    assert rows.shape[1] == n * 8
    assert lib.icw_process_streams(ctx.h, 0, 2, rows.ctypes.data, n * 8 - 1, out.ctypes.data, out.strides[0], n, 0, None,
                                   None) == abi.EINVAL
    assert lib.icw_process_streams(ctx.h, 0, 2, rows.ctypes.data, n * 4, out.ctypes.data, out.strides[0], n, 0, None,
                                   None) == abi.EINVAL
    still_the_same("in_stride too small for the widest stream")
    rig.check("refusals")
    rig.close()

    # a context whose input is CWAVE
    ctx = icw.Context(copy_cfg(cfg, in_format=abi.FMT_CW_F64), nodes, 2)
    assert ctx._lib.icw_set_stream_input(ctx.h, 0, 1, 48000, abi.FMT_I16, 2) == abi.EUNSUPPORTED
    assert ctx.stream_input_count() == 1
    raw = synth.batch_pcm(2, 300, 48000, fmt=abi.FMT_CW_F64)
    sts = [oracle.Stream(copy_cfg(cfg, in_format=abi.FMT_CW_F64), nodes) for _ in range(2)]
    got, pre = ctx.process(raw, 300, want_pre=True)
    for s in range(2):
        ro, rp = sts[s].process(raw[s], 300, want_pre=True)
        assert np.array_equal(bits(pre[s]), bits(rp)) and np.array_equal(got[s], ro)
    ctx.close()

    # the FIR converter on
    ctx = icw.Context(copy_cfg(cfg), nodes, 2)
    ctx.set_fir_hilbert(64, 8.0)
    assert ctx._lib.icw_set_stream_input(ctx.h, 0, 1, 44100, abi.FMT_I16, 2) == abi.EUNSUPPORTED
    assert ctx.stream_input_count() == 1
    raw = synth.batch_pcm(2, 300, 48000)
    got, pre = ctx.process(raw, 300, want_pre=True)
    for s in range(2):
        st = oracle.Stream(copy_cfg(cfg), nodes)
        st.set_fir(64, 8.0)
        ro, rp = st.process(raw[s], 300, want_pre=True)
        assert np.array_equal(bits(pre[s]), bits(rp)) and np.array_equal(got[s], ro)
    ctx.close()


def test_list_edits_between_calls(icw, oracle):
    """a one-list context with per-stream inputs: live list edits between calls over the same range take
    effect from the next call -- Master to Shift + Master (the rotation code comes in), a chain to a
    register-file list, more rotation channels (the slab pitch grows), register form to bus form and
    back, and the list primitives"""
    cfg = graph.default_config(48000)
    inputs = [(44100, abi.FMT_I16, 2), (96000, abi.FMT_F32, 1), (44100, abi.FMT_I16, 2), (96000, abi.FMT_F32, 1)]
    rig = StreamRig(icw, oracle, cfg, 3000, inputs=inputs, nodes=graph.graph_master_only())
    assert rig.ctx.stream_input_count() == 2 and rig.ctx.stream_graph_count() == 1
    rig.step(300, what="master only")
    no_chain = [graph.master(inputs=("A", "B")), graph.shift(inputs=("in",), out="A", fr=3.0), graph.mix(inputs=("in",), out="B")]
    assert icw.graph_form(cfg, no_chain) == 0
    edits = [("shift + master", graph.graph_shift_master()), ("register file", no_chain),
             ("pm + shift", graph.graph_pm_shift_mix()), ("bus form", graph.graph_feedback_pm_shift()),
             ("register form again", graph.graph_shift_master()), ("master only again", graph.graph_master_only())]
    assert icw.graph_form(cfg, edits[3][1]) == 1
    for what, nodes in edits:
        assert rig.ctx.set_graph(nodes)
        for st in rig.sts:
            assert st.set_graph(nodes)
        rig.step(300, what=what)
    extra = graph.shift(inputs=("in",), out="Q", fr=-1.5)
    assert rig.ctx.graph_add_last(extra)
    for st in rig.sts:
        assert st.add_lastdsp(extra)
    rig.step(300, what="add_last")
    rig.ctx.graph_del_last()
    for st in rig.sts:
        st.del_lastdsp()
    rig.step(300, what="del_last")
    rig.check("list edits")
    rig.close()
