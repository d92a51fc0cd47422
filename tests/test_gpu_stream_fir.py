"""GPU: per-stream DSP lists and per-stream inputs with the FIR Hilbert converter on (icw_set_fir_hilbert
beside icw_set_stream_graph / icw_set_stream_input) against the oracle -- one oracle.Stream per GPU
stream, each with its own list, rate, sample format and channels, and the converter set on it.  Every
comparison is bit for bit: rendered bytes, pre-render doubles where asked, clips, peaks and the frame
counter.  Nothing here has a tolerance.

Frame counts follow the converter's tiles: a stereo KF2 tile is 1 024 frames, a mono one 2 048, and the
signature form (icw_fir_sig) takes the tiles before the last -- so a 2 500-frame call without pre-render
doubles runs two signature tiles and a generic one for stereo streams, one and one for mono streams; the
calls of 577 and 1 frames after it carry the FIR history across calls."""

import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth
from in_cwave_amd import lib as L

from tests.streamrig import StreamRig, copy_cfg, shift_list

from test_gpu_stream_input import INPUTS10

pytestmark = pytest.mark.gpu

BETA = 8.0
CALLS = (2500, 577, 1)


@pytest.fixture(autouse=True, params=["fused", "split"])
def fir_form(request, monkeypatch):
    """KF2 (converter, graph and render in one kernel) and KF + K2 (ICW_FIR_FUSED=0)"""
    monkeypatch.setenv("ICW_FIR_FUSED", "1" if request.param == "fused" else "0")
    return request.param


class FirRig(StreamRig):
    """the rig with the converter on: stream s has inputs[s] and runs lists[s]
    (bypass[s]); fir_first: icw_set_fir_hilbert before the per-stream setters, else after them"""

    def __init__(self, icw, oracle, cfg, inputs, lists, n_total, order, fir_first=False, bypass=None):
        S = len(inputs)
        self.ctx = icw.Context(copy_cfg(cfg), lists[0], S)
        self.ctx.enable_stream_fir()
        self.order = order
        if fir_first:
            self.ctx.set_fir_hilbert(order, BETA)
        self.sts = []
        for s in range(S):
            byp = bypass[s] if bypass else cfg.bypass_list
            if lists[s] is not lists[0] or byp != cfg.bypass_list:
                assert self.ctx.set_stream_graph(lists[s], s, 1, byp)
            st = oracle.Stream(copy_cfg(cfg), lists[s])
            if byp != cfg.bypass_list:
                st.set_graph(lists[s], byp)
            st.set_fir(order, BETA)
            self.sts.append(st)
        self.inputs, self.cur = [None] * S, [None] * S
        for s, (rate, fmt, ch) in enumerate(inputs):
            self.set_input(s, rate, fmt, ch)
        if not fir_first:
            self.ctx.set_fir_hilbert(order, BETA)
        self.raw = [synth.stream_pcm(s, n_total, rate, channels=ch, fmt=fmt) for s, (rate, fmt, ch) in enumerate(inputs)]
        self.osz = [2 * self.ctx.render_size] * S
        self.t, self.pad = [0] * S, 0

    def run(self, n, **kw):
        """a call without pre-render doubles (the signature form's condition): rendered bytes only"""
        self.step(n, want_pre=False, **kw)

    def go(self, n, pre, **kw):
        (self.step if pre else self.run)(n, **kw)


def master_only(gl, gr):
    m = graph.master(inputs=("in",))
    m.gain[0], m.gain[1] = gl, gr
    return [m]


@pytest.mark.parametrize("order", [30, 254])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("pre", [False, True], ids=["bytes", "pre"])
def test_matrix(icw, oracle, order, device, pre):
    """ten streams, five formats x mono / stereo at five rates, one Shift + Master list"""
    cfg = graph.default_config(48000)
    rig = FirRig(icw, oracle, cfg, INPUTS10, [graph.graph_shift_master()] * 10, sum(CALLS), order)
    assert rig.ctx.stream_input_count() == 10 and rig.ctx.stream_graph_count() == 1
    for n in CALLS:
        rig.go(n, pre, device=device, what="matrix")
    rig.check("matrix")
    rig.close()


@pytest.mark.parametrize("order", [30, 254])
@pytest.mark.parametrize("pre", [False, True], ids=["bytes", "pre"])
def test_lists(icw, oracle, order, pre):
    """eight stereo i16 streams at one rate, each its own Shift frequency: one signature, eight lists.
    Then one stream more with PM -> Shift -> Mix -> Master (the class leaves the signature form) and
    a bypassed list"""
    cfg = graph.default_config(48000)
    inputs = [(48000, abi.FMT_I16, 2)] * 8
    lists = [shift_list(1.0 + 0.75 * s) for s in range(8)]
    rig = FirRig(icw, oracle, cfg, inputs, lists, sum(CALLS), order, fir_first=True)
    assert rig.ctx.stream_graph_count() == 8 and rig.ctx.stream_input_count() == 1
    for n in CALLS:
        rig.go(n, pre, what="eight shifts")
    rig.check("eight shifts")
    rig.close()
    lists9 = lists + [graph.graph_pm_shift_mix()]
    bypass = [0] * 9
    bypass[3] = 1
    rig = FirRig(icw, oracle, cfg, inputs + [(48000, abi.FMT_I16, 2)], lists9, sum(CALLS), order, bypass=bypass)
    assert rig.ctx.stream_graph_count() == 9
    for n in CALLS:
        rig.go(n, pre, what="nine lists")
    rig.check("nine lists")
    rig.close()


@pytest.mark.parametrize("out_of_step", [False, True], ids=["in_step", "one_reset"])
def test_slabs(icw, oracle, out_of_step):
    """(list A, 44 100), (list A, 48 000), (list B, 48 000), two streams each; with one stream's counter
    reset mid-run its factors are computed inline beside the others' table factors in one launch"""
    cfg = graph.default_config(48000)
    a, b = shift_list(2.0), shift_list(3.5)
    inputs = [(44100, abi.FMT_I16, 2)] * 2 + [(48000, abi.FMT_I16, 2)] * 4
    rig = FirRig(icw, oracle, cfg, inputs, [a, a, a, a, b, b], 2 * sum(CALLS), 254)
    assert rig.ctx.stream_input_count() == 2 and rig.ctx.stream_graph_count() == 2
    for n in CALLS:
        rig.run(n, what="slabs")
    if out_of_step:
        rig.ctx.stream_reset_framecnt(3)
        rig.sts[3].set_n_frame(0)
    for n in CALLS:
        rig.run(n, what="slabs, second pass")
    rig.check("slabs")
    rig.close()


@pytest.mark.parametrize("need24", [False, True], ids=["16bit", "24bit"])
def test_mono_stereo_lr_same(icw, oracle, need24):
    """mono streams with equal-gain Masters (one computation for both channels) beside one with unequal
    gains (the class drops lr_same), plus stereo streams, in one call"""
    cfg = graph.default_config(48000, need24bits=need24)
    inputs = [(48000, abi.FMT_I16, 1), (44100, abi.FMT_F32, 1), (96000, abi.FMT_I24, 1), (48000, abi.FMT_I16, 2),
              (44100, abi.FMT_I32, 2)]
    lists = [master_only(0.5, 0.5), master_only(0.25, 0.25), master_only(0.5, 0.5), master_only(0.5, 0.5), master_only(0.7, 0.3)]
    rig = FirRig(icw, oracle, cfg, inputs, lists, sum(CALLS), 30)
    for n in CALLS:
        rig.run(n, what="lr_same")
    rig.check("lr_same")
    rig.close()
    lists[1] = master_only(0.5, 0.25)
    rig = FirRig(icw, oracle, cfg, inputs, lists, sum(CALLS), 30)
    for n in CALLS:
        rig.run(n, what="unequal gains")
    rig.check("unequal gains")
    rig.close()


def test_sub_ranges(icw, oracle, monkeypatch):
    """calls over [first, first + count) with several launch blocks per call: a range whose streams share
    one list and input (a one-list call's launches), a range that mixes; the others keep their history"""
    monkeypatch.setenv("ICW_BLOCK", "263")
    cfg = graph.default_config(48000)
    a, b = shift_list(2.0), shift_list(-3.25)
    inputs = [(48000, abi.FMT_I16, 2)] * 3 + [(44100, abi.FMT_I24, 1), (96000, abi.FMT_F32, 2), (44100, abi.FMT_I24, 1)]
    rig = FirRig(icw, oracle, cfg, inputs, [a, a, a, a, b, b], 3000, 254)
    rig.step(700, what="all")
    # streams 0-2: one entry; the oracles of 3-5 are not advanced, and neither is their history
    rig.step(900, first=0, count=3, what="shared range")
    rig.step(900, first=3, count=3, what="mixing range")
    rig.run(1100, what="all again")
    rig.check("sub-ranges")
    rig.close()


@pytest.mark.parametrize("shaper", ["flat", "mew44"])
def test_renders(icw, oracle, shaper):
    """TPDF + flat shaper (frame-parallel in KF2, K3a's dither rows) and TPDF + MEW44 at 24 bit (the serial
    render after KF2) over mixed inputs and lists"""
    cfg = graph.default_config(48000, need24bits=shaper == "mew44")
    cfg.render.render_type = abi.RENDER_TPDF
    if shaper == "mew44":
        cfg.render.nshape_type = abi.NSHAPE_MEW44
    inputs = [(48000, abi.FMT_I16, 2), (44100, abi.FMT_F32, 1), (96000, abi.FMT_I24, 2), (44100, abi.FMT_U8, 1)]
    lists = [shift_list(2.0), shift_list(2.0), master_only(0.5, 0.5), shift_list(5.0)]
    rig = FirRig(icw, oracle, cfg, inputs, lists, sum(CALLS), 254)
    for n in CALLS:
        rig.run(n, what=shaper)
    rig.check(shaper)
    rig.close()


def test_setter_order(icw, oracle):
    """the converter off and on again mid-run with lists and inputs in force; then icw_set_graph and
    icw_set_input collapse both counts, and the next call is a one-list context's"""
    cfg = graph.default_config(48000)
    inputs = [(48000, abi.FMT_I16, 2), (44100, abi.FMT_I16, 2), (48000, abi.FMT_F32, 1), (48000, abi.FMT_I16, 2)]
    lists = [shift_list(2.0), shift_list(3.0), shift_list(2.0), shift_list(4.5)]
    rig = FirRig(icw, oracle, cfg, inputs, lists, 6000, 30, fir_first=True)
    rig.run(1500, what="on")
    rig.ctx.set_fir_hilbert(0, BETA)
    for st in rig.sts:
        st.set_fir(0, BETA)
    assert rig.ctx.stream_graph_count() == 3 and rig.ctx.stream_input_count() == 3
    rig.step(700, what="off")
    rig.ctx.set_fir_hilbert(254, BETA)
    for st in rig.sts:
        st.set_fir(254, BETA)
    rig.run(1500, what="on again")
    # collapse: one list, one input -- a fresh one-list context with the same state gives the same bytes
    one = shift_list(7.0)
    assert rig.ctx.set_graph(one)
    rig.ctx.set_input(48000, abi.FMT_I16, 2)
    for s, st in enumerate(rig.sts):
        st.set_graph(one, 0)
        st.set_input(48000, abi.FMT_I16, 2)
        rig.inputs[s] = (48000, abi.FMT_I16, 2)
        rig.raw[s] = synth.stream_pcm(s, 6000, 48000, channels=2, fmt=abi.FMT_I16)
    assert rig.ctx.stream_graph_count() == 1 and rig.ctx.stream_input_count() == 1
    rig.run(2300, what="collapsed")
    rig.check("setter order")
    rig.close()


def test_still_refused(icw, oracle):
    """a bus-form list per stream, a CWAVE format per stream and icw_encode_cwave over differing inputs are
    refused as before, and change nothing"""
    cfg = graph.default_config(48000)
    inputs = [(48000, abi.FMT_I16, 2), (44100, abi.FMT_I16, 2)]
    rig = FirRig(icw, oracle, cfg, inputs, [shift_list(2.0), shift_list(3.0)], 2000, 30)
    rig.run(600, what="before")
    ctx = rig.ctx
    with pytest.raises(L.IcwError):
        ctx.set_stream_graph(graph.graph_leaky_feedback(), 1, 1)
    with pytest.raises(L.IcwError):
        ctx.set_stream_input(48000, abi.FMT_CW_F64, 2, 1, 1)
    rows = rig.rows(100, 0, 2)
    out = np.zeros((2, 100 * 32), np.uint8)
    rc = ctx._lib.icw_encode_cwave(ctx.h, 0, 2, rows.ctypes.data, rows.strides[0], out.ctypes.data, out.strides[0], 100,
                                   abi.FMT_CW_F64, 0, None)
    assert rc == abi.EUNSUPPORTED and not out.any()
    assert ctx.stream_graph_count() == 2 and ctx.stream_input_count() == 2
    rig.run(900, what="after")
    rig.check("refusals")
    rig.close()


def test_off_by_default(icw, oracle):
    """a context that never called icw_enable_stream_fir keeps the old refusals; one that did cannot turn it
    off while the converter runs beside differing lists"""
    cfg = graph.default_config(48000)
    ctx = icw.Context(copy_cfg(cfg), shift_list(2.0), 2)
    ctx.set_fir_hilbert(30, BETA)
    with pytest.raises(L.IcwError):
        ctx.set_stream_graph(shift_list(3.0), 1, 1)
    with pytest.raises(L.IcwError):
        ctx.set_stream_input(44100, abi.FMT_I16, 2, 1, 1)
    ctx.enable_stream_fir()
    assert ctx.set_stream_graph(shift_list(3.0), 1, 1)
    assert ctx._lib.icw_enable_stream_fir(ctx.h, 0) == abi.EUNSUPPORTED
    ctx.set_fir_hilbert(0, BETA)
    ctx.enable_stream_fir(False)
    with pytest.raises(L.IcwError):
        ctx.set_fir_hilbert(30, BETA)
    assert ctx.stream_graph_count() == 2
    ctx.close()


def test_state_blob(icw, oracle):
    """one stream of a mixed context: its blob taken mid-run and put back replays the same bytes"""
    cfg = graph.default_config(48000)
    inputs = [(48000, abi.FMT_I16, 2), (44100, abi.FMT_F32, 1), (96000, abi.FMT_I24, 2)]
    rig = FirRig(icw, oracle, cfg, inputs, [shift_list(2.0), shift_list(3.0), shift_list(2.0)], 3000, 254)
    rig.run(1300, what="before")
    blob = rig.ctx.get_state(1)
    rows = rig.rows(900, 1, 1)
    first, _ = rig.ctx.process(rows, 900, first=1, count=1)
    first = first.copy()
    rig.ctx.set_state(1, blob)
    again, _ = rig.ctx.process(rows, 900, first=1, count=1)
    assert np.array_equal(first, again)
    f = rig.fsz(1)
    ro, _ = rig.sts[1].process(rig.raw[1][1300 * f:2200 * f], 900)
    assert np.array_equal(again[0], ro)
    rig.close()
