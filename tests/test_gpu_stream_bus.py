"""GPU: per-stream bus-form DSP lists in one context (icw_enable_stream_bus) against the oracle -- one
oracle.Stream per GPU stream, each with its own list: feedback loops, one-frame delays, lists of more than 16
nodes.  Every comparison is StreamRig's, bit for bit: pre-render doubles, rendered bytes, guard bytes, meters.
Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

from in_cwave_amd import abi, graph
from tests.streamrig import StreamRig, bits, copy_cfg, entry

pytestmark = pytest.mark.gpu


def feedback(gain):
    """graph_leaky_feedback with its own gain: C = gain * (in + C[t-1])"""
    return [graph.master(inputs=("C",)), graph.mix(inputs=("in", "C"), out="C", gain=gain)]


def loop_pm_shift(gain, fr):
    """graph_feedback_pm_shift with its own loop gain and Shift frequency"""
    return [graph.master(inputs=("in", "B")), graph.shift(inputs=("A",), out="B", fr=fr), graph.pm(inputs=("in", "B"), out="A", gain=gain)]


def bus_rig(icw, oracle, cfg, n_total, S, assign, nodes=None, **kw):
    """a rig of S streams on `nodes` (a register-form list) with the opt-in on, then every (first, count, list)
    of assign through icw_set_stream_graph and the oracle's set_graph"""
    rig = StreamRig(icw, oracle, cfg, n_total, S=S, nodes=nodes or graph.graph_master_only(), **kw)
    rig.ctx.enable_stream_bus()
    for first, count, nl in assign:
        rig.set_graph(first, nl, count)
    return rig


def test_two_streams_two_bus_lists(icw, oracle):
    cfg = graph.default_config(48000)
    assert icw.graph_form(cfg, graph.graph_leaky_feedback()) == 1 and icw.graph_form(cfg, graph.graph_feedback_pm_shift()) == 1
    rig = bus_rig(icw, oracle, cfg, 300, 2, [(0, 1, graph.graph_leaky_feedback()), (1, 1, graph.graph_feedback_pm_shift())])
    assert rig.ctx.stream_graph_count() == 2
    rig.step(300, what="two bus-form lists")
    rig.check("two bus-form lists")
    rig.close()


def test_wave_and_run_edges_and_subsets(icw, oracle, monkeypatch):
    """70 streams, 900 frames in four launch blocks (the bus goes through HBM between them): runs of 1 / 63 / 6
    streams over three lists, one of them bus form by its node count; subset calls inside one run, across two
    runs and over one stream; then every stream its own list -- 70 runs of one lane"""
    monkeypatch.setenv("ICW_BLOCK", "256")
    cfg = graph.default_config(48000)
    assert icw.graph_form(cfg, graph.graph_long_chain(24)) == 1
    rig = bus_rig(icw, oracle, cfg, 2400, 70, [(0, 1, graph.graph_leaky_feedback()), (1, 63, graph.graph_long_chain(24)),
                                               (64, 6, graph.graph_feedback_pm_shift())])
    assert rig.ctx.stream_graph_count() == 3
    rig.step(900, what="runs 1 / 63 / 6")
    rig.step(300, first=10, count=20, what="inside one run")
    rig.step(300, first=60, count=8, device=True, what="across two runs")
    rig.step(300, first=65, count=1, what="one stream")
    for s in range(70):
        rig.set_graph(s, feedback(0.25 + s / 256.0))
    assert rig.ctx.stream_graph_count() == 70
    rig.step(900, what="70 one-lane runs")
    rig.check("70 streams")
    rig.close()


@pytest.mark.parametrize("case", ["real_two_rates", "cw_f64"])
def test_per_stream_inputs_beside_it(icw, oracle, case):
    """PM and Shift inside the loop at each stream's own rate (44.1 k i16 and 96 k i24 in one call), and a
    CW_F64 context, where no K1 runs"""
    if case == "real_two_rates":
        cfg = graph.default_config(44100)
        inputs = [(44100, abi.FMT_I16, 2), (96000, abi.FMT_I24, 2), (44100, abi.FMT_I16, 1), (96000, abi.FMT_I24, 2)]
    else:
        cfg = graph.default_config(48000, fmt=abi.FMT_CW_F64)
        inputs = [None] * 4
    lists = [loop_pm_shift(0.25, 2.0), loop_pm_shift(0.25, 2.0), loop_pm_shift(0.3, 3.5), feedback(0.4)]
    rig = bus_rig(icw, oracle, cfg, 700, 4, [(s, 1, nl) for s, nl in enumerate(lists)], inputs=inputs)
    assert rig.ctx.stream_graph_count() == 3
    rig.step(450, what=case)
    rig.step(250, what=case)
    rig.check(case)
    rig.close()


@pytest.mark.parametrize("render", [entry(abi.RENDER_TPDF, abi.NSHAPE_MEW44, b24=True), entry(abi.RENDER_GAUSS, abi.NSHAPE_FLAT)],
                         ids=["tpdf_mew44_24", "gauss_flat_16"])
def test_dithered_serial_render_behind_it(icw, oracle, monkeypatch, render):
    """the context's one render, dithered, runs serial behind the mixed K4; two launch blocks"""
    monkeypatch.setenv("ICW_BLOCK", "256")
    r, b24 = render
    cfg = copy_cfg(graph.default_config(48000), need24bits=int(b24))
    cfg.render = r
    rig = bus_rig(icw, oracle, cfg, 800, 3, [(0, 1, feedback(0.5)), (1, 1, graph.graph_feedback_pm_shift()), (2, 1, feedback(0.3))])
    rig.step(400, what="dithered")
    rig.step(400, what="dithered")
    rig.check("dithered")
    rig.close()


def test_mixed_form_call(icw, oracle):
    """register-form and bus-form streams alternate in one call (every stream runs in bus form); a 576-frame
    call of a register-form stream alone takes its usual path (K5 on the row recurrence); then the whole range
    again: the persistent bus is the same whichever form wrote it"""
    cfg = graph.default_config(48000)
    # stream 2's list keeps slot B on the bus and reads it, so a difference between the forms' write-backs shows
    keep = [graph.master(inputs=("C",)), graph.mix(inputs=("in", "B"), out="C"), graph.shift(inputs=("in",), out="B")]
    lists = [graph.graph_shift_master(), graph.graph_leaky_feedback(), graph.graph_pm_shift_mix(), graph.graph_feedback_pm_shift(), keep]
    rig = bus_rig(icw, oracle, cfg, 1800, 5, [(s, 1, nl) for s, nl in enumerate(lists)])
    assert [icw.graph_form(cfg, nl) for nl in lists] == [0, 1, 0, 1, 0]
    rig.step(300, what="both forms")
    rig.step(576, first=0, count=1, what="register form alone")
    assert rig.ctx.last_k1_kernel() == abi.K1_ROW
    rig.step(300, first=2, count=1, what="register form alone, stream 2")
    rig.step(300, what="both forms again")
    rig.step(300, first=4, count=1, what="register form after the bus-form call")
    # the register-form streams alone in one call: their usual kernels, per-stream lists
    rig.ctx.set_stream_graph(graph.graph_shift_master(), 1, 1)
    assert rig.sts[1].set_graph(graph.graph_shift_master())
    rig.step(300, first=0, count=3, what="register-form streams together")
    rig.check("both forms")
    rig.close()


def test_live_edits_per_stream(icw, oracle):
    """register form -> bus form -> a register-form list reading a slot, per stream, with an
    icw_clear_stream_bus_slot in between; icw_set_graph with a bus-form list on a mixed table gives count 1"""
    cfg = graph.default_config(48000)
    reg1 = [graph.master(inputs=("C",)), graph.mix(inputs=("in", "B"), out="C"), graph.shift(inputs=("in",), out="B")]
    bus = [graph.master(inputs=("C",)), graph.mix(inputs=("in", "C"), out="C", gain=0.5), graph.shift(inputs=("in",), out="B", fr=3.0)]
    reg2 = [graph.master(inputs=("in", "B", "C")), graph.mix(inputs=("in",), out="C"), graph.shift(inputs=("in",), out="B", fr=1.5)]
    assert [icw.graph_form(cfg, nl) for nl in (reg1, bus, reg2)] == [0, 1, 0]
    rig = bus_rig(icw, oracle, cfg, 2400, 3, [(0, 3, reg1)], nodes=reg1)
    ctx = rig.ctx
    rig.step(300, what="register form")
    rig.set_graph(1, bus)
    assert ctx.stream_graph_count() == 2
    rig.step(300, what="stream 1 in bus form")
    Cs = graph.slot("C")
    ctx.clear_stream_bus_slot(Cs, 1, 1)
    rig.sts[1].clear_bus_slot(Cs)
    blob = abi.StateBlob.from_buffer_copy(ctx.get_state(1))
    assert [blob.bus[Cs][k] for k in range(4)] == [0.0] * 4
    rig.step(300, what="slot C of stream 1 cleared")
    rig.set_graph(1, reg2)
    rig.set_graph(2, bus)
    rig.step(300, what="stream 1 back in register form, stream 2 in bus form")
    assert ctx.stream_graph_count() == 3
    assert ctx.set_graph(graph.graph_feedback_pm_shift())
    for st in rig.sts:
        assert st.set_graph(graph.graph_feedback_pm_shift())
    assert ctx.stream_graph_count() == 1
    rig.step(300, what="collapsed to one bus-form list")
    ctx.graph_del_last()                              # one list again: the primitives work on it
    for st in rig.sts:
        st.del_lastdsp()
    rig.step(300, what="del_last after the collapse")
    rig.check("live edits")
    rig.close()


def test_state_round_trip(icw, oracle):
    """get_state from a bus-form stream of a mixed context, set_state into another context where that stream
    carries the same list: the continuation equals an uninterrupted run"""
    cfg = graph.default_config(48000)
    lists = [graph.graph_shift_master(), graph.graph_leaky_feedback(), graph.graph_feedback_pm_shift()]
    rig = bus_rig(icw, oracle, cfg, 1000, 3, [(s, 1, nl) for s, nl in enumerate(lists)])
    rig.step(600, what="before the checkpoint")
    blob = rig.ctx.get_state(2)
    rig.close()
    other = bus_rig(icw, oracle, cfg, 1000, 2, [(0, 1, lists[2]), (1, 1, lists[1])]).ctx
    other.set_state(0, blob)
    raw = rig.frames(2, 400)
    out, pre = other.process(raw[None, :], 400, first=0, count=1, want_pre=True)
    ro, rp = rig.sts[2].process(raw, 400, want_pre=True)
    assert np.array_equal(bits(pre[0]), bits(rp)) and np.array_equal(out[0], ro)
    other.close()


def test_refusals_change_nothing(icw, oracle):
    cfg = graph.default_config(48000)
    arr = lambda nodes: graph.node_array(nodes)

    # without the opt-in a fresh context refuses exactly as before
    rig = StreamRig(icw, oracle, cfg, 600, nodes=graph.graph_master_only(), lists=[graph.graph_shift_master(), graph.graph_pm_shift_mix()])
    ctx, lib = rig.ctx, rig.ctx._lib
    acc = C.c_int(-1)
    assert lib.icw_set_stream_graph(ctx.h, 0, 1, arr(graph.graph_leaky_feedback()), 2, 0, C.byref(acc)) == abi.EUNSUPPORTED
    assert acc.value == 1
    assert lib.icw_set_graph(ctx.h, arr(graph.graph_leaky_feedback()), 2, 0, None) == abi.EUNSUPPORTED
    assert ctx.stream_graph_count() == 2
    rig.step(300, what="no opt-in")
    # the opt-in goes on and off again freely while no bus-form entry stands beside others
    assert lib.icw_enable_stream_bus(ctx.h, 1) == abi.OK and lib.icw_enable_stream_bus(ctx.h, 0) == abi.OK
    assert lib.icw_set_stream_graph(ctx.h, 0, 1, arr(graph.graph_leaky_feedback()), 2, 0, None) == abi.EUNSUPPORTED
    rig.step(300, what="opt-in off again")
    rig.close()
    rig = StreamRig(icw, oracle, cfg, 300, S=2, nodes=graph.graph_leaky_feedback())
    assert rig.ctx._lib.icw_set_stream_graph(rig.ctx.h, 0, 1, arr(graph.graph_master_only()), 1, 0, None) == abi.EUNSUPPORTED
    rig.step(300, what="bus-form list in force, no opt-in")
    rig.close()

    # with the opt-in, a bus-form entry beside another one
    rig = bus_rig(icw, oracle, cfg, 2100, 3, [(1, 1, graph.graph_leaky_feedback()), (2, 1, graph.graph_shift_master())])
    ctx, lib = rig.ctx, rig.ctx._lib

    def still_the_same(what):
        assert (ctx.stream_graph_count(), ctx.stream_render_count(), ctx.stream_hilbert_count(), ctx.stream_input_count()) == (3, 1, 1, 1), what
        rig.step(300, what=what)

    r, b24 = entry(abi.RENDER_TPDF, abi.NSHAPE_MEW44, b24=True)
    assert lib.icw_set_stream_render(ctx.h, 0, 1, C.byref(r), int(b24)) == abi.EUNSUPPORTED
    still_the_same("a second render")
    assert lib.icw_set_stream_hilbert(ctx.h, 0, 1, 4, 1, 1) == abi.EUNSUPPORTED
    still_the_same("a second converter")
    assert lib.icw_set_fir_hilbert(ctx.h, 64, 8.0) == abi.EUNSUPPORTED
    still_the_same("the FIR converter")
    extra = graph.mix(inputs=("in",), out="Q")
    assert lib.icw_graph_del_last(ctx.h) == abi.EUNSUPPORTED
    assert lib.icw_graph_del_all(ctx.h) == abi.EUNSUPPORTED
    assert lib.icw_graph_add_last(ctx.h, C.byref(extra)) == abi.EUNSUPPORTED
    assert lib.icw_graph_set_output_plug(ctx.h, 1, 5) == abi.EUNSUPPORTED
    still_the_same("the list primitives")
    assert lib.icw_enable_stream_bus(ctx.h, 0) == abi.EUNSUPPORTED
    still_the_same("the opt-in off")
    rig.check("refusals")
    rig.close()

    # a bus-form list on the call that would put it beside several renders / converters
    rig = bus_rig(icw, oracle, cfg, 600, 2, [])
    ctx, lib = rig.ctx, rig.ctx._lib
    rig.set_render(1, (r, b24))
    assert lib.icw_set_stream_graph(ctx.h, 0, 1, arr(graph.graph_leaky_feedback()), 2, 0, None) == abi.EUNSUPPORTED
    assert (ctx.stream_graph_count(), ctx.stream_render_count()) == (1, 2)
    rig.step(300, what="bus-form list beside two renders")
    rig.close()

    # an FP_CHECK context takes no bus-form list beside another
    rig = bus_rig(icw, oracle, copy_cfg(cfg, fp_check=1), 300, 2, [])
    assert rig.ctx._lib.icw_set_stream_graph(rig.ctx.h, 0, 1, arr(graph.graph_leaky_feedback()), 2, 0, None) == abi.EUNSUPPORTED
    assert rig.ctx.stream_graph_count() == 1
    rig.step(300, what="fp_check")
    rig.check("fp_check", census=True)
    rig.close()
