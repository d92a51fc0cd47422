"""GPU: per-stream Hilbert converters in one context (icw_set_stream_hilbert, icw_stream_hilbert_count)
against the oracle -- one oracle.Stream per GPU stream, each with its own hilbert_type, iir_kahan and
iir_subnorm_reject, edited with set_hilbert_filter / set_hilbert_config where a case edits.  Every comparison
is bit for bit: rendered bytes, pre-render doubles, clips, peak dB bits, de-subnorm counts and the frame
counter.  Nothing here has a tolerance."""

import ctypes as C

import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth
from tests.streamrig import StreamRig, bits, copy_cfg, entry

pytestmark = pytest.mark.gpu

FS = 48000
ORDER = {0: 15, 1: 19, 2: 18, 3: 19, 4: 20, 5: 20}      # the canned filters' orders by type
KR = (1, 1)                                             # Kahan + reject: what the row form runs
# three calls on one context: odd, >= 3 N and a remainder for every N; below every N; the first again
CALLS = (1003, 7, 1003)


def by_runs(runs):
    """[(streams, (type, kahan, reject)), ...] -> one setting per stream"""
    return [e for n, e in runs for _ in range(n)]


# runs of 3 / 1 / 5 / 2 streams, orders 15 / 20 / 18 / 19: none a multiple of the 2 streams a wave pair holds
ROW_RUNS = [(3, (0,) + KR), (1, (4,) + KR), (5, (2,) + KR), (2, (1,) + KR)]


def row_every_order(icw, oracle, device, what):
    cfg = graph.default_config(FS)
    # stream 1 is silent and shares its waves with stream 0: every sum is rejected, the speculative blocks
    # hand over to the exact ones
    rig = StreamRig(icw, oracle, cfg, sum(CALLS), settings=by_runs(ROW_RUNS), silent=(1,))
    assert rig.ctx.stream_hilbert_count() == 4
    for n in CALLS:
        rig.step(n, device=device, what=what)
        assert rig.ctx.last_k1_kernel() == abi.K1_ROW, what
    rig.check(what)
    assert rig.sts[1].meters()["desubnorm"] > 0
    rig.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("block", [None, "256"], ids=["one block", "ICW_BLOCK=256"])
def test_row_form_every_order(icw, oracle, monkeypatch, device, block):
    """11 stereo streams, the four orders in one row-form launch, three calls; with 256-frame launch blocks
    each long call spans 4 blocks and both scratch sets"""
    if block:
        monkeypatch.setenv("ICW_BLOCK", block)
    row_every_order(icw, oracle, device, f"row form, block {block}")


# 70 streams in runs of 33 / 1 / 31 / 5: across the 32-stream lane-group boundary; every summation and reject
LANE_RUNS = [(33, (3, 0, 1)), (1, (5, 1, 0)), (31, (0, 1, 1)), (5, (4, 0, 0))]


def test_lane_form(icw, oracle, monkeypatch):
    monkeypatch.setenv("ICW_K1_MODE", "plain")
    cfg = graph.default_config(FS)
    rig = StreamRig(icw, oracle, cfg, sum(CALLS), settings=by_runs(LANE_RUNS))
    assert rig.ctx.stream_hilbert_count() == 4
    for n in CALLS:
        rig.step(n, what="lane form")
        assert rig.ctx.last_k1_kernel() == abi.K1_LANE
    rig.check("lane form")
    rig.close()


def test_auto_takes_the_lane_form_without_kahan_and_reject(icw, oracle):
    """automatic mode, one entry of the call baseline: a batch this small would take the row form"""
    cfg = graph.default_config(FS)
    rig = StreamRig(icw, oracle, cfg, 1400, settings=by_runs([(2, (1,) + KR), (3, (4, 0, 1)), (1, (0,) + KR)]))
    rig.step(1003, what="auto, one baseline entry")
    assert rig.ctx.last_k1_kernel() == abi.K1_LANE
    rig.step(397, first=0, count=2, what="auto, a Kahan + reject run alone")
    assert rig.ctx.last_k1_kernel() == abi.K1_ROW
    rig.check("auto")
    rig.close()


@pytest.mark.parametrize("form", ["row", "plain"])
def test_mono_dedup(icw, oracle, monkeypatch, form):
    """6 mono streams in runs of 1 / 3 / 2: the left chains only, in both forms"""
    monkeypatch.setenv("ICW_K1_MODE", form)
    cfg = graph.default_config(FS, channels=1)
    rig = StreamRig(icw, oracle, cfg, sum(CALLS), settings=by_runs([(1, (4,) + KR), (3, (0,) + KR), (2, (2,) + KR)]))
    for n in CALLS:
        rig.step(n, what=f"mono, {form}")
        assert rig.ctx.last_k1_kernel() == (abi.K1_ROW if form == "row" else abi.K1_LANE)
    rig.check(f"mono, {form}")
    rig.close()


def test_subset_and_one_stream_calls(icw, oracle, monkeypatch):
    """a subset across runs takes the mixed path; a subset inside one run and a one-stream call launch what a
    one-setting context with that entry launches -- the one-stream call is K5's case"""
    monkeypatch.setenv("ICW_K1_MODE", "row")
    monkeypatch.setenv("ICW_STREAM1", "1")
    cfg = graph.default_config(FS)
    rig = StreamRig(icw, oracle, cfg, 4000, settings=by_runs(ROW_RUNS))
    rig.step(300, what="whole batch")
    rig.step(301, first=2, count=5, what="[2, 7) across three runs")
    inside = rig.step(700, first=5, count=3, timing=True, what="inside the run of five")
    k1_in, (_, l_in) = rig.ctx.last_k1_kernel(), rig.ctx.last_timing()
    one = rig.step(576, first=3, count=1, timing=True, what="one stream, type 4")
    k1_one, (_, l_one) = rig.ctx.last_k1_kernel(), rig.ctx.last_timing()
    rig.step(333, what="whole batch again")
    rig.check("subsets")
    rig.close()
    # the same streams in one-setting contexts of their type: the same calls before, then the call
    for t, s, n, frames, (got, k1, launches) in ((2, 5, 3, 700, (inside, k1_in, l_in)), (4, 3, 1, 576, (one, k1_one, l_one))):
        ref = StreamRig(icw, oracle, copy_cfg(cfg, hilbert_type=t), 4000, settings=[None] * 11)
        assert ref.ctx.stream_hilbert_count() == 1
        ref.step(300, what="one-setting context")
        ref.step(301, first=2, count=5, what="one-setting context")
        want = ref.step(frames, first=s, count=n, timing=True, what="one-setting context")
        assert (ref.ctx.last_k1_kernel(), ref.ctx.last_timing()[1]) == (k1, launches)
        if n == 1:
            assert (k1, launches) == (abi.K1_ROW, (1, 1))
        assert np.array_equal(got, want)
        ref.close()


def test_count_one_is_todays_path(icw, oracle, monkeypatch):
    """one setting given to every stream through icw_set_stream_hilbert is a one-setting context: the bytes
    and the launch counts of a context set through icw_set_hilbert_filter + icw_set_hilbert_config"""
    monkeypatch.setenv("ICW_BLOCK", "256")
    cfg = graph.default_config(FS)
    e = (4, 0, 1)
    res = []
    for how in ("stream", "context", "stream by stream"):
        rig = StreamRig(icw, oracle, cfg, 1500, settings=[None] * 4)
        if how == "stream":
            rig.set_hilbert(0, e, count=4)
        elif how == "stream by stream":
            for s in (2, 0, 3, 1):
                rig.set_hilbert(s, e)
        else:
            rig.ctx.set_hilbert_filter(e[0])
            rig.ctx.set_hilbert_config(e[1], e[2])
            for s, st in enumerate(rig.sts):
                st.set_hilbert_filter(e[0])
                st.set_hilbert_config(e[1], e[2])
                rig.cur[s] = e
        assert rig.ctx.stream_hilbert_count() == 1, how
        out = rig.step(1100, timing=True, what=how)
        res.append((out, rig.ctx.last_timing()[1], rig.ctx.last_k1_kernel(), rig.ctx.last_dither_chunks()))
        rig.check(how)
        assert abi.StateBlob.from_buffer_copy(rig.ctx.get_state(1)).nord == 20
        rig.close()
    for out, launches, k1, chunks in res[1:]:
        assert np.array_equal(out, res[0][0]) and (launches, k1, chunks) == res[0][1:]
    assert res[0][1][0] > 1


def test_context_wide_setters_on_a_mixed_context(icw, oracle):
    """icw_set_hilbert_filter on a mixed context: the streams already at the type keep their rings, the others
    restart, every stream keeps its summation; icw_set_hilbert_config: every stream keeps type and rings, the
    counters restart"""
    cfg = graph.default_config(FS)
    settings = by_runs([(2, (0,) + KR), (2, (4, 0, 1)), (1, (2, 1, 0)), (1, (4,) + KR)])
    rig = StreamRig(icw, oracle, cfg, 3000, settings=settings, silent=(3,))
    rig.step(500, what="mixed")
    rig.ctx.set_hilbert_filter(4)
    for s, st in enumerate(rig.sts):
        st.set_hilbert_filter(4)
        rig.cur[s] = (4,) + rig.cur[s][1:]
    assert rig.ctx.stream_hilbert_count() == 3          # (4, K, R), (4, 0, 1), (4, 1, 0)
    rig.step(611, what="after icw_set_hilbert_filter")
    rig.check("after icw_set_hilbert_filter")
    assert rig.sts[3].meters()["desubnorm"] > 0         # a kept stream's counter went on
    rig.set_hilbert(0, (1,) + KR)
    rig.ctx.set_hilbert_config(1, 1)
    for s, st in enumerate(rig.sts):
        st.set_hilbert_config(1, 1)
        rig.cur[s] = (rig.cur[s][0],) + KR
    assert rig.ctx.stream_hilbert_count() == 2
    rig.step(450, what="after icw_set_hilbert_config")
    rig.check("after icw_set_hilbert_config")
    rig.ctx.set_hilbert_filter(1)
    for s, st in enumerate(rig.sts):
        st.set_hilbert_filter(1)
        rig.cur[s] = (1,) + KR
    assert rig.ctx.stream_hilbert_count() == 1
    rig.step(300, what="one setting again")
    rig.check("context-wide setters")
    rig.close()


def test_edits_between_calls(icw, oracle):
    """a range changes type mid-sequence: only those streams restart; a configuration-only change keeps the
    rings and restarts the counters; an unchanged setting restarts the counters all the same"""
    cfg = graph.default_config(FS)
    rig = StreamRig(icw, oracle, cfg, 3000, settings=[None] * 5, silent=(2,))
    rig.step(700, what="one setting")
    rig.set_hilbert(1, (2,) + KR, count=2)
    assert rig.ctx.stream_hilbert_count() == 2
    rig.step(650, what="streams 1, 2 at type 2")
    rig.check("after the type change")
    rig.set_hilbert(2, (2, 0, 1), count=2)                    # stream 2 keeps its rings, stream 3 restarts
    assert rig.ctx.stream_hilbert_count() == 3
    rig.step(333, what="configuration change")
    rig.set_hilbert(2, (2, 0, 1))                             # unchanged: the counters restart
    rig.step(500, what="the same setting again")
    rig.check("after the configuration change")
    rig.set_hilbert(1, (cfg.hilbert_type,) + KR, count=3)
    assert rig.ctx.stream_hilbert_count() == 1
    rig.step(200, what="one setting again")
    rig.check("edits")
    rig.close()


def test_with_per_stream_lists_inputs_and_renders(icw, oracle):
    """four streams that differ in input, list, render and converter in one context"""
    cfg = graph.default_config(FS)
    inputs = [(44100, abi.FMT_I16, 2), (48000, abi.FMT_I16, 2), (96000, abi.FMT_I24, 2), (48000, abi.FMT_F32, 2)]
    la = [graph.master(inputs=("A",), gain=0.9), graph.shift(inputs=("in",), out="A", fr=2.0)]
    lb = [graph.master(inputs=("A",), gain=0.8), graph.shift(inputs=("in",), out="A", fr=-3.5)]
    lists = [la, lb, lb, la]
    r16, r24s = entry(), entry(abi.RENDER_TPDF, abi.NSHAPE_MEW44, True)
    renders = [r16, r24s, r24s, r16]
    settings = [(0,) + KR, (4, 0, 1), (4, 0, 1), (2, 1, 0)]
    rig = StreamRig(icw, oracle, cfg, 1200, settings=settings, lists=lists, inputs=inputs, renders=renders)
    assert (rig.ctx.stream_hilbert_count(), rig.ctx.stream_graph_count(), rig.ctx.stream_input_count(),
            rig.ctx.stream_render_count()) == (3, 2, 4, 2)
    rig.step(700, what="combined")
    rig.step(500, device=True, what="combined, device pointers")
    rig.check("combined")
    rig.close()


def test_state_blob_round_trip(icw, oracle):
    """a type-4 stream's blob from a mixed context into another context's stream set to the same entry; the
    blob records the stream's own order, and a stream of another order refuses it"""
    cfg = graph.default_config(FS)
    a = StreamRig(icw, oracle, cfg, 2000, settings=by_runs([(2, (0,) + KR), (1, (4,) + KR), (1, (2,) + KR)]))
    a.step(700, what="source")
    blob = a.ctx.get_state(2)
    assert [abi.StateBlob.from_buffer_copy(a.ctx.get_state(s)).nord for s in range(4)] == [15, 15, 20, 18]
    b = StreamRig(icw, oracle, cfg, 2000, settings=[None, (4,) + KR, (1, 0, 1)])
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    for s in (0, 2):
        assert b.ctx._lib.icw_set_state(b.ctx.h, s, buf, len(blob)) == abi.EINVAL
    b.ctx.set_state(1, blob)
    # stream 1 of b goes on as stream 2 of a: a's oracle and signal
    b.sts[1], b.raw[1], b.t[1] = a.sts[2], a.raw[2], a.t[2]
    b.step(600, first=1, count=1, what="the restored stream alone")
    b.t[0] = b.t[2] = 0
    b.step(500, what="the restored stream in a mixed call")
    for s in (1,):
        m, r = b.ctx.meters(s), b.sts[s].meters()
        assert m["desubnorm"] == r["desubnorm"] and b.ctx.n_frame(s) == b.sts[s].n_frame()
    a.close()
    b.close()


def test_refusals_change_nothing(icw, oracle):
    cfg = graph.default_config(FS)
    rig = StreamRig(icw, oracle, cfg, 6000, settings=[(0,) + KR, (4, 0, 1), (2, 1, 0)])
    ctx, lib = rig.ctx, rig.ctx._lib

    def still_the_same(what):
        assert ctx.stream_hilbert_count() == 3, what
        rig.step(250, what=what)

    for first, count in ((-1, 1), (0, 0), (1, 3), (3, 1), (0, 4)):
        assert lib.icw_set_stream_hilbert(ctx.h, first, count, 1, 1, 1) == abi.EINVAL
    assert lib.icw_set_stream_hilbert(ctx.h, 0, 1, 6, 1, 1) == abi.EINVAL
    still_the_same("bad arguments")
    # while the count is above 1: the FIR converter, bus-form lists, the context encoders
    assert lib.icw_set_fir_hilbert(ctx.h, 64, 8.0) == abi.EUNSUPPORTED
    still_the_same("icw_set_fir_hilbert")
    bus = graph.graph_feedback_pm_shift()
    assert icw.graph_form(cfg, bus) == 1
    acc = C.c_int()
    assert lib.icw_set_graph(ctx.h, graph.node_array(bus), len(bus), 0, C.byref(acc)) == abi.EUNSUPPORTED
    still_the_same("icw_set_graph with a bus-form list")
    late = graph.shift(inputs=("A",), out="B", fr=1.0)      # appended after the tail it runs first: a one-frame delay
    assert icw.graph_form(cfg, graph.graph_shift_master() + [late]) == 1
    assert lib.icw_graph_add_last(ctx.h, C.byref(late)) == abi.EUNSUPPORTED
    still_the_same("a list primitive with a bus-form list")
    n = 64
    rows = rig.rows(n, 0, 3)
    out = np.zeros((3, n * 32), np.uint8)
    for enc in (lib.icw_encode_cwave, lib.icw_encode_cwave_iir):
        assert enc(ctx.h, 0, 3, rows.ctypes.data, rows.shape[1], out.ctypes.data, out.shape[1], n, abi.FMT_CW_F64, 0,
                   None) == abi.EUNSUPPORTED
    assert not out.any()
    still_the_same("the context encoders")
    rig.check("refusals")
    rig.close()

    # the call that would raise the count above 1: the FIR converter on, FP_CHECK, a bus-form list in force
    def refused(ctx, sts, raw, what):
        assert ctx._lib.icw_set_stream_hilbert(ctx.h, 0, 1, 4, 1, 1) == abi.EUNSUPPORTED, what
        assert ctx.stream_hilbert_count() == 1, what
        got, pre = ctx.process(raw, 300, want_pre=True)
        for s, st in enumerate(sts):
            ro, rp = st.process(raw[s], 300, want_pre=True)
            assert np.array_equal(bits(pre[s]), bits(rp)) and np.array_equal(got[s], ro), what
        # one setting for every stream keeps the count at 1 and is served
        ctx.set_stream_hilbert(4, 1, 1)
        assert ctx.stream_hilbert_count() == 1, what
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
