"""GPU: per-stream DSP lists in one context (icw_set_stream_graph, icw_clear_stream_bus_slot,
icw_stream_graph_count) against the oracle -- one oracle.Stream per GPU stream, each with its own
list.  Every comparison is bit for bit: rendered bytes, pre-render doubles, clips, peaks and
de-subnorm counts.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

from in_cwave_amd import abi, graph
from tests import graphgen
from tests.streamrig import StreamRig, bits, copy_cfg, shift_list

pytestmark = pytest.mark.gpu


def mixed(icw, oracle, cfg, lists, n_total, **kw):
    """a rig whose stream s runs lists[s] (bypass[s]), every list given through icw_set_stream_graph"""
    return StreamRig(icw, oracle, cfg, n_total, nodes=graph.graph_master_only(), lists=lists, **kw)


def exec_reads(nodes):
    """per op in execution order (tail first): (the slots it reads, its output slot or None)"""
    return [([k for k in range(abi.N_INPUTS) if n.inputs[k]], n.n_out if n.mode != abi.MODE_MASTER else None)
            for n in nodes[::-1]]


def is_chain(nodes):
    """every op reads only `in` and / or the op just before it (IcwProg.chain)"""
    prev = None
    for reads, out in exec_reads(nodes):
        if any(k != 0 and k != prev for k in reads):
            return False
        prev = out
    return True


def register_list(icw, cfg, rng, bypass=0, want_chain=None):
    """a graphgen list that compiles to the register form (and is / is not a chain, if asked)"""
    while True:
        nodes = graphgen.random_list(rng)
        if icw.graph_form(cfg, nodes, bypass) == 0 and (want_chain is None or is_chain(nodes) == want_chain):
            return nodes


def test_mixed_lists(icw, oracle):
    """five streams, four lists (one shared by two streams that are not adjacent), chain and
    register-file programs in one launch; calls crossing K2's tiles and its 1 024-frame workgroup"""
    cfg = graph.default_config(48000)
    rng = np.random.default_rng(20260)
    lists = [graph.graph_shift_master(), graph.graph_master_only(), graph.graph_shift_master(),
             graph.graph_pm_shift_mix(), register_list(icw, cfg, rng, want_chain=False)]
    rig = mixed(icw, oracle, cfg, lists, 1707)
    assert rig.ctx.stream_graph_count() == 4
    for n in (1100, 7, 600):
        rig.step(n, what="mixed")
    rig.check("mixed")
    rig.close()


@pytest.mark.parametrize("batch", range(4))
def test_random_lists(icw, oracle, batch):
    """64 seeds: four streams with four register-form lists of graphgen (and a bypass flag each), 300 frames"""
    for seed in range(batch * 16, batch * 16 + 16):
        rng = np.random.default_rng(7_000_003 * seed + 5)
        cfg = graphgen.random_config(rng)
        bypass = [int(rng.random() < 0.2) for _ in range(4)]
        lists = [register_list(icw, cfg, rng, bypass[s]) for s in range(4)]
        rig = mixed(icw, oracle, cfg, lists, 300, bypass=bypass, sig0=seed * 4)
        rig.step(300, what=f"seed {seed}")
        rig.check(f"seed {seed}")
        rig.close()


def test_rotation_table_slabs(icw, oracle):
    """two Shift programs over six streams in step (both slabs read); one stream's counter reset (it
    computes its factors inline); a call over streams 2-4 (each slab's reference inside the range)"""
    cfg = graph.default_config(48000)
    a, b = shift_list(2.0), shift_list(3.5)
    lists = [a, b, a, b, a, b]
    rig = mixed(icw, oracle, cfg, lists, 1500)
    ctx = rig.ctx
    assert ctx.stream_graph_count() == 2
    rig.step(500, what="in step")
    ctx.stream_reset_framecnt(2)
    rig.sts[2].set_n_frame(0)
    rig.step(400, what="stream 2 out of step")
    assert ctx.n_frame(2) == 400 and ctx.n_frame(0) == 900
    rig.step(300, first=2, count=3, what="streams 2-4")
    rig.t[0] = rig.t[1] = 1200
    rig.step(300, first=0, count=2, what="streams 0-1")
    rig.check("slabs")
    rig.close()


def test_per_stream_edits(icw, oracle):
    """deleting a node of one stream's list clears that stream's slot only; icw_clear_stream_bus_slot;
    a per-stream bypass flag"""
    cfg = graph.default_config(48000)
    full = [graph.master(inputs=("C",)), graph.mix(inputs=("in", "B"), out="C"), graph.shift(inputs=("in",), out="B")]
    cut = full[:2]                                   # the Mix then reads slot B from the bus
    rig = StreamRig(icw, oracle, cfg, 1600, S=2, nodes=full)
    ctx, sts = rig.ctx, rig.sts
    rig.step(400, what="both full")
    B = graph.slot("B")
    blob = [abi.StateBlob.from_buffer_copy(ctx.get_state(s)) for s in range(2)]
    assert all(any(blob[s].bus[B][k] != 0.0 for k in range(4)) for s in range(2))
    # the Shift goes on stream 1 only: its slot B is zeroed and its Mix reads 0; stream 0 is untouched
    assert ctx.set_stream_graph(cut, 1, 1)
    assert sts[1].set_graph(cut)
    assert ctx.stream_graph_count() == 2
    after = [abi.StateBlob.from_buffer_copy(ctx.get_state(s)) for s in range(2)]
    assert [after[1].bus[B][k] for k in range(4)] == [0.0] * 4
    assert bytes(after[0].bus) == bytes(blob[0].bus)
    rig.step(400, what="stream 1 cut")
    # slot C (written every frame, kept on the bus) of stream 0 only
    Cs = graph.slot("C")
    ctx.clear_stream_bus_slot(Cs, 0, 1)
    sts[0].clear_bus_slot(Cs)
    after = [abi.StateBlob.from_buffer_copy(ctx.get_state(s)) for s in range(2)]
    assert [after[0].bus[Cs][k] for k in range(4)] == [0.0] * 4
    assert any(after[1].bus[Cs][k] != 0.0 for k in range(4))
    rig.step(400, what="slot C of stream 0 cleared")
    # bypass on stream 0 only
    assert ctx.set_stream_graph(full, 0, 1, bypass_list=1)
    assert sts[0].set_graph(full, 1)
    rig.step(400, what="stream 0 bypassed")
    rig.check("edits")
    rig.close()


def test_collapse_and_primitives(icw, oracle):
    """the list primitives are refused while the lists differ (nothing changes); icw_set_graph
    collapses the table, each stream's clears matched against its own old list; then they work again"""
    cfg = graph.default_config(48000)
    lists = [graph.graph_shift_master(), graph.graph_pm_shift_mix()]
    rig = mixed(icw, oracle, cfg, lists, 1500)
    ctx, sts = rig.ctx, rig.sts
    assert ctx.stream_graph_count() == 2
    rig.step(300, what="mixed")
    lib = ctx._lib
    extra = graph.mix(inputs=("in",), out="Q")
    assert lib.icw_graph_del_last(ctx.h) == abi.EUNSUPPORTED
    assert lib.icw_graph_del_all(ctx.h) == abi.EUNSUPPORTED
    assert lib.icw_graph_add_last(ctx.h, C.byref(extra)) == abi.EUNSUPPORTED
    assert lib.icw_graph_set_output_plug(ctx.h, 1, 5) == abi.EUNSUPPORTED
    assert ctx.stream_graph_count() == 2
    rig.step(300, what="after the refused primitives")
    new = [graph.master(inputs=("A",)), graph.shift(inputs=("in",), out="A", fr=5.0), graph.mix(inputs=("in",), out="D")]
    assert ctx.set_graph(new)
    for st in sts:
        assert st.set_graph(new)
    assert ctx.stream_graph_count() == 1
    rig.step(300, what="collapsed")
    ctx.graph_del_last()
    for st in sts:
        st.del_lastdsp()
    rig.step(300, what="del_last after the collapse")
    assert ctx.graph_add_last(extra)
    for st in sts:
        assert st.add_lastdsp(extra)
    rig.step(300, what="add_last after the collapse")
    rig.check("collapse")
    rig.close()


def test_same_list_for_all_is_one_entry(icw, oracle):
    """every stream given one list through the new call: one entry, a one-list context again"""
    cfg = graph.default_config(48000)
    rig = mixed(icw, oracle, cfg, [graph.graph_shift_master(), graph.graph_master_only(), graph.graph_pm_shift_mix()], 500)
    ctx = rig.ctx
    assert ctx.stream_graph_count() == 3
    assert ctx.set_stream_graph(graph.graph_pm_shift_mix())
    assert ctx.stream_graph_count() == 1
    rig.sts = [oracle.Stream(cfg, graph.graph_pm_shift_mix()) for _ in range(3)]
    rig.step(500, what="one entry")
    ctx.graph_del_last()                              # the primitives work on it
    rig.close()


MATRIX = {
    "tpdf_flat": dict(render=(abi.RENDER_TPDF, abi.NSHAPE_FLAT)),
    "tpdf_mew44": dict(render=(abi.RENDER_TPDF, abi.NSHAPE_MEW44)),
    "bits24": dict(need24bits=1),
    "mono": dict(in_channels=1),
    "cw_f64": dict(in_format=abi.FMT_CW_F64),
    "fp_check": dict(fp_check=1),
    "baseline_type4": dict(iir_kahan=0, hilbert_type=4),
}


@pytest.mark.parametrize("case", sorted(MATRIX))
def test_render_and_input_matrix(icw, oracle, case):
    """two streams with different lists through each render / input path K2 serves"""
    kw = dict(MATRIX[case])
    render = kw.pop("render", None)
    cfg = copy_cfg(graph.default_config(48000), **kw)
    if render:
        cfg.render.render_type, cfg.render.nshape_type = render
    lists = [graph.graph_shift_master(), graph.graph_pm_shift_mix()]
    n = 700
    rig = mixed(icw, oracle, cfg, lists, n)
    assert rig.ctx.stream_graph_count() == 2
    rig.step(450, what=case)
    rig.step(n - 450, what=case)
    rig.check(case, census=bool(cfg.fp_check))
    rig.close()


def test_one_stream_context(icw, oracle):
    """576-frame blocks of a one-stream context (K5): icw_set_stream_graph(0, 1) between blocks is the
    oracle's set_graph"""
    cfg = graph.default_config(48000)
    rig = StreamRig(icw, oracle, cfg, 4 * 576, S=1)
    rig.step(576, what="k5")
    for k, nl in enumerate((graph.graph_pm_shift_mix(), graph.graph_master_only(), shift_list(7.25)), 1):
        rig.set_graph(0, nl)
        assert rig.ctx.stream_graph_count() == 1
        rig.step(576, what=f"k5 block {k}")
    rig.check("k5")
    rig.close()


def test_one_stream_calls_of_a_mixed_context(icw, oracle):
    """a call over one stream of a mixed context runs that stream's own program (K5 for 576 frames)"""
    cfg = graph.default_config(48000)
    lists = [graph.graph_shift_master(), graph.graph_pm_shift_mix(), graph.graph_master_only()]
    rig = mixed(icw, oracle, cfg, lists, 576)
    for s in (1, 2, 0):
        rig.step(576, first=s, count=1, what="one stream of three")
    rig.close()


def test_multi_block(icw, oracle, monkeypatch):
    """two streams, two lists, a call of four launch blocks (ICW_BLOCK at its smallest, 256 frames)"""
    monkeypatch.setenv("ICW_BLOCK", "256")
    cfg = graph.default_config(48000)
    lists = [shift_list(2.0), graph.graph_pm_shift_mix()]
    rig = mixed(icw, oracle, cfg, lists, 900)
    rig.step(900, what="four blocks")
    rig.check("four blocks")
    rig.close()


def test_refusals_change_nothing(icw, oracle):
    cfg = graph.default_config(48000)
    lists = [graph.graph_shift_master(), graph.graph_pm_shift_mix()]
    rig = mixed(icw, oracle, cfg, lists, 1800)
    ctx, lib = rig.ctx, rig.ctx._lib

    def still_the_same(what):
        assert ctx.stream_graph_count() == 2
        rig.step(300, what=what)

    def raw_call(nodes, first, count):
        acc = C.c_int(-1)
        arr = graph.node_array(nodes)
        return lib.icw_set_stream_graph(ctx.h, first, count, arr, len(nodes), 0, C.byref(acc)), acc.value

    # a bus-form list (a Mix feeding itself)
    assert raw_call(graph.graph_leaky_feedback(), 0, 1) == (abi.EUNSUPPORTED, 1)
    still_the_same("bus-form list")
    # the same list context-wide while the lists differ
    assert lib.icw_set_graph(ctx.h, graph.node_array(graph.graph_leaky_feedback()), 2, 0, None) == abi.EUNSUPPORTED
    still_the_same("bus-form icw_set_graph on a mixed context")
    # the FIR converter on a mixed context
    assert lib.icw_set_fir_hilbert(ctx.h, 64, 8.0) == abi.EUNSUPPORTED
    still_the_same("set_fir_hilbert on a mixed context")
    # bad ranges, a null list
    for first, count in ((-1, 1), (0, 0), (1, 2), (2, 1), (0, 3)):
        assert raw_call(graph.graph_master_only(), first, count)[0] == abi.EINVAL
    assert lib.icw_set_stream_graph(ctx.h, 0, 1, None, 1, 0, None) == abi.EINVAL
    assert lib.icw_clear_stream_bus_slot(ctx.h, 1, 2, 3) == abi.EINVAL
    assert lib.icw_clear_stream_bus_slot(ctx.h, 0, 1, 27) == abi.EINVAL
    still_the_same("bad ranges")
    # lists amod_init rejects: no Master at the head, two Masters
    assert raw_call([graph.shift()], 0, 1) == (abi.EGRAPH, 0)
    assert raw_call([graph.master(), graph.master()], 1, 1) == (abi.EGRAPH, 0)
    assert ctx.set_stream_graph([graph.shift()], 0, 1) is False
    still_the_same("rejected lists")
    rig.close()

    # the FIR converter on: per-stream lists are refused, the context-wide list goes on
    rig = StreamRig(icw, oracle, cfg, 300, S=2)
    ctx = rig.ctx
    ctx.set_fir_hilbert(64, 8.0)
    arr = graph.node_array(graph.graph_master_only())
    assert ctx._lib.icw_set_stream_graph(ctx.h, 0, 1, arr, 1, 0, None) == abi.EUNSUPPORTED
    assert ctx.stream_graph_count() == 1
    for st in rig.sts:
        st.set_fir(64, 8.0)
    rig.step(300, what="FIR converter on")
    rig.close()

    # a bus-form list in force: per-stream lists are refused
    rig = StreamRig(icw, oracle, cfg, 300, S=2, nodes=graph.graph_leaky_feedback())
    assert rig.ctx._lib.icw_set_stream_graph(rig.ctx.h, 0, 1, arr, 1, 0, None) == abi.EUNSUPPORTED
    rig.step(300, what="bus-form list in force")
    rig.close()


def test_state_round_trip(icw, oracle):
    """get_state from a mixed context, set_state into another context where that stream has the same
    list: the continuation equals an uninterrupted run"""
    cfg = graph.default_config(48000)
    cfg.render.render_type = abi.RENDER_TPDF
    lists = [graph.graph_shift_master(), graph.graph_pm_shift_mix(), graph.graph_master_only()]
    rig = mixed(icw, oracle, cfg, lists, 1000)
    rig.step(600, what="before the checkpoint")
    blob = rig.ctx.get_state(1)
    rig.close()
    # stream 1's state goes to stream 0 of a two-stream context that runs its list there
    other = mixed(icw, oracle, cfg, [lists[1], lists[0]], 1000).ctx
    other.set_state(0, blob)
    raw = rig.frames(1, 400)
    out, pre = other.process(raw[None, :], 400, first=0, count=1, want_pre=True)
    ro, rp = rig.sts[1].process(raw, 400, want_pre=True)
    assert np.array_equal(bits(pre[0]), bits(rp)) and np.array_equal(out[0], ro)
    other.close()
