"""GPU: the two routes to one setting agree.  Two contexts of three streams with the same config and list;
one is edited with the context-wide setters (set_render then set_outbits, set_hilbert_filter then
set_hilbert_config, set_graph, set_input), the other with the per-stream setters over every stream, with the
same values.  A 600-frame call on every stream comes between the edits (every launch block has an odd tail).
After every call, for every stream, byte for byte between the two: the rendered bytes, clips, the peak dB
bits, the de-subnorm counts, the frame counter and the state blob; and both contexts hold one list, one
input, one render and one converter setting throughout.  Nothing here has a tolerance."""

import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth
from tests.streamrig import NS_FIR20, entry

pytestmark = pytest.mark.gpu

S = 3
N = 600
FS = 48000


# Master loud enough that the -12 dBFS test tones clip; the Mix reads slot B, which the Shift writes
FULL = [graph.master(inputs=("C",), gain=3.0), graph.mix(inputs=("in", "B"), out="C"),
        graph.shift(inputs=("in",), out="B", fr=2.0)]
CUT = FULL[:2]        # the Shift goes: its slot B is cleared (matched by position) and the Mix reads zero


def ed_render(r, b24):
    return (f"render type {r.render_type} shaper {r.nshape_type} bits16 {r.sign_bits16} depth {24 if b24 else 16}",
            lambda a: (a.set_render(r), a.set_outbits(b24)),
            lambda b: b.set_stream_render(r, b24, 0, S), None)


def ed_hilbert(t, kahan, subn):
    return (f"hilbert type {t} kahan {kahan} reject {subn}",
            lambda a: (a.set_hilbert_filter(t), a.set_hilbert_config(kahan, subn)),
            lambda b: b.set_stream_hilbert(t, kahan, subn, 0, S), None)


def ed_graph(nodes):
    def wide(a):
        assert a.set_graph(nodes)

    def each(b):
        assert b.set_stream_graph(nodes, 0, S)
    return (f"list of {len(nodes)} nodes", wide, each, None)


def ed_input(rate, fmt, ch):
    return (f"input {rate} Hz fmt {fmt} x{ch}",
            lambda a: a.set_input(rate, fmt, ch),
            lambda b: b.set_stream_input(rate, fmt, ch, 0, S), (rate, fmt, ch))


EDITS = [
    ed_render(*entry(abi.RENDER_TPDF, abi.NSHAPE_MEW44, True)),       # dither + shaping; 16 -> 24 moves hi
    ed_render(*entry(abi.RENDER_TPDF, abi.NSHAPE_MEW44)),             # the depth alone
    ed_render(*entry(abi.RENDER_GAUSS, NS_FIR20, dth=1.5, sb16=14)),  # hi moves at one depth
    ed_hilbert(3, 1, 1),                                               # the type: rings restart
    ed_hilbert(3, 0, 1),                                               # the summation alone: rings stay
    ed_render(*entry()),                                              # back to ROUND + flat
    ed_graph(CUT),                                                     # a matched clear
    ed_input(44100, abi.FMT_I24, 1),
    ed_hilbert(1, 1, 0),
    ed_graph(FULL),
]


def counts(ctx):
    return (ctx.stream_graph_count(), ctx.stream_input_count(), ctx.stream_render_count(), ctx.stream_hilbert_count())


def test_context_wide_and_per_stream_setters_agree(icw):
    cfg = graph.default_config(FS)
    a = icw.Context(abi.Config.from_buffer_copy(cfg), FULL, S)
    b = icw.Context(abi.Config.from_buffer_copy(cfg), FULL, S)
    n_total = N * (len(EDITS) + 1)
    inp = (FS, abi.FMT_I16, 2)
    raw = {}

    def rows(k):
        if inp not in raw:
            raw[inp] = synth.batch_pcm(S, n_total, inp[0], channels=inp[2], fmt=inp[1])
        fsz = abi.FMT_BYTES[inp[1]] * inp[2]
        return np.ascontiguousarray(raw[inp][:, k * N * fsz:(k + 1) * N * fsz])

    def call(k, what):
        x = rows(k)
        oa, _ = a.process(x, N)
        ob, _ = b.process(x, N)
        assert oa.shape == ob.shape and np.array_equal(oa, ob), f"{what}: rendered bytes"
        assert counts(a) == (1, 1, 1, 1) and counts(b) == (1, 1, 1, 1), (what, counts(a), counts(b))
        for s in range(S):
            ma, mb = a.meters(s), b.meters(s)
            assert ma["clips"] == mb["clips"], (what, s, ma, mb)
            assert np.array_equal(np.array(ma["peak_db"]).view(np.uint64), np.array(mb["peak_db"]).view(np.uint64)), (what, s, ma, mb)
            assert ma["desubnorm"] == mb["desubnorm"], (what, s, ma, mb)
            assert a.n_frame(s) == b.n_frame(s) == (k + 1) * N, (what, s)
            assert a.stream_render_size(s) == b.stream_render_size(s), (what, s)
            assert a.get_state(s) == b.get_state(s), f"{what}: state blob of stream {s}"
        return oa

    try:
        out = call(0, "fresh")
        for k, (what, wide, each, new_inp) in enumerate(EDITS, 1):
            wide(a)
            each(b)
            inp = new_inp or inp               # the rows of the calls from here on
            out = call(k, what)
            assert out.any(), what
        clipped = any(sum(a.meters(s)["clips"]) > 0 for s in range(S))
        assert clipped, "the loud Master never clipped: the clip counters were compared at zero"
    finally:
        a.close()
        b.close()
