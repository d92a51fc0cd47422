"""GPU: per-stream FIR Hilbert converters (icw_set_stream_fir) against the oracle -- one oracle.Stream per GPU
stream, each given its own set_fir(order, beta).  Every comparison is bit for bit: rendered bytes, pre-render
doubles where asked, the guard bytes past a stream's frames, clips, peaks and the frame counter
(tests/streamrig.py: call_streams, check_meters).  Nothing here has a tolerance.

Every test calls icw_set_stream_fir, which the library did not have before this file: each fails without it.

Frame counts follow the converter's tiles, as in tests/test_gpu_stream_fir.py: a stereo KF2 tile is 1 024
frames, a mono one 2 048, and the signature form takes the tiles before the last, so a 2 500-frame call without
pre-render doubles runs signature tiles and a generic one.  Orders 2 .. 4 096 stand beside each other, so a
call is shorter than one stream's order and longer than its neighbour's."""

import ctypes as C

import numpy as np
import pytest

from in_cwave_amd import abi, graph
from in_cwave_amd import lib as L

from tests.streamrig import StreamRig, copy_cfg, entry, shift_list

from test_gpu_stream_encode import encode_call, loud_pcm, rows_of
from test_gpu_stream_fir import master_only

pytestmark = pytest.mark.gpu

BETA = 8.0
I16S = (48000, abi.FMT_I16, 2)
# orders 2, 30, 254, 1 022, then 30 at another beta, then 254 again (shares an entry): five entries
CONVS6 = [(2, BETA), (30, BETA), (254, BETA), (1022, BETA), (30, 5.0), (254, BETA)]


@pytest.fixture(autouse=True, params=["fused", "split"])
def fir_form(request, monkeypatch):
    """KF2 (converter, graph and render in one kernel: the generic and the signature form) and KF + K2
    (ICW_FIR_FUSED=0), as tests/test_gpu_stream_fir.py switches them"""
    monkeypatch.setenv("ICW_FIR_FUSED", "1" if request.param == "fused" else "0")
    return request.param


def runs_of(values):
    """(first, count, value) of the maximal runs of equal consecutive values"""
    out, s = [], 0
    while s < len(values):
        n = 1
        while s + n < len(values) and values[s + n] == values[s]:
            n += 1
        out.append((s, n, values[s]))
        s += n
    return out


class ConvRig(StreamRig):
    """the rig with a converter per stream: stream s has inputs[s], runs lists[s] and converts with convs[s] =
    (order, beta).  The converter goes on for every stream through the per-stream setter over the whole range
    (all FIR or none), then every run of equal pairs gets its own.  conv_first: before the per-stream lists and
    inputs, else after them.  An input equal to cfg's is not set: a context whose streams share one list and
    one input keeps one-entry tables beside the converters"""

    def __init__(self, icw, oracle, cfg, inputs, lists, convs, n_total, conv_first=True):
        S = len(inputs)
        self.ctx = icw.Context(copy_cfg(cfg), lists[0], S)
        self.ctx.enable_stream_fir()
        self.convs = [None] * S
        own = (cfg.sample_rate, cfg.in_format, cfg.in_channels)
        self.sts = [oracle.Stream(copy_cfg(cfg), lists[s]) for s in range(S)]
        self.inputs, self.cur = [own] * S, [None] * S
        if conv_first:
            self.set_convs(convs)
        for s in range(S):
            if lists[s] is not lists[0]:
                assert self.ctx.set_stream_graph(lists[s], s, 1, cfg.bypass_list)
        for s, inp in enumerate(inputs):
            if tuple(inp) != own:
                self.set_input(s, *inp)
        if not conv_first:
            self.set_convs(convs)
        self.raw = [self.signal(s, n_total, *inp) for s, inp in enumerate(self.inputs)]
        self.osz = [2 * self.ctx.render_size] * S
        self.t, self.pad = [0] * S, 0

    def set_convs(self, convs):
        self.set_conv(0, len(convs), *convs[0])
        for first, count, (order, beta) in runs_of(list(convs)):
            if (order, beta) != tuple(convs[0]):
                self.set_conv(first, count, order, beta)
        assert self.ctx.stream_fir_count() == len(set(convs))

    def set_conv(self, s, count, order, beta):
        """icw_set_stream_fir on the context, set_fir on the range's oracles: they restart from a zero history"""
        self.ctx.set_stream_fir(order, beta, s, count)
        for i in range(s, s + count):
            self.sts[i].set_fir(order, beta)
            self.convs[i] = self.cur[i] = (order, beta)

    def run(self, n, **kw):
        """a call without pre-render doubles (the signature form's condition): rendered bytes only"""
        return self.step(n, want_pre=False, **kw)

    def go(self, n, pre, **kw):
        return (self.step if pre else self.run)(n, **kw)


def refused(rc, what):
    assert rc == abi.EUNSUPPORTED, f"{what}: returned {rc}, not ICW_EUNSUPPORTED"


# ------------------------------------------------------------------ 1. matrix
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("pre", [False, True], ids=["bytes", "pre"])
def test_matrix(icw, oracle, device, pre):
    """six stereo int16 streams, a Master-only list, five entries: one list, one input, so only the converters
    differ; calls of 900, 2 500 and 1 frames"""
    cfg = graph.default_config(48000)
    rig = ConvRig(icw, oracle, cfg, [I16S] * 6, [master_only(0.5, 0.5)] * 6, CONVS6, 3401)
    assert rig.ctx.stream_fir_count() == 5 and rig.ctx.stream_graph_count() == 1 and rig.ctx.stream_input_count() == 1
    for n in (900, 2500, 1):
        rig.go(n, pre, device=device, what="matrix")
    rig.check("matrix")
    rig.close()


# ------------------------------------------------------------------ 2. beside lists and inputs
@pytest.mark.parametrize("conv_first", [True, False], ids=["conv_first", "conv_last"])
def test_beside_lists_and_inputs(icw, oracle, conv_first):
    """mono and stereo streams in int16, int24 and float32 at two rates, Shift -> Master lists of different
    frequencies, orders 30, 254 and 1 022 across them; the converters set before and after the other tables"""
    cfg = graph.default_config(48000)
    inputs = [(48000, abi.FMT_I16, 2), (44100, abi.FMT_I24, 1), (48000, abi.FMT_F32, 2), (44100, abi.FMT_I16, 1),
              (48000, abi.FMT_I24, 2), (44100, abi.FMT_F32, 1), (48000, abi.FMT_I16, 1)]
    lists = [shift_list(1.0 + 0.75 * s) for s in range(7)]
    convs = [(254, BETA), (30, BETA), (1022, BETA), (1022, BETA), (30, BETA), (254, BETA), (254, 5.0)]
    rig = ConvRig(icw, oracle, cfg, inputs, lists, convs, 3401, conv_first=conv_first)
    assert rig.ctx.stream_fir_count() == 4 and rig.ctx.stream_graph_count() == 7
    rig.run(2500, what="lists and inputs")
    rig.step(900, what="lists and inputs, pre")
    rig.run(1, what="lists and inputs, one frame")
    rig.check("lists and inputs")
    rig.close()


# ------------------------------------------------------------------ 3. blocks shorter than an order
def test_blocks_shorter_than_an_order(icw, oracle):
    """orders 2 and 1 022 side by side: five calls of 100 frames (shorter than one history, longer than the
    other), then one of 3 000"""
    cfg = graph.default_config(48000)
    convs = [(2, BETA), (1022, BETA), (1022, BETA), (2, BETA)]
    rig = ConvRig(icw, oracle, cfg, [I16S] * 4, [graph.graph_shift_master()] * 4, convs, 3500)
    for k in range(5):
        rig.go(100, k & 1, what=f"short call {k}")
    rig.run(3000, what="long call")
    rig.check("short blocks")
    rig.close()


# ------------------------------------------------------------------ 4. several launch blocks per call
def test_launch_blocks_and_sub_ranges(icw, oracle, monkeypatch):
    """launch blocks of 263 frames, shorter than orders 1 022 and 254 and longer than 30 and 2: sub-range calls
    that each mix orders (the others keep their history where it is), then the whole batch"""
    monkeypatch.setenv("ICW_BLOCK", "263")
    cfg = graph.default_config(48000)
    convs = [(30, BETA), (1022, BETA), (254, BETA), (2, BETA), (254, BETA), (1022, 5.0)]
    inputs = [I16S, I16S, (44100, abi.FMT_I24, 1), I16S, (96000, abi.FMT_F32, 2), I16S]
    rig = ConvRig(icw, oracle, cfg, inputs, [shift_list(2.0)] * 6, convs, 3000)
    rig.step(700, first=0, count=3, what="[0, 3)")
    rig.step(900, first=3, count=3, what="[3, 6)")
    rig.run(1100, first=0, count=3, what="[0, 3) again")
    rig.run(1100, what="all")
    rig.check("launch blocks")
    rig.close()


# ------------------------------------------------------------------ 5. edits keep the neighbours
def test_edits_keep_the_neighbours(icw, oracle):
    """icw_set_stream_fir on streams [2, 4) after two calls: the largest order in force goes from 254 to 2 048
    (the history is re-laid wider), later down to 30 (narrower).  The streams outside continue their oracle
    streams bit for bit; the streams inside restart as set_fir restarts the oracle's"""
    cfg = graph.default_config(48000)
    convs = [(30, BETA), (2, BETA), (254, BETA), (254, BETA), (30, BETA), (30, 5.0)]
    rig = ConvRig(icw, oracle, cfg, [I16S] * 6, [graph.graph_shift_master()] * 6, convs, 6000)
    size = lambda: rig.ctx._lib.icw_state_size(rig.ctx.h)
    base = size() - 2 * 254 * 8
    rig.run(900, what="first")
    rig.step(577, what="second")
    rig.set_conv(2, 2, 2048, BETA)
    assert rig.ctx.stream_fir_count() == 4 and size() == base + 2 * 2048 * 8
    rig.step(900, what="after the raise")
    rig.run(1100, first=1, count=3, what="after the raise, [1, 4)")
    rig.set_conv(2, 2, 30, BETA)
    assert rig.ctx.stream_fir_count() == 3 and size() == base + 2 * 30 * 8
    rig.step(900, what="after the fall")
    rig.set_conv(2, 2, 30, BETA)                      # unchanged setting: the range restarts all the same
    rig.run(1200, what="after the same again")
    rig.check("edits")
    rig.close()


# ------------------------------------------------------------------ 6. collapse
@pytest.mark.parametrize("how", ["stream_setter", "context_setter"])
def test_collapse(icw, oracle, how):
    """a mixed context given one pair again, through either setter, is a one-converter context: count 1, the
    launch blocks and the bytes of a context that only ever called icw_set_fir_hilbert"""
    cfg = graph.default_config(48000)
    rig = ConvRig(icw, oracle, cfg, [I16S] * 4, [graph.graph_shift_master()] * 4, [(30, BETA), (1022, BETA)] * 2, 4000)
    rig.run(700, what="mixed")
    if how == "stream_setter":
        rig.set_conv(0, 4, 254, BETA)
    else:
        rig.ctx.set_fir_hilbert(254, BETA)
        for st in rig.sts:
            st.set_fir(254, BETA)
    assert rig.ctx.stream_fir_count() == 1
    rig.run(2500, timing=True, what="collapsed")
    launches = rig.ctx.last_timing()[1]
    # the launch blocks of a context that only ever called icw_set_fir_hilbert, over the same frames
    one = icw.Context(copy_cfg(cfg), graph.graph_shift_master(), 4)
    one.set_fir_hilbert(254, BETA)
    assert one.stream_fir_count() == 1
    rows = rig.rows(2500, 0, 4, t=700)
    sink = np.zeros((4, 2500 * 4), np.uint8)
    rc = one._lib.icw_process_streams(one.h, 0, 4, rows.ctypes.data, rows.shape[1], sink.ctypes.data, sink.shape[1], 2500,
                                      abi.F_TIMING, None, None)
    assert rc == abi.OK and one.last_timing()[1] == launches
    one.close()
    rig.check("collapse")
    rig.close()
    # the bytes, against that context's own: fresh contexts, the same frames, a Master-only list
    m = master_only(0.5, 0.25)
    a = ConvRig(icw, oracle, cfg, [I16S] * 4, [m] * 4, [(30, BETA), (1022, BETA)] * 2, 2500)
    if how == "stream_setter":
        a.set_conv(0, 4, 254, BETA)
    else:
        a.ctx.set_fir_hilbert(254, BETA)
        for st in a.sts:
            st.set_fir(254, BETA)
    got = a.run(2500, what="collapsed, fresh")
    b = icw.Context(copy_cfg(cfg), m, 4)
    b.set_fir_hilbert(254, BETA)
    ref, _ = b.process(a.rows(2500, 0, 4, t=0), 2500)
    assert np.array_equal(got[:, :ref.shape[1]], ref)
    a.close()
    b.close()


# ------------------------------------------------------------------ 7. too wide for the fused kernel
def test_too_wide_for_the_fused_kernel(icw, oracle, fir_form):
    """one stereo stream at order 4 096 beside order 2: icw_fir_graph_lds says which side of the fused kernel's
    limit each falls on; a call with a stream that does not fit runs KF + K2 for its streams, bit-exact"""
    lds = icw.load().icw_fir_graph_lds
    lds.restype, lds.argtypes = C.c_size_t, [C.c_int] * 4
    nt = lambda M: (M // 2 + 1) // 2
    assert lds(2, nt(2), 2, 0) > 0 and lds(1022, nt(1022), 2, 0) > 0
    assert lds(4096, nt(4096), 2, 0) == 0, "order 4 096 stereo fits the fused kernel: the test's premise moved"
    cfg = graph.default_config(48000)
    rig = ConvRig(icw, oracle, cfg, [I16S] * 3, [graph.graph_shift_master()] * 3, [(2, BETA), (4096, BETA), (2, BETA)], 6000)
    rig.run(2500, what="too wide")
    rig.step(900, what="too wide, pre")
    rig.run(1100, first=0, count=1, what="the narrow stream alone")
    rig.check("too wide")
    rig.close()


# ------------------------------------------------------------------ 8. serial render
def test_serial_render(icw, oracle):
    """24-bit TPDF + MEW44, context-wide (the serial render behind the converter), over orders 30 and 1 022"""
    cfg = graph.default_config(48000, need24bits=True)
    cfg.render.render_type = abi.RENDER_TPDF
    cfg.render.nshape_type = abi.NSHAPE_MEW44
    convs = [(30, BETA), (1022, BETA), (1022, BETA), (30, BETA)]
    inputs = [I16S, (44100, abi.FMT_F32, 1), I16S, (96000, abi.FMT_I24, 2)]
    rig = ConvRig(icw, oracle, cfg, inputs, [shift_list(2.0)] * 4, convs, 2500)
    rig.run(2500, what="mew44")
    rig.check("mew44")
    rig.close()


# ------------------------------------------------------------------ 9. refusals
def test_refusals_change_nothing(icw, oracle):
    cfg = graph.default_config(48000)
    lib = icw.load()
    # a fresh context without icw_enable_stream_fir
    ctx = icw.Context(copy_cfg(cfg), graph.graph_shift_master(), 4)
    ctx.set_fir_hilbert(30, BETA)
    refused(lib.icw_set_stream_fir(ctx.h, 0, 2, 254, BETA), "without icw_enable_stream_fir")
    refused(lib.icw_set_stream_fir(ctx.h, 0, 4, 254, BETA), "without icw_enable_stream_fir, whole range")
    assert ctx.stream_fir_count() == 1
    ctx.close()
    # an IIR context: k_M > 0 on a sub-range; then the converter beside two stream renders, and beside two stream
    # Hilbert settings -- the streams go on bit-exact after each
    for axis in ("render", "hilbert"):
        kw = dict(renders=[None, entry(b24=True), None, None]) if axis == "render" else dict(settings=[None, None, (4, 0, 0), None])
        rig = StreamRig(icw, oracle, cfg, 2000, **kw)
        ctx = rig.ctx
        ctx.enable_stream_fir()
        rig.step(600, what=f"two {axis}s, before")
        refused(lib.icw_set_stream_fir(ctx.h, 1, 2, 30, BETA), "k_M > 0 on a sub-range of an IIR context")
        refused(lib.icw_set_stream_fir(ctx.h, 0, 4, 30, BETA), f"beside two stream {axis} settings")
        assert ctx.stream_fir_count() == 1
        assert (ctx.stream_render_count(), ctx.stream_hilbert_count()) == ((2, 1) if axis == "render" else (1, 2))
        rig.step(900, what=f"two {axis}s, after the refusals")
        rig.check(f"two {axis}s")
        rig.close()
    # a cfg.fp_check context
    ctx = icw.Context(copy_cfg(cfg, fp_check=1), graph.graph_shift_master(), 2)
    ctx.enable_stream_fir()
    refused(lib.icw_set_stream_fir(ctx.h, 0, 2, 30, BETA), "a cfg.fp_check context")
    assert ctx.stream_fir_count() == 1
    ctx.close()
    # a mixed context: every refusal leaves the count and the streams where they were
    convs = [(30, BETA), (254, BETA), (254, BETA), (30, BETA)]
    rig = ConvRig(icw, oracle, cfg, [I16S] * 4, [graph.graph_shift_master()] * 4, convs, 4000)
    ctx = rig.ctx
    rig.run(700, what="before")
    refused(lib.icw_set_stream_fir(ctx.h, 1, 2, 0, BETA), "k_M = 0 on a sub-range")
    for order, beta in ((31, BETA), (4098, BETA), (-2, BETA), (30, -1.0), (30, 1e3)):
        rc = lib.icw_set_stream_fir(ctx.h, 1, 2, order, beta)
        assert rc == abi.EINVAL, f"order {order} beta {beta}: returned {rc}"
    for first, count in ((-1, 2), (3, 2), (0, 0), (0, 5)):
        assert lib.icw_set_stream_fir(ctx.h, first, count, 30, BETA) == abi.EINVAL, (first, count)
    r, b24 = entry(b24=True)
    refused(lib.icw_set_stream_render(ctx.h, 1, 1, C.byref(r), 1), "icw_set_stream_render at FIR count 2")
    refused(lib.icw_set_stream_hilbert(ctx.h, 1, 1, 4, 0, 0), "icw_set_stream_hilbert at FIR count 2")
    refused(lib.icw_enable_stream_fir(ctx.h, 0), "icw_enable_stream_fir(ctx, 0) at FIR count 2")
    assert ctx.stream_fir_count() == 2 and ctx.stream_render_count() == 1 and ctx.stream_hilbert_count() == 1
    rig.step(900, what="after the refusals")
    rig.run(1100, what="after the refusals, bytes")
    rig.check("refusals")
    # the whole context off through the per-stream setter is icw_set_fir_hilbert(ctx, 0, ..)
    rig.set_conv(0, 4, 0, BETA)
    assert ctx.stream_fir_count() == 1
    rig.step(700, what="off")
    rig.close()


# ------------------------------------------------------------------ 10. state blob
def test_state_blob(icw, oracle):
    """an order-254 stream's state goes from a mixed context into another context's order-254 stream, whose next
    900 frames are the source's; into an order-30 stream it is ICW_EINVAL"""
    cfg = graph.default_config(48000)
    convs = [(30, BETA), (254, BETA), (1022, BETA)]
    rig = ConvRig(icw, oracle, cfg, [I16S] * 3, [graph.graph_shift_master()] * 3, convs, 3000)
    rig.run(1300, what="before")
    blob = rig.ctx.get_state(1)
    assert len(blob) == rig.ctx._lib.icw_state_size(rig.ctx.h)
    rows = rig.rows(900, 1, 1)
    src = rig.step(900, first=1, count=1, what="the source").copy()
    # the target also holds an order-1 022 stream, so its own blobs are larger than an order-254 stream's: a blob
    # need hold no more than its own order's history
    other = icw.Context(copy_cfg(cfg), graph.graph_shift_master(), 3)
    other.enable_stream_fir()
    other.set_stream_fir(30, BETA)
    other.set_stream_fir(254, BETA, 1, 1)
    other.set_stream_fir(1022, BETA, 2, 1)
    assert other.stream_fir_count() == 3
    fixed = other._lib.icw_state_size(other.h) - 2 * 1022 * 8
    own = blob[:fixed + 2 * 254 * 8]
    assert not any(blob[len(own):]), "the blob past the stream's own history is zero"
    other.set_state(1, own)
    got, _ = other.process(rows, 900, first=1, count=1)
    assert np.array_equal(got[0], src[0, :got.shape[1]])
    buf = (C.c_uint8 * len(own)).from_buffer_copy(own)
    assert other._lib.icw_set_state(other.h, 0, buf, len(own)) == abi.EINVAL          # an order-30 stream
    assert other._lib.icw_set_state(other.h, 1, buf, len(own) - 8) == abi.EINVAL      # short of its own history
    other.close()
    rig.close()


# ------------------------------------------------------------------ 11. encoder
ENC_INPUTS = {"mixed_inputs": [(48000, abi.FMT_I16, 2), (44100, abi.FMT_I24, 1), (48000, abi.FMT_F32, 2), (48000, abi.FMT_I16, 1)],
              "one_input": [I16S] * 4}
ENC_CONVS = [(30, BETA), (254, BETA), (1022, BETA), (254, BETA)]
ENC_CALLS = (2500, 577)


@pytest.mark.parametrize("cw_format", [abi.FMT_CW_F64, abi.FMT_CW_I16], ids=["f64", "i16"])
@pytest.mark.parametrize("case", list(ENC_INPUTS))
@pytest.mark.parametrize("block", [None, "263"], ids=["one_block", "blocks_of_263"])
def test_encoder(icw, cw_format, case, block, monkeypatch):
    """icw_encode_cwave writes stream s with stream s's own converter: its frames and icw_encode_clipped are,
    byte for byte, what a one-converter context of that pair writes for the same input.  blocks_of_263: several
    launch blocks per call, where the per-stream kernel places each block's tile by the block offset"""
    if block:
        monkeypatch.setenv("ICW_BLOCK", block)
    inputs = ENC_INPUTS[case]
    n_total = sum(ENC_CALLS)
    raws = [loud_pcm(s, n_total, r, c, f) for s, (r, f, c) in enumerate(inputs)]
    rate, fmt, ch = inputs[0]
    ctx = icw.Context(graph.default_config(rate, fmt=fmt, channels=ch), graph.graph_shift_master(), len(inputs))
    ctx.enable_stream_fir()
    ctx.set_stream_fir(*ENC_CONVS[0])
    for first, count, conv in runs_of(ENC_CONVS):
        ctx.set_stream_fir(*conv, first, count)
    if case == "mixed_inputs":
        for s, (r, f, c) in enumerate(inputs):
            ctx.set_stream_input(r, f, c, s, 1)
    assert ctx.stream_fir_count() == 3
    # without icw_enable_stream_encode the mixed converters are refused, as differing inputs are
    rows = rows_of(inputs, raws, 0, 100)
    out = np.zeros((len(inputs), 100 * 32), np.uint8)
    rc = ctx._lib.icw_encode_cwave(ctx.h, 0, len(inputs), rows.ctypes.data, rows.strides[0], out.ctypes.data, out.strides[0],
                                   100, cw_format, 0, None)
    assert rc == abi.EUNSUPPORTED and not out.any()
    ctx.enable_stream_encode()
    parts, t = [[] for _ in inputs], 0
    for n in ENC_CALLS:
        got = encode_call(ctx, "fir", rows_of(inputs, raws, t, n), n, cw_format)
        for s in range(len(inputs)):
            parts[s].append(got[s])
        t += n
    clipped = [ctx.encode_clipped(s) for s in range(len(inputs))]
    ctx.close()
    for s, (inp, conv) in enumerate(zip(inputs, ENC_CONVS)):
        one = icw.Context(graph.default_config(inp[0], fmt=inp[1], channels=inp[2]), graph.graph_shift_master(), 1)
        one.set_fir_hilbert(*conv)
        t = 0
        for k, n in enumerate(ENC_CALLS):
            ref = encode_call(one, "fir", rows_of([inp], [raws[s]], t, n), n, cw_format)[0]
            assert np.array_equal(parts[s][k], ref), f"stream {s} {inp} order {conv[0]}: call {k} of {n} frames differs"
            t += n
        assert one.encode_clipped(0) == clipped[s], f"stream {s} {inp} order {conv[0]}: clipped"
        one.close()
