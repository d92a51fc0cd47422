"""The row IIR (icw_iir_row, and K5's icw_iir_row_body) with its regenerated term block
(in_cwave_amd/csrc/icw_row_asm.inc: the compensation update as VOP2 v_fmac_f64), bit for bit against the
oracle at the smallest shapes where the block, its register constraints or its encoding can go wrong:
  - w rows: the last N states of all four filters (the state blob's hist) against oracle.iir_block run
    over the filters' own input rows ({x, 0, -x, 0} / {0, -x, 0, x}, lpf_hilbert_quad.c:129-156);
  - pre-render doubles, rendered bytes and meters against oracle.Stream.
Cases: all six filter types (orders 15 / 18 / 19 / 20), Kahan with reject; call lengths below, at and above
the speculative path's 3N threshold, with an odd-order lone leading block and a remainder; 1, 2, 3 and 5
streams (a wave with empty rows, a wave pair with one filled slot); two consecutive calls (the second
speculates from carried state, at the other phase parity for the odd lengths); a wave whose streams' Hilbert
phases differ in parity (the vote falls back); a stream whose sums dip below 1 after the first speculative
pair; the mono dedup; the 576-frame one-stream call through K5.

The dip case needs a state the oracle has no entry point to load, so there the references are the
independent Python restatement (tests/pyref_iir.py, pinned to the oracle by tests/test_oracle_pyref.py) for
the w rows and reject counts, and the lane-per-chain kernel (icw_iir_state, not touched by the block; pinned
to the oracle by tests/test_gpu_parity.py) for the pre-render doubles, bytes and meters."""
import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth
from tests.pyref_iir import PyHilbert

pytestmark = pytest.mark.gpu

FS = 48000


def _row(monkeypatch, stream1="0"):
    monkeypatch.setenv("ICW_K1_MODE", "row")
    monkeypatch.setenv("ICW_RENDER", "row")
    monkeypatch.setenv("ICW_STREAM1", stream1)


def _order(oracle, htype):
    return len(oracle.iir_coeffs(htype)[0])


def _lengths(n):
    return [3 * n - 1, 3 * n, 3 * n + 1, 5 * n + 7, 2 * (2 * n) + n + 3]


def _filter_inputs(x):
    """the I and Q filters' input rows of one channel from phase 0 (hq_rp_process): the sample at the
    filter's own phases, signed, and the literal +0.0 at the others"""
    x = np.asarray(x, dtype=np.float64)
    k = np.arange(x.size) & 3
    fi = np.where(k == 0, x, np.where(k == 2, -x, 0.0))
    fq = np.where(k == 3, x, np.where(k == 1, -x, 0.0))
    return fi, fq


def _assert_w_rows(oracle, ctx, s, htype, n, chans):
    """hist[ch * 2 + f][i] = w[last - i] of filter f of channel ch; chans: the channels' samples since
    the stream's last Hilbert reset"""
    blob = abi.StateBlob.from_buffer_copy(ctx.get_state(s))
    h = np.ctypeslib.as_array(blob.hist)
    for ch, x in enumerate(chans):
        for f, seq in enumerate(_filter_inputs(x)):
            _, w, cnt = oracle.iir_block(seq, htype, 1, 1)
            want = w[::-1][:n]
            got = h[ch * 2 + f][:want.size]
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (s, ch, f)
            assert blob.sncnt[ch * 2 + f] == cnt, (s, ch, f)


def _pcm16(raw, channels=2):
    return raw.view(np.int16).reshape(raw.shape[0], -1, channels).astype(np.float64)


def _run_calls(oracle, icw, cfg, nodes, raw, lens, htype, n, channels=2):
    """the calls through one context and one oracle stream per stream: pre-render doubles and bytes per
    call, then meters and w rows"""
    S = raw.shape[0]
    ctx = icw.Context(cfg, nodes, S)
    refs = [oracle.Stream(cfg, nodes) for _ in range(S)]
    fsz, t = ctx.fsz, 0
    for L in lens:
        seg = np.ascontiguousarray(raw[:, t * fsz:(t + L) * fsz])
        out, pre = ctx.process(seg, L, want_pre=True)
        for s in range(S):
            ro, rp = refs[s].process(seg[s], L, want_pre=True)
            bad = np.flatnonzero(pre[s].view(np.uint64) != rp.view(np.uint64))
            assert bad.size == 0, (S, L, t, s, bad[:5])
            assert np.array_equal(out[s], ro), (S, L, t, s)
        t += L
    x = _pcm16(raw, channels)
    for s in range(S):
        assert ctx.meters(s) == refs[s].meters(), (S, lens, s)
        chans = [x[s, :t, c] for c in range(channels)] * (2 // channels)
        _assert_w_rows(oracle, ctx, s, htype, n, chans)
    ctx.close()


@pytest.mark.parametrize("htype", [0, 1, 2, 3, 4, 5])
def test_lengths_streams_two_calls(oracle, icw, htype, monkeypatch):
    """T in {3N-1, 3N, 3N+1, 5N+7, 2(2N)+N+3} x streams in {1, 2, 3, 5}, each length twice in a row"""
    _row(monkeypatch)
    n = _order(oracle, htype)
    cfg = graph.default_config(FS, hilbert_type=htype)
    nodes = graph.graph_master_only()
    lens = _lengths(n)
    raw = synth.batch_pcm(5, 2 * max(lens), FS, first=htype)
    for S in (1, 2, 3, 5):
        for L in lens:
            _run_calls(oracle, icw, cfg, nodes, np.ascontiguousarray(raw[:S, :2 * L * 4]), [L, L], htype, n)


@pytest.mark.parametrize("htype", [0, 1, 2, 3, 4, 5])
def test_wave_mate_of_other_parity(oracle, icw, htype, monkeypatch):
    """after an odd-length call one of three streams restarts its Hilbert phase: its wave holds both
    parities and takes the generic blocks, and so does the next call's"""
    _row(monkeypatch)
    n = _order(oracle, htype)
    cfg = graph.default_config(FS, hilbert_type=htype)
    nodes = graph.graph_master_only()
    S, L0, L1 = 3, 3 * n + 1 + (n & 1), 5 * n + 7       # L0 odd
    assert L0 & 1
    ctx = icw.Context(cfg, nodes, S)
    refs = [oracle.Stream(cfg, nodes) for _ in range(S)]
    raw = synth.batch_pcm(S, L0 + 2 * L1, FS, first=10 + htype)
    fsz = ctx.fsz
    t = 0
    for i, L in enumerate((L0, L1, L1)):
        if i == 1:
            ctx.stream_open(1, 1 << 40, clr_hilb=1)
            refs[1].open(1 << 40, clr_hilb=1)
        seg = np.ascontiguousarray(raw[:, t * fsz:(t + L) * fsz])
        out, pre = ctx.process(seg, L, want_pre=True)
        for s in range(S):
            ro, rp = refs[s].process(seg[s], L, want_pre=True)
            assert np.array_equal(pre[s].view(np.uint64), rp.view(np.uint64)), (i, s)
            assert np.array_equal(out[s], ro), (i, s)
        t += L
    x = _pcm16(raw)
    for s in range(S):
        t0 = L0 if s == 1 else 0                       # stream 1's filters restarted at the reopen
        _assert_w_rows(oracle, ctx, s, htype, n, [x[s, t0:t, c] for c in range(2)])
    ctx.close()


@pytest.mark.parametrize("htype", [0, 1, 2, 3, 4, 5])
def test_mono_dedup(oracle, icw, htype, monkeypatch):
    """mono input on fresh streams: the left chains only, the right converters' state a copy"""
    _row(monkeypatch)
    n = _order(oracle, htype)
    cfg = graph.default_config(FS, channels=1, hilbert_type=htype)
    L = 5 * n + 7
    raw = synth.batch_pcm(3, 2 * L, FS, channels=1, first=20 + htype)
    _run_calls(oracle, icw, cfg, graph.graph_master_only(), raw, [L, L], htype, n, channels=1)


@pytest.mark.parametrize("htype", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("ch", [1, 2])
def test_k5_576_frames(oracle, icw, htype, ch, monkeypatch):
    """one stream, one 576-frame launch block: the fused kernel's icw_iir_row_body<N, true>; twice"""
    _row(monkeypatch, stream1="1")
    n = _order(oracle, htype)
    cfg = graph.default_config(44100, channels=ch, hilbert_type=htype)
    raw = synth.batch_pcm(1, 1152, 44100, channels=ch, first=30 + htype)
    _run_calls(oracle, icw, cfg, graph.graph_master_only(), raw, [576, 576], htype, n, channels=ch)


def _pick_scale(htype, hist, n, phase, frames):
    """a power of two such that stream 0's first rejected sum under silence lands in [4N, frames - 4N):
    past the first speculative pair (and an odd order's lone leading block), well before the call's end.
    Until the first reject the recurrence is linear and a power of two scales every sum exactly, so one
    unscaled run of the Python restatement gives every |w|."""
    m = np.empty((frames, 4))
    for c in range(2):
        hil = _pyhil(htype, hist[c * 2][:n], hist[c * 2 + 1][:n], phase)
        assert hil.fi.subnorm_cnt == hil.fq.subnorm_cnt == 0
        for t in range(frames):
            hil.step(0.0)
            m[t, c * 2], m[t, c * 2 + 1] = abs(hil.fi.hist[0]), abs(hil.fq.hist[0])
        assert hil.fi.subnorm_cnt == hil.fq.subnorm_cnt == 0      # the unscaled run rejected nothing
    m = m.min(axis=1)
    head = m[:4 * n].min()
    e = int(np.floor(np.log2(head)))                              # 2^e <= every |w| before 4N
    assert m[4 * n:frames - 4 * n].min() < 2.0 ** e, "no dip inside the window"
    return 2.0 ** -e


def _pyhil(htype, hist_i, hist_q, phase):
    h = PyHilbert(htype, 1, 1)
    h.fi.hist, h.fq.hist, h.k = [float(v) for v in hist_i], [float(v) for v in hist_q], phase & 3
    return h


@pytest.mark.parametrize("htype", [1, 2])
def test_sums_dip_below_one_after_the_first_pair(oracle, icw, htype, monkeypatch):
    """Stream 0 falls silent with its states scaled down (in the state blob, by a power of two) so far
    that the first rejected sum comes after the first speculative pair of the call and well before its
    end: the pair that holds it fails its check and the exact blocks take over mid-launch.  Streams 1
    and 2 keep their states and stay speculative in the same wave pair.  Orders 19 (pairs) and 18."""
    n = _order(oracle, htype)
    cfg = graph.default_config(FS, hilbert_type=htype)
    nodes = graph.graph_master_only()
    S, L0, L1 = 3, 6 * n, 40 * n
    raw = synth.batch_pcm(S, L0 + L1, FS, first=40 + htype)
    x = raw.view(np.int16).reshape(S, L0 + L1, 2)
    x[0, L0:] = 0
    fsz = 4
    seg0 = np.ascontiguousarray(raw[:, :L0 * fsz])
    seg1 = np.ascontiguousarray(raw[:, L0 * fsz:])

    _row(monkeypatch)
    row = icw.Context(cfg, nodes, S)
    row.process(seg0, L0)
    blob0 = row.get_state(0)
    b = abi.StateBlob.from_buffer_copy(blob0)
    hist = np.ctypeslib.as_array(b.hist).copy()
    scale = _pick_scale(htype, hist, n, L0, L1)
    np.ctypeslib.as_array(b.hist)[:] = hist * scale
    blob = bytes(b) + blob0[len(bytes(b)):]
    row.set_state(0, blob)

    monkeypatch.setenv("ICW_K1_MODE", "plain")
    monkeypatch.setenv("ICW_RENDER", "serial")
    plain = icw.Context(cfg, nodes, S)
    plain.process(seg0, L0)
    plain.set_state(0, blob)

    out_r, pre_r = row.process(seg1, L1, want_pre=True)
    out_p, pre_p = plain.process(seg1, L1, want_pre=True)
    assert np.array_equal(pre_r.view(np.uint64), pre_p.view(np.uint64))
    assert np.array_equal(out_r, out_p)
    for s in range(S):
        assert row.meters(s) == plain.meters(s), s
    # w rows and reject counts of the silent stream against the Python restatement
    got = abi.StateBlob.from_buffer_copy(row.get_state(0))
    rejected = 0
    gh = np.ctypeslib.as_array(got.hist)
    for c in range(2):
        hil = _pyhil(htype, hist[c * 2][:n] * scale, hist[c * 2 + 1][:n] * scale, L0)
        for _ in range(L1):
            hil.step(0.0)
        for f, fil in enumerate((hil.fi, hil.fq)):
            want = np.array(fil.hist)
            assert np.array_equal(gh[c * 2 + f][:n].view(np.uint64), want.view(np.uint64)), (c, f)
            assert got.sncnt[c * 2 + f] - b.sncnt[c * 2 + f] == fil.subnorm_cnt, (c, f)
            rejected += fil.subnorm_cnt
    assert rejected > 0
    # the other streams ran on from their own states: the oracle's
    for s in (1, 2):
        ref = oracle.Stream(cfg, nodes)
        ref.process(seg0[s], L0)
        ro, rp = ref.process(seg1[s], L1, want_pre=True)
        assert np.array_equal(pre_r[s].view(np.uint64), rp.view(np.uint64)), s
        assert np.array_equal(out_r[s], ro), s
    row.close()
    plain.close()
