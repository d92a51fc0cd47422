"""The split dither generator across its chunk boundaries, rejected pairs included.

icw_launch_dither cuts a launch block into chunks of as many frames as a generator's row of tempered words
holds (icw_dith_chunk_frames); a block splits only from about 2^25 / W frames per call on (W words per
sample: RPDF and STPDF 2, TPDF 4, GAUSS 24), or from 2 731 generators on, where the rows stay at 1 024
GAUSS frames.  The cases below are the smallest shapes at which the sizing rule of size_scratch splits a
block; each asserts through icw_last_dither_chunks that the split happened, so a change of the rule
fails the case instead of silently leaving the path uncovered (re-derive the shape then).

What is compared: every stream of every case, bit for bit with the oracle -- the rendered bytes, the
meters, and the pre-render doubles where the frame-parallel render exports them.  Six or seven streams of a
case carry planted rejected dsopen pairs (tests/mtplant.py) at the chunk boundaries, handed to the context
through the state blob and to the oracle stream through set_mt after a short first call; before anything
is compared, the numpy model of the draws (mtplant.consumption), fed the very words handed over, must show
each pair consumed as a pair in the intended sample of the intended chunk.

The launch-block plan is pinned by ICW_BLOCK / ICW_FIRST_BLOCK / ICW_TAPER where the case names a block:
the main call is one 65 536-frame block and 4 096 frames more, so a second block starts from the state
the chunks left.  Cases e, f and h set no block switch: their calls are shorter than a default block (e, f),
or -- h, the c5fir configuration -- 100 000 frames, which plan_blocks keeps in uniform blocks (the 2 048-frame
first block and the 1.5 ramp need four blocks' worth of frames), so the call's first block is 65 536
frames and splits in four without ICW_FIRST_BLOCK.
"""
import ctypes as C
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth

import mtplant

pytestmark = pytest.mark.gpu

FS = 48000
L0 = 64                       # the short first call: the blob then holds a used generator state
BLOCK = 65536
EXTRA = 4096                  # frames past the first launch block
W_OF = {abi.RENDER_RPDF: 2, abi.RENDER_TPDF: 4, abi.RENDER_STPDF: 2, abi.RENDER_GAUSS: 24}
FIR_SHAPER, IIR_SHAPER = abi.NSHAPE_MEW44, 16
PIN = {"ICW_BLOCK": str(BLOCK), "ICW_FIRST_BLOCK": "0", "ICW_TAPER": "0"}

# name: render type, streams, first launch block, frames of the main call, environment, chunks stated
# (None: at least two), plants
CASES = {
    "a": (abi.RENDER_GAUSS, 64, BLOCK, BLOCK + EXTRA, PIN, 4, (1, 2, 3, 4, 5, 6, 7)),
    "b": (abi.RENDER_TPDF, 160, BLOCK, BLOCK + EXTRA, PIN, 2, (1, 2, 3, 4, 5, 7)),
    "c": (abi.RENDER_STPDF, 288, BLOCK, BLOCK + EXTRA, PIN, 2, (1, 2, 3, 4, 5, 7)),
    "d": (abi.RENDER_RPDF, 288, BLOCK, BLOCK + EXTRA, PIN, 2, (1, 2, 3, 4, 5, 7)),
    "e": (abi.RENDER_GAUSS, 1366, 6000, 6000, {}, 6, ()),
    "f": (abi.RENDER_STPDF, 1366, 12800, 12800, {}, 2, (1, 2, 3, 4, 5, 7)),
    "g": (abi.RENDER_GAUSS, 64, BLOCK, BLOCK + EXTRA, dict(PIN, ICW_RENDER="serial"), 4, (1, 2, 3, 4, 5, 7)),
    "h": (abi.RENDER_GAUSS, 64, BLOCK, 100000, {}, None, ()),
}


def chunk_rule(n_streams, block, W):
    """size_scratch's rows and icw_dith_chunk_frames, restated: the case's shape is derived from it, and the
    accessor must report the same after the real call"""
    G = 2 * n_streams
    cap = max((1 << 26) // G, 24 * 1024)
    cap = min(cap, 24 * (block + 1))
    cap = (cap + 3) & ~3
    return min(block, cap // W)


def plant_specs(kind, c, block, chunks, W, ch):
    """-> (samples, chunks of them, straddle): the samples whose draw is to consume a rejected pair.  The L
    and R generators of a stream reject different pairs of a sample where it has more than one."""
    last = (chunks - 1) * c - 1 if chunks == 4 else block - 1          # a, g: the last sample of chunk 2
    mid = c + (min(2 * c, block) - c) // 2
    return {1: ([c - 1], [0], False), 2: ([c], [1], False), 3: ([mid], [1], False), 4: (None, [1], True),
            5: ([last], [last // c], False), 6: ([block - 1], [chunks - 1], False),
            7: ([c - 1, c], [0, 1], False)}[kind]


def make_plant(kind, words, idx, c, block, chunks, W, ch, n_main):
    """-> (words, idx, samples, chunks): the planted state of one generator and where its pairs are to be
    consumed"""
    samples, chk, straddle = plant_specs(kind, c, block, chunks, W, ch)
    pair = 0 if ch == 0 else W - 2                      # word offset of the rejected pair inside the sample
    if straddle:
        assert idx < 623
        idx |= 1                                        # pairs are aligned to the call's start: an odd index
        off = W * (c + 10)                              # puts words 623 | 0 into one pair
        off += (623 - (idx + off)) % 624
        assert off % 2 == 0 and (idx + off) % 624 == 623
        w = mtplant.plant(words, idx, [off, off + 1])
        samples = [off // W]
    else:
        off = W * samples[0] + pair
        w = mtplant.plant(words, idx, [off, off + 1])
        if len(samples) == 2:
            # the sample that opens chunk 1 after the shift: its first pair, where the model says it starts
            _, starts = mtplant.consumption(w, idx, W, samples[1] + 1)
            off2 = int(starts[samples[1]])
            assert off2 == W * samples[1] + 2
            w = mtplant.plant(words, idx, [off, off + 1, off2, off2 + 1])
    rej, _ = mtplant.consumption(w, idx, W, min(n_main, max(samples) + 8))
    assert [t for t, _ in rej] == samples, f"plant {kind}: pairs consumed in {rej}, wanted samples {samples}"
    assert all(o % 2 == 0 for _, o in rej)
    assert [t // c for t in samples] == chk, f"plant {kind}: samples {samples} not in chunks {chk} of {c}"
    return w, idx, samples, chk


_PLANTS = {}


def run_case(oracle, icw, monkeypatch, name, nshape, calls=None, fir=None):
    rtype, S, block, n_main, env, want_chunks, kinds = CASES[name]
    W = W_OF[rtype]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t_start = time.time()
    cfg = graph.default_config(FS, fmt=abi.FMT_I16, channels=2, hilbert_type=0)
    cfg.render.render_type, cfg.render.nshape_type, cfg.render.dth_bits = rtype, nshape, 1.5
    nodes = graph.graph_master_only()
    flat = nshape == abi.NSHAPE_FLAT
    l0 = L0 if kinds else 0
    nw = synth.cpu_workers()
    raw = synth.batch_pcm(S, l0 + n_main, FS, workers=nw)
    c = chunk_rule(S, block, W)
    chunks = -(-block // c)
    assert chunks >= 2 and (want_chunks is None or chunks == want_chunks), \
        f"case {name}: the sizing rule gives {chunks} chunks of {c}: it has moved, re-derive the shape"
    ctx = icw.Context(cfg, nodes, S)
    if fir:
        ctx.set_fir_hilbert(*fir)
    fsz = ctx.fsz
    outs, pres = [], []
    if l0:
        o, p = ctx.process(np.ascontiguousarray(raw[:, :l0 * fsz]), l0, want_pre=flat)
        outs.append(o)
        pres.append(p)
        assert ctx.last_dither_chunks() == (1, l0)
    # the plants: stream ids[j] takes kind j in its L generator and another kind in its R generator
    ids = [(3 + 37 * j) % S for j in range(len(kinds))]
    assert len(set(ids)) == len(ids)
    planted = {}
    for j, s in enumerate(ids):
        full = ctx.get_state(s)
        blob = abi.StateBlob.from_buffer_copy(full)
        assert blob.has_render == 1
        for ch in range(2):
            kind = kinds[(j + 3 * ch) % len(kinds)]
            words = np.frombuffer(bytes(blob.mt[ch]), dtype=np.uint32).copy()
            # (a case's runs share their plants: the state after the short first call is the seed's)
            key = (name, s, ch, words.tobytes(), int(blob.mt_idx[ch]))
            if key not in _PLANTS:
                _PLANTS[key] = make_plant(kind, words, int(blob.mt_idx[ch]), c, block, chunks, W, ch, n_main)
            w, idx, samples, chk = _PLANTS[key]
            C.memmove(C.addressof(blob.mt[ch]), w.ctypes.data, 624 * 4)
            blob.mt_idx[ch] = idx
            planted[(s, ch)] = (w, idx)
        ctx.set_state(s, bytes(blob) + full[C.sizeof(blob):])
    # the main call, whole or in two calls
    t = l0
    reported = []
    for n in (calls or [n_main]):
        o, p = ctx.process(np.ascontiguousarray(raw[:, t * fsz:(t + n) * fsz]), n, want_pre=flat)
        outs.append(o)
        pres.append(p)
        reported.append(ctx.last_dither_chunks())
        t += n
    assert t == l0 + n_main
    got_chunks, got_c = reported[0]
    assert got_c == c, f"case {name}: the accessor reports chunks of {got_c}, the rule restated here gives {c}"
    if calls:
        assert got_chunks >= 2 and got_chunks == -(-min(calls[0], block) // c)
    else:
        assert got_chunks == chunks
    out = np.concatenate(outs, axis=1)
    pre = np.concatenate(pres, axis=1) if flat else None
    meters = [ctx.meters(s) for s in range(S)]
    ctx.close()
    t_gpu = time.time()

    def check(s):
        st = oracle.Stream(cfg, nodes)
        if fir:
            st.set_fir(*fir)
        parts = []
        if l0:
            parts.append(st.process(raw[s, :l0 * fsz], l0, want_pre=flat))
        for ch in range(2):
            if (s, ch) in planted:
                st.set_mt(ch, *planted[(s, ch)])
        parts.append(st.process(raw[s, l0 * fsz:], n_main, want_pre=flat))
        ref = np.concatenate([q[0] for q in parts])
        bad = np.flatnonzero(out[s] != ref)
        if bad.size:
            return f"stream {s}: {bad.size} output bytes differ, first in frame {bad[0] // 4 - l0} of the main call"
        if flat:
            rp = np.concatenate([q[1] for q in parts])
            badp = np.flatnonzero(pre[s].view(np.uint64) != rp.view(np.uint64))
            if badp.size:
                return f"stream {s}: {badp.size} pre-render doubles differ, first at {badp[:4]}"
        if meters[s] != st.meters():
            return f"stream {s}: meters {meters[s]} != oracle {st.meters()}"
        return None

    with ThreadPoolExecutor(nw) as pool:
        errs = [e for e in pool.map(check, range(S)) if e]
    print(f"\ncase {name} nshape {nshape} calls {calls or [n_main]}: {S} streams, first block {block}: "
          f"{reported} (chunks, chunk frames) per call; gpu side {t_gpu - t_start:.1f} s, oracle "
          f"{time.time() - t_gpu:.1f} s")
    assert not errs, f"case {name}: {len(errs)} of {S} streams differ: {errs[:4]}"


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
@pytest.mark.parametrize("nshape", [FIR_SHAPER, abi.NSHAPE_FLAT])
def test_chunks_both_renders(oracle, icw, monkeypatch, name, nshape):
    """a noise shaper: the row render K3c over generator-major rows; NSHAPE_FLAT: the frame-parallel render
    inside K2, the pre-render doubles compared too"""
    run_case(oracle, icw, monkeypatch, name, nshape)


def test_chunks_iir_shaper(oracle, icw, monkeypatch):
    run_case(oracle, icw, monkeypatch, "a", IIR_SHAPER)


def test_floor_regime_time_major_gauss(oracle, icw, monkeypatch):
    """e: 2 732 generators, rows of 24 576 words: chunks of 1 024 GAUSS frames, five and one of 880; the
    default render above 2 048 channels is the lane-per-channel K3b over time-major rows"""
    run_case(oracle, icw, monkeypatch, "e", FIR_SHAPER)


def test_floor_regime_time_major_stpdf(oracle, icw, monkeypatch):
    """f: the same rows hold 12 288 STPDF frames; the prev_rnd hand-off and the plants over time-major rows"""
    run_case(oracle, icw, monkeypatch, "f", FIR_SHAPER)


def test_time_major_small_batch(oracle, icw, monkeypatch):
    """g: ICW_RENDER=serial, K3b's time-major rows with case a's chunks"""
    run_case(oracle, icw, monkeypatch, "g", FIR_SHAPER)


def test_fir_converter_plan(oracle, icw, monkeypatch):
    """h: the c5fir configuration (FIR converter 254 / 8.0, GAUSS, a shaper, 64 streams), no switch set"""
    run_case(oracle, icw, monkeypatch, "h", FIR_SHAPER, fir=(254, 8.0))


@pytest.mark.parametrize("name,nshape,first", [("a", FIR_SHAPER, 2 * 21845 + 100), ("c", abi.NSHAPE_FLAT, 58254 + 3000),
                                               ("f", FIR_SHAPER, 12288 + 200)])
def test_chunks_two_calls(oracle, icw, monkeypatch, name, nshape, first):
    """the main call cut in two, the second starting part-way into a chunk of the one-call run: the state
    carries across calls as across blocks.  The first call still splits (asserted), the plants stay
    where they were, so those past the cut are consumed wherever the second call's chunks put them."""
    n_main = CASES[name][3]
    run_case(oracle, icw, monkeypatch, name, nshape, calls=[first, n_main - first])
