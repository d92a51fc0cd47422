"""GPU: icw_transcode_files_pool -- a fixed pool of stream slots, a slot re-initialised and refilled with the next
file of the queue as its file ends -- against the oracle (one oracle.Stream per file) and against
icw_transcode_files_lists on the same files: all three byte for byte, header included, whatever the slots, the
order and the neighbours are.  A slot that kept any piece of its last file's state (converter rings, bus, frame
counter, generator words, shaper rings, meters) changes the next file's first frames or its meters."""
import numpy as np
import pytest

from in_cwave_amd import abi, cwave, graph, synth
from in_cwave_amd import lib as L

import wavgen as W

pytestmark = pytest.mark.gpu

B = 256
LENGTHS = (2, 255, 256, 257, 700, 1000, 512)             # every edge of a 256-frame block
INPUTS = ((abi.FMT_I16, 2, 44100), (abi.FMT_F32, 1, 48000), (abi.FMT_I24, 2, 96000), (abi.FMT_U8, 1, 48000))
FADE = 2


def encode(sig, fmt):
    """[frames, channels] doubles in -1 .. 1 as interleaved samples of a real input format"""
    if fmt == abi.FMT_I16:
        return np.clip(np.round(sig * 32767.0), -32768, 32767).astype("<i2").reshape(-1).view(np.uint8)
    if fmt == abi.FMT_F32:
        return sig.astype("<f4").reshape(-1).view(np.uint8)
    if fmt == abi.FMT_I24:
        q = np.clip(np.round(sig * 8388607.0), -8388608, 8388607).astype("<i4").reshape(-1)
        return np.ascontiguousarray(q.view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)
    assert fmt == abi.FMT_U8
    return np.clip(np.round(sig * 127.0) + 128, 0, 255).astype(np.uint8).reshape(-1)


def loud_pcm(seed, n, fs, ch, fmt):
    """two sines near full scale each, hard-limited: the modulated sum clips the render"""
    rng = np.random.default_rng(5000 + seed)
    t = np.arange(n, dtype=np.float64) / fs
    sig = np.zeros((n, ch))
    for c in range(ch):
        f, ph = rng.uniform(200.0, 0.3 * fs, size=2), rng.uniform(0, 2 * np.pi, size=2)
        sig[:, c] = np.clip(0.98 * np.sin(2 * np.pi * f[0] * t + ph[0]) + 0.98 * np.sin(2 * np.pi * f[1] * t + ph[1]), -1, 1)
    return encode(sig, fmt)


def shaped_cfg():
    """24-bit TPDF + MEW44: a slot's generator words and shaper rings must start again with every file"""
    cfg = graph.default_config(48000, need24bits=True)
    cfg.render.render_type = abi.RENDER_TPDF
    cfg.render.nshape_type = abi.NSHAPE_MEW44
    return cfg


def zero_pad(fmt, ch, frames):
    return np.full(frames * abi.FMT_BYTES[fmt] * ch, 0x80 if fmt == abi.FMT_U8 else 0, np.uint8)


def oracle_file(oracle, cfg0, nodes, fmt, ch, fs, n, data, fade, sec_align=0, block=0):
    """the file's expected image (44-byte header + total frames) and, with block > 0, the meters once the whole
    last block -- the zero sample beyond `total` -- has gone through, as the pool reads them"""
    c = graph.default_config(fs, fmt=fmt, channels=ch, need24bits=bool(cfg0.need24bits))
    c.render = cfg0.render
    total = n + ((fs * sec_align - n % (fs * sec_align)) % (fs * sec_align) if sec_align else 0)
    s = oracle.Stream(c, nodes)
    s.open(n, fade, fade, sec_align)
    ref, _ = s.process(np.concatenate([data, zero_pad(fmt, ch, total - n)]), total)
    meters = None
    if block:
        rest = -total % block
        if rest:
            s.process(zero_pad(fmt, ch, rest), rest)
        meters = s.meters()
    osz = 6 if cfg0.need24bits else 4
    hdr = (b"RIFF" + (36 + total * osz).to_bytes(4, "little") + b"WAVEfmt " + (16).to_bytes(4, "little") +
           (1).to_bytes(2, "little") + (2).to_bytes(2, "little") + fs.to_bytes(4, "little") +
           (fs * osz).to_bytes(4, "little") + osz.to_bytes(2, "little") + (4 * osz).to_bytes(2, "little") +
           b"data" + (total * osz).to_bytes(4, "little"))
    return hdr + ref.tobytes(), total, meters


class Library:
    """the seven files of the edge test: written once, with the oracle's images and meters and the bytes
    icw_transcode_files_lists writes for them; nothing here changes afterwards"""

    def __init__(self, root, oracle, loud):
        self.cfg = shaped_cfg()
        self.ins, self.lists, self.want, self.totals, self.meters = [], [], [], [], []
        for i, n in enumerate(LENGTHS):
            fmt, ch, fs = INPUTS[i % len(INPUTS)]
            d = loud_pcm(i, n, fs, ch, fmt) if loud else synth.stream_pcm(i, n, fs, channels=ch, fmt=fmt)
            path = root / f"in_{i}.wav"
            W.write(path, d, fmt, ch, fs, kind="float" if fmt == abi.FMT_F32 else "pcm")
            nodes = graph.graph_pm_shift_mix() if i == 4 else [graph.master(inputs=("A",)), graph.shift(out="A", fr=1.5 + 2.25 * i)]
            img, total, m = oracle_file(oracle, self.cfg, nodes, fmt, ch, fs, n, d, FADE, block=B)
            self.ins.append(path)
            self.lists.append(nodes)
            self.want.append(img)
            self.totals.append(total)
            self.meters.append(m)
        outs = [root / f"lists_{i}.wav" for i in range(len(LENGTHS))]
        rc, _, status = L.transcode_files_lists(self.cfg, self.lists, self.ins, outs, fade_in_ms=FADE, fade_out_ms=FADE,
                                                block_frames=B)
        assert rc == abi.OK and status == [abi.OK] * len(LENGTHS)
        for i, o in enumerate(outs):
            assert o.read_bytes() == self.want[i], f"icw_transcode_files_lists against the oracle, file {i}"

    def pool(self, out_dir, tag, **kw):
        outs = [out_dir / f"{tag}_{i}.wav" for i in range(len(LENGTHS))]
        rc, st, status, meters = L.transcode_files_pool(self.cfg, self.lists, self.ins, outs, fade_in_ms=FADE,
                                                        fade_out_ms=FADE, block_frames=B, **kw)
        assert rc == abi.OK and status == [abi.OK] * len(LENGTHS)
        return st, [o.read_bytes() for o in outs], meters


@pytest.fixture(scope="module")
def library(tmp_path_factory, oracle):
    return Library(tmp_path_factory.mktemp("pool_lib"), oracle, loud=False)


@pytest.mark.parametrize("order", [abi.POOL_AS_GIVEN, abi.POOL_LONGEST_FIRST])
def test_refill_at_every_edge(tmp_path, library, order):
    st, got, _ = library.pool(tmp_path, "p", slots=3, order=order)
    for i, g in enumerate(got):
        assert g == library.want[i], f"file {i} ({LENGTHS[i]} frames)"
    rc, _, _, plan = L.pool_plan(library.totals, 3, B, order)
    assert rc == abi.OK and st.refills == 4 == plan.refills and st.slots == 3
    assert (st.blocks, st.slot_blocks, st.busy_slot_blocks) == (plan.blocks, plan.slot_blocks, plan.busy_slot_blocks)
    assert st.busy_slot_blocks == sum(-(-n // B) for n in LENGTHS) and st.slot_blocks == 3 * st.blocks
    assert st.batch.n_files == 7 and st.batch.n_groups == 1
    assert st.batch.frames_in == sum(LENGTHS) == st.batch.frames_out


def test_one_slot_and_one_slot_per_file(tmp_path, library):
    """slots = 1: every file after the first runs in a reused slot, on the one-stream path; slots = 0: no refill"""
    st, got, _ = library.pool(tmp_path, "one", slots=1)
    assert got == library.want
    assert st.slots == 1 and st.refills == 6 and st.blocks == st.slot_blocks == st.busy_slot_blocks == sum(-(-n // B) for n in LENGTHS)
    st, got, _ = library.pool(tmp_path, "all", slots=0)
    assert got == library.want
    assert st.slots == 7 and st.refills == 0 and st.blocks == -(-max(LENGTHS) // B)
    st, got, _ = library.pool(tmp_path, "wide", slots=64, want_meters=False)
    assert got == library.want and st.slots == 7 and st.refills == 0


def test_bus_state_does_not_leak(tmp_path, oracle):
    """five self-feeding Mix -> Master lists, each with its own feedback gain, on 2 slots: a bus slot that
    survives the refill changes the next file's first frames"""
    fs, lengths, gains = 44100, (700, 300, 513, 256, 900), (0.5, 0.9, 0.7, 0.85, 0.6)
    cfg = graph.default_config(48000)
    ins, lists, want = [], [], []
    for i, (n, g) in enumerate(zip(lengths, gains)):
        d = loud_pcm(20 + i, n, fs, 2, abi.FMT_I16)
        W.write(tmp_path / f"in_{i}.wav", d, abi.FMT_I16, 2, fs, kind="pcm")
        nodes = [graph.master(inputs=("C",)), graph.mix(inputs=("in", "C"), out="C", gain=g)]
        assert L.graph_form(cfg, nodes) == 1
        ins.append(tmp_path / f"in_{i}.wav")
        lists.append(nodes)
        want.append(oracle_file(oracle, cfg, nodes, abi.FMT_I16, 2, fs, n, d, FADE)[0])
    ref = [tmp_path / f"l_{i}.wav" for i in range(5)]
    rc, _, status = L.transcode_files_lists(cfg, lists, ins, ref, fade_in_ms=FADE, fade_out_ms=FADE, block_frames=B)
    assert rc == abi.OK and status == [abi.OK] * 5
    for order in (abi.POOL_AS_GIVEN, abi.POOL_LONGEST_FIRST):
        outs = [tmp_path / f"p{order}_{i}.wav" for i in range(5)]
        rc, st, status, _ = L.transcode_files_pool(cfg, lists, ins, outs, slots=2, order=order, fade_in_ms=FADE,
                                                   fade_out_ms=FADE, block_frames=B)
        assert rc == abi.OK and status == [abi.OK] * 5 and st.refills == 3 and st.batch.n_groups == 1
        for i in range(5):
            assert outs[i].read_bytes() == want[i] == ref[i].read_bytes(), f"file {i}, order {order}"


def test_cwave_pool(tmp_path, oracle):
    """six CWAVE files in the four frame formats, mono and stereo, at two rates, on 2 slots -- and a WAV beside
    them, which runs in the pool of its own kind"""
    specs = [(abi.FMT_CW_F64, 2, 2000, 600), (abi.FMT_CW_I16, 1, 3000, 257), (abi.FMT_CW_I16_F32, 2, 3000, 512),
             (abi.FMT_CW_F32, 1, 2000, 900), (abi.FMT_CW_I16, 2, 2000, 255), (abi.FMT_CW_F64, 1, 3000, 400)]
    cfg = graph.default_config(48000)
    cfg.render.render_type = abi.RENDER_TPDF
    ins, lists, want = [], [], []
    for i, (fmt, ch, fs, n) in enumerate(specs):
        d = synth.stream_cwave(i, n, fs, channels=ch, fmt=fmt)
        (tmp_path / f"in_{i}.cwave").write_bytes(cwave.make_image(d, fmt, ch, fs).tobytes())
        nodes = [graph.master(inputs=("A",)), graph.shift(out="A", fr=-3.0 + 1.75 * i)]
        ins.append(tmp_path / f"in_{i}.cwave")
        lists.append(nodes)
        want.append(oracle_file(oracle, cfg, nodes, fmt, ch, fs, n, d, FADE)[0])
    d = synth.stream_pcm(40, 300, 3000, channels=2, fmt=abi.FMT_I16)
    W.write(tmp_path / "in_6.wav", d, abi.FMT_I16, 2, 3000, kind="pcm")
    ins.append(tmp_path / "in_6.wav")
    lists.append(graph.graph_shift_master())
    want.append(oracle_file(oracle, cfg, lists[-1], abi.FMT_I16, 2, 3000, 300, d, FADE)[0])
    ref = [tmp_path / f"l_{i}.wav" for i in range(7)]
    rc, _, status = L.transcode_files_lists(cfg, lists, ins, ref, fade_in_ms=FADE, fade_out_ms=FADE, block_frames=B)
    assert rc == abi.OK and status == [abi.OK] * 7
    outs = [tmp_path / f"p_{i}.wav" for i in range(7)]
    rc, st, status, _ = L.transcode_files_pool(cfg, lists, ins, outs, slots=2, fade_in_ms=FADE, fade_out_ms=FADE, block_frames=B)
    assert rc == abi.OK and status == [abi.OK] * 7
    assert st.batch.n_groups == 2 and st.slots == 2 and st.refills == 4       # the CWAVE pool's; the WAV's pool has one slot
    for i in range(7):
        assert outs[i].read_bytes() == want[i] == ref[i].read_bytes(), f"file {i}"


def test_ragged_width(tmp_path, oracle):
    """150 files of 300 .. 3 000 frames on 70 slots: one full wave and a partial one, many refills per boundary"""
    rng = np.random.default_rng(150)
    lengths = [int(v) for v in rng.integers(300, 3001, size=150)]
    kinds = ((abi.FMT_I16, 2, 44100), (abi.FMT_F32, 1, 48000))
    cfg = graph.default_config(48000)
    ins, lists, want = [], [], []
    for i, n in enumerate(lengths):
        fmt, ch, fs = kinds[i % 2]
        d = synth.stream_pcm(100 + i, n, fs, channels=ch, fmt=fmt)
        W.write(tmp_path / f"in_{i}.wav", d, fmt, ch, fs, kind="float" if fmt == abi.FMT_F32 else "pcm")
        nodes = [graph.master(inputs=("A",)), graph.shift(out="A", fr=0.5 + 0.125 * i)]
        ins.append(tmp_path / f"in_{i}.wav")
        lists.append(nodes)
        want.append(oracle_file(oracle, cfg, nodes, fmt, ch, fs, n, d, FADE)[0])
    ref = [tmp_path / f"l_{i}.wav" for i in range(150)]
    rc, _, status = L.transcode_files_lists(cfg, lists, ins, ref, fade_in_ms=FADE, fade_out_ms=FADE, block_frames=1024,
                                            merge_inputs=True)
    assert rc == abi.OK and status == [abi.OK] * 150
    outs = [tmp_path / f"p_{i}.wav" for i in range(150)]
    rc, st, status, _ = L.transcode_files_pool(cfg, lists, ins, outs, slots=70, fade_in_ms=FADE, fade_out_ms=FADE,
                                               block_frames=1024, want_meters=False)
    assert rc == abi.OK and status == [abi.OK] * 150
    _, _, _, plan = L.pool_plan(lengths, 70, 1024, abi.POOL_AS_GIVEN)
    assert st.slots == 70 and st.refills == 80 and st.blocks == plan.blocks and st.busy_slot_blocks == plan.busy_slot_blocks
    for i in range(150):
        assert outs[i].read_bytes() == want[i] == ref[i].read_bytes(), f"file {i} ({lengths[i]} frames)"


def test_failures_in_the_queue(tmp_path, oracle):
    """a broken header at position 2 of 6 and a file cut short of the 900 frames its header claims at position 4:
    both refused, the other four complete, and the call returns the file error as icw_transcode_files_lists does"""
    fs, lengths = 44100, (600, 300, 500, 257, 900, 800)
    cfg = graph.default_config(48000)
    ins, lists, want = [], [], []
    for i, n in enumerate(lengths):
        d = synth.stream_pcm(60 + i, n, fs, channels=2, fmt=abi.FMT_I16)
        img = W.wav_bytes(d, abi.FMT_I16, 2, fs, kind="pcm")
        if i == 2:
            img = b"RIFX" + bytes(img[4:])
        if i == 4:
            img = bytes(img[:44 + 400 * 4])
        (tmp_path / f"in_{i}.wav").write_bytes(bytes(img))
        nodes = [graph.master(inputs=("A",)), graph.shift(out="A", fr=2.0 + i)]
        ins.append(tmp_path / f"in_{i}.wav")
        lists.append(nodes)
        want.append(oracle_file(oracle, cfg, nodes, abi.FMT_I16, 2, fs, n, d, FADE)[0])
    ref = [tmp_path / f"l_{i}.wav" for i in range(6)]
    rc_l, _, status_l = L.transcode_files_lists(cfg, lists, ins, ref, fade_in_ms=FADE, fade_out_ms=FADE, block_frames=B)
    outs = [tmp_path / f"p_{i}.wav" for i in range(6)]
    rc, st, status, meters = L.transcode_files_pool(cfg, lists, ins, outs, slots=2, fade_in_ms=FADE, fade_out_ms=FADE,
                                                    block_frames=B)
    assert status[2] != abi.OK and status[4] != abi.OK and [status[i] for i in (0, 1, 3, 5)] == [abi.OK] * 4
    assert status == status_l and rc == rc_l != abi.OK
    assert st.batch.n_files == 4 and st.slots == 2 and st.refills == 2          # the refused files took no slot
    for i in (0, 1, 3, 5):
        assert outs[i].read_bytes() == want[i] == ref[i].read_bytes(), f"file {i}"
    assert meters[2] == meters[4] == {"clips": (0, 0), "peak_db": (0.0, 0.0), "desubnorm": 0}


def test_meters_per_file(tmp_path, oracle):
    """input loud enough to clip: meters[i] are the oracle stream's, and the file that follows in the same slot
    does not inherit them"""
    lib = Library(tmp_path, oracle, loud=True)
    assert sum(sum(m["clips"]) > 0 for m in lib.meters) >= 4 and len({m["clips"] for m in lib.meters}) >= 4
    for order in (abi.POOL_AS_GIVEN, abi.POOL_LONGEST_FIRST):
        st, got, meters = lib.pool(tmp_path, f"m{order}", slots=3, order=order)
        assert got == lib.want
        for i, (m, r) in enumerate(zip(meters, lib.meters)):
            assert m["clips"] == r["clips"] and m["peak_db"] == r["peak_db"] and m["desubnorm"] == r["desubnorm"], (i, order, m, r)
    # longest first, file 3 follows file 6 in slot 2 and file 0 follows file 2 in slot 1 (the plan): the two that
    # follow do not clip, the two before them do
    _, slot, start, _ = L.pool_plan(lib.totals, 3, B, abi.POOL_LONGEST_FIRST)
    assert slot[3] == slot[6] and start[3] > start[6] and slot[0] == slot[2] and start[0] > start[2]
    assert lib.meters[0]["clips"] == lib.meters[3]["clips"] == (0, 0)
    assert sum(lib.meters[6]["clips"]) > 0 and sum(lib.meters[2]["clips"]) > 0


def test_sec_align_tails(tmp_path, oracle):
    """sec_align = 1 on three short files of different rates on 2 slots: every tail is the file's own, at its
    rate, and a slot stays busy through its tail"""
    specs = [(abi.FMT_I16, 2, 2000, 700), (abi.FMT_F32, 1, 3000, 3100), (abi.FMT_I16, 1, 2500, 2500)]
    cfg = graph.default_config(48000)
    ins, lists, want, totals = [], [], [], []
    for i, (fmt, ch, fs, n) in enumerate(specs):
        d = synth.stream_pcm(80 + i, n, fs, channels=ch, fmt=fmt)
        W.write(tmp_path / f"in_{i}.wav", d, fmt, ch, fs, kind="float" if fmt == abi.FMT_F32 else "pcm")
        nodes = [graph.master(inputs=("A",)), graph.shift(out="A", fr=3.0 + i)]
        img, total, _ = oracle_file(oracle, cfg, nodes, fmt, ch, fs, n, d, FADE, sec_align=1)
        ins.append(tmp_path / f"in_{i}.wav")
        lists.append(nodes)
        want.append(img)
        totals.append(total)
    assert totals == [2000, 6000, 2500]
    ref = [tmp_path / f"l_{i}.wav" for i in range(3)]
    rc, _, status = L.transcode_files_lists(cfg, lists, ins, ref, fade_in_ms=FADE, fade_out_ms=FADE, sec_align=1, block_frames=B)
    assert rc == abi.OK and status == [abi.OK] * 3
    outs = [tmp_path / f"p_{i}.wav" for i in range(3)]
    rc, st, status, _ = L.transcode_files_pool(cfg, lists, ins, outs, slots=2, fade_in_ms=FADE, fade_out_ms=FADE, sec_align=1,
                                               block_frames=B)
    assert rc == abi.OK and status == [abi.OK] * 3
    for i in range(3):
        assert outs[i].read_bytes() == want[i] == ref[i].read_bytes(), f"file {i}"
    # file 2 waits for slot 0 until file 0's tail is through: block ceil(2000 / 256) = 8
    _, slot, start, plan = L.pool_plan(totals, 2, B, abi.POOL_AS_GIVEN)
    assert (slot[2], start[2]) == (0, 8)
    assert st.busy_slot_blocks == sum(-(-t // B) for t in totals) == plan.busy_slot_blocks and st.blocks == plan.blocks == 24
    assert st.batch.frames_in == 700 + 3100 + 2500 and st.batch.frames_out == sum(totals)
