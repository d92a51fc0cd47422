"""GPU: icw_transcode_files_jobs -- the pool of stream slots with every file's own job: its list, its render and
depth, its Hilbert converter -- against the oracle (one oracle.Stream per file, made with the job's config) and
against icw_transcode_files_lists called for that file alone with that config: all three byte for byte, the
44-byte header at the file's own depth included, whatever the slots, the order and the neighbours are.  Meters are
the oracle stream's, against the stream's own bound.  Nothing here has a tolerance."""
import numpy as np
import pytest

from in_cwave_amd import abi, cwave, graph, synth
from in_cwave_amd import lib as L

import wavgen as W

pytestmark = pytest.mark.gpu

B = 256
LENGTHS = (2, 255, 256, 257, 700, 1000, 512, 300, 513, 256, 900, 257)     # every edge of a 256-frame block, 12 files
INPUTS = ((abi.FMT_I16, 2, 44100), (abi.FMT_F32, 1, 48000), (abi.FMT_I24, 2, 96000), (abi.FMT_U8, 1, 48000))
FADE = 2


def job_cfg(hilbert, render_type, nshape, need24):
    """a config that carries a job's settings: hilbert = (type, kahan, reject)"""
    cfg = graph.default_config(48000, need24bits=bool(need24), hilbert_type=hilbert[0])
    cfg.iir_kahan, cfg.iir_subnorm_reject = hilbert[1], hilbert[2]
    cfg.render.render_type, cfg.render.nshape_type = render_type, nshape
    return cfg


# two Hilbert settings x renders that cover every output path, and a third setting: K2's in-kernel render when alone
# and KR when mixed; the serial run; dithered and frame-parallel; 24-bit ROUND
CLASSES = (
    lambda: job_cfg((1, 1, 1), abi.RENDER_ROUND, abi.NSHAPE_FLAT, 0),
    lambda: job_cfg((1, 1, 1), abi.RENDER_TPDF, abi.NSHAPE_MEW44, 1),
    lambda: job_cfg((0, 0, 0), abi.RENDER_TPDF, abi.NSHAPE_FLAT, 0),
    lambda: job_cfg((4, 1, 1), abi.RENDER_ROUND, abi.NSHAPE_FLAT, 1),
)


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
    rng = np.random.default_rng(7000 + seed)
    t = np.arange(n, dtype=np.float64) / fs
    sig = np.zeros((n, ch))
    for c in range(ch):
        f, ph = rng.uniform(200.0, 0.3 * fs, size=2), rng.uniform(0, 2 * np.pi, size=2)
        sig[:, c] = np.clip(0.98 * np.sin(2 * np.pi * f[0] * t + ph[0]) + 0.98 * np.sin(2 * np.pi * f[1] * t + ph[1]), -1, 1)
    return encode(sig, fmt)


def zero_pad(fmt, ch, frames):
    return np.full(frames * abi.FMT_BYTES[fmt] * ch, 0x80 if fmt == abi.FMT_U8 else 0, np.uint8)


def oracle_file(oracle, jc, nodes, fmt, ch, fs, n, data, block=B):
    """the file's expected image (44-byte header at the job's depth + n frames) from a fresh oracle stream with the
    job's config jc, and the meters once the whole last block -- the zero sample beyond n -- has gone through, as
    the pool reads them"""
    c = graph.default_config(fs, fmt=fmt, channels=ch, need24bits=bool(jc.need24bits), hilbert_type=jc.hilbert_type)
    c.iir_kahan, c.iir_subnorm_reject, c.render = jc.iir_kahan, jc.iir_subnorm_reject, jc.render
    s = oracle.Stream(c, nodes)
    s.open(n, FADE, FADE, 0)
    ref, _ = s.process(data, n)
    rest = -n % block
    if rest:
        s.process(zero_pad(fmt, ch, rest), rest)
    osz = 6 if jc.need24bits else 4
    hdr = (b"RIFF" + (36 + n * osz).to_bytes(4, "little") + b"WAVEfmt " + (16).to_bytes(4, "little") +
           (1).to_bytes(2, "little") + (2).to_bytes(2, "little") + fs.to_bytes(4, "little") +
           (fs * osz).to_bytes(4, "little") + osz.to_bytes(2, "little") + (4 * osz).to_bytes(2, "little") +
           b"data" + (n * osz).to_bytes(4, "little"))
    return hdr + ref.tobytes(), s.meters()


def lists_alone(root, tag, jc, nodes, path):
    """what icw_transcode_files_lists writes for the file alone with the job's config"""
    out = root / f"{tag}.wav"
    rc, _, status = L.transcode_files_lists(jc, [nodes], [path], [out], fade_in_ms=FADE, fade_out_ms=FADE, block_frames=B)
    assert rc == abi.OK and status == [abi.OK]
    return out.read_bytes()


class Files:
    """a set of input files with their jobs, the oracle's images and meters, and the bytes of the lists entry for
    each file alone: made once, never changed"""

    def __init__(self):
        self.cfg = graph.default_config(48000)            # what stays context-wide; its own render and converter are not read
        self.ins, self.nodes, self.cfgs, self.jobs, self.want, self.meters, self.lens = [], [], [], [], [], [], []

    def add(self, root, oracle, path, data, fmt, ch, fs, n, jc, nodes):
        img, m = oracle_file(oracle, jc, nodes, fmt, ch, fs, n, data)
        i = len(self.ins)
        assert lists_alone(root, f"alone_{i}", jc, nodes, path) == img, f"icw_transcode_files_lists against the oracle, file {i}"
        self.ins.append(path)
        self.nodes.append(nodes)
        self.cfgs.append(jc)
        self.jobs.append(L.file_job(jc, nodes))
        self.want.append(img)
        self.meters.append(m)
        self.lens.append(n)

    def add_wav(self, root, oracle, seed, n, fmt, ch, fs, jc, nodes):
        d = loud_pcm(seed, n, fs, ch, fmt)
        path = root / f"in_{len(self.ins)}.wav"
        W.write(path, d, fmt, ch, fs, kind="float" if fmt == abi.FMT_F32 else "pcm")
        self.add(root, oracle, path, d, fmt, ch, fs, n, jc, nodes)

    def run(self, out_dir, tag, ok=True, **kw):
        outs = [out_dir / f"{tag}_{i}.wav" for i in range(len(self.ins))]
        rc, st, status, meters = L.transcode_files_jobs(self.cfg, self.jobs, self.ins, outs, fade_in_ms=FADE, fade_out_ms=FADE,
                                                        block_frames=B, **kw)
        if ok:
            assert rc == abi.OK and status == [abi.OK] * len(self.ins)
        return st, [o.read_bytes() if o.exists() else None for o in outs], meters, status, rc

    def check(self, got, meters, which=None):
        for i in (range(len(self.ins)) if which is None else which):
            assert got[i][:44] == self.want[i][:44], f"file {i}: header"
            assert got[i] == self.want[i], f"file {i} ({self.lens[i]} frames)"
            m, r = meters[i], self.meters[i]
            assert m["clips"] == r["clips"] and m["peak_db"] == r["peak_db"] and m["desubnorm"] == r["desubnorm"], (i, m, r)

    def plan(self, slots, order, cwave=False):
        """the plan the call executes for these files as one pool context: the jobs' classes, the files ordered by
        class"""
        K, cls = L.file_job_classes(self.jobs, cwave)
        by_class = sorted(range(len(cls)), key=lambda i: cls[i])
        rc, _, _, st = L.pool_plan_classes([self.lens[i] for i in by_class], [cls[i] for i in by_class], slots, B, order)
        assert rc == abi.OK and st.classes == K
        return st


@pytest.fixture(scope="module")
def four(tmp_path_factory, oracle):
    """12 loud files of mixed input formats, each with its own list (one of them graph_pm_shift_mix), the four
    classes dealt round-robin: in the arrays no two neighbours share a setting"""
    root = tmp_path_factory.mktemp("jobs_lib")
    f = Files()
    for i, n in enumerate(LENGTHS):
        fmt, ch, fs = INPUTS[(i + i // 4) % len(INPUTS)]
        nodes = graph.graph_pm_shift_mix() if i == 4 else [graph.master(inputs=("A",)), graph.shift(out="A", fr=1.5 + 2.25 * i)]
        f.add_wav(root, oracle, i, n, fmt, ch, fs, CLASSES[i % 4](), nodes)
    assert sum(sum(m["clips"]) > 0 for m in f.meters) >= 4 and len({m["clips"] for m in f.meters}) >= 4   # loud: the meters tell files apart
    return f


@pytest.mark.parametrize("order", [abi.POOL_AS_GIVEN, abi.POOL_LONGEST_FIRST])
def test_four_classes_on_ragged_ranges(tmp_path, four, order):
    """5 slots over 4 classes of 3 files: one class has 2 slots, every range is refilled"""
    st, got, meters, _, _ = four.run(tmp_path, "r", slots=5, order=order)
    four.check(got, meters)
    plan = four.plan(5, order)
    assert st.classes == 4 and st.hilbert_runs_max == 3 and st.render_runs_max <= 4
    assert st.pool.slots == 5 and st.pool.refills == 7 == plan.pool.refills and st.pool.refills > 0
    assert (st.pool.blocks, st.pool.slot_blocks, st.pool.busy_slot_blocks) == \
           (plan.pool.blocks, plan.pool.slot_blocks, plan.pool.busy_slot_blocks)
    assert st.pool.busy_slot_blocks == sum(-(-n // B) for n in LENGTHS)
    assert st.pool.batch.n_files == 12 and st.pool.batch.n_groups == 1
    assert st.pool.batch.frames_in == sum(LENGTHS) == st.pool.batch.frames_out and st.kernel_s == 0.0


def test_one_slot_per_file_and_a_width_raised_to_the_classes(tmp_path, four):
    st, got, meters, _, _ = four.run(tmp_path, "all", slots=0)
    four.check(got, meters)
    assert st.pool.slots == 12 and st.pool.refills == 0 and st.pool.blocks == -(-max(LENGTHS) // B) and st.classes == 4
    st, got, meters, _, _ = four.run(tmp_path, "two", slots=2, order=abi.POOL_LONGEST_FIRST)
    four.check(got, meters)
    assert st.pool.slots == 4 and st.pool.refills == 8 and st.classes == 4 and st.hilbert_runs_max == 3
    assert st.pool.blocks == four.plan(2, abi.POOL_LONGEST_FIRST).pool.blocks


def test_slot_reuse_inside_a_table_of_several_renders(tmp_path, oracle):
    """a TPDF + MEW44 range of ONE slot runs three files in turn beside a ROUND range: generator words, shaper rings
    and the dB mirror start again with every file (icw_stream_init with more than one render entry in force)"""
    f = Files()
    shaped, plain = CLASSES[1], CLASSES[0]
    for i, (n, mk) in enumerate(((700, shaped), (900, plain), (513, shaped), (300, plain), (600, shaped))):
        f.add_wav(tmp_path, oracle, 30 + i, n, abi.FMT_I16, 2, 44100, mk(),
                  [graph.master(inputs=("A",)), graph.shift(out="A", fr=2.0 + i)])
    st, got, meters, _, _ = f.run(tmp_path, "s", slots=2)
    f.check(got, meters)
    assert st.classes == 2 and st.pool.slots == 2 and st.pool.refills == 3 and st.hilbert_runs_max == 1 and st.render_runs_max == 2
    assert [f.cfgs[i].need24bits for i in range(5)] == [1, 0, 1, 0, 1] and [len(g) for g in got] == [44 + (6, 4)[i % 2] * f.lens[i] for i in range(5)]


def test_one_class_is_the_pool(tmp_path, oracle):
    f = Files()
    for i, n in enumerate(LENGTHS[:7]):
        fmt, ch, fs = INPUTS[i % len(INPUTS)]
        f.add_wav(tmp_path, oracle, 50 + i, n, fmt, ch, fs, CLASSES[1](), [graph.master(inputs=("A",)), graph.shift(out="A", fr=1.0 + i)])
    st, got, meters, _, _ = f.run(tmp_path, "j", slots=3)
    f.check(got, meters)
    outs = [tmp_path / f"p_{i}.wav" for i in range(7)]
    rc, sp, status, mp = L.transcode_files_pool(CLASSES[1](), f.nodes, f.ins, outs, slots=3, fade_in_ms=FADE, fade_out_ms=FADE,
                                                block_frames=B)
    assert rc == abi.OK and status == [abi.OK] * 7
    assert [o.read_bytes() for o in outs] == got and mp == meters
    for name in ("slots", "refills", "blocks", "slot_blocks", "busy_slot_blocks"):
        assert getattr(st.pool, name) == getattr(sp, name), name
    for name in ("n_files", "n_groups", "frames_in", "frames_out"):
        assert getattr(st.pool.batch, name) == getattr(sp.batch, name), name
    assert st.classes == st.hilbert_runs_max == st.render_runs_max == 1


def test_cwave_jobs(tmp_path, oracle):
    """CWAVE files in two frame formats with two renders and three Hilbert settings: no recurrence runs, so the
    class is the render and the depth alone"""
    specs = [(abi.FMT_CW_I16, 2, 2000, 600, 0), (abi.FMT_CW_F32, 1, 3000, 257, 1), (abi.FMT_CW_I16, 1, 3000, 512, 2),
             (abi.FMT_CW_F32, 2, 2000, 900, 3), (abi.FMT_CW_I16, 2, 2000, 255, 0)]
    f = Files()
    for i, (fmt, ch, fs, n, c) in enumerate(specs):
        d = synth.stream_cwave(i, n, fs, channels=ch, fmt=fmt)
        path = tmp_path / f"in_{i}.cwave"
        path.write_bytes(cwave.make_image(d, fmt, ch, fs).tobytes())
        jc = CLASSES[c]()
        if c in (0, 3):                                    # 0 / 3 and 1: two renders; the Hilbert fields differ throughout
            jc.render, jc.need24bits = CLASSES[1]().render, 1
        f.add(tmp_path, oracle, path, d, fmt, ch, fs, n, jc, [graph.master(inputs=("A",)), graph.shift(out="A", fr=-3.0 + 1.75 * i)])
    assert len({(c.hilbert_type, c.iir_kahan) for c in f.cfgs}) == 3
    st, got, meters, _, _ = f.run(tmp_path, "c", slots=2)
    f.check(got, meters)
    assert st.classes == 2 and st.pool.slots == 2 and st.pool.refills == 3 and st.pool.batch.n_groups == 1
    assert st.hilbert_runs_max == 0 and st.render_runs_max == 2
    assert st.pool.blocks == f.plan(2, abi.POOL_AS_GIVEN, cwave=True).pool.blocks


def test_bus_form_jobs_run_in_a_context_per_class(tmp_path, oracle):
    """self-feeding Mix -> Master lists of two classes: bus-form lists stand beside no differing render or
    converter, so each class gets a pool context of its own, its setting context-wide"""
    f = Files()
    for i, (n, g, c) in enumerate(((700, 0.5, 1), (300, 0.9, 3), (513, 0.7, 1), (256, 0.85, 3), (900, 0.6, 1))):
        nodes = [graph.master(inputs=("C",)), graph.mix(inputs=("in", "C"), out="C", gain=g)]
        assert L.graph_form(f.cfg, nodes) == 1
        f.add_wav(tmp_path, oracle, 70 + i, n, abi.FMT_I16, 2, 44100, CLASSES[c](), nodes)
    st, got, meters, _, _ = f.run(tmp_path, "b", slots=1)
    f.check(got, meters)
    assert st.pool.batch.n_groups == 2 and st.classes == 2 and st.pool.slots == 1 and st.pool.refills == 3
    assert st.hilbert_runs_max == st.render_runs_max == 1


def test_bad_jobs_take_no_slot(tmp_path, four):
    """hilbert_type 6, a render field out of range and a list without a Master: refused, and the neighbours'
    bytes and meters are what they are without them"""
    f = Files()
    keep = (0, 1, 2, 3, 5, 6)
    for name in ("ins", "nodes", "cfgs", "want", "meters", "lens"):
        setattr(f, name, [getattr(four, name)[i] for i in keep])
    f.jobs = [L.file_job(c, nl) for c, nl in zip(f.cfgs, f.nodes)]
    f.jobs[1].hilbert_type = 6
    f.jobs[3].render.sign_bits16 = 17
    f.jobs[4] = L.file_job(f.cfgs[4], [graph.shift(out="A", fr=3.0)])
    st, got, meters, status, rc = f.run(tmp_path, "e", ok=False, slots=2)
    assert status == [abi.OK, abi.EINVAL, abi.OK, abi.EINVAL, abi.EGRAPH, abi.OK] and rc != abi.OK
    f.check(got, meters, which=(0, 2, 5))
    assert st.pool.batch.n_files == 3 and st.classes == 2 and st.pool.slots == 2     # files 0, 5 (class 0 and 2 of CLASSES) and 2
    assert meters[1] == meters[3] == meters[4] == {"clips": (0, 0), "peak_db": (0.0, 0.0), "desubnorm": 0}


def test_timing_flag(tmp_path, four):
    st, got, meters, _, _ = four.run(tmp_path, "t", slots=5, timing=True)
    four.check(got, meters)
    assert st.kernel_s > 0.0 and st.kernel_s < st.pool.batch.wall_s
    # the pool keeps ignoring the bit: files 0 and 4, both of the first class, through it with the bit set
    import ctypes as C
    pick = (0, 4)
    ins = (C.c_char_p * 2)(*[str(four.ins[i]).encode() for i in pick])
    outs = (C.c_char_p * 2)(*[str(tmp_path / f"pool_{i}.wav").encode() for i in pick])
    arrs = [L.graph_nodes(four.nodes[i]) for i in pick]
    ptrs = (C.POINTER(abi.Node) * 2)(*[C.cast(a, C.POINTER(abi.Node)) for a in arrs])
    cnt = (C.c_int * 2)(*[len(four.nodes[i]) for i in pick])
    o = abi.PoolOpts(abi.BatchOpts(FADE, FADE, 0, B, -1, abi.BATCH_TIMING), 1, 0)
    sp, status = abi.PoolStats(), (C.c_int * 2)()
    rc = L.load().icw_transcode_files_pool(C.byref(CLASSES[0]()), ptrs, cnt, None, ins, outs, 2, C.byref(o), C.byref(sp), None, status)
    assert rc == abi.OK and list(status) == [abi.OK] * 2 and sp.refills == 1
    assert [(tmp_path / f"pool_{i}.wav").read_bytes() for i in pick] == [four.want[i] for i in pick]
