"""GPU: the file transcoder with ICW_BATCH_MERGE_CWAVE -- all CWAVE files in one context, every stream on
its own file's frame format, channels and rate -- against the oracle and against the same call without
the flag, byte for byte."""
import numpy as np
import pytest

from in_cwave_amd import abi, cwave, graph, synth
from in_cwave_amd import lib as L

import wavgen as W

pytestmark = pytest.mark.gpu

# one file per CWAVE frame format, mono and stereo, two rates (low: the sec_align tails stay short)
CW_SPECS = [("a.cwave", abi.FMT_CW_F64, 2, 2000, 1500), ("b.cwave", abi.FMT_CW_I16, 1, 3000, 1999),
            ("c.cwave", abi.FMT_CW_I16_F32, 2, 3000, 1200), ("d.cwave", abi.FMT_CW_F32, 1, 2000, 2000)]
WAV_SPECS = [("e.wav", abi.FMT_I16, 2, 2000, 1500), ("f.wav", abi.FMT_F32, 1, 2500, 700)]


def write_files(tmp_path):
    files = []
    for i, (name, fmt, ch, fs, n) in enumerate(CW_SPECS):
        d = synth.stream_cwave(i, n, fs, channels=ch, fmt=fmt)
        (tmp_path / name).write_bytes(cwave.make_image(d, fmt, ch, fs).tobytes())
        files.append((tmp_path / name, fmt, ch, fs, n, d))
    for i, (name, fmt, ch, fs, n) in enumerate(WAV_SPECS):
        d = synth.stream_pcm(10 + i, n, fs, channels=ch, fmt=fmt)
        W.write(tmp_path / name, d, fmt, ch, fs, kind="float" if fmt == abi.FMT_F32 else "pcm")
        files.append((tmp_path / name, fmt, ch, fs, n, d))
    return files


def oracle_bytes(oracle, cfg0, nodes, fmt, ch, fs, n, data, fade_in, fade_out):
    c = graph.default_config(fs, fmt=fmt, channels=ch, need24bits=bool(cfg0.need24bits))
    c.render = cfg0.render
    total = n + ((fs - n % fs) % fs)
    raw = np.concatenate([data, np.zeros((total - n) * abi.FMT_BYTES[fmt] * ch, np.uint8)])
    s = oracle.Stream(c, nodes)
    s.open(n, fade_in, fade_out, 1)
    ref, _ = s.process(raw, total)
    return total, ref


def test_merged_vs_oracle_and_grouped(tmp_path, oracle):
    """four CWAVE files and two WAVs: two contexts with both bits (the CWAVE one and the real one), six with
    neither; the same bytes either way, and the oracle's"""
    files = write_files(tmp_path)
    cfg = graph.default_config(48000)
    cfg.render.render_type = abi.RENDER_TPDF
    nodes = graph.graph_shift_master()
    ins = [f[0] for f in files]
    merged = [tmp_path / f"m_{i}.wav" for i in range(len(ins))]
    grouped = [tmp_path / f"g_{i}.wav" for i in range(len(ins))]
    rc, st, status = L.transcode_files(cfg, nodes, ins, merged, fade_in_ms=10, fade_out_ms=20, sec_align=1, block_frames=1024,
                                       merge_inputs=True, merge_cwave=True)
    assert rc == abi.OK and status == [abi.OK] * len(ins)
    assert st.n_files == len(ins) and st.n_groups == 2
    rc, st, status = L.transcode_files(cfg, nodes, ins, grouped, fade_in_ms=10, fade_out_ms=20, sec_align=1, block_frames=1024)
    assert rc == abi.OK and st.n_groups == 6
    # each bit alone merges its own kind only
    only = [tmp_path / f"o_{i}.wav" for i in range(len(ins))]
    rc, st, status = L.transcode_files(cfg, nodes, ins, only, fade_in_ms=10, fade_out_ms=20, sec_align=1, block_frames=1024,
                                       merge_cwave=True)
    assert rc == abi.OK and st.n_groups == 3
    for m, g, o in zip(merged, grouped, only):
        assert m.read_bytes() == g.read_bytes() == o.read_bytes(), m.name
    for (path, fmt, ch, fs, n, data), out in zip(files, merged):
        total, ref = oracle_bytes(oracle, cfg, nodes, fmt, ch, fs, n, data, 10, 20)
        got = np.frombuffer(out.read_bytes(), np.uint8)
        assert int.from_bytes(got[24:28].tobytes(), "little") == fs
        assert int.from_bytes(got[40:44].tobytes(), "little") == total * 4
        assert np.array_equal(got[44:], ref), path.name


def test_merged_lists(tmp_path, oracle):
    """the lists entry with two lists over the CWAVE files: they share the one CWAVE context"""
    files = write_files(tmp_path)[:4]
    a, b = graph.graph_shift_master(), [graph.master(inputs=("A",)), graph.shift(out="A", fr=-7.5)]
    lists = [a, b, b, a]
    cfg = graph.default_config(48000)
    ins = [f[0] for f in files]
    merged = [tmp_path / f"m_{i}.wav" for i in range(len(ins))]
    grouped = [tmp_path / f"g_{i}.wav" for i in range(len(ins))]
    rc, st, status = L.transcode_files_lists(cfg, lists, ins, merged, fade_in_ms=10, fade_out_ms=20, sec_align=1,
                                             block_frames=1024, merge_cwave=True)
    assert rc == abi.OK and status == [abi.OK] * len(ins)
    assert st.n_files == len(ins) and st.n_groups == 1
    rc, st, status = L.transcode_files_lists(cfg, lists, ins, grouped, fade_in_ms=10, fade_out_ms=20, sec_align=1,
                                             block_frames=1024)
    assert rc == abi.OK and st.n_groups == 4
    for (path, fmt, ch, fs, n, data), nodes, m, g in zip(files, lists, merged, grouped):
        total, ref = oracle_bytes(oracle, cfg, nodes, fmt, ch, fs, n, data, 10, 20)
        assert np.array_equal(np.frombuffer(m.read_bytes(), np.uint8)[44:], ref), path.name
        assert m.read_bytes() == g.read_bytes(), path.name
