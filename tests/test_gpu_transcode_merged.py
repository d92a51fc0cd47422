"""GPU: the file transcoder with ICW_BATCH_MERGE_INPUTS -- all real-input files in one context, every
stream on its own file's rate, format and channels -- against the oracle and against the same call
without the flag, byte for byte."""
import numpy as np
import pytest

from in_cwave_amd import abi, cwave, graph, synth
from in_cwave_amd import lib as L

import wavgen as W

pytestmark = pytest.mark.gpu

# low rates keep the sec_align tails (one second) short
SPECS = [("a.wav", abi.FMT_I16, 2, 2000, 1500), ("b.wav", abi.FMT_I24, 2, 3000, 2901), ("c.wav", abi.FMT_F32, 1, 2500, 700),
         ("d.wav", abi.FMT_U8, 2, 2000, 2000), ("e.wav", abi.FMT_I16, 2, 2000, 333), ("f.wav", abi.FMT_I32, 1, 1500, 1499)]


def write_files(tmp_path):
    files = []
    for i, (name, fmt, ch, fs, n) in enumerate(SPECS):
        d = synth.stream_pcm(i, n, fs, channels=ch, fmt=fmt)
        W.write(tmp_path / name, d, fmt, ch, fs, kind="float" if fmt == abi.FMT_F32 else "pcm")
        files.append((tmp_path / name, fmt, ch, fs, n, d))
    return files


def oracle_bytes(oracle, cfg0, nodes, fmt, ch, fs, n, data, fade_in, fade_out):
    c = graph.default_config(fs, fmt=fmt, channels=ch, need24bits=bool(cfg0.need24bits))
    c.render = cfg0.render
    total = n + ((fs - n % fs) % fs)
    fsz = abi.FMT_BYTES[fmt] * ch
    raw = np.concatenate([data, np.full((total - n) * fsz, 0x80 if fmt == abi.FMT_U8 else 0, np.uint8)])
    s = oracle.Stream(c, nodes)
    s.open(n, fade_in, fade_out, 1)
    ref, _ = s.process(raw, total)
    return total, ref


def test_merged_vs_oracle_and_grouped(tmp_path, oracle):
    """five (rate, format, channels) combinations and one CWAVE file: two contexts with the flag (the merged
    one and the CWAVE one), six without; the same bytes either way, and the oracle's"""
    files = write_files(tmp_path)
    cw = synth.stream_cwave(9, 1200, 2000, fmt=abi.FMT_CW_I16)
    (tmp_path / "g.cwave").write_bytes(cwave.make_image(cw, abi.FMT_CW_I16, 2, 2000).tobytes())
    cfg = graph.default_config(48000)
    cfg.render.render_type = abi.RENDER_TPDF
    nodes = graph.graph_shift_master()
    ins = [f[0] for f in files] + [tmp_path / "g.cwave"]
    merged = [tmp_path / f"m_{i}.wav" for i in range(len(ins))]
    grouped = [tmp_path / f"g_{i}.wav" for i in range(len(ins))]
    rc, st, status = L.transcode_files(cfg, nodes, ins, merged, fade_in_ms=10, fade_out_ms=20, sec_align=1, block_frames=1024,
                                       merge_inputs=True)
    assert rc == abi.OK and status == [abi.OK] * len(ins)
    assert st.n_files == len(ins) and st.n_groups == 2
    rc, st, status = L.transcode_files(cfg, nodes, ins, grouped, fade_in_ms=10, fade_out_ms=20, sec_align=1, block_frames=1024)
    assert rc == abi.OK and st.n_groups == 6
    for m, g in zip(merged, grouped):
        assert m.read_bytes() == g.read_bytes(), m.name
    for (path, fmt, ch, fs, n, data), out in zip(files, merged):
        total, ref = oracle_bytes(oracle, cfg, nodes, fmt, ch, fs, n, data, 10, 20)
        got = np.frombuffer(out.read_bytes(), np.uint8)
        assert int.from_bytes(got[24:28].tobytes(), "little") == fs
        assert int.from_bytes(got[40:44].tobytes(), "little") == total * 4
        assert np.array_equal(got[44:], ref), path.name
    c = graph.default_config(2000, fmt=abi.FMT_CW_I16, channels=2)
    c.render = cfg.render
    s = oracle.Stream(c, nodes)
    s.open(1200, 10, 20, 1)
    ref, _ = s.process(np.concatenate([cw, np.zeros(800 * 8, np.uint8)]), 2000)
    assert np.array_equal(np.frombuffer(merged[-1].read_bytes(), np.uint8)[44:], ref)


def test_merged_lists(tmp_path, oracle):
    """the lists entry with the flag: register-form lists across formats share one context, a bus-form
    file keeps its own"""
    files = write_files(tmp_path)
    lists = [graph.graph_shift_master(), graph.graph_leaky_feedback(), graph.graph_pm_shift_mix(), graph.graph_master_only(),
             [graph.master(inputs=("A",)), graph.shift(out="A", fr=-7.5)], graph.graph_shift_master()]
    cfg = graph.default_config(48000)
    assert L.graph_form(cfg, lists[1]) == 1
    ins = [f[0] for f in files]
    merged = [tmp_path / f"m_{i}.wav" for i in range(len(ins))]
    grouped = [tmp_path / f"g_{i}.wav" for i in range(len(ins))]
    rc, st, status = L.transcode_files_lists(cfg, lists, ins, merged, fade_in_ms=10, fade_out_ms=20, sec_align=1,
                                             block_frames=1024, merge_inputs=True)
    assert rc == abi.OK and status == [abi.OK] * len(ins)
    assert st.n_files == len(ins) and st.n_groups == 2      # the register-form files, and the bus-form one
    rc, st, status = L.transcode_files_lists(cfg, lists, ins, grouped, fade_in_ms=10, fade_out_ms=20, sec_align=1,
                                             block_frames=1024)
    assert rc == abi.OK and st.n_groups == 5
    for (path, fmt, ch, fs, n, data), nodes, m, g in zip(files, lists, merged, grouped):
        total, ref = oracle_bytes(oracle, cfg, nodes, fmt, ch, fs, n, data, 10, 20)
        got = np.frombuffer(m.read_bytes(), np.uint8)
        assert np.array_equal(got[44:], ref), path.name
        assert m.read_bytes() == g.read_bytes(), path.name
