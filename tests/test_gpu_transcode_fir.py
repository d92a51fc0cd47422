"""GPU: icw_transcode_files_fir -- every file through its own DSP list and the FIR Hilbert converter --
against the oracle, byte for byte, with and without ICW_BATCH_MERGE_INPUTS; a CWAVE file in the batch
comes out as icw_transcode_files_lists gives it."""
import numpy as np
import pytest

from in_cwave_amd import abi, cwave, graph, synth
from in_cwave_amd import lib as L

import wavgen as W

pytestmark = pytest.mark.gpu

ORDER, BETA = 254, 8.0
# three formats, two rates, mono and stereo, about 3 000 frames; low rates keep the one-second tails short
SPECS = [("a.wav", abi.FMT_I16, 2, 2000, 3000), ("b.wav", abi.FMT_I24, 2, 3000, 2901), ("c.wav", abi.FMT_F32, 1, 2000, 3100),
         ("d.wav", abi.FMT_I16, 1, 3000, 2999), ("e.wav", abi.FMT_I24, 1, 2000, 3333), ("f.wav", abi.FMT_F32, 2, 3000, 2500)]


def file_lists():
    return [graph.graph_shift_master(), [graph.master(inputs=("A",)), graph.shift(out="A", fr=-7.5)], graph.graph_pm_shift_mix(),
            graph.graph_master_only(), [graph.master(inputs=("A",)), graph.shift(out="A", fr=3.25)], graph.graph_shift_master()]


def oracle_bytes(oracle, cfg0, nodes, fmt, ch, fs, n, data, fade_in, fade_out):
    c = graph.default_config(fs, fmt=fmt, channels=ch, need24bits=bool(cfg0.need24bits))
    c.render = cfg0.render
    total = n + ((fs - n % fs) % fs)
    raw = np.concatenate([data, np.zeros((total - n) * abi.FMT_BYTES[fmt] * ch, np.uint8)])
    s = oracle.Stream(c, nodes)
    s.set_fir(ORDER, BETA)
    s.open(n, fade_in, fade_out, 1)
    ref, _ = s.process(raw, total)
    return total, ref


@pytest.mark.parametrize("merge", [False, True], ids=["grouped", "merged"])
def test_files_vs_oracle(tmp_path, oracle, merge):
    files = []
    for i, (name, fmt, ch, fs, n) in enumerate(SPECS):
        d = synth.stream_pcm(i, n, fs, channels=ch, fmt=fmt)
        W.write(tmp_path / name, d, fmt, ch, fs, kind="float" if fmt == abi.FMT_F32 else "pcm")
        files.append((tmp_path / name, fmt, ch, fs, n, d))
    cw = synth.stream_cwave(9, 1200, 2000, fmt=abi.FMT_CW_I16)
    (tmp_path / "g.cwave").write_bytes(cwave.make_image(cw, abi.FMT_CW_I16, 2, 2000).tobytes())
    lists = file_lists() + [graph.graph_shift_master()]
    cfg = graph.default_config(48000)
    ins = [f[0] for f in files] + [tmp_path / "g.cwave"]
    outs = [tmp_path / f"o_{i}.wav" for i in range(len(ins))]
    plain = [tmp_path / f"p_{i}.wav" for i in range(len(ins))]
    rc, st, status = L.transcode_files_fir(cfg, lists, ins, outs, ORDER, BETA, fade_in_ms=10, fade_out_ms=20, sec_align=1,
                                           block_frames=1024, merge_inputs=merge)
    assert rc == abi.OK and status == [abi.OK] * len(ins)
    assert st.n_files == len(ins)
    assert st.n_groups == (2 if merge else 7)          # merged: the real-input context and the CWAVE one
    for (path, fmt, ch, fs, n, data), nodes, out in zip(files, lists, outs):
        total, ref = oracle_bytes(oracle, cfg, nodes, fmt, ch, fs, n, data, 10, 20)
        got = np.frombuffer(out.read_bytes(), np.uint8)
        assert int.from_bytes(got[24:28].tobytes(), "little") == fs
        assert int.from_bytes(got[40:44].tobytes(), "little") == total * 4
        assert np.array_equal(got[44:], ref), path.name
    # the CWAVE file is analytic already: the converter is not applied to it
    rc, _, status = L.transcode_files_lists(cfg, lists, ins, plain, fade_in_ms=10, fade_out_ms=20, sec_align=1,
                                            block_frames=1024, merge_inputs=merge)
    assert rc == abi.OK
    assert outs[-1].read_bytes() == plain[-1].read_bytes()
    assert outs[0].read_bytes() != plain[0].read_bytes()
