"""GPU: icw_transcode_files_lists -- every file through its own DSP list -- against the oracle, byte
for byte.  Four files in three (rate, format, channels) groups, one list of them bus form (it runs in
a context of its own), fades and the sec_align tail; a fifth file with a rejected list gets
ICW_EGRAPH while the others complete."""
import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth
from in_cwave_amd import lib as L

import wavgen as W

pytestmark = pytest.mark.gpu


def test_transcode_lists_vs_oracle(tmp_path, oracle):
    specs = [("a.wav", abi.FMT_I16, 2, 44100, 3000, graph.graph_shift_master()),
             ("b.wav", abi.FMT_I16, 2, 44100, 2901, graph.graph_leaky_feedback()),      # bus form
             ("c.wav", abi.FMT_F32, 1, 48000, 3100, graph.graph_pm_shift_mix()),
             ("d.wav", abi.FMT_I24, 2, 44100, 2800, graph.graph_master_only()),
             ("e.wav", abi.FMT_I16, 2, 44100, 3001, [graph.master(inputs=("A",)), graph.shift(out="A", fr=-7.5)]),
             ("f.wav", abi.FMT_I16, 2, 44100, 3000, [graph.shift()])]                   # rejected: no Master
    files = []
    for i, (name, fmt, ch, fs, n, nodes) in enumerate(specs):
        d = synth.stream_pcm(i, n, fs, channels=ch, fmt=fmt)
        W.write(tmp_path / name, d, fmt, ch, fs, kind="float" if fmt == abi.FMT_F32 else "pcm")
        files.append((tmp_path / name, fmt, ch, fs, n, d, nodes))
    cfg = graph.default_config(48000)
    assert L.graph_form(cfg, specs[1][5]) == 1 and L.graph_form(cfg, specs[0][5]) == 0
    assert L.graph_form(cfg, specs[5][5]) == abi.EGRAPH
    ins = [f[0] for f in files]
    outs = [tmp_path / f"out_{i}.wav" for i in range(len(ins))]
    rc, st, status = L.transcode_files_lists(cfg, [f[6] for f in files], ins, outs, fade_in_ms=10, fade_out_ms=20,
                                             sec_align=1, block_frames=1024)
    assert status == [abi.OK] * 5 + [abi.EGRAPH] and rc == abi.EGRAPH
    assert st.n_files == 5 and st.n_groups == 4          # three formats, and the bus-form list's own context
    for (path, fmt, ch, fs, n, data, nodes), out in list(zip(files, outs))[:5]:
        c = graph.default_config(fs, fmt=fmt, channels=ch)
        total = n + ((fs - n % fs) % fs)
        fsz = abi.FMT_BYTES[fmt] * ch
        raw = np.concatenate([data, np.zeros((total - n) * fsz, np.uint8)])
        s = oracle.Stream(c, nodes)
        s.open(n, 10, 20, 1)
        ref, _ = s.process(raw, total)
        got = np.frombuffer(out.read_bytes(), np.uint8)
        assert int.from_bytes(got[40:44].tobytes(), "little") == total * 4
        assert np.array_equal(got[44:], ref), path.name
