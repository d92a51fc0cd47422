"""GPU: the file transcoder with ICW_BATCH_MERGE_BUS -- the bus-form files of a group in one context, every
stream on its own file's list -- against the oracle and against the same call without the bit, byte for byte."""
import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth
from in_cwave_amd import lib as L

import wavgen as W

pytestmark = pytest.mark.gpu

FS, FADE_IN, FADE_OUT = 3000, 10, 20            # a low rate keeps the sec_align tail (one second) short
FRAMES = (3000, 2901, 2750, 3100)


def test_bus_files_share_one_context(tmp_path, oracle):
    """one (rate, format, channels) group: a register-form list and three distinct bus-form lists -- four
    contexts without the bit, two with it (the register-form file keeps its own); the same bytes either way,
    and the oracle's, file by file"""
    lists = [graph.graph_shift_master(), graph.graph_leaky_feedback(), graph.graph_feedback_pm_shift(), graph.graph_long_chain(24)]
    cfg = graph.default_config(48000)
    assert [L.graph_form(cfg, nl) for nl in lists] == [0, 1, 1, 1]
    ins, data = [], []
    for i, n in enumerate(FRAMES):
        d = synth.stream_pcm(i, n, FS, channels=2, fmt=abi.FMT_I16)
        W.write(tmp_path / f"in_{i}.wav", d, abi.FMT_I16, 2, FS, kind="pcm")
        ins.append(tmp_path / f"in_{i}.wav")
        data.append(d)
    merged = [tmp_path / f"m_{i}.wav" for i in range(4)]
    apart = [tmp_path / f"a_{i}.wav" for i in range(4)]
    rc, st, status = L.transcode_files_lists(cfg, lists, ins, apart, fade_in_ms=FADE_IN, fade_out_ms=FADE_OUT, sec_align=1,
                                             block_frames=1024)
    assert rc == abi.OK and status == [abi.OK] * 4
    assert st.n_files == 4 and st.n_groups == 4
    rc, st, status = L.transcode_files_lists(cfg, lists, ins, merged, fade_in_ms=FADE_IN, fade_out_ms=FADE_OUT, sec_align=1,
                                             block_frames=1024, merge_bus=True)
    assert rc == abi.OK and status == [abi.OK] * 4
    assert st.n_files == 4 and st.n_groups == 2
    for i, (n, d, nodes) in enumerate(zip(FRAMES, data, lists)):
        assert merged[i].read_bytes() == apart[i].read_bytes(), f"file {i}: the bit changed the output"
        total = n + ((FS - n % FS) % FS)
        s = oracle.Stream(graph.default_config(FS), nodes)
        s.open(n, FADE_IN, FADE_OUT, 1)
        ref, _ = s.process(np.concatenate([d, np.zeros((total - n) * 4, np.uint8)]), total)
        got = np.frombuffer(merged[i].read_bytes(), np.uint8)
        assert int.from_bytes(got[40:44].tobytes(), "little") == total * 4
        assert np.array_equal(got[44:], ref), f"file {i} against the oracle"
