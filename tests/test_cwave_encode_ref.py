"""The pure-Python restatement of the CWAVE encoder (tests/cwenc_ref.py) against the oracle's FIR
converter (oracle/icw_oracle.c fir_process), on the CPU: decoding the restatement's ICW_FMT_CW_F64 frames
must give exactly what the oracle gives for the PCM through its own converter -- pre-render doubles and
rendered bytes.  The GPU tests of the encoder (tests/test_gpu_cwave_encode.py) rely on the restatement
only after this.

Parity is unpinned against the reference, like the converter itself: in_cwave ships no converter."""
import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth

import cwenc_ref

BETA = 8.0
N = 600


@pytest.mark.parametrize("k_M", [30, 62])
@pytest.mark.parametrize("fmt,ch", [(abi.FMT_I16, 2), (abi.FMT_F32, 1)])
def test_restatement_decodes_to_the_oracles_fir(oracle, k_M, fmt, ch):
    nodes = graph.graph_shift_master()
    raw = synth.batch_pcm(2, N, 48000, channels=ch, fmt=fmt)
    cfg = graph.default_config(48000, fmt=fmt, channels=ch)
    ref_out, ref_pre = oracle.process_streams(cfg, nodes, raw, N, want_pre=True, fir=(k_M, BETA))

    g = oracle.fir_taps(k_M, BETA)
    enc = np.stack([cwenc_ref.encode(raw[s], fmt, ch, k_M, g)[0] for s in range(raw.shape[0])])
    assert enc.shape[1] == N * 16 * ch
    cfg_cw = graph.default_config(48000, fmt=abi.FMT_CW_F64, channels=ch)
    out, pre = oracle.process_streams(cfg_cw, nodes, enc, N, want_pre=True)

    bad = np.flatnonzero(pre.view(np.uint64) != ref_pre.view(np.uint64))
    assert bad.size == 0, f"{bad.size} pre-render doubles differ, first at {bad[:5]}"
    assert np.array_equal(out, ref_out)
    assert np.abs(pre).max() > 1000.0          # a real signal went through


def test_quantisers_ties_and_saturation():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 32767.4, 32767.5, -32768.5, -32769.0, np.nan, np.inf, -np.inf, 1e300])
    q, n = cwenc_ref.quant_i16(v)
    assert q.tolist() == [0, 2, 2, 0, -2, 32767, 32767, -32768, -32768, 0, 32767, -32768, 32767]
    assert n == 6                              # 32767.5 -> 32768, -32769, nan, +inf, -inf, 1e300
    data, clipped = cwenc_ref.frames(v[:, None], v[:, None], abi.FMT_CW_I16_F32)
    assert data.size == v.size * 6 and clipped == 6
