"""GPU parity with misaligned input: the unpack is specialised per format (icw_unpack_dev.h
icw_fmt_dispatch) and reads a sample with one typed load when the base address and the strides keep
every sample aligned to its size, with byte loads otherwise.  The reader's buffers carry no such
promise (xwave_reader.c:205-239 reads bytes), so both forms must give the oracle's bytes: device
input at byte offsets 0-3 with odd and even row strides, through K0 (quadrature IIR), the FIR
converter (KF2 and KF + K2) and the one-stream kernel K5.

Misaligned output: KF2 stores a lane's packed frames with 16- / 8-byte stores where the address allows
and all the lane's frames lie in the block, else as dwords (16-bit) or bytes (24-bit)
(test_fir_output_alignment)."""
import numpy as np
import pytest

from in_cwave_amd import abi, graph, synth

pytestmark = pytest.mark.gpu


def run(oracle, icw, cfg, nodes, S, T, off, pad, fir=None):
    import torch
    raw = synth.batch_pcm(S, T, cfg.sample_rate, channels=cfg.in_channels, fmt=cfg.in_format, first=3)
    row = raw.shape[1] + pad
    buf = np.zeros((S, row + 4), dtype=np.uint8)
    buf[:, off:off + raw.shape[1]] = raw
    d_buf = torch.from_numpy(buf).cuda()
    d_in = d_buf[:, off:]
    ctx = icw.Context(cfg, nodes, S)
    if fir:
        ctx.set_fir_hilbert(fir, 8.0)
    osz = 2 * ctx.render_size
    d_out = torch.zeros((S, T * osz), dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 8 == off
    ctx.process_device(d_in, d_buf.stride(0), d_out, d_out.stride(0), T)
    ctx.synchronize()
    out = d_out.cpu().numpy()
    for s in range(S):
        st = oracle.Stream(cfg, nodes)
        if fir:
            st.set_fir(fir, 8.0)
        ro, _ = st.process(raw[s], T)
        assert np.array_equal(out[s], ro), (s, off, pad)
    ctx.close()


FORMATS = [(abi.FMT_I16, 2), (abi.FMT_I16, 1), (abi.FMT_I32, 2), (abi.FMT_F32, 1), (abi.FMT_I24, 2),
           (abi.FMT_U8, 2)]


@pytest.mark.parametrize("off,pad", [(0, 0), (1, 0), (2, 1), (3, 2), (2, 0)])
@pytest.mark.parametrize("fmt,ch", FORMATS)
def test_iir_unaligned_input(oracle, icw, fmt, ch, off, pad):
    cfg = graph.default_config(48000, fmt=fmt, channels=ch)
    run(oracle, icw, cfg, graph.graph_shift_master(), 3, 1500, off, pad)


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("off,pad", [(1, 0), (2, 1), (2, 0)])
@pytest.mark.parametrize("fmt,ch", FORMATS)
def test_fir_unaligned_input(oracle, icw, fmt, ch, off, pad, fused, monkeypatch):
    monkeypatch.setenv("ICW_FIR_FUSED", fused)
    cfg = graph.default_config(48000, fmt=fmt, channels=ch)
    run(oracle, icw, cfg, graph.graph_shift_master(), 2, 2500, off, pad, fir=254)


@pytest.mark.parametrize("off", [0, 1, 2])
@pytest.mark.parametrize("fmt,ch", FORMATS)
def test_stream1_unaligned_input(oracle, icw, fmt, ch, off, monkeypatch):
    monkeypatch.setenv("ICW_STREAM1", "1")
    monkeypatch.setenv("ICW_K1_MODE", "row")
    cfg = graph.default_config(44100, fmt=fmt, channels=ch)
    run(oracle, icw, cfg, graph.graph_shift_master(), 1, 576, off, 0)


_FIR_OUT_REF = {}


def fir_out_ref(oracle, cfg, gname, nodes, raw, n):
    """the oracle's bytes and meters of the output-alignment cases, computed once per (input, depth, graph)"""
    key = (cfg.in_channels, cfg.need24bits, gname)
    if key not in _FIR_OUT_REF:
        ref, _ = oracle.process_streams(cfg, nodes, raw, n, want_pre=False, fir=(254, 8.0))
        meters = []
        for s in range(raw.shape[0]):
            st = oracle.Stream(cfg, nodes)
            st.set_fir(254, 8.0)
            st.process(raw[s], n)
            meters.append(st.meters())
        ref.setflags(write=False)
        _FIR_OUT_REF[key] = (ref, meters)
    return _FIR_OUT_REF[key]


@pytest.mark.parametrize("sig", ["1", "0"])
@pytest.mark.parametrize("step", [0, 1, 2])
@pytest.mark.parametrize("gname", ["master", "shift_master"])
@pytest.mark.parametrize("b24", [False, True])
@pytest.mark.parametrize("ch", [1, 2])
def test_fir_output_alignment(oracle, icw, ch, b24, gname, step, sig, monkeypatch):
    """KF2's packed stores at output addresses off a 16-byte boundary: one signature-form tile plus a
    short last tile through icw_fir_graph (ICW_FIR_SIG=0: icw_fir_graph for both), so the full-lane and
    the partial-lane forms both run.  16-bit output shifted by 0, 4, 8 bytes (dword stores), 24-bit by 0,
    2, 4 (byte stores); the row stride adds 4 bytes, so the second row sits at yet another phase.  Rows
    and meters are the oracle's, and no byte outside the frames is written."""
    import torch
    monkeypatch.setenv("ICW_FIR_SIG", sig)
    nodes = {"master": graph.graph_master_only, "shift_master": graph.graph_shift_master}[gname]()
    cfg = graph.default_config(48000, fmt=abi.FMT_I16, channels=ch, need24bits=b24)
    S, n = 2, (1024 if ch == 2 else 2048) + 5
    raw = synth.batch_pcm(S, n, 48000, channels=ch, first=5)
    ref, ref_meters = fir_out_ref(oracle, cfg, gname, nodes, raw, n)
    osz = 6 if b24 else 4
    shift = step * (2 if b24 else 4)
    stride = n * osz + 4
    first = 16 + shift
    d_in = torch.from_numpy(raw).cuda()
    d_flat = torch.zeros(first + S * stride + 16, dtype=torch.uint8, device="cuda")
    assert d_flat.data_ptr() % 16 == 0
    ctx = icw.Context(cfg, nodes, S)
    ctx.set_fir_hilbert(254, 8.0)
    ctx.process_device(d_in, d_in.stride(0), d_flat[first:], stride, n)
    ctx.synchronize()
    got = d_flat.cpu().numpy()
    meters = [ctx.meters(s) for s in range(S)]
    ctx.close()
    outside = np.ones(got.size, dtype=bool)
    for s in range(S):
        lo = first + s * stride
        bad = np.flatnonzero(got[lo:lo + n * osz] != ref[s])
        assert bad.size == 0, f"row {s}: {bad.size} bytes differ, first at {bad[:5]}"
        outside[lo:lo + n * osz] = False
    assert not got[outside].any(), f"bytes written outside the frames at {np.flatnonzero(outside & (got != 0))[:5]}"
    assert meters == ref_meters
