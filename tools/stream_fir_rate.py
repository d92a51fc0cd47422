#!/usr/bin/env python3
"""What per-stream lists and inputs cost and buy with the FIR Hilbert converter on, on the c2fir shape: 256
stereo streams, 2^20 frames, 255 taps (order 254, Kaiser beta 8), Shift -> Master, 16-bit ROUND render,
device pointers, every stream with its own generated input.

    python tools/stream_fir_rate.py [--streams 256] [--frames 1048576] [--runs 3] [--steps 3]
                                    [--warmup 1] [--legs a,b,c,d,e,f] [--out FILE]

The legs, `--runs` runs of each in one session:
  a_one           one list and one input (48 kHz int16) through icw_set_graph / icw_set_input
  b_same          the same through icw_set_stream_graph / icw_set_stream_input (one entry: the same launches)
  c_lists         one Shift frequency per stream: `streams` lists of one signature, one input
  d_merged        four inputs x streams / 4 in ONE context: 44.1 k int16, 48 k int16, 96 k int24, 48 k float32
  e_split         the streams of d as four contexts of streams / 4, one after the other on one HIP stream
  f_merged_c5 / f_split_c5   d and e with the C5 render (24-bit TPDF + MEW44): the serial render bounds the
                  step, so the rate is the batch width
One JSON line per leg and run: Msamples/s (frames x 2 channels x streams per second of the call(s), HIP
events on the stream; the unit of bench.py), the median, and the converter's kernel time and launch-block
count of one extra timed call (icw_last_timing)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def device_pcm16(torch, S, T, fs, seed):
    """[S, T, 2] int16 on the device: per stream and channel two sines at -12 dBFS"""
    rng = np.random.default_rng(seed)
    f = torch.tensor(rng.uniform(40.0, 0.4 * fs, size=(S, 2, 2)), device="cuda")
    ph = torch.tensor(rng.uniform(0, 2 * np.pi, size=(S, 2, 2)), device="cuda")
    out = torch.empty((S, T, 2), dtype=torch.int16, device="cuda")
    a = 32767.0 * 10 ** (-12 / 20)
    chunk = 1 << 16
    for t0 in range(0, T, chunk):
        t = torch.arange(t0, min(T, t0 + chunk), device="cuda", dtype=torch.float64) / fs
        for ch in range(2):
            x = torch.zeros((S, t.numel()), dtype=torch.float64, device="cuda")
            for k in range(2):
                x += torch.sin(2 * np.pi * f[:, ch, k, None] * t[None, :] + ph[:, ch, k, None])
            out[:, t0:t0 + t.numel(), ch] = torch.clamp(torch.round(a * x), -32768, 32767).to(torch.int16)
    return out


def pack(torch, abi, pcm, fmt):
    """the int16 signal in the sample format fmt: uint8 [S, T * frame bytes]"""
    S, T, _ = pcm.shape
    if fmt == abi.FMT_I16:
        return pcm.contiguous().view(torch.uint8).reshape(S, T * 4)
    if fmt == abi.FMT_F32:
        return (pcm.to(torch.float32) / 32768.0).contiguous().view(torch.uint8).reshape(S, T * 8)
    if fmt == abi.FMT_I24:
        b = (pcm.to(torch.int32) << 8).contiguous().view(torch.uint8).reshape(S, T, 2, 4)[..., :3]
        return b.contiguous().reshape(S, T * 6)
    raise ValueError(fmt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--order", type=int, default=254)
    ap.add_argument("--legs", default="a,b,c,d,e,f", help="the legs to run, by their first letters")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    from in_cwave_amd import abi, graph
    from in_cwave_amd import lib as L

    S, T = a.streams, a.frames
    assert S % 4 == 0
    Q = S // 4
    BETA = 8.0
    inputs = [(44100, abi.FMT_I16, 2), (48000, abi.FMT_I16, 2), (96000, abi.FMT_I24, 2), (48000, abi.FMT_F32, 2)]
    nodes = graph.graph_shift_master()
    wide = max(abi.FMT_BYTES[f] * ch for _, f, ch in inputs)
    d_in = torch.zeros((S, T * wide), dtype=torch.uint8, device="cuda")
    for q, (rate, fmt, ch) in enumerate(inputs):
        rows = pack(torch, abi, device_pcm16(torch, Q, T, rate, 1000 + q), fmt)
        d_in[q * Q:(q + 1) * Q, :rows.shape[1]] = rows
    d_one = pack(torch, abi, device_pcm16(torch, S, T, 48000, 2000), abi.FMT_I16).contiguous()
    d_out = torch.empty((S, T * 6), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    lines = []

    def config(rate=48000, fmt=abi.FMT_I16, c5=False):
        cfg = graph.default_config(rate, fmt=fmt, channels=2, need24bits=c5)
        if c5:
            cfg.render.render_type = abi.RENDER_TPDF
            cfg.render.nshape_type = abi.NSHAPE_MEW44
        return cfg

    def leg(name, run):
        c5 = name.endswith("_c5")
        osz = 6 if c5 else 4
        if name.startswith(("e_split", "f_split")):
            ctxs = []
            for q, (rate, fmt, ch) in enumerate(inputs):
                c = L.Context(config(rate, fmt, c5), nodes, Q)
                c.set_fir_hilbert(a.order, BETA)
                ctxs.append((c, d_in[q * Q:(q + 1) * Q], d_out[q * Q:(q + 1) * Q]))
        else:
            ctx = L.Context(config(c5=c5), nodes, S)
            ctx.enable_stream_fir()
            ctx.set_fir_hilbert(a.order, BETA)
            src = d_one
            if name == "a_one":
                assert ctx.set_graph(nodes)
                ctx.set_input(48000, abi.FMT_I16, 2)
            elif name == "b_same":
                assert ctx.set_stream_graph(nodes)
                ctx.set_stream_input(48000, abi.FMT_I16, 2)
            elif name == "c_lists":
                for s in range(S):
                    own = [graph.master(inputs=("A",)), graph.shift(inputs=("in",), out="A", fr=0.5 + 0.125 * s)]
                    assert ctx.set_stream_graph(own, s, 1)
            else:
                for q, (rate, fmt, ch) in enumerate(inputs):
                    ctx.set_stream_input(rate, fmt, ch, q * Q, Q)
                src = d_in
            want = (S if name == "c_lists" else 1, 4 if src is d_in else 1)
            assert (ctx.stream_graph_count(), ctx.stream_input_count()) == want
            ctxs = [(ctx, src, d_out)]

        def call(timing=False):
            for c, i, o in ctxs:
                c.process_device(i, i.stride(0), o, o.stride(0), T, timing=timing, hip_stream=stream.cuda_stream)

        torch.cuda.synchronize()
        ms = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                call()
                e1.record(stream)
            stream.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        kf = 0.0
        nb = 0
        for c, i, o in ctxs:
            c.process_device(i, i.stride(0), o, o.stride(0), T, timing=True, hip_stream=stream.cuda_stream)
            stream.synchronize()
            (x1, _), (m1, _) = c.last_timing()
            kf, nb = kf + x1, nb + m1
        for c, _, _ in ctxs:
            c.close()
        med = float(np.median(ms))
        rec = {"tool": "stream_fir_rate", "leg": name, "run": run, "streams": S, "frames": T, "order": a.order,
               "contexts": len(ctxs), "out_bytes_per_frame": osz, "ms": [round(v, 3) for v in ms], "median_ms": round(med, 3),
               "msamples_per_s": round(2.0 * S * T / med / 1e3, 1), "converter_ms": round(kf, 3), "launch_blocks": nb}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    names = ("a_one", "b_same", "c_lists", "d_merged", "e_split", "f_merged_c5", "f_split_c5")
    for run in range(a.runs):
        for name in names:
            if name[0] in a.legs.split(","):
                leg(name, run)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
