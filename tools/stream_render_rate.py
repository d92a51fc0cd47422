#!/usr/bin/env python3
"""What per-stream renders buy on the C2 shape: 256 stereo streams, 2^20 frames, Shift -> Master, device
pointers, every stream with its own generated input.

    python tools/stream_render_rate.py [--streams 256] [--frames 1048576] [--runs 3] [--steps 10]
                                       [--warmup 5] [--legs a,b,c,d] [--input pcm|cwave] [--out FILE]

Four legs per run, `--runs` runs of each in one session:
  a_one_render    one render (16-bit ROUND) through icw_set_render + icw_set_outbits: the reference point
  b_same_render   the same render given to every stream through icw_set_stream_render (the count reads 1: a
                  one-render context again, the same launches)
  c_merged        four entries x streams / 4 consecutive streams in ONE context: 16-bit ROUND, 16-bit TPDF flat,
                  24-bit TPDF + MEW44, 24-bit ROUND
  d_split         the same streams as four contexts of streams / 4, one per entry, run one after the other on
                  one HIP stream
--input cwave feeds CW_F64 frames (no quadrature IIR: K1 does not hide the render).
One JSON line per leg and run: Msamples/s (frames x 2 channels x streams per second of the call(s), HIP events
on the stream; the unit of bench.py), the median, and the K1 time and the output side's time (K2 to the end of
the render) per call summed over the launch blocks (icw_last_timing, taken in one extra timed call so that the
event records stay out of the rate; d_split: summed over its four contexts)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def device_tones(torch, S, T, fs, seed):
    """[S, T, 2] float64 on the device, 16-bit scale: per stream and channel two sines at -12 dBFS"""
    rng = np.random.default_rng(seed)
    f = torch.tensor(rng.uniform(40.0, 0.4 * fs, size=(S, 2, 2)), device="cuda")
    ph = torch.tensor(rng.uniform(0, 2 * np.pi, size=(S, 2, 2)), device="cuda")
    out = torch.empty((S, T, 2), dtype=torch.float64, device="cuda")
    a = 32767.0 * 10 ** (-12 / 20)
    chunk = 1 << 16
    for t0 in range(0, T, chunk):
        t = torch.arange(t0, min(T, t0 + chunk), device="cuda", dtype=torch.float64) / fs
        for ch in range(2):
            x = torch.zeros((S, t.numel()), dtype=torch.float64, device="cuda")
            for k in range(2):
                x += torch.sin(2 * np.pi * f[:, ch, k, None] * t[None, :] + ph[:, ch, k, None])
            out[:, t0:t0 + t.numel(), ch] = a * x
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--legs", default="a,b,c,d", help="the legs to run, by their first letters")
    ap.add_argument("--input", default="pcm", choices=["pcm", "cwave"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    from in_cwave_amd import abi, graph
    from in_cwave_amd import lib as L

    S, T = a.streams, a.frames
    assert S % 4 == 0
    Q = S // 4

    def render(rtype, ns):
        r = abi.RenderCfg.from_buffer_copy(bytes(graph.default_config().render))
        r.render_type, r.nshape_type = rtype, ns
        return r

    entries = [(render(abi.RENDER_ROUND, abi.NSHAPE_FLAT), 0), (render(abi.RENDER_TPDF, abi.NSHAPE_FLAT), 0),
               (render(abi.RENDER_TPDF, abi.NSHAPE_MEW44), 1), (render(abi.RENDER_ROUND, abi.NSHAPE_FLAT), 1)]
    fmt = abi.FMT_I16 if a.input == "pcm" else abi.FMT_CW_F64
    cfg = graph.default_config(48000, fmt=fmt)
    nodes = graph.graph_shift_master()
    tones = device_tones(torch, S, T, 48000, 3000)
    if a.input == "pcm":
        d_in = torch.clamp(torch.round(tones), -32768, 32767).to(torch.int16).contiguous().view(torch.uint8).reshape(S, T * 4)
    else:
        # analytic-looking frames: (re, im) per channel, the imaginary part the tone a quarter period on
        z = torch.stack((tones, torch.roll(tones, 12, dims=1)), dim=-1)
        d_in = z.contiguous().view(torch.uint8).reshape(S, T * 32)
    del tones
    d_out = torch.empty((S, T * 6), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    lines = []

    def leg(name, run):
        if name == "d_split":
            ctxs = []
            for q, (r, b24) in enumerate(entries):
                c = L.Context(abi.Config.from_buffer_copy(cfg), nodes, Q)
                c.set_render(r)
                c.set_outbits(b24)
                ctxs.append((c, d_in[q * Q:(q + 1) * Q], d_out[q * Q:(q + 1) * Q]))
            count = len(ctxs)
        else:
            ctx = L.Context(abi.Config.from_buffer_copy(cfg), nodes, S)
            if name == "a_one_render":
                ctx.set_render(entries[0][0])
                ctx.set_outbits(entries[0][1])
            elif name == "b_same_render":
                ctx.set_stream_render(*entries[0])
            else:
                for q, (r, b24) in enumerate(entries):
                    ctx.set_stream_render(r, b24, q * Q, Q)
            count = ctx.stream_render_count()
            assert count == (4 if name == "c_merged" else 1), count
            ctxs = [(ctx, d_in, d_out)]

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
        k1 = k2 = 0.0
        n1 = n2 = 0
        for c, i, o in ctxs:
            c.process_device(i, i.stride(0), o, o.stride(0), T, timing=True, hip_stream=stream.cuda_stream)
            stream.synchronize()
            (x1, x2), (m1, m2) = c.last_timing()
            k1, k2, n1, n2 = k1 + x1, k2 + x2, n1 + m1, n2 + m2
        for c, _, _ in ctxs:
            c.close()
        med = float(np.median(ms))
        rec = {"tool": "stream_render_rate", "input": a.input, "leg": name, "run": run, "streams": S, "frames": T,
               "contexts": len(ctxs), "renders": count, "ms": [round(v, 3) for v in ms], "median_ms": round(med, 3),
               "msamples_per_s": round(2.0 * S * T / med / 1e3, 1),
               "k1_ms": round(k1, 3), "output_ms": round(k2, 3), "launches": [n1, n2]}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for run in range(a.runs):
        for name in ("a_one_render", "b_same_render", "c_merged", "d_split"):
            if name[0] in a.legs.split(","):
                leg(name, run)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
