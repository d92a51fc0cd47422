#!/usr/bin/env python3
"""What per-stream DSP lists cost on the C2 shape: 256 x 48 kHz stereo int16 streams, 2^20 frames,
Shift -> Master, 16-bit ROUND render, device pointers, every stream with its own generated input.

    python tools/stream_graphs_rate.py [--streams 256] [--frames 1048576] [--runs 3] [--steps 3]
                                       [--warmup 1] [--out FILE]

Three legs per run, `--runs` runs of each in one session:
  one_list      one list through icw_set_graph (the reference point of the session)
  same_list     the same list given to every stream through icw_set_stream_graph (the count reads 1:
                a one-list context again, the same launches)
  own_lists     one list per stream, `--streams` different Shift frequencies (no two streams share a
                list, so every stream computes its rotation factors inline)
One JSON line per leg and run: Msamples/s (frames x 2 channels x streams per second of the call, HIP
events on its stream; the unit of bench.py), the median call, and the K1 / K2 kernel time per call summed
over the launch blocks (icw_last_timing, taken in one extra timed call so that the event records stay
out of the rate)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def device_input(torch, S, T, fs):
    """[S, T * 4] uint8 on the device: per stream and channel two sines at -12 dBFS (frequencies and
    phases from the stream's own generator), int16 interleaved L, R"""
    rng = np.random.default_rng(1000)
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
    return out.view(torch.uint8).reshape(S, T * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    from in_cwave_amd import graph
    from in_cwave_amd import lib as L

    S, T, fs = a.streams, a.frames, 48000
    cfg = graph.default_config(fs)
    base = graph.graph_shift_master()
    d_in = device_input(torch, S, T, fs)
    d_out = torch.empty((S, T * 4), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    lines = []

    def own(s):
        return [graph.master(inputs=("A",)), graph.shift(inputs=("in",), out="A", fr=0.5 + 19.0 * s / max(1, S - 1))]

    def leg(name, run):
        ctx = L.Context(cfg, graph.graph_master_only(), S)
        if name == "one_list":
            assert ctx.set_graph(base)
        elif name == "same_list":
            assert ctx.set_stream_graph(base)
        else:
            for s in range(S):
                assert ctx.set_stream_graph(own(s), s, 1)
        count = ctx.stream_graph_count()
        assert count == (S if name == "own_lists" else 1), count
        torch.cuda.synchronize()
        ms = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                ctx.process_device(d_in, d_in.stride(0), d_out, d_out.stride(0), T, hip_stream=stream.cuda_stream)
                e1.record(stream)
            stream.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        ctx.process_device(d_in, d_in.stride(0), d_out, d_out.stride(0), T, timing=True, hip_stream=stream.cuda_stream)
        stream.synchronize()
        (k1, k2), (n1, n2) = ctx.last_timing()
        ctx.close()
        med = float(np.median(ms))
        rec = {"tool": "stream_graphs_rate", "leg": name, "run": run, "streams": S, "frames": T, "lists": count,
               "ms": [round(v, 3) for v in ms], "median_ms": round(med, 3),
               "msamples_per_s": round(2.0 * S * T / med / 1e3, 1),
               "k1_ms": round(k1, 3), "k2_ms": round(k2, 3), "launches": [n1, n2]}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for run in range(a.runs):
        for name in ("one_list", "same_list", "own_lists"):
            leg(name, run)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
