#!/usr/bin/env python3
"""What per-stream inputs buy on the C2 shape: 256 stereo streams, 2^20 frames, Shift -> Master, 16-bit
ROUND render, device pointers, every stream with its own generated input.

    python tools/stream_inputs_rate.py [--streams 256] [--frames 1048576] [--runs 3] [--steps 3]
                                       [--warmup 1] [--legs a,b,c,d] [--out FILE]

Four legs per run, `--runs` runs of each in one session:
  a_one_input     one input (48 kHz int16) through icw_set_input: the reference point of the session
  b_same_input    the same input given to every stream through icw_set_stream_input (the count reads 1:
                  a one-input context again, the same launches)
  c_merged        four inputs x streams / 4 in ONE context: 44.1 k int16, 48 k int16, 96 k int24, 48 k float32
  d_split         the same streams as four contexts of streams / 4, one per input, run one after the
                  other on one HIP stream -- what the file transcoder does without ICW_BATCH_MERGE_INPUTS
One JSON line per leg and run: Msamples/s (frames x 2 channels x streams per second of the call(s), HIP
events on the stream; the unit of bench.py), the median, and the K0 / K1 / K2 kernel time per call summed
over the launch blocks (icw_last_k0_timing, icw_last_timing, taken in one extra timed call so that the event
records stay out of the rate; d_split: summed over its four contexts)."""
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
    ap.add_argument("--legs", default="a,b,c,d", help="the legs to run, by their first letters")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    from in_cwave_amd import abi, graph
    from in_cwave_amd import lib as L

    S, T = a.streams, a.frames
    assert S % 4 == 0
    Q = S // 4
    inputs = [(44100, abi.FMT_I16, 2), (48000, abi.FMT_I16, 2), (96000, abi.FMT_I24, 2), (48000, abi.FMT_F32, 2)]
    cfg = graph.default_config(48000)
    nodes = graph.graph_shift_master()
    # one buffer for the merged context, rows of the widest frame (float32 stereo); the split contexts and
    # the one-input legs read the same memory (a view of their rows, or the 48 kHz int16 quarter)
    wide = max(abi.FMT_BYTES[f] * ch for _, f, ch in inputs)
    d_in = torch.zeros((S, T * wide), dtype=torch.uint8, device="cuda")
    for q, (rate, fmt, ch) in enumerate(inputs):
        rows = pack(torch, abi, device_pcm16(torch, Q, T, rate, 1000 + q), fmt)
        d_in[q * Q:(q + 1) * Q, :rows.shape[1]] = rows
    d_one = pack(torch, abi, device_pcm16(torch, S, T, 48000, 2000), abi.FMT_I16).contiguous()
    d_out = torch.empty((S, T * 4), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    lines = []

    def leg(name, run):
        if name == "d_split":
            ctxs = []
            for q, (rate, fmt, ch) in enumerate(inputs):
                c = L.Context(graph.default_config(rate, fmt=fmt, channels=ch), nodes, Q)
                ctxs.append((c, d_in[q * Q:(q + 1) * Q], d_out[q * Q:(q + 1) * Q]))
            count = len(ctxs)
        else:
            ctx = L.Context(cfg, nodes, S)
            if name == "a_one_input":
                ctx.set_input(48000, abi.FMT_I16, 2)
            elif name == "b_same_input":
                ctx.set_stream_input(48000, abi.FMT_I16, 2)
            else:
                for q, (rate, fmt, ch) in enumerate(inputs):
                    ctx.set_stream_input(rate, fmt, ch, q * Q, Q)
            count = ctx.stream_input_count()
            assert count == (4 if name == "c_merged" else 1), count
            ctxs = [(ctx, d_in if name == "c_merged" else d_one, d_out)]

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
        k0 = k1 = k2 = 0.0
        n1 = n2 = 0
        for c, i, o in ctxs:
            c.process_device(i, i.stride(0), o, o.stride(0), T, timing=True, hip_stream=stream.cuda_stream)
            stream.synchronize()
            (x1, x2), (m1, m2) = c.last_timing()
            k0, k1, k2, n1, n2 = k0 + c.last_k0_ms(), k1 + x1, k2 + x2, n1 + m1, n2 + m2
        k1_kernel = ctxs[0][0].last_k1_kernel()
        for c, _, _ in ctxs:
            c.close()
        med = float(np.median(ms))
        rec = {"tool": "stream_inputs_rate", "leg": name, "run": run, "streams": S, "frames": T, "contexts": len(ctxs),
               "inputs": count, "ms": [round(v, 3) for v in ms], "median_ms": round(med, 3),
               "msamples_per_s": round(2.0 * S * T / med / 1e3, 1),
               "k0_ms": round(k0, 3), "k1_ms": round(k1, 3), "k2_ms": round(k2, 3), "launches": [n1, n2], "k1_kernel": k1_kernel}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for run in range(a.runs):
        for name in ("a_one_input", "b_same_input", "c_merged", "d_split"):
            if name[0] in a.legs.split(","):
                leg(name, run)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
