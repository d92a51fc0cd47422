#!/usr/bin/env python3
"""What per-stream CWAVE inputs buy on the C2 shape: 256 streams, 2^20 frames, Shift -> Master, device
pointers, every stream with its own generated analytic signal; each leg with the 16-bit ROUND render and
with the C5 render (24-bit TPDF + MEW44, the serial render).

    python tools/stream_cwave_rate.py [--streams 256] [--frames 1048576] [--runs 3] [--steps 10]
                                      [--warmup 5] [--legs a,b,c,d] [--renders round,c5] [--out FILE]

Four legs per render and run, `--runs` runs of each in one session:
  a_one_input     one input (48 kHz CW_F64 stereo) context-wide: K0 + K2, the reference point of the session
  b_same_input    the same input given to every stream through icw_set_stream_input with
                  icw_enable_stream_cwave on (the count reads 1: a one-input context again, the same launches)
  c_merged        four inputs x streams / 4 in ONE context: 48 k CW_F64 stereo, 44.1 k CW_I16 stereo,
                  96 k CW_I16_F32 stereo, 48 k CW_F32 mono -- no K0, the output kernel reads the frames itself
  d_split         the same streams as four contexts of streams / 4, one per input, run one after the other
                  on one HIP stream -- what the file transcoder does without ICW_BATCH_MERGE_CWAVE
One JSON line per leg, render and run: Msamples/s (frames x 2 channels x streams per second of the call(s),
HIP events on the stream; the unit of bench.py), the median, and the K0 / K2 kernel time per call summed
over the launch blocks (icw_last_k0_timing, icw_last_timing, taken in one extra timed call so that the event
records stay out of the rate; d_split: summed over its four contexts)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def device_iq(torch, S, T, fs, ch, seed):
    """[S, T, ch, 2] float64 (Re, Im) on the device: per stream and channel two complex exponentials, one
    of positive and one of negative frequency, at -12 dBFS each on the 16-bit scale"""
    rng = np.random.default_rng(seed)
    f = torch.tensor(rng.uniform(40.0, 0.4 * fs, size=(S, ch, 2)) * np.array([1.0, -1.0]), device="cuda")
    ph = torch.tensor(rng.uniform(0, 2 * np.pi, size=(S, ch, 2)), device="cuda")
    out = torch.empty((S, T, ch, 2), dtype=torch.float64, device="cuda")
    a = 32767.0 * 10 ** (-12 / 20)
    chunk = 1 << 16
    for t0 in range(0, T, chunk):
        t = torch.arange(t0, min(T, t0 + chunk), device="cuda", dtype=torch.float64) / fs
        for c in range(ch):
            arg = 2 * np.pi * f[:, c, :, None] * t[None, None, :] + ph[:, c, :, None]      # [S, 2, n]
            out[:, t0:t0 + t.numel(), c, 0] = a * torch.cos(arg).sum(1)
            out[:, t0:t0 + t.numel(), c, 1] = a * torch.sin(arg).sum(1)
    return out


def pack(torch, abi, iq, fmt):
    """the signal in the CWAVE frame format fmt: uint8 [S, T * frame bytes]"""
    S, T, ch, _ = iq.shape
    i16 = lambda v: torch.clamp(torch.round(v), -32768, 32767).to(torch.int16)
    if fmt == abi.FMT_CW_F64:
        return iq.contiguous().view(torch.uint8).reshape(S, T * ch * 16)
    if fmt == abi.FMT_CW_F32:
        return iq.to(torch.float32).contiguous().view(torch.uint8).reshape(S, T * ch * 8)
    if fmt == abi.FMT_CW_I16:
        return i16(iq).contiguous().view(torch.uint8).reshape(S, T * ch * 4)
    if fmt == abi.FMT_CW_I16_F32:
        b = torch.empty((S, T, ch, 6), dtype=torch.uint8, device="cuda")
        b[..., :2] = i16(iq[..., 0]).contiguous().view(torch.uint8).reshape(S, T, ch, 2)
        b[..., 2:] = iq[..., 1].to(torch.float32).contiguous().view(torch.uint8).reshape(S, T, ch, 4)
        return b.reshape(S, T * ch * 6)
    raise ValueError(fmt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--legs", default="a,b,c,d", help="the legs to run, by their first letters")
    ap.add_argument("--renders", default="round,c5")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    from in_cwave_amd import abi, graph
    from in_cwave_amd import lib as L

    S, T = a.streams, a.frames
    assert S % 4 == 0
    Q = S // 4
    inputs = [(48000, abi.FMT_CW_F64, 2), (44100, abi.FMT_CW_I16, 2), (96000, abi.FMT_CW_I16_F32, 2), (48000, abi.FMT_CW_F32, 1)]
    one = inputs[0]
    nodes = graph.graph_shift_master()
    # one buffer for the merged context, rows of the widest frame (CW_F64 stereo); the split contexts read the
    # same memory (a view of their rows); the one-input legs their own buffer
    wide = max(abi.FMT_BYTES[f] * ch for _, f, ch in inputs)
    d_in = torch.zeros((S, T * wide), dtype=torch.uint8, device="cuda")
    d_one = torch.empty((S, T * wide), dtype=torch.uint8, device="cuda")
    for q, (rate, fmt, ch) in enumerate(inputs):
        rows = pack(torch, abi, device_iq(torch, Q, T, rate, ch, 1000 + q), fmt)
        d_in[q * Q:(q + 1) * Q, :rows.shape[1]] = rows
        d_one[q * Q:(q + 1) * Q] = pack(torch, abi, device_iq(torch, Q, T, one[0], one[2], 2000 + q), one[1])
        del rows
    stream = torch.cuda.Stream()
    lines = []

    def config(render, rate, fmt, ch):
        cfg = graph.default_config(rate, fmt=fmt, channels=ch, need24bits=render == "c5")
        if render == "c5":
            cfg.render.render_type, cfg.render.nshape_type = abi.RENDER_TPDF, abi.NSHAPE_MEW44
        return cfg

    def leg(name, render, run, d_out):
        if name == "d_split":
            ctxs = []
            for q, (rate, fmt, ch) in enumerate(inputs):
                c = L.Context(config(render, rate, fmt, ch), nodes, Q)
                ctxs.append((c, d_in[q * Q:(q + 1) * Q], d_out[q * Q:(q + 1) * Q]))
            count = len(ctxs)
        else:
            ctx = L.Context(config(render, *one), nodes, S)
            if name == "b_same_input":
                ctx.enable_stream_cwave()
                ctx.set_stream_input(*one)
            elif name == "c_merged":
                ctx.enable_stream_cwave()
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
        k0 = k2 = 0.0
        n2 = 0
        for c, i, o in ctxs:
            c.process_device(i, i.stride(0), o, o.stride(0), T, timing=True, hip_stream=stream.cuda_stream)
            stream.synchronize()
            (_, x2), (_, m2) = c.last_timing()
            k0, k2, n2 = k0 + c.last_k0_ms(), k2 + x2, n2 + m2
        for c, _, _ in ctxs:
            c.close()
        med = float(np.median(ms))
        rec = {"tool": "stream_cwave_rate", "leg": name, "render": render, "run": run, "streams": S, "frames": T,
               "contexts": len(ctxs), "inputs": count, "ms": [round(v, 3) for v in ms], "median_ms": round(med, 3),
               "msamples_per_s": round(2.0 * S * T / med / 1e3, 1), "k0_ms": round(k0, 3), "k2_ms": round(k2, 3),
               "launches": n2}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for render in a.renders.split(","):
        assert render in ("round", "c5"), render
        d_out = torch.empty((S, T * (6 if render == "c5" else 4)), dtype=torch.uint8, device="cuda")
        for run in range(a.runs):
            for name in ("a_one_input", "b_same_input", "c_merged", "d_split"):
                if name[0] in a.legs.split(","):
                    leg(name, render, run, d_out)
        del d_out
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
