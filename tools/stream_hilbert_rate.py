#!/usr/bin/env python3
"""What per-stream Hilbert converters buy on the C2 shape: 256 stereo streams, 2^20 frames of int16, Shift ->
Master, 16-bit ROUND, device pointers, every stream with its own generated input.

    python tools/stream_hilbert_rate.py [--streams 256] [--frames 1048576] [--runs 3] [--steps 10]
                                        [--warmup 5] [--legs a,b,c,d,e] [--out FILE]

Five legs per run, `--runs` runs of each in one session (every setting Kahan + reject, the row form's):
  a_one_setting    one setting (type 0) through icw_set_hilbert_filter + icw_set_hilbert_config: the reference point
  b_same_setting   the same setting given to every stream through icw_set_stream_hilbert (the count reads 1: a
                   one-setting context again, the same launches)
  c_merged         four entries x streams / 4 consecutive streams in ONE context: types 0 / 2 / 1 / 4 (orders
                   15 / 18 / 19 / 20) -- four runs, one mixed recurrence launch per block
  d_split          the same streams as four contexts of streams / 4, one per entry, run one after the other on
                   one HIP stream
  e_interleaved    the four entries interleaved stream by stream in ONE context: as many runs as streams, the
                   cost of many runs (every run rounds up to a wave pair, and K2 is one launch per run)
One JSON line per leg and run: Msamples/s (frames x 2 channels x streams per second of the call(s), HIP events
on the stream; the unit of bench.py), the median, and the K1 time and the output side's time (K2) per call
summed over the launch blocks (icw_last_timing, taken in one extra timed call so that the event records stay
out of the rate; d_split: summed over its four contexts), and the K1 form of that call."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tools.stream_render_rate import device_tones  # noqa: E402

TYPES = (0, 2, 1, 4)
LEGS = ("a_one_setting", "b_same_setting", "c_merged", "d_split", "e_interleaved")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--legs", default="a,b,c,d,e", help="the legs to run, by their first letters")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    from in_cwave_amd import abi, graph
    from in_cwave_amd import lib as L

    S, T = a.streams, a.frames
    assert S % 4 == 0
    Q = S // 4
    cfg = graph.default_config(48000)
    nodes = graph.graph_shift_master()
    tones = device_tones(torch, S, T, 48000, 3000)
    d_in = torch.clamp(torch.round(tones), -32768, 32767).to(torch.int16).contiguous().view(torch.uint8).reshape(S, T * 4)
    del tones
    d_out = torch.empty((S, T * 4), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    lines = []

    def leg(name, run):
        if name == "d_split":
            ctxs = []
            for q, t in enumerate(TYPES):
                c = L.Context(abi.Config.from_buffer_copy(cfg), nodes, Q)
                c.set_hilbert_filter(t)
                c.set_hilbert_config(1, 1)
                ctxs.append((c, d_in[q * Q:(q + 1) * Q], d_out[q * Q:(q + 1) * Q]))
            count = len(ctxs)
        else:
            ctx = L.Context(abi.Config.from_buffer_copy(cfg), nodes, S)
            if name == "a_one_setting":
                ctx.set_hilbert_filter(TYPES[0])
                ctx.set_hilbert_config(1, 1)
            elif name == "b_same_setting":
                ctx.set_stream_hilbert(TYPES[0], 1, 1)
            elif name == "c_merged":
                for q, t in enumerate(TYPES):
                    ctx.set_stream_hilbert(t, 1, 1, q * Q, Q)
            else:
                for s in range(S):
                    ctx.set_stream_hilbert(TYPES[s % 4], 1, 1, s, 1)
            count = ctx.stream_hilbert_count()
            assert count == (4 if name in ("c_merged", "e_interleaved") else 1), count
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
        form = []
        for c, i, o in ctxs:
            c.process_device(i, i.stride(0), o, o.stride(0), T, timing=True, hip_stream=stream.cuda_stream)
            stream.synchronize()
            (x1, x2), (m1, m2) = c.last_timing()
            k1, k2, n1, n2 = k1 + x1, k2 + x2, n1 + m1, n2 + m2
            form.append(c.last_k1_kernel())
        for c, _, _ in ctxs:
            c.close()
        med = float(np.median(ms))
        rec = {"tool": "stream_hilbert_rate", "leg": name, "run": run, "streams": S, "frames": T,
               "contexts": len(ctxs), "settings": count, "ms": [round(v, 3) for v in ms], "median_ms": round(med, 3),
               "msamples_per_s": round(2.0 * S * T / med / 1e3, 1),
               "k1_ms": round(k1, 3), "k2_ms": round(k2, 3), "launch_blocks": [n1, n2],
               "k1_form": sorted(set(form))}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for run in range(a.runs):
        for name in LEGS:
            if name[0] in a.legs.split(","):
                leg(name, run)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
