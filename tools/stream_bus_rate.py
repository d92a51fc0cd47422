#!/usr/bin/env python3
"""What per-stream bus-form DSP lists cost on the C2 shape: 256 x 48 kHz stereo int16 streams, 2^20 frames,
a self-feeding Mix -> Master (graph_leaky_feedback), 16-bit ROUND render, device pointers, every stream with its
own generated input.

    python tools/stream_bus_rate.py [--streams 256] [--frames 1048576] [--runs 3] [--steps 3]
                                    [--warmup 1] [--legs a,b,c,d,e] [--out FILE]

Five legs per run, `--runs` runs of each in one session:
  a one_list     one bus-form list through icw_set_graph (the reference point of the session)
  b same_list    the same list given to every stream through icw_set_stream_graph (the count reads 1: a
                 one-list context again, the same launches -- judge its rate against a's own spread)
  c own_lists    one list per stream, `--streams` feedback gains, one context: the mixed serial graph kernel,
                 every run one lane wide
  d four_ctx     the same lists as four contexts of streams / 4 in turn (their calls one after the other)
  e both_forms   c with register-form (Shift -> Master) and bus-form streams alternating, so the call is
                 forced into bus form
One JSON line per leg and run: Msamples/s (frames x 2 channels x streams per second of the call, HIP events
on its stream; the unit of bench.py), the median call, and the K1 / K2 kernel time per call summed over the
launch blocks (icw_last_timing, taken in one extra timed call so that the event records stay out of the rate;
the second figure runs to the end of the block's serial render, K4 included)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

LEGS = {"a": "one_list", "b": "same_list", "c": "own_lists", "d": "four_ctx", "e": "both_forms"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", default="a,b,c,d,e")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    from in_cwave_amd import graph
    from in_cwave_amd import lib as L
    from stream_graphs_rate import device_input

    S, T, fs = a.streams, a.frames, 48000
    cfg = graph.default_config(fs)
    base = graph.graph_leaky_feedback()
    d_in = device_input(torch, S, T, fs)
    d_out = torch.empty((S, T * 4), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    lines = []

    def own(s, both=False):
        if both and s % 2 == 0:
            return [graph.master(inputs=("A",)), graph.shift(inputs=("in",), out="A", fr=0.5 + 19.0 * s / max(1, S - 1))]
        return [graph.master(inputs=("C",)), graph.mix(inputs=("in", "C"), out="C", gain=0.25 + 0.5 * s / max(1, S - 1))]

    def context(name, first, count):
        ctx = L.Context(cfg, graph.graph_master_only(), count)
        if name == "one_list":
            assert ctx.set_graph(base)
        else:
            ctx.enable_stream_bus()
            if name == "same_list":
                assert ctx.set_stream_graph(base)
            else:
                for s in range(count):
                    assert ctx.set_stream_graph(own(first + s, name == "both_forms"), s, 1)
        return ctx

    def leg(name, run):
        parts = 4 if name == "four_ctx" else 1
        n = S // parts
        ctxs = [context(name, k * n, n) for k in range(parts)]
        count = sum(c.stream_graph_count() for c in ctxs)
        assert count == (1 if name in ("one_list", "same_list") else n * parts), count
        torch.cuda.synchronize()

        def step(timing=False):
            for k, c in enumerate(ctxs):
                c.process_device(d_in[k * n:], d_in.stride(0), d_out[k * n:], d_out.stride(0), T, timing=timing,
                                 hip_stream=stream.cuda_stream)

        ms = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                step()
                e1.record(stream)
            stream.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        k1 = k2 = 0.0
        launches = [0, 0]
        for k, c in enumerate(ctxs):       # a timed call per context: the event reads wait for it
            c.process_device(d_in[k * n:], d_in.stride(0), d_out[k * n:], d_out.stride(0), T, timing=True,
                             hip_stream=stream.cuda_stream)
            stream.synchronize()
            (x1, x2), (n1, n2) = c.last_timing()
            k1, k2, launches = k1 + x1, k2 + x2, [launches[0] + n1, launches[1] + n2]
            c.close()
        med = float(np.median(ms))
        rec = {"tool": "stream_bus_rate", "leg": name, "run": run, "streams": n * parts, "frames": T, "lists": count,
               "ms": [round(v, 3) for v in ms], "median_ms": round(med, 3),
               "msamples_per_s": round(2.0 * n * parts * T / med / 1e3, 1),
               "k1_ms": round(k1, 3), "k2_ms": round(k2, 3), "launches": launches}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    names = [LEGS[k.strip()] for k in a.legs.split(",") if k.strip()]
    for run in range(a.runs):
        for name in names:
            leg(name, run)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
