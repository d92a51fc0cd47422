#!/usr/bin/env python3
"""What per-stream FIR converters cost and buy, on the c2fir shape: 256 stereo int16 streams at 48 kHz, 2^20
frames, Shift -> Master, 16-bit ROUND render, device pointers, every stream with its own generated input.

    python tools/stream_firconv_rate.py [--streams 256] [--frames 1048576] [--runs 3] [--steps 10]
                                        [--warmup 5] [--legs a,b,c,d,e] [--out FILE]

The legs, `--runs` runs of each in one session:
  a_one           one converter (order 254, Kaiser beta 8) through icw_set_fir_hilbert
  b_same          the same through icw_set_stream_fir (count 1: the same launch blocks)
  c_merged        orders 30, 254, 510 and 1 022 x streams / 4 consecutive streams in ONE context: every launch's
                  LDS is sized by order 1 022, whatever order a workgroup runs
  d_split         the streams of c as four contexts of streams / 4, one converter each, one after the other on
                  one HIP stream
  e_merged_c5 / e_split_c5   c and d with the C5 render (24-bit TPDF + MEW44): the serial render bounds the
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
sys.path.insert(0, str(ROOT / "tools"))

from stream_fir_rate import device_pcm16, pack  # noqa: E402

ORDERS = (30, 254, 510, 1022)


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
    BETA = 8.0
    nodes = graph.graph_shift_master()
    d_in = pack(torch, abi, device_pcm16(torch, S, T, 48000, 2000), abi.FMT_I16).contiguous()
    d_out = torch.empty((S, T * 6), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    lines = []

    def config(c5=False):
        cfg = graph.default_config(48000, fmt=abi.FMT_I16, channels=2, need24bits=c5)
        if c5:
            cfg.render.render_type = abi.RENDER_TPDF
            cfg.render.nshape_type = abi.NSHAPE_MEW44
        return cfg

    def leg(name, run):
        c5 = name.endswith("_c5")
        if "split" in name:
            ctxs = []
            for q, order in enumerate(ORDERS):
                c = L.Context(config(c5), nodes, Q)
                c.set_fir_hilbert(order, BETA)
                ctxs.append((c, d_in[q * Q:(q + 1) * Q], d_out[q * Q:(q + 1) * Q]))
        else:
            ctx = L.Context(config(c5), nodes, S)
            ctx.enable_stream_fir()
            if name == "a_one":
                ctx.set_fir_hilbert(254, BETA)
            elif name == "b_same":
                ctx.set_stream_fir(254, BETA)
            else:
                ctx.set_stream_fir(ORDERS[0], BETA)
                for q, order in enumerate(ORDERS):
                    ctx.set_stream_fir(order, BETA, q * Q, Q)
            assert ctx.stream_fir_count() == (len(ORDERS) if "merged" in name else 1)
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
        rec = {"tool": "stream_firconv_rate", "leg": name, "run": run, "streams": S, "frames": T,
               "orders": [254] if name[0] in "ab" else list(ORDERS), "contexts": len(ctxs), "out_bytes_per_frame": 6 if c5 else 4,
               "ms": [round(v, 3) for v in ms], "median_ms": round(med, 3), "msamples_per_s": round(2.0 * S * T / med / 1e3, 1),
               "converter_ms": round(kf, 3), "launch_blocks": nb}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    names = ("a_one", "b_same", "c_merged", "d_split", "e_merged_c5", "e_split_c5")
    for run in range(a.runs):
        for name in names:
            if name[0] in a.legs.split(","):
                leg(name, run)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
