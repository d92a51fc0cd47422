#!/usr/bin/env python3
"""Encode rate of the CWAVE encoder (icw_encode_cwave, kernel KFE) on the C2 shape: 256 x 48 kHz stereo
int16 streams, k_M 254 (Kaiser beta 8), device pointers, timed with HIP events on the call's stream.

    python tools/encode_rate.py [--streams 256] [--frames 1048576] [--steps 5] [--warmup 1] [--out FILE]

Prints one JSON line per output format (ICW_FMT_CW_F64 and ICW_FMT_CW_I16): Msamples/s (frames x 2
channels x streams per second, the unit of bench.py), the HBM bytes written and read per frame, and the
store bandwidth that rate amounts to.  Every stream holds the same synthetic track (the rate does not
depend on the data).  Run `python bench.py --gpus 1 --workload c2fir` in the same session for the
converter's rate with the graph and the render behind it.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--order", type=int, default=254)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    from in_cwave_amd import abi, graph, synth
    from in_cwave_amd import lib as L

    S, T = a.streams, a.frames
    cfg = graph.default_config(48000)
    row = torch.from_numpy(synth.stream_pcm(0, T, 48000).copy()).cuda()
    d_in = row.repeat(S, 1).contiguous()
    stream = torch.cuda.Stream()
    lines = []
    for name, cw in (("cw_f64", abi.FMT_CW_F64), ("cw_i16", abi.FMT_CW_I16)):
        fb = L.cwave_frame_bytes(cw, 2)
        d_out = torch.empty((S, T * fb), dtype=torch.uint8, device="cuda")
        ctx = L.Context(cfg, graph.graph_shift_master(), S)
        ctx.set_fir_hilbert(a.order, 8.0)
        torch.cuda.synchronize()
        ms = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                ctx.encode_cwave_device(d_in, d_in.stride(0), d_out, d_out.stride(0), T, cw, hip_stream=stream.cuda_stream)
                e1.record(stream)
            stream.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        ctx.close()
        med = float(np.median(ms))
        rec = {"tool": "encode_rate", "format": name, "streams": S, "frames": T, "order": a.order,
               "ms": [round(v, 3) for v in ms], "median_ms": round(med, 3),
               "msamples_per_s": round(2.0 * S * T / med / 1e3, 1),
               "bytes_written_per_frame": fb, "bytes_read_per_frame": 4,
               "store_gb_per_s": round(S * T * fb / med / 1e6, 1),
               # per channel sample and odd tap: one subtraction and one FMA = 3 flop
               "tap_tflops": round(2.0 * S * T * ((a.order // 2 + 1) // 2) * 3 / med / 1e9, 2)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del d_out
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
