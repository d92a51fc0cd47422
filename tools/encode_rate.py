#!/usr/bin/env python3
"""Encode rate of the CWAVE encoders on the C2 shape: 256 x 48 kHz stereo int16 streams, device pointers,
timed with HIP events on the call's stream.  --converter fir (default): icw_encode_cwave, kernel KFE, k_M 254
(Kaiser beta 8).  --converter iir: icw_encode_cwave_iir (K0, K1, K2 up to `in`, the packer KIP), see below.

    python tools/encode_rate.py [--converter fir|iir] [--streams 256] [--frames 1048576] [--steps 5]
                                [--warmup 1] [--runs 1] [--out FILE]

Prints one JSON line per output format (ICW_FMT_CW_F64 and ICW_FMT_CW_I16): Msamples/s (frames x 2
channels x streams per second, the unit of bench.py), the HBM bytes written and read per frame, and the
store bandwidth that rate amounts to.  Every stream holds the same synthetic track (the rate does not
depend on the data).  Run `python bench.py --gpus 1 --workload c2fir` in the same session for the
converter's rate with the graph and the render behind it.

--converter iir prints, per run (--runs 2: the same measurement twice, for the spread):
  iir_c2_step     the C2 call on the same streams (icw_process_streams, Shift -> Master, 16-bit ROUND) with its
                  K1 and K2 time per step summed over the launch blocks (icw_last_timing) -- the yardstick:
                  the encode is expected to take the sum of the two, the packer and K0 hiding beside nothing
  iir_encode      icw_encode_cwave_iir to ICW_FMT_CW_F64 and to ICW_FMT_CW_I16, ms per call and its excess
                  over that sum
  iir_cw_decode   the C2 graph on the stored F64 frames (a CW_F64-input context, Hilbert bypassed) and its
                  rate over the real-input one: what encoding once buys every later decode
Run `python bench.py --gpus 1 --workload c2` in the same session for the benchmark's own c2 line.
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
    ap.add_argument("--converter", default="fir", choices=["fir", "iir"])
    ap.add_argument("--runs", type=int, default=1, help="iir: repeat the whole measurement this many times")
    a = ap.parse_args()
    if a.converter == "iir":
        return main_iir(a)

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


def main_iir(a):
    import torch

    from in_cwave_amd import abi, graph, synth
    from in_cwave_amd import lib as L

    S, T = a.streams, a.frames
    nodes = graph.graph_shift_master()
    row = torch.from_numpy(synth.stream_pcm(0, T, 48000).copy()).cuda()
    d_in = row.repeat(S, 1).contiguous()
    d_pcm = torch.empty((S, T * 4), dtype=torch.uint8, device="cuda")          # 16-bit stereo renders
    d_f64 = torch.empty((S, T * 32), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def timed(fn, after=None):
        """ms of the timed calls; after() runs behind each one, outside its events"""
        ms = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                fn()
                e1.record(stream)
            stream.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
                if after:
                    after()
        return ms

    def rate(ms):
        return round(2.0 * S * T / ms / 1e3, 1)

    for run in range(a.runs):
        base = {"tool": "encode_rate", "converter": "iir", "run": run, "streams": S, "frames": T}
        # ---- the C2 call and its K1 / K2 sums
        ctx = L.Context(graph.default_config(48000), nodes, S)
        k12 = []
        ms = timed(lambda: ctx.process_device(d_in, d_in.stride(0), d_pcm, d_pcm.stride(0), T, timing=True,
                                              hip_stream=stream.cuda_stream),
                   after=lambda: k12.append(ctx.last_timing()[0]))
        k1_kind = ctx.last_k1_kernel()
        ctx.close()
        # the last call's render.  Every context below makes the same number of calls, so the F64 frames left
        # in d_f64 are this call's analytic signal and their decode's last call must render these bytes
        ref_pcm = d_pcm.clone()
        c2_ms = float(np.median(ms))
        k1_ms, k2_ms = float(np.median([v[0] for v in k12])), float(np.median([v[1] for v in k12]))
        emit(dict(base, what="iir_c2_step", ms=[round(v, 3) for v in ms], median_ms=round(c2_ms, 3),
                  msamples_per_s=rate(c2_ms), k1_kernel=k1_kind, k1_sum_ms=round(k1_ms, 3), k2_sum_ms=round(k2_ms, 3),
                  k1_plus_k2_ms=round(k1_ms + k2_ms, 3)))
        # ---- the encode, to F64 and to I16
        for name, cw in (("cw_f64", abi.FMT_CW_F64), ("cw_i16", abi.FMT_CW_I16)):
            fb = L.cwave_frame_bytes(cw, 2)
            d_out = d_f64 if cw == abi.FMT_CW_F64 else torch.empty((S, T * fb), dtype=torch.uint8, device="cuda")
            ctx = L.Context(graph.default_config(48000), nodes, S)
            ms = timed(lambda: ctx.encode_cwave_iir_device(d_in, d_in.stride(0), d_out, d_out.stride(0), T, cw,
                                                           hip_stream=stream.cuda_stream))
            assert ctx.last_k1_kernel() == k1_kind
            ctx.close()
            med = float(np.median(ms))
            emit(dict(base, what="iir_encode", format=name, ms=[round(v, 3) for v in ms], median_ms=round(med, 3),
                      msamples_per_s=rate(med), bytes_written_per_frame=fb,
                      over_k1_plus_k2_pct=round(100.0 * (med / (k1_ms + k2_ms) - 1.0), 2),
                      over_c2_step_pct=round(100.0 * (med / c2_ms - 1.0), 2)))
        # ---- the stored F64 frames through the C2 graph
        ctx = L.Context(graph.default_config(48000, fmt=abi.FMT_CW_F64), nodes, S)
        ms = timed(lambda: ctx.process_device(d_f64, d_f64.stride(0), d_pcm, d_pcm.stride(0), T,
                                              hip_stream=stream.cuda_stream))
        ctx.close()
        med = float(np.median(ms))
        emit(dict(base, what="iir_cw_decode", format="cw_f64", ms=[round(v, 3) for v in ms], median_ms=round(med, 3),
                  msamples_per_s=rate(med), bytes_read_per_frame=32, load_gb_per_s=round(S * T * 32 / med / 1e6, 1),
                  times_the_real_input_rate=round(c2_ms / med, 2), bytes_equal_real_input=bool(torch.equal(d_pcm, ref_pcm))))
        del ref_pcm
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
