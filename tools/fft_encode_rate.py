#!/usr/bin/env python3
"""Rate of the direct-FFT CWAVE encoder on the C2 shape: 256 stereo int16 tracks of 2^20 frames, device
pointers, to ICW_FMT_CW_F64 and to ICW_FMT_CW_I16, beside the FIR encoder's kernel (icw_encode_cwave at
k_M 254, what icw_cwave_encode_files runs) on the same input in the same session.

    python tools/fft_encode_rate.py [--tracks 256] [--frames 1048576] [--runs 3] [--steps 3] [--warmup 1]
                                    [--out FILE]

One JSON line per leg and run: Msamples/s (frames x 2 channels x tracks per second of the call, HIP events
on the stream; the unit of bench.py), the median, and for the FFT legs the time of every pass (one extra call
with ICW_FFT_TIMING=1, so that the event records stay out of the rate), the bytes each pass moves to and from
HBM by its structure (workspace points 16 B, PCM frames, file frames) and the HBM rate that implies."""
import argparse
import ctypes as C
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    from in_cwave_amd import abi, graph
    from in_cwave_amd import lib as L

    S, T = a.tracks, a.frames
    lib = L.load()
    gen = torch.Generator(device="cuda").manual_seed(20)
    d_in = torch.randint(-30000, 30001, (S, T * 2), dtype=torch.int16, device="cuda", generator=gen).view(torch.uint8)
    fsz = 4
    stream = torch.cuda.Stream()
    lines = []
    P = 1
    while P < T:
        P *= 2
    passes = L.encode_cwave_fft_passes(T)

    def timed(call):
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
        return ms

    def emit(rec, ms):
        med = float(np.median(ms))
        rec.update({"tool": "fft_encode_rate", "tracks": S, "frames": T, "ms": [round(v, 3) for v in ms],
                    "median_ms": round(med, 3), "msamples_per_s": round(2.0 * S * T / med / 1e3, 1)})
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def fft_leg(cw_format, name, run):
        fb = L.cwave_frame_bytes(cw_format, 2)
        d_out = torch.empty((S, T * fb), dtype=torch.uint8, device="cuda")
        ioff, ooff, nfr = [s * T * fsz for s in range(S)], [s * T * fb for s in range(S)], [T] * S

        def call():
            L.encode_cwave_fft_device(d_in, ioff, nfr, abi.FMT_I16, 2, d_out, ooff, cw_format, hip_stream=stream.cuda_stream)

        ms = timed(call)
        os.environ["ICW_FFT_TIMING"] = "1"
        call()
        os.environ["ICW_FFT_TIMING"] = "0"
        buf = (C.c_double * 64)()
        k = lib.icw_encode_cwave_fft_last_ms(buf, 64)
        pass_ms = [buf[i] for i in range(min(k, 64))]
        # bytes by the pass structure, per track: the first pass reads the PCM, the last reads it again and
        # writes the frames, every other side of a pass is the P-point workspace
        ws = 16 * P
        moved = []
        for j in range(k):
            rd = T * fsz if j == 0 else ws
            wr = T * fb + T * fsz if j == k - 1 else ws
            moved.append(S * (rd + wr))
        med = float(np.median(ms))
        emit({"leg": name, "run": run, "cw_format": cw_format, "P": P, "passes_per_direction": passes, "kernels": k,
              "pass_ms": [round(v, 3) for v in pass_ms], "pass_hbm_gb_per_s": [round(b / v / 1e6, 1) for b, v in zip(moved, pass_ms)],
              "bytes_per_frame": round(sum(moved) / (S * T), 1), "algorithmic_bytes_per_frame": round(2 * 16 * P / T, 1),
              "hbm_gb_per_s": round(sum(moved) / med / 1e6, 1)}, ms)
        del d_out

    def fir_leg(run):
        cw_format = abi.FMT_CW_F64
        fb = L.cwave_frame_bytes(cw_format, 2)
        d_out = torch.empty((S, T * fb), dtype=torch.uint8, device="cuda")
        ctx = L.Context(graph.default_config(48000), graph.graph_shift_master(), S)
        ctx.set_fir_hilbert(254, 8.0)

        def call():
            ctx.encode_cwave_device(d_in, T * fsz, d_out, T * fb, T, cw_format, hip_stream=stream.cuda_stream)

        ms = timed(call)
        ctx.close()
        emit({"leg": "fir_k254_f64", "run": run, "cw_format": cw_format}, ms)
        del d_out

    for run in range(a.runs):
        fft_leg(abi.FMT_CW_F64, "fft_f64", run)
        fft_leg(abi.FMT_CW_I16, "fft_i16", run)
        fir_leg(run)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
