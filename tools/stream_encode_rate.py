#!/usr/bin/env python3
"""What per-stream inputs buy the CWAVE encoders on the C2 shape: 256 streams, 2^20 frames, device pointers, to
ICW_FMT_CW_F64, every stream with its own generated input.

    python tools/stream_encode_rate.py [--streams 256] [--frames 1048576] [--runs 3] [--steps 3] [--warmup 1]
                                       [--encoders iir,fir] [--taps 254] [--legs a,b,c,d] [--out FILE]

Per encoder (iir: icw_encode_cwave_iir, filter type 1, Kahan sums with the reject; fir: icw_encode_cwave with
k_M = --taps, k_beta 8) four legs per run, `--runs` runs of each in one session:
  a_one_input     one input (48 kHz int16 stereo), icw_enable_stream_encode never called: the reference point
  b_same_input    the same input given to every stream through icw_set_stream_input with the opt-in on (the
                  count reads 1: the same launches)
  c_merged        four inputs x streams / 4 in ONE context: 44.1 k int16 stereo, 48 k int16 stereo, 96 k int24
                  stereo, 48 k float32 mono
  d_split         the same streams as four contexts of streams / 4, one per input, run one after the other
                  on one HIP stream -- what the file encoders do without ICW_ENC_MERGE_INPUTS
One JSON line per encoder, leg and run: the call times in ms (HIP events on the stream), their median, and
Mframes/s (streams x frames per second of the call(s)), and the library (ICW_LIB names an A/B build beside
libicw.so; leg a runs on a build without the opt-in)."""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from stream_inputs_rate import device_pcm16, pack  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--encoders", default="iir,fir")
    ap.add_argument("--taps", type=int, default=254)
    ap.add_argument("--legs", default="a,b,c,d", help="the legs to run, by their first letters")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    from in_cwave_amd import abi, graph
    from in_cwave_amd import lib as L

    S, T = a.streams, a.frames
    assert S % 4 == 0
    Q = S // 4
    cw = abi.FMT_CW_F64
    inputs = [(44100, abi.FMT_I16, 2), (48000, abi.FMT_I16, 2), (96000, abi.FMT_I24, 2), (48000, abi.FMT_F32, 1)]
    wide = max(abi.FMT_BYTES[f] * ch for _, f, ch in inputs)
    d_in = torch.zeros((S, T * wide), dtype=torch.uint8, device="cuda")
    for q, (rate, fmt, ch) in enumerate(inputs):
        pcm = device_pcm16(torch, Q, T, rate, 1000 + q)
        if ch == 2:
            rows = pack(torch, abi, pcm, fmt)
        else:                                                # the one mono input: the left channel as float32
            rows = (pcm[:, :, 0].to(torch.float32) / 32768.0).contiguous().view(torch.uint8).reshape(Q, T * 4)
        d_in[q * Q:(q + 1) * Q, :rows.shape[1]] = rows
        del pcm, rows
    d_one = pack(torch, abi, device_pcm16(torch, S, T, 48000, 2000), abi.FMT_I16).contiguous()
    FB = L.cwave_frame_bytes(cw, 2)
    d_out = torch.empty((S, T * FB), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    lines = []

    def make(enc, inp, n, opt_in):
        rate, fmt, ch = inp
        c = L.Context(graph.default_config(rate, fmt=fmt, channels=ch, hilbert_type=1), graph.graph_shift_master(), n)
        if opt_in:
            c.enable_stream_encode()
            if enc == "fir":
                c.enable_stream_fir()
        if enc == "fir":
            c.set_fir_hilbert(a.taps, 8.0)
        return c

    def leg(enc, name, run):
        if name == "d_split":
            ctxs = [(make(enc, inp, Q, False), d_in[q * Q:(q + 1) * Q], d_out[q * Q:(q + 1) * Q]) for q, inp in enumerate(inputs)]
            count = len(ctxs)
        else:
            ctx = make(enc, (48000, abi.FMT_I16, 2), S, name != "a_one_input")
            if name == "b_same_input":
                ctx.set_stream_input(48000, abi.FMT_I16, 2)
            elif name == "c_merged":
                for q, (rate, fmt, ch) in enumerate(inputs):
                    ctx.set_stream_input(rate, fmt, ch, q * Q, Q)
            count = ctx.stream_input_count()
            assert count == (4 if name == "c_merged" else 1), count
            ctxs = [(ctx, d_in if name == "c_merged" else d_one, d_out)]

        def call():
            for c, i, o in ctxs:
                fn = c.encode_cwave_iir_device if enc == "iir" else c.encode_cwave_device
                fn(i, i.stride(0), o, o.stride(0), T, cw, hip_stream=stream.cuda_stream)

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
        k1_kernel = ctxs[0][0].last_k1_kernel() if enc == "iir" else None
        for c, _, _ in ctxs:
            c.close()
        med = float(np.median(ms))
        rec = {"tool": "stream_encode_rate", "encoder": enc, "leg": name, "run": run, "streams": S, "frames": T,
               "contexts": len(ctxs), "inputs": count, "ms": [round(v, 3) for v in ms], "median_ms": round(med, 3),
               "mframes_per_s": round(S * T / med / 1e3, 1), "k1_kernel": k1_kernel,
               "taps": a.taps if enc == "fir" else None, "lib": os.environ.get("ICW_LIB", "libicw.so")}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for enc in a.encoders.split(","):
        for run in range(a.runs):
            for name in ("a_one_input", "b_same_input", "c_merged", "d_split"):
                if name[0] in a.legs.split(","):
                    leg(enc, name, run)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
