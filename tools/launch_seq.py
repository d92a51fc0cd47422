#!/usr/bin/env python3
"""The kernel launches of one call in each branch of the host scheduler, for comparing two builds.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/launch_seq.py
    python tools/launch_seq.py --reduce DIR/.../*_kernel_trace.csv [--drop queue] > listing.txt

Without arguments: one call each over a fixed list of small configurations (below), ending at the
first error.  Tracing only -- collect counters in a run of their own.  --reduce turns the trace into
one line per dispatch, in dispatch order: kernel name, grid size, workgroup size, LDS bytes, queue id
(--drop queue leaves the last column out, for when the ids the runtime deals do not repeat from run
to run).  The runtime's own fill and copy kernels (hipMemset, hipMemcpy) are dispatches like any
other and are listed.  Two builds launch the same kernels when their listings are equal; select the
other build with ICW_LIB (tools/ab_lib.sh).
"""
import argparse
import csv
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SWITCHES = ("ICW_BLOCK", "ICW_FIR_FUSED", "ICW_K1_MODE")


def run():
    from in_cwave_amd import abi, graph, synth
    from in_cwave_amd import lib as L

    def ctx_for(nodes, streams, env=None, fir=0, **cfg_kw):
        """the switches are read when the context is created"""
        render = cfg_kw.pop("render", None)
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env or {})
        cfg = graph.default_config(48000, **cfg_kw)
        if render:
            cfg.render.render_type, cfg.render.nshape_type = render
        ctx = L.Context(cfg, nodes, streams, device=0)
        if fir:
            ctx.set_fir_hilbert(fir, 8.0)
        return ctx

    def call(name, ctx, frames, channels=2, pinned=False, lists=None):
        for s, nodes in enumerate(lists or []):
            ctx.set_stream_graph(nodes, first=s, count=1)
        raw = synth.batch_pcm(ctx.n_streams, frames, 48000, channels=channels)
        out = None
        if pinned:
            buf = L.host_array(raw.shape)
            buf[:] = raw
            raw = buf
            out = L.host_array((ctx.n_streams, frames * 2 * ctx.render_size))
        ctx.process(raw, frames, out=out)
        ctx.close()
        print(f"launch_seq: {name}", flush=True)

    sm, mo = graph.graph_shift_master(), graph.graph_master_only()
    four = [sm, mo, graph.graph_pm_shift_mix(), [graph.master(inputs=("A",)), graph.pm(inputs=("in",), out="A")]]
    blk = {"ICW_BLOCK": "1024"}
    tpdf_shaped, tpdf_flat = (abi.RENDER_TPDF, abi.NSHAPE_FW44), (abi.RENDER_TPDF, abi.NSHAPE_FLAT)

    call("K5, zero-copy", ctx_for(sm, 1), 576)
    call("row K1, one block", ctx_for(sm, 4), 3000)
    call("several blocks, two sets, tail", ctx_for(sm, 4, blk), 5000)
    call("plain K1, dedup, CU split", ctx_for(mo, 300, channels=1), 2048, channels=1)
    call("serial render, dither stream", ctx_for(sm, 4, blk, need24bits=True, render=tpdf_shaped), 5000)
    call("frame-parallel dither", ctx_for(sm, 4, render=tpdf_flat), 3000)
    call("bus-form list (K4)", ctx_for(graph.graph_pure_delay(), 4), 3000)
    call("four lists (mix)", ctx_for(sm, 4), 3000, lists=four)
    call("four lists, pipelined I/O", ctx_for(sm, 4, {"ICW_BLOCK": "8192"}), 40000, pinned=True, lists=four)
    call("FIR 255 taps, fused", ctx_for(sm, 4, fir=254), 3000)
    call("FIR 255 taps, two kernels", ctx_for(sm, 4, {"ICW_FIR_FUSED": "0", **blk}, fir=254), 5000)
    call("FIR + serial render (ramp)", ctx_for(sm, 4, fir=254, need24bits=True, render=tpdf_shaped), 70000)
    for cw in (abi.FMT_CW_F64, abi.FMT_CW_I16):
        ctx = ctx_for(sm, 4, fir=254)
        ctx.encode_cwave(synth.batch_pcm(4, 3000, 48000), 3000, cw)
        ctx.close()
        print(f"launch_seq: icw_encode_cwave {cw}", flush=True)
    for channels in (1, 2):
        for mode in ("plain", "row"):
            ctx = ctx_for(sm, 4, {"ICW_K1_MODE": mode, **blk}, channels=channels)
            ctx.encode_cwave_iir(synth.batch_pcm(4, 3000, 48000, channels=channels), 3000, abi.FMT_CW_F64)
            ctx.close()
            print(f"launch_seq: icw_encode_cwave_iir {channels} ch, {mode} K1", flush=True)


def reduce(path, drop):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    if not rows:
        sys.exit(f"{path}: no dispatches")
    low = {k.lower(): k for k in rows[0]}

    def col(*names):
        for n in names:
            if n in low:
                return low[n]
        sys.exit(f"{path}: none of the columns {names}")

    order = col("dispatch_id", "start_timestamp")
    name, queue = col("kernel_name"), col("queue_id")
    lds = col("lds_block_size", "group_segment_size", "lds_block_size_v")
    grid = [col(f"grid_size_{a}", f"grid_size{a}") for a in "xyz"]
    wg = [col(f"workgroup_size_{a}", f"workgroup_size{a}") for a in "xyz"]
    rows.sort(key=lambda r: int(r[order]))
    for r in rows:
        f = [r[name], "x".join(r[c] for c in grid), "x".join(r[c] for c in wg), r[lds]]
        if "queue" not in drop:
            f.append(r[queue])
        print("\t".join(f))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reduce", metavar="CSV", help="reduce a rocprofv3 kernel trace to a listing")
    ap.add_argument("--drop", action="append", default=[], choices=["queue"])
    a = ap.parse_args()
    reduce(a.reduce, a.drop) if a.reduce else run()
