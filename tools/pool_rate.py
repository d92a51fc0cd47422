#!/usr/bin/env python3
"""What the slot pool (icw_transcode_files_pool) buys on a library of ragged lengths: `--files` stereo int16
48 kHz WAV files, lengths log-uniform between 2^16 and 2^20 frames (seeded), every file with its own
Shift -> Master list, 16-bit ROUND render, default block (65 536 frames).

    python tools/pool_rate.py [--files 1024] [--runs 3] [--dir /dev/shm/icw_pool_rate] [--slots 256,1024]
                              [--min-log2 16] [--max-log2 20] [--out FILE]

The library is generated into --dir (a tmpfs directory, so that the disk stays out of the figures) and removed
afterwards.  Legs, `--runs` runs of each in one session, the leg order reversed on every other run:
  a lists          icw_transcode_files_lists with ICW_BATCH_MERGE_INPUTS: one context of --files streams run
                   to the longest file
  b pool_<slots>   the pool at each --slots width, files as given
  c long_<slots>   the same widths, longest first
One JSON line per leg and run: wall_s and io_s (the call's own statistics), blocks, slot_blocks and
busy_slot_blocks (the plan's; for leg a files x ceil(longest / block) and the sum of the files' blocks), the
pinned staging bytes (2 input + 2 output buffers of slots x block frames), and max/mean of the lengths.  The file
entry points take no ICW_F_TIMING flag, so there is no kernel-time column: wall_s - io_s bounds the time the
host spent waiting for the device and in the refill boundaries."""
import argparse
import json
import resource
import shutil
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm/icw_pool_rate")
    ap.add_argument("--slots", default="256,1024")
    ap.add_argument("--min-log2", type=float, default=16.0)
    ap.add_argument("--max-log2", type=float, default=20.0)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    from in_cwave_amd import abi, graph, synth
    from in_cwave_amd import lib as L
    import wavgen as W

    # every file and its output stay open for a whole lists call
    soft, hard = resource.getrlimit(resource.RLIMIT_NOFILE)
    want = 2 * a.files + 256
    if soft < want:
        resource.setrlimit(resource.RLIMIT_NOFILE, (min(want, hard) if hard != resource.RLIM_INFINITY else want, hard))

    fs, B, n = 48000, 65536, a.files
    rng = np.random.default_rng(a.seed)
    lengths = [int(v) for v in np.exp2(rng.uniform(a.min_log2, a.max_log2, size=n))]
    root = Path(a.dir)
    shutil.rmtree(root, ignore_errors=True)
    (root / "out").mkdir(parents=True)
    # one generated track of the longest length; every file is a window of it from a seeded offset (wrapped)
    base = synth.stream_pcm(0, max(lengths), fs, channels=2, fmt=abi.FMT_I16).reshape(-1, 4)
    ins, lists = [], []
    for i, ln in enumerate(lengths):
        off = int(rng.integers(0, len(base)))
        d = np.concatenate([base[off:off + ln], base[:max(0, off + ln - len(base))]]).reshape(-1)
        ins.append(W.write(root / f"in_{i:05d}.wav", d, abi.FMT_I16, 2, fs, kind="pcm"))
        lists.append([graph.master(inputs=("A",)), graph.shift(out="A", fr=0.5 + 19.0 * i / max(1, n - 1))])
    outs = [root / "out" / f"out_{i:05d}.wav" for i in range(n)]
    cfg = graph.default_config(fs)
    nb = [-(-ln // B) for ln in lengths]
    shape = {"files": n, "max_over_mean": round(max(lengths) / (sum(lengths) / n), 3), "frames": sum(lengths)}
    widths = [int(s) for s in a.slots.split(",") if s.strip()]
    legs = [("lists", None, None)] + [(f"pool_{s}", s, abi.POOL_AS_GIVEN) for s in widths] + \
           [(f"long_{s}", s, abi.POOL_LONGEST_FIRST) for s in widths]
    lines = []
    try:
        for run in range(a.runs):
            for name, slots, order in (legs if run % 2 == 0 else legs[::-1]):
                if slots is None:
                    rc, st, status = L.transcode_files_lists(cfg, lists, ins, outs, merge_inputs=True)
                    bs, S = st, n
                    blocks, slot_blocks, busy, refills = max(nb), n * max(nb), sum(nb), 0
                else:
                    rc, st, status, _ = L.transcode_files_pool(cfg, lists, ins, outs, slots=slots, order=order, want_meters=False)
                    bs, S = st.batch, st.slots
                    blocks, slot_blocks, busy, refills = st.blocks, st.slot_blocks, st.busy_slot_blocks, st.refills
                assert rc == abi.OK and bs.n_files == n, (name, rc, bs.n_files)
                rec = dict(tool="pool_rate", leg=name, run=run, **shape, slots=S, wall_s=round(bs.wall_s, 4),
                           io_s=round(bs.io_s, 4), blocks=blocks, slot_blocks=slot_blocks, busy_slot_blocks=busy,
                           busy_ratio=round(busy / slot_blocks, 4), refills=refills, pinned_bytes=2 * S * B * (4 + 4))
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
