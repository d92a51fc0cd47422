#!/usr/bin/env python3
"""What per-file settings in one slot pool (icw_transcode_files_jobs) buy against one pool call per setting:
`--files` stereo int16 48 kHz WAV files, lengths log-uniform between 2^16 and 2^20 frames (seeded), every file
with its own Shift -> Master list, default block (65 536 frames), four classes in equal shares --
    0  Hilbert type 1, Kahan + reject    16-bit ROUND
    1  Hilbert type 1, Kahan + reject    24-bit TPDF + MEW44
    2  Hilbert type 0, baseline          16-bit TPDF flat
    3  Hilbert type 4, Kahan + reject    24-bit ROUND

    python tools/jobs_rate.py [--files 384] [--runs 3] [--dir /dev/shm/icw_jobs_rate] [--slots 256]
                              [--min-log2 16] [--max-log2 20] [--out FILE]

The library is generated into --dir (a tmpfs directory, so that the disk stays out of the figures) and removed
afterwards.  Legs, `--runs` runs of each in one session, the leg order reversed on every other run:
  a pool_one    every file as class 0 through icw_transcode_files_pool
  b jobs_one    the same through icw_transcode_files_jobs: one class, the same launches
  c jobs_four   the four classes in ONE jobs call, the files of a class adjacent in the arrays
  d pools_four  what a host does without the jobs call: four icw_transcode_files_pool calls, one per class, one
                after the other, each at --slots; timed as one leg (walls and I/O summed)
  e jobs_dealt  leg c with the files' classes dealt round-robin in the arrays: the plan keeps every class in its
                own range of slots, so this must equal c
One JSON line per leg and run: wall_s and io_s (the calls' own statistics), blocks, slot_blocks and
busy_slot_blocks (the plan's; summed over the calls of leg d), slots, classes and the runs a call was cut into,
and for the jobs legs kernel_s -- from a second call with ICW_BATCH_TIMING, which waits for every block's kernels
and is therefore not the call whose wall time is reported."""
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
    ap.add_argument("--files", type=int, default=384)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm/icw_jobs_rate")
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--min-log2", type=float, default=16.0)
    ap.add_argument("--max-log2", type=float, default=20.0)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    from in_cwave_amd import abi, graph, synth
    from in_cwave_amd import lib as L
    import wavgen as W

    soft, hard = resource.getrlimit(resource.RLIMIT_NOFILE)
    want = 2 * a.files + 256
    if soft < want:
        resource.setrlimit(resource.RLIMIT_NOFILE, (min(want, hard) if hard != resource.RLIM_INFINITY else want, hard))

    def class_cfg(hilbert, render_type, nshape, need24):
        cfg = graph.default_config(48000, need24bits=bool(need24), hilbert_type=hilbert[0])
        cfg.iir_kahan, cfg.iir_subnorm_reject = hilbert[1], hilbert[2]
        cfg.render.render_type, cfg.render.nshape_type = render_type, nshape
        return cfg

    cfgs = [class_cfg((1, 1, 1), abi.RENDER_ROUND, abi.NSHAPE_FLAT, 0), class_cfg((1, 1, 1), abi.RENDER_TPDF, abi.NSHAPE_MEW44, 1),
            class_cfg((0, 0, 0), abi.RENDER_TPDF, abi.NSHAPE_FLAT, 0), class_cfg((4, 1, 1), abi.RENDER_ROUND, abi.NSHAPE_FLAT, 1)]
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
    cls = [i * 4 // n for i in range(n)]                     # a class's files adjacent in the arrays
    dealt = sorted(range(n), key=lambda i: (i - cls[i] * n // 4, cls[i]))   # the same files, the classes round-robin
    shape = {"files": n, "max_over_mean": round(max(lengths) / (sum(lengths) / n), 3), "frames": sum(lengths)}
    base_cfg = graph.default_config(fs)

    def jobs_leg(order, classes):
        jobs = [L.file_job(cfgs[classes[i]], lists[i]) for i in order]
        args = (base_cfg, jobs, [ins[i] for i in order], [outs[i] for i in order])
        rc, st, _, _ = L.transcode_files_jobs(*args, slots=a.slots, want_meters=False)
        rc_t, st_t, _, _ = L.transcode_files_jobs(*args, slots=a.slots, want_meters=False, timing=True)
        assert rc == abi.OK == rc_t and st.pool.batch.n_files == n, (rc, rc_t, st.pool.batch.n_files)
        p = st.pool
        return dict(slots=p.slots, wall_s=p.batch.wall_s, io_s=p.batch.io_s, blocks=p.blocks, slot_blocks=p.slot_blocks,
                    busy_slot_blocks=p.busy_slot_blocks, refills=p.refills, contexts=p.batch.n_groups, classes=st.classes,
                    hilbert_runs_max=st.hilbert_runs_max, render_runs_max=st.render_runs_max, kernel_s=round(st_t.kernel_s, 4),
                    timed_wall_s=round(st_t.pool.batch.wall_s, 4))

    def pool_leg(groups):
        tot = dict(slots=0, wall_s=0.0, io_s=0.0, blocks=0, slot_blocks=0, busy_slot_blocks=0, refills=0, contexts=0,
                   classes=len(groups))
        for c, members in groups:
            rc, st, _, _ = L.transcode_files_pool(cfgs[c], [lists[i] for i in members], [ins[i] for i in members],
                                                  [outs[i] for i in members], slots=a.slots, want_meters=False)
            assert rc == abi.OK and st.batch.n_files == len(members), (rc, st.batch.n_files)
            tot["slots"] = max(tot["slots"], st.slots)
            for k, v in (("wall_s", st.batch.wall_s), ("io_s", st.batch.io_s), ("blocks", st.blocks), ("slot_blocks", st.slot_blocks),
                         ("busy_slot_blocks", st.busy_slot_blocks), ("refills", st.refills), ("contexts", st.batch.n_groups)):
                tot[k] += v
        return tot

    everyone = list(range(n))
    legs = [("pool_one", lambda: pool_leg([(0, everyone)])),
            ("jobs_one", lambda: jobs_leg(everyone, [0] * n)),
            ("jobs_four", lambda: jobs_leg(everyone, cls)),
            ("pools_four", lambda: pool_leg([(c, [i for i in everyone if cls[i] == c]) for c in range(4)])),
            ("jobs_dealt", lambda: jobs_leg(dealt, cls))]
    lines = []
    try:
        for run in range(a.runs):
            for name, leg in (legs if run % 2 == 0 else legs[::-1]):
                r = leg()
                r["wall_s"], r["io_s"] = round(r["wall_s"], 4), round(r["io_s"], 4)
                rec = dict(tool="jobs_rate", leg=name, run=run, **shape, **r, busy_ratio=round(r["busy_slot_blocks"] / r["slot_blocks"], 4))
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
