"""Host: the plan with classes of icw_transcode_files_jobs (icw_pool_plan_classes, icw_file_job_classes;
in_cwave_amd/csrc/icw_pool_plan.cpp) through ctypes -- no GPU.  The rules (include/icw_reader.h): every class of
files keeps one contiguous range of slots for the whole run, the ranges follow each other in the order of each
class's first file, a class's share of the width is apportioned by largest remainder in proportion to its busy
slot-blocks, at least 1 and at most its files, and inside its range a class is planned as a pool of its own.
Everything is checked against a block-by-block occupancy recomputed here from slot / start_block / total, which
shares nothing with the planner; the apportionment is pinned on cases worked out by hand."""
import ctypes as C
import random
import re
import subprocess
from pathlib import Path

import pytest

from in_cwave_amd import abi, graph
from in_cwave_amd import lib as L

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "in_cwave_amd" / "csrc"
B = 256


def nblocks(total, b=B):
    return -(-total // b)


def plan(totals, cls, slots, order=abi.POOL_AS_GIVEN, b=B):
    rc, slot, start, st = L.pool_plan_classes(totals, cls, slots, b, order)
    assert rc == abi.OK
    return slot, start, st


def first_appearance(totals, cls):
    """the classes of the files that take a slot, in the order of their first file"""
    order = []
    for t, c in zip(totals, cls):
        if t > 0 and c not in order:
            order.append(c)
    return order


def occupancy(totals, slot, start, b=B):
    """block by block: occ[k][s] = the file whose frames slot s holds in block k (None: idle); a slot that two
    files claim in one block fails here"""
    takers = [i for i, t in enumerate(totals) if t > 0]
    blocks = max((start[i] + nblocks(totals[i], b) for i in takers), default=0)
    width = max((slot[i] for i in takers), default=-1) + 1
    occ = [[None] * width for _ in range(blocks)]
    for i in takers:
        assert slot[i] >= 0 and start[i] >= 0, i
        for k in range(start[i], start[i] + nblocks(totals[i], b)):
            assert occ[k][slot[i]] is None, f"slot {slot[i]} holds files {occ[k][slot[i]]} and {i} in block {k}"
            occ[k][slot[i]] = i
    return occ


def check_plan(totals, cls, slots, order, b=B):
    """every invariant of the header on one library; returns (ranges by class, stats)"""
    slot, start, st = plan(totals, cls, slots, order, b)
    takers = [i for i, t in enumerate(totals) if t > 0]
    classes = first_appearance(totals, cls)
    K, m = len(classes), len(takers)
    for i, t in enumerate(totals):
        if t <= 0:
            assert (slot[i], start[i]) == (-1, -1)
    # the width: min(slots, files), all files for 0, raised to K
    W = max(m if slots == 0 or slots >= m else slots, K)
    assert st.pool.slots == W and st.classes == K
    occ = occupancy(totals, slot, start, b)                 # no slot holds two files at once
    # at every block the slots that hold, or last held, files of one class are exactly that class's range: so the
    # slots a class ever uses are one interval, the intervals are disjoint, follow each other from slot 0 in
    # first-appearance order and add up to the width
    used = {c: sorted({slot[i] for i in takers if cls[i] == c}) for c in classes}
    at, ranges = 0, {}
    for c in classes:
        files = [i for i in takers if cls[i] == c]
        share = len(used[c])
        assert used[c] == list(range(at, at + share)), (c, used[c], at)
        assert 1 <= share <= len(files)
        ranges[c] = (at, share)
        at += share
    assert at == W
    last = {}
    for k, row in enumerate(occ):
        for s, i in enumerate(row):
            if i is not None:
                last[s] = cls[i]
        for s, c in last.items():
            assert ranges[c][0] <= s < ranges[c][0] + ranges[c][1], (k, s, c)
    # within a range: the class's files start in queue order, each in the lowest slot of the range that is free in
    # its block, and no earlier block had a free slot for it
    for c in classes:
        lo, share = ranges[c]
        q = [i for i in takers if cls[i] == c]
        if order == abi.POOL_LONGEST_FIRST:
            q = sorted(q, key=lambda i: -totals[i])                          # sorted() is stable
        assert [start[i] for i in q] == sorted(start[i] for i in q), c
        end = {}
        for n, i in enumerate(q):
            free = [s for s in range(lo, lo + share) if end.get(s, 0) <= start[i]]
            assert slot[i] == min(free), (c, i)
            if n and start[i] > start[q[n - 1]]:
                assert all(end.get(s, 0) >= start[i] for s in range(lo, lo + share)) and min(end.values()) == start[i]
            elif n == 0:
                assert start[i] == 0
            end[slot[i]] = start[i] + nblocks(totals[i], b)
    # the statistics, from the occupancy
    busy = sum(1 for row in occ for i in row if i is not None)
    assert st.pool.blocks == len(occ) and st.pool.busy_slot_blocks == busy == sum(nblocks(totals[i], b) for i in takers)
    assert st.pool.slot_blocks == W * len(occ) and st.pool.refills == m - W
    assert st.kernel_s == 0.0 and st.pool.batch.n_files == 0
    return ranges, st


def random_library(rng, max_classes=5):
    K = rng.randint(1, max_classes)
    n = K + rng.randint(0, 40)
    totals = [rng.choice([rng.randint(1, 8 * B), rng.randint(1, 4) * B, rng.randint(1, 4) * B + rng.choice([-1, 1]), 0])
              for _ in range(n)]
    names = rng.sample(range(100), K)
    cls = [names[rng.randrange(K)] for _ in range(n)]
    return totals, cls


def test_invariants_on_random_libraries():
    rng = random.Random(20261021)
    seen_raise = seen_refill = 0
    for case in range(300):
        totals, cls = random_library(rng)
        slots, order = rng.randint(0, 12), rng.randint(0, 1)
        ranges, st = check_plan(totals, cls, slots, order)
        seen_raise += 0 < slots < len(ranges)
        seen_refill += st.pool.refills > 0
    assert seen_raise >= 10 and seen_refill >= 100          # the width raised to K, and refills, were exercised


def test_one_class_is_the_pool_plan():
    rng = random.Random(11)
    for case in range(100):
        totals, _ = random_library(rng, 1)
        slots, order = rng.randint(0, 9), rng.randint(0, 1)
        slot, start, st = plan(totals, [7] * len(totals), slots, order)
        rc, slot_p, start_p, st_p = L.pool_plan(totals, slots, B, order)
        assert rc == abi.OK and slot == slot_p and start == start_p
        assert bytes(st.pool) == bytes(st_p), case                          # field for field
        assert st.classes == (1 if any(t > 0 for t in totals) else 0)


def shares(totals, cls, slots):
    ranges, _ = check_plan(totals, cls, slots, abi.POOL_AS_GIVEN)
    return [ranges[c][1] for c in first_appearance(totals, cls)]


def files(blocks, c):
    """a class of files by their lengths in blocks"""
    return [(n * B, c) for n in blocks]


def test_apportionment_by_hand():
    def lib(*groups):
        fl = [f for g in groups for f in g]
        return [t for t, _ in fl], [c for _, c in fl]
    # loads 6 : 3 : 1 on 5 slots: quotas 3, 1.5, 0.5 -- the third class gets its one slot, the 4 left go over 6 : 3,
    # 2.67 and 1.33: whole parts 2 and 1, the leftover slot to the larger remainder (6/9 over 3/9)
    assert shares(*lib(files([1] * 6, 0), files([1] * 3, 1), files([1], 2)), 5) == [3, 1, 1]
    # equal loads on 4 slots: three remainders of 1/3, the tie goes to the class laid out first
    assert shares(*lib(files([2, 2], 30), files([2, 2], 20), files([1, 3], 10)), 4) == [2, 1, 1]
    # loads 100 : 10 : 10 on 6 slots, the first class ONE file of 100 blocks: quotas 5, 0.5, 0.5 give 4, 1, 1; the first
    # class is capped at its one file, and the 5 slots left go over 10 : 10 -- 2.5 each, the leftover to the lower class
    assert shares(*lib(files([100], 0), files([2] * 5, 1), files([2] * 5, 2)), 6) == [1, 3, 2]
    # loads 5 : 100, the second class ONE file: it is capped at 1 and the class that had its minimum takes the rest
    assert shares(*lib(files([1] * 5, 0), files([100], 1)), 6) == [5, 1]
    # as wide as classes, whatever the loads; and narrower: raised
    assert shares(*lib(files([500, 500], 0), files([1], 1), files([1], 2)), 3) == [1, 1, 1]
    assert shares(*lib(files([500, 500], 0), files([1], 1), files([1], 2)), 1) == [1, 1, 1]
    # proportional to busy slot-blocks, not to files: 2 files of 8 blocks against 8 files of 1 on 6 slots -- 16 : 8
    # gives 4 and 2, the first class is capped at its 2 files and the other takes 4
    assert shares(*lib(files([8, 8], 0), files([1] * 8, 1)), 6) == [2, 4]
    # 32 : 8 on 6 slots: 4.8 and 1.2 -- whole parts 4 and 1, the leftover slot to 0.8; 5 exceeds the 4 files of the first
    # class, which keeps 4, and the second gets 2
    assert shares(*lib(files([8, 8, 8, 8], 0), files([1] * 8, 1)), 6) == [4, 2]
    # interleaved in the arrays: the same shares, the ranges in first-appearance order
    t, c = lib(files([1] * 6, 0), files([1] * 3, 1), files([1], 2))
    perm = [9, 0, 6, 1, 2, 7, 3, 4, 8, 5]
    ranges, _ = check_plan([t[i] for i in perm], [c[i] for i in perm], 5, abi.POOL_AS_GIVEN)
    assert ranges == {2: (0, 1), 0: (1, 3), 1: (4, 1)}


def test_a_range_is_not_handed_on():
    """class 0's one short file ends after block 0; class 1's queue waits for its own single slot -- the deliberate
    limit, and its cost shows in busy / all slot-blocks"""
    totals, cls = [B, 3 * B, 3 * B, 3 * B], [0, 1, 1, 1]
    slot, start, st = plan(totals, cls, 2)
    assert slot == [0, 1, 1, 1] and start == [0, 0, 3, 6]
    assert (st.pool.blocks, st.pool.slot_blocks, st.pool.busy_slot_blocks) == (9, 18, 10)


def make_job(hilbert, render):
    """hilbert: (type, kahan, reject); render: (render_type, nshape_type, need24bits)"""
    cfg = graph.default_config(48000, need24bits=bool(render[2]), hilbert_type=hilbert[0])
    cfg.iir_kahan, cfg.iir_subnorm_reject = hilbert[1], hilbert[2]
    cfg.render.render_type, cfg.render.nshape_type = render[0], render[1]
    return L.file_job(cfg, [graph.master()])


HILBERTS = [(1, 1, 1), (0, 0, 0), (4, 1, 1), (1, 0, 1), (5, 1, 0)]
RENDERS = [(abi.RENDER_ROUND, abi.NSHAPE_FLAT, 0), (abi.RENDER_TPDF, abi.NSHAPE_MEW44, 1), (abi.RENDER_TPDF, abi.NSHAPE_FLAT, 0),
           (abi.RENDER_ROUND, abi.NSHAPE_FLAT, 1)]


def test_job_classes_keep_hilbert_settings_adjacent():
    """the classes of random jobs, as the transcoder makes them, then the plan of the files ordered by class: equal
    keys are one class, the layout is by the Hilbert setting's first appearance and then the render's, so the
    ranges of Hilbert-equal classes are neighbours and a call has as many Hilbert runs as Hilbert settings"""
    rng = random.Random(5)
    for case in range(60):
        n = rng.randint(1, 30)
        nh, nr = rng.randint(1, len(HILBERTS)), rng.randint(1, len(RENDERS))
        keys = [(rng.randrange(nh), rng.randrange(nr)) for _ in range(n)]
        jobs = [make_job(HILBERTS[h], RENDERS[r]) for h, r in keys]
        K, cls = L.file_job_classes(jobs)
        assert K == len(set(keys)) and sorted(set(cls)) == list(range(K))
        h_order = list(dict.fromkeys(h for h, _ in keys))
        r_order = list(dict.fromkeys(r for _, r in keys))
        layout = sorted(set(keys), key=lambda k: (h_order.index(k[0]), r_order.index(k[1])))
        assert cls == [layout.index(k) for k in keys], case
        # CWAVE input: the render and the depth alone
        Kc, cls_c = L.file_job_classes(jobs, cwave=True)
        assert Kc == len(r_order) and cls_c == [r_order.index(r) for _, r in keys]
        # the plan the transcoder executes: the files ordered by class (stable), so first appearance is the layout
        totals = [rng.randint(1, 6 * B) for _ in range(n)]
        by_class = sorted(range(n), key=lambda i: cls[i])
        ranges, st = check_plan([totals[i] for i in by_class], [cls[i] for i in by_class], rng.randint(1, 10), rng.randint(0, 1))
        assert [ranges[c][0] for c in range(K)] == sorted(ranges[c][0] for c in range(K))
        h_of_slot = []
        for c in range(K):
            h_of_slot += [layout[c][0]] * ranges[c][1]
        runs = 1 + sum(a != b for a, b in zip(h_of_slot, h_of_slot[1:]))
        assert runs == len(h_order), (case, h_of_slot)


def test_job_fields():
    cfg = graph.default_config(48000)
    job = L.file_job(cfg, [graph.master(), graph.shift(out="A", fr=2.0)])
    assert (job.n_nodes, job.bypass_list, job.need24bits, job.hilbert_type, job.iir_kahan, job.iir_subnorm_reject) == (2, 0, 0, 1, 1, 1)
    assert bytes(job.render) == bytes(cfg.render) and job.nodes[1].mode == abi.MODE_SHIFT
    cfg.need24bits, cfg.bypass_list, cfg.hilbert_type, cfg.iir_kahan = 1, 1, 4, 0
    job = L.file_job(cfg, [])
    assert (job.n_nodes, job.bypass_list, job.need24bits, job.hilbert_type, job.iir_kahan) == (0, 1, 1, 4, 0)
    bad_h, bad_r = make_job((6, 1, 1), RENDERS[0]), make_job(HILBERTS[0], (5, 0, 0))
    assert L.file_job_classes([make_job(HILBERTS[0], RENDERS[0]), bad_h, bad_r]) == (1, [0, -1, -1])


def test_bad_options():
    for slots, b, order in ((-1, B, 0), (2, -1, 0), (2, B, 2), (2, B, -1)):
        rc, *_ = L.pool_plan_classes([5, 6], [0, 1], slots, b, order)
        assert rc == abi.EINVAL
    assert L.pool_plan_classes([5, 6], [0, -1], 2, B)[0] == abi.EINVAL
    assert L.pool_plan_classes([5, 0], [0, -1], 2, B)[0] == abi.OK        # the class of a file without frames counts for nothing
    rc, _, _, st = L.pool_plan_classes([65536, 65537], [3, 3], 1, 0)      # block_frames 0: 65536
    assert rc == abi.OK and st.pool.blocks == 3
    lib = L.load()
    assert lib.icw_pool_plan_classes(None, None, 0, 3, B, 0, None, None, None) == abi.OK
    # the transcoder refuses bad options before it opens a file
    cfg = abi.Config()
    for slots, order in ((-1, 0), (2, 7)):
        o = abi.PoolOpts(abi.BatchOpts(0, 0, 0, B, -1, 0), slots, order)
        assert lib.icw_transcode_files_jobs(C.byref(cfg), None, None, None, 0, C.byref(o), None, None, None) == abi.EINVAL
    cfg.fp_check = 1
    assert lib.icw_transcode_files_jobs(C.byref(cfg), None, None, None, 0, None, None, None, None) == abi.EUNSUPPORTED


def test_host_check_under_sanitizers(tmp_path):
    """tests/native/pool_plan_classes_host_check.cpp, a program of its own over icw_pool_plan.cpp: ASan + UBSan"""
    exe = tmp_path / "pool_plan_classes_host_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), str(ROOT / "tests" / "native" / "pool_plan_classes_host_check.cpp"), str(CSRC / "icw_pool_plan.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "pool_plan_classes_host_check: ok", r.stdout + r.stderr


def test_host_check_detects_a_wrong_remainder_rule(tmp_path):
    """negative control: with the leftover slots handed to the SMALLEST remainders, the hand-computed cases fail"""
    text = (CSRC / "icw_pool_plan.cpp").read_text()
    old = "return rem[a] > rem[b];"
    assert text.count(old) == 1
    (tmp_path / "icw_pool_plan.cpp").write_text(text.replace(old, "return rem[a] < rem[b];")
                                                .replace('"icw_pool_plan.h"', f'"{CSRC}/icw_pool_plan.h"')
                                                .replace('"../../include/icw_reader.h"', f'"{ROOT}/include/icw_reader.h"'))
    exe = tmp_path / "neg"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), str(ROOT / "tests" / "native" / "pool_plan_classes_host_check.cpp"),
                    str(tmp_path / "icw_pool_plan.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 1 and "FAIL" in r.stderr, r.stdout + r.stderr


def test_abi_mirror(tmp_path):
    hdr = (ROOT / "include" / "icw_reader.h").read_text()
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "in_cwave_amd" / "libicw.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    for name in ("icw_transcode_files_jobs", "icw_pool_plan_classes", "icw_file_job_classes", "icw_file_job_from_config"):
        assert name in exported and name in abi.SIGNATURES and re.search(r"^(int|void) +%s\(" % name, hdr, flags=re.M), name
    assert not [s for s in exported if "make_plan" in s or "apportion" in s or "pool_job" in s]   # the C++ side stays internal
    # layouts: a pointer, two int32, icw_render_cfg (8 + 5 * 4 = 28, padded to 32), four int32; icw_pool_stats (72),
    # three int32 (+ 4 of padding), a double
    assert C.sizeof(abi.RenderCfg) == 32 and C.sizeof(abi.FileJob) == 64
    assert (abi.FileJob.render.offset, abi.FileJob.need24bits.offset, abi.FileJob.iir_subnorm_reject.offset) == (16, 48, 60)
    assert C.sizeof(abi.JobsStats) == 96 and abi.JobsStats.classes.offset == 72 and abi.JobsStats.kernel_s.offset == 88
    assert abi.BATCH_TIMING == 8 and "#define ICW_BATCH_TIMING 8" in hdr
    assert abi.BATCH_TIMING & (abi.BATCH_MERGE_INPUTS | abi.BATCH_MERGE_CWAVE | abi.BATCH_MERGE_BUS) == 0
    assert L.load().icw_abi_version() == 2                              # additions only
    # the same layouts as a C compiler sees them
    (tmp_path / "v.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icw_reader.h"\n'
                                  'int main(void) { printf("%zu %zu %zu %zu %zu %d\\n", sizeof(icw_file_job), '
                                  'offsetof(icw_file_job, iir_subnorm_reject), sizeof(icw_jobs_stats), '
                                  'offsetof(icw_jobs_stats, classes), offsetof(icw_jobs_stats, kernel_s), ICW_BATCH_TIMING); '
                                  'return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), "-o", str(tmp_path / "v"), str(tmp_path / "v.c")], check=True)
    out = subprocess.run([str(tmp_path / "v")], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["64", "60", "96", "72", "88", "8"]
