"""Host: the slot plan of icw_transcode_files_pool (icw_pool_plan, in_cwave_amd/csrc/icw_pool_plan.cpp) through
ctypes -- no GPU.  The rules (include/icw_reader.h): a file starts at a block boundary in the lowest-numbered free
slot, files start in queue order (as given, or longest first, stable), and a slot is free from the block after the
one that holds its file's last frame.  The statistics are checked against a block-by-block simulation written
here, which shares nothing with the planner."""
import ctypes as C
import random
import re
import subprocess
from pathlib import Path

import pytest

from in_cwave_amd import abi
from in_cwave_amd import lib as L

ROOT = Path(__file__).resolve().parents[1]
B = 256
EDGES = [1 * B, B - 1, B + 1, 2, 5 * B + 3, B, 3 * B]


def nblocks(total, b=B):
    return -(-total // b)


def queue_of(totals, order):
    q = [i for i, t in enumerate(totals) if t > 0]
    return sorted(q, key=lambda i: -totals[i]) if order == abi.POOL_LONGEST_FIRST else q     # sorted() is stable


def simulate(totals, slots, order, b=B, early=0):
    """block by block: owners leave after their last block, then the queue's head files take the lowest free
    slots.  early = 1 plants the bug of a slot freed one block early.  Returns per-file (slot, start), blocks,
    busy slot-blocks, refills, width."""
    q = queue_of(totals, order)
    S = len(q) if slots == 0 or slots >= len(q) else slots
    left, held, where = [0] * S, [False] * S, {}
    k = busy = refills = 0
    while q or any(v > 0 for v in left):
        for s in range(S):
            if q and left[s] <= early and (left[s] <= 0 or held[s]):
                i = q.pop(0)
                where[i] = (s, k)
                left[s] = nblocks(totals[i], b)
                refills += held[s]
                held[s] = True
        for s in range(S):
            if left[s] > 0:
                left[s] -= 1
                busy += 1
        k += 1
    return where, k, busy, refills, S


def intervals(totals, slot, start, b=B):
    """every file's [start, end) by slot"""
    per = {}
    for i, t in enumerate(totals):
        if t > 0:
            per.setdefault(slot[i], []).append((start[i], start[i] + nblocks(t, b), i))
    return per


def overlaps(per):
    bad = []
    for s, iv in per.items():
        iv = sorted(iv)
        bad += [(s, a[2], c[2]) for a, c in zip(iv, iv[1:]) if c[0] < a[1]]
    return bad


def plan(totals, slots, order=abi.POOL_AS_GIVEN, b=B):
    rc, slot, start, st = L.pool_plan(totals, slots, b, order)
    assert rc == abi.OK
    return slot, start, st


@pytest.mark.parametrize("order", [abi.POOL_AS_GIVEN, abi.POOL_LONGEST_FIRST])
def test_edges_on_three_slots(order):
    slot, start, st = plan(EDGES, 3, order)
    assert st.slots == 3 and st.refills == 4
    # exactly one interval per file, inside the pool
    assert all(0 <= s < 3 for s in slot) and all(k >= 0 for k in start)
    per = intervals(EDGES, slot, start)
    assert sorted(i for iv in per.values() for _, _, i in iv) == list(range(len(EDGES)))
    assert not overlaps(per)
    # starts in queue order, each in the lowest slot free in its block
    q = queue_of(EDGES, order)
    assert [start[i] for i in q] == sorted(start[i] for i in q)
    for n, i in enumerate(q):
        end = {}
        for j in q[:n]:
            end[slot[j]] = start[j] + nblocks(EDGES[j])
        free = [s for s in range(3) if end.get(s, 0) <= start[i]]
        assert slot[i] == min(free), (i, slot, start)
        # ... and no earlier block had a free slot for it: the file before it started no earlier, or every slot was held
        if n and start[i] > start[q[n - 1]]:
            assert all(end.get(s, 0) >= start[i] for s in range(3)) and min(end.values()) == start[i]
    where, blocks, busy, refills, S = simulate(EDGES, 3, order)
    assert {i: (slot[i], start[i]) for i in q} == where
    assert (st.blocks, st.slot_blocks, st.busy_slot_blocks) == (blocks, 3 * blocks, busy)


def test_file_ending_on_a_boundary_frees_its_slot_for_the_next_block():
    # one slot: a file of exactly B frames holds block 0 alone; B + 1 frames spill into a second block
    slot, start, st = plan([B, 5, B + 1, 5], 1)
    assert start == [0, 1, 2, 4] and st.blocks == 5
    # on 3 slots as given: file 0 (B frames) ends with block 0, and file 3 takes its slot 0 in block 1
    slot, start, _ = plan(EDGES, 3)
    assert (slot[0], start[0]) == (0, 0) and (slot[3], start[3]) == (0, 1)
    assert (slot[1], start[1]) == (1, 0) and (slot[4], start[4]) == (1, 1)          # B - 1 frames: one block too
    assert (slot[2], start[2]) == (2, 0) and (slot[5], start[5]) == (0, 2)          # B + 1 frames: two blocks


def test_statistics_against_simulation():
    rng = random.Random(20261021)
    for case in range(200):
        n, slots, order = rng.randint(1, 40), rng.randint(1, 9), rng.randint(0, 1)
        totals = [rng.choice([rng.randint(1, 8 * B), rng.randint(1, 4) * B, rng.randint(1, 4) * B + rng.choice([-1, 1])])
                  for _ in range(n)]
        slot, start, st = plan(totals, slots, order)
        where, blocks, busy, refills, S = simulate(totals, slots, order)
        assert (st.slots, st.blocks, st.slot_blocks, st.busy_slot_blocks, st.refills) == (S, blocks, S * blocks, busy, refills), case
        assert {i: (slot[i], start[i]) for i in range(n)} == where, case
        assert not overlaps(intervals(totals, slot, start)), case
        assert busy == sum(nblocks(t) for t in totals)


def test_identities():
    rng = random.Random(7)
    for case in range(100):
        n = rng.randint(1, 40)
        totals = [rng.randint(1, 8 * B) for _ in range(n)]
        for slots in (0, n, n + 5):
            slot, start, st = plan(totals, slots, rng.randint(0, 1))
            assert sorted(slot) == list(range(n)) and start == [0] * n and st.refills == 0 and st.slots == n
            assert st.blocks == max(nblocks(t) for t in totals)
        for order in (abi.POOL_AS_GIVEN, abi.POOL_LONGEST_FIRST):
            _, _, st = plan(totals, 1, order)
            assert st.blocks == sum(nblocks(t) for t in totals) == st.busy_slot_blocks == st.slot_blocks
            assert st.refills == n - 1
        slots = rng.randint(1, 9)
        asc = sorted(totals)
        _, _, st_long = plan(asc, slots, abi.POOL_LONGEST_FIRST)
        _, _, st_asc = plan(asc, slots, abi.POOL_AS_GIVEN)
        assert st_long.blocks <= st_asc.blocks, (case, totals, slots)


def test_longest_first_is_stable_and_files_without_frames_take_no_slot():
    totals = [300, 0, 700, 300, 700, -1]
    slot, start, st = plan(totals, 1, abi.POOL_LONGEST_FIRST)
    assert [start[i] for i in (2, 4, 0, 3)] == [0, 3, 6, 8]              # 700, 700, 300, 300 in their given order
    assert (slot[1], start[1], slot[5], start[5]) == (-1, -1, -1, -1) and st.slots == 1 and st.refills == 3


def test_negative_control_early_free_is_caught():
    """a planner that frees a slot one block early, planted in the simulation: the overlap check sees it"""
    where, *_ = simulate(EDGES, 3, abi.POOL_AS_GIVEN, early=1)
    slot = [where[i][0] for i in range(len(EDGES))]
    start = [where[i][1] for i in range(len(EDGES))]
    assert overlaps(intervals(EDGES, slot, start))
    good, *_ = simulate(EDGES, 3, abi.POOL_AS_GIVEN)
    assert not overlaps(intervals(EDGES, [good[i][0] for i in range(7)], [good[i][1] for i in range(7)]))


def test_bad_options():
    for slots, b, order in ((-1, B, 0), (2, -1, 0), (2, B, 2), (2, B, -1)):
        rc, *_ = L.pool_plan([5, 6], slots, b, order)
        assert rc == abi.EINVAL
    rc, _, _, st = L.pool_plan([65536, 65537], 1, 0)                    # block_frames 0: 65536
    assert rc == abi.OK and st.blocks == 3
    lib = L.load()
    assert lib.icw_pool_plan(None, 0, 3, B, 0, None, None, None) == abi.OK
    # the transcoder refuses them before it opens a file
    o = abi.PoolOpts(abi.BatchOpts(0, 0, 0, B, -1, 0), -1, 0)
    cfg = abi.Config()
    assert lib.icw_transcode_files_pool(C.byref(cfg), None, None, None, None, None, 0, C.byref(o), None, None, None) == abi.EINVAL
    o = abi.PoolOpts(abi.BatchOpts(0, 0, 0, B, -1, 0), 2, 7)
    assert lib.icw_transcode_files_pool(C.byref(cfg), None, None, None, None, None, 0, C.byref(o), None, None, None) == abi.EINVAL


def test_abi_mirror():
    hdr = (ROOT / "include" / "icw_reader.h").read_text()
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "in_cwave_amd" / "libicw.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    for name in ("icw_transcode_files_pool", "icw_pool_plan"):
        assert name in exported and name in abi.SIGNATURES and re.search(r"^int %s\(" % name, hdr, flags=re.M)
    assert not [s for s in exported if "make_plan" in s]               # the C++ planner stays internal
    # layouts: icw_batch_opts (24 bytes) + two int32; icw_batch_stats (40) + two int32 + three uint64
    assert C.sizeof(abi.BatchOpts) == 24 and C.sizeof(abi.BatchStats) == 40
    assert C.sizeof(abi.PoolOpts) == 32 and abi.PoolOpts.slots.offset == 24 and abi.PoolOpts.order.offset == 28
    assert C.sizeof(abi.PoolStats) == 72 and abi.PoolStats.slots.offset == 40 and abi.PoolStats.blocks.offset == 48
    assert abi.PoolStats.busy_slot_blocks.offset == 64
    assert (abi.POOL_AS_GIVEN, abi.POOL_LONGEST_FIRST) == (0, 1)
    assert "#define ICW_POOL_AS_GIVEN      0" in hdr and "#define ICW_POOL_LONGEST_FIRST 1" in hdr
    assert L.load().icw_abi_version() == 2                              # additions only
