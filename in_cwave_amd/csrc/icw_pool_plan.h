/*
 * icw_pool_plan.h -- internal: the slot plan of icw_transcode_files_pool (include/icw_reader.h).  Host
 * arithmetic only, no HIP: which slot each file of a pool runs in and the block in which it starts.  The
 * transcoder executes the plan rather than deciding on the fly, so its statistics are the plan's and the
 * plan can be checked on a CPU (tests/native/pool_plan_host_check.cpp, tests/test_pool_plan.py).
 *
 * The rules: a file starts at a block boundary, in the lowest-numbered free slot; files start in queue
 * order (as given, or by `total` descending, stable); a slot is free from the block after the one that
 * holds its file's last frame.
 */
#ifndef ICW_POOL_PLAN_H
#define ICW_POOL_PLAN_H

#include <stdint.h>

#include <vector>

/* internal: not a dynamic symbol of the library (its C entry is icw_pool_plan, include/icw_reader.h) */
#pragma GCC visibility push(hidden)

struct IcwPoolPlan {
    std::vector<int32_t> slot;        /* per file: its slot, -1 for a file that takes none (total <= 0) */
    std::vector<int64_t> start;       /* per file: the block in which it starts (-1 likewise) */
    std::vector<int64_t> n_blocks;    /* per file: ceil(total / B), the blocks it holds its slot for */
    std::vector<int32_t> queue;       /* the files that take a slot, in the order they start */
    int32_t slots = 0;                /* the pool's width: min(slots asked for, files), all files for 0 */
    int32_t refills = 0;              /* files that start in a slot that had held another */
    uint64_t blocks = 0;              /* blocks until the last file has ended */
    uint64_t slot_blocks = 0;         /* slots * blocks */
    uint64_t busy_slot_blocks = 0;    /* sum of n_blocks */
};

/* total[i]: file i's frames (tail included); slots >= 0 (0: one per file), B >= 1, order ICW_POOL_AS_GIVEN or
 * ICW_POOL_LONGEST_FIRST.  Returns ICW_OK or ICW_EINVAL (nothing written). */
int icw_pool_make_plan(const int64_t *total, int n, int32_t slots, int32_t B, int32_t order, IcwPoolPlan &plan);

#pragma GCC visibility pop

#endif
