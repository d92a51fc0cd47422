/*
 * icw_pool_plan.h -- internal: the slot plan of icw_transcode_files_pool and, with classes, of
 * icw_transcode_files_jobs (include/icw_reader.h).  Host
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

#include <utility>
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

/* The plan of icw_transcode_files_jobs: the files of a pool carry a class, every class keeps one contiguous
 * range of slots for the whole run, and inside its range a class is planned by the rules above.  The pool's
 * width is min(slots, files), raised to the number of classes; a class's share of it is apportioned by largest
 * remainder, in proportion to its busy slot-blocks (the sum of its files' n_blocks), at least 1 and at most its
 * file count (icw_pool_apportion).  With one class the plan is icw_pool_make_plan's. */
struct IcwClassPlan {
    IcwPoolPlan pool;                 /* slot / start / n_blocks per file, slots over the whole width; queue: the files
                                         that take a slot by start block, equal starts by slot */
    std::vector<int32_t> first;       /* per class: the first slot of its range (ranges follow each other from slot 0) */
    std::vector<int32_t> share;       /* per class: the slots of its range */
};

/* W slots over classes of `load` busy slot-blocks and `files` files each, K <= W <= the sum of files, every load
 * and file count >= 1.  A round gives every class still open its quota R * load / L of the R slots not yet
 * settled (L: the open classes' load): the classes whose quota is below 1 get one slot and the round is repeated
 * over the others with what is left, then whole parts and the leftover slots by largest remainder, ties to the
 * lower class.  A class given more than its files is settled at its file count and leaves; the round starts
 * again over the classes that remain (those that had got one slot included) until no class exceeds its files.
 * Returns false, writing nothing, for arguments outside those limits. */
bool icw_pool_apportion(const std::vector<uint64_t> &load, const std::vector<int32_t> &files, int32_t W,
                        std::vector<int32_t> &share);

/* cls[i]: file i's class as its position in the layout, 0 .. K-1, every position with a file that takes a slot
 * (ignored for a file with total <= 0).  Other arguments and the result as icw_pool_make_plan's. */
int icw_pool_make_plan_classes(const int64_t *total, const int32_t *cls, int n, int K, int32_t slots, int32_t B,
                               int32_t order, IcwClassPlan &plan);

/* The class positions icw_transcode_files_jobs gives the files of one pool context (icw_file_job_classes,
 * include/icw_reader.h, is this function): pos[i] for the jobs with take[i] != 0, -1 for the others.  Two jobs
 * are one class when their (render, depth) are equal and -- real input only -- their (hilbert_type, kahan,
 * reject); classes are ordered by the first appearance of their Hilbert setting, then of their render.
 * settings (nullable): per class, in layout order, the index of its Hilbert setting (0 for CWAVE) and of its
 * render among the distinct ones, each numbered by first appearance.  Returns the number of classes. */
struct icw_file_job;
int icw_pool_job_classes(const icw_file_job *jobs, const char *take, int n, bool cwave, std::vector<int32_t> &pos,
                         std::vector<std::pair<int, int>> *settings);
/* whether a job's render fields and hilbert_type are in range (what the two per-stream setters would take) */
bool icw_pool_job_ok(const icw_file_job &job);

#pragma GCC visibility pop

#endif
