/*
 * icw_pool_plan.cpp -- the slot plan of icw_transcode_files_pool (icw_pool_plan.h: the rules).  Plain C++,
 * no HIP header: it is also built alone, under ASan + UBSan, by the Makefile's hostcheck-pool.
 */
#include "icw_pool_plan.h"

#include <string.h>

#include <algorithm>

#include "../../include/icw_reader.h"

int icw_pool_make_plan(const int64_t *total, int n, int32_t slots, int32_t B, int32_t order, IcwPoolPlan &plan)
{
    if (n < 0 || (n > 0 && !total) || slots < 0 || B < 1 || (order != ICW_POOL_AS_GIVEN && order != ICW_POOL_LONGEST_FIRST))
        return ICW_EINVAL;
    IcwPoolPlan p;
    p.slot.assign((size_t)n, -1);
    p.start.assign((size_t)n, -1);
    p.n_blocks.assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        if (total[i] <= 0) continue;
        p.queue.push_back(i);
        p.n_blocks[(size_t)i] = (total[i] - 1) / B + 1;
    }
    if (order == ICW_POOL_LONGEST_FIRST)
        std::stable_sort(p.queue.begin(), p.queue.end(), [&](int a, int b) { return total[a] > total[b]; });
    const size_t m = p.queue.size();
    p.slots = (int32_t)(slots == 0 || (size_t)slots >= m ? m : (size_t)slots);
    std::vector<int64_t> free_at((size_t)p.slots, 0);     /* the first block each slot is free in */
    std::vector<char> held((size_t)p.slots, 0);
    int64_t cur = 0;                                      /* starts never go back: files start in queue order */
    for (int i : p.queue) {
        cur = std::max(cur, *std::min_element(free_at.begin(), free_at.end()));
        size_t s = 0;
        while (free_at[s] > cur) ++s;                     /* the lowest-numbered slot free in block cur */
        p.slot[(size_t)i] = (int32_t)s;
        p.start[(size_t)i] = cur;
        free_at[s] = cur + p.n_blocks[(size_t)i];
        p.refills += held[s];
        held[s] = 1;
        p.busy_slot_blocks += (uint64_t)p.n_blocks[(size_t)i];
    }
    for (int64_t f : free_at) p.blocks = std::max(p.blocks, (uint64_t)f);
    p.slot_blocks = (uint64_t)p.slots * p.blocks;
    plan = std::move(p);
    return ICW_OK;
}

extern "C" int icw_pool_plan(const int64_t *total, int n, int32_t slots, int32_t block_frames, int32_t order,
                             int32_t *slot, int64_t *start_block, icw_pool_stats *stats)
{
    if (block_frames < 0) return ICW_EINVAL;
    IcwPoolPlan p;
    const int rc = icw_pool_make_plan(total, n, slots, block_frames > 0 ? block_frames : 65536, order, p);
    if (rc != ICW_OK) return rc;
    for (int i = 0; i < n; ++i) {
        if (slot) slot[i] = p.slot[(size_t)i];
        if (start_block) start_block[i] = p.start[(size_t)i];
    }
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->slots = p.slots;
        stats->refills = p.refills;
        stats->blocks = p.blocks;
        stats->slot_blocks = p.slot_blocks;
        stats->busy_slot_blocks = p.busy_slot_blocks;
    }
    return ICW_OK;
}
