/*
 * pool_plan_host_check.cpp -- the slot plan of icw_transcode_files_pool (icw_pool_make_plan / icw_pool_plan,
 * icw_pool_plan.cpp) as a stand-alone program: built with AddressSanitizer + UBSan and run on a CPU
 * (`make -C in_cwave_amd/csrc hostcheck-pool`).  No device, no HIP call.
 *
 * For every case: each file that takes a slot gets one interval [start, start + ceil(total / B)) in a slot
 * below the pool's width; no two files overlap in a slot; files start in queue order, each in the
 * lowest-numbered slot free in its block and no later than a free slot allows; and blocks, slot_blocks,
 * busy_slot_blocks and refills equal a block-by-block simulation that shares no code with the planner.
 */
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../in_cwave_amd/csrc/icw_pool_plan.h"
#include "../../include/icw_reader.h"

static int failures = 0;

#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            fprintf(stderr, "FAIL %s: ", what);               \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, " (%s:%d)\n", __FILE__, __LINE__); \
            ++failures;                                       \
        }                                                     \
    } while (0)

static void check_case(const char *what, const std::vector<int64_t> &total, int slots, int B, int order)
{
    const int n = (int)total.size();
    IcwPoolPlan p;
    const int rc = icw_pool_make_plan(total.data(), n, slots, B, order, p);
    CHECK(rc == ICW_OK, "rc = %d", rc);
    if (rc != ICW_OK) return;
    /* the queue, made here: the files with frames, as given or by length descending (stable) */
    std::vector<int> queue;
    for (int i = 0; i < n; ++i)
        if (total[(size_t)i] > 0) queue.push_back(i);
    if (order == ICW_POOL_LONGEST_FIRST)
        std::stable_sort(queue.begin(), queue.end(), [&](int a, int b) { return total[(size_t)a] > total[(size_t)b]; });
    const int m = (int)queue.size(), S = slots == 0 || slots >= m ? m : slots;
    CHECK(p.slots == S, "%d slots, expected %d", p.slots, S);
    CHECK(p.queue.size() == queue.size() && std::equal(queue.begin(), queue.end(), p.queue.begin()), "queue order");
    if (p.slots != S) return;
    /* block by block: a slot's owner leaves after its last block; then the queue's head files take the
     * lowest-numbered free slots */
    std::vector<int64_t> left((size_t)S, 0);
    std::vector<char> held((size_t)S, 0);
    size_t head = 0;
    uint64_t blocks = 0, busy = 0;
    int refills = 0;
    for (int64_t k = 0; head < queue.size() || std::any_of(left.begin(), left.end(), [](int64_t v) { return v > 0; }); ++k) {
        for (int s = 0; s < S && head < queue.size(); ++s) {
            if (left[(size_t)s] > 0) continue;
            const int i = queue[head++];
            CHECK(p.slot[(size_t)i] == s && p.start[(size_t)i] == k, "file %d: slot %d block %lld, expected slot %d block %lld",
                  i, p.slot[(size_t)i], (long long)p.start[(size_t)i], s, (long long)k);
            left[(size_t)s] = (total[(size_t)i] + B - 1) / B;
            refills += held[(size_t)s];
            held[(size_t)s] = 1;
        }
        for (int s = 0; s < S; ++s)
            if (left[(size_t)s] > 0) {
                --left[(size_t)s];
                ++busy;
            }
        blocks = (uint64_t)k + 1;
    }
    CHECK(p.blocks == blocks, "%llu blocks, expected %llu", (unsigned long long)p.blocks, (unsigned long long)blocks);
    CHECK(p.slot_blocks == (uint64_t)S * blocks, "slot_blocks %llu", (unsigned long long)p.slot_blocks);
    CHECK(p.busy_slot_blocks == busy, "busy %llu, expected %llu", (unsigned long long)p.busy_slot_blocks, (unsigned long long)busy);
    CHECK(p.refills == refills && refills == m - S, "refills %d, expected %d", p.refills, refills);
    for (int i = 0; i < n; ++i)
        if (total[(size_t)i] <= 0) CHECK(p.slot[(size_t)i] == -1 && p.start[(size_t)i] == -1, "file %d has no frames but a slot", i);
    /* the C entry gives the same plan */
    std::vector<int32_t> slot((size_t)n + 1, -7);
    std::vector<int64_t> start((size_t)n + 1, -7);
    icw_pool_stats st;
    CHECK(icw_pool_plan(total.data(), n, slots, B, order, slot.data(), start.data(), &st) == ICW_OK, "icw_pool_plan");
    for (int i = 0; i < n; ++i)
        CHECK(slot[(size_t)i] == p.slot[(size_t)i] && start[(size_t)i] == p.start[(size_t)i], "icw_pool_plan: file %d", i);
    CHECK(slot[(size_t)n] == -7 && start[(size_t)n] == -7, "icw_pool_plan wrote past n entries");
    CHECK(st.slots == p.slots && st.refills == p.refills && st.blocks == p.blocks && st.slot_blocks == p.slot_blocks &&
              st.busy_slot_blocks == p.busy_slot_blocks && st.batch.n_files == 0,
          "icw_pool_plan: stats");
}

int main()
{
    const char *what = "options";
    const int B = 256;
    const std::vector<int64_t> edge = {1 * B, B - 1, B + 1, 2, 5 * B + 3, B, 3 * B};
    for (int order = 0; order < 2; ++order) {
        check_case("edges on 3 slots", edge, 3, B, order);
        check_case("edges on 1 slot", edge, 1, B, order);
        check_case("edges, one slot per file", edge, 0, B, order);
        check_case("edges, more slots than files", edge, 50, B, order);
        check_case("no files", {}, 4, B, order);
        check_case("files without frames", {0, 700, -3, 256, 0}, 1, B, order);
        check_case("one-frame blocks", {3, 1, 4, 1, 5, 9, 2, 6}, 3, 1, order);
        check_case("long files", {(int64_t)1 << 40, ((int64_t)1 << 40) + 1, 5}, 2, 65536, order);
    }
    uint64_t x = 88172645463325252ull;                       /* xorshift64 */
    auto rnd = [&](uint64_t m) {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x % m;
    };
    for (int c = 0; c < 500; ++c) {
        std::vector<int64_t> t((size_t)(1 + rnd(40)));
        for (int64_t &v : t) v = (int64_t)rnd(8 * B) + (rnd(9) ? 1 : 0);
        check_case("random", t, (int)rnd(10), B, (int)rnd(2));
    }
    /* refusals: nothing is written */
    IcwPoolPlan keep;
    keep.slots = 77;
    const int64_t one = 5;
    CHECK(icw_pool_make_plan(&one, 1, -1, B, 0, keep) == ICW_EINVAL && keep.slots == 77, "slots < 0");
    CHECK(icw_pool_make_plan(&one, 1, 1, B, 2, keep) == ICW_EINVAL && keep.slots == 77, "unknown order");
    CHECK(icw_pool_make_plan(&one, 1, 1, 0, 0, keep) == ICW_EINVAL && keep.slots == 77, "B < 1");
    CHECK(icw_pool_make_plan(nullptr, 1, 1, B, 0, keep) == ICW_EINVAL, "no totals");
    CHECK(icw_pool_plan(&one, 1, 1, -1, 0, nullptr, nullptr, nullptr) == ICW_EINVAL, "block_frames < 0");
    CHECK(icw_pool_plan(&one, 1, 1, 0, 0, nullptr, nullptr, nullptr) == ICW_OK, "all outputs nullable");
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("pool_plan_host_check: ok\n");
    return 0;
}
