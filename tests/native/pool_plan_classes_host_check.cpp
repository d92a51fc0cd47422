/*
 * pool_plan_classes_host_check.cpp -- the plan with classes of icw_transcode_files_jobs (icw_pool_apportion,
 * icw_pool_make_plan_classes, icw_pool_plan_classes, icw_pool_job_classes / icw_file_job_classes;
 * icw_pool_plan.cpp) as a stand-alone program: built with AddressSanitizer + UBSan and run on a CPU
 * (`make -C in_cwave_amd/csrc hostcheck-pool-classes`).  No device, no HIP call.
 *
 * For every case: the shares add up to the width, each at least 1 and at most the class's files; the ranges
 * follow each other from slot 0 in class order; every file lies in its class's range; inside a range the plan
 * equals a block-by-block simulation of that class alone, which shares no code with the planner; the statistics
 * are the sums of the ranges'; one class gives icw_pool_make_plan's plan field for field.  The apportionment is
 * pinned on cases worked out by hand.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

static void check_shares(const char *what, std::vector<uint64_t> load, std::vector<int32_t> files, int W,
                         std::vector<int32_t> want)
{
    std::vector<int32_t> got;
    CHECK(icw_pool_apportion(load, files, W, got), "refused");
    CHECK(got == want, "shares differ");
    if (got != want)
        for (size_t c = 0; c < got.size(); ++c) fprintf(stderr, "  class %zu: %d, expected %d\n", c, got[c], want[c]);
}

static void check_case(const char *what, const std::vector<int64_t> &total, const std::vector<int32_t> &cls, int K, int slots,
                       int B, int order)
{
    const int n = (int)total.size();
    IcwClassPlan p;
    const int rc = icw_pool_make_plan_classes(total.data(), cls.data(), n, K, slots, B, order, p);
    CHECK(rc == ICW_OK, "rc = %d", rc);
    if (rc != ICW_OK) return;
    int m = 0;
    std::vector<int> files((size_t)K, 0);
    for (int i = 0; i < n; ++i)
        if (total[(size_t)i] > 0) {
            ++m;
            ++files[(size_t)cls[(size_t)i]];
        }
    const int W = std::max(slots == 0 || slots >= m ? m : slots, K);
    CHECK(p.pool.slots == W, "%d slots, expected %d", p.pool.slots, W);
    CHECK((int)p.share.size() == K && (int)p.first.size() == K, "ranges");
    if (p.pool.slots != W || (int)p.share.size() != K) return;
    int at = 0;
    uint64_t blocks = 0, busy = 0;
    int refills = 0;
    for (int c = 0; c < K; ++c) {
        const int S = p.share[(size_t)c];
        CHECK(p.first[(size_t)c] == at, "class %d starts at slot %d, expected %d", c, p.first[(size_t)c], at);
        CHECK(S >= 1 && S <= files[(size_t)c], "class %d: %d slots for %d files", c, S, files[(size_t)c]);
        if (S < 1) return;
        /* the class alone, block by block, in S slots from `at` on */
        std::vector<int> queue;
        for (int i = 0; i < n; ++i)
            if (total[(size_t)i] > 0 && cls[(size_t)i] == c) queue.push_back(i);
        if (order == ICW_POOL_LONGEST_FIRST)
            std::stable_sort(queue.begin(), queue.end(), [&](int a, int b) { return total[(size_t)a] > total[(size_t)b]; });
        std::vector<int64_t> left((size_t)S, 0);
        std::vector<char> held((size_t)S, 0);
        size_t head = 0;
        for (int64_t k = 0; head < queue.size() || std::any_of(left.begin(), left.end(), [](int64_t v) { return v > 0; }); ++k) {
            for (int s = 0; s < S && head < queue.size(); ++s) {
                if (left[(size_t)s] > 0) continue;
                const int i = queue[head++];
                CHECK(p.pool.slot[(size_t)i] == at + s && p.pool.start[(size_t)i] == k,
                      "file %d: slot %d block %lld, expected slot %d block %lld", i, p.pool.slot[(size_t)i],
                      (long long)p.pool.start[(size_t)i], at + s, (long long)k);
                left[(size_t)s] = (total[(size_t)i] + B - 1) / B;
                refills += held[(size_t)s];
                held[(size_t)s] = 1;
            }
            for (int s = 0; s < S; ++s)
                if (left[(size_t)s] > 0) {
                    --left[(size_t)s];
                    ++busy;
                }
            blocks = std::max(blocks, (uint64_t)k + 1);
        }
        at += S;
    }
    CHECK(at == W, "the shares add up to %d, the width is %d", at, W);
    CHECK(p.pool.blocks == blocks && p.pool.slot_blocks == (uint64_t)W * blocks && p.pool.busy_slot_blocks == busy &&
              p.pool.refills == refills && refills == m - W,
          "statistics: %llu blocks (%llu), busy %llu (%llu), refills %d (%d)", (unsigned long long)p.pool.blocks,
          (unsigned long long)blocks, (unsigned long long)p.pool.busy_slot_blocks, (unsigned long long)busy, p.pool.refills, refills);
    CHECK((int)p.pool.queue.size() == m, "queue of %zu, %d files take a slot", p.pool.queue.size(), m);
    for (size_t q = 1; q < p.pool.queue.size(); ++q)
        CHECK(p.pool.start[(size_t)p.pool.queue[q - 1]] <= p.pool.start[(size_t)p.pool.queue[q]], "queue not by start block");
    for (int i = 0; i < n; ++i)
        if (total[(size_t)i] <= 0) CHECK(p.pool.slot[(size_t)i] == -1 && p.pool.start[(size_t)i] == -1, "file %d has no frames but a slot", i);
    /* the C entry: classes named by any numbers, laid out by first appearance -- here the positions permuted */
    std::vector<int32_t> name((size_t)n), slot((size_t)n + 1, -7);
    std::vector<int64_t> start((size_t)n + 1, -7);
    for (int i = 0; i < n; ++i) name[(size_t)i] = 1000 - 7 * cls[(size_t)i];
    bool in_order = true;                                  /* do the positions follow first appearance already? */
    int seen = 0;
    for (int i = 0; i < n; ++i)
        if (total[(size_t)i] > 0) {
            if (cls[(size_t)i] > seen) in_order = false;
            if (cls[(size_t)i] == seen) ++seen;
        }
    icw_jobs_stats st;
    CHECK(icw_pool_plan_classes(total.data(), name.data(), n, slots, B, order, slot.data(), start.data(), &st) == ICW_OK, "C entry");
    CHECK(slot[(size_t)n] == -7 && start[(size_t)n] == -7, "icw_pool_plan_classes wrote past n entries");
    CHECK(st.classes == K && st.hilbert_runs_max == K && st.render_runs_max == K && st.kernel_s == 0.0 && st.pool.slots == W &&
              st.pool.busy_slot_blocks == busy && st.pool.batch.n_files == 0,
          "icw_pool_plan_classes: stats");
    if (in_order) {
        for (int i = 0; i < n; ++i)
            CHECK(slot[(size_t)i] == p.pool.slot[(size_t)i] && start[(size_t)i] == p.pool.start[(size_t)i], "C entry: file %d", i);
        CHECK(st.pool.blocks == blocks && st.pool.refills == refills, "C entry: blocks, refills");
    }
    if (K == 1) {
        IcwPoolPlan one;
        CHECK(icw_pool_make_plan(total.data(), n, slots, B, order, one) == ICW_OK, "icw_pool_make_plan");
        CHECK(one.slot == p.pool.slot && one.start == p.pool.start && one.n_blocks == p.pool.n_blocks && one.queue == p.pool.queue &&
                  one.slots == p.pool.slots && one.refills == p.pool.refills && one.blocks == p.pool.blocks &&
                  one.slot_blocks == p.pool.slot_blocks && one.busy_slot_blocks == p.pool.busy_slot_blocks,
              "one class is not the pool's plan");
    }
}

static icw_file_job job(uint32_t type, int kahan, int reject, uint32_t render_type, uint32_t nshape, int is24)
{
    icw_file_job j;
    memset(&j, 0, sizeof(j));
    j.render.dth_bits = 1.0;
    j.render.quantz_type = ICW_QUANTZ_MID_RISER;
    j.render.render_type = render_type;
    j.render.nshape_type = nshape;
    j.render.sign_bits16 = 16;
    j.render.sign_bits24 = 24;
    j.need24bits = is24;
    j.hilbert_type = type;
    j.iir_kahan = kahan;
    j.iir_subnorm_reject = reject;
    return j;
}

int main()
{
    const char *what = "apportionment";
    /* quotas 3, 1.5, 0.5: the third gets its one slot, then 4 slots over loads 6 : 3 -- 2.67 and 1.33, whole parts
     * 2 and 1, the leftover slot to the remainder 6/9 over 3/9 */
    check_shares("6:3:1 on 5", {6, 3, 1}, {10, 10, 10}, 5, {3, 1, 1});
    /* three equal remainders of 1/3: the tie goes to the class laid out first */
    check_shares("tie", {1, 1, 1}, {9, 9, 9}, 4, {2, 1, 1});
    check_shares("even", {5, 5}, {9, 9}, 6, {3, 3});
    /* quotas 5, 0.5, 0.5: one slot each for the small ones and 4 for the first, which has ONE file: it keeps 1, and
     * the 5 slots left go over loads 10 : 10 -- 2.5 each, the leftover slot to the lower class */
    check_shares("capped, its slots go elsewhere", {100, 10, 10}, {1, 5, 5}, 6, {1, 3, 2});
    /* quotas 0.06 and 5.94: the first gets one slot, the second 5 and is capped at its one file -- the class that
     * had its minimum takes the 5 slots left */
    check_shares("capped, its slots go to a class at its minimum", {1, 100}, {5, 1}, 6, {5, 1});
    check_shares("as wide as classes", {1000, 1, 1}, {2, 1, 1}, 3, {1, 1, 1});
    check_shares("one slot per file", {7, 1, 90}, {2, 3, 1}, 6, {2, 3, 1});
    check_shares("one class", {12}, {8}, 5, {5});
    {
        std::vector<int32_t> keep = {42};
        CHECK(!icw_pool_apportion({1, 1}, {1, 1}, 1, keep) && keep == std::vector<int32_t>{42}, "narrower than classes");
        CHECK(!icw_pool_apportion({1, 1}, {1, 1}, 3, keep) && keep == std::vector<int32_t>{42}, "wider than files");
        CHECK(!icw_pool_apportion({1, 0}, {1, 1}, 2, keep) && keep == std::vector<int32_t>{42}, "a class without load");
    }
    const int B = 256;
    what = "plans";
    const std::vector<int64_t> edge = {1 * B, B - 1, B + 1, 2, 5 * B + 3, B, 3 * B, 700, 1000};
    for (int order = 0; order < 2; ++order) {
        check_case("edges, one class", edge, std::vector<int32_t>(edge.size(), 0), 1, 3, B, order);
        check_case("edges, two classes on 3", edge, {0, 1, 0, 1, 0, 1, 0, 1, 0}, 2, 3, B, order);
        check_case("edges, four classes on 5", edge, {0, 1, 2, 3, 0, 1, 2, 3, 0}, 4, 5, B, order);
        check_case("edges, four classes on 2: raised to 4", edge, {0, 1, 2, 3, 0, 1, 2, 3, 0}, 4, 2, B, order);
        check_case("edges, one slot per file", edge, {0, 1, 2, 3, 0, 1, 2, 3, 0}, 4, 0, B, order);
        check_case("classes out of first-appearance order", edge, {2, 0, 1, 2, 0, 1, 2, 0, 1}, 3, 4, B, order);
        check_case("files without frames", {0, 700, -3, 256, 0, 9}, {5, 0, -1, 1, 9, 0}, 2, 2, B, order);
        check_case("no files", {}, {}, 0, 4, B, order);
        check_case("long files", {(int64_t)1 << 40, ((int64_t)1 << 40) + 1, 5, 70000}, {0, 1, 0, 1}, 2, 3, 65536, order);
    }
    uint64_t x = 88172645463325252ull;                       /* xorshift64 */
    auto rnd = [&](uint64_t mod) {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x % mod;
    };
    for (int c = 0; c < 500; ++c) {
        const int K = 1 + (int)rnd(5), n = K + (int)rnd(40);
        std::vector<int64_t> t((size_t)n);
        std::vector<int32_t> cl((size_t)n);
        for (int i = 0; i < n; ++i) {
            t[(size_t)i] = (int64_t)rnd(8 * B) + (i < K || rnd(9) ? 1 : 0);
            cl[(size_t)i] = i < K ? i : (int32_t)rnd((uint64_t)K);          /* every class has a file with frames */
        }
        if (rnd(2)) {                                                        /* positions not by first appearance */
            std::swap(t[0], t[(size_t)K - 1]);
            std::swap(cl[0], cl[(size_t)K - 1]);
        }
        check_case("random", t, cl, K, (int)rnd(12), B, (int)rnd(2));
    }
    what = "refusals";
    {
        IcwClassPlan keep;
        keep.pool.slots = 77;
        const int64_t t2[2] = {5, 6};
        const int32_t c2[2] = {0, 1}, gap[2] = {0, 2}, neg[2] = {0, -1};
        CHECK(icw_pool_make_plan_classes(t2, c2, 2, 2, -1, B, 0, keep) == ICW_EINVAL && keep.pool.slots == 77, "slots < 0");
        CHECK(icw_pool_make_plan_classes(t2, c2, 2, 2, 1, B, 2, keep) == ICW_EINVAL && keep.pool.slots == 77, "unknown order");
        CHECK(icw_pool_make_plan_classes(t2, c2, 2, 2, 1, 0, 0, keep) == ICW_EINVAL && keep.pool.slots == 77, "B < 1");
        CHECK(icw_pool_make_plan_classes(t2, gap, 2, 3, 1, B, 0, keep) == ICW_EINVAL && keep.pool.slots == 77, "a class without files");
        CHECK(icw_pool_make_plan_classes(t2, c2, 2, 1, 1, B, 0, keep) == ICW_EINVAL && keep.pool.slots == 77, "a class beyond K");
        CHECK(icw_pool_make_plan_classes(t2, nullptr, 2, 2, 1, B, 0, keep) == ICW_EINVAL, "no classes");
        CHECK(icw_pool_plan_classes(t2, neg, 2, 1, B, 0, nullptr, nullptr, nullptr) == ICW_EINVAL, "a negative class");
        CHECK(icw_pool_plan_classes(t2, c2, 2, 1, -1, 0, nullptr, nullptr, nullptr) == ICW_EINVAL, "block_frames < 0");
        CHECK(icw_pool_plan_classes(t2, c2, 2, 1, 0, 0, nullptr, nullptr, nullptr) == ICW_OK, "all outputs nullable");
        CHECK(icw_pool_plan_classes(nullptr, nullptr, 0, 1, 0, 0, nullptr, nullptr, nullptr) == ICW_OK, "no files");
    }
    what = "classes of jobs";
    {
        /* Hilbert settings in order of appearance: (1,K,R) (0,b,-) (4,K,R); renders: 16 ROUND, 24 TPDF+MEW44, 16 TPDF.
         * Layout: by Hilbert first, then render -- (1;16R) (1;24S) (1;16T) (0;16R) (0;16T) (4;24S) */
        const icw_file_job jobs[] = {
            job(1, 1, 1, ICW_RENDER_ROUND, 0, 0), job(0, 0, 0, ICW_RENDER_ROUND, 0, 0), job(1, 1, 1, ICW_RENDER_TPDF, ICW_NSHAPE_MEW44, 1),
            job(4, 1, 1, ICW_RENDER_TPDF, ICW_NSHAPE_MEW44, 1), job(0, 0, 0, ICW_RENDER_TPDF, 0, 0), job(1, 1, 1, ICW_RENDER_TPDF, 0, 0),
            job(1, 7, 1, ICW_RENDER_ROUND, 0, 0),   /* kahan as a flag: the class of job 0 */
            job(6, 1, 1, ICW_RENDER_ROUND, 0, 0),   /* out of range */
            job(0, 0, 0, ICW_RENDER_ROUND, 0, 9),   /* depth as a flag: 24 bit, a class of its own */
        };
        const int n = (int)(sizeof(jobs) / sizeof(jobs[0]));
        int32_t cls[16];
        CHECK(icw_file_job_classes(jobs, n, 0, cls) == 7, "real input: classes");
        const int32_t want[] = {0, 3, 1, 6, 4, 2, 0, -1, 5};
        for (int i = 0; i < n; ++i) CHECK(cls[i] == want[i], "job %d: class %d, expected %d", i, cls[i], want[i]);
        /* CWAVE: the render and the depth alone -- 16R, 24S, 16T, 24R by first appearance */
        CHECK(icw_file_job_classes(jobs, n, 1, cls) == 4, "CWAVE: classes");
        const int32_t want_cw[] = {0, 0, 1, 1, 2, 2, 0, -1, 3};
        for (int i = 0; i < n; ++i) CHECK(cls[i] == want_cw[i], "CWAVE job %d: class %d, expected %d", i, cls[i], want_cw[i]);
        CHECK(icw_file_job_classes(nullptr, 0, 0, nullptr) == 0 && icw_file_job_classes(nullptr, 2, 0, cls) == ICW_EINVAL, "arguments");
        icw_file_job bad = jobs[0];
        bad.render.sign_bits16 = 1;
        CHECK(!icw_pool_job_ok(bad) && icw_pool_job_ok(jobs[0]) && !icw_pool_job_ok(jobs[7]), "field ranges");
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("pool_plan_classes_host_check: ok\n");
    return 0;
}
