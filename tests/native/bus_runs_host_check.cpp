/*
 * bus_runs_host_check.cpp -- the run cutting of the mixed serial graph kernel (icw_k4_cut_runs,
 * icw_graph_compile.cpp) as a stand-alone program: built with AddressSanitizer + UBSan and run on a CPU
 * (`make -C in_cwave_amd/csrc hostcheck-bus`).  No device, no HIP call.
 *
 * For every case: each stream is covered exactly once, no wave (a 64-lane workgroup) holds two runs, wg0
 * ascends from 0 without gaps, consecutive runs differ in their entry, the returned workgroup count is the
 * runs' sum, and W -- the lanes a row of the LDS bus holds -- is the power of two that holds the widest run's
 * lanes in a workgroup, 1 .. 64.
 */
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../in_cwave_amd/csrc/icw_graph_compile.h"

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

/* ent: the list entry of every stream of the call's range; want_runs / want_W: what the case must give */
static void check_case(const char *what, const std::vector<int32_t> &ent, size_t want_runs, int want_W)
{
    const int count = (int)ent.size();
    std::vector<IcwK4Run> runs;
    int W = -1;
    const int wgs = icw_k4_cut_runs(ent.data(), count, runs, &W);
    CHECK(runs.size() == want_runs, "%zu runs, expected %zu", runs.size(), want_runs);
    CHECK(W == want_W, "W = %d, expected %d", W, want_W);
    CHECK(W >= 1 && W <= 64 && (W & (W - 1)) == 0, "W = %d is no power of two in 1 .. 64", W);
    std::vector<int> seen((size_t)count, 0);
    std::vector<int> wg_run((size_t)(wgs > 0 ? wgs : 0), -1);
    int wg = 0;
    for (size_t k = 0; k < runs.size(); ++k) {
        const IcwK4Run &r = runs[k];
        CHECK(r.wg0 == wg, "run %zu starts at workgroup %d, expected %d", k, r.wg0, wg);
        CHECK(r.n >= 1 && r.s0 >= 0 && r.s0 + r.n <= count, "run %zu covers [%d, %d) of %d streams", k, r.s0, r.s0 + r.n, count);
        CHECK(k == 0 || runs[k - 1].entry != r.entry, "runs %zu and %zu share entry %d", k - 1, k, r.entry);
        if (r.n < 1 || r.s0 < 0 || r.s0 + r.n > count) return;
        const int nw = (r.n + 63) / 64;
        for (int i = 0; i < r.n; ++i) {
            ++seen[(size_t)(r.s0 + i)];
            CHECK(ent[(size_t)(r.s0 + i)] == r.entry, "stream %d is on entry %d, its run on %d", r.s0 + i, ent[(size_t)(r.s0 + i)], r.entry);
            /* the kernel's mapping: stream s0 + i is lane i % 64 of workgroup wg0 + i / 64 */
            const int w = r.wg0 + i / 64;
            CHECK(w < wgs, "stream %d lands in workgroup %d of %d", r.s0 + i, w, wgs);
            if (w < wgs) {
                CHECK(wg_run[(size_t)w] < 0 || wg_run[(size_t)w] == (int)k, "workgroup %d holds runs %d and %zu", w, wg_run[(size_t)w], k);
                wg_run[(size_t)w] = (int)k;
            }
            CHECK(i % 64 < W, "lane %d of a workgroup is past the bus row of %d lanes", i % 64, W);
        }
        wg += nw;
    }
    CHECK(wg == wgs, "the runs take %d workgroups, the call was told %d", wg, wgs);
    for (int s = 0; s < count; ++s) CHECK(seen[(size_t)s] == 1, "stream %d is covered %d times", s, seen[(size_t)s]);
    for (int w = 0; w < wgs; ++w) CHECK(wg_run[(size_t)w] >= 0, "workgroup %d holds no stream", w);
}

int main()
{
    /* one run of 1 / 64 / 65 streams */
    check_case("one run of 1", std::vector<int32_t>(1, 3), 1, 1);
    check_case("one run of 64", std::vector<int32_t>(64, 0), 1, 64);
    check_case("one run of 65", std::vector<int32_t>(65, 2), 1, 64);
    /* 70 one-stream runs: 70 workgroups of one lane */
    {
        std::vector<int32_t> e(70);
        for (int i = 0; i < 70; ++i) e[(size_t)i] = i;
        check_case("70 one-stream runs", e, 70, 1);
    }
    /* runs of 1 / 63 / 6 over three entries, and a subset that starts inside the middle run */
    std::vector<int32_t> e;
    e.push_back(0);
    e.insert(e.end(), 63, 1);
    e.insert(e.end(), 6, 2);
    check_case("runs 1 / 63 / 6", e, 3, 64);
    check_case("subset inside a run", std::vector<int32_t>(e.begin() + 10, e.begin() + 40), 1, 32);
    check_case("subset across two runs", std::vector<int32_t>(e.begin() + 60, e.end()), 2, 8);
    check_case("subset from inside a run to the end of the next", std::vector<int32_t>(e.begin() + 61, e.begin() + 67), 2, 4);
    /* an entry that comes back is a run of its own; widths 3 / 2 / 5 round up to 8 lanes */
    check_case("an entry that returns", {4, 4, 4, 1, 1, 4, 4, 4, 4, 4}, 3, 8);
    /* 200 streams of one entry, then 2 of another: workgroups 0-3 and 4 */
    {
        std::vector<int32_t> f(200, 7);
        f.push_back(8);
        f.push_back(8);
        check_case("200 + 2", f, 2, 64);
    }
    check_case("no streams", std::vector<int32_t>(), 0, 1);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("bus_runs_host_check: ok\n");
    return 0;
}
