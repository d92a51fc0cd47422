/*
 * stream_table_check.cpp -- StreamTable (in_cwave_amd/csrc/icw_stream_table.h) against a plain per-stream
 * array, on the host: tables of 1, 2, 3 and 7 streams through random range assignments, whole-table
 * transforms that make entries collide, and resets; the entry is an int under an equality that identifies
 * some distinct values (equal modulo 5).  After every operation the table's invariants and every stream's
 * value are checked, and a candidate that is built and dropped must leave the table as it was; and runs() is
 * cut for the empty range, a one-stream range, the whole table and three random ranges and checked against
 * the model.
 * Built with -fsanitize=address,undefined and run directly (tests/test_stream_table.py).
 *
 *   stream_table_check [operations per table] [seed]      exit status 1 and a line per failure
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../in_cwave_amd/csrc/icw_stream_table.h"

static bool same(const int &a, const int &b) { return a % 5 == b % 5; }

static uint64_t rng_state;
static uint32_t rnd(uint32_t n)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33) % n;
}

/* the model: every stream's value, equal values written as the one the lowest stream holds */
static void settle(std::vector<int> &m)
{
    for (size_t s = 0; s < m.size(); ++s)
        for (size_t u = 0; u < s; ++u)
            if (same(m[u], m[s])) {
                m[s] = m[u];
                break;
            }
}

static int failures;
#define CHECK(cond, ...)                              \
    do {                                              \
        if (!(cond)) {                                \
            if (++failures <= 20) {                   \
                printf("FAIL %s: ", #cond);           \
                printf(__VA_ARGS__);                  \
                printf("\n");                         \
            }                                         \
        }                                             \
    } while (0)

/* the ranges runs() is cut for draw from a generator of their own, so the operations stay the ones they were */
static uint64_t range_state = 0x2545F4914F6CDD1Dull;
static uint32_t range_rnd(uint32_t n)
{
    range_state = range_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(range_state >> 33) % n;
}

/* runs(first, count) against the model: the runs tile the range in order without a gap, every stream of a
 * run is at the run's entry, neighbours differ in entry (each run is maximal), an empty range has none
 * and a one-entry table exactly one */
static void check_runs(const StreamTable<int> &t, const std::vector<int> &m, size_t first, size_t count, const char *op, long step)
{
    const StreamRuns<int> r = t.runs(first, count);
    CHECK((r.size() == 0) == (count == 0), "%s step %ld: runs(%zu, %zu) has %zu", op, step, first, count, r.size());
    CHECK(r.end() == r.begin() + r.size(), "%s step %ld: runs(%zu, %zu) end", op, step, first, count);
    if (count > 0 && t.size() == 1) CHECK(r.size() == 1, "%s step %ld: runs(%zu, %zu) of one entry has %zu", op, step, first, count, r.size());
    size_t at = 0, k = 0;
    for (const StreamRun<int> &q : r) {
        CHECK(&q == &r[k], "%s step %ld: runs(%zu, %zu) run %zu by index", op, step, first, count, k);
        CHECK(q.n >= 1 && (size_t)q.s0 == at, "%s step %ld: runs(%zu, %zu) run %zu at %d for %d, expected at %zu", op, step, first, count, k, q.s0, q.n, at);
        if (q.n < 1 || (size_t)q.s0 != at || at + (size_t)q.n > count) return;
        for (size_t i = 0; i < (size_t)q.n; ++i) {
            const size_t s = first + at + i;
            CHECK(q.e == &t.at(s) && *q.e == m[s], "%s step %ld: runs(%zu, %zu) run %zu stream %zu", op, step, first, count, k, s);
        }
        if (k > 0) {
            CHECK(q.e != r[k - 1].e && !same(m[first + at], m[first + at - 1]), "%s step %ld: runs(%zu, %zu) runs %zu and %zu on one entry", op, step, first, count, k - 1, k);
        }
        at += (size_t)q.n;
        ++k;
    }
    CHECK(at == count, "%s step %ld: runs(%zu, %zu) cover %zu", op, step, first, count, at);
}

static void check(const StreamTable<int> &t, const std::vector<int> &m, const char *op, long step)
{
    const size_t S = m.size();
    if (t.of.size() == S && t.size() >= 1) {
        check_runs(t, m, range_rnd((uint32_t)S + 1), 0, op, step);
        check_runs(t, m, range_rnd((uint32_t)S), 1, op, step);
        check_runs(t, m, 0, S, op, step);
        for (int i = 0; i < 3; ++i) {
            const size_t first = range_rnd((uint32_t)S);
            check_runs(t, m, first, 1 + range_rnd((uint32_t)(S - first)), op, step);
        }
    }
    CHECK(t.of.size() == S && t.size() >= 1, "%s step %ld", op, step);
    size_t distinct = 0;
    for (size_t s = 0; s < S; ++s) {
        size_t u = 0;
        while (u < s && !same(m[u], m[s])) ++u;
        if (u == s) ++distinct;
    }
    CHECK(t.size() == distinct, "%s step %ld: size %zu, model %zu", op, step, t.size(), distinct);
    for (size_t s = 0; s < S; ++s) {
        CHECK(t.index(s) >= 0 && (size_t)t.index(s) < t.size(), "%s step %ld stream %zu", op, step, s);
        CHECK(t.at(s) == m[s], "%s step %ld stream %zu: %d, model %d", op, step, s, t.at(s), m[s]);
    }
    for (size_t a = 0; a < t.size(); ++a)
        for (size_t b = a + 1; b < t.size(); ++b)
            CHECK(!same(t.ents[a], t.ents[b]), "%s step %ld: entries %zu and %zu equal (%d, %d)", op, step, a, b, t.ents[a], t.ents[b]);
    /* every entry is used, and entry k's first stream comes before entry k + 1's */
    long prev = -1;
    for (size_t k = 0; k < t.size(); ++k) {
        long f = -1;
        for (size_t s = 0; s < S && f < 0; ++s)
            if ((size_t)t.index(s) == k) f = (long)s;
        CHECK(f >= 0, "%s step %ld: entry %zu unused", op, step, k);
        CHECK(f > prev, "%s step %ld: entry %zu first at stream %ld, entry before it at %ld", op, step, k, f, prev);
        prev = f;
    }
    for (size_t f = 0; f < S; ++f)
        for (size_t n = 1; f + n <= S; ++n) {
            bool one = true;
            for (size_t i = 1; i < n; ++i) one = one && same(m[f + i], m[f]);
            CHECK(t.uniform(f, n) == one, "%s step %ld: uniform(%zu, %zu)", op, step, f, n);
        }
}

int main(int argc, char **argv)
{
    const long ops = argc > 1 ? atol(argv[1]) : 3000;
    rng_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
    const size_t sizes[] = {1, 2, 3, 7};
    long total = 0;
    for (size_t S : sizes) {
        StreamTable<int> t;
        std::vector<int> m(S, 3);
        t.reset(S, 3);
        check(t, m, "reset", 0);
        for (long step = 1; step <= ops; ++step, ++total) {
            const uint32_t what = rnd(16);
            const size_t first = rnd((uint32_t)S), count = 1 + rnd((uint32_t)(S - first));
            const int v = (int)rnd(15), mul = 1 + (int)rnd(4), add = (int)rnd(5);
            const auto f = [&](const int &e) { return what & 1 ? e / 2 : (e * mul + add) % 15; };
            const bool drop = rnd(3) == 0;               /* the candidate is built and dropped */
            const StreamTable<int> before = t;
            if (what == 0) {
                t.reset(S, v);
                m.assign(S, v);
                check(t, m, "reset", step);
            } else if (what < 10) {
                StreamTable<int> c = t.assigned(first, count, v, same);
                CHECK(t.ents == before.ents && t.of == before.of, "assigned step %ld changed the table", step);
                if (drop) continue;
                for (size_t s = first; s < first + count; ++s) m[s] = v;
                settle(m);
                check(c, m, "assigned", step);
                t = std::move(c);
            } else {
                StreamTable<int> c = t.mapped(f, same);
                CHECK(t.ents == before.ents && t.of == before.of, "mapped step %ld changed the table", step);
                if (drop) continue;
                for (int &x : m) x = f(x);
                settle(m);
                check(c, m, "mapped", step);
                t = std::move(c);
            }
            check(t, m, "after", step);
        }
    }
    printf("operations %ld failures %d\n", total, failures);
    return failures ? 1 : 0;
}
