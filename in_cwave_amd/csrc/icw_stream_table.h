/*
 * icw_stream_table.h -- internal: a per-stream setting of a context as a table of its distinct values and
 * every stream's index into it.  Plain C++17, no HIP: it compiles alone (tests/native/stream_table_check.cpp).
 * Never installed.
 *
 * A table always has at least one entry; a context whose streams all share a setting is a one-entry table
 * and not a special case.  The entries are pairwise distinct under the equality the setting is compared by,
 * every entry has a stream, and they are numbered in order of their first stream.  An edit builds a
 * candidate copy (assigned, mapped), which the setting's install puts in force or drops.  A call reads a
 * setting as the runs of its range (runs): consecutive streams on one entry.
 */
#ifndef ICW_STREAM_TABLE_H
#define ICW_STREAM_TABLE_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

/* consecutive streams of a range on one entry: the first of them, relative to the range, and how many */
template <class E> struct StreamRun {
    int s0, n;
    const E *e;
};

/* The runs of a range, in order.  One run is held in place, so a range on one entry allocates nothing;
 * the vector is used only for more than one. */
template <class E> struct StreamRuns {
    StreamRun<E> one{};
    std::vector<StreamRun<E>> more;
    size_t count = 0;

    /* n streams on entry e as one run */
    static StreamRuns single(int n, const E *e)
    {
        StreamRuns r;
        r.one = StreamRun<E>{0, n, e};
        r.count = 1;
        return r;
    }

    size_t size() const { return count; }
    const StreamRun<E> *begin() const { return count > 1 ? more.data() : &one; }
    const StreamRun<E> *end() const { return begin() + count; }
    const StreamRun<E> &operator[](size_t k) const { return begin()[k]; }
};

template <class E> struct StreamTable {
    std::vector<E> ents;                  /* never empty; pairwise distinct; numbered in order of their first stream */
    std::vector<int32_t> of;              /* [streams] */

    /* one entry for n streams */
    void reset(size_t n, const E &e)
    {
        ents.assign(1, e);
        of.assign(n, 0);
    }

    size_t size() const { return ents.size(); }
    int32_t index(size_t s) const { return of[s]; }
    const E &at(size_t s) const { return ents[(size_t)of[s]]; }

    /* whether streams [first, first + count) run one entry; a one-entry table is not scanned */
    bool uniform(size_t first, size_t count) const
    {
        if (ents.size() > 1)
            for (size_t i = 1; i < count; ++i)
                if (of[first + i] != of[first]) return false;
        return true;
    }

    /* streams [first, first + count) cut into the maximal runs of consecutive streams on one entry (none for
     * an empty range); a one-entry table is not scanned */
    StreamRuns<E> runs(size_t first, size_t count) const
    {
        if (count == 0) return StreamRuns<E>{};
        StreamRuns<E> r = StreamRuns<E>::single((int)count, &at(first));
        if (ents.size() == 1) return r;
        StreamRun<E> *cur = &r.one;
        cur->n = 1;
        for (size_t i = 1; i < count; ++i) {
            const E *e = &at(first + i);
            if (e == cur->e) {
                ++cur->n;
                continue;
            }
            if (r.more.empty()) r.more.push_back(r.one);
            r.more.push_back(StreamRun<E>{(int)i, 1, e});
            cur = &r.more.back();
        }
        if (!r.more.empty()) r.count = r.more.size();
        return r;
    }

    /* a candidate: this table with streams [first, first + count) on entry e */
    template <class Eq> StreamTable assigned(size_t first, size_t count, const E &e, Eq same) const
    {
        StreamTable t = *this;
        t.ents.push_back(e);
        for (size_t s = first; s < first + count; ++s) t.of[s] = (int32_t)t.ents.size() - 1;
        t.compact(same);
        return t;
    }

    /* a candidate: this table with every entry e replaced by f(e) */
    template <class F, class Eq> StreamTable mapped(F f, Eq same) const
    {
        StreamTable t = *this;
        for (E &e : t.ents) e = f(e);
        t.compact(same);
        return t;
    }

    /* equal entries become one (the one met first), entries no stream runs go, and the survivors are
     * numbered in order of their first stream */
    template <class Eq> void compact(Eq same)
    {
        std::vector<E> ne;
        std::vector<int32_t> map(ents.size(), -1);
        for (int32_t &e : of) {
            if (map[(size_t)e] < 0) {
                size_t k = 0;
                while (k < ne.size() && !same(ne[k], ents[(size_t)e])) ++k;
                if (k == ne.size()) ne.push_back(ents[(size_t)e]);
                map[(size_t)e] = (int32_t)k;
            }
            e = map[(size_t)e];
        }
        ents.swap(ne);
    }
};

#endif
