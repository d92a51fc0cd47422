/*
 * icw_pool_plan.cpp -- the slot plans of icw_transcode_files_pool and icw_transcode_files_jobs (icw_pool_plan.h:
 * the rules).  Plain C++, no HIP header: it is also built alone, under ASan + UBSan, by the Makefile's
 * hostcheck-pool and hostcheck-pool-classes.
 */
#include "icw_pool_plan.h"

#include <string.h>

#include <algorithm>
#include <numeric>

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

bool icw_pool_apportion(const std::vector<uint64_t> &load, const std::vector<int32_t> &files, int32_t W,
                        std::vector<int32_t> &share)
{
    typedef unsigned __int128 u128;
    const size_t K = load.size();
    if (files.size() != K || W < 0 || (size_t)W < K) return false;
    uint64_t all = 0;
    for (size_t c = 0; c < K; ++c) {
        if (load[c] < 1 || files[c] < 1) return false;
        all += (uint64_t)files[c];
    }
    if ((uint64_t)W > all) return false;
    std::vector<int32_t> sh(K, 0);
    std::vector<char> capped(K, 0);
    uint64_t R0 = (uint64_t)W;                            /* the slots not settled on a capped class */
    for (bool again = K > 0; again;) {
        /* one slot for every open class whose quota is below 1, until the others' quotas are all 1 or more */
        std::vector<size_t> open;
        uint64_t R = R0;
        u128 L = 0;
        for (size_t c = 0; c < K; ++c)
            if (!capped[c]) {
                open.push_back(c);
                L += load[c];
            }
        for (bool cut = true; cut;) {
            cut = false;
            std::vector<size_t> rest;
            u128 L2 = 0;
            uint64_t R2 = R;
            for (size_t c : open) {
                if ((u128)R * load[c] < L) {
                    sh[c] = 1;
                    --R2;
                    cut = true;
                } else {
                    rest.push_back(c);
                    L2 += load[c];
                }
            }
            open.swap(rest);
            L = L2;
            R = R2;
        }
        /* whole parts, then the leftover slots by largest remainder (ties: the lower class) */
        std::vector<u128> rem(K, 0);
        uint64_t given = 0;
        for (size_t c : open) {
            const u128 q = (u128)R * load[c];
            sh[c] = (int32_t)(q / L);
            rem[c] = q % L;
            given += (uint64_t)sh[c];
        }
        std::vector<size_t> by_rem(open);
        std::stable_sort(by_rem.begin(), by_rem.end(), [&](size_t a, size_t b) { return rem[a] > rem[b]; });
        for (size_t k = 0; k < by_rem.size() && given < R; ++k, ++given) ++sh[by_rem[k]];
        again = false;
        for (size_t c = 0; c < K; ++c)
            if (!capped[c] && sh[c] > files[c]) {
                sh[c] = files[c];
                capped[c] = 1;
                R0 -= (uint64_t)files[c];
                again = true;
            }
    }
    share.swap(sh);
    return true;
}

int icw_pool_make_plan_classes(const int64_t *total, const int32_t *cls, int n, int K, int32_t slots, int32_t B,
                               int32_t order, IcwClassPlan &plan)
{
    if (n < 0 || (n > 0 && (!total || !cls)) || K < 0 || slots < 0 || B < 1 ||
        (order != ICW_POOL_AS_GIVEN && order != ICW_POOL_LONGEST_FIRST))
        return ICW_EINVAL;
    std::vector<std::vector<int>> of((size_t)K);          /* per class: its files that take a slot, as given */
    std::vector<uint64_t> load((size_t)K, 0);
    std::vector<int32_t> files((size_t)K, 0);
    size_t m = 0;
    for (int i = 0; i < n; ++i) {
        if (total[i] <= 0) continue;
        if (cls[i] < 0 || cls[i] >= K) return ICW_EINVAL;
        of[(size_t)cls[i]].push_back(i);
        load[(size_t)cls[i]] += (uint64_t)((total[i] - 1) / B + 1);
        ++files[(size_t)cls[i]];
        ++m;
    }
    for (int c = 0; c < K; ++c)
        if (!files[(size_t)c]) return ICW_EINVAL;
    IcwClassPlan p;
    IcwPoolPlan &pp = p.pool;
    pp.slot.assign((size_t)n, -1);
    pp.start.assign((size_t)n, -1);
    pp.n_blocks.assign((size_t)n, 0);
    const size_t W = std::max<size_t>(slots == 0 || (size_t)slots >= m ? m : (size_t)slots, (size_t)K);
    pp.slots = (int32_t)W;
    if (!icw_pool_apportion(load, files, pp.slots, p.share)) return ICW_EINVAL;
    p.first.assign((size_t)K, 0);
    for (int c = 0, at = 0; c < K; at += p.share[(size_t)c], ++c) {
        /* the class alone, by the rules of a pool, in its share of the slots */
        p.first[(size_t)c] = at;
        std::vector<int64_t> t;
        for (int i : of[(size_t)c]) t.push_back(total[i]);
        IcwPoolPlan sub;
        const int rc = icw_pool_make_plan(t.data(), (int)t.size(), p.share[(size_t)c], B, order, sub);
        if (rc != ICW_OK) return rc;
        for (size_t q = 0; q < t.size(); ++q) {
            const size_t i = (size_t)of[(size_t)c][q];
            pp.slot[i] = at + sub.slot[q];
            pp.start[i] = sub.start[q];
            pp.n_blocks[i] = sub.n_blocks[q];
            pp.queue.push_back((int32_t)i);
        }
        pp.refills += sub.refills;
        pp.blocks = std::max(pp.blocks, sub.blocks);
        pp.busy_slot_blocks += sub.busy_slot_blocks;
    }
    std::sort(pp.queue.begin(), pp.queue.end(), [&](int a, int b) {
        return pp.start[(size_t)a] != pp.start[(size_t)b] ? pp.start[(size_t)a] < pp.start[(size_t)b]
                                                          : pp.slot[(size_t)a] < pp.slot[(size_t)b];
    });
    pp.slot_blocks = (uint64_t)pp.slots * pp.blocks;
    plan = std::move(p);
    return ICW_OK;
}

namespace {

bool same_job_render(const icw_file_job &a, const icw_file_job &b)
{
    return !a.need24bits == !b.need24bits && !memcmp(&a.render.dth_bits, &b.render.dth_bits, sizeof(double)) &&
           a.render.quantz_type == b.render.quantz_type && a.render.render_type == b.render.render_type &&
           a.render.nshape_type == b.render.nshape_type && a.render.sign_bits16 == b.render.sign_bits16 &&
           a.render.sign_bits24 == b.render.sign_bits24;
}

bool same_job_hilbert(const icw_file_job &a, const icw_file_job &b)
{
    return a.hilbert_type == b.hilbert_type && !a.iir_kahan == !b.iir_kahan && !a.iir_subnorm_reject == !b.iir_subnorm_reject;
}

/* the index of job i's setting among the distinct ones seen so far (firsts: a job of each), added when new */
template <class Same>
int setting_index(const icw_file_job *jobs, std::vector<int> &firsts, int i, Same same)
{
    for (size_t k = 0; k < firsts.size(); ++k)
        if (same(jobs[firsts[k]], jobs[i])) return (int)k;
    firsts.push_back(i);
    return (int)firsts.size() - 1;
}

}  // namespace

int icw_pool_job_classes(const icw_file_job *jobs, const char *take, int n, bool cwave, std::vector<int32_t> &pos,
                         std::vector<std::pair<int, int>> *settings)
{
    pos.assign((size_t)(n > 0 ? n : 0), -1);
    std::vector<int> hfirst, rfirst;
    std::vector<std::pair<int, int>> key((size_t)(n > 0 ? n : 0)), classes;
    for (int i = 0; i < n; ++i) {
        if (!take[i]) continue;
        const int h = cwave ? 0 : setting_index(jobs, hfirst, i, same_job_hilbert);
        key[(size_t)i] = std::make_pair(h, setting_index(jobs, rfirst, i, same_job_render));
        if (std::find(classes.begin(), classes.end(), key[(size_t)i]) == classes.end()) classes.push_back(key[(size_t)i]);
    }
    std::sort(classes.begin(), classes.end());
    if (settings) *settings = classes;
    for (int i = 0; i < n; ++i)
        if (take[i]) pos[(size_t)i] = (int32_t)(std::lower_bound(classes.begin(), classes.end(), key[(size_t)i]) - classes.begin());
    return (int)classes.size();
}

namespace {

void pool_stats_of(const IcwPoolPlan &p, icw_pool_stats *st)
{
    memset(st, 0, sizeof(*st));
    st->slots = p.slots;
    st->refills = p.refills;
    st->blocks = p.blocks;
    st->slot_blocks = p.slot_blocks;
    st->busy_slot_blocks = p.busy_slot_blocks;
}

}  // namespace

/* the limits of icw_set_stream_render (render_cfg_ok, icw_graph_compile.cpp) and of icw_set_stream_hilbert */
bool icw_pool_job_ok(const icw_file_job &j)
{
    const icw_render_cfg &r = j.render;
    return r.sign_bits16 >= 2 && r.sign_bits16 <= 16 && r.sign_bits24 >= 2 && r.sign_bits24 <= 24 && r.quantz_type <= 1 &&
           r.render_type <= 4 && j.hilbert_type <= 5;
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
    if (stats) pool_stats_of(p, stats);
    return ICW_OK;
}

extern "C" int icw_pool_plan_classes(const int64_t *total, const int32_t *cls, int n, int32_t slots, int32_t block_frames,
                                     int32_t order, int32_t *slot, int64_t *start_block, icw_jobs_stats *stats)
{
    if (block_frames < 0 || n < 0 || (n > 0 && (!total || !cls))) return ICW_EINVAL;
    /* the classes' positions: by the first file of each that takes a slot */
    std::vector<int32_t> seen, pos((size_t)n, -1);
    for (int i = 0; i < n; ++i) {
        if (total[i] <= 0) continue;
        if (cls[i] < 0) return ICW_EINVAL;
        const auto it = std::find(seen.begin(), seen.end(), cls[i]);
        pos[(size_t)i] = (int32_t)(it - seen.begin());
        if (it == seen.end()) seen.push_back(cls[i]);
    }
    IcwClassPlan p;
    const int rc = icw_pool_make_plan_classes(total, pos.data(), n, (int)seen.size(), slots,
                                              block_frames > 0 ? block_frames : 65536, order, p);
    if (rc != ICW_OK) return rc;
    for (int i = 0; i < n; ++i) {
        if (slot) slot[i] = p.pool.slot[(size_t)i];
        if (start_block) start_block[i] = p.pool.start[(size_t)i];
    }
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        pool_stats_of(p.pool, &stats->pool);
        stats->classes = stats->hilbert_runs_max = stats->render_runs_max = (int32_t)seen.size();
    }
    return ICW_OK;
}

extern "C" int icw_file_job_classes(const icw_file_job *jobs, int n, int cwave, int32_t *cls)
{
    if (n < 0 || (n > 0 && (!jobs || !cls))) return ICW_EINVAL;
    std::vector<char> take((size_t)n, 0);
    for (int i = 0; i < n; ++i) take[(size_t)i] = icw_pool_job_ok(jobs[i]);
    std::vector<int32_t> pos;
    const int K = icw_pool_job_classes(jobs, take.data(), n, cwave != 0, pos, nullptr);
    for (int i = 0; i < n; ++i) cls[i] = pos[(size_t)i];
    return K;
}
