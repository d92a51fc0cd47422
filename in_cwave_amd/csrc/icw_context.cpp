/*
 * icw_context.cpp -- the context of the in_cwave_amd C ABI (include/icw.h): its life (icw_create,
 * icw_destroy, icw_stream_init), every setter and live list edit, per-stream state in HBM, meters,
 * state (de)serialisation and the census.  The calls that run kernels are in icw_host.cpp.
 *
 * There is no CPU compute path here: every sample goes through the gfx950 kernels.  A missing or
 * unusable HIP device is an error (ICW_EDEVICE), never a fallback.
 */
#include <hip/hip_runtime_api.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/icw.h"
#include "../../include/icw_cwave.h"
#include "icw_ctx.h"
#include "icw_tables.inc"

int set_dev(icw_ctx *c)
{
    return hipSetDevice(c->device) == hipSuccess ? ICW_OK : ICW_EDEVICE;
}

/* page-locked host memory (hipHostMalloc / hipHostRegister) that device `dev` may copy from: the DMA
 * engines read it directly, so an asynchronous copy does not block the host thread.  Memory pinned
 * while another device was current counts only if it was pinned portable (hipHostMallocPortable /
 * hipHostRegisterPortable, as icw_host_alloc does): the shards of icw_group_process hand slices of one
 * caller buffer to contexts on different devices.  Anything else takes the whole-call staging copies.
 * A pageable pointer makes the query fail; the error is cleared so that it does not surface as the
 * call's own. */
bool host_pinned(const void *p, int dev)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost && (a.device == dev || (a.allocationFlags & hipHostMallocPortable));
}

/* wait for every kernel and copy of the context (they run on several streams, the caller's among
 * them); host-side state changes and reads happen only between calls */
hipError_t quiesce(icw_ctx *c)
{
    (void)c;
    return hipDeviceSynchronize();
}

namespace {

/* The CU-masked stream sets are shared by the contexts of a device (created on first use, destroyed
 * with the device's last context), so a process that opens many contexts does not multiply queues.
 * Sharing only adds ordering between contexts that run on the same device at the same time. */
std::mutex g_split_mu;
std::list<std::pair<int, CuSplit>> g_splits;     /* list: entries never move */
std::map<int, int> g_live;                       /* device -> live contexts */

void split_ref(int device, int delta)
{
    std::lock_guard<std::mutex> lk(g_split_mu);
    if ((g_live[device] += delta) > 0) return;
    for (auto it = g_splits.begin(); it != g_splits.end();) {
        if (it->first != device) { ++it; continue; }
        for (hipStream_t q : {it->second.k1, it->second.rest, it->second.dith, it->second.render})
            if (q) (void)hipStreamDestroy(q);
        it = g_splits.erase(it);
    }
}

}  // namespace

/* The stream set for a K1 of k1_cus CUs (a multiple of the XCD count): K1's CUs are spread evenly
 * over the XCDs and their shader engines, the other streams get the remaining CUs.
 * Queue CU-mask bits on gfx950 are dealt round-robin: bit b selects XCD b % 8, and within it the
 * (b / 8)-th CU, whose shader-engine group is again (b / 8) % 4 (measured, tools/cumask_probe.hip).
 * An XCD with no bit set in a mask runs that queue's work on ALL of its CUs, so each mask must
 * name CUs in every XCD: the K1 mask is bits [0, k1_cus), the rest its complement. */
const CuSplit *cu_split(icw_ctx *c, int k1_cus)
{
    std::lock_guard<std::mutex> lk(g_split_mu);
    const int rest_cus = c->tn.rest_cus >= 0 ? c->tn.rest_cus : std::max(c->n_cu - k1_cus - 32, c->n_cu / 2);
    for (auto &x : g_splits)
        if (x.first == c->device && x.second.k1_cus == k1_cus && x.second.rest_cus == rest_cus) return &x.second;
    const int n = c->n_cu, words = (n + 31) / 32;
    std::vector<uint32_t> mk(words, 0u), mr(words, 0u);
    std::vector<char> used(n, 0);
    for (int i = 0; i < k1_cus && i < n; ++i) used[i] = 1;
    int n_rest = 0;
    for (int cu = 0; cu < n; ++cu) {
        if (used[cu]) mk[cu / 32] |= 1u << (cu % 32);
        else if (rest_cus == 0 || n_rest++ < rest_cus) mr[cu / 32] |= 1u << (cu % 32);
    }
    CuSplit x;
    x.k1_cus = k1_cus;
    x.rest_cus = rest_cus;
    if (hipExtStreamCreateWithCUMask(&x.k1, (uint32_t)words, mk.data()) != hipSuccess ||
        hipExtStreamCreateWithCUMask(&x.rest, (uint32_t)words, mr.data()) != hipSuccess ||
        hipExtStreamCreateWithCUMask(&x.dith, (uint32_t)words, mr.data()) != hipSuccess ||
        hipExtStreamCreateWithCUMask(&x.render, (uint32_t)words, mr.data()) != hipSuccess) {
        for (hipStream_t q : {x.k1, x.rest, x.dith, x.render})
            if (q) (void)hipStreamDestroy(q);
        return nullptr;
    }
    g_splits.emplace_back(c->device, x);
    return &g_splits.back().second;
}

namespace {

/* modified Bessel function I0 by its power series sum ((x/2)^k / k!)^2, to a relative 1e-17 */
double bessel_i0(double x)
{
    const double h = x / 2.0;
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 1000; ++k) {
        term *= h / (double)k;
        const double t2 = term * term;
        sum += t2;
        if (t2 < sum * 1e-17) break;
    }
    return sum;
}

/* FIR histories of streams [f, f+n) to zero (a fresh or reset converter) */
bool fir_clear(icw_ctx *c, size_t f, size_t n, hipStream_t st)
{
    bool ok = true;
    const size_t at = c->fir_off[f], len = c->fir_off[f + n] - at;     /* every stream's rows at its own order */
    for (double *h : c->fir_hist)
        if (h && len) ok &= hipMemsetAsync(h + at, 0, len * sizeof(double), st) == hipSuccess;
    return ok;
}

void free_all(icw_ctx *c)
{
    DevState &s = c->st;
    void *ptrs[] = {c->enc_clipped, c->s1_stamps, s.mt, s.mt_idx, s.rs, s.lr_equal, s.fes, s.err, s.hist, s.sncnt, s.hq_phase, s.pos, s.fade,
                    s.n_frame, s.bus, s.clips, s.peak_bits, c->d_prog, c->d_progs, c->d_bprogs, c->d_bruns, c->d_pid, c->d_inputs, c->d_rtab, c->d_hpc, c->trig, c->d_in, c->d_out,
                    c->d_pre, c->d_xin,
                    c->d_fir_g, c->d_fconv, c->fir_hist[0], c->fir_hist[1], c->dwords, c->dbk, c->dflag};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    for (int p = 0; p < kSets; ++p) {
        for (void *q : {(void *)c->info_dup[p], (void *)c->w[p], (void *)c->xd[p], (void *)c->dith[p],
                        (void *)c->rpre[p], (void *)c->iq[p]})
            if (q) (void)hipFree(q);
        for (hipEvent_t e : {c->ditdone[p], c->k1done[p], c->k2done[p], c->k0done[p], c->k3done[p]})
            if (e) (void)hipEventDestroy(e);
    }
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->stream3) (void)hipStreamDestroy(c->stream3);
    if (c->stream4) (void)hipStreamDestroy(c->stream4);
    if (c->stream_io) (void)hipStreamDestroy(c->stream_io);
    for (auto e : c->ev_io) (void)hipEventDestroy(e);
    if (c->join) (void)hipEventDestroy(c->join);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    for (auto e : c->ev) (void)hipEventDestroy(e);
    for (auto e : c->ev_k0) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
}

/* a (type, summation, reject) setting as a table entry: the filter coefficients of the type exactly as
 * iir_rp_create (hblpf.c:849-856) */
HilbEnt make_hilb(uint32_t type, int kahan, int subn)
{
    HilbEnt e;
    const int t = (int)type;
    e.type = type;
    e.kahan = kahan ? 1 : 0;
    e.subn = subn ? 1 : 0;
    e.nord = icw_hb_order[t];
    const double a0 = u2d(icw_hb_a[t][0]);
    e.d0 = u2d(icw_hb_b[t][0]) / a0;
    for (int i = 0; i < e.nord; ++i) {
        e.pc[i] = -u2d(icw_hb_a[t][i + 1]) / a0;
        e.pd[i] = u2d(icw_hb_b[t][i + 1]) / a0;
    }
    return e;
}

bool same_hilb(const HilbEnt &a, const HilbEnt &b) { return a.type == b.type && a.kahan == b.kahan && a.subn == b.subn; }

/* the converter table's mirrors: cfg's three fields and the coefficients of entry 0 */
void mirror_hilbs(icw_ctx *c)
{
    const HilbEnt &e = c->hilbs.ents[0];
    c->cfg.hilbert_type = e.type;
    c->cfg.iir_kahan = e.kahan;
    c->cfg.iir_subnorm_reject = e.subn;
    c->nord = e.nord;
    c->d0 = e.d0;
    memcpy(c->pc, e.pc, sizeof(c->pc));
    memcpy(c->pd, e.pd, sizeof(c->pd));
}

/* converters of streams [f, f + n) as hq_rp_create leaves them: zero rings, phases 0, counters 0, lr_equal 1.
 * Queued on st; the caller waits for it */
bool reset_rings(icw_ctx *c, size_t f, size_t n, hipStream_t st)
{
    DevState &s = c->st;
    bool ok = hipMemsetAsync(s.hist + f * 4 * ICW_HIST_PITCH, 0, n * 4 * ICW_HIST_PITCH * sizeof(double), st) == hipSuccess;
    ok &= hipMemsetAsync(s.sncnt + f * 4, 0, n * 4 * sizeof(unsigned long long), st) == hipSuccess;
    ok &= hipMemsetAsync(s.hq_phase + f * 2, 0, n * 2 * sizeof(uint32_t), st) == hipSuccess;
    ok &= hipMemsetD32Async((hipDeviceptr_t)(s.lr_equal + f * 2), 1, n * 2, st) == hipSuccess;
    for (size_t i = 0; i < n; ++i) c->lr_known[f + i] = 1;
    return ok;
}

/* renders of streams [f, f + n) as sound_render_init leaves them (in_cwave.c:69-70): MT19937
 * seeded (mtrnd_init_seed), next draw twists, shaping state zero.  Synchronous. */
bool seed_renders(icw_ctx *c, size_t f, size_t n, hipStream_t st)
{
    DevState &s = c->st;
    const size_t G = (size_t)c->n_streams * 2;
    std::vector<uint32_t> col((size_t)624 * n * 2);
    for (int i = 0; i < 624; ++i)
        for (size_t k = 0; k < n * 2; ++k) col[(size_t)i * n * 2 + k] = c->mt_seed_state[k & 1][i];
    std::vector<int32_t> idx(n * 2, 624);
    bool ok = hipMemcpy2DAsync(s.mt + f * 2, G * 4, col.data(), n * 2 * 4, n * 2 * 4, 624, hipMemcpyHostToDevice,
                               st) == hipSuccess;
    ok &= hipMemcpyAsync(s.mt_idx + f * 2, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, st) == hipSuccess;
    ok &= hipMemsetAsync(s.rs + f * 2 * ICW_RSTATE, 0, n * 2 * ICW_RSTATE * sizeof(double), st) == hipSuccess;
    ok &= hipStreamSynchronize(st) == hipSuccess;   /* the host sources live until here */
    return ok;
}

/* the serial render's per-channel state, allocated when a live change first needs it.  Until then
 * every render was ROUND + flat, which draws no random numbers and keeps no shaping state, so the
 * freshly seeded state is the reference's state at this point. */
int ensure_render_state(icw_ctx *c)
{
    DevState &s = c->st;
    if (s.mt) return ICW_OK;
    const size_t S = (size_t)c->n_streams;
    int rc = dalloc(&s.mt, (size_t)624 * S * 2);
    rc |= dalloc(&s.mt_idx, S * 2);
    rc |= dalloc(&s.rs, S * 2 * ICW_RSTATE);
    if (rc == ICW_OK && !seed_renders(c, 0, S, c->stream)) rc = ICW_EDEVICE;
    if (rc != ICW_OK) {
        for (void *p : {(void *)s.mt, (void *)s.mt_idx, (void *)s.rs})
            if (p) (void)hipFree(p);
        s.mt = nullptr;
        s.mt_idx = nullptr;
        s.rs = nullptr;
        return rc == ICW_ENOMEM ? ICW_ENOMEM : ICW_EDEVICE;
    }
    return ICW_OK;
}

/* sound_render_recalc for streams [f, f + n): prev_rnd, the shaper rings and prev_ns_err start again, the
 * MT19937 words go on (sound_render.c:527-580) */
bool restart_shaping(icw_ctx *c, size_t f, size_t n)
{
    return !c->st.rs || hipMemset(c->st.rs + f * 2 * ICW_RSTATE, 0, n * 2 * ICW_RSTATE * sizeof(double)) == hipSuccess;
}

/* mod_context_clear_all_inouts (in_cwave.c:255-261) for streams [first, first + count): slot `slot` of their
 * bus to zero.  The context's work has been waited for (quiesce). */
int clear_slot_range(icw_ctx *c, int first, int count, int slot)
{
    if (slot < 0 || slot >= ICW_N_INPUTS || count <= 0) return ICW_OK;
    const size_t pitch = (size_t)ICW_N_INPUTS * 4 * sizeof(double);
    return hipMemset2D(c->st.bus + ((size_t)first * ICW_N_INPUTS + (size_t)slot) * 4, pitch, 0, 4 * sizeof(double),
                       (size_t)count) == hipSuccess ? ICW_OK : ICW_EDEVICE;
}

/* ---- the render table (icw_set_render, icw_set_outbits, icw_set_stream_render) ---- */

/* a (render, depth) pair as a table entry: render_consts, and how it runs behind the context's list */
RenderEnt make_render(const icw_ctx *c, const icw_render_cfg &r, int is24)
{
    RenderEnt e;
    e.cfg = r;
    e.is24 = is24 ? 1 : 0;
    render_consts(r, e.is24, c->tn.k3r_spec, e.rk);
    icw_config cfg = c->cfg;
    cfg.render = r;
    cfg.need24bits = e.is24;
    /* it follows the list while the context has one; with bus-form lists beside others (bus_lists) it is the
     * render's own -- a call adds its form -- and the state is kept for the calls that run serial */
    static const IcwProg reg_form{};
    const IcwProg &lp = c->bus_lists ? reg_form : c->prog;
    e.serial = needs_serial(cfg, e.rk, lp, c->tn.dith_par);
    e.rstate = needs_render_state(cfg, e.rk, lp, c->tn.dith_par) || c->bus_lists;
    e.dither = r.render_type != ICW_RENDER_ROUND;
    return e;
}

bool same_render(const RenderEnt &a, const RenderEnt &b)
{
    return a.is24 == b.is24 && !memcmp(&a.cfg.dth_bits, &b.cfg.dth_bits, sizeof(double)) &&
           a.cfg.quantz_type == b.cfg.quantz_type && a.cfg.render_type == b.cfg.render_type &&
           a.cfg.nshape_type == b.cfg.nshape_type && a.cfg.sign_bits16 == b.cfg.sign_bits16 &&
           a.cfg.sign_bits24 == b.cfg.sign_bits24;
}

/* the render table's mirrors: entry 0, and whether any entry runs serial / keeps render state */
void mirror_renders(icw_ctx *c)
{
    const RenderEnt &e0 = c->renders.ents[0];
    c->cfg.render = e0.cfg;
    c->cfg.need24bits = e0.is24;
    c->rk = e0.rk;
    c->serial_render = c->render_state = false;
    for (const RenderEnt &e : c->renders.ents) {
        c->serial_render |= e.serial;
        c->render_state |= e.rstate;
    }
}

/* The device keeps each channel's largest |q| and get_meters turns it into dB against the render's
 * current hi bound.  Before a render change moves that bound, the peaks so far are folded into the
 * host's dB meters against the old bound (the reference converts every sample with the bound of
 * its time, sound_render.c:769-780) and the device maxima start again: for the streams of [first, first +
 * count) whose bound differs in t, a stretch of them per memset; nothing is read when no bound moves. */
bool fold_peaks(icw_ctx *c, const StreamTable<RenderEnt> &t, int first, int count)
{
    const auto moves = [&](int s) { return c->renders.at((size_t)s).rk.hi != t.at((size_t)s).rk.hi; };
    const int end = first + count;
    int i = first;
    while (i < end && !moves(i)) ++i;
    if (i == end) return true;
    std::vector<unsigned long long> pb((size_t)count * 2);
    if (hipMemcpy(pb.data(), c->st.peak_bits + (size_t)first * 2, pb.size() * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return false;
    while (i < end) {
        int j = i + 1;
        while (j < end && moves(j)) ++j;
        if (hipMemset(c->st.peak_bits + (size_t)i * 2, 0, (size_t)(j - i) * 16) != hipSuccess) return false;
        for (size_t k = (size_t)i * 2; k < (size_t)j * 2; ++k) {
            double mx;
            memcpy(&mx, &pb[k - (size_t)first * 2], 8);
            const double cv = mx ? 20.0 * log10(mx / c->renders.at(k / 2).rk.hi) : ICW_SR_ZERO_SIGNAL_DB;
            if (cv > c->peak_db[k]) c->peak_db[k] = cv;
        }
        for (i = j; i < end && !moves(i); ++i) {}
    }
    return true;
}

/* Install a candidate render table (the caller holds c->mu and has waited for the context's work); the
 * shaping state of streams [first, first + count) restarts.  Refusals and the device copies (table and index
 * row, into fresh memory) come before any state is touched, so a failure leaves the old renders in force;
 * then the peaks of the streams whose bound moves are folded against their old bound, the shaping state
 * restarts (the MT19937 words go on) and the host side follows. */
int install_renders(icw_ctx *c, StreamTable<RenderEnt> &t, int first, int count)
{
    const size_t n = t.size(), S = (size_t)c->n_streams;
    /* more than one render: K3's FP_CHECK form, K4 and the FIR converter's fused render take one */
    if (n > 1 && (c->fir_M > 0 || c->cfg.fp_check || c->prog.is_bus || c->bus_lists)) return ICW_EUNSUPPORTED;
    bool rstate = false;
    for (const RenderEnt &e : t.ents) rstate |= e.rstate;
    int rc;
    if (rstate && (rc = ensure_render_state(c))) return rc;
    IcwRenderEnt *fresh = nullptr;
    if (n > 1) {
        const size_t tb = n * sizeof(IcwRenderEnt);
        std::vector<unsigned char> h(tb + S * sizeof(int32_t), 0);
        for (size_t k = 0; k < n; ++k) {
            IcwRenderEnt d;
            memset(&d, 0, sizeof(d));
            d.rk = t.ents[k].rk;
            d.serial = t.ents[k].serial ? 1 : 0;
            d.dither = t.ents[k].dither ? 1 : 0;
            d.fsz = t.ents[k].osz();
            memcpy(h.data() + k * sizeof(IcwRenderEnt), &d, sizeof(d));
        }
        memcpy(h.data() + tb, t.of.data(), S * sizeof(int32_t));
        if (hipMalloc((void **)&fresh, h.size()) != hipSuccess) return ICW_ENOMEM;
        if (hipMemcpy(fresh, h.data(), h.size(), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(fresh);
            return ICW_EDEVICE;
        }
    }
    if (!fold_peaks(c, t, first, count) || !restart_shaping(c, (size_t)first, (size_t)count)) {
        if (fresh) (void)hipFree(fresh);
        return ICW_EDEVICE;
    }
    if (c->d_rtab) (void)hipFree(c->d_rtab);
    c->d_rtab = fresh;
    c->d_rof = fresh ? (int32_t *)((unsigned char *)fresh + n * sizeof(IcwRenderEnt)) : nullptr;
    c->renders = std::move(t);
    mirror_renders(c);
    return ICW_OK;
}

/* ---- the list table (icw_set_graph, icw_set_stream_graph, the list primitives) ---- */

bool same_list(const ListEnt &a, const ListEnt &b)
{
    return !memcmp(&a.prog, &b.prog, sizeof(IcwProg)) && a.nodes.size() == b.nodes.size() &&
           (a.nodes.empty() || !memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(icw_node)));
}

/* the list table's mirrors: entry 0 (with several entries the render setters ask bus_lists, not its is_bus) */
void mirror_lists(icw_ctx *c)
{
    const ListEnt &e = c->lists.ents[0];
    c->prog = e.prog;
    c->nodes = e.nodes;
    c->cfg.bypass_list = e.prog.bypass;
}

/* Install a candidate list table (the caller holds c->mu and has waited for the context's work).  The
 * device copies come first, into memory the running table does not use where the table grows, so a
 * failed copy leaves the old lists in force on both sides.  One entry: the context launches from d_prog,
 * as it always did. */
int install_lists(icw_ctx *c, StreamTable<ListEnt> &t)
{
    const size_t n = t.size();
    IcwProg *fresh = nullptr;
    /* bus-form lists beside others: a call over them renders serial whatever the render is */
    bool bus_lists = false;
    for (const ListEnt &e : t.ents) bus_lists = bus_lists || (n > 1 && e.prog.is_bus);
    int rs;
    if (bus_lists && (rs = ensure_render_state(c)) != ICW_OK) return rs;
    if (n > 1) {
        std::vector<IcwProg> h(n);                   /* the contiguous array d_progs holds */
        for (size_t k = 0; k < n; ++k) h[k] = t.ents[k].prog;
        if (n > c->d_progs_cap && hipMalloc((void **)&fresh, n * sizeof(IcwProg)) != hipSuccess) return ICW_ENOMEM;
        if (!c->d_pid && dalloc(&c->d_pid, (size_t)c->n_streams * kPidWords) != ICW_OK) {
            if (fresh) (void)hipFree(fresh);
            c->d_pid = nullptr;
            return ICW_ENOMEM;
        }
        if (hipMemcpy(fresh ? fresh : c->d_progs, h.data(), n * sizeof(IcwProg), hipMemcpyHostToDevice) != hipSuccess) {
            if (fresh) (void)hipFree(fresh);
            return ICW_EDEVICE;
        }
    }
    /* d_prog follows prog (entry 0): the paths that read the pair (the encoders) see one program */
    if (hipMemcpy(c->d_prog, &t.ents[0].prog, sizeof(IcwProg), hipMemcpyHostToDevice) != hipSuccess) {
        if (fresh) (void)hipFree(fresh);
        return ICW_EDEVICE;
    }
    if (fresh) {
        if (c->d_progs) (void)hipFree(c->d_progs);
        c->d_progs = fresh;
        c->d_progs_cap = n;
    }
    c->lists = std::move(t);
    mirror_lists(c);
    c->bus_lists = bus_lists;
    ++c->lists_gen;                       /* the mixed K4's programs and runs follow the lists too */
    /* c->mix and the selection rows are built from the lists (prepare_mix): rebuilt by the next call */
    c->pid_valid = false;
    return ICW_OK;
}

/* the normalised list nv as a table entry: compiled under the context's config with its own bypass flag */
int compile_list(const icw_ctx *c, const std::vector<icw_node> &nv, int bypass, ListEnt &L)
{
    icw_config cfg = c->cfg;
    cfg.bypass_list = bypass;
    L.nodes = nv;
    const int rc = build_prog(cfg, nv, L.prog);
    if (rc == ICW_OK && !c->tn.chain_ok) L.prog.chain = L.prog.sig = 0;
    return rc;
}

/* replace_output_plug (adv_modulator.c:176-209) of the nodes a list edit removed or re-plugged, matched by
 * position against every old entry (include/icw.h): their old output slots read zero from now on */
std::vector<std::vector<int>> matched_clears_per_entry(const icw_ctx *c, const std::vector<icw_node> &nv)
{
    std::vector<std::vector<int>> per(c->lists.size());
    for (size_t e = 0; e < per.size(); ++e) matched_clears(c->lists.ents[e].nodes, nv, per[e]);
    return per;
}

/* the clears of an installed list edit over streams [first, first + count): per[e] for the streams that ran
 * entry e before (old_of), a stretch of them per memset.  The lists went to the device first, so a failed
 * copy left the old lists and the old bus on both sides; a failed clear here returns ICW_EDEVICE with the new
 * lists in place (the context is quiesced, so the order of the two steps changes no output). */
int clear_matched(icw_ctx *c, const std::vector<int32_t> &old_of, int first, int count, const std::vector<std::vector<int>> &per)
{
    for (int i = first; i < first + count;) {
        int j = i + 1;
        while (j < first + count && old_of[(size_t)j] == old_of[(size_t)i]) ++j;
        for (int slot : per[(size_t)old_of[(size_t)i]])
            if (clear_slot_range(c, i, j - i, slot) != ICW_OK) return ICW_EDEVICE;
        i = j;
    }
    return ICW_OK;
}

/* A context-wide list edit (icw_set_graph, the list primitives; the caller holds c->mu and has waited for
 * the context's work): compile the normalised list nv and put every stream on it; per[e] are the clears of
 * the streams of entry e. */
int apply_graph(icw_ctx *c, const std::vector<icw_node> &nv, int bypass, const std::vector<std::vector<int>> &per)
{
    ListEnt L;
    int rc = compile_list(c, nv, bypass, L);
    if (rc) return rc;
    /* a bus-form list runs K4, one lane per stream on one program into one serial render, and one K2
     * instance: refused while the lists, the renders or the converters differ (include/icw.h; the host
     * collapses with a register-form list first).  With icw_enable_stream_bus differing lists do not refuse
     * it: the table collapses to this list as to any other */
    if (L.prog.is_bus && ((c->lists.size() > 1 && !c->bus_streams) || c->renders.size() > 1 || c->hilbs.size() > 1))
        return ICW_EUNSUPPORTED;
    /* How the render runs follows the list only here, and only for the one render of a one-render context: a
     * bus-form list makes it serial.  Several renders stand beside register-form lists alone (above), which
     * change none of them, and the per-stream list setter takes register-form lists only -- so neither
     * recomputes, as neither ever did. */
    RenderEnt r0 = c->renders.ents[0];
    if (c->renders.size() == 1) {
        r0.serial = needs_serial(c->cfg, r0.rk, L.prog, c->tn.dith_par);
        r0.rstate = needs_render_state(c->cfg, r0.rk, L.prog, c->tn.dith_par);
        if (r0.rstate && (rc = ensure_render_state(c))) return rc;
    }
    const std::vector<int32_t> old_of = c->lists.of;
    StreamTable<ListEnt> t;
    t.reset((size_t)c->n_streams, L);
    if ((rc = install_lists(c, t)) != ICW_OK) return rc;
    if (c->renders.size() == 1) {
        c->renders.ents[0] = r0;
        mirror_renders(c);
    }
    return clear_matched(c, old_of, 0, c->n_streams, per);
}


/* ---- the input table (icw_set_input, icw_set_stream_input) ---- */

IcwInDesc make_input(uint32_t sample_rate, uint32_t fmt, uint32_t channels)
{
    IcwInDesc d;
    memset(&d, 0, sizeof(d));
    d.fmt = fmt;
    d.csz = fmt_size(fmt);
    d.fsz = d.csz * channels;
    d.nch = channels;
    d.sample_rate = sample_rate;
    d.ssr = (unsigned long long)sample_rate * ICW_HZ_SCALE;
    return d;
}

bool same_input(const IcwInDesc &a, const IcwInDesc &b)
{
    return a.fmt == b.fmt && a.nch == b.nch && a.sample_rate == b.sample_rate;
}

bool any_cwave(const StreamTable<IcwInDesc> &t)
{
    for (const IcwInDesc &d : t.ents)
        if (d.fmt >= ICW_FMT_CW_F64) return true;
    return false;
}

/* the input table's mirrors: cfg's three fields are the one input.  While the inputs differ they keep the
 * one last in force alone, not entry 0: icw_set_stream_input's CWAVE refusal and the encoders' plan read
 * them, and did so before the inputs were a table */
void mirror_inputs(icw_ctx *c)
{
    if (c->inputs.size() > 1) return;
    const IcwInDesc &d = c->inputs.ents[0];
    c->cfg.sample_rate = d.sample_rate;
    c->cfg.in_format = d.fmt;
    c->cfg.in_channels = d.nch;
}

/* Install a candidate input table (the caller holds c->mu and has waited for the context's work).  The device
 * table, one descriptor per stream, comes first (it is allocated by the first install that needs it): a
 * failed allocation or copy leaves the old inputs in force */
int install_inputs(icw_ctx *c, StreamTable<IcwInDesc> &t)
{
    if (t.size() > 1) {
        const size_t S = (size_t)c->n_streams;
        std::vector<IcwInDesc> h(S);
        for (size_t s = 0; s < S; ++s) h[s] = t.at(s);
        IcwInDesc *fresh = nullptr;
        if (!c->d_inputs && hipMalloc((void **)&fresh, S * sizeof(IcwInDesc)) != hipSuccess) return ICW_ENOMEM;
        if (!c->d_pid && dalloc(&c->d_pid, S * kPidWords) != ICW_OK) {
            if (fresh) (void)hipFree(fresh);
            if (c->d_pid) (void)hipFree(c->d_pid);
            c->d_pid = nullptr;
            return ICW_ENOMEM;
        }
        if (hipMemcpy(fresh ? fresh : c->d_inputs, h.data(), S * sizeof(IcwInDesc), hipMemcpyHostToDevice) != hipSuccess) {
            if (fresh) (void)hipFree(fresh);
            return ICW_EDEVICE;
        }
        if (fresh) c->d_inputs = fresh;
    }
    c->inputs = std::move(t);
    mirror_inputs(c);
    c->pid_valid = false;                 /* the selection rows carry the rate and the channels */
    return ICW_OK;
}

/* ---- the converter table (icw_set_hilbert_filter, icw_set_hilbert_config, icw_set_stream_hilbert) ---- */

/* Install a candidate converter table (the caller holds c->mu and has waited for the context's work).
 * Refusals and the device copy (the entries' coefficients, into fresh memory with room for a call's run
 * descriptors) come before any state is touched, so a failure leaves the old settings in force.  Then every
 * stream whose type changes has its converters re-created (reset_rings), a stretch of them at a time; a
 * stream that keeps its type keeps its rings; and the de-subnorm counters of streams [first, first + count)
 * restart (iir_rp_setcfg: "new world"). */
int install_hilberts(icw_ctx *c, StreamTable<HilbEnt> &t, int first, int count)
{
    const size_t n = t.size(), S = (size_t)c->n_streams;
    /* more than one setting: the FIR converter replaces the IIR for every stream, K1f (FP_CHECK) and the
     * bus-form path run one instance */
    if (n > 1 && (c->fir_M > 0 || c->cfg.fp_check || c->prog.is_bus || c->bus_lists)) return ICW_EUNSUPPORTED;
    double *fresh = nullptr;
    const size_t pc_bytes = n * 20 * sizeof(double), run_bytes = S * sizeof(IcwK1Run);
    if (n > 1) {
        std::vector<double> h(n * 20);
        for (size_t k = 0; k < n; ++k) memcpy(&h[k * 20], t.ents[k].pc, sizeof(t.ents[k].pc));
        if (hipMalloc((void **)&fresh, pc_bytes + run_bytes + 5 * S * sizeof(int32_t)) != hipSuccess) return ICW_ENOMEM;
        if (hipMemcpy(fresh, h.data(), pc_bytes, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(fresh);
            return ICW_EDEVICE;
        }
    }
    const auto changes = [&](size_t s) { return t.at(s).type != c->hilbs.at(s).type; };
    bool ok = true;
    for (size_t i = 0; i < S && ok; ++i) {
        if (!changes(i)) continue;
        size_t j = i + 1;
        while (j < S && changes(j)) ++j;
        ok = reset_rings(c, i, j - i, c->stream);
        i = j;
    }
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
    if (ok && count > 0)
        ok = hipMemset(c->st.sncnt + (size_t)first * 4, 0, (size_t)count * 4 * sizeof(unsigned long long)) == hipSuccess;
    if (!ok) {
        if (fresh) (void)hipFree(fresh);
        return ICW_EDEVICE;
    }
    if (c->d_hpc) (void)hipFree(c->d_hpc);
    c->d_hpc = fresh;
    c->d_hruns = fresh ? (IcwK1Run *)((unsigned char *)fresh + pc_bytes) : nullptr;
    c->d_hpid = fresh ? (int32_t *)((unsigned char *)fresh + pc_bytes + run_bytes) : nullptr;
    c->hrun_valid = false;
    c->hilbs = std::move(t);
    mirror_hilbs(c);
    return ICW_OK;
}

/* ---- the FIR converter table (icw_set_fir_hilbert, icw_set_stream_fir) ---- */

bool same_fir(const FirEnt &a, const FirEnt &b) { return a.M == b.M && !memcmp(&a.beta, &b.beta, sizeof(double)); }

/* Install a candidate FIR converter table (the caller holds c->mu and has waited for the context's work); the
 * streams [first, first + count) start from a zero history.  Everything the device needs -- the entries' taps,
 * the two history buffers at the new orders, the streams' descriptors while the entries are several -- is
 * built in fresh memory first, so a failure leaves the old converters in force.  The history is re-laid by
 * the new orders: a stream outside the range keeps its order, so the streams before the range keep their
 * offsets and the streams after it move as one piece; both pieces are copied from the buffer in force
 * (fir_par) into the fresh buffer 0, the range itself stays zero, and the parity restarts. */
int install_firs(icw_ctx *c, StreamTable<FirEnt> &t, int first, int count)
{
    const size_t n = t.size(), S = (size_t)c->n_streams, f = (size_t)first, e = f + (size_t)count;
    const bool on = t.ents[0].M > 0;                  /* all FIR or none: every entry is, or the one is off */
    std::vector<double> g;
    std::vector<size_t> off(S + 1, 0);
    int mmax = 0;
    for (FirEnt &x : t.ents) {
        if (!on) break;
        x.goff = g.size();
        x.nt = (x.M / 2 + 1) / 2;
        g.resize(x.goff + (size_t)((x.nt + 1) & ~1));   /* every entry's taps 16-byte aligned */
        if (icw_fir_taps(x.M, x.beta, g.data() + x.goff, x.nt) != x.nt) return ICW_EINVAL;
        mmax = std::max(mmax, x.M);
    }
    for (size_t s = 0; s < S; ++s) off[s + 1] = off[s] + 2 * (size_t)t.at(s).M;
    double *fg = nullptr, *h0 = nullptr, *h1 = nullptr;
    IcwFirConv *fd = nullptr;
    int32_t *pid = nullptr;
    const auto drop = [&](int rc) {
        for (void *p : {(void *)fg, (void *)h0, (void *)h1, (void *)fd, (void *)pid})
            if (p) (void)hipFree(p);
        return rc;
    };
    if (on) {
        int rc = dalloc(&fg, g.size());
        rc |= dalloc(&h0, off[S]);
        rc |= dalloc(&h1, off[S]);
        /* several entries: every call takes the per-stream kernels, which read K2's selection rows */
        if (n > 1 && !c->d_pid) rc |= dalloc(&pid, S * kPidWords);
        if (n > 1 && hipMalloc((void **)&fd, S * sizeof(IcwFirConv)) != hipSuccess) rc |= ICW_ENOMEM;
        if (rc != ICW_OK) return drop(rc == ICW_ENOMEM ? ICW_ENOMEM : ICW_EDEVICE);
        bool ok = hipMemcpy(fg, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
        const double *old = c->fir_hist[c->fir_par];
        if (old && c->fir_M > 0) {
            const std::vector<size_t> &oo = c->fir_off;
            if (oo[f]) ok = ok && hipMemcpy(h0, old, oo[f] * sizeof(double), hipMemcpyDeviceToDevice) == hipSuccess;
            if (oo[S] > oo[e])
                ok = ok && hipMemcpy(h0 + off[e], old + oo[e], (oo[S] - oo[e]) * sizeof(double), hipMemcpyDeviceToDevice) == hipSuccess;
        }
        if (n > 1) {
            std::vector<IcwFirConv> h(S);
            for (size_t s = 0; s < S; ++s) {
                const FirEnt &x = t.at(s);
                h[s].M = x.M;
                h[s].nt = x.nt;
                h[s].g = fg + x.goff;
                h[s].hoff = off[s];
            }
            ok = ok && hipMemcpy(fd, h.data(), S * sizeof(IcwFirConv), hipMemcpyHostToDevice) == hipSuccess;
        }
        /* the fills and copies above ran on the null stream: all of them done before a call on the context's
         * or the caller's stream may read the fresh buffers */
        ok = ok && hipDeviceSynchronize() == hipSuccess;
        if (!ok) return drop(ICW_EDEVICE);
    }
    for (void *p : {(void *)c->d_fir_g, (void *)c->fir_hist[0], (void *)c->fir_hist[1], (void *)c->d_fconv})
        if (p) (void)hipFree(p);
    c->d_fir_g = fg;
    c->fir_hist[0] = h0;
    c->fir_hist[1] = h1;
    c->d_fconv = fd;
    if (pid) c->d_pid = pid;
    c->fir_par = 0;
    c->fir_off = std::move(off);
    c->fir_Mmax = mmax;
    c->firs = std::move(t);
    c->fir_M = c->firs.ents[0].M;
    c->fir_nt = c->firs.ents[0].nt;
    c->fir_beta = on ? c->firs.ents[0].beta : 0.0;
    c->pid_valid = false;                 /* with the converter on, every (list, rate) pair has a slab */
    return ICW_OK;
}

/* icw_set_fir_hilbert (every stream) and icw_set_stream_fir (a range): the refusals both share, the candidate
 * table, the install */
int set_fir_range(icw_ctx *c, int first, int count, int32_t M, double beta)
{
    /* beside per-stream lists or inputs only once the host has asked for it (icw_enable_stream_fir): the
     * converter's kernels then run their per-stream form */
    if (M > 0 && !c->fir_streams && (c->lists.size() > 1 || c->inputs.size() > 1)) return ICW_EUNSUPPORTED;
    /* nor beside per-stream CWAVE inputs (icw_enable_stream_cwave): the converter's per-stream kernels read
     * real formats only, and icw_set_stream_input refuses to build that state from its side */
    if (M > 0 && c->inputs.size() > 1 && any_cwave(c->inputs)) return ICW_EUNSUPPORTED;
    /* nor beside per-stream renders (icw_set_stream_render): the fused converter renders with one */
    if (M > 0 && c->renders.size() > 1) return ICW_EUNSUPPORTED;
    /* nor beside per-stream Hilbert converters (icw_set_stream_hilbert): it replaces the IIR for every stream */
    if (M > 0 && c->hilbs.size() > 1) return ICW_EUNSUPPORTED;
    /* nor beside bus-form lists that stand beside others (icw_enable_stream_bus): the mixed K4 follows K2 */
    if (M > 0 && c->bus_lists) return ICW_EUNSUPPORTED;
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    FirEnt x;
    x.M = M;
    x.beta = M > 0 ? beta : 0.0;
    StreamTable<FirEnt> t = c->firs.assigned((size_t)first, (size_t)count, x, same_fir);
    return install_firs(c, t, first, count);
}

}  // namespace

extern "C" {

const char *icw_version(void) { return "in_cwave_amd 0.1 (gfx950)"; }

int icw_abi_version(void) { return ICW_ABI_VERSION; }

const char *icw_strerror(int s)
{
    switch (s) {
    case ICW_OK: return "ok";
    case ICW_EINVAL: return "invalid argument";
    case ICW_ENOMEM: return "out of memory";
    case ICW_EDEVICE: return "HIP device error";
    case ICW_EGRAPH: return "DSP list rejected";
    case ICW_EUNSUPPORTED: return "configuration not supported on the device path";
    }
    return "unknown";
}

int icw_create(const icw_config *cfg, const icw_node *nodes, int n_nodes, int n_streams, int device,
               icw_ctx **out, int *accepted)
{
    if (!cfg || !out || n_streams <= 0 || n_nodes < 0 || (n_nodes > 0 && !nodes)) return ICW_EINVAL;
    *out = nullptr;
    if (cfg->hilbert_type > 5 || cfg->in_format > ICW_FMT_CW_F32 || cfg->in_channels == 0 ||
        cfg->sample_rate == 0 || cfg->sample_rate > ICW_MAX_FS_SRC)
        return ICW_EINVAL;
    if (!render_cfg_ok(cfg->render)) return ICW_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ICW_EDEVICE;
    icw_ctx *c = new (std::nothrow) icw_ctx();
    if (!c) return ICW_ENOMEM;
    c->cfg = *cfg;
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) { delete c; return ICW_EDEVICE; }
    }
    c->device = device;
    if (set_dev(c)) { delete c; return ICW_EDEVICE; }
    ListEnt L;
    L.nodes.assign(nodes, nodes + n_nodes);
    const bool ok = graph_accept(L.nodes);
    if (!ok) L.nodes.assign(1, default_master());
    if (accepted) *accepted = ok ? 1 : 0;
    c->tn = icw_read_tuning();
    int rc = build_prog(*cfg, L.nodes, L.prog);
    if (rc) { delete c; return rc; }
    if (!c->tn.chain_ok) L.prog.chain = L.prog.sig = 0;
    /* the four tables, one entry each, and their mirrors (the render's entry is made behind the list's) */
    c->n_streams = n_streams;
    c->lists.reset((size_t)n_streams, L);
    mirror_lists(c);
    c->inputs.reset((size_t)n_streams, make_input(cfg->sample_rate, cfg->in_format, cfg->in_channels));
    c->hilbs.reset((size_t)n_streams, make_hilb(cfg->hilbert_type, cfg->iir_kahan, cfg->iir_subnorm_reject));
    mirror_hilbs(c);
    c->firs.reset((size_t)n_streams, FirEnt{});
    c->fir_off.assign((size_t)n_streams + 1, 0);
    c->renders.reset((size_t)n_streams, make_render(c, cfg->render, cfg->need24bits));
    mirror_renders(c);
    for (int ch = 0; ch < 2; ++ch) {
        uint32_t *st = c->mt_seed_state[ch];
        st[0] = ch ? cfg->seed_right : cfg->seed_left;         /* mtrnd_init_seed, mt_jrnd.c:28-47 */
        for (uint32_t j = 1; j < 624; ++j) st[j] = 1812433253u * (st[j - 1] ^ (st[j - 1] >> 30)) + j;
    }
    const size_t S = (size_t)n_streams, C = S * 4;
    rc = ICW_OK;
    DevState &s = c->st;
    rc |= dalloc(&s.hist, C * ICW_HIST_PITCH);
    rc |= dalloc(&s.sncnt, C);
    rc |= dalloc(&s.hq_phase, S * 2);
    rc |= dalloc(&s.pos, S);
    rc |= dalloc(&s.fade, S * 3);
    rc |= dalloc(&s.n_frame, S);
    rc |= dalloc(&s.bus, S * ICW_N_INPUTS * 4);
    rc |= dalloc(&s.clips, S * 2);
    rc |= dalloc(&s.peak_bits, S * 2);
    rc |= dalloc(&s.err, 1);
    if (c->render_state) {
        rc |= dalloc(&s.mt, (size_t)624 * S * 2);
        rc |= dalloc(&s.mt_idx, S * 2);
        rc |= dalloc(&s.rs, S * 2 * ICW_RSTATE);
    }
    rc |= dalloc(&s.lr_equal, S * 2);
    if (cfg->fp_check) rc |= dalloc(&s.fes, S * 4 * ICW_FES_PITCH);
    for (int p = 0; p < kSets; ++p) rc |= dalloc(&c->info_dup[p], S * 2);
    rc |= dalloc(&c->d_prog, 1);
    if (rc == ICW_OK && hipMemcpy(c->d_prog, &c->prog, sizeof(IcwProg), hipMemcpyHostToDevice) != hipSuccess)
        rc = ICW_EDEVICE;
    if (rc == ICW_OK && hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) rc = ICW_EDEVICE;
    if (rc == ICW_OK && hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess) rc = ICW_EDEVICE;
    if (rc == ICW_OK && hipStreamCreateWithFlags(&c->stream3, hipStreamNonBlocking) != hipSuccess) rc = ICW_EDEVICE;
    if (rc == ICW_OK && hipStreamCreateWithFlags(&c->stream4, hipStreamNonBlocking) != hipSuccess) rc = ICW_EDEVICE;
    if (rc == ICW_OK && hipStreamCreateWithFlags(&c->stream_io, hipStreamNonBlocking) != hipSuccess) rc = ICW_EDEVICE;
    for (int p = 0; p < kSets && rc == ICW_OK; ++p)
        if (hipEventCreateWithFlags(&c->k1done[p], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->k2done[p], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ditdone[p], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->k0done[p], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->k3done[p], hipEventDisableTiming) != hipSuccess)
            rc = ICW_EDEVICE;
    if (rc == ICW_OK && hipEventCreateWithFlags(&c->join, hipEventDisableTiming) != hipSuccess) rc = ICW_EDEVICE;
    if (rc != ICW_OK) {
        free_all(c);
        delete c;
        return rc < 0 ? (rc == ICW_ENOMEM ? ICW_ENOMEM : ICW_EDEVICE) : ICW_EDEVICE;
    }
    c->peak_db.assign(S * 2, ICW_SR_ZERO_SIGNAL_DB);
    c->lr_known.assign(S, 1);
    c->nf_host.assign(S, 0ull);
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, c->device) == hipSuccess) c->n_cu = prop.multiProcessorCount;
    }
    if (c->tn.s1_stamps && dalloc(&c->s1_stamps, 8) != ICW_OK) c->s1_stamps = nullptr;
    rc = icw_stream_init(c, 0, n_streams);
    if (rc) { free_all(c); delete c; return rc; }
    split_ref(c->device, +1);
    *out = c;
    return ICW_OK;
}

int icw_destroy(icw_ctx *c)
{
    if (!c) return ICW_EINVAL;
    set_dev(c);
    (void)quiesce(c);
    free_all(c);
    split_ref(c->device, -1);
    delete c;
    return ICW_OK;
}

int icw_stream_init(icw_ctx *c, int first, int count)
{
    if (!c || first < 0 || count < 0 || first + count > c->n_streams) return ICW_EINVAL;
    if (count == 0) return ICW_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c)) return ICW_EDEVICE;
    DevState &s = c->st;
    const size_t f = (size_t)first, n = (size_t)count;
    hipStream_t st = c->stream;
    /* a stream that has run (a pool slot between two files, icw_transcode_files_pool): its kernels are on
     * several streams, the caller's among them, and none of them may still write the state reset here */
    bool ok = quiesce(c) == hipSuccess;
    ok &= reset_rings(c, f, n, st);
    /* the encoders' saturation counts (icw_encode_clipped), where a call has made them */
    if (c->enc_clipped) ok &= hipMemsetAsync(c->enc_clipped + f, 0, n * sizeof(unsigned long long), st) == hipSuccess;
    ok &= hipMemsetAsync(s.pos + f, 0, n * sizeof(long long), st) == hipSuccess;
    ok &= hipMemsetAsync(s.n_frame + f, 0, n * sizeof(unsigned long long), st) == hipSuccess;
    for (size_t i = 0; i < n; ++i) c->nf_host[f + i] = 0;
    ok &= hipMemsetAsync(s.bus + f * ICW_N_INPUTS * 4, 0, n * ICW_N_INPUTS * 4 * sizeof(double), st) == hipSuccess;
    ok &= hipMemsetAsync(s.clips + f * 2, 0, n * 2 * sizeof(uint32_t), st) == hipSuccess;
    ok &= hipMemsetAsync(s.peak_bits + f * 2, 0, n * 2 * sizeof(unsigned long long), st) == hipSuccess;
    if (s.fes) ok &= hipMemsetAsync(s.fes + f * 4 * ICW_FES_PITCH, 0, n * 4 * ICW_FES_PITCH * 4, st) == hipSuccess;
    ok &= fir_clear(c, f, n, st);
    /* no track open: n_samples "infinite", no fades (xwave_unpack_csample never fades) */
    std::vector<long long> fd(n * 3);
    for (size_t i = 0; i < n; ++i) { fd[i * 3] = (long long)1 << 62; fd[i * 3 + 1] = 0; fd[i * 3 + 2] = 0; }
    ok &= hipMemcpyAsync(s.fade + f * 3, fd.data(), fd.size() * sizeof(long long), hipMemcpyHostToDevice, st) == hipSuccess;
    /* renders re-seeded (mod_context_init -> sound_render_init, in_cwave.c:69-70) wherever their
     * state exists (a context whose renders never needed it has none yet, ensure_render_state) */
    if (s.mt) ok &= seed_renders(c, f, n, st);
    ok &= hipStreamSynchronize(st) == hipSuccess;
    for (size_t i = f * 2; i < (f + n) * 2; ++i) c->peak_db[i] = ICW_SR_ZERO_SIGNAL_DB;
    return ok ? ICW_OK : ICW_EDEVICE;
}

int icw_stream_open(icw_ctx *c, int s, int64_t n_samples, uint32_t fade_in, uint32_t fade_out,
                    uint32_t sec_align, int clr_nframe, int clr_hilb)
{
    if (!c || s < 0 || s >= c->n_streams || n_samples < 0) return ICW_EINVAL;
    (void)sec_align;   /* the virtual zero tail is produced by the reader (xwave_read_samples) */
    std::lock_guard<std::mutex> lk(c->mu);
    /* the fades at the stream's own rate (icw_set_stream_input; the context's while the inputs are one) */
    const uint64_t rate = c->inputs.at((size_t)s).sample_rate;
    long long nfi = (long long)(((uint64_t)fade_in * rate) / 1000ULL);
    long long nfo = (long long)(((uint64_t)fade_out * rate) / 1000ULL);
    if (nfi + nfo >= n_samples) {
        if (n_samples < 300LL) nfi = nfo = 0;
        else {
            if (nfi) nfi = n_samples / 3;
            if (nfo) nfo = n_samples / 3;
        }
    }
    if (set_dev(c)) return ICW_EDEVICE;
    long long fd[3] = {(long long)n_samples, nfi, nfo};
    c->touched = true;
    bool ok = quiesce(c) == hipSuccess;
    ok &= hipMemcpy(c->st.fade + (size_t)s * 3, fd, sizeof(fd), hipMemcpyHostToDevice) == hipSuccess;
    ok &= hipMemset(c->st.pos + s, 0, sizeof(long long)) == hipSuccess;
    if (clr_nframe) {
        ok &= hipMemset(c->st.n_frame + s, 0, sizeof(unsigned long long)) == hipSuccess;
        c->nf_host[s] = 0;
    }
    if (clr_hilb)
        ok &= reset_rings(c, (size_t)s, 1, c->stream) && fir_clear(c, (size_t)s, 1, c->stream) &&
              hipStreamSynchronize(c->stream) == hipSuccess;
    /* sound_render_set_outbits -> sound_render_recalc */
    ok &= restart_shaping(c, (size_t)s, 1);
    return ok ? ICW_OK : ICW_EDEVICE;
}

int icw_stream_reset_hilbert(icw_ctx *c, int s)
{
    if (!c || s < 0 || s >= c->n_streams) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c)) return ICW_EDEVICE;
    c->touched = true;
    bool ok = quiesce(c) == hipSuccess;
    ok &= reset_rings(c, (size_t)s, 1, c->stream) && fir_clear(c, (size_t)s, 1, c->stream) &&
          hipStreamSynchronize(c->stream) == hipSuccess;
    return ok ? ICW_OK : ICW_EDEVICE;
}

int icw_fir_taps(int32_t M, double beta, double *g, int n)
{
    if (M < 2 || M > ICW_FIR_MAX_ORDER || (M & 1) || !(beta >= 0.0 && beta < 1e3) || !g) return ICW_EINVAL;
    const int c = M / 2, nt = (c + 1) / 2;
    if (n < nt) return ICW_EINVAL;
    const double i0b = bessel_i0(beta);
    for (int k = 0; k < nt; ++k) {
        const int m = 2 * k + 1;
        const double r = (double)m / (double)c;
        const double w = bessel_i0(beta * sqrt(1.0 - r * r)) / i0b;
        g[k] = (2.0 / (ICW_PI_H * (double)m)) * w;
    }
    return nt;
}

int icw_set_fir_hilbert(icw_ctx *c, int32_t M, double beta)
{
    static_assert(ICW_FIR_MAX_ORDER == ICW_FIR_MAX_M, "FIR order limit of the header and the kernel");
    if (!c || (M != 0 && (M < 2 || M > ICW_FIR_MAX_ORDER || (M & 1))) || !(beta >= 0.0 && beta < 1e3))
        return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    /* every stream: a context whose converters differed is a one-converter context again */
    return set_fir_range(c, 0, c->n_streams, M, beta);
}

/* icw_set_fir_hilbert for streams [first, first + count) (include/icw.h) */
int icw_set_stream_fir(icw_ctx *c, int first, int count, int32_t M, double beta)
{
    if (!c || first < 0 || count <= 0 || first > c->n_streams - count || M < 0 || M > ICW_FIR_MAX_ORDER || (M & 1) ||
        !(beta >= 0.0 && beta < 1e3))
        return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    /* the per-stream kernel instances serve it: asked for like per-stream lists and inputs beside the converter */
    if (!c->fir_streams || c->cfg.fp_check) return ICW_EUNSUPPORTED;
    /* all FIR or none: whether K1 runs is the call's decision, so a range goes neither off beside streams that
     * stay on nor on beside streams that stay off */
    const bool whole = first == 0 && count == c->n_streams;
    if (!whole && (M == 0 || c->fir_M == 0)) return ICW_EUNSUPPORTED;
    return set_fir_range(c, first, count, M, beta);
}

int icw_stream_fir_count(const icw_ctx *c)
{
    if (!c) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(const_cast<icw_ctx *>(c)->mu);
    return (int)c->firs.size();
}

/* per-stream lists and inputs beside the FIR converter, on or off (include/icw.h) */
int icw_enable_stream_fir(icw_ctx *c, int on)
{
    if (!c) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    /* off while the two are in force together would leave a state the setters refuse to build */
    if (!on && c->fir_M > 0 && (c->lists.size() > 1 || c->inputs.size() > 1)) return ICW_EUNSUPPORTED;
    if (!on && c->firs.size() > 1) return ICW_EUNSUPPORTED;
    c->fir_streams = on != 0;
    return ICW_OK;
}

/* bus-form lists beside other lists, on or off (include/icw.h) */
int icw_enable_stream_bus(icw_ctx *c, int on)
{
    if (!c) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    /* off while a bus-form entry stands beside others would leave a table the setters refuse to build */
    if (!on && c->bus_lists) return ICW_EUNSUPPORTED;
    c->bus_streams = on != 0;
    return ICW_OK;
}

/* per-stream inputs through the CWAVE encoders, on or off (include/icw.h).  Off again is the fresh
 * context's state whatever the inputs are -- the encoders then refuse while they differ -- so there is
 * nothing it could leave half built */
int icw_enable_stream_encode(icw_ctx *c, int on)
{
    if (!c) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->enc_streams = on != 0;
    return ICW_OK;
}

/* per-stream CWAVE inputs, on or off (include/icw.h).  Off while a stream holds a per-stream CWAVE input
 * would leave a table the setter refuses to build */
int icw_enable_stream_cwave(icw_ctx *c, int on)
{
    if (!c) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!on && c->inputs.size() > 1 && any_cwave(c->inputs)) return ICW_EUNSUPPORTED;
    c->cw_streams = on != 0;
    return ICW_OK;
}

int icw_stream_reset_framecnt(icw_ctx *c, int s)
{
    if (!c || s < 0 || s >= c->n_streams) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c)) return ICW_EDEVICE;
    if (quiesce(c) != hipSuccess) return ICW_EDEVICE;
    c->touched = true;
    c->nf_host[s] = 0;
    return hipMemset(c->st.n_frame + s, 0, sizeof(unsigned long long)) == hipSuccess ? ICW_OK : ICW_EDEVICE;
}

int icw_stream_seek(icw_ctx *c, int s, int64_t frame_pos)
{
    if (!c || s < 0 || s >= c->n_streams || frame_pos < 0) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c)) return ICW_EDEVICE;
    long long v = (long long)frame_pos;
    c->touched = true;
    bool ok = quiesce(c) == hipSuccess;
    ok &= hipMemcpy(c->st.pos + s, &v, sizeof(v), hipMemcpyHostToDevice) == hipSuccess;
    return ok ? ICW_OK : ICW_EDEVICE;
}

int icw_set_input(icw_ctx *c, uint32_t sample_rate, uint32_t fmt, uint32_t channels)
{
    if (!c || sample_rate == 0 || sample_rate > ICW_MAX_FS_SRC || fmt > ICW_FMT_CW_F32 || channels == 0) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    /* every stream: a context whose streams differed is a one-input context again */
    StreamTable<IcwInDesc> t;
    t.reset((size_t)c->n_streams, make_input(sample_rate, fmt, channels));
    return install_inputs(c, t);
}

/* icw_set_input for streams [first, first + count) (include/icw.h) */
int icw_set_stream_input(icw_ctx *c, int first, int count, uint32_t sample_rate, uint32_t fmt, uint32_t channels)
{
    if (!c || first < 0 || count <= 0 || first > c->n_streams - count || sample_rate == 0 ||
        sample_rate > ICW_MAX_FS_SRC || fmt > ICW_FMT_CW_F32 || channels == 0)
        return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    /* whether K1 runs at all is a per-call decision: CWAVE input stays context-wide until
     * icw_enable_stream_cwave said otherwise (a call then covers streams of one kind).  The FIR converter is
     * context-wide too; it reads every stream's own real format once icw_enable_stream_fir said so, and never
     * stands beside per-stream CWAVE inputs */
    const bool cwf = fmt >= ICW_FMT_CW_F64;
    if (!c->cw_streams && (cwf || c->cfg.in_format >= ICW_FMT_CW_F64)) return ICW_EUNSUPPORTED;
    if (c->fir_M > 0 && (!c->fir_streams || cwf)) return ICW_EUNSUPPORTED;
    StreamTable<IcwInDesc> t = c->inputs.assigned((size_t)first, (size_t)count, make_input(sample_rate, fmt, channels), same_input);
    if (c->fir_M > 0 && t.size() > 1 && any_cwave(t)) return ICW_EUNSUPPORTED;
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    return install_inputs(c, t);
}

int icw_stream_input_count(const icw_ctx *c)
{
    if (!c) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(const_cast<icw_ctx *>(c)->mu);
    return (int)c->inputs.size();
}

/* Live edits: what the reference's GUI thread changes while a decode thread runs
 * applies here from the next call on, to every stream of the context; the running call finishes
 * with the old parameters (quiesce).  Per-stream state carries over as in the reference. */
int icw_set_graph(icw_ctx *c, const icw_node *nodes, int n_nodes, int bypass_list, int *accepted)
{
    if (!c || n_nodes < 0 || (n_nodes > 0 && !nodes)) return ICW_EINVAL;
    std::vector<icw_node> nv(nodes, nodes + n_nodes);
    const bool ok = graph_accept(nv);
    if (accepted) *accepted = ok ? 1 : 0;
    if (!ok) return ICW_EGRAPH;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    /* every stream's list is replaced (a table of several collapses to this list), each stream's clears
     * matched against its own old list */
    return apply_graph(c, nv, bypass_list ? 1 : 0, matched_clears_per_entry(c, nv));
}

/* icw_set_graph for streams [first, first + count) (include/icw.h) */
int icw_set_stream_graph(icw_ctx *c, int first, int count, const icw_node *nodes, int n_nodes, int bypass_list,
                         int *accepted)
{
    if (!c || first < 0 || count <= 0 || first > c->n_streams - count || n_nodes < 0 || (n_nodes > 0 && !nodes))
        return ICW_EINVAL;
    std::vector<icw_node> nv(nodes, nodes + n_nodes);
    const bool ok = graph_accept(nv);
    if (accepted) *accepted = ok ? 1 : 0;
    if (!ok) return ICW_EGRAPH;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    /* K4 runs one lane per stream on a scalar program: bus-form lists stay context-wide until
     * icw_enable_stream_bus said otherwise (the mixed K4 then runs a wave per run of one list); the FIR
     * converter serves per-stream lists once icw_enable_stream_fir said so */
    if ((c->fir_M > 0 && !c->fir_streams) || (c->prog.is_bus && !c->bus_streams)) return ICW_EUNSUPPORTED;
    ListEnt L;
    int rc = compile_list(c, nv, bypass_list ? 1 : 0, L);
    if (rc) return rc;
    if (L.prog.is_bus && !c->bus_streams) return ICW_EUNSUPPORTED;
    const std::vector<std::vector<int>> per = matched_clears_per_entry(c, nv);
    const std::vector<int32_t> old_of = c->lists.of;
    StreamTable<ListEnt> t = c->lists.assigned((size_t)first, (size_t)count, L, same_list);
    bool any_bus = false;
    for (const ListEnt &e : t.ents) any_bus = any_bus || e.prog.is_bus;
    /* a bus-form list runs one K2 instance into one serial render, as behind icw_set_graph; beside other
     * lists it stands neither beside the FIR converter nor in an FP_CHECK context (include/icw.h) */
    if (any_bus && (c->renders.size() > 1 || c->hilbs.size() > 1)) return ICW_EUNSUPPORTED;
    if (any_bus && t.size() > 1 && (c->fir_M > 0 || c->cfg.fp_check)) return ICW_EUNSUPPORTED;
    if (any_bus && (rc = ensure_render_state(c)) != ICW_OK) return rc;
    if ((rc = install_lists(c, t)) != ICW_OK) return rc;
    /* the one render follows the lists, as behind icw_set_graph: serial behind one bus-form list, its own
     * beside several (make_render) */
    if (c->bus_streams && c->renders.size() == 1) {
        const RenderEnt r0 = c->renders.ents[0];
        c->renders.ents[0] = make_render(c, r0.cfg, r0.is24);
        mirror_renders(c);
    }
    return clear_matched(c, old_of, first, count, per);
}

int icw_clear_stream_bus_slot(icw_ctx *c, int first, int count, int slot)
{
    if (!c || first < 0 || count <= 0 || first > c->n_streams - count || slot < 0 || slot >= ICW_N_INPUTS)
        return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    return clear_slot_range(c, first, count, slot);
}

/* host only: the form a list compiles to (include/icw.h) */
int icw_graph_form(const icw_config *cfg, const icw_node *nodes, int n_nodes, int bypass_list)
{
    if (!cfg || n_nodes < 0 || (n_nodes > 0 && !nodes)) return ICW_EINVAL;
    std::vector<icw_node> nv(nodes, nodes + n_nodes);
    if (!graph_accept(nv)) return ICW_EGRAPH;
    icw_config c2 = *cfg;
    c2.bypass_list = bypass_list ? 1 : 0;
    std::unique_ptr<IcwProg> P(new IcwProg);
    const int rc = build_prog(c2, nv, *P);
    if (rc) return rc;
    return P->is_bus ? 1 : 0;
}

int icw_stream_graph_count(const icw_ctx *c)
{
    if (!c) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(const_cast<icw_ctx *>(c)->mu);
    return (int)c->lists.size();
}

/* the list primitives (include/icw.h): the reference's own edits, each with replace_output_plug's
 * clear (adv_modulator.c:176-209) and nothing else */
int icw_graph_del_last(icw_ctx *c)
{
    if (!c) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->lists.size() > 1) return ICW_EUNSUPPORTED;               /* no one list to edit (include/icw.h) */
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    if (c->nodes.size() <= 1) return ICW_OK;                        /* am.tail->prev == NULL */
    std::vector<icw_node> nv(c->nodes.begin(), c->nodes.end() - 1);
    std::vector<int> clears;
    const int r = plug_slot(c->nodes.back());
    if (r >= 0) clears.push_back(r);
    return apply_graph(c, nv, c->cfg.bypass_list, {clears});
}

int icw_graph_del_all(icw_ctx *c)
{
    if (!c) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->lists.size() > 1) return ICW_EUNSUPPORTED;
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    if (c->nodes.size() <= 1) return ICW_OK;
    std::vector<int> clears;
    for (size_t i = c->nodes.size() - 1; i >= 1; --i) {             /* tail first (adv_modulator.c:364-371) */
        const int r = plug_slot(c->nodes[i]);
        if (r >= 0) clears.push_back(r);
    }
    std::vector<icw_node> nv(c->nodes.begin(), c->nodes.begin() + 1);
    return apply_graph(c, nv, c->cfg.bypass_list, {clears});
}

int icw_graph_add_last(icw_ctx *c, const icw_node *node)
{
    if (!c || !node) return ICW_EINVAL;
    if (node->mode == ICW_MODE_MASTER) return ICW_EGRAPH;           /* create_node_dsp: NULL */
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->lists.size() > 1) return ICW_EUNSUPPORTED;
    std::vector<icw_node> nv(c->nodes);
    nv.push_back(*node);
    if (!graph_accept(nv)) return ICW_EGRAPH;
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    return apply_graph(c, nv, c->cfg.bypass_list, {{}});
}

int icw_graph_set_output_plug(icw_ctx *c, int index, int n)
{
    if (!c || n < -1 || n >= ICW_N_INPUTS || n == 0) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->lists.size() > 1) return ICW_EUNSUPPORTED;
    if (index < 0 || index >= (int)c->nodes.size()) return ICW_EINVAL;
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    std::vector<icw_node> nv(c->nodes);
    std::vector<int> clears;
    const int r = plug_slot(nv[index]);
    if (r >= 0) {
        clears.push_back(r);
        if (n >= 0) nv[index].n_out = n;
    }
    return apply_graph(c, nv, c->cfg.bypass_list, {clears});
}

int icw_clear_bus_slot(icw_ctx *c, int slot)
{
    if (!c || slot < 0 || slot >= ICW_N_INPUTS) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    return clear_slot_range(c, 0, c->n_streams, slot);
}

/* srenders_set_vcfg: every stream gets the setting at its own depth (a table of several collapses to as many
 * entries as depths in force), and every stream's shaping state restarts */
int icw_set_render(icw_ctx *c, const icw_render_cfg *r)
{
    if (!c || !r || !render_cfg_ok(*r)) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    StreamTable<RenderEnt> t = c->renders.mapped([&](const RenderEnt &e) { return make_render(c, *r, e.is24); }, same_render);
    return install_renders(c, t, 0, c->n_streams);
}

/* sound_render_set_outbits (sound_render.c:617-621) on both renders of every stream, as
 * mod_context_fopen applies the.cfg.need24bits at every track open (in_cwave.c:212, 233-234): the
 * new bounds, norm_mul and norm_shift, then sound_render_recalc (prev_rnd, the shaper rings and
 * prev_ns_err restart; the MT19937 generators go on).  Applied even when the depth is unchanged,
 * since recalc runs either way.  Every stream keeps its own setting. */
int icw_set_outbits(icw_ctx *c, int need24bits)
{
    if (!c) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    StreamTable<RenderEnt> t = c->renders.mapped([&](const RenderEnt &e) { return make_render(c, e.cfg, need24bits); }, same_render);
    return install_renders(c, t, 0, c->n_streams);
}

/* icw_set_render followed by icw_set_outbits for streams [first, first + count) (include/icw.h) */
int icw_set_stream_render(icw_ctx *c, int first, int count, const icw_render_cfg *r, int need24bits)
{
    if (!c || first < 0 || count <= 0 || first > c->n_streams - count || !r || !render_cfg_ok(*r)) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    StreamTable<RenderEnt> t = c->renders.assigned((size_t)first, (size_t)count, make_render(c, *r, need24bits), same_render);
    return install_renders(c, t, first, count);
}

int icw_stream_render_count(const icw_ctx *c)
{
    if (!c) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(const_cast<icw_ctx *>(c)->mu);
    return (int)c->renders.size();
}

int icw_stream_render_size(const icw_ctx *c, int s)
{
    if (!c || s < 0 || s >= c->n_streams) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(const_cast<icw_ctx *>(c)->mu);
    return c->renders.at((size_t)s).is24 ? 3 : 2;
}

/* the largest sample size in force, so that a buffer sized by it holds every stream's frames */
int icw_render_size(const icw_ctx *c)
{
    if (!c) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(const_cast<icw_ctx *>(c)->mu);
    int is24 = 0;
    for (const RenderEnt &e : c->renders.ents) is24 |= e.is24;
    return is24 ? 3 : 2;
}

/* mod_context_change_all_hilberts_filter: every stream gets the type and keeps its summation (a table of
 * several collapses to as many entries as summations in force).  Only the streams whose type changes restart
 * (hq_rp_create), and no de-subnorm counter restarts otherwise */
int icw_set_hilbert_filter(icw_ctx *c, uint32_t type)
{
    if (!c || type > 5) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    /* the one type in force again: nothing to do, and the device is neither touched nor waited for */
    if (c->hilbs.size() == 1 && c->hilbs.ents[0].type == type) return ICW_OK;
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    StreamTable<HilbEnt> t = c->hilbs.mapped([&](const HilbEnt &e) { return make_hilb(type, e.kahan, e.subn); }, same_hilb);
    return install_hilberts(c, t, 0, 0);
}

/* mod_context_change_all_hilberts_config -> iir_rp_setcfg: every stream gets the summation and keeps its type
 * and its rings; the de-subnorm counters of every stream start again */
int icw_set_hilbert_config(icw_ctx *c, int kahan, int subnorm_reject)
{
    if (!c) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    StreamTable<HilbEnt> t = c->hilbs.mapped([&](const HilbEnt &e) { return make_hilb(e.type, kahan, subnorm_reject); }, same_hilb);
    return install_hilberts(c, t, 0, c->n_streams);
}

/* icw_set_hilbert_filter followed by icw_set_hilbert_config for streams [first, first + count) (include/icw.h) */
int icw_set_stream_hilbert(icw_ctx *c, int first, int count, uint32_t type, int kahan, int subnorm_reject)
{
    if (!c || first < 0 || count <= 0 || first > c->n_streams - count || type > 5) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    StreamTable<HilbEnt> t = c->hilbs.assigned((size_t)first, (size_t)count, make_hilb(type, kahan, subnorm_reject), same_hilb);
    return install_hilberts(c, t, first, count);
}

int icw_stream_hilbert_count(const icw_ctx *c)
{
    if (!c) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(const_cast<icw_ctx *>(c)->mu);
    return (int)c->hilbs.size();
}

int icw_host_alloc(size_t bytes, void **p)
{
    if (!p || !bytes) return ICW_EINVAL;
    *p = nullptr;
    /* portable: pinned for every device, so an icw_group's shards on other devices pipeline their
     * slices of the same buffer too (host_pinned) */
    return hipHostMalloc(p, bytes, hipHostMallocPortable) == hipSuccess ? ICW_OK : ICW_ENOMEM;
}

int icw_host_free(void *p)
{
    return (!p || hipHostFree(p) == hipSuccess) ? ICW_OK : ICW_EINVAL;
}

int icw_host_pinned(const void *p, int device)
{
    return p && host_pinned(p, device) ? 1 : 0;
}

int icw_synchronize(icw_ctx *c)
{
    if (!c) return ICW_EINVAL;
    if (set_dev(c)) return ICW_EDEVICE;
    if (quiesce(c) != hipSuccess) return ICW_EDEVICE;
    int e = 0;
    if (hipMemcpy(&e, c->st.err, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess || e) return ICW_EDEVICE;
    return ICW_OK;
}

/* amod_get_clips_peaks (adv_modulator.c:445-465): with isReset the clip counters and peaks are
 * cleared FIRST and the cleared values (0, SR_ZERO_SIGNAL_DB) are returned; the de-subnorm count
 * (mod_context_get_desubnorm_counter, in_cwave.c:300-310) is not reset by it.  The meters are
 * written by kernels that may still run (ICW_F_DEVICE_PTRS calls return early, on several
 * streams), so the read waits for the context's work first, as get_state does. */
int icw_get_meters(icw_ctx *c, int s, int reset, icw_meters *m)
{
    if (!c || !m || s < 0 || s >= c->n_streams) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    uint32_t cl[2];
    unsigned long long pb[2], sn[4];
    bool ok = true;
    if (reset) {
        ok &= hipMemset(c->st.clips + (size_t)s * 2, 0, sizeof(cl)) == hipSuccess;
        ok &= hipMemset(c->st.peak_bits + (size_t)s * 2, 0, sizeof(pb)) == hipSuccess;
        c->peak_db[(size_t)s * 2] = c->peak_db[(size_t)s * 2 + 1] = ICW_SR_ZERO_SIGNAL_DB;
    }
    ok &= hipMemcpy(cl, c->st.clips + (size_t)s * 2, sizeof(cl), hipMemcpyDeviceToHost) == hipSuccess;
    ok &= hipMemcpy(pb, c->st.peak_bits + (size_t)s * 2, sizeof(pb), hipMemcpyDeviceToHost) == hipSuccess;
    ok &= hipMemcpy(sn, c->st.sncnt + (size_t)s * 4, sizeof(sn), hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) return ICW_EDEVICE;
    for (int ch = 0; ch < 2; ++ch) {
        /* peak meter (sound_render.c:769-780): max over samples of 20*log10(|q|/hi) equals
         * 20*log10(max|q| / hi) because the map is monotone; 0 -> SR_ZERO_SIGNAL_DB */
        double mx;
        memcpy(&mx, &pb[ch], 8);
        double cv = mx / c->renders.at((size_t)s).rk.hi;     /* the stream's own bound */
        cv = cv ? 20.0 * log10(cv) : ICW_SR_ZERO_SIGNAL_DB;
        double &pv = c->peak_db[(size_t)s * 2 + ch];
        if (cv > pv) pv = cv;
        m->clips[ch] = cl[ch];
        m->peak_db[ch] = pv;
    }
    m->desubnorm = sn[0] + sn[1] + sn[2] + sn[3];
    return ICW_OK;
}

int icw_n_frame(icw_ctx *c, int s, uint64_t *nf)
{
    if (!c || !nf || s < 0 || s >= c->n_streams) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    unsigned long long v = 0;
    if (hipMemcpy(&v, c->st.n_frame + s, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return ICW_EDEVICE;
    *nf = v;
    /* the host mirror decides whether the fused FIR kernel may take every Shift / PM factor from the
     * shared table (in_step): a device-side write it did not follow would give the stream another
     * stream's rotation, so a divergence fails this read loudly */
    if (c->nf_host[s] != v) {
        fprintf(stderr, "icw_n_frame: stream %d frame counter %llu, host mirror %llu\n", s, v, c->nf_host[s]);
        return ICW_EDEVICE;
    }
    return ICW_OK;
}

/* canonical state blob: see DESIGN.md "Per-stream state" */
struct IcwBlob {
    uint64_t magic, n_frame;
    int64_t pos, n_samples, n_fade_in, n_fade_out;
    uint32_t hq_phase[2], nord, has_render;
    uint32_t fir_M, reserved;         /* FIR converter order in force (0: the quadrature IIR) */
    double hist[4][ICW_HIST_PITCH];
    uint64_t sncnt[4];
    double bus[ICW_N_INPUTS][4];
    /* serial render state per channel (dithered / noise-shaped renders only, else zero):
     * MT19937 words and next index (624: twist due), prev_rnd, prev_ns_err, shaper history by age */
    uint32_t mt[2][624];
    int32_t mt_idx[2];
    double rs[2][ICW_RSTATE];
};
constexpr uint64_t kBlobMagic = 0x33574349ull;   /* "ICW3" */

/* with the FIR Hilbert converter on, the stream's history (2 x its own k_M doubles, oldest first) follows the
 * blob; the size is that of the largest order in force, so one buffer serves every stream */
size_t icw_state_size(const icw_ctx *c) { return c ? sizeof(IcwBlob) + 2 * (size_t)c->fir_Mmax * sizeof(double) : 0; }

int icw_get_state(icw_ctx *c, int s, void *blob, size_t size)
{
    if (!c || !blob || size < icw_state_size(c) || s < 0 || s >= c->n_streams) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c)) return ICW_EDEVICE;
    IcwBlob b;
    memset(&b, 0, sizeof(b));
    b.magic = kBlobMagic;
    b.nord = (uint32_t)c->hilbs.at((size_t)s).nord;     /* the stream's own order */
    b.has_render = c->render_state ? 1u : 0u;
    b.fir_M = (uint32_t)c->firs.at((size_t)s).M;        /* the stream's own order */
    long long fd[3];
    bool ok = quiesce(c) == hipSuccess;
    ok &= hipMemcpy(&b.n_frame, c->st.n_frame + s, 8, hipMemcpyDeviceToHost) == hipSuccess;
    ok &= hipMemcpy(&b.pos, c->st.pos + s, 8, hipMemcpyDeviceToHost) == hipSuccess;
    ok &= hipMemcpy(fd, c->st.fade + (size_t)s * 3, sizeof(fd), hipMemcpyDeviceToHost) == hipSuccess;
    ok &= hipMemcpy(b.hq_phase, c->st.hq_phase + (size_t)s * 2, 8, hipMemcpyDeviceToHost) == hipSuccess;
    ok &= hipMemcpy(b.hist, c->st.hist + (size_t)s * 4 * ICW_HIST_PITCH, sizeof(b.hist), hipMemcpyDeviceToHost) == hipSuccess;
    ok &= hipMemcpy(b.sncnt, c->st.sncnt + (size_t)s * 4, sizeof(b.sncnt), hipMemcpyDeviceToHost) == hipSuccess;
    ok &= hipMemcpy(b.bus, c->st.bus + (size_t)s * ICW_N_INPUTS * 4, sizeof(b.bus), hipMemcpyDeviceToHost) == hipSuccess;
    if (c->render_state) {
        const size_t G = (size_t)c->n_streams * 2;
        for (int ch = 0; ch < 2; ++ch)
            ok &= hipMemcpy2D(b.mt[ch], 4, c->st.mt + (size_t)s * 2 + ch, G * 4, 4, 624, hipMemcpyDeviceToHost) == hipSuccess;
        ok &= hipMemcpy(b.mt_idx, c->st.mt_idx + (size_t)s * 2, sizeof(b.mt_idx), hipMemcpyDeviceToHost) == hipSuccess;
        ok &= hipMemcpy(b.rs, c->st.rs + (size_t)s * 2 * ICW_RSTATE, sizeof(b.rs), hipMemcpyDeviceToHost) == hipSuccess;
    }
    b.n_samples = fd[0]; b.n_fade_in = fd[1]; b.n_fade_out = fd[2];
    if (b.fir_M) {
        const size_t hrow = 2 * (size_t)b.fir_M;
        ok &= hipMemcpy((unsigned char *)blob + sizeof(b), c->fir_hist[c->fir_par] + c->fir_off[(size_t)s],
                        hrow * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (!ok) return ICW_EDEVICE;
    memcpy(blob, &b, sizeof(b));
    /* the blob is sized by the largest order in force: what lies past this stream's own history is zero */
    const size_t used = sizeof(b) + 2 * (size_t)b.fir_M * sizeof(double);
    memset((unsigned char *)blob + used, 0, icw_state_size(c) - used);
    return ICW_OK;
}

int icw_set_state(icw_ctx *c, int s, const void *blob, size_t size)
{
    if (!c || !blob || size < sizeof(IcwBlob) || s < 0 || s >= c->n_streams) return ICW_EINVAL;
    IcwBlob b;
    memcpy(&b, blob, sizeof(b));
    /* a blob need hold no more than its own stream's history: one taken in a context whose largest order was
     * the stream's fits a stream of that order in a context that also holds larger ones */
    if (b.fir_M > ICW_FIR_MAX_ORDER || size < sizeof(IcwBlob) + 2 * (size_t)b.fir_M * sizeof(double)) return ICW_EINVAL;
    /* a blob holds the state of the render and converter forms in force when it was saved: the
     * serial-render words exist only with a dithered / shaped render, the FIR history only at its order */
    if (b.magic != kBlobMagic || b.nord != (uint32_t)c->hilbs.at((size_t)s).nord || b.has_render != (c->render_state ? 1u : 0u) ||
        b.fir_M != (uint32_t)c->firs.at((size_t)s).M)
        return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c)) return ICW_EDEVICE;
    long long fd[3] = {b.n_samples, b.n_fade_in, b.n_fade_out};
    c->touched = true;
    bool ok = quiesce(c) == hipSuccess;
    ok &= hipMemcpy(c->st.n_frame + s, &b.n_frame, 8, hipMemcpyHostToDevice) == hipSuccess;
    c->nf_host[s] = b.n_frame;
    ok &= hipMemcpy(c->st.pos + s, &b.pos, 8, hipMemcpyHostToDevice) == hipSuccess;
    ok &= hipMemcpy(c->st.fade + (size_t)s * 3, fd, sizeof(fd), hipMemcpyHostToDevice) == hipSuccess;
    ok &= hipMemcpy(c->st.hq_phase + (size_t)s * 2, b.hq_phase, 8, hipMemcpyHostToDevice) == hipSuccess;
    ok &= hipMemcpy(c->st.hist + (size_t)s * 4 * ICW_HIST_PITCH, b.hist, sizeof(b.hist), hipMemcpyHostToDevice) == hipSuccess;
    ok &= hipMemcpy(c->st.sncnt + (size_t)s * 4, b.sncnt, sizeof(b.sncnt), hipMemcpyHostToDevice) == hipSuccess;
    ok &= hipMemcpy(c->st.bus + (size_t)s * ICW_N_INPUTS * 4, b.bus, sizeof(b.bus), hipMemcpyHostToDevice) == hipSuccess;
    const uint32_t eq = (b.hq_phase[0] == b.hq_phase[1] && !memcmp(b.hist[0], b.hist[2], sizeof(b.hist[0]) * 2)) ? 1u : 0u;
    const uint32_t eq2[2] = {eq, eq};
    ok &= hipMemcpy(c->st.lr_equal + (size_t)s * 2, eq2, sizeof(eq2), hipMemcpyHostToDevice) == hipSuccess;
    c->lr_known[s] = eq ? 1 : 0;
    if (c->render_state) {
        const size_t G = (size_t)c->n_streams * 2;
        for (int ch = 0; ch < 2; ++ch)
            ok &= hipMemcpy2D(c->st.mt + (size_t)s * 2 + ch, G * 4, b.mt[ch], 4, 4, 624, hipMemcpyHostToDevice) == hipSuccess;
        ok &= hipMemcpy(c->st.mt_idx + (size_t)s * 2, b.mt_idx, sizeof(b.mt_idx), hipMemcpyHostToDevice) == hipSuccess;
        ok &= hipMemcpy(c->st.rs + (size_t)s * 2 * ICW_RSTATE, b.rs, sizeof(b.rs), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (b.fir_M) {
        const size_t hrow = 2 * (size_t)b.fir_M;
        ok &= hipMemcpy(c->fir_hist[c->fir_par] + c->fir_off[(size_t)s], (const unsigned char *)blob + sizeof(b),
                        hrow * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    }
    return ok ? ICW_OK : ICW_EDEVICE;
}

int icw_get_fp_census(icw_ctx *c, int s, int reset, uint32_t counts[4][ICW_FES_N])
{
    if (!c || !counts || s < 0 || s >= c->n_streams) return ICW_EINVAL;
    if (!c->st.fes) {
        memset(counts, 0, sizeof(uint32_t) * 4 * ICW_FES_N);
        return ICW_OK;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
    uint32_t buf[4 * ICW_FES_PITCH];
    uint32_t *src = c->st.fes + (size_t)s * 4 * ICW_FES_PITCH;
    if (hipMemcpy(buf, src, sizeof(buf), hipMemcpyDeviceToHost) != hipSuccess) return ICW_EDEVICE;
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < ICW_FES_N; ++k) counts[i][k] = buf[i * ICW_FES_PITCH + k];
    if (reset && hipMemset(src, 0, sizeof(buf)) != hipSuccess) return ICW_EDEVICE;
    return ICW_OK;
}

int icw_last_k1_kernel(const icw_ctx *c)
{
    if (!c) return ICW_EINVAL;
    return c->last_k1;
}

int icw_last_dither_chunks(const icw_ctx *c, int *chunk_frames)
{
    if (!c) return ICW_EINVAL;
    if (chunk_frames) *chunk_frames = c->last_dchunk_frames;
    return c->last_dchunks;
}

int icw_last_timing(icw_ctx *c, double ms[2], int launches[2])
{
    if (!c || !ms || !launches) return ICW_EINVAL;
    ms[0] = c->last_ms[0];
    ms[1] = c->last_ms[1];
    launches[0] = c->last_launches[0];
    launches[1] = c->last_launches[1];
    return ICW_OK;
}

int icw_last_k0_timing(icw_ctx *c, double *ms)
{
    if (!c || !ms) return ICW_EINVAL;
    *ms = c->last_k0_ms;
    return ICW_OK;
}

}  /* extern "C" */
