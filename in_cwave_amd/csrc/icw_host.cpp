/*
 * icw_host.cpp -- the calls of the in_cwave_amd C ABI (include/icw.h) that run kernels:
 * icw_process_streams, the two CWAVE encoders and icw_prepare.  Each builds a CallPlan (one call's
 * resolved configuration, the one place every kernel-argument struct is filled) and runs its steps;
 * block scheduling is here.  The context's life, setters and state are in icw_context.cpp, the DSP-list
 * compiler in icw_graph_compile.cpp.  (The file keeps its name so that its history follows it.)
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
#include <mutex>
#include <optional>
#include <vector>

#include "../../include/icw.h"
#include "../../include/icw_cwave.h"
#include "icw_ctx.h"
#include "icw_launch.h"

namespace {

int grow(void **p, size_t *cur, size_t need)
{
    if (*cur >= need) return ICW_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cur = 0;
    if (hipMalloc(p, need) != hipSuccess) return ICW_ENOMEM;
    *cur = need;
    return ICW_OK;
}

/* bytes of n_frames frames of frame_bytes each: what an encoder call's stride must hold, what its staging
 * rows are */
size_t icw_enc_row_bytes(int n_frames, uint32_t frame_bytes) { return (size_t)n_frames * frame_bytes; }

/* Launch blocks of one call: (offset, frames) pairs of at most Tb frames.  A block pipeline fills
 * with K0 of the first block alone and drains with K2 (and the serial render) of the last block
 * alone, each on the whole chip (sF).  For calls of many blocks both ends are made short:
 *   - the first block is `first` frames, long enough that K1 of it covers K0 of the next full one;
 *   - the tail shrinks geometrically (ratio r) down to `tmin`, so that K2 of every tail block, which
 *     runs beside K1 of the next one, stays no longer than that K1 (C4: K2 ~0.8 K1 per frame).
 * With `ramp` > 1 the blocks after the first grow by that ratio up to Tb (the FIR converter's fill,
 * below).  Block sizes stay multiples of 64 frames; short calls keep uniform blocks. */
std::vector<std::pair<int, int>> plan_blocks(int n_frames, int Tb, int first, double r, int tmin, double ramp = 0.0)
{
    std::vector<std::pair<int, int>> bl;
    std::vector<int> tail;
    const bool shape = n_frames >= 4 * Tb;
    if (shape && r > 0.0) {
        for (double x = Tb * r; x >= tmin; x *= r) tail.push_back(((int)x) & ~63);
        long sum = 0;
        for (int v : tail) sum += v;
        if (sum > n_frames / 2) tail.clear();
    }
    int t = 0;
    double grow = 0.0;
    if (shape && first >= 64 && first < Tb) {
        bl.emplace_back(0, first);
        t = first;
        if (ramp > 1.0) grow = first * ramp;
    }
    long tail_sum = 0;
    for (int v : tail) tail_sum += v;
    const int body_end = n_frames - (int)tail_sum;
    while (t < body_end) {
        int T = std::min(Tb, body_end - t);
        if (grow > 0.0 && grow < Tb) {
            T = std::min(T, std::max(64, ((int)grow) & ~63));
            grow *= ramp;
        }
        bl.emplace_back(t, T);
        t += T;
    }
    for (int v : tail) {
        bl.emplace_back(t, v);
        t += v;
    }
    return bl;
}

/* wait for a K5 call's sequence number in host memory; the stream is queried now and then, so a
 * failed launch or a device fault ends the wait with an error instead of a hang */
bool poll_done(const uint32_t *flag, uint32_t seq, hipStream_t st)
{
    for (unsigned it = 1;; ++it) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return true;
        if ((it & 255u) == 0u) {
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess) return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq;
            if (q != hipErrorNotReady) return false;
        }
        __builtin_ia32_pause();
    }
}

/* a Master-only chain (signature count 1, mode MASTER, chain_in `in`: ICW_SIG_M) whose gains are
 * bit-identical: on mono input L and R are one computation (IcwFirArgs.lr_same) */
bool lr_same_master(const IcwProg &P)
{
    const IcwOp &m = P.ops[0];
    return P.chain && (P.sig & ~ICW_SIG_UNIT) == ICW_SIG_M && !memcmp(&m.gain[0], &m.gain[1], sizeof(double)) &&
           m.unit_gain[0] == m.unit_gain[1];
}

/* A call over streams [first, first + count) that run different lists or have different inputs: K2's
 * selection rows and the rotation table's slabs on the device, the launch configuration in c->mix.
 * The factors depend on the list, the counter and the rate, so the slabs are keyed by (list, rate):
 * one slab per pair with an active Shift / PM channel that at least two of the call's streams
 * share, at the counter of the first of them; a pair one stream has computes its factors inline
 * (the table would do the same work and add its traffic); a program without Shift / PM reads
 * nothing, so it is marked as using slab 0 against itself and skips the counter arithmetic.
 * fir: the FIR converter is on.  Its signature form reads every factor from the table, so every pair
 * with an active Shift / PM channel gets a slab, one stream or many (256 lists of one shape stay one
 * signature launch); and the call's streams are listed by channel class for KF2's stream maps. */
int prepare_mix(icw_ctx *c, int first, int count, bool fir, hipStream_t st)
{
    if (c->pid_valid && c->pid_first == first && c->pid_count == count && c->pid_fir == fir) return ICW_OK;
    const size_t S = (size_t)count;
    struct Pair {
        int32_t e;
        uint32_t rate;
        int uses, ref, slab;
    };
    std::vector<Pair> pairs;
    std::vector<size_t> pair_of(S);
    for (int i = 0; i < count; ++i) {
        const int32_t e = c->lists.index((size_t)(first + i));
        const uint32_t rate = c->inputs.at((size_t)(first + i)).sample_rate;
        size_t k = 0;
        while (k < pairs.size() && !(pairs[k].e == e && pairs[k].rate == rate)) ++k;
        if (k == pairs.size()) pairs.push_back(Pair{e, rate, 0, i, -1});
        ++pairs[k].uses;
        pair_of[(size_t)i] = k;
    }
    IcwProg &M = c->mix;
    M.is_bus = 0;                            /* a call with one bus-form stream runs every stream in bus form */
    M.needs_omega = 0;
    M.n_trig = 0;
    M.chain = 1;
    M.sig = 0;
    M.n_regs = 0;
    int n_slabs = 0;
    for (Pair &q : pairs) {
        const IcwProg &P = c->lists.ents[(size_t)q.e].prog;
        M.is_bus |= P.is_bus;
        M.needs_omega |= P.needs_omega;
        if (!P.chain) {
            M.chain = 0;
            M.n_regs = std::max(M.n_regs, P.n_regs);
        }
        if (P.needs_omega && P.n_trig > 0 && !P.is_bus && (q.uses >= 2 || fir)) {
            q.slab = n_slabs++;
            M.n_trig = std::max(M.n_trig, P.n_trig);
        }
    }
    /* [5][count] selection rows, the stream map [count], then [3][n_slabs] (n_slabs <= count: kPidWords per
     * stream hold them all) */
    std::vector<int32_t> h(S * 6 + (size_t)n_slabs * 3, 0);
    for (const Pair &q : pairs)
        if (q.slab >= 0) {
            int32_t *sl = h.data() + S * 6;
            sl[q.slab] = q.e;
            sl[n_slabs + q.slab] = q.ref;
            sl[2 * n_slabs + q.slab] = (int32_t)q.rate;
        }
    for (int i = 0; i < count; ++i) {
        const Pair &q = pairs[pair_of[(size_t)i]];
        const IcwProg &P = c->lists.ents[(size_t)q.e].prog;
        const bool no_trig = !(P.needs_omega && P.n_trig > 0);
        h[(size_t)i] = q.e;
        h[S + (size_t)i] = no_trig ? 0 : q.slab;
        h[2 * S + (size_t)i] = no_trig ? i : (q.slab >= 0 ? q.ref : i);
        h[3 * S + (size_t)i] = (int32_t)q.rate;
        h[4 * S + (size_t)i] = (int32_t)c->inputs.at((size_t)(first + i)).nch;
    }
    /* the channel classes: mono streams first in the map, then stereo ones.  A class keeps the signature
     * form while every stream's program is a chain of one signature; lr_same (IcwFirArgs) must hold for
     * every mono stream */
    c->pid_slab.assign(h.begin() + (long)S, h.begin() + 2 * (long)S);
    c->pid_ref.assign(h.begin() + 2 * (long)S, h.begin() + 3 * (long)S);
    size_t at = 0;
    for (int k = 0; k < 2; ++k) {
        IcwFirClass &fc = c->pid_cls[k];
        fc = IcwFirClass{};
        fc.map = c->d_pid + 5 * S + at;
        fc.nch = k + 1;
        fc.lr_same = k == 0;
        for (int i = 0; i < count; ++i) {
            if ((c->inputs.at((size_t)(first + i)).nch > 1) != (k == 1)) continue;
            const IcwProg &P = c->lists.ents[(size_t)pairs[pair_of[(size_t)i]].e].prog;
            const int32_t sig = P.chain ? P.sig : 0;
            if (fc.n == 0) fc.sig = sig;
            else if (fc.sig != sig) fc.sig = 0;
            fc.trig |= P.needs_omega ? 1 : 0;
            if (!lr_same_master(P)) fc.lr_same = 0;
            h[5 * S + at++] = i;
            ++fc.n;
        }
    }
    c->pid_map.assign(h.begin() + 5 * (long)S, h.begin() + 6 * (long)S);
    /* ordered after the earlier calls on st, which may still read the rows; waited for, since h goes */
    if (hipMemcpyAsync(c->d_pid, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return ICW_EDEVICE;
    c->pid_valid = true;
    ++c->pid_gen;
    c->pid_first = first;
    c->pid_count = count;
    c->pid_slabs = n_slabs;
    c->pid_fir = fir;
    return ICW_OK;
}

/* ---- the call plan ---- */

/* One call's resolved configuration.  It lives on the stack of the entry point, is filled once
 * (resolve_plan, stage_io, size_scratch, pick_streams; the encoders fill what their kernels read) and
 * is only read after that.  Its builders are the one place each kernel-argument struct is filled;
 * the structs are zeroed first and returned by value (the kernels read them whole). */
struct CallPlan {
    /* the context, the call's range (count and first also as sizes) and the caller's buffers */
    icw_ctx *const c;
    const icw_config &cfg;
    DevState &ds;
    const int first, count, n_frames;
    const size_t S, f0;
    const void *const in;
    void *const out, *dbg = nullptr;
    const size_t in_stride, out_stride;
    const unsigned flags;
    const bool dev, legacy;
    bool timing = false, xin = false;
    /* the resolved input: the one every stream of the call has, or (mixin, icw_set_stream_input) streams
     * with different inputs -- then fsz is the widest frame, nch the most channels, and the kernels
     * take each stream's own from the context's table dD or the selection rows */
    unsigned fmt = 0, rate = 0;
    bool mixin = false;
    /* mixin over CWAVE streams (icw_enable_stream_cwave): no K0 and no xd rows, K2 reads the frames itself */
    bool din = false;
    const IcwInDesc *dD = nullptr;
    unsigned csz = 0, nch = 0, fsz = 0;
    /* the resolved render.  The call's streams are cut into runs of one render table entry each
     * (StreamTable::runs); the render step works through the runs.  One run: the entry every stream of the
     * call has, and rk, serial_render and osz are its.  More (mixr, icw_set_stream_render): K2 leaves every
     * stream's pre-render doubles (serial_render holds, as for a serial render), osz is the widest frame
     * and rk is unread */
    IcwRenderK rk{};
    bool serial_render = false, mixr = false;
    unsigned render_type = 0;
    StreamRuns<RenderEnt> runs;
    int serial_gen = 0;            /* the call's channels with a serial entry (the K3c / K3b choice) */
    bool any_par = false;          /* some stream's entry is frame-parallel (mixr: KR runs) */
    int osz = 0;
    /* the encoders: the CWAVE output format and its frame bytes at the call's channels (mixin: the widest
     * stream's -- every stream's row holds n_frames of them, its own frames are icw_enc_frame_bytes) */
    uint32_t cw_format = 0;
    int efb = 0;
    unsigned long long ssr = 0;
    /* the list in use */
    const IcwProg *lp = nullptr, *dP = nullptr;
    bool mix = false;
    int n_slabs = 1;
    IcwFirClass fir_cls[2] = {};   /* mix with the FIR converter fused: the call's channel classes (prepare_mix) */
    size_t slab_stride = 0;
    /* the mode flags */
    bool cw = false, fir = false, fir_fused = false, fir_async = false, bus = false, fcm = false, dedup = false;
    /* fir over a context with several FIR converters (icw_set_stream_fir): the per-stream kernels read each
     * stream's own from the context's table, and fir_M / fir_nt are the widest among the call's streams (the
     * launches' LDS); one converter: the context's */
    bool firmix = false;
    int fir_M = 0, fir_nt = 0;
    /* bus, over several list entries (icw_enable_stream_bus): the mixed K4 over the call's runs of one entry
     * (prepare_bus_runs: its workgroups and the lanes of a bus row), every entry in bus form.  call_render: the
     * context's one render entry as this call runs it, serial behind a bus-form call (bus_lists) */
    bool busmix = false;
    int bwgs = 0, bW = 0;
    RenderEnt call_render{};
    bool dither = false, dith_par = false, table = false, in_step = false, s1 = false;
    int k1_mode = 0, row_waves = 0;
    /* the resolved Hilbert converter, cut into runs like the render; K2 is one launch per run.  One run: the
     * entry every stream of the call has (hb) -- also what a CWAVE-input call and the encoders hold, which
     * cut nothing.  More (mixh, icw_set_stream_hilbert, real input): K1 is one mixed launch over the runs'
     * descriptors and hb, the first run's entry, is unread.  max_nord sizes the w rows (each run keeps its
     * own N history rows in front) */
    const HilbEnt *hb;
    bool mixh = false;
    StreamRuns<HilbEnt> hruns;
    int max_nord, hwgs = 0;        /* mixh: the mixed launch's workgroups (prepare_hruns) */
    /* the block plan */
    std::vector<std::pair<int, int>> blocks;
    int n_blocks = 0, n_sets = 1, Tb = 0;
    size_t w_pitch = 0, x_pitch = 0;
    /* device pointers and strides; the host-pointer paths */
    const unsigned char *d_in = nullptr;
    unsigned char *d_out = nullptr;
    size_t dis = 0, dos = 0;
    double *d_pre = nullptr;
    size_t stage_in = 0, done_off = 0;
    bool pinned = false, pipe_io = false, zcopy = false, s1_poll = false;
    uint32_t s1_seq = 0u;
    std::vector<uint32_t> xin_phase;
    /* the streams: the caller's (a NULL handle with device pointers is the legacy default stream), then
     * the pipeline's */
    const hipStream_t st;
    hipStream_t sK = nullptr, sA = nullptr, sD = nullptr, sR = nullptr, sF = nullptr, sC = nullptr;

    CallPlan(icw_ctx *c_, int first_, int count_, const void *in_, size_t in_stride_, void *out_, size_t out_stride_,
             int n_frames_, unsigned flags_, void *hip_stream)
        : c(c_), cfg(c_->cfg), ds(c_->st), first(first_), count(count_), n_frames(n_frames_), S((size_t)count_), f0((size_t)first_), in(in_), out(out_),
          in_stride(in_stride_), out_stride(out_stride_), flags(flags_), dev(flags_ & ICW_F_DEVICE_PTRS),
          legacy(!hip_stream && (flags_ & ICW_F_DEVICE_PTRS)), hb(&c_->hilbs.at((size_t)first_)),
          hruns(StreamRuns<HilbEnt>::single(count_, hb)), max_nord(hb->nord),
          st(hip_stream ? (hipStream_t)hip_stream : c_->stream)
    {
    }

    /* waves per workgroup of the call's K1 (the row form: 2 unless ICW_K1_WG says otherwise) */
    int k1_wg_waves(bool row) const { return (c->tn.k1_wg_env || !row) ? c->tn.k1_wg : 2; }

    /* mixh: the waves of the mixed launch in either form -- every run rounded up to whole workgroups */
    int mixed_waves(bool row) const
    {
        const int wgw = k1_wg_waves(row);
        int w = 0;
        for (const auto &r : hruns) w += icw_k1_run_wgs(r.n, dedup, row, wgw) * wgw;
        return w;
    }

    /* what K0 and the FIR converter take alike: the reader's side of block b */
    template <class A>
    void reader_args(A &a, int b) const
    {
        a.in = d_in + (mixin ? 0 : (size_t)blocks[b].first * fsz);   /* mixin: K0 applies the offset per stream */
        a.in_stride = dis;
        a.fmt = fmt;
        a.csz = csz;
        a.fsz = fsz;
        a.nch = nch;
        a.n_streams = count;
        a.T = blocks[b].second;
        a.t0 = blocks[b].first;
        a.pos = c->st.pos + f0;
        a.fade = c->st.fade + f0 * 3;
    }

    /* K0 of block b: xd[p] was last read by K1 of block b-2 (and, complex input, by K2 of block
     * b-2, which precedes it on sA) */
    IcwK0Args k0_args(int b) const
    {
        IcwK0Args a0;
        memset(&a0, 0, sizeof(a0));
        reader_args(a0, b);
        a0.hq_phase = c->st.hq_phase + f0 * 2;
        a0.xd = c->xd[b % n_sets];
        a0.x_pitch = x_pitch;
        a0.dedup = dedup ? 1 : 0;
        return a0;
    }

    IcwK1Args k1_args(int b) const
    {
        const int p = b % n_sets;
        IcwK1Args a1;
        memset(&a1, 0, sizeof(a1));
        a1.xd = c->xd[p];
        a1.x_pitch = x_pitch;
        a1.nch = nch;
        a1.n_streams = count;
        a1.n_chains = count * 4;
        a1.T = blocks[b].second;
        a1.hist = ds.hist + f0 * 4 * ICW_HIST_PITCH;
        a1.sncnt = ds.sncnt + f0 * 4;
        a1.err = ds.err;
        a1.w = c->w[p];
        a1.w_pitch = w_pitch;
        a1.lr_equal = ds.lr_equal + f0 * 2;
        a1.hq_phase = ds.hq_phase + f0 * 2;
        a1.t0 = blocks[b].first;
        a1.info_dup = c->info_dup[p];
        memcpy(a1.pc, hb->pc, sizeof(a1.pc));      /* (mixh: unread, every run reads its entry's from the table) */
        a1.wg_waves = k1_wg_waves(k1_mode == 3);
        a1.dedup = dedup ? 1 : 0;
        a1.fes = fcm ? ds.fes + f0 * 4 * ICW_FES_PITCH : nullptr;
        return a1;
    }

    /* what is the call's of block b's K2 arguments; k2_run_args completes them for a run */
    IcwK2Args k2_args(int b) const
    {
        const int t0 = blocks[b].first, T = blocks[b].second, p = b % n_sets;
        IcwK2Args a2;
        memset(&a2, 0, sizeof(a2));
        a2.w = c->w[p];
        a2.w_pitch = w_pitch;
        a2.n_streams = count;
        a2.T = T;
        a2.n_chains = count * 4;
        a2.nch = nch;
        a2.t0 = t0;
        a2.hq_phase = ds.hq_phase + f0 * 2;
        a2.n_frame = ds.n_frame + f0;
        a2.ssr = ssr;
        a2.scaled = cfg.frmod_scaled;
        a2.sample_rate = rate;
        a2.prog = dP;
        a2.bus = ds.bus + f0 * ICW_N_INPUTS * 4;
        a2.out = d_out + (size_t)t0 * osz;
        a2.out_stride = dos;
        if (d_pre) {
            a2.pre = d_pre + (size_t)t0 * 2;
            a2.pre_stride = (size_t)n_frames * 2;
        } else if (serial_render) {
            a2.pre = c->rpre[p];
            a2.pre_stride = (size_t)T * 2;
        }
        a2.do_render = serial_render ? 0 : 1;
        a2.n_regs = lp->chain ? 0 : lp->n_regs;    /* a chain program keeps its values in VGPRs */
        a2.clips = ds.clips + f0 * 2;
        a2.peak_bits = ds.peak_bits + f0 * 2;
        a2.rk = rk;
        a2.cw = cw ? 1 : 0;
        a2.info_dup = cw ? nullptr : c->info_dup[p];
        a2.xin = c->xd[p];
        a2.x_pitch = x_pitch;
        if (bus) a2.iq_out = c->iq[p];
        a2.trig = lp->needs_omega;
        if (mix) {
            a2.prog_id = c->d_pid;
            a2.slab_stride = slab_stride;
        }
        a2.fes = fcm ? ds.fes + f0 * 4 * ICW_FES_PITCH : nullptr;
        return a2;
    }

    /* K2 of one run of the call's converters: the block's arguments as run_blocks completed them, offset to
     * the run's first stream the way a subset call offsets by f0, with the run's streams, its entry's
     * coefficients and its reject (real input only: a CWAVE or FIR call counts no rejections).  A call's one
     * run changes no address and keeps the call's selection rows.  Of several (mixh) each has rows of its
     * own (prepare_hruns); without rows the rotation table is read against the launch's stream 0, so a run
     * whose first stream is not in step with the call's gets none and computes its factors inline. */
    IcwK2Args k2_run_args(const IcwK2Args &a2, const StreamRun<HilbEnt> &r) const
    {
        const size_t s0 = (size_t)r.s0;
        IcwK2Args a = a2;
        a.w = a2.w + s0 * 4 * a2.w_pitch;
        a.n_streams = r.n;
        a.n_chains = r.n * 4;
        a.hq_phase = a2.hq_phase + s0 * 2;
        a.n_frame = a2.n_frame + s0;
        a.bus = a2.bus + s0 * ICW_N_INPUTS * 4;
        a.out = a2.out + s0 * a2.out_stride;
        if (a2.pre) a.pre = a2.pre + s0 * a2.pre_stride;
        a.clips = a2.clips + s0 * 2;
        a.peak_bits = a2.peak_bits + s0 * 2;
        memcpy(a.pc, r.e->pc, sizeof(a.pc));
        memcpy(a.pd, r.e->pd, sizeof(a.pd));
        a.d0 = r.e->d0;
        a.info_dup = a2.info_dup + s0 * 2;
        a.sncnt = (!cw && r.e->subn) ? ds.sncnt + (f0 + s0) * 4 : nullptr;
        if (a2.dith) a.dith = a2.dith + s0 * 2 * a2.dith_pitch;
        if (a2.prog_id) a.prog_id = mixh ? c->d_hpid + 5 * s0 : a2.prog_id;
        else if (a2.trig_tab && c->nf_host[f0 + s0] != c->nf_host[f0]) a.trig_tab = nullptr;
        return a;
    }

    /* what K2's direct-input form takes beside k2_args(b): the call's first frame (the kernel applies the
     * block offset at the stream's own frame size), the reader's state and the descriptor table */
    IcwDinArgs din_args() const
    {
        IcwDinArgs ad;
        memset(&ad, 0, sizeof(ad));
        ad.in = d_in;
        ad.in_stride = dis;
        ad.pos = ds.pos + f0;
        ad.fade = ds.fade + f0 * 3;
        ad.desc = dD;
        return ad;
    }

    /* The dither generator's / serial render's arguments for block b and one run of the call's renders: the
     * arguments offset to the run's first stream, the way a subset call offsets by f0; n_streams and n_gen
     * are the run's, rk its entry's, and its frames are the entry's size.  The K3c / K3b choice is the
     * call's (serial_gen).  The dither scratch is addressed by the run's first generator -- the rows at
     * g0 * (T rounded up to even) doubles, which holds either layout of a run -- so runs never alias. */
    IcwK3Args k3_args(int b, const IcwK2Args &a2, const StreamRun<RenderEnt> &r) const
    {
        const int t0 = blocks[b].first, T = blocks[b].second;
        const size_t r0 = f0 + (size_t)r.s0, g0 = (size_t)r.s0 * 2, Tp = (size_t)(T + (T & 1));
        IcwK3Args a3;
        memset(&a3, 0, sizeof(a3));
        a3.pre = a2.pre + (size_t)r.s0 * a2.pre_stride;
        a3.pre_stride = a2.pre_stride;
        a3.n_streams = r.n;
        a3.T = T;
        a3.out = d_out + (size_t)r.s0 * dos + (size_t)t0 * r.e->osz();
        a3.out_stride = dos;
        a3.mt = ds.mt + r0 * 2;
        a3.mt_idx = ds.mt_idx + r0 * 2;
        a3.rs = ds.rs + r0 * 2 * ICW_RSTATE;
        a3.clips = ds.clips + r0 * 2;
        a3.peak_bits = ds.peak_bits + r0 * 2;
        a3.n_gen = r.n * 2;
        a3.mt_pitch = c->n_streams * 2;
        a3.rk = r.e->rk;
        a3.fes = fcm ? ds.fes + r0 * 4 * ICW_FES_PITCH : nullptr;   /* (FP_CHECK: one render entry, one run) */
        /* the row-broadcast render (16 lanes per channel) while its waves stay few; FP_CHECK
         * keeps the compact lane-per-channel form */
        a3.row = r.e->serial && !fcm && (c->tn.render_row == 1 || (c->tn.render_row < 0 && serial_gen <= kRowRenderMax)) ? 1 : 0;
        a3.err = ds.err;
        if (r.e->dither) {
            a3.dith = c->dith[b % n_sets] + g0 * Tp;
            a3.dith_gm = (a3.row || !r.e->serial) ? 1 : 0;
            a3.dith_pitch = a3.dith_gm ? Tp : (size_t)r.n * 2;
            a3.wbuf = c->dwords + g0 * c->dwcap;
            a3.wpitch = a3.wcap = c->dwcap;
            a3.dflag = c->dflag + g0;
            a3.dbk = c->dbk + g0 * ICW_DBK;
            if (b == 0 && c->last_dchunks == 0) {    /* the call's first generator run (icw_last_dither_chunks) */
                c->last_dchunk_frames = icw_dith_chunk_frames(T, a3.wcap, icw_dith_words(a3.rk.render_type));
                c->last_dchunks = c->last_dchunk_frames > 0 ? (T + c->last_dchunk_frames - 1) / c->last_dchunk_frames : 0;
            }
        }
        return a3;
    }

    /* KR of block b: every stream of the call whose entry is frame-parallel, from K2's pre rows.  The
     * dither rows are the runs' (generator-major, T rounded up to even apart: row 2s + ch of the call) */
    IcwKRArgs kr_args(int b, const IcwK2Args &a2) const
    {
        const int T = blocks[b].second;
        IcwKRArgs ar;
        memset(&ar, 0, sizeof(ar));
        ar.pre = a2.pre;
        ar.pre_stride = a2.pre_stride;
        ar.out = d_out;
        ar.out_stride = dos;
        ar.tab = c->d_rtab;
        ar.ent = c->d_rof + f0;
        if (dither) {
            ar.dith = c->dith[b % n_sets];
            ar.dith_pitch = (size_t)(T + (T & 1));
        }
        ar.clips = ds.clips + f0 * 2;
        ar.peak_bits = ds.peak_bits + f0 * 2;
        ar.n_streams = count;
        ar.T = T;
        ar.t0 = blocks[b].first;
        return ar;
    }

    /* the bus-form graph of block b, behind its K2 */
    IcwK4Args k4_args(int b, const IcwK2Args &a2) const
    {
        IcwK4Args a4;
        memset(&a4, 0, sizeof(a4));
        a4.iq = c->iq[b % n_sets];
        a4.n_streams = count;
        a4.T = blocks[b].second;
        a4.t0 = blocks[b].first;
        a4.n_frame = a2.n_frame;
        a4.ssr = a2.ssr;
        a4.scaled = a2.scaled;
        a4.sample_rate = a2.sample_rate;
        a4.prog = dP;
        a4.bus = a2.bus;
        a4.pre = a2.pre;
        a4.pre_stride = a2.pre_stride;
        a4.desc = dD;
        return a4;
    }

    /* the same over the call's runs of one list entry each (busmix) */
    IcwK4MixArgs k4_mix_args(int b, const IcwK2Args &a2) const
    {
        IcwK4MixArgs m;
        memset(&m, 0, sizeof(m));
        m.k4 = k4_args(b, a2);
        m.k4.prog = c->d_bprogs;
        m.runs = c->d_bruns;
        m.n_runs = c->brun_n;
        m.W = bW;
        return m;
    }

    /* the rotation table of block b: the factors of every active Shift / PM channel per frame */
    IcwTrigArgs trig_args(int b) const
    {
        const int T = blocks[b].second;
        IcwTrigArgs at;
        memset(&at, 0, sizeof(at));
        at.prog = dP;
        at.n_frame = c->st.n_frame + f0;
        at.t0 = blocks[b].first;
        at.T = T;
        at.scaled = c->cfg.frmod_scaled;
        at.trig_pitch = 2 * lp->n_trig;
        at.ssr = ssr;
        at.sample_rate = rate;
        at.tab = c->trig;
        if (mix) {
            at.slabs = c->d_pid + 6 * (size_t)count;
            at.n_slabs = n_slabs;
            at.slab_stride = slab_stride;
        }
        /* the fused FIR kernel's lanes hold 4 / 8 consecutive frames: rows 8 frames apart */
        at.perm_q = fir_fused ? (T + 7) / 8 : 0;
        return at;
    }

    /* KF's arguments for launch block b; it reads the history buffer the previous block wrote
     * (same stream, block order) and writes the other one */
    IcwFirArgs fir_args(int b) const
    {
        IcwFirArgs af;
        memset(&af, 0, sizeof(af));
        reader_args(af, b);
        af.M = fir_M;
        af.nt = fir_nt;
        af.g = c->d_fir_g;
        /* the rows of the call's first stream; firmix: the whole buffers, every stream finds its own rows */
        const size_t h0 = firmix ? 0 : c->fir_off[f0];
        af.hist_in = c->fir_hist[(c->fir_par + b) & 1] + h0;
        af.hist_out = c->fir_hist[(c->fir_par + b + 1) & 1] + h0;
        af.conv = firmix ? c->d_fconv + f0 : nullptr;
        af.xd = c->xd[b % n_sets];
        af.x_pitch = x_pitch;
        af.sig = lp->chain ? lp->sig : 0;
        af.desc = fir && mixin ? dD : nullptr;      /* streams with different inputs: the kernels read each one's own */
        /* per-stream lists: signature and lr_same are per channel class (fir_cls) */
        if (mix) af.sig = 0;
        else af.lr_same = nch == 1 && lr_same_master(*lp);
        return af;
    }

    /* where block b's frames go: the one-input kernels get the block's first frame (the host knows the one
     * frame size); the per-stream ones the call's first frame and apply the offset at their stream's own */
    unsigned char *enc_out(int b) const { return d_out + (mixin || firmix ? 0 : (size_t)blocks[b].first * efb); }

    /* KFE of block b: KF's arguments, the packed frames as the output.  It packs frames instead of writing
     * K2's rows, and no graph follows it: no row buffer, no chain signature */
    IcwEncArgs enc_args(int b) const
    {
        IcwEncArgs e;
        memset(&e, 0, sizeof(e));
        e.f = fir_args(b);
        e.f.xd = nullptr;
        e.f.x_pitch = 0;
        e.f.sig = 0;
        e.f.lr_same = 0;
        e.out = enc_out(b);
        e.out_stride = dos;
        e.clipped = c->enc_clipped + f0;
        return e;
    }

    /* the IIR encoder's K2 of block b -- up to `in`: the output sums and the fs/4 un-mix, then the rows
     * instead of the graph (they go out although the list is not bus form: K2 ends there); it still counts
     * the block's de-subnorm rejections.  Nothing is rendered: no output bytes, no pre-render rows.  With
     * do_render 0 and iq_out set K2 returns after the rows, so what k2_args filled of the render (rk, clips,
     * peak_bits) is unread; and no graph runs, so no rotation factors whatever the list holds */
    IcwK2Args enc_k2_args(int b) const
    {
        IcwK2Args a2 = k2_args(b);
        a2.iq_out = c->iq[0];
        a2.do_render = 0;
        a2.out = nullptr;
        a2.out_stride = 0;
        a2.pre = nullptr;
        a2.pre_stride = 0;
        a2.trig = 0;
        return a2;
    }

    /* KIP of block b, behind that K2 */
    IcwPackArgs pack_args(int b) const
    {
        IcwPackArgs ap;
        memset(&ap, 0, sizeof(ap));
        ap.iq = c->iq[0];
        ap.n_streams = count;
        ap.T = blocks[b].second;
        ap.out = enc_out(b);
        ap.out_stride = dos;
        ap.clipped = c->enc_clipped + f0;
        return ap;
    }

    IcwAdvArgs adv_args() const
    {
        IcwAdvArgs av;
        memset(&av, 0, sizeof(av));
        av.n_streams = count;
        av.cw = cw ? 1 : 0;
        av.n = n_frames;
        av.hq_phase = ds.hq_phase + f0 * 2;
        av.pos = ds.pos + f0;
        av.n_frame = ds.n_frame + f0;
        av.ssr = ssr;
        av.scaled = c->cfg.frmod_scaled;
        if (pinned) {
            av.err = ds.err;
            av.err_copy = (int *)(d_out + dos * S);        /* the output buffer has 16 spare bytes */
        }
        if (s1_poll) {
            av.done = (uint32_t *)(d_out + done_off);
            av.seq = s1_seq;
        }
        return av;
    }

    /* the steps of a call, in the order the entry points take them */
    void pick_k1();
    hipError_t launch_unpack(int b, hipStream_t s) const;
    hipError_t launch_k1(const IcwK1Args &a1, hipStream_t s) const;
    hipError_t launch_k2(const IcwK2Args &a2, hipStream_t s) const;
    hipError_t launch_fir_encode(int b, int cwf) const;
    hipError_t launch_pack(int b, int cwf) const;
    hipError_t launch_advance() const;
    void stereo_diverged() const;
    int prepare_hruns();
    int prepare_bus_runs();
    int join_legacy_stream() const;
    int stage_host_io(size_t in_row, size_t out_row);
    bool stage_copy_in() const;
    bool stage_copy_out(size_t row_bytes) const;
    size_t out_row_bytes(size_t i) const;
    bool copy_out_own() const;
    bool fir_hist_back() const;
    void resolve_fir();
    int enc_format(uint32_t cw_fmt, bool fir_ok);
    int enc_buffers();
    int enc_mix_lists();
    bool enc_copy_out() const;
    void set_pitches();
    void plan_uniform(int max_block);
    int resolve_plan();
    int stage_io();
    int size_scratch();
    int pick_streams();
    int run_stream1() const;
    int io_in(int b, hipStream_t s0) const;
    int launch_k0(int b) const;
    int run_blocks() const;
    int finish_call() const;
};


/* The K1 of a call over the plan's streams of real input (cw, fcm and nch are set): dedup, k1_mode
 * and row_waves, the row kernel's waves over these streams. */
void CallPlan::pick_k1()
{
    /* mono dedup: every stream of the call known to hold identical left / right converters */
    dedup = !cw && !fcm && nch == 1 && c->tn.dedup_ok && (c->tn.k1_mode <= 0 || c->tn.k1_mode == 3);   /* plain / row K1 */
    for (int i = 0; dedup && i < count; ++i) dedup = c->lr_known[first + i] != 0;
    /* K1 variant of this call.  Auto: the row-broadcast kernel (4 chains per wave, ~17 % fewer
     * instructions per sample) when its waves fit k1_wpc per CU on at most half the chip, else the
     * lane-per-chain kernel (64 chains per wave).  The row kernel needs Kahan + the reject.  (Round
     * 1 kept it off with a serial render; with the partition working, C5 gains 9 % from it.) */
    row_waves = (int)(((dedup ? count : 2L * count) + 3) / 4) * 2;
    bool row_ok = hb->kahan && hb->subn;
    if (mixh) {
        /* streams with different converters: the rule on the mixed launch's real waves (every run rounds up
         * to whole wave pairs, so many short runs need more waves than their streams in one run), and the
         * row form only when every entry of the call is Kahan + reject */
        row_waves = mixed_waves(true);
        row_ok = true;
        for (const auto &r : hruns) row_ok = row_ok && r.e->kahan && r.e->subn;
    }
    k1_mode = c->tn.k1_mode;
    if (k1_mode < 0) k1_mode = (row_ok && row_waves <= (c->n_cu / 2) * c->tn.k1_wpc) ? 3 : 0;
    if (k1_mode == 3 && !row_ok) k1_mode = 0;
    if (fcm) k1_mode = ICW_K1_FC;                  /* FP_CHECK: FC() kernels, no shortcuts */
}

/* the plan's K1 on stream s */
hipError_t CallPlan::launch_k1(const IcwK1Args &a1, hipStream_t s) const
{
    if (mixh) return icw_launch_iir_mixed(&a1, k1_mode == 3, c->d_hruns, (int)hruns.size(), hwgs, c->d_hpc, s);
    return k1_mode == ICW_K1_FC ? icw_launch_iir_fc(&a1, hb->nord, hb->kahan, hb->subn, s)
         : k1_mode == 3         ? icw_launch_iir_row(&a1, hb->nord, hb->kahan, hb->subn, s)
                                   : icw_launch_iir_state(&a1, hb->nord, hb->kahan, hb->subn, s);
}

/* K0 of block b on stream s; streams with different inputs: K0 takes each one's format from the table */
hipError_t CallPlan::launch_unpack(int b, hipStream_t s) const
{
    IcwK0MixArgs m;
    memset(&m, 0, sizeof(m));
    m.k0 = k0_args(b);
    m.desc = dD;
    if (mixin) return icw_launch_unpack_mixed(&m, s);
    return icw_launch_unpack(&m.k0, s);
}

/* KFE of block b on the caller's stream; streams with different inputs or converters: its per-stream form */
hipError_t CallPlan::launch_fir_encode(int b, int cwf) const
{
    const auto e = enc_args(b);
    if (mixin || firmix) return icw_launch_fir_encode_mixed(&e, cwf, st);
    return icw_launch_fir_encode(&e, cwf, st);
}

/* KIP of block b on the caller's stream; streams with different inputs: every stream's own channels, its
 * tile at its own frame size */
hipError_t CallPlan::launch_pack(int b, int cwf) const
{
    IcwPackMixArgs m;
    memset(&m, 0, sizeof(m));
    m.p = pack_args(b);
    m.desc = dD;
    m.t0 = blocks[b].first;
    if (mixin) return icw_launch_iq_pack_mixed(&m, cwf, st);
    return icw_launch_iq_pack(&m.p, cwf, nch > 1 ? 2 : 1, st);
}

/* icw_advance on the caller's stream, behind every kernel of the call; streams with different inputs wrap
 * their frame counters at their own rates */
hipError_t CallPlan::launch_advance() const
{
    IcwAdvMixArgs m;
    memset(&m, 0, sizeof(m));
    m.adv = adv_args();
    m.desc = dD;
    if (mixin) return icw_launch_advance_mixed(&m, st);
    return icw_launch_advance(&m.adv, st);
}

/* after a call over real input: a stereo stream's left / right converters are no longer known equal */
void CallPlan::stereo_diverged() const
{
    if (!cw && nch > 1)
        for (int i = 0; i < count; ++i)
            if (c->inputs.at(f0 + (size_t)i).nch > 1) c->lr_known[first + i] = 0;
}

/* the plan's K2 on stream s: one launch per run of the call's converters */
hipError_t CallPlan::launch_k2(const IcwK2Args &a2, hipStream_t s) const
{
    for (const auto &r : hruns) {
        const IcwK2Args ar = k2_run_args(a2, r);
        const hipError_t e = icw_launch_output(&ar, r.e->nord, r.e->kahan, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

/* A call over streams with different Hilbert converters: the run descriptors of the mixed K1 launch on the
 * device (and, where the lists or inputs differ too, every run's own K2 selection rows: the call's rows cut
 * by run, the reference stream relative to the run's first).  Kept while the call's shape and the settings
 * stay; rebuilt otherwise, ordered after the earlier calls on st, which may still read the old ones. */
int CallPlan::prepare_hruns()
{
    const bool row = k1_mode == 3;
    const int wgw = k1_wg_waves(row);
    if (c->hrun_valid && c->hrun_first == first && c->hrun_count == count && c->hrun_dedup == dedup && c->hrun_row == row &&
        c->hrun_waves == wgw && c->hrun_mix == mix && (!mix || c->hrun_pid_gen == c->pid_gen)) {
        hwgs = c->hrun_wgs;
        return ICW_OK;
    }
    std::vector<IcwK1Run> h(hruns.size());
    int wg = 0;
    for (size_t k = 0; k < hruns.size(); ++k) {
        const auto &r = hruns[k];
        IcwK1Run d;
        memset(&d, 0, sizeof(d));
        d.wg0 = wg;
        d.s0 = r.s0;
        d.n = r.n;
        d.nord = r.e->nord;
        d.kahan = r.e->kahan;
        d.subn = r.e->subn;
        d.pc_off = (int32_t)(r.e - c->hilbs.ents.data()) * 20;
        h[k] = d;
        wg += icw_k1_run_wgs(r.n, dedup, row, wgw);
    }
    std::vector<int32_t> rows;
    if (mix) {
        rows.assign(5 * S, 0);
        for (const auto &r : hruns) {
            int32_t *q = rows.data() + 5 * (size_t)r.s0;
            for (int i = 0; i < r.n; ++i) {
                const size_t k = (size_t)(r.s0 + i);
                q[i] = c->lists.index(f0 + k);
                q[r.n + i] = c->pid_slab[k];
                q[2 * r.n + i] = c->pid_ref[k] - r.s0;
                q[3 * r.n + i] = (int32_t)c->inputs.at(f0 + k).sample_rate;
                q[4 * r.n + i] = (int32_t)c->inputs.at(f0 + k).nch;
            }
        }
    }
    if (hipMemcpyAsync(c->d_hruns, h.data(), h.size() * sizeof(IcwK1Run), hipMemcpyHostToDevice, st) != hipSuccess ||
        (mix && hipMemcpyAsync(c->d_hpid, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        return ICW_EDEVICE;
    c->hrun_valid = true;
    c->hrun_first = first;
    c->hrun_count = count;
    c->hrun_dedup = dedup;
    c->hrun_row = row;
    c->hrun_waves = wgw;
    c->hrun_mix = mix;
    c->hrun_pid_gen = c->pid_gen;
    c->hrun_n = (int)hruns.size();
    c->hrun_wgs = hwgs = wg;
    return ICW_OK;
}

/* A bus-form call over several list entries: every entry's bus-form program on the device -- its own, or for
 * a register-form entry the twin, compiled here the first time -- and the call's runs of one entry each
 * (icw_k4_cut_runs).  The programs are kept while the lists stay (every list edit waits for the context's work
 * first, so nothing reads the old ones), the runs while the lists and the call's range stay; rebuilt runs are
 * ordered after the earlier calls on st, which may still read the old ones. */
int CallPlan::prepare_bus_runs()
{
    const size_t n = c->lists.size();
    if (c->bprogs_gen != c->lists_gen) {
        std::vector<IcwProg> h(n);
        for (size_t k = 0; k < n; ++k) {
            ListEnt &e = c->lists.ents[k];
            if (!e.prog.is_bus && !e.has_twin) {
                icw_config tc = c->cfg;
                tc.bypass_list = e.prog.bypass;
                const int rc = build_prog_bus(tc, e.nodes, e.twin);
                if (rc != ICW_OK) return rc;
                e.has_twin = true;
            }
            h[k] = e.prog.is_bus ? e.prog : e.twin;
        }
        IcwProg *fresh = nullptr;
        if (hipMalloc((void **)&fresh, n * sizeof(IcwProg)) != hipSuccess) return ICW_ENOMEM;
        if (hipMemcpy(fresh, h.data(), n * sizeof(IcwProg), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(fresh);
            return ICW_EDEVICE;
        }
        if (c->d_bprogs) (void)hipFree(c->d_bprogs);
        c->d_bprogs = fresh;
        c->bprogs_gen = c->lists_gen;
    }
    /* (no clearing fill: it would run on the null stream, which st does not wait for, and could land on the
     * runs copied below; every run a launch reads has been written) */
    if (!c->d_bruns && hipMalloc((void **)&c->d_bruns, (size_t)c->n_streams * sizeof(IcwK4Run)) != hipSuccess) {
        c->d_bruns = nullptr;
        return ICW_ENOMEM;
    }
    if (c->brun_gen != c->lists_gen || c->brun_first != first || c->brun_count != count) {
        std::vector<IcwK4Run> h;
        int W = 0;
        const int wgs = icw_k4_cut_runs(c->lists.of.data() + f0, count, h, &W);
        if (hipMemcpyAsync(c->d_bruns, h.data(), h.size() * sizeof(IcwK4Run), hipMemcpyHostToDevice, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return ICW_EDEVICE;
        c->brun_gen = c->lists_gen;
        c->brun_first = first;
        c->brun_count = count;
        c->brun_n = (int)h.size();
        c->brun_wgs = wgs;
        c->brun_W = W;
    }
    bwgs = c->brun_wgs;
    bW = c->brun_W;
    return ICW_OK;
}

/* ---- what the process call and the encoders share ---- */

/* A NULL handle with device pointers means the legacy default stream (torch's default stream):
 * the call starts after the work already queued there, and returns when its results are in
 * place, so that stream's later work sees them.  The end is a host wait, not an operation on the
 * null stream: a null-stream wait behind the context's CU-masked streams cost C2 13-25 % (its
 * implicit synchronisation with every blocking stream serialises the block pipeline). */
int CallPlan::join_legacy_stream() const
{
    if (legacy && (hipEventRecord(c->join, nullptr) != hipSuccess || hipStreamWaitEvent(st, c->join, 0) != hipSuccess))
        return ICW_EDEVICE;
    return ICW_OK;
}

/* the encoders' per-stream count of saturated / NaN int16 samples, allocated by the first encode */
int ensure_enc_clipped(icw_ctx *c)
{
    if (c->enc_clipped) return ICW_OK;
    const int rc = dalloc(&c->enc_clipped, (size_t)c->n_streams);
    if (rc != ICW_OK) {
        if (c->enc_clipped) (void)hipFree(c->enc_clipped);
        c->enc_clipped = nullptr;
    }
    return rc;
}

/* Host pointers: the device staging pair, rows of dis / dos bytes per stream (the output has 16 spare
 * bytes for the error flag's copy), and the plain 2-D copies of the whole call in and out on st. */
int CallPlan::stage_host_io(size_t in_row, size_t out_row)
{
    if (grow((void **)&c->d_in, &c->d_in_bytes, in_row * S)) return ICW_ENOMEM;
    if (grow((void **)&c->d_out, &c->d_out_bytes, out_row * S + 16)) return ICW_ENOMEM;
    d_in = c->d_in;
    d_out = c->d_out;
    dis = in_row;
    dos = out_row;
    return ICW_OK;
}

bool CallPlan::stage_copy_in() const
{
    return hipMemcpy2DAsync(c->d_in, dis, in, in_stride, dis, S, hipMemcpyHostToDevice, st) == hipSuccess;
}

bool CallPlan::stage_copy_out(size_t row_bytes) const
{
    return hipMemcpy2DAsync(out, out_stride, c->d_out, dos, row_bytes, S, hipMemcpyDeviceToHost, st) == hipSuccess;
}

/* the rendered bytes of stream i of the call: n_frames frames of its own size (mixr), else of the call's */
size_t CallPlan::out_row_bytes(size_t i) const
{
    return (size_t)n_frames * (size_t)(mixr ? c->renders.at(f0 + i).osz() : osz);
}

/* the staged frames of a call over streams with different renders back to host pointers: every stream's own
 * bytes, so a 16-bit stream's row is written no further than its frames (a 2-D copy has one width) */
bool CallPlan::copy_out_own() const
{
    for (size_t i = 0; i < S; ++i)
        if (hipMemcpyAsync((unsigned char *)out + i * out_stride, c->d_out + i * dos, out_row_bytes(i), hipMemcpyDeviceToHost, st) != hipSuccess)
            return false;
    return true;
}

/* FIR history: the current rows of every stream stay in fir_hist[fir_par] between calls (a call on
 * a subset of the streams must not move the others' rows); after an odd number of blocks this
 * call's rows are in the other buffer and come back */
bool CallPlan::fir_hist_back() const
{
    if (!(n_blocks & 1)) return true;
    const size_t at = c->fir_off[f0], len = c->fir_off[f0 + S] - at;     /* the call's streams, each at its own order */
    return hipMemcpyAsync(c->fir_hist[c->fir_par] + at, c->fir_hist[c->fir_par ^ 1] + at, len * sizeof(double),
                          hipMemcpyDeviceToDevice, st) == hipSuccess;
}

/* the FIR converter of the call's streams (fir is set): the context's one, or -- several in force -- the table,
 * with the widest order and taps of the call.  A call whose own streams share an entry takes the table too:
 * the bytes are the same, and the history is then found one way */
void CallPlan::resolve_fir()
{
    fir_M = c->fir_M;
    fir_nt = c->fir_nt;
    firmix = fir && c->firs.size() > 1;
    if (!firmix) return;
    fir_M = fir_nt = 0;
    for (size_t i = 0; i < S; ++i) {
        fir_M = std::max(fir_M, c->firs.at(f0 + i).M);
        fir_nt = std::max(fir_nt, c->firs.at(f0 + i).nt);
    }
}

/* The encoders' input and format checks.  The input of the call's streams is resolved as resolve_plan
 * resolves it -- the one all of them have (the launches are then those of a one-input context), or mixin:
 * the table; the rate plays no part in an encode (no fades of its own, no graph), so streams that differ in
 * it alone share one input here.  Then: real input, the converter asked for on or off, a CWAVE output
 * format, and strides that hold the call -- n_frames of the widest input frame and of the widest output
 * frame; a one-input call with device pointers is not checked, as ever.  Nothing has run when this fails. */
int CallPlan::enc_format(uint32_t cw_fmt, bool fir_ok)
{
    const IcwInDesc &d0 = c->inputs.at(f0);
    fmt = d0.fmt;
    rate = d0.sample_rate;
    csz = d0.csz;
    nch = d0.nch;
    fsz = d0.fsz;
    for (int i = 1; i < count && c->inputs.size() > 1; ++i) {
        const IcwInDesc &d = c->inputs.at(f0 + (size_t)i);
        if (d.fmt != fmt || d.nch != d0.nch) mixin = true;
        if (d.fmt >= ICW_FMT_CW_F64) fmt = d.fmt;     /* a CWAVE stream anywhere in the call: refused below */
        fsz = std::max(fsz, d.fsz);
        nch = std::max(nch, d.nch);
    }
    if (mixin) dD = c->d_inputs + f0;
    fir = c->fir_M > 0;
    resolve_fir();
    cw_format = cw_fmt;
    efb = icw_cwave_frame_bytes(cw_fmt, nch);
    if (fmt >= ICW_FMT_CW_F64 || !fir_ok || efb == 0) return ICW_EINVAL;
    if ((!dev || mixin) && (in_stride < icw_enc_row_bytes(n_frames, fsz) || out_stride < icw_enc_row_bytes(n_frames, (uint32_t)efb)))
        return ICW_EINVAL;
    return ICW_OK;
}

/* the encoders' buffers: the caller's device pointers, or the staging pair with every stream's frames
 * 16-byte aligned */
int CallPlan::enc_buffers()
{
    d_in = (const unsigned char *)in;
    d_out = (unsigned char *)out;
    dis = in_stride;
    dos = out_stride;
    return dev ? ICW_OK : stage_host_io(icw_enc_row_bytes(n_frames, fsz), (icw_enc_row_bytes(n_frames, (uint32_t)efb) + 15) & ~(size_t)15);
}

/* the staged frames back to host pointers: every stream's own n_frames * FB_s bytes, so a narrower stream's
 * row is written no further than its frames.  One copy per stream where the one-input path makes one 2-D
 * copy: a 2-D copy has one width, and the widest would write a narrower stream's row past its frames.  Not
 * measured; the host-pointer path is the convenience path (the file layer and the rate tool use device
 * pointers), and a host that minds the per-copy cost passes device pointers. */
bool CallPlan::enc_copy_out() const
{
    if (!mixin) return stage_copy_out(icw_enc_row_bytes(n_frames, (uint32_t)efb));
    for (size_t i = 0; i < S; ++i) {
        const size_t nb = icw_enc_row_bytes(n_frames, (uint32_t)icw_cwave_frame_bytes(cw_format, c->inputs.at(f0 + i).nch));
        if (hipMemcpyAsync((unsigned char *)out + i * out_stride, c->d_out + i * dos, nb, hipMemcpyDeviceToHost, st) != hipSuccess)
            return false;
    }
    return true;
}

/* The IIR encoder over streams with different inputs runs K2's per-stream instances, as a mixed-input
 * process call does: the selection rows (prepare_mix: each stream's channels, its list where the lists
 * differ too) and their launch configuration.  After plan_uniform, which chose the context's one list. */
int CallPlan::enc_mix_lists()
{
    const int rc = prepare_mix(c, first, count, false, st);
    if (rc != ICW_OK) return rc;
    mix = true;
    lp = &c->mix;
    dP = c->lists.size() > 1 ? c->d_progs : c->d_prog;
    return ICW_OK;
}

/* at least n events in v */
bool grow_events(std::vector<hipEvent_t> &v, int n, unsigned flags)
{
    while ((int)v.size() < n) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, flags) != hipSuccess) return false;
        v.push_back(e);
    }
    return true;
}

/* ---- icw_process_streams, step by step ---- */

/* the format, the list and the modes of the call, and its launch blocks */
int CallPlan::resolve_plan()
{
    /* the input of the call's streams: the one table entry all of them have, resolved here (the launches
     * are then those of a one-input context), or the table.  A one-entry table is not scanned, here and below */
    const IcwInDesc &d0 = c->inputs.at(f0);
    fmt = d0.fmt;
    rate = d0.sample_rate;
    csz = d0.csz;
    nch = d0.nch;
    fsz = d0.fsz;
    for (int i = 1; i < count && c->inputs.size() > 1; ++i) {
        const IcwInDesc &d = c->inputs.at(f0 + (size_t)i);
        if (d.fmt != fmt || d.nch != d0.nch || d.sample_rate != rate) mixin = true;
        /* one kind per call: whether K1 runs is the call's decision, and the scratch rows differ (2 per
         * real stream, 4 per complex one) */
        if ((d.fmt >= ICW_FMT_CW_F64) != (fmt >= ICW_FMT_CW_F64)) return ICW_EUNSUPPORTED;
        fsz = std::max(fsz, d.fsz);
        nch = std::max(nch, d.nch);
    }
    if (mixin) dD = c->d_inputs + f0;
    din = mixin && fmt >= ICW_FMT_CW_F64;
    /* the render of the call's streams: the runs of its table; the first one's entry is the call's while
     * it is the only one */
    runs = c->renders.runs(f0, S);
    const RenderEnt &r0 = *runs[0].e;
    rk = r0.rk;
    serial_render = r0.serial;
    render_type = r0.cfg.render_type;
    mixr = runs.size() > 1;
    if (mixr) serial_render = true;
    for (const auto &r : runs) {
        osz = std::max(osz, r.e->osz());
        if (r.e->serial) serial_gen += 2 * r.n;
        else any_par = true;
    }
    /* the Hilbert converter of the call's streams (hb: the first stream's entry), cut like the render.  A
     * CWAVE-input call runs no recurrence and no output sums: it keeps that entry as its one run */
    if (fmt < ICW_FMT_CW_F64) hruns = c->hilbs.runs(f0, S);
    mixh = hruns.size() > 1;
    for (const auto &r : hruns) max_nord = std::max(max_nord, r.e->nord);
    ssr = (unsigned long long)rate * ICW_HZ_SCALE;
    timing = flags & 4u;
    /* ICW_F_DEBUG_INPUT: K0's output of every launch block is copied aside (test hook, host dbg) */
    xin = flags & ICW_F_DEBUG_INPUT;
    if (xin && c->inputs.size() > 1) return ICW_EUNSUPPORTED;
    if (xin && (dev || !dbg || (flags & ICW_F_DEBUG_PRE) || fmt >= ICW_FMT_CW_F64 || c->fir_M > 0 ||
                   cfg.fp_check))
        return ICW_EINVAL;
    /* every stream's row holds the call's frames at the widest frame of the call (mixin: K0 reads by
     * the table, so the bound is checked for device pointers too) */
    if ((!dev || mixin) && in_stride < (size_t)n_frames * fsz) return ICW_EINVAL;
    if ((!dev || mixr) && out_stride < (size_t)n_frames * osz) return ICW_EINVAL;

    /* FIR Hilbert converter (icw_set_fir_hilbert): real input becomes complex samples in KF and
     * the block continues as CWAVE input does */
    fir = c->fir_M > 0 && fmt < ICW_FMT_CW_F64;
    cw = fmt >= ICW_FMT_CW_F64 || fir;
    resolve_fir();
    /* the list of the call's streams: the one table entry all of them run, or -- streams with different
     * lists or inputs -- the table with K2's per-stream selection (prepare_mix).  The device holds the table
     * only for more than one entry; a one-list context launches from d_prog */
    lp = &c->lists.at(f0).prog;
    dP = c->lists.size() > 1 ? c->d_progs : c->d_prog;
    mix = mixin || firmix || !c->lists.uniform(f0, S);
    if (!mix) dP += c->lists.index(f0);
    if (mix) {
        const int rc = prepare_mix(c, first, count, fir, st);
        if (rc != ICW_OK) return rc;
        lp = &c->mix;
    }
    const IcwProg &LP = *lp;
    n_slabs = mix ? c->pid_slabs : 1;
    bus = LP.is_bus;
    busmix = bus && mix && c->lists.size() > 1;
    if (c->bus_lists) {
        /* bus-form lists beside others: the one render entry holds the render's own form, and a bus-form
         * call renders serial behind K4 whatever it is; a register-form call keeps its usual kernels */
        call_render = *runs[0].e;
        call_render.serial = call_render.serial || bus;
        runs = StreamRuns<RenderEnt>::single(count, &call_render);
        serial_render = call_render.serial;
        serial_gen = call_render.serial ? 2 * count : 0;
        any_par = !call_render.serial;
    }
    fcm = cfg.fp_check != 0;
    pick_k1();
    if (!cw) c->last_k1 = k1_mode;
    /* launch blocks.  The tail taper (plan_blocks) is on by default where it fits: a small batch
     * (the row kernel K1r) with a serial render -- its drain is the render of the last block, and
     * the frame-parallel kernels take well under K1r's time per frame (C5: +2 %).  Large batches
     * keep uniform blocks (K0 + K2 take ~0.9 of K1's time there), ICW_TAPER overrides. */
    /* FIR converter: fused with the graph and render (KF2, one kernel per block) where its LDS fits;
     * else KF on its own stream (the caller's: K1's, idle without the IIR) beside K2.  KF2 needs no
     * block scratch and has no recurrence to pipeline against, so its blocks are as long as the
     * scratch bound allows (fewer launches, fewer partly filled waves of workgroups at their ends) */
    /* (per-stream lists: LP is the mixed program, its n_regs the largest of the call's streams; every
     * channel class present must fit) */
    const int fir_regs = LP.chain ? 0 : LP.n_regs;
    bool fir_fits = icw_fir_graph_lds(fir_M, fir_nt, (int)nch, fir_regs) > 0;
    if (fir && mix) {
        for (int k = 0; k < 2; ++k) fir_cls[k] = c->pid_cls[k];
        /* several converters: each class's launch is sized by the widest entry among its own streams */
        for (size_t i = 0; firmix && i < S; ++i) {
            IcwFirClass &fc = fir_cls[c->inputs.at(f0 + i).nch > 1 ? 1 : 0];
            fc.M = std::max(fc.M, (int32_t)c->firs.at(f0 + i).M);
            fc.nt = std::max(fc.nt, (int32_t)c->firs.at(f0 + i).nt);
        }
        for (int k = 0; k < 2; ++k) {
            const IcwFirClass &fc = fir_cls[k];
            if (fc.n > 0 && !icw_fir_graph_lds(firmix ? fc.M : fir_M, firmix ? fc.nt : fir_nt, k + 1, fir_regs)) fir_fits = false;
        }
    }
    fir_fused = fir && c->tn.fir_fuse && fir_fits && !LP.is_bus;
    /* The row kernel without a serial render (C2) has K2 at ~0.16 of K1r's time per frame: 65 536-frame
     * blocks (a quarter of the launches, of their gaps and prologues) ending in a steep tail
     * (65 536 -> 16 384 -> 4 096 -> 1 024: the drain stays one short K2) measured +0.8 % on C2
     * (3 170 -> 3 196 Msamples/s; 32 768 with r = 0.5 +0.5 %, 65 536 with no tail +0.5 %). */
    const bool row_long = !cw && k1_mode == 3 && !serial_render && !c->tn.block_env && n_frames >= 4 * kMaxBlockFrames;
    /* a dithered render with the flat shaper, rendered frame-parallel in the output kernel (K2 / KF2 /
     * K5) from K3a's dither rows (needs_serial) */
    dith_par = !serial_render && render_type != ICW_RENDER_ROUND;
    for (const auto &r : runs) dither = dither || r.e->dither;   /* K3a, serial or frame-parallel render: for the runs with a dithered entry */
    /* (with a dither generator, blocks of kMaxBlockFrames let K3a of the next block run beside KF2) */
    const bool fir_long = fir_fused && dev && !serial_render && !bus && !dith_par;
    Tb = std::min(n_frames, ((fir_fused || row_long) && !c->tn.block_env)
                                   ? (fir_long ? kMaxFirBlockFrames : kMaxBlockFrames) : c->tn.max_block);
    /* per-stream lists through the long FIR blocks: a slab per (list, rate) pair, so the blocks shorten
     * until the call's table fits kMaxMixTabDoubles */
    if (mix && fir_long && !c->tn.block_env && n_slabs > 0 && LP.n_trig > 0) {
        const size_t cap = kMaxMixTabDoubles / ((size_t)n_slabs * 2 * (size_t)LP.n_trig);
        Tb = std::min(Tb, std::max(kMaxBlockFrames, (int)std::min<size_t>(cap, (size_t)kMaxFirBlockFrames) & ~1023));
    }
    const double taper = c->tn.taper >= 0.0 ? c->tn.taper
                       : (!cw && k1_mode == 3) ? (serial_render ? kAutoTaper : (row_long ? kRowTaper : 0.0)) : 0.0;
    /* the fused FIR converter with a serial render (c5fir): the render of block 0 waits for its
     * converter and dither alone, so block 0 is short and the next ones ramp up (kFirRenderRamp:
     * profiles/r04_c5fir_timeline_after.txt had 2.2 ms of fill in a 24.3 ms step) */
    const bool fir_ramp = fir_fused && serial_render && !c->tn.block_env && c->tn.first_block > 0;
    blocks = fir_ramp ? plan_blocks(n_frames, Tb, c->tn.first_block_env ? c->tn.first_block : kFirRenderFirst, 0.0,
                                       c->tn.taper_min, c->tn.fir_ramp > 0.0 ? c->tn.fir_ramp : kFirRenderRamp)
                         : plan_blocks(n_frames, Tb, fir_fused ? 0 : c->tn.first_block, taper, c->tn.taper_min);
    n_blocks = (int)blocks.size();
    /* K5 (icw_stream1): one stream, one block, the row recurrence, register-form graph, ROUND / flat */
    s1 = c->tn.stream1 && count == 1 && n_blocks == 1 && !cw && !fcm && k1_mode == 3 && !serial_render &&
            !bus && n_frames <= ICW_S1_MAX && !xin;
    return ICW_OK;
}

/* where the kernels read the input and write the output: the caller's device buffers, or for host
 * pointers the staging pair (through pinned memory for a small call, block by block for pinned
 * caller buffers); the debug hooks' buffers */
int CallPlan::stage_io()
{
    /* a small host-pointer call stages through pinned memory (asynchronous copies, one wait) */
    stage_in = (size_t)n_frames * fsz * S;
    const size_t stage_out = (size_t)n_frames * osz * S;
    pinned = !dev && stage_in + stage_out + 16 <= kPinnedStage;
    /* pinned host buffers on a call of several launch blocks: each block's input slice goes in and
     * its output slice comes out on the copy stream, beside the other blocks' kernels */
    pipe_io = !dev && !pinned && n_blocks > 1 && !c->tn.serialize && !mixin && !mixr && host_pinned(in, c->device) &&
                 host_pinned(out, c->device);       /* (mixin, mixr: a block's slice differs per stream, one copy up front / at the end) */
    if (pinned) {
        if (c->h_stage_bytes < stage_in + stage_out + 16) {
            if (c->h_stage) (void)hipHostFree(c->h_stage);
            c->h_stage = nullptr;
            c->h_stage_bytes = 0;
            if (hipHostMalloc((void **)&c->h_stage, kPinnedStage, hipHostMallocDefault) != hipSuccess) return ICW_ENOMEM;
            c->h_stage_bytes = kPinnedStage;
            void *dp = nullptr;
            c->h_stage_dev = hipHostGetDevicePointer(&dp, c->h_stage, 0) == hipSuccess ? (unsigned char *)dp : nullptr;
            if (!c->h_stage_dev) (void)hipGetLastError();
        }
        zcopy = c->tn.zero_copy && c->h_stage_dev && !(flags & ICW_F_DEBUG_PRE);
    }
    if (dev) {
        d_in = (const unsigned char *)in;
        d_out = (unsigned char *)out;
        dis = in_stride;
        dos = out_stride;
    } else {
        const int rc = stage_host_io((size_t)n_frames * fsz, (size_t)n_frames * osz);
        if (rc != ICW_OK) return rc;
        if (pinned) {
            for (size_t i = 0; i < S; ++i)
                memcpy(c->h_stage + i * dis, (const unsigned char *)in + i * in_stride, dis);
            if (!zcopy && hipMemcpyAsync(c->d_in, c->h_stage, dis * S, hipMemcpyHostToDevice, st) != hipSuccess)
                return ICW_EDEVICE;
        } else if (!pipe_io && !stage_copy_in()) {
            return ICW_EDEVICE;
        }
        /* zero copy: K0 reads the staged input across PCIe and the last kernel writes the output
         * (and icw_advance the error flag) straight into the staging buffer -- a few KB, where the
         * two DMA transfers each cost a setup latency (the 576-frame drop-in) */
        if (zcopy) {
            d_in = c->h_stage_dev;
            d_out = c->h_stage_dev + stage_in;
        }
    }
    /* K5 on the zero-copy buffer: the kernel stores the call's sequence number after its output and
     * the host polls for it -- no completion signal and no waking of a waiting thread.  The word is
     * 4-byte aligned inside the output's 16 spare bytes, after the error flag. */
    s1_poll = s1 && zcopy && c->tn.spin_wait && !timing && !c->s1_stamps;
    done_off = ((stage_in + dos * S + sizeof(int) + 3) & ~(size_t)3) - stage_in;
    if (s1_poll) {
        if (++c->s1_seq == 0u) ++c->s1_seq;           /* 0 is never a call's number */
        s1_seq = c->s1_seq;
        /* the word sits in the reused staging buffer, where an earlier, larger call may have left
         * input or output bytes that happen to equal this call's number: store a value that cannot
         * match before the launch (which orders after this store), so the poll sees only the
         * kernel's own store */
        __atomic_store_n((uint32_t *)(c->h_stage + stage_in + done_off), ~s1_seq, __ATOMIC_RELEASE);
    }
    if (xin) {
        if (grow((void **)&c->d_xin, &c->d_xin_bytes, S * 2 * (size_t)n_frames * sizeof(double))) return ICW_ENOMEM;
        xin_phase.resize(S * 2);
        /* the device's Hilbert phases of the call's streams: [stream][L, R] */
        if (hipMemcpyAsync(xin_phase.data(), c->st.hq_phase + f0 * 2, S * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return ICW_EDEVICE;
    }
    if (flags & ICW_F_DEBUG_PRE) {
        if (!dbg) return ICW_EINVAL;
        if (dev) d_pre = (double *)dbg;
        else {
            if (grow((void **)&c->d_pre, &c->d_pre_bytes, S * (size_t)n_frames * 2 * sizeof(double))) return ICW_ENOMEM;
            d_pre = c->d_pre;
        }
    }
    return ICW_OK;
}

/* row pitches of the block scratch for blocks of at most Tb frames */
void CallPlan::set_pitches()
{
    w_pitch = (size_t)Tb + max_nord + 1;
    x_pitch = ((size_t)Tb + ICW_MAX_IIR_ORDER + 2) & ~(size_t)1;   /* look-ahead pad */
}

/* The encoders' plan: uniform launch blocks of at most max_block frames (no pipeline to fill or drain,
 * so as long as the scratch allows) on one scratch set, and the context's own list rather than a
 * per-stream table entry -- the encoders stop before the graph and read only its register count. */
void CallPlan::plan_uniform(int max_block)
{
    lp = &c->prog;
    dP = c->d_prog;
    ssr = (unsigned long long)c->cfg.sample_rate * ICW_HZ_SCALE;
    Tb = std::min(n_frames, c->tn.block_env ? c->tn.max_block : max_block);
    blocks = plan_blocks(n_frames, Tb, 0, 0.0, c->tn.taper_min);
    n_blocks = (int)blocks.size();
    n_sets = 1;
    set_pitches();
}

/* the block scratch of the call's n_sets sets (icw_prepare relies on this order of growth) */
int CallPlan::size_scratch()
{
    const IcwProg &LP = *lp;
    set_pitches();
    n_sets = std::min(n_blocks, c->tn.max_sets);
    if (mixh) {
        const int rc = prepare_hruns();
        if (rc != ICW_OK) return rc;
    }
    if (busmix) {
        const int rc = prepare_bus_runs();
        if (rc != ICW_OK) return rc;
    }
    for (int p = 0; p < n_sets && !fir_fused; ++p) {
        if (!cw && grow((void **)&c->w[p], &c->w_bytes[p], S * 4 * w_pitch * sizeof(double))) return ICW_ENOMEM;
        if (!din && grow((void **)&c->xd[p], &c->xd_bytes[p], S * 4 * x_pitch * sizeof(double))) return ICW_ENOMEM;
    }
    if (serial_render && !d_pre)
        for (int p = 0; p < n_sets; ++p)
            if (grow((void **)&c->rpre[p], &c->rpre_bytes[p], S * (size_t)Tb * 2 * sizeof(double))) return ICW_ENOMEM;
    /* the shared rotation table pays from two streams on; one stream computes its factors inline */
    table = LP.needs_omega && !bus && LP.n_trig > 0 && count > 1;
    in_step = table;
    for (int i = 1; in_step && i < count; ++i) in_step = c->nf_host[first + i] == c->nf_host[first];
    /* per-stream lists through KF2: a class is in step when each of its streams is in step with its
     * slab's reference stream (a stream without Shift / PM is its own reference) */
    if (mix && fir_fused) {
        size_t at = 0;
        for (IcwFirClass &fc : fir_cls) {
            bool ok = table && fc.trig;
            for (int j = 0; j < fc.n; ++j) {
                const size_t i = (size_t)c->pid_map[at + (size_t)j];
                ok = ok && c->pid_slab[i] >= 0 && c->nf_host[f0 + i] == c->nf_host[f0 + (size_t)c->pid_ref[i]];
            }
            fc.in_step = ok ? 1 : 0;
            at += (size_t)fc.n;
        }
    }
    /* per-stream lists: one slab per program that has one (prepare_mix), all of the widest one's pitch */
    slab_stride = (size_t)((Tb + 7) & ~7) * 2 * (size_t)LP.n_trig;
    if (table && grow((void **)&c->trig, &c->trig_bytes, (size_t)n_slabs * slab_stride * sizeof(double)))
        return ICW_ENOMEM;
    if (bus)
        for (int p = 0; p < n_sets; ++p)
            if (grow((void **)&c->iq[p], &c->iq_bytes[p], S * (size_t)Tb * 4 * sizeof(double))) return ICW_ENOMEM;
    if (dither)
        for (int p = 0; p < n_sets; ++p)
            if (grow((void **)&c->dith[p], &c->dith_bytes[p], S * 2 * (size_t)(Tb + 1) * sizeof(double))) return ICW_ENOMEM;
    if (dither) {
        /* chunk rows (a row of cap words holds icw_dith_chunk_frames frames of the call's draw, icw_device.h:
         * the one place the chunk length is worked out): 2^26 words (256 MB) shared among the G
         * generators, but never less than 1 024 frames of the widest draw (GAUSS, 24 words per sample)
         * and never more than the block's.  The floor wins over the 2^26 share from 2 731 generators on,
         * so the buffer is G * cap <= max(2^26, 24 576 G) words: 256 MB up to there, 96 KB per generator
         * beyond */
        const size_t G = S * 2;
        size_t cap = std::max<size_t>(((size_t)1 << 26) / G, (size_t)24 * 1024);
        cap = std::min(cap, (size_t)24 * (size_t)(Tb + 1));
        cap = (cap + 3) & ~(size_t)3;                      /* rows 16-byte aligned */
        if (grow((void **)&c->dwords, &c->dwords_bytes, G * cap * 4) ||
            grow((void **)&c->dbk, &c->dbk_bytes, G * ICW_DBK * 4) ||
            grow((void **)&c->dflag, &c->dflag_bytes, G * 4))
            return ICW_ENOMEM;
        c->dwcap = cap;
    }
    return ICW_OK;
}

/* Streams.  sK runs the IIR state kernel K1 (the serial, issue-bound one); sA runs the input
 * prep K0, the output kernel K2 and the serial graph / render; sD the dither generator.  When
 * K1 needs few CUs (4 waves per CU, one per SIMD) sK is confined to those CUs and sA / sD to
 * the rest, so the frame-parallel kernels never share a SIMD with a recurrence. */
int CallPlan::pick_streams()
{
    sK = st;
    sA = c->stream2;
    sD = c->stream3;
    sR = c->stream4;
    /* One launch block: K0 -> K1 -> K2 run in sequence anyway, so everything goes on the caller's
     * stream -- no cross-stream event waits, which cost the 576-frame drop-in call ~135 us (C1
     * p50 361 -> 226 us per call). */
    if (c->tn.serialize || n_blocks == 1) {
        sA = sD = sR = st;
    } else if (!cw) {
        /* plain K1: 128-lane groups of 32 streams (64 with the dedup); the variants: a lane per chain */
        const int k1_waves = mixh ? mixed_waves(k1_mode == 3)
                           : (k1_mode == 0 || k1_mode == ICW_K1_FC)
                                 ? ((count + (dedup ? 63 : 31)) / (dedup ? 64 : 32)) * 2 : row_waves;
        constexpr int kXcd = 8;                               /* MI355X: 8 XCDs */
        const int k1_cus = ((k1_waves + c->tn.k1_wpc - 1) / c->tn.k1_wpc + kXcd - 1) / kXcd * kXcd;
        if (c->tn.cu_split && k1_cus * 2 <= c->n_cu) {
            const CuSplit *cs = cu_split(c, k1_cus);
            if (!cs) return ICW_EDEVICE;
            sK = cs->k1;
            sA = cs->rest;
            sD = cs->dith;
            sR = cs->render;
            /* sF: an unmasked stream for the pipeline's fill and drain under the CU partition -- K0 of the
             * first block and K2 of the last run while no recurrence does, so they get the whole chip
             * instead of the partition's share (C3 / C4: the drain was one partitioned K2, ~5 % of a step) */
            if (c->tn.fill_drain) sF = c->stream2;
        }
    } else {
        /* complex input or the FIR converter: no recurrence kernel, so the dither generator runs after
         * the converter / output kernel on sA, beside the serial render of the previous block on sR.
         * On its own stream it shared a hardware queue with the render (4 queues per process,
         * GPU_MAX_HW_QUEUES, streams dealt round-robin): K3a of block b + 1 waited for the render of block b,
         * 1.2 of every 6.7 ms per c5fir block (profiles/r04_c5fir_timeline.txt).  With a frame-parallel
         * render (no render stream) it gets a stream of its own, ahead of the converter. */
        sD = dith_par ? c->stream3 : sA;
    }
    sC = pipe_io ? c->stream_io : nullptr;
    if (pipe_io && !grow_events(c->ev_io, n_blocks, hipEventDisableTiming)) return ICW_EDEVICE;
    /* every stream starts after everything already queued on st (inputs, previous calls); a call
     * whose kernels all run on st (one launch block: the drop-in) records no event -- the marker
     * packet sat in front of its kernel on the queue */
    bool other = false;
    for (hipStream_t x : {sK, sA, sD, sR, sF, sC}) other = other || (x && x != st);
    if (other && hipEventRecord(c->join, st) != hipSuccess)
        return ICW_EDEVICE;
    for (hipStream_t x : {sK, sA, sD, sR, sF, sC})
        if (x && x != st && hipStreamWaitEvent(x, c->join, 0) != hipSuccess) return ICW_EDEVICE;

    if (timing && (!grow_events(c->ev, 4 * n_blocks, hipEventDefault) || !grow_events(c->ev_k0, 2 * n_blocks, hipEventDefault)))
        return ICW_EDEVICE;
    fir_async = fir && !fir_fused && sK != sA;
    return ICW_OK;
}

/* K5: a one-stream call of one block (the drop-in's 576-frame calls, playback.c:619) runs its four
 * kernels as phases of one workgroup (icw_stream1): no launch gaps, one launch per call */
int CallPlan::run_stream1() const
{
    const IcwProg &LP = *lp;
    IcwS1Args a5;
    memset(&a5, 0, sizeof(a5));
    a5.k0 = k0_args(0);
    a5.k1 = k1_args(0);
    a5.k2 = k2_run_args(k2_args(0), hruns[0]);     /* one stream: one run */
    a5.adv = adv_args();
    a5.stamps = c->s1_stamps;
    a5.ovl = c->tn.s1_ovl ? 1 : 0;
    if (LP.needs_omega && LP.n_trig > 0 && !bus) {
        /* the one stream's rotation factors, computed by the kernel's idle waves beside the
         * recurrence: the output phase reads them instead of evaluating sin / cos per frame */
        if (grow((void **)&c->trig, &c->trig_bytes, (size_t)n_frames * 2 * LP.n_trig * sizeof(double)))
            return ICW_ENOMEM;
        a5.trig = trig_args(0);
        a5.has_trig = 1;
        a5.k2.trig_tab = c->trig;
        a5.k2.trig_pitch = a5.trig.trig_pitch;
    }
    if (dith_par) {
        /* the dithered flat render: K3a of the call's block first, on the same stream */
        const auto a3 = k3_args(0, a5.k2, runs[0]);
        if (icw_launch_dither(&a3, st) != hipSuccess) return ICW_EDEVICE;
        a5.k2.dith = a3.dith;
        a5.k2.dith_pitch = a3.dith_pitch;
    }
    if (timing && hipEventRecord(c->ev[0], st) != hipSuccess) return ICW_EDEVICE;
    if (icw_launch_stream1(&a5, hb->nord, st) != hipSuccess) return ICW_EDEVICE;
    if (timing && (hipEventRecord(c->ev[1], st) != hipSuccess || hipEventRecord(c->ev[2], st) != hipSuccess ||
                      hipEventRecord(c->ev[3], st) != hipSuccess))
        return ICW_EDEVICE;
    stereo_diverged();
    return ICW_OK;
}

/* pinned host input: block b's input slice of every stream goes in on the copy stream, and the
 * stream of the block's first reader (K0, KF or the fused KF2) waits for it */
int CallPlan::io_in(int b, hipStream_t s0) const
{
    if (!pipe_io) return ICW_OK;
    const int t0 = blocks[b].first, T = blocks[b].second;
    if (hipMemcpy2DAsync(c->d_in + (size_t)t0 * fsz, dis, (const unsigned char *)in + (size_t)t0 * fsz,
                         in_stride, (size_t)T * fsz, S, hipMemcpyHostToDevice, sC) != hipSuccess ||
        hipEventRecord(c->ev_io[b], sC) != hipSuccess || hipStreamWaitEvent(s0, c->ev_io[b], 0) != hipSuccess)
        return ICW_EDEVICE;
    return ICW_OK;
}

/* K0 (or the unfused converter KF) of block b */
int CallPlan::launch_k0(int b) const
{
    if (fir_fused) return ICW_OK;                   /* KF2 converts inside the block's kernel */
    if (din) return io_in(b, sA);                   /* K2 reads the frames itself: no kernel, no k0done to wait for */
    const int p = b % n_sets;
    if (b >= n_sets && !cw && sK != sA && hipStreamWaitEvent(sA, c->k1done[p], 0) != hipSuccess) return ICW_EDEVICE;
    hipStream_t s0 = (b == 0 && sF) ? sF : sA;         /* the fill: nothing else runs yet */
    /* the FIR converter runs on the caller's stream (K1's, idle without the IIR), so KF of the
     * next block overlaps K2 of this one; it rewrites xd[p] after K2(b - n_sets) has read it */
    if (fir_async) {
        s0 = sK;
        if (b >= n_sets && hipStreamWaitEvent(sK, c->k2done[p], 0) != hipSuccess) return ICW_EDEVICE;
    }
    if (io_in(b, s0) != ICW_OK) return ICW_EDEVICE;
    if (fir) {
        const auto af = fir_args(b);
        if (timing && hipEventRecord(c->ev[4 * b], s0) != hipSuccess) return ICW_EDEVICE;
        if (icw_launch_fir(&af, s0) != hipSuccess) return ICW_EDEVICE;
        if (timing && hipEventRecord(c->ev[4 * b + 1], s0) != hipSuccess) return ICW_EDEVICE;
    } else {
        if (timing && hipEventRecord(c->ev_k0[2 * b], s0) != hipSuccess) return ICW_EDEVICE;
        if (launch_unpack(b, s0) != hipSuccess) return ICW_EDEVICE;
        if (timing && hipEventRecord(c->ev_k0[2 * b + 1], s0) != hipSuccess) return ICW_EDEVICE;
    }
    /* test hook: this block's rows aside before K1 may start (K1 waits for k0done) */
    if (xin && hipMemcpy2DAsync(c->d_xin + blocks[b].first, (size_t)n_frames * sizeof(double), c->xd[p], x_pitch * sizeof(double),
                                   (size_t)blocks[b].second * sizeof(double), S * 2, hipMemcpyDeviceToDevice, s0) != hipSuccess)
        return ICW_EDEVICE;
    if (hipEventRecord(c->k0done[p], s0) != hipSuccess) return ICW_EDEVICE;
    return ICW_OK;
}

/* The block pipeline.  n_sets scratch sets (2 by default, ICW_SETS=3): K0 of the first n_sets blocks
 * is queued up front, K0(b + n_sets) as soon as its xd set is free (below); K1(b + n_sets) reuses the
 * w / info_dup set that K2(b) read and waits for it.  Three sets measured slower for large
 * batches (C3: K1 3.96 vs 3.16 ms per launch), so two is the default. */
int CallPlan::run_blocks() const
{
    int rc0 = ICW_OK;
    for (int b = 0; b < n_sets; ++b)
        if ((rc0 = launch_k0(b)) != ICW_OK) return rc0;
    for (int b = 0; b < n_blocks; ++b) {
        const int t0 = blocks[b].first, T = blocks[b].second, p = b % n_sets;

        if (!cw) {
            const auto a1 = k1_args(b);
            /* K0(b) done, and K2(b-2), the last reader of w[p] / info_dup[p] */
            if (sK != sA && hipStreamWaitEvent(sK, c->k0done[p], 0) != hipSuccess) return ICW_EDEVICE;
            if (b >= n_sets && sK != sA && hipStreamWaitEvent(sK, c->k2done[p], 0) != hipSuccess) return ICW_EDEVICE;
            if (timing && hipEventRecord(c->ev[4 * b], sK) != hipSuccess) return ICW_EDEVICE;
            if (launch_k1(a1, sK) != hipSuccess) return ICW_EDEVICE;
            if (timing && hipEventRecord(c->ev[4 * b + 1], sK) != hipSuccess) return ICW_EDEVICE;
            if (hipEventRecord(c->k1done[p], sK) != hipSuccess) return ICW_EDEVICE;
            if (sK != sA && hipStreamWaitEvent(sA, c->k1done[p], 0) != hipSuccess) return ICW_EDEVICE;
            /* real input: K0(b + n_sets) reuses xd[p], which K1(b) read; queued before K2(b) it
             * runs beside K1(b+1) instead of between two recurrences */
            if (b + n_sets < n_blocks && (rc0 = launch_k0(b + n_sets)) != ICW_OK) return rc0;
        } else if (timing && !fir) {
            if (hipEventRecord(c->ev[4 * b], sA) != hipSuccess || hipEventRecord(c->ev[4 * b + 1], sA) != hipSuccess)
                return ICW_EDEVICE;
        }

        /* the drain: K2 of the last block on the unmasked stream, after K1 of the block and K2 of
         * the one before it (the rotation table and the block order of the meters' owners) */
        const bool drain = sF && b == n_blocks - 1;
        hipStream_t s2 = drain ? sF : sA;
        if (drain && (hipStreamWaitEvent(sF, c->k1done[p], 0) != hipSuccess ||
                      (b >= 1 && hipStreamWaitEvent(sF, c->k2done[(b - 1) % n_sets], 0) != hipSuccess)))
            return ICW_EDEVICE;
        auto a2 = k2_args(b);
        if (table) {
            const auto at = trig_args(b);
            /* same stream as K2: the previous block's K2 has read the table before it is rewritten */
            if (icw_launch_trig_table(&at, s2) != hipSuccess) return ICW_EDEVICE;
            a2.trig_tab = c->trig;
            a2.trig_pitch = at.trig_pitch;
            a2.trig_perm_q = at.perm_q;
        }
        /* rpre[p] / iq[p] were last read by the serial render of block b - n_sets (on sR) */
        if (serial_render && b >= n_sets && sR != s2 && hipStreamWaitEvent(s2, c->k3done[p], 0) != hipSuccess)
            return ICW_EDEVICE;
        if (dith_par) {
            /* K3a of this block on its own stream (it depends only on the generators' state, so it runs
             * ahead, beside the converter / output kernel of the block before); dith[p] was last read
             * by the output kernel of block b - n_sets */
            const auto a3 = k3_args(b, a2, runs[0]);      /* (a frame-parallel render: one run) */
            if (b >= n_sets && sD != s2 && hipStreamWaitEvent(sD, c->k2done[p], 0) != hipSuccess) return ICW_EDEVICE;
            const hipError_t ed = icw_launch_dither(&a3, sD);
            if (ed != hipSuccess || hipEventRecord(c->ditdone[p], sD) != hipSuccess ||
                (sD != s2 && hipStreamWaitEvent(s2, c->ditdone[p], 0) != hipSuccess))
                return ICW_EDEVICE;
            a2.dith = a3.dith;
            a2.dith_pitch = a3.dith_pitch;
        }
        if (timing && hipEventRecord(c->ev[4 * b + 2], s2) != hipSuccess) return ICW_EDEVICE;
        if (fir_fused) {
            const auto af = fir_args(b);
            const auto ar = k2_run_args(a2, hruns[0]);      /* the converter's output: one run */
            if (io_in(b, s2) != ICW_OK) return ICW_EDEVICE;
            if (timing && hipEventRecord(c->ev[4 * b], s2) != hipSuccess) return ICW_EDEVICE;
            if ((mix ? icw_launch_fir_graph_mix(&af, &ar, fir_cls, 2, c->tn.fir_sig, s2)
                     : icw_launch_fir_graph(&af, &ar, in_step, c->tn.fir_sig, s2)) != hipSuccess)
                return ICW_EDEVICE;
            if (timing && hipEventRecord(c->ev[4 * b + 1], s2) != hipSuccess) return ICW_EDEVICE;
        } else {
            if (fir_async && hipStreamWaitEvent(s2, c->k0done[p], 0) != hipSuccess) return ICW_EDEVICE;
            if (din) {
                const auto ad = din_args();
                const auto ar = k2_run_args(a2, hruns[0]);  /* CWAVE input: one run */
                if (icw_launch_output_cw(&ar, &ad, s2) != hipSuccess) return ICW_EDEVICE;
            } else if (launch_k2(a2, s2) != hipSuccess) {
                return ICW_EDEVICE;
            }
        }
        if (hipEventRecord(c->k2done[p], s2) != hipSuccess) return ICW_EDEVICE;
        /* the serial part (K4, K3b) on sR after K2(b): it then overlaps K2(b+1) instead of
         * delaying it on sA */
        if (serial_render && sR != s2 && hipStreamWaitEvent(sR, c->k2done[p], 0) != hipSuccess) return ICW_EDEVICE;
        if (busmix) {
            const auto m4 = k4_mix_args(b, a2);
            if (icw_launch_graph_serial_mixed(&m4, bwgs, sR) != hipSuccess) return ICW_EDEVICE;
        } else if (bus) {
            const auto a4 = k4_args(b, a2);
            if (icw_launch_graph_serial(&a4, sR) != hipSuccess) return ICW_EDEVICE;
        }
        if (serial_render) {
            /* K3a of every run with a dithered entry on the dither stream (dith[p] was last read by the renders
             * of block b - n_sets), then on the render stream the serial runs in order and KR for every
             * frame-parallel stream.  A call with one render is the one run */
            if (dither) {
                if (b >= n_sets && sD != sR && hipStreamWaitEvent(sD, c->k3done[p], 0) != hipSuccess) return ICW_EDEVICE;
                for (const auto &r : runs) {
                    if (!r.e->dither) continue;
                    const auto a3 = k3_args(b, a2, r);
                    if (icw_launch_dither(&a3, sD) != hipSuccess) return ICW_EDEVICE;
                }
                if (hipEventRecord(c->ditdone[p], sD) != hipSuccess ||
                    (sD != sR && hipStreamWaitEvent(sR, c->ditdone[p], 0) != hipSuccess))
                    return ICW_EDEVICE;
            }
            for (const auto &r : runs) {
                if (!r.e->serial) continue;
                const auto a3 = k3_args(b, a2, r);
                if (icw_launch_render(&a3, sR) != hipSuccess) return ICW_EDEVICE;
            }
            if (any_par) {
                const auto ar = kr_args(b, a2);
                if (icw_launch_render_mixed(&ar, sR) != hipSuccess) return ICW_EDEVICE;
            }
            if (hipEventRecord(c->k3done[p], sR) != hipSuccess) return ICW_EDEVICE;
        }
        if (timing && hipEventRecord(c->ev[4 * b + 3], serial_render ? sR : s2) != hipSuccess) return ICW_EDEVICE;
        if (pipe_io) {
            /* this block's output slice, once its last writer (K2, or the serial render) is done */
            if (hipStreamWaitEvent(sC, serial_render ? c->k3done[p] : c->k2done[p], 0) != hipSuccess ||
                hipMemcpy2DAsync((unsigned char *)out + (size_t)t0 * osz, out_stride, d_out + (size_t)t0 * osz,
                                 dos, (size_t)T * osz, S, hipMemcpyDeviceToHost, sC) != hipSuccess)
                return ICW_EDEVICE;
        }
        /* complex input: K0(b + n_sets) reuses xd[p], which K2(b) read */
        if (cw && b + n_sets < n_blocks && (rc0 = launch_k0(b + n_sets)) != ICW_OK) return rc0;
    }
    stereo_diverged();
    /* join: the caller's stream continues after every kernel of the call, then the call-start
     * position / phases / frame counters advance (icw_advance) */
    for (hipStream_t x : {sK, sA, sD, sR, sF, sC})
        if (x && x != st && (hipEventRecord(c->join, x) != hipSuccess || hipStreamWaitEvent(st, c->join, 0) != hipSuccess))
            return ICW_EDEVICE;
    if (fir && !fir_hist_back()) return ICW_EDEVICE;
    return launch_advance() == hipSuccess ? ICW_OK : ICW_EDEVICE;
}

/* after the kernels: the host mirror of the frame counters, the results back to host pointers, the
 * debug hooks' copies, stamps and timing */
int CallPlan::finish_call() const
{
    for (int i = 0; i < count; ++i) {   /* icw_advance's arithmetic */
        unsigned long long &v = c->nf_host[first + i];
        const unsigned long long wrap = c->inputs.at(f0 + (size_t)i).ssr;    /* the stream's own (ssr while they are one) */
        v = c->cfg.frmod_scaled ? (v + (unsigned long long)n_frames) % wrap : v + (unsigned long long)n_frames;
    }
    if (legacy && hipStreamSynchronize(st) != hipSuccess) return ICW_EDEVICE;
    if (!dev) {
        unsigned char *h_out = pinned ? c->h_stage + stage_in : nullptr;
        if (pinned ? (!zcopy && hipMemcpyAsync(h_out, d_out, dos * S + sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess)
                      : (!pipe_io && !(mixr ? copy_out_own() : stage_copy_out(dos))))
            return ICW_EDEVICE;
        if (d_pre && hipMemcpyAsync(dbg, d_pre, S * (size_t)n_frames * 2 * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess)
            return ICW_EDEVICE;
        std::vector<double> rows;
        if (xin) {
            rows.resize(S * 2 * (size_t)n_frames);
            if (hipMemcpyAsync(rows.data(), c->d_xin, rows.size() * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess)
                return ICW_EDEVICE;
        }
        int e = 0;
        if (pinned) {
            if (s1_poll ? !poll_done((const uint32_t *)(h_out + done_off), s1_seq, st)
                           : hipStreamSynchronize(st) != hipSuccess)
                return ICW_EDEVICE;
            memcpy(&e, h_out + dos * S, sizeof(int));     /* the flag icw_advance copied */
            for (size_t i = 0; i < S; ++i) memcpy((unsigned char *)out + i * out_stride, h_out + i * dos, out_row_bytes(i));
        } else {
            if (hipStreamSynchronize(st) != hipSuccess) return ICW_EDEVICE;
            if (hipMemcpy(&e, c->st.err, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return ICW_EDEVICE;
        }
        if (e) return ICW_EDEVICE;
        if (xin) {
            /* the rows hold the channel's signed sample {x, -x, -x, x}[k] at Hilbert phase k (icw_store_frame):
             * the sign undone is x exactly; a mono call (R = L, the dedup writes the left row only) repeats L */
            if (hipStreamSynchronize(st) != hipSuccess) return ICW_EDEVICE;
            double *o = (double *)dbg;
            for (size_t i = 0; i < S; ++i)
                for (int ch = 0; ch < 2; ++ch) {
                    const int rc = nch > 1 ? ch : 0;
                    const double *r = rows.data() + (i * 2 + rc) * (size_t)n_frames;
                    for (int t = 0; t < n_frames; ++t) {
                        const unsigned k = (xin_phase[i * 2 + rc] + (unsigned)t) & 3u;
                        o[(i * (size_t)n_frames + t) * 2 + ch] = (k == 0u || k == 3u) ? r[t] : -r[t];
                    }
                }
        }
    }
    if (s1 && c->s1_stamps) {
        unsigned long long sp[8];
        if (hipStreamSynchronize(st) == hipSuccess && hipMemcpy(sp, c->s1_stamps, sizeof(sp), hipMemcpyDeviceToHost) == hipSuccess)
            fprintf(stderr, "icw_s1 %d %llu %llu %llu %llu %llu %llu\n", n_frames, sp[2] - sp[0], sp[3] - sp[1],
                    sp[4] - sp[2], sp[5] - sp[3], sp[6] - sp[4], sp[7] - sp[5]);
    }
    if (timing) {
        if (hipStreamSynchronize(st) != hipSuccess) return ICW_EDEVICE;
        double m1 = 0, m2 = 0;
        for (int b = 0; b < n_blocks; ++b) {
            float x = 0, y = 0;
            if (hipEventElapsedTime(&x, c->ev[4 * b], c->ev[4 * b + 1]) != hipSuccess ||
                hipEventElapsedTime(&y, c->ev[4 * b + 2], c->ev[4 * b + 3]) != hipSuccess)
                return ICW_EDEVICE;
            m1 += x;
            m2 += y;
        }
        /* K0 of every launch block (a K5 call, the FIR converter and K2's direct-input form launch none) */
        double m0 = 0;
        for (int b = 0; b < n_blocks && !s1 && !fir && !din; ++b) {
            float x = 0;
            if (hipEventElapsedTime(&x, c->ev_k0[2 * b], c->ev_k0[2 * b + 1]) != hipSuccess) return ICW_EDEVICE;
            m0 += x;
        }
        c->last_k0_ms = m0;
        c->last_ms[0] = m1;
        c->last_ms[1] = m2;
        c->last_launches[0] = c->last_launches[1] = n_blocks;
    }
    return hipGetLastError() == hipSuccess ? ICW_OK : ICW_EDEVICE;
}

/* The two encoders' shared opening: the argument check, then under the context's lock (lk, the caller's from
 * here on) the refusals of what no encoder serves, the call's plan and its input and format checks
 * (enc_format) for the encoder whose converter is the FIR one (fir) or the IIR.  Nothing has run when this
 * fails. */
int enc_begin(std::optional<CallPlan> &plan, std::unique_lock<std::mutex> &lk, bool fir, icw_ctx *c, int first, int count,
              const void *in, size_t in_stride, void *out, size_t out_stride, int n_frames, uint32_t cw_format, unsigned flags,
              void *hip_stream)
{
    if (!c || first < 0 || count <= 0 || first + count > c->n_streams || n_frames < 0 || !in || !out ||
        (flags & ~ICW_F_DEVICE_PTRS))
        return ICW_EINVAL;
    lk = std::unique_lock<std::mutex>(c->mu);
    if (c->inputs.size() > 1 && !c->enc_streams) return ICW_EUNSUPPORTED;   /* per-stream inputs: asked for (include/icw.h) */
    if (c->hilbs.size() > 1) return ICW_EUNSUPPORTED;                   /* per-stream Hilbert converters: not served */
    if (c->firs.size() > 1 && !c->enc_streams) return ICW_EUNSUPPORTED;    /* per-stream FIR converters: asked for, as inputs are */
    plan.emplace(c, first, count, in, in_stride, out, out_stride, n_frames, flags, hip_stream);
    return plan->enc_format(cw_format, (c->fir_M > 0) == fir);
}

}  // namespace

extern "C" {

int icw_process_streams(icw_ctx *c, int first, int count, const void *in, size_t in_stride, void *out,
                        size_t out_stride, int n_frames, unsigned flags, void *dbg, void *hip_stream)
{
    if (!c || first < 0 || count <= 0 || first + count > c->n_streams || n_frames < 0 || !in || !out)
        return ICW_EINVAL;
    if (n_frames == 0) return ICW_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    if (set_dev(c)) return ICW_EDEVICE;
    ++c->calls;
    c->last_dchunks = c->last_dchunk_frames = 0;
    CallPlan pl(c, first, count, in, in_stride, out, out_stride, n_frames, flags, hip_stream);
    pl.dbg = dbg;
    int rc;
    if ((rc = pl.join_legacy_stream()) != ICW_OK) return rc;
    if ((rc = pl.resolve_plan()) != ICW_OK) return rc;
    if ((rc = pl.stage_io()) != ICW_OK) return rc;
    if ((rc = pl.size_scratch()) != ICW_OK) return rc;
    if ((rc = pl.pick_streams()) != ICW_OK) return rc;
    if ((rc = pl.s1 ? pl.run_stream1() : pl.run_blocks()) != ICW_OK) return rc;
    return pl.finish_call();
}


/* ------------------------------------------------------------- CWAVE encoder (icw_cwave.h) -- */
int icw_cwave_frame_bytes(uint32_t cw_format, uint32_t channels)
{
    if (cw_format < ICW_FMT_CW_F64 || cw_format > ICW_FMT_CW_F32 || channels == 0) return 0;
    return (int)(fmt_size(cw_format) * (channels > 1 ? 2u : 1u));
}

/* The FIR converter's analytic signal as packed CWAVE frames (KFE).  The call shares icw_process_streams'
 * converter state -- the per-stream history (double-buffered by launch block, back in fir_hist[fir_par]
 * at the end) and the reader position -- and nothing else of the context.  Streams with different inputs
 * (icw_enable_stream_encode) run KFE's per-stream form; a call whose streams share one runs the kernels of a
 * one-input context. */
int icw_encode_cwave(icw_ctx *c, int first, int count, const void *in, size_t in_stride, void *out, size_t out_stride,
                     int n_frames, uint32_t cw_format, unsigned flags, void *hip_stream)
{
    std::unique_lock<std::mutex> lk;
    std::optional<CallPlan> plan;
    int rc = enc_begin(plan, lk, true, c, first, count, in, in_stride, out, out_stride, n_frames, cw_format, flags, hip_stream);
    if (rc != ICW_OK) return rc;
    CallPlan &pl = *plan;
    if (n_frames == 0) return ICW_OK;
    if (set_dev(c)) return ICW_EDEVICE;
    ++c->calls;
    if ((rc = pl.join_legacy_stream()) != ICW_OK) return rc;
    if ((rc = ensure_enc_clipped(c)) != ICW_OK) return rc;
    if ((rc = pl.enc_buffers()) != ICW_OK) return rc;
    if (!pl.dev && !pl.stage_copy_in()) return ICW_EDEVICE;
    pl.plan_uniform(kMaxFirBlockFrames);
    const int cwf = (int)(cw_format - ICW_FMT_CW_F64);
    for (int b = 0; b < pl.n_blocks; ++b)
        if (pl.launch_fir_encode(b, cwf) != hipSuccess) return ICW_EDEVICE;
    if (!pl.fir_hist_back()) return ICW_EDEVICE;
    if (icw_launch_enc_advance(c->st.pos + pl.f0, nullptr, count, (long long)n_frames, pl.st) != hipSuccess) return ICW_EDEVICE;
    if (pl.legacy && hipStreamSynchronize(pl.st) != hipSuccess) return ICW_EDEVICE;
    if (!pl.dev && (!pl.enc_copy_out() || hipStreamSynchronize(pl.st) != hipSuccess)) return ICW_EDEVICE;
    return hipGetLastError() == hipSuccess ? ICW_OK : ICW_EDEVICE;
}

/* The quadrature IIR converter's analytic signal as packed CWAVE frames.  Per launch block the kernels of
 * a process call up to the graph -- K0, the K1 the context would pick, K2 with iq_out set (it stops at
 * the `in` rows: no graph, no render, no meters) -- then the packer KIP.  The recurrence bounds the call
 * and nothing of a block can start before the block's K1 has ended, so the four run in sequence on the
 * caller's stream with one scratch set; the call shares icw_process_streams' converter state (rings,
 * phases, de-subnorm counters, lr_equal) and the reader position, and nothing else of the context.
 * Streams with different inputs (icw_enable_stream_encode) take what a mixed-input process call takes --
 * the table-reading K0, the same K1, K2's per-stream instances -- and KIP's per-stream form. */
int icw_encode_cwave_iir(icw_ctx *c, int first, int count, const void *in, size_t in_stride, void *out, size_t out_stride,
                         int n_frames, uint32_t cw_format, unsigned flags, void *hip_stream)
{
    std::unique_lock<std::mutex> lk;
    std::optional<CallPlan> plan;
    int rc = enc_begin(plan, lk, false, c, first, count, in, in_stride, out, out_stride, n_frames, cw_format, flags, hip_stream);
    if (rc != ICW_OK) return rc;
    CallPlan &pl = *plan;
    const size_t S = pl.S;
    /* FC() arithmetic changes the values: refused, so K1 / K2 take no census (fes null, fcm false) */
    if (c->cfg.fp_check) return ICW_EUNSUPPORTED;
    if (n_frames == 0) return ICW_OK;
    if (set_dev(c)) return ICW_EDEVICE;
    /* the K1 of a process call over these streams */
    pl.pick_k1();
    pl.plan_uniform(kMaxBlockFrames);
    if (pl.mixin && (rc = pl.enc_mix_lists()) != ICW_OK) return rc;
    if ((rc = ensure_enc_clipped(c)) != ICW_OK) return rc;
    if (grow((void **)&c->w[0], &c->w_bytes[0], S * 4 * pl.w_pitch * sizeof(double)) ||
        grow((void **)&c->xd[0], &c->xd_bytes[0], S * 4 * pl.x_pitch * sizeof(double)) ||
        grow((void **)&c->iq[0], &c->iq_bytes[0], S * (size_t)pl.Tb * 4 * sizeof(double)))
        return ICW_ENOMEM;
    if ((rc = pl.enc_buffers()) != ICW_OK) return rc;
    /* counted only now that the allocations succeeded: an early ICW_ENOMEM leaves icw_prepare usable */
    ++c->calls;
    c->last_k1 = pl.k1_mode;
    if ((rc = pl.join_legacy_stream()) != ICW_OK) return rc;
    if (!pl.dev && !pl.stage_copy_in()) return ICW_EDEVICE;
    const DevState &ds = c->st;
    const int cwf = (int)(cw_format - ICW_FMT_CW_F64);
    for (int b = 0; b < pl.n_blocks; ++b) {
        if (pl.launch_unpack(b, pl.st) != hipSuccess) return ICW_EDEVICE;
        const auto a1 = pl.k1_args(b);
        if (pl.launch_k1(a1, pl.st) != hipSuccess) return ICW_EDEVICE;
        const auto a2 = pl.enc_k2_args(b);
        if (pl.launch_k2(a2, pl.st) != hipSuccess) return ICW_EDEVICE;
        if (pl.launch_pack(b, cwf) != hipSuccess) return ICW_EDEVICE;
    }
    pl.stereo_diverged();
    if (icw_launch_enc_advance(ds.pos + pl.f0, ds.hq_phase + pl.f0 * 2, count, (long long)n_frames, pl.st) != hipSuccess)
        return ICW_EDEVICE;
    if (pl.legacy && hipStreamSynchronize(pl.st) != hipSuccess) return ICW_EDEVICE;
    if (!pl.dev) {
        if (!pl.enc_copy_out() || hipStreamSynchronize(pl.st) != hipSuccess) return ICW_EDEVICE;
        int e = 0;
        if (hipMemcpy(&e, ds.err, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess || e) return ICW_EDEVICE;
    }
    return hipGetLastError() == hipSuccess ? ICW_OK : ICW_EDEVICE;
}

int icw_encode_clipped(icw_ctx *c, int s, int reset, uint64_t *clipped)
{
    if (!c || s < 0 || s >= c->n_streams) return ICW_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    unsigned long long v = 0;
    if (c->enc_clipped) {
        if (set_dev(c) || quiesce(c) != hipSuccess) return ICW_EDEVICE;
        if (hipMemcpy(&v, c->enc_clipped + s, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return ICW_EDEVICE;
        if (reset && hipMemset(c->enc_clipped + s, 0, sizeof(v)) != hipSuccess) return ICW_EDEVICE;
    }
    if (clipped) *clipped = v;
    return ICW_OK;
}

/* Warm-up of a fresh context (include/icw.h): one call of n_frames frames of digital silence through
 * the path the context's configuration takes, then the fresh state back (icw_stream_init is exactly
 * the state icw_create leaves).  What the first call would otherwise pay happens here: the pinned
 * staging buffer, the device buffers (sized for the widest frame, so a later track's format does
 * not grow them) and the lazy load of the kernels' code objects on the first launch.  The drop-in
 * measured 7 ms for its first 576-frame block (BENCH_r03 C1 block_latency_us.first), against
 * ~113 us for the others. */
int icw_prepare(icw_ctx *c, int n_frames)
{
    if (!c || n_frames < 0) return ICW_EINVAL;
    if (n_frames == 0) n_frames = ICW_S1_MAX;
    const size_t S = (size_t)c->n_streams;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if (c->calls || c->touched) return ICW_EINVAL;   /* would have to restore state it cannot know */
        if (set_dev(c)) return ICW_EDEVICE;
        const size_t widest = 2 * fmt_size(ICW_FMT_CW_F64), osz = 2 * 3;
        if (grow((void **)&c->d_in, &c->d_in_bytes, (size_t)n_frames * widest * S) ||
            grow((void **)&c->d_out, &c->d_out_bytes, (size_t)n_frames * osz * S + 16))
            return ICW_ENOMEM;
    }
    /* rows of the widest frame among the streams' inputs (one input: the context's frame) */
    unsigned fsz = 0;
    for (const IcwInDesc &d : c->inputs.ents) fsz = std::max(fsz, d.fsz);
    const size_t osz = 2 * (size_t)icw_render_size(c), row = (size_t)n_frames * fsz;
    std::vector<unsigned char> in(row * S, 0), out((size_t)n_frames * osz * S);
    for (size_t i = 0; i < S; ++i)
        if (c->inputs.at(i).fmt == ICW_FMT_U8) std::fill(in.begin() + i * row, in.begin() + (i + 1) * row, (unsigned char)0x80);   /* u8 silence */
    int rc = icw_process_streams(c, 0, (int)S, in.data(), (size_t)n_frames * fsz, out.data(), (size_t)n_frames * osz,
                                 n_frames, 0u, nullptr, nullptr);
    if (rc == ICW_OK) rc = icw_stream_init(c, 0, (int)S);
    std::lock_guard<std::mutex> lk(c->mu);
    c->calls = 0;
    return rc;
}

int icw_process_batch(icw_ctx *c, const void *in, size_t in_stride, void *out, size_t out_stride, int n_frames,
                      unsigned flags, void *dbg, void *hip_stream)
{
    if (!c) return ICW_EINVAL;
    return icw_process_streams(c, 0, c->n_streams, in, in_stride, out, out_stride, n_frames, flags, dbg, hip_stream);
}

}  /* extern "C" */
