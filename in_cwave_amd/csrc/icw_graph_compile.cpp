/*
 * icw_graph_compile.cpp -- the DSP list as the device runs it, and the render's constants: list
 * normalisation (graph_accept), the register and bus forms (build_prog), sound_render_recalc's
 * arithmetic (render_consts) and what a configuration needs of the render (needs_serial,
 * needs_render_state).  Host arithmetic only: no HIP call, no context.
 */
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "icw_graph_compile.h"
#include "icw_tables.inc"

/* bytes per channel sample: HRW_FMT_* (xwave_reader.c:553-580), CWAVE cw_slen (xwave_reader.c:246-252) */
unsigned fmt_size(unsigned fmt)
{
    static const unsigned sz[9] = {1, 2, 3, 4, 4, 16, 4, 6, 8};
    return fmt < 9 ? sz[fmt] : 0;
}

/* amod_init (adv_modulator.c:216-331): accept the list only if its head is the one and only
 * Master and every mode is known; apply the L/R locks.  Otherwise the default Master. */
bool graph_accept(std::vector<icw_node> &n)
{
    if (n.empty() || n[0].mode != ICW_MODE_MASTER) return false;
    bool was_master = false;
    for (auto &t : n) {
        if (t.lock_gain) { t.gain[1] = t.gain[0]; t.iq_invert[1] = t.iq_invert[0]; }
        switch (t.mode) {
        case ICW_MODE_MASTER:
            if (was_master) return false;
            was_master = true;
            break;
        case ICW_MODE_SHIFT:
            if (t.lock_shift) {
                t.fr_shift[1] = t.sign_lock_shift ? -t.fr_shift[0] : t.fr_shift[0];
                t.is_shift[1] = t.is_shift[0];
            }
            break;
        case ICW_MODE_PM:
            if (t.lock_freq) { t.pm_freq[1] = t.pm_freq[0]; t.is_pm[1] = t.is_pm[0]; }
            if (t.lock_phase) t.pm_phase[1] = t.pm_phase[0];
            if (t.lock_level) t.pm_level[1] = t.pm_level[0];
            if (t.lock_angle) t.pm_angle[1] = t.pm_angle[0];
            break;
        case ICW_MODE_MIX:
            break;
        default:
            return false;
        }
    }
    return true;
}

icw_node default_master()
{
    icw_node n;
    memset(&n, 0, sizeof(n));
    n.mode = ICW_MODE_MASTER;
    n.gain[0] = n.gain[1] = 0.8;           /* DEF_GAIN_MASTER, in_cwave.h:167 */
    n.tout[0] = n.tout[1] = ICW_S_ADD_REIM;
    n.inputs[0] = 1;                       /* adv_modulator.c:112-118 */
    n.lock_gain = 1;
    return n;
}

namespace {

/* DGET_SCALED_FR (adv_modulator.c:35-39) */
double scaled_fr(double f) { return (double)((unsigned)(f * ((double)ICW_HZ_SCALE) + 0.5)); }

/* Compile the normalised DSP list into register form.  Execution order is tail -> head
 * (adv_modulator.c:637).  Each input slot resolves to the value most recently written in the
 * same frame; a slot never written by any node reads its persistent bus value.  A slot read
 * before its writer runs (a one-frame delay, doc 3.1) is not yet on the device path. */
/* per-op parameters shared by the register and bus forms */
void op_params(const icw_node &n, IcwOp &op)
{
    op.mode = n.mode;
    op.wb_slot = -1;
    op.xch = n.xch_mode;
    op.iqinv[0] = n.iq_invert[0];
    op.iqinv[1] = n.iq_invert[1];
    op.gain[0] = n.gain[0];
    op.gain[1] = n.gain[1];
    op.unit_gain[0] = op.gain[0] == 1.0;
    op.unit_gain[1] = op.gain[1] == 1.0;
    op.out_slot = n.mode == ICW_MODE_MASTER ? 0 : n.n_out;
    op.in_mask = 0;
    for (int k = 0; k < ICW_N_INPUTS; ++k)
        if (n.inputs[k]) op.in_mask |= 1u << k;
    for (int c = 0; c < 2; ++c) {
        op.tout[c] = n.tout[c];
        if (n.mode == ICW_MODE_SHIFT) {
            op.act[c] = n.is_shift[c];
            double f = n.fr_shift[c];
            op.neg[c] = f < 0.0;
            if (f < 0.0) f = -f;
            op.f[c] = f;   /* scaled below if frmod_scaled */
        } else if (n.mode == ICW_MODE_PM) {
            op.act[c] = n.is_pm[c];
            op.f[c] = n.pm_freq[c];
            op.pp[c] = n.pm_phase[c] * ICW_PI_H;              /* fphase * PI */
            op.lp[c] = n.pm_level[c] * ICW_PI_H;              /* flevel * PI */
            op.fa[c] = n.pm_angle[c];
        }
    }
}

/* norm_omega is only read by active Shift / PM nodes (adv_modulator.c:519-583): frame-parallel
 * kernels skip the counter arithmetic and its division otherwise */
void set_needs_omega(IcwProg &P)
{
    P.needs_omega = 0;
    P.n_trig = 0;
    for (int i = 0; i < P.n_ops; ++i) {
        IcwOp &op = P.ops[i];
        op.tslot[0] = op.tslot[1] = -1;
        if (op.mode != ICW_MODE_SHIFT && op.mode != ICW_MODE_PM) continue;
        for (int c = 0; c < 2; ++c)
            if (op.act[c]) {
                op.tslot[c] = P.n_trig++;     /* a column of the per-frame rotation table */
                P.needs_omega = 1;
            }
    }
}

/* Bus form: the list as the reference runs it (tail -> head, or the head alone when bypassed) */
int compile_bus(const std::vector<icw_node> &nodes, int bypass, IcwProg &P)
{
    memset(&P, 0, sizeof(P));
    P.is_bus = 1;
    P.bypass = bypass;
    std::vector<int> order;
    if (bypass) order.push_back(0);
    else for (int i = (int)nodes.size() - 1; i >= 0; --i) order.push_back(i);
    if ((int)order.size() > ICW_MAX_OPS) return ICW_EUNSUPPORTED;
    for (size_t oi = 0; oi < order.size(); ++oi) {
        const icw_node &n = nodes[order[oi]];
        if (n.mode != ICW_MODE_MASTER && (n.n_out < 1 || n.n_out >= ICW_N_INPUTS)) return ICW_EGRAPH;
        op_params(n, P.ops[oi]);
    }
    P.n_ops = (int)order.size();
    P.n_regs = 1;
    set_needs_omega(P);
    return ICW_OK;
}

/* Register form for the frame-parallel output kernel; ICW_EUNSUPPORTED when a slot is read
 * before it is written in the frame (one-frame delay) or the list exceeds the register budget --
 * the caller then compiles the bus form.
 *
 * Value registers live in K2's LDS (8 KB each per 256-frame workgroup), so they are allocated by
 * liveness: `in` is register 0 for the frame; a node's output takes the lowest register whose value
 * has had its last reader (an op may write over its own inputs: it reads them all first); a slot
 * read but never written in the frame is loaded once per workgroup and keeps its register.  A
 * written slot's final value goes to the persistent bus from the op that writes it (wb_slot), at
 * the block's last frame, so it need not stay live to the end.  PM -> Shift -> Mix -> Master
 * (C4) takes 2 registers instead of 4, which lets K2 keep 4 waves per SIMD. */
int compile_graph(const std::vector<icw_node> &nodes, int bypass, IcwProg &P)
{
    memset(&P, 0, sizeof(P));
    P.bypass = bypass;
    std::vector<int> order;
    if (bypass) order.push_back(0);
    else for (int i = (int)nodes.size() - 1; i >= 0; --i) order.push_back(i);
    if ((int)order.size() > ICW_MAX_REG_OPS) return ICW_EUNSUPPORTED;
    const int n_ops = (int)order.size();

    bool written_any[ICW_N_INPUTS] = {false};
    for (int i : order)
        if (nodes[i].mode != ICW_MODE_MASTER) {
            const int o = nodes[i].n_out;
            if (o < 0 || o >= ICW_N_INPUTS) return ICW_EGRAPH;
            written_any[o] = true;
        }
    /* values: 0 = `in`, then persistent slots and op outputs in order of appearance */
    std::vector<int> last_use(1, -1), def_op(1, -1);
    std::vector<char> pinned(1, 0);
    std::vector<std::vector<int>> reads(n_ops);
    std::vector<int> out_val(n_ops, -1);
    int cur[ICW_N_INPUTS];
    for (int k = 0; k < ICW_N_INPUTS; ++k) cur[k] = -1;
    cur[0] = 0;
    std::vector<int> persist_val, persist_slot;
    for (int oi = 0; oi < n_ops; ++oi) {
        const icw_node &n = nodes[order[oi]];
        if (!bypass) {
            for (int k = 0; k < ICW_N_INPUTS; ++k) {
                if (!n.inputs[k]) continue;
                int v = cur[k];
                if (v < 0) {
                    if (written_any[k]) return ICW_EUNSUPPORTED;   /* delayed (feedback) read */
                    v = (int)last_use.size();
                    last_use.push_back(-1);
                    def_op.push_back(-1);
                    pinned.push_back(1);
                    persist_val.push_back(v);
                    persist_slot.push_back(k);
                    cur[k] = v;
                }
                reads[oi].push_back(v);
                last_use[v] = oi;
            }
        }
        if (n.mode != ICW_MODE_MASTER) {
            const int v = (int)last_use.size();
            last_use.push_back(-1);
            def_op.push_back(oi);
            pinned.push_back(0);
            out_val[oi] = v;
            cur[n.n_out] = v;
        }
    }
    /* the op that leaves each written slot its final value */
    std::vector<int> wb(n_ops, -1);
    for (int k = 0; k < ICW_N_INPUTS; ++k)
        if (written_any[k] && cur[k] >= 0) wb[def_op[cur[k]]] = k;
    /* physical registers */
    std::vector<int> phys(last_use.size(), -1), holder(ICW_MAX_REGS, -1);
    phys[0] = 0;
    holder[0] = 0;
    for (size_t q = 0; q < persist_val.size(); ++q) {
        int r = 1;
        while (r < ICW_MAX_REGS && holder[r] >= 0) ++r;
        if (r >= ICW_MAX_REGS) return ICW_EUNSUPPORTED;
        phys[persist_val[q]] = r;
        holder[r] = persist_val[q];
    }
    int n_regs = 1 + (int)persist_val.size();
    for (int oi = 0; oi < n_ops; ++oi) {
        IcwOp &op = P.ops[oi];
        const icw_node &n = nodes[order[oi]];
        op.mode = n.mode;
        for (int v : reads[oi]) op.in_reg[op.n_in++] = phys[v];
        op_params(n, op);
        op.wb_slot = wb[oi];
        /* free the registers whose values were read for the last time by this op */
        for (int r = 0; r < ICW_MAX_REGS; ++r) {
            const int v = holder[r];
            if (v >= 0 && !pinned[v] && last_use[v] <= oi) holder[r] = -1;
        }
        if (out_val[oi] >= 0) {
            int r = 0;
            while (r < ICW_MAX_REGS && holder[r] >= 0) ++r;
            if (r >= ICW_MAX_REGS) return ICW_EUNSUPPORTED;
            phys[out_val[oi]] = r;
            holder[r] = out_val[oi];
            op.out_reg = r;
            n_regs = std::max(n_regs, r + 1);
        }
    }
    P.n_ops = n_ops;
    P.n_regs = n_regs;
    for (size_t q = 0; q < persist_val.size(); ++q) {
        P.persist_reg[q] = phys[persist_val[q]];
        P.persist_slot[q] = persist_slot[q];
    }
    P.n_persist = (int)persist_val.size();
    /* chain program (C2's Shift -> Master, C4's PM -> Shift -> Mix(in + B) -> Master): every op reads
     * only `in` and / or the output of the op just before it.  Reads are in slot order and `in` is
     * slot 0, so the sum is 0.0 + in + prev in the reference's order (adv_modulator.c:655-665) */
    P.chain = P.n_persist == 0 ? 1 : 0;
    for (int oi = 0; oi < n_ops && P.chain; ++oi) {
        int bits = 0;
        for (int v : reads[oi]) {
            if (v == 0 && !(bits & 1) && !(bits & 2)) bits |= 1;
            else if (oi > 0 && v == out_val[oi - 1] && v >= 0 && !(bits & 2)) bits |= 2;
            else P.chain = 0;
        }
        P.ops[oi].chain_in = bits;
    }
    /* the signature of a chain of plain ops (the device runs it straight, icw_chain_sig): no channel
     * exchange or I/Q swap, both channels of a Shift / PM rotating, a Master summing re + im */
    P.sig = 0;
    bool plain = P.chain && n_ops <= 6;
    for (int oi = 0; oi < n_ops && plain; ++oi) {
        const IcwOp &op = P.ops[oi];
        plain = op.xch == ICW_XCH_NORMAL && !op.iqinv[0] && !op.iqinv[1];
        if (op.mode == ICW_MODE_MASTER) plain &= op.tout[0] == ICW_S_ADD_REIM && op.tout[1] == ICW_S_ADD_REIM;
        else if (op.mode != ICW_MODE_MIX) plain &= op.act[0] && op.act[1];
    }
    if (plain) {
        P.sig = n_ops;
        for (int oi = 0; oi < n_ops; ++oi) P.sig |= ((P.ops[oi].mode & 3) | (P.ops[oi].chain_in << 2)) << (4 + 4 * oi);
        /* bit 30: every op but the Master has gain 1.0 on both channels (ICW_SIG_UNIT) */
        bool unit = true;
        for (int oi = 0; oi < n_ops; ++oi)
            if (P.ops[oi].mode != ICW_MODE_MASTER) unit &= P.ops[oi].gain[0] == 1.0 && P.ops[oi].gain[1] == 1.0;
        if (unit) P.sig |= ICW_SIG_UNIT;
    }
    set_needs_omega(P);
    return ICW_OK;
}

}  // namespace

/* sound_render_recalc arithmetic (sound_render.c:499-581); spec: the row render's clamp-free blocks
 * (IcwTuning.k3r_spec) */
void render_consts(const icw_render_cfg &cfg, int is24, bool spec, IcwRenderK &k)
{
    memset(&k, 0, sizeof(k));
    k.dth_mul = pow(2.0, cfg.dth_bits) - 1.0;
    if (cfg.quantz_type == ICW_QUANTZ_MID_TREAD) { k.round_offset = 0.5; k.sign_delta = 0; }
    else { k.round_offset = 0.0; k.sign_delta = -1; }
    if (is24) {
        long long hib = 0x800000LL;
        k.norm_shift = 24 - (int)cfg.sign_bits24;
        hib >>= k.norm_shift;
        k.hi = (double)hib;
        k.lo = -(double)(hib + 1 + k.sign_delta);
        k.norm_mul = (k.norm_shift < 8) ? (double)(0x100 >> k.norm_shift)
                                         : 1.0 / (double)(1ULL << (k.norm_shift - 8));
    } else {
        long long hib = 0x8000LL;
        k.norm_shift = 16 - (int)cfg.sign_bits16;
        hib >>= k.norm_shift;
        k.hi = (double)hib;
        k.lo = -(double)(hib + 1 + k.sign_delta);
        k.norm_mul = 1.0 / (double)(1ULL << k.norm_shift);
    }
    k.lo -= (double)k.sign_delta;
    k.clip_abs = std::min(k.hi, -k.lo);
    k.lo1 = (int32_t)k.lo + 1;
    k.hi1 = (int32_t)k.hi - 1;
    k.unit_mul = k.norm_mul == 1.0;
    k.is24 = is24;
    k.render_type = (int)cfg.render_type;
    unsigned t = cfg.nshape_type > ICW_NSHAPE_MAX ? ICW_NSHAPE_FLAT : cfg.nshape_type;
    k.ns_kind = icw_ns_kind[t];
    k.ns_n = icw_ns_n[t];
    const int nc = k.ns_kind == 2 ? 2 * k.ns_n : k.ns_n;
    for (int i = 0; i < nc; ++i) k.ns_c[i] = u2d(icw_ns_c[t][i]);
    /* the row render's clamp-free blocks (icw_render_rowc).  Without a clip the error fed back is small: with
     * q = input + d and the integer trunc(q) + delta (mid-riser) or trunc(q +- 0.5) (mid-tread),
     * |ev| = |(double)val - input| <= 1.5 + Dm, Dm the largest |rnd * dth_mul| of the render type
     * (sound_render.c:711-751: RPDF |dsopen| / SQRT2 < 0.708, TPDF and STPDF < 1, GAUSS 12 / (2 SQRT6)
     * < 2.45), so a FIR shaper's output |prev_ns_err| <= B (1.5 + Dm), B = sum |c_i|.  A block whose
     * inputs all have |x * norm_mul| <= spec_thr, after a block without a clip (so the shaper history
     * holds only such errors), then has |q| <= spec_thr + B (1.5 + Dm) + Dm + 0.5 < clip_abs for every
     * sample: nothing clips and the clamp is the identity, so the block runs without it.  The IIR
     * shaper feeds back its own output: never. */
    k.spec_thr = -1.0;
    if (spec && k.ns_kind != 2 && cfg.render_type <= ICW_RENDER_GAUSS) {
        static const double cdm[5] = {0.0, 0.708, 1.0, 1.0, 2.45};
        double B = 0.0;
        if (k.ns_kind == 1)
            for (int i = 0; i < k.ns_n; ++i) B += fabs(k.ns_c[i]);
        const double Dm = cfg.render_type == ICW_RENDER_ROUND ? 0.0 : fabs(k.dth_mul) * cdm[cfg.render_type];
        const double thr = k.clip_abs - B * (1.5 + Dm) * 1.001 - Dm - 0.5 - 1.0;
        if (thr > 0.0) k.spec_thr = thr;             /* NaN / inf dth_mul: never */
    }
}

/* The normalised list (graph_accept) as the device program: register form, or the bus form when a
 * slot is read before its writer runs.  With frmod_scaled the PM frequencies are scaled from f
 * (dsp_pm) and the Shift ones from |f| (dsp_shift), as DGET_SCALED_FR does per frame. */
int build_prog(const icw_config &cfg, std::vector<icw_node> nodes, IcwProg &P)
{
    /* by value: the context keeps the list as given (unscaled), so that the list primitives can edit
     * and recompile it */
    if (cfg.frmod_scaled)
        for (auto &n : nodes)
            if (n.mode == ICW_MODE_PM)
                for (int ch = 0; ch < 2; ++ch) n.pm_freq[ch] = scaled_fr(n.pm_freq[ch]);
    int rc = compile_graph(nodes, cfg.bypass_list, P);
    if (rc == ICW_EUNSUPPORTED) rc = compile_bus(nodes, cfg.bypass_list, P);
    if (rc) return rc;
    if (cfg.frmod_scaled)
        for (int i = 0; i < P.n_ops; ++i)
            if (P.ops[i].mode == ICW_MODE_SHIFT)
                for (int ch = 0; ch < 2; ++ch) P.ops[i].f[ch] = scaled_fr(P.ops[i].f[ch]);
    return ICW_OK;
}

/* The bus form of any accepted list, also of one build_prog compiles to the register form: a register-form
 * list is a valid input to the reference's per-frame loop too, which K4 runs.  A call over streams of both
 * forms runs every stream in this one (ListEnt's twin). */
int build_prog_bus(const icw_config &cfg, std::vector<icw_node> nodes, IcwProg &P)
{
    if (cfg.frmod_scaled)
        for (auto &n : nodes)
            if (n.mode == ICW_MODE_PM)
                for (int ch = 0; ch < 2; ++ch) n.pm_freq[ch] = scaled_fr(n.pm_freq[ch]);
    const int rc = compile_bus(nodes, cfg.bypass_list, P);
    if (rc) return rc;
    if (cfg.frmod_scaled)
        for (int i = 0; i < P.n_ops; ++i)
            if (P.ops[i].mode == ICW_MODE_SHIFT)
                for (int ch = 0; ch < 2; ++ch) P.ops[i].f[ch] = scaled_fr(P.ops[i].f[ch]);
    return ICW_OK;
}

/* The runs of the mixed K4 (IcwK4Run): streams [0, count) of a call, stream i on list entry ent[i], cut into
 * the maximal runs of consecutive streams on one entry.  A run takes whole one-wave workgroups of 64 lanes,
 * so no wave holds two runs; wg0 ascends.  Returns the launch's workgroups; *W is the lanes a row of the
 * LDS bus must hold -- the widest run's lanes in a workgroup, min(64, n) -- rounded up to a power of two, so
 * that a row starts at a multiple of its own length and a half-wave's 32 consecutive doubles fall on the 64
 * banks once, as K4's 64-lane rows do. */
int icw_k4_cut_runs(const int32_t *ent, int count, std::vector<IcwK4Run> &runs, int *W)
{
    runs.clear();
    int wg = 0, widest = 0;
    for (int i = 0; i < count;) {
        int j = i + 1;
        while (j < count && ent[j] == ent[i]) ++j;
        runs.push_back(IcwK4Run{wg, i, j - i, ent[i]});
        wg += (j - i + 63) / 64;
        widest = std::max(widest, std::min(64, j - i));
        i = j;
    }
    int w = 1;
    while (w < widest) w <<= 1;
    if (W) *W = w;
    return wg;
}

/* A render with the flat shaper is elementwise: ns_empty returns 0.0 (sound_render.c:396-400), so
 * prev_ns_err stays 0.0 (:800) and sound_render_value (:754-809) is a function of the sample and its
 * dither term alone.  ROUND draws no dither; RPDF / TPDF / STPDF / GAUSS take theirs from K3a (the
 * MT19937 stream is serial per channel, the render is not), so all of them render inside the output
 * kernel, frame-parallel (ICW_DITH_PAR=0: the dithered ones through the serial render, A/B).  A noise
 * shaper feeds each sample's error into the next: serial per channel, in the serial render kernel --
 * as is every render behind a bus-form graph (frame-serial, hands lOut / rOut over) or with FP_CHECK
 * (the FC() render arithmetic lives in the serial render kernel only). */
bool needs_serial(const icw_config &cfg, const IcwRenderK &rk, const IcwProg &P, bool dith_par)
{
    const bool elementwise = rk.ns_kind == 0 && (cfg.render.render_type == ICW_RENDER_ROUND || dith_par);
    return !elementwise || P.is_bus || cfg.fp_check;
}

/* the per-channel render state (MT19937 words, prev_rnd, shaper rings): a serial render, or a dithered
 * one rendered frame-parallel (its generator still runs, K3a) */
bool needs_render_state(const icw_config &cfg, const IcwRenderK &rk, const IcwProg &P, bool dith_par)
{
    return needs_serial(cfg, rk, P, dith_par) || cfg.render.render_type != ICW_RENDER_ROUND;
}

bool render_cfg_ok(const icw_render_cfg &r)
{
    return r.sign_bits16 >= 2 && r.sign_bits16 <= 16 && r.sign_bits24 >= 2 && r.sign_bits24 <= 24 &&
           r.quantz_type <= 1 && r.render_type <= 4;
}

/* the output slot replace_output_plug clears for node n (adv_modulator.c:180-205): Shift / PM / Mix
 * own one, a Master none (-1) */
int plug_slot(const icw_node &n)
{
    return (n.mode == ICW_MODE_SHIFT || n.mode == ICW_MODE_PM || n.mode == ICW_MODE_MIX) ? n.n_out : -1;
}

/* the position-matched clears of icw_set_graph (include/icw.h): old list o against the new list nv */
void matched_clears(const std::vector<icw_node> &o, const std::vector<icw_node> &nv, std::vector<int> &clears)
{
    for (size_t i = 0; i < o.size(); ++i) {
        if (plug_slot(o[i]) < 0) continue;
        if (i >= nv.size() || nv[i].mode != o[i].mode || nv[i].n_out != o[i].n_out) clears.push_back(o[i].n_out);
    }
}
