/*
 * icw_tuning.h -- the ICW_* environment switches of the host side, as one record.  They are
 * measurement aids (A/B runs, profiling), not configuration: icw_create reads them once into its
 * context, so a context keeps the values of its creation and two contexts of one process may differ.
 * No HIP types; nothing else in csrc/ reads the environment.
 */
#ifndef ICW_TUNING_H_
#define ICW_TUNING_H_

#include <stdlib.h>
#include <string.h>

/* frames per kernel launch: bounds the w scratch buffer (n_chains * (T+N) doubles) */
constexpr int kMaxBlockFrames = 1 << 16;
constexpr int kDefBlockFrames = 1 << 14;   /* launch block: shorter pipeline fill / drain */
constexpr int kSets = 3;                    /* most block scratch sets (ICW_SETS); default 2 */

struct IcwTuning {
    int k1_mode = -1;         /* ICW_K1_MODE=plain|row: K1 variant, -1 auto (row / plain), 0 plain lanes,
                                 3 row broadcast */
    int render_row = -1;      /* ICW_RENDER=serial|row: serial render kernel, -1 auto (row broadcast for
                                 <= kRowRenderMax channels), 0 lane per channel, 1 row */
    bool serialize = false;   /* ICW_SERIALIZE=1: every kernel on the caller's stream (profiling) */
    bool cu_split = true;     /* ICW_CU_SPLIT=0 disables the partition */
    /* ICW_K1_WPC: K1 waves per CU.  Two: measured under a working partition, 4 per CU (one per
     * SIMD) made K1 +21 % slower even alone (C3, 4-wave workgroups), 3 per CU +27 % beside K2, and 1
     * per CU leaves the frame-parallel kernels too few CUs (C4 K2 2.57 -> 3.70 ms) */
    int k1_wpc = 2;
    /* ICW_K1_WG: K1 waves per workgroup.  Default 1 for the lane kernel, 2 for the row kernel: its I and
     * Q filter waves of the same streams then share a CU, so the second one reads the channel rows
     * (one per channel since round 3) from the L2 / L1 the first one filled (C2 +0.7 %, C5 +0.4 %; the
     * lane kernel loses 2-2.5 % on C3 / C4 with 2) */
    int k1_wg = 1;
    bool k1_wg_env = false;   /* ICW_K1_WG given */
    double fir_ramp = 0.0;    /* ICW_FIR_RAMP: the ramp of a FIR + serial-render call (0: kFirRenderRamp) */
    /* ICW_REST_CUS: at most this many CUs for the frame-parallel kernels beside K1 (0: all the rest).
     * Default (-1): all but 32 (4 per XCD) -- idle CUs leave K1 power headroom: C3 41.6-42.2k ->
     * 42.6-42.9k, C4 20.9k -> 21.1-21.3k Msamples/s at 160 and 176 (profiles/r04_rest_cus.txt);
     * below 160 K2 falls behind (C3 38.0k at 144 and 128) */
    int rest_cus = -1;
    int max_block = kDefBlockFrames;      /* ICW_BLOCK: frames per launch block */
    bool block_env = false;               /* ICW_BLOCK given */
    int max_sets = 2;                     /* ICW_SETS: block scratch sets (2..kSets) */
    /* ICW_ZEROCOPY=0: small calls copy the staging buffer to and from HBM instead of the kernels
     * reading the input from, and writing the output to, the pinned buffer directly */
    bool zero_copy = true;
    bool spin_wait = true;                /* ICW_SPIN=0: K5 zero-copy calls wait on the stream instead */
    /* block schedule of long calls (plan_blocks): a short first block (the pipeline fill is K0 of
     * block 0 alone: C3 +2.5 %, C4 +1.4 %) and an optional geometric tail (the drain is K2 / K3 of
     * the last block alone).  The tail pays only if K0 + K2 (and K3) of a block fit beside K1 of a
     * block r times shorter: in C3 / C4 they take 0.87 / 0.94 of K1's time per frame, and r = 0.85
     * measured C3 -4 %, C4 -8 %; in C5 (K1r, K2 0.12 and the row render 0.64 of K1r on their own
     * streams) r = 0.85 measured +2 %.  So it is on by default for the row kernel with a serial
     * render only (icw_process_streams). */
    int first_block = 4096;               /* ICW_FIRST_BLOCK (0: uniform blocks) */
    bool first_block_env = false;         /* ICW_FIRST_BLOCK given */
    double taper = -1.0;                  /* ICW_TAPER: tail block ratio (0: no tail; -1: auto) */
    int taper_min = 1024;                 /* ICW_TAPER_MIN: smallest tail block */
    bool dedup_ok = true;                 /* ICW_DEDUP=0 disables the mono K1 dedup (A/B) */
    bool fill_drain = true;               /* ICW_FILL_DRAIN=0: first K0 / last K2 stay partitioned (A/B) */
    bool fir_fuse = true;                 /* ICW_FIR_FUSED=0: KF + K2 as two kernels (A/B) */
    bool chain_ok = true;                 /* ICW_CHAIN=0: chain programs keep the LDS register file (A/B) */
    bool stream1 = true;                  /* ICW_STREAM1=0: one-stream calls keep the four kernels (A/B) */
    bool s1_ovl = true;                   /* ICW_S1_OVL=0: K5's output phase after the recurrence (A/B) */
    bool s1_stamps = false;               /* ICW_S1_STAMPS=1: K5 phase stamps, printed per call */
    bool k3r_spec = true;                 /* ICW_K3R_SPEC=0: the row render without clamp-free blocks (A/B) */
    bool dith_par = true;                 /* ICW_DITH_PAR=0: dithered flat renders through the serial render (A/B) */
    bool fir_sig = true;                  /* ICW_FIR_SIG=0: icw_fir_graph for every tile (A/B) */
};

inline IcwTuning icw_read_tuning()
{
    IcwTuning t;
    const auto is = [](const char *name, const char *v) {
        const char *e = getenv(name);
        return e && !strcmp(e, v);
    };
    const auto off = [](const char *name) {          /* set to a number that is 0 (or to no number) */
        const char *e = getenv(name);
        return e && atoi(e) == 0;
    };
    const char *e;
    if (is("ICW_K1_MODE", "plain")) t.k1_mode = 0;
    if (is("ICW_K1_MODE", "row")) t.k1_mode = 3;
    if (is("ICW_RENDER", "serial")) t.render_row = 0;
    if (is("ICW_RENDER", "row")) t.render_row = 1;
    t.serialize = is("ICW_SERIALIZE", "1");
    t.cu_split = !is("ICW_CU_SPLIT", "0");
    if ((e = getenv("ICW_K1_WPC")) && atoi(e) >= 1 && atoi(e) <= 8) t.k1_wpc = atoi(e);
    if ((e = getenv("ICW_K1_WG")) && atoi(e) >= 1 && atoi(e) <= 4) { t.k1_wg = atoi(e); t.k1_wg_env = true; }
    if ((e = getenv("ICW_FIR_RAMP")) && atof(e) > 1.0 && atof(e) <= 16.0) t.fir_ramp = atof(e);
    if ((e = getenv("ICW_REST_CUS")) && (atoi(e) == 0 || atoi(e) >= 8)) t.rest_cus = atoi(e);
    if ((e = getenv("ICW_BLOCK")) && atoi(e) >= 256 && atoi(e) <= kMaxBlockFrames) { t.max_block = atoi(e); t.block_env = true; }
    if ((e = getenv("ICW_SETS")) && atoi(e) >= 2 && atoi(e) <= kSets) t.max_sets = atoi(e);
    t.zero_copy = !is("ICW_ZEROCOPY", "0");
    t.spin_wait = !is("ICW_SPIN", "0");
    if ((e = getenv("ICW_FIRST_BLOCK")) && atoi(e) >= 0) { t.first_block = atoi(e); t.first_block_env = true; }
    if ((e = getenv("ICW_TAPER")) && atof(e) >= 0.0 && atof(e) < 1.0) t.taper = atof(e);
    if ((e = getenv("ICW_TAPER_MIN")) && atoi(e) >= 64) t.taper_min = atoi(e);
    t.dedup_ok = !is("ICW_DEDUP", "0");
    t.fill_drain = !is("ICW_FILL_DRAIN", "0");
    t.fir_fuse = !is("ICW_FIR_FUSED", "0");
    t.chain_ok = !is("ICW_CHAIN", "0");
    t.stream1 = !is("ICW_STREAM1", "0");
    t.s1_ovl = !is("ICW_S1_OVL", "0");
    t.s1_stamps = is("ICW_S1_STAMPS", "1");
    t.k3r_spec = !off("ICW_K3R_SPEC");
    t.dith_par = !off("ICW_DITH_PAR");
    t.fir_sig = !off("ICW_FIR_SIG");
    return t;
}

#endif
