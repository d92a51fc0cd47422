/*
 * icw_ctx.h -- internal: the context (struct icw_ctx), the scheduler's constants and the few helpers
 * that icw_context.cpp and icw_host.cpp share.  Never installed.
 */
#ifndef ICW_CTX_H
#define ICW_CTX_H

#include <hip/hip_runtime_api.h>

#include <mutex>
#include <vector>

#include "../../include/icw.h"
#include "icw_device.h"
#include "icw_graph_compile.h"
#include "icw_stream_table.h"
#include "icw_tuning.h"

constexpr double kAutoTaper = 0.85;          /* tail block ratio where the taper is on by default */
constexpr double kRowTaper = 0.25;           /* tail ratio of the row kernel's long blocks (no serial render) */
/* FIR converter + serial render: the first blocks grow by this ratio from kFirRenderFirst frames, so
 * that each block's converter and dither generator (one stream, ~30 us per 1 000 frames of c5fir) are
 * done before the render of the block before it ends (K3c: ~52 us per 1 000 frames).  Round 4's 2.5
 * was set for K3r at ~2.6x the converter + generator; with K3c the ratio is ~1.7, and 2.5 left ~1 ms of
 * gaps per c5fir step (profiles/r06_c5fir_fill.txt).  2 048 / 1.5 measured best of the first-block x
 * ramp grid, c5fir 9 110 -> 9 482 Msamples/s over three runs (profiles/r06_c5fir_ramp_ab.txt).
 * Running the generator beside the converter on a stream of its own removed the gaps but lowered
 * the render's clock more than that (same file). */
constexpr double kFirRenderRamp = 1.5;
constexpr int kFirRenderFirst = 2048;
/* the fused FIR converter on device buffers with nothing after it (no serial render, no host copies
 * to overlap): one launch block per 2^20 frames.  At 65 536 each block paid a rotation-table launch
 * and two ~12 us gaps beside its 0.26 ms kernel, 13 % of a c2fir step */
constexpr int kMaxFirBlockFrames = 1 << 20;
constexpr int kRowRenderMax = 2048;          /* channels up to which the render runs a row per channel */
/* int32 words of d_pid per stream of the context: a call's 5 selection rows [5][count], the FIR
 * converter's stream map [count] and the rotation table's [3][n_slabs], n_slabs <= count (with the FIR
 * converter on every (list, rate) pair has a slab; without it a slab needs two streams) */
constexpr size_t kPidWords = 9;
/* doubles of rotation table a call over per-stream lists may ask for with the FIR converter's long
 * blocks (2 GB): every (list, rate) pair has a slab there, so the launch blocks shorten instead */
constexpr size_t kMaxMixTabDoubles = (size_t)1 << 28;
constexpr size_t kPinnedStage = 1u << 20;   /* host-pointer calls up to this size stage through pinned memory */

/* internal types and helpers, shared between the library's objects and not with its users: hidden,
 * so that neither they nor the templates instantiated over them become dynamic symbols */
#pragma GCC visibility push(hidden)

struct DevState {
    double *hist = nullptr;               /* [chains][20] */
    unsigned long long *sncnt = nullptr;  /* [chains] */
    uint32_t *hq_phase = nullptr;         /* [streams][2] */
    long long *pos = nullptr;             /* [streams] */
    long long *fade = nullptr;            /* [streams][3] */
    unsigned long long *n_frame = nullptr;/* [streams] */
    double *bus = nullptr;                /* [streams][27][4] */
    uint32_t *clips = nullptr;            /* [streams][2] */
    unsigned long long *peak_bits = nullptr; /* [streams][2] */
    int *err = nullptr;                   /* kernel hand-off timeout flag */
    /* serial render state (only when the render is not ROUND/flat) */
    uint32_t *mt = nullptr;               /* [624][2*streams] */
    int32_t *mt_idx = nullptr;            /* [2*streams] */
    double *rs = nullptr;                 /* [2*streams][ICW_RSTATE] */
    uint32_t *lr_equal = nullptr;         /* [streams][2] right converters bit-identical to left ones, per filter */
    uint32_t *fes = nullptr;              /* FP_CHECK: [streams][4][ICW_FES_PITCH] FP-exception census */
};

/* streams confined to disjoint CU sets: K1 on k1_cus CUs spread over the device, the rest on
 * the other CUs (hipExtStreamCreateWithCUMask) */
struct CuSplit {
    int k1_cus = 0, rest_cus = 0;
    hipStream_t k1 = nullptr, rest = nullptr, dith = nullptr, render = nullptr;
};

/* one entry of the context's list table: the compiled program -- register or, with icw_enable_stream_bus
 * beside other entries too, bus form -- and the normalised list it came from.  A register-form entry has a
 * bus-form twin, compiled by the first call that runs it beside a bus-form stream (bus_twin) */
struct ListEnt {
    IcwProg prog{};
    std::vector<icw_node> nodes;
    IcwProg twin{};
    bool has_twin = false;
};

/* one entry of the context's render table: the setting as given, its constants and how it runs behind the
 * list in force.  With more than one entry no list is bus form and FP_CHECK is off (both refused), so
 * `serial` is the render's own; it is the render's own too while bus-form lists stand beside others
 * (icw_ctx.bus_lists, one render entry): a call then adds its own form (CallPlan::resolve_plan) */
struct RenderEnt {
    icw_render_cfg cfg{};
    int is24 = 0;
    IcwRenderK rk{};
    bool serial = false, dither = false, rstate = false;
    int osz() const { return is24 ? 6 : 4; }      /* bytes per output frame */
};

/* one entry of the context's Hilbert converter table: the setting as given, its order and coefficients
 * (iir_rp_create, hblpf.c:849-856) */
struct HilbEnt {
    uint32_t type = 0;
    int kahan = 1, subn = 1;
    int nord = 0;
    double pc[20]{}, pd[20]{}, d0 = 0.0;
};

/* one entry of the context's FIR converter table: the setting as given (M 0: the converter is off, the one
 * entry of such a table), its taps and where they start in d_fir_g.  Entries are compared by (M, the bit
 * pattern of beta) */
struct FirEnt {
    int M = 0, nt = 0;
    double beta = 0.0;
    size_t goff = 0;                      /* doubles into d_fir_g */
};

/* workgroups of wg_waves waves that a run of n streams takes in a mixed recurrence launch: whole wave
 * pairs of 4 chain slots per filter in the row form, whole 128-lane groups of 32 streams (64 under the
 * mono dedup) in the lane form, then whole workgroups */
inline int icw_k1_run_wgs(int n, bool dedup, bool row, int wg_waves)
{
    const int waves = row ? (((dedup ? n : 2 * n) + 3) / 4) * 2 : ((n + (dedup ? 63 : 31)) / (dedup ? 64 : 32)) * 2;
    return (waves + wg_waves - 1) / wg_waves;
}

#pragma GCC visibility pop

struct icw_ctx {
    icw_config cfg{};
    IcwTuning tn;                         /* the ICW_* switches as icw_create found them */
    std::vector<icw_node> nodes;
    int n_streams = 0;
    int device = 0;
    int nord = 0;
    double pc[20]{}, pd[20]{}, d0 = 0.0;
    IcwRenderK rk{};
    IcwProg prog{};
    IcwProg *d_prog = nullptr;
    /* The five per-stream settings -- DSP lists (icw_set_stream_graph), inputs (icw_set_stream_input), renders
     * (icw_set_stream_render), Hilbert converters (icw_set_stream_hilbert) and FIR converters
     * (icw_set_stream_fir) -- are one StreamTable each: the
     * distinct values in force and every stream's index.  A context whose streams share a setting holds a
     * one-entry table; nothing asks whether a table is "there".  Every edit, context-wide or per-stream,
     * builds a candidate table and goes through the setting's install (icw_context.cpp), which puts the
     * device side in place first and then swaps the table in.
     * The fields the rest of the library reads are mirrors of entry 0, each written by its table's mirror_*
     * function alone: nodes / prog / cfg.bypass_list (lists), cfg.render / cfg.need24bits / rk (renders) and
     * cfg.hilbert_type / iir_kahan / iir_subnorm_reject / nord / pc / pd / d0 (converters) and fir_M / fir_nt /
     * fir_beta (FIR converters); serial_render and
     * render_state are "some render entry needs it"; cfg.sample_rate / in_format / in_channels are the one
     * input, and while the inputs differ the one last in force alone.
     * The device keeps tables only for more than one entry: d_progs (the entries' programs; bus form among
     * them only with icw_enable_stream_bus),
     * d_inputs (one descriptor per stream), d_rtab + d_rof (entries, then the index row, one allocation),
     * d_hpc (below), d_fconv (one descriptor per stream).  A one-entry context launches from d_prog and the
     * scalar arguments. */
    StreamTable<ListEnt> lists;
    StreamTable<IcwInDesc> inputs;
    StreamTable<RenderEnt> renders;
    StreamTable<HilbEnt> hilbs;
    StreamTable<FirEnt> firs;
    IcwProg *d_progs = nullptr;
    size_t d_progs_cap = 0;               /* entries d_progs has room for */
    /* icw_enable_stream_bus: bus-form lists are served beside other lists.  Off on a fresh context, where the
     * list setters keep the refusals they always had.  bus_lists: the table has several entries and one of
     * them is bus form (install_lists) -- the state the render, converter, FIR and FP_CHECK refusals ask for.
     * A call over several entries of which one is bus form runs every stream in bus form through the mixed K4:
     * d_bprogs holds every entry's bus-form program (its own, or the twin) and d_bruns the call's runs, both
     * built by the first such call and kept while the lists (lists_gen) and the call's range stay */
    bool bus_streams = false, bus_lists = false;
    IcwProg *d_bprogs = nullptr;
    IcwK4Run *d_bruns = nullptr;          /* [n_streams] */
    unsigned long long lists_gen = 0, bprogs_gen = ~0ull, brun_gen = ~0ull;
    int brun_first = 0, brun_count = 0, brun_n = 0, brun_wgs = 0, brun_W = 0;
    /* a call over streams with different lists or inputs: K2's [5][count] selection rows, then the
     * rotation table's [3][n_slabs] (IcwK2Args.prog_id, IcwTrigArgs.slabs), rebuilt when the lists, the
     * inputs or the range change */
    int32_t *d_pid = nullptr;
    bool pid_valid = false;
    int pid_first = 0, pid_count = 0, pid_slabs = 0;
    /* the same call with the FIR converter on (KF2's per-stream form): the streams by channel class --
     * the map row lists the mono ones, then the stereo ones -- what the launcher needs of each class
     * (in_step is the call's), and the host's copy of rows 1 and 2 for the in-step test */
    bool pid_fir = false;
    IcwFirClass pid_cls[2] = {};
    std::vector<int32_t> pid_map, pid_slab, pid_ref;
    IcwProg mix{};                        /* that call's launch configuration: needs_omega, n_trig, chain, n_regs */
    IcwInDesc *d_inputs = nullptr;
    IcwRenderEnt *d_rtab = nullptr;
    int32_t *d_rof = nullptr;
    /* the converter table on the device, one allocation: the entries' pc[20] rows, then room for a call's run
     * descriptors [n_streams] and their K2 selection rows [5][n_streams] (d_hruns, d_hpid point into it).  The
     * run descriptors are built by the first call that needs them and kept while the call's shape (hrun_*)
     * and the settings stay. */
    double *d_hpc = nullptr;
    IcwK1Run *d_hruns = nullptr;
    int32_t *d_hpid = nullptr;
    bool hrun_valid = false;
    int hrun_first = 0, hrun_count = 0, hrun_n = 0, hrun_wgs = 0, hrun_waves = 0;
    bool hrun_dedup = false, hrun_row = false, hrun_mix = false;
    unsigned long long pid_gen = 0, hrun_pid_gen = 0;   /* prepare_mix rebuilds counted: the selection rows' source */
    DevState st;
    /* host mirrors of meters that survive "reset" semantics */
    std::vector<double> peak_db;          /* [streams][2] */
    /* scratch */
    /* double-buffered block scratch: block b uses set b & 1, so the output kernel of block b
     * (second stream) overlaps the IIR state kernel of block b+1 */
    double *w[kSets] = {};
    size_t w_bytes[kSets] = {};
    double *xd[kSets] = {};
    size_t xd_bytes[kSets] = {};
    uint32_t *info_dup[kSets] = {};
    hipStream_t stream2 = nullptr;
    hipEvent_t k1done[kSets] = {}, k2done[kSets] = {}, join = nullptr;
    hipEvent_t k0done[kSets] = {};
    /* dither generation (K3a) runs on its own stream, double-buffered like the block scratch */
    hipStream_t stream3 = nullptr;
    hipEvent_t ditdone[kSets] = {};
    double *dith[kSets] = {};
    size_t dith_bytes[kSets] = {};
    /* the split dither generator's chunk buffers (icw_launch_dither): tempered words, rejection flags,
     * starting-state backups; one set, used in order on the dither stream */
    uint32_t *dwords = nullptr, *dbk = nullptr;
    int32_t *dflag = nullptr;
    size_t dwords_bytes = 0, dbk_bytes = 0, dflag_bytes = 0;
    size_t dwcap = 0;                     /* words per generator row of dwords */
    unsigned char *d_in = nullptr, *d_out = nullptr;
    size_t d_in_bytes = 0, d_out_bytes = 0;
    double *d_pre = nullptr;
    size_t d_pre_bytes = 0;
    double *d_xin = nullptr;              /* ICW_F_DEBUG_INPUT: K0's rows of the call, [2*streams][n_frames] */
    size_t d_xin_bytes = 0;
    /* small host-pointer calls (the one-stream drop-in, 576-frame blocks): inputs and outputs are
     * staged through this pinned buffer, so the copies are asynchronous and the call waits once */
    unsigned char *h_stage = nullptr;
    unsigned char *h_stage_dev = nullptr; /* the same memory as the device addresses it */
    size_t h_stage_bytes = 0;
    uint32_t s1_seq = 0;                  /* K5 completion sequence number (host-polled) */
    /* the serial render (K4 bus-form graph + K3b) runs on a fourth stream, one block behind K2:
     * its inputs are double-buffered like the block scratch */
    hipStream_t stream4 = nullptr;
    /* copy stream of the block-pipelined host I/O (pinned host buffers): per-block H2D / D2H */
    hipStream_t stream_io = nullptr;
    std::vector<hipEvent_t> ev_io;        /* H2D of launch block b done */
    hipEvent_t k3done[kSets] = {};
    double *rpre[kSets] = {};             /* per-block pre-render buffer for the serial render */
    size_t rpre_bytes[kSets] = {};
    double *iq[kSets] = {};               /* per-block `in` buffer for the bus-form graph */
    size_t iq_bytes[kSets] = {};
    double *trig = nullptr;               /* per-block rotation table [T][2 * n_trig] */
    size_t trig_bytes = 0;
    /* per stream: known on the host to have bit-identical left / right converters (fresh or reset
     * state, or a set_state with equal halves, and no stereo block since) -- mono calls over such
     * streams run K1 on the left chains only */
    std::vector<char> lr_known;
    /* host mirror of every stream's modulator frame counter (the device's n_frame, advanced by the same
     * arithmetic as icw_advance): a call whose streams are all in step has every Shift / PM factor in
     * the shared rotation table, so the fused FIR kernel takes its variant without the per-stream
     * fallback (whose out-of-line call cost it scratch spills) */
    std::vector<unsigned long long> nf_host;
    bool serial_render = false;
    bool render_state = false;            /* needs_render_state: the state blob carries the render words */
    uint32_t mt_seed_state[2][624];       /* seeded MT19937 states for L / R (mtrnd_init_seed) */
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> ev;
    std::vector<hipEvent_t> ev_k0;        /* ICW_F_TIMING: a pair around K0 of each launch block */
    double last_k0_ms = 0.0;
    int n_cu = 256;
    double last_ms[2]{};
    int last_launches[2]{};
    int last_k1 = -1;                     /* ICW_K1_* of the last real-input call */
    /* the dither generator's chunks of the last icw_process_* call's first launch block and their length
     * (icw_last_dither_chunks; 0: no generator ran) */
    int last_dchunks = 0, last_dchunk_frames = 0;
    /* FIR Hilbert converter (icw_set_fir_hilbert, icw_set_stream_fir): the mirror of entry 0 of firs -- order
     * (0: the quadrature IIR; every entry is then off), taps, beta -- the entries' taps one after the other
     * (FirEnt.goff), and the per-stream input history, double-buffered by launch block (fir_par): stream s
     * holds [2][M_s] doubles from fir_off[s] on, fir_off the running sum of 2 M_s ([streams + 1]; one entry:
     * [streams][2][M]).  fir_Mmax: the largest order in force (the state blob's size).  d_fconv: every
     * stream's descriptor, while the table has several entries */
    int fir_M = 0, fir_nt = 0, fir_Mmax = 0;
    double fir_beta = 0.0;
    double *d_fir_g = nullptr;
    double *fir_hist[2] = {};
    int fir_par = 0;
    std::vector<size_t> fir_off;
    IcwFirConv *d_fconv = nullptr;
    /* icw_enable_stream_fir: per-stream lists and inputs are served beside the converter.  Off on a fresh
     * context, where the three setters keep the refusals they always had */
    bool fir_streams = false;
    /* icw_enable_stream_encode: the CWAVE encoders serve calls over streams with different inputs.  Off on
     * a fresh context, where they keep their refusal while the count is above 1 */
    bool enc_streams = false;
    /* icw_enable_stream_cwave: icw_set_stream_input takes the CWAVE formats, also on a context whose input is
     * CWAVE.  Off on a fresh context, where it keeps both refusals */
    bool cw_streams = false;
    unsigned long long *enc_clipped = nullptr; /* [streams] icw_encode_cwave: saturated / NaN int16 samples (lazy) */
    unsigned long long *s1_stamps = nullptr;   /* ICW_S1_STAMPS=1: K5 phase stamps, printed per call */
    unsigned long long calls = 0;         /* icw_process_* calls so far (icw_prepare needs a fresh context) */
    /* per-stream state set by an entry point other than a call (stream_open, seek, set_state, the
     * resets): icw_prepare's closing icw_stream_init would wipe it, so it refuses.  Context-wide
     * setters (set_outbits, set_render, ...) leave it false: the warm-up runs with them. */
    bool touched = false;
    std::mutex mu;
};

#pragma GCC visibility push(hidden)

int set_dev(icw_ctx *c);
hipError_t quiesce(icw_ctx *c);
bool host_pinned(const void *p, int dev);
const CuSplit *cu_split(icw_ctx *c, int k1_cus);

template <class T>
int dalloc(T **p, size_t n)
{
    *p = nullptr;
    if (n == 0) n = 1;
    if (hipMalloc((void **)p, n * sizeof(T)) != hipSuccess) return ICW_ENOMEM;
    if (hipMemset(*p, 0, n * sizeof(T)) != hipSuccess) return ICW_EDEVICE;
    return ICW_OK;
}

#pragma GCC visibility pop

#endif
