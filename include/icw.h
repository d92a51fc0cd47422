/*
 * icw.h -- C ABI of in_cwave_amd: the MI355X-native Hilbert -> modulator-graph -> render
 * hot path of rat-and-catcher/in_cwave (V2.4.4), batched over many independent streams.
 *
 * Plain C types only (no torch, no HIP types).  Every entry point returns an int status:
 * ICW_OK (0) or a negative ICW_E* code -- an improvement over the reference's overloaded 0
 * return of amod_process_samples (adv_modulator.c:601-602), which cannot tell EOF from error.
 *
 * Reference interfaces replaced (file:line into the reference tree):
 *   icw_process_batch / icw_process_block
 *        <- int amod_process_samples(char *buf, MOD_CONTEXT *mc)      in_cwave.h:648,
 *           adv_modulator.c:587-763 (one block: n_frame -> unpack+Hilbert -> graph -> render)
 *   icw_create(cfg, nodes)     <- mod_context_init (in_cwave.c:46-80) + amod_init
 *                                 (adv_modulator.c:216-331: head==Master validation, L/R locks)
 *   icw_stream_open            <- mod_context_fopen (in_cwave.c:207-236) + the fade /
 *                                 sec_align arithmetic of xwave_reader_create
 *                                 (xwave_reader.c:688-725)
 *   icw_stream_reset_hilbert   <- mod_context_reset_hilbert / hq_rp_reset (lpf_hilbert_quad.c:160-165)
 *   icw_stream_reset_framecnt  <- mod_context_reset_framecnt (in_cwave.c:287-296)
 *   icw_get_meters             <- amod_get_clips_peaks (adv_modulator.c:445-465) and
 *                                 mod_context_get_desubnorm_counter (in_cwave.c:300-321)
 *   icw_render_size            <- sound_render_size (sound_render.c:684-687)
 *
 * Threading: a context is driven by one host thread at a time (as MOD_CONTEXT is driven by one
 * decode thread, playback.c:567-671); parameters are snapshotted per call (block granularity,
 * SURVEY 3.4).  Different contexts may be used concurrently from different threads / devices.
 */
#ifndef ICW_H_
#define ICW_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
#define ICW_OK              0
#define ICW_EINVAL         -1   /* bad argument / unsupported configuration */
#define ICW_ENOMEM         -2   /* device or host allocation failed */
#define ICW_EDEVICE        -3   /* HIP runtime error */
#define ICW_EGRAPH         -4   /* DSP list rejected (no unique Master at head, bad plug ...) */
#define ICW_EUNSUPPORTED   -5   /* valid for the reference, not (yet) on this path */

/* ---- constants mirrored from in_cwave.h / sound_render.h / lpf_hilbert_quad.h ---- */
#define ICW_N_INPUTS        27  /* in[0], A[1]..Z[26]             in_cwave.h:244 */
#define ICW_MAX_IIR_ORDER   20  /* largest canned HB LPF order    hblpf.c:740-820 */
#define ICW_MAX_NS_TAPS     20  /* largest noise shaper            sound_render.c:75-235 */
#define ICW_HZ_SCALE        1000u
#define ICW_MAX_FS_SRC      2000000u

/* node modes (NODE_DSP.mode, in_cwave.h:283-287) */
#define ICW_MODE_MASTER 0
#define ICW_MODE_SHIFT  1
#define ICW_MODE_PM     2
#define ICW_MODE_MIX    3
/* master output conversions (in_cwave.h:152-155) */
#define ICW_S_ADD_REIM  0
#define ICW_S_SUB_REIM  1
#define ICW_S_RE        2
#define ICW_S_IM        3
/* channel exchange (in_cwave.h:186-193) */
#define ICW_XCH_NORMAL    0
#define ICW_XCH_SWAP      1
#define ICW_XCH_LEFTONLY  2
#define ICW_XCH_RIGHTONLY 3
#define ICW_XCH_MIXLR     4
/* real (RWAVE/WAV) input sample formats (HRW_FMT_*, in_cwave.h:318-323) */
#define ICW_FMT_U8   0
#define ICW_FMT_I16  1
#define ICW_FMT_I24  2
#define ICW_FMT_I32  3
#define ICW_FMT_F32  4
/* complex (CWAVE) input sample formats, ICW_FMT_CW_F64 + HCW_FMT_* (cwave.h:70-80).  The analytic
 * signal is used as read: the Hilbert converters are bypassed and keep their state, fades scale
 * I and Q alike (xwave_unpack_csample, xwave_reader.c:939-966); mono feeds R with L's I/Q. */
#define ICW_FMT_CW_F64      5     /* double Re, Im           HCW_FMT_PCM_DBL64 */
#define ICW_FMT_CW_I16      6     /* int16 Re, Im            HCW_FMT_PCM_INT16 */
#define ICW_FMT_CW_I16_F32  7     /* int16 Re, float Im      HCW_FMT_PCM_INT16_FLT32 */
#define ICW_FMT_CW_F32      8     /* float Re, Im            HCW_FMT_PCM_FLT32 */
/* render (sound_render.h:54-84) */
#define ICW_QUANTZ_MID_TREAD 0
#define ICW_QUANTZ_MID_RISER 1
#define ICW_RENDER_ROUND 0
#define ICW_RENDER_RPDF  1
#define ICW_RENDER_TPDF  2
#define ICW_RENDER_STPDF 3
#define ICW_RENDER_GAUSS 4
#define ICW_NSHAPE_FLAT  0
#define ICW_NSHAPE_MEW44 2
#define ICW_NSHAPE_MAX   17
/* default render seeds (in_cwave.c:69-70) */
#define ICW_SEED_LEFT   0x13579BDFu
#define ICW_SEED_RIGHT  0x479B22ABu
#define ICW_SR_ZERO_SIGNAL_DB (-555.0)

/* One DSP node (NODE_DSP, in_cwave.h:273-287, without list links / name).  Channel arrays are
 * [0]=left, [1]=right.  The list is passed head first: nodes[0] must be the Master. */
typedef struct icw_node {
    int32_t  mode;                    /* ICW_MODE_* */
    int32_t  n_out;                   /* output bus slot 1..26 (SHIFT/PM/MIX) */
    double   gain[2];                 /* l_gain / r_gain */
    uint8_t  inputs[ICW_N_INPUTS];    /* bus slots mixed into the node */
    uint8_t  pad_[1];
    int32_t  xch_mode;                /* ICW_XCH_* */
    int32_t  iq_invert[2];            /* l_iq_invert / r_iq_invert */
    int32_t  tout[2];                 /* MASTER: ICW_S_* */
    double   fr_shift[2];             /* SHIFT: signed shift, Hz */
    int32_t  is_shift[2];
    double   pm_freq[2], pm_phase[2], pm_level[2], pm_angle[2];   /* PM */
    int32_t  is_pm[2];
    /* L/R locks applied at icw_create exactly as amod_init does (adv_modulator.c:247-293) */
    int32_t  lock_gain, lock_shift, sign_lock_shift;
    int32_t  lock_freq, lock_phase, lock_level, lock_angle;
    int32_t  reserved_;
} icw_node;

/* SR_VCONFIG (sound_render.h:145-153) */
typedef struct icw_render_cfg {
    double   dth_bits;
    uint32_t quantz_type, render_type, nshape_type, sign_bits16, sign_bits24;
} icw_render_cfg;

/* Context-wide configuration (IN_CWAVE_CFG hot-path fields, in_cwave.h:435-459) */
typedef struct icw_config {
    uint32_t sample_rate;         /* Hz, <= ICW_MAX_FS_SRC */
    uint32_t in_format;           /* ICW_FMT_* */
    uint32_t in_channels;         /* 1 (mono: R fed with L) or >= 2 (channels > 2 skipped) */
    uint32_t hilbert_type;        /* IX_LPF_HILB_TYPE0..5 (default 1) */
    int32_t  iir_kahan;           /* IIR_SUM_KAHAN (default 1) */
    int32_t  iir_subnorm_reject;  /* IIR_SUBN_ZERO (default 1) */
    int32_t  frmod_scaled;        /* FRMOD_SCALED (default 1) */
    int32_t  need24bits;          /* NEED24BITS */
    int32_t  bypass_list;         /* am.is_bypass_list */
    uint32_t seed_left, seed_right;
    icw_render_cfg render;
    int32_t  fp_check;            /* FP_CHECK (default 0): the FC() arithmetic and census of
                                     fp_check.c:52-100 in the IIR (hblpf.c:928-950, 1058-1095) and
                                     the render (sound_render.c:403-489, 815-903); icw_get_fp_census */
} icw_config;

/* Per-stream meters.  The reference keeps one set, global in `am` (adv_modulator.c:54-56), that
 * both decoding contexts feed (adv_modulator.c:757-758); icw_amod_get_clips_peaks (icw_amod.h)
 * combines the per-context meters into it: clips summed, peaks maxed, a reset clearing all. */
typedef struct icw_meters {
    uint32_t clips[2];            /* InterlockedIncrement'ed clip counters, sound_render.c:782-795 */
    double   peak_db[2];          /* max 20*log10(|q|/hi_bound), SR_ZERO_SIGNAL_DB if silent */
    uint64_t desubnorm;           /* sum of the 4 IIR subnorm_cnt of the stream, hblpf.c:918/1049 */
} icw_meters;

typedef struct icw_ctx icw_ctx;

/* flags for icw_process_batch */
#define ICW_F_DEVICE_PTRS  1u     /* in/out are device pointers already resident in HBM */
#define ICW_F_DEBUG_PRE    2u     /* also write the 2 pre-render doubles/frame to dbg (tests) */
#define ICW_F_TIMING       4u     /* time the kernels with HIP events (icw_last_timing) */
#define ICW_F_DEBUG_INPUT  8u     /* tests: write the unpacked, faded samples the Hilbert converters get
                                     (what xwave_unpack_csample hands hq_rp_process, xwave_reader.c:
                                     974-998; R = L for mono) to dbg as double[n_streams][n_frames][2]:
                                     real input through the quadrature IIR, host pointers only */

/* Create a context for n_streams streams on HIP device `device` (-1: current device).
 * The DSP list is normalised exactly as amod_init (adv_modulator.c:216-331) does; a list it
 * would reject (no Master at head, 2 Masters, bad mode) is replaced by the default Master
 * (S_ADD_REIM, gain 0.8, input `in`) and *accepted is set to 0, like amod_init's return. */
int icw_create(const icw_config *cfg, const icw_node *nodes, int n_nodes, int n_streams,
               int device, icw_ctx **out, int *accepted);
int icw_destroy(icw_ctx *ctx);

/* Fresh reference state for streams [first, first+count): Hilbert rings zeroed, n_frame=0,
 * bus zeroed, renders re-seeded (mod_context_init, in_cwave.c:46-80). */
int icw_stream_init(icw_ctx *ctx, int first, int count);
/* Open a track on stream s (mod_context_fopen): track length in frames, fades in ms,
 * sec_align in s.  Resets the renders' shaping state (sound_render_set_outbits), not the RNG;
 * clears n_frame / Hilbert only if the flags say so (is_clr_nframe_trk / is_clr_hilb_trk). */
int icw_stream_open(icw_ctx *ctx, int s, int64_t n_samples, uint32_t fade_in_ms,
                    uint32_t fade_out_ms, uint32_t sec_align, int clr_nframe, int clr_hilb);
int icw_stream_reset_hilbert(icw_ctx *ctx, int s);
int icw_stream_reset_framecnt(icw_ctx *ctx, int s);
/* reader seek (xwave_seek_samples, xwave_reader.c:752-785): frame position inside the track,
 * virtual tail included, from which fades are evaluated */
int icw_stream_seek(icw_ctx *ctx, int s, int64_t frame_pos);
/* input format of the next blocks (a new track, mod_context_fopen): sample rate, ICW_FMT_*,
 * channels; applies to every stream of the context */
int icw_set_input(icw_ctx *ctx, uint32_t sample_rate, uint32_t fmt, uint32_t channels);

/* Per-stream inputs: a batch whose streams each read their own track format (mod_context_fopen
 * builds a reader per file) -- rate, sample format, channels -- in ONE context, so a library that
 * mixes 44.1 / 48 / 96 kHz, 16 / 24 bit / float and mono / stereo keeps the batch width.
 *   icw_set_stream_input      icw_set_input for streams [first, first + count) only, in force from
 *                             the next call on (the context's work is waited for).  Streams given
 *                             the same input share it: giving every stream one input leaves a
 *                             one-input context, which issues the launches it always did.
 *   icw_stream_input_count    distinct inputs in force (1 on a fresh context).
 * icw_create and icw_set_input keep their meaning, every stream: icw_set_input on a context whose
 * streams differ collapses it to one input.
 * A call's input layout: stream s starts at in + s*in_stride_bytes, as ever, and its frames have that
 * stream's own frame size; in_stride_bytes must hold n_frames frames of every stream of the call
 * (device pointers included), else ICW_EINVAL.  Host staging rows are sized by the call's widest frame.
 * A call whose streams all share one input is resolved on the host and runs the kernels of a
 * one-input context; only a call over differing inputs takes the table-reading kernel instances.
 * icw_stream_open takes its fades at stream s's own rate.  The five real formats, 1 or >= 2 channels,
 * any rate up to ICW_MAX_FS_SRC; host and device pointers; icw_process_batch and icw_process_streams;
 * register-form and bus-form lists, per-stream lists in the same context, every render, FP_CHECK, and
 * the FIR converter (icw_set_fir_hilbert, context-wide, in either order with this call) on a context
 * that asked for it with icw_enable_stream_fir: its kernels read every stream's own real format, rate
 * and channels.
 * Limits, each refusal changing nothing:
 *   ICW_EINVAL        a range outside the context, rate 0 or above ICW_MAX_FS_SRC, channels 0, fmt
 *                     out of range.
 *   ICW_EUNSUPPORTED  - without icw_enable_stream_cwave: a CWAVE format (fmt >= ICW_FMT_CW_F64), or a context
 *                       whose input is CWAVE: whether the quadrature IIR runs at all is decided per call;
 *                     - without icw_enable_stream_fir: the FIR converter is on (icw_set_fir_hilbert with
 *                       k_M > 0), or, while the count is above 1, icw_set_fir_hilbert(k_M > 0);
 *                     - while the count is above 1: ICW_F_DEBUG_INPUT, and -- without
 *                       icw_enable_stream_encode -- icw_encode_cwave and icw_encode_cwave_iir.
 *   icw_enable_stream_encode(ctx, 1)  the two CWAVE encoders (icw_cwave.h) serve calls over streams with
 *                     different inputs from then on: input rows as above, stream s's frames at
 *                     out + s*out_stride_bytes at its own icw_cwave_frame_bytes(cw_format, channels_s).  A
 *                     fresh context has it off and keeps the refusal above, so a host that relies on it
 *                     sees no change.  (ctx, 0) turns it off again and is ICW_OK whatever is in force (the
 *                     fresh state: the encoders refuse while the count is above 1); only a NULL context is
 *                     refused (ICW_EINVAL).  It lifts nothing else: icw_encode_cwave_iir still refuses a
 *                     cfg.fp_check context, ICW_F_DEBUG_INPUT stays refused, and icw_encode_cwave needs the
 *                     converter, which beside differing inputs needs icw_enable_stream_fir (without it
 *                     icw_set_fir_hilbert / icw_set_stream_input return ICW_EUNSUPPORTED as listed, the
 *                     converter stays off, and icw_encode_cwave returns its ICW_EINVAL for a context
 *                     without one).  icw_encode_cwave_fft takes no context and is not concerned.
 *   icw_enable_stream_cwave(ctx, 1)  icw_set_stream_input takes ICW_FMT_CW_F64 .. ICW_FMT_CW_F32 from then on (1 or
 *                     >= 2 channels, any rate up to ICW_MAX_FS_SRC; IcwInDesc-wise the "channel" is the I/Q
 *                     pair), also on a context created with a CWAVE in_format: a library of CWAVE files in the
 *                     four frame formats, mono and stereo, at several rates decodes in ONE context.  A fresh
 *                     context has it off and keeps the two refusals above.  (ctx, 0) returns ICW_EUNSUPPORTED,
 *                     changing nothing, while the count is above 1 and some stream's input is CWAVE; otherwise
 *                     ICW_OK.  A NULL context: ICW_EINVAL.
 *                     A context may then hold real and CWAVE streams side by side, but a call
 *                     (icw_process_streams, icw_process_batch; icw_prepare's warm-up is one over every stream)
 *                     covers streams of ONE kind: over both it returns ICW_EUNSUPPORTED and changes nothing --
 *                     whether K1 runs stays a per-call decision.  A call whose CWAVE streams share one input
 *                     runs the complex-input launches of a one-input context (K0 + K2); a call over differing
 *                     CWAVE inputs launches no K0 -- the output kernel reads the file frames itself, with one
 *                     typed load per I/Q pair where the stream's row and frame size are aligned to the pair
 *                     (byte loads otherwise, and always for the 6-byte ICW_FMT_CW_I16_F32 pair).  Rows and
 *                     the stride rule are as above.  Per stream the semantics are the reference's: mono feeds
 *                     R with L's I/Q, the fade scales all four values at the stream's own rate, the frame
 *                     counter wraps at the stream's own rate, and the Hilbert phases and rings are not touched
 *                     -- a stream that plays WAV, CWAVE, WAV continues its converter where the first WAV
 *                     track left it.  Host and device pointers, register-form and bus-form lists, per-stream
 *                     lists, every render and FP_CHECK are served.  Refused, changing nothing
 *                     (ICW_EUNSUPPORTED): a CWAVE format through icw_set_stream_input while the FIR converter
 *                     is on (k_M > 0), or a real one that would leave CWAVE and other inputs side by side
 *                     under it; icw_set_fir_hilbert(k_M > 0) while the count is above 1 and some stream's
 *                     input is CWAVE; ICW_F_DEBUG_INPUT while the count is above 1, as ever.  The encoders
 *                     return their ICW_EINVAL for a call with a CWAVE stream in it, as for CWAVE input.
 * Not served: icw_group and the icw_amod_* drop-in (their input stays context-wide).  The state blob
 * does not carry the input, as it does not carry the list: icw_set_state expects the stream's input to
 * be set as it was. */
int icw_set_stream_input(icw_ctx *ctx, int first, int count, uint32_t sample_rate, uint32_t fmt,
                         uint32_t channels);
int icw_stream_input_count(const icw_ctx *ctx);
int icw_enable_stream_encode(icw_ctx *ctx, int on);
int icw_enable_stream_cwave(icw_ctx *ctx, int on);

/* Live parameter changes (the GUI thread edits the DSP list, the renders and the
 * Hilbert converters while a decode thread runs).  Each applies to every stream of the context from
 * the next call on; a call already queued finishes with the old parameters.  Per-stream state
 * (bus slots, rings, MT19937, meters) carries over exactly as the reference carries it.
 *
 * icw_set_graph   <- amod_add_lastdsp / amod_del_lastdsp / amod_del_dsplist
 *                    (adv_modulator.c:358-400), the node-field writes of the GUI
 *                    (amod_gui_control.c:259-420, 1433-1482) and amod_set_bypass_list_flag
 *                    (adv_modulator.c:422-425): the whole new list, head first, normalised as
 *                    icw_create does (locks fanned out).  A list amod_init would reject (no Master
 *                    at the head, two Masters, unknown mode) returns ICW_EGRAPH with *accepted = 0
 *                    and leaves the running list in place.  The 27-slot bus keeps its values,
 *                    except the slots the reference clears: amod_del_lastdsp, amod_del_dsplist and
 *                    amod_set_output_plug go through replace_output_plug (adv_modulator.c:176-209),
 *                    which zeroes the removed / re-plugged node's old output slot in every context
 *                    (mod_context_clear_all_inouts, in_cwave.c:255-261).  The new list is matched to
 *                    the old one by position: an old Shift / PM / Mix node whose position is gone,
 *                    now holds a node of another mode, or whose n_out changed has its old slot
 *                    zeroed for every stream.  Edits that position matching cannot see (a re-plug to
 *                    the same slot, delete + add of an identical node) are the list primitives below:
 *                    a host that binds the GUI forwards each primitive as it happens, not a diff.
 * icw_clear_bus_slot <- mod_context_clear_all_inouts (in_cwave.c:255-261): bus slot 0..26 of
 *                    every stream to zero (the 4 doubles L re/im, R re/im).
 * icw_set_render  <- srenders_set_vcfg (in_cwave.c:457-469) -> sound_render_setup
 *                    (sound_render.c:625-629): the new SR_VCONFIG for both renders of every
 *                    stream; sound_render_recalc restarts prev_rnd, the shaper rings and
 *                    prev_ns_err, the MT19937 generators go on.  16/24 bits stay (need24bits;
 *                    a new track's depth is icw_set_outbits below).
 * icw_set_hilbert_filter <- mod_context_change_all_hilberts_filter (in_cwave.c:186-199): a
 *                    different type re-creates every converter (hq_rp_create: zero rings, phase 0,
 *                    de-subnorm counters 0); the same type changes nothing.  type 0..5.
 * icw_set_hilbert_config <- mod_context_change_all_hilberts_config (in_cwave.c:171-182) ->
 *                    iir_rp_setcfg (hblpf.c:1117-1127): Kahan / baseline summation and the
 *                    subnormal reject; the rings stay, the de-subnorm counters restart. */
int icw_set_graph(icw_ctx *ctx, const icw_node *nodes, int n_nodes, int bypass_list, int *accepted);
int icw_clear_bus_slot(icw_ctx *ctx, int slot);

/* The list primitives one by one, each with exactly the reference's bus clearing -- no position
 * matching.  replace_output_plug (adv_modulator.c:176-209) clears a Shift / PM / Mix node's OLD
 * output slot in every stream, also when it is re-plugged to the same slot; a Master clears nothing.
 *   icw_graph_del_last      <- amod_del_lastdsp (adv_modulator.c:378-390): the tail node goes and
 *                              its slot is cleared; a list of the Master alone is left as it is.
 *   icw_graph_del_all       <- amod_del_dsplist (adv_modulator.c:360-374): tail first, down to the
 *                              Master, each removed node's slot cleared.
 *   icw_graph_add_last      <- amod_add_lastdsp (adv_modulator.c:394-411) followed by the GUI's
 *                              field writes of the new node (amod_gui_control.c:1858): `node` is
 *                              appended after the tail, its L/R locks fanned out as amod_init does;
 *                              nothing is cleared.  A Master is refused (create_node_dsp, :112-123):
 *                              ICW_EGRAPH.
 *   icw_graph_set_output_plug <- amod_set_output_plug (adv_modulator.c:436-441, the GUI's plug
 *                              selector amod_gui_control.c:1125): node `index` (0 = the head) gets
 *                              output slot n (1..26), or keeps its slot with n = -1 ("remove only");
 *                              either way its old slot is cleared.
 * The field writes of existing nodes (gains, frequencies, inputs, locks) and the bypass flag clear
 * nothing: icw_set_graph with the same structure. */
int icw_graph_del_last(icw_ctx *ctx);
int icw_graph_del_all(icw_ctx *ctx);
int icw_graph_add_last(icw_ctx *ctx, const icw_node *node);
int icw_graph_set_output_plug(icw_ctx *ctx, int index, int n);
int icw_set_render(icw_ctx *ctx, const icw_render_cfg *render);

/* Per-stream DSP lists: a batch whose streams each carry their own NODE_DSP settings (Shift
 * frequency, PM settings, gains, bypass flag) in ONE context, so the batch keeps its width.
 *   icw_set_stream_graph      icw_set_graph for streams [first, first + count) only: the same
 *                             normalisation and validation (a list amod_init would reject returns
 *                             ICW_EGRAPH with *accepted = 0 and the running lists stay), in force
 *                             from the next call on.  The position-matched bus clearing is applied
 *                             to those streams only, each against its own old list; bypass_list is
 *                             per stream.  The context keeps the distinct compiled lists and an
 *                             index per stream; streams given the same list share one entry, so a
 *                             call that gives every stream one list leaves a one-list context.
 *   icw_clear_stream_bus_slot icw_clear_bus_slot for streams [first, first + count) only.
 *   icw_stream_graph_count    distinct lists in force (1 on a fresh context).
 * icw_create and icw_set_graph keep their meaning, every stream: on a context whose streams differ,
 * icw_set_graph replaces all the lists (count back to 1), its clears matched per stream against
 * that stream's old list.
 * Limits, each refusal changing nothing:
 *   ICW_EINVAL        a range outside the context, or nodes == NULL with n_nodes > 0.
 *   ICW_EUNSUPPORTED  - the new list, or the list in force, compiles to the bus form (a one-frame
 *                       delay, feedback, more than 16 nodes): the serial graph kernel runs one lane
 *                       per stream on one program.  Such lists stay context-wide (icw_set_graph);
 *                     - without icw_enable_stream_fir: the FIR converter is on (icw_set_fir_hilbert with
 *                       k_M > 0), or, while the count is above 1, icw_set_fir_hilbert(k_M > 0);
 *                     - while the count is above 1: icw_set_graph with
 *                       a bus-form list (collapse with a register-form icw_set_graph first), and the
 *                       list primitives icw_graph_del_last / _del_all / _add_last / _set_output_plug
 *                       ("the context's list" is undefined then: edit such streams with
 *                       icw_set_stream_graph and icw_clear_stream_bus_slot).
 * FP_CHECK contexts, CWAVE input and -- on a context that asked for it with icw_enable_stream_fir -- the
 * FIR converter (icw_set_fir_hilbert, on or off, in either order with this call) are served: with the
 * converter on, streams that share a chain signature -- 256
 * Shift frequencies of one list shape -- stay on its signature kernel in one launch.  Not served: icw_group (its lists stay
 * context-wide), the icw_amod_* drop-in and the encoders (they run no list).  The state blob does not
 * carry a list: icw_set_state expects the stream's list to be set as it was.
 *   icw_enable_stream_bus(ctx, 1)  serves bus-form lists per stream from then on -- feedback loops, one-frame
 *                                  delays, lists of more than 16 nodes, each stream with its own: the first
 *                                  and the third refusal above fall.  icw_set_stream_graph takes bus-form
 *                                  lists (also while the list in force is one), icw_set_graph takes one
 *                                  while the lists differ and collapses the table to count 1 as ever, and
 *                                  the position-matched clearing and icw_clear_stream_bus_slot work per
 *                                  stream as for register-form lists.  A call whose streams share one list
 *                                  entry launches what a one-list context launches; a call over several
 *                                  bus-form entries runs the serial graph kernel's per-stream form, a wave
 *                                  per run of consecutive streams on one entry, and the one serial render
 *                                  behind it.  A call over register-form and bus-form streams is served:
 *                                  every stream of that call runs in bus form (a register-form list is a
 *                                  valid input to the reference's per-frame loop), and the persistent bus
 *                                  is the same either way, so a register-form stream called alone, or with
 *                                  other register-form streams, takes its usual kernels again.
 *                                  A fresh context has it off and refuses exactly as listed above, so a
 *                                  host that relies on the refusals sees no change.  (ctx, 0) turns it off
 *                                  again; ICW_EUNSUPPORTED, changing nothing, while the count is above 1
 *                                  and some entry is bus form.  NULL ctx: ICW_EINVAL.
 *                                  Still refused (ICW_EUNSUPPORTED, nothing changes) while a bus-form
 *                                  entry is in force beside a count above 1, or on the call that would
 *                                  create that state: icw_set_stream_render / icw_set_stream_hilbert that
 *                                  leave their count above 1 (and a bus-form list while either count is
 *                                  above 1, as icw_set_graph refuses it); icw_set_fir_hilbert(k_M > 0),
 *                                  and the list while the converter is on; a cfg.fp_check context; the
 *                                  list primitives, as ever while the lists differ.  Not served: icw_group
 *                                  and the icw_amod_* drop-in. */
int icw_enable_stream_bus(icw_ctx *ctx, int on);
int icw_set_stream_graph(icw_ctx *ctx, int first, int count, const icw_node *nodes, int n_nodes,
                         int bypass_list, int *accepted);
int icw_clear_stream_bus_slot(icw_ctx *ctx, int first, int count, int slot);
int icw_stream_graph_count(const icw_ctx *ctx);
/* The form a list would compile to, on the host alone (no context, no device): 0 the register form
 * (icw_set_stream_graph takes it), 1 the bus form (context-wide only), ICW_EGRAPH a list amod_init
 * or the compiler rejects.  icw_transcode_files_lists sorts its files with it. */
int icw_graph_form(const icw_config *cfg, const icw_node *nodes, int n_nodes, int bypass_list);
/* icw_set_outbits <- sound_render_set_outbits (sound_render.c:617-621), which mod_context_fopen
 *                    applies to both renders with the.cfg.need24bits at every track open
 *                    (in_cwave.c:212, 233-234; the GUI flips the flag between tracks,
 *                    amod_gui_control.c:1641): 16 (0) or 24 (!= 0) output bits for every stream of
 *                    the context.  New bounds, norm_mul and norm_shift, then sound_render_recalc:
 *                    prev_rnd, the shaper rings and prev_ns_err restart (also at an unchanged
 *                    depth), the MT19937 generators go on.  The peaks so far are kept in dB against
 *                    the old bound; icw_render_size follows the new depth. */
int icw_set_outbits(icw_ctx *ctx, int need24bits);
int icw_set_hilbert_filter(icw_ctx *ctx, uint32_t type);
int icw_set_hilbert_config(icw_ctx *ctx, int kahan, int subnorm_reject);

/* Per-stream renders: a batch whose streams each carry their own render -- output depth, dither type,
 * quantiser, noise shaper, sign bits (the reference reads need24bits per track, in_cwave.c:212, and its
 * SR_VCONFIG is an ordinary per-job setting) -- in ONE context, so a host that wants some tracks as 16-bit
 * TPDF + MEW44 and others as 24-bit ROUND keeps the batch width.
 *   icw_set_stream_render     icw_set_render followed by icw_set_outbits for streams [first, first + count)
 *                             only, in force from the next call on (the context's work is waited for).  For
 *                             those streams: new constants, prev_rnd, the shaper rings and prev_ns_err
 *                             restart (also when the setting is unchanged, as sound_render_recalc does),
 *                             the MT19937 words go on, and the peaks so far are folded into the stream's dB
 *                             meter against its old bound.  A context whose renders were all ROUND + flat
 *                             gets its serial-render state on the first edit that needs it, seeded as
 *                             icw_set_render seeds it.  The context keeps the distinct (render, depth)
 *                             entries and an index per stream; streams given the same pair share one
 *                             entry, unused entries go, and one entry left is a one-render context again,
 *                             which issues the launches it always did.
 *   icw_stream_render_count   distinct (render, depth) pairs in force (1 on a fresh context).
 *   icw_stream_render_size    bytes per output channel-sample of stream s: 2 or 3.  icw_render_size returns
 *                             the largest in force, so a buffer sized by it stays large enough.
 * icw_set_render and icw_set_outbits keep their meaning, every stream: icw_set_render gives every stream the
 * new icw_render_cfg and keeps each stream's own depth (the table collapses to as many entries as depths in
 * force); icw_set_outbits gives every stream the new depth and keeps each stream's own icw_render_cfg; each
 * restarts the shaping state of every stream, as ever.  icw_get_meters converts stream s's peak against
 * stream s's own bound.
 * A call's output layout: stream s starts at out + s*out_stride_bytes, as ever, and its frames have that
 * stream's own size, 4 or 6 bytes; out_stride_bytes must hold n_frames frames of every stream of the call
 * (device pointers included where the call's streams differ), else ICW_EINVAL.  Host staging rows are sized
 * by the widest, and a call over differing renders does not take the block-by-block copy of pinned host
 * buffers.  A call whose streams all share one entry (a one-stream call included) is resolved on the host
 * and launches exactly what a one-render context with that entry launches; only a call over differing
 * entries takes the new path: the output kernel leaves every stream's pre-render doubles, the serial
 * entries' streams go through the dither generator and the serial render in runs of consecutive streams
 * with one entry, and one kernel renders every stream whose entry is frame-parallel.
 * Per-stream lists and per-stream inputs, real and CWAVE, are served in the same context, in any order of
 * the setters; host and device pointers; icw_process_batch and icw_process_streams.
 * Limits, each refusal changing nothing:
 *   ICW_EINVAL        a range outside the context, render == NULL, or a field of it out of range.
 *   ICW_EUNSUPPORTED  while the count is above 1, or on the call that would raise it above 1:
 *                     - the FIR converter on (k_M > 0), and icw_set_fir_hilbert(k_M > 0);
 *                     - a cfg.fp_check context;
 *                     - a bus-form list in force, and icw_set_graph (or a list primitive) with a bus-form
 *                       list.
 * Not served: icw_group and the icw_amod_* drop-in (their render stays context-wide).  Per-file renders are
 * icw_transcode_files_jobs (icw_reader.h); the other icw_transcode_files* entry points take one render.  The two
 * encoders run no render and are not concerned.  The state blob does not
 * carry the render selection, as it carries neither list nor input: icw_set_state expects the stream's
 * render to be set as it was. */
int icw_set_stream_render(icw_ctx *ctx, int first, int count, const icw_render_cfg *render, int need24bits);
int icw_stream_render_count(const icw_ctx *ctx);      /* distinct (render, depth) in force; 1 on a fresh context */
int icw_stream_render_size(const icw_ctx *ctx, int s); /* bytes per output channel-sample of stream s: 2 or 3 */

/* Per-stream Hilbert converters: a batch whose streams each carry their own quadrature IIR converter -- the
 * type (IIR_HBLPF_IX of a job's in_cwave.cfg, 0..5: orders 15 / 19 / 18 / 19 / 20 / 20), the summation
 * (IIR_SUM_KAHAN) and the subnormal reject (IIR_SUBN_ZERO) -- in ONE context, so a host that serves jobs from
 * several configs keeps the batch width, and with it the rate of the serial recurrence that bounds every
 * real-input call.
 *   icw_set_stream_hilbert    icw_set_hilbert_filter followed by icw_set_hilbert_config for streams [first,
 *                             first + count) only, in force from the next call on (the context's work is
 *                             waited for).  A stream whose type changes has its converters re-created as
 *                             hq_rp_create does (zero rings, phases 0, de-subnorm counters 0, the left / right
 *                             identity known again); a stream already at that type keeps its rings.  The
 *                             de-subnorm counters of every stream of the range restart, also when the setting
 *                             is unchanged (iir_rp_setcfg).  The context keeps the distinct (type, kahan,
 *                             reject) entries, each with its order and coefficients, and an index per stream;
 *                             streams given the same setting share one entry, unused entries go, and one
 *                             entry left is a one-setting context again, which issues the launches it always
 *                             did.
 *   icw_stream_hilbert_count  distinct (type, kahan, reject) settings in force (1 on a fresh context).
 * icw_set_hilbert_filter and icw_set_hilbert_config keep their meaning, every stream: icw_set_hilbert_filter
 * gives every stream the type and keeps each stream's summation and reject (only the streams whose type
 * differs are re-created); icw_set_hilbert_config gives every stream the summation and the reject, keeps each
 * stream's type and rings, and restarts every counter.
 * A call whose streams all share one entry (a one-stream call, a subset inside one run) is resolved on the
 * host and launches exactly what a one-setting context with that entry launches.  Only a call over differing
 * entries takes the new path: its streams are cut into runs of consecutive streams with one entry; the
 * recurrence is one launch of a mixed kernel over all runs (the row form when every entry of the call is
 * Kahan + reject and the automatic rule holds on the launch's real waves -- every run rounds up to whole wave
 * pairs --, else the lane form; ICW_K1_MODE forces either as ever), and the output kernel runs once per run.
 * Many short runs therefore cost many small output launches.  A CWAVE-input call runs no recurrence and is
 * not concerned.  The state blob records the stream's own order; it does not carry the selection, as it
 * carries neither list, input nor render: icw_set_state expects the stream's setting to be as it was.
 * Per-stream lists, per-stream inputs (real and CWAVE) and per-stream renders are served in the same
 * context, in any order of the setters; host and device pointers; icw_process_batch and icw_process_streams.
 * Limits, each refusal changing nothing:
 *   ICW_EINVAL        a range outside the context, or type > 5.
 *   ICW_EUNSUPPORTED  while the count is above 1, or on the call that would raise it above 1:
 *                     - the FIR converter on (k_M > 0), and icw_set_fir_hilbert(k_M > 0);
 *                     - a cfg.fp_check context;
 *                     - a bus-form list in force, and icw_set_graph (or a list primitive) with a bus-form
 *                       list;
 *                     and, while the count is above 1, the two context encoders icw_encode_cwave and
 *                     icw_encode_cwave_iir.
 * Not served: icw_group and the icw_amod_* drop-in (their converter stays context-wide).  Per-file converter
 * settings are icw_transcode_files_jobs (icw_reader.h), which keeps the streams of one setting adjacent; the
 * other icw_transcode_files* entry points take one setting. */
int icw_set_stream_hilbert(icw_ctx *ctx, int first, int count, uint32_t type, int kahan, int subnorm_reject);
int icw_stream_hilbert_count(const icw_ctx *ctx);     /* distinct (type, kahan, reject) in force; 1 on a fresh context */

/* FIR Hilbert converter: the converter that CWAVE files record in their header (cwave.h:40,56-58:
 * "Hilbert FIR filter order" k_M, "Hilbert FIR filter parameter" k_beta; gui_cwave.c:159-172 shows
 * them; the converter program is not part of in_cwave).  With k_M > 0, real input is turned on the
 * device into the analytic signal such a file would hold -- a Kaiser-windowed (beta = k_beta)
 * Hilbert FIR of order k_M, odd taps m only, delay k_M/2:
 *     I[n] = x[n - k_M/2],  Q[n] = sum_{m odd <= k_M/2} g_m (x[n - k_M/2 - m] - x[n - k_M/2 + m]),
 *     g_m = 2 I0(beta sqrt(1 - (2m/k_M)^2)) / (pi m I0(beta)),  summed in ascending m with an FMA
 * per tap -- and the block continues as CWAVE input does (no quadrature IIR; graph and render as
 * for complex samples).  k_M = 0 restores the reference's own quadrature IIR Hilbert (the default).
 * k_M even, 2..ICW_FIR_MAX_ORDER.  Every stream's FIR history (its last k_M inputs) starts at zero;
 * icw_stream_init / icw_stream_reset_hilbert / icw_stream_open(clr_hilb) clear it too.
 * icw_set_fir_hilbert gives every stream the converter -- one k_M, one k_beta -- or turns it off with 0.
 * Per-stream FIR converters: a batch whose streams each carry their own (k_M, k_beta), as every CWAVE header
 * records its own, in ONE context, so a host that encodes or decodes a library at several orders keeps the
 * batch width.
 *   icw_set_stream_fir        icw_set_fir_hilbert for streams [first, first + count) only, in force from the
 *                             next call on (the context's work is waited for).  The streams of the range
 *                             start from a zero FIR history, also when the setting is unchanged (as
 *                             icw_set_fir_hilbert does for every stream); every stream outside the range keeps
 *                             its history bit for bit, whatever the edit does to the largest order in force.
 *                             The context keeps the distinct (k_M, bit pattern of k_beta) entries, each with
 *                             its taps, and an index per stream; streams given the same pair share one entry,
 *                             unused entries go, and one entry left is a one-converter context again, which
 *                             issues the launches it always did.
 *   icw_stream_fir_count      distinct (k_M, k_beta) in force; 1 on a fresh context and with the converter off.
 * icw_set_fir_hilbert keeps its meaning, every stream, and leaves one entry.  In a context with more than one
 * entry every converter call takes the kernels' per-stream form -- also a call whose own streams share an
 * entry; the bytes are the same either way.  A workgroup is one stream and works at its stream's own order; a
 * launch's LDS is sized by the widest order among its streams, and where some stream of a call does not fit
 * the fused kernel the call runs the converter and the output kernel apart, as a one-converter call does.
 * All FIR or none: k_M == 0 is accepted only for the whole context (first == 0, count == n_streams), where it
 * is icw_set_fir_hilbert(ctx, 0, ..); k_M > 0 on a proper sub-range of a context whose converter is off is
 * refused.
 * The state blob is sized by the largest order in force (icw_state_size), records the stream's own order and
 * carries that many history doubles per channel (the rest of the blob is zero); icw_set_state takes a blob of
 * at least the fixed part plus its own order's history, and returns ICW_EINVAL when the blob's order is not
 * the target stream's.  It does not carry the selection, as it carries no other.
 * icw_encode_cwave writes stream s with stream s's own converter once the host asked for both
 * icw_enable_stream_encode and icw_enable_stream_fir (ICW_EUNSUPPORTED while the count is above 1 without
 * the former); the frames are byte for byte those a one-converter context of that pair writes.
 * Limits, each refusal changing nothing:
 *   ICW_EINVAL        a range outside the context; k_M odd, negative or above ICW_FIR_MAX_ORDER; k_beta outside
 *                     [0, 1e3).
 *   ICW_EUNSUPPORTED  - icw_enable_stream_fir not on (the per-stream kernel instances serve this);
 *                     - the two all-or-none cases above;
 *                     - a cfg.fp_check context;
 *                     - what icw_set_fir_hilbert(k_M > 0) refuses: per-stream CWAVE inputs, a bus-form list
 *                       beside others, per-stream renders or per-stream IIR Hilbert settings with a count
 *                       above 1;
 *                     icw_set_stream_render and icw_set_stream_hilbert keep refusing while the converter is
 *                     on, and icw_enable_stream_fir(ctx, 0) is refused while the FIR count is above 1.
 * Not served: icw_group, the icw_amod_* drop-in and every file entry point (icw_reader.h: they keep their one
 * k_M).
 *   icw_enable_stream_fir(ctx, 1)  serves per-stream lists (icw_set_stream_graph) and per-stream inputs
 *                                  (icw_set_stream_input) beside the converter from then on: the three
 *                                  setters work in any order, the converter on or off at any count, and
 *                                  the converter's kernels take each stream's own list, rate and format.
 *                                  A fresh context has it off and keeps the refusals listed at the two
 *                                  setters, so a host that relies on them sees no change.  (ctx, 0) turns
 *                                  it off again; ICW_EUNSUPPORTED, changing nothing, while the converter
 *                                  is on and either count is above 1.  icw_transcode_files_fir sets it
 *                                  on its own contexts.
 * No reference implementation exists for this stage: its parity is unpinned. */
#define ICW_FIR_MAX_ORDER 4096
int icw_set_fir_hilbert(icw_ctx *ctx, int32_t k_M, double k_beta);
int icw_enable_stream_fir(icw_ctx *ctx, int on);
int icw_set_stream_fir(icw_ctx *ctx, int first, int count, int32_t k_M, double k_beta);
int icw_stream_fir_count(const icw_ctx *ctx);   /* distinct (k_M, k_beta) in force; 1 on a fresh context and with the converter off */
/* The taps of that design: g[k] = g_{2k+1}, k < nt = (k_M/2 + 1)/2.  Returns nt (or ICW_EINVAL). */
int icw_fir_taps(int32_t k_M, double k_beta, double *g, int n);

/* Process n_frames frames of every stream (the batched amod_process_samples).
 *   in  : stream s starts at (char*)in  + s*in_stride_bytes,  frames interleaved by channel
 *         in cfg->in_format (what xwave_read_samples leaves in xr->tbuff).
 *   out : stream s starts at (char*)out + s*out_stride_bytes, interleaved L,R, 2 or 3 bytes LE.
 *   dbg : ICW_F_DEBUG_PRE only -- double[n_streams][n_frames][2] pre-render values (lOut,rOut).
 * Host pointers are staged through pinned buffers; host buffers that are pinned themselves
 * (icw_host_alloc, hipHostMalloc, hipHostRegister) are copied block by block on a copy stream,
 * beside the kernels of the other launch blocks.  With ICW_F_DEVICE_PTRS nothing crosses PCIe.  hip_stream: the hipStream_t the call is ordered on (it starts after the work queued there,
 * and the stream's later work sees its results; the call returns before the kernels finish).
 * NULL: with host pointers the context's own stream (the call returns when its output is in
 * `out`); with ICW_F_DEVICE_PTRS the legacy default stream (stream 0, torch's default stream): the
 * call starts after the work queued there and returns when its output is in place.
 * icw_get_meters / icw_n_frame / icw_get_state wait for the context's work.  Returns ICW_OK. */
int icw_process_batch(icw_ctx *ctx, const void *in, size_t in_stride_bytes, void *out,
                      size_t out_stride_bytes, int n_frames, unsigned flags, void *dbg,
                      void *hip_stream);
/* Same for a subset of streams [first, first+count) (e.g. one decode thread's stream). */
int icw_process_streams(icw_ctx *ctx, int first, int count, const void *in,
                        size_t in_stride_bytes, void *out, size_t out_stride_bytes,
                        int n_frames, unsigned flags, void *dbg, void *hip_stream);

/* Warm a FRESH context (no call made yet) for calls of up to n_frames frames per stream (0: 4096,
 * the longest one-launch call of one stream): one call of silence through the path its
 * configuration takes, then the fresh state back (icw_stream_init).  The pinned staging, the device
 * buffers and the lazily loaded kernel code objects are then in place, so the first real call costs
 * what the later ones do -- the DecodeThread's first block (playback.c:619) included.
 * icw_mod_context_create calls it.  ICW_EINVAL once a call has been made, or once per-stream state
 * was set another way (icw_stream_open, _seek, _reset_hilbert, _reset_framecnt, icw_set_state), since
 * the closing icw_stream_init would wipe it.  Context-wide settings (icw_set_input, _set_graph,
 * _set_render, _set_outbits, the Hilbert setters) may come first: the warm-up runs with them. */
int icw_prepare(icw_ctx *ctx, int n_frames);

int icw_synchronize(icw_ctx *ctx);
/* Pinned (page-locked) host memory for a call's in / out buffers: their copies then overlap the
 * kernels (cudaMallocHost-style helper; the reference's buffers are the caller's own).  0 / ICW_ENOMEM. */
int icw_host_alloc(size_t bytes, void **p);
int icw_host_free(void *p);
/* Whether a host buffer takes the block-by-block copies on a context of `device`: 1 when it is
 * page-locked and was pinned while `device` was current or pinned portable (icw_host_alloc,
 * hipHostMallocPortable, hipHostRegisterPortable), 0 otherwise (the call then stages it through the
 * context's own pinned buffers: correct for any host memory, without the overlap). */
int icw_host_pinned(const void *p, int device);
/* Meters of stream s (amod_get_clips_peaks, adv_modulator.c:445-465).  reset != 0 clears the clip
 * counters and peaks FIRST, as the reference does, so the call returns 0 clips and
 * ICW_SR_ZERO_SIGNAL_DB peaks; the de-subnorm count is not reset (mod_context_get_desubnorm_counter,
 * in_cwave.c:300-310).  Waits for the context's running work. */
int icw_get_meters(icw_ctx *ctx, int s, int reset, icw_meters *m);
int icw_render_size(const icw_ctx *ctx);     /* bytes per output channel-sample: 2 or 3 */
int icw_n_frame(icw_ctx *ctx, int s, uint64_t *n_frame);

/* Serialisable per-stream state (checkpoint / resume).  Canonical layout documented
 * in DESIGN.md: IIR histories most-recent-first, Hilbert phases, n_frame, bus, render state. */
size_t icw_state_size(const icw_ctx *ctx);
int icw_get_state(icw_ctx *ctx, int s, void *blob, size_t size);
int icw_set_state(icw_ctx *ctx, int s, const void *blob, size_t size);

/* Kernel timing of the last icw_process_* call, measured with HIP events on the stream the
 * kernels ran on (bench.py roofline).  ms[0] = IIR state kernel total, ms[1] = output kernel
 * total, launches[0..1] = launch counts. */
int icw_last_timing(icw_ctx *ctx, double ms[2], int launches[2]);
/* The same for the input prep kernel K0 of that call, summed over its launch blocks (0 for a one-stream
 * call that ran as one kernel, and under the FIR converter, whose kernel is ms[0] above). */
int icw_last_k0_timing(icw_ctx *ctx, double *ms);

/* IIR state kernel (the serial recurrence) the last real-input icw_process_* call ran: ICW_K1_*.
 * The host picks the row-broadcast kernel for small batches (its waves fit two per CU on half
 * the chip, Kahan sum with the reject) and the lane-per-chain kernel otherwise;
 * ICW_K1_MODE=plain|row in the environment at icw_create forces one (A/B runs).  Codes 1 and 2
 * named two archived experiments (tools/k1_experimental.hip) and are no longer returned. */
#define ICW_K1_LANE   0   /* icw_iir_state: one lane per DF-II chain */
#define ICW_K1_ROW    3   /* icw_iir_row: one 16-lane DPP row per chain */
#define ICW_K1_FC     4   /* icw_iir_state_fc: FP_CHECK (cfg.fp_check) arithmetic and census */
int icw_last_k1_kernel(const icw_ctx *ctx);

/* The split dither generator cuts a launch block into chunks, as many frames as its word rows hold
 * (DESIGN 4).  Returns the number of chunks of the first launch block of the last icw_process_* call, 0 if
 * that call ran no generator (a ROUND render); chunk_frames, which may be null, receives the chunk length
 * used for that block (the last chunk may be shorter). */
int icw_last_dither_chunks(const icw_ctx *ctx, int *chunk_frames);

/* FP-exception census of stream s (FP_EXCEPT_STATS, fp_check.h:62-72) when cfg.fp_check is set:
 * counts[0] Hilbert left (mc->fes_hilb_left), [1] Hilbert right, [2] render left (fes_sr_left),
 * [3] render right; each {total, snan, qnan, ninf, nden, pden, pinf}.  reset != 0 clears them
 * afterwards (except_stats_reset, fp_check.c:36-48). */
#define ICW_FES_N 7
int icw_get_fp_census(icw_ctx *ctx, int s, int reset, uint32_t counts[4][ICW_FES_N]);

const char *icw_version(void);
const char *icw_strerror(int status);

/* The C ABI's version, for bindings to check at load time against the header they were built with.
 *   1  rounds 1-4;
 *   2  icw_mod_context_fopen takes need24bits (its 11th argument, in_cwave.c:212) -- a binding built
 *      against version 1 would pass an undefined bit depth.
 * Entry points that were only added (the per-stream setters and their opt-ins, icw_enable_stream_cwave,
 * icw_last_dither_chunks, icw_enable_stream_bus, icw_set_stream_fir the latest) leave it: a binding built against an earlier header of version 2 still
 * calls what it knows. */
#define ICW_ABI_VERSION 2
int icw_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ICW_H_ */
