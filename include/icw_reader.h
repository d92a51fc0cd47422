/*
 * icw_reader.h -- file-side ingestion: the reference's WAV / CWAVE header acceptance rules and a
 * batched transcoder that streams many files through the GPU path with pinned, double-buffered
 * host staging (the many-file form of the reference's transcode.c loop).
 *
 * Reference interfaces replaced (file:line into the reference tree):
 *   icw_wav_parse_file   <- xwave_reader_create (xwave_reader.c:593-700): extension check
 *                           (check_file_ext, xwave_reader.c:118-131), rwave_reader_create
 *                           (xwave_reader.c:362-585) / cwave_reader_create (xwave_reader.c:243-339),
 *                           the MAX_FS_SRC check (xwave_reader.c:672-674)
 *   icw_transcode_files  <- winampGetExtendedRead_open / _getData / _close (transcode.c:39-120)
 *                           driving amod_process_samples per block, for n files at once: each file
 *                           is one stream of a context; the output is the 2-channel 16/24-bit PCM
 *                           the transcoder returns, written as a WAV file
 */
#ifndef ICW_READER_H_
#define ICW_READER_H_

#include "icw.h"

#ifdef __cplusplus
extern "C" {
#endif

/* header type of a RIFF/WAVE file (HRW_HTYPE_*, in_cwave.h) */
#define ICW_HTYPE_WFONLY 0      /* WAVEFORMAT only: bits per sample derived from nBlockAlign */
#define ICW_HTYPE_PCMW   1      /* PCMWAVEFORMAT / WAVE_FORMAT_IEEE_FLOAT */
#define ICW_HTYPE_EXT    2      /* WAVEFORMATEXTENSIBLE */
#define ICW_HTYPE_CWAVE  3      /* a CWAVE file */

typedef struct icw_wav_info {
    uint32_t fmt;               /* ICW_FMT_* (ICW_FMT_CW_* for CWAVE) */
    uint32_t channels;          /* 1 or 2 */
    uint32_t sample_rate;
    uint32_t frame_bytes;       /* bytes per frame in the file */
    int64_t  n_samples;         /* frames in the data part */
    int64_t  data_offset;       /* byte offset of the data part */
    uint32_t htype;             /* ICW_HTYPE_* */
    uint32_t reserved_;
} icw_wav_info;

/* Open `path` the way xwave_reader_create does: the extension selects the reader (".wav" and
 * ".rwave" -> RIFF/WAVE, ".cwave" -> CWAVE; case-insensitive), then the header must pass the
 * reference's checks.  Returns ICW_OK and fills *info, or ICW_EINVAL for a file the reference
 * would refuse (ICW_ENOMEM / ICW_EDEVICE never; I/O errors read as refusals). */
int icw_wav_parse_file(const char *path, icw_wav_info *info);

typedef struct icw_batch_opts {
    uint32_t fade_in_ms, fade_out_ms;   /* FADE_IN / FADE_OUT */
    uint32_t sec_align;                 /* SEC_ALIGN: virtual zero tail to a multiple of it, s */
    int32_t  block_frames;              /* frames per stream per GPU block (0: 65536) */
    int32_t  device;                    /* HIP device, -1: current */
    int32_t  reserved_;                 /* flags word, ICW_BATCH_* (the member keeps its name; 0: the grouping below) */
} icw_batch_opts;

/* icw_batch_opts.reserved_ bits.  ICW_BATCH_MERGE_INPUTS: icw_transcode_files, _lists and _devices put
 * all real-input (WAV / RWAVE) files into ONE context per device, whatever their rate, format and
 * channels -- every stream gets its file's input through icw_set_stream_input (and its list where
 * lists differ) -- so a library of mixed formats keeps the batch width.  CWAVE files keep the grouping
 * by (rate, format, channels), a bus-form list still runs in a context of the files that carry the
 * same list, fades and tails are per file at the file's rate, and stats->n_groups counts contexts.
 * ICW_BATCH_MERGE_CWAVE: the same for the CWAVE files -- all of them in ONE context per device (another one
 * than the real-input files': a call covers streams of one kind), which has icw_enable_stream_cwave on and
 * gives every stream its file's CWAVE format, channels and rate, so a library encoded in the four frame
 * formats, mono and stereo, at several rates decodes at full batch width.  Honoured by icw_transcode_files,
 * _lists, _devices and _fir (there the CWAVE context runs without the converter, as CWAVE groups do).  The
 * bits are independent; without a bit that kind of file is grouped as before, and the output bytes are the
 * same either way.
 * ICW_BATCH_MERGE_BUS: icw_transcode_files_lists puts the bus-form files of a group into ONE context, which
 * has icw_enable_stream_bus on and gives every stream its file's list, instead of one context per distinct
 * bus-form list; with ICW_BATCH_MERGE_INPUTS that is all real-input bus-form files.  Register-form files keep
 * their own context (in a call forced into bus form they would lose the frame-parallel output kernel).  The
 * output bytes are the same with and without the bit.  icw_transcode_files and _devices carry one list, so
 * there is nothing for the bit to merge; icw_transcode_files_fir ignores it (the converter refuses bus-form
 * lists beside others), as does a cfg.fp_check call. */
#define ICW_BATCH_MERGE_INPUTS 1
#define ICW_BATCH_MERGE_CWAVE  2
#define ICW_BATCH_MERGE_BUS    (1 << 2)   /* 4: the third bit of the flags word */

typedef struct icw_batch_stats {
    int32_t  n_files, n_groups;         /* files transcoded; contexts used (one per input format) */
    uint64_t frames_in, frames_out;     /* data frames read; frames written (tails included) */
    double   wall_s;                    /* whole call */
    double   io_s;                      /* host time spent reading and writing files */
} icw_batch_stats;

/* Transcode n files: in_paths[i] -> out_paths[i] (a 2-channel PCM WAV, 16 or 24 bit per
 * cfg->need24bits), every file a fresh stream (mod_context_init state) with its own fades and
 * tail.  Files are grouped by (sample rate, format, channels); each group is one context whose
 * streams advance together block by block while the host reads the next block and writes the
 * previous one (pinned buffers, a copy stream, HIP events).  status (nullable, n entries) gets
 * ICW_OK or the file's error.  Returns ICW_OK if every file was transcoded. */
int icw_transcode_files(const icw_config *cfg, const icw_node *nodes, int n_nodes, const char *const *in_paths,
                        const char *const *out_paths, int n, const icw_batch_opts *opts, icw_batch_stats *stats,
                        int *status);

/* icw_transcode_files with file i's own DSP list: nodes[i] / n_nodes[i], and bypass_list[i] where
 * bypass_list is not NULL (else cfg->bypass_list).  The grouping stays by (sample rate, format,
 * channels): one context per group, every stream given its list through icw_set_stream_graph
 * before the first block, so files that differ only in their lists keep one batch.  A file whose
 * list amod_init rejects gets ICW_EGRAPH in status and the rest of the batch completes.  A file
 * whose list compiles to the bus form (icw_graph_form: context-wide only) runs in a context of the
 * files of its group that carry the same list; stats->n_groups counts the contexts. */
int icw_transcode_files_lists(const icw_config *cfg, const icw_node *const *nodes, const int *n_nodes,
                              const int *bypass_list, const char *const *in_paths, const char *const *out_paths, int n,
                              const icw_batch_opts *opts, icw_batch_stats *stats, int *status);

/* icw_transcode_files_lists through the FIR Hilbert converter: icw_set_fir_hilbert(k_M, k_beta) is applied
 * to every context of real-input (WAV / RWAVE) files before the first block; CWAVE files are analytic
 * already and run as in icw_transcode_files_lists.  ICW_BATCH_MERGE_INPUTS is honoured: a library of mixed
 * formats with per-file lists goes through the converter in one context per device (per-stream inputs
 * and lists beside the converter, include/icw.h).  k_M and k_beta as icw_set_fir_hilbert takes them with
 * the converter on: k_M even, 2..ICW_FIR_MAX_ORDER (0 is refused: that call is icw_transcode_files_lists),
 * 0 <= k_beta < 1e3; anything else returns ICW_EINVAL before a file is opened -- nothing runs, nothing is
 * written, stats and status are left alone.
 * Not offered: a converter per file.  Every context of the call gets the one (k_M, k_beta); a context whose
 * streams each carry their own is icw_set_stream_fir's (icw.h). */
int icw_transcode_files_fir(const icw_config *cfg, const icw_node *const *nodes, const int *n_nodes,
                            const int *bypass_list, const char *const *in_paths, const char *const *out_paths, int n,
                            int32_t k_M, double k_beta, const icw_batch_opts *opts, icw_batch_stats *stats, int *status);

/* ---- a fixed pool of stream slots, refilled as files end ---- */
#define ICW_POOL_AS_GIVEN      0        /* files start in the order of the call's arrays */
#define ICW_POOL_LONGEST_FIRST 1        /* by frames (tail included), descending; equal lengths keep their order */

typedef struct icw_pool_opts {
    icw_batch_opts batch;               /* fades, sec_align, block_frames, device; the MERGE bits are ignored: a
                                           pool merges by construction */
    int32_t slots;                      /* streams per pool context; 0 or >= the kind's file count: one slot per file */
    int32_t order;                      /* ICW_POOL_* */
} icw_pool_opts;

typedef struct icw_pool_stats {
    icw_batch_stats batch;              /* n_groups counts pool contexts */
    int32_t  slots;                     /* widest pool used */
    int32_t  refills;                   /* files opened in a slot that had held another */
    uint64_t blocks;                    /* launch calls, summed over the pools */
    uint64_t slot_blocks, busy_slot_blocks;   /* slots * blocks; those in which the slot held frames of a file */
} icw_pool_stats;

/* icw_transcode_files_lists through pools of `slots` streams: a context no wider than the chip needs,
 * whatever the library's size, and no slot-blocks spent on files that have ended while the longest still
 * runs.  A slot whose file has ended is re-initialised (icw_stream_init: the state of a fresh context's
 * stream, every piece of it) and opens the next file of the queue at the next block boundary; the staging
 * buffers are slots * block_frames frames.
 * nodes / n_nodes / bypass_list are per file, as in icw_transcode_files_lists (NULL bypass_list: cfg's).
 * A call covers streams of one kind, so the files run in one pool context per kind, each of min(slots, files
 * of that kind) streams: real-input files with register-form lists; real-input files with bus-form lists
 * (icw_enable_stream_bus); CWAVE files (icw_enable_stream_cwave) -- those too apart by the form of their
 * lists, as ICW_BATCH_MERGE_BUS keeps them.
 * Per-file semantics are icw_transcode_files_lists' own: every file a fresh stream, fades and the sec_align
 * tail at the file's own rate, a 44-byte header and `total` frames, the same refusals and per-file status --
 * and the bytes of every output file equal what icw_transcode_files_lists writes for it, whatever slots,
 * order, block_frames and the file's neighbours are.
 * The schedule is a plan made before the first block (icw_pool_plan: the same function): a file starts at a
 * block boundary in the lowest-numbered free slot, files start in queue order, a slot is free from the block
 * after the one that holds its file's last frame (tail included).  stats are the plan's.  A file refused at
 * parse or open time takes no slot; one that fails mid-way (short read) keeps its status and its slot until
 * its planned end.  A slot with no file is fed the zero sample of its last input; its output is written
 * nowhere and counted in nothing.
 * meters (nullable, n entries): entry i gets file i's clips, peaks and de-subnorm count, read with
 * icw_get_meters after the file's last block and before its slot is re-initialised (a pool makes them
 * unrecoverable afterwards).  The last block is whole: up to block_frames - 1 frames of the zero sample
 * beyond `total` have gone through the stream by then.  Entries of files that took no slot are zero.
 * Returns ICW_EINVAL for slots < 0 or an unknown order (nothing runs, nothing is written) and
 * ICW_EUNSUPPORTED for cfg->fp_check; else ICW_OK if every file was transcoded, else one of the files'
 * errors, as icw_transcode_files_lists returns it.
 * Not offered: the FIR converter, the three CWAVE encoders, icw_transcode_files_devices / icw_group.  Per-file
 * renders and Hilbert settings: icw_transcode_files_jobs below.  Per-file FIR converters (icw_set_stream_fir,
 * icw.h, serves them in a context): no file entry point -- icw_transcode_files_fir and icw_cwave_encode_files keep
 * their one k_M, and neither the pool nor the jobs call runs the converter. */
int icw_transcode_files_pool(const icw_config *cfg, const icw_node *const *nodes, const int *n_nodes,
                             const int *bypass_list, const char *const *in_paths, const char *const *out_paths,
                             int n, const icw_pool_opts *opts, icw_pool_stats *stats, icw_meters *meters, int *status);

/* The plan icw_transcode_files_pool executes for ONE pool (host arithmetic; no device is touched).  total[i]:
 * file i's frames, tail included; a file with total <= 0 takes no slot.  slot / start_block (nullable, n
 * entries): file i's slot and the block in which it starts, -1 for a file that takes none.  stats (nullable):
 * slots, refills, blocks, slot_blocks and busy_slot_blocks of the plan; `batch` is zeroed.  block_frames 0:
 * 65536.  Returns ICW_EINVAL for slots < 0, block_frames < 0 or an unknown order. */
int icw_pool_plan(const int64_t *total, int n, int32_t slots, int32_t block_frames, int32_t order,
                  int32_t *slot, int64_t *start_block, icw_pool_stats *stats);

/* ---- the pool with per-file settings: every file a job of its own in_cwave.cfg ---- */
/* What a job takes from its configuration: the DSP list and, beyond what icw_transcode_files_pool carries per
 * file, the render with its depth and the Hilbert converter. */
typedef struct icw_file_job {
    const icw_node *nodes; int32_t n_nodes; int32_t bypass_list;
    icw_render_cfg render; int32_t need24bits;
    uint32_t hilbert_type; int32_t iir_kahan, iir_subnorm_reject;
} icw_file_job;

typedef struct icw_jobs_stats {
    icw_pool_stats pool;
    int32_t classes;                       /* distinct settings, summed over the pool contexts */
    int32_t hilbert_runs_max, render_runs_max;   /* the most runs any one call was cut into (from the plan) */
    double  kernel_s;                      /* with ICW_BATCH_TIMING: icw_last_timing summed over the blocks; else 0 */
} icw_jobs_stats;

/* icw_batch_opts.reserved_ bit of icw_transcode_files_jobs alone: every block's call runs with ICW_F_TIMING and
 * stats->kernel_s sums what icw_last_timing reports (the recurrence and the output kernel), in seconds.  The call
 * then waits for every block's kernels, so its wall time is not that of a run without the bit; the bytes are.
 * Every other file entry point ignores the bit, icw_transcode_files_pool included. */
#define ICW_BATCH_TIMING 8

/* job <- the per-job fields of a configuration (icw_config_load's icw_file_config.cfg, or a hand-made one): its
 * render, need24bits, hilbert_type, iir_kahan, iir_subnorm_reject and bypass_list, with the list given. */
void icw_file_job_from_config(const icw_config *cfg, const icw_node *nodes, int n_nodes, icw_file_job *job);

/* icw_transcode_files_pool with file i's own job: its list, its render and depth, its Hilbert converter.  A host
 * whose jobs come from several in_cwave.cfg files makes ONE call, and the files share pool contexts as wide as
 * the chip needs, instead of one call -- one narrow context -- per distinct setting.
 * cfg supplies what stays context-wide: frmod_scaled, the seeds, fp_check (ICW_EUNSUPPORTED, as the pool);
 * its render, need24bits, Hilbert and list fields are not read.
 * Kinds are the pool's, one pool context each: real input with register-form lists, real input with bus-form
 * lists, CWAVE input by the form of the list.  Within a kind, files of one setting are one CLASS:
 *   - real input, register form: equal (hilbert_type, kahan, reject) and equal (render, depth) -- the equalities
 *     of icw_set_stream_hilbert and icw_set_stream_render;
 *   - CWAVE input, register form: equal (render, depth) alone -- no recurrence runs, so two files that differ
 *     only in Hilbert fields are one class;
 *   - bus-form lists cannot stand beside differing renders or converters in one context (icw.h lists the
 *     refusals): each class of them runs in a pool context of its own, its setting installed context-wide.
 *     stats->pool.batch.n_groups counts contexts.
 * The plan (icw_pool_plan_classes below; icw_file_job_classes gives the classes) keeps every class in one
 * contiguous range of slots for the whole run, so the streams of one setting are neighbours whatever the order of
 * the files: a call is cut into as many Hilbert runs as the context has distinct Hilbert settings (classes that
 * share one are laid out side by side) and at most as many render runs as it has classes.  Before block 0 each
 * range gets its setting once (icw_set_stream_hilbert on real input, icw_set_stream_render on every range); a
 * refill is the pool's: input and list setters, icw_stream_init, icw_stream_open.
 * Limits: a range is never handed to another class, also when its queue is empty -- the price shows in
 * stats->pool.busy_slot_blocks / slot_blocks; a pool is at least as wide as it has classes, also when opts->slots
 * is smaller (stats->pool.slots reports the width used); frmod_scaled, the seeds and fp_check are not per file.
 * Output: every file's header carries its own depth (block align 4 or 6); staging rows are sized by the widest
 * frame of the context.  The bytes of every output file, header included, are those icw_transcode_files_lists
 * writes for that file with a config that carries the job's settings, whatever slots, order, block_frames and
 * the neighbours are.  meters as in the pool, each against its stream's own bound.
 * Per-file status as in the pool; a job whose render fields or hilbert_type are out of range gets ICW_EINVAL, a
 * rejected list ICW_EGRAPH: such a file takes no slot, belongs to no class, and the rest completes.
 * Not offered: what the pool does not offer. */
int  icw_transcode_files_jobs(const icw_config *cfg, const icw_file_job *jobs, const char *const *in_paths,
                              const char *const *out_paths, int n, const icw_pool_opts *opts,
                              icw_jobs_stats *stats, icw_meters *meters, int *status);

/* icw_pool_plan with classes: the plan icw_transcode_files_jobs executes for ONE pool context (host arithmetic).
 * cls[i] >= 0: file i's class; a file with total <= 0 takes no slot and its class counts for nothing.  K: the
 * distinct classes among the files that take a slot.
 * Every class gets one contiguous range of slots, fixed for the whole run; the ranges follow each other from
 * slot 0 in the order of each class's first file in the arrays.  The width is min(slots, files), all files for
 * slots 0, raised to K where it would be smaller.  A class's share of it is apportioned by largest remainder in
 * proportion to its busy slot-blocks, the sum of ceil(total / block_frames) over its files: a class whose
 * proportional part is below 1 gets one slot and the others share the rest in proportion; whole parts first,
 * then the leftover slots to the largest remainders, ties to the class laid out first.  A class given more than
 * its file count keeps its file count, and the slots so freed are apportioned among the other classes by the
 * same rule.  Within its range a class is planned as icw_pool_plan plans a pool of that many slots: lowest free
 * slot, queue order (as given or longest first, stable) among the class's files, a slot free from the block after
 * its file's last.  With one class the plan and its statistics are icw_pool_plan's.
 * stats (nullable): pool.slots (the width used), refills, blocks (the longest range's), slot_blocks,
 * busy_slot_blocks; classes = K; the classes are opaque here, so hilbert_runs_max = render_runs_max = K;
 * pool.batch and kernel_s are zeroed.  Returns ICW_EINVAL for what icw_pool_plan refuses and for a negative class
 * of a file that takes a slot. */
int icw_pool_plan_classes(const int64_t *total, const int32_t *cls, int n, int32_t slots, int32_t block_frames,
                          int32_t order, int32_t *slot, int64_t *start_block, icw_jobs_stats *stats);

/* The classes icw_transcode_files_jobs makes of the jobs of one pool context (host arithmetic): cls[i] is job
 * i's class as its position in the layout, -1 for a job whose fields are out of range; cwave != 0: the CWAVE rule
 * (render and depth alone).  Classes are ordered by the first appearance of their Hilbert setting, then of their
 * render, so classes that share a Hilbert setting are neighbours.  Files ordered by cls (stable) and given to
 * icw_pool_plan_classes give the transcoder's plan.  Returns the number of classes, or ICW_EINVAL. */
int icw_file_job_classes(const icw_file_job *jobs, int n, int cwave, int32_t *cls);

/* ---- convert: WAV files -> CWAVE files (the external converter cwave.h:56-58 names) ---- */
/* icw_cwave_enc_opts.reserved_ / icw_cwave_enc_iir_opts.reserved_ are the flags word (0: one context per
 * (rate, format, channels) group).  ICW_ENC_MERGE_INPUTS: every accepted file goes into ONE context, each
 * stream given its file's input (icw_set_stream_input, icw_enable_stream_encode; with the FIR converter
 * icw_enable_stream_fir), so a library of mixed formats pays the serial IIR once, at full batch width.
 * The files written are byte for byte those of the flag 0 -- header (each file's own channels and rate),
 * frames, n_CRC32 -- and `clipped` and the per-file status are the same; stats->n_groups is 1.  align = 1
 * is unchanged: every file drops its first k_M/2 frames. */
#define ICW_ENC_MERGE_INPUTS 1

typedef struct icw_cwave_enc_opts {
    int32_t  k_M;                       /* FIR Hilbert order: even, 2 .. ICW_FIR_MAX_ORDER */
    int32_t  align;                     /* 0: causal (what the in-context converter feeds the graph: file frame n
                                           holds I = x[n - k_M/2]); 1: delay-compensated (file frame n is centred
                                           on input frame n) */
    double   k_beta;                    /* Kaiser window parameter */
    uint32_t cw_format;                 /* ICW_FMT_CW_* of the output */
    int32_t  block_frames;              /* frames per stream per GPU block (0: 65536) */
    int32_t  device;                    /* HIP device, -1: current */
    int32_t  reserved_;                 /* flags: 0 or ICW_ENC_MERGE_INPUTS */
} icw_cwave_enc_opts;

/* Encode n WAV files: in_paths[i] -> out_paths[i], a V2 CWAVE file (magic, hsize 48, version 2, format,
 * channels, n_samples = the input's frames, rate, k_M, k_beta, n_CRC32) of icw_encode_cwave's frames
 * (icw_cwave.h: layout and conversions).  Files are grouped by (sample rate, format, channels), one
 * context per group; every file is one fresh stream with no fades and no tail, staged like
 * icw_transcode_files.  n_CRC32 is computed on the GPU over the packed frames while they are in HBM,
 * chained block by block (icw_crc32_batch); the host makes no CRC pass.
 * align = 1 is the causal encode of the input followed by k_M/2 zero frames, with the first k_M/2
 * output frames dropped (they count neither in the CRC nor in `clipped`).
 * status (nullable, n entries) gets ICW_OK or the file's error: ICW_EINVAL for a CWAVE input (already
 * analytic), a WAV icw_wav_parse_file refuses, fewer than 2 frames (the reader would refuse the result),
 * 2^32 frames or more, or an I/O error; the rest of the batch still completes.  clipped (nullable, n
 * entries) gets the file's saturated / NaN int16 samples.  Returns ICW_EINVAL for bad options (nothing
 * runs), else ICW_OK if every file was encoded, else one of the files' errors.
 * Not covered: V1 headers.  Not offered: a converter per file (one k_M and k_beta for the batch; per-stream
 * converters are icw_set_stream_fir with icw_encode_cwave, icw.h). */
int icw_cwave_encode_files(const char *const *in_paths, const char *const *out_paths, int n,
                           const icw_cwave_enc_opts *opts, icw_batch_stats *stats, uint64_t *clipped, int *status);

/* ---- convert with the reference's own converter: the quadrature half-band IIR (hq_rp_process) ---- */
typedef struct icw_cwave_enc_iir_opts {
    uint32_t hilbert_type;              /* filter type 0 .. 5 (icw_config.hilbert_type) */
    int32_t  iir_kahan;                 /* 0 / 1: baseline or Kahan sums */
    int32_t  iir_subnorm_reject;        /* 0 / 1: the `< 1.0` reject */
    uint32_t cw_format;                 /* ICW_FMT_CW_* of the output */
    int32_t  block_frames;              /* frames per stream per GPU block (0: 65536) */
    int32_t  device;                    /* HIP device, -1: current */
    int32_t  reserved_;                 /* flags: 0 or ICW_ENC_MERGE_INPUTS */
} icw_cwave_enc_iir_opts;

/* icw_cwave_encode_files through icw_encode_cwave_iir (icw_cwave.h): file frame n holds exactly the (I, Q)
 * pairs the in-context converter of that type and configuration feeds the graph at frame n, so playing the
 * .cwave file renders what playing the .wav renders -- the serial IIR is paid once, at the conversion.
 * Grouping, staging, the n_CRC32 chained on the GPU, per-file status and `clipped` as above; every file is
 * a fresh stream with no fades and no tail.  There is no aligned mode: the IIR's group delay is not a
 * constant number of frames.  The header is V2 with hsize 48, n_samples = the input's frames, k_M = 0 and
 * k_beta = 0.0 -- the reference's reader shows k_M 0 as an unknown converter (gui_cwave.c:164-170) and
 * plays the file like any other.  Returns ICW_EINVAL for bad options (hilbert_type > 5, a flag that is not
 * 0 or 1, a cw_format outside ICW_FMT_CW_*, block_frames < 0; nothing runs, nothing is written). */
int icw_cwave_encode_files_iir(const char *const *in_paths, const char *const *out_paths, int n,
                               const icw_cwave_enc_iir_opts *opts, icw_batch_stats *stats, uint64_t *clipped,
                               int *status);

/* ---- convert with the direct-FFT converter (k_M = -1): the Hilbert transform of the whole track ---- */
typedef struct icw_cwave_enc_fft_opts {
    uint32_t cw_format;                 /* ICW_FMT_CW_* of the output */
    int32_t  device;                    /* HIP device, -1: current */
    uint64_t max_bytes;                 /* device working-set budget of one call (PCM + transforms + frames);
                                           0: 16 GiB */
} icw_cwave_enc_fft_opts;

/* icw_cwave_encode_files through icw_encode_cwave_fft (icw_cwave.h: the definition): file frame n holds
 * I = the input's sample n and Q = the Hilbert transform of the whole zero-padded track at n -- no filter
 * order, no transition band, no delay.  The header is V2 with hsize 48, n_samples = the input's frames,
 * k_M = -1 ("direct FFT", gui_cwave.c:159-170) and k_beta = 0.0; n_CRC32 is computed on the GPU over the packed
 * frames while they are in HBM (icw_crc32_batch).  Tracks are whole: files are grouped by (format, channels)
 * -- the rate plays no part -- and packed, in order, into calls whose working set fits max_bytes (a file
 * that alone exceeds it runs alone).  Per-file status and `clipped` as above, and ICW_EUNSUPPORTED for a
 * track of more than 2^ICW_FFT_MAX_LOG2 frames; the rest of the batch still completes.  Returns ICW_EINVAL
 * for bad options (a cw_format outside ICW_FMT_CW_*; nothing runs, nothing is written). */
int icw_cwave_encode_files_fft(const char *const *in_paths, const char *const *out_paths, int n,
                               const icw_cwave_enc_fft_opts *opts, icw_batch_stats *stats, uint64_t *clipped,
                               int *status);

#ifdef __cplusplus
}
#endif
#endif /* ICW_READER_H_ */
