/*
 * icw_cwave.h -- CWAVE (complex wave) file support: the header checks of the reference's CWAVE
 * reader, and a batched GPU CRC32 for the integrity check of CWAVE data parts.
 *
 * Reference interfaces replaced (file:line into the reference tree):
 *   icw_cwave_parse    <- cwave_reader_create (xwave_reader.c:243-300): header field checks, the
 *                         sample format -> unpacker choice (xwave_reader.c:311-335)
 *   icw_crc32_batch    <- crc32init / crc32update / crc32final (crc32.c) as driven by check_cwave
 *                         (gui_cwave.c:82-129): CRC-32 (poly 0xEDB88320, reflected, init and final
 *                         inversion) over the data part, compared with HCWAVE_V2.n_CRC32
 *   icw_cwave_check    <- check_cwave (gui_cwave.c:82-129) on a file image in host or HBM memory
 *   icw_crc32_combine  <- the block-by-block crc32update chaining of check_cwave
 * The CWAVE sample data itself is decoded by icw_process_* with cfg.in_format = ICW_FMT_CW_*.
 */
#ifndef ICW_CWAVE_H_
#define ICW_CWAVE_H_

#include "icw.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ICW_CWAVE_HEADER_BYTES 48      /* 8 + 7 * 4 + 4 + 8: the known part, xwave_reader.c:255-256 */

/* HCWAVE_V2 (cwave.h:48-60).  A V1 header (cwave.h:31-43) has the same field positions, with pad0
 * where V2 has n_CRC32; the reference reads both the same way. */
typedef struct icw_cwave_header {
    char     magic[8];                 /* "cPLXwAVE" */
    uint32_t hsize;                    /* header size, data part starts here */
    uint32_t version;                  /* 1 or 2 */
    uint32_t format;                   /* HCW_FMT_PCM_* 0..3 */
    uint32_t n_channels;               /* 1 or 2 */
    uint32_t n_samples;                /* frames */
    uint32_t sample_rate;
    int32_t  k_M;                      /* external Hilbert FIR order (informational) */
    uint32_t n_crc32;                  /* CRC32 of the data part (V2) */
    double   k_beta;                   /* external Hilbert FIR parameter (informational) */
} icw_cwave_header;

/* Decode and validate the first ICW_CWAVE_HEADER_BYTES of a CWAVE file of file_size bytes, with
 * the reference's checks in the reference's order: magic, hsize (>= 48 and < file size), version
 * (1 or 2), format (<= 3), channels (1..2), n_samples (>= 2 and data part inside the file),
 * sample_rate != 0.  On success fills *h, the ICW_FMT_CW_* input format and the frame size in
 * bytes, and returns ICW_OK; returns ICW_EINVAL for a file the reference refuses. */
int icw_cwave_parse(const void *hdr, size_t hdr_len, int64_t file_size, icw_cwave_header *h,
                    uint32_t *icw_fmt, uint32_t *frame_bytes);

/* CRC-32 of n byte ranges [base + offsets[i], + lengths[i]) on the GPU, one pass over HBM.
 * crc_in[i] (nullable: 0) continues an earlier CRC the way zlib's crc32(crc, buf, len) does;
 * crc_out[i] receives the result.  With ICW_F_DEVICE_PTRS base is a device pointer (the ranges
 * are resident in HBM); otherwise it is a host pointer and the ranges are staged over PCIe.
 * offsets/lengths/crc_in/crc_out are host arrays.  device: HIP device (-1: current);
 * hip_stream: hipStream_t or NULL.  Returns ICW_OK when crc_out is filled. */
int icw_crc32_batch(const void *base, const uint64_t *offsets, const uint64_t *lengths, int n,
                    const uint32_t *crc_in, uint32_t *crc_out, unsigned flags, int device,
                    void *hip_stream);

/* CRC-32 of A||B from crc(A), crc(B) and |B| (GF(2) arithmetic on the host, no data access). */
uint32_t icw_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* check_cwave on a whole CWAVE file image (host or, with ICW_F_DEVICE_PTRS, device memory):
 * parses the header, CRCs the data part (n_samples * frame bytes from hsize) on the GPU.
 * *crc gets the computed CRC; *crc_ok is 1 if it equals n_CRC32, 0 if not, -1 for a V1 file
 * (no CRC stored; the reference only reports the value, gui_cwave.c:124-127). */
int icw_cwave_check(const void *file, uint64_t file_size, unsigned flags, int device, uint32_t *crc,
                    int *crc_ok);

/* ---- CWAVE encoders: real PCM -> the analytic-signal frames a CWAVE file holds ----
 * icw_encode_cwave: the converter is the context's FIR Hilbert (icw_set_fir_hilbert, k_M > 0): the same
 * kernel code stages and sums, so I[n] = x[n - k_M/2] and Q[n] are bit for bit what icw_process_* feeds the graph.
 * Frame layout (cwave.h:74-81), per channel Re then Im, stereo Re(L) Im(L) Re(R) Im(R):
 *   ICW_FMT_CW_F64 16 bytes, ICW_FMT_CW_I16 4, ICW_FMT_CW_I16_F32 6 (float unaligned), ICW_FMT_CW_F32 8.
 * Mono input gives 1-channel frames; input of 2 or more channels gives 2-channel frames of the first two.
 * Conversions (the project's definition; the reference ships no converter, so parity is unpinned, like
 * the FIR converter itself): double = the bits; float = round to nearest even; int16 = round to nearest,
 * ties to even, saturated to [-32768, 32767], NaN -> 0.
 * icw_encode_cwave_iir (below) writes the same frames from the quadrature IIR converter, whose values
 * are the reference's (hq_rp_process) bit for bit.  icw_encode_cwave_fft (at the end) writes them from the
 * direct-FFT converter (k_M -1): the Hilbert transform of the whole track.
 * Not covered: V1 headers. */

/* bytes of one frame of cw_format for an input of `channels` channels; 0 if either is invalid */
int icw_cwave_frame_bytes(uint32_t cw_format, uint32_t channels);

/* Encode n_frames frames of streams [first, first + count): stream i's PCM (the context's input
 * format) at in + i*in_stride, its CWAVE frames to out + i*out_stride.  Pointers, ICW_F_DEVICE_PTRS,
 * hip_stream and the ordering are those of icw_process_streams (host pointers: the call returns with
 * `out` filled; device pointers: stream-ordered); long calls run in launch blocks the same way.
 * For these streams the call advances the FIR history and the reader position (fades included)
 * exactly as a process call of n_frames would, so two calls equal one and icw_get_state /
 * icw_set_state carry an encode to another context.  It leaves n_frame, the bus, the IIR Hilbert, the
 * renders, the dither generators and the meters alone.
 * Errors: ICW_EINVAL -- nothing ran, no state changed -- for a bad range or pointer, a host stride
 * shorter than the frames, a flag other than ICW_F_DEVICE_PTRS, a cw_format outside ICW_FMT_CW_*, a
 * context with CWAVE input (already analytic) or without icw_set_fir_hilbert(k_M > 0).  ICW_ENOMEM /
 * ICW_EDEVICE: a buffer or a HIP call failed; the streams' state is then unspecified (reset or
 * icw_set_state them).
 * Per-stream inputs (icw_set_stream_input, include/icw.h).  While icw_stream_input_count() is above 1 both
 * encoders return ICW_EUNSUPPORTED, nothing run, unless the context asked with icw_enable_stream_encode(ctx, 1).
 * Then a call serves streams with different inputs: stream i's PCM at in + i*in_stride at its own frame size
 * (as icw_process_streams lays it out), its frames at out + i*out_stride at its own
 * icw_cwave_frame_bytes(cw_format, channels_i) -- bit for bit the bytes a one-input context writes for that
 * stream.  Both strides must hold n_frames frames of the call's widest stream -- in_stride of the widest input
 * frame, out_stride n_frames * icw_cwave_frame_bytes(cw_format, the call's most channels) -- for host and
 * device pointers alike, else ICW_EINVAL, nothing run, nothing written.  The rate plays no part in an
 * encode; a call whose streams share format and channels runs the kernels of a one-input context (the same
 * launches, the same arguments), and only a call over differing ones takes the per-stream kernel instances.
 * cw_format is one per call.  icw_encode_cwave beside differing inputs needs the converter there, hence
 * icw_enable_stream_fir (include/icw.h); without a converter it returns ICW_EINVAL as above. */
int icw_encode_cwave(icw_ctx *ctx, int first, int count, const void *in, size_t in_stride_bytes,
                     void *out, size_t out_stride_bytes, int n_frames, uint32_t cw_format,
                     unsigned flags, void *hip_stream);

/* The same call through the quadrature half-band IIR converter (hq_rp_process: cfg.hilbert_type 0..5,
 * iir_kahan, iir_subnorm_reject with its `< 1.0` reject), for a context without icw_set_fir_hilbert: frame n
 * holds, per channel, exactly the (I, Q) pair icw_process_* feeds the graph at frame n, so a stored file
 * decoded with cfg.in_format = ICW_FMT_CW_F64 renders what the PCM renders.  Frame layout, conversions,
 * pointers, ICW_F_DEVICE_PTRS, hip_stream, ordering and launch blocks (ICW_BLOCK) as in icw_encode_cwave.
 * Per launch block the call runs the process call's own kernels up to the graph (the unpack / fade / fs/4
 * mix, the recurrence the context would pick for a process call -- ICW_K1_MODE honoured --, the output
 * sums and un-mix) and a packer.
 * State: for these streams the IIR delay lines, the Hilbert phases, the de-subnorm counters
 * (icw_get_meters().desubnorm), the left / right identity flags and the reader position (fades included)
 * advance exactly as a process call of n_frames would.  n_frame, the bus, the FIR history, the renders,
 * the dither generators and the clip / peak meters are left alone.  So two calls equal one, icw_get_state /
 * icw_set_state carry an encode to another context, and a process call after an encode continues the
 * converters as if the encoded frames had been processed.
 * Errors: ICW_EINVAL -- nothing ran, no state changed -- for a bad range or pointer, a host stride shorter
 * than the frames, a flag other than ICW_F_DEVICE_PTRS, a cw_format outside ICW_FMT_CW_*, a context with
 * CWAVE input, or one with the FIR converter on (icw_set_fir_hilbert(k_M > 0): icw_encode_cwave is its
 * call).  ICW_EUNSUPPORTED for a cfg.fp_check context (FC() arithmetic changes the values), with or without
 * per-stream inputs.  ICW_ENOMEM / ICW_EDEVICE as above.
 * Per-stream inputs: as at icw_encode_cwave.  A call over differing inputs runs what a process call over
 * them runs up to the graph (the table-reading unpack, the same recurrence, the output sums of each stream's
 * own channels); the mono left = right shortcut applies when every stream of the call is mono, and a call
 * ends the left / right identity of its stereo streams only. */
int icw_encode_cwave_iir(icw_ctx *ctx, int first, int count, const void *in, size_t in_stride_bytes,
                         void *out, size_t out_stride_bytes, int n_frames, uint32_t cw_format,
                         unsigned flags, void *hip_stream);

/* Saturated or NaN int16 samples (Re and Im counted separately) stream s has encoded, by either
 * encoder (one counter), since the count was last reset; waits for the context's queued work.  reset != 0 clears it after the read.
 * clipped may be NULL. */
int icw_encode_clipped(icw_ctx *ctx, int s, int reset, uint64_t *clipped);

/* ---- the direct-FFT converter (k_M = -1, cwave.h:40,56; gui_cwave.c:159-170): whole-track analytic signal ----
 * Definition (the project's: the reference ships no converter, so parity is unpinned).  For one
 * channel of one track x[0..N) -- the reader's unpacked doubles on the 16-bit scale, no fades, no tail, a
 * fresh stream, as in the other two encoders --
 *   P = the smallest power of two >= max(N, 2); x zero-padded to P;
 *   Q = Re( IDFT_P( m[k] * DFT_P(x)[k] ) ),  m[k] = -j for 0 < k < P/2, +j for k > P/2, m[0] = m[P/2] = 0,
 *   DFT the forward transform sum x[n] e^(-2 pi j k n / P), IDFT its inverse with the factor 1/P
 * (scipy.signal.hilbert(x, P).imag; x = A cos(theta) gives Q = A sin(theta), so I + jQ rotates positively).
 * File frame n < N holds I[n] = x[n], the unpacked sample itself bit for bit (never the transform's round
 * trip), and Q[n].  Frame layout, mono / stereo rules and conversions are icw_encode_cwave's (above).
 * There is no design parameter, no transition band at DC or Nyquist and no group delay.
 * The bytes of a track depend only on that track and on opts->max_pass_log2: not on what else is in the
 * call, nor on the pointer kind.  The transform is a multi-pass radix-2 FP64 FFT on the GPU; a stereo pair
 * runs as one complex transform (L + jR), a mono track carries a zero imaginary part.
 *
 * Limits: 2 <= N <= P <= 2^ICW_FFT_MAX_LOG2.  The working set is 16 bytes per point of P in HBM: 2 GiB for
 * a track of the largest P (icw_encode_cwave_fft_workspace gives a call's figure). */
#define ICW_FFT_MAX_LOG2 27

typedef struct icw_fft_enc_opts {
    int32_t device;         /* HIP device, -1: current */
    int32_t max_pass_log2;  /* 0: default; 2..: cap of a pass's sub-transform, 2^cap points (tests; values above
                               the default's 7 mean the default) */
} icw_fft_enc_opts;

/* Encode n tracks in one call: track i's PCM (format fmt, `channels` interleaved channels, n_frames[i] frames) at
 * in + in_offsets[i], its CWAVE frames of cw_format to out + out_offsets[i] (n_frames[i] *
 * icw_cwave_frame_bytes(cw_format, channels) bytes; any alignment).  Tracks of different lengths run in one
 * call.  flags: 0 -- in / out are host pointers, staged through the device -- or ICW_F_DEVICE_PTRS.  Either way
 * the call returns with `out` filled (it waits for hip_stream, on which its work is queued).  clipped
 * (nullable host array, n entries) gets every track's saturated / NaN int16 samples.  opts may be NULL
 * (device -1, default passes).
 * Errors, all found on the host before the device is touched, nothing run: ICW_EINVAL for a null pointer,
 * n < 0, a CWAVE fmt, channels 0, a cw_format outside ICW_FMT_CW_*, a track of fewer than 2 frames, a flag
 * other than ICW_F_DEVICE_PTRS, max_pass_log2 negative or 1; then ICW_EUNSUPPORTED for a track of more than
 * 2^ICW_FFT_MAX_LOG2 frames.  ICW_ENOMEM / ICW_EDEVICE: a buffer or a HIP call failed. */
int icw_encode_cwave_fft(const void *in, const uint64_t *in_offsets, const uint64_t *n_frames, int n,
                         uint32_t fmt, uint32_t channels, void *out, const uint64_t *out_offsets,
                         uint32_t cw_format, uint64_t *clipped, unsigned flags, const icw_fft_enc_opts *opts,
                         void *hip_stream);

/* working-set bytes the call needs on the device beside in and out: 16 bytes per point of every track's P
 * (a complex double; mono tracks carry a zero imaginary part, so `channels` does not change it) and 40 bytes
 * of bookkeeping per track.  A host-pointer call stages in and out on the device on top of it.  0 for
 * arguments icw_encode_cwave_fft refuses. */
size_t icw_encode_cwave_fft_workspace(const uint64_t *n_frames, int n, uint32_t channels);

/* passes per transform direction of a track of n_frames frames at this max_pass_log2 (host arithmetic): a
 * call runs 2 * passes - 1 kernels over such a track (the last forward and the first inverse pass are one).
 * ICW_EINVAL / ICW_EUNSUPPORTED as icw_encode_cwave_fft. */
int icw_encode_cwave_fft_passes(uint64_t n_frames, int32_t max_pass_log2);

/* Measurement hook (tools/fft_encode_rate.py): with ICW_FFT_TIMING=1 in the environment a call records every
 * kernel launch between two HIP events; this returns the number of launches of the process's last such call
 * and copies up to `max` of their times in ms, in launch order, to ms (nullable). */
int icw_encode_cwave_fft_last_ms(double *ms, int max);

#ifdef __cplusplus
}
#endif
#endif /* ICW_CWAVE_H_ */
