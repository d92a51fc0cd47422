/*
 * icw_launch.h -- internal: every kernel launcher of the library, declared once.  The .hip file that
 * defines a launcher and the host file that calls it both include this, so a changed parameter
 * list is a compile error instead of garbage in a kernel's arguments (the launchers are extern "C").
 */
#ifndef ICW_LAUNCH_H
#define ICW_LAUNCH_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "icw_crc.h"
#include "icw_device.h"

extern "C" {

/* icw_kernels.hip */
hipError_t icw_launch_unpack(const IcwK0Args *a, hipStream_t st);
hipError_t icw_launch_unpack_mixed(const IcwK0MixArgs *a, hipStream_t st);
hipError_t icw_launch_output(const IcwK2Args *a, int nord, int kahan, hipStream_t st);
/* K2 reading the CWAVE file frames itself (no K0, no xd rows): a call over CWAVE streams with different inputs */
hipError_t icw_launch_output_cw(const IcwK2Args *a, const IcwDinArgs *d, hipStream_t st);
hipError_t icw_launch_trig_table(const IcwTrigArgs *a, hipStream_t st);
hipError_t icw_launch_graph_serial(const IcwK4Args *a, hipStream_t st);
/* K4 over the runs of a call whose streams carry different bus-form programs: n_wgs one-wave workgroups */
hipError_t icw_launch_graph_serial_mixed(const IcwK4MixArgs *m, int n_wgs, hipStream_t st);
hipError_t icw_launch_advance(const IcwAdvArgs *a, hipStream_t st);
hipError_t icw_launch_advance_mixed(const IcwAdvMixArgs *a, hipStream_t st);
hipError_t icw_launch_stream1(const IcwS1Args *a, int nord, hipStream_t st);

/* icw_fir.hip */
hipError_t icw_launch_fir(const IcwFirArgs *a, hipStream_t st);
hipError_t icw_launch_fir_graph(const IcwFirArgs *f, const IcwK2Args *a, int in_step, int sig_on, hipStream_t st);
/* the same over streams with different lists or inputs (a->prog_id set): one launch per class present,
 * the signature form included */
hipError_t icw_launch_fir_graph_mix(const IcwFirArgs *f, const IcwK2Args *a, const IcwFirClass *cls, int n_cls, int sig_on,
                                    hipStream_t st);
size_t icw_fir_graph_lds(int M, int nt, int nch, int n_regs);

/* icw_render.hip */
hipError_t icw_launch_render(const IcwK3Args *a, hipStream_t st);
hipError_t icw_launch_dither(const IcwK3Args *a, hipStream_t st);
/* KR: the frame-parallel renders of a call over streams with different renders, from K2's pre-render rows */
hipError_t icw_launch_render_mixed(const IcwKRArgs *a, hipStream_t st);

/* icw_iir.hip */
hipError_t icw_launch_iir_state(const IcwK1Args *a, int nord, int kahan, int subn, hipStream_t st);
hipError_t icw_launch_iir_row(const IcwK1Args *a, int nord, int kahan, int subn, hipStream_t st);
hipError_t icw_launch_iir_fc(const IcwK1Args *a, int nord, int kahan, int subn, hipStream_t st);
/* the mixed recurrence kernels (streams with different Hilbert converters): the call's runs as a device
 * table ordered by wg0, n_wgs workgroups of a->wg_waves waves in all, pctab the entries' coefficients.
 * row: the row form (every run Kahan + reject), else the lane form */
hipError_t icw_launch_iir_mixed(const IcwK1Args *a, int row, const IcwK1Run *runs, int n_runs, int n_wgs,
                                const double *pctab, hipStream_t st);

/* icw_encode.hip */
hipError_t icw_launch_fir_encode(const IcwEncArgs *e, int cwf, hipStream_t st);
hipError_t icw_launch_iq_pack(const IcwPackArgs *a, int cwf, int nc, hipStream_t st);
/* the two over streams with different inputs: every workgroup column takes its stream's own format and
 * channels from the table (e->f.desc / a->desc; a null table is refused) and places its tile at the stream's
 * own frame size; e->f.nch is the call's widest stream (it sizes KFE's LDS) */
hipError_t icw_launch_fir_encode_mixed(const IcwEncArgs *e, int cwf, hipStream_t st);
hipError_t icw_launch_iq_pack_mixed(const IcwPackMixArgs *a, int cwf, hipStream_t st);
/* hq_phase: null for the FIR encoder (the reader position alone) */
hipError_t icw_launch_enc_advance(long long *pos, uint32_t *hq_phase, int n_streams, long long n, hipStream_t st);

/* icw_fft.hip: one pass of the direct-FFT encoder over n_tracks tracks of one transform length */
hipError_t icw_launch_fft_pass(const IcwFftArgs *a, int n_tracks, hipStream_t st);

/* icw_crc.hip */
hipError_t icw_launch_crc32(const IcwCrcArgs *a, uint64_t max_cells, int n_cu, hipStream_t st);

}  /* extern "C" */

#endif
