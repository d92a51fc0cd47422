/*
 * icw_fir.hip -- gfx950 (CDNA4) kernels of the FIR Hilbert converter, built like icw_kernels.hip: KF
 * (icw_fir_hilbert: I / Q rows for K2), KF2 fused with graph and render (icw_fir_graph, icw_fir_sig) and their
 * launchers.  Staging and tap sums: icw_fir_dev.h (shared with icw_encode.hip); the per-frame graph, chain and
 * render code: icw_graph_dev.h (shared with K2, icw_kernels.hip).
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/icw.h"
#include "icw_device.h"
#include "icw_iir_dev.h"
#include "icw_launch.h"
#include "icw_libm.h"

#pragma clang fp contract(off)

#include "icw_quant_dev.h"

#include "icw_unpack_dev.h"

#include "icw_fir_dev.h"
#include "icw_graph_dev.h"

/* The per-stream form of the FIR kernels (PS; streams with different lists or inputs, as K2's MIX): the
 * workgroup is one stream, so what it selects is wave-uniform and comes in by scalar loads through the
 * constant address space.  The PS = false instances are the kernels of a one-list, one-input call.
 * (icw_fir_own_input and icw_fir_own_conv, the stream's own input and converter: icw_fir_dev.h, shared with the
 * encoder.) */
typedef const __attribute__((address_space(4))) int32_t icw_csel;

/* KF: the converter alone, one workgroup per channel and 2048-frame tile of a stream; I / Q rows
 * go out coalesced through LDS to the CWAVE rows K2 reads */
template <bool PS>
__device__ __forceinline__ void icw_fir_hilbert_body(IcwFirArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double xs[];   /* staged inputs (padded), taps, Q */
    constexpr int TF = 256 * ICW_FIR_R;
    const int ch = blockIdx.y, s = blockIdx.z;
    if constexpr (PS) {
        /* the grid has the widest stream's channels: a mono stream's second column has nothing to do */
        icw_fir_own_input(a, s);
        icw_fir_own_conv(a, s);
        if (ch >= (a.nch > 1 ? 2 : 1)) return;
    }
    const int tt = blockIdx.x * TF;
    const int M = a.M, c = M >> 1;
    const int sh = icw_fir_sh(c), av = icw_fir_av(c, sh);   /* c - 1 + sh = 8 av */
    const int nf = min(TF, a.T - tt);
    icw_fir_stage<1>(a, s, ch, xs, 0, tt, TF, sh, threadIdx.x, 256);
    const int px = icw_fir_px(sh, M, TF);
    double *qs = xs + px + ((a.nt + 1) & ~1);
    icw_ctap *gs = (icw_ctap *)a.g;
    __syncthreads();
    double acc[ICW_FIR_R];
    icw_fir_sums(xs, gs, a.nt, threadIdx.x, av, sh, c, acc);
#pragma unroll
    for (int r = 0; r < ICW_FIR_R; ++r) qs[ICW_FIR_R * threadIdx.x + r] = acc[r];
    __syncthreads();
    double *rowI = a.xd + ((size_t)s * 4 + ch * 2) * a.x_pitch + tt;
    double *rowQ = rowI + a.x_pitch;
    const bool mono = a.nch == 1;
    for (int f = threadIdx.x; f < nf; f += 256) {
        const double vi = xs[icw_fir_phys(f + 8 * av + 1)], vq = qs[f];
        rowI[f] = vi;
        rowQ[f] = vq;
        if (mono) {
            rowI[f + 2 * a.x_pitch] = vi;
            rowQ[f + 2 * a.x_pitch] = vq;
        }
    }
}

__global__ __launch_bounds__(256) void icw_fir_hilbert(IcwFirArgs a)
{
    icw_fir_hilbert_body<false>(a);
}

/* KF over streams with different inputs (a.desc); K2's MIX instances take the rows from there */
__global__ __launch_bounds__(256) void icw_fir_hilbert_mixed(IcwFirArgs a)
{
    icw_fir_hilbert_body<true>(a);
}

/* Fused FIR converter + graph + render (KF2): one workgroup per stream and 1024-frame tile (2048
 * for mono).  Wave w owns frames [256 w, 256 w + 256) of the tile: lanes 0-31 sum channel L's
 * outputs and lanes 32-63 channel R's, 8 consecutive frames each (icw_fir_sums).  A lane pair
 * (l, l + 32) then swaps half of its I / Q values (v_permlane32_swap), so lane l holds both channels
 * of frames 0-3 of its eight and lane l + 32 of frames 4-7, and each takes its 4 frames straight
 * through K2's per-frame code (icw_frame_graph: DSP list, pre-render, ROUND render, meters).  The
 * analytic signal never leaves the registers (KF + K2 move 32 B per frame through HBM twice); the
 * sums are KF's, in the same order, so the results are KF + K2's bit for bit.  Dynamic LDS: the
 * padded inputs of each computed channel, the taps, the DSP register file. */
/* Occupancy: 4 workgroups per CU (4 waves per SIMD, <= 128 VGPRs).  TAB: every stream of the launch
 * is in step with the rotation table (the host's frame-counter mirror says so), so the per-stream
 * fallback (icw_trig_call) is compiled out.  With the call in the kernel the allocator kept values
 * live across it in scratch -- 44 B per thread written to HBM, most of the kernel's 2.95x write
 * traffic (profiles/r02_c2fir_pmc.json: 198 MB per launch against 67 MB of output); giving that
 * variant 168 VGPRs instead (3 workgroups per CU) removed the spills but cost c2fir 22 %. */

/* NC: computed channels (1: mono input, 2: stereo), a template parameter so that each form gets its
 * own register allocation (the mono graph phase holds 8 frames per lane, the stereo one 4) */
#if ICW_FIR_STAMPS
/* diagnostic build only (tools/fir_phases.py): per workgroup of the last KF2 launch, wave 0's
 * shader-clock stamps at the phase boundaries and the 100 MHz clock at its start and end */
__device__ unsigned long long icw_fir_stp[(1 << 16) * 8];
#define ICW_FIR_STAMP(k)                                                                              \
    do {                                                                                              \
        if (threadIdx.x == 0 && blockIdx.y * gridDim.x + blockIdx.x < (1u << 16))                     \
            icw_fir_stp[(blockIdx.y * gridDim.x + blockIdx.x) * 8 + (k)] =                            \
                ((k) == 0 || (k) == 7) ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime(); \
    } while (0)
extern "C" int icw_fir_stamps_read(unsigned long long *dst, size_t n)
{
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(icw_fir_stp), n * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#else
#define ICW_FIR_STAMP(k) do { } while (0)
#endif

/* KF2's mono chain form: the lane's ICW_FIR_R frames (from t0, nv of them in the block) two at a time
 * through one signature (SIG; 0: the generic op loop, ROWP: rows at known offsets), the rendered
 * frames packed into w (16-bit: w[0..8), 24-bit: 12 words).  B24 is a template parameter for the reason
 * icw_pack2 gives (icw_fir_dev.h). */
template <bool TRIG, int SIG, bool ROWP, bool B24>
__device__ __forceinline__ void icw_mono_passes(const IcwK2Args &a, icw_cprog *P, int s, int t0, int nv,
                                                const double (&vi)[ICW_FIR_R], const double (&q)[ICW_FIR_R],
                                                unsigned &clip_l, unsigned &clip_r, double &pk_l, double &pk_r,
                                                unsigned (&w)[ICW_FIR_R / 2 * 3], uint32_t tro_lane, size_t pq,
                                                size_t tab_off = 0)
{
#pragma unroll
    for (int hh = 0; hh < ICW_FIR_R; hh += 2) {
        IcwLR in2[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            in2[r].lre = in2[r].rre = vi[hh + r];
            in2[r].lim = in2[r].rim = q[hh + r];
        }
        int dv[2][2];
        const int n2 = min(2, max(nv - hh, 0));
        if constexpr (!ROWP)
            icw_chain_frames<TRIG, 2>(a, P, s, t0 + hh, n2, in2, clip_l, clip_r, pk_l, pk_r, dv, 0, tab_off);
        else if constexpr (SIG != 0)
            icw_chain_frames<TRIG, 2, true, SIG>(a, P, s, t0 + hh, n2, in2, clip_l, clip_r, pk_l, pk_r, dv, tro_lane,
                                                 (size_t)hh * pq + tab_off, pq);
        else
            icw_chain_frames<TRIG, 2, true>(a, P, s, t0 + hh, n2, in2, clip_l, clip_r, pk_l, pk_r, dv, tro_lane,
                                            (size_t)hh * pq + tab_off, pq);
        icw_pack2<B24>(dv[0][0], dv[0][1], dv[1][0], dv[1][1], w + hh / 2 * ICW_PACK2_WORDS(B24));
    }
}

/* ICW_FIR_OCC 5 (96 VGPRs) spills and ran 2.4x slower (profiles/r03_fir_swap_ab.jsonl) */
template <bool TRIG, bool TAB, int NC, bool PS = false>
__global__ __launch_bounds__(256, ICW_FIR_OCC) void icw_fir_graph(IcwFirArgs f, IcwK2Args a)
{
    ICW_FIR_STAMP(0);
    ICW_FIR_STAMP(1);                                /* diagnostic build: 0 / 7 = 100 MHz clock, 1-6 shader clock */
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ unsigned red_clip[2][ICW_PK_SLOTS];
    __shared__ double red_pk[2][ICW_PK_SLOTS];
    /* workgroups in stream-fastest order (the grid is streams x tiles): the workgroups of one tile run
     * together, so its rotation-table rows come from the L2 for every stream, where tile-fastest order
     * swept the whole block's table once per stream (a 2^20-frame block's table is 32 MB: c2fir 37 HBM
     * bytes per frame against 9.4) */
    int s = blockIdx.x;
    if constexpr (PS) {
        /* the launch's class of streams through its map, then the stream's own input */
        if (f.map) s = ((icw_csel *)f.map)[blockIdx.x];
        icw_fir_own_input(f, s);
        icw_fir_own_conv(f, s);
    }
    constexpr int nchc = NC;
    const int TF = 256 * ICW_FIR_R / nchc;
    const int tt = (blockIdx.y + f.tile0) * TF;
    const int M = f.M, c = M >> 1;
    const int sh = icw_fir_sh(c), av = icw_fir_av(c, sh);   /* c - 1 + sh = 8 av */
    const int nf = min(TF, f.T - tt);
    const int px = icw_fir_px(sh, M, TF);                /* doubles per staged channel (even) */
    double *lregs = lds + nchc * px + ((f.nt + 1) & ~1);
    icw_ctap *gs = (icw_ctap *)f.g;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ch = nchc == 2 ? lane >> 5 : 0;
    const int ll = nchc == 2 ? wv * 32 + (lane & 31) : threadIdx.x;   /* lane index within the channel */
    if (nchc == 2) icw_fir_stage<2>(f, s, 0, lds, px, tt, TF, sh, threadIdx.x, 256);
    else icw_fir_stage<1>(f, s, 0, lds, px, tt, TF, sh, threadIdx.x, 256);
    ICW_FIR_STAMP(2);
    __syncthreads();
    ICW_FIR_STAMP(3);
    double q[ICW_FIR_R], vi[ICW_FIR_R];
#if ICW_FIR_CUT >= 2
#pragma unroll
    for (int r = 0; r < ICW_FIR_R; ++r) q[r] = 0.0;
#else
    icw_fir_sums(lds + ch * px, gs, f.nt, ll, av, sh, c, q);
#endif
    const int ix = 8 * av + 1;                               /* logical index of x[tt - c] */
#pragma unroll
    for (int r = 0; r < ICW_FIR_R; ++r) vi[r] = lds[ch * px + icw_fir_phys(ICW_FIR_R * ll + r + ix)];
#if ICW_FIR_STAMPS
    if (threadIdx.x == 0 && q[0] + vi[0] == 1.2345e300) icw_fir_stp[0] = 1;     /* the sums before stamp 4 */
#endif
    ICW_FIR_STAMP(4);
#if ICW_FIR_CUT
    /* diagnostic build only (VALU accounting by phase): no graph, no render */
    {
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < ICW_FIR_R; ++r) acc += q[r] + vi[r];
        if (acc == 1.2345e300) a.out[threadIdx.x] = 1;
        return;
    }
#endif

    icw_cprog *P = icw_prog_c(a.prog);
    /* PS: the stream's program, its slab of the rotation table (tab_off) and that slab's reference stream,
     * and its own rate for the inline factors -- the selection rows K2's MIX instances read */
    size_t tab_off = 0;
    [[maybe_unused]] IcwRate rt;
    [[maybe_unused]] bool own_tab = false;
    if constexpr (PS) {
        icw_csel *id = (icw_csel *)a.prog_id;
        P += id[s];
        const int slab = id[a.n_streams + s];
        rt.sample_rate = (uint32_t)id[3 * a.n_streams + s];
        rt.ssr = (unsigned long long)rt.sample_rate * ICW_HZ_SCALE;
        own_tab = TRIG && a.trig_tab && slab >= 0 && a.n_frame[s] == a.n_frame[id[2 * a.n_streams + s]];
        tab_off = slab >= 0 ? (size_t)slab * a.slab_stride : 0;
    }
    IcwRegFile Rf;
    Rf.base = lregs + threadIdx.x;
    for (int r = 0; r < P->n_persist; ++r) {
        const double *b = a.bus + ((size_t)s * ICW_N_INPUTS + P->persist_slot[r]) * 4;
        IcwLR v; v.lre = b[0]; v.lim = b[1]; v.rre = b[2]; v.rim = b[3];
        Rf.set(P->persist_reg[r], v);
    }
    const bool use_tab = TAB || (PS ? own_tab : (TRIG && a.trig_tab && a.n_frame[s] == a.n_frame[0]));
    unsigned clip_l = 0, clip_r = 0;
    double pk_l = 0.0, pk_r = 0.0;
    if (nchc == 2) {
        /* lane l (L) keeps frames 0-3 and gets R's values of them; lane l + 32 (R) frames 4-7.  Their
         * rendered frames are stored together: lane l's four at byte 32 ll, lane l + 32's at 32 ll + 16
         * (16-bit output), so one 16-byte store per lane covers the wave's 1 KB contiguously.  One
         * 4-byte store per frame instead put 2 of every 32 bytes in each store instruction, and the L2
         * wrote the partial sectors out 2.3x over (r03_c2fir_pmc.json before this change: WRITE_SIZE
         * 153 MB per launch against 67 MB of output). */
        const int h = ch ? 4 : 0;
        int dv[4][2];
        const int fr0 = ICW_FIR_R * ll + h;
        if (ICW_CHAIN4 && P->chain && (TAB || !TRIG) && !a.iq_out && a.do_render && !a.dith) {
            /* chain program, factors from the table (or none): the four frames op by op, two per
             * pass (four at once spill at 128 VGPRs), each pass's I / Q exchange just before it.
             * Frame tt + fr0 + hh + j (tt a multiple of 8, fr0 = 8 ll + h) sits in table row
             * (h + hh + j) q + tt / 8 + ll (icw_trig_index, q = trig_perm_q): a per-lane part and a
             * uniform one.  The last tile of a launch block keeps the clamped index (frames past
             * the block would point past the table). */
            const bool rowp = (TRIG || P->sig) && tt + TF <= f.T;
            const int sig = P->sig;
            const size_t pq = (size_t)a.trig_perm_q * a.trig_pitch;
            const uint32_t tro_lane = (uint32_t)(((size_t)h * a.trig_perm_q + (size_t)(tt >> 3) + ll) * a.trig_pitch);
#pragma unroll
            for (int hh = 0; hh < 4; hh += 2) {
                IcwLR in2[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int r = hh + j;
                    double xl = vi[r], xr = vi[r + 4], yl = q[r], yr = q[r + 4];
                    icw_swap32(xl, xr);
                    icw_swap32(yl, yr);
                    in2[j].lre = xl; in2[j].lim = yl; in2[j].rre = xr; in2[j].rim = yr;
                }
                int dv2[2][2];
                if (rowp)
                    icw_chain_frames_rowp<TRIG, 2>(a, P, sig, s, tt + fr0 + hh, min(2, max(nf - fr0 - hh, 0)), in2, clip_l,
                                                   clip_r, pk_l, pk_r, dv2, tro_lane, (size_t)hh * pq + tab_off, pq);
                else
                    icw_chain_frames<TRIG, 2>(a, P, s, tt + fr0 + hh, min(2, max(nf - fr0 - hh, 0)), in2, clip_l, clip_r,
                                              pk_l, pk_r, dv2, 0, tab_off);
                dv[hh][0] = dv2[0][0]; dv[hh][1] = dv2[0][1];
                dv[hh + 1][0] = dv2[1][0]; dv[hh + 1][1] = dv2[1][1];
            }
        } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double xl = vi[r], xr = vi[r + 4], yl = q[r], yr = q[r + 4];
            icw_swap32(xl, xr);
            icw_swap32(yl, yr);
            const int fr = fr0 + r;
            dv[r][0] = dv[r][1] = 0;
            if (fr < nf) {
                IcwLR in;
                in.lre = xl; in.lim = yl; in.rre = xr; in.rim = yr;
                if constexpr (PS)
                    icw_frame_graph<TRIG, TAB, true, true>(a, P, Rf, s, tt + fr, in, use_tab, clip_l, clip_r, pk_l, pk_r, dv[r],
                                                           tab_off, &rt);
                else
                    icw_frame_graph<TRIG, TAB, true>(a, P, Rf, s, tt + fr, in, use_tab, clip_l, clip_r, pk_l, pk_r, dv[r]);
            }
        }
        }
        if (a.do_render && !a.iq_out) {
            unsigned char *o = a.out + (size_t)s * a.out_stride;
            const int nv = min(4, nf - fr0);
            /* 16-bit: 16 contiguous bytes per lane, 24-bit: 24 */
            if (a.rk.is24) {
                unsigned w[6];
                icw_pack2<true>(dv[0][0], dv[0][1], dv[1][0], dv[1][1], w);
                icw_pack2<true>(dv[2][0], dv[2][1], dv[3][0], dv[3][1], w + 3);
                icw_store_packed<true, 4>(o + (size_t)(tt + fr0) * 6, w, nv);
            } else {
                unsigned w[4];
                icw_pack2<false>(dv[0][0], dv[0][1], dv[1][0], dv[1][1], w);
                icw_pack2<false>(dv[2][0], dv[2][1], dv[3][0], dv[3][1], w + 2);
                icw_store_packed<false, 4>(o + (size_t)(tt + fr0) * 4, w, nv);
            }
        }
    } else if (ICW_CHAIN4 && P->chain && (TAB || !TRIG) && !a.iq_out && a.do_render && !a.dith) {
        /* mono input, chain program: the lane's 8 frames op by op, two at a time, and their 8
         * rendered frames stored together (32 / 48 contiguous bytes per lane) */
        const int fr0 = ICW_FIR_R * ll;
        const bool b24 = a.rk.is24;
        unsigned w[ICW_FIR_R / 2 * 3];               /* packed output: 16-bit frames in w[0..8) */
        /* table rows as in the stereo form: frame tt + 8 ll + hh + j at row (hh + j) q + tt / 8 + ll */
        const bool rowp = (TRIG || P->sig) && tt + TF <= f.T;
        const int sig = P->sig;
        const size_t pq = (size_t)a.trig_perm_q * a.trig_pitch;
        const uint32_t tro_lane = (uint32_t)(((size_t)(tt >> 3) + ll) * a.trig_pitch);
        /* the signature is chosen once for the lane's four passes (inside the pass loop every pass
         * carried all variants while the eight inputs stayed live, and the rotating kernel spilled) */
#define ICW_MONO(SIGV, RP)                                                                                    \
    do {                                                                                                      \
        if (b24) icw_mono_passes<TRIG, SIGV, RP, true>(a, P, s, tt + fr0, nf - fr0, vi, q, clip_l, clip_r, pk_l,  \
                                                       pk_r, w, tro_lane, pq, tab_off);                       \
        else icw_mono_passes<TRIG, SIGV, RP, false>(a, P, s, tt + fr0, nf - fr0, vi, q, clip_l, clip_r, pk_l,    \
                                                    pk_r, w, tro_lane, pq, tab_off);                          \
    } while (0)
        if (!rowp) {
            ICW_MONO(0, false);
        } else if constexpr (TRIG) {
            switch (sig) {
#define ICW_MONO_ALIAS(S) case (S):
#define ICW_MONO_CASE(S) case (S): ICW_MONO((S), true); break;
                ICW_SIG_LIST(ICW_MONO_ALIAS, ICW_MONO_CASE)
#undef ICW_MONO_ALIAS
#undef ICW_MONO_CASE
            default: ICW_MONO(0, true); break;
            }
        } else {
            if (sig == ICW_SIG_M || sig == (ICW_SIG_M | ICW_SIG_UNIT)) ICW_MONO(ICW_SIG_M | ICW_SIG_UNIT, true);
            else ICW_MONO(0, true);
        }
#undef ICW_MONO
        unsigned char *o = a.out + (size_t)s * a.out_stride;
        const int nv = min(ICW_FIR_R, max(nf - fr0, 0));
        if (b24) icw_store_packed<true, ICW_FIR_R>(o + (size_t)(tt + fr0) * 6, w, nv);
        else icw_store_packed<false, ICW_FIR_R>(o + (size_t)(tt + fr0) * 4, w, nv);
    } else {
#pragma unroll 1
        for (int r = 0; r < ICW_FIR_R; ++r) {
            const int fr = ICW_FIR_R * ll + r;
            if (fr < nf) {
                IcwLR in;
                in.lre = in.rre = vi[r];
                in.lim = in.rim = q[r];
                if constexpr (PS)
                    icw_frame_graph<TRIG, TAB, false, true>(a, P, Rf, s, tt + fr, in, use_tab, clip_l, clip_r, pk_l, pk_r, nullptr,
                                                            tab_off, &rt);
                else
                    icw_frame_graph<TRIG, TAB>(a, P, Rf, s, tt + fr, in, use_tab, clip_l, clip_r, pk_l, pk_r);
            }
        }
    }
    ICW_FIR_STAMP(5);
    if (a.do_render) icw_meters_wg(a, s, clip_l, clip_r, pk_l, pk_r, red_clip, red_pk);
    ICW_FIR_STAMP(6);
    ICW_FIR_STAMP(7);
}

/* KF2's signature form (icw_fir_sig): the tiles of a launch block before the one holding its last
 * frame, for a chain program of one of the specialised signatures (ICW_SIG_*), a ROUND / flat render
 * and no pre-render doubles -- the production form of the BASELINE FIR legs.  Every lane then takes
 * icw_chain_frames' render-only branch (full frames, no block-end bus write), so the kernel holds only
 * the staging, the sums, that branch (SIG and the output depth B24 at compile time) and the meters:
 * icw_fir_graph's register allocation is set by its generic paths (the per-frame graph, the exact
 * chain pass, the runtime signature switch), and their scalars spilled to VGPR lanes in the hot
 * phases.  icw_launch_fir_graph runs the last tile of each stream through icw_fir_graph (tile0).
 * Same staging, sums and render arithmetic, so the bytes and meters are icw_fir_graph's. */
/* Occupancy of the signature form: without the generic paths it fits 114 VGPRs at 4 workgroups per CU,
 * no scratch.  It also fits 96 (5 per CU) with 4-tap register blocks in the sums, and the mono form 80
 * (6 per CU): measured the same within the box noise (c2fir -1 / +1.7 %, c4fir +0.5 / +0.8 %, c3fir
 * -1.9 / +0.2 %, profiles/r06_fir_sig_ab.txt) with 24 more VALU and 48 more LDS instructions per wave,
 * so the FP64 pipe, not latency, bounds it at 4. */
#ifndef ICW_FIR_SIG_OCC
#define ICW_FIR_SIG_OCC 4
#endif
#ifndef ICW_FIR_SIG_OCC1
#define ICW_FIR_SIG_OCC1 4                           /* the mono form */
#endif
#ifndef ICW_FIR_SIG_NTAP
#define ICW_FIR_SIG_NTAP ICW_FIR_NTAP
#endif
template <int SIG, int NC, bool B24, bool PS = false>
__global__ __launch_bounds__(256, NC == 2 ? ICW_FIR_SIG_OCC : ICW_FIR_SIG_OCC1) void icw_fir_sig(IcwFirArgs f, IcwK2Args a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ unsigned red_clip[2][ICW_PK_SLOTS];
    __shared__ double red_pk[2][ICW_PK_SLOTS];
    constexpr bool TRIG = (SIG & ~ICW_SIG_UNIT) != ICW_SIG_M;
    constexpr int TF = 256 * ICW_FIR_R / NC;
    /* Prologue, packing and stores stay written out here (icw_fir_sh / _av / _px, icw_pack2 and icw_store_packed
     * say the same): through them the schedule moved and c2fir / c3fir measured 0.6-2.7 % slower. */
    int s = blockIdx.x;
    if constexpr (PS) {
        if (f.map) s = ((icw_csel *)f.map)[blockIdx.x];
        icw_fir_own_input(f, s);
        icw_fir_own_conv(f, s);
    }
    const int tt = blockIdx.y * TF;
    const int M = f.M, c = M >> 1;
    const int sh = (8 - ((c - 1) & 7)) & 7;
    const int av = (c - 1 + sh) >> 3;
    const int px = (icw_fir_phys(sh + M + TF + 24) + 2) & ~1;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ch = NC == 2 ? lane >> 5 : 0;
    const int ll = NC == 2 ? wv * 32 + (lane & 31) : threadIdx.x;
    icw_fir_stage<NC>(f, s, 0, lds, px, tt, TF, sh, threadIdx.x, 256);
    __syncthreads();
    double q[ICW_FIR_R], vi[ICW_FIR_R];
    icw_fir_sums<ICW_FIR_SIG_NTAP>(lds + ch * px, (icw_ctap *)f.g, f.nt, ll, av, sh, c, q);
    const int ix = 8 * av + 1;
#pragma unroll
    for (int r = 0; r < ICW_FIR_R; ++r) vi[r] = lds[ch * px + icw_fir_phys(ICW_FIR_R * ll + r + ix)];
    icw_cprog *P = icw_prog_c(a.prog);
    /* PS: the stream's own program (its constants) and slab (its factors); every stream of the launch has
     * this kernel's signature and is in step with its slab (icw_launch_fir_graph_mix) */
    size_t tab_off = 0;
    if constexpr (PS) {
        icw_csel *id = (icw_csel *)a.prog_id;
        P += id[s];
        if constexpr (TRIG) tab_off = (size_t)id[a.n_streams + s] * a.slab_stride;
    }
    unsigned clip_l = 0, clip_r = 0;
    double pk_l = 0.0, pk_r = 0.0;
    const size_t pq = (size_t)a.trig_perm_q * a.trig_pitch;
    unsigned char *o = a.out + (size_t)s * a.out_stride;
    if constexpr (NC == 2) {
        /* lane l (L) frames 0-3 of its eight with R's values swapped in, lane l + 32 frames 4-7 */
        const int h = ch ? 4 : 0;
        const int fr0 = ICW_FIR_R * ll + h;
        const uint32_t tro_lane = (uint32_t)(((size_t)h * a.trig_perm_q + (size_t)(tt >> 3) + ll) * a.trig_pitch);
        int dv[4][2];
#pragma unroll
        for (int hh = 0; hh < 4; hh += 2) {
            IcwLR in2[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int r = hh + j;
                double xl = vi[r], xr = vi[r + 4], yl = q[r], yr = q[r + 4];
                icw_swap32(xl, xr);
                icw_swap32(yl, yr);
                in2[j].lre = xl; in2[j].lim = yl; in2[j].rre = xr; in2[j].rim = yr;
            }
            int dv2[2][2];
            icw_sig_fast<TRIG, 2, SIG>(a, P, in2, clip_l, clip_r, pk_l, pk_r, dv2, tro_lane, (size_t)hh * pq + tab_off, pq);
            dv[hh][0] = dv2[0][0]; dv[hh][1] = dv2[0][1];
            dv[hh + 1][0] = dv2[1][0]; dv[hh + 1][1] = dv2[1][1];
        }
        if constexpr (B24) {
            unsigned char *p = o + (size_t)(tt + fr0) * 6;
            unsigned w[6];
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
                const unsigned l0 = (unsigned)dv[r][0] & 0xffffffu, r0 = (unsigned)dv[r][1] & 0xffffffu;
                const unsigned l1 = (unsigned)dv[r + 1][0] & 0xffffffu, r1 = (unsigned)dv[r + 1][1] & 0xffffffu;
                w[r / 2 * 3 + 0] = l0 | (r0 << 24);
                w[r / 2 * 3 + 1] = (r0 >> 8) | (l1 << 16);
                w[r / 2 * 3 + 2] = (l1 >> 16) | (r1 << 8);
            }
            if (!((uintptr_t)p & 7)) {
                uint2 *q2 = (uint2 *)p;
                q2[0] = make_uint2(w[0], w[1]);
                q2[1] = make_uint2(w[2], w[3]);
                q2[2] = make_uint2(w[4], w[5]);
            } else {
#pragma unroll
                for (int i = 0; i < 24; ++i) p[i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
            }
        } else {
            unsigned pk[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) pk[r] = ((unsigned)dv[r][0] & 0xffffu) | ((unsigned)dv[r][1] << 16);
            unsigned *p = (unsigned *)(o + (size_t)(tt + fr0) * 4);
            if (!((uintptr_t)p & 15)) {
                *(uint4 *)p = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) p[r] = pk[r];
            }
        }
    } else {
        /* mono: the lane's 8 frames two at a time, packed as icw_mono_passes does */
        const int fr0 = ICW_FIR_R * ll;
        const uint32_t tro_lane = (uint32_t)(((size_t)(tt >> 3) + ll) * a.trig_pitch);
        int dl[ICW_FIR_R], dr[ICW_FIR_R];
        if (!TRIG && f.lr_same) {
            /* both channels run the same arithmetic on the same inputs (mono input, a Master whose two
             * gains are the same double: icw_launch_fir_graph's lr_same), so a pass takes two frames in
             * its L / R slots and each result serves both channels: half the graph and render */
#pragma unroll
            for (int hh = 0; hh < ICW_FIR_R; hh += 4) {
                IcwLR in2[2];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    in2[r].lre = vi[hh + 2 * r];
                    in2[r].lim = q[hh + 2 * r];
                    in2[r].rre = vi[hh + 2 * r + 1];
                    in2[r].rim = q[hh + 2 * r + 1];
                }
                int dv[2][2];
                icw_sig_fast<TRIG, 2, SIG>(a, P, in2, clip_l, clip_r, pk_l, pk_r, dv, tro_lane, 0, pq);
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int c = 0; c < 2; ++c) dl[hh + 2 * r + c] = dr[hh + 2 * r + c] = dv[r][c];
            }
            /* the slots held frames: every frame's clips and peak count for both channels */
            clip_l = clip_r = clip_l + clip_r;
            pk_l = pk_r = icw_vmax(pk_l, pk_r);
        } else {
#pragma unroll
            for (int hh = 0; hh < ICW_FIR_R; hh += 2) {
                IcwLR in2[2];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    in2[r].lre = in2[r].rre = vi[hh + r];
                    in2[r].lim = in2[r].rim = q[hh + r];
                }
                int dv[2][2];
                icw_sig_fast<TRIG, 2, SIG>(a, P, in2, clip_l, clip_r, pk_l, pk_r, dv, tro_lane, (size_t)hh * pq + tab_off, pq);
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    dl[hh + r] = dv[r][0];
                    dr[hh + r] = dv[r][1];
                }
            }
        }
        unsigned w[ICW_FIR_R / 2 * 3];
#pragma unroll
        for (int hh = 0; hh < ICW_FIR_R; hh += 2) {
            if constexpr (B24) {
                const unsigned l0 = (unsigned)dl[hh] & 0xffffffu, r0 = (unsigned)dr[hh] & 0xffffffu;
                const unsigned l1 = (unsigned)dl[hh + 1] & 0xffffffu, r1 = (unsigned)dr[hh + 1] & 0xffffffu;
                w[hh / 2 * 3 + 0] = l0 | (r0 << 24);
                w[hh / 2 * 3 + 1] = (r0 >> 8) | (l1 << 16);
                w[hh / 2 * 3 + 2] = (l1 >> 16) | (r1 << 8);
            } else {
                w[hh] = ((unsigned)dl[hh] & 0xffffu) | ((unsigned)dr[hh] << 16);
                w[hh + 1] = ((unsigned)dl[hh + 1] & 0xffffu) | ((unsigned)dr[hh + 1] << 16);
            }
        }
        if constexpr (B24) {
            unsigned char *p = o + (size_t)(tt + fr0) * 6;
            if (!((uintptr_t)p & 7)) {
                uint2 *q2 = (uint2 *)p;
#pragma unroll
                for (int i = 0; i < ICW_FIR_R / 2 * 3 / 2; ++i) q2[i] = make_uint2(w[2 * i], w[2 * i + 1]);
            } else {
#pragma unroll
                for (int i = 0; i < ICW_FIR_R * 6; ++i) p[i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
            }
        } else {
            unsigned *p = (unsigned *)(o + (size_t)(tt + fr0) * 4);
            if (!((uintptr_t)p & 15)) {
                *(uint4 *)p = make_uint4(w[0], w[1], w[2], w[3]);
                *(uint4 *)(p + 4) = make_uint4(w[4], w[5], w[6], w[7]);
            } else {
#pragma unroll
                for (int r = 0; r < ICW_FIR_R; ++r) p[r] = w[r];
            }
        }
    }
    icw_meters_wg(a, s, clip_l, clip_r, pk_l, pk_r, red_clip, red_pk);
}

/* ---------------------------------------------------------------- launch wrappers ------- */
/* dynamic LDS of the FIR kernels: staged channels (padded), taps, Q, the DSP register file */
static size_t fir_lds(int M, int nt, int nchc, int tf, int n_regs)
{
    return ((size_t)nchc * icw_fir_px(M, tf) + (size_t)((nt + 1) & ~1) + (size_t)nchc * tf +
            (size_t)n_regs * 4 * ICW_K2_TILE) * sizeof(double);
}

static bool fir_ok(int M, int nt)
{
    return M >= 2 && M <= ICW_FIR_MAX_M && !(M & 1) && nt >= 1 && 2 * nt - 1 <= M / 2;
}

/* LDS above 64 KB per workgroup needs the kernel attribute (gfx950: 160 KB per CU) */
static hipError_t fir_lds_attr(const void *fn, size_t lds)
{
    return lds > 64 * 1024 ? hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
}

extern "C" hipError_t icw_launch_fir(const IcwFirArgs *a, hipStream_t st)
{
    if (!fir_ok(a->M, a->nt)) return hipErrorInvalidValue;
    constexpr int TF = 256 * ICW_FIR_R;
    const size_t lds = fir_lds(a->M, a->nt, 1, TF, 0);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    /* streams with different inputs (a->desc) or converters (a->conv): the instance that reads each stream's
     * own; a->nch, a->M and a->nt are then the widest stream's */
    const bool ps = a->desc || a->conv;
    const void *fn = ps ? (const void *)icw_fir_hilbert_mixed : (const void *)icw_fir_hilbert;
    if (fir_lds_attr(fn, lds) != hipSuccess) return hipErrorInvalidValue;
    dim3 grid((a->T + TF - 1) / TF, a->nch > 1 ? 2 : 1, a->n_streams);
    if (ps) hipLaunchKernelGGL(icw_fir_hilbert_mixed, grid, dim3(256), lds, st, *a);
    else hipLaunchKernelGGL(icw_fir_hilbert, grid, dim3(256), lds, st, *a);
    return hipGetLastError();
}

/* bytes of dynamic LDS the fused converter needs (0: more than a workgroup may hold -- run KF + K2) */
extern "C" size_t icw_fir_graph_lds(int M, int nt, int nch, int n_regs)
{
    const int nchc = nch > 1 ? 2 : 1;
    const size_t lds = fir_lds(M, nt, nchc, 256 * ICW_FIR_R / nchc, n_regs) - (size_t)256 * ICW_FIR_R * sizeof(double);
    return lds <= 96 * 1024 ? lds : 0;
}

/* in_step: every stream of the launch is in step with the rotation table (a->trig_tab); PS: with its
 * own slab of it.  The grid's columns are f->n_streams: the call's streams, or (PS) the class's */
template <int NC, bool PS>
static hipError_t launch_fir_graph_nc(const IcwFirArgs *f, const IcwK2Args *a, int in_step, size_t lds, hipStream_t st)
{
    const int TF = 256 * ICW_FIR_R / NC;
    dim3 grid(f->n_streams, (f->T + TF - 1) / TF - f->tile0);  /* stream-fastest (icw_fir_graph); <= 1 024 tiles */
    const void *fn = !a->trig ? (const void *)icw_fir_graph<false, false, NC, PS>
                   : in_step ? (const void *)icw_fir_graph<true, true, NC, PS> : (const void *)icw_fir_graph<true, false, NC, PS>;
    if (fir_lds_attr(fn, lds) != hipSuccess) return hipErrorInvalidValue;
    if (!a->trig) hipLaunchKernelGGL((icw_fir_graph<false, false, NC, PS>), grid, dim3(256), lds, st, *f, *a);
    else if (in_step) hipLaunchKernelGGL((icw_fir_graph<true, true, NC, PS>), grid, dim3(256), lds, st, *f, *a);
    else hipLaunchKernelGGL((icw_fir_graph<true, false, NC, PS>), grid, dim3(256), lds, st, *f, *a);
    return hipGetLastError();
}

/* the signature form over tiles [0, ntile) of every stream */
template <int SIG, int NC, bool B24, bool PS>
static hipError_t launch_fir_sig_t(const IcwFirArgs *f, const IcwK2Args *a, int ntile, size_t lds, hipStream_t st)
{
    const void *fn = (const void *)icw_fir_sig<SIG, NC, B24, PS>;
    if (fir_lds_attr(fn, lds) != hipSuccess) return hipErrorInvalidValue;
    hipLaunchKernelGGL((icw_fir_sig<SIG, NC, B24, PS>), dim3(f->n_streams, ntile), dim3(256), lds, st, *f, *a);
    return hipGetLastError();
}

template <int NC, bool B24, bool PS>
static hipError_t launch_fir_sig_d(const IcwFirArgs *f, const IcwK2Args *a, int sig, int ntile, size_t lds,
                                   hipStream_t st)
{
    hipError_t e = hipErrorInvalidValue;             /* a signature without code of its own */
    icw_sig_dispatch(sig, [&](auto sc) { e = launch_fir_sig_t<decltype(sc)::value, NC, B24, PS>(f, a, ntile, lds, st); });
    return e;
}

static bool fir_sig_known(int sig)
{
    return icw_sig_dispatch(sig, [](auto) {});
}

/* KF2 over the f->n_streams columns of one launch (PS: one class of a call's streams, f->map) */
template <bool PS>
static hipError_t launch_fir_graph(const IcwFirArgs *f, const IcwK2Args *a, int in_step, int sig_on, hipStream_t st)
{
    if (!fir_ok(f->M, f->nt)) return hipErrorInvalidValue;
    /* the render-only form (icw_fast_render) takes the quantiser from sign_delta alone: mid-riser
     * (sign_delta -1, round_offset 0) or mid-tread (0, 0.5), the only pairs render_consts gives */
    if (a->rk.sign_delta != 0 ? (a->rk.sign_delta != -1 || a->rk.round_offset != 0.0) : a->rk.round_offset != 0.5)
        return hipErrorInvalidValue;
    const size_t lds = icw_fir_graph_lds(f->M, f->nt, f->nch, a->n_regs);
    if (!lds) return hipErrorInvalidValue;
    if (in_step && !(a->trig && a->trig_tab)) return hipErrorInvalidValue;
    const int nc = f->nch > 1 ? 2 : 1, TF = 256 * ICW_FIR_R / nc;
    IcwFirArgs fl = *f;
    fl.tile0 = 0;
    /* the signature form takes the tiles before the one holding the block's last frame when every
     * lane of them would take icw_chain_frames' render-only branch: a chain program of a known
     * signature, its rotation factors (if any) from the table, a render here, no pre-render doubles,
     * no I / Q hand-off, no dither rows.  sig_on 0 (IcwTuning.fir_sig): icw_fir_graph for every tile. */
    const int sig = f->sig;
    const bool rot = (sig & ~ICW_SIG_UNIT) != ICW_SIG_M;
    if (sig_on && ICW_CHAIN4 && fir_sig_known(sig) && (rot ? (a->trig && in_step) : !a->trig) && a->do_render &&
        !a->iq_out && !a->pre && !a->dith) {
        const int nsig = (f->T - 1) / TF;
        if (nsig > 0) {
            const bool b24 = a->rk.is24 != 0;
            const size_t ls = icw_fir_graph_lds(f->M, f->nt, f->nch, 0);   /* no DSP register file */
            const hipError_t e = nc == 2 ? (b24 ? launch_fir_sig_d<2, true, PS>(f, a, sig, nsig, ls, st)
                                                : launch_fir_sig_d<2, false, PS>(f, a, sig, nsig, ls, st))
                                         : (b24 ? launch_fir_sig_d<1, true, PS>(f, a, sig, nsig, ls, st)
                                                : launch_fir_sig_d<1, false, PS>(f, a, sig, nsig, ls, st));
            if (e != hipSuccess) return e;
            fl.tile0 = nsig;
        }
    }
    return nc == 2 ? launch_fir_graph_nc<2, PS>(&fl, a, in_step, lds, st) : launch_fir_graph_nc<1, PS>(&fl, a, in_step, lds, st);
}

extern "C" hipError_t icw_launch_fir_graph(const IcwFirArgs *f, const IcwK2Args *a, int in_step, int sig_on,
                                           hipStream_t st)
{
    if (f->desc || f->map || f->conv || a->prog_id) return hipErrorInvalidValue;   /* icw_launch_fir_graph_mix's call */
    return launch_fir_graph<false>(f, a, in_step, sig_on, st);
}

/* KF2 over streams with different lists or inputs: the per-stream instances, once per channel class present
 * (mono streams, stereo streams), each class through its stream map.  A class whose streams all have one
 * known signature keeps the signature form for its leading tiles -- every stream with its own program's
 * constants and its own slab's factors; "in step" is each stream with its slab's reference stream.  The
 * class's trig replaces the call's (a Master-only class beside a Shift class runs the kernels without the
 * Shift / PM code). */
extern "C" hipError_t icw_launch_fir_graph_mix(const IcwFirArgs *f, const IcwK2Args *a, const IcwFirClass *cls, int n_cls,
                                               int sig_on, hipStream_t st)
{
    if (!a->prog_id) return hipErrorInvalidValue;
    for (int k = 0; k < n_cls; ++k) {
        const IcwFirClass &c = cls[k];
        if (c.n <= 0) continue;
        if (!c.map || c.n > a->n_streams) return hipErrorInvalidValue;
        IcwFirArgs fc = *f;
        fc.n_streams = c.n;
        fc.nch = (uint32_t)(c.nch > 1 ? 2 : 1);
        fc.map = c.map;
        fc.sig = c.sig;
        fc.lr_same = c.nch == 1 ? c.lr_same : 0;
        if (f->conv && c.M > 0) {                    /* LDS for the widest converter among the class's streams */
            fc.M = c.M;
            fc.nt = c.nt;
        }
        IcwK2Args ac = *a;
        ac.trig = c.trig ? 1 : 0;
        const hipError_t e = launch_fir_graph<true>(&fc, &ac, c.in_step, sig_on, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
