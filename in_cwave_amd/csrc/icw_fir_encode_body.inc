/*
 * icw_fir_encode_body.inc -- KFE's workgroup, as text: tile blockIdx.x of stream blockIdx.y of NC computed
 * channels in format CWF, from `IcwEncArgs e`.  Included in the body of icw_fir_encode (PS false: the host passes
 * the block's first frame in e.out) and of the per-stream kernel's device function (PS true: e.out is the
 * call's first frame and the tile goes to frame e.f.t0 + tt of the stream's row at the stream's own FB).
 * Text and not a function of its own: called as a shared __device__ function the one-input kernels came out
 * with other instruction orders (and icw_fir_encode<0, 2> with 162 VGPRs for 160), and the C2-shape encode to
 * F64 measured 2.6 - 3 % slower than the parent's; as text they assemble to the parent's instructions.
 */
    extern __shared__ __attribute__((aligned(16))) double xs[];   /* staged inputs (padded); then the frames */
    __shared__ unsigned nclip;
    const IcwFirArgs &a = e.f;
    constexpr int TF = 256 * ICW_FIR_R;
    constexpr int CB = icw_cw_bytes<CWF>::value, FB = NC * CB;    /* bytes per channel, per frame */
    constexpr int NW = ICW_FIR_R * FB / 4;                        /* dwords a lane packs */
    constexpr int CU = FB / 2, PADU = (CU & 1) ? 0 : 1;           /* its 16-byte units, pad units */
    const int s = blockIdx.y, tid = threadIdx.x;
    const int tt = blockIdx.x * TF;
    const int M = a.M, c = M >> 1;
    const int sh = icw_fir_sh(c), av = icw_fir_av(c, sh);   /* c - 1 + sh = 8 av */
    const int nf = min(TF, a.T - tt);
    const int px = icw_fir_px(sh, M, TF);
    if (tid == 0) nclip = 0u;
    icw_fir_stage<NC>(a, s, 0, xs, px, tt, TF, sh, tid, 256);
    icw_ctap *gs = (icw_ctap *)a.g;
    __syncthreads();
    uint32_t w[NW];
    unsigned clip = 0u;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        double q[ICW_FIR_R], vi[ICW_FIR_R];
        icw_fir_sums(xs + k * px, gs, a.nt, tid, av, sh, c, q);
#pragma unroll
        for (int r = 0; r < ICW_FIR_R; ++r) vi[r] = xs[k * px + icw_fir_phys(ICW_FIR_R * tid + r + 8 * av + 1)];
#pragma unroll
        for (int r = 0; r < ICW_FIR_R; ++r) {
            const int o = r * FB + k * CB;               /* byte offset in the lane's run: even, a constant */
            const bool live = ICW_FIR_R * tid + r < nf;
            if constexpr (CWF == 0) {
                const unsigned long long bi = (unsigned long long)__double_as_longlong(vi[r]);
                const unsigned long long bq = (unsigned long long)__double_as_longlong(q[r]);
                w[o / 4] = (uint32_t)bi;
                w[o / 4 + 1] = (uint32_t)(bi >> 32);
                w[o / 4 + 2] = (uint32_t)bq;
                w[o / 4 + 3] = (uint32_t)(bq >> 32);
            } else if constexpr (CWF == 1) {
                w[o / 4] = icw_enc_i16(vi[r], live, clip) | (icw_enc_i16(q[r], live, clip) << 16);
            } else if constexpr (CWF == 2) {
                const uint32_t re = icw_enc_i16(vi[r], live, clip), im = __float_as_uint((float)q[r]);
                if (o & 2) {                             /* the frame starts in a dword's upper half */
                    w[o / 4] |= re << 16;
                    w[o / 4 + 1] = im;
                } else {
                    w[o / 4] = re | (im << 16);
                    w[o / 4 + 1] = im >> 16;
                }
            } else {
                w[o / 4] = __float_as_uint((float)vi[r]);
                w[o / 4 + 1] = __float_as_uint((float)q[r]);
            }
        }
    }
    __syncthreads();                                     /* every lane has read its inputs */
    uint4 *ob = (uint4 *)xs;
#pragma unroll
    for (int i = 0; i < CU; ++i) ob[tid * (CU + PADU) + i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    if (CWF == 1 || CWF == 2) {
        if (clip) atomicAdd(&nclip, clip);
    }
    __syncthreads();
    if ((CWF == 1 || CWF == 2) && tid == 0 && nclip) atomicAdd(e.clipped + s, (unsigned long long)nclip);
    unsigned char *dst = e.out + (size_t)s * e.out_stride + (size_t)tt * FB;
    if constexpr (PS) dst += (size_t)a.t0 * FB;           /* e.out is the call's first frame */
    const int nbytes = nf * FB;
    icw_tile_out<PADU, CU>(dst, nbytes, xs, tid);
