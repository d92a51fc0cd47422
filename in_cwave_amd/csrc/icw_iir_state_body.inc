/*
 * icw_iir_state_body.inc -- the body of the lane-per-chain recurrence, included twice by icw_iir.hip: in the
 * kernel icw_iir_state<N, KAHAN, SUBN> itself, where `a` is the kernel's by-value argument (passing it on by
 * reference made the compiler copy the argument struct and moved the register allocation of every instance:
 * C3 -2.1 %), and in icw_iir_state_run, the device function the mixed kernel's runs call.  The includer
 * defines ICW_K1S_LANE, the global lane index, and ICW_K1S_PC(i), loop-back coefficient i; N, KAHAN, SUBN
 * and `a` (IcwK1Args) are in scope.
 */
    int s, ch, f;
    if (!icw_k1_chain(ICW_K1S_LANE, a.n_streams,
                      a.dedup != 0, s, ch, f))
        return;
    const int g = s * 4 + ch * 2 + f;
    const int n_chains = a.n_chains;
    double pc[20];
#pragma unroll
    for (int i = 0; i < 20; ++i) pc[i] = ICW_K1S_PC(i);

    double R[N];
#pragma unroll
    for (int i = 0; i < N; ++i) R[N - 1 - i] = a.hist[(size_t)g * ICW_HIST_PITCH + i];

    /* this block's start (for K2); each (stream, filter) flag is read and written by one wave */
    if (ch == 0) a.info_dup[s * 2 + f] = a.lr_equal[s * 2 + f];
    const double *xp = a.xd + (size_t)(s * 2 + ch) * a.x_pitch;     /* the channel's signed row (K0) */
    double *wrow = a.w + (size_t)g * a.w_pitch;
    /* block-relative sample n has a zero input iff (phi + n) is odd (I: k = hq + t0 + n odd;
     * Q: k + 1 odd) */
    const unsigned phi = (a.hq_phase[s * 2 + ch] + (unsigned)a.t0 + (unsigned)f) & 1u;
    /* history rows [0, N): row j = z_{N-1-j} = R[j] */
#pragma unroll
    for (int j = 0; j < N; ++j) wrow[j] = R[j];

    const int T = a.T;
    unsigned cnt = 0;
    int t = 0;
    if (T >= N) {
        /* xv[j] holds the input of step j of the current block; right after a step consumes it the
         * same register is refilled with the next block's input, so loads run N samples ahead
         * with no register copies */
        double xv[N];
        icw_load_x<N>(xv, xp);
        bool zfast = false;
        unsigned phi0 = 0;
        if constexpr (KAHAN && SUBN) {
            /* the fast path needs one zero-input parity across the wave */
            phi0 = __builtin_amdgcn_readfirstlane(phi);
            zfast = __all(phi == phi0) && T >= 3 * N;
        }
        if constexpr (KAHAN && SUBN && !(N & 1)) {
            /* even order: block-relative step J of every block (t a multiple of N) is a zero input
             * iff (phi0 + J) is odd */
            if (zfast) {
                if (phi0) icw_even_blocks<N, 0, SUBN>(R, xv, xp, wrow, pc, cnt, t, T);
                else icw_even_blocks<N, 1, SUBN>(R, xv, xp, wrow, pc, cnt, t, T);
            }
        }
        if constexpr (KAHAN && SUBN && (N & 1)) {
            if (zfast) {
                /* speculative pairs of blocks ("Speculative blocks") that start on a nonzero sample; a
                 * failed block ends them and the exact loops below take over at its start */
                if ((phi0 + (unsigned)t) & 1u) {
                    icw_block_steps_pf<N, 0, KAHAN, SUBN>(R, xv, xp + t + N, pc, cnt, true);
                    icw_store_block<N>(R, wrow + N + t);
                    t += N;
                }
                double mn = __builtin_inf();       /* smallest |sum| of the speculative block */
                bool fail = false;
                ICW_DRAIN_VMEM();
                while (!fail && t + 2 * N <= T) {
                    /* a failed pair's stores land past [t, t + N), the restart state, and the
                     * exact re-run overwrites them */
                    icw_block_steps_zpf<N, 0, 1, SUBN, true>(R, xv, xp + t + N, pc, cnt, &mn);
                    icw_store_block<N>(R, wrow + N + t);
                    icw_block_steps_zpf<N, 0, 0, SUBN, true>(R, xv, xp + t + 2 * N, pc, cnt, &mn);
                    icw_store_block<N>(R, wrow + 2 * N + t);
                    fail = __any(mn < 1.0);
                    if (!fail) t += 2 * N;
                }
                if (fail) {
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
#pragma unroll
                    for (int j = 0; j < N; ++j) R[j] = wrow[t + j];
                }
                icw_load_x<N>(xv, xp + t);   /* the block's inputs (the zero steps left slots unloaded) */
                if (fail) {
                    /* exact from here: the same zero-input pairs with the reject */
                    ICW_DRAIN_VMEM();
                    if (((phi0 + (unsigned)t) & 1u) && t + N <= T) {
                        icw_block_steps_pf<N, 0, KAHAN, SUBN>(R, xv, xp + t + N, pc, cnt, true);
                        icw_store_block<N>(R, wrow + N + t);
                        t += N;
                    }
                    for (; t + 2 * N <= T; t += 2 * N) {
                        icw_block_steps_zpf<N, 0, 1, SUBN>(R, xv, xp + t + N, pc, cnt);
                        icw_store_block<N>(R, wrow + N + t);
                        icw_block_steps_zpf<N, 0, 0, SUBN>(R, xv, xp + t + 2 * N, pc, cnt);
                        icw_store_block<N>(R, wrow + 2 * N + t);
                    }
                    icw_load_x<N>(xv, xp + t);
                }
            }
        }
        for (; t + N <= T; t += N) {
            icw_block_steps_pf<N, 0, KAHAN, SUBN>(R, xv, xp + t + N, pc, cnt, ((phi + (unsigned)t) & 1u) != 0u);
            icw_store_block<N>(R, wrow + N + t);
        }
    }
    const int rem = T - t;
    if (rem > 0) {
        double xv[N];
#pragma unroll
        for (int j = 0; j < N; ++j) xv[j] = (j < rem) ? xp[t + j] : 0.0;
        icw_block_steps<N, 0, KAHAN, SUBN>(R, xv, pc, cnt, rem, ((phi + (unsigned)t) & 1u) != 0u);
        double *wo = wrow + N + t;
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (j < rem) wo[j] = R[j];
        icw_normalise_ring<N>(R, rem);
    }
    /* the de-subnorm count is taken by K2 from the w rows (a rejected w is exactly 0.0), so the
     * recurrence does not spend issue slots on it: cnt is dead here and compiled away */
    (void)cnt;
    icw_store_hist<N, 0>(R, a.hist, g, n_chains);
    if (a.dedup) {
        icw_store_hist<N, 0>(R, a.hist, g + 2, n_chains);
        a.lr_equal[s * 2 + f] = 1u;
        return;
    }
    /* is this (stream, filter)'s right converter still bit-identical to its left one?  The two
     * channels of a stream are lanes l, l ^ 1 of this wave */
    bool eq = true;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double o = __shfl_xor(R[i], 1);
        eq = eq && (__double_as_longlong(o) == __double_as_longlong(R[i]));
    }
    if (ch == 0) a.lr_equal[s * 2 + f] = eq ? 1u : 0u;
