/*
 * icw_fft.h -- internal: the pass plan of the direct-FFT encoder, shared by its launcher (icw_fft.hip) and
 * its host side (icw_cwave_fft.cpp).  Plain C++, no HIP types.
 *
 * A transform of P = 2^logP points runs as n_pass passes of sub-transforms of 2^l[i] points (sum l = logP).
 * The sizes depend on logP and the cap alone, never on the call, so a track's bytes depend only on it.
 */
#ifndef ICW_FFT_H_
#define ICW_FFT_H_

#include <stdint.h>

#include "../../include/icw_cwave.h"

#define ICW_FFT_PASS_LOG2 7        /* default (and largest) cap of a pass's sub-transform: 128 points */
#define ICW_FFT_TILE_LOG2 11       /* points a workgroup holds in LDS: 2048 x 16 B, four workgroups per CU */
#define ICW_FFT_MAX_PASSES 14      /* logP 27 at the smallest cap, 2 */

struct IcwFftPlan {
    int logP, n_pass;
    int l[ICW_FFT_MAX_PASSES];
};

/* the plan of a track of n frames (2 <= n <= 2^ICW_FFT_MAX_LOG2); cap 0: the default, else 2 .. */
static inline void icw_fft_plan(uint64_t n, int cap, IcwFftPlan *p)
{
    int logP = 1;
    while (((uint64_t)1 << logP) < n) ++logP;
    const int L = cap <= 0 || cap > ICW_FFT_PASS_LOG2 ? ICW_FFT_PASS_LOG2 : cap;
    const int k = (logP + L - 1) / L;
    p->logP = logP;
    p->n_pass = k;
    for (int i = 0; i < k; ++i) p->l[i] = logP / k + (i < logP % k ? 1 : 0);
}

/* columns per workgroup of a pass of 2^l-point sub-transforms */
static inline int icw_fft_logc(int logP, int l)
{
    const int room = ICW_FFT_TILE_LOG2 - l, have = logP - l;
    return room < have ? room : have;
}

#endif /* ICW_FFT_H_ */
