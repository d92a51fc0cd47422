/*
 * icw_cwave_fft.cpp -- host side of the direct-FFT CWAVE encoder (include/icw_cwave.h: icw_encode_cwave_fft):
 * the argument checks, the pass plan of every transform length in the call and the launches of KX
 * (icw_fft.hip).  A call without a context, like icw_crc32_batch.
 */
#include <hip/hip_runtime_api.h>
#include <string.h>

#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/icw_cwave.h"
#include "icw_fft.h"
#include "icw_launch.h"

namespace {

/* the host-side checks of the call and its queries: ICW_OK, ICW_EINVAL or ICW_EUNSUPPORTED */
int check_tracks(const uint64_t *n_frames, int n, int32_t max_pass_log2)
{
    if (n < 0 || (n > 0 && !n_frames) || max_pass_log2 < 0 || max_pass_log2 == 1) return ICW_EINVAL;
    for (int i = 0; i < n; ++i)
        if (n_frames[i] < 2) return ICW_EINVAL;
    for (int i = 0; i < n; ++i)
        if (n_frames[i] > ((uint64_t)1 << ICW_FFT_MAX_LOG2)) return ICW_EUNSUPPORTED;
    return ICW_OK;
}

uint32_t sample_bytes(uint32_t fmt) { return fmt == ICW_FMT_U8 ? 1u : fmt == ICW_FMT_I16 ? 2u : fmt == ICW_FMT_I24 ? 3u : 4u; }

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    bool alloc(size_t n) { return hipMalloc(&p, n ? n : 16) == hipSuccess; }
};

/* ICW_FFT_TIMING=1 (tools/fft_encode_rate.py): every launch of a call between two events; the last call's
 * times, in launch order, for icw_encode_cwave_fft_last_ms */
std::mutex g_ms_lock;
std::vector<double> g_ms;

}  // namespace

extern "C" {

int icw_encode_cwave_fft_last_ms(double *ms, int max)
{
    std::lock_guard<std::mutex> lk(g_ms_lock);
    for (int i = 0; i < max && i < (int)g_ms.size() && ms; ++i) ms[i] = g_ms[i];
    return (int)g_ms.size();
}

size_t icw_encode_cwave_fft_workspace(const uint64_t *n_frames, int n, uint32_t channels)
{
    if (!channels || check_tracks(n_frames, n, 0) != ICW_OK) return 0;
    size_t tot = 0;
    for (int i = 0; i < n; ++i) {
        IcwFftPlan p;
        icw_fft_plan(n_frames[i], 0, &p);
        tot += ((size_t)16 << p.logP) + sizeof(IcwFftTrack) + sizeof(unsigned long long);
    }
    return tot;
}

int icw_encode_cwave_fft_passes(uint64_t n_frames, int32_t max_pass_log2)
{
    const int rc = check_tracks(&n_frames, 1, max_pass_log2);
    if (rc != ICW_OK) return rc;
    IcwFftPlan p;
    icw_fft_plan(n_frames, max_pass_log2, &p);
    return p.n_pass;
}

int icw_encode_cwave_fft(const void *in, const uint64_t *in_offsets, const uint64_t *n_frames, int n, uint32_t fmt,
                         uint32_t channels, void *out, const uint64_t *out_offsets, uint32_t cw_format, uint64_t *clipped,
                         unsigned flags, const icw_fft_enc_opts *opts, void *hip_stream)
{
    icw_fft_enc_opts o = {-1, 0};
    if (opts) o = *opts;
    if (!in || !out || !in_offsets || !out_offsets || !n_frames || fmt > ICW_FMT_F32 || !channels ||
        cw_format < ICW_FMT_CW_F64 || cw_format > ICW_FMT_CW_F32 || (flags & ~(unsigned)ICW_F_DEVICE_PTRS))
        return ICW_EINVAL;
    int rc = check_tracks(n_frames, n, o.max_pass_log2);
    if (rc != ICW_OK) return rc;
    if (clipped) memset(clipped, 0, (size_t)n * sizeof(*clipped));
    if (n == 0) return ICW_OK;

    if (o.device >= 0 && hipSetDevice(o.device) != hipSuccess) return ICW_EDEVICE;
    hipStream_t st = (hipStream_t)hip_stream;
    const bool devp = flags & ICW_F_DEVICE_PTRS;
    const size_t fsz = (size_t)sample_bytes(fmt) * channels;
    const size_t FB = (size_t)icw_cwave_frame_bytes(cw_format, channels);

    /* the tracks ordered by transform length (a launch covers tracks of one length), each with its plan */
    std::vector<IcwFftPlan> plan(n);
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) {
        icw_fft_plan(n_frames[i], o.max_pass_log2, &plan[i]);
        order[i] = i;
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return plan[a].logP < plan[b].logP; });

    /* host pointers: every track's PCM and frames staged back to back on the device (16-byte aligned) */
    std::vector<IcwFftTrack> tr(n);
    uint64_t ws_pts = 0, in_b = 0, out_b = 0;
    for (int k = 0; k < n; ++k) {
        const int i = order[k];
        IcwFftTrack &t = tr[k];
        memset(&t, 0, sizeof(t));
        t.n = (uint32_t)n_frames[i];
        t.in_off = devp ? in_offsets[i] : in_b;
        t.out_off = devp ? out_offsets[i] : out_b;
        in_b = (in_b + n_frames[i] * fsz + 15) & ~(uint64_t)15;
        out_b = (out_b + n_frames[i] * FB + 15) & ~(uint64_t)15;
        if (plan[i].n_pass > 1) {                        /* a one-pass track stays in LDS */
            t.ws_off = ws_pts;
            ws_pts += (uint64_t)1 << plan[i].logP;
        }
    }
    DevBuf ws, meta, din, dout;
    const size_t tr_b = (size_t)n * sizeof(IcwFftTrack), meta_b = tr_b + (size_t)n * sizeof(unsigned long long);
    if ((ws_pts && !ws.alloc(ws_pts * 16)) || !meta.alloc(meta_b) || (!devp && (!din.alloc(in_b) || !dout.alloc(out_b))))
        return ICW_ENOMEM;
    if (hipMemcpyAsync(meta.p, tr.data(), tr_b, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync((unsigned char *)meta.p + tr_b, 0, (size_t)n * sizeof(unsigned long long), st) != hipSuccess)
        return ICW_EDEVICE;
    if (!devp)
        for (int k = 0; k < n; ++k)
            if (hipMemcpyAsync((unsigned char *)din.p + tr[k].in_off, (const unsigned char *)in + in_offsets[order[k]],
                               n_frames[order[k]] * fsz, hipMemcpyHostToDevice, st) != hipSuccess)
                return ICW_EDEVICE;

    IcwFftArgs a;
    memset(&a, 0, sizeof(a));
    a.in = devp ? (const unsigned char *)in : (const unsigned char *)din.p;
    a.out = devp ? (unsigned char *)out : (unsigned char *)dout.p;
    a.ws = (double *)ws.p;
    a.fmt = fmt;
    a.channels = channels;
    a.cwf = cw_format - ICW_FMT_CW_F64;
    const char *tenv = getenv("ICW_FFT_TIMING");
    const bool timing = tenv && tenv[0] == '1';
    std::vector<hipEvent_t> ev;
    for (int k0 = 0; k0 < n && rc == ICW_OK;) {
        const IcwFftPlan &p = plan[order[k0]];
        int k1 = k0 + 1;
        while (k1 < n && k1 - k0 < 65535 && plan[order[k1]].logP == p.logP) ++k1;
        a.tracks = (const IcwFftTrack *)meta.p + k0;
        a.clipped = (unsigned long long *)((unsigned char *)meta.p + tr_b) + k0;
        a.logP = p.logP;
        /* forward passes 0 .. n_pass - 2, the middle pass, inverse passes n_pass - 2 .. 0 */
        const int K = p.n_pass;
        for (int j = 0; j < 2 * K - 1 && rc == ICW_OK; ++j) {
            const int i = j < K ? j : 2 * K - 2 - j;
            int done = 0;
            for (int q = 0; q <= i; ++q) done += p.l[q];
            a.l = p.l[i];
            a.logR = p.logP - done;
            a.logC = icw_fft_logc(p.logP, a.l);
            a.kind = j < K - 1 ? ICW_FFT_FWD : j == K - 1 ? ICW_FFT_MID : ICW_FFT_INV;
            a.first = j == 0;
            a.last = j == 2 * K - 2;
            hipEvent_t e0 = nullptr, e1 = nullptr;
            if (timing && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
                ev.push_back(e0);
                ev.push_back(e1);
                (void)hipEventRecord(e0, st);
            }
            if (icw_launch_fft_pass(&a, k1 - k0, st) != hipSuccess) rc = ICW_EDEVICE;
            if (e1) (void)hipEventRecord(e1, st);
        }
        k0 = k1;
    }
    std::vector<unsigned long long> clip(n, 0);
    if (rc == ICW_OK && hipMemcpyAsync(clip.data(), (unsigned char *)meta.p + tr_b, (size_t)n * sizeof(unsigned long long),
                                       hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = ICW_EDEVICE;
    if (rc == ICW_OK && !devp)
        for (int k = 0; k < n && rc == ICW_OK; ++k)
            if (hipMemcpyAsync((unsigned char *)out + out_offsets[order[k]], (unsigned char *)dout.p + tr[k].out_off,
                               n_frames[order[k]] * FB, hipMemcpyDeviceToHost, st) != hipSuccess)
                rc = ICW_EDEVICE;
    if (hipStreamSynchronize(st) != hipSuccess && rc == ICW_OK) rc = ICW_EDEVICE;
    if (timing) {
        std::lock_guard<std::mutex> lk(g_ms_lock);
        g_ms.clear();
        for (size_t i = 0; i + 1 < ev.size(); i += 2) {
            float ms = 0.f;
            if (rc == ICW_OK && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) g_ms.push_back(ms);
        }
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    if (rc == ICW_OK && clipped)
        for (int k = 0; k < n; ++k) clipped[order[k]] = clip[k];
    return rc;
}

}  /* extern "C" */
