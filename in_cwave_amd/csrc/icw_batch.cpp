/*
 * icw_batch.cpp -- WAV / CWAVE file headers and the batched many-file transcoder
 * (include/icw_reader.h).  Host C++ over the C ABI of icw.h; the samples are processed only by the
 * gfx950 kernels (icw_process_streams with device pointers).
 *
 * Mirrors: check_file_ext (xwave_reader.c:123-131), rwave_reader_create (xwave_reader.c:362-585),
 * cwave_reader_create (via icw_cwave_parse), xwave_reader_create's MAX_FS_SRC check and virtual
 * zero tail (xwave_reader.c:672-697), xwave_read_samples (xwave_reader.c:838-904: data, then the
 * format's zero sample for the tail), transcode.c:39-120 (2-channel output of out_size bytes).
 */
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <string.h>
#include <strings.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "../../include/icw_cwave.h"
#include "../../include/icw_reader.h"
#include "icw_pool_plan.h"

namespace {

uint32_t le16(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
uint32_t le32(const unsigned char *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

struct File {
    FILE *f = nullptr;
    ~File() { if (f) fclose(f); }
};

int64_t file_size(FILE *f)
{
    if (fseeko(f, 0, SEEK_END)) return -1;
    const int64_t n = ftello(f);
    if (fseeko(f, 0, SEEK_SET)) return -1;
    return n;
}

bool rd(FILE *f, void *b, size_t n) { return fread(b, 1, n, f) == n; }

/* pcmBpsToFormat (xwave_reader.c:342-358) */
int bps_format(unsigned bps)
{
    switch (bps) {
    case 8: return ICW_FMT_U8;
    case 16: return ICW_FMT_I16;
    case 24: return ICW_FMT_I24;
    case 32: return ICW_FMT_I32;
    }
    return -1;
}

/* rwave_reader_create (xwave_reader.c:362-585) */
int parse_rwave(FILE *f, int64_t fsize, icw_wav_info *w)
{
    static const unsigned char guid_tail[14] = {0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00,
                                                0x00, 0xaa, 0x00, 0x38, 0x9b, 0x71};
    const size_t sz_wf = 14, sz_pcmwf = 16, sz_ext = 40;   /* WAVEFORMAT, PCMWAVEFORMAT, ..EXTENSIBLE */
    unsigned char h[12], ch[8], fmt[40];
    int64_t fpos = 0;
    uint32_t fmt_len = 0, data_len = 0;
    if (!rd(f, h, 12) || memcmp(h, "RIFF", 4) || memcmp(h + 8, "WAVE", 4)) return ICW_EINVAL;
    fpos = 12;
    for (;;) {                                             /* "fmt " before any "data" */
        if (!rd(f, ch, 8)) return ICW_EINVAL;
        fmt_len = le32(ch + 4);
        fpos += 8;
        if (fpos + fmt_len > fsize) return ICW_EINVAL;
        if (!memcmp(ch, "fmt ", 4)) break;
        if (!memcmp(ch, "data", 4)) return ICW_EINVAL;
        if (fseeko(f, fmt_len, SEEK_CUR)) return ICW_EINVAL;
        fpos += fmt_len;
    }
    if (fmt_len < sz_wf) return ICW_EINVAL;
    const size_t toread = fmt_len < sz_ext ? fmt_len : sz_ext;
    memset(fmt, 0, sizeof(fmt));
    if (!rd(f, fmt, toread)) return ICW_EINVAL;
    if (toread < fmt_len && fseeko(f, (off_t)(fmt_len - toread), SEEK_CUR)) return ICW_EINVAL;
    fpos += fmt_len;
    const uint32_t tag = le16(fmt), nch = le16(fmt + 2), rate = le32(fmt + 4), align = le16(fmt + 12);
    uint32_t bps = (le16(fmt + 14) + 7) & ~7u;            /* rounded up to whole bytes */
    if (!nch || nch > 2 || !rate) return ICW_EINVAL;
    int format = -1;
    switch (tag) {
    case 1:                                                /* WAVE_FORMAT_PCM */
        if (fmt_len < sz_pcmwf) {
            if (align % nch) return ICW_EINVAL;
            bps = (align / nch) << 3;
            w->htype = ICW_HTYPE_WFONLY;
        } else {
            w->htype = ICW_HTYPE_PCMW;
        }
        format = bps_format(bps);
        break;
    case 3:                                                /* WAVE_FORMAT_IEEE_FLOAT */
        if (fmt_len < sz_pcmwf || bps != 32) return ICW_EINVAL;
        w->htype = ICW_HTYPE_PCMW;
        format = ICW_FMT_F32;
        break;
    case 0xFFFE:                                           /* WAVE_FORMAT_EXTENSIBLE */
        if (fmt_len < sz_ext || le16(fmt + 16) < 2 + 4 + 16) return ICW_EINVAL;
        w->htype = ICW_HTYPE_EXT;
        if (!memcmp(fmt + 26, guid_tail, 14) && (le16(fmt + 24) == 1 || le16(fmt + 24) == 3)) {
            if (le16(fmt + 24) == 1) format = bps_format(bps);
            else format = bps == 32 ? ICW_FMT_F32 : -1;
        }
        break;
    default:
        return ICW_EINVAL;
    }
    if (format < 0) return ICW_EINVAL;
    for (;;) {                                             /* then the "data" chunk */
        if (!rd(f, ch, 8)) return ICW_EINVAL;
        fpos += 8;
        data_len = le32(ch + 4);
        if (fpos + data_len > fsize) return ICW_EINVAL;
        if (!memcmp(ch, "data", 4)) break;
        if (fseeko(f, data_len, SEEK_CUR)) return ICW_EINVAL;
        fpos += data_len;
    }
    const uint32_t csz = bps >> 3, frame = csz * nch;
    w->n_samples = data_len / frame;
    if (w->n_samples < 2 || align != frame) return ICW_EINVAL;   /* MIN_FILE_SAMPLES, nBlockAlign */
    w->fmt = (uint32_t)format;
    w->channels = nch;
    w->sample_rate = rate;
    w->frame_bytes = frame;
    w->data_offset = fpos;
    return ICW_OK;
}

/* the format's zero sample (zero_u8 = 0x80 for unsigned 8 bit, zero bytes otherwise) */
unsigned char zero_byte(uint32_t fmt) { return fmt == ICW_FMT_U8 ? 0x80 : 0x00; }

struct Job {
    int idx;
    icw_wav_info info;
    FILE *in = nullptr, *out = nullptr;
    int64_t total = 0;        /* n_samples + tail */
    int64_t read = 0;         /* data frames read so far */
    int64_t written = 0;      /* output frames written so far */
    int slot = -1;            /* icw_transcode_files_pool: the slot the plan gives it */
};

void wav_header(unsigned char *h, uint32_t rate, int bytes_per_sample, uint64_t frames)
{
    const uint32_t block = 2u * (uint32_t)bytes_per_sample;
    const uint64_t data = frames * block;
    const uint32_t d32 = data > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)data;
    auto p32 = [](unsigned char *q, uint32_t v) { q[0] = v; q[1] = v >> 8; q[2] = v >> 16; q[3] = v >> 24; };
    auto p16 = [](unsigned char *q, uint32_t v) { q[0] = v; q[1] = v >> 8; };
    memcpy(h, "RIFF", 4); p32(h + 4, 36 + d32); memcpy(h + 8, "WAVE", 4);
    memcpy(h + 12, "fmt ", 4); p32(h + 16, 16); p16(h + 20, 1); p16(h + 22, 2); p32(h + 24, rate);
    p32(h + 28, rate * block); p16(h + 32, block); p16(h + 34, 8 * bytes_per_sample);
    memcpy(h + 36, "data", 4); p32(h + 40, d32);
}

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

/* icw_transcode_files_lists: file i's own list (indexed like the files), null for the one-list call */
struct FileLists {
    const icw_node *const *nodes = nullptr;
    const int *n_nodes = nullptr;
    const int *bypass = nullptr;       /* nullable: cfg->bypass_list */
    bool per_stream = false;           /* the group's lists may differ (all register form, or bus: all bus form) */
    bool bus = false;                  /* ICW_BATCH_MERGE_BUS: the group's files carry bus-form lists, each its own */
    int32_t k_M = 0;                   /* icw_transcode_files_fir: the FIR converter for real-input groups (0: the IIR) */
    double k_beta = 0.0;
};

/* The frame of a many-file call: parse and open every file, group the accepted ones by (rate, format,
 * channels, key), run each group, close the files and count the results.  accept(i, job) fills the
 * job's info and returns file i's status (ICW_OK to go on); key(i) is the caller's own part of the
 * group key, asked once the file is open; run(key, jobs, stats, status) processes one group. */
/* merge, the ICW_BATCH_* bits: with ICW_BATCH_MERGE_INPUTS the real-input files group by the key alone -- one
 * context whose streams each get their own input (icw_set_stream_input) -- and with ICW_BATCH_MERGE_CWAVE the
 * CWAVE files do, in a context of their own (a call covers streams of one kind); without its bit a kind
 * keeps the grouping above. */
template <class Accept, class Key, class Run>
int for_file_groups(const char *const *in_paths, const char *const *out_paths, int n, icw_batch_stats *stats, int *status,
                    Accept accept, Key key, Run run, unsigned merge = 0)
{
    const double t0 = now_s();
    icw_batch_stats st;
    memset(&st, 0, sizeof(st));
    std::vector<int> stat_local(n > 0 ? n : 1, ICW_OK);
    int *sts = status ? status : stat_local.data();
    std::vector<Job> jobs(n);
    std::map<std::tuple<uint32_t, uint32_t, uint32_t, int>, std::vector<Job *>> groups;
    for (int i = 0; i < n; ++i) {
        Job &j = jobs[i];
        j.idx = i;
        if ((sts[i] = accept(i, j)) != ICW_OK) continue;
        if (!(j.in = fopen(in_paths[i], "rb")) || !(j.out = fopen(out_paths[i], "wb"))) {
            sts[i] = ICW_EINVAL;
            continue;
        }
        setvbuf(j.in, nullptr, _IOFBF, 1 << 20);
        setvbuf(j.out, nullptr, _IOFBF, 1 << 20);
        const bool cwf = j.info.fmt >= ICW_FMT_CW_F64;
        if (merge & (cwf ? ICW_BATCH_MERGE_CWAVE : ICW_BATCH_MERGE_INPUTS))
            groups[std::make_tuple(0u, cwf ? 1u : 0u, 0u, key(i))].push_back(&j);
        else groups[std::make_tuple(j.info.sample_rate, j.info.fmt, j.info.channels, key(i))].push_back(&j);
    }
    int rc = ICW_OK;
    for (auto &g : groups) {
        const int r = run(std::get<3>(g.first), g.second, st, sts);
        if (r != ICW_OK) {
            rc = r;
            for (Job *j : g.second) if (sts[j->idx] == ICW_OK) sts[j->idx] = r;
        }
        ++st.n_groups;
    }
    for (Job &j : jobs) {
        if (j.in) fclose(j.in);
        if (j.out && fclose(j.out) != 0 && sts[j.idx] == ICW_OK) sts[j.idx] = ICW_EINVAL;
        if (sts[j.idx] == ICW_OK) ++st.n_files;
        else if (rc == ICW_OK) rc = sts[j.idx];
    }
    st.wall_s = now_s() - t0;
    if (stats) *stats = st;
    return rc;
}

/* a file the WAV / CWAVE parser takes: its status, ICW_EINVAL for a missing path */
int accept_wav(const char *in_path, const char *out_path, icw_wav_info *info)
{
    if (!in_path || !out_path) return ICW_EINVAL;
    return icw_wav_parse_file(in_path, info);
}

/* One group's file pipeline: pinned double buffers, device double buffers, a copy stream (cs) and a
 * compute stream (ks).  Block k of B frames per stream is read from the files, copied in, computed,
 * copied out and written, with the host's file I/O beside the GPU's work on the other buffer. */
struct GroupPipe {
    std::vector<Job *> &jobs;
    icw_batch_stats &st;
    int *status;
    const int S, B;
    const size_t fsz, osz;                /* bytes per input frame (the group's widest: the rows' pitch) / output frame */
    const size_t in_b, out_b;
    std::vector<size_t> ofs;              /* merged encode: every stream's own output frame (<= osz, the rows' pitch); empty: osz */
    /* A slot is a stream of the context and a row of the buffers.  cur: the job each slot reads from (a group:
     * its file, for the whole job; a pool: whatever the plan has put there, nullptr while it is idle).
     * held[p]: the job each slot held when input buffer p was read; wheld[p]: the same for output buffer p, taken
     * over from held[p] when the block is queued.  Block k is written after block k + 1 has been read and
     * queued, so who owned a slot in block k is remembered with buffer k & 1, not looked up from the slot's owner
     * of the moment -- and apart from the input side's map, which block k + 2 overwrites before block k is
     * written.  zb: the zero sample of the slot's last input, what an idle slot is fed. */
    std::vector<Job *> cur, held[2], wheld[2];
    std::vector<unsigned char> zb;
    bool close_done = false;              /* a pool closes a file with its last block, not with the call */
    unsigned char *hin[2] = {nullptr, nullptr}, *hout[2] = {nullptr, nullptr}, *din[2] = {nullptr, nullptr},
                  *dout[2] = {nullptr, nullptr};
    hipStream_t cs = nullptr, ks = nullptr;
    hipEvent_t h2d[2] = {nullptr, nullptr}, comp[2] = {nullptr, nullptr}, d2h[2] = {nullptr, nullptr};

    GroupPipe(std::vector<Job *> &jobs_, int B_, size_t fsz_, size_t osz_, icw_batch_stats &st_, int *status_)
        : GroupPipe(jobs_, (int)jobs_.size(), B_, fsz_, osz_, st_, status_)
    {
        cur = jobs;
        for (int s = 0; s < S; ++s) zb[(size_t)s] = zero_byte(jobs[(size_t)s]->info.fmt);
    }
    /* S_ slots, all idle: a pool, whose jobs come and go (cur) */
    GroupPipe(std::vector<Job *> &jobs_, int S_, int B_, size_t fsz_, size_t osz_, icw_batch_stats &st_, int *status_)
        : jobs(jobs_), st(st_), status(status_), S(S_), B(B_), fsz(fsz_), osz(osz_),
          in_b((size_t)S * B_ * fsz_), out_b((size_t)S * B_ * osz_), cur((size_t)S_, nullptr), zb((size_t)S_, 0)
    {
        held[0] = held[1] = wheld[0] = wheld[1] = cur;
    }
    GroupPipe(const GroupPipe &) = delete;

    ~GroupPipe()
    {
        if (cs) (void)hipStreamSynchronize(cs);
        if (ks) (void)hipStreamSynchronize(ks);
        for (int p = 0; p < 2; ++p) {
            if (hin[p]) (void)hipHostFree(hin[p]);
            if (hout[p]) (void)hipHostFree(hout[p]);
            if (din[p]) (void)hipFree(din[p]);
            if (dout[p]) (void)hipFree(dout[p]);
            for (hipEvent_t e : {h2d[p], comp[p], d2h[p]}) if (e) (void)hipEventDestroy(e);
        }
        if (cs) (void)hipStreamDestroy(cs);
        if (ks) (void)hipStreamDestroy(ks);
    }

    bool alloc()
    {
        bool ok = true;
        for (int p = 0; p < 2 && ok; ++p) {
            ok = hipHostMalloc((void **)&hin[p], in_b, hipHostMallocDefault) == hipSuccess &&
                 hipHostMalloc((void **)&hout[p], out_b, hipHostMallocDefault) == hipSuccess &&
                 hipMalloc((void **)&din[p], in_b) == hipSuccess && hipMalloc((void **)&dout[p], out_b) == hipSuccess &&
                 hipEventCreateWithFlags(&h2d[p], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&comp[p], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&d2h[p], hipEventDisableTiming) == hipSuccess;
        }
        return ok && hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) == hipSuccess &&
               hipStreamCreateWithFlags(&ks, hipStreamNonBlocking) == hipSuccess;
    }

    /* xwave_read_samples: the next nfr input frames of every stream into buf -- data frames, then the
     * format's zero sample */
    void read_frames(unsigned char *buf, int nfr)
    {
        const double t0 = now_s();
        held[buf == hin[1]] = cur;
        for (int s = 0; s < S; ++s) {
            unsigned char *row = buf + (size_t)s * B * fsz;
            if (!cur[(size_t)s]) {
                memset(row, zb[(size_t)s], (size_t)B * fsz);
                continue;
            }
            Job &j = *cur[(size_t)s];
            zb[(size_t)s] = zero_byte(j.info.fmt);
            const size_t jf = j.info.frame_bytes;                          /* the file's own frame (<= fsz) */
            const int64_t want = std::min<int64_t>(nfr, std::max<int64_t>(0, j.info.n_samples - j.read));
            size_t got = 0;
            if (want > 0 && status[j.idx] == ICW_OK) {
                got = fread(row, jf, (size_t)want, j.in);
                if ((int64_t)got != want) status[j.idx] = ICW_EINVAL;      /* short read: broken file */
                j.read += (int64_t)got;
                st.frames_in += got;
            }
            memset(row + got * jf, zero_byte(j.info.fmt), (size_t)(B - (int64_t)got) * jf);
        }
        st.io_s += now_s() - t0;
    }

    void write_block(int k)
    {
        const double t0 = now_s();
        const unsigned char *buf = hout[k & 1];
        for (int s = 0; s < S; ++s) {
            if (!wheld[k & 1][(size_t)s]) continue;
            Job &j = *wheld[k & 1][(size_t)s];
            const int64_t n = std::min<int64_t>(B, j.total - j.written);
            if (n <= 0) continue;
            if (status[j.idx] == ICW_OK) {
                if (fwrite(buf + (size_t)s * B * osz, ofs.empty() ? osz : ofs[(size_t)s], (size_t)n, j.out) != (size_t)n)
                    status[j.idx] = ICW_EINVAL;
                st.frames_out += (uint64_t)n;
            }
            j.written += n;
            if (close_done && j.written == j.total) {
                fclose(j.in);
                j.in = nullptr;
                if (fclose(j.out) != 0 && status[j.idx] == ICW_OK) status[j.idx] = ICW_EINVAL;
                j.out = nullptr;
            }
        }
        st.io_s += now_s() - t0;
    }

    /* nb blocks: compute(p) runs block k from din[p] to dout[p] on ks; after(k, p) follows it once the
     * block's D2H is queued (the encoder's CRC over the frames in HBM) */
    template <class Compute, class After>
    int run(int nb, Compute compute, After after)
    {
        return run(nb, compute, after, [](int) {}, [](int) { return (int)ICW_OK; });
    }

    /* the same for a pool: assign(k) changes the slots' jobs (cur) before block k is read; prepare(k) brings
     * the context's streams in line with them before block k is queued (it waits for the context's work) */
    template <class Compute, class After, class Assign, class Prepare>
    int run(int nb, Compute compute, After after, Assign assign, Prepare prepare)
    {
        int rc = ICW_OK;
        assign(0);
        read_frames(hin[0], B);
        for (int k = 0; k < nb && rc == ICW_OK; ++k) {
            const int p = k & 1;
            if ((rc = prepare(k)) != ICW_OK) break;
            wheld[p] = held[p];
            /* H2D(k): d_in[p] was last read by compute(k-2); d_out[p] by D2H(k-2), which compute(k) waits for */
            if (k >= 2 && (hipStreamWaitEvent(cs, comp[p], 0) != hipSuccess || hipStreamWaitEvent(ks, d2h[p], 0) != hipSuccess))
                rc = ICW_EDEVICE;
            if (rc == ICW_OK && (hipMemcpyAsync(din[p], hin[p], in_b, hipMemcpyHostToDevice, cs) != hipSuccess ||
                                 hipEventRecord(h2d[p], cs) != hipSuccess || hipStreamWaitEvent(ks, h2d[p], 0) != hipSuccess))
                rc = ICW_EDEVICE;
            if (rc == ICW_OK) rc = compute(p);
            if (rc == ICW_OK && (hipEventRecord(comp[p], ks) != hipSuccess || hipStreamWaitEvent(cs, comp[p], 0) != hipSuccess ||
                                 hipMemcpyAsync(hout[p], dout[p], out_b, hipMemcpyDeviceToHost, cs) != hipSuccess ||
                                 hipEventRecord(d2h[p], cs) != hipSuccess))
                rc = ICW_EDEVICE;
            if (rc != ICW_OK) break;
            if ((rc = after(k, p)) != ICW_OK) break;
            /* host work overlapping the GPU: read block k+1 (after H2D(k-1) released its buffer),
             * write block k-1 (after its D2H) */
            if (k + 1 < nb) {
                if (k >= 1 && hipEventSynchronize(h2d[(k + 1) & 1]) != hipSuccess) { rc = ICW_EDEVICE; break; }
                assign(k + 1);
                read_frames(hin[(k + 1) & 1], B);
            }
            if (k >= 1) {
                if (hipEventSynchronize(d2h[(k - 1) & 1]) != hipSuccess) { rc = ICW_EDEVICE; break; }
                write_block(k - 1);
            }
        }
        if (rc == ICW_OK && nb >= 1) {
            if (hipEventSynchronize(d2h[(nb - 1) & 1]) != hipSuccess) rc = ICW_EDEVICE;
            else write_block(nb - 1);
        }
        return rc;
    }
};

/* One group of files: one context, one stream per file.  The files share (rate, format, channels), or
 * (ICW_BATCH_MERGE_INPUTS, ICW_BATCH_MERGE_CWAVE) every stream gets its own file's input before the first
 * block. */
int run_group(const icw_config &cfg0, const icw_node *nodes, int n_nodes, std::vector<Job *> &jobs,
              const icw_batch_opts &o, icw_batch_stats &st, int *status, const FileLists &fl = FileLists())
{
    const int S = (int)jobs.size();
    const icw_wav_info &wi = jobs[0]->info;
    icw_config cfg = cfg0;
    cfg.sample_rate = wi.sample_rate;
    cfg.in_format = wi.fmt;
    cfg.in_channels = wi.channels;
    if (fl.nodes) {
        /* the context starts on the first file's list; a group of differing lists then gives every
         * stream its own before the first block */
        nodes = fl.nodes[jobs[0]->idx];
        n_nodes = fl.n_nodes[jobs[0]->idx];
        if (fl.bypass) cfg.bypass_list = fl.bypass[jobs[0]->idx];
    }
    icw_ctx *ctx = nullptr;
    int accepted = 0;
    int rc = icw_create(&cfg, nodes, n_nodes, S, o.device, &ctx, &accepted);
    if (rc != ICW_OK) return rc;
    std::unique_ptr<icw_ctx, int (*)(icw_ctx *)> guard(ctx, icw_destroy);
    /* a CWAVE group is analytic already: the converter is for real input */
    if (fl.k_M > 0 && wi.fmt < ICW_FMT_CW_F64 &&
        ((rc = icw_enable_stream_fir(ctx, 1)) != ICW_OK || (rc = icw_set_fir_hilbert(ctx, fl.k_M, fl.k_beta)) != ICW_OK))
        return rc;
    /* a merged group of CWAVE files: per-stream CWAVE inputs are the context's to ask for */
    if (wi.fmt >= ICW_FMT_CW_F64 && (o.reserved_ & ICW_BATCH_MERGE_CWAVE) && (rc = icw_enable_stream_cwave(ctx, 1)) != ICW_OK)
        return rc;
    /* a merged group of bus-form files: per-stream bus-form lists are the context's to ask for */
    if (fl.bus && (rc = icw_enable_stream_bus(ctx, 1)) != ICW_OK) return rc;
    for (int s = 1; s < S && fl.per_stream; ++s) {
        const int i = jobs[s]->idx;
        rc = icw_set_stream_graph(ctx, s, 1, fl.nodes[i], fl.n_nodes[i], fl.bypass ? fl.bypass[i] : cfg0.bypass_list,
                                  &accepted);
        if (rc != ICW_OK) return rc;
    }
    size_t fsz = wi.frame_bytes;
    for (int s = 1; s < S; ++s) {
        const icw_wav_info &ji = jobs[s]->info;
        fsz = std::max<size_t>(fsz, ji.frame_bytes);
        if ((ji.sample_rate != wi.sample_rate || ji.fmt != wi.fmt || ji.channels != wi.channels) &&
            (rc = icw_set_stream_input(ctx, s, 1, ji.sample_rate, ji.fmt, ji.channels)) != ICW_OK)
            return rc;
    }
    const int rs = icw_render_size(ctx), osz = 2 * rs;
    const int B = o.block_frames > 0 ? o.block_frames : 65536;
    int64_t T = 0;
    for (int s = 0; s < S; ++s) {
        Job &j = *jobs[s];
        /* xwave_reader_create's virtual zero tail (xwave_reader.c:688-697) */
        int64_t tail = 0;
        if (o.sec_align) {
            const int64_t mt = (int64_t)j.info.sample_rate * (int64_t)o.sec_align, fr = j.info.n_samples % mt;
            tail = fr ? mt - fr : 0;
        }
        j.total = j.info.n_samples + tail;
        T = std::max(T, j.total);
        if ((rc = icw_stream_open(ctx, s, j.info.n_samples, o.fade_in_ms, o.fade_out_ms, o.sec_align, 0, 0)) != ICW_OK)
            return rc;
        unsigned char hdr[44];
        wav_header(hdr, j.info.sample_rate, rs, (uint64_t)j.total);
        if (fwrite(hdr, 1, 44, j.out) != 44) status[j.idx] = ICW_EINVAL;
        if (fseeko(j.in, j.info.data_offset, SEEK_SET)) status[j.idx] = ICW_EINVAL;
    }
    GroupPipe pp(jobs, B, fsz, (size_t)osz, st, status);
    if (!pp.alloc()) return ICW_ENOMEM;
    rc = pp.run((int)((T + B - 1) / B),
                [&](int p) {
                    return icw_process_streams(ctx, 0, S, pp.din[p], (size_t)B * fsz, pp.dout[p], (size_t)B * osz, B,
                                               ICW_F_DEVICE_PTRS, nullptr, pp.ks);
                },
                [](int, int) { return (int)ICW_OK; });
    if (rc == ICW_OK) rc = icw_synchronize(ctx);
    return rc;
}

/* files a and b of a lists call carry the same list */
bool same_file_list(const FileLists &fl, int cfg_bypass, int a, int b)
{
    const int ba = fl.bypass ? fl.bypass[a] : cfg_bypass, bb = fl.bypass ? fl.bypass[b] : cfg_bypass;
    return fl.n_nodes[a] == fl.n_nodes[b] && !ba == !bb &&
           (fl.n_nodes[a] == 0 || !memcmp(fl.nodes[a], fl.nodes[b], (size_t)fl.n_nodes[a] * sizeof(icw_node)));
}

/* One pool of icw_transcode_files_pool: the files of one kind through one context of plan.slots streams.  The
 * plan (icw_pool_plan.h) says which slot every file runs in and the block in which it starts; this executes
 * it.  At a block boundary the slots' jobs change on the host side first (assign: before the block is read),
 * then, all refills of the boundary together and before the block is queued, the context follows (prepare):
 * the ended files' meters; the new file's input and list where they differ from what the slot holds;
 * icw_stream_init for a slot that has held a file; icw_stream_open last, since it takes the fades at the
 * stream's rate. */
/* icw_transcode_files_jobs: file i's own render and converter beside its list (jobs null: the pool proper).  The
 * plan then keeps every class of files in a range of slots of its own (icw_pool_make_plan_classes); each range
 * gets its class's setting once, before block 0, and a refill stays what it is. */
struct PoolJobs {
    const icw_file_job *jobs = nullptr;   /* indexed like the files */
    bool timing = false;                  /* ICW_BATCH_TIMING */
    icw_jobs_stats *js = nullptr;
};

int run_pool(const icw_config &cfg0, std::vector<Job *> &jobs, const icw_pool_opts &po, const FileLists &fl,
             icw_batch_stats &st, icw_pool_stats &ps, icw_meters *meters, int *status, const PoolJobs &pj = PoolJobs())
{
    const icw_batch_opts &o = po.batch;
    const int n = (int)jobs.size();
    const int B = o.block_frames > 0 ? o.block_frames : 65536;
    std::vector<int64_t> totals((size_t)n);
    size_t fsz = 0;
    for (int q = 0; q < n; ++q) {
        Job &j = *jobs[(size_t)q];
        /* xwave_reader_create's virtual zero tail (xwave_reader.c:688-697) */
        int64_t tail = 0;
        if (o.sec_align) {
            const int64_t mt = (int64_t)j.info.sample_rate * (int64_t)o.sec_align, fr = j.info.n_samples % mt;
            tail = fr ? mt - fr : 0;
        }
        totals[(size_t)q] = j.total = j.info.n_samples + tail;
        fsz = std::max<size_t>(fsz, j.info.frame_bytes);
    }
    IcwPoolPlan plan;
    IcwClassPlan cplan;
    std::vector<const icw_file_job *> class_job;          /* jobs: a job of every class, in layout order */
    int rc = ICW_OK;
    if (pj.jobs) {
        /* a bus-form context holds one class (the caller's grouping); else the classes of the files' settings */
        std::vector<icw_file_job> gj;
        for (const Job *j : jobs) gj.push_back(pj.jobs[j->idx]);
        const std::vector<char> take((size_t)n, 1);
        std::vector<int32_t> pos((size_t)n, 0);
        std::vector<std::pair<int, int>> settings(1);
        const bool cw = jobs[0]->info.fmt >= ICW_FMT_CW_F64;
        const int K = fl.bus ? 1 : icw_pool_job_classes(gj.data(), take.data(), n, cw, pos, &settings);
        if ((rc = icw_pool_make_plan_classes(totals.data(), pos.data(), n, K, po.slots, B, po.order, cplan)) != ICW_OK) return rc;
        plan = cplan.pool;
        class_job.assign((size_t)K, nullptr);
        for (int q = n - 1; q >= 0; --q) class_job[(size_t)pos[(size_t)q]] = &pj.jobs[jobs[(size_t)q]->idx];
        int hruns = cw ? 0 : 1, rruns = 1;
        for (int c = 1; c < K; ++c) {
            hruns += !cw && settings[(size_t)c].first != settings[(size_t)c - 1].first;
            rruns += settings[(size_t)c].second != settings[(size_t)c - 1].second;
        }
        pj.js->classes += K;
        pj.js->hilbert_runs_max = std::max(pj.js->hilbert_runs_max, hruns);
        pj.js->render_runs_max = std::max(pj.js->render_runs_max, rruns);
    } else if ((rc = icw_pool_make_plan(totals.data(), n, po.slots, B, po.order, plan)) != ICW_OK) {
        return rc;
    }
    const int S = plan.slots, nb = (int)plan.blocks;
    std::vector<std::vector<Job *>> starts((size_t)nb + 1), ends((size_t)nb + 1);
    for (int q : plan.queue) {
        Job *j = jobs[(size_t)q];
        j->slot = plan.slot[(size_t)q];
        starts[(size_t)plan.start[(size_t)q]].push_back(j);
        ends[(size_t)(plan.start[(size_t)q] + plan.n_blocks[(size_t)q])].push_back(j);
    }
    /* the context starts on the input and the list of the first file to run; every slot holds them until a
     * file brings its own */
    const Job &j0 = *jobs[(size_t)plan.queue[0]];
    icw_config cfg = cfg0;
    cfg.sample_rate = j0.info.sample_rate;
    cfg.in_format = j0.info.fmt;
    cfg.in_channels = j0.info.channels;
    if (fl.bypass) cfg.bypass_list = fl.bypass[j0.idx];
    if (pj.jobs) {
        /* the context starts on the first file's setting too: a bus-form context keeps it, it has one class */
        const icw_file_job &fj = pj.jobs[j0.idx];
        cfg.render = fj.render;
        cfg.need24bits = fj.need24bits;
        cfg.hilbert_type = fj.hilbert_type;
        cfg.iir_kahan = fj.iir_kahan;
        cfg.iir_subnorm_reject = fj.iir_subnorm_reject;
    }
    icw_ctx *ctx = nullptr;
    int accepted = 0;
    if ((rc = icw_create(&cfg, fl.nodes[j0.idx], fl.n_nodes[j0.idx], S, o.device, &ctx, &accepted)) != ICW_OK) return rc;
    std::unique_ptr<icw_ctx, int (*)(icw_ctx *)> guard(ctx, icw_destroy);
    if (j0.info.fmt >= ICW_FMT_CW_F64 && (rc = icw_enable_stream_cwave(ctx, 1)) != ICW_OK) return rc;
    if (fl.bus && (rc = icw_enable_stream_bus(ctx, 1)) != ICW_OK) return rc;
    /* every class's range gets its setting, once: the ranges never change class */
    for (size_t c = 0; pj.jobs && !fl.bus && c < class_job.size(); ++c) {
        const icw_file_job &fj = *class_job[c];
        const int first = cplan.first[c], count = cplan.share[c];
        if (j0.info.fmt < ICW_FMT_CW_F64 &&
            (rc = icw_set_stream_hilbert(ctx, first, count, fj.hilbert_type, fj.iir_kahan, fj.iir_subnorm_reject)) != ICW_OK)
            return rc;
        if ((rc = icw_set_stream_render(ctx, first, count, &fj.render, fj.need24bits)) != ICW_OK) return rc;
    }
    const int rs = icw_render_size(ctx), osz = 2 * rs;    /* the widest in force: the rows' pitch */
    std::vector<const Job *> in_of((size_t)S, &j0), list_of((size_t)S, &j0);   /* whose input / list a slot holds */
    std::vector<char> used((size_t)S, 0);
    GroupPipe pp(jobs, S, B, fsz, (size_t)osz, st, status);
    pp.close_done = true;
    /* every slot's own sample size, constant like its class: its files' headers and the bytes written of a row */
    std::vector<int> slot_rs((size_t)S, rs);
    for (int s = 0; pj.jobs && s < S; ++s) {
        slot_rs[(size_t)s] = icw_stream_render_size(ctx, s);
        pp.ofs.push_back(2 * (size_t)slot_rs[(size_t)s]);
    }
    if (!pp.alloc()) return ICW_ENOMEM;
    const unsigned flags = ICW_F_DEVICE_PTRS | (pj.timing ? ICW_F_TIMING : 0u);
    const auto read_meters = [&](int k) {
        int r = ICW_OK;
        for (Job *j : ends[(size_t)k])
            if (meters && r == ICW_OK) r = icw_get_meters(ctx, j->slot, 0, &meters[j->idx]);
        return r;
    };
    rc = pp.run(nb,
                [&](int p) {
                    int r = icw_process_streams(ctx, 0, S, pp.din[p], (size_t)B * fsz, pp.dout[p], (size_t)B * osz, B, flags,
                                                nullptr, pp.ks);
                    double ms[2] = {0.0, 0.0};
                    int launches[2];
                    if (r == ICW_OK && pj.timing && (r = icw_last_timing(ctx, ms, launches)) == ICW_OK)
                        pj.js->kernel_s += (ms[0] + ms[1]) * 1e-3;
                    return r;
                },
                [](int, int) { return (int)ICW_OK; },
                [&](int k) {
                    for (Job *j : ends[(size_t)k]) pp.cur[(size_t)j->slot] = nullptr;
                    for (Job *j : starts[(size_t)k]) {
                        pp.cur[(size_t)j->slot] = j;
                        unsigned char hdr[44];
                        wav_header(hdr, j->info.sample_rate, slot_rs[(size_t)j->slot], (uint64_t)j->total);
                        if (fwrite(hdr, 1, 44, j->out) != 44) status[j->idx] = ICW_EINVAL;
                        if (fseeko(j->in, j->info.data_offset, SEEK_SET)) status[j->idx] = ICW_EINVAL;
                    }
                },
                [&](int k) {
                    int r = read_meters(k);
                    for (Job *j : starts[(size_t)k]) {
                        if (r != ICW_OK) break;
                        const size_t s = (size_t)j->slot;
                        const icw_wav_info &ji = j->info, &si = in_of[s]->info;
                        if (ji.sample_rate != si.sample_rate || ji.fmt != si.fmt || ji.channels != si.channels)
                            r = icw_set_stream_input(ctx, j->slot, 1, ji.sample_rate, ji.fmt, ji.channels);
                        in_of[s] = j;
                        if (r == ICW_OK && !same_file_list(fl, cfg0.bypass_list, list_of[s]->idx, j->idx))
                            r = icw_set_stream_graph(ctx, j->slot, 1, fl.nodes[j->idx], fl.n_nodes[j->idx],
                                                     fl.bypass ? fl.bypass[j->idx] : cfg0.bypass_list, &accepted);
                        list_of[s] = j;
                        if (r == ICW_OK && used[s]) r = icw_stream_init(ctx, j->slot, 1);
                        used[s] = 1;
                        if (r == ICW_OK)
                            r = icw_stream_open(ctx, j->slot, ji.n_samples, o.fade_in_ms, o.fade_out_ms, o.sec_align, 0, 0);
                    }
                    return r;
                });
    if (rc == ICW_OK) rc = icw_synchronize(ctx);
    if (rc == ICW_OK) rc = read_meters(nb);
    ps.slots = std::max(ps.slots, plan.slots);
    ps.refills += plan.refills;
    ps.blocks += plan.blocks;
    ps.slot_blocks += plan.slot_blocks;
    ps.busy_slot_blocks += plan.busy_slot_blocks;
    return rc;
}

/* what a group needs of an encoder's options: icw_cwave_enc_opts (the FIR converter),
 * icw_cwave_enc_iir_opts (iir: the quadrature IIR; k_M 0, k_beta 0.0, no aligned mode), or
 * icw_cwave_enc_fft_opts (the direct FFT: k_M -1, k_beta 0.0, whole tracks within max_bytes) */
struct EncSpec {
    int32_t k_M = 0, align = 0;
    double k_beta = 0.0;
    uint32_t cw_format = 0;
    int32_t block_frames = 0, device = -1;
    bool iir = false;
    uint32_t hilbert_type = 1;
    int32_t iir_kahan = 1, iir_subnorm_reject = 1;
    uint64_t max_bytes = 0;
    bool merge = false;                /* ICW_ENC_MERGE_INPUTS: one context, every stream its file's input */
};

/* bytes of block k (B frames per block) that belong to a file of `total` frames of FB bytes: its part of the
 * file's CRC and of what is written */
uint64_t enc_block_bytes(int64_t total, int64_t k, int64_t B, size_t FB)
{
    return (uint64_t)std::max<int64_t>(0, std::min<int64_t>(B, total - k * B)) * FB;
}

/* HCWAVE_V2 (cwave.h:48-60), little-endian */
void cwave_header(unsigned char *h, const EncSpec &o, uint32_t channels, uint32_t frames, uint32_t rate, uint32_t crc)
{
    auto p32 = [](unsigned char *q, uint32_t v) { q[0] = v; q[1] = v >> 8; q[2] = v >> 16; q[3] = v >> 24; };
    memcpy(h, "cPLXwAVE", 8);
    p32(h + 8, ICW_CWAVE_HEADER_BYTES);
    p32(h + 12, 2);
    p32(h + 16, o.cw_format - ICW_FMT_CW_F64);
    p32(h + 20, channels);
    p32(h + 24, frames);
    p32(h + 28, rate);
    p32(h + 32, (uint32_t)o.k_M);
    p32(h + 36, crc);
    uint64_t b;
    memcpy(&b, &o.k_beta, 8);
    p32(h + 40, (uint32_t)b);
    p32(h + 44, (uint32_t)(b >> 32));
}

/* One group of WAV files sharing (rate, format, channels) -- or (o.merge) every accepted file, each stream
 * given its own file's input; the rows are then as wide as the widest input and output frame, and headers,
 * CRC lengths and writes use each file's own -- through the CWAVE encoder: one context, one
 * fresh stream per file, no fades, no tail.  The CRC of every file's data is chained block by block
 * over the packed frames while they are in HBM (icw_crc32_batch, device pointers). */
int run_enc_group(std::vector<Job *> &jobs, const EncSpec &o, icw_batch_stats &st, uint64_t *clipped, int *status)
{
    const int S = (int)jobs.size();
    const icw_wav_info &wi = jobs[0]->info;
    icw_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.sample_rate = wi.sample_rate;
    cfg.in_format = wi.fmt;
    cfg.in_channels = wi.channels;
    cfg.hilbert_type = o.hilbert_type;
    cfg.iir_kahan = o.iir_kahan;
    cfg.iir_subnorm_reject = o.iir_subnorm_reject;
    cfg.frmod_scaled = 1;
    cfg.seed_left = ICW_SEED_LEFT;
    cfg.seed_right = ICW_SEED_RIGHT;
    cfg.render.dth_bits = 1.0;
    cfg.render.sign_bits16 = 16;
    cfg.render.sign_bits24 = 24;
    icw_ctx *ctx = nullptr;
    int rc = icw_create(&cfg, nullptr, 0, S, o.device, &ctx, nullptr);
    if (rc != ICW_OK) return rc;
    std::unique_ptr<icw_ctx, int (*)(icw_ctx *)> guard(ctx, icw_destroy);
    if (o.merge && ((rc = icw_enable_stream_encode(ctx, 1)) != ICW_OK || (!o.iir && (rc = icw_enable_stream_fir(ctx, 1)) != ICW_OK)))
        return rc;
    if (!o.iir && (rc = icw_set_fir_hilbert(ctx, o.k_M, o.k_beta)) != ICW_OK) return rc;
    const auto encode = o.iir ? icw_encode_cwave_iir : icw_encode_cwave;
    size_t fsz = 0, FB = 0;
    std::vector<size_t> FBs((size_t)S);
    for (int s = 0; s < S; ++s) {
        const icw_wav_info &ji = jobs[s]->info;
        FBs[(size_t)s] = (size_t)icw_cwave_frame_bytes(o.cw_format, ji.channels);
        fsz = std::max<size_t>(fsz, ji.frame_bytes);
        FB = std::max(FB, FBs[(size_t)s]);
        if ((ji.sample_rate != wi.sample_rate || ji.fmt != wi.fmt || ji.channels != wi.channels) &&
            (rc = icw_set_stream_input(ctx, s, 1, ji.sample_rate, ji.fmt, ji.channels)) != ICW_OK)
            return rc;
    }
    const int skip = o.align ? o.k_M / 2 : 0;            /* aligned: the first k_M/2 output frames are dropped */
    const int B = std::max(o.block_frames > 0 ? o.block_frames : 65536, std::max(skip, 64));
    int64_t T = 0;
    for (int s = 0; s < S; ++s) {
        Job &j = *jobs[s];
        j.total = j.info.n_samples;                       /* file frames */
        T = std::max(T, j.total);
        if ((rc = icw_stream_open(ctx, s, j.info.n_samples + skip, 0, 0, 0, 0, 0)) != ICW_OK) return rc;
        unsigned char hdr[ICW_CWAVE_HEADER_BYTES];
        cwave_header(hdr, o, j.info.channels, (uint32_t)j.total, j.info.sample_rate, 0);
        if (fwrite(hdr, 1, sizeof(hdr), j.out) != sizeof(hdr)) status[j.idx] = ICW_EINVAL;
        if (fseeko(j.in, j.info.data_offset, SEEK_SET)) status[j.idx] = ICW_EINVAL;
    }
    GroupPipe pp(jobs, B, fsz, FB, st, status);
    if (o.merge) pp.ofs = FBs;
    if (!pp.alloc()) return ICW_ENOMEM;
    /* aligned mode: the k_M/2 frames that are dropped go through first, on their own (so that neither the
     * CRC nor the clip counts see them) */
    if (skip) {
        pp.read_frames(pp.hin[0], skip);
        if (hipMemcpyAsync(pp.din[0], pp.hin[0], pp.in_b, hipMemcpyHostToDevice, pp.ks) != hipSuccess) rc = ICW_EDEVICE;
        if (rc == ICW_OK)
            rc = encode(ctx, 0, S, pp.din[0], (size_t)B * fsz, pp.dout[0], (size_t)B * FB, skip, o.cw_format, ICW_F_DEVICE_PTRS, pp.ks);
        for (int s = 0; s < S && rc == ICW_OK; ++s) rc = icw_encode_clipped(ctx, s, 1, nullptr);
        if (rc != ICW_OK) return rc;
    }
    std::vector<uint32_t> crc(S, 0u);
    std::vector<uint64_t> off(S), len(S);
    rc = pp.run((int)((T + B - 1) / B),
                [&](int p) {
                    return encode(ctx, 0, S, pp.din[p], (size_t)B * fsz, pp.dout[p], (size_t)B * FB, B, o.cw_format,
                                  ICW_F_DEVICE_PTRS, pp.ks);
                },
                /* this block's part of every file's CRC, from the frames in HBM (returns once the kernel is done) */
                [&](int k, int p) {
                    for (int s = 0; s < S; ++s) {
                        off[s] = (uint64_t)s * B * FB;
                        len[s] = enc_block_bytes(jobs[s]->total, k, B, FBs[(size_t)s]);
                    }
                    return icw_crc32_batch(pp.dout[p], off.data(), len.data(), S, crc.data(), crc.data(), ICW_F_DEVICE_PTRS,
                                           o.device, pp.ks);
                });
    if (rc == ICW_OK) rc = icw_synchronize(ctx);
    for (int s = 0; s < S && rc == ICW_OK; ++s) {
        Job &j = *jobs[s];
        uint64_t nclip = 0;
        rc = icw_encode_clipped(ctx, s, 0, &nclip);
        if (clipped) clipped[j.idx] = nclip;
        unsigned char hdr[ICW_CWAVE_HEADER_BYTES];
        cwave_header(hdr, o, j.info.channels, (uint32_t)j.total, j.info.sample_rate, crc[s]);
        if (status[j.idx] == ICW_OK && (fseeko(j.out, 0, SEEK_SET) || fwrite(hdr, 1, sizeof(hdr), j.out) != sizeof(hdr)))
            status[j.idx] = ICW_EINVAL;
    }
    return rc;
}

/* icw_cwave_encode_files / icw_cwave_encode_files_iir after their option checks */
int encode_files(const char *const *in_paths, const char *const *out_paths, int n, const EncSpec &o,
                 icw_batch_stats *stats, uint64_t *clipped, int *status)
{
    return for_file_groups(
        in_paths, out_paths, n, stats, status,
        [&](int i, Job &j) {
            if (clipped) clipped[i] = 0;
            if (accept_wav(in_paths[i], out_paths[i], &j.info) != ICW_OK ||
                j.info.fmt >= ICW_FMT_CW_F64 ||                      /* a CWAVE file is analytic already */
                j.info.n_samples < 2 || j.info.n_samples >= ((int64_t)1 << 32))
                return (int)ICW_EINVAL;
            return (int)ICW_OK;
        },
        [](int) { return 0; },
        [&](int, std::vector<Job *> &g, icw_batch_stats &st, int *sts) { return run_enc_group(g, o, st, clipped, sts); },
        o.merge ? ICW_BATCH_MERGE_INPUTS : 0u);
}

/* One group of WAV files sharing (format, channels) through the direct-FFT encoder: whole tracks, no blocks.
 * The files are packed, in order, into calls whose device working set (PCM, transforms, frames) fits
 * o.max_bytes; a file that alone exceeds it runs alone.  Per call: read the files, one copy in,
 * icw_encode_cwave_fft and icw_crc32_batch on the frames in HBM (device pointers), one copy out, write. */
int run_fft_group(std::vector<Job *> &jobs, const EncSpec &o, icw_batch_stats &st, uint64_t *clipped, int *status)
{
    const icw_wav_info &wi = jobs[0]->info;
    const size_t fsz = wi.frame_bytes, FB = (size_t)icw_cwave_frame_bytes(o.cw_format, wi.channels);
    const uint64_t budget = o.max_bytes ? o.max_bytes : (uint64_t)16 << 30;
    auto al16 = [](uint64_t v) { return (v + 15) & ~(uint64_t)15; };
    if (o.device >= 0 && hipSetDevice(o.device) != hipSuccess) return ICW_EDEVICE;
    icw_fft_enc_opts fo = {o.device, 0};
    for (size_t k0 = 0; k0 < jobs.size();) {
        std::vector<uint64_t> nfr, ioff, ooff, len;
        uint64_t need = 0, in_b = 0, out_b = 0;
        size_t k1 = k0;
        for (; k1 < jobs.size(); ++k1) {
            const uint64_t N = (uint64_t)jobs[k1]->info.n_samples;
            const uint64_t cost = icw_encode_cwave_fft_workspace(&N, 1, wi.channels) + al16(N * fsz) + al16(N * FB);
            if (k1 > k0 && need + cost > budget) break;
            need += cost;
            nfr.push_back(N);
            ioff.push_back(in_b);
            ooff.push_back(out_b);
            len.push_back(N * FB);
            in_b += al16(N * fsz);
            out_b += al16(N * FB);
        }
        const int cnt = (int)(k1 - k0);
        std::vector<unsigned char> hin(in_b), hout(out_b);
        double t0 = now_s();
        for (int k = 0; k < cnt; ++k) {
            Job &j = *jobs[k0 + k];
            if (fseeko(j.in, j.info.data_offset, SEEK_SET) || fread(hin.data() + ioff[k], fsz, nfr[k], j.in) != nfr[k])
                status[j.idx] = ICW_EINVAL;                /* short read: broken file */
            else
                st.frames_in += nfr[k];
        }
        st.io_s += now_s() - t0;
        unsigned char *din = nullptr, *dout = nullptr;
        int rc = ICW_OK;
        if (hipMalloc((void **)&din, in_b) != hipSuccess || hipMalloc((void **)&dout, out_b) != hipSuccess) rc = ICW_ENOMEM;
        if (rc == ICW_OK && hipMemcpy(din, hin.data(), in_b, hipMemcpyHostToDevice) != hipSuccess) rc = ICW_EDEVICE;
        std::vector<uint64_t> clip(cnt, 0);
        std::vector<uint32_t> crc(cnt, 0u);
        if (rc == ICW_OK)
            rc = icw_encode_cwave_fft(din, ioff.data(), nfr.data(), cnt, wi.fmt, wi.channels, dout, ooff.data(), o.cw_format,
                                      clip.data(), ICW_F_DEVICE_PTRS, &fo, nullptr);
        if (rc == ICW_OK)
            rc = icw_crc32_batch(dout, ooff.data(), len.data(), cnt, nullptr, crc.data(), ICW_F_DEVICE_PTRS, o.device, nullptr);
        if (rc == ICW_OK && hipMemcpy(hout.data(), dout, out_b, hipMemcpyDeviceToHost) != hipSuccess) rc = ICW_EDEVICE;
        if (din) (void)hipFree(din);
        if (dout) (void)hipFree(dout);
        if (rc != ICW_OK) return rc;
        t0 = now_s();
        for (int k = 0; k < cnt; ++k) {
            Job &j = *jobs[k0 + k];
            if (status[j.idx] != ICW_OK) continue;
            unsigned char hdr[ICW_CWAVE_HEADER_BYTES];
            cwave_header(hdr, o, wi.channels, (uint32_t)nfr[k], j.info.sample_rate, crc[k]);
            if (fwrite(hdr, 1, sizeof(hdr), j.out) != sizeof(hdr) || fwrite(hout.data() + ooff[k], FB, nfr[k], j.out) != nfr[k]) {
                status[j.idx] = ICW_EINVAL;
                continue;
            }
            if (clipped) clipped[j.idx] = clip[k];
            j.total = j.written = (int64_t)nfr[k];
            st.frames_out += nfr[k];
        }
        st.io_s += now_s() - t0;
        k0 = k1;
    }
    return ICW_OK;
}

}  // namespace

extern "C" {

int icw_cwave_encode_files_fft(const char *const *in_paths, const char *const *out_paths, int n,
                               const icw_cwave_enc_fft_opts *opts, icw_batch_stats *stats, uint64_t *clipped, int *status)
{
    if (!opts || n < 0 || (n > 0 && (!in_paths || !out_paths))) return ICW_EINVAL;
    if (opts->cw_format < ICW_FMT_CW_F64 || opts->cw_format > ICW_FMT_CW_F32) return ICW_EINVAL;
    EncSpec e;
    e.k_M = -1;
    e.cw_format = opts->cw_format;
    e.device = opts->device;
    e.max_bytes = opts->max_bytes;
    /* the groups: (format, channels) alone -- the rate only goes into the header */
    std::vector<int> shape(n > 0 ? n : 1, 0);
    return for_file_groups(
        in_paths, out_paths, n, stats, status,
        [&](int i, Job &j) {
            if (clipped) clipped[i] = 0;
            if (accept_wav(in_paths[i], out_paths[i], &j.info) != ICW_OK || j.info.fmt >= ICW_FMT_CW_F64 || j.info.n_samples < 2)
                return (int)ICW_EINVAL;
            if (j.info.n_samples > ((int64_t)1 << ICW_FFT_MAX_LOG2)) return (int)ICW_EUNSUPPORTED;
            shape[i] = (int)(j.info.fmt * 16 + j.info.channels);
            return (int)ICW_OK;
        },
        [&](int i) { return shape[i]; },
        [&](int, std::vector<Job *> &g, icw_batch_stats &st, int *sts) { return run_fft_group(g, e, st, clipped, sts); },
        ICW_BATCH_MERGE_INPUTS);
}

int icw_cwave_encode_files(const char *const *in_paths, const char *const *out_paths, int n, const icw_cwave_enc_opts *opts,
                           icw_batch_stats *stats, uint64_t *clipped, int *status)
{
    if (!opts || n < 0 || (n > 0 && (!in_paths || !out_paths))) return ICW_EINVAL;
    const icw_cwave_enc_opts &o = *opts;
    if (o.k_M < 2 || o.k_M > ICW_FIR_MAX_ORDER || (o.k_M & 1) || !(o.k_beta >= 0.0 && o.k_beta < 1e3) ||
        o.cw_format < ICW_FMT_CW_F64 || o.cw_format > ICW_FMT_CW_F32 || (o.align != 0 && o.align != 1) || o.block_frames < 0)
        return ICW_EINVAL;
    EncSpec e;
    e.k_M = o.k_M;
    e.align = o.align;
    e.k_beta = o.k_beta;
    e.cw_format = o.cw_format;
    e.block_frames = o.block_frames;
    e.device = o.device;
    e.merge = (o.reserved_ & ICW_ENC_MERGE_INPUTS) != 0;
    return encode_files(in_paths, out_paths, n, e, stats, clipped, status);
}

int icw_cwave_encode_files_iir(const char *const *in_paths, const char *const *out_paths, int n,
                               const icw_cwave_enc_iir_opts *opts, icw_batch_stats *stats, uint64_t *clipped, int *status)
{
    if (!opts || n < 0 || (n > 0 && (!in_paths || !out_paths))) return ICW_EINVAL;
    const icw_cwave_enc_iir_opts &o = *opts;
    if (o.hilbert_type > 5 || (o.iir_kahan != 0 && o.iir_kahan != 1) || (o.iir_subnorm_reject != 0 && o.iir_subnorm_reject != 1) ||
        o.cw_format < ICW_FMT_CW_F64 || o.cw_format > ICW_FMT_CW_F32 || o.block_frames < 0)
        return ICW_EINVAL;
    EncSpec e;
    e.iir = true;
    e.hilbert_type = o.hilbert_type;
    e.iir_kahan = o.iir_kahan;
    e.iir_subnorm_reject = o.iir_subnorm_reject;
    e.cw_format = o.cw_format;
    e.block_frames = o.block_frames;
    e.device = o.device;
    e.merge = (o.reserved_ & ICW_ENC_MERGE_INPUTS) != 0;
    return encode_files(in_paths, out_paths, n, e, stats, clipped, status);
}

int icw_wav_parse_file(const char *path, icw_wav_info *info)
{
    if (!path || !info) return ICW_EINVAL;
    memset(info, 0, sizeof(*info));
    const char *dot = strrchr(path, '.');
    if (!dot) return ICW_EINVAL;
    const bool cw = !strcasecmp(dot + 1, "CWAVE");
    if (!cw && strcasecmp(dot + 1, "WAV") && strcasecmp(dot + 1, "RWAVE")) return ICW_EINVAL;
    File fh;
    if (!(fh.f = fopen(path, "rb"))) return ICW_EINVAL;
    const int64_t fsize = file_size(fh.f);
    if (fsize < 0) return ICW_EINVAL;
    int rc;
    if (cw) {
        unsigned char hdr[ICW_CWAVE_HEADER_BYTES];
        if (!rd(fh.f, hdr, sizeof(hdr))) return ICW_EINVAL;
        icw_cwave_header h;
        uint32_t fmt = 0, fb = 0;
        if ((rc = icw_cwave_parse(hdr, sizeof(hdr), fsize, &h, &fmt, &fb)) != ICW_OK) return rc;
        info->fmt = fmt;
        info->channels = h.n_channels;
        info->sample_rate = h.sample_rate;
        info->frame_bytes = fb;
        info->n_samples = h.n_samples;
        info->data_offset = h.hsize;
        info->htype = ICW_HTYPE_CWAVE;
    } else if ((rc = parse_rwave(fh.f, fsize, info)) != ICW_OK) {
        return rc;
    }
    if (info->sample_rate > ICW_MAX_FS_SRC) return ICW_EINVAL;         /* xwave_reader.c:672-674 */
    return ICW_OK;
}

int icw_transcode_files(const icw_config *cfg, const icw_node *nodes, int n_nodes, const char *const *in_paths,
                        const char *const *out_paths, int n, const icw_batch_opts *opts, icw_batch_stats *stats,
                        int *status)
{
    if (!cfg || n < 0 || (n > 0 && (!in_paths || !out_paths))) return ICW_EINVAL;
    icw_batch_opts o;
    memset(&o, 0, sizeof(o));
    o.device = -1;
    if (opts) o = *opts;
    return for_file_groups(
        in_paths, out_paths, n, stats, status,
        [&](int i, Job &j) { return accept_wav(in_paths[i], out_paths[i], &j.info); },
        [](int) { return 0; },
        [&](int, std::vector<Job *> &g, icw_batch_stats &st, int *sts) { return run_group(*cfg, nodes, n_nodes, g, o, st, sts); },
        (unsigned)o.reserved_ & (ICW_BATCH_MERGE_INPUTS | ICW_BATCH_MERGE_CWAVE));
}

namespace {

/* icw_transcode_files_lists, with the FIR converter (k_M > 0) on every context of real-input files */
int transcode_lists(const icw_config *cfg, const icw_node *const *nodes, const int *n_nodes, const int *bypass_list,
                    const char *const *in_paths, const char *const *out_paths, int n, int32_t k_M, double k_beta,
                    const icw_batch_opts *opts, icw_batch_stats *stats, int *status)
{
    if (!cfg || n < 0 || (n > 0 && (!in_paths || !out_paths || !nodes || !n_nodes))) return ICW_EINVAL;
    icw_batch_opts o;
    memset(&o, 0, sizeof(o));
    o.device = -1;
    if (opts) o = *opts;
    /* the group key's last part: -1 for the register-form lists, which share a context whatever
     * they are; a bus-form list groups with the files that carry the same one -- or, with
     * ICW_BATCH_MERGE_BUS, all bus-form lists share a context of their own (-2: icw_enable_stream_bus, every
     * stream its file's list).  The register-form files keep theirs: in a call forced into bus form they
     * would lose the frame-parallel K2.  Beside the FIR converter the bit does nothing: it refuses bus-form
     * lists beside others */
    const bool merge_bus = (o.reserved_ & ICW_BATCH_MERGE_BUS) && k_M == 0 && !cfg->fp_check;
    std::vector<int> form(n > 0 ? n : 1, 0);
    std::vector<int> bus_first;                     /* file index of each distinct bus-form list */
    auto same = [&](int a, int b) {
        const int ba = bypass_list ? bypass_list[a] : cfg->bypass_list, bb = bypass_list ? bypass_list[b] : cfg->bypass_list;
        return n_nodes[a] == n_nodes[b] && !ba == !bb &&
               (n_nodes[a] == 0 || !memcmp(nodes[a], nodes[b], (size_t)n_nodes[a] * sizeof(icw_node)));
    };
    return for_file_groups(
        in_paths, out_paths, n, stats, status,
        [&](int i, Job &j) {
            if (n_nodes[i] < 0 || (n_nodes[i] > 0 && !nodes[i])) return (int)ICW_EINVAL;
            form[i] = icw_graph_form(cfg, nodes[i], n_nodes[i], bypass_list ? bypass_list[i] : cfg->bypass_list);
            if (form[i] < 0) return form[i];            /* ICW_EGRAPH: the rest of the batch goes on */
            return accept_wav(in_paths[i], out_paths[i], &j.info);
        },
        [&](int i) {
            int key = -1;
            if (form[i] == 1 && merge_bus) return -2;
            if (form[i] == 1) {
                for (size_t k = 0; k < bus_first.size() && key < 0; ++k)
                    if (same(bus_first[k], i)) key = (int)k;
                if (key < 0) {
                    key = (int)bus_first.size();
                    bus_first.push_back(i);
                }
            }
            return key;
        },
        [&](int key, std::vector<Job *> &g, icw_batch_stats &st, int *sts) {
            FileLists fl;
            fl.nodes = nodes;
            fl.n_nodes = n_nodes;
            fl.bypass = bypass_list;
            fl.per_stream = key < 0;
            fl.bus = key == -2;
            fl.k_M = k_M;
            fl.k_beta = k_beta;
            return run_group(*cfg, nullptr, 0, g, o, st, sts, fl);
        },
        (unsigned)o.reserved_ & (ICW_BATCH_MERGE_INPUTS | ICW_BATCH_MERGE_CWAVE));
}

}  // namespace

/* icw_transcode_files with file i's own list (include/icw_reader.h) */
int icw_transcode_files_lists(const icw_config *cfg, const icw_node *const *nodes, const int *n_nodes,
                              const int *bypass_list, const char *const *in_paths, const char *const *out_paths, int n,
                              const icw_batch_opts *opts, icw_batch_stats *stats, int *status)
{
    return transcode_lists(cfg, nodes, n_nodes, bypass_list, in_paths, out_paths, n, 0, 0.0, opts, stats, status);
}

/* the same through the FIR converter (include/icw_reader.h); icw_set_fir_hilbert's own checks first, so a
 * bad order or window parameter opens no file */
int icw_transcode_files_fir(const icw_config *cfg, const icw_node *const *nodes, const int *n_nodes,
                            const int *bypass_list, const char *const *in_paths, const char *const *out_paths, int n,
                            int32_t k_M, double k_beta, const icw_batch_opts *opts, icw_batch_stats *stats, int *status)
{
    if (k_M < 2 || k_M > ICW_FIR_MAX_ORDER || (k_M & 1) || !(k_beta >= 0.0 && k_beta < 1e3)) return ICW_EINVAL;
    return transcode_lists(cfg, nodes, n_nodes, bypass_list, in_paths, out_paths, n, k_M, k_beta, opts, stats, status);
}

/* icw_transcode_files_lists through pools of opts->slots streams (include/icw_reader.h) */
int icw_transcode_files_pool(const icw_config *cfg, const icw_node *const *nodes, const int *n_nodes,
                             const int *bypass_list, const char *const *in_paths, const char *const *out_paths,
                             int n, const icw_pool_opts *opts, icw_pool_stats *stats, icw_meters *meters, int *status)
{
    if (!cfg || n < 0 || (n > 0 && (!in_paths || !out_paths || !nodes || !n_nodes))) return ICW_EINVAL;
    icw_pool_opts po;
    memset(&po, 0, sizeof(po));
    po.batch.device = -1;
    if (opts) po = *opts;
    if (po.slots < 0 || (po.order != ICW_POOL_AS_GIVEN && po.order != ICW_POOL_LONGEST_FIRST)) return ICW_EINVAL;
    if (cfg->fp_check) return ICW_EUNSUPPORTED;
    if (meters && n > 0) memset(meters, 0, (size_t)n * sizeof(icw_meters));
    icw_pool_stats ps;
    memset(&ps, 0, sizeof(ps));
    std::vector<int> form(n > 0 ? n : 1, 0);
    /* the kinds: real input or CWAVE (the frame of the call keeps them apart), and within each the form of the
     * list -- register (-1) or bus (-2), as ICW_BATCH_MERGE_BUS keeps them apart */
    const int rc = for_file_groups(
        in_paths, out_paths, n, &ps.batch, status,
        [&](int i, Job &j) {
            if (n_nodes[i] < 0 || (n_nodes[i] > 0 && !nodes[i])) return (int)ICW_EINVAL;
            form[i] = icw_graph_form(cfg, nodes[i], n_nodes[i], bypass_list ? bypass_list[i] : cfg->bypass_list);
            if (form[i] < 0) return form[i];            /* ICW_EGRAPH: the rest of the call goes on */
            return accept_wav(in_paths[i], out_paths[i], &j.info);
        },
        [&](int i) { return form[i] == 1 ? -2 : -1; },
        [&](int key, std::vector<Job *> &g, icw_batch_stats &st, int *sts) {
            FileLists fl;
            fl.nodes = nodes;
            fl.n_nodes = n_nodes;
            fl.bypass = bypass_list;
            fl.per_stream = true;
            fl.bus = key == -2;
            return run_pool(*cfg, g, po, fl, st, ps, meters, sts);
        },
        ICW_BATCH_MERGE_INPUTS | ICW_BATCH_MERGE_CWAVE);
    if (stats) *stats = ps;
    return rc;
}

void icw_file_job_from_config(const icw_config *cfg, const icw_node *nodes, int n_nodes, icw_file_job *job)
{
    if (!cfg || !job) return;
    memset(job, 0, sizeof(*job));
    job->nodes = nodes;
    job->n_nodes = n_nodes;
    job->bypass_list = cfg->bypass_list;
    job->render = cfg->render;
    job->need24bits = cfg->need24bits;
    job->hilbert_type = cfg->hilbert_type;
    job->iir_kahan = cfg->iir_kahan;
    job->iir_subnorm_reject = cfg->iir_subnorm_reject;
}

/* icw_transcode_files_pool with file i's own render and Hilbert converter (include/icw_reader.h) */
int icw_transcode_files_jobs(const icw_config *cfg, const icw_file_job *jobs, const char *const *in_paths,
                             const char *const *out_paths, int n, const icw_pool_opts *opts, icw_jobs_stats *stats,
                             icw_meters *meters, int *status)
{
    if (!cfg || n < 0 || (n > 0 && (!in_paths || !out_paths || !jobs))) return ICW_EINVAL;
    icw_pool_opts po;
    memset(&po, 0, sizeof(po));
    po.batch.device = -1;
    if (opts) po = *opts;
    if (po.slots < 0 || (po.order != ICW_POOL_AS_GIVEN && po.order != ICW_POOL_LONGEST_FIRST)) return ICW_EINVAL;
    if (cfg->fp_check) return ICW_EUNSUPPORTED;
    if (meters && n > 0) memset(meters, 0, (size_t)n * sizeof(icw_meters));
    icw_jobs_stats js;
    memset(&js, 0, sizeof(js));
    std::vector<const icw_node *> nodes((size_t)(n > 0 ? n : 1), nullptr);
    std::vector<int> n_nodes((size_t)(n > 0 ? n : 1), 0), bypass((size_t)(n > 0 ? n : 1), 0), form((size_t)(n > 0 ? n : 1), 0);
    std::vector<char> cwf((size_t)(n > 0 ? n : 1), 0);
    for (int i = 0; i < n; ++i) {
        nodes[(size_t)i] = jobs[i].nodes;
        n_nodes[(size_t)i] = jobs[i].n_nodes;
        bypass[(size_t)i] = jobs[i].bypass_list;
    }
    PoolJobs pj;
    pj.jobs = jobs;
    pj.timing = (po.batch.reserved_ & ICW_BATCH_TIMING) != 0;
    pj.js = &js;
    /* the kinds are the pool's -- real input or CWAVE, register form (-1) -- but a bus-form list runs in a context
     * of the files of its kind that carry its setting: key k >= 0, the k-th distinct one of them */
    std::vector<int> bus_first;
    const auto same_setting = [&](int a, int b) {
        const char one[2] = {1, 1};
        const icw_file_job two[2] = {jobs[a], jobs[b]};
        std::vector<int32_t> pos;
        return cwf[(size_t)a] == cwf[(size_t)b] && icw_pool_job_classes(two, one, 2, cwf[(size_t)a] != 0, pos, nullptr) == 1;
    };
    const int rc = for_file_groups(
        in_paths, out_paths, n, &js.pool.batch, status,
        [&](int i, Job &j) {
            if (n_nodes[(size_t)i] < 0 || (n_nodes[(size_t)i] > 0 && !nodes[(size_t)i]) || !icw_pool_job_ok(jobs[i]))
                return (int)ICW_EINVAL;
            form[(size_t)i] = icw_graph_form(cfg, nodes[(size_t)i], n_nodes[(size_t)i], bypass[(size_t)i]);
            if (form[(size_t)i] < 0) return form[(size_t)i];   /* ICW_EGRAPH: the rest of the call goes on */
            const int r = accept_wav(in_paths[i], out_paths[i], &j.info);
            cwf[(size_t)i] = r == ICW_OK && j.info.fmt >= ICW_FMT_CW_F64;
            return r;
        },
        [&](int i) {
            if (form[(size_t)i] != 1) return -1;
            for (size_t k = 0; k < bus_first.size(); ++k)
                if (same_setting(bus_first[k], i)) return (int)k;
            bus_first.push_back(i);
            return (int)bus_first.size() - 1;
        },
        [&](int key, std::vector<Job *> &g, icw_batch_stats &st, int *sts) {
            FileLists fl;
            fl.nodes = nodes.data();
            fl.n_nodes = n_nodes.data();
            fl.bypass = bypass.data();
            fl.per_stream = true;
            fl.bus = key >= 0;
            return run_pool(*cfg, g, po, fl, st, js.pool, meters, sts, pj);
        },
        ICW_BATCH_MERGE_INPUTS | ICW_BATCH_MERGE_CWAVE);
    if (stats) *stats = js;
    return rc;
}

}  /* extern "C" */
