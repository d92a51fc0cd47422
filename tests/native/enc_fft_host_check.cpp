/*
 * enc_fft_host_check.cpp -- the host side of the direct-FFT CWAVE encoder in a stand-alone program, for a
 * sanitizer build of the host sources (`make -C in_cwave_amd/csrc hostcheck-fft`; runs on a machine without a
 * GPU): every refusal of icw_encode_cwave_fft (all of them come back before a device is touched), the
 * workspace and pass queries, icw_cwave_encode_files_fft's option checks and per-file refusals, and the error
 * path of a group that finds no device (ICW_EDEVICE / ICW_ENOMEM for its files, nothing leaks).  With a GPU
 * present the last case encodes instead and the program checks the header it wrote.
 *
 *     enc_fft_host_check <scratch directory>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/icw_cwave.h"
#include "../../include/icw_reader.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static void p32(unsigned char *q, uint32_t v) { q[0] = v; q[1] = v >> 8; q[2] = v >> 16; q[3] = v >> 24; }
static void p16(unsigned char *q, uint32_t v) { q[0] = v; q[1] = v >> 8; }

/* a 16-bit stereo PCM WAV of n frames */
static bool write_wav(const std::string &path, int n)
{
    std::vector<unsigned char> b(44 + (size_t)n * 4);
    memcpy(&b[0], "RIFF", 4); p32(&b[4], 36 + n * 4); memcpy(&b[8], "WAVEfmt ", 8); p32(&b[16], 16);
    p16(&b[20], 1); p16(&b[22], 2); p32(&b[24], 48000); p32(&b[28], 48000 * 4); p16(&b[32], 4); p16(&b[34], 16);
    memcpy(&b[36], "data", 4); p32(&b[40], n * 4);
    for (int i = 0; i < 2 * n; ++i) p16(&b[44 + 2 * i], (uint32_t)(int16_t)((i * 7919) % 20000 - 10000));
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(b.data(), 1, b.size(), f) == b.size();
    return fclose(f) == 0 && ok;
}

static bool exists(const std::string &p)
{
    FILE *f = fopen(p.c_str(), "rb");
    if (f) fclose(f);
    return f != nullptr;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <scratch directory>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    std::vector<unsigned char> in(4096, 7), out(8192, 0);
    const uint64_t off[2] = {0, 0}, two[2] = {100, 100};
    uint64_t cl[2] = {99, 99};
    icw_fft_enc_opts fo = {-1, 0};

    /* icw_encode_cwave_fft: every refusal, before a device is touched */
    auto call = [&](const void *i, const uint64_t *io, const uint64_t *nf, int n, uint32_t fmt, uint32_t ch, void *o,
                    const uint64_t *oo, uint32_t cwf, unsigned flags, const icw_fft_enc_opts *op) {
        return icw_encode_cwave_fft(i, io, nf, n, fmt, ch, o, oo, cwf, cl, flags, op, nullptr);
    };
    CHECK(call(nullptr, off, two, 2, ICW_FMT_I16, 2, out.data(), off, ICW_FMT_CW_F64, 0, &fo) == ICW_EINVAL);
    CHECK(call(in.data(), nullptr, two, 2, ICW_FMT_I16, 2, out.data(), off, ICW_FMT_CW_F64, 0, &fo) == ICW_EINVAL);
    CHECK(call(in.data(), off, nullptr, 2, ICW_FMT_I16, 2, out.data(), off, ICW_FMT_CW_F64, 0, &fo) == ICW_EINVAL);
    CHECK(call(in.data(), off, two, 2, ICW_FMT_I16, 2, nullptr, off, ICW_FMT_CW_F64, 0, &fo) == ICW_EINVAL);
    CHECK(call(in.data(), off, two, 2, ICW_FMT_I16, 2, out.data(), nullptr, ICW_FMT_CW_F64, 0, &fo) == ICW_EINVAL);
    CHECK(call(in.data(), off, two, -1, ICW_FMT_I16, 2, out.data(), off, ICW_FMT_CW_F64, 0, &fo) == ICW_EINVAL);
    CHECK(call(in.data(), off, two, 2, ICW_FMT_CW_F64, 2, out.data(), off, ICW_FMT_CW_F64, 0, &fo) == ICW_EINVAL);
    CHECK(call(in.data(), off, two, 2, ICW_FMT_I16, 0, out.data(), off, ICW_FMT_CW_F64, 0, &fo) == ICW_EINVAL);
    CHECK(call(in.data(), off, two, 2, ICW_FMT_I16, 2, out.data(), off, ICW_FMT_F32, 0, &fo) == ICW_EINVAL);
    CHECK(call(in.data(), off, two, 2, ICW_FMT_I16, 2, out.data(), off, ICW_FMT_CW_F32 + 1, 0, &fo) == ICW_EINVAL);
    CHECK(call(in.data(), off, two, 2, ICW_FMT_I16, 2, out.data(), off, ICW_FMT_CW_F64, ICW_F_DEBUG_PRE, &fo) == ICW_EINVAL);
    CHECK(call(in.data(), off, two, 2, ICW_FMT_I16, 2, out.data(), off, ICW_FMT_CW_F64, ICW_F_DEVICE_PTRS | 16u, &fo) == ICW_EINVAL);
    {
        const uint64_t one[2] = {100, 1}, big[2] = {100, ((uint64_t)1 << ICW_FFT_MAX_LOG2) + 1}, both[2] = {(uint64_t)1 << 40, 1};
        CHECK(call(in.data(), off, one, 2, ICW_FMT_I16, 2, out.data(), off, ICW_FMT_CW_F64, 0, &fo) == ICW_EINVAL);
        CHECK(call(in.data(), off, big, 2, ICW_FMT_I16, 2, out.data(), off, ICW_FMT_CW_F64, 0, &fo) == ICW_EUNSUPPORTED);
        CHECK(call(in.data(), off, big, 2, ICW_FMT_I16, 2, out.data(), off, ICW_FMT_CW_F64, ICW_F_DEVICE_PTRS, &fo) == ICW_EUNSUPPORTED);
        CHECK(call(in.data(), off, both, 2, ICW_FMT_I16, 2, out.data(), off, ICW_FMT_CW_F64, 0, &fo) == ICW_EINVAL);
        icw_fft_enc_opts bad = {-1, 1};
        CHECK(call(in.data(), off, two, 2, ICW_FMT_I16, 2, out.data(), off, ICW_FMT_CW_F64, 0, &bad) == ICW_EINVAL);
        bad.max_pass_log2 = -2;
        CHECK(call(in.data(), off, two, 2, ICW_FMT_I16, 2, out.data(), off, ICW_FMT_CW_F64, 0, &bad) == ICW_EINVAL);
        CHECK(icw_encode_cwave_fft_workspace(one, 2, 2) == 0 && icw_encode_cwave_fft_workspace(big, 2, 2) == 0);
    }
    CHECK(cl[0] == 99 && cl[1] == 99);
    for (unsigned char v : out) if (v) { CHECK(!"output written by a refused call"); break; }

    /* the queries */
    CHECK(icw_encode_cwave_fft_workspace(two, 2, 2) == 2 * (16 * 128 + 40));
    CHECK(icw_encode_cwave_fft_workspace(two, 2, 0) == 0 && icw_encode_cwave_fft_workspace(nullptr, 0, 2) == 0);
    CHECK(icw_encode_cwave_fft_passes(128, 0) == 1 && icw_encode_cwave_fft_passes(128, 4) == 2 &&
          icw_encode_cwave_fft_passes(128, 3) == 3 && icw_encode_cwave_fft_passes(1 << 20, 0) == 3 &&
          icw_encode_cwave_fft_passes((uint64_t)1 << ICW_FFT_MAX_LOG2, 2) == 14);
    CHECK(icw_encode_cwave_fft_passes(1, 0) == ICW_EINVAL && icw_encode_cwave_fft_passes(5, 1) == ICW_EINVAL &&
          icw_encode_cwave_fft_passes(((uint64_t)1 << ICW_FFT_MAX_LOG2) + 1, 0) == ICW_EUNSUPPORTED);

    const std::string good = dir + "/good.wav", bad = dir + "/bad.wav", none = dir + "/none.wav", tiny = dir + "/tiny.wav";
    CHECK(write_wav(good, 300) && write_wav(tiny, 1));
    {
        FILE *f = fopen(bad.c_str(), "wb");
        CHECK(f && fwrite("RIFF\0\0\0\0WAVEjunk", 1, 16, f) == 16 && fclose(f) == 0);
    }
    const std::string o0 = dir + "/f0.cwave", o1 = dir + "/f1.cwave", o2 = dir + "/f2.cwave", o3 = dir + "/f3.cwave";
    icw_cwave_enc_fft_opts ok;
    memset(&ok, 0, sizeof(ok));
    ok.cw_format = ICW_FMT_CW_I16_F32;
    ok.device = -1;

    /* option checks: nothing runs, nothing is written */
    const char *in1[1] = {good.c_str()}, *out1[1] = {o0.c_str()};
    for (uint32_t cwf : {(uint32_t)ICW_FMT_I16, (uint32_t)ICW_FMT_CW_F32 + 1u, 0u}) {
        icw_cwave_enc_fft_opts o = ok;
        o.cw_format = cwf;
        int st = 77;
        uint64_t c1 = 77;
        CHECK(icw_cwave_encode_files_fft(in1, out1, 1, &o, nullptr, &c1, &st) == ICW_EINVAL);
        CHECK(st == 77 && c1 == 77 && !exists(o0));
    }
    CHECK(icw_cwave_encode_files_fft(in1, out1, 1, nullptr, nullptr, nullptr, nullptr) == ICW_EINVAL);
    CHECK(icw_cwave_encode_files_fft(nullptr, out1, 1, &ok, nullptr, nullptr, nullptr) == ICW_EINVAL);
    CHECK(icw_cwave_encode_files_fft(in1, nullptr, 1, &ok, nullptr, nullptr, nullptr) == ICW_EINVAL);
    CHECK(icw_cwave_encode_files_fft(in1, out1, -1, &ok, nullptr, nullptr, nullptr) == ICW_EINVAL);
    icw_batch_stats bs;
    memset(&bs, 0x55, sizeof(bs));
    CHECK(icw_cwave_encode_files_fft(nullptr, nullptr, 0, &ok, &bs, nullptr, nullptr) == ICW_OK);
    CHECK(bs.n_files == 0 && bs.n_groups == 0 && bs.frames_in == 0 && bs.frames_out == 0);

    /* per-file refusals (no device call: the files never reach a group) */
    {
        const char *ins[4] = {bad.c_str(), none.c_str(), nullptr, tiny.c_str()};
        const char *outs[4] = {o0.c_str(), o1.c_str(), o2.c_str(), o3.c_str()};
        int st[4] = {0, 0, 0, 0};
        uint64_t c4[4] = {9, 9, 9, 9};
        CHECK(icw_cwave_encode_files_fft(ins, outs, 4, &ok, &bs, c4, st) == ICW_EINVAL);
        CHECK(st[0] == ICW_EINVAL && st[1] == ICW_EINVAL && st[2] == ICW_EINVAL && st[3] == ICW_EINVAL);
        CHECK(c4[0] == 0 && c4[1] == 0 && c4[2] == 0 && c4[3] == 0 && bs.n_files == 0 && bs.n_groups == 0);
        CHECK(!exists(o0) && !exists(o1) && !exists(o2) && !exists(o3));
    }

    /* a good file beside a bad one: without a device the group fails and the file gets its error; with one,
     * the file is encoded and its header is the V2 header of the direct-FFT converter (k_M -1) */
    {
        const char *ins[2] = {good.c_str(), bad.c_str()}, *outs[2] = {o0.c_str(), o1.c_str()};
        int st[2] = {0, 0};
        uint64_t c2[2] = {9, 9};
        const int rc = icw_cwave_encode_files_fft(ins, outs, 2, &ok, &bs, c2, st);
        CHECK(st[1] == ICW_EINVAL && !exists(o1) && bs.n_groups == 1);
        if (st[0] == ICW_OK) {
            CHECK(rc == ICW_EINVAL && bs.n_files == 1 && bs.frames_out == 300);
            icw_wav_info wi;
            CHECK(icw_wav_parse_file(o0.c_str(), &wi) == ICW_OK && wi.fmt == ICW_FMT_CW_I16_F32 && wi.n_samples == 300 &&
                  wi.channels == 2 && wi.data_offset == 48 && wi.frame_bytes == 12);
            unsigned char h[48];
            FILE *f = fopen(o0.c_str(), "rb");
            CHECK(f && fread(h, 1, 48, f) == 48);
            if (f) fclose(f);
            static const unsigned char zero8[8] = {0}, m1[4] = {0xff, 0xff, 0xff, 0xff};
            CHECK(!memcmp(h, "cPLXwAVE", 8) && h[8] == 48 && h[12] == 2 && !memcmp(h + 32, m1, 4) && !memcmp(h + 40, zero8, 8));
            printf("device present: encoded %s\n", o0.c_str());
        } else {
            CHECK(rc != ICW_OK && (st[0] == ICW_EDEVICE || st[0] == ICW_ENOMEM) && bs.n_files == 0);
            printf("no device: the group's error path ran (status %d)\n", st[0]);
        }
    }
    printf(fails ? "%d check(s) failed\n" : "enc_fft_host_check ok\n", fails);
    return fails ? 1 : 0;
}
