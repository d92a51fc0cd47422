/*
 * enc_iir_host_check.cpp -- the host side of the IIR-Hilbert CWAVE encoder in a stand-alone program, for a
 * sanitizer build of the host sources (`make -C in_cwave_amd/csrc hostcheck`; runs on a machine without a GPU):
 * the argument-check front of icw_encode_cwave_iir, icw_cwave_encode_files_iir's option checks, its per-file
 * refusals, and the error path of a group whose context cannot be created (no device: ICW_EDEVICE, every
 * file of the group gets it, nothing leaks).  With a GPU present the last case encodes instead and the
 * program checks the header it wrote.
 *
 *     enc_iir_host_check <scratch directory>
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
    unsigned char buf[256] = {0};

    /* icw_encode_cwave_iir: refused before the context is touched */
    CHECK(icw_encode_cwave_iir(nullptr, 0, 1, buf, 64, buf + 64, 64, 4, ICW_FMT_CW_F64, 0, nullptr) == ICW_EINVAL);
    CHECK(icw_encode_cwave_iir(nullptr, 0, 1, buf, 64, buf + 64, 64, 4, ICW_FMT_CW_F64, ICW_F_DEVICE_PTRS, nullptr) == ICW_EINVAL);
    CHECK(icw_encode_clipped(nullptr, 0, 0, nullptr) == ICW_EINVAL);
    CHECK(icw_cwave_frame_bytes(ICW_FMT_CW_I16_F32, 1) == 6 && icw_cwave_frame_bytes(ICW_FMT_CW_F64, 2) == 32);

    const std::string good = dir + "/good.wav", bad = dir + "/bad.wav", none = dir + "/none.wav";
    CHECK(write_wav(good, 300));
    {
        FILE *f = fopen(bad.c_str(), "wb");
        CHECK(f && fwrite("RIFF\0\0\0\0WAVEjunk", 1, 16, f) == 16 && fclose(f) == 0);
    }
    const std::string o0 = dir + "/o0.cwave", o1 = dir + "/o1.cwave", o2 = dir + "/o2.cwave";

    icw_cwave_enc_iir_opts ok;
    memset(&ok, 0, sizeof(ok));
    ok.hilbert_type = 1;
    ok.iir_kahan = ok.iir_subnorm_reject = 1;
    ok.cw_format = ICW_FMT_CW_I16_F32;
    ok.device = -1;

    /* option checks: nothing runs, nothing is written */
    const char *in1[1] = {good.c_str()}, *out1[1] = {o0.c_str()};
    struct { int field; int64_t v; } bads[] = {{0, 6}, {0, 0xFFFFFFFFll}, {1, 2}, {1, -1}, {2, 2}, {3, ICW_FMT_I16},
                                                {3, ICW_FMT_CW_F32 + 1}, {4, -1}};
    for (const auto &b : bads) {
        icw_cwave_enc_iir_opts o = ok;
        switch (b.field) {
        case 0: o.hilbert_type = (uint32_t)b.v; break;
        case 1: o.iir_kahan = (int32_t)b.v; break;
        case 2: o.iir_subnorm_reject = (int32_t)b.v; break;
        case 3: o.cw_format = (uint32_t)b.v; break;
        default: o.block_frames = (int32_t)b.v; break;
        }
        int st = 77;
        uint64_t cl = 77;
        CHECK(icw_cwave_encode_files_iir(in1, out1, 1, &o, nullptr, &cl, &st) == ICW_EINVAL);
        CHECK(st == 77 && cl == 77 && !exists(o0));
    }
    CHECK(icw_cwave_encode_files_iir(in1, out1, 1, nullptr, nullptr, nullptr, nullptr) == ICW_EINVAL);
    CHECK(icw_cwave_encode_files_iir(nullptr, out1, 1, &ok, nullptr, nullptr, nullptr) == ICW_EINVAL);
    CHECK(icw_cwave_encode_files_iir(in1, nullptr, 1, &ok, nullptr, nullptr, nullptr) == ICW_EINVAL);
    CHECK(icw_cwave_encode_files_iir(in1, out1, -1, &ok, nullptr, nullptr, nullptr) == ICW_EINVAL);
    icw_batch_stats bs;
    memset(&bs, 0x55, sizeof(bs));
    CHECK(icw_cwave_encode_files_iir(nullptr, nullptr, 0, &ok, &bs, nullptr, nullptr) == ICW_OK);
    CHECK(bs.n_files == 0 && bs.n_groups == 0 && bs.frames_in == 0 && bs.frames_out == 0);

    /* per-file refusals (no device call: the files never reach a group) */
    {
        const char *ins[3] = {bad.c_str(), none.c_str(), nullptr}, *outs[3] = {o0.c_str(), o1.c_str(), o2.c_str()};
        int st[3] = {0, 0, 0};
        uint64_t cl[3] = {9, 9, 9};
        CHECK(icw_cwave_encode_files_iir(ins, outs, 3, &ok, &bs, cl, st) == ICW_EINVAL);
        CHECK(st[0] == ICW_EINVAL && st[1] == ICW_EINVAL && st[2] == ICW_EINVAL);
        CHECK(cl[0] == 0 && cl[1] == 0 && cl[2] == 0 && bs.n_files == 0 && bs.n_groups == 0);
        CHECK(!exists(o0) && !exists(o1) && !exists(o2));
    }

    /* a good file beside a bad one: without a device the group's context fails and the file gets its error;
     * with one, the file is encoded and its header is the V2 header of an unknown converter (k_M 0) */
    {
        const char *ins[2] = {good.c_str(), bad.c_str()}, *outs[2] = {o0.c_str(), o1.c_str()};
        int st[2] = {0, 0};
        uint64_t cl[2] = {9, 9};
        const int rc = icw_cwave_encode_files_iir(ins, outs, 2, &ok, &bs, cl, st);
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
            static const unsigned char zero8[8] = {0};
            CHECK(!memcmp(h, "cPLXwAVE", 8) && h[8] == 48 && h[12] == 2 && !memcmp(h + 32, zero8, 4) && !memcmp(h + 40, zero8, 8));
            printf("device present: encoded %s\n", o0.c_str());
        } else {
            CHECK(rc != ICW_OK && (st[0] == ICW_EDEVICE || st[0] == ICW_ENOMEM) && bs.n_files == 0);
            printf("no device: the group's error path ran (status %d)\n", st[0]);
        }
    }
    printf(fails ? "%d check(s) failed\n" : "enc_iir_host_check ok\n", fails);
    return fails ? 1 : 0;
}
