// Stand-alone check of the host entropy stage (csrc/jpeg_host.h) for the host sanitizers: no HIP, no Python.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_host_check.cpp -o jpeg_host_check
//   ./jpeg_host_check file.jpg [more.jpg ...]
//
// Each file, and 2000 deterministic mutations of it (byte flips and truncations from a fixed LCG), goes through probe() and
// entropy_decode() with a coefficient buffer of exactly the probed size.  The contract checked on every stream:
//   - the status is HS_OK, HS_JPEG_ERR_CORRUPT or one of the refusals, and both functions agree on everything but "corrupt"
//     (only the decoder reads the entropy-coded bytes);
//   - a refusal writes nothing; a buffer one byte short is HS_ERR_ARG and writes nothing;
//   - the guard words after coef_bytes and after the three tables are never written (the sanitizer sees what lies beyond);
//   - decoding the same stream twice gives the same status and the same bytes.
// The unmutated files must decode (HS_OK) or be refused, never be corrupt.  Exit status 0 when all of it holds.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../multimodal-diagnosis-ham-spine_amd/hamspine/csrc/jpeg_host.h"

static const int kMutations = 2000;
static const int16_t kGuard = 0x5a5a;
static const int kGuardWords = 64;

static bool is_refusal(int st) { return st >= HS_JPEG_ERR_PROGRESSIVE && st <= HS_JPEG_ERR_TOO_LARGE; }

static int fail(const char* what, const char* file, int mutation, int st) {
    fprintf(stderr, "jpeg_host_check: %s (%s, mutation %d, status %d)\n", what, file, mutation, st);
    return 1;
}

// 0 when the stream behaves within the contract; *status_out is the decoder's status
static int check_stream(const std::vector<uint8_t>& s, const char* file, int mutation, int* status_out) {
    // a copy sized exactly, so that the sanitizer catches a read past the end
    uint8_t* data = (uint8_t*)malloc(s.size() ? s.size() : 1);
    if (!s.empty()) memcpy(data, s.data(), s.size());
    hs_jpeg_info probe_info, info;
    memset(&probe_info, 0, sizeof probe_info);
    const int pst = hs_jpeg::probe(data, (int64_t)s.size(), &probe_info);
    int rc = 0, st = pst;
    if (pst != HS_OK && pst != HS_JPEG_ERR_CORRUPT && !is_refusal(pst)) rc = fail("probe: status outside the contract", file, mutation, pst);
    if (!rc && pst == HS_OK) {
        if (probe_info.coef_bytes <= 0 || probe_info.coef_bytes % 128 || probe_info.width < 1 || probe_info.height < 1 ||
            (probe_info.components != 1 && probe_info.components != 3))
            rc = fail("probe: impossible geometry", file, mutation, pst);
        // a probed frame cannot ask for more than 512 bytes of coefficients per byte of scan (2 bits per block at least)
        if (!rc && probe_info.coef_bytes > 512 * (int64_t)s.size()) rc = fail("probe: a frame its scan cannot hold", file, mutation, pst);
        if (!rc) {
            const size_t words = (size_t)probe_info.coef_bytes / 2;
            std::vector<int16_t> coef(words + kGuardWords, kGuard), again(words + kGuardWords, kGuard);
            std::vector<uint16_t> qtab(3 * 64 + kGuardWords, (uint16_t)kGuard), qagain(3 * 64 + kGuardWords, (uint16_t)kGuard);
            if (hs_jpeg::entropy_decode(data, (int64_t)s.size(), coef.data(), probe_info.coef_bytes - 1, qtab.data(), &info) != HS_ERR_ARG)
                rc = fail("a short buffer was not refused", file, mutation, 0);
            for (size_t i = 0; i < coef.size() && !rc; ++i)
                if (coef[i] != kGuard) rc = fail("a short buffer was written", file, mutation, 0);
            st = hs_jpeg::entropy_decode(data, (int64_t)s.size(), coef.data(), probe_info.coef_bytes, qtab.data(), &info);
            const int st2 = hs_jpeg::entropy_decode(data, (int64_t)s.size(), again.data(), probe_info.coef_bytes, qagain.data(), &info);
            if (!rc && st != HS_OK && st != HS_JPEG_ERR_CORRUPT) rc = fail("decode: status outside the contract after a good probe", file, mutation, st);
            if (!rc && (st != st2 || coef != again || qtab != qagain)) rc = fail("decode: not repeatable", file, mutation, st);
            for (int i = 0; i < kGuardWords && !rc; ++i)
                if (coef[words + i] != kGuard || qtab[3 * 64 + i] != (uint16_t)kGuard) rc = fail("guard words written", file, mutation, st);
            if (!rc && st == HS_OK && memcmp(&info, &probe_info, sizeof info) != 0) rc = fail("probe and decode disagree on the geometry", file, mutation, st);
        }
    } else if (!rc) {
        int16_t coef[kGuardWords];
        uint16_t qtab[3 * 64];
        for (int i = 0; i < kGuardWords; ++i) coef[i] = kGuard;
        for (int i = 0; i < 3 * 64; ++i) qtab[i] = (uint16_t)kGuard;
        st = hs_jpeg::entropy_decode(data, (int64_t)s.size(), coef, (int64_t)1 << 40, qtab, &info);
        if (st != pst) rc = fail("probe and decode disagree on a stream neither accepts", file, mutation, st);
        for (int i = 0; i < kGuardWords && !rc; ++i)
            if (coef[i] != kGuard) rc = fail("a refused stream was written", file, mutation, st);
        for (int i = 0; i < 3 * 64 && !rc; ++i)
            if (qtab[i] != (uint16_t)kGuard) rc = fail("a refused stream's tables were written", file, mutation, st);
    }
    free(data);
    *status_out = st;
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s file.jpg [more.jpg ...]\n", argv[0]);
        return 2;
    }
    long long counts[3] = {0, 0, 0};   // ok, corrupt, refused
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) return fail("cannot open", argv[a], -1, 0);
        std::vector<uint8_t> orig;
        uint8_t chunk[4096];
        size_t got;
        while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) orig.insert(orig.end(), chunk, chunk + got);
        fclose(f);
        int st = 0;
        if (check_stream(orig, argv[a], -1, &st)) return 1;
        if (st == HS_JPEG_ERR_CORRUPT) return fail("the unmutated file is corrupt", argv[a], -1, st);
        uint32_t lcg = 0x2545f491u;
        auto next = [&]() {
            lcg = lcg * 1664525u + 1013904223u;
            return lcg >> 8;
        };
        for (int m = 0; m < kMutations; ++m) {
            std::vector<uint8_t> s = orig;
            const uint32_t kind = next() % 4;
            if (kind == 0 && !s.empty()) {
                s.resize(next() % s.size());                                   // truncation
            } else {
                const int flips = 1 + (int)(next() % (kind == 1 ? 1 : 4));      // one flip, or up to four
                for (int i = 0; i < flips && !s.empty(); ++i) s[next() % s.size()] ^= (uint8_t)(1u << (next() % 8));
                if (kind == 3 && !s.empty()) s[next() % s.size()] = (uint8_t)next();   // and a whole byte replaced
            }
            if (check_stream(s, argv[a], m, &st)) return 1;
            ++counts[st == HS_OK ? 0 : st == HS_JPEG_ERR_CORRUPT ? 1 : 2];
        }
    }
    printf("jpeg_host_check: %d files, %d mutations each: %lld decoded, %lld corrupt, %lld refused\n", argc - 1, kMutations, counts[0],
           counts[1], counts[2]);
    return 0;
}
