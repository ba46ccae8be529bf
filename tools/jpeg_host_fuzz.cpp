// The host entropy stage of the JPEG decoder (imagenet-models_amd/csrc/jpeg_host.h) alone, for a build under the host sanitizers
// (`make -C imagenet-models_amd/csrc jpeg_host_fuzz`: -fsanitize=address,undefined): for every file given, every prefix length and
// 2,000 seeded single-byte mutations go through probe + entropy_decode into heap buffers of EXACTLY the size the probe reported (the
// input is copied into an exact-size heap block too), so that one byte read or written outside them is a sanitizer report.  The
// files are the fixture's: `python tools/gen_golden_jpeg.py --dump DIR`, then `jpeg_host_fuzz DIR/*.jpg`.  Exit status 0: every call
// returned OK, UNSUPPORTED or CORRUPT and the intact file decoded as OK or UNSUPPORTED.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../imagenet-models_amd/csrc/jpeg_host.h"

static int run(const std::vector<uint8_t>& data, size_t n, long counts[3]) {
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(in, data.data(), n);
    int64_t info[ga_jpeg::INFO_LEN];
    int rc = ga_jpeg::probe(in, n, info);
    const size_t ncoef = rc == ga_jpeg::OK ? (size_t)info[5] : 0;
    int16_t* coef = (int16_t*)malloc(ncoef ? ncoef * sizeof(int16_t) : 1);
    uint16_t* qt = (uint16_t*)malloc(192 * sizeof(uint16_t));
    const int rc2 = ga_jpeg::entropy_decode(in, n, coef, ncoef, qt);
    if (rc != ga_jpeg::OK && rc2 != rc) rc = -1;          // the two parse the same header
    if (rc == ga_jpeg::OK) rc = rc2;
    free(qt);
    free(coef);
    free(in);
    if (rc < 0 || rc > 2) return -1;
    ++counts[rc];
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s FILE.jpg ...\n", argv[0]);
        return 2;
    }
    long total[3] = {0, 0, 0};
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> data;
        uint8_t chunk[4096];
        for (size_t k; (k = fread(chunk, 1, sizeof(chunk), f)) > 0;) data.insert(data.end(), chunk, chunk + k);
        fclose(f);
        long counts[3] = {0, 0, 0};
        const int whole = run(data, data.size(), counts);
        if (whole != ga_jpeg::OK && whole != ga_jpeg::UNSUPPORTED) {
            fprintf(stderr, "%s: the intact file gives %d\n", argv[a], whole);
            return 1;
        }
        for (size_t n = 0; n < data.size(); ++n)
            if (run(data, n, counts) < 0) return 1;
        uint64_t state = 0x9E3779B97F4A7C15ull ^ (uint64_t)a;          // xorshift64*: the same mutations on every machine
        for (int m = 0; m < 2000 && !data.empty(); ++m) {
            state ^= state >> 12; state ^= state << 25; state ^= state >> 27;
            const uint64_t r = state * 0x2545F4914F6CDD1Dull;
            std::vector<uint8_t> mut(data);
            mut[(size_t)((r >> 16) % mut.size())] = (uint8_t)(r & 255);
            if (run(mut, mut.size(), counts) < 0) return 1;
        }
        for (int k = 0; k < 3; ++k) total[k] += counts[k];
    }
    printf("%d files: %ld calls OK, %ld UNSUPPORTED, %ld CORRUPT\n", argc - 1, total[0], total[1], total[2]);
    return 0;
}
