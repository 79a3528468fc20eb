// Stand-alone check of the HOST half of the loose-image-file path under AddressSanitizer and UndefinedBehaviorSanitizer: the JPEG
// entry points for frames of any size (gx_jpeg_info_any, gx_jpeg_entropy_decode_any: gx_jpeg.cpp) and the PNG chunk walk and
// inflate (gx_png_info, gx_png_inflate: gx_png.cpp).  Host code only: no HIP call is made, no GPU is needed and none is used.
// It is compiled together with those two sources (tools/README.md has the command), never loaded into Python.
//
//   imagefile_host_check DIR     DIR holds the streams tests/golden/make_golden_imagefile.py --dump DIR writes (*.jpg, *.png)
//
// Per stream: the whole stream must decode (or, for refuse_*, be refused with GX_EDATA); then EVERY prefix of the small streams
// (every 97th length of the others) and 2000 seeded single-byte corruptions run through the same calls.  Input and output live in
// exact-size heap blocks, so a read or write one byte out of bounds is a sanitizer report.  Every call must return GX_OK,
// GX_EDATA or -- a corrupted header may ask for more room than the buffer has -- GX_EINVAL.  Exit status 0: no bad return code;
// a sanitizer report ends the program with its own status.
#include <dirent.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/genesis_hip.h"

// the library's error sink (gx_api.cpp there): the message is kept for the report
static char g_error[512];
void gx_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

namespace {

struct Lcg {      // seeded, the same on every machine
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
};

std::vector<unsigned char> read_file(const std::string& path) {
    std::vector<unsigned char> v;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return v;
    unsigned char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int g_bad = 0;
long g_calls = 0;

bool known(int rc) { return rc == GX_OK || rc == GX_EDATA || rc == GX_EINVAL; }

// One run over data[0..n): the input in its own exact-size block, the outputs exact-size for the GOOD stream's geometry.
int run_jpeg(const unsigned char* data, size_t n, size_t coef_values) {
    unsigned char* in = (unsigned char*)malloc(n ? n : 1);
    memcpy(in, data, n);
    short* coef = (short*)malloc(coef_values * sizeof(short));
    unsigned short* qtab = (unsigned short*)malloc(192 * sizeof(unsigned short));
    int info[8];
    const int rc0 = gx_jpeg_info_any(in, n, info);
    const int rc = gx_jpeg_entropy_decode_any(in, n, coef, coef_values, qtab, info);
    g_calls += 2;
    if (!known(rc0) || !known(rc) || rc0 == GX_EINVAL) {
        fprintf(stderr, "jpeg: return codes %d, %d for %zu bytes\n", rc0, rc, n);
        ++g_bad;
    }
    free(in);
    free(coef);
    free(qtab);
    return rc;
}

int run_png(const unsigned char* data, size_t n, size_t frame_bytes) {
    unsigned char* in = (unsigned char*)malloc(n ? n : 1);
    memcpy(in, data, n);
    unsigned char* dst = (unsigned char*)malloc(frame_bytes ? frame_bytes : 1);
    int info[8];
    const int rc0 = gx_png_info(in, n, info);
    const int rc = gx_png_inflate(in, n, dst, frame_bytes, info);
    g_calls += 2;
    if (!known(rc0) || !known(rc)) {
        fprintf(stderr, "png: return codes %d, %d for %zu bytes\n", rc0, rc, n);
        ++g_bad;
    }
    free(in);
    free(dst);
    return rc;
}

void sweep(const std::string& name, const std::vector<unsigned char>& s) {
    const bool png = s.size() >= 4 && s[1] == 'P' && s[2] == 'N' && s[3] == 'G';
    const bool refused = name.compare(0, 7, "refuse_") == 0;
    int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int rc_info = png ? gx_png_info(s.data(), s.size(), info) : gx_jpeg_info_any(s.data(), s.size(), info);
    if (refused ? rc_info != GX_EDATA : rc_info != GX_OK) {
        fprintf(stderr, "%s: the header gives %d (%s)\n", name.c_str(), rc_info, g_error);
        ++g_bad;
        return;
    }
    const size_t room = refused ? 4096 : (png ? (size_t)info[7] : ((size_t)info[4] + info[5] + info[6]) * 64);
    auto run = [&](const unsigned char* d, size_t n) { return png ? run_png(d, n, room) : run_jpeg(d, n, room); };
    const int whole = run(s.data(), s.size());
    if (refused ? whole != GX_EDATA : whole != GX_OK) {
        fprintf(stderr, "%s: the whole stream gives %d (%s)\n", name.c_str(), whole, g_error);
        ++g_bad;
    }
    const size_t stride = s.size() <= 4096 ? 1 : 97;
    for (size_t n = 0; n < s.size(); n += stride) run(s.data(), n);
    Lcg rng = {0x9e3779b97f4a7c15ull ^ s.size()};
    std::vector<unsigned char> bad(s);
    const int trials = s.size() <= 65536 ? 2000 : 300;
    for (int i = 0; i < trials; ++i) {
        const size_t at = rng.next() % s.size();
        const unsigned char keep = bad[at];
        bad[at] = (unsigned char)rng.next();
        run(bad.data(), bad.size());
        bad[at] = keep;
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s DIR   (the folder tests/golden/make_golden_imagefile.py --dump DIR writes)\n", argv[0]);
        return 2;
    }
    DIR* dir = opendir(argv[1]);
    if (!dir) {
        fprintf(stderr, "%s: cannot open the folder\n", argv[1]);
        return 2;
    }
    std::vector<std::string> names;
    while (dirent* e = readdir(dir)) {
        const std::string n = e->d_name;
        if (n.size() > 4 && (n.substr(n.size() - 4) == ".jpg" || n.substr(n.size() - 4) == ".png")) names.push_back(n);
    }
    closedir(dir);
    if (names.empty()) {
        fprintf(stderr, "%s: no streams\n", argv[1]);
        return 2;
    }
    for (const std::string& n : names) {
        const std::vector<unsigned char> s = read_file(std::string(argv[1]) + "/" + n);
        if (s.empty()) {
            fprintf(stderr, "%s: cannot be read\n", n.c_str());
            ++g_bad;
            continue;
        }
        sweep(n, s);
    }
    printf("imagefile_host_check: %zu streams, %ld calls, %d bad return codes\n", names.size(), g_calls, g_bad);
    return g_bad ? 1 : 0;
}
