// Host half of the PNG decoder (genesis_amd/png.py): ShapeStacks and Sketchy store one PNG file per frame
// (datasets/shapestacks_config.py:141, datasets/sketchy_config.py:91: Image.open).  The serial part of decoding -- the
// chunk walk, the checksums and zlib's inflate -- runs here; everything that touches a pixel (undoing the scanline
// filters first of all) runs in gx_png.hip.  Plain host functions, no HIP calls: they work without a GPU.
//   accepted  8-bit samples, not interlaced, colour type 0 (grey, C = 1), 2 (RGB, C = 3) or 6 (RGBA, C = 4), any number of
//             CONSECUTIVE IDAT chunks (empty ones included); ancillary chunks and a suggested palette (PLTE) are skipped
//   output    the inflated IDAT data as it is stored: per row one filter byte and W * C FILTERED bytes
// Inflate and CRC-32 are zlib's (uncompress, crc32), resolved from libz.so.1 at first use, so the library has no link-time
// dependency on it.  Every length is checked against the stream and the output capacity before it is used: no input
// makes these functions read or write out of bounds.
#include "gx_common.h"

#include <dlfcn.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

namespace {

constexpr int kMaxDim = kGxPngMaxDim;   // the device kernel's frame limit (gx_common.h)

struct Zlib {
    void* handle;
    int (*uncompress)(unsigned char* dest, unsigned long* dest_len, const unsigned char* source, unsigned long source_len);
    unsigned long (*crc32)(unsigned long crc, const unsigned char* buf, unsigned int len);
    char error[256];
};
Zlib g_zlib = {};
std::once_flag g_zlib_once;

int fail(const char* what) {
    gx_set_error("gx_png: %s", what);
    return GX_EDATA;
}

void resolve_zlib() {
    const char* names[] = {"libz.so.1", "libz.so"};
    void* h = nullptr;
    for (const char* n : names) {
        h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (h) break;
    }
    if (!h) {
        const char* e = dlerror();
        snprintf(g_zlib.error, sizeof(g_zlib.error), "libz.so.1 not found (zlib inflates the IDAT data): %s", e ? e : "");
        return;
    }
    *(void**)(&g_zlib.uncompress) = dlsym(h, "uncompress");
    *(void**)(&g_zlib.crc32) = dlsym(h, "crc32");
    if (!g_zlib.uncompress || !g_zlib.crc32) {
        snprintf(g_zlib.error, sizeof(g_zlib.error), "uncompress / crc32 missing from libz.so.1");
        return;
    }
    g_zlib.handle = h;
}

int need_zlib() {
    std::call_once(g_zlib_once, resolve_zlib);
    if (!g_zlib.handle) {
        gx_set_error("gx_png: %s", g_zlib.error);
        return GX_EINVAL;
    }
    return GX_OK;
}

inline size_t be32(const unsigned char* p) { return ((size_t)p[0] << 24) | ((size_t)p[1] << 16) | ((size_t)p[2] << 8) | (size_t)p[3]; }

const unsigned char kSignature[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};

// The chunk at pos: its data [*data, *data + *len) and type; pos moves past its CRC, which is verified.  GX_EDATA when the
// chunk runs past the stream or its checksum differs.
int next_chunk(const unsigned char* p, size_t n, size_t* pos, char type[5], size_t* data, size_t* len) {
    if (n - *pos < 12) return fail("the stream ends early (inside a chunk header)");
    const size_t l = be32(p + *pos);
    memcpy(type, p + *pos + 4, 4);
    type[4] = 0;
    for (int i = 0; i < 4; ++i)
        if (!((type[i] >= 'A' && type[i] <= 'Z') || (type[i] >= 'a' && type[i] <= 'z'))) return fail("a chunk type that is not four letters");
    if (l > 0x7fffffffu || l > n - *pos - 12) {
        gx_set_error("gx_png: the stream ends early (inside the %s chunk)", type);
        return GX_EDATA;
    }
    const unsigned long want = (unsigned long)be32(p + *pos + 8 + l);
    const unsigned long got = g_zlib.crc32(0ul, p + *pos + 4, (unsigned int)(l + 4));
    if (want != got) {
        gx_set_error("gx_png: CRC mismatch in the %s chunk (stored %08lx, computed %08lx)", type, want, got);
        return GX_EDATA;
    }
    *data = *pos + 8;
    *len = l;
    *pos += 12 + l;
    return GX_OK;
}

// Signature and IHDR -> info[8]; *pos is left behind IHDR.
int parse_header(const unsigned char* p, size_t n, size_t* pos, int* info) {
    if (n < 8 || memcmp(p, kSignature, 8) != 0) return fail("not a PNG stream (bad signature)");
    *pos = 8;
    char type[5];
    size_t at, len;
    const int rc = next_chunk(p, n, pos, type, &at, &len);
    if (rc != GX_OK) return rc;
    if (strcmp(type, "IHDR") != 0 || len != 13) return fail("missing IHDR (the first chunk must be a 13-byte IHDR)");
    const size_t w = be32(p + at), h = be32(p + at + 4);
    const int depth = p[at + 8], colour = p[at + 9], compression = p[at + 10], filter = p[at + 11], interlace = p[at + 12];
    if (colour == 3) return fail("palette images (colour type 3) are not supported");
    if (colour == 4) return fail("grey+alpha images (colour type 4) are not supported");
    if (colour != 0 && colour != 2 && colour != 6) return fail("bad colour type");
    if (depth == 16) return fail("16-bit samples are not supported");
    if (depth == 1 || depth == 2 || depth == 4) return fail("samples under 8 bits are not supported");
    if (depth != 8) return fail("bad bit depth");
    if (compression != 0 || filter != 0) return fail("bad compression or filter method");
    if (interlace == 1) return fail("Adam7 interlacing is not supported");
    if (interlace != 0) return fail("bad interlace method");
    if (w == 0 || h == 0) return fail("a frame without pixels");
    if (w > (size_t)kMaxDim || h > (size_t)kMaxDim) {
        gx_set_error("gx_png: a %zu x %zu frame is larger than the %d x %d the kernel takes", w, h, kMaxDim, kMaxDim);
        return GX_EDATA;
    }
    const int C = colour == 0 ? 1 : (colour == 2 ? 3 : 4);
    info[0] = (int)w;
    info[1] = (int)h;
    info[2] = C;
    info[3] = C;                                   // bytes per pixel: 8-bit samples
    info[4] = colour;
    info[5] = depth;
    info[6] = interlace;
    info[7] = (int)(h * (1 + w * (size_t)C));      // at most 4096 * (1 + 16384): fits
    return GX_OK;
}

}  // namespace

extern "C" {

int gx_png_info(const unsigned char* data, size_t len, int* info) {
    GX_CHECK_ARG(data && info, "gx_png_info: null pointer");
    const int rc = need_zlib();
    if (rc != GX_OK) return rc;
    size_t pos;
    return parse_header(data, len, &pos, info);
}

int gx_png_inflate(const unsigned char* data, size_t len, unsigned char* dst, size_t dst_capacity, int* info) {
    GX_CHECK_ARG(data && dst && info, "gx_png_inflate: null pointer");
    int rc = need_zlib();
    if (rc != GX_OK) return rc;
    size_t pos;
    rc = parse_header(data, len, &pos, info);
    if (rc != GX_OK) return rc;
    const size_t expected = (size_t)info[7];
    GX_CHECK_ARG(dst_capacity >= expected, "gx_png_inflate: the frame inflates to %zu bytes, dst holds %zu", expected, dst_capacity);

    // first pass: every chunk's checksum, the IDAT total, IEND
    size_t idat_total = 0, idat_chunks = 0, first_at = 0, first_len = 0;
    bool have_iend = false, idat_run_over = false;
    const size_t body = pos;
    while (pos < len) {
        char type[5];
        size_t at, l;
        rc = next_chunk(data, len, &pos, type, &at, &l);
        if (rc != GX_OK) return rc;
        const bool idat = strcmp(type, "IDAT") == 0;
        if (!idat && idat_chunks) idat_run_over = true;          // the run of IDAT chunks has ended: the PNG specification wants them consecutive
        if (idat) {
            if (idat_run_over) return fail("IDAT chunks that are not consecutive (another chunk between them)");
            if (idat_chunks == 0 || first_len == 0) { first_at = at; first_len = l; }
            ++idat_chunks;
            idat_total += l;
        } else if (strcmp(type, "IEND") == 0) {
            have_iend = true;
            break;
        } else if (strcmp(type, "IHDR") == 0) {
            return fail("a second IHDR");
        } else if (!(type[0] & 0x20) && strcmp(type, "PLTE") != 0) {
            gx_set_error("gx_png: unknown critical chunk %s", type);
            return GX_EDATA;
        }
    }
    if (!have_iend) return fail("missing IEND (the stream ends early)");
    if (idat_chunks == 0) return fail("missing IDAT");

    // the zlib stream: in place when one chunk holds all of it, else the payloads concatenated
    const unsigned char* z = data + first_at;
    unsigned char* joined = nullptr;
    if (idat_total != first_len) {
        joined = (unsigned char*)malloc(idat_total);
        if (!joined) {
            gx_set_error("gx_png_inflate: out of memory (%zu bytes of IDAT data)", idat_total);
            return GX_EINVAL;
        }
        size_t fill = 0;
        pos = body;
        while (pos < len) {                        // the same walk: lengths were checked above
            const size_t l = be32(data + pos);
            const bool idat = memcmp(data + pos + 4, "IDAT", 4) == 0;
            if (memcmp(data + pos + 4, "IEND", 4) == 0) break;
            if (idat && fill + l <= idat_total) {
                memcpy(joined + fill, data + pos + 8, l);
                fill += l;
            }
            pos += 12 + l;
        }
        z = joined;
    }
    unsigned long out_len = (unsigned long)expected;
    const int zrc = g_zlib.uncompress(dst, &out_len, z, (unsigned long)idat_total);
    free(joined);
    if (zrc == -5) {                               // Z_BUF_ERROR
        gx_set_error("gx_png: the IDAT data does not inflate to the expected %zu bytes (it is longer, or its zlib stream ends early)", expected);
        return GX_EDATA;
    }
    if (zrc != 0) {
        gx_set_error("gx_png: the IDAT data is not a valid zlib stream (zlib error %d)", zrc);
        return GX_EDATA;
    }
    if ((size_t)out_len != expected) {
        gx_set_error("gx_png: the IDAT data inflates to %lu bytes, not the expected %zu", out_len, expected);
        return GX_EDATA;
    }
    const size_t stride = 1 + (size_t)info[0] * info[2];
    for (int r = 0; r < info[1]; ++r)
        if (dst[r * stride] > 4) {
            gx_set_error("gx_png: filter byte %d in row %d (above 4)", (int)dst[r * stride], r);
            return GX_EDATA;
        }
    return GX_OK;
}

}  // extern "C"
