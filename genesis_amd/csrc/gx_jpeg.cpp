// Host half of the JPEG decoder (genesis_amd/jpeg.py): GQN's frames are baseline JPEG strings inside TFRecords
// (third_party/tf_gqn/gqn_tfr_provider.py:141-143: tf.image.decode_jpeg).  The serial part of decoding -- marker
// parsing and Huffman decoding -- runs here; everything that touches a pixel runs in gx_jpeg.hip.  Plain host
// functions, no HIP calls: they work without a GPU, as gx_tfrecord.cpp does.
//   accepted  SOF0, 8-bit samples, three components in one interleaved scan, luma 1x1 / 2x1 / 2x2 with chroma 1x1,
//             8-bit quantisation tables, any DHT tables, DRI with RSTn markers; APPn and COM are skipped
//   _any      the entry points of the ragged decoder (gx_imagefile.hip, genesis_amd/imagefile.py) share every line of the
//             marker walk and the Huffman code with the two above; they differ in two limits only: frames up to
//             kGxImageMaxDim on a side instead of 128, and one-component (greyscale) streams, whose single plane is
//             padded to whole 8 x 8 blocks
//   output    per component the blocks of its padded plane (whole MCUs) in raster order, each block 64 QUANTISED int16
//             coefficients in natural (row-major) order with the DC prediction undone; coefficient x quantiser does
//             not fit int16, so the kernel multiplies
// Every length and index is checked against the stream, the tables and the output capacity before it is used: no input
// makes these functions read or write out of bounds.
#include "gx_common.h"

#include <string.h>

namespace {

constexpr int kMaxDim = 128;           // gx_jpeg_decode_f32chw's frame limit (three planes in LDS)
constexpr int kLook = 9;               // bits of the Huffman lookahead table

const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool defined;
    unsigned char sym[256];
    int count;                         // symbols in the table
    int maxcode[18];                   // largest code of each length, -1 when the length has none
    int valptr[17], mincode[17];
    unsigned short look[1 << kLook];   // (length << 8) | symbol of every code of at most kLook bits; 0: longer
};

struct Frame {
    int width, height, sampling, hs, vs, mcux, mcuy, restart;
    int ncomp;                         // 3, or 1 (greyscale: the _any entry points only)
    int comp_id[3], comp_tq[3];
    int blocks_w[3], blocks_h[3];
    bool have_sof;
};

struct Parser {
    const unsigned char* p;
    size_t n, pos;
    unsigned short q[4][64];           // natural order
    bool q_defined[4];
    Huff dc[4], ac[4];
    Frame f;
    int scan_td[3], scan_ta[3];
    int max_dim;                       // kMaxDim, or kGxImageMaxDim for the _any entry points
    bool grey_ok;
};

int fail(const char* what) {
    gx_set_error("gx_jpeg: %s", what);
    return GX_EDATA;
}

// Canonical code assignment of a DHT table (counts of codes per length 1..16, symbols in code order).
bool build_huff(Huff* h, const unsigned char* counts, const unsigned char* symbols, int total) {
    memset(h->look, 0, sizeof(h->look));
    memcpy(h->sym, symbols, (size_t)total);
    h->count = total;
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        h->valptr[l] = k;
        h->mincode[l] = code;
        for (int i = 0; i < counts[l - 1]; ++i, ++k, ++code) {
            if (code >= (1 << l)) return false;                  // more codes than the length holds
            if (l <= kLook) {
                const int first = code << (kLook - l);
                for (int j = 0; j < (1 << (kLook - l)); ++j) h->look[first + j] = (unsigned short)((l << 8) | symbols[k]);
            }
        }
        h->maxcode[l] = counts[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
    h->maxcode[17] = 0x7fffffff;
    h->defined = true;
    return true;
}

// A marker segment's payload [start, start + len) from its two-byte length at pos; false when it runs past the stream.
bool segment(Parser* s, size_t* start, size_t* len) {
    if (s->n - s->pos < 2) return false;
    const size_t l = ((size_t)s->p[s->pos] << 8) | s->p[s->pos + 1];
    if (l < 2 || l > s->n - s->pos) return false;
    *start = s->pos + 2;
    *len = l - 2;
    s->pos += l;
    return true;
}

int parse_dqt(Parser* s, size_t at, size_t len) {
    const unsigned char* d = s->p + at;
    size_t i = 0;
    while (i < len) {
        const int pq = d[i] >> 4, tq = d[i] & 15;
        if (pq == 1) return fail("16-bit quantisation tables are not supported");
        if (pq != 0 || tq > 3) return fail("bad quantisation table header");
        if (len - i < 65) return fail("the stream ends early (inside a quantisation table)");
        for (int k = 0; k < 64; ++k) s->q[tq][kZigzag[k]] = d[i + 1 + k];
        s->q_defined[tq] = true;
        i += 65;
    }
    return GX_OK;
}

int parse_dht(Parser* s, size_t at, size_t len) {
    const unsigned char* d = s->p + at;
    size_t i = 0;
    while (i < len) {
        const int tc = d[i] >> 4, th = d[i] & 15;
        if (tc > 1 || th > 3) return fail("bad Huffman table header");
        if (len - i < 17) return fail("the stream ends early (inside a Huffman table)");
        int total = 0;
        for (int k = 0; k < 16; ++k) total += d[i + 1 + k];
        if (total > 256 || len - i - 17 < (size_t)total) return fail("bad Huffman table (symbol count)");
        if (!build_huff(tc ? &s->ac[th] : &s->dc[th], d + i + 1, d + i + 17, total)) return fail("bad Huffman table (code lengths)");
        i += 17 + (size_t)total;
    }
    return GX_OK;
}

int parse_sof0(Parser* s, size_t at, size_t len) {
    const unsigned char* d = s->p + at;
    Frame& f = s->f;
    if (len < 6) return fail("the stream ends early (inside the frame header)");
    if (d[0] != 8) {
        gx_set_error("gx_jpeg: %d-bit sample precision is not supported (8-bit only)", (int)d[0]);
        return GX_EDATA;
    }
    f.height = (d[1] << 8) | d[2];
    f.width = (d[3] << 8) | d[4];
    const int nf = d[5];
    if (nf == 1 && !s->grey_ok) return fail("greyscale (one component) is not supported");
    if (nf == 4) return fail("four components (CMYK / YCCK) are not supported");
    if (nf != 3 && nf != 1) return fail("bad component count");
    if (len < 6 + 3 * (size_t)nf) return fail("the stream ends early (inside the frame header)");
    if (f.width <= 0 || f.height <= 0) return fail("empty frame");
    if (f.width > s->max_dim || f.height > s->max_dim) {
        gx_set_error("gx_jpeg: a %d x %d frame is larger than the %d x %d the device kernel decodes", f.width, f.height, s->max_dim,
                     s->max_dim);
        return GX_EDATA;
    }
    f.ncomp = nf;
    int h[3] = {1, 1, 1}, v[3] = {1, 1, 1};
    for (int c = 0; c < nf; ++c) {
        f.comp_id[c] = d[6 + 3 * c];
        h[c] = d[7 + 3 * c] >> 4;
        v[c] = d[7 + 3 * c] & 15;
        f.comp_tq[c] = d[8 + 3 * c];
        if (f.comp_tq[c] > 3) return fail("bad quantisation table selector");
    }
    const bool chroma11 = h[1] == 1 && v[1] == 1 && h[2] == 1 && v[2] == 1;
    if (nf == 1) {                     // a single component is never interleaved: its blocks are 8 x 8 whatever its factors say
        h[0] = v[0] = 1;
        f.sampling = 0;
    } else if (chroma11 && h[0] == 1 && v[0] == 1) f.sampling = 0;
    else if (chroma11 && h[0] == 2 && v[0] == 1) f.sampling = 1;
    else if (chroma11 && h[0] == 2 && v[0] == 2) f.sampling = 2;
    else {
        gx_set_error("gx_jpeg: sampling factors %dx%d, %dx%d, %dx%d are not supported (luma 1x1, 2x1 or 2x2 with chroma 1x1)", h[0],
                     v[0], h[1], v[1], h[2], v[2]);
        return GX_EDATA;
    }
    f.hs = h[0];
    f.vs = v[0];
    f.mcux = (f.width + 8 * f.hs - 1) / (8 * f.hs);
    f.mcuy = (f.height + 8 * f.vs - 1) / (8 * f.vs);
    f.blocks_w[0] = f.mcux * f.hs;
    f.blocks_h[0] = f.mcuy * f.vs;
    f.blocks_w[1] = f.blocks_w[2] = nf == 3 ? f.mcux : 0;
    f.blocks_h[1] = f.blocks_h[2] = nf == 3 ? f.mcuy : 0;
    f.have_sof = true;
    return GX_OK;
}

int parse_sos(Parser* s, size_t at, size_t len) {
    const unsigned char* d = s->p + at;
    if (!s->f.have_sof) return fail("a scan before the frame header");
    if (len < 1) return fail("the stream ends early (inside the scan header)");
    const int nc = s->f.ncomp;
    if (d[0] != nc) return fail(nc == 3 ? "the three components must come in one interleaved scan" : "the scan does not hold the frame's one component");
    if (len < 1 + 2 * (size_t)nc + 3) return fail("the stream ends early (inside the scan header)");
    for (int c = 0; c < nc; ++c) {
        if (d[1 + 2 * c] != s->f.comp_id[c]) return fail("the scan's components are not the frame's, in order");
        s->scan_td[c] = d[2 + 2 * c] >> 4;
        s->scan_ta[c] = d[2 + 2 * c] & 15;
        if (s->scan_td[c] > 3 || s->scan_ta[c] > 3 || !s->dc[s->scan_td[c]].defined || !s->ac[s->scan_ta[c]].defined)
            return fail("the scan names a Huffman table that was not defined");
        if (!s->q_defined[s->f.comp_tq[c]]) return fail("the frame names a quantisation table that was not defined");
    }
    if (d[1 + 2 * nc] != 0 || d[2 + 2 * nc] != 63 || d[3 + 2 * nc] != 0) return fail("a progressive scan (spectral selection / successive approximation)");
    return GX_OK;
}

// Walks the markers up to and including the first SOS; s->pos is then the first byte of the entropy-coded segment.
int parse_headers(Parser* s) {
    if (s->n < 2 || s->p[0] != 0xFF || s->p[1] != 0xD8) return fail("not a JPEG stream (no SOI marker)");
    s->pos = 2;
    for (;;) {
        if (s->n - s->pos < 2) return fail("the stream ends early (before the scan)");
        if (s->p[s->pos] != 0xFF) return fail("a marker was expected");
        const int m = s->p[s->pos + 1];
        if (m == 0xFF) {               // fill byte
            ++s->pos;
            continue;
        }
        s->pos += 2;
        if (m == 0xD9) return fail("the stream ends early (EOI before the scan)");
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;      // markers without a segment
        size_t at, len;
        if (!segment(s, &at, &len)) return fail("the stream ends early (inside a marker segment)");
        int rc = GX_OK;
        if (m == 0xC0) rc = parse_sof0(s, at, len);
        else if (m == 0xC2 || m == 0xC6) return fail("progressive JPEG is not supported");
        else if (m == 0xC1 || m == 0xC3 || m == 0xC5 || m == 0xC7) return fail("extended / lossless / hierarchical SOF is not supported (baseline SOF0 only)");
        else if (m >= 0xC9 && m <= 0xCF) return fail("arithmetic coding is not supported");
        else if (m == 0xC4) rc = parse_dht(s, at, len);
        else if (m == 0xDB) rc = parse_dqt(s, at, len);
        else if (m == 0xDD) {
            if (len < 2) return fail("the stream ends early (inside DRI)");
            s->f.restart = (s->p[at] << 8) | s->p[at + 1];
        } else if (m == 0xDA) {
            return parse_sos(s, at, len);
        } else if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {
            // APPn, COM: skipped
        } else {
            gx_set_error("gx_jpeg: unsupported marker 0xFF%02X", m);
            return GX_EDATA;
        }
        if (rc != GX_OK) return rc;
    }
}

void fill_info(const Frame& f, int* info) {
    info[0] = f.width;
    info[1] = f.height;
    info[2] = f.ncomp;
    info[3] = f.sampling;
    for (int c = 0; c < 3; ++c) info[4 + c] = f.blocks_w[c] * f.blocks_h[c];      // at most 512 * 512
    info[7] = f.restart;
}

// Bit reader over the entropy-coded segment: FF 00 is a stuffed FF; any other marker ends the supply of bits.
struct Bits {
    const unsigned char* p;
    size_t n, pos;
    uint64_t buf;                      // the next bits, left-aligned at bit (count - 1)
    int count;

    void fill() {
        while (count <= 56) {
            if (pos >= n) return;
            unsigned b = p[pos];
            if (b == 0xFF) {
                if (pos + 1 >= n) return;
                if (p[pos + 1] != 0) return;                     // a marker: no more bits from here
                pos += 2;
            } else {
                ++pos;
            }
            buf = (buf << 8) | b;
            count += 8;
        }
    }
    // the next k <= 16 bits; false when the segment holds fewer
    bool get(int k, int* v) {
        if (k == 0) {
            *v = 0;
            return true;
        }
        if (count < k) {
            fill();
            if (count < k) return false;
        }
        *v = (int)((buf >> (count - k)) & ((1u << k) - 1));
        count -= k;
        return true;
    }
};

// 0: decoded, 1: the segment ends early, 2: a code that is not in the table
int huff_decode(Bits* b, const Huff& h, int* sym) {
    if (b->count < 16) b->fill();
    if (b->count >= kLook) {
        const unsigned short e = h.look[(b->buf >> (b->count - kLook)) & ((1u << kLook) - 1)];
        if (e) {
            b->count -= e >> 8;
            *sym = e & 0xff;
            return 0;
        }
    }
    int code = 0;
    for (int l = 1; l <= 16; ++l) {
        int bit;
        if (!b->get(1, &bit)) return 1;
        code = (code << 1) | bit;
        if (h.maxcode[l] >= 0 && code <= h.maxcode[l] && code >= h.mincode[l]) {
            const int idx = h.valptr[l] + code - h.mincode[l];
            if (idx >= h.count) return 2;
            *sym = h.sym[idx];
            return 0;
        }
    }
    return 2;
}

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

int decode_block(Bits* b, const Huff& dc, const Huff& ac, int* pred, short* out) {
    int s, v;
    int rc = huff_decode(b, dc, &s);
    if (rc == 1) return fail("the stream ends early (inside the entropy-coded segment)");
    if (rc == 2) return fail("a Huffman code that is not in the table");
    if (s > 11) return fail("a DC difference of more than 11 bits");
    if (s) {
        if (!b->get(s, &v)) return fail("the stream ends early (inside the entropy-coded segment)");
        *pred += extend(v, s);
    }
    out[0] = (short)*pred;
    int k = 1;
    while (k < 64) {
        int rs;
        rc = huff_decode(b, ac, &rs);
        if (rc == 1) return fail("the stream ends early (inside the entropy-coded segment)");
        if (rc == 2) return fail("a Huffman code that is not in the table");
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;        // end of block
            k += 16;
            if (k > 64) return fail("a coefficient index past 63");
            continue;
        }
        k += r;
        if (k > 63) return fail("a coefficient index past 63");
        if (!b->get(s, &v)) return fail("the stream ends early (inside the entropy-coded segment)");
        out[kZigzag[k]] = (short)extend(v, s);
        ++k;
    }
    return GX_OK;
}

int decode_scan(Parser* s, short* coef) {
    const Frame& f = s->f;
    Bits b = {s->p, s->n, s->pos, 0, 0};
    short* plane[3];
    plane[0] = coef;
    plane[1] = plane[0] + (size_t)f.blocks_w[0] * f.blocks_h[0] * 64;
    plane[2] = plane[1] + (size_t)f.blocks_w[1] * f.blocks_h[1] * 64;
    int pred[3] = {0, 0, 0};
    const int total = f.mcux * f.mcuy;
    int until_restart = f.restart, next_rst = 0;
    for (int m = 0; m < total; ++m) {
        if (f.restart && until_restart == 0) {
            // byte-align, then the expected RSTn marker (fill bytes before it allowed)
            b.buf = 0;
            b.count = 0;
            while (b.n - b.pos >= 2 && b.p[b.pos] == 0xFF && b.p[b.pos + 1] == 0xFF) ++b.pos;
            if (b.n - b.pos < 2) return fail("the stream ends early (a restart marker is missing)");
            if (b.p[b.pos] != 0xFF || b.p[b.pos + 1] != 0xD0 + next_rst) return fail("a restart marker is missing or out of sequence");
            b.pos += 2;
            next_rst = (next_rst + 1) & 7;
            until_restart = f.restart;
            pred[0] = pred[1] = pred[2] = 0;
        }
        const int my = m / f.mcux, mx = m - my * f.mcux;
        for (int c = 0; c < f.ncomp; ++c) {
            const int ch = c == 0 ? f.hs : 1, cv = c == 0 ? f.vs : 1;
            for (int v = 0; v < cv; ++v)
                for (int h = 0; h < ch; ++h) {
                    const int by = my * cv + v, bx = mx * ch + h;           // inside the padded plane by construction
                    short* out = plane[c] + ((size_t)by * f.blocks_w[c] + bx) * 64;
                    const int rc = decode_block(&b, s->dc[s->scan_td[c]], s->ac[s->scan_ta[c]], &pred[c], out);
                    if (rc != GX_OK) return rc;
                }
        }
        --until_restart;
    }
    return GX_OK;
}

// the two pairs of entry points differ in the limits only
int info_entry(const unsigned char* data, size_t len, int* info, int max_dim, bool grey_ok) {
    Parser s = {};
    s.p = data;
    s.n = len;
    s.max_dim = max_dim;
    s.grey_ok = grey_ok;
    const int rc = parse_headers(&s);
    if (rc == GX_OK) fill_info(s.f, info);
    return rc;
}

int decode_entry(const char* name, const unsigned char* data, size_t len, short* coef, size_t coef_capacity, unsigned short* qtab, int* info,
                 int max_dim, bool grey_ok) {
    Parser s = {};
    s.p = data;
    s.n = len;
    s.max_dim = max_dim;
    s.grey_ok = grey_ok;
    int rc = parse_headers(&s);
    if (rc == GX_OK) {
        fill_info(s.f, info);
        const size_t need = ((size_t)info[4] + info[5] + info[6]) * 64;
        if (need > coef_capacity) {
            gx_set_error("%s: the frame needs %zu coefficients, the buffer holds %zu", name, need, coef_capacity);
            rc = GX_EINVAL;
        } else {
            memset(coef, 0, need * sizeof(short));
            // a grey frame's second and third table are its first: all 192 values are always written
            for (int c = 0; c < 3; ++c) memcpy(qtab + 64 * c, s.q[s.f.comp_tq[c < s.f.ncomp ? c : 0]], 64 * sizeof(unsigned short));
            rc = decode_scan(&s, coef);
        }
    }
    return rc;
}

}  // namespace

extern "C" {

int gx_jpeg_info(const unsigned char* data, size_t len, int* info) {
    GX_CHECK_ARG(data && info, "gx_jpeg_info: null pointer");
    return info_entry(data, len, info, kMaxDim, false);
}

int gx_jpeg_entropy_decode(const unsigned char* data, size_t len, short* coef, size_t coef_capacity, unsigned short* qtab,
                           int* info) {
    GX_CHECK_ARG(data && coef && qtab && info, "gx_jpeg_entropy_decode: null pointer");
    return decode_entry("gx_jpeg_entropy_decode", data, len, coef, coef_capacity, qtab, info, kMaxDim, false);
}

int gx_jpeg_info_any(const unsigned char* data, size_t len, int* info) {
    GX_CHECK_ARG(data && info, "gx_jpeg_info_any: null pointer");
    return info_entry(data, len, info, kGxImageMaxDim, true);
}

int gx_jpeg_entropy_decode_any(const unsigned char* data, size_t len, short* coef, size_t coef_capacity, unsigned short* qtab,
                               int* info) {
    GX_CHECK_ARG(data && coef && qtab && info, "gx_jpeg_entropy_decode_any: null pointer");
    return decode_entry("gx_jpeg_entropy_decode_any", data, len, coef, coef_capacity, qtab, info, kGxImageMaxDim, true);
}

}  // extern "C"
