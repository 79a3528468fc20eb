// Host side of the TFRecord reader (genesis_amd/tfrecord.py): the multi-object datasets the reference opens through
// TensorFlow (datasets/multi_object_config.py:65-100, third_party/multi_object_datasets/*.py) are TFRecord files of
// tf.Example protos whose `image` and `mask` features store every pixel byte as its own one-byte string of a bytes_list:
// `0A 01 vv` on the wire, three bytes per byte.  Plain host functions, no HIP calls: they work without a GPU, as
// gx_pil_bilinear_coeffs does.
//   framing   u64 length | u32 masked crc32c(length) | data | u32 masked crc32c(data), little endian
//   Example   features(1) -> Features.feature(1) map entries (key 1, value 2) -> Feature.bytes_list(1) -> BytesList.value(1)
#include "gx_common.h"

#include <string.h>

namespace {

// CRC-32C (Castagnoli, reflected polynomial 0x82F63B78), slicing by 8.
struct Crc32cTables {
    uint32_t t[8][256];
    Crc32cTables() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xff];
    }
};

uint32_t crc32c(const unsigned char* p, size_t n) {
    static const Crc32cTables tab;
    uint32_t c = 0xffffffffu;
    while (n && ((uintptr_t)p & 7)) {
        c = (c >> 8) ^ tab.t[0][(c ^ *p++) & 0xff];
        --n;
    }
    while (n >= 8) {
        uint64_t w;
        memcpy(&w, p, 8);
        w ^= c;
        c = tab.t[7][w & 0xff] ^ tab.t[6][(w >> 8) & 0xff] ^ tab.t[5][(w >> 16) & 0xff] ^ tab.t[4][(w >> 24) & 0xff] ^
            tab.t[3][(w >> 32) & 0xff] ^ tab.t[2][(w >> 40) & 0xff] ^ tab.t[1][(w >> 48) & 0xff] ^ tab.t[0][w >> 56];
        p += 8;
        n -= 8;
    }
    while (n--) c = (c >> 8) ^ tab.t[0][(c ^ *p++) & 0xff];
    return ~c;
}

uint32_t mask_crc(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

uint32_t load_u32(const unsigned char* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

uint64_t load_u64(const unsigned char* p) { return (uint64_t)load_u32(p) | ((uint64_t)load_u32(p + 4) << 32); }

// A protobuf varint at *pos of p[0..n): false when it runs past n or past ten bytes.
bool read_varint(const unsigned char* p, size_t n, size_t* pos, uint64_t* v) {
    uint64_t r = 0;
    for (int shift = 0; shift < 70; shift += 7) {
        if (*pos >= n) return false;
        const unsigned char b = p[(*pos)++];
        r |= (uint64_t)(b & 0x7f) << (shift < 64 ? shift : 63);
        if (!(b & 0x80)) {
            *v = r;
            return true;
        }
    }
    return false;
}

// A length-delimited field's payload: its varint length, then that many bytes inside p[0..n).
bool read_span(const unsigned char* p, size_t n, size_t* pos, size_t* start, size_t* len) {
    uint64_t l;
    if (!read_varint(p, n, pos, &l) || l > n - *pos) return false;
    *start = *pos;
    *len = (size_t)l;
    *pos += (size_t)l;
    return true;
}

// Skips a field's value by wire type (0 varint, 1 fixed64, 2 length-delimited, 5 fixed32); groups (3, 4) are refused.
bool skip_field(const unsigned char* p, size_t n, size_t* pos, unsigned wire) {
    uint64_t v;
    size_t s, l;
    switch (wire) {
        case 0: return read_varint(p, n, pos, &v);
        case 1: if (n - *pos < 8) return false; *pos += 8; return true;
        case 2: return read_span(p, n, pos, &s, &l);
        case 5: if (n - *pos < 4) return false; *pos += 4; return true;
        default: return false;
    }
}

// The payload of the last field `field` with wire type 2 among the fields of the message p[0..n); other fields are
// skipped.  0: found, 1: absent, -1: malformed.
int find_field(const unsigned char* p, size_t n, unsigned field, size_t* start, size_t* len) {
    size_t pos = 0;
    int found = 1;
    while (pos < n) {
        uint64_t tag;
        if (!read_varint(p, n, &pos, &tag)) return -1;
        if ((tag >> 3) == field && (tag & 7) == 2) {
            if (!read_span(p, n, &pos, start, len)) return -1;
            found = 0;
        } else if (!skip_field(p, n, &pos, (unsigned)(tag & 7))) {
            return -1;
        }
    }
    return found;
}

}  // namespace

extern "C" {

unsigned int gx_crc32c(const void* data, size_t n) { return (n && !data) ? 0u : crc32c((const unsigned char*)data, n); }

unsigned int gx_crc32c_masked(const void* data, size_t n) { return mask_crc(gx_crc32c(data, n)); }

int gx_tfrecord_scan(const unsigned char* buf, size_t n, int verify_crc, long long first_index, int max_records,
                     long long* offsets, long long* lengths, int* num_records, size_t* consumed) {
    GX_CHECK_ARG((buf || n == 0) && offsets && lengths && num_records && consumed, "gx_tfrecord_scan: null pointer");
    GX_CHECK_ARG(max_records >= 0, "gx_tfrecord_scan: bad max_records %d", max_records);
    size_t pos = 0;
    int k = 0;
    *num_records = 0;
    *consumed = 0;
    while (k < max_records && n - pos >= 12) {
        const uint64_t len = load_u64(buf + pos);
        if (verify_crc && mask_crc(crc32c(buf + pos, 8)) != load_u32(buf + pos + 8)) {
            gx_set_error("gx_tfrecord_scan: record %lld: the checksum of its length field does not match (length reads %llu)",
                         first_index + k, (unsigned long long)len);
            return GX_EDATA;
        }
        if (len > ((uint64_t)1 << 40)) {
            gx_set_error("gx_tfrecord_scan: record %lld: implausible length %llu", first_index + k, (unsigned long long)len);
            return GX_EDATA;
        }
        if (n - pos - 12 < len || n - pos - 12 - (size_t)len < 4) break;      // a partial record: the caller feeds a stream
        const unsigned char* data = buf + pos + 12;
        if (verify_crc && mask_crc(crc32c(data, (size_t)len)) != load_u32(data + len)) {
            gx_set_error("gx_tfrecord_scan: record %lld: the checksum of its %llu data bytes does not match", first_index + k,
                         (unsigned long long)len);
            return GX_EDATA;
        }
        offsets[k] = (long long)(pos + 12);
        lengths[k] = (long long)len;
        ++k;
        pos += 12 + (size_t)len + 4;
    }
    *num_records = k;
    *consumed = pos;
    return GX_OK;
}

int gx_tfexample_find_bytes_list(const unsigned char* rec, size_t n, const char* name, long long* offset, long long* length) {
    GX_CHECK_ARG(rec && name && offset && length, "gx_tfexample_find_bytes_list: null pointer");
    const size_t name_len = strlen(name);
    size_t pos = 0;
    bool found = false;
    while (pos < n) {                                           // Example: every `features` field (a split message merges)
        uint64_t tag;
        size_t fs, fl;
        if (!read_varint(rec, n, &pos, &tag)) goto malformed;
        if ((tag >> 3) != 1 || (tag & 7) != 2) {
            if (!skip_field(rec, n, &pos, (unsigned)(tag & 7))) goto malformed;
            continue;
        }
        if (!read_span(rec, n, &pos, &fs, &fl)) goto malformed;
        const unsigned char* feats = rec + fs;
        size_t fp = 0;
        while (fp < fl) {                                       // Features: the map entries
            size_t es, el, ks = 0, kl = 0, vs = 0, vl = 0;
            if (!read_varint(feats, fl, &fp, &tag)) goto malformed;
            if ((tag >> 3) != 1 || (tag & 7) != 2) {
                if (!skip_field(feats, fl, &fp, (unsigned)(tag & 7))) goto malformed;
                continue;
            }
            if (!read_span(feats, fl, &fp, &es, &el)) goto malformed;
            const unsigned char* entry = feats + es;
            const int hk = find_field(entry, el, 1, &ks, &kl);
            if (hk < 0) goto malformed;
            if (hk != 0 || kl != name_len || memcmp(entry + ks, name, name_len) != 0) continue;
            const int hv = find_field(entry, el, 2, &vs, &vl);
            if (hv < 0) goto malformed;
            size_t bs = 0, bl = 0;
            const int hb = hv == 0 ? find_field(entry + vs, vl, 1, &bs, &bl) : 1;
            if (hb < 0) goto malformed;
            if (hb != 0) {
                gx_set_error("gx_tfexample_find_bytes_list: feature '%s' is not a bytes_list", name);
                return GX_EDATA;
            }
            *offset = (long long)(fs + es + vs + bs);
            *length = (long long)bl;
            found = true;
        }
    }
    if (!found) {
        gx_set_error("gx_tfexample_find_bytes_list: no feature '%s' in the record", name);
        return GX_EDATA;
    }
    return GX_OK;
malformed:
    gx_set_error("gx_tfexample_find_bytes_list: malformed tf.Example (a varint or a length runs past the %zu-byte record)", n);
    return GX_EDATA;
}

int gx_bytes_list_unpack(const unsigned char* payload, size_t n, unsigned char* dst, size_t expected) {
    GX_CHECK_ARG((payload || n == 0) && (dst || expected == 0), "gx_bytes_list_unpack: null pointer");
    if (n == 3 * expected) {
        // every value one byte long: a strict `0A 01 vv` stride.  Copied while the two constant bytes are checked; a
        // mismatch anywhere sends the whole list through the general walk, which overwrites dst.
        unsigned bad = 0;
        for (size_t i = 0; i < expected; ++i) {
            bad |= (unsigned)(payload[3 * i] ^ 0x0A) | (unsigned)(payload[3 * i + 1] ^ 0x01);
            dst[i] = payload[3 * i + 2];
        }
        if (!bad) return GX_OK;
    }
    size_t pos = 0, total = 0;
    while (pos < n) {
        uint64_t tag;
        size_t s, l;
        if (!read_varint(payload, n, &pos, &tag)) goto malformed;
        if ((tag >> 3) == 1 && (tag & 7) == 2) {
            if (!read_span(payload, n, &pos, &s, &l)) goto malformed;
            if (l <= expected - (total < expected ? total : expected)) memcpy(dst + total, payload + s, l);
            total += l;                                         // past `expected` only counted, for the message
        } else if (!skip_field(payload, n, &pos, (unsigned)(tag & 7))) {
            goto malformed;
        }
    }
    if (total != expected) {
        gx_set_error("gx_bytes_list_unpack: the list holds %zu bytes, expected %zu", total, expected);
        return GX_EDATA;
    }
    return GX_OK;
malformed:
    gx_set_error("gx_bytes_list_unpack: malformed bytes_list (a varint or a length runs past its %zu bytes)", n);
    return GX_EDATA;
}

int gx_bytes_list_index(const unsigned char* payload, size_t n, int max_values, long long* offsets, long long* lengths,
                        int* count) {
    GX_CHECK_ARG((payload || n == 0) && offsets && lengths && count, "gx_bytes_list_index: null pointer");
    GX_CHECK_ARG(max_values >= 0, "gx_bytes_list_index: bad max_values %d", max_values);
    size_t pos = 0;
    long long k = 0;
    *count = 0;
    while (pos < n) {
        uint64_t tag;
        size_t s, l;
        if (!read_varint(payload, n, &pos, &tag)) goto malformed;
        if ((tag >> 3) == 1 && (tag & 7) == 2) {
            if (!read_span(payload, n, &pos, &s, &l)) goto malformed;
            if (k < max_values) {
                offsets[k] = (long long)s;
                lengths[k] = (long long)l;
            }
            ++k;                                                // past max_values only counted, for the message
        } else if (!skip_field(payload, n, &pos, (unsigned)(tag & 7))) {
            goto malformed;
        }
    }
    if (k > max_values) {
        gx_set_error("gx_bytes_list_index: the list holds %lld values, the caller gave %d slots", k, max_values);
        return GX_EDATA;
    }
    *count = (int)k;
    return GX_OK;
malformed:
    gx_set_error("gx_bytes_list_index: malformed bytes_list (a varint or a length runs past its %zu bytes)", n);
    return GX_EDATA;
}

}  // extern "C"
