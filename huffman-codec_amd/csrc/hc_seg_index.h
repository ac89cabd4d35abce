// hc_seg_index.h — the host's reading of a segmented container's header and index (HCSEG1,
// include/hcodec.h): the cut rule, every header rule, the segments a byte range covers, and the
// index scan that hc_seg_decompress_range runs before it uploads anything. Plain C++, no HIP
// types: hc_seg.hip includes it, and so does tests/seg_index_check.cpp, which runs it under the
// sanitizers. Everything here parses untrusted lengths: sums saturate and ranges are compared by
// subtraction, as in the device scan (seg_open_kernel), whose verdicts these must equal.
#pragma once

#include <stdint.h>
#include <string.h>

#include "hcodec.h"

namespace hc_seg_index {

constexpr uint32_t kSegFlags = HC_FLAG_DIFF | HC_FLAG_ADAPT | HC_SEG_CHECK_CRC32;
const uint8_t kMagic[8] = {0x48, 0x43, 0x53, 0x45, 0x47, 0x31, 0x00, 0xFF};

inline uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }
inline uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
// header and index: 8 bytes of enc_len per segment, and 4 of crc in a checked container
inline bool checked(uint32_t flags) { return (flags & HC_SEG_CHECK_CRC32) != 0; }
inline uint64_t index_end(uint64_t n, bool check) { return 48 + (check ? 12 : 8) * n; }

// The cut rule: segment k is raw bytes [k full, k full + (k == n - 1 ? last : full)). n == 0:
// invalid arguments. No product here overflows: every one is at most raw.
struct Cuts {
    uint64_t n, full, last;
};
inline Cuts seg_cuts(uint64_t raw, uint64_t seg, bool adapt, uint64_t width)
{
    Cuts c{0, 0, 0};
    if (seg == 0 || (seg & 15u)) return c;
    if (!adapt) {
        c.n = raw / seg + (raw % seg != 0);
        if (c.n == 0) c.n = 1;
        c.full = seg;
        c.last = raw - (c.n - 1) * seg;
        return c;
    }
    if (width < 8 || raw % width != 0 || raw / width < 8) return c;
    // bands of `rows` rows, a multiple of 4 so that every band starts 4-byte aligned; a band
    // that would leave fewer than 8 rows (too few for a matrix) takes those too
    const uint64_t h = raw / width;
    uint64_t rows = (seg / width) & ~3ull;
    if (rows < 8) rows = 8;
    const uint64_t q = h / rows, r = h % rows;
    c.full = rows * width;
    if (q == 0) {
        c.n = 1;
        c.last = raw;
    } else if (r < 8) {
        c.n = q;
        c.last = (rows + r) * width;
    } else {
        c.n = q + 1;
        c.last = r * width;
    }
    return c;
}

// every header rule that needs no index entry (hc_seg_info; the device decoders on their info)
inline bool info_ok(const hc_seg_info_t &f, uint64_t in_len, Cuts &c)
{
    if (in_len < 48) return false;
    if (f.flags & ~kSegFlags) return false;
    const bool adapt = (f.flags & HC_FLAG_ADAPT) != 0;
    if (!adapt && f.width != 0) return false;
    c = seg_cuts(f.raw_len, f.seg_bytes, adapt, f.width);
    if (c.n == 0 || c.n != f.n_segments) return false;
    if (c.n > (in_len - 48) / (checked(f.flags) ? 12 : 8)) return false;  // 48 + 8 n (checked: 12 n) <= in_len
    // at most 8 symbols per payload byte, and 4 symbols expand to at most 258 bytes
    if (in_len <= ~0ull / 520 && f.raw_len > 520 * in_len) return false;
    return true;
}

inline uint64_t get64(const uint8_t *p)
{
    uint64_t v = 0;
    for (int i = 7; i >= 0; --i) v = (v << 8) | p[i];
    return v;
}

// hc_seg_info after its null check: the 48 header bytes against in_len
inline int parse_header(const uint8_t *in, uint64_t in_len, hc_seg_info_t *info)
{
    memset(info, 0, sizeof(*info));
    if (!in || in_len < 48) return HC_ERR_SEG_HEADER;
    if (memcmp(in, kMagic, 8) != 0) return HC_ERR_SEG_HEADER;
    if (in[9] > 1) return HC_ERR_SEG_HEADER;  // the check kind: none or CRC-32
    for (int i = 10; i < 16; ++i)
        if (in[i]) return HC_ERR_SEG_HEADER;
    hc_seg_info_t f;
    f.flags = in[8] | ((uint32_t)in[9] << 8);
    f.raw_len = get64(in + 16);
    f.seg_bytes = get64(in + 24);
    f.width = get64(in + 32);
    f.n_segments = get64(in + 40);
    Cuts c;
    if (!info_ok(f, in_len, c)) return HC_ERR_SEG_HEADER;
    *info = f;
    return HC_OK;
}

// The segments that hold raw bytes [offset, offset + length), length > 0 inside raw_len: k0 ..
// k0 + count - 1. The clamp to n - 1 is for an adaptive container whose last band took leftover
// rows (last > full): bytes past n full belong to it. length == 0: none (k0 0, count 0).
struct Cover {
    uint64_t k0, count;
};
inline bool range_ok(uint64_t raw_len, uint64_t offset, uint64_t length)
{
    return offset <= raw_len && length <= raw_len - offset;
}
inline Cover range_cover(const Cuts &c, uint64_t offset, uint64_t length)
{
    if (length == 0) return Cover{0, 0};
    uint64_t k0 = offset / c.full, k1 = (offset + length - 1) / c.full;
    if (k0 > c.n - 1) k0 = c.n - 1;
    if (k1 > c.n - 1) k1 = c.n - 1;
    return Cover{k0, k1 - k0 + 1};
}

// The index of a container whose header passed info_ok (so the n entries lie inside in_len):
// HC_OK when the entries tile [align16(index end), in_len) exactly, else HC_ERR_SEG_HEADER.
// *s0, *s1: the encoded bytes [s0, s1) of the covered segments, from segment k0's first byte to
// the last byte of segment k0 + count - 1 (count 0: both the first segment's offset).
inline int index_scan(const uint8_t *in, uint64_t in_len, uint64_t n, bool check, Cover cv, uint64_t *s0,
                      uint64_t *s1)
{
    uint64_t off = align16(index_end(n, check));
    *s0 = *s1 = off;
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t len = get64(in + 48 + 8 * k);
        if (len > in_len || off > in_len || len > in_len - off) return HC_ERR_SEG_HEADER;
        if (k == n - 1 && off + len != in_len) return HC_ERR_SEG_HEADER;  // truncated, or trailing bytes
        if (cv.count && k == cv.k0) *s0 = off;
        if (cv.count && k == cv.k0 + cv.count - 1) *s1 = off + len;
        off = sat_add(off, align16(len));
    }
    return HC_OK;
}

// ---------------------------------------------------------------------------------------------
// Range write (hc_seg_update*): the host's plan of a patch list. The covered segments of a call,
// in container order, are the entries 0 .. covered - 1 of its covered array; those among them
// that must be decoded first (every one whose cut does not lie inside ONE patch) are the entries
// 0 .. decoded - 1 of its decoded array, in the same order. A segment that two patches share
// belongs to the first of them.
// ---------------------------------------------------------------------------------------------
// The patch list's rules: every patch inside raw_len, sorted by offset, none overlapping, and
// (data_len != nullptr) every source range inside *data_len. n_patches > 0 needs the list.
inline bool patches_ok(uint64_t raw_len, const hc_seg_patch_t *p, uint32_t n_patches, const uint64_t *data_len)
{
    if (n_patches && !p) return false;
    uint64_t prev_end = 0;
    for (uint32_t i = 0; i < n_patches; ++i) {
        if (!range_ok(raw_len, p[i].offset, p[i].length)) return false;
        if (p[i].offset < prev_end) return false;  // unsorted, or overlapping the one before
        prev_end = p[i].offset + p[i].length;      // (<= raw_len: no wrap)
        if (data_len && !range_ok(*data_len, p[i].src_off, p[i].length)) return false;
    }
    return true;
}

// One patch as the device stages read it. Its bytes go to `dst` of the staging region, where
// covered entry c holds its segment's raw bytes from c full on. It newly covers the segments k0 ..
// k0 + cnt - 1, the entries e0 .. e0 + cnt - 1; of those, the first (dmask bit 0) and, when cnt > 1,
// the last (bit 1) are sent to the decoder, as decoded entries d0 and d0 + (dmask & 1).
struct PatchRec {
    uint64_t src_off, length, dst;
    uint64_t k0, cnt, e0;
    uint64_t d0, dmask;
};
struct UpdPlan {
    uint64_t covered, decoded;
    uint64_t cov_raw, dec_raw;  // the raw bytes of the covered, of the decoded segments
    uint64_t cov_bound;         // the sum of align16(bound(cut)) over the covered segments
};
// segment k's cut [b, e) (raw: raw_len)
inline void cut_of(const Cuts &c, uint64_t raw, uint64_t k, uint64_t *b, uint64_t *e)
{
    *b = k * c.full;
    *e = k == c.n - 1 ? raw : *b + c.full;
}
// Walks a patch list that passed patches_ok once. recs (or null): n_patches records. bound_full,
// bound_last: align16(hc_compress_bound) of a full cut and of the last one.
inline UpdPlan update_plan(const Cuts &c, uint64_t raw, const hc_seg_patch_t *p, uint32_t n_patches, uint64_t bound_full,
                           uint64_t bound_last, PatchRec *recs)
{
    UpdPlan u{0, 0, 0, 0, 0};
    uint64_t next = 0;  // every segment below this one is placed
    for (uint32_t i = 0; i < n_patches; ++i) {
        PatchRec r{p[i].src_off, p[i].length, 0, 0, 0, u.covered, u.decoded, 0};
        const uint64_t o = p[i].offset, end = o + p[i].length;
        const Cover cv = range_cover(c, o, p[i].length);
        if (cv.count) {
            const uint64_t a = cv.k0, b = cv.k0 + cv.count - 1;
            // a < next: the patch before ended in segment a, the last entry so far
            r.dst = (a >= next ? u.covered : u.covered - 1) * c.full + (o - a * c.full);
            r.k0 = a > next ? a : next;
            r.cnt = b >= r.k0 ? b - r.k0 + 1 : 0;
        }
        if (r.cnt) {
            const uint64_t kl = r.k0 + r.cnt - 1;
            uint64_t sb, se;
            cut_of(c, raw, r.k0, &sb, &se);
            if (!(o <= sb && end >= se)) {
                r.dmask |= 1;
                u.dec_raw += se - sb;
            }
            if (r.cnt > 1) {
                cut_of(c, raw, kl, &sb, &se);
                if (!(o <= sb && end >= se)) {
                    r.dmask |= 2;
                    u.dec_raw += se - sb;
                }
            }
            u.decoded += (r.dmask & 1) + (r.dmask >> 1);
            u.covered += r.cnt;
            const bool tail = kl == c.n - 1;
            u.cov_raw += (r.cnt - 1) * c.full + (tail ? raw - kl * c.full : c.full);
            u.cov_bound = sat_add(u.cov_bound, sat_add((r.cnt - 1) * bound_full, tail ? bound_last : bound_full));
            next = kl + 1;
        }
        if (recs) recs[i] = r;
    }
    return u;
}

// ---------------------------------------------------------------------------------------------
// List read (hc_seg_decompress_ranges*): the host's plan of a read list. The covered segments of
// a call, in container order, are the entries 0 .. covered - 1 of its covered array, each once
// however many reads name it; covered entry c decodes to c full of a staging region. A read's
// covered segments are consecutive entries, and only segment n - 1 (the highest entry when it is
// covered) has another length than full, so a read's bytes are one contiguous run of that region.
// ---------------------------------------------------------------------------------------------
// The read list's rules: every read inside raw_len, sorted by offset (source ranges may overlap
// or repeat), no dst_off + length that wraps. n_reads > 0 needs the list. *need (or null): the
// highest dst_off + length of the reads that are not empty, 0 when there is none.
inline bool reads_ok(uint64_t raw_len, const hc_seg_read_t *r, uint32_t n_reads, uint64_t *need)
{
    if (n_reads && !r) return false;
    uint64_t prev = 0, top = 0;
    for (uint32_t i = 0; i < n_reads; ++i) {
        if (!range_ok(raw_len, r[i].offset, r[i].length)) return false;
        if (r[i].offset < prev) return false;  // unsorted
        prev = r[i].offset;
        if (r[i].dst_off + r[i].length < r[i].dst_off) return false;
        if (r[i].length && r[i].dst_off + r[i].length > top) top = r[i].dst_off + r[i].length;
    }
    if (need) *need = top;
    return true;
}

// One read as the device stages see it. It covers the segments k0 .. k0 + cnt - 1, the covered
// entries e0 .. e0 + cnt - 1, and its `length` bytes lie at `src` of the staging region, e0 full +
// (offset - k0 full); they go to out + dst_off. An empty read covers nothing (cnt 0) and carries
// the k0 and e0 of the read before it (0 and 0 when it is the first), so that e0 ascends over the
// whole list and k0 - e0 is what it is for every entry of the run of segments the list has reached.
struct ReadRec {
    uint64_t k0, cnt, e0;
    uint64_t src, length, dst_off;
};
struct ReadPlan {
    uint64_t covered, cov_raw;  // the covered segments, their raw bytes
    uint64_t k_lo, k_hi;        // the lowest and the highest covered segment (covered > 0)
};
// Walks a read list that passed reads_ok once. recs (or null): n_reads records. The offsets
// ascend, so the first covered segments do, and every segment below `next` is counted: a read that
// starts below it starts inside the last run of covered segments, next - a entries from its end.
inline ReadPlan reads_plan(const Cuts &c, uint64_t raw, const hc_seg_read_t *r, uint32_t n_reads, ReadRec *recs)
{
    ReadPlan u{0, 0, 0, 0};
    uint64_t next = 0, k0 = 0, e0 = 0;
    for (uint32_t i = 0; i < n_reads; ++i) {
        const Cover cv = range_cover(c, r[i].offset, r[i].length);
        ReadRec rec{k0, 0, e0, 0, r[i].length, r[i].dst_off};
        if (cv.count) {
            const uint64_t a = cv.k0, b = cv.k0 + cv.count - 1;
            if (u.covered == 0) u.k_lo = a;
            k0 = a;
            e0 = a >= next ? u.covered : u.covered - (next - a);
            rec.k0 = k0;
            rec.cnt = cv.count;
            rec.e0 = e0;
            rec.src = e0 * c.full + (r[i].offset - a * c.full);
            if (b >= next) {  // the segments max(a, next) .. b are new
                const uint64_t first = a > next ? a : next, cnt = b - first + 1;
                u.covered += cnt;
                u.cov_raw += (cnt - 1) * c.full + (b == c.n - 1 ? raw - b * c.full : c.full);
                u.k_hi = b;
                next = b + 1;
            }
        }
        if (recs) recs[i] = rec;
    }
    return u;
}
// hc_seg_decompress_ranges_work_bound without the adaptive workspace (P reads, C covered segments
// of W raw bytes): the records, the three gather arrays, the covered entries' segment and five
// decoder arrays, the status (and crc) words, 16 of control words and the staging region.
inline uint64_t reads_work_base(uint64_t P, uint64_t C, uint64_t W, bool check)
{
    if (W > ~0ull - 15) return ~0ull;
    const uint64_t t = align16(sizeof(ReadRec) * P) + 3 * align16(8 * P) + 6 * align16(8 * C) + align16(4 * C) +
                       (check ? align16(4 * C) : 0) + 16;
    return sat_add(t, align16(W));
}
// hc_seg_rect_reads after its null check: row r of the rectangle is bytes [(y + r) pitch + x, + w).
// rect_ok: the argument rules alone.
inline bool rect_ok(uint64_t raw_len, uint64_t pitch, uint64_t x, uint64_t y, uint64_t w, uint64_t h)
{
    if (pitch == 0 || x + w < x || x + w > pitch) return false;
    if (h) {
        // the last row's end, (y + h - 1) pitch + x + w, and the last destination's, h w, without a wrap
        const uint64_t row = y + (h - 1);
        if (row < y || row > ~0ull / pitch || row * pitch > ~0ull - (x + w) || (w && h > ~0ull / w)) return false;
        if (w && row * pitch + x + w > raw_len) return false;
    }
    return true;
}
inline bool rect_reads(uint64_t raw_len, uint64_t pitch, uint64_t x, uint64_t y, uint64_t w, uint64_t h,
                       hc_seg_read_t *reads)
{
    if (!rect_ok(raw_len, pitch, x, y, w, h)) return false;
    for (uint64_t r = 0; r < h; ++r) reads[r] = hc_seg_read_t{(y + r) * pitch + x, w, r * w};
    return true;
}

// ---------------------------------------------------------------------------------------------
// Append (hc_seg_append*): the host's plan of raw bytes added behind a container. The cuts of
// raw + add agree with the old ones on every segment below the old last one, and on that one too
// when it already had the shape of a cut that is not the last. Segments 0 .. K - 1 are kept; the
// coded segments K .. n' - 1 hold raw bytes [K full, raw + add): the open tail [K full, raw), then
// the added bytes. Coded entry c (segment K + c) has its raw bytes at c full of a staging region.
// ---------------------------------------------------------------------------------------------
inline uint64_t sat_mul(uint64_t a, uint64_t b) { return b && a > ~0ull / b ? ~0ull : a * b; }
struct AppPlan {
    Cuts nc;            // the cuts of raw + add (full is the old one)
    uint64_t K, coded;  // the first coded segment; n' - K
    uint64_t decoded;   // 1: old segment n - 1 is decoded first (K == n - 1 and it is not empty)
    uint64_t tail;      // the open tail's bytes: raw - K full, and none when K == n
    uint64_t stage;     // tail + add: the raw bytes of the coded segments
};
// c: the cuts of raw (from info_ok). HC_OK, HC_ERR_ARG (raw + add wraps) or HC_ERR_MATRIX_SIZE (an
// adaptive container and add is no multiple of width).
inline int append_plan(const Cuts &c, uint64_t raw, uint64_t add, uint64_t seg, bool adapt, uint64_t width, AppPlan *p)
{
    memset(p, 0, sizeof(*p));
    if (raw + add < raw) return HC_ERR_ARG;
    if (adapt && add % width != 0) return HC_ERR_MATRIX_SIZE;
    p->nc = seg_cuts(raw + add, seg, adapt, width);  // valid: raw's cuts are, and rows are only added
    // n' >= n. Old cut n - 1 is new cut n - 1 when the new one is no longer the last and the old
    // one was a full cut; with n' == n the last cut grew by add.
    p->K = (add == 0 || (p->nc.n > c.n && c.last == c.full)) ? c.n : c.n - 1;
    p->coded = p->nc.n - p->K;
    p->decoded = (p->K == c.n - 1 && c.last > 0) ? 1 : 0;
    p->tail = p->K == c.n ? 0 : raw - p->K * c.full;  // (K == n: empty, and with add == 0 n full may pass raw)
    p->stage = p->tail + add;
    return HC_OK;
}
// the length of coded entry e's cut
inline uint64_t append_cut(const AppPlan &p, uint64_t e) { return e == p.coded - 1 ? p.nc.last : p.nc.full; }
// S: the sum of align16(bound(cut)) over the coded segments. bound_full, bound_last:
// align16(hc_compress_bound) of a full cut and of the new last one.
inline uint64_t append_slots(const AppPlan &p, uint64_t bound_full, uint64_t bound_last)
{
    return p.coded ? sat_add(sat_mul(p.coded - 1, bound_full), bound_last) : 0;
}
// hc_seg_append_bound: in_len, the index's growth, the kept block's padding, the slots
inline uint64_t append_bound(const AppPlan &p, uint64_t in_len, uint64_t old_n, bool check, uint64_t slots)
{
    const uint64_t grow = align16(sat_mul(check ? 12 : 8, p.nc.n - old_n));
    return sat_add(sat_add(in_len, grow), sat_add(16, slots));
}
// hc_seg_append_work_bound without the adaptive workspace (C = coded): 9 arrays of 8 C bytes, the
// status (and crc) words, 2 C + 1 copy pieces, the one decoder entry (96 bytes; checked: 112), 64 of
// control words, the staging region and the slots. For C <= 2^31 - 1 (the calls refuse more).
inline uint64_t append_work_base(const AppPlan &p, bool check, uint64_t slots)
{
    const uint64_t C = p.coded;
    if (p.stage > ~0ull - 15) return ~0ull;
    uint64_t t = 9 * align16(8 * C) + align16(4 * C) + (check ? align16(4 * C) : 0) + 3 * align16(8 * (2 * C + 1));
    t += (check ? 112 : 96) + 64;
    return sat_add(sat_add(t, align16(p.stage)), slots);
}

}  // namespace hc_seg_index
