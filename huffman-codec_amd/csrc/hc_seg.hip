// hc_seg.hip — the segmented container (HCSEG1, include/hcodec.h): one large input cut into
// independent segments that the existing batch launches code side by side.
//
// Nothing here codes a byte: the FGK and adaptive batch launchers (launch_encode, launch_decode,
// adapt_encode_batch, adapt_decode_batch) do, unchanged. This file is the glue that turns one
// buffer into a batch and back:
//
//   encode  seg_plan    per-segment in_offs / in_lens / widths and a bound-sized output slot
//           <checked containers: CRC-32 of every segment's raw bytes (hc_crc.hip), into work>
//           <encode launch over the n segments>
//           seg_seal    one workgroup: scan of align16(enc_len) with a carried prefix, first
//                       failing segment, capacity check, header and index
//           seg_gather  slots -> their final places, 16 bytes per lane, zeroed padding
//   decode  seg_open    one workgroup: header against the caller's host copy, index scan
//                       (overflow-safe), segment arrays pointing straight into the output
//           <decode launch: segments decode in place>
//           <checked containers: CRC-32 of every cleanly decoded segment, in place in out>
//           seg_close   status (a checksum that differs from the index fails its segment),
//                       bad_segment, out_len
//   range   the same launches over the segments that hold a byte range alone (the whole decoder
//           is the range (0, raw_len)): seg_open still scans the whole index, but writes arrays
//           for the covered segments only; one that the range covers in part, or any at an offset
//           that is no multiple of 4, decodes into a slot of the workspace, and a pack launch
//           (hc_pipe.hip) moves its covered part to its place in out before seg_close
//
// Every launch is asynchronous on the caller's stream; no allocation, no host synchronisation,
// no host read of device memory in the device entry points. A container-level error zeroes
// every in_lens, which the coders answer with HC_ERR_HEADER before touching anything.
#include <stdlib.h>
#include <string.h>

#include "hc_internal.h"
#include "hc_seg_index.h"

namespace {

using hc::Batch;
using hc::DevBuf;

constexpr uint64_t kNoSeg = ~0ull;
constexpr uint32_t kScan = 1024;  // threads of the one-workgroup kernels = entries per scan tile
constexpr uint64_t kMaxSegs = 0x7FFFFFFFull;  // Batch::n is 32 bits
using hc_seg_index::kMagic;

#define HC_CK(x)                                     \
    do {                                             \
        if ((x) != hipSuccess) return HC_ERR_DEVICE; \
    } while (0)

__host__ __device__ inline uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }
__host__ __device__ inline uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
__host__ __device__ inline uint64_t index_end(uint64_t n, bool check) { return 48 + (check ? 12 : 8) * n; }

// the host's rules (the cut rule, the header rules, the covered segments, the host index scan)
using hc_seg_index::checked;
using hc_seg_index::Cover;
using hc_seg_index::Cuts;
using hc_seg_index::get64;
using hc_seg_index::info_ok;
using hc_seg_index::kSegFlags;
using hc_seg_index::range_cover;
using hc_seg_index::range_ok;
using hc_seg_index::seg_cuts;

// the 48 header bytes as six little-endian words (what the device holds at in / out + 0..47)
struct Header {
    uint64_t w[6];
};
Header make_header(uint32_t flags, uint64_t raw_len, uint64_t seg_bytes, uint64_t width, uint64_t n)
{
    Header h;
    h.w[0] = get64(kMagic);
    h.w[1] = flags & 0xFFFFu;  // byte 8 the flags, byte 9 the check kind
    h.w[2] = raw_len;
    h.w[3] = seg_bytes;
    h.w[4] = width;
    h.w[5] = n;
    return h;
}

// ---------------------------------------------------------------------------------------------
// Workspace layouts (host-side carving; every region 16-byte aligned)
// ---------------------------------------------------------------------------------------------
struct EncWs {
    uint64_t *in_offs, *in_lens, *widths, *out_offs, *out_caps, *out_lens, *dst_offs;
    int32_t *status;
    uint32_t *crc;   // checked containers: the segments' CRC-32 (otherwise no bytes)
    uint64_t *ctl;   // [0] 1: sealed, the gather may copy
    uint8_t *slots;  // the segments' bound-sized output slots
    void *awork;     // the adaptive batch workspace
    uint64_t awork_bytes, total;
};
EncWs carve_enc(void *work, uint64_t n, uint64_t slot_bytes, uint64_t awork_bytes, bool check)
{
    EncWs w;
    uint8_t *p = static_cast<uint8_t *>(work);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) {
        uint8_t *q = p ? p + o : nullptr;  // null: sizing only
        o += align16(bytes);
        return q;
    };
    w.in_offs = reinterpret_cast<uint64_t *>(take(8 * n));
    w.in_lens = reinterpret_cast<uint64_t *>(take(8 * n));
    w.widths = reinterpret_cast<uint64_t *>(take(8 * n));
    w.out_offs = reinterpret_cast<uint64_t *>(take(8 * n));
    w.out_caps = reinterpret_cast<uint64_t *>(take(8 * n));
    w.out_lens = reinterpret_cast<uint64_t *>(take(8 * n));
    w.dst_offs = reinterpret_cast<uint64_t *>(take(8 * n));
    w.status = reinterpret_cast<int32_t *>(take(4 * n));
    w.crc = reinterpret_cast<uint32_t *>(take(check ? 4 * n : 0));
    w.ctl = reinterpret_cast<uint64_t *>(take(16));
    w.slots = take(slot_bytes);
    w.awork = take(awork_bytes);
    w.awork_bytes = awork_bytes;
    w.total = o;
    return w;
}

// ---------------------------------------------------------------------------------------------
// Kernels
// ---------------------------------------------------------------------------------------------

// Exclusive scan of v over the workgroup's kScan threads under sat_add (associative on
// unsigned values, identity 0); `total` is the whole tile's sum. part: 16 words of LDS.
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t *part, uint64_t &total)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up((unsigned long long)inc, d, 64);
        if (lane >= d) inc = sat_add(o, inc);
    }
    uint64_t excl = __shfl_up((unsigned long long)inc, 1, 64);
    if (lane == 0) excl = 0;
    __syncthreads();  // the tile before is done with part[]
    if (lane == 63) part[wv] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScan / 64; ++k) {
        const uint64_t pk = part[k];
        if (k < wv) before = sat_add(before, pk);
        all = sat_add(all, pk);
    }
    total = all;
    return sat_add(before, excl);
}

struct PlanArgs {
    uint64_t *in_offs, *in_lens, *widths, *out_offs, *out_caps, *out_lens;
    int32_t *status;
    uint64_t n, full, last, slot_full, cap_full, cap_last, width;
};

// segment k's input range and its output slot (all in closed form: only the last segment differs)
__global__ __launch_bounds__(256) void seg_plan_kernel(PlanArgs a)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.n) return;
    const bool tail = k == a.n - 1;
    a.in_offs[k] = k * a.full;
    a.in_lens[k] = tail ? a.last : a.full;
    a.widths[k] = a.width;
    a.out_offs[k] = k * a.slot_full;
    a.out_caps[k] = tail ? a.cap_last : a.cap_full;
    a.out_lens[k] = 0;
    a.status[k] = HC_ERR_DEVICE;  // every segment is coded by exactly one launch, which overwrites this
}

struct SealArgs {
    const uint64_t *enc_lens;
    const int32_t *seg_status;
    const uint32_t *crc;  // null: an unchecked container
    uint64_t *dst_offs, *ctl;
    uint64_t n;
    uint8_t *out;
    uint64_t out_cap;
    uint64_t *out_len;
    int32_t *status;
    Header hdr;
};

__global__ __launch_bounds__(kScan) void seg_seal_kernel(SealArgs a)
{
    __shared__ uint64_t part[kScan / 64];
    __shared__ unsigned long long s_bad, s_end;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        s_bad = kNoSeg;
        s_end = 0;
    }
    __syncthreads();
    const uint64_t idx_end = index_end(a.n, a.crc != nullptr);
    uint64_t carry = align16(idx_end);  // where segment 0 starts
    uint64_t bad = kNoSeg;
    for (uint64_t base = 0; base < a.n; base += kScan) {
        const uint64_t k = base + tid;
        const bool in = k < a.n;
        const uint64_t len = in ? a.enc_lens[k] : 0;
        if (in && a.seg_status[k] != 0 && bad == kNoSeg) bad = k;
        uint64_t total;
        const uint64_t off = sat_add(carry, block_scan(in ? align16(len) : 0, part, total));
        if (in) a.dst_offs[k] = off;
        if (in && k == a.n - 1) s_end = sat_add(off, len);  // no padding after the last segment
        carry = sat_add(carry, total);
    }
    if (bad != kNoSeg) atomicMin(&s_bad, (unsigned long long)bad);
    __syncthreads();
    const uint64_t first_bad = s_bad, end = s_end;
    int32_t st = 0;
    if (first_bad != kNoSeg) st = a.seg_status[first_bad];
    else if (end > a.out_cap) st = HC_ERR_CAPACITY;
    if (tid == 0) {
        *a.status = st;
        *a.out_len = (st == 0 || st == HC_ERR_CAPACITY) ? end : 0;
        a.ctl[0] = st == 0 ? 1 : 0;
    }
    if (st != 0) return;
    // sealed: end <= out_cap, so the header, the index and its padding lie inside out
    uint64_t *o64 = reinterpret_cast<uint64_t *>(a.out);
    uint32_t *o32 = reinterpret_cast<uint32_t *>(a.out);
    if (tid < 6) o64[tid] = a.hdr.w[tid];
    // the index ends on a multiple of 4: zero words up to segment 0
    if (tid >= 8 && tid < 8 + (align16(idx_end) - idx_end) / 4) o32[idx_end / 4 + (tid - 8)] = 0;
    for (uint64_t k = tid; k < a.n; k += kScan) o64[6 + k] = a.enc_lens[k];
    if (a.crc)
        for (uint64_t k = tid; k < a.n; k += kScan) o32[12 + 2 * a.n + k] = a.crc[k];
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Slot k -> out + dst_offs[k], one workgroup per segment. Both ends are 16-byte aligned, so whole
// 16-byte chunks per lane; the chunk that holds the stream's last bytes goes out with its
// padding zeroed, except the last segment's (the container ends with its last byte: bytes).
__global__ __launch_bounds__(256) void seg_gather_kernel(const uint8_t *slots, const uint64_t *slot_offs,
                                                         const uint64_t *enc_lens, const uint64_t *dst_offs,
                                                         const uint64_t *ctl, uint64_t n, uint8_t *out)
{
    if (ctl[0] == 0) return;  // not sealed: nothing is copied
    for (uint64_t k = blockIdx.x; k < n; k += gridDim.x) {
        const uint64_t len = enc_lens[k];
        const u32x4 *src = reinterpret_cast<const u32x4 *>(slots + slot_offs[k]);
        u32x4 *dst = reinterpret_cast<u32x4 *>(out + dst_offs[k]);
        const uint64_t chunks = len / 16;
        for (uint64_t c = threadIdx.x; c < chunks; c += 256) dst[c] = src[c];
        const uint32_t rem = (uint32_t)(len & 15u);
        if (rem == 0 || threadIdx.x != 255) continue;
        if (k == n - 1) {
            const uint8_t *s8 = reinterpret_cast<const uint8_t *>(src + chunks);
            uint8_t *d8 = reinterpret_cast<uint8_t *>(dst + chunks);
            for (uint32_t b = 0; b < rem; ++b) d8[b] = s8[b];
        } else {
            u32x4 v = src[chunks];  // inside the slot: slots are multiples of 16 bytes
            uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t d = 0; d < 4; ++d) {
                if (rem <= 4 * d) w[d] = 0;
                else if (rem < 4 * d + 4) w[d] &= (1u << (8 * (rem - 4 * d))) - 1u;
            }
            v.x = w[0];
            v.y = w[1];
            v.z = w[2];
            v.w = w[3];
            dst[chunks] = v;
        }
    }
}

// hc_seg_decompress_dev with an info that fails the host checks: the verdict alone
__global__ void seg_reject_kernel(uint64_t *out_len, int32_t *status, uint64_t *bad_segment)
{
    *status = HC_ERR_SEG_HEADER;
    *out_len = 0;
    if (bad_segment) *bad_segment = kNoSeg;
}

// ---------------------------------------------------------------------------------------------
// Decode: raw bytes [offset, offset + length) of the container; the whole decoder is the range
// (0, raw_len) over every segment. The covered segments k0 .. k0 + count - 1 go through one decode
// launch. One that lies wholly inside the range decodes in place in out when offset is a multiple
// of 4 (every cut starts on one, and the coders need a 4-byte aligned output); every other one is
// staged: it decodes whole into a slot of the workspace, and a pack launch moves its covered part
// to out at any byte alignment. The slots of an aligned range: one for segment k0 when the range
// starts inside it, then one for the last covered segment when the range ends inside it (none for
// the whole decoder); of an unaligned range: slot s for segment k0 + s.
// ---------------------------------------------------------------------------------------------
struct DecWs {
    uint64_t *in_offs, *in_lens, *out_offs, *out_caps, *out_lens;
    int32_t *status;
    uint32_t *crc;  // checked containers: the decoded segments' CRC-32 (otherwise no bytes)
    uint64_t *ctl;  // [0] the container-level status (0, HC_ERR_SEG_HEADER, HC_ERR_CAPACITY)
    uint64_t *cp_src, *cp_len, *cp_dst;  // slot s: cp_len[s] bytes from slots + cp_src[s] to out + cp_dst[s]
    uint8_t *slots;
    void *awork;
    uint64_t awork_bytes, total;
};
DecWs carve_dec(void *work, uint64_t count, uint64_t nslots, uint64_t slot, uint64_t awork_bytes, bool check)
{
    DecWs w;
    uint8_t *p = static_cast<uint8_t *>(work);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) {
        uint8_t *q = p ? p + o : nullptr;  // null: sizing only
        o += align16(bytes);
        return q;
    };
    w.in_offs = reinterpret_cast<uint64_t *>(take(8 * count));
    w.in_lens = reinterpret_cast<uint64_t *>(take(8 * count));
    w.out_offs = reinterpret_cast<uint64_t *>(take(8 * count));
    w.out_caps = reinterpret_cast<uint64_t *>(take(8 * count));
    w.out_lens = reinterpret_cast<uint64_t *>(take(8 * count));
    w.status = reinterpret_cast<int32_t *>(take(4 * count));
    w.crc = reinterpret_cast<uint32_t *>(take(check ? 4 * count : 0));
    w.ctl = reinterpret_cast<uint64_t *>(take(16));
    w.cp_src = reinterpret_cast<uint64_t *>(take(8 * nslots));
    w.cp_len = reinterpret_cast<uint64_t *>(take(8 * nslots));
    w.cp_dst = reinterpret_cast<uint64_t *>(take(8 * nslots));
    w.slots = take(nslots * slot);
    w.awork = take(awork_bytes);
    w.awork_bytes = awork_bytes;
    w.total = o;
    return w;
}

// the sizes of a range inside raw_len; whole: the range (0, raw_len) over all n segments (an empty
// container's one empty segment included, which the empty range would not cover)
struct DecPlan {
    Cover cv;
    uint64_t nslots, slot, raw;  // staging slots, bytes of each, raw bytes of the covered segments
};
DecPlan dec_plan(const Cuts &c, uint64_t offset, uint64_t length, bool whole)
{
    DecPlan p;
    p.cv = whole ? Cover{0, c.n} : range_cover(c, offset, length);
    p.slot = align16(c.full > c.last ? c.full : c.last);
    p.nslots = p.raw = 0;
    if (p.cv.count == 0) return p;
    const uint64_t k1 = p.cv.k0 + p.cv.count - 1;
    p.raw = (p.cv.count - 1) * c.full + (k1 == c.n - 1 ? c.last : c.full);
    if (offset & 3u) {
        p.nslots = p.cv.count;
    } else {
        const bool head = offset != p.cv.k0 * c.full, tail = offset + length != p.cv.k0 * c.full + p.raw;
        p.nslots = p.cv.count == 1 ? (head || tail) : (uint64_t)head + tail;
    }
    return p;
}

struct OpenArgs {
    const uint8_t *in;
    uint64_t in_len, skip;  // skip: what the covered segments' input offsets lose (a compact upload)
    Header hdr;             // the caller's host copy (checked on the host already)
    uint64_t n, full, last, offset, length, out_cap;
    uint64_t k0, count, nslots, slot;
    uint64_t out_d, slot_d;  // out and the slots from the batch's output base
    uint64_t *in_offs, *in_lens, *out_offs, *out_caps, *out_lens;
    uint64_t *cp_src, *cp_len, *cp_dst;
    int32_t *status;
    uint64_t *ctl;
    bool check;
};

// The host has checked its copy of the header against in_len (48 + 8 n <= in_len among the rest;
// 12 n in a checked container, whose crc words follow the lengths); here the device bytes must
// equal that copy, and the index must tile [align16(48 + 8 n or 12 n), in_len) exactly, whatever
// the range. enc_len entries are untrusted: the offsets add with saturation and every range is
// compared by subtraction, so a forged length cannot wrap into a valid offset. Segment arrays for
// the covered segments only (entry k - k0), and the staged ones' copies.
__global__ __launch_bounds__(kScan) void seg_open_kernel(OpenArgs a)
{
    __shared__ uint64_t part[kScan / 64];
    __shared__ uint32_t s_err;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_err = 0;
    for (uint64_t s = tid; s < a.nslots; s += kScan) a.cp_len[s] = 0;  // a slot nothing is staged in
    __syncthreads();
    bool err = false;
    const uint64_t *i64 = reinterpret_cast<const uint64_t *>(a.in);
    if (tid < 6 && i64[tid] != a.hdr.w[tid]) err = true;
    const uint64_t end = a.offset + a.length;  // (inside raw_len: the host's check)
    const bool all_staged = (a.offset & 3u) != 0;
    const uint64_t tail_slot = a.offset != a.k0 * a.full;  // aligned: after segment k0's slot, if it has one
    uint64_t carry = align16(index_end(a.n, a.check));
    for (uint64_t base = 0; base < a.n; base += kScan) {
        const uint64_t k = base + tid;
        const bool in = k < a.n;
        const uint64_t len = in ? i64[6 + k] : 0;
        const bool big = len > a.in_len;
        uint64_t total;
        const uint64_t off = sat_add(carry, block_scan(in && !big ? align16(len) : 0, part, total));
        if (in) {
            const bool tail = k == a.n - 1;
            if (big || off > a.in_len || len > a.in_len - off) err = true;
            else if (tail && off + len != a.in_len) err = true;  // truncated, or trailing bytes
        }
        if (in && k >= a.k0 && k - a.k0 < a.count) {
            const uint64_t i = k - a.k0;
            const uint64_t b = k * a.full, cap = k == a.n - 1 ? a.last : a.full, e = b + cap;
            const uint64_t lo = b > a.offset ? b : a.offset, hi = e < end ? e : end;
            a.in_offs[i] = off - a.skip;  // (a wrapped value is never read: err zeroes in_lens)
            a.in_lens[i] = len;
            a.out_caps[i] = cap;
            a.out_lens[i] = 0;
            a.status[i] = HC_ERR_DEVICE;  // overwritten by the launch that owns the segment
            if (all_staged || lo != b || hi != e) {
                const uint64_t s = all_staged ? i : (i == 0 ? 0 : tail_slot);
                a.out_offs[i] = a.slot_d + s * a.slot;
                a.cp_src[s] = s * a.slot + (lo - b);
                a.cp_len[s] = hi - lo;
                a.cp_dst[s] = lo - a.offset;
            } else {
                a.out_offs[i] = a.out_d + (b - a.offset);
            }
        }
        carry = sat_add(carry, total);
    }
    if (err) s_err = 1;
    __syncthreads();
    const int32_t st = s_err ? HC_ERR_SEG_HEADER : (a.length > a.out_cap ? HC_ERR_CAPACITY : 0);
    if (tid == 0) a.ctl[0] = (uint64_t)st;
    if (st == 0) return;
    // nothing may be decoded or copied: empty inputs, which the coders answer with HC_ERR_HEADER
    // before they touch anything, and empty copies
    for (uint64_t i = tid; i < a.count; i += kScan) a.in_lens[i] = 0;
    for (uint64_t s = tid; s < a.nslots; s += kScan) a.cp_len[s] = 0;
}

struct CloseArgs {
    const uint64_t *out_lens, *out_caps, *ctl;
    const int32_t *seg_status;
    const uint32_t *crc, *want_crc;  // checked containers: of the decoded bytes, and the index's from k0 (else null)
    uint64_t k0, count, length;
    uint64_t *out_len, *bad_segment;
    int32_t *status;
};

// the verdict over the covered segments; bad_segment is the container's index
__global__ __launch_bounds__(kScan) void seg_close_kernel(CloseArgs a)
{
    __shared__ unsigned long long s_bad;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_bad = kNoSeg;
    __syncthreads();
    const int32_t top = (int32_t)a.ctl[0];
    if (top == 0) {
        // the lowest segment that failed, decoded cleanly to another length than its cut, or to
        // that length with another checksum (crc[i] is written exactly for those that reach it)
        uint64_t bad = kNoSeg;
        for (uint64_t i = tid; i < a.count && bad == kNoSeg; i += kScan)
            if (a.seg_status[i] != 0 || a.out_lens[i] != a.out_caps[i] || (a.crc && a.crc[i] != a.want_crc[i]))
                bad = i;
        if (bad != kNoSeg) atomicMin(&s_bad, (unsigned long long)bad);
    }
    __syncthreads();
    if (tid != 0) return;
    const uint64_t bad = s_bad;
    int32_t st = top;
    uint64_t len = top == HC_ERR_CAPACITY ? a.length : 0;
    if (top == 0) {
        if (bad != kNoSeg) {
            st = a.seg_status[bad];
            // 64: it wanted more room than its cut; 0: it decoded to fewer bytes, or to the wrong ones
            if (st == 0 && a.out_lens[bad] == a.out_caps[bad]) st = HC_ERR_SEG_CHECK;
            else if (st == 0 || st == HC_ERR_CAPACITY) st = HC_ERR_SEG_SIZE;
        } else {
            len = a.length;
        }
    }
    *a.status = st;
    *a.out_len = len;
    if (a.bad_segment) *a.bad_segment = bad == kNoSeg ? kNoSeg : a.k0 + bad;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the encoder's sizes for valid arguments
struct EncPlan {
    Cuts c;
    uint64_t cap_full, cap_last, slot_full, slot_bytes, awork_bytes;
};
bool enc_plan(uint64_t in_len, uint64_t seg_bytes, int use_adapt, uint64_t width, EncPlan &p)
{
    p.c = seg_cuts(in_len, seg_bytes ? seg_bytes : HC_SEG_DEFAULT_BYTES, use_adapt != 0, width);
    if (p.c.n == 0 || p.c.n > kMaxSegs) return false;
    p.cap_full = hc_compress_bound(p.c.full, use_adapt);
    p.cap_last = hc_compress_bound(p.c.last, use_adapt);
    p.slot_full = align16(p.cap_full);
    p.slot_bytes = (p.c.n - 1) * p.slot_full + align16(p.cap_last);
    p.awork_bytes = use_adapt ? hc::adapt_encode_work_bound(in_len, (uint32_t)p.c.n) : 0;
    return true;
}

// hc_compress's host-decided statuses, in its order (main.cpp:195-199, 54-58; transform.cpp:300-304)
int host_status(uint64_t n, int use_adapt, uint64_t width)
{
    if (width == 0) return HC_ERR_WIDTH;
    if (use_adapt && n % width != 0) return HC_ERR_MATRIX_SIZE;
    if (use_adapt && (width < 8 || n / width < 8)) return HC_ERR_DIMS;
    return HC_OK;
}

int seg_decompress_host(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap, bool alloc,
                        uint8_t **out_alloc, uint64_t *out_len, uint64_t *bad_segment)
{
    if (bad_segment) *bad_segment = kNoSeg;
    *out_len = 0;
    hc_seg_info_t info;
    if (hc_seg_info(in, in_len, &info) != HC_OK) return HC_ERR_SEG_HEADER;
    if (!hc_device_ok()) return HC_ERR_DEVICE;
    if (alloc) out_cap = info.raw_len;
    hipStream_t st = nullptr;
    const uint64_t room = out_cap < info.raw_len ? out_cap : info.raw_len;  // never more than raw_len is written
    const uint64_t wb = hc_seg_decompress_work_bound(&info, in_len);
    DevBuf din, dout, work, meta;
    HC_CK(din.alloc(in_len + 16));
    HC_CK(dout.alloc(room + 16));
    HC_CK(work.alloc(wb));
    HC_CK(meta.alloc(32));
    HC_CK(hipMemcpyAsync(din.p, in, in_len, hipMemcpyHostToDevice, st));
    uint64_t *m = meta.as<uint64_t>();
    const int rc = hc_seg_decompress_dev(din.as<uint8_t>(), in_len, &info, dout.as<uint8_t>(), out_cap, m,
                                         reinterpret_cast<int32_t *>(m + 1), m + 2, work.p, wb, st);
    if (rc) return rc;
    uint64_t h[4] = {0, 0, 0, 0};
    HC_CK(hipMemcpyAsync(h, meta.p, sizeof(h), hipMemcpyDeviceToHost, st));
    HC_CK(hipStreamSynchronize(st));
    const int status = (int32_t)(uint32_t)h[1];
    *out_len = h[0];
    if (bad_segment) *bad_segment = h[2];
    if (status) return status;
    if (alloc) {
        out = static_cast<uint8_t *>(malloc(h[0] ? h[0] : 1));
        if (!out) return HC_ERR_DEVICE;
        *out_alloc = out;
    }
    if (h[0]) HC_CK(hipMemcpy(out, dout.p, h[0], hipMemcpyDeviceToHost));
    return HC_OK;
}

// hc_seg_compress / hc_seg_compress2 after their own argument checks
int seg_compress_host(const uint8_t *in, uint64_t in_len, uint32_t flags, uint64_t width, uint64_t seg_bytes,
                      uint8_t *out, uint64_t out_cap, uint64_t *out_len)
{
    if (seg_bytes & 15u) return HC_ERR_ARG;
    const int use_adapt = (flags & HC_FLAG_ADAPT) ? 1 : 0;
    const int hs = host_status(in_len, use_adapt, width);
    if (hs) return hs;
    if (!hc_device_ok()) return HC_ERR_DEVICE;
    const uint64_t cap = hc_seg_compress_bound2(in_len, seg_bytes, flags, width);
    const uint64_t wb = hc_seg_compress_work_bound2(in_len, seg_bytes, flags, width);
    if (cap == 0 || wb == 0) return HC_ERR_ARG;
    hipStream_t st = nullptr;
    DevBuf din, dout, work, meta;
    HC_CK(din.alloc(in_len + 16));
    HC_CK(dout.alloc(cap));
    HC_CK(work.alloc(wb));
    HC_CK(meta.alloc(32));
    if (in_len) HC_CK(hipMemcpyAsync(din.p, in, in_len, hipMemcpyHostToDevice, st));
    uint64_t *m = meta.as<uint64_t>();
    const int rc = hc_seg_compress_dev(din.as<uint8_t>(), in_len, flags, width, seg_bytes, dout.as<uint8_t>(), cap, m,
                                       reinterpret_cast<int32_t *>(m + 1), work.p, wb, st);
    if (rc) return rc;
    uint64_t h[2] = {0, 0};
    HC_CK(hipMemcpyAsync(h, meta.p, sizeof(h), hipMemcpyDeviceToHost, st));
    HC_CK(hipStreamSynchronize(st));
    const int status = (int32_t)(uint32_t)h[1];
    if (status) return status;
    *out_len = h[0];
    if (h[0] > out_cap) return HC_ERR_CAPACITY;
    HC_CK(hipMemcpy(out, dout.p, h[0], hipMemcpyDeviceToHost));
    return HC_OK;
}

// the workspace of a range inside raw_len of a container whose info passed; enc_total: an upper
// bound of the covered segments' encoded bytes (the adaptive batch workspace grows with it)
DecWs dec_ws(void *work, const hc_seg_info_t &info, const Cuts &c, uint64_t offset, uint64_t length, bool whole,
             uint64_t enc_total, DecPlan &p)
{
    p = dec_plan(c, offset, length, whole);
    const uint64_t aw = ((info.flags & HC_FLAG_ADAPT) && p.cv.count)
                            ? hc::adapt_decode_work_bound(enc_total, p.raw, (uint32_t)p.cv.count)
                            : 0;
    return carve_dec(work, p.cv.count, p.nslots, p.slot, aw, checked(info.flags));
}

// hc_seg_decompress_dev (whole: the range (0, raw_len) over every segment) and
// hc_seg_decompress_range_dev; the host range call passes its compact upload's skip and span
int decode_dev(const uint8_t *in, uint64_t in_len, const hc_seg_info_t *info, uint64_t offset, uint64_t length,
               bool whole, uint8_t *out, uint64_t out_cap, uint64_t *out_len, int32_t *status, uint64_t *bad_segment,
               void *work, uint64_t work_bytes, void *stream, uint64_t skip, uint64_t enc_total)
{
    if (!in || !info || !out || !out_len || !status || !work) return HC_ERR_ARG;
    if (!aligned16(in) || !aligned16(out) || !aligned16(work)) return HC_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Cuts c;
    if (!info_ok(*info, in_len, c)) {
        seg_reject_kernel<<<1, 1, 0, st>>>(out_len, status, bad_segment);
        HC_CK(hipGetLastError());
        return HC_OK;
    }
    if (whole) length = info->raw_len;
    else if (!range_ok(info->raw_len, offset, length)) return HC_ERR_ARG;
    if (c.n > kMaxSegs) return HC_ERR_ARG;
    const bool adapt = (info->flags & HC_FLAG_ADAPT) != 0;
    const bool check = checked(info->flags);
    DecPlan p;
    const DecWs w = dec_ws(work, *info, c, offset, length, whole, enc_total, p);
    if (work_bytes < w.total) return HC_ERR_ARG;
    const uint32_t count = (uint32_t)p.cv.count;

    // one output base for the batch: whichever of out and the slots lies lower
    uint8_t *base = (p.nslots && w.slots < out) ? w.slots : out;
    const OpenArgs oa{in, in_len, skip, make_header(info->flags, info->raw_len, info->seg_bytes, info->width, c.n),
                      c.n, c.full, c.last, offset, length, out_cap,
                      p.cv.k0, p.cv.count, p.nslots, p.slot,
                      (uint64_t)(out - base), p.nslots ? (uint64_t)(w.slots - base) : 0,
                      w.in_offs, w.in_lens, w.out_offs, w.out_caps, w.out_lens,
                      w.cp_src, w.cp_len, w.cp_dst, w.status, w.ctl, check};
    seg_open_kernel<<<1, kScan, 0, st>>>(oa);
    HC_CK(hipGetLastError());
    if (count) {
        Batch b{in, w.in_offs, w.in_lens, count, base, w.out_offs, w.out_caps, w.out_lens, w.status, 0};
        if (adapt) HC_CK(hc::adapt_decode_batch(b, w.awork, w.awork_bytes, st));
        else HC_CK(hc::launch_decode(b, hc::DST_RAW, st));
        // segments that decoded cleanly to their cut's length, staged or in place (every covered
        // one decodes whole, so its checksum is verifiable); none when the verdict is set
        if (check)
            HC_CK(hc::launch_crc32(base, w.out_offs, w.out_caps, count, w.crc, hc::CrcGate{w.ctl, w.status, w.out_lens}, st));
    }
    // the staged segments' covered parts to their places in out (empty copies when the verdict is set)
    if (p.nslots) HC_CK(hc::launch_pack(w.slots, w.cp_src, w.cp_len, (uint32_t)p.nslots, out, w.cp_dst, st));
    const CloseArgs ca{w.out_lens, w.out_caps, w.ctl, w.status, check ? w.crc : nullptr,
                       check ? reinterpret_cast<const uint32_t *>(in + 48 + 8 * c.n) + p.cv.k0 : nullptr,
                       p.cv.k0, p.cv.count, length, out_len, bad_segment, status};
    seg_close_kernel<<<1, kScan, 0, st>>>(ca);
    HC_CK(hipGetLastError());
    return HC_OK;
}

}  // namespace

extern "C" {

uint64_t hc_seg_count(uint64_t in_len, uint64_t seg_bytes, int use_adapt, uint64_t width)
{
    return seg_cuts(in_len, seg_bytes ? seg_bytes : HC_SEG_DEFAULT_BYTES, use_adapt != 0, width).n;
}

uint64_t hc_seg_compress_bound(uint64_t in_len, uint64_t seg_bytes, int use_adapt, uint64_t width)
{
    return hc_seg_compress_bound2(in_len, seg_bytes, use_adapt ? HC_FLAG_ADAPT : 0u, width);
}

uint64_t hc_seg_compress_bound2(uint64_t in_len, uint64_t seg_bytes, uint32_t flags, uint64_t width)
{
    EncPlan p;
    if ((flags & ~kSegFlags) || !enc_plan(in_len, seg_bytes, (flags & HC_FLAG_ADAPT) != 0, width, p)) return 0;
    return align16(index_end(p.c.n, checked(flags))) + p.slot_bytes;
}

int hc_seg_info(const uint8_t *in, uint64_t in_len, hc_seg_info_t *info)
{
    if (!info) return HC_ERR_ARG;
    return hc_seg_index::parse_header(in, in_len, info);
}

uint64_t hc_seg_compress_work_bound(uint64_t in_len, uint64_t seg_bytes, int use_adapt, uint64_t width)
{
    // The segments are coded into slots of hc_compress_bound(segment) bytes each, the same
    // worst case every batch caller sizes by, and gathered afterwards: nothing is guessed and
    // retried. That bound is 6 bytes per symbol, so this is about 6x the input (8x with the
    // adaptive workspace), most of it never touched.
    return hc_seg_compress_work_bound2(in_len, seg_bytes, use_adapt ? HC_FLAG_ADAPT : 0u, width);
}

uint64_t hc_seg_compress_work_bound2(uint64_t in_len, uint64_t seg_bytes, uint32_t flags, uint64_t width)
{
    EncPlan p;
    if ((flags & ~kSegFlags) || !enc_plan(in_len, seg_bytes, (flags & HC_FLAG_ADAPT) != 0, width, p)) return 0;
    return carve_enc(nullptr, p.c.n, p.slot_bytes, p.awork_bytes, checked(flags)).total;
}

int hc_seg_compress_dev(const uint8_t *in, uint64_t in_len, uint32_t flags, uint64_t width, uint64_t seg_bytes,
                        uint8_t *out, uint64_t out_cap, uint64_t *out_len, int32_t *status, void *work,
                        uint64_t work_bytes, void *stream)
{
    if ((!in && in_len) || !out || !out_len || !status || !work) return HC_ERR_ARG;
    if (flags & ~kSegFlags) return HC_ERR_ARG;
    if (seg_bytes & 15u) return HC_ERR_ARG;
    if (!aligned16(in) || !aligned16(out) || !aligned16(work)) return HC_ERR_ARG;
    const int use_adapt = (flags & HC_FLAG_ADAPT) ? 1 : 0;
    const int hs = host_status(in_len, use_adapt, width);
    if (hs) return hs;
    if (!seg_bytes) seg_bytes = HC_SEG_DEFAULT_BYTES;
    EncPlan p;
    if (!enc_plan(in_len, seg_bytes, use_adapt, width, p)) return HC_ERR_ARG;
    const bool check = checked(flags);
    const EncWs w = carve_enc(work, p.c.n, p.slot_bytes, p.awork_bytes, check);
    if (work_bytes < w.total) return HC_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t n = (uint32_t)p.c.n;

    const PlanArgs pa{w.in_offs, w.in_lens, w.widths, w.out_offs, w.out_caps, w.out_lens, w.status,
                      p.c.n, p.c.full, p.c.last, p.slot_full, p.cap_full, p.cap_last, use_adapt ? width : 0};
    seg_plan_kernel<<<(n + 255) / 256, 256, 0, st>>>(pa);
    HC_CK(hipGetLastError());
    Batch b{in ? in : out, w.in_offs, w.in_lens, n, w.slots, w.out_offs, w.out_caps, w.out_lens, w.status,
            flags & HC_FLAG_DIFF};
    // the raw bytes of every cut, before the diff model (an empty input has one empty segment: crc 0)
    if (check) HC_CK(hc::launch_crc32(b.in, w.in_offs, w.in_lens, n, w.crc, hc::CrcGate{nullptr, nullptr, nullptr}, st));
    if (use_adapt) HC_CK(hc::adapt_encode_batch(b, w.widths, w.awork, w.awork_bytes, st));
    else HC_CK(hc::launch_encode(b, (flags & HC_FLAG_DIFF) ? hc::SRC_RAW_DIFF : hc::SRC_RAW, st));
    const SealArgs sa{w.out_lens, w.status, check ? w.crc : nullptr, w.dst_offs, w.ctl, p.c.n, out, out_cap, out_len, status,
                      make_header(flags, in_len, seg_bytes, use_adapt ? width : 0, p.c.n)};
    seg_seal_kernel<<<1, kScan, 0, st>>>(sa);
    seg_gather_kernel<<<n < 65536u ? n : 65536u, 256, 0, st>>>(w.slots, w.out_offs, w.out_lens, w.dst_offs, w.ctl,
                                                               p.c.n, out);
    HC_CK(hipGetLastError());
    return HC_OK;
}

uint64_t hc_seg_decompress_work_bound(const hc_seg_info_t *info, uint64_t in_len)
{
    if (!info) return 0;
    Cuts c;
    if (!info_ok(*info, in_len, c) || c.n > kMaxSegs) return 16;  // rejected without a workspace
    DecPlan p;
    return dec_ws(nullptr, *info, c, 0, info->raw_len, true, in_len, p).total;
}

int hc_seg_decompress_dev(const uint8_t *in, uint64_t in_len, const hc_seg_info_t *info, uint8_t *out,
                          uint64_t out_cap, uint64_t *out_len, int32_t *status, uint64_t *bad_segment, void *work,
                          uint64_t work_bytes, void *stream)
{
    return decode_dev(in, in_len, info, 0, 0, true, out, out_cap, out_len, status, bad_segment, work, work_bytes, stream,
                      0, in_len);
}

int hc_seg_compress(const uint8_t *in, uint64_t in_len, int use_diff, int use_adapt, uint64_t width,
                    uint64_t seg_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_len)
{
    if ((!in && in_len) || !out_len || (!out && out_cap)) return HC_ERR_ARG;
    const uint32_t flags = (use_diff ? HC_FLAG_DIFF : 0u) | (use_adapt ? HC_FLAG_ADAPT : 0u);
    return seg_compress_host(in, in_len, flags, width, seg_bytes, out, out_cap, out_len);
}

int hc_seg_compress2(const uint8_t *in, uint64_t in_len, uint32_t flags, uint64_t width, uint64_t seg_bytes,
                     uint8_t *out, uint64_t out_cap, uint64_t *out_len)
{
    if ((!in && in_len) || !out_len || (!out && out_cap)) return HC_ERR_ARG;
    if (flags & ~kSegFlags) return HC_ERR_ARG;
    return seg_compress_host(in, in_len, flags, width, seg_bytes, out, out_cap, out_len);
}

int hc_seg_decompress(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                      uint64_t *bad_segment)
{
    if ((!in && in_len) || !out_len || (!out && out_cap)) return HC_ERR_ARG;
    return seg_decompress_host(in, in_len, out, out_cap, false, nullptr, out_len, bad_segment);
}

int hc_seg_decompress_alloc(const uint8_t *in, uint64_t in_len, uint8_t **out, uint64_t *out_len,
                            uint64_t *bad_segment)
{
    if ((!in && in_len) || !out || !out_len) return HC_ERR_ARG;
    *out = nullptr;
    return seg_decompress_host(in, in_len, nullptr, 0, true, out, out_len, bad_segment);
}

int hc_seg_range_segments(const hc_seg_info_t *info, uint64_t in_len, uint64_t offset, uint64_t length,
                          uint64_t *first, uint64_t *count)
{
    if (!info || !first || !count) return HC_ERR_ARG;
    Cuts c;
    if (!info_ok(*info, in_len, c) || !range_ok(info->raw_len, offset, length)) return HC_ERR_ARG;
    const Cover cv = range_cover(c, offset, length);
    *first = cv.k0;
    *count = cv.count;
    return HC_OK;
}

uint64_t hc_seg_decompress_range_work_bound(const hc_seg_info_t *info, uint64_t in_len, uint64_t offset,
                                            uint64_t length)
{
    if (!info) return 0;
    Cuts c;
    if (!info_ok(*info, in_len, c) || c.n > kMaxSegs) return 16;  // rejected without a workspace
    if (!range_ok(info->raw_len, offset, length)) return 0;
    DecPlan p;
    return dec_ws(nullptr, *info, c, offset, length, false, in_len, p).total;
}

int hc_seg_decompress_range_dev(const uint8_t *in, uint64_t in_len, const hc_seg_info_t *info, uint64_t offset,
                                uint64_t length, uint8_t *out, uint64_t out_cap, uint64_t *out_len, int32_t *status,
                                uint64_t *bad_segment, void *work, uint64_t work_bytes, void *stream)
{
    return decode_dev(in, in_len, info, offset, length, false, out, out_cap, out_len, status, bad_segment, work,
                      work_bytes, stream, 0, in_len);
}

int hc_seg_decompress_range(const uint8_t *in, uint64_t in_len, uint64_t offset, uint64_t length, uint8_t *out,
                            uint64_t out_cap, uint64_t *out_len, uint64_t *bad_segment)
{
    if ((!in && in_len) || !out_len || (!out && out_cap)) return HC_ERR_ARG;
    auto fail = [&](int rc, uint64_t len) {
        *out_len = len;
        if (bad_segment) *bad_segment = kNoSeg;
        return rc;
    };
    hc_seg_info_t info;
    if (hc_seg_info(in, in_len, &info) != HC_OK) return fail(HC_ERR_SEG_HEADER, 0);
    if (!range_ok(info.raw_len, offset, length)) return HC_ERR_ARG;
    Cuts c;
    (void)info_ok(info, in_len, c);
    if (c.n > kMaxSegs) return HC_ERR_ARG;
    // the index on the host: the verdict without a device, and the covered segments' bytes [s0, s1)
    uint64_t s0 = 0, s1 = 0;
    const bool check = checked(info.flags);
    const uint64_t idx = align16(index_end(c.n, check));
    if (hc_seg_index::index_scan(in, in_len, c.n, check, range_cover(c, offset, length), &s0, &s1) != HC_OK)
        return fail(HC_ERR_SEG_HEADER, 0);
    if (!hc_device_ok()) return fail(HC_ERR_DEVICE, 0);
    if (out_cap < length) return fail(HC_ERR_CAPACITY, length);
    (void)fail(HC_OK, 0);  // (what a HIP error below leaves behind)
    // the compact upload: header and index [0, idx), then the span; in_len stays the container's
    const uint64_t span = s1 - s0;
    DecPlan p;
    const uint64_t wb = dec_ws(nullptr, info, c, offset, length, false, span, p).total;
    hipStream_t st = nullptr;
    DevBuf din, dout, work, meta;
    HC_CK(din.alloc(idx + span + 16));
    HC_CK(dout.alloc(length + 16));
    HC_CK(work.alloc(wb));
    HC_CK(meta.alloc(32));
    HC_CK(hipMemcpyAsync(din.p, in, idx, hipMemcpyHostToDevice, st));
    if (span) HC_CK(hipMemcpyAsync(din.as<uint8_t>() + idx, in + s0, span, hipMemcpyHostToDevice, st));
    uint64_t *m = meta.as<uint64_t>();
    const int rc = decode_dev(din.as<uint8_t>(), in_len, &info, offset, length, false, dout.as<uint8_t>(), length, m,
                              reinterpret_cast<int32_t *>(m + 1), m + 2, work.p, wb, st, s0 - idx, span);
    if (rc) return rc;
    uint64_t h[4] = {0, 0, 0, 0};
    HC_CK(hipMemcpyAsync(h, meta.p, sizeof(h), hipMemcpyDeviceToHost, st));
    HC_CK(hipStreamSynchronize(st));
    const int status = (int32_t)(uint32_t)h[1];
    *out_len = h[0];
    if (bad_segment) *bad_segment = h[2];
    if (status) return status;
    if (h[0]) HC_CK(hipMemcpy(out, dout.p, h[0], hipMemcpyDeviceToHost));
    return HC_OK;
}

}  // extern "C"
