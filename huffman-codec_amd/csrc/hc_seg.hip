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
//
// Every launch is asynchronous on the caller's stream; no allocation, no host synchronisation,
// no host read of device memory in the device entry points. A container-level error zeroes
// every in_lens, which the coders answer with HC_ERR_HEADER before touching anything.
#include <stdlib.h>
#include <string.h>

#include "hc_internal.h"

namespace {

using hc::Batch;
using hc::DevBuf;

constexpr uint64_t kNoSeg = ~0ull;
constexpr uint32_t kScan = 1024;  // threads of the one-workgroup kernels = entries per scan tile
constexpr uint64_t kMaxSegs = 0x7FFFFFFFull;  // Batch::n is 32 bits
const uint8_t kMagic[8] = {0x48, 0x43, 0x53, 0x45, 0x47, 0x31, 0x00, 0xFF};

#define HC_CK(x)                                     \
    do {                                             \
        if ((x) != hipSuccess) return HC_ERR_DEVICE; \
    } while (0)

__host__ __device__ inline uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }
__host__ __device__ inline uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

constexpr uint32_t kSegFlags = HC_FLAG_DIFF | HC_FLAG_ADAPT | HC_SEG_CHECK_CRC32;
// header and index: 8 bytes of enc_len per segment, and 4 of crc in a checked container
inline bool checked(uint32_t flags) { return (flags & HC_SEG_CHECK_CRC32) != 0; }
__host__ __device__ inline uint64_t index_end(uint64_t n, bool check) { return 48 + (check ? 12 : 8) * n; }

// The cut rule: segment k is raw bytes [k full, k full + (k == n - 1 ? last : full)). n == 0:
// invalid arguments. No product here overflows: every one is at most raw.
struct Cuts {
    uint64_t n, full, last;
};
Cuts seg_cuts(uint64_t raw, uint64_t seg, bool adapt, uint64_t width)
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

// every header rule that needs no index entry (hc_seg_info; hc_seg_decompress_dev on its info)
bool info_ok(const hc_seg_info_t &f, uint64_t in_len, Cuts &c)
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

uint64_t get64(const uint8_t *p)
{
    uint64_t v = 0;
    for (int i = 7; i >= 0; --i) v = (v << 8) | p[i];
    return v;
}

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

struct DecWs {
    uint64_t *in_offs, *in_lens, *out_offs, *out_caps, *out_lens;
    int32_t *status;
    uint32_t *crc;  // checked containers: the decoded segments' CRC-32 (otherwise no bytes)
    uint64_t *ctl;  // [0] the container-level status (0, HC_ERR_SEG_HEADER, HC_ERR_CAPACITY)
    void *awork;
    uint64_t awork_bytes, total;
};
DecWs carve_dec(void *work, uint64_t n, uint64_t awork_bytes, bool check)
{
    DecWs w;
    uint8_t *p = static_cast<uint8_t *>(work);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) {
        uint8_t *q = p ? p + o : nullptr;  // null: sizing only
        o += align16(bytes);
        return q;
    };
    w.in_offs = reinterpret_cast<uint64_t *>(take(8 * n));
    w.in_lens = reinterpret_cast<uint64_t *>(take(8 * n));
    w.out_offs = reinterpret_cast<uint64_t *>(take(8 * n));
    w.out_caps = reinterpret_cast<uint64_t *>(take(8 * n));
    w.out_lens = reinterpret_cast<uint64_t *>(take(8 * n));
    w.status = reinterpret_cast<int32_t *>(take(4 * n));
    w.crc = reinterpret_cast<uint32_t *>(take(check ? 4 * n : 0));
    w.ctl = reinterpret_cast<uint64_t *>(take(16));
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

struct OpenArgs {
    const uint8_t *in;
    uint64_t in_len;
    Header hdr;  // the caller's host copy (checked on the host already)
    uint64_t n, full, last, raw_len, out_cap;
    uint64_t *in_offs, *in_lens, *out_offs, *out_caps, *out_lens;
    int32_t *status;
    uint64_t *ctl;
    bool check;
};

// The host has checked its copy of the header against in_len (48 + 8 n <= in_len among the rest;
// 12 n in a checked container, whose crc words follow the lengths); here the device bytes must
// equal that copy, and the index must tile [align16(48 + 8 n or 12 n), in_len) exactly. enc_len entries are untrusted: the offsets add with saturation and every range is
// compared by subtraction, so a forged length cannot wrap into a valid offset.
__global__ __launch_bounds__(kScan) void seg_open_kernel(OpenArgs a)
{
    __shared__ uint64_t part[kScan / 64];
    __shared__ uint32_t s_err;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_err = 0;
    __syncthreads();
    bool err = false;
    const uint64_t *i64 = reinterpret_cast<const uint64_t *>(a.in);
    if (tid < 6 && i64[tid] != a.hdr.w[tid]) err = true;
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
            a.in_offs[k] = off;
            a.in_lens[k] = len;
            a.out_offs[k] = k * a.full;
            a.out_caps[k] = tail ? a.last : a.full;
            a.out_lens[k] = 0;
            a.status[k] = HC_ERR_DEVICE;  // overwritten by the launch that owns the segment
        }
        carry = sat_add(carry, total);
    }
    if (err) s_err = 1;
    __syncthreads();
    const int32_t st = s_err ? HC_ERR_SEG_HEADER : (a.raw_len > a.out_cap ? HC_ERR_CAPACITY : 0);
    if (tid == 0) a.ctl[0] = (uint64_t)st;
    if (st == 0) return;
    // nothing may be decoded (the output ranges need not even lie inside out): empty inputs,
    // which the coders answer with HC_ERR_HEADER before they touch anything
    for (uint64_t k = tid; k < a.n; k += kScan) a.in_lens[k] = 0;
}

struct CloseArgs {
    const uint64_t *out_lens, *out_caps, *ctl;
    const int32_t *seg_status;
    const uint32_t *crc, *want_crc;  // checked containers: of the decoded bytes, and the index's (else null)
    uint64_t n, raw_len;
    uint64_t *out_len, *bad_segment;
    int32_t *status;
};

__global__ __launch_bounds__(kScan) void seg_close_kernel(CloseArgs a)
{
    __shared__ unsigned long long s_bad;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_bad = kNoSeg;
    __syncthreads();
    const int32_t top = (int32_t)a.ctl[0];
    if (top == 0) {
        // the lowest segment that failed, decoded cleanly to another length than its cut, or to
        // that length with another checksum (crc[k] is written exactly for those that reach it)
        uint64_t bad = kNoSeg;
        for (uint64_t k = tid; k < a.n && bad == kNoSeg; k += kScan)
            if (a.seg_status[k] != 0 || a.out_lens[k] != a.out_caps[k] || (a.crc && a.crc[k] != a.want_crc[k]))
                bad = k;
        if (bad != kNoSeg) atomicMin(&s_bad, (unsigned long long)bad);
    }
    __syncthreads();
    if (tid != 0) return;
    const uint64_t bad = s_bad;
    int32_t st = top;
    uint64_t len = top == HC_ERR_CAPACITY ? a.raw_len : 0;
    if (top == 0) {
        if (bad != kNoSeg) {
            st = a.seg_status[bad];
            // 64: it wanted more room than its cut; 0: it decoded to fewer bytes, or to the wrong ones
            if (st == 0 && a.out_lens[bad] == a.out_caps[bad]) st = HC_ERR_SEG_CHECK;
            else if (st == 0 || st == HC_ERR_CAPACITY) st = HC_ERR_SEG_SIZE;
        } else {
            len = a.raw_len;
        }
    }
    *a.status = st;
    *a.out_len = len;
    if (a.bad_segment) *a.bad_segment = bad;
}

// hc_seg_decompress_dev with an info that fails the host checks: the verdict alone
__global__ void seg_reject_kernel(uint64_t *out_len, int32_t *status, uint64_t *bad_segment)
{
    *status = HC_ERR_SEG_HEADER;
    *out_len = 0;
    if (bad_segment) *bad_segment = kNoSeg;
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
    const uint64_t aw =
        (info->flags & HC_FLAG_ADAPT) ? hc::adapt_decode_work_bound(in_len, info->raw_len, (uint32_t)c.n) : 0;
    return carve_dec(nullptr, c.n, aw, checked(info->flags)).total;
}

int hc_seg_decompress_dev(const uint8_t *in, uint64_t in_len, const hc_seg_info_t *info, uint8_t *out,
                          uint64_t out_cap, uint64_t *out_len, int32_t *status, uint64_t *bad_segment, void *work,
                          uint64_t work_bytes, void *stream)
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
    if (c.n > kMaxSegs) return HC_ERR_ARG;
    const bool adapt = (info->flags & HC_FLAG_ADAPT) != 0;
    const uint32_t n = (uint32_t)c.n;
    const bool check = checked(info->flags);
    const DecWs w = carve_dec(work, c.n, adapt ? hc::adapt_decode_work_bound(in_len, info->raw_len, n) : 0, check);
    if (work_bytes < w.total) return HC_ERR_ARG;

    const OpenArgs oa{in, in_len, make_header(info->flags, info->raw_len, info->seg_bytes, info->width, c.n),
                      c.n, c.full, c.last, info->raw_len, out_cap,
                      w.in_offs, w.in_lens, w.out_offs, w.out_caps, w.out_lens, w.status, w.ctl, check};
    seg_open_kernel<<<1, kScan, 0, st>>>(oa);
    HC_CK(hipGetLastError());
    Batch b{in, w.in_offs, w.in_lens, n, out, w.out_offs, w.out_caps, w.out_lens, w.status, 0};
    if (adapt) HC_CK(hc::adapt_decode_batch(b, w.awork, w.awork_bytes, st));
    else HC_CK(hc::launch_decode(b, hc::DST_RAW, st));
    // segments that decoded cleanly to their cut's length, in place; none when the verdict is set
    if (check) HC_CK(hc::launch_crc32(out, w.out_offs, w.out_caps, n, w.crc, hc::CrcGate{w.ctl, w.status, w.out_lens}, st));
    const CloseArgs ca{w.out_lens, w.out_caps, w.ctl, w.status, check ? w.crc : nullptr,
                       check ? reinterpret_cast<const uint32_t *>(in + 48 + 8 * c.n) : nullptr,
                       c.n, info->raw_len, out_len, bad_segment, status};
    seg_close_kernel<<<1, kScan, 0, st>>>(ca);
    HC_CK(hipGetLastError());
    return HC_OK;
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

}  // extern "C"
