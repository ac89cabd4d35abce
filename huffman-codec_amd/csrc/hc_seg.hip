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
//   reads   a list of byte ranges of one container (hc_seg_decompress_ranges*): the union of the
//           segments they cover decodes once, every segment whole into one staging region of the
//           workspace, and a pack launch moves every read's bytes to its own place in out (its own
//           block comment below has the stages)
//   update  a range write (hc_seg_update*): decode the segments that a patch covers in part, lay
//           the patches over them, code the covered segments, and splice their new streams
//           and the old container's other bytes into the new container (its own block comment
//           below has the stages)
//   append  raw bytes added behind a container (hc_seg_append*): decode the partly filled last segment,
//           lay the new bytes behind it, code that segment and the new ones, and splice them behind
//           the kept segments under a new index (its own block comment below has the stages)
//   items   a call codes one item (an input, or a container and a range of it) or many
//           (hc_seg_*_batch_dev): the segments of all items lie in one concatenated array, so the
//           same coder launches serve them all. Each glue stage above is written once, against an
//           item record (EncItem, DecItem) that it gets from an item source: One, a single call's
//           record in the kernel arguments, or Many, a batch's records in the workspace, carried
//           there as kernel arguments by seg_items_kernel. Seal, open and close run one workgroup
//           per item.
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

// ---------------------------------------------------------------------------------------------
// Workspace layouts (host-side carving; every region 16-byte aligned)
// ---------------------------------------------------------------------------------------------
// hands out the regions of a workspace one after the other, from `from` on
struct Carver {
    uint8_t *p;  // null: sizing only
    uint64_t o;
    explicit Carver(void *work, uint64_t from = 0) : p(static_cast<uint8_t *>(work)), o(from) {}
    uint8_t *take(uint64_t bytes)
    {
        uint8_t *q = p ? p + o : nullptr;
        o += align16(bytes);
        return q;
    }
    template <class T>
    T *arr(uint64_t n)
    {
        return reinterpret_cast<T *>(take(sizeof(T) * n));
    }
    uint64_t *take64(uint64_t n) { return arr<uint64_t>(n); }
    uint64_t total() const { return o; }
};

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
    Carver cv(work);
    w.in_offs = cv.take64(n);
    w.in_lens = cv.take64(n);
    w.widths = cv.take64(n);
    w.out_offs = cv.take64(n);
    w.out_caps = cv.take64(n);
    w.out_lens = cv.take64(n);
    w.dst_offs = cv.take64(n);
    w.status = cv.arr<int32_t>(n);
    w.crc = cv.arr<uint32_t>(check ? n : 0);
    w.ctl = cv.take64(2);
    w.slots = cv.take(slot_bytes);
    w.awork = cv.take(awork_bytes);
    w.awork_bytes = awork_bytes;
    w.total = cv.total();
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

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the six header words of a container, as the caller's host copy has them
struct HeaderWords {
    uint64_t magic, flags, raw_len, seg_bytes, width, n;
};

// The header and the index of the container at `in`, by the whole workgroup of kScan threads; the
// open kernel of every operation is built on it. The host has checked its copy of the header
// against in_len (48 + 8 n <= in_len among the rest; 12 n in a checked container, whose crc words
// follow the lengths); here the device bytes must equal that copy, and the index must tile
// [align16(48 + 8 n or 12 n), in_len) exactly. enc_len entries are untrusted: the offsets add with
// saturation and every range is compared by subtraction, so a forged length cannot wrap into a
// valid offset. each(k, off, len) runs for every segment that passes the range rules, with its
// place in the container. Returns, to every thread, whether the header or any entry failed.
template <class Each>
__device__ __forceinline__ bool scan_index(const uint8_t *in, const HeaderWords &h, uint64_t in_len, bool check, Each each)
{
    __shared__ uint64_t part[kScan / 64];
    __shared__ uint32_t s_err;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_err = 0;
    __syncthreads();
    bool err = false;
    const uint64_t *i64 = reinterpret_cast<const uint64_t *>(in);
    if (tid < 6) {
        const uint64_t want = tid == 0 ? h.magic : tid == 1 ? h.flags : tid == 2 ? h.raw_len
                              : tid == 3 ? h.seg_bytes : tid == 4 ? h.width : h.n;
        if (i64[tid] != want) err = true;
    }
    uint64_t carry = align16(index_end(h.n, check));
    for (uint64_t base = 0; base < h.n; base += kScan) {
        const uint64_t k = base + tid;
        const bool in_k = k < h.n;
        const uint64_t len = in_k ? i64[6 + k] : 0;
        const bool big = len > in_len;
        uint64_t total;
        const uint64_t off = sat_add(carry, block_scan(in_k && !big ? align16(len) : 0, part, total));
        if (in_k) {
            if (big || off > in_len || len > in_len - off) err = true;
            else if (k == h.n - 1 && off + len != in_len) err = true;  // truncated, or trailing bytes
            else each(k, off, len);
        }
        carry = sat_add(carry, total);
    }
    if (err) s_err = 1;
    __syncthreads();
    return s_err != 0;
}

// The lowest entry of [0, n) that `failed` names, by the workgroup's kScan threads: each takes
// the entries of its stride and leaves its lowest in *s_bad by atomicMin. *s_bad is a word of LDS
// that the caller sets to kNoSeg before a barrier and reads after the next one (kNoSeg: none).
template <class Failed>
__device__ __forceinline__ void lowest_failing(uint64_t n, unsigned long long *s_bad, Failed failed)
{
    uint64_t bad = kNoSeg;
    for (uint64_t i = threadIdx.x; i < n && bad == kNoSeg; i += kScan)
        if (failed(i)) bad = i;
    if (bad != kNoSeg) atomicMin(s_bad, (unsigned long long)bad);
}

// The status of a decoded segment that failed (its coder did, or it decoded cleanly to another
// length than its cut, or to that length with another checksum than the index has): the coder's
// own, except HC_ERR_CAPACITY (it wanted more room than its cut) and a clean decode to fewer bytes,
// which are HC_ERR_SEG_SIZE, and a clean decode to the cut's length, which only the checksum can
// have failed.
__device__ __forceinline__ int32_t decoded_verdict(int32_t st, uint64_t len, uint64_t cut)
{
    if (st == 0 && len == cut) return HC_ERR_SEG_CHECK;
    if (st == 0 || st == HC_ERR_CAPACITY) return HC_ERR_SEG_SIZE;
    return st;
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

// what a synchronous call that the host decides leaves in its outputs: rc, with no segment to blame
int fail(int rc, uint64_t len, uint64_t *out_len, uint64_t *bad_segment)
{
    *out_len = len;
    if (bad_segment) *bad_segment = kNoSeg;
    return rc;
}
// The verdict of a device call that wrote out_len, status and bad_segment to words 0, 1 and 2 of
// `meta`, once the stream is through: the outputs, and the status (HC_ERR_DEVICE: the read failed)
int read_verdict(const DevBuf &meta, hipStream_t st, uint64_t *out_len, uint64_t *bad_segment)
{
    uint64_t h[4] = {0, 0, 0, 0};
    HC_CK(hipMemcpyAsync(h, meta.p, sizeof(h), hipMemcpyDeviceToHost, st));
    HC_CK(hipStreamSynchronize(st));
    *out_len = h[0];
    if (bad_segment) *bad_segment = h[2];
    return (int32_t)(uint32_t)h[1];
}

int seg_decompress_host(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap, bool alloc,
                        uint8_t **out_alloc, uint64_t *out_len, uint64_t *bad_segment)
{
    (void)fail(HC_OK, 0, out_len, bad_segment);
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
    const int status = read_verdict(meta, st, out_len, bad_segment);
    if (status) return status;
    if (alloc) {
        out = static_cast<uint8_t *>(malloc(*out_len ? *out_len : 1));
        if (!out) return HC_ERR_DEVICE;
        *out_alloc = out;
    }
    if (*out_len) HC_CK(hipMemcpy(out, dout.p, *out_len, hipMemcpyDeviceToHost));
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

// ---------------------------------------------------------------------------------------------
// Items and the glue stages. A call codes one item or many (hc_seg_*_batch_dev) over one
// concatenated segment array, so one launch of each coder serves them all. The item record
// (EncItem, DecItem) is the one description of an item, and every stage is written once against
// it. A batch's records reach the device as kernel arguments, a chunk per launch (seg_items_kernel;
// the only launches that grow with n_items), and live in the workspace from then on (Many); a
// single call is the one-item case (seg0, slot0 and every *_off 0, hs 0) with the record in the
// stages' own kernel arguments (One): no seg_items_kernel launch, no record in memory, no search,
// no map. Seal, open and close run one workgroup per item, each with its own tiled scan; plan and
// gather run over the segments and, in a batch, find their item by search and by the map that
// plan leaves. ctl is one word per item.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kEncChunk = 32, kDecChunk = 16;  // items per descriptor launch (arguments: 4 KB at most)

struct EncItem {
    uint64_t seg0, n;  // its segments: [seg0, seg0 + n) of the arrays; n 0: hs alone
    uint64_t full, last, slot_full, cap_full, cap_last, width;
    uint64_t in_off, slot_off, out_off, out_cap;  // from in, the slots, out
    uint64_t raw_len;
    int64_t hs;  // the host-decided status
};
struct DecItem {
    uint64_t in_off, in_len, skip;  // skip: what the covered segments' input offsets lose (a compact upload)
    uint64_t flags, raw_len, seg_bytes, width;  // header words 1 .. 4 (0: the magic, 5: n), the caller's host copy
    uint64_t n, full, last, offset, length, out_cap;
    uint64_t k0, count, nslots, slot;
    uint64_t out_off, slot_off;  // from out, the slots
    uint64_t seg0, slot0;        // its first entry of the segment arrays, of the copy arrays
    uint32_t check;
    int32_t hs;  // the host-decided status
};
static_assert(sizeof(EncItem) == 112 && sizeof(DecItem) == 176, "the work bounds of hcodec.h count these");

// What the one item of a single call has by construction (enc_item, dec_item with seg0, slot0 and
// slot_off 0 over a public item without offsets, after the host's checks), as constants: the
// single calls' kernels carry no host-status branch and less offset arithmetic, and keep the
// registers and the occupancy they had as kernels of their own (without this seg_seal_kernel<One>
// has 7 waves for 8 and seg_open_kernel<One> 5 for 6; profiles/seg_unify_resource_usage.txt).
__device__ inline EncItem alone(EncItem it)
{
    it.seg0 = it.in_off = it.slot_off = it.out_off = 0;
    it.hs = 0;
    return it;
}
__device__ inline DecItem alone(DecItem it)
{
    it.seg0 = it.slot0 = 0;  // (its three byte offsets stay values: folding them too doubles seg_open's scalar spills)
    it.hs = 0;
    return it;
}

// The item sources. at(i): item i's record; find(k): the item of segment k, the last one whose
// seg0 is <= k (an item without segments shares its seg0 with the next one, which the search
// passes); own / owner: the segment -> item map (encoder batches: plan writes it, gather reads it).
template <class Item>
struct One {
    Item it;
    __device__ Item at(uint32_t) const { return alone(it); }
    __device__ uint32_t find(uint64_t) const { return 0; }
    __device__ void own(uint64_t, uint32_t) const {}
    __device__ uint32_t owner(uint64_t) const { return 0; }
};
template <class Item>
struct Many {
    const Item *items;
    uint32_t n_items;
    uint32_t *seg_item;  // (the decoder has none)
    __device__ const Item &at(uint32_t i) const { return items[i]; }
    __device__ uint32_t find(uint64_t k) const
    {
        uint32_t lo = 0, hi = n_items;  // items[lo].seg0 <= k < items[hi].seg0 (hi == n_items: the end)
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (items[mid].seg0 <= k) lo = mid;
            else hi = mid;
        }
        return lo;
    }
    __device__ void own(uint64_t k, uint32_t i) const { seg_item[k] = i; }
    __device__ uint32_t owner(uint64_t k) const { return seg_item[k]; }
};

template <class Item, uint32_t N>
struct ItemChunk {
    Item it[N];
    Item *dst;
    uint32_t count;
};
static_assert(sizeof(ItemChunk<EncItem, kEncChunk>) <= 3968 && sizeof(ItemChunk<DecItem, kDecChunk>) <= 3968,
              "kernel arguments");

template <class Chunk>
__global__ __launch_bounds__(64) void seg_items_kernel(Chunk c)
{
    if (threadIdx.x < c.count) c.dst[threadIdx.x] = c.it[threadIdx.x];
}

// collects the records of a call and launches a chunk whenever one is full
template <class Item, uint32_t N>
struct ItemFeed {
    ItemChunk<Item, N> c;
    Item *dst;
    hipStream_t st;
    ItemFeed(Item *d, hipStream_t s) : dst(d), st(s) { c.count = 0; }
    void flush()
    {
        if (c.count == 0) return;
        c.dst = dst;
        seg_items_kernel<<<1, 64, 0, st>>>(c);
        dst += c.count;
        c.count = 0;
    }
    void push(const Item &it)
    {
        c.it[c.count++] = it;
        if (c.count == N) flush();
    }
};

struct EncBatchWs {
    EncWs s;  // the single call's arrays over all N segments (its ctl word is not used)
    EncItem *items;
    uint32_t *seg_item;  // segment -> item
    uint64_t *ctl;       // [i] 1: item i is sealed, the gather may copy
    uint64_t total;
};
EncBatchWs carve_enc_batch(void *work, uint64_t n_items, uint64_t n, uint64_t slot_bytes, uint64_t awork_bytes,
                           bool check)
{
    EncBatchWs w;
    w.s = carve_enc(work, n, slot_bytes, awork_bytes, check);
    Carver cv(work, w.s.total);
    w.items = cv.arr<EncItem>(n_items);
    w.seg_item = cv.arr<uint32_t>(n);
    w.ctl = cv.take64(n_items);
    w.total = cv.total();
    return w;
}

// what the encoder's stages share: the arrays over all n segments of the call, and its outputs
struct EncCall {
    uint64_t n;
    uint64_t *in_offs, *in_lens, *widths, *slot_offs, *slot_caps, *enc_lens, *dst_offs;
    int32_t *seg_status;
    const uint32_t *crc;  // null: unchecked containers
    uint64_t *ctl;        // [i] 1: item i is sealed, the gather may copy
    const uint8_t *slots;
    uint8_t *out;
    uint64_t *out_lens;  // per item
    int32_t *status;     // per item
    uint64_t magic, flags, seg_bytes;  // header words 0, 1 and 3
};

// segment k's input range and its output slot (all in closed form: only an item's last segment differs)
template <class Src>
__global__ __launch_bounds__(256) void seg_plan_kernel(Src items, EncCall a)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.n) return;
    const uint32_t item = items.find(k);
    const EncItem &it = items.at(item);
    const uint64_t j = k - it.seg0;
    const bool tail = j == it.n - 1;
    a.in_offs[k] = it.in_off + j * it.full;
    a.in_lens[k] = tail ? it.last : it.full;
    a.widths[k] = it.width;
    a.slot_offs[k] = it.slot_off + j * it.slot_full;
    a.slot_caps[k] = tail ? it.cap_last : it.cap_full;
    a.enc_lens[k] = 0;
    a.seg_status[k] = HC_ERR_DEVICE;  // every segment is coded by exactly one launch, which overwrites this
    items.own(k, item);
}

// item blockIdx.x: its segments' places from out (dst_offs), its verdict, its header and index at
// out + out_off
template <class Src>
__global__ __launch_bounds__(kScan) void seg_seal_kernel(Src items, EncCall a)
{
    __shared__ uint64_t part[kScan / 64];
    __shared__ unsigned long long s_bad, s_end;
    const uint32_t tid = threadIdx.x, item = blockIdx.x;
    const EncItem it = items.at(item);
    if (it.hs != 0) {  // decided on the host: no segment, no output byte
        if (tid == 0) {
            a.status[item] = (int32_t)it.hs;
            a.out_lens[item] = 0;
            a.ctl[item] = 0;
        }
        return;
    }
    if (tid == 0) {
        s_bad = kNoSeg;
        s_end = 0;
    }
    __syncthreads();
    const uint64_t *enc_lens = a.enc_lens + it.seg0;
    const int32_t *seg_status = a.seg_status + it.seg0;
    const uint32_t *crc = a.crc ? a.crc + it.seg0 : nullptr;
    const uint64_t idx_end = index_end(it.n, crc != nullptr);
    uint64_t carry = align16(idx_end);  // where segment 0 starts
    uint64_t bad = kNoSeg;
    for (uint64_t base = 0; base < it.n; base += kScan) {
        const uint64_t k = base + tid;
        const bool in = k < it.n;
        const uint64_t len = in ? enc_lens[k] : 0;
        if (in && seg_status[k] != 0 && bad == kNoSeg) bad = k;
        uint64_t total;
        const uint64_t off = sat_add(carry, block_scan(in ? align16(len) : 0, part, total));
        if (in) a.dst_offs[it.seg0 + k] = it.out_off + off;  // (read by the gather of a sealed item alone)
        if (in && k == it.n - 1) s_end = sat_add(off, len);  // no padding after the last segment
        carry = sat_add(carry, total);
    }
    if (bad != kNoSeg) atomicMin(&s_bad, (unsigned long long)bad);
    __syncthreads();
    const uint64_t first_bad = s_bad, end = s_end;
    int32_t st = 0;
    if (first_bad != kNoSeg) st = seg_status[first_bad];
    else if (end > it.out_cap) st = HC_ERR_CAPACITY;
    if (tid == 0) {
        a.status[item] = st;
        a.out_lens[item] = (st == 0 || st == HC_ERR_CAPACITY) ? end : 0;
        a.ctl[item] = st == 0 ? 1 : 0;
    }
    if (st != 0) return;
    // sealed: end <= out_cap, so the header, the index and its padding lie inside the item's output
    uint64_t *o64 = reinterpret_cast<uint64_t *>(a.out + it.out_off);
    uint32_t *o32 = reinterpret_cast<uint32_t *>(a.out + it.out_off);
    if (tid < 6)
        o64[tid] = tid == 0 ? a.magic : tid == 1 ? a.flags : tid == 2 ? it.raw_len : tid == 3 ? a.seg_bytes
                   : tid == 4 ? it.width : it.n;
    if (tid >= 8 && tid < 8 + (align16(idx_end) - idx_end) / 4) o32[idx_end / 4 + (tid - 8)] = 0;
    for (uint64_t k = tid; k < it.n; k += kScan) o64[6 + k] = enc_lens[k];
    if (crc)
        for (uint64_t k = tid; k < it.n; k += kScan) o32[12 + 2 * it.n + k] = crc[k];
}

// Slot k -> out + dst_offs[k] (dst_offs count from out), one workgroup per segment. Both ends are
// 16-byte aligned, so whole 16-byte chunks per lane; the chunk that holds the stream's last bytes
// goes out with its padding zeroed, except that of an item's last segment (a container ends with
// its last byte: bytes).
template <class Src>
__global__ __launch_bounds__(256) void seg_gather_kernel(Src items, EncCall a)
{
    for (uint64_t k = blockIdx.x; k < a.n; k += gridDim.x) {
        const uint32_t item = items.owner(k);
        if (a.ctl[item] == 0) continue;  // not sealed: nothing is copied
        const EncItem &it = items.at(item);
        const bool last = k == it.seg0 + it.n - 1;
        const uint64_t len = a.enc_lens[k];
        const u32x4 *src = reinterpret_cast<const u32x4 *>(a.slots + a.slot_offs[k]);
        u32x4 *dst = reinterpret_cast<u32x4 *>(a.out + a.dst_offs[k]);
        const uint64_t chunks = len / 16;
        for (uint64_t c = threadIdx.x; c < chunks; c += 256) dst[c] = src[c];
        const uint32_t rem = (uint32_t)(len & 15u);
        if (rem == 0 || threadIdx.x != 255) continue;
        if (last) {
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

// the sums an encode batch is sized by, over the items that pass host_status; false: too many segments
struct EncTotals {
    uint64_t n, slot_bytes, in_bytes;
};
bool enc_totals(const hc_seg_enc_item_t *items, uint32_t n_items, int use_adapt, uint64_t seg_bytes, EncTotals &t)
{
    t = EncTotals{0, 0, 0};
    for (uint32_t i = 0; i < n_items; ++i) {
        if (host_status(items[i].in_len, use_adapt, items[i].width)) continue;
        EncPlan p;
        if (!enc_plan(items[i].in_len, seg_bytes, use_adapt, items[i].width, p)) return false;
        t.n += p.c.n;
        t.slot_bytes += p.slot_bytes;
        t.in_bytes += items[i].in_len;
        if (t.n > kMaxSegs) return false;
    }
    return true;
}
EncBatchWs enc_batch_ws(void *work, uint32_t n_items, const EncTotals &t, int use_adapt, bool check)
{
    const uint64_t aw = (use_adapt && t.n) ? hc::adapt_encode_work_bound(t.in_bytes, (uint32_t)t.n) : 0;
    return carve_enc_batch(work, n_items, t.n, t.slot_bytes, aw, check);
}

// the record of one input: hs its host_status; p (hs 0 alone) its plan; seg0 and slot_off where
// its segments and their slots start
EncItem enc_item(const hc_seg_enc_item_t &h, int hs, const EncPlan &p, int use_adapt, uint64_t seg0, uint64_t slot_off)
{
    EncItem r;
    memset(&r, 0, sizeof(r));
    r.seg0 = seg0;
    r.hs = hs;
    if (hs) return r;
    return EncItem{seg0, p.c.n, p.c.full, p.c.last, p.slot_full, p.cap_full, p.cap_last,
                   use_adapt ? h.width : 0, h.in_off, slot_off, h.out_off, h.out_cap, h.in_len, 0};
}

// The encoder's launches over the n_items records of `items`, whose n_segs segments fill the
// arrays of s; ctl: a word per item. seg_bytes: the size in use, never 0.
template <class Src>
int encode_launch(const Src &items, uint32_t n_items, uint64_t n_segs, const EncWs &s, uint64_t *ctl,
                  const uint8_t *in, uint8_t *out, uint32_t flags, uint64_t seg_bytes, uint64_t *out_lens,
                  int32_t *status, hipStream_t st)
{
    const uint32_t n = (uint32_t)n_segs;
    const bool check = checked(flags);
    const EncCall ec{n_segs, s.in_offs, s.in_lens, s.widths, s.out_offs, s.out_caps, s.out_lens, s.dst_offs,
                     s.status, check ? s.crc : nullptr, ctl, s.slots, out, out_lens, status,
                     get64(kMagic), flags & 0xFFFFu, seg_bytes};  // byte 8 the flags, byte 9 the check kind
    if (n) {
        seg_plan_kernel<<<(n + 255) / 256, 256, 0, st>>>(items, ec);
        HC_CK(hipGetLastError());
        Batch b{in ? in : out, s.in_offs, s.in_lens, n, s.slots, s.out_offs, s.out_caps, s.out_lens, s.status,
                flags & HC_FLAG_DIFF};
        // the raw bytes of every cut, before the diff model (an empty input has one empty segment: crc 0)
        if (check) HC_CK(hc::launch_crc32(b.in, s.in_offs, s.in_lens, n, s.crc, hc::CrcGate{nullptr, nullptr}, st));
        if (flags & HC_FLAG_ADAPT) HC_CK(hc::adapt_encode_batch(b, s.widths, s.awork, s.awork_bytes, st));
        else HC_CK(hc::launch_encode(b, (flags & HC_FLAG_DIFF) ? hc::SRC_RAW_DIFF : hc::SRC_RAW, st));
    }
    seg_seal_kernel<<<n_items, kScan, 0, st>>>(items, ec);
    if (n) seg_gather_kernel<<<n < 65536u ? n : 65536u, 256, 0, st>>>(items, ec);
    HC_CK(hipGetLastError());
    return HC_OK;
}

// --- decode ---
// `count` covered segments and `nslots` staging slots over all items. What differs between the
// calls comes in as byte counts: a single call has crc words for a checked container alone, one
// 16-byte ctl region and no records; a batch has a crc word per segment (entry k of a checked
// item's segment k alone is written and read), a ctl word and a record per item.
struct DecWs {
    uint64_t *in_offs, *in_lens, *out_offs, *out_caps, *out_lens;
    int32_t *status;
    uint32_t *crc;  // the decoded segments' CRC-32
    uint64_t *ctl;  // [i] item i's container-level status (0, HC_ERR_SEG_HEADER, HC_ERR_CAPACITY, or hs)
    DecItem *items;
    uint64_t *cp_src, *cp_len, *cp_dst;  // slot s: cp_len[s] bytes from slots + cp_src[s] to out + cp_dst[s]
    uint8_t *slots;
    void *awork;
    uint64_t awork_bytes, total;
};
DecWs carve_dec(void *work, uint64_t count, uint64_t nslots, uint64_t slot_bytes, uint64_t awork_bytes,
                uint64_t crc_bytes, uint64_t ctl_bytes, uint64_t n_records)
{
    DecWs w;
    Carver cv(work);
    w.in_offs = cv.take64(count);
    w.in_lens = cv.take64(count);
    w.out_offs = cv.take64(count);
    w.out_caps = cv.take64(count);
    w.out_lens = cv.take64(count);
    w.status = cv.arr<int32_t>(count);
    w.crc = reinterpret_cast<uint32_t *>(cv.take(crc_bytes));
    w.ctl = reinterpret_cast<uint64_t *>(cv.take(ctl_bytes));
    w.items = cv.arr<DecItem>(n_records);
    w.cp_src = cv.take64(nslots);
    w.cp_len = cv.take64(nslots);
    w.cp_dst = cv.take64(nslots);
    w.slots = cv.take(slot_bytes);
    w.awork = cv.take(awork_bytes);
    w.awork_bytes = awork_bytes;
    w.total = cv.total();
    return w;
}

// what the decoder's stages share: the arrays over all covered segments and all staging slots of
// the call, and its outputs
struct DecCall {
    const uint8_t *in;
    uint64_t magic;          // header word 0
    uint64_t out_d, slot_d;  // out and the slots from the call's output base
    uint64_t *in_offs, *in_lens, *out_offs, *out_caps, *seg_out_lens;
    uint64_t *cp_src, *cp_len, *cp_dst;
    int32_t *seg_status;
    const uint32_t *crc;  // of the decoded bytes (checked items' entries alone)
    uint64_t *ctl;        // [i] item i's container-level status
    uint64_t *out_lens, *bad_segments;  // per item (bad_segments: or null)
    int32_t *status;                    // per item
};

// Item blockIdx.x: scan_index's header compare and index scan, whatever the range, written out in
// this one kernel because built on scan_index it spills more scalar registers than it does as it
// stands (profiles/seg_write_resource_usage.txt); a change of the rules goes into both. Segment
// arrays for the covered segments only (entry seg0 + k - k0; input offsets from the call's `in`,
// outputs from the call's base), and the staged ones' copies from slot0 on (sources from the
// slots' start, destinations from `out`).
template <class Src>
__global__ __launch_bounds__(kScan) void seg_open_kernel(Src items, DecCall a)
{
    __shared__ uint64_t part[kScan / 64];
    __shared__ uint32_t s_err;
    const uint32_t tid = threadIdx.x, item = blockIdx.x;
    const DecItem it = items.at(item);
    if (it.hs != 0) {  // decided on the host: no segment (count and nslots are 0), no output byte
        if (tid == 0) a.ctl[item] = (uint64_t)it.hs;
        return;
    }
    uint64_t *cp_src = a.cp_src + it.slot0, *cp_len = a.cp_len + it.slot0, *cp_dst = a.cp_dst + it.slot0;
    if (tid == 0) s_err = 0;
    for (uint64_t s = tid; s < it.nslots; s += kScan) cp_len[s] = 0;  // a slot nothing is staged in
    __syncthreads();
    bool err = false;
    const uint64_t *i64 = reinterpret_cast<const uint64_t *>(a.in + it.in_off);
    if (tid < 6) {
        const uint64_t want = tid == 0 ? a.magic : tid == 1 ? it.flags : tid == 2 ? it.raw_len
                              : tid == 3 ? it.seg_bytes : tid == 4 ? it.width : it.n;
        if (i64[tid] != want) err = true;
    }
    const uint64_t end = it.offset + it.length;  // (inside raw_len: the host's check)
    const bool all_staged = (it.offset & 3u) != 0;
    const uint64_t tail_slot = it.offset != it.k0 * it.full;  // aligned: after segment k0's slot, if it has one
    uint64_t carry = align16(index_end(it.n, it.check != 0));
    for (uint64_t base = 0; base < it.n; base += kScan) {
        const uint64_t k = base + tid;
        const bool in = k < it.n;
        const uint64_t len = in ? i64[6 + k] : 0;
        const bool big = len > it.in_len;
        uint64_t total;
        const uint64_t off = sat_add(carry, block_scan(in && !big ? align16(len) : 0, part, total));
        if (in) {
            const bool tail = k == it.n - 1;
            if (big || off > it.in_len || len > it.in_len - off) err = true;
            else if (tail && off + len != it.in_len) err = true;  // truncated, or trailing bytes
        }
        if (in && k >= it.k0 && k - it.k0 < it.count) {
            const uint64_t i = k - it.k0, e_i = it.seg0 + i;
            const uint64_t b = k * it.full, cap = k == it.n - 1 ? it.last : it.full, e = b + cap;
            const uint64_t lo = b > it.offset ? b : it.offset, hi = e < end ? e : end;
            a.in_offs[e_i] = it.in_off + off - it.skip;  // (a wrapped value is never read: err zeroes in_lens)
            a.in_lens[e_i] = len;
            a.out_caps[e_i] = cap;
            a.seg_out_lens[e_i] = 0;
            a.seg_status[e_i] = HC_ERR_DEVICE;  // overwritten by the launch that owns the segment
            if (all_staged || lo != b || hi != e) {
                const uint64_t s = all_staged ? i : (i == 0 ? 0 : tail_slot);
                a.out_offs[e_i] = a.slot_d + it.slot_off + s * it.slot;
                cp_src[s] = it.slot_off + s * it.slot + (lo - b);
                cp_len[s] = hi - lo;
                cp_dst[s] = it.out_off + (lo - it.offset);
            } else {
                a.out_offs[e_i] = a.out_d + it.out_off + (b - it.offset);
            }
        }
        carry = sat_add(carry, total);
    }
    if (err) s_err = 1;
    __syncthreads();
    const int32_t st = s_err ? HC_ERR_SEG_HEADER : (it.length > it.out_cap ? HC_ERR_CAPACITY : 0);
    if (tid == 0) a.ctl[item] = (uint64_t)st;
    if (st == 0) return;
    // nothing of this item may be decoded or copied: empty inputs, which the coders answer with
    // HC_ERR_HEADER before they touch anything (and which the CRC gate then passes over), empty copies
    for (uint64_t i = tid; i < it.count; i += kScan) a.in_lens[it.seg0 + i] = 0;
    for (uint64_t s = tid; s < it.nslots; s += kScan) cp_len[s] = 0;
}

// item blockIdx.x: the verdict over its covered segments; bad_segment is the container's index
template <class Src>
__global__ __launch_bounds__(kScan) void seg_close_kernel(Src items, DecCall a)
{
    __shared__ unsigned long long s_bad;
    const uint32_t tid = threadIdx.x, item = blockIdx.x;
    const DecItem &it = items.at(item);
    const uint64_t seg0 = it.seg0, count = it.count, k0 = it.k0, length = it.length;
    const uint64_t *out_lens = a.seg_out_lens + seg0, *out_caps = a.out_caps + seg0;
    const int32_t *seg_status = a.seg_status + seg0;
    // checked containers: the decoded bytes' crc, and the index's from k0
    const uint32_t *crc = it.check ? a.crc + seg0 : nullptr;
    const uint32_t *want_crc = reinterpret_cast<const uint32_t *>(a.in + it.in_off + 48 + 8 * it.n) + k0;
    if (tid == 0) s_bad = kNoSeg;
    __syncthreads();
    const int32_t top = (int32_t)a.ctl[item];
    // the lowest segment that failed, decoded cleanly to another length than its cut, or to that
    // length with another checksum (crc[i] is written exactly for those that reach it)
    if (top == 0)
        lowest_failing(count, &s_bad, [&](uint64_t i) {
            return seg_status[i] != 0 || out_lens[i] != out_caps[i] || (crc && crc[i] != want_crc[i]);
        });
    __syncthreads();
    if (tid != 0) return;
    const uint64_t bad = s_bad;
    int32_t st = top;
    uint64_t len = top == HC_ERR_CAPACITY ? length : 0;
    if (top == 0) {
        if (bad != kNoSeg) st = decoded_verdict(seg_status[bad], out_lens[bad], out_caps[bad]);
        else len = length;
    }
    a.status[item] = st;
    a.out_lens[item] = len;
    if (a.bad_segments) a.bad_segments[item] = bad == kNoSeg ? kNoSeg : k0 + bad;
}

// One decoder item on the host: its status when the host decides it (0: none), else its cuts, its
// range (whole: (0, raw_len)) and its sizes. The segment arrays hold the items in four groups, so
// that each launch covers one run of entries: plain unchecked, plain checked, adaptive checked,
// adaptive unchecked (FGK the first two, adaptive the last two, CRC the middle two). A single
// call's item is the one non-empty group, from entry 0 on.
struct DecOne {
    int hs;
    Cuts c;
    uint64_t offset, length;
    DecPlan p;
    uint32_t group;
    bool adapt, check;
};
DecOne dec_one(const hc_seg_dec_item_t &it)
{
    DecOne d;
    d.hs = 0;
    d.c = Cuts{0, 0, 0};
    d.offset = d.length = 0;
    d.p.cv = Cover{0, 0};
    d.p.nslots = d.p.slot = d.p.raw = 0;
    d.group = 0;
    d.adapt = d.check = false;
    if (!info_ok(it.info, it.in_len, d.c)) {
        d.hs = HC_ERR_SEG_HEADER;
        return d;
    }
    const bool whole = it.length == HC_SEG_WHOLE && it.offset == 0;
    d.offset = it.offset;
    d.length = whole ? it.info.raw_len : it.length;
    if (!whole && !range_ok(it.info.raw_len, it.offset, it.length)) {
        d.hs = HC_ERR_ARG;
        return d;
    }
    d.adapt = (it.info.flags & HC_FLAG_ADAPT) != 0;
    d.check = checked(it.info.flags);
    d.group = d.adapt ? (d.check ? 2u : 3u) : (d.check ? 1u : 0u);
    d.p = dec_plan(d.c, d.offset, d.length, whole);
    return d;
}

struct DecTotals {
    uint64_t seg[4];  // covered segments per group
    uint64_t count, nslots, slot_bytes;
    uint64_t a_enc, a_raw, a_count;  // the adaptive items: encoded bytes (a bound), raw bytes, segments
};
// enc_totals: per item, a bound of its covered segments' encoded bytes (null: in_len)
bool dec_totals(const hc_seg_dec_item_t *items, uint32_t n_items, const uint64_t *enc_totals, DecTotals &t)
{
    memset(&t, 0, sizeof(t));
    for (uint32_t i = 0; i < n_items; ++i) {
        const DecOne d = dec_one(items[i]);
        if (d.hs) continue;
        if (d.c.n > kMaxSegs) return false;
        t.seg[d.group] += d.p.cv.count;
        t.count += d.p.cv.count;
        t.nslots += d.p.nslots;
        t.slot_bytes += d.p.nslots * d.p.slot;
        if (d.adapt && d.p.cv.count) {
            t.a_enc += enc_totals ? enc_totals[i] : items[i].in_len;
            t.a_raw += d.p.raw;
            t.a_count += d.p.cv.count;
        }
        if (t.count > kMaxSegs) return false;
    }
    return true;
}
// single: the one-item call's layout (n_items 1)
DecWs dec_ws(void *work, bool single, uint32_t n_items, const DecTotals &t)
{
    const uint64_t aw = t.a_count ? hc::adapt_decode_work_bound(t.a_enc, t.a_raw, (uint32_t)t.a_count) : 0;
    if (single) return carve_dec(work, t.count, t.nslots, t.slot_bytes, aw, 4 * (t.seg[1] + t.seg[2]), 16, 0);
    return carve_dec(work, t.count, t.nslots, t.slot_bytes, aw, 4 * t.count, 8ull * n_items, n_items);
}

// the record of one item: skip what its compact upload leaves out; seg0, slot0 and slot_off where
// its entries of the segment arrays, of the copy arrays, and its slots start
DecItem dec_item(const hc_seg_dec_item_t &h, const DecOne &d, uint64_t skip, uint64_t seg0, uint64_t slot0,
                 uint64_t slot_off)
{
    DecItem r;
    memset(&r, 0, sizeof(r));
    r.hs = d.hs;
    if (d.hs) return r;
    return DecItem{h.in_off, h.in_len, skip,
                   h.info.flags & 0xFFFFu, h.info.raw_len, h.info.seg_bytes, h.info.width,
                   d.c.n, d.c.full, d.c.last, d.offset, d.length, h.out_cap,
                   d.p.cv.k0, d.p.cv.count, d.p.nslots, d.p.slot,
                   h.out_off, slot_off, seg0, slot0, d.check ? 1u : 0u, 0};
}

template <class Src>
int decode_launch(const Src &items, uint32_t n_items, const DecTotals &t, const DecWs &w, const uint8_t *in, uint8_t *out,
                  uint64_t *out_lens, int32_t *status, uint64_t *bad_segments, hipStream_t st);

// hc_seg_decompress_batch_dev; the host batch call passes its compact uploads' skips and spans
int decode_batch_dev(const uint8_t *in, uint8_t *out, const hc_seg_dec_item_t *items, uint32_t n_items,
                     uint64_t *out_lens, int32_t *status, uint64_t *bad_segments, void *work, uint64_t work_bytes,
                     void *stream, const uint64_t *skips, const uint64_t *enc_totals)
{
    if (n_items == 0) return HC_OK;
    if (!in || !out || !items || !out_lens || !status || !work) return HC_ERR_ARG;
    if (!aligned16(in) || !aligned16(out) || !aligned16(work)) return HC_ERR_ARG;
    for (uint32_t i = 0; i < n_items; ++i)
        if ((items[i].in_off | items[i].out_off) & 15u) return HC_ERR_ARG;
    DecTotals t;
    if (!dec_totals(items, n_items, enc_totals, t)) return HC_ERR_ARG;
    const DecWs w = dec_ws(work, false, n_items, t);
    if (work_bytes < w.total) return HC_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);

    // the groups' first entries, and the records
    uint64_t next[4] = {0, t.seg[0], t.seg[0] + t.seg[1], t.seg[0] + t.seg[1] + t.seg[2]};
    uint64_t slot0 = 0, slot_off = 0;
    ItemFeed<DecItem, kDecChunk> feed(w.items, st);
    for (uint32_t i = 0; i < n_items; ++i) {
        const DecOne d = dec_one(items[i]);
        feed.push(dec_item(items[i], d, skips ? skips[i] : 0, next[d.group], slot0, slot_off));
        if (d.hs) continue;
        next[d.group] += d.p.cv.count;
        slot0 += d.p.nslots;
        slot_off += d.p.nslots * d.p.slot;
    }
    feed.flush();
    HC_CK(hipGetLastError());
    return decode_launch(Many<DecItem>{w.items, n_items, nullptr}, n_items, t, w, in, out, out_lens, status, bad_segments,
                         st);
}

// The decoder's launches over the n_items records of `items`, whose covered segments fill the
// arrays of w group by group (t): open, the coder or coders, CRC, pack, close.
template <class Src>
int decode_launch(const Src &items, uint32_t n_items, const DecTotals &t, const DecWs &w, const uint8_t *in, uint8_t *out,
                  uint64_t *out_lens, int32_t *status, uint64_t *bad_segments, hipStream_t st)
{
    // the groups' runs of entries: FGK [0, n_fgk), adaptive the rest, CRC [crc0, crc0 + n_crc)
    const uint64_t n_fgk = t.seg[0] + t.seg[1], crc0 = t.seg[0], n_crc = t.seg[1] + t.seg[2];
    // one output base for the call: whichever of out and the slots lies lower
    uint8_t *base = (t.nslots && w.slots < out) ? w.slots : out;
    const DecCall dc{in, get64(kMagic), (uint64_t)(out - base), t.nslots ? (uint64_t)(w.slots - base) : 0,
                     w.in_offs, w.in_lens, w.out_offs, w.out_caps, w.out_lens,
                     w.cp_src, w.cp_len, w.cp_dst, w.status, w.crc, w.ctl, out_lens, bad_segments, status};
    seg_open_kernel<<<n_items, kScan, 0, st>>>(items, dc);
    HC_CK(hipGetLastError());
    if (n_fgk) {
        Batch b{in, w.in_offs, w.in_lens, (uint32_t)n_fgk, base, w.out_offs, w.out_caps, w.out_lens, w.status, 0};
        HC_CK(hc::launch_decode(b, hc::DST_RAW, st));
    }
    if (t.count > n_fgk) {
        Batch b{in, w.in_offs + n_fgk, w.in_lens + n_fgk, (uint32_t)(t.count - n_fgk), base, w.out_offs + n_fgk,
                w.out_caps + n_fgk, w.out_lens + n_fgk, w.status + n_fgk, 0};
        HC_CK(hc::adapt_decode_batch(b, w.awork, w.awork_bytes, st));
    }
    // the checked items' segments that decoded cleanly to their cut's length, staged or in place
    // (every covered one decodes whole, so its checksum is verifiable); an item whose verdict
    // is set has empty inputs, which no coder answers with status 0, so the per-segment gate
    // keeps the launch away from it
    if (n_crc)
        HC_CK(hc::launch_crc32(base, w.out_offs + crc0, w.out_caps + crc0, n_crc, w.crc + crc0,
                               hc::CrcGate{w.status + crc0, w.out_lens + crc0}, st));
    // the staged segments' covered parts to their places in out (empty copies when the verdict is set)
    if (t.nslots) HC_CK(hc::launch_pack(w.slots, w.cp_src, w.cp_len, (uint32_t)t.nslots, out, w.cp_dst, st));
    seg_close_kernel<<<n_items, kScan, 0, st>>>(items, dc);
    HC_CK(hipGetLastError());
    return HC_OK;
}

// The single calls' item: a range inside raw_len of a container whose info passed info_ok (whole:
// the range (0, raw_len) over every segment), and its workspace; enc_total as in dec_totals.
hc_seg_dec_item_t single_item(const hc_seg_info_t &info, uint64_t in_len, uint64_t offset, uint64_t length, bool whole,
                              uint64_t out_cap)
{
    return hc_seg_dec_item_t{0, in_len, info, whole ? 0 : offset, whole ? HC_SEG_WHOLE : length, 0, out_cap};
}
uint64_t single_work_bound(const hc_seg_info_t &info, uint64_t in_len, uint64_t offset, uint64_t length, bool whole,
                           uint64_t enc_total)
{
    const hc_seg_dec_item_t h = single_item(info, in_len, offset, length, whole, 0);
    DecTotals t;
    if (!dec_totals(&h, 1, &enc_total, t)) return 0;
    return dec_ws(nullptr, true, 1, t).total;
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
    if (!whole && !range_ok(info->raw_len, offset, length)) return HC_ERR_ARG;
    if (c.n > kMaxSegs) return HC_ERR_ARG;
    const hc_seg_dec_item_t h = single_item(*info, in_len, offset, length, whole, out_cap);
    DecTotals t;
    if (!dec_totals(&h, 1, &enc_total, t)) return HC_ERR_ARG;
    const DecWs w = dec_ws(work, true, 1, t);
    if (work_bytes < w.total) return HC_ERR_ARG;
    const One<DecItem> item{dec_item(h, dec_one(h), skip, 0, 0, 0)};
    return decode_launch(item, 1, t, w, in, out, out_len, status, bad_segment, st);
}

// ---------------------------------------------------------------------------------------------
// List read (hc_seg_decompress_ranges*): many byte ranges of one container, each covered segment
// decoded once. The host plans the read list (hc_seg_index.h): the covered segments, in container
// order, are the entries of one covered array, and covered entry c decodes whole to c full of a
// staging region (only the container's last segment has another length, and it can only be the
// last entry, so every entry starts 4-byte aligned and a read's bytes are one contiguous run).
//
//   rdesc    the read records, a chunk per launch as kernel arguments: the gather arrays
//   rplan    covered entry c: its segment and the decoder's output, c full of the staging region
//   ropen    one workgroup: header against the caller's copy, scan of the whole index (scan_index),
//            the stream of every covered segment; the index's verdict, then the capacity's: either
//            empties every decoder input and every gather range
//   <decode launch over the covered entries, into staging; checked containers: their CRC-32>
//   <pack launch: every read's bytes from staging to out + dst_off, at any byte alignment>
//   rclose   one workgroup: the lowest failing covered entry, as its container index; the outputs
// ---------------------------------------------------------------------------------------------
using hc_seg_index::ReadPlan;
using hc_seg_index::ReadRec;
constexpr uint32_t kReadChunk = 80;  // read records per descriptor launch

struct ReadWs {
    ReadRec *recs;
    uint64_t *g_src, *g_len, *g_dst;  // per read: g_len bytes from stage + g_src to out + g_dst
    uint64_t *cov_seg;                // per covered entry: its segment
    uint64_t *in_offs, *in_lens, *out_offs, *out_caps, *out_lens;  // per covered entry: the decoder's
    int32_t *status;
    uint32_t *crc;  // checked containers: the decoded segments' CRC-32
    uint64_t *ctl;  // [0] the open kernel's verdict (0, HC_ERR_SEG_HEADER, HC_ERR_CAPACITY)
    uint8_t *stage;
    void *awork;
    uint64_t awork_bytes, total;
};
ReadWs carve_reads(void *work, uint64_t P, uint64_t C, bool check, uint64_t stage_bytes, uint64_t awork_bytes)
{
    ReadWs w;
    Carver cv(work);
    w.recs = cv.arr<ReadRec>(P);
    w.g_src = cv.take64(P);
    w.g_len = cv.take64(P);
    w.g_dst = cv.take64(P);
    w.cov_seg = cv.take64(C);
    w.in_offs = cv.take64(C);
    w.in_lens = cv.take64(C);
    w.out_offs = cv.take64(C);
    w.out_caps = cv.take64(C);
    w.out_lens = cv.take64(C);
    w.status = cv.arr<int32_t>(C);
    w.crc = cv.arr<uint32_t>(check ? C : 0);
    w.ctl = cv.take64(2);
    w.stage = cv.take(stage_bytes);
    w.awork = cv.take(awork_bytes);
    w.awork_bytes = awork_bytes;
    w.total = cv.total();
    return w;
}
static_assert(sizeof(ReadRec) == 48, "the work bound of hcodec.h counts this");

// what the stages of a list read share
struct ReadCall {
    const uint8_t *in;
    uint64_t in_len, skip;  // skip: what the covered segments' input offsets lose (a compact upload)
    uint64_t out_cap, need;
    HeaderWords h;  // the caller's host copy
    uint64_t full, last;
    uint64_t P, C;
    uint32_t check;
    ReadWs w;
    uint64_t *out_len, *bad_segment;  // the call's three outputs
    int32_t *status;
};

struct ReadChunk {
    ReadRec rec[kReadChunk];
    ReadRec *recs;
    uint64_t *g_src, *g_len, *g_dst;
    uint64_t base;
    uint32_t count;
};
static_assert(sizeof(ReadChunk) <= 3968, "kernel arguments");

__global__ __launch_bounds__(128) void seg_rdesc_kernel(ReadChunk c)
{
    if (threadIdx.x >= c.count) return;
    const ReadRec r = c.rec[threadIdx.x];
    const uint64_t g = c.base + threadIdx.x;
    c.recs[g] = r;
    c.g_src[g] = r.src;
    c.g_len[g] = r.length;
    c.g_dst[g] = r.dst_off;
}

// Covered entry c: its segment and its place in the staging region. The record to go by is the last
// one whose e0 is <= c: e0 ascends over the list, that record's first segment lies in the same run
// of covered segments as entry c (a record of a later run has a higher e0, and the record that
// starts c's run has an e0 <= c), and inside a run k - c does not change.
__global__ __launch_bounds__(256) void seg_rplan_kernel(ReadCall a)
{
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    const ReadWs &w = a.w;
    uint64_t lo = 0, hi = a.P;  // recs[0].e0 is 0
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (w.recs[mid].e0 <= c) lo = mid;
        else hi = mid;
    }
    const uint64_t k = w.recs[lo].k0 + (c - w.recs[lo].e0);
    w.cov_seg[c] = k;
    w.in_offs[c] = 0;
    w.in_lens[c] = 0;
    w.out_offs[c] = c * a.full;
    w.out_caps[c] = k == a.h.n - 1 ? a.last : a.full;
    w.out_lens[c] = 0;
    w.status[c] = HC_ERR_DEVICE;  // overwritten by the decode launch
}

// scan_index for a list read: the stream of every covered segment (found in cov_seg, which
// ascends, by search). A failed index, or an output too small for the reads, empties every decoder
// input, which the coders answer with HC_ERR_HEADER before they touch anything (and which the CRC
// gate then passes over), and every gather range: nothing of the container is read, no byte of out
// is written.
__global__ __launch_bounds__(kScan) void seg_ropen_kernel(ReadCall a)
{
    const uint32_t tid = threadIdx.x;
    const ReadWs &w = a.w;
    const bool bad = scan_index(a.in, a.h, a.in_len, a.check != 0, [&](uint64_t k, uint64_t off, uint64_t len) {
        uint64_t lo = 0, hi = a.C;  // the first entry whose segment is >= k
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (w.cov_seg[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        if (lo < a.C && w.cov_seg[lo] == k) {
            w.in_offs[lo] = off - a.skip;
            w.in_lens[lo] = len;
        }
    });
    const int32_t st = bad ? HC_ERR_SEG_HEADER : (a.out_cap < a.need ? HC_ERR_CAPACITY : 0);
    if (tid == 0) w.ctl[0] = (uint64_t)st;
    if (st == 0) return;
    for (uint64_t c = tid; c < a.C; c += kScan) w.in_lens[c] = 0;
    for (uint64_t i = tid; i < a.P; i += kScan) w.g_len[i] = 0;
}

// the verdict over the covered entries; bad_segment is the container's index
__global__ __launch_bounds__(kScan) void seg_rclose_kernel(ReadCall a)
{
    __shared__ unsigned long long s_bad;
    const uint32_t tid = threadIdx.x;
    const ReadWs &w = a.w;
    // checked containers: the decoded bytes' crc against the index's
    const uint32_t *want_crc = a.check ? reinterpret_cast<const uint32_t *>(a.in + 48 + 8 * a.h.n) : nullptr;
    if (tid == 0) s_bad = kNoSeg;
    __syncthreads();
    const int32_t top = (int32_t)w.ctl[0];
    if (top == 0)
        lowest_failing(a.C, &s_bad, [&](uint64_t c) {
            return w.status[c] != 0 || w.out_lens[c] != w.out_caps[c] || (want_crc && w.crc[c] != want_crc[w.cov_seg[c]]);
        });
    __syncthreads();
    if (tid != 0) return;
    const uint64_t bad = s_bad;
    int32_t st = top;
    uint64_t len = top == HC_ERR_CAPACITY ? a.need : 0;
    if (top == 0) {
        if (bad != kNoSeg) st = decoded_verdict(w.status[bad], w.out_lens[bad], w.out_caps[bad]);
        else len = a.need;
    }
    *a.status = st;
    *a.out_len = len;
    if (a.bad_segment) *a.bad_segment = bad == kNoSeg ? kNoSeg : w.cov_seg[bad];
}

// the sizes of a list read whose info passed info_ok and whose reads passed reads_ok; enc_total: a
// bound of the covered segments' encoded bytes (the adaptive decoder's workspace goes by it)
struct ReadSizes {
    Cuts c;
    ReadPlan u;
    uint64_t need, awork_bytes;
    bool adapt, check;
};
ReadSizes read_sizes(const hc_seg_info_t &info, uint64_t in_len, const hc_seg_read_t *reads, uint32_t n_reads,
                     uint64_t enc_total, ReadRec *recs)
{
    ReadSizes s;
    (void)info_ok(info, in_len, s.c);
    (void)hc_seg_index::reads_ok(info.raw_len, reads, n_reads, &s.need);
    s.adapt = (info.flags & HC_FLAG_ADAPT) != 0;
    s.check = checked(info.flags);
    s.u = hc_seg_index::reads_plan(s.c, info.raw_len, reads, n_reads, recs);
    s.awork_bytes = (s.adapt && s.u.covered && s.u.covered <= kMaxSegs)
                        ? hc::adapt_decode_work_bound(enc_total, s.u.cov_raw, (uint32_t)s.u.covered)
                        : 0;
    return s;
}
ReadWs reads_ws(void *work, const ReadSizes &s, uint32_t n_reads)
{
    return carve_reads(work, n_reads, s.u.covered, s.check, s.u.cov_raw, s.awork_bytes);
}

// hc_seg_decompress_ranges_dev; the host call passes its compact upload's skip and span
int reads_dev(const uint8_t *in, uint64_t in_len, const hc_seg_info_t *info, const hc_seg_read_t *reads,
              uint32_t n_reads, uint8_t *out, uint64_t out_cap, uint64_t *out_len, int32_t *status, uint64_t *bad_segment,
              void *work, uint64_t work_bytes, void *stream, uint64_t skip, uint64_t enc_total)
{
    if (!in || !info || !out || !out_len || !status || !work || (!reads && n_reads)) return HC_ERR_ARG;
    if (!aligned16(in) || !aligned16(out) || !aligned16(work)) return HC_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Cuts c;
    if (!info_ok(*info, in_len, c)) {
        seg_reject_kernel<<<1, 1, 0, st>>>(out_len, status, bad_segment);
        HC_CK(hipGetLastError());
        return HC_OK;
    }
    if (!hc_seg_index::reads_ok(info->raw_len, reads, n_reads, nullptr)) return HC_ERR_ARG;
    std::vector<ReadRec> recs(n_reads);
    const ReadSizes s = read_sizes(*info, in_len, reads, n_reads, enc_total, recs.data());
    if (s.u.covered > kMaxSegs) return HC_ERR_ARG;
    const ReadWs w = reads_ws(work, s, n_reads);
    if (work_bytes < w.total) return HC_ERR_ARG;
    const uint64_t P = n_reads, C = s.u.covered;
    const ReadCall a{in, in_len, skip, out_cap, s.need,
                     HeaderWords{get64(kMagic), info->flags & 0xFFFFu, info->raw_len, info->seg_bytes, info->width, c.n},
                     c.full, c.last, P, C, s.check ? 1u : 0u, w, out_len, bad_segment, status};

    for (uint64_t base = 0; base < P; base += kReadChunk) {
        ReadChunk ch;
        ch.count = (uint32_t)(P - base < kReadChunk ? P - base : kReadChunk);
        memcpy(ch.rec, recs.data() + base, sizeof(ReadRec) * ch.count);
        ch.recs = w.recs;
        ch.g_src = w.g_src;
        ch.g_len = w.g_len;
        ch.g_dst = w.g_dst;
        ch.base = base;
        seg_rdesc_kernel<<<1, 128, 0, st>>>(ch);
    }
    if (C) seg_rplan_kernel<<<(uint32_t)((C + 255) / 256), 256, 0, st>>>(a);
    seg_ropen_kernel<<<1, kScan, 0, st>>>(a);
    HC_CK(hipGetLastError());
    if (C) {
        Batch b{in, w.in_offs, w.in_lens, (uint32_t)C, w.stage, w.out_offs, w.out_caps, w.out_lens, w.status, 0};
        if (s.adapt) HC_CK(hc::adapt_decode_batch(b, w.awork, w.awork_bytes, st));
        else HC_CK(hc::launch_decode(b, hc::DST_RAW, st));
        // every covered segment decodes whole, so its checksum is verifiable; the gate keeps the launch
        // away from one that did not decode cleanly to its cut's length
        if (s.check)
            HC_CK(hc::launch_crc32(w.stage, w.out_offs, w.out_caps, C, w.crc, hc::CrcGate{w.status, w.out_lens}, st));
        // every read's bytes to its place in out (empty copies when the open kernel's verdict is set)
        HC_CK(hc::launch_pack(w.stage, w.g_src, w.g_len, n_reads, out, w.g_dst, st));
    }
    seg_rclose_kernel<<<1, kScan, 0, st>>>(a);
    HC_CK(hipGetLastError());
    return HC_OK;
}

// ---------------------------------------------------------------------------------------------
// Range write (hc_seg_update*): the container with some raw byte ranges overwritten, without
// recoding the rest. The host plans the patch list (hc_seg_index.h): the covered segments, in
// container order, are the entries of one covered array, and those that a patch covers only in part
// are also the entries of a decoded array. Covered entry c keeps its raw bytes at c full of a
// staging region (only the container's last segment has another length, and it can only be the
// last entry, so every entry starts 4-byte aligned) and its new stream in a bound-sized slot.
//
//   upatch   the patch records, a chunk per launch as kernel arguments: the pack arrays and the
//            decoded entries' covered entries
//   uplan    covered entry c: its segment, its staging range, its slot
//   uopen    one workgroup: header against the caller's copy, scan of the whole index (scan_index),
//            the old place of every covered segment, the decoder's arrays
//   <decode_to_stage: decode launch over the decoded entries, into staging; checked containers:
//    their CRC-32>
//   <code_from_stage: pack launch, every patch's bytes over the staging region; checked
//    containers: CRC-32 of the covered entries' new raw bytes; encode launch into the slots>
//   useal    one workgroup: the verdict (seal_failed, seal_fits), and the pieces of the new
//            container: 2 C + 1 of them, old block j (the old bytes between covered entries j - 1
//            and j; the first one holds the header and the index) at 2 j and covered entry j's slot
//            at 2 j + 1, each at the next multiple of 16 after the one before
//   splice   the pieces to their places, 16 bytes per lane; gated by the verdict
//   uindex   the covered segments' enc_len and crc words over the copied index; gated too
//
// The append below runs the same stages over its own coded entries: what the two keep per coded
// entry, per decoded entry and per piece is one block of the workspace (CodedWs), and what they do
// with it (the plan of an entry, the coder launches, the seal's verdict, the splice) is written
// once, here.
// ---------------------------------------------------------------------------------------------
using hc_seg_index::PatchRec;
using hc_seg_index::UpdPlan;
constexpr uint32_t kPatchChunk = 48;  // patch records per descriptor launch
constexpr uint32_t kSpliceChunks = 8;  // 16-byte chunks per lane and tile: a workgroup's tile is 32 KiB

// What a write call (the range write, the append) keeps of the C segments it codes, of the D among
// them that it decodes first, and of the 2 C + 1 pieces its result is spliced from. Coded entry c
// has its raw bytes at c full of the staging region and its new stream in a bound-sized slot.
struct CodedWs {
    uint64_t *in_offs, *in_lens, *widths, *slot_offs, *slot_caps, *enc_lens;  // per coded entry
    int32_t *status;
    uint32_t *crc;  // checked containers
    uint64_t *pc_src, *pc_dst, *pc_len;  // per piece
    uint64_t *d_in_offs, *d_in_lens, *d_out_offs, *d_out_caps, *d_out_lens;  // per decoded entry
    int32_t *d_status;
    uint32_t *d_crc;  // checked containers
    // [0] 1: sealed, the splice may copy; [1] the spliced bytes' end; [2] the open kernel's verdict;
    // from [3] on: the operation's own
    uint64_t *ctl;
    uint8_t *stage, *slots;
    void *awork;
    uint64_t awork_bytes;
};
CodedWs carve_coded(Carver &cv, uint64_t C, uint64_t D, bool check, uint64_t ctl_words, uint64_t stage_bytes,
                    uint64_t slot_bytes, uint64_t awork_bytes)
{
    CodedWs w;
    w.in_offs = cv.take64(C);
    w.in_lens = cv.take64(C);
    w.widths = cv.take64(C);
    w.slot_offs = cv.take64(C);
    w.slot_caps = cv.take64(C);
    w.enc_lens = cv.take64(C);
    w.status = cv.arr<int32_t>(C);
    w.crc = cv.arr<uint32_t>(check ? C : 0);
    w.pc_src = cv.take64(2 * C + 1);
    w.pc_dst = cv.take64(2 * C + 1);
    w.pc_len = cv.take64(2 * C + 1);
    w.d_in_offs = cv.take64(D);
    w.d_in_lens = cv.take64(D);
    w.d_out_offs = cv.take64(D);
    w.d_out_caps = cv.take64(D);
    w.d_out_lens = cv.take64(D);
    w.d_status = cv.arr<int32_t>(D);
    w.d_crc = cv.arr<uint32_t>(check ? D : 0);
    w.ctl = cv.take64(ctl_words);
    w.stage = cv.take(stage_bytes);
    w.slots = cv.take(slot_bytes);
    w.awork = cv.take(awork_bytes);
    w.awork_bytes = awork_bytes;
    return w;
}

// a write call's three outputs
struct WriteOut {
    uint64_t *out_len, *bad_segment;
    int32_t *status;
};

// coded entry c: `len` raw bytes at in_off of the staging region, and `cap` bytes at slot_off of the slots
__device__ __forceinline__ void plan_coded(const CodedWs &w, uint64_t c, uint64_t in_off, uint64_t len,
                                           uint64_t width, uint64_t slot_off, uint64_t cap)
{
    w.in_offs[c] = in_off;
    w.in_lens[c] = len;
    w.widths[c] = width;
    w.slot_offs[c] = slot_off;
    w.slot_caps[c] = cap;
    w.enc_lens[c] = 0;
    w.status[c] = HC_ERR_DEVICE;  // overwritten by the encode launch
}
// decoded entry d: its stream in the old container (none when the open kernel failed: nothing of
// the container is read), and its cut's place in the staging region
__device__ __forceinline__ void plan_decoded(const CodedWs &w, uint64_t d, bool bad, uint64_t in_off,
                                             uint64_t in_len, uint64_t out_off, uint64_t cut)
{
    w.d_in_offs[d] = bad ? 0 : in_off;
    w.d_in_lens[d] = bad ? 0 : in_len;
    w.d_out_offs[d] = out_off;
    w.d_out_caps[d] = cut;
    w.d_out_lens[d] = 0;
    w.d_status[d] = HC_ERR_DEVICE;  // overwritten by the decode launch
}

// The verdict of a write call before its pieces, by the seal's whole workgroup: the open kernel's,
// else that of the lowest failing decoded entry (seg_close_kernel's rules), else the own status of
// the lowest failing coded entry (an encoder never fails in a bound-sized slot; if one does, the
// call must not succeed). want_crc: the old index's crc words, read in a checked container alone;
// seg_d(d), seg_c(c): the container's segment of a decoded, of a coded entry. True: the call
// failed, its outputs say so, and nothing will be spliced.
template <class SegD, class SegC>
__device__ __forceinline__ bool seal_failed(const CodedWs &w, uint64_t D, uint64_t C, const uint32_t *want_crc,
                                            const WriteOut &o, SegD seg_d, SegC seg_c)
{
    __shared__ unsigned long long s_dbad, s_ebad;
    if (threadIdx.x == 0) s_dbad = s_ebad = kNoSeg;
    __syncthreads();
    const int32_t top = (int32_t)w.ctl[2];
    if (top == 0) {
        lowest_failing(D, &s_dbad, [&](uint64_t d) {
            return w.d_status[d] != 0 || w.d_out_lens[d] != w.d_out_caps[d] ||
                   (want_crc && w.d_crc[d] != want_crc[seg_d(d)]);
        });
        lowest_failing(C, &s_ebad, [&](uint64_t c) { return w.status[c] != 0; });
    }
    __syncthreads();
    const uint64_t dbad = s_dbad, ebad = s_ebad;
    int32_t st = top;
    uint64_t bad_seg = kNoSeg;
    if (dbad != kNoSeg) {
        st = decoded_verdict(w.d_status[dbad], w.d_out_lens[dbad], w.d_out_caps[dbad]);
        bad_seg = seg_d(dbad);
    } else if (ebad != kNoSeg) {
        st = w.status[ebad];
        bad_seg = seg_c(ebad);
    }
    if (st == 0) return false;
    if (threadIdx.x == 0) {
        *o.status = st;
        *o.out_len = 0;
        if (o.bad_segment) *o.bad_segment = bad_seg;
        w.ctl[0] = 0;
        w.ctl[1] = 0;
    }
    return true;
}
// The verdict after the pieces, by one thread: the container ends at `end`, the spliced bytes at `spliced`
__device__ __forceinline__ void seal_fits(const CodedWs &w, const WriteOut &o, uint64_t out_cap, uint64_t end,
                                          uint64_t spliced)
{
    const bool fits = end <= out_cap;
    *o.status = fits ? 0 : HC_ERR_CAPACITY;
    *o.out_len = end;
    if (o.bad_segment) *o.bad_segment = kNoSeg;
    w.ctl[0] = fits ? 1 : 0;
    w.ctl[1] = spliced;
}

struct UpdWs {
    PatchRec *recs;
    uint64_t *pk_src, *pk_len, *pk_dst;      // per patch
    uint64_t *d_cov;                         // per decoded entry: its covered entry
    uint64_t *cov_seg, *old_off, *old_len;   // per covered entry: its segment and that segment's old place
    CodedWs co;                              // the covered entries are the coded ones; 4 ctl words
    uint64_t total;
};
UpdWs carve_upd(void *work, uint64_t P, uint64_t D, uint64_t C, bool check, uint64_t stage_bytes, uint64_t slot_bytes,
                uint64_t awork_bytes)
{
    UpdWs w;
    Carver cv(work);
    w.recs = cv.arr<PatchRec>(P);
    w.pk_src = cv.take64(P);
    w.pk_len = cv.take64(P);
    w.pk_dst = cv.take64(P);
    w.d_cov = cv.take64(D);
    w.cov_seg = cv.take64(C);
    w.old_off = cv.take64(C);
    w.old_len = cv.take64(C);
    w.co = carve_coded(cv, C, D, check, 4, stage_bytes, slot_bytes, awork_bytes);
    w.total = cv.total();
    return w;
}
static_assert(sizeof(PatchRec) == 64, "the work bound of hcodec.h counts this");

// what the stages of a range write share
struct UpdCall {
    const uint8_t *in;
    uint8_t *out;
    uint64_t in_len, out_cap;
    HeaderWords h;  // the caller's host copy
    uint64_t full, last, slot_full, cap_full, cap_last;
    uint64_t P, D, C;
    uint32_t check;
    UpdWs w;
    WriteOut o;
};

struct PatchChunk {
    PatchRec rec[kPatchChunk];
    PatchRec *recs;
    uint64_t *pk_src, *pk_len, *pk_dst, *d_cov;
    uint64_t base;
    uint32_t count;
};
static_assert(sizeof(PatchChunk) <= 3968, "kernel arguments");

__global__ __launch_bounds__(64) void seg_upatch_kernel(PatchChunk c)
{
    if (threadIdx.x >= c.count) return;
    const PatchRec r = c.rec[threadIdx.x];
    const uint64_t g = c.base + threadIdx.x;
    c.recs[g] = r;
    c.pk_src[g] = r.src_off;
    c.pk_len[g] = r.length;
    c.pk_dst[g] = r.dst;
    if (r.dmask & 1) c.d_cov[r.d0] = r.e0;
    if (r.dmask & 2) c.d_cov[r.d0 + (r.dmask & 1)] = r.e0 + r.cnt - 1;
}

// covered entry c: its segment (the record that holds it is the last one whose e0 is <= c: a
// record without new segments shares its e0 with the next one, which the search passes), its
// staging range and its slot
__global__ __launch_bounds__(256) void seg_uplan_kernel(UpdCall a)
{
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    uint64_t lo = 0, hi = a.P;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a.w.recs[mid].e0 <= c) lo = mid;
        else hi = mid;
    }
    const uint64_t k = a.w.recs[lo].k0 + (c - a.w.recs[lo].e0);
    const bool tail = k == a.h.n - 1;
    a.w.cov_seg[c] = k;
    a.w.old_off[c] = 0;
    a.w.old_len[c] = 0;
    plan_coded(a.w.co, c, c * a.full, tail ? a.last : a.full, a.h.width, c * a.slot_full, tail ? a.cap_last : a.cap_full);
}

// scan_index for a range write: the old place of every covered segment (found in cov_seg, which
// ascends, by search), then the decoder's arrays from those. On failure every decoder input is
// empty: nothing of the container is read. (The encoders still code what the staging region
// holds, into their slots; the seal's verdict keeps it from out.)
__global__ __launch_bounds__(kScan) void seg_uopen_kernel(UpdCall a)
{
    const uint32_t tid = threadIdx.x;
    const UpdWs &w = a.w;
    const bool bad = scan_index(a.in, a.h, a.in_len, a.check != 0, [&](uint64_t k, uint64_t off, uint64_t len) {
        uint64_t lo = 0, hi = a.C;  // the first entry whose segment is >= k
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (w.cov_seg[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        if (lo < a.C && w.cov_seg[lo] == k) {
            w.old_off[lo] = off;
            w.old_len[lo] = len;
        }
    });
    if (tid == 0) w.co.ctl[2] = bad ? (uint64_t)HC_ERR_SEG_HEADER : 0;
    for (uint64_t d = tid; d < a.D; d += kScan) {
        const uint64_t c = w.d_cov[d];
        plan_decoded(w.co, d, bad, w.old_off[c], w.old_len[c], c * a.full, w.cov_seg[c] == a.h.n - 1 ? a.last : a.full);
    }
}

// The verdict (seal_failed, then the capacity) and the pieces. Piece p starts at the sum of
// align16(length) of the pieces before it.
__global__ __launch_bounds__(kScan) void seg_useal_kernel(UpdCall a)
{
    __shared__ uint64_t part[kScan / 64];
    __shared__ unsigned long long s_end;
    const uint32_t tid = threadIdx.x;
    const UpdWs &u = a.w;
    const CodedWs &w = u.co;
    const uint32_t *want_crc = a.check ? reinterpret_cast<const uint32_t *>(a.in + 48 + 8 * a.h.n) : nullptr;
    if (seal_failed(w, a.D, a.C, want_crc, a.o, [&](uint64_t d) { return u.cov_seg[u.d_cov[d]]; },
                    [&](uint64_t c) { return u.cov_seg[c]; }))
        return;
    // the index tiles the old container exactly (uopen), so no sum below can wrap
    const uint64_t pieces = 2 * a.C + 1;
    const bool tail_covered = a.C && u.cov_seg[a.C - 1] == a.h.n - 1;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < pieces; base += kScan) {
        const uint64_t p = base + tid, j = p >> 1;
        const bool in = p < pieces;
        uint64_t src = 0, len = 0;
        if (in && (p & 1)) {
            src = w.slot_offs[j];
            len = w.enc_lens[j];
        } else if (in) {
            const uint64_t be = j == a.C ? a.in_len : u.old_off[j];
            src = j == 0 ? 0 : align16(u.old_off[j - 1] + u.old_len[j - 1]);
            if (src > be) src = be;  // after the container's last segment
            len = be - src;
        }
        uint64_t total;
        const uint64_t dst = carry + block_scan(in ? align16(len) : 0, part, total);
        if (in) {
            w.pc_src[p] = src;
            w.pc_dst[p] = dst;
            w.pc_len[p] = len;
            // the container ends with its last segment's last byte: bytes
            if (p == (tail_covered ? pieces - 2 : pieces - 1)) s_end = dst + len;
        }
        carry += total;
    }
    __syncthreads();
    if (tid == 0) seal_fits(w, a.o, a.out_cap, s_end, s_end);
}

// The pieces to their places. Output chunk g (16 bytes at 16 g) belongs to the last piece whose
// start is <= 16 g (a piece without bytes shares its start with the next one). A workgroup takes
// tiles of 256 x kSpliceChunks chunks, whatever pieces they fall in: two lanes find the pieces of
// the tile's first and last chunk, and every lane searches between those alone, so a block of
// hundreds of megabytes is as many workgroups' work as its bytes call for. Sources and
// destinations are 16-byte aligned. A piece's last chunk, when it is short, goes out byte by byte
// with its padding zeroed, except at the container's end, where nothing follows the last byte.
struct SpliceCall {
    const uint8_t *in;     // the even pieces' source: the old container
    const uint8_t *slots;  // the odd pieces' source
    uint8_t *out;
    const uint64_t *pc_src, *pc_dst, *pc_len;
    const uint64_t *ctl;  // [0] 1: sealed; [1] the spliced bytes' end
    uint64_t pieces;
};
__global__ __launch_bounds__(256) void seg_splice_kernel(SpliceCall a)
{
    __shared__ uint64_t s_p[2];
    if (a.ctl[0] == 0) return;  // not sealed: nothing is copied
    const uint64_t end = a.ctl[1], chunks = (end + 15) / 16, pieces = a.pieces;
    constexpr uint64_t kTile = 256ull * kSpliceChunks;
    auto find = [&](uint64_t x, uint64_t lo, uint64_t hi) {  // pc_dst[lo] <= x; hi: one past the candidates
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (a.pc_dst[mid] <= x) lo = mid;
            else hi = mid;
        }
        return lo;
    };
    for (uint64_t g0 = (uint64_t)blockIdx.x * kTile; g0 < chunks; g0 += (uint64_t)gridDim.x * kTile) {
        const uint64_t g1 = (g0 + kTile < chunks ? g0 + kTile : chunks) - 1;
        __syncthreads();  // the tile before is done with s_p
        if (threadIdx.x == 0) s_p[0] = find(16 * g0, 0, pieces);
        if (threadIdx.x == 64) s_p[1] = find(16 * g1, 0, pieces);
        __syncthreads();
        const uint64_t p_lo = s_p[0], p_hi = s_p[1] + 1;
        const u32x4 *src[kSpliceChunks];
        uint64_t rest[kSpliceChunks];  // the piece's bytes from this chunk on (0: no chunk)
        bool last_piece[kSpliceChunks];
#pragma unroll
        for (uint32_t i = 0; i < kSpliceChunks; ++i) {
            const uint64_t g = g0 + (uint64_t)i * 256 + threadIdx.x;
            rest[i] = 0;
            src[i] = nullptr;
            last_piece[i] = false;
            if (g > g1) continue;
            const uint64_t p = find(16 * g, p_lo, p_hi), off = 16 * g - a.pc_dst[p], len = a.pc_len[p];
            if (off >= len) continue;  // (never: a piece's chunks end with its last byte's)
            rest[i] = len - off;
            src[i] = reinterpret_cast<const u32x4 *>(((p & 1) ? a.slots : a.in) + a.pc_src[p] + off);
            last_piece[i] = 16 * g + rest[i] == end;
        }
        u32x4 v[kSpliceChunks];
#pragma unroll
        for (uint32_t i = 0; i < kSpliceChunks; ++i)
            if (rest[i] >= 16) v[i] = *src[i];
#pragma unroll
        for (uint32_t i = 0; i < kSpliceChunks; ++i) {
            const uint64_t g = g0 + (uint64_t)i * 256 + threadIdx.x;
            if (rest[i] >= 16) {
                reinterpret_cast<u32x4 *>(a.out)[g] = v[i];
            } else if (rest[i]) {
                const uint8_t *s8 = reinterpret_cast<const uint8_t *>(src[i]);
                uint8_t *d8 = a.out + 16 * g;
                for (uint32_t b = 0; b < (uint32_t)rest[i]; ++b) d8[b] = s8[b];
                if (!last_piece[i])
                    for (uint32_t b = (uint32_t)rest[i]; b < 16; ++b) d8[b] = 0;
            }
        }
    }
}

// the covered segments' index words, from the seal's arrays
__global__ __launch_bounds__(256) void seg_uindex_kernel(UpdCall a)
{
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C || a.w.co.ctl[0] == 0) return;
    const uint64_t k = a.w.cov_seg[c];
    reinterpret_cast<uint64_t *>(a.out)[6 + k] = a.w.co.enc_lens[c];
    if (a.check) reinterpret_cast<uint32_t *>(a.out)[12 + 2 * a.h.n + k] = a.w.co.crc[c];
}

// What both write calls size their coded entries by: the slots of a full cut and of the new
// container's last one, and the adaptive coders' workspace.
struct CodedSizes {
    uint64_t cap_full, cap_last, slot_full, slot_bytes, awork_bytes;
    bool adapt, check;
};
CodedSizes coded_sizes(const hc_seg_info_t &info, uint64_t full, uint64_t last)
{
    CodedSizes s;
    s.adapt = (info.flags & HC_FLAG_ADAPT) != 0;
    s.check = checked(info.flags);
    s.cap_full = hc_compress_bound(full, s.adapt);
    s.cap_last = hc_compress_bound(last, s.adapt);
    s.slot_full = align16(s.cap_full);
    s.slot_bytes = s.awork_bytes = 0;
    return s;
}
// C entries of coded_raw bytes in all are coded after D entries of dec_raw bytes, out of dec_in
// bytes of streams, are decoded (more than kMaxSegs entries: the caller refuses the call)
uint64_t coded_awork(bool adapt, uint64_t C, uint64_t coded_raw, uint64_t D, uint64_t dec_in, uint64_t dec_raw)
{
    if (!adapt || C > kMaxSegs) return 0;
    const uint64_t e = C ? hc::adapt_encode_work_bound(coded_raw, (uint32_t)C) : 0;
    const uint64_t d = D ? hc::adapt_decode_work_bound(dec_in, dec_raw, (uint32_t)D) : 0;
    return e > d ? e : d;  // the decode launch is over before the encode launch starts
}

// The coder launches of a write call, in the two halves that the append plans between. First the
// D decoded entries from the old container into the staging region and, in a checked container,
// the CRC-32 of those that decoded cleanly to their cut's length.
int decode_to_stage(const uint8_t *in, const CodedWs &w, uint64_t D, const CodedSizes &s, hipStream_t st)
{
    if (!D) return HC_OK;
    Batch b{in, w.d_in_offs, w.d_in_lens, (uint32_t)D, w.stage, w.d_out_offs, w.d_out_caps, w.d_out_lens, w.d_status, 0};
    if (s.adapt) HC_CK(hc::adapt_decode_batch(b, w.awork, w.awork_bytes, st));
    else HC_CK(hc::launch_decode(b, hc::DST_RAW, st));
    if (s.check)
        HC_CK(hc::launch_crc32(w.stage, w.d_out_offs, w.d_out_caps, D, w.d_crc, hc::CrcGate{w.d_status, w.d_out_lens}, st));
    return HC_OK;
}
// Then n_pack ranges of new bytes from `src` over the staging region, at any byte alignment (an
// empty range costs nothing), in a checked container the CRC-32 of the C coded cuts, and the
// encode launch into the slots.
int code_from_stage(const uint8_t *src, const uint64_t *pk_src, const uint64_t *pk_len, const uint64_t *pk_dst,
                    uint32_t n_pack, const CodedWs &w, uint64_t C, const CodedSizes &s, uint32_t flags, hipStream_t st)
{
    if (!C) return HC_OK;
    HC_CK(hc::launch_pack(src, pk_src, pk_len, n_pack, w.stage, pk_dst, st));
    Batch b{w.stage, w.in_offs, w.in_lens, (uint32_t)C, w.slots, w.slot_offs, w.slot_caps, w.enc_lens, w.status,
            flags & HC_FLAG_DIFF};
    if (s.check) HC_CK(hc::launch_crc32(w.stage, w.in_offs, w.in_lens, C, w.crc, hc::CrcGate{nullptr, nullptr}, st));
    if (s.adapt) HC_CK(hc::adapt_encode_batch(b, w.widths, w.awork, w.awork_bytes, st));
    else HC_CK(hc::launch_encode(b, (flags & HC_FLAG_DIFF) ? hc::SRC_RAW_DIFF : hc::SRC_RAW, st));
    return HC_OK;
}
// The splice over the seal's pieces; the grid by the longest result there can be (the rest by stride)
void launch_splice(const uint8_t *in, uint8_t *out, const CodedWs &w, uint64_t C, uint64_t longest, hipStream_t st)
{
    const uint64_t tiles = longest / (4096ull * kSpliceChunks) + 1;
    seg_splice_kernel<<<(uint32_t)(tiles < 4096 ? tiles : 4096), 256, 0, st>>>(
        SpliceCall{in, w.slots, out, w.pc_src, w.pc_dst, w.pc_len, w.ctl, 2 * C + 1});
}

// the sizes of a range write whose info passed info_ok and whose patches passed patches_ok
struct UpdSizes {
    Cuts c;
    UpdPlan u;
    CodedSizes co;
    uint64_t stage_bytes;
};
UpdSizes upd_sizes(const hc_seg_info_t &info, uint64_t in_len, const hc_seg_patch_t *patches, uint32_t n_patches,
                   PatchRec *recs)
{
    UpdSizes s;
    (void)info_ok(info, in_len, s.c);
    s.co = coded_sizes(info, s.c.full, s.c.last);
    s.u = hc_seg_index::update_plan(s.c, info.raw_len, patches, n_patches, s.co.slot_full, align16(s.co.cap_last), recs);
    s.stage_bytes = align16(s.u.cov_raw);
    s.co.slot_bytes = s.u.cov_bound;
    s.co.awork_bytes = coded_awork(s.co.adapt, s.u.covered, s.u.cov_raw, s.u.decoded, in_len, s.u.dec_raw);
    return s;
}
UpdWs upd_ws(void *work, const UpdSizes &s, uint32_t n_patches)
{
    return carve_upd(work, n_patches, s.u.decoded, s.u.covered, s.co.check, s.stage_bytes, s.co.slot_bytes,
                     s.co.awork_bytes);
}

// ---------------------------------------------------------------------------------------------
// Append (hc_seg_append*): the container of raw followed by add from the container of raw, without recoding
// the rest. The host plans the cuts (hc_seg_index.h): segments 0 .. K - 1 are kept, and the coded
// segments K .. n' - 1 hold the open tail (old segment n - 1 when it is not yet a complete cut; the
// only segment that is ever decoded) and the added bytes. Coded entry c keeps its raw bytes at
// c full of a staging region and its new stream in a bound-sized slot, as in the range write.
//
//   aopen    one workgroup: header against the caller's copy, scan of the whole index (scan_index),
//            the kept block (segment 0's first byte to segment K - 1's last), the decoder's one entry
//   <decode_to_stage: decode launch of old segment n - 1 to staging offset 0; checked containers:
//    its CRC-32>
//   aplan    coded entry c: its staging range, its slot, its own part of the added bytes as one
//            pack range (so a large append packs on as many workgroups as it codes segments)
//   <code_from_stage: pack launch, the added bytes behind the open tail, at any byte alignment;
//    checked containers: CRC-32 of the coded cuts; encode launch into the slots>
//   aseal    one workgroup: the verdict (seal_failed, seal_fits), the new segments' places, and the
//            copy pieces in the range write's layout (2 C + 1 of them: the kept block at 0, coded
//            entry c's slot at 2 c + 1, nothing at the other even places)
//   splice   the range write's splice kernel moves the pieces, 16 bytes per lane; gated
//   aindex   the new header words, enc_len[0 .. n'), crc[0 .. n') (kept entries from the old index
//            at its old place), the zero padding up to the first segment; gated
//
// The host call runs the same stages on a compact upload (header, index, old segment n - 1's
// stream: `skip` is what that stream's offset loses) and in gather mode: the kept block stays on
// the host, the pieces are the slots alone, packed from byte 0 of a device buffer, and aindex is
// not run (the host writes the index from the coded entries' words).
// ---------------------------------------------------------------------------------------------
using hc_seg_index::AppPlan;

struct AppWs {
    // the one decoded entry is carved whether the call decodes or not; 8 ctl words: [3], [4] the kept
    // block's first byte in `in` and its length
    CodedWs co;
    uint64_t *pk_src, *pk_len, *pk_dst;  // per coded entry: its part of the added bytes
    uint64_t total;
};
AppWs carve_app(void *work, uint64_t C, bool check, uint64_t stage_bytes, uint64_t slot_bytes, uint64_t awork_bytes)
{
    AppWs w;
    Carver cv(work);
    w.pk_src = cv.take64(C);
    w.pk_len = cv.take64(C);
    w.pk_dst = cv.take64(C);
    w.co = carve_coded(cv, C, 1, check, 8, stage_bytes, slot_bytes, awork_bytes);
    w.total = cv.total();
    return w;
}

// what the stages of an append share
struct AppCall {
    const uint8_t *in;
    uint8_t *out;
    uint64_t in_len, out_cap, skip;
    HeaderWords h;         // the old header, the caller's host copy
    uint64_t full, last;   // the old cuts
    uint64_t new_raw, new_n, new_last;                    // the new header words and the new last cut
    uint64_t K, C, D, tail, add_len;
    uint64_t slot_full, cap_full, cap_last;
    uint32_t check, gather;
    AppWs w;
    WriteOut o;
};

// scan_index for an append: where the kept block ends and where old segment n - 1 lies. On failure
// the decoder's input is empty: nothing of the container is read.
__global__ __launch_bounds__(kScan) void seg_aopen_kernel(AppCall a)
{
    __shared__ uint64_t s_kept_end, s_last_off, s_last_len;
    const uint32_t tid = threadIdx.x;
    const uint64_t first = align16(index_end(a.h.n, a.check != 0));
    if (tid == 0) {
        s_kept_end = first;
        s_last_off = s_last_len = 0;
    }
    const bool bad = scan_index(a.in, a.h, a.in_len, a.check != 0, [&](uint64_t k, uint64_t off, uint64_t len) {
        if (k + 1 == a.K) s_kept_end = off + len;
        if (k == a.h.n - 1) {
            s_last_off = off;
            s_last_len = len;
        }
    });
    if (tid != 0) return;
    const CodedWs &w = a.w.co;
    w.ctl[2] = bad ? (uint64_t)HC_ERR_SEG_HEADER : 0;
    w.ctl[3] = first;
    w.ctl[4] = bad ? 0 : s_kept_end - first;  // (K == 0: nothing is kept)
    if (a.D) plan_decoded(w, 0, bad, s_last_off - a.skip, s_last_len, 0, a.last);
}

// coded entry c: its staging range, its slot, and the added bytes that fall into its cut: the
// staging region holds the open tail in [0, tail) and the added bytes in [tail, tail + add_len)
__global__ __launch_bounds__(256) void seg_aplan_kernel(AppCall a)
{
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    const AppWs &w = a.w;
    const bool tail = c == a.C - 1;
    const uint64_t b = c * a.full, e = b + (tail ? a.new_last : a.full);
    const uint64_t lo = b > a.tail ? b : a.tail;  // (e <= tail + add_len: the cuts end with the added bytes)
    w.pk_src[c] = lo < e ? lo - a.tail : 0;
    w.pk_len[c] = lo < e ? e - lo : 0;
    w.pk_dst[c] = lo < e ? lo : 0;
    plan_coded(w.co, c, b, e - b, a.h.width, c * a.slot_full, tail ? a.cap_last : a.cap_full);
}

// The verdict (the decoded segment by seg_close_kernel's mapping, then the capacity), the new
// segments' places and the pieces. The kept block goes to align16 of the new index end, the coded
// entries follow it, each at the next multiple of 16. In gather mode the kept block is no piece and
// the places count from the first coded segment's.
__global__ __launch_bounds__(kScan) void seg_aseal_kernel(AppCall a)
{
    __shared__ uint64_t part[kScan / 64];
    __shared__ unsigned long long s_end;
    const uint32_t tid = threadIdx.x;
    const CodedWs &w = a.w.co;
    const uint64_t kept_len = w.ctl[4];
    const uint64_t first = align16(index_end(a.new_n, a.check != 0)), base0 = first + align16(kept_len);
    // no coded entry: nothing is added, the kept block is the old container's rest
    if (tid == 0) s_end = first + kept_len;
    const uint32_t *want_crc = a.check ? reinterpret_cast<const uint32_t *>(a.in + 48 + 8 * a.h.n) : nullptr;
    if (seal_failed(w, a.D, a.C, want_crc, a.o, [&](uint64_t) { return a.h.n - 1; }, [&](uint64_t c) { return a.K + c; }))
        return;
    // the index tiles the old container exactly (aopen) and every enc_len fits its slot, so no sum below can wrap
    const uint64_t shift = a.gather ? base0 : 0;
    if (tid == 0) {
        w.pc_src[0] = w.ctl[3];
        w.pc_dst[0] = a.gather ? 0 : first;
        w.pc_len[0] = a.gather ? 0 : kept_len;
    }
    uint64_t carry = base0;
    for (uint64_t base = 0; base < a.C; base += kScan) {
        const uint64_t c = base + tid;
        const bool in = c < a.C;
        const uint64_t len = in ? w.enc_lens[c] : 0;
        uint64_t total;
        const uint64_t dst = carry + block_scan(in ? align16(len) : 0, part, total);
        if (in) {
            w.pc_src[2 * c + 1] = w.slot_offs[c];
            w.pc_dst[2 * c + 1] = dst - shift;
            w.pc_len[2 * c + 1] = len;
            w.pc_src[2 * c + 2] = 0;  // (the range write's old block between two covered entries: none here)
            w.pc_dst[2 * c + 2] = dst + align16(len) - shift;
            w.pc_len[2 * c + 2] = 0;
            if (c == a.C - 1) s_end = dst + len;  // the container ends with its last segment's last byte
        }
        carry += total;
    }
    __syncthreads();
    if (tid == 0) seal_fits(w, a.o, a.out_cap, s_end, s_end - shift);
}

// The new header and index in front of the spliced bytes: header words 0 .. 5 (raw_len and
// n_segments new), enc_len[0 .. n') and, in a checked container, crc[0 .. n'): the kept entries from
// the old index, whose crc words lie at their old place behind 8 n bytes of lengths, the coded
// entries from the seal's arrays; then the zero padding up to the first segment.
__global__ __launch_bounds__(256) void seg_aindex_kernel(AppCall a)
{
    const CodedWs &w = a.w.co;
    if (w.ctl[0] == 0) return;  // not sealed: nothing is written
    const uint64_t *i64 = reinterpret_cast<const uint64_t *>(a.in);
    const uint32_t *i32 = reinterpret_cast<const uint32_t *>(a.in);
    uint64_t *o64 = reinterpret_cast<uint64_t *>(a.out);
    uint32_t *o32 = reinterpret_cast<uint32_t *>(a.out);
    const uint64_t idx_end = index_end(a.new_n, a.check != 0);
    if (blockIdx.x == 0 && threadIdx.x >= 8 && threadIdx.x < 14) {
        const uint32_t t = threadIdx.x - 8;
        o64[t] = t == 0 ? a.h.magic : t == 1 ? a.h.flags : t == 2 ? a.new_raw : t == 3 ? a.h.seg_bytes
                 : t == 4 ? a.h.width : a.new_n;
    }
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < a.new_n; k += (uint64_t)gridDim.x * 256) {
        o64[6 + k] = k < a.K ? i64[6 + k] : w.enc_lens[k - a.K];
        if (a.check) o32[12 + 2 * a.new_n + k] = k < a.K ? i32[12 + 2 * a.h.n + k] : w.crc[k - a.K];
    }
    if (blockIdx.x == 0 && threadIdx.x < (align16(idx_end) - idx_end) / 4) o32[idx_end / 4 + threadIdx.x] = 0;
}

// the sizes of an append whose info passed info_ok
struct AppSizes {
    Cuts c;
    AppPlan p;
    CodedSizes co;
};
// HC_OK, or the status that the host decides (HC_ERR_ARG, HC_ERR_MATRIX_SIZE). dec_in: the decoded
// segment's stream length when the host knows it (the host call); null: the longest stream this
// library writes for that cut, or in_len when that is less.
int app_sizes(const hc_seg_info_t &info, uint64_t in_len, uint64_t add_len, const uint64_t *dec_in, AppSizes &s)
{
    (void)info_ok(info, in_len, s.c);
    const bool adapt = (info.flags & HC_FLAG_ADAPT) != 0;
    const int rc = hc_seg_index::append_plan(s.c, info.raw_len, add_len, info.seg_bytes, adapt, info.width, &s.p);
    if (rc) return rc;
    if (s.p.coded > kMaxSegs) return HC_ERR_ARG;
    s.co = coded_sizes(info, s.c.full, s.p.nc.last);
    s.co.slot_bytes = hc_seg_index::append_slots(s.p, s.co.slot_full, align16(s.co.cap_last));
    const uint64_t old_bound = hc_compress_bound(s.c.last, 1);
    const uint64_t din = dec_in ? *dec_in : (in_len < old_bound ? in_len : old_bound);
    s.co.awork_bytes = coded_awork(adapt, s.p.coded, s.p.stage, s.p.decoded, din, s.c.last);
    return HC_OK;
}
AppWs app_ws(void *work, const AppSizes &s)
{
    return carve_app(work, s.p.coded, s.co.check, s.p.stage, s.co.slot_bytes, s.co.awork_bytes);
}

// hc_seg_append_dev, and the host call's device part (gather; `in` is then its compact upload and
// `out` its buffer for the coded streams, while in_len and out_cap stay the caller's)
int append_dev(const uint8_t *in, uint64_t in_len, const hc_seg_info_t *info, const uint8_t *add, uint64_t add_len,
               uint8_t *out, uint64_t out_cap, uint64_t *out_len, int32_t *status, uint64_t *bad_segment, void *work,
               uint64_t work_bytes, void *stream, bool gather, uint64_t skip, const uint64_t *dec_in)
{
    if (!in || !info || !out || !out_len || !status || !work || (!add && add_len)) return HC_ERR_ARG;
    if (!aligned16(in) || !aligned16(out) || !aligned16(work)) return HC_ERR_ARG;
    if (!gather) {
        const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), o0 = reinterpret_cast<uintptr_t>(out);
        if (i0 < o0 ? in_len > o0 - i0 : out_cap > i0 - o0) return HC_ERR_ARG;  // the two buffers overlap
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    Cuts c;
    if (!info_ok(*info, in_len, c)) {
        seg_reject_kernel<<<1, 1, 0, st>>>(out_len, status, bad_segment);
        HC_CK(hipGetLastError());
        return HC_OK;
    }
    AppSizes s;
    const int rc = app_sizes(*info, in_len, add_len, dec_in, s);
    if (rc) return rc;
    const AppWs w = app_ws(work, s);
    if (work_bytes < w.total) return HC_ERR_ARG;
    const uint64_t C = s.p.coded, D = s.p.decoded;
    const AppCall a{in, out, in_len, out_cap, skip,
                    HeaderWords{get64(kMagic), info->flags & 0xFFFFu, info->raw_len, info->seg_bytes, info->width, c.n},
                    c.full, c.last, info->raw_len + add_len, s.p.nc.n, s.p.nc.last,
                    s.p.K, C, D, s.p.tail, add_len, s.co.slot_full, s.co.cap_full, s.co.cap_last,
                    s.co.check ? 1u : 0u, gather ? 1u : 0u, w, WriteOut{out_len, bad_segment, status}};

    seg_aopen_kernel<<<1, kScan, 0, st>>>(a);
    HC_CK(hipGetLastError());
    if (decode_to_stage(in, w.co, D, s.co, st) != HC_OK) return HC_ERR_DEVICE;
    if (C) {
        seg_aplan_kernel<<<(uint32_t)((C + 255) / 256), 256, 0, st>>>(a);
        HC_CK(hipGetLastError());
    }
    // the added bytes behind the open tail, one range per coded entry
    if (code_from_stage(add, w.pk_src, w.pk_len, w.pk_dst, (uint32_t)C, w.co, C, s.co, info->flags, st) != HC_OK)
        return HC_ERR_DEVICE;
    seg_aseal_kernel<<<1, kScan, 0, st>>>(a);
    const uint64_t longest =
        gather ? s.co.slot_bytes : hc_seg_index::append_bound(s.p, in_len, c.n, s.co.check, s.co.slot_bytes);
    launch_splice(in, out, w.co, C, longest, st);
    if (!gather) {
        const uint64_t blocks = (s.p.nc.n + 255) / 256;
        seg_aindex_kernel<<<(uint32_t)(blocks < 65536 ? blocks : 65536), 256, 0, st>>>(a);
    }
    HC_CK(hipGetLastError());
    return HC_OK;
}

// the host batch calls' sub-batch limit, as hc_pipe.hip reads it
uint64_t pipe_bytes()
{
    const char *v = getenv("HC_PIPE_BYTES");
    const uint64_t x = (v && *v) ? strtoull(v, nullptr, 0) : 0;
    return x ? x : 1ull << 30;
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
    const EncWs w = carve_enc(work, p.c.n, p.slot_bytes, p.awork_bytes, checked(flags));
    if (work_bytes < w.total) return HC_ERR_ARG;
    const One<EncItem> item{enc_item(hc_seg_enc_item_t{0, in_len, width, 0, out_cap}, 0, p, use_adapt, 0, 0)};
    return encode_launch(item, 1, p.c.n, w, w.ctl, in, out, flags, seg_bytes, out_len, status,
                         static_cast<hipStream_t>(stream));
}

uint64_t hc_seg_decompress_work_bound(const hc_seg_info_t *info, uint64_t in_len)
{
    if (!info) return 0;
    Cuts c;
    if (!info_ok(*info, in_len, c) || c.n > kMaxSegs) return 16;  // rejected without a workspace
    return single_work_bound(*info, in_len, 0, 0, true, in_len);
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
    return single_work_bound(*info, in_len, offset, length, false, in_len);
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
    hc_seg_info_t info;
    if (hc_seg_info(in, in_len, &info) != HC_OK) return fail(HC_ERR_SEG_HEADER, 0, out_len, bad_segment);
    if (!range_ok(info.raw_len, offset, length)) return HC_ERR_ARG;
    Cuts c;
    (void)info_ok(info, in_len, c);
    if (c.n > kMaxSegs) return HC_ERR_ARG;
    // the index on the host: the verdict without a device, and the covered segments' bytes [s0, s1)
    uint64_t s0 = 0, s1 = 0;
    const bool check = checked(info.flags);
    const uint64_t idx = align16(index_end(c.n, check));
    if (hc_seg_index::index_scan(in, in_len, c.n, check, range_cover(c, offset, length), &s0, &s1) != HC_OK)
        return fail(HC_ERR_SEG_HEADER, 0, out_len, bad_segment);
    if (!hc_device_ok()) return fail(HC_ERR_DEVICE, 0, out_len, bad_segment);
    if (out_cap < length) return fail(HC_ERR_CAPACITY, length, out_len, bad_segment);
    (void)fail(HC_OK, 0, out_len, bad_segment);  // (what a HIP error below leaves behind)
    // the compact upload: header and index [0, idx), then the span; in_len stays the container's
    const uint64_t span = s1 - s0;
    const uint64_t wb = single_work_bound(info, in_len, offset, length, false, span);
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
    const int status = read_verdict(meta, st, out_len, bad_segment);
    if (status) return status;
    if (*out_len) HC_CK(hipMemcpy(out, dout.p, *out_len, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_seg_reads_segments(const hc_seg_info_t *info, uint64_t in_len, const hc_seg_read_t *reads, uint32_t n_reads,
                          uint64_t *n_covered, uint64_t *need)
{
    if (!info || !n_covered || !need) return HC_ERR_ARG;
    Cuts c;
    uint64_t top = 0;
    if (!info_ok(*info, in_len, c) || !hc_seg_index::reads_ok(info->raw_len, reads, n_reads, &top)) return HC_ERR_ARG;
    *n_covered = hc_seg_index::reads_plan(c, info->raw_len, reads, n_reads, nullptr).covered;
    *need = top;
    return HC_OK;
}

uint64_t hc_seg_decompress_ranges_work_bound(const hc_seg_info_t *info, uint64_t in_len, const hc_seg_read_t *reads,
                                             uint32_t n_reads)
{
    if (!info) return 0;
    Cuts c;
    if (!info_ok(*info, in_len, c)) return 16;  // rejected without a workspace
    if (!hc_seg_index::reads_ok(info->raw_len, reads, n_reads, nullptr)) return 0;
    const ReadSizes s = read_sizes(*info, in_len, reads, n_reads, in_len, nullptr);
    if (s.u.covered > kMaxSegs) return 0;
    return reads_ws(nullptr, s, n_reads).total;
}

int hc_seg_decompress_ranges_dev(const uint8_t *in, uint64_t in_len, const hc_seg_info_t *info,
                                 const hc_seg_read_t *reads, uint32_t n_reads, uint8_t *out, uint64_t out_cap,
                                 uint64_t *out_len, int32_t *status, uint64_t *bad_segment, void *work,
                                 uint64_t work_bytes, void *stream)
{
    return reads_dev(in, in_len, info, reads, n_reads, out, out_cap, out_len, status, bad_segment, work, work_bytes, stream,
                     0, in_len);
}

int hc_seg_decompress_ranges(const uint8_t *in, uint64_t in_len, const hc_seg_read_t *reads, uint32_t n_reads,
                             uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *bad_segment)
{
    if ((!in && in_len) || !out_len || (!out && out_cap) || (!reads && n_reads)) return HC_ERR_ARG;
    hc_seg_info_t info;
    if (hc_seg_info(in, in_len, &info) != HC_OK) return fail(HC_ERR_SEG_HEADER, 0, out_len, bad_segment);
    if (!hc_seg_index::reads_ok(info.raw_len, reads, n_reads, nullptr)) return HC_ERR_ARG;
    ReadSizes s = read_sizes(info, in_len, reads, n_reads, in_len, nullptr);
    if (s.u.covered > kMaxSegs) return HC_ERR_ARG;
    // the index on the host: the verdict without a device, and the encoded bytes [s0, s1) from the
    // first covered segment's stream to the last covered one's
    uint64_t s0 = 0, s1 = 0;
    const uint64_t idx = align16(index_end(s.c.n, s.check));
    const Cover span_cv = s.u.covered ? Cover{s.u.k_lo, s.u.k_hi - s.u.k_lo + 1} : Cover{0, 0};
    if (hc_seg_index::index_scan(in, in_len, s.c.n, s.check, span_cv, &s0, &s1) != HC_OK)
        return fail(HC_ERR_SEG_HEADER, 0, out_len, bad_segment);
    if (!hc_device_ok()) return fail(HC_ERR_DEVICE, 0, out_len, bad_segment);
    if (out_cap < s.need) return fail(HC_ERR_CAPACITY, s.need, out_len, bad_segment);
    (void)fail(HC_OK, 0, out_len, bad_segment);  // (what a HIP error below leaves behind)
    // the compact upload: header and index [0, idx), then the span; in_len stays the container's
    const uint64_t span = s1 - s0;
    s = read_sizes(info, in_len, reads, n_reads, span, nullptr);  // the adaptive workspace by the span's own length
    const uint64_t wb = reads_ws(nullptr, s, n_reads).total;
    hipStream_t st = nullptr;
    DevBuf din, dout, work, meta;
    HC_CK(din.alloc(idx + span + 16));
    HC_CK(dout.alloc(s.need + 16));
    HC_CK(work.alloc(wb));
    HC_CK(meta.alloc(32));
    HC_CK(hipMemcpyAsync(din.p, in, idx, hipMemcpyHostToDevice, st));
    if (span) HC_CK(hipMemcpyAsync(din.as<uint8_t>() + idx, in + s0, span, hipMemcpyHostToDevice, st));
    uint64_t *m = meta.as<uint64_t>();
    const int rc = reads_dev(din.as<uint8_t>(), in_len, &info, reads, n_reads, dout.as<uint8_t>(), s.need, m,
                             reinterpret_cast<int32_t *>(m + 1), m + 2, work.p, wb, st, s0 - idx, span);
    if (rc) return rc;
    const int status = read_verdict(meta, st, out_len, bad_segment);
    if (status) return status;
    // the destination bytes [0, need) come down, and go into out read by read: no byte outside the
    // destination ranges is written here either
    if (s.need) {
        std::vector<uint8_t> down(s.need);
        HC_CK(hipMemcpy(down.data(), dout.p, s.need, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n_reads; ++i)
            if (reads[i].length) memcpy(out + reads[i].dst_off, down.data() + reads[i].dst_off, reads[i].length);
    }
    return HC_OK;
}

int hc_seg_rect_reads(uint64_t raw_len, uint64_t pitch, uint64_t x, uint64_t y, uint64_t w, uint64_t h,
                      hc_seg_read_t *reads)
{
    if (!reads && h) return HC_ERR_ARG;
    return hc_seg_index::rect_reads(raw_len, pitch, x, y, w, h, reads) ? HC_OK : HC_ERR_ARG;
}

int hc_seg_update_segments(const hc_seg_info_t *info, uint64_t in_len, const hc_seg_patch_t *patches,
                           uint32_t n_patches, uint64_t *n_covered, uint64_t *n_decoded)
{
    if (!info || !n_covered || !n_decoded) return HC_ERR_ARG;
    Cuts c;
    if (!info_ok(*info, in_len, c) || !hc_seg_index::patches_ok(info->raw_len, patches, n_patches, nullptr))
        return HC_ERR_ARG;
    const UpdPlan u = hc_seg_index::update_plan(c, info->raw_len, patches, n_patches, 0, 0, nullptr);
    *n_covered = u.covered;
    *n_decoded = u.decoded;
    return HC_OK;
}

uint64_t hc_seg_update_bound(const hc_seg_info_t *info, uint64_t in_len, const hc_seg_patch_t *patches,
                             uint32_t n_patches)
{
    if (!info) return 0;
    Cuts c;
    if (!info_ok(*info, in_len, c) || !hc_seg_index::patches_ok(info->raw_len, patches, n_patches, nullptr)) return 0;
    return sat_add(in_len, upd_sizes(*info, in_len, patches, n_patches, nullptr).co.slot_bytes);
}

uint64_t hc_seg_update_work_bound(const hc_seg_info_t *info, uint64_t in_len, const hc_seg_patch_t *patches,
                                  uint32_t n_patches)
{
    if (!info) return 0;
    Cuts c;
    if (!info_ok(*info, in_len, c)) return 16;  // rejected without a workspace
    if (!hc_seg_index::patches_ok(info->raw_len, patches, n_patches, nullptr)) return 0;
    const UpdSizes s = upd_sizes(*info, in_len, patches, n_patches, nullptr);
    if (s.u.covered > kMaxSegs) return 0;
    return upd_ws(nullptr, s, n_patches).total;
}

int hc_seg_update_dev(const uint8_t *in, uint64_t in_len, const hc_seg_info_t *info, const hc_seg_patch_t *patches,
                      uint32_t n_patches, const uint8_t *patch_data, uint64_t patch_data_len, uint8_t *out,
                      uint64_t out_cap, uint64_t *out_len, int32_t *status, uint64_t *bad_segment, void *work,
                      uint64_t work_bytes, void *stream)
{
    if (!in || !info || !out || !out_len || !status || !work) return HC_ERR_ARG;
    if ((!patches && n_patches) || (!patch_data && patch_data_len)) return HC_ERR_ARG;
    if (!aligned16(in) || !aligned16(out) || !aligned16(work)) return HC_ERR_ARG;
    {
        const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), o0 = reinterpret_cast<uintptr_t>(out);
        if (i0 < o0 ? in_len > o0 - i0 : out_cap > i0 - o0) return HC_ERR_ARG;  // the two buffers overlap
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    Cuts c;
    if (!info_ok(*info, in_len, c)) {
        seg_reject_kernel<<<1, 1, 0, st>>>(out_len, status, bad_segment);
        HC_CK(hipGetLastError());
        return HC_OK;
    }
    if (!hc_seg_index::patches_ok(info->raw_len, patches, n_patches, &patch_data_len)) return HC_ERR_ARG;
    std::vector<PatchRec> recs(n_patches);
    const UpdSizes s = upd_sizes(*info, in_len, patches, n_patches, recs.data());
    if (s.u.covered > kMaxSegs) return HC_ERR_ARG;
    const UpdWs w = upd_ws(work, s, n_patches);
    if (work_bytes < w.total) return HC_ERR_ARG;
    const uint64_t P = n_patches, D = s.u.decoded, C = s.u.covered;
    const UpdCall a{in, out, in_len, out_cap,
                    HeaderWords{get64(kMagic), info->flags & 0xFFFFu, info->raw_len, info->seg_bytes, info->width, c.n},
                    c.full, c.last, s.co.slot_full, s.co.cap_full, s.co.cap_last,
                    P, D, C, s.co.check ? 1u : 0u, w, WriteOut{out_len, bad_segment, status}};

    for (uint64_t base = 0; base < P; base += kPatchChunk) {
        PatchChunk ch;
        ch.count = (uint32_t)(P - base < kPatchChunk ? P - base : kPatchChunk);
        memcpy(ch.rec, recs.data() + base, sizeof(PatchRec) * ch.count);
        ch.recs = w.recs;
        ch.pk_src = w.pk_src;
        ch.pk_len = w.pk_len;
        ch.pk_dst = w.pk_dst;
        ch.d_cov = w.d_cov;
        ch.base = base;
        seg_upatch_kernel<<<1, 64, 0, st>>>(ch);
    }
    if (C) seg_uplan_kernel<<<(uint32_t)((C + 255) / 256), 256, 0, st>>>(a);
    seg_uopen_kernel<<<1, kScan, 0, st>>>(a);
    HC_CK(hipGetLastError());
    if (decode_to_stage(in, w.co, D, s.co, st) != HC_OK) return HC_ERR_DEVICE;
    // every patch's bytes over the covered segments' raw bytes
    if (code_from_stage(patch_data, w.pk_src, w.pk_len, w.pk_dst, n_patches, w.co, C, s.co, info->flags, st) != HC_OK)
        return HC_ERR_DEVICE;
    seg_useal_kernel<<<1, kScan, 0, st>>>(a);
    // the longest result there can be: the old container and every slot filled
    launch_splice(in, out, w.co, C, in_len + s.co.slot_bytes, st);
    if (C) seg_uindex_kernel<<<(uint32_t)((C + 255) / 256), 256, 0, st>>>(a);
    HC_CK(hipGetLastError());
    return HC_OK;
}

int hc_seg_update(const uint8_t *in, uint64_t in_len, const hc_seg_patch_t *patches, uint32_t n_patches,
                  const uint8_t *patch_data, uint64_t patch_data_len, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                  uint64_t *bad_segment)
{
    if ((!in && in_len) || !out_len || (!out && out_cap)) return HC_ERR_ARG;
    if ((!patches && n_patches) || (!patch_data && patch_data_len)) return HC_ERR_ARG;
    hc_seg_info_t info;
    if (hc_seg_info(in, in_len, &info) != HC_OK) return fail(HC_ERR_SEG_HEADER, 0, out_len, bad_segment);
    if (!hc_seg_index::patches_ok(info.raw_len, patches, n_patches, &patch_data_len)) return HC_ERR_ARG;
    const UpdSizes s = upd_sizes(info, in_len, patches, n_patches, nullptr);
    if (s.u.covered > kMaxSegs) return HC_ERR_ARG;
    uint64_t s0 = 0, s1 = 0;
    if (hc_seg_index::index_scan(in, in_len, s.c.n, s.co.check, Cover{0, 0}, &s0, &s1) != HC_OK)
        return fail(HC_ERR_SEG_HEADER, 0, out_len, bad_segment);
    if (!hc_device_ok()) return fail(HC_ERR_DEVICE, 0, out_len, bad_segment);
    (void)fail(HC_OK, 0, out_len, bad_segment);  // (what a HIP error below leaves behind)
    // the whole container and every patch byte go up, the whole result comes down
    const uint64_t bound = sat_add(in_len, s.co.slot_bytes), cap = out_cap < bound ? out_cap : bound;
    const uint64_t wb = upd_ws(nullptr, s, n_patches).total;
    hipStream_t st = nullptr;
    DevBuf din, dpatch, dout, work, meta;
    HC_CK(din.alloc(in_len + 16));
    HC_CK(dpatch.alloc(patch_data_len + 16));
    HC_CK(dout.alloc(cap + 16));
    HC_CK(work.alloc(wb));
    HC_CK(meta.alloc(32));
    HC_CK(hipMemcpyAsync(din.p, in, in_len, hipMemcpyHostToDevice, st));
    if (patch_data_len) HC_CK(hipMemcpyAsync(dpatch.p, patch_data, patch_data_len, hipMemcpyHostToDevice, st));
    uint64_t *m = meta.as<uint64_t>();
    const int rc = hc_seg_update_dev(din.as<uint8_t>(), in_len, &info, patches, n_patches, dpatch.as<uint8_t>(),
                                     patch_data_len, dout.as<uint8_t>(), cap, m, reinterpret_cast<int32_t *>(m + 1), m + 2,
                                     work.p, wb, st);
    if (rc) return rc;
    const int status = read_verdict(meta, st, out_len, bad_segment);
    if (status) return status;
    if (*out_len) HC_CK(hipMemcpy(out, dout.p, *out_len, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_seg_append_plan(const hc_seg_info_t *info, uint64_t in_len, uint64_t add_len, hc_seg_info_t *new_info,
                       uint64_t *first_coded, uint64_t *n_decoded)
{
    if (!info || !new_info || !first_coded || !n_decoded) return HC_ERR_ARG;
    Cuts c;
    if (!info_ok(*info, in_len, c)) return HC_ERR_ARG;
    AppPlan p;
    const int rc = hc_seg_index::append_plan(c, info->raw_len, add_len, info->seg_bytes,
                                             (info->flags & HC_FLAG_ADAPT) != 0, info->width, &p);
    if (rc) return rc;
    *new_info = *info;
    new_info->raw_len = info->raw_len + add_len;
    new_info->n_segments = p.nc.n;
    *first_coded = p.K;
    *n_decoded = p.decoded;
    return HC_OK;
}

uint64_t hc_seg_append_bound(const hc_seg_info_t *info, uint64_t in_len, uint64_t add_len)
{
    if (!info) return 0;
    Cuts c;
    AppSizes s;
    if (!info_ok(*info, in_len, c) || app_sizes(*info, in_len, add_len, nullptr, s) != HC_OK) return 0;
    return hc_seg_index::append_bound(s.p, in_len, c.n, s.co.check, s.co.slot_bytes);
}

uint64_t hc_seg_append_work_bound(const hc_seg_info_t *info, uint64_t in_len, uint64_t add_len)
{
    if (!info) return 0;
    Cuts c;
    if (!info_ok(*info, in_len, c)) return 16;  // rejected without a workspace
    AppSizes s;
    if (app_sizes(*info, in_len, add_len, nullptr, s) != HC_OK) return 0;
    return app_ws(nullptr, s).total;
}

int hc_seg_append_dev(const uint8_t *in, uint64_t in_len, const hc_seg_info_t *info, const uint8_t *add,
                      uint64_t add_len, uint8_t *out, uint64_t out_cap, uint64_t *out_len, int32_t *status,
                      uint64_t *bad_segment, void *work, uint64_t work_bytes, void *stream)
{
    return append_dev(in, in_len, info, add, add_len, out, out_cap, out_len, status, bad_segment, work, work_bytes,
                      stream, false, 0, nullptr);
}

int hc_seg_append(const uint8_t *in, uint64_t in_len, const uint8_t *add, uint64_t add_len, uint8_t *out,
                  uint64_t out_cap, uint64_t *out_len, uint64_t *bad_segment)
{
    if ((!in && in_len) || !out_len || (!out && out_cap) || (!add && add_len)) return HC_ERR_ARG;
    hc_seg_info_t info;
    if (hc_seg_info(in, in_len, &info) != HC_OK) return fail(HC_ERR_SEG_HEADER, 0, out_len, bad_segment);
    AppSizes s;
    {
        const int rc = app_sizes(info, in_len, add_len, nullptr, s);
        if (rc) return rc;
    }
    // The index on the host: the verdict without a device, and the kept block's last byte. Old segment
    // n - 1, when it is not kept, starts at the next multiple of 16 and ends with the container.
    const bool check = s.co.check;
    const uint64_t n = s.c.n, K = s.p.K, C = s.p.coded;
    const uint64_t first = align16(index_end(n, check)), new_first = align16(index_end(s.p.nc.n, check));
    uint64_t s0 = 0, kept_end = 0;
    if (hc_seg_index::index_scan(in, in_len, n, check, K ? Cover{K - 1, 1} : Cover{0, 0}, &s0, &kept_end) != HC_OK)
        return fail(HC_ERR_SEG_HEADER, 0, out_len, bad_segment);
    if (!hc_device_ok()) return fail(HC_ERR_DEVICE, 0, out_len, bad_segment);
    if (K == 0) kept_end = first;
    const uint64_t kept_len = kept_end - first;
    if (C == 0) {  // nothing is added: the input container
        if (in_len > out_cap) return fail(HC_ERR_CAPACITY, in_len, out_len, bad_segment);
        memcpy(out, in, in_len);
        return fail(HC_OK, in_len, out_len, bad_segment);
    }
    (void)fail(HC_OK, 0, out_len, bad_segment);  // (what a HIP error below leaves behind)
    // The compact upload: header and index [0, first), then old segment n - 1's stream when it is
    // decoded; in_len stays the container's. The kept bytes never leave the host.
    const uint64_t last_off = K == n ? in_len : align16(kept_end);
    const uint64_t dec_in = s.p.decoded ? in_len - last_off : 0;
    {
        const int rc = app_sizes(info, in_len, add_len, &dec_in, s);  // the decoder's workspace by the stream's own length
        if (rc) return rc;
    }
    const uint64_t wb = app_ws(nullptr, s).total;
    hipStream_t st = nullptr;
    DevBuf din, dadd, dout, work, meta;
    HC_CK(din.alloc(first + dec_in + 16));
    HC_CK(dadd.alloc(add_len + 16));
    HC_CK(dout.alloc(s.co.slot_bytes + 16));
    HC_CK(work.alloc(wb));
    HC_CK(meta.alloc(32));
    HC_CK(hipMemcpyAsync(din.p, in, first, hipMemcpyHostToDevice, st));
    if (dec_in) HC_CK(hipMemcpyAsync(din.as<uint8_t>() + first, in + last_off, dec_in, hipMemcpyHostToDevice, st));
    HC_CK(hipMemcpyAsync(dadd.p, add, add_len, hipMemcpyHostToDevice, st));
    uint64_t *m = meta.as<uint64_t>();
    const int rc = append_dev(din.as<uint8_t>(), in_len, &info, dadd.as<uint8_t>(), add_len, dout.as<uint8_t>(), out_cap, m,
                              reinterpret_cast<int32_t *>(m + 1), m + 2, work.p, wb, st, true, last_off - first, &dec_in);
    if (rc) return rc;
    const int status = read_verdict(meta, st, out_len, bad_segment);
    if (status) return status;
    // the result on the host: header, index, the kept block from `in`, the coded streams as gathered
    const CodedWs w = app_ws(work.p, s).co;
    const uint64_t new_n = s.p.nc.n, base = new_first + align16(kept_len), gathered = *out_len - base;
    std::vector<uint64_t> lens(C);
    std::vector<uint32_t> crcs(check ? C : 0);
    HC_CK(hipMemcpyAsync(lens.data(), w.enc_lens, 8 * C, hipMemcpyDeviceToHost, st));
    if (check) HC_CK(hipMemcpyAsync(crcs.data(), w.crc, 4 * C, hipMemcpyDeviceToHost, st));
    HC_CK(hipMemcpyAsync(out + base, dout.p, gathered, hipMemcpyDeviceToHost, st));
    memcpy(out, in, 16);
    const uint64_t words[4] = {info.raw_len + add_len, info.seg_bytes, info.width, new_n};
    memcpy(out + 16, words, 32);
    memcpy(out + 48, in + 48, 8 * K);
    if (check) memcpy(out + 48 + 8 * new_n, in + 48 + 8 * n, 4 * K);
    const uint64_t idx_end = index_end(new_n, check);
    memset(out + idx_end, 0, new_first - idx_end);
    memcpy(out + new_first, in + first, kept_len);
    memset(out + new_first + kept_len, 0, base - (new_first + kept_len));
    HC_CK(hipStreamSynchronize(st));
    memcpy(out + 48 + 8 * K, lens.data(), 8 * C);
    if (check) memcpy(out + 48 + 8 * new_n + 4 * K, crcs.data(), 4 * C);
    return HC_OK;
}

uint64_t hc_seg_compress_batch_work_bound(const hc_seg_enc_item_t *items, uint32_t n_items, uint32_t flags,
                                          uint64_t seg_bytes)
{
    if ((flags & ~kSegFlags) || (seg_bytes & 15u) || (!items && n_items)) return 0;
    const int use_adapt = (flags & HC_FLAG_ADAPT) ? 1 : 0;
    EncTotals t;
    if (!enc_totals(items, n_items, use_adapt, seg_bytes ? seg_bytes : HC_SEG_DEFAULT_BYTES, t)) return 0;
    return enc_batch_ws(nullptr, n_items, t, use_adapt, checked(flags)).total;
}

int hc_seg_compress_batch_dev(const uint8_t *in, uint8_t *out, const hc_seg_enc_item_t *items, uint32_t n_items,
                              uint32_t flags, uint64_t seg_bytes, uint64_t *out_lens, int32_t *status, void *work,
                              uint64_t work_bytes, void *stream)
{
    if (n_items == 0) return HC_OK;
    if (!out || !items || !out_lens || !status || !work) return HC_ERR_ARG;
    if (flags & ~kSegFlags) return HC_ERR_ARG;
    if (seg_bytes & 15u) return HC_ERR_ARG;
    if (!aligned16(in) || !aligned16(out) || !aligned16(work)) return HC_ERR_ARG;
    for (uint32_t i = 0; i < n_items; ++i) {
        if (!in && items[i].in_len) return HC_ERR_ARG;
        if ((items[i].in_off | items[i].out_off) & 15u) return HC_ERR_ARG;
    }
    const int use_adapt = (flags & HC_FLAG_ADAPT) ? 1 : 0;
    if (!seg_bytes) seg_bytes = HC_SEG_DEFAULT_BYTES;
    const bool check = checked(flags);
    EncTotals t;
    if (!enc_totals(items, n_items, use_adapt, seg_bytes, t)) return HC_ERR_ARG;
    const EncBatchWs w = enc_batch_ws(work, n_items, t, use_adapt, check);
    if (work_bytes < w.total) return HC_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);

    uint64_t seg0 = 0, slot_off = 0;
    ItemFeed<EncItem, kEncChunk> feed(w.items, st);
    for (uint32_t i = 0; i < n_items; ++i) {
        const hc_seg_enc_item_t &h = items[i];
        const int hs = host_status(h.in_len, use_adapt, h.width);
        EncPlan p{};
        if (!hs) (void)enc_plan(h.in_len, seg_bytes, use_adapt, h.width, p);
        feed.push(enc_item(h, hs, p, use_adapt, seg0, slot_off));
        if (hs) continue;
        seg0 += p.c.n;
        slot_off += p.slot_bytes;
    }
    feed.flush();
    HC_CK(hipGetLastError());
    return encode_launch(Many<EncItem>{w.items, n_items, w.seg_item}, n_items, t.n, w.s, w.ctl, in, out, flags, seg_bytes,
                         out_lens, status, st);
}

uint64_t hc_seg_decompress_batch_work_bound(const hc_seg_dec_item_t *items, uint32_t n_items)
{
    if (!items && n_items) return 0;
    DecTotals t;
    if (!dec_totals(items, n_items, nullptr, t)) return 0;
    return dec_ws(nullptr, false, n_items, t).total;
}

int hc_seg_decompress_batch_dev(const uint8_t *in, uint8_t *out, const hc_seg_dec_item_t *items, uint32_t n_items,
                                uint64_t *out_lens, int32_t *status, uint64_t *bad_segments, void *work,
                                uint64_t work_bytes, void *stream)
{
    return decode_batch_dev(in, out, items, n_items, out_lens, status, bad_segments, work, work_bytes, stream, nullptr,
                            nullptr);
}

int hc_seg_compress_host_batch(const uint8_t *const *in, const uint64_t *in_lens, const uint64_t *widths,
                               uint32_t n_items, uint32_t flags, uint64_t seg_bytes, uint8_t *const *out,
                               const uint64_t *out_caps, uint64_t *out_lens, int32_t *status)
{
    if (n_items == 0) return HC_OK;
    if (!in || !in_lens || !out || !out_caps || !out_lens || !status) return HC_ERR_ARG;
    if ((flags & ~kSegFlags) || (seg_bytes & 15u)) return HC_ERR_ARG;
    const int use_adapt = (flags & HC_FLAG_ADAPT) ? 1 : 0;
    if (use_adapt && !widths) return HC_ERR_ARG;
    for (uint32_t i = 0; i < n_items; ++i)
        if ((!in[i] && in_lens[i]) || (!out[i] && out_caps[i])) return HC_ERR_ARG;
    auto width = [&](uint32_t i) { return widths ? widths[i] : 512; };
    std::vector<uint32_t> todo;
    for (uint32_t i = 0; i < n_items; ++i) {
        out_lens[i] = 0;
        status[i] = host_status(in_lens[i], use_adapt, width(i));
        if (!status[i]) todo.push_back(i);
    }
    if (todo.empty()) return HC_OK;
    if (!hc_device_ok()) {
        for (uint32_t i : todo) status[i] = HC_ERR_DEVICE;
        return HC_OK;
    }
    const uint64_t limit = pipe_bytes();
    hipStream_t st = nullptr;
    DevBuf din, dout, work, meta;
    for (size_t a = 0; a < todo.size();) {
        // the sub-batch [a, b): input bytes up to the limit, an item above it alone
        size_t b = a;
        uint64_t in_total = 0, out_total = 0;
        std::vector<hc_seg_enc_item_t> items;
        for (; b < todo.size(); ++b) {
            const uint32_t i = todo[b];
            if (b > a && in_total + in_lens[i] > limit) break;
            const uint64_t cap = hc_seg_compress_bound2(in_lens[i], seg_bytes, flags, width(i));
            if (cap == 0) return HC_ERR_ARG;  // (more segments than one call takes)
            items.push_back(hc_seg_enc_item_t{in_total, in_lens[i], width(i), out_total, cap});
            in_total += align16(in_lens[i]) + 16;
            out_total += align16(cap);
        }
        const uint32_t m = (uint32_t)items.size();
        const uint64_t wb = hc_seg_compress_batch_work_bound(items.data(), m, flags, seg_bytes);
        if (wb == 0) return HC_ERR_ARG;
        HC_CK(din.alloc(in_total));
        HC_CK(dout.alloc(out_total + 16));
        HC_CK(work.alloc(wb));
        HC_CK(meta.alloc(12ull * m));
        for (uint32_t j = 0; j < m; ++j)
            if (items[j].in_len)
                HC_CK(hipMemcpyAsync(din.as<uint8_t>() + items[j].in_off, in[todo[a + j]], items[j].in_len,
                                     hipMemcpyHostToDevice, st));
        uint64_t *d_lens = meta.as<uint64_t>();
        int32_t *d_st = reinterpret_cast<int32_t *>(d_lens + m);
        const int rc = hc_seg_compress_batch_dev(din.as<uint8_t>(), dout.as<uint8_t>(), items.data(), m, flags, seg_bytes,
                                                 d_lens, d_st, work.p, wb, st);
        if (rc) return rc;
        std::vector<uint64_t> h_lens(m);
        std::vector<int32_t> h_st(m);
        HC_CK(hipMemcpyAsync(h_lens.data(), d_lens, 8ull * m, hipMemcpyDeviceToHost, st));
        HC_CK(hipMemcpyAsync(h_st.data(), d_st, 4ull * m, hipMemcpyDeviceToHost, st));
        HC_CK(hipStreamSynchronize(st));
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t i = todo[a + j];
            status[i] = h_st[j];
            if (h_st[j]) continue;
            out_lens[i] = h_lens[j];
            if (h_lens[j] > out_caps[i]) status[i] = HC_ERR_CAPACITY;
            else HC_CK(hipMemcpy(out[i], dout.as<uint8_t>() + items[j].out_off, h_lens[j], hipMemcpyDeviceToHost));
        }
        a = b;
    }
    return HC_OK;
}

int hc_seg_decompress_host_batch(const uint8_t *const *in, const uint64_t *in_lens, const uint64_t *offsets,
                                 const uint64_t *lengths, uint32_t n_items, uint8_t *const *out,
                                 const uint64_t *out_caps, uint64_t *out_lens, int32_t *status, uint64_t *bad_segments)
{
    if (n_items == 0) return HC_OK;
    if (!in || !in_lens || !out || !out_caps || !out_lens || !status) return HC_ERR_ARG;
    if ((offsets == nullptr) != (lengths == nullptr)) return HC_ERR_ARG;
    for (uint32_t i = 0; i < n_items; ++i)
        if ((!in[i] && in_lens[i]) || (!out[i] && out_caps[i])) return HC_ERR_ARG;
    // what the host decides, in the single calls' order; the rest goes to the device
    struct Todo {
        uint32_t i;
        hc_seg_dec_item_t item;       // in_off / out_off: set per sub-batch
        uint64_t idx, s0, span, room;  // ranged: the upload is [0, idx) and [s0, s0 + span); whole: idx = in_len, span 0
    };
    std::vector<Todo> todo;
    const bool device = hc_device_ok() != 0;
    for (uint32_t i = 0; i < n_items; ++i) {
        out_lens[i] = 0;
        status[i] = HC_OK;
        if (bad_segments) bad_segments[i] = kNoSeg;
        Todo t;
        t.i = i;
        if (hc_seg_info(in[i], in_lens[i], &t.item.info) != HC_OK) {
            status[i] = HC_ERR_SEG_HEADER;
            continue;
        }
        const hc_seg_info_t &info = t.item.info;
        const bool whole = !lengths || (lengths[i] == HC_SEG_WHOLE && offsets[i] == 0);
        Cuts c;
        (void)info_ok(info, in_lens[i], c);
        if (whole) {
            if (c.n > kMaxSegs) status[i] = HC_ERR_ARG;
            else if (!device) status[i] = HC_ERR_DEVICE;
            if (status[i]) continue;
            t.item = hc_seg_dec_item_t{0, in_lens[i], info, 0, HC_SEG_WHOLE, 0, out_caps[i]};
            t.idx = in_lens[i];
            t.s0 = t.span = 0;
            t.room = out_caps[i] < info.raw_len ? out_caps[i] : info.raw_len;  // never more than raw_len is written
        } else {
            const uint64_t offset = offsets[i], length = lengths[i];
            const bool check = checked(info.flags);
            uint64_t s0 = 0, s1 = 0;
            if (!range_ok(info.raw_len, offset, length) || c.n > kMaxSegs) status[i] = HC_ERR_ARG;
            else if (hc_seg_index::index_scan(in[i], in_lens[i], c.n, check, range_cover(c, offset, length), &s0, &s1) != HC_OK)
                status[i] = HC_ERR_SEG_HEADER;
            else if (!device) status[i] = HC_ERR_DEVICE;
            else if (out_caps[i] < length) {
                status[i] = HC_ERR_CAPACITY;
                out_lens[i] = length;
            }
            if (status[i]) continue;
            t.item = hc_seg_dec_item_t{0, in_lens[i], info, offset, length, 0, length};
            t.idx = align16(index_end(c.n, check));
            t.s0 = s0;
            t.span = s1 - s0;
            t.room = length;
        }
        todo.push_back(t);
    }
    if (todo.empty()) return HC_OK;
    const uint64_t limit = pipe_bytes();
    hipStream_t st = nullptr;
    DevBuf din, dout, work, meta;
    for (size_t a = 0; a < todo.size();) {
        // the sub-batch [a, b): uploaded bytes up to the limit, an item above it alone
        size_t b = a;
        uint64_t in_total = 0, out_total = 0;
        std::vector<hc_seg_dec_item_t> items;
        std::vector<uint64_t> skips, spans;
        for (; b < todo.size(); ++b) {
            Todo &t = todo[b];
            const uint64_t up = t.idx + t.span;
            if (b > a && in_total + up > limit) break;
            t.item.in_off = in_total;
            t.item.out_off = out_total;
            items.push_back(t.item);
            const bool ranged = t.item.length != HC_SEG_WHOLE;
            skips.push_back(ranged ? t.s0 - t.idx : 0);
            spans.push_back(ranged ? t.span : t.item.in_len);
            in_total += align16(up) + 16;
            out_total += align16(t.room) + 16;
        }
        const uint32_t m = (uint32_t)items.size();
        DecTotals tot;
        if (!dec_totals(items.data(), m, spans.data(), tot)) return HC_ERR_ARG;
        const uint64_t wb = dec_ws(nullptr, false, m, tot).total;
        HC_CK(din.alloc(in_total));
        HC_CK(dout.alloc(out_total));
        HC_CK(work.alloc(wb));
        HC_CK(meta.alloc(20ull * m));
        for (uint32_t j = 0; j < m; ++j) {
            const Todo &t = todo[a + j];
            uint8_t *d = din.as<uint8_t>() + items[j].in_off;
            if (t.idx) HC_CK(hipMemcpyAsync(d, in[t.i], t.idx, hipMemcpyHostToDevice, st));
            if (t.span) HC_CK(hipMemcpyAsync(d + t.idx, in[t.i] + t.s0, t.span, hipMemcpyHostToDevice, st));
        }
        uint64_t *d_lens = meta.as<uint64_t>(), *d_bad = d_lens + m;
        int32_t *d_st = reinterpret_cast<int32_t *>(d_bad + m);
        const int rc = decode_batch_dev(din.as<uint8_t>(), dout.as<uint8_t>(), items.data(), m, d_lens, d_st, d_bad, work.p,
                                        wb, st, skips.data(), spans.data());
        if (rc) return rc;
        std::vector<uint64_t> h(2ull * m);
        std::vector<int32_t> h_st(m);
        HC_CK(hipMemcpyAsync(h.data(), d_lens, 16ull * m, hipMemcpyDeviceToHost, st));
        HC_CK(hipMemcpyAsync(h_st.data(), d_st, 4ull * m, hipMemcpyDeviceToHost, st));
        HC_CK(hipStreamSynchronize(st));
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t i = todo[a + j].i;
            status[i] = h_st[j];
            out_lens[i] = h[j];
            if (bad_segments) bad_segments[i] = h[m + j];
            if (h_st[j] == 0 && h[j])
                HC_CK(hipMemcpy(out[i], dout.as<uint8_t>() + items[j].out_off, h[j], hipMemcpyDeviceToHost));
        }
        a = b;
    }
    return HC_OK;
}

}  // extern "C"
