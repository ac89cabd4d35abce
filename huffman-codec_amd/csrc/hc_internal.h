// hc_internal.h — launchers shared between the kernel translation units and the C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <utility>
#include <vector>

#include "hcodec.h"

namespace hc {

// One batch of independent streams. All pointers are device pointers.
struct Batch {
    const uint8_t *in;
    const uint64_t *in_offs;
    const uint64_t *in_lens;
    uint32_t n;
    uint8_t *out;
    const uint64_t *out_offs;
    const uint64_t *out_caps;
    uint64_t *out_lens;
    int32_t *status;
    uint32_t flags;  // header flags byte for SRC_SYMBOLS encodes
    uint32_t min_tree;  // set by the launchers: the smallest FGK tree layout (hc_debug_set_min_tree)
    uint32_t dec_small;  // set by launch_decode: 0 by payload rate, 1 / 2 every / no narrow stream small (hc_debug_set_dec_small)
};

enum EncSrc { SRC_RAW = 0, SRC_RAW_DIFF = 1, SRC_SYMBOLS = 2 };
enum DecDst { DST_RAW = 0, DST_SYMBOLS = 1 };

// Largest FGK symbol count the packed ("narrow") tree layout handles: weights live in 22 bits.
constexpr uint64_t kNarrowMaxSymbols = (1ull << 22) - 2;
// Largest count of the wide layout (32-bit weights, sentinel 0xFFFFFFFF).
constexpr uint64_t kWideMaxSymbols = 0xFFFFFFFFull - 1;

// fused [diff] -> RLE -> FGK encode, or FGK over a ready symbol stream (adaptive path)
hipError_t launch_encode(const Batch &b, EncSrc src, hipStream_t st, hipStream_t aux = nullptr);
// fused FGK decode -> RLE revert -> [diff revert] (diff taken from each stream's flags byte),
// or FGK decode to the symbol stream
hipError_t launch_decode(const Batch &b, DecDst dst, hipStream_t st);

// adaptive block RLE (hc_adapt.hip), batched: device pointers as in Batch, asynchronous on st.
// Encode: matrix i = in[in_offs[i] ..) of in_lens[i] bytes and width widths[i]; flags
// HC_FLAG_DIFF or 0; the whole -a stream (FGK included) lands in out. Decode: adaptive streams
// -> matrices (diff revert from each stream's flags byte). `work` (16-byte aligned) must hold
// the bound below; streams that do not fit report HC_ERR_CAPACITY.
hipError_t adapt_encode_batch(const Batch &b, const uint64_t *widths, void *work, uint64_t work_bytes,
                              hipStream_t st);
hipError_t adapt_decode_batch(const Batch &b, void *work, uint64_t work_bytes, hipStream_t st);
uint64_t adapt_encode_work_bound(uint64_t total_in, uint32_t n);
uint64_t adapt_decode_work_bound(uint64_t total_in, uint64_t total_out, uint32_t n);

// CRC-32 of n byte ranges in[offs[i] .. +lens[i]) into crc[i] (hc_crc.hip), asynchronous on st.
// With a gate (the segmented decoder's; both pointers or none) range i is skipped, crc[i] left
// alone, unless status[i] == 0 and got_lens[i] == lens[i]. (The decoder's verdicts are per item
// and reach the segments' status: an item that may not be read has no segment with status 0.)
struct CrcGate {
    const int32_t *status;
    const uint64_t *got_lens;
};
hipError_t launch_crc32(const uint8_t *in, const uint64_t *offs, const uint64_t *lens, uint64_t n, uint32_t *crc,
                        const CrcGate &gate, hipStream_t st);

// lens[i] bytes from src + soffs[i] to dst + doffs[i] for n ranges (hc_pipe.hip's pack_kernel, the
// kernel behind hc_pack_batch), asynchronous on st: any byte alignment, no byte outside a source
// range read, none outside a destination range written; an empty range costs nothing
hipError_t launch_pack(const uint8_t *src, const uint64_t *soffs, const uint64_t *lens, uint32_t n, uint8_t *dst,
                       const uint64_t *doffs, hipStream_t st);

// frees the host-batch pipeline slots' cached buffers (hc_release_cached; slots in use by a
// running call are left alone)
void pipe_release();


// Device scratch of the single-buffer API. A call takes buffers from a per-device free list
// (hipMalloc only when none is large enough) and gives them back at its end, so a process that
// codes file after file (the CLI, C2) stops allocating after its first call. The list keeps at
// most kKeepBytes per device (larger leftovers are freed at once) and hc_release_cached() frees
// it. It caches memory only: no result depends on it, and concurrent calls never share a buffer.
constexpr uint64_t kKeepBytes = 1ull << 30;
struct FreeList {
    std::mutex mu;
    std::vector<std::pair<void *, uint64_t>> bufs[64];  // per device: (pointer, bytes)
    uint64_t kept[64] = {};
};
inline FreeList &free_list()
{
    static FreeList *const f = new FreeList;  // never destroyed: the HIP runtime may be gone at exit
    return *f;
}

struct DevBuf {
    void *p = nullptr;
    uint64_t cap = 0;
    int dev = -1;
    ~DevBuf() { give_back(); }
    void give_back()
    {
        if (!p) return;
        // the single-buffer API runs on the null stream; a call that returns early (an error
        // after an asynchronous launch) may still have kernels writing this buffer, so wait for
        // them before the next call can take it
        (void)hipStreamSynchronize(nullptr);
        FreeList &f = free_list();
        {
            std::lock_guard<std::mutex> lk(f.mu);
            if (dev >= 0 && dev < 64 && f.kept[dev] + cap <= kKeepBytes) {
                f.bufs[dev].emplace_back(p, cap);
                f.kept[dev] += cap;
                p = nullptr;
            }
        }
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    // at least n bytes: the smallest cached buffer that fits, else a new one (one retry after
    // freeing the cache when the device is short of memory)
    hipError_t alloc(uint64_t n)
    {
        give_back();
        n = n < 16 ? 16 : (n + 255) & ~255ull;
        if (hipGetDevice(&dev) != hipSuccess) dev = -1;
        if (dev >= 0 && dev < 64) {
            FreeList &f = free_list();
            std::lock_guard<std::mutex> lk(f.mu);
            auto &v = f.bufs[dev];
            size_t best = v.size();
            for (size_t k = 0; k < v.size(); ++k)
                if (v[k].second >= n && (best == v.size() || v[k].second < v[best].second)) best = k;
            if (best != v.size()) {
                p = v[best].first;
                cap = v[best].second;
                f.kept[dev] -= cap;
                v.erase(v.begin() + (long)best);
                return hipSuccess;
            }
        }
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            hc_release_cached();
            e = hipMalloc(&p, n);
        }
        cap = e == hipSuccess ? n : 0;
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    template <class T>
    T *as() const
    {
        return reinterpret_cast<T *>(p);
    }
};

}  // namespace hc
