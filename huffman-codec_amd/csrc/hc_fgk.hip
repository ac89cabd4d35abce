// hc_fgk.hip — FGK adaptive-Huffman encode / decode for gfx950, one stream per wavefront.
//
// Reference: huffman.cpp:23-217 (HuffTree), transform.cpp:363-406 (applyHuffman /
// revertHuffman), fused with transform.cpp:220-292 (diff model, MNP-5 RLE and their inverses)
// and the header / bit packing of headers.cpp:107-125 and main.cpp:39-128.
//
// Design:
//  * The FGK stream is serial, so parallelism comes from the batch: each 64-lane wavefront owns
//    one stream, four wavefronts per 256-thread workgroup, 8 workgroups (32 waves) per CU.
//  * The tree lives in LDS in the implicit slot form of SURVEY.md Appendix A.5: position p in
//    0..512 carries the reference's node number p (root = 512), siblings are (2k, 2k+1), code
//    bit = p & 1, weights non-decreasing in p. Per position one packed word
//    weight << 10 | parent ("narrow", <= 2^22-2 symbols) or a 32-bit weight plus a separate
//    parent array ("wide").
//  * Per update level ONE lane-parallel LDS read fetches the words of positions s..s+63; a
//    64-bit ballot of "weight == w[s]" is a prefix mask (weights sorted), so its trailing-ones
//    count gives the block leader of huffman.cpp:157-184 (highest number with equal weight)
//    in one step.
//  * All control state (positions, bit accumulators, run-length FSM) is wave-uniform and lives
//    in SGPRs. To keep the compiler from turning it into exec-masked VGPR code, the hot loops
//    contain NO lane-divergent control flow: a store "from lane 0 only" is an all-lane store
//    whose other lanes land in a per-wave scratch row, and global memory goes through buffer
//    descriptors whose hardware range check replaces per-lane bounds tests.
//  * Output bits gather in a 64-bit scalar accumulator, flush as big-endian dwords into a VGPR
//    stage and leave as one coalesced 256-byte buffer store per 64 words.
#include <type_traits>

#include "hc_internal.h"

// llvm.amdgcn.writelane has no clang builtin in this toolchain; binding the intrinsic by name
// lets the compiler schedule it and handle its lane-select hazard (unlike inline asm)
extern "C" __device__ int amdgcn_writelane(int x, int l, int v) __asm("llvm.amdgcn.writelane.i32");

namespace hc {

// Test and diagnostic hooks exist only in the debug build (libhcodec_dbg.so, -DHC_DEBUG_HOOKS;
// tests and bench.py's stage pass load it). The shipping libhcodec.so has no mutable globals:
// its windows, tree layouts and encoder modes are the constants below.
#if defined(HC_PROF) && !defined(HC_DEBUG_HOOKS)
#define HC_DEBUG_HOOKS 1
#endif
// the most codes one decoder batch step takes (a multiple of 4 up to 24; described with the
// decoder's other knobs below, HC_DEC_CHAIN -- how the step finds their starts -- among them)
#ifndef HC_DEC_PACK
#define HC_DEC_PACK 16
#endif
#ifdef HC_DEBUG_HOOKS
// when non-null, every FGK wave records (start, end, HW_ID | XCC_ID << 16) at [3 * stream]
// (scripts/residency.py measures how many waves share each SIMD); hc_debug_set_trace
__device__ uint64_t *g_trace = nullptr;
// the buffer window (below); hc_debug_set_window shrinks it so that tests cross many window
// edges on small streams
__device__ uint32_t g_window = 1u << 30;
// the lowest tree layout (0 narrow, 1 wide, 2 huge) any stream may use (hc_debug_set_min_tree:
// tests run the wide and huge kernels on small streams); the launchers pass it in Batch::min_tree
static uint32_t g_min_tree = 0;
// encoder mode for narrow / wide streams: 0 = per stream by enc_mode_kernel (default), 1 = path
// cache for all, 2 = tables for all (hc_debug_set_enc_tab; tests run both on every input)
static uint32_t g_enc_tab = 0;
// decoder launch for narrow streams: 0 = by payload rate (dec_small_stream), 1 = small-alphabet
// for all, 2 = regular for all (hc_debug_set_dec_small)
static uint32_t g_dec_small = 0;
// the most codes one decoder batch step takes (Dec::decode_batch; hc_debug_set_dec_pack: 1, 7 or
// HC_DEC_PACK)
__device__ uint32_t g_dec_pack = HC_DEC_PACK;
__device__ __forceinline__ uint32_t dec_pack_max(uint32_t k) { return min(k, (uint32_t)__builtin_amdgcn_readfirstlane(g_dec_pack)); }
// the most symbols one regular encoder batch step takes (code_all_batch; hc_debug_set_enc_pack: 1,
// 7 or HC_ENC_PACK)
__device__ uint32_t g_enc_pack = 16;
__device__ __forceinline__ uint32_t enc_pack_max(uint32_t k) { return min(k, (uint32_t)__builtin_amdgcn_readfirstlane(g_enc_pack)); }
__device__ __forceinline__ uint64_t *trace_buf() { return g_trace; }
__device__ __forceinline__ uint32_t window_bytes() { return __builtin_amdgcn_readfirstlane(g_window); }
static uint32_t min_tree() { return g_min_tree; }
static uint32_t enc_tab() { return g_enc_tab; }
static uint32_t dec_small() { return g_dec_small; }
#else
__device__ __forceinline__ uint32_t dec_pack_max(uint32_t k) { return k; }
__device__ __forceinline__ uint32_t enc_pack_max(uint32_t k) { return k; }
__device__ __forceinline__ uint64_t *trace_buf() { return nullptr; }
__device__ __forceinline__ uint32_t window_bytes() { return 1u << 30; }
static uint32_t min_tree() { return 0; }
static uint32_t enc_tab() { return 0; }
static uint32_t dec_small() { return 0; }
#endif
// Streams are addressed through buffer descriptors, whose offsets are 32-bit: each stream's input
// and output are reached through windows that slide forward by whole multiples of 256 bytes
// once the offset inside them passes window_bytes() (1 GiB), so streams of any length fit.

// the tree layout for a stream of at most `max_sym` FGK symbols
__device__ __forceinline__ uint32_t tree_kind(uint64_t max_sym, uint32_t lo)
{
    const uint32_t k = max_sym <= kNarrowMaxSymbols ? 0u : (max_sym <= kWideMaxSymbols ? 1u : 2u);
    return k > lo ? k : lo;
}

namespace {

__device__ __forceinline__ void trace_wave(uint32_t sid, uint64_t t0, uint32_t lane)
{
    uint64_t *const tr = trace_buf();
#ifdef HC_PROF
    return;  // the buffer holds the path profile (prof_store)
#endif
    if (tr == nullptr) return;
    const uint64_t t1 = __builtin_amdgcn_s_memtime();
    uint32_t hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    if (lane == 0) {
        tr[3 * sid] = t0;
        tr[3 * sid + 1] = t1;
        tr[3 * sid + 2] = (hw & 0xFFFFu) | ((xcc & 0xFu) << 16);
    }
}

// Diagnostic build (-DHC_PROF, scripts/path_prof.py): lane i of a per-wave accumulator sums the
// s_memtime cycles spent in region i of the kernel; at the end lanes 0..7 go to g_trace[8 *
// stream + i], lane 0 holding the wave's whole life. Absent from normal builds.
// -DHC_COUNT (with -DHC_PROF): the lanes count events instead (HC_CNT(i): lane i), e.g. the
// batch steps, retests and symbols coded alone of the batched paths
#if defined(HC_PROF) && !defined(HC_COUNT)
#define HC_PROF_BEGIN() const uint64_t hc_p0_ = __builtin_amdgcn_s_memtime()
#define HC_PROF_END(i) (pacc += lane == (i) ? __builtin_amdgcn_s_memtime() - hc_p0_ : 0)
#else
#define HC_PROF_BEGIN()
#define HC_PROF_END(i)
#endif
#ifdef HC_COUNT
#define HC_CNT(i) (pacc += lane == (i) ? 1 : 0)
#else
#define HC_CNT(i)
#endif
__device__ __forceinline__ void prof_store(uint32_t sid, uint64_t t0, uint64_t pacc, uint32_t lane)
{
#ifdef HC_PROF
    uint64_t *const tr = trace_buf();
    if (tr != nullptr && lane < 8) tr[8 * sid + lane] = lane == 0 ? __builtin_amdgcn_s_memtime() - t0 : pacc;
#endif
}

// The issue arbiter prefers higher priority, then older waves: left alone, the oldest of a
// SIMD's 8 waves run ahead and the last ones finish long after, on a half-empty SIMD. Waves
// that are behind (by the share of their stream done: below 1/2, 4/5, 19/20, the rest) take a
// higher priority instead. Within a band the arbiter goes by age, so the last bands are short.
// The band is recomputed only when progress reaches the next band edge (one scalar compare per
// chunk or block; the 64-bit products per call, with their operands spilled, cost ~10 instructions).
template <class I>  // uint32_t, or uint64_t for the huge layout's symbol counts
struct Prio {
    I next = 0;  // the progress at which the band changes next
    __device__ __forceinline__ void at(I done, I total)
    {
        if (done < next) return;
        const uint64_t d = (uint64_t)done * 20, t = total;
        // the band and the first progress past it: ceil(t * k / 20) for k = 10, 16, 19
        uint64_t k;
        if (d < 10 * t) {
            __builtin_amdgcn_s_setprio(3);
            k = 10;
        } else if (d < 16 * t) {
            __builtin_amdgcn_s_setprio(2);
            k = 16;
        } else if (d < 19 * t) {
            __builtin_amdgcn_s_setprio(1);
            k = 19;
        } else {
            __builtin_amdgcn_s_setprio(0);
            k = 0;
        }
        next = k ? (I)((t * k + 19) / 20) : (I)~(I)0;
    }
};

constexpr uint32_t kRoot = 512;
constexpr uint32_t kWords = 576;  // positions 0..512 + sentinels 513..575 (s + 63)
constexpr uint32_t kInner = 0x100;
constexpr uint32_t kNyt = 0x200;
#ifndef HC_WAVES
#define HC_WAVES 4
#endif
constexpr int kWaves = HC_WAVES;  // wavefronts (streams) per workgroup
constexpr uint32_t kMaxBufBytes = 0x7FFFFF00u;  // per-stream limit of the 32-bit buffer offsets
constexpr uint32_t kDrop = 0x7FFFFFF8u;         // buffer offset past every range: access dropped

constexpr uint32_t kMissPos = kWords - 2;  // sentinel: w[kMissPos + 1] <= w[kMissPos], so it fails
constexpr uint32_t kSlots = 16;     // encoder path cache: entries
constexpr uint32_t kSlotDepth = 12; // row capacity: levels per cache entry
#ifndef HC_INSERT_DEPTH
#define HC_INSERT_DEPTH 9
#endif
// deepest path a miss inserts: deeper (rarer) symbols would only evict paths that are used
// again (slot-form model, photo -c -m: misses 5.84 % at 12, 4.95 % at 9, 5.10 % at 8)
constexpr uint32_t kInsertDepth = HC_INSERT_DEPTH;
#ifndef HC_PROBE
#define HC_PROBE 7
#endif
// encoder: a miss chases this many levels, then looks the position reached up in the path cache
constexpr uint32_t kProbe = HC_PROBE;
// HC_CHASE_GROUP n > 0: the path-cache encoder's miss chase climbs without a per-level root test:
// levels 0..kProbe as one group, then n levels between two tests (Fgk::chase_grouped). 0: the
// per-level climb (Fgk::chase), which the table-mode encoder and the decoder keep either way.
#ifndef HC_CHASE_GROUP
#define HC_CHASE_GROUP 4
#endif
constexpr uint32_t kRow = 16;       // u16 per cache entry
// 1: path-cache streams (narrow and wide layouts) code cached symbols up to HC_ENC_PACK (1..16)
// at a time, packed by path depth (code_all_batch). A symbol's depth and its code record both
// come from one read of its cache row's record word.
// Measured and dropped: uncached symbols joining the batch with lane-parallel chased paths,
// inserted into the cache after the commit (570 ms)
#ifndef HC_ENC_BATCH
#define HC_ENC_BATCH 1
#endif
#ifndef HC_ENC_PACK
#define HC_ENC_PACK 16
#endif
static_assert(HC_ENC_PACK >= 1 && HC_ENC_PACK <= 16, "a step's symbols are the lanes of one DPP row");
// The symbol that ends a regular batch step is finished from what the step's lanes hold (model:
// tests/fgk_handoff_model.py). HC_ENC_HANDOFF_MISS: an uncached symbol's byte and where[] word
// come from the step's lanes instead of three more dependent LDS round trips.
// HC_ENC_HANDOFF_LEVEL: a cached symbol with a reported level keeps the increments of its levels
// below the report and walks from the reported level (no second test and store of every level).
// Measured (C5 encode, alternating pairs): the miss hand-off alone 340.3 -> 330.2 ms, the level
// hand-off alone 341.0 -> 338.3, both 332.8 / 332.8 / 334.0 against the miss hand-off alone 330.4 /
// 332.1 / 331.5: four in ten reports on a photo stream are false, and each now costs a walk (exact
// test, store, chase back, update_from) where update_fast ended it. Off.
// scripts/build_rel.sh builds any combination (-DHC_ENC_HANDOFF_...=0 / 1).
#ifndef HC_ENC_HANDOFF_MISS
#define HC_ENC_HANDOFF_MISS 1
#endif
#ifndef HC_ENC_HANDOFF_LEVEL
#define HC_ENC_HANDOFF_LEVEL 0
#endif
// HC_ENC_MISS_RUN 1 (the path-cache kernel): after the symbol that ended a regular step is coded
// alone, the symbols right behind it that the step read as uncached are coded alone too, up to
// HC_ENC_MISS_RUN_MAX (1..15) of them, instead of starting a step that takes nothing (model:
// tests/fgk_missrun_model.py; photo -c -m: 13 % of the steps took nothing, 5 % with the rule).
// Measured (C5 encode, alternating pairs against the parent's 306.3 / 306.2 / 306.5 ms): as an
// inner loop round the one call site of the miss path 316.1 / 316.2 / 316.1, as a loop that
// takes a step or a run symbol per pass 318.8 / 318.9 / 318.7: the steps saved are fewer
// instructions in the model and more time on the GPU. Off. DESIGN.md section 7.
#ifndef HC_ENC_MISS_RUN
#define HC_ENC_MISS_RUN 0
#endif
#ifndef HC_ENC_MISS_RUN_MAX
#define HC_ENC_MISS_RUN_MAX 15
#endif
static_assert(HC_ENC_MISS_RUN_MAX >= 1 && HC_ENC_MISS_RUN_MAX <= 15, "a run lies inside one step's 16 read lanes");
// decoder (narrow and wide layouts): HC_DEC_BATCH != 0: up to HC_DEC_PACK (4, 8, ... 24) codes
// per step, packed by bit offset (one lane per code bit), from one read of the level tables at
// every bit offset and one tentative commit (Dec::decode_batch; HC_DEC_BATCH 0: the one-symbol
// loop only). Measured on the earlier layout of nine lanes per code, C5 decode: one-symbol loop
// 490 ms, 6 per step 443, 7 per step 430; eight per step in 8-lane groups (the root's increments
// apart) 437; a first code of >= 8 bits sent to the one-symbol step before the chain
// (HC_DEC_EXIT8): noise decode 237 -> 198 ms, C5 +0.5 %
#ifndef HC_DEC_BATCH
#define HC_DEC_BATCH 7
#endif
// HC_DEC_CHAIN (1, 2 or 4): the stride of the packed step's serial chain of code starts. 1: one
// link (lane read, add, lane write) per code, up to HC_DEC_PACK of them. 2 / 4: the depth map is
// composed with itself once / twice, lane-parallel (dep2[o] = dep[o] + dep[o + dep[o]], one
// ds_bpermute each), the chain visits every second / fourth start, and the starts in between are
// filled in afterwards, lane-parallel again (one DPP move, one ds_bpermute, an add and a min per
// level). Built after the HC_DEC_EXIT8 exit, so a step that leaves there pays nothing. The step
// takes the same codes whatever the stride (model: tests/fgk_chain_model.py; Dec::decode_small
// keeps its own chain). On 64 true window bits nearly every photo step runs all 16 links (the chain
// leaves early only once 12 codes fill 63 bits). Measured, C5 decode: 1: 340.3-341.5 ms, 2:
// 328.1-328.4, 4: 326.7-327.3; the latency-bound configs prefer 2 (one 4096 x 4096 stream -c -a -m:
// 1202 / 1169 / 1177 ms; one 512 x 512 stream: 27.3 / 26.5 / 26.8), the flat alphabets leave at the
// gate before any of it: 2 ships.
#ifndef HC_DEC_CHAIN
#define HC_DEC_CHAIN 2
#endif
static_assert(HC_DEC_CHAIN == 1 || HC_DEC_CHAIN == 2 || HC_DEC_CHAIN == 4, "chain stride");
// HC_DEC_TOPUP 1: a batch step works on 64 true window bits -- the top 64 - nwin bits of the next
// unread word are peeked into the window before the step (BitSource::peek), so a step takes codes
// up to bit 62 whatever the window held; 0: the window's own 32..64 bits bound the step (tests/
// fgk_topup_model.py; photo -c -m: 8-15 % fewer steps, C5 decode -3 %; with the full window 20 and
// 24 codes a step take fewer steps still but send more symbols to the one-symbol step, and measured
// slower than 16: DESIGN.md section 7)
// The parent's decoder (round 9) is -DHC_DEC_TOPUP=0 -DHC_DEC_NEXTW=0: HC_DEC_NEXTW below also
// changes every refill of the one-symbol loop, so the A/B of the shipped build against that one
// measures both together.
// HC_DEC_TOPUP_SMALL 1: the small-alphabet launch (streams under 2.5 payload bits per symbol: both
// Dec::decode_small and its copy of decode_batch) takes the full window too. Off: its 15 or 16
// symbols of ~1.7 bits (grad -c -m) never reach the end of the window's own bits, so the peek and
// the refill test only cost (grad decode 1.12 -> 1.15 ms with it on)
#ifndef HC_DEC_TOPUP
#define HC_DEC_TOPUP 1
#endif
// HC_DESC_GROUP 1: the descent of a code longer than the level tables reach (Dec::finish_symbol)
// takes its first levels in groups with one inner test a group; HC_DESC_SCHED lists the levels
// (counted from where the descent starts) after which the test happens, the last one being the
// levels run this way before the per-level loop takes over. 0: the per-level loop alone.
// (Measured: a test after every level, {1, 2, ..., 8}, fewer instructions in the model's count, is
// no faster and its times spread wider: DESIGN.md section 7.)
#ifndef HC_DESC_GROUP
#define HC_DESC_GROUP 1
#endif
#ifndef HC_DESC_SCHED
#define HC_DESC_SCHED {1, 4, 5, 6, 8}
#endif
constexpr uint32_t kDescSched[] = HC_DESC_SCHED;
constexpr uint32_t kDescLevels = kDescSched[sizeof(kDescSched) / sizeof(kDescSched[0]) - 1];
static_assert(kDescLevels <= 24, "the grouped levels take their bits from the window's high word");
#ifndef HC_DEC_TOPUP_SMALL
#define HC_DEC_TOPUP_SMALL 0
#endif
static_assert(HC_DEC_TOPUP || !HC_DEC_TOPUP_SMALL, "the small-alphabet step's top-up needs HC_DEC_TOPUP");
// HC_DEC_NEXTW 1: the next unread word is kept in a scalar register (BitSource::nw, read in
// next_word() where refill() read its lane before): a peek is a shift and an OR, and a refill no
// longer waits for a lane read. Measured against 0 (the word read from its lane at the peek and at
// the refill): C3 decode 154.7 -> 152.1 ms, noise 161.9 -> 160.6, grad 1.160 -> 1.147, C5 356.0 ->
// 356.8 (the flat alphabets wait on dependencies, C5 on issue slots)
#ifndef HC_DEC_NEXTW
#define HC_DEC_NEXTW 1
#endif
#ifndef HC_DEC_EXIT8
#define HC_DEC_EXIT8 1
#endif
// (measured and dropped with the nine-lane layout, HC_BATCH_RETRY: a batch whose first failing
// symbol's failure may be false -- its test counts no earlier batch symbol through the next
// position -- tested again from that symbol with the earlier ones committed; model:
// fgk_batch_model.retry_len. grad / C5 / noise: decode -5.5 % / +-0 / +2 % at best: the retest's
// ~35-55 instructions cost what the restarts they save do)
// the encoder vote's spread sample: eight segments' loads in flight at once (enc_mode_kernel)
#ifndef HC_VOTE_BATCH
#define HC_VOTE_BATCH 1
#endif
#ifndef HC_BATCH_YIELD
#define HC_BATCH_YIELD 5
#endif
// Dec::run: a stream whose batches are off tries them again every HC_BATCH_PROBE-th block (a power
// of two); HC_DEC_EXIT8: a first code of HC_DEC_EXIT_BITS bits or more leaves the step to the
// one-symbol loop. A packed step costs two LDS round trips more than the nine-lane one did, which
// the flat alphabets' few waves per SIMD wait out: with 8 blocks and 8 bits (the nine-lane
// layout's values) noise decode was 167.0 ms and C3 156.5 against 161.8 and 154.6 before the
// packed step (159.6 / 152.0 with no batches at all); 32 blocks alone 164.2 / 153.7, 7 bits alone
// 164.4 / 156.6, both 161.5 / 154.4; C5 decode 367.4 against 365.7 ms
#ifndef HC_BATCH_PROBE
#define HC_BATCH_PROBE 32
#endif
#ifndef HC_DEC_EXIT_BITS
#define HC_DEC_EXIT_BITS 7
#endif
static_assert((HC_BATCH_PROBE & (HC_BATCH_PROBE - 1)) == 0 && HC_DEC_EXIT_BITS >= 2 && HC_DEC_EXIT_BITS <= 8, "gate knobs");
constexpr uint32_t kBatchYield = HC_BATCH_YIELD;  // Dec::run: twice the symbols per batch worth it
// walk(): after a swap at a position lighter than this, the parent's level is walked at once
// instead of chasing back to the known path. Measured (C5 encode / decode, noise encode /
// decode, ms): never 410 / 397, 206 / 184; always 392 / 381, 218 / 197; below 64: 393 / 381,
// 211 / 190; below 512: 394 / 382, 214 / 193
#ifndef HC_WALK_LIGHT
#define HC_WALK_LIGHT 64
#endif
constexpr uint32_t kWalkLight = HC_WALK_LIGHT;
// HC_WALK_LEAN 1: walk()'s climb back to the known path carries only the level's own work: the
// lane to write is a running 64-bit mask (no counter beside it, the level count read off it once
// after the loop), the select writes its register in place, the bound is the mask running out (64
// levels), the loop branches on the compare and the meeting lanes are formed once after it
// (climb_to: 7 VALU + SALU a level where the compiled loop had 12). A climb of no level (the parent
// is on the known path) keeps that path and updates it from the meeting lane up, without the shift
// through ds_bpermute. In the path-cache encoders and the decoders (Fgk::kLean). 0: the loop as
// before everywhere (the parent commit's assembly). Measured (C5, alternating pairs):
// encode 306.30 / 306.17 / 306.45 -> 302.51 / 301.95 / 302.29 ms, decode 348.46 / 349.04 / 349.16
// -> 340.81 / 343.49 / 343.66. Model: tests/fgk_walk_model.py.
#ifndef HC_WALK_LEAN
#define HC_WALK_LEAN 1
#endif
constexpr uint32_t kSymWords = 88;  // encoder: MNP-5 symbols of one 256-byte chunk, <= 342
                                    // (a byte emits 2 only at a run start that follows a run of
                                    // >= 3, so such bytes are >= 3 apart)
#ifndef HC_REFRESH
#define HC_REFRESH 16
#endif
constexpr uint32_t kRefresh = HC_REFRESH;   // decoder: rebuild the level tables after this many lookups
                                    // they left short of depth 8
constexpr uint32_t kMarkShift = 10; // decoder: body bits 10..14 = table generation (per position)
constexpr uint32_t kNotLeaf = 0x8000; // decoder: body bit 15 = inner or NYT (moves with the content)
constexpr uint32_t kContent = 0x83FF; // decoder: the body bits that move with the content

// Tree layouts by the stream's FGK symbol count (the root's weight): kW = 0 "narrow" (<= 2^22 - 2
// symbols: weight << 10 | parent in one u32), 1 "wide" (< 2^32 - 1: u32 weight, u16 parent), 2
// "huge" (any count: u64 weight, as the reference's uint64_t freq, huffman.hpp:26).
template <int kW>
using WeightT = std::conditional_t<kW == 2, uint64_t, uint32_t>;

// One wavefront's LDS; <= 5 KB so that 8 four-wave workgroups fit a CU (narrow). Encoder and
// decoder each add their cache (tests/fgk_cache_model.py is the executable model of both,
// checked against the plain slot form). kTab: the encoder's table mode (no path cache; the
// decoder's level tables plus pcode[], ~6.5 KB, 6 waves per SIMD).
template <int kW, bool kDec, bool kTab = false, bool kSmall = false>
struct alignas(16) Tree {
    WeightT<kW> wt[kWords];           // narrow: weight << 10 | parent; wide / huge: weight
    uint32_t scratch[kW == 2 ? 128 : 64];  // landing words of lanes that must not write
    // symbol | kInner + child pair | kNyt; decoder: bits 10..15 = generation of the level
    // tables that walked through this position
    uint16_t body[516];
    uint16_t where[kDec ? 2 : 256];   // encoder: symbol -> position | (entry + 1) << 10; 0 = unseen
    uint16_t up[kW ? 516 : 2];        // wide / huge: parent position
    // encoder path cache, entry e = row e: positions of levels 0..11 (kRoot above the path),
    // [12] code record 1 << depth | code bits, [13] depth | valid << 5 | symbol << 8, [14..15]
    // unused. One lane-based
    // address reads a lane's position and (lane 0) the row's metadata.
    // row "entry -1" (where[] entry 0: not cached): level 0 at sentinel position kMissPos, whose
    // leader test always fails at lane 0, so a miss leaves the hot loop like a failed update
    alignas(16) uint16_t pc_miss[(kDec || kTab) ? 2 : kRow];
    uint16_t pc[(kDec || kTab) ? 2 : kSlots * kRow];
    alignas(8) uint32_t syms[kDec ? 64 : kSymWords];  // MNP-5 symbols: encoder one chunk, decoder one block
    // decoder level tables: level j (1..8) at 2^j - 2 + prefix: position | depth << 10 where
    // the walk from the root along the prefix's bits stops; lvl_root (indices -2, -1: "level
    // 0") holds the root, which the lanes above a path's depth read
    uint16_t lvl_root[2];
    uint16_t lvl[(kDec || kTab) ? 512 : 2];
    // table mode: position -> its code as the level tables reached it: the prefix left-aligned
    // to 8 bits | (depth - 1) << 8 (checked against the tables at every use: stale entries fail)
    uint16_t pcode[kTab ? 516 : 2];
    // the small-alphabet kernels (kSmall, narrow layout): the batch steps' membership marks (code_all_batch):
    // bit 16 (a & 1) + j of word (a - 480) >> 1 says batch symbol j's path holds position a (480..513)
    uint32_t smark[kSmall ? 17 : 1];
};

typedef __attribute__((address_space(3))) uint8_t lds_u8;  // a byte in LDS (32-bit address)
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) uint16_t lds_u16;
// the 32-bit LDS address of a word of the wave's tree
template <class P>
__device__ __forceinline__ uint32_t lds_off(P *p)
{
    return (uint32_t)(size_t)(__attribute__((address_space(3))) P *)p;
}
__device__ __forceinline__ uint32_t lds_off16(uint16_t *p) { return (uint32_t)(size_t)(lds_u16 *)p; }
__device__ __forceinline__ uint32_t uni(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint64_t uni64(uint64_t x)
{
    return (uint64_t)uni((uint32_t)x) | ((uint64_t)uni((uint32_t)(x >> 32)) << 32);
}
// the value unchanged, opaque to the optimizer: a u16 LDS load kept as a 32-bit value (left
// alone, masks of it are narrowed to 16-bit ops that cost an extra re-extension each)
__device__ __forceinline__ uint32_t opaque(uint32_t x)
{
    asm("" : "+v"(x));
    return x;
}
__device__ __forceinline__ uint32_t lane_id()
{
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}
__device__ __forceinline__ uint32_t lane_read(uint32_t v, uint32_t l)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l);
}
// lane l of v := x (x, l wave-uniform): the llvm.amdgcn.writelane intrinsic (declared above)
__device__ __forceinline__ uint32_t writelane(uint32_t v, uint32_t x, uint32_t l)
{
    return (uint32_t)amdgcn_writelane((int)x, (int)l, (int)v);
}
__device__ __forceinline__ uint64_t ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// lowest set bit of a wave mask, 0xFFFFFFFF for 0 (s_ff1_i32_b64 without the zero test)
__device__ __forceinline__ uint32_t ff1(uint64_t m)
{
    uint32_t r;
    asm("s_ff1_i32_b64 %0, %1" : "=s"(r) : "s"(m));
    return r;
}
// the lanes below k: (1 << (k & 63)) - 1 (k = 0xFFFFFFFF: lanes 0..62; in every path vector lane
// 63 holds the root, whose duplicates in the lanes below it store the same word)
__device__ __forceinline__ uint64_t below_mask(uint32_t k)
{
    uint64_t r;
    asm("s_bfm_b64 %0, %1, 0" : "=s"(r) : "s"(k));
    return r;
}
// per lane: bit lane of m ? t : f (one v_cndmask on a scalar mask)
__device__ __forceinline__ uint32_t sel(uint64_t m, uint32_t t, uint32_t f)
{
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(t), "s"(m));
    return r;
}
// ballot(a == b) as an instruction of its own
[[maybe_unused]] __device__ __forceinline__ uint64_t lanes_eq(uint32_t a, uint32_t b)
{
    uint64_t r;
    asm("v_cmp_eq_u32_e64 %0, %1, %2" : "=s"(r) : "v"(a), "v"(b));
    return r;
}
// walk()'s climb from position c (wave-uniform, in a VGPR) until it equals a lane of pv: the j-th
// position passed goes to lane j of td, c := its parent. kWide 0: the parent is the low ten bits
// of the 32-bit word at base + 4 c; 1: the 16-bit word at base + 2 c. lm starts as 1 and ends as
// 1 << (positions passed); 0: 64 were passed and no lane of pv met (the caller reports the bug).
// Written out because the compiler, given the same loop in C++ with the select in place ("+v"),
// copies td and the mask into fresh registers and back every level (12 instructions a level, as
// with the counter and the shift it had before); here a level is 7 (6 wide): address, [mask of
// the parent field,] compare, branch, select into the mask's lane, mask shift, branch on its
// carry-out. The read is waited for inside (lgkmcnt(0)); nothing else is in flight that matters.
template <bool kWide>
[[maybe_unused]] __device__ __forceinline__ void climb_to(uint32_t &c, uint32_t &td, uint64_t &lm, uint32_t pv, uint32_t base)
{
    uint32_t a;
    if constexpr (kWide) {
        asm volatile("s_branch 3f\n"
                     "1:\n\t"
                     "v_lshl_add_u32 %3, %0, 1, %5\n\t"
                     "ds_read_u16 %0, %3\n\t"
                     "s_waitcnt lgkmcnt(0)\n"
                     "3:\n\t"
                     "v_cmp_eq_u32_e32 vcc, %4, %0\n\t"
                     "s_cbranch_vccnz 2f\n\t"
                     "v_cndmask_b32_e64 %1, %1, %0, %2\n\t"
                     "s_lshl_b64 %2, %2, 1\n\t"
                     "s_cbranch_scc1 1b\n"
                     "2:"
                     : "+v"(c), "+v"(td), "+s"(lm), "=&v"(a)
                     : "v"(pv), "s"(base)
                     : "vcc", "scc", "memory");
    } else {
        asm volatile("s_branch 3f\n"
                     "1:\n\t"
                     "v_lshl_add_u32 %3, %0, 2, %5\n\t"
                     "ds_read_b32 %0, %3\n\t"
                     "s_waitcnt lgkmcnt(0)\n\t"
                     "v_and_b32_e32 %0, 0x3ff, %0\n"
                     "3:\n\t"
                     "v_cmp_eq_u32_e32 vcc, %4, %0\n\t"
                     "s_cbranch_vccnz 2f\n\t"
                     "v_cndmask_b32_e64 %1, %1, %0, %2\n\t"
                     "s_lshl_b64 %2, %2, 1\n\t"
                     "s_cbranch_scc1 1b\n"
                     "2:"
                     : "+v"(c), "+v"(td), "+s"(lm), "=&v"(a)
                     : "v"(pv), "s"(base)
                     : "vcc", "scc", "memory");
    }
}
// A wave-uniform value held in a VGPR: hiding its uniformity from the compiler moves the
// arithmetic on it from the (saturated) scalar unit to the vector ALUs. Branches on such
// values go through ballot(), which is uniform again.
__device__ __forceinline__ uint32_t vreg(uint32_t x)
{
    asm volatile("" : "+v"(x));
    return x;
}

// lane l gets x of lane l - 1, lane 0 gets fill (a DPP wave shift: no LDS round trip)
__device__ __forceinline__ uint32_t wave_shr1(uint32_t x, uint32_t fill)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)x, 0x138, 0xF, 0xF, false);
}

// Range-checked view of one stream's bytes: base and size, turned into a buffer descriptor at
// each access with readfirstlane on every part. The descriptor must be wave-uniform; kept as a
// value across the loops, the compiler sometimes held it in VGPRs (a u64 min() lowered through
// f64, or SGPR pressure) and wrapped every load through it in a waterfall loop over lanes (~12
// instructions and an exec save per chunk). The readfirstlanes fold away when the parts sit in
// SGPRs, and cost 3 VALU instead of a waterfall when they do not.
struct rsrc_t {
    uint64_t base;
    uint32_t bytes;
};
__device__ __forceinline__ rsrc_t make_rsrc(const uint8_t *p, uint32_t bytes)
{
    return rsrc_t{(uint64_t)(size_t)p, bytes};
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t hw_rsrc(rsrc_t r)
{
    // (readfirstlane returns int: each half goes through uint32_t before widening, or a low
    // word with bit 31 set would sign-extend into the high word)
    const uint64_t ua = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)r.base) |
                        ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(r.base >> 32)) << 32);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<uint8_t *>((size_t)ua), (short)0,
                                             (int)__builtin_amdgcn_readfirstlane(r.bytes), 0x00020000);
}
__device__ __forceinline__ uint32_t buf_load(rsrc_t r, uint32_t off)
{
    return __builtin_amdgcn_raw_buffer_load_b32(hw_rsrc(r), (int)off, 0, 0);
}
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 buf_load4(rsrc_t r, uint32_t off)
{
    return __builtin_amdgcn_raw_buffer_load_b128(hw_rsrc(r), (int)off, 0, 0);
}
__device__ __forceinline__ void buf_store(rsrc_t r, uint32_t off, uint32_t v)
{
    __builtin_amdgcn_raw_buffer_store_b32(v, hw_rsrc(r), (int)off, 0, 0);
}
__device__ __forceinline__ void buf_store8(rsrc_t r, uint32_t off, uint32_t v)
{
    __builtin_amdgcn_raw_buffer_store_b8((unsigned char)v, hw_rsrc(r), (int)off, 0, 0);
}
__device__ __forceinline__ void buf_store4(rsrc_t r, uint32_t off, u32x4 v)
{
    __builtin_amdgcn_raw_buffer_store_b128(v, hw_rsrc(r), (int)off, 0, 0);
}

// inclusive prefix sum over the wave (row shifts, then row broadcasts 15 and 31)
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t x)
{
    x += __builtin_amdgcn_update_dpp(0u, x, 0x111, 0xF, 0xF, true);  // row_shr:1
    x += __builtin_amdgcn_update_dpp(0u, x, 0x112, 0xF, 0xF, true);  // row_shr:2
    x += __builtin_amdgcn_update_dpp(0u, x, 0x114, 0xF, 0xF, true);  // row_shr:4
    x += __builtin_amdgcn_update_dpp(0u, x, 0x118, 0xF, 0xF, true);  // row_shr:8
    x += __builtin_amdgcn_update_dpp(0u, x, 0x142, 0xA, 0xF, false); // row_bcast:15
    x += __builtin_amdgcn_update_dpp(0u, x, 0x143, 0xC, 0xF, false); // row_bcast:31
    return x;
}

// ------------------------------------------------------------------------------ the tree --

template <int kW, bool kDec, bool kTab = false, bool kSmall = false>
struct Fgk {
    static constexpr bool kTabs = kDec || kTab;  // keeps the level tables
    static constexpr bool kWide = kW != 0;  // weights apart from parents (wide / huge)
    static constexpr bool kHuge = kW == 2;  // 64-bit weights
    using Wt = WeightT<kW>;
    static constexpr Wt kInc = kWide ? 1u : 1024u;
    // walk(): the lean climb (HC_WALK_LEAN) in the path-cache encoder and the decoder; the table-mode
    // and the small-alphabet encoder keep the compiled loop (their assembly is the parent's): noise
    // -c -m encode 203.8 / 204.9 -> 207.0 / 206.8 ms and grad 1.267 / 1.268 -> 1.272 / 1.276 with it
    static constexpr bool kLean = HC_WALK_LEAN && (kDec || (!kTab && !kSmall));

    Tree<kW, kDec, kTab, kSmall> &T;
    uint32_t lane;
    uint32_t nyt;    // position of the NYT leaf: 512 - 2 * (symbols seen)
    uint32_t bad;    // a structural invariant broke (a bug, never valid input): stop, report
    uint32_t pc_next;  // encoder: FIFO hand of the path cache
    uint32_t pc_free;  // encoder: entries dropped by swaps (or never used), taken first
    uint32_t pc_lb;    // encoder: a weight no cached path's position is below (pc_bound)
    uint32_t pc_lb_ok; // encoder: no insert since pc_bound
    uint32_t gen;      // decoder: generation of the level tables
    uint32_t stale;    // decoder: lookups the level tables left short (kRefresh: from := 0)
    uint32_t from;     // decoder: rebuild levels from..8 of the tables (9: none, 0: all, in a new
                       // generation); a swap moved a position they reach at level from - 1
    const uint16_t *pc_lane;  // encoder: &pc[(lane & 15) - kRow]: where[] entry e's row (0: pc_miss)
    uint64_t pacc = 0;        // HC_PROF regions inside the tree code

    __device__ __forceinline__ Fgk(Tree<kW, kDec, kTab, kSmall> &t, uint32_t l)
        : T(t), lane(l), nyt(kRoot), bad(0), pc_next(0), pc_free(0xFFFFu), pc_lb(0), pc_lb_ok(0), gen(0), stale(0), from(0),
          pc_lane(&t.pc[0] + (l & 15u) - (kTabs ? 0 : kRow))
    {
        // huffman.cpp:23-31: a lone NYT root
        // narrow: sentinels above every weight word; the encoder's last word (above kMissPos)
        // is 0, the decoder's all ones - 1 (see update_fast) but its last 0 too: the pair
        // (kMissPos, kMissPos + 1) fails every leader test
        for (uint32_t i = lane; i < kWords; i += 64)
            T.wt[i] = i <= kRoot ? (Wt)0 : (kWide ? ~(Wt)0 : (Wt)(i == kWords - 1 && (kDec || !kTabs) ? 0u : (kTabs ? 0xFFFFFFFEu : 0xFFFFFFFFu)));
        if (lane < 2) T.lvl_root[lane] = kRoot;
        for (uint32_t i = lane; i < 516; i += 64) {
            T.body[i] = i == kRoot ? (kDec ? kNyt | kNotLeaf : kNyt) : 0;
            if (kWide) T.up[i] = 0;
        }
        if (kSmall && lane < sizeof(T.smark) / 4) T.smark[lane] = 0;
        if (!kDec) {
            for (uint32_t i = lane; i < 256; i += 64) T.where[i] = 0;
            if constexpr (kTab) {
                for (uint32_t i = lane; i < 516; i += 64) T.pcode[i] = 0;
            } else {
                for (uint32_t i = lane; i < kSlots * kRow; i += 64) T.pc[i] = (i % kRow) < kSlotDepth ? 0xFFFF : 0;
                // (word 12, the code record: 1 = depth 0, no lane of a packed batch step)
                if (lane < kRow) T.pc_miss[lane] = lane == 0 ? kMissPos : (lane == kSlotDepth ? 1u : kRoot);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }

    // own scratch slot of this lane (16- and 32-bit views)
    __device__ __forceinline__ uint32_t *scr32() const { return &T.scratch[lane]; }
    __device__ __forceinline__ uint16_t *scr16() const
    {
        return reinterpret_cast<uint16_t *>(&T.scratch[lane]);
    }
    __device__ __forceinline__ uint8_t *scr8() const { return reinterpret_cast<uint8_t *>(&T.scratch[lane]); }
    // ... and a weight-sized one
    __device__ __forceinline__ Wt *scrw() const { return reinterpret_cast<Wt *>(&T.scratch[kHuge ? 2 * lane : lane]); }
    // a weight read on the lanes, made wave-uniform / taken from lane l
    static __device__ __forceinline__ Wt uniw(Wt x)
    {
        if constexpr (kHuge) return uni64(x);
        else return uni(x);
    }
    static __device__ __forceinline__ Wt readw(Wt x, uint32_t l)
    {
        if constexpr (kHuge) return (uint64_t)lane_read((uint32_t)x, l) | ((uint64_t)lane_read((uint32_t)(x >> 32), l) << 32);
        else return lane_read(x, l);
    }

    // ---- encoder path cache: root paths of recently coded symbols (tests/fgk_cache_model.py).
    // A path changes only when a swap moves a position on it; splits touch no symbol's path.

    // hit: pr = entry e's row as read lane-parallel at pc_lane[e * kRow] (lane k < 12: position
    // of level k, kRoot padding from the depth on); the path to pv, returns the row's code
    // record (word 12, see RecSink) in an SGPR
    __device__ __forceinline__ uint32_t pc_use(uint32_t e, uint32_t pr, uint32_t &pv)
    {
        pv = lane < kSlotDepth ? pr : kRoot;
        return lane_read(pr, kSlotDepth);
    }

    // forget entry e (its symbol's where[] keeps only the position: level 0 of the path)
    __device__ __forceinline__ void pc_forget(uint32_t e, uint16_t *other, uint32_t oval)
    {
        const uint32_t m = uni(T.pc[e * kRow + kSlotDepth + 1]);
        const uint32_t opos = uni(T.pc[e * kRow]);
        uint16_t *q = lane == 0 ? ((m >> 5) & 1u ? &T.where[m >> 8] : scr16()) : other;
        *q = (uint16_t)(lane == 0 ? opos : oval);
    }

    // after a miss: cache symbol sym at position s with its path (lanes >= d hold kRoot) and
    // its code record rec (1 << d | code bits). Replacement: an entry dropped by a swap (or
    // never used) first, lowest number; otherwise FIFO (tests/fgk_cache_model.py: on the photo
    // streams this misses less than a clock with reference bits, and a hit costs nothing).
    __device__ __forceinline__ void pc_insert(uint32_t sym, uint32_t s, uint32_t pv, uint32_t d, uint32_t rec)
    {
        if (d > kInsertDepth) return;
        pc_lb_ok = 0;
        uint32_t e;
        if (pc_free) {
            e = (uint32_t)__builtin_ctz(pc_free);
            pc_free &= pc_free - 1;
        } else {
            e = pc_next;
            pc_next = (e + 1) & (kSlots - 1);
        }
        // lane 0: the evicted symbol forgets its entry; lane 1: this symbol takes it
        pc_forget(e, lane == 1 ? &T.where[sym] : scr16(), s | ((e + 1) << 10));
        // lanes 0..11 the positions, 12 the code record, 13 depth | valid | symbol
        const uint32_t rv = lane < kSlotDepth ? pv : (lane == kSlotDepth ? rec : (d | 32u | (sym << 8)));
        *(lane < kSlotDepth + 2 ? &T.pc[e * kRow + lane] : scr16()) = (uint16_t)rv;
        __builtin_amdgcn_wave_barrier();
    }

    // pc_lb := the lightest cached leaf. Every position on a cached path weighs at least its
    // leaf and weights only grow, so until the next insert a swap of positions lighter than
    // that (the ties of rare symbols) touches no cached path and needs no scan.
    __device__ __forceinline__ void pc_bound()
    {
        if (pc_lb_ok) return;
        pc_lb_ok = 1;
        if constexpr (kHuge) {  // no bound: every swap scans the cache
            pc_lb = 0;
            return;
        }
        const uint32_t p0 = T.pc[(lane & (kSlots - 1)) * kRow];  // row (lane & 15)'s leaf
        const uint32_t w0 = (uint32_t)T.wt[min(p0, kRoot)];
        uint32_t lw = p0 <= kRoot ? (kWide ? w0 : w0 >> 10) : 0xFFFFFFFFu;  // 0xFFFF: unused row
        lw = min(lw, (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)lw, 0x111, 0xF, 0xF, false));
        lw = min(lw, (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)lw, 0x112, 0xF, 0xF, false));
        lw = min(lw, (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)lw, 0x114, 0xF, 0xF, false));
        lw = min(lw, (uint32_t)__builtin_amdgcn_update_dpp(~0, (int)lw, 0x118, 0xF, 0xF, false));
        pc_lb = lane_read(lw, 15);
    }

    __device__ __forceinline__ void pc_drop(uint32_t e)
    {
        pc_forget(e, scr16(), 0);
        *(lane < kSlotDepth + 2 ? &T.pc[e * kRow + lane] : scr16()) = (uint16_t)(lane < kSlotDepth ? 0xFFFFu : 0u);
        __builtin_amdgcn_wave_barrier();
        pc_free |= 1u << e;
    }

    // positions s and l traded contents: drop every cached path through either. Read r covers
    // entries 4r..4r+3, one position per lane (lane 16j + k: level k of entry 4r + j; words
    // 12..15 of a row are metadata, masked out of the ballot); 16-bit segment j flags entry
    // 4r + j.
    __device__ __forceinline__ void pc_swapped(uint32_t s, uint32_t l)
    {
        constexpr uint64_t kLevels = 0x0FFF0FFF0FFF0FFFull;
        uint32_t q[kSlots / 4];
        uint64_t m[kSlots / 4];
#pragma unroll
        for (uint32_t r = 0; r < kSlots / 4; ++r) q[r] = T.pc[64 * r + lane];
#pragma unroll
        for (uint32_t r = 0; r < kSlots / 4; ++r) m[r] = (ballot(q[r] == s) | ballot(q[r] == l)) & kLevels;
#pragma unroll
        for (uint32_t r = 0; r < kSlots / 4; ++r) {
            while (m[r]) {
                const uint32_t j = (uint32_t)__builtin_ctzll(m[r]) >> 4;
                m[r] &= ~(0xFFFFull << (16 * j));
                pc_drop(4 * r + j);
            }
        }
    }

    // ---- decoder level tables (tests/fgk_cache_model.py: LevelTables). Level j's entry for a
    // j-bit prefix is where the walk from the root along those bits stops (position | depth <<
    // 10); built breadth first, each level from the one above. A swap stales them only when it
    // moves the content of a position some walk passes through: those carry the generation.
    // from = 0: all levels, a new generation; otherwise levels from..8 (the entries above reach
    // neither swapped position, so they and the marks they set stand)
    __device__ __forceinline__ void build_levels()
    {
        uint32_t j0 = from;
        if (j0 == 0) {
            gen = gen == 31 ? 1u : gen + 1;
            j0 = 1;
            stale = 0;
        }
        from = 9;
#pragma unroll 1
        for (uint32_t j = j0; j <= 8; ++j) {
            const uint32_t cnt = 1u << j;
            for (uint32_t r = 0; r * 64 < cnt; ++r) {
                const uint32_t q = lane + 64 * r;
                const bool on = q < cnt;
                const uint32_t pe = j == 1 ? kRoot : T.lvl[(cnt >> 1) - 2 + (on ? q >> 1 : 0)];
                const uint32_t x = pe & 1023u;
                const uint32_t b = T.body[x];
                const bool inner = (b & kInner) && (pe >> 10) == j - 1;
                *(on && inner ? &T.body[x] : scr16()) = (uint16_t)((b & kContent) | (gen << kMarkShift));
                const uint32_t ne = inner ? (((b & 255u) * 2 + (q & 1u)) | (j << 10)) : pe;
                *(on ? &T.lvl[cnt - 2 + q] : scr16()) = (uint16_t)ne;
                if constexpr (kTab)  // the child reached at depth j has code q
                    *(on && inner ? &T.pcode[(b & 255u) * 2 + (q & 1u)] : scr16()) = (uint16_t)((q << (8 - j)) | ((j - 1) << 8));
            }
            __builtin_amdgcn_wave_barrier();
        }
    }

    // decoder: the shallowest level < 8 whose entries hold position s or l (8 if none does).
    // Level j's entries sit at 2^j - 2 .. 2^(j+1) - 3 and a position first appears at its
    // depth, so the lowest matching index names it (level 8's entries stay right: a position
    // they stop at is walked on by the descent). Entries of levels >= from may predate a swap
    // earlier in this walk; a match there gives a level >= from - 1, leaving from as it is.
    __device__ __forceinline__ uint32_t table_level(uint32_t s, uint32_t l)
    {
        for (uint32_t r = 0; r < 4; ++r) {
            const uint32_t i = r * 64 + lane;
            const uint32_t p = T.lvl[i] & 1023u;
            const uint64_t m = (ballot(p == s) | ballot(p == l)) & (r == 3 ? 0x3FFFFFFFFFFFFFFFull : ~0ull);
            if (m) return 31 - __builtin_clz(r * 64 + ff1(m) + 2);
        }
        return 8;
    }

    // huffman.cpp:99-111: split NYT at t -> NYT at t-2 (left), symbol leaf at t-1 (right).
    // Lanes 0..2 write the three bodies, lanes 0..1 the two parent links, lane 0 the map.
    __device__ __forceinline__ uint32_t split(uint32_t sym)
    {
        const uint32_t t = nyt;
        const uint32_t bpos = lane == 0 ? t : (lane == 1 ? t - 2 : t - 1);
        constexpr uint32_t nl = kDec ? kNotLeaf : 0u;
        const uint32_t bval = lane == 0 ? (kInner | nl | ((t - 2) >> 1)) : (lane == 1 ? kNyt | nl : sym);
        *(lane < 3 ? &T.body[bpos] : scr16()) = (uint16_t)bval;
        if (!kDec) *(lane == 0 ? &T.where[sym] : scr16()) = (uint16_t)(t - 1);
        if constexpr (kWide) *(lane < 2 ? &T.up[t - 2 + lane] : scr16()) = (uint16_t)t;
        else *(lane < 2 ? &T.wt[t - 2 + lane] : scr32()) = t;  // weight 0, parent t
        __builtin_amdgcn_wave_barrier();
        nyt = t - 2;
        return t - 1;
    }

    // huffman.cpp:186-217 in slot form: exchange the contents of positions s and l (their
    // weights are equal), then re-point what hangs below them. Lane k < 2 writes the content
    // moving into (k ? l : s); lane k < 4 re-parents child (k & 1) of content (k >> 1).
    __device__ __forceinline__ void swap(uint32_t s, uint32_t l, bool scan)
    {
        // encoder: drop the cached paths through s or l first (scan: they may lie on one); the
        // relink below then gives a moved leaf's where[] its new position
        if (!kTabs && scan) {
            HC_PROF_BEGIN();
            pc_swapped(s, l);
            HC_PROF_END(7);
        }
        // lane-parallel: lane & 1 = 0 handles the content moving to s (read at l), 1 the one
        // moving to l; lanes 2, 3 (lane >> 1 = 1) re-parent the second child of the same content
        const uint32_t pos = (lane & 1) ? l : s;        // where the lane's content goes
        const uint32_t b = T.body[(lane & 1) ? s : l];  // that content
        if (kTabs) {
            // generation marks stay with the positions: the destination's own word is the
            // partner lane's read (quad_perm [1,0,3,2])
            const uint32_t bo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)b, 0xB1, 0xF, 0xF, false);
            *(lane < 2 ? &T.body[pos] : scr16()) = (uint16_t)((b & kContent) | (bo & (31u << kMarkShift)));
            if (ballot(((b >> kMarkShift) & 31u) == gen) & 3u) from = min(from, table_level(s, l) + 1);
            if (!kDec) *(lane < 2 && !(b & kInner) ? &T.where[b & 255u] : scr16()) = (uint16_t)pos;
        } else {
            *(lane < 2 ? &T.body[pos] : scr16()) = (uint16_t)b;
            *(lane < 2 && !(b & kInner) ? &T.where[b & 255u] : scr16()) = (uint16_t)pos;
        }
        const bool inner = lane < 4 && (b & kInner);
        const uint32_t c = (b & 255u) * 2 + (lane >> 1);
        if constexpr (kWide) {
            *(inner ? &T.up[c] : scr16()) = (uint16_t)pos;
        } else {
            // the parent field, in place: LDS and / or without return (no read round trip; this
            // wave's later LDS reads come after them in order)
            uint32_t *q = inner ? &T.wt[c] : scr32();
            __hip_atomic_fetch_and(q, ~1023u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            __hip_atomic_fetch_or(q, pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
        __builtin_amdgcn_wave_barrier();
    }

    // highest position >= from whose weight equals that of word w, when positions
    // from-64..from-1 all had it (the sentinels above the root end the scan)
    __device__ __forceinline__ uint32_t leader_far(uint32_t from, Wt w)
    {
        const Wt lim = kWide ? w : (w | 1023u);
        for (;;) {
            const uint64_t le = ballot(T.wt[min(from + lane, kWords - 1)] <= lim);
            if (le != ~0ull) return from + (uint32_t)__builtin_ctzll(~le) - 1;
            from += 64;
        }
    }

    // decoder: the position of symbol sym's leaf, 0xFFFFFFFF if it has none (lane-parallel scan
    // of body[]; only a corrupted stream names a known symbol after the NYT code)
    __device__ __forceinline__ uint32_t find_leaf(uint32_t sym)
    {
        for (uint32_t r = 0; r * 64 <= kRoot; ++r) {
            const uint32_t p = r * 64 + lane;
            const uint32_t b = T.body[min(p, kRoot)];
            // positions at or below the NYT are unused (body 0 would read as symbol 0)
            const uint64_t m = ballot(p > nyt && p <= kRoot && !(b & (kInner | kNyt)) && (b & 255u) == sym);
            if (m) return r * 64 + (uint32_t)__builtin_ctzll(m);
        }
        return 0xFFFFFFFFu;
    }

    __device__ __forceinline__ uint32_t parent(uint32_t x) const
    {
        return kWide ? uni(T.up[x]) : (uni((uint32_t)T.wt[x]) & 1023u);
    }

#if HC_CHASE_GROUP
    // chase() of the path-cache encoder with the levels climbed back to back (parent read, mask,
    // next address) and the root tested once per group: level k's position goes straight into
    // lane k (a select on a one-bit scalar mask), so the path arrives bottom-up. The first group
    // is levels 0..kProbe, where the path cache is probed as in chase(); the groups after a failed
    // probe are HC_CHASE_GROUP levels each. A climb that passes the root stays in the tree: the
    // root's parent field (narrow) and up[kRoot] (wide / huge) are 0 and never written, and
    // position 0 holds 0 or a real node's parent, so every position read is <= kRoot. The depth is
    // the first lane holding kRoot (the lanes not yet written hold it too); the lanes from there
    // on are set to kRoot. (tests/fgk_climb_model.py: Climb)
    __device__ __forceinline__ uint32_t chase_grouped(uint32_t s0, uint32_t &pv)
    {
        constexpr uint32_t kGroup = HC_CHASE_GROUP;
        static_assert(kProbe < 63 && (63 - kProbe) % kGroup == 0, "the groups end at lane 63");
        uint32_t s = vreg(s0);  // per-level work on the VALU (see vreg)
        uint32_t tv = kRoot;    // lane k: level k
#pragma unroll
        for (uint32_t i = 0; i < kProbe; ++i) {
            tv = sel(1ull << i, s, tv);
            s = kWide ? (uint32_t)T.up[s] : ((uint32_t)T.wt[s] & 1023u);
        }
        tv = sel(1ull << kProbe, s, tv);
        uint32_t d = ff1(ballot(tv == kRoot));
        if (d > kProbe) {
            // s: level kProbe, below the root. A cached path through it (rows stay valid paths)
            // gives the rest of the climb at once
            constexpr uint64_t kLevels = 0x0FFF0FFF0FFF0FFFull;
            uint32_t q[kSlots / 4];
            uint64_t m[kSlots / 4];
#pragma unroll
            for (uint32_t r = 0; r < kSlots / 4; ++r) q[r] = T.pc[64 * r + lane];
#pragma unroll
            for (uint32_t r = 0; r < kSlots / 4; ++r) m[r] = ballot(q[r] == s) & kLevels;
            const uint64_t m01 = m[0] | m[1], m23 = m[2] | m[3];
            if (m01 | m23) {
                // the first hit: entry e, level lv of its row
                const uint32_t r = m01 ? (m[0] ? 0u : 1u) : (m[2] ? 2u : 3u);
                const uint32_t b = ff1(r == 0 ? m[0] : r == 1 ? m[1] : r == 2 ? m[2] : m[3]);
                const uint32_t e = 4 * r + (b >> 4), lv = b & 15u;
                // lane j >= kProbe: level j = the row's level lv + j - kProbe (kRoot from the
                // row's depth on, and past its 12 levels)
                const uint32_t idx = lv + lane - kProbe;
                const uint32_t rv = T.pc[e * kRow + min(idx, kRow - 1)];
                const uint32_t drow = uni(T.pc[e * kRow + kSlotDepth + 1]) & 31u;
                pv = lane < kProbe ? tv : (idx < kSlotDepth ? rv : kRoot);
                return kProbe + drow - lv;
            }
            uint64_t mk = 1ull << kProbe;  // the lane of the last level recorded
            uint32_t nx = kProbe + 1;      // the next lane
#pragma unroll 1
            do {  // fixed trip bound: the lanes
#pragma unroll
                for (uint32_t i = 0; i < kGroup; ++i) {
                    s = kWide ? (uint32_t)T.up[s] : ((uint32_t)T.wt[s] & 1023u);
                    mk <<= 1;
                    tv = sel(mk, s, tv);
                }
                nx += kGroup;
                d = ff1(ballot(tv == kRoot));
            } while (min(d, 63u) >= nx);  // (nx ends at 64)
        }
        // no root within 63 levels (parents sit above children, so this only bounds a bug):
        // d = 0xFFFFFFFF
        bad |= d >> 6;
        pv = sel(below_mask(d), tv, kRoot);
        return min(d, 64u);
    }
#endif

    // Encoder: the path from position s to the root, BEFORE the update (the code of
    // huffman.cpp:136-155): the position of level k (0 = s) goes to lane k; returns the levels.
    // Each level enters at lane 0 by a DPP wave shift (lane 0 keeps the new position), so the
    // path arrives top-down; one permute turns it bottom-up at the end.
    __device__ __forceinline__ uint32_t chase(uint32_t s0, uint32_t &pv)
    {
#if HC_CHASE_GROUP
        // (the small-alphabet launch keeps the per-level climb: its trees are rarely deeper than
        // the grouped climb's first kProbe levels, which always run)
        if constexpr (!kTabs && !kSmall) return chase_grouped(s0, pv);
#endif
        int32_t km = -64;       // levels - 64
        uint32_t s = vreg(s0);  // per-level work on the VALU (see vreg)
        uint32_t td = kRoot;    // lane j: level k - 1 - j
        if (!kTabs) {
            // encoder: kProbe levels, then look the position up in the path cache: a cached
            // path through it (rows stay valid paths) gives the rest of the climb at once
#pragma unroll
            for (uint32_t i = 0; i < kProbe; ++i) {
                const uint32_t sh = __builtin_amdgcn_update_dpp(0u, td, 0x138, 0xF, 0xF, true);
                td = lane == 0 ? s : sh;
                ++km;
                s = kWide ? (uint32_t)T.up[s] : ((uint32_t)T.wt[s] & 1023u);
                if (uni(s) == kRoot) break;
            }
            const uint32_t c = uni(s);
            if (c != kRoot) {
                constexpr uint64_t kLevels = 0x0FFF0FFF0FFF0FFFull;
                uint32_t q[kSlots / 4];
                uint64_t m[kSlots / 4];
#pragma unroll
                for (uint32_t r = 0; r < kSlots / 4; ++r) q[r] = T.pc[64 * r + lane];
#pragma unroll
                for (uint32_t r = 0; r < kSlots / 4; ++r) m[r] = ballot(q[r] == c) & kLevels;
                const uint64_t m01 = m[0] | m[1], m23 = m[2] | m[3];
                if (m01 | m23) {
                    // the first hit: entry e, level lv of its row
                    const uint32_t r = m01 ? (m[0] ? 0u : 1u) : (m[2] ? 2u : 3u);
                    const uint32_t b = ff1(r == 0 ? m[0] : r == 1 ? m[1] : r == 2 ? m[2] : m[3]);
                    const uint32_t e = 4 * r + (b >> 4), lv = b & 15u;
                    const uint32_t n = (uint32_t)(km + 64);  // levels chased: c is level n
                    // lane j >= n: level j = the row's level lv + j - n (kRoot from the row's
                    // depth on, and past its 12 levels)
                    const uint32_t idx = lv + lane - n;
                    const uint32_t rv = T.pc[e * kRow + min(idx, kRow - 1)];
                    const uint32_t drow = uni(T.pc[e * kRow + kSlotDepth + 1]) & 31u;
                    const uint32_t dn =
                        (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((n - 1 - lane) & 63u) * 4), (int)td);
                    pv = lane < n ? dn : (idx < kSlotDepth ? rv : kRoot);
                    return n + drow - lv;
                }
            }
        }
        if (kTabs || uni(s) != kRoot) do {
            // wave_shr:1, lane 0 taking s
            const uint32_t sh = __builtin_amdgcn_update_dpp(0u, td, 0x138, 0xF, 0xF, true);
            td = lane == 0 ? s : sh;
            ++km;
            s = kWide ? (uint32_t)T.up[s] : ((uint32_t)T.wt[s] & 1023u);
            // go on while s is not the root (x - 1 >= 0) and fewer than 64 levels (km < 0;
            // parents sit above children, so this only bounds a bug): one sign test
        } while ((int32_t)((uint32_t)km & ~((uni(s) ^ kRoot) - 1u)) < 0);
        uint32_t k = (uint32_t)(km + 64);
        asm volatile("" : "+s"(k));  // the depth, opaque: no loop-strength-reduced copies of it
        bad |= uni(s) ^ kRoot;
        const uint32_t j = k - 1 - lane;  // lane < k: the lane holding this lane's level
        pv = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((j & 63u) * 4), (int)td);
        pv = lane < k ? pv : kRoot;
        return k;
    }

    // huffman.cpp:95-128 (update), serial form, from position s upward: per level one
    // lane-parallel read of positions s..s+63, one ballot (the trailing-ones count of
    // "weight == w[s]" is the block leader, highest number first), a swap when the leader is
    // neither s nor its parent, one store.
    // pv: the root path the update started on (lane k: level k, kRoot lanes above). After the
    // level at s, the climb from its parent is chased (one LDS read per position, no leader
    // test) until it meets a position of pv -- every swap so far moved only positions below
    // that one, and pv's kRoot lanes end any climb at the root. The chased positions and pv
    // above the meeting point are the rest of the root path, finished lane-parallel like
    // update_fast; a level that reports there is walked again, the new path taking pv's role.
    // bounded: the encoder's pc_lb is current (pc_bound since the last insert): swaps below it
    // skip the cache scan
    __device__ __forceinline__ void walk(uint32_t s, uint32_t pv, bool bounded = false)
    {
        for (;;) {
            const Wt v = T.wt[s + lane];  // sentinels cover s + 63 <= 575
            Wt ws = uniw(v);
            const uint64_t le = ballot(v <= (kWide ? ws : (ws | 1023u)));
            uint32_t p = kWide ? uni(T.up[s]) : ((uint32_t)ws & 1023u);
            // lane 0 read position s: its address and word, incremented, are the store's
            Wt *dst = &T.wt[s + lane];
            Wt nv = v + kInc;
            bool again = false;  // the parent's level is walked too (no chase)
            if ((uint32_t)le & 2u) {  // s+1 weighs the same: find the block leader
                const uint32_t lead =
                    ~le ? s + (uint32_t)__builtin_ctzll(~le) - 1 : leader_far(s + 64, ws);
                if (lead != p) {
                    // a light position that swapped: in the long blocks of equal small weights
                    // its new parent usually ties as well, and testing it here costs one read
                    // where the chase back to pv and update_from cost several
                    again = (kWide ? ws : ws >> 10) < kWalkLight;
                    swap(s, lead, !kDec && (!bounded || (kWide ? ws : ws >> 10) >= pc_lb));
                    // the swap rewrites only parent fields below s and lead, never their own
                    // words, so the pre-swap read still holds lead's word when in range
                    const uint32_t off = lead - s;
                    ws = off < 64 ? readw(v, off) : uniw(T.wt[lead]);
                    s = lead;
                    p = kWide ? uni(T.up[s]) : ((uint32_t)ws & 1023u);
                    dst = &T.wt[s];
                    nv = ws + kInc;
                }
            }
            *(lane == 0 ? dst : scrw()) = nv;
            __builtin_amdgcn_wave_barrier();
            if (again && p != kRoot) {
                s = p;
                continue;
            }
            // chase from the parent until a position of pv; lane j of td: the j-th one passed. The
            // climbing position stays in a VGPR (wave-uniform): each level is a compare, a select
            // into lane n (a scalar bit mask), the parent read and a mask -- no hop through the
            // scalar unit (with the position in an SGPR the compiler spent ~6 VALU + 11 SALU per
            // level on copies, readfirstlane and the address)
            if constexpr (kLean) {
                uint32_t c = p, td = kRoot;
                uint64_t lm = 1;  // the lane the next chased position goes to
                climb_to<kWide>(c, td, lm, pv, kWide ? lds_off16(&T.up[0]) : lds_off(&T.wt[0]));
                if (lm == 0) {  // 64 levels: a valid path is shorter (pv's kRoot lanes end every climb): a bug
                    bad = 1;
                    return;
                }
                const uint64_t on = lanes_eq(pv, c);
                uint32_t k;
                if (lm == 1) {
                    // met at once: pv from the meeting lane up is the rest of the path as it stands
                    k = update_from(pv, ff1(on));
                } else {
                    const uint32_t n = (uint32_t)__builtin_ctzll(lm);
                    const uint32_t src = lane - n + ff1(on);
                    const uint32_t up = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src * 4), (int)pv);
                    pv = lane < n ? td : (src < 64 ? up : kRoot);
                    k = update_from(pv, 0);
                }
                if (k == 0xFFFFFFFFu) return;  // the root too
                s = lane_read(pv, k);
            } else {
                uint32_t c = vreg(p), n = 0, td = kRoot;
                uint64_t on;
#pragma unroll 1
                while ((on = ballot(pv == c)) == 0) {
                    td = sel(1ull << n, c, td);
                    if (++n >= 63) {  // a valid path is shorter (pv's kRoot lanes end every climb): a bug
                        bad = 1;
                        return;
                    }
                    c = kWide ? (uint32_t)T.up[c] : ((uint32_t)T.wt[c] & 1023u);
                }
                // lane j < n: chased; lane j >= n: pv's lane j - n + m (kRoot past its lane 63)
                const uint32_t src = lane - n + ff1(on);
                const uint32_t up = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src * 4), (int)pv);
                pv = lane < n ? td : (src < 64 ? up : kRoot);
                const uint32_t k = update_from(pv, 0);
                if (k == 0xFFFFFFFFu) return;  // the root too
                s = lane_read(pv, k);
            }
        }
    }

    // The same update when the path is already known: lanes 0..d-1 hold the positions of
    // levels 0..d-1, the other lanes kRoot. Until the first swap the tree does not change, so
    // every level's leader test reads the pre-update words in parallel. A level leads its block
    // when the next position is heavier; the test cannot miss a non-leader, and it reports one
    // falsely only when that next position is the level's own parent and the sibling weighs 0
    // (the NYT): the walk, which repeats the exact test from the first reported level, handles
    // both. The root lanes always lead (the sentinel above is heavier). Levels below the first
    // reported one increment with one store; without a report the root lanes bump the root in
    // the same store. update_fast() is this lane-parallel part; it returns the first reported
    // level (0xFFFFFFFF: none), where walk() continues.
    // force (wave-uniform, 0 or 0xFFFFFFFF): report level 0, store nothing (the limit becomes
    // all ones, above every weight word and sentinel)
    template <class Ahead>
    __device__ __forceinline__ uint32_t update_fast(uint32_t a, Ahead &&ahead, uint32_t force = 0)
    {
        const Wt w0 = T.wt[a], w1 = T.wt[a + 1];
        ahead();  // the caller's reads for later symbols go out behind these
        const Wt nv = w0 + kInc;
        const Wt fw = (Wt)0 - (Wt)(force & 1u);  // force as a weight-wide mask
        // narrow: w1 < w0 + 1024 (the increment stored anyway) reports every level whose next
        // position is not heavier, and falsely (the walk then decides) only one whose next
        // position is exactly one heavier with a lower parent field (parents grow with the
        // position in practice: 0 of 600k level tests on a photo stream, 1 of 7.7k on a
        // gradient, slot-form model). The encoder's miss row's sentinel pair (all ones, 0)
        // fails: all ones + 1024 wraps to 1023; the decoder's force makes the limit all ones,
        // above its sentinels (all ones - 1).
        const uint64_t fail = ballot(kHuge ? (w1 <= (w0 | fw)) : kWide ? (w1 <= (w0 | force | (force >> 1))) : (w1 < (nv | force)));
        const uint32_t k = ff1(fail);  // 0xFFFFFFFF without a failure: every lane increments
        // lanes below k store: the select runs on a scalar mask (s_bfm_b64), one vector op
        // (measured: an exec-masked store, s_bfm + save/restore of exec, made the encoder 3 %
        // slower than a compare and select)
        *(__attribute__((address_space(3))) Wt *)(size_t)sel(below_mask(k), lds_off(&T.wt[a]), lds_off(scrw())) = nv;
        __builtin_amdgcn_wave_barrier();
        return k;
    }
    // update_fast for the levels from lane m up (the lanes below are levels already done):
    // returns the first reported level >= m (0xFFFFFFFF: none, the root lanes bumped the root)
    __device__ __forceinline__ uint32_t update_from(uint32_t a, uint32_t m)
    {
        const Wt w0 = T.wt[a], w1 = T.wt[a + 1];
        const Wt nv = w0 + kInc;
        const uint64_t lo = below_mask(m);
        const uint64_t fail = ballot(kWide ? (w1 <= w0) : (w1 < nv)) & ~lo;
        const uint32_t k = ff1(fail);
        *(__attribute__((address_space(3))) Wt *)(size_t)sel(below_mask(k) & ~lo, lds_off(&T.wt[a]), lds_off(scrw())) = nv;
        __builtin_amdgcn_wave_barrier();
        return k;
    }
    __device__ __forceinline__ void update_path(uint32_t a)
    {
        const uint32_t k = update_fast(a, [] {});
        if (k != 0xFFFFFFFFu) walk(lane_read(a, k), a);
    }
};

// -------------------------------------------------------------- MNP-5 pre-pass (encoder) --

// Carry between chunks: last raw byte (diff model), run counter after the last byte (0 = no
// run: stream start or a 258-byte cut), last transformed byte.
struct RleCarry {
    uint32_t x, R, c;
};

__device__ __forceinline__ uint32_t byte_of(uint32_t w, uint32_t b) { return (w >> (8 * b)) & 255u; }

// transform.cpp:220-229 + 241-279 for one chunk, all lanes at once (model and derivation:
// tests/rle_chunk_model.py). Lane l holds raw bytes 4l..4l+3 of the chunk in x4, m (1..256) are
// valid, fin says byte m-1 is the stream's last. Per byte: k = offset in its run (the run may
// continue from the previous chunk), km = k mod 258, run counter R = km + 1 (0 at the cut);
// a byte emits the previous run's count byte and itself when a run starts (or it is the final
// byte), itself at km 1..2, 255 at km 257, nothing otherwise. The chunk's symbols are appended
// to the at symbols pending in sb[] (room for cap); returns the symbols pending after the chunk,
// or -- when they would not fit -- sets full, writes nothing and leaves the carry as it was (the
// caller codes the pending symbols and runs the chunk again).
// Fast path (rle_chunk_model.pure_chunk): a full, non-final chunk whose 256 transformed bytes all
// continue the carried byte's run puts byte i at km = (R + i) mod 258, so it emits only the
// events of the residues 257 (255), 0, 1, 2 (the byte) that fall on i <= 255: in byte order the
// cyclic order 257, 0, 1, 2 rotated to start at R when R <= 2, lane j < 4 taking entry j.
template <int kSrc>
__device__ __forceinline__ uint32_t rle_chunk(uint32_t x4, uint32_t m, uint32_t fin, RleCarry &cy, uint8_t *sb,
                                              uint32_t at, uint32_t cap, uint32_t *scr, uint32_t lane, uint32_t &full,
                                              uint32_t &start_lanes)
{
    const uint32_t xprev = (x4 << 8) | (wave_shr1(x4, cy.x << 24) >> 24);
    // bytewise x - xprev (mod 256), SWAR
    const uint32_t c4 = kSrc == SRC_RAW_DIFF
                            ? (((x4 | 0x80808080u) - (xprev & 0x7F7F7F7Fu)) ^ ((x4 ^ ~xprev) & 0x80808080u))
                            : x4;
    uint8_t *sc = reinterpret_cast<uint8_t *>(scr);
    if (m == 256 && !fin && ballot(c4 != cy.c * 0x01010101u) == 0) {
        start_lanes = cy.R == 0 ? 1u : 0u;
        const uint32_t R = cy.R;
        const uint32_t rot = R <= 2 ? R + 1 : 0;
        const uint32_t q = (lane + rot) & 3u;
        const uint32_t e = q == 0 ? 257u : q - 1;
        uint32_t i = e + 258 - R;
        i = i >= 258 ? i - 258 : i;
        const bool on = lane < 4 && i <= 255;
        const uint32_t total = (uint32_t)__builtin_popcountll(ballot(on));
        if (at + total > cap) {
            full = 1;
            return at;
        }
        *(on ? sb + at + lane : sc) = (uint8_t)(e == 257 ? 255u : cy.c);
        __builtin_amdgcn_wave_barrier();
        cy.x = lane_read(x4, 63) >> 24;
        cy.R = R + 256 >= 258 ? R - 2 : R + 256;
        return at + total;
    }
    const uint32_t cprev = (c4 << 8) | (wave_shr1(c4, cy.c << 24) >> 24);
    const int i0 = (int)(lane * 4);
    uint32_t start[4], any = 0;
    int last = -1;
    for (uint32_t b = 0; b < 4; ++b) {
        uint32_t same = byte_of(c4, b) == byte_of(cprev, b);
        if (b == 0) same &= lane != 0 || cy.R != 0;  // lane 0 byte 0: continues the carry's run?
        start[b] = (uint32_t)(i0 + (int)b < (int)m) & (same ^ 1u);
        any |= start[b];
        last = start[b] ? i0 + (int)b : last;
    }
    // latest run start in the lanes below (else the carried run, begun at -R)
    const uint64_t anyl = ballot(any != 0);
    start_lanes = (uint32_t)__builtin_popcountll(anyl);
    const uint64_t amask = anyl & ((1ull << lane) - 1ull);
    const int src = amask ? 63 - __builtin_clzll(amask) : 0;
    const int below = __builtin_amdgcn_ds_bpermute(src * 4, last);
    int ls = amask ? below : -(int)cy.R;
    uint32_t R[4], km[4];
    for (uint32_t b = 0; b < 4; ++b) {
        ls = start[b] ? i0 + (int)b : ls;
        const uint32_t k = (uint32_t)(i0 + (int)b - ls);
        km[b] = k >= 258 ? k - 258 : k;
        R[b] = km[b] == 257 ? 0u : km[b] + 1;
    }
    const uint32_t upR = wave_shr1(R[3], cy.R);
    uint32_t n[4], s0[4], s1[4], tot = 0;
    for (uint32_t b = 0; b < 4; ++b) {
        const uint32_t i = (uint32_t)i0 + b;
        const uint32_t rp = b ? R[b - 1] : upR;
        const uint32_t c = byte_of(c4, b);
        const uint32_t valid = i < m ? 1u : 0u;
        const uint32_t newrun = ((fin & (i + 1 == m ? 1u : 0u)) | (km[b] == 0 ? 1u : 0u));
        const uint32_t cnt = newrun & (rp >= 3 ? 1u : 0u);
        const uint32_t lit = km[b] == 1 || km[b] == 2 ? 1u : 0u;
        const uint32_t cut = km[b] == 257 && !newrun ? 1u : 0u;
        n[b] = valid * (newrun ? 1 + cnt : (lit | cut));
        s0[b] = cnt ? rp - 3 : (cut ? 255u : c);
        s1[b] = c;
        tot += n[b];
    }
    // exclusive prefix of the per-lane totals (<= 8): bit planes, ballot + mbcnt
    uint32_t basepos = 0;
    for (uint32_t p = 0; p < 4; ++p) {
        const uint64_t bm = ballot((tot >> p) & 1u);
        basepos += __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u)) << p;
    }
    const uint32_t total = lane_read(basepos + tot, 63);
    if (at + total > cap) {
        full = 1;
        return at;
    }
    uint32_t o = at + basepos;
    for (uint32_t b = 0; b < 4; ++b) {
        *(n[b] >= 1 ? sb + o : sc) = (uint8_t)s0[b];
        *(n[b] == 2 ? sb + o + 1 : sc + 1) = (uint8_t)s1[b];
        o += n[b];
    }
    __builtin_amdgcn_wave_barrier();
    // carries: the chunk's last byte
    const uint32_t L = m - 1, ll = L >> 2, lb = L & 3u;
    const uint32_t rl = lb == 0 ? R[0] : (lb == 1 ? R[1] : (lb == 2 ? R[2] : R[3]));
    cy.x = byte_of(lane_read(x4, ll), lb);
    cy.c = byte_of(lane_read(c4, ll), lb);
    cy.R = lane_read(rl, ll);
    return at + total;
}

// A full, non-final block of kQ KB of a run-heavy stream (tests/rle_chunk_model.py: sparse_block,
// rle_blocked), lane l holding bytes 16 kQ l .. 16 kQ l + 16 kQ - 1 in x[0..4 kQ) (kQ 16-byte
// loads). When the block has at most kSparseStarts run starts and at most 63 symbols, it is coded
// by segments instead of byte by byte: the carried segment [0, p_0) continues the run before the
// block, and segment j = [p_j, p_j+1) is a new run. A segment emits its start's count (when the
// run before it reached R' >= 3: R' - 3) and c, then a symbol for every offset whose residue mod
// 258 is 0, 1, 2 (c) or 257 (255): the t-th of those is 255 when t % 4 == 3. The carried segment's
// residues start at the carried counter R instead. Lane j < S holds start j (its segment's length
// and event count), a scan of the counts places the segments, and each symbol's lane finds its
// segment by a max-scan over markers (one LDS row). Returns the symbols pending after the block,
// or kDense with nothing written and the carry unchanged (the caller then codes the block as
// 256-byte chunks). The caller guarantees room for 63 symbols.
#ifndef HC_SPARSE
#define HC_SPARSE 1
#endif
// KB per sparse block (1 or 2): 2 halves the blocks of a run-heavy stream (grad: every 2 KB block
// stays within the 16 starts and 63 symbols, slot-form model), 4 KB would not fit them
#ifndef HC_SPARSE_KB
#define HC_SPARSE_KB 2
#endif
// rle_block's start mask is 32 bits (one per run start slot), its positions stay below 2048 and
// mod258's exactness bound (v < 2321) holds only up to 2 KB blocks
static_assert(HC_SPARSE_KB == 1 || HC_SPARSE_KB == 2, "rle_block supports 1 KB and 2 KB sparse blocks only");
constexpr uint32_t kSparseStarts = 16;
constexpr uint32_t kDense = 0xFFFFFFFFu;
template <int kSrc, uint32_t kQ>
__device__ __forceinline__ uint32_t rle_block(const u32x4 *blk, RleCarry &cy, uint8_t *sb, uint32_t at, uint32_t *row,
                                              uint32_t lane)
{
    constexpr uint32_t kX = 4 * kQ;          // dwords per lane
    constexpr uint32_t kBytes = 1024 * kQ;   // bytes per block
    uint32_t x[kX];
#pragma unroll
    for (uint32_t k = 0; k < kX; ++k) x[k] = blk[k >> 2][k & 3];
    // transform.cpp:220-229: the diffed bytes (lane 0's previous byte is the carry's)
    uint32_t c[kX];
    uint32_t pb = wave_shr1(x[kX - 1], cy.x << 24) >> 24;
#pragma unroll
    for (uint32_t k = 0; k < kX; ++k) {
        const uint32_t xp = (x[k] << 8) | pb;
        c[k] = kSrc == SRC_RAW_DIFF ? (((x[k] | 0x80808080u) - (xp & 0x7F7F7F7Fu)) ^ ((x[k] ^ ~xp) & 0x80808080u)) : x[k];
        pb = x[k] >> 24;
    }
    // run starts: bit 4 k + b of M for byte b of c[k] (byte 0 of the block also when R = 0: a cut)
    uint32_t M = 0;
    pb = wave_shr1(c[kX - 1], cy.c << 24) >> 24;
#pragma unroll
    for (uint32_t k = 0; k < kX; ++k) {
        const uint32_t d = c[k] ^ ((c[k] << 8) | pb);
        const uint32_t f = ((((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u) >> 7;  // 1 per nonzero byte
        M |= ((f | (f >> 7) | (f >> 14) | (f >> 21)) & 15u) << (4 * k);
        pb = c[k] >> 24;
    }
    M |= lane == 0 && cy.R == 0 ? 1u : 0u;
    const uint32_t cnt = (uint32_t)__builtin_popcount(M);
    const uint32_t incl = wave_scan_add(cnt);
    const uint32_t S = lane_read(incl, 63);
    if (S > kSparseStarts) return kDense;
    // the starts in order: row[r] = position | run byte << 16 (writes past S land on row[63])
    {
        uint32_t r = incl - cnt, m = M;
        while (ballot(m != 0)) {
            const uint32_t b = m ? (uint32_t)__builtin_ctz(m) : 0u;
            uint32_t ck = c[0];
#pragma unroll
            for (uint32_t k = 1; k < kX; ++k) ck = (b >> 2) == k ? c[k] : ck;
            row[m ? r : 63u] = (lane * 4 * kX + b) | (((ck >> (8 * (b & 3u))) & 255u) << 16);
            r += m ? 1u : 0u;
            m &= m - 1u;
        }
    }
    __builtin_amdgcn_wave_barrier();
    const uint32_t pw = row[lane];
    const bool st = lane < S;
    const uint32_t p = st ? pw & 0xFFFFu : kBytes;
    const uint32_t cb = (pw >> 16) & 255u;
    const uint32_t R0 = cy.R;
    const uint32_t p0 = S ? lane_read(p, 0) : kBytes;
    // segment j: [p, pn); the run counter before its start: (R0 + p_0) mod 258 for j = 0, the
    // previous new run's length mod 258 otherwise
    const uint32_t pn = (uint32_t)__builtin_amdgcn_update_dpp((int)kBytes, (int)p, 0x130, 0xF, 0xF, false);  // wave_shl:1
    const uint32_t pp = wave_shr1(p, 0u);
    const uint32_t L = pn - p;
    auto mod258 = [](uint32_t v) {  // v < 2321 (the largest here: R0 + 2048 < 2306)
        return v - 258u * ((v * 2033u) >> 19);
    };
    const uint32_t Rp = mod258(lane == 0 ? R0 + p : p - pp);
    const uint32_t hc = Rp >= 3 ? 1u : 0u;  // the start emits a count R' - 3 first
    const uint32_t qL = (L * 2033u) >> 19;
    const uint32_t ne = st ? hc + 4 * qL + min(L - 258u * qL, 3u) : 0u;
    const uint32_t ninc = wave_scan_add(ne);
    // the carried segment: lane t < 16 kQ tests its t-th candidate (cycle t >> 2, entry t & 3 of
    // 257, 0, 1, 2 rotated to start at R0)
    const uint32_t rot = R0 <= 2 ? R0 + 1 : 0u;
    const uint32_t q = (lane + rot) & 3u;
    const uint32_t e = q == 0 ? 257u : q - 1u;
    const uint32_t ic = mod258(e + 258u - R0) + 258u * (lane >> 2);
    const uint32_t nc = (uint32_t)__builtin_popcountll(ballot(lane < 16 * kQ && ic < p0));
    const uint32_t total = nc + lane_read(ninc, 63);
    if (total > 63) return kDense;
    // markers: each start's key (its first symbol's index, count flag and value, run byte) at row
    // [its index]; an inclusive max-scan gives every symbol lane its segment (0: the carried one)
    row[lane] = 0u;
    __builtin_amdgcn_wave_barrier();
    const uint32_t base = nc + ninc - ne;
    row[st ? base : 63u] = 0x80000000u | (base << 24) | (hc << 23) | (((Rp - 3u) & 255u) << 8) | cb;
    __builtin_amdgcn_wave_barrier();
    uint32_t key = row[lane];
    key = max(key, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key, 0x111, 0xF, 0xF, false));  // row_shr:1
    key = max(key, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key, 0x112, 0xF, 0xF, false));  // row_shr:2
    key = max(key, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key, 0x114, 0xF, 0xF, false));  // row_shr:4
    key = max(key, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key, 0x118, 0xF, 0xF, false));  // row_shr:8
    key = max(key, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key, 0x142, 0xA, 0xF, false));  // row_bcast:15
    key = max(key, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key, 0x143, 0xC, 0xF, false));  // row_bcast:31
    // a start segment's symbol (selects per lane), else the carried segment's
    const uint32_t u = lane - ((key >> 24) & 63u), kc = (key >> 23) & 1u;
    const uint32_t vs = kc && u == 0 ? (key >> 8) & 255u : (((u - kc) & 3u) == 3u ? 255u : key & 255u);
    const uint32_t v = (key >> 31) ? vs : (e == 257 ? 255u : cy.c);
    *(lane < total ? sb + at + lane : reinterpret_cast<uint8_t *>(row + 63)) = (uint8_t)v;
    __builtin_amdgcn_wave_barrier();
    // carries: the block's last raw and diffed byte, the run counter after it
    cy.x = lane_read(x[kX - 1], 63) >> 24;
    cy.c = lane_read(c[kX - 1], 63) >> 24;
    cy.R = mod258(S ? kBytes - lane_read(p, S - 1) : R0 + kBytes);
    return at + total;
}

// ------------------------------------------------------------------------- output stage --

// Code records: the encoder does not shift bits per symbol. Symbol t's code becomes one record
// in lane t of a VGPR, 1 << len | code (len <= 31; the leading 1 marks the length), written with
// one compare + select. Every 64 records (and at the end) pack() turns them into bytes on the
// lanes: a DPP scan of the lengths gives each record its bit offset, each record ORs its head
// (and the tail that spills into the next word) into a 64-word LDS stage, and the complete
// words leave as one buffer store, big-endian. 64 records of <= 31 bits plus < 32 pending bits
// fill at most 63 words. The u64 count (words 0-1) is written at the end by the lanes that
// stored those words first, so program order keeps it last.
struct RecSink {
    rsrc_t rs;           // window of the output at byte 4 * wbase
    uint32_t wbase;      // first word of the window
    uint32_t lane;
    uint32_t *stage;  // the wave's 64 scratch words
    uint32_t vrec;    // lane k: record k of the current group
    uint32_t n;       // records in the group (outside the hot loop)
    uint32_t pend;    // bits of the first unfinished output word, MSB-aligned
    uint32_t nb;      // how many (< 32)
    uint32_t wout;    // its word index

    static __device__ __forceinline__ uint32_t scan_add(uint32_t x) { return wave_scan_add(x); }

    // append record rec as number n of the group (outside the hot loop)
    __device__ __forceinline__ void push(uint32_t rec)
    {
        vrec = lane == n ? rec : vrec;
        if (++n == 64) pack();
    }
    // the low n (<= 64) bits of x, MSB first, as records of <= 24 bits
    __device__ void push_bits(uint64_t x, uint32_t nbits)
    {
        while (nbits > 24) {
            nbits -= 24;
            push((1u << 24) | ((uint32_t)(x >> nbits) & 0xFFFFFFu));
        }
        if (nbits) push((1u << nbits) | ((uint32_t)x & ((1u << nbits) - 1u)));
    }

    __device__ void pack()
    {
        const uint32_t rec = lane < n ? vrec : 0u;
        const uint32_t len = rec ? 31u - (uint32_t)__builtin_clz(rec) : 0u;
        const uint32_t code = rec & ((1u << len) - 1u);
        const uint32_t msb = code << ((32u - len) & 31u);  // len 0: code 0
        const uint32_t incl = scan_add(len);
        const uint32_t p = nb + incl - len;  // bit offset in the group's words
        const uint32_t w = p >> 5, o = p & 31u;
        uint32_t head = msb >> o;
        const uint32_t tail = o + len > 32u ? msb << (32u - o) : 0u;
        head |= lane == 0 ? pend : 0u;
        stage[lane] = 0u;
        __builtin_amdgcn_wave_barrier();
        __hip_atomic_fetch_or(&stage[w], head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        __hip_atomic_fetch_or(&stage[w + 1], tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        __builtin_amdgcn_wave_barrier();
        const uint32_t word = stage[lane];
        const uint32_t total = nb + lane_read(incl, 63);
        const uint32_t full = total >> 5;  // <= 62
        buf_store(rs, lane < full ? (wout - wbase + lane) * 4 : kDrop, __builtin_bswap32(word));
        pend = lane_read(word, full);
        nb = total & 31u;
        wout += full;
        n = 0;
        __builtin_amdgcn_wave_barrier();
    }

    // the window starts at the current word (stores past cap fall outside every range); called
    // between input chunks (a chunk adds < 2 KB of output)
    __device__ void rebase(uint8_t *out, uint64_t cap)
    {
        wbase = wout;
        const uint64_t at = 4ull * wbase;
        rs = make_rsrc(out + at, at < cap ? (uint32_t)min(cap - at, (uint64_t)kMaxBufBytes) : 0u);
    }

    // pack what is left, zero-pad to a byte (transform.cpp:379-381), store the last 0..4 bytes;
    // returns the byte length
    __device__ __forceinline__ uint64_t finish()
    {
        if (n) pack();
        const uint32_t tail = (nb + 7u) >> 3;  // 0..4 bytes
        for (uint32_t b = 0; b < 4; ++b)
            buf_store8(rs, lane == 0 && b < tail ? (wout - wbase) * 4 + b : kDrop, pend >> (24 - 8 * b));
        return (uint64_t)wout * 4 + tail;
    }
};

// --------------------------------------------------------------------------- the encoder --

// Waves per SIMD each tree layout's LDS admits (8 four-wave workgroups per CU narrow, 6 wide, 4
// huge): the register budget the compiler may use (fewer scalar spills in the wide kernels,
// which C4's single long stream runs)
#ifndef HC_WPE0
#define HC_WPE0 8
#endif
template <int kW, bool kTab = false>
constexpr int kWavesPerSimd = kTab ? (kW == 0 ? 6 : 5) : (kW == 0 ? HC_WPE0 : (kW == 1 ? 6 : 4));

// Which way the encoder finds codes, voted per stream (status[] carries the vote until the
// encoder overwrites it with the stream's status; the two modes' launches run side by side on two
// HIP streams, launch_encode_src): the path cache when the stream's 16 most frequent
// symbols cover most of it (>= 60 %: the diff model's photos, 95 %), the level tables when the
// alphabet is flat (< 9 %: noise, ramps, 6-8 %) -- measured: photo -c -m 8192 streams cache 67
// ms / tables 131, noise -c -m 2048 485 / 227, ramps -c 8192 623 / 365 -- and in between (photos
// without the diff model, 10-13 %; hd01 -c -m 41 %) the tables only when every stream is
// resident at once in table mode's occupancy (photo -c 4096 streams 325 / 231 ms, 8192 401 /
// 436; the 4096^2 -c -a matrix, one stream, 6.25 / 2.97 s; hd01 -c -m alone 108 / 55 ms).
// Estimated from a sample of 16 KB (below): the byte of every run start (diff model applied), a
// 256-bin histogram per wave in LDS, the top 16 by repeated max.
constexpr int32_t kModeTables = -0x7A0, kModeCache = -0x7A1, kModeSmall = -0x7A2;
// small alphabet: at most this many distinct run-start bytes in the sample (grad -c -m: 2)
constexpr uint32_t kSmallVote = 4;
// the small-alphabet steps (encoder code_all_batch, decoder Dec::decode_small): kSmallK symbols
// of kSmallG lanes (levels, depth <= kSmallG) each, while every position is >= kSmallNyt (at
// most 16 symbols seen)
constexpr uint32_t kSmallG = 4, kSmallK = 15, kSmallNyt = kRoot - 32;
template <int kSrc>
__global__ __launch_bounds__(256) void enc_mode_kernel(Batch bt, uint32_t low_occ, uint32_t forced)
{
    __shared__ uint32_t hist[4][256];
    const uint32_t lane = lane_id(), wv = uni(threadIdx.x >> 6);
    const uint32_t sid = blockIdx.x * 4 + wv;
    if (sid >= bt.n) return;
    if (forced) {
        if (lane == 0) bt.status[sid] = forced == 2 ? kModeTables : (forced == 3 ? kModeSmall : kModeCache);
        return;
    }
    uint32_t *h = hist[wv];
    for (uint32_t i = lane; i < 256; i += 64) h[i] = 0;
    __builtin_amdgcn_wave_barrier();
    const uint64_t n = bt.in_lens[sid];
    const uint8_t *const in = bt.in + bt.in_offs[sid];
    // The sample: a stream of <= 16 KB whole, a longer one as 64 segments of 256 bytes spread
    // evenly over it (its first 16 KB alone misjudged hd01 -c -m, a flat top and then a wide
    // alphabet: cache 108 ms against tables 55 ms as a lone stream). Four bytes per lane and
    // segment, one dword load (the bytes of a last dword past the stream masked off); each byte's
    // previous byte comes from the dword before (lane - 1, lane 63 of the segment before when they
    // are contiguous, else the byte before the segment) and a spread segment's first symbol
    // starts a run.
    const bool spread = n > 16384;
    const uint32_t nseg = spread ? 64u : (uint32_t)((n + 255) / 256);
    uint32_t prev_raw = 0, prev_sym = 0, total = 0;  // lane 63's dwords of the last segment; run starts
#if HC_VOTE_BATCH
    // the spread segments are independent (each one's first symbol starts a run, its previous raw
    // byte is the byte before it): kVB segments' loads go out together, then their histogram
    // updates (one at a time, each waiting for its load, the vote was 64 global round trips long:
    // 0.11 ms of grad's 1.25 ms encode)
    if (spread) {
        constexpr uint32_t kVB = 8;
        // segment k starts at ((n - 256) k / 63) & ~3, stepped without a 64-bit division per
        // segment (the scalar unit has none: each was a long SALU sequence, 70 SALU a segment)
        const uint64_t q = uni64((n - 256) / 63);
        const uint32_t r = uni((uint32_t)((n - 256) - 63 * q));
        uint64_t ob = 0;   // q k + (r k) / 63
        uint32_t oa = 0;   // (r k) % 63
        for (uint32_t k0 = 0; k0 < 64; k0 += kVB) {
            uint32_t w[kVB], pr[kVB];
#pragma unroll
            for (uint32_t u = 0; u < kVB; ++u) {
                const uint64_t o = ob & ~3ull;
                ob += q;
                oa += r;
                if (oa >= 63) {
                    oa -= 63;
                    ++ob;
                }
                w[u] = buf_load(make_rsrc(in + o, 256u), 4 * lane);
                // the dword ending at the segment's first byte (its top byte: the byte before)
                // (no branch: a load under one would be waited for at the join)
                pr[u] = buf_load(make_rsrc(in + (o ? o - 4 : 0), 4u), 0u) & (o ? 0xFF000000u : 0u);
            }
#pragma unroll
            for (uint32_t u = 0; u < kVB; ++u) {
                uint32_t sy = w[u];
                if (kSrc == SRC_RAW_DIFF) {  // transform.cpp:220-229 (m[-1] = 0), bytewise
                    const uint32_t xp = (w[u] << 8) | (wave_shr1(w[u], pr[u]) >> 24);
                    sy = ((w[u] | 0x80808080u) - (xp & 0x7F7F7F7Fu)) ^ ((w[u] ^ ~xp) & 0x80808080u);
                }
                const uint32_t sp = (sy << 8) | (wave_shr1(sy, 0u) >> 24);
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t i = 4 * lane + j, v = byte_of(sy, j);
                    const bool start = i == 0 || v != byte_of(sp, j);
                    if (start) atomicAdd(&h[v], 1u);
                    total += (uint32_t)__builtin_popcountll(ballot(start));
                }
            }
        }
    }
    for (uint32_t k = 0; k < (spread ? 0u : nseg); ++k) {
#else
    for (uint32_t k = 0; k < nseg; ++k) {
#endif
        const uint64_t o = spread ? ((n - 256) * k / 63) & ~3ull : 256ull * k;
        const uint32_t len = (uint32_t)min(n - o, (uint64_t)256);
        const uint32_t w = buf_load(make_rsrc(in + o, (len + 3u) & ~3u), 4 * lane);
        if (spread) prev_raw = o ? (uint32_t)in[o - 1] << 24 : 0u;
        uint32_t sy = w;
        if (kSrc == SRC_RAW_DIFF) {  // transform.cpp:220-229 (m[-1] = 0), bytewise
            const uint32_t xp = (w << 8) | (wave_shr1(w, prev_raw) >> 24);
            sy = ((w | 0x80808080u) - (xp & 0x7F7F7F7Fu)) ^ ((w ^ ~xp) & 0x80808080u);
            prev_raw = lane_read(w, 63);
        }
        const uint32_t sp = (sy << 8) | (wave_shr1(sy, prev_sym) >> 24);
        prev_sym = lane_read(sy, 63);
        const bool first = spread || k == 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t i = 4 * lane + j, v = byte_of(sy, j);
            const bool start = i < len && ((first && i == 0) || v != byte_of(sp, j));
            if (start) atomicAdd(&h[v], 1u);
            total += (uint32_t)__builtin_popcountll(ballot(start));
        }
    }
    __builtin_amdgcn_wave_barrier();
    uint32_t c[4], top = 0;
    for (uint32_t k = 0; k < 4; ++k) c[k] = h[64 * k + lane];
    for (uint32_t r = 0; r < 16; ++r) {
        uint32_t mx = max(max(c[0], c[1]), max(c[2], c[3]));
        for (uint32_t d = 32; d; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64));
        top += mx;
        const uint64_t who = ballot(c[0] == mx || c[1] == mx || c[2] == mx || c[3] == mx);
        if (lane == (uint32_t)__builtin_ctzll(who)) {  // take out one of the maxima
            if (c[0] == mx) c[0] = 0;
            else if (c[1] == mx) c[1] = 0;
            else if (c[2] == mx) c[2] = 0;
            else c[3] = 0;
        }
    }
    const bool cache = total == 0 || 100ull * top >= 60ull * total || (100ull * top >= 9ull * total && !low_occ);
    // the distinct run-start bytes: at most kSmallVote -> the small-alphabet launch (whose steps
    // need <= 16 FGK symbols; a stream whose count bytes widen the alphabet falls back to the
    // regular batches there)
    uint32_t distinct = 0;
    for (uint32_t k = 0; k < 4; ++k) distinct += (uint32_t)__builtin_popcountll(ballot(h[64 * k + lane] != 0));
    const bool small = total != 0 && distinct <= kSmallVote;
    if (lane == 0) bt.status[sid] = small ? kModeSmall : (cache ? kModeCache : kModeTables);
}

template <int kW, int kSrc, bool kTab = false, bool kSmall = false>
__global__ __launch_bounds__(64 * HC_WAVES) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd<kW, kTab>))) void encode_kernel(Batch bt)
{
    __shared__ Tree<kW, false, kTab, kSmall> trees[kWaves];
    const uint64_t t0 = __builtin_amdgcn_s_memtime();
    const uint32_t lane = lane_id();
    const uint32_t wv = uni(threadIdx.x >> 6);
    const uint32_t sid = blockIdx.x * kWaves + wv;
    if (sid >= bt.n) return;
    uint64_t pacc = 0;  // HC_PROF regions
    (void)pacc;

    const uint64_t in_off = uni64(bt.in_offs[sid]);
    const uint64_t n = uni64(bt.in_lens[sid]);
    const uint64_t out_off = uni64(bt.out_offs[sid]);
    const uint64_t cap = uni64(bt.out_caps[sid]);

    // the worst-case symbol count (MNP-5 expands by at most 4/3) decides the tree layout; the
    // other layouts' launches skip the stream
    const uint64_t max_sym = kSrc == SRC_SYMBOLS ? n : n + n / 3 + 2;
    if (tree_kind(max_sym, bt.min_tree) != (uint32_t)kW) return;
    // narrow and wide: the cache, table and (narrow) small-alphabet launches split the streams
    // (enc_mode_kernel; a wide stream voted small takes the cache launch)
    if (kW <= 1) {
        const int32_t mode = (int32_t)uni((uint32_t)bt.status[sid]);
        if ((mode == kModeTables) != kTab || (kW == 0 && mode == kModeSmall) != kSmall) return;
    }
    const uint32_t window = window_bytes();

    Fgk<kW, false, kTab, kSmall> fgk(trees[wv], lane);
    RecSink sink;
    sink.rs = make_rsrc(bt.out + out_off, (uint32_t)min(cap, (uint64_t)kMaxBufBytes));
    sink.wbase = 0;
    sink.lane = lane;
    sink.stage = fgk.T.scratch;
    sink.vrec = 0;
    sink.n = 0;
    // headers.cpp:118-122: the flags byte opens word 2 (words 0-1: the u64 symbol count,
    // written at the end)
    const uint32_t flags = kSrc == SRC_SYMBOLS ? bt.flags : (kSrc == SRC_RAW_DIFF ? 0x80u : 0u);
    sink.pend = flags << 24;
    sink.nb = 8;
    sink.wout = 2;

    // input: 256-byte chunks ci < nch through a window; ioff = the next load's offset in it
    rsrc_t rin = make_rsrc(bt.in + in_off, (uint32_t)min((n + 3u) & ~3ull, (uint64_t)kMaxBufBytes));
    const uint32_t nch = (uint32_t)((n + 255) / 256);
    uint32_t ioff = 256;

    // transform.cpp:363-384: per symbol encode (path before update), then update. A symbol
    // whose root path is cached (the common case) takes the hot path, written so that its
    // wave-uniform values stay in VGPRs (the scalar unit is shared by the CU's 32 waves): the
    // symbol's path-cache row, the lane-parallel update, its record in lane t - koff. Anything
    // else (a symbol not cached, or unseen) takes the miss path, which appends its records
    // through the sink and re-bases koff. Positions stay in range by construction, so `bad` (a
    // bug detector) is checked once per chunk.
    const uint8_t *const sb = reinterpret_cast<const uint8_t *>(fgk.T.syms);
    uint8_t *const sb_w = reinterpret_cast<uint8_t *>(fgk.T.syms);
    // sym and its where[] word whw, both wave-uniform (a batch step hands over its own reads)
    auto miss_at = [&](uint32_t sym, uint32_t whw) {
        uint32_t s = whw & 1023u;
        const uint32_t fresh = s == 0;
        if (fresh) s = uni(fgk.split(sym));
        uint32_t pv;
        uint32_t d;
        {
            HC_PROF_BEGIN();
            d = fgk.chase(s, pv);
            HC_PROF_END(5);
        }
        // bit k = code bit (position parity, left = even) of level k; read MSB first it is the
        // root-to-leaf code (the kRoot lanes are even)
        const uint64_t bits = ballot(pv & 1u);
        if (d <= kInsertDepth) fgk.pc_insert(sym, s, pv, d, (1u << d) | (uint32_t)bits);
        {
            HC_PROF_BEGIN();
            // a path too deep to cache belongs to a rare symbol, whose leaf nearly always ties
            // with the next position (9 in 10 on the slot-form model): walk from the leaf at once
            if (d > kInsertDepth) {
                fgk.pc_bound();
                fgk.walk(s, pv, true);
            }
            else fgk.update_path(pv);
            HC_PROF_END(6);
        }
        if (fresh) {
            // the path starts at the new leaf, one level below the NYT whose code is sent
            // (huffman.cpp:44-50): drop that lowest bit, then 8 raw bits
            sink.push_bits(bits >> 1, d - 1);
            sink.push((1u << 8) | sym);
        } else {
            sink.push_bits(bits, d);
        }
    };
    auto miss = [&](uint32_t sv) {
        const uint32_t sym = uni(sv);
        miss_at(sym, uni(fgk.T.where[sym]));
    };
    // code symbols syms[0..ns) of the LDS buffer. The hot loop carries only vt, the records, the
    // cache's reference bits and its read pipeline: a miss or a failed leader test leaves it
    // (what = 1 / 2) and is finished outside, so the compiler adds no copies of the rare paths'
    // state per symbol. Pipeline: while symbol t updates, the cache row of t+1, the where[]
    // entry of t+2 and the byte of t+3 are already in flight. where[] and the rows change only
    // on the paths that leave the loop (split, insert, swap), so what was read ahead stays
    // valid inside it; the loop is re-primed after every exit. Bytes past ns are older symbols
    // of the same buffer: their reads are harmless.
    auto code_all = [&](uint32_t ns) __attribute__((always_inline)) {
        uint32_t t = 0;
        while (t < ns) {
            uint32_t rl = sink.n;  // record lane of symbol t (scalar)
            const uint32_t rend = min(64u, rl + (ns - t));
            uint32_t vt = vreg(t);
            uint32_t ws0 = vreg(fgk.T.where[sb[vt]]);      // where[] entry of symbol t
            uint32_t ws1 = vreg(fgk.T.where[sb[vt + 1]]);  // ... of t+1
            uint32_t e0 = ws0 >> 10;
            uint32_t pr0 = vreg(fgk.pc_lane[e0 * kRow]);   // cache row of t (pc_miss if none)
            uint32_t sv2 = vreg(sb[vt + 2]);               // byte of t+2
            // LDS address of the byte of t+3, in a VGPR (one add per symbol, no base add)
            const lds_u8 *vb = (const lds_u8 *)sb + t + 3;
            asm("" : "+v"(vb));
            uint32_t pv, k;
            // loop while no level failed (k = 0xFFFFFFFF) and record lanes are left (left < 0):
            // both sign bits set, one scalar AND
            int32_t left = (int32_t)(rl - rend);
            do {
                const uint32_t rec = fgk.pc_use(e0, pr0, pv);
                k = fgk.update_fast(pv, [&] {
                    // (v_bfe + v_lshl_add; left alone the compiler emits shift, and, add)
                    const uint32_t pr1 = fgk.pc_lane[opaque(__builtin_amdgcn_ubfe(ws1, 10, 6)) * kRow];
                    const uint32_t ws2 = fgk.T.where[sv2];
                    const uint32_t sv3 = *vb;
                    pr0 = pr1;
                    ws1 = ws2;
                    sv2 = sv3;
                });
                sink.vrec = writelane(sink.vrec, rec, (uint32_t)((int32_t)rend + left));
                ++vb;
                ++left;
            } while ((int32_t)(k & (uint32_t)left) < 0);
            rl = (uint32_t)((int32_t)rend + left);
            t += rl - sink.n;
            if (k != 0xFFFFFFFFu) {
                // not cached (the miss row's sentinel at level 0): nothing was written; code it
                // from scratch
                if (lane_read(pv, 0) == kMissPos) {
                    --t;
                    sink.n = rl - 1;  // its record lane, overwritten by the miss path
                    HC_PROF_BEGIN();
                    miss(sb[t]);
                    HC_PROF_END(1);
                    ++t;
                    continue;
                }
                HC_PROF_BEGIN();
                fgk.walk(lane_read(pv, k), pv);
                HC_PROF_END(2);
            }
            sink.n = rl;
            if (rl == 64) {
#ifndef HC_PROF_PASS
                HC_PROF_BEGIN();
                sink.pack();
                HC_PROF_END(3);
#else
                sink.pack();
#endif
            }
        }
    };

    // Batched hot path (path-cache mode, narrow and wide layouts, HC_ENC_BATCH; model:
    // tests/fgk_batch_model.py, test tests/test_batch_model.py).
    // Between swaps and splits the tree's shape is fixed and an update only adds 1 to the
    // weights on the symbol's root path, so the updates of consecutive cached symbols commute.
    // Up to HC_ENC_PACK (16) symbols at a time, packed by path depth as the decoder packs codes by
    // bit offset (Dec::decode_batch; model: tests/fgk_encpack_model.py): symbol j's d_j path
    // positions (levels 0 .. d_j - 1 of its cached row) take lanes S_j .. S_j + d_j - 1, S_j the
    // depths of the symbols before it; no lane pads a short path, lane 63 is the root. The step:
    //  0. lane j (of every row of 16 lanes) reads symbol t + j's byte, its where[] word and word
    //     12 of its row, the finished code record 1 << d_j | code bits: the top bit's index is the
    //     depth (the miss row's record is 1: depth 0; measured and dropped: the depths as sixteen
    //     nibbles in scalar registers, kept beside pc_insert, which takes the record's read off the
    //     step's chain of dependent LDS round trips: C5 encode 320.5 ms against 318.1), four row-DPP
    //     adds give the starts, and the
    //     step takes the symbols before the first of: the cap, the pass's end, a symbol without a
    //     row, a symbol whose last lane would pass lane 62. A mark sent to every start lane
    //     (ds_permute) and one ballot give each lane its symbol, one ds_bpermute of that symbol's
    //     row address less its start the word to read: the lane's path position;
    //  1. every path position of every symbol taken gets its increment (one LDS add: +1024 to the
    //     narrow weight word, +1 to a wide weight, the root once per symbol by lane 63), the words
    //     of the next positions having been read before;
    //  2. a level fails when that next word is below the position's word after the adds -- the
    //     one-symbol loop's update_fast test with every step symbol through the position counted
    //     as earlier and none through the next one, so it reports levels falsely at worst (the
    //     exact counts, from membership bits ORed into the body words, measured 394 ms on C5
    //     where the tentative test took 371);
    //  3. the first symbol with a failed level ends the step: its increments and those after it
    //     are taken back; so does a symbol without a cached row, which never got lanes. Record
    //     lane sink.n + q takes symbol q's record as lane q read it (one ds_bpermute), for the
    //     symbols before that one, and it is coded alone (miss / update_path: walk), its byte and
    //     where[] word taken from lane j of the step's reads (`alone` below).
    // Measured against the layout before it, seven symbols in groups of nine lanes with root
    // padding above each path (photo -c -m: six lanes in ten padding, 57 % of the steps ending at
    // the cap of seven) and the records rebuilt from ballots of the positions' parities: DESIGN.md
    // section 0, round 9.
    // Small alphabets (narrow layout, while at most 16 symbols are seen, so every position is >=
    // 480; model: tests/fgk_batch_model.py small_len, encode(small=True)). A run-heavy stream with a
    // few symbols (grad -c -m: 1, 3, 250, 255) ties on every row, and the tentative test below
    // counts no earlier batch symbol through the next position: it ends a batch every ~4 symbols
    // (1034 batches and 523 symbols alone per 512x512 stream). Here the counts are exact and the
    // paths short, so up to 15 symbols go per step, four lanes each (levels 0..3: depth <= 4;
    // lane 63 holds the root): every path position ORs its symbol's bit into a membership mark
    // (smark, 2 positions per word), and symbol j's test at position a reads the pre-batch words
    // of a and a + 1 and the marks of both: with c0 / c1 the earlier symbols through a / a + 1
    // (c1 = j at the root: every symbol passes it) the level passes iff weight(a + 1) + c1 >=
    // weight(a) + c0 + 1 -- the one-symbol loop's leader test on the tree as the earlier symbols
    // leave it. The first symbol with a failing level (or no cached path, or a path deeper than
    // four) ends the step: the ones before it commit with one add, it is coded alone. grad:
    // 319 steps and 13 symbols alone per stream. Returns where the regular batches take over.
    constexpr uint32_t kSG = kSmallG, kSK = kSmallK;
    constexpr uint32_t kPack = HC_ENC_PACK, kNone = 0xFFFFFFFFu;
    static_assert(kInsertDepth <= 63 && kSlotDepth < kRow, "a cached path fits a step's lanes; word 12 is the record");
    constexpr uint32_t kIncU = kW ? 1u : 1024u;
    auto code_all_batch = [&](uint32_t ns) __attribute__((always_inline)) {
        const uint32_t pcb = lds_off16(&fgk.T.pc[0]) - 2 * kRow;  // + 32 e: row e - 1 (e = 0: pc_miss)
        const uint32_t wtb = lds_off(&fgk.T.wt[0]);
        const uint32_t whb = lds_off16(&fgk.T.where[0]);
        const uint32_t scb = lds_off(fgk.scr32());
        constexpr uint64_t kL63 = 1ull << 63;
        uint32_t t = 0;
#if HC_ENC_MISS_RUN
        uint32_t stepmm = 0;  // the last step's mm: bit j: symbol j had no row when the step read it
#endif
        // One regular step from symbol t on (the comment above). Returns the index in the step of
        // the symbol that ended it and is to be coded alone (kNone: the cap, the lanes or the pass
        // ended it), with t and sink.n moved past the symbols before it; sv, wh: lane j holds the
        // byte and the where[] word of symbol j; lv: the level reported (HC_ENC_HANDOFF_LEVEL).
        auto step = [&](uint32_t &sv, uint32_t &wh, uint32_t &lv) __attribute__((always_inline)) -> uint32_t {
            if (sink.n > 64 - kPack) sink.pack();
            HC_CNT(1);
            const uint32_t lim = enc_pack_max(min(kPack, ns - t));  // 1..16
            // 0. lane j of every row: symbol t + j (bytes past ns are older symbols of the buffer
            // or the tree's words behind it: any byte names a where[] word)
            const uint32_t ln = vreg(lane);  // (opaque: the lane's constants are made here, not kept from the kernel's entry)
            sv = opaque(*(const lds_u8 *)(size_t)((uint32_t)(size_t)(const lds_u8 *)sb + t + (ln & 15u)));
            wh = opaque(*(const lds_u16 *)(size_t)(whb + 2 * sv));
            const uint32_t ra = pcb + ((wh >> 10) << 5);
            const uint32_t rec = opaque(*(const lds_u16 *)(size_t)(ra + 2 * kSlotDepth));
            const uint32_t d = 31u - (uint32_t)__builtin_clz(rec);  // (a row in use holds a record >= 2, the miss row 1)
            uint32_t inc = d;  // the depths up to and with symbol j's
            inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x111, 0xF, 0xF, true);
            inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x112, 0xF, 0xF, true);
            inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x114, 0xF, 0xF, true);
            inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x118, 0xF, 0xF, true);
            // the symbols without a row, within the cap and the pass; the first symbol not taken
            const uint32_t mm = (uint32_t)ballot(wh < 1024u) & ((1u << lim) - 1u);
            const uint32_t jmax = (uint32_t)__builtin_ctz(mm | (uint32_t)ballot(inc > 63u) | (1u << lim));
#if HC_ENC_MISS_RUN
            stepmm = mm;
#endif
            lv = 0;
            if (jmax == 0) return 0;  // (a cached path is at most kInsertDepth lanes: the first symbol has no row)
            const uint32_t se = lane_read(inc, jmax - 1);  // the lanes of the symbols taken, <= 63
            const uint32_t exc = inc - d;                  // symbol j's first lane
            // lane j < jmax sends a mark to symbol j's first lane (the other lanes to lane 63, whose
            // bit is not used); the lane's symbol: the starts in lanes 1..lane
            const uint32_t to = sel(below_mask(jmax), exc << 2, 63u << 2);
            const uint64_t sm = ballot(__builtin_amdgcn_ds_permute((int)to, 1) != 0);
            const uint32_t jv = __builtin_amdgcn_mbcnt_hi((uint32_t)(sm >> 33), __builtin_amdgcn_mbcnt_lo((uint32_t)(sm >> 1), 0u));
            // the lane's level l = lane - S_j of its symbol's row: the word at row + 2 l
            const uint32_t rl = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(jv << 2), (int)(ra - 2 * exc));
            const uint64_t act = below_mask(se);  // the lanes of the symbols taken
            uint32_t pos = opaque(*(const lds_u16 *)(size_t)(rl + 2 * ln));
            pos = sel(act, pos, kRoot);  // lane 63 and the idle lanes hold the root; lane 63 adds one increment per symbol
            const uint32_t wa = wtb + 4 * pos;
            // 1. tentative increments (each path position once, the root once per symbol)
            const uint32_t w1 = *(const lds_u32 *)(size_t)(wa + 4);
            __hip_atomic_fetch_add((uint32_t *)(lds_u32 *)(size_t)sel(act | kL63, wa, scb), sel(kL63, jmax * kIncU, kIncU),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            const uint32_t wn = *(const lds_u32 *)(size_t)wa;
            // 2. the tests; 3. the increments from the first failing symbol on taken back
            const uint64_t fm = ballot(w1 < wn) & act;
            uint32_t jf = jmax;
            if (fm) {
                const uint32_t fl = ff1(fm);
                jf = lane_read(jv, fl);  // the failing lane's symbol
                const uint32_t sj = lane_read(exc, jf);
                lv = fl - sj;
                // (HC_ENC_HANDOFF_LEVEL: symbol jf's levels below the reported one stay committed)
                const uint64_t back = (act & (~0ull << (HC_ENC_HANDOFF_LEVEL ? fl : sj))) | kL63;
                __hip_atomic_fetch_add((uint32_t *)(lds_u32 *)(size_t)sel(back, wa, scb), sel(kL63, (jf - jmax) * kIncU, 0u - kIncU),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
            // record lane sink.n + q takes symbol q's record, which lane q read
            const uint32_t q = ln - sink.n;
            const uint32_t r = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(q << 2), (int)rec);
            sink.vrec = q < jf ? r : sink.vrec;
            __builtin_amdgcn_wave_barrier();
            sink.n += jf;
            t += jf;
            // symbol jf: a level reported, or (none reported: jf = jmax) not cached
            return fm || ((mm >> jf) & 1u) ? jf : kNone;
        };
        // The symbol syms[t] that ended a batch step (record lane sink.n), coded alone. stepd
        // (wave-uniform): the step was a regular one, which hands over what its lanes hold: ja =
        // the symbol's index in the step, lv its reported level (if one was); sv, wh the step's
        // bytes and where[] words.
        //  * Lane ja of sv and wh gives the symbol's byte and where[] word, with them whether it is
        //    cached and which row is its own, instead of three dependent reads of syms[t] and
        //    where[] (HC_ENC_HANDOFF_MISS).
        //  * A cached symbol's levels below the report have kept their increments: they passed a
        //    test that passes no level that fails. The walk starts at the reported level, where it
        //    repeats the exact test (the report may be false); no level is tested or stored a
        //    second time (HC_ENC_HANDOFF_LEVEL, off: see its definition). One read of the row gives the known path and the
        //    record (the step's positions kept for them, one ds_bpermute and two ballots, cost the
        //    small-alphabet kernel of the symbol source two VGPRs).
        // Otherwise (a small-alphabet step, or a part compiled out) the symbol is looked up and
        // every level tested again. One call site per kernel: the miss path stays inlined once.
        auto alone = [&](bool stepd, uint32_t ja, uint32_t lv, uint32_t sv, uint32_t wh) __attribute__((always_inline)) {
            const bool hm = HC_ENC_HANDOFF_MISS && stepd, hl = HC_ENC_HANDOFF_LEVEL && stepd;
            uint32_t sym, whw;
            if (hm) {
                sym = lane_read(sv, ja);
                whw = lane_read(wh, ja);
            } else {
                if (sink.n == 64) sink.pack();
                sym = uni(sb[t]);
                whw = uni(fgk.T.where[sym]);
            }
            const uint32_t ent = whw >> 10;
            if (ent == 0) {
                HC_PROF_BEGIN();
                miss_at(sym, hm ? whw : uni(fgk.T.where[sym]));
                HC_PROF_END(1);
            } else {
                HC_PROF_BEGIN();
                uint32_t pv;
                const uint32_t rc = fgk.pc_use(ent, fgk.pc_lane[ent * kRow], pv);
                sink.push(rc);
                // (update_path, with the reported level handed over)
                const uint32_t k = hl ? lv : fgk.update_fast(pv, [] {});
                if (k != 0xFFFFFFFFu) fgk.walk(lane_read(pv, k), pv);
                HC_PROF_END(2);
            }
        };
        // small-alphabet steps (above) while the stream has seen <= 16 symbols; re-checked only
        // after a symbol coded alone (splits happen there), so a regular step pays nothing for it
        if constexpr (!kSmall) {
#if HC_ENC_MISS_RUN
            // (the path-cache kernel: one regular batch step per pass of this loop; behind the
            // symbol coded alone, those the step read as uncached too are coded alone at once --
            // a step from there would take nothing (jmax == 0) after three dependent LDS round
            // trips. Only the count crosses the miss path; the run's symbols are looked up afresh,
            // which is right whatever became of them meanwhile (one equal to a symbol just
            // inserted is cached by now). mm ends at the step's cap and the pass's end, so does
            // the run. One call site: the miss path stays inlined once. sink.n < 64 throughout:
            // the step leaves room for the symbol that ends it, and push() packs at 64. Model:
            // tests/fgk_missrun_model.py.)
            static_assert(HC_ENC_HANDOFF_MISS && !HC_ENC_HANDOFF_LEVEL, "the run takes the step's hand-off of the byte and the where[] word only");
            while (t < ns) {
                uint32_t sv, wh, lv;
                const uint32_t ja = step(sv, wh, lv);
                if (ja != kNone) {  // symbol t: not cached, or a level reported: alone
                    uint32_t sym = lane_read(sv, ja), whw = lane_read(wh, ja);
                    uint32_t run = min((uint32_t)__builtin_ctz(~(stepmm >> (ja + 1))), (uint32_t)HC_ENC_MISS_RUN_MAX);
                    for (;;) {
                        HC_CNT(2);
                        const uint32_t ent = whw >> 10;
                        if (ent == 0) {
                            HC_PROF_BEGIN();
                            miss_at(sym, whw);
                            HC_PROF_END(1);
                        } else {
                            HC_PROF_BEGIN();
                            uint32_t pv;
                            const uint32_t rc = fgk.pc_use(ent, fgk.pc_lane[ent * kRow], pv);
                            sink.push(rc);
                            const uint32_t k = fgk.update_fast(pv, [] {});
                            if (k != 0xFFFFFFFFu) fgk.walk(lane_read(pv, k), pv);
                            HC_PROF_END(2);
                        }
                        ++t;
                        if (run == 0) break;
                        --run;
                        sym = uni(sb[t]);
                        whw = uni(fgk.T.where[sym]);
                    }
                }
            }
#else
            // (the path-cache kernel: one regular batch step per pass of this loop)
            while (t < ns) {
                uint32_t sv, wh, lv;
                const uint32_t ja = step(sv, wh, lv);
                if (ja != kNone) {  // symbol t: not cached, or a level reported: alone
                    HC_CNT(2);
                    alone(true, ja, lv, sv, wh);
                    ++t;
                }
            }
#endif
        } else {
            bool small = fgk.nyt >= kSmallNyt;
            while (t < ns) {
                uint32_t ja = kNone;
                uint32_t lv = 0, sv = 0, wh = 0;  // of a regular step, for the symbol that ends it
                if (small) {
                    uint32_t jf, jmax;
                    // (the lane index opaque: these per-lane values are made here, not hoisted to the
                    // kernel's entry beside the regular step's)
                    const uint32_t ln = vreg(lane);
                    const uint32_t g = ln < kSK * kSG ? ln >> 2 : kSK;  // the lane's symbol (kSK: idle)
                    const uint32_t srow = lds_off16(&fgk.T.pc[0]) + 2 * (ln & 3u) - 2 * kRow;
                    const uint32_t ssv = (uint32_t)(size_t)(const lds_u8 *)sb + (g < kSK ? g : 0u);
                    const uint32_t sscb = lds_off(&fgk.T.scratch[0]) + 4 * ln;
                    const uint32_t mkb = lds_off(&fgk.T.smark[0]);
                    // the cached path of the step's symbols: symbol byte -> where[] -> row (level
                    // 4 too, for the depth test). (Measured: read one step ahead, for the step
                    // that follows if this one takes all its symbols -- rows and where[] change
                    // only on the alone path -- grad encode 1.28 -> 1.33 ms.)
                    auto row_read = [&](uint32_t t0, uint32_t &p4v) __attribute__((always_inline)) {
                        const uint32_t sv = opaque(*(const lds_u8 *)(size_t)(ssv + t0));
                        const uint32_t wh = opaque(*(const lds_u16 *)(size_t)(whb + 2 * sv));
                        const uint32_t ra = srow + 32 * (wh >> 10);
                        p4v = opaque(*(const lds_u16 *)(size_t)(ra + 8));  // lane l = 0: level 4
                        return opaque(*(const lds_u16 *)(size_t)ra);
                    };
                    do {
                        if (sink.n > 64 - kSK) sink.pack();
                        HC_CNT(1);
                        jmax = min(kSK, ns - t);
                        uint32_t p4, pos = row_read(t, p4);
                        pos = sel(~0ull << (kSK * kSG), kRoot, pos);
                        const uint32_t wa = wtb + 4 * pos;
                        const uint64_t gm = below_mask(kSG * jmax);
                        const uint64_t am = ballot(pos < kRoot) & gm;
                        // no cached path, or one deeper than four: the step ends there
                        const uint64_t em = (ballot(pos == kMissPos) | ballot((ln & 3u) == 0 && p4 != kRoot)) & gm;
                        const uint32_t w0 = *(const lds_u32 *)(size_t)wa, w1 = *(const lds_u32 *)(size_t)(wa + 4);
                        const uint32_t ma = pos - kSmallNyt, odd = ma & 1u;  // (pos >= 480 on the am lanes)
                        const uint32_t mda = sel(am, mkb + 4 * (ma >> 1), sscb);
                        __hip_atomic_fetch_or((uint32_t *)(lds_u32 *)(size_t)mda, (1u << g) << (odd << 4),
                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        // the marks of a (half `odd` of its word) and a + 1 (the other half, or the next word)
                        const uint32_t mlo = *(const lds_u32 *)(size_t)mda;
                        const uint32_t mhi = *(const lds_u32 *)(size_t)(mda + 4 * odd);
                        const uint32_t c0 = (uint32_t)__builtin_popcount(__builtin_amdgcn_ubfe(mlo, odd << 4, g));
                        const uint32_t c1 = pos + 1 == kRoot ? g
                                                             : (uint32_t)__builtin_popcount(__builtin_amdgcn_ubfe(odd ? mhi : mlo, (odd ^ 1u) << 4, g));
                        const uint64_t fm = (ballot((w1 >> 10) + c1 < (w0 >> 10) + c0 + 1) & am) | em;
                        jf = min(ff1(fm) >> 2, jmax);
                        // symbols < jf commit (+1 per path position and symbol, the root once each: lane
                        // 63); the marks are cleared
                        __hip_atomic_fetch_add((uint32_t *)(lds_u32 *)(size_t)sel((am & below_mask(kSG * jf)) | kL63, wa, sscb),
                                               sel(kL63, jf << 10, 1u << 10), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        *(lds_u32 *)(size_t)mda = 0u;
                        // code records (as below): record lane sink.n + q takes symbol q's
                        const uint32_t q = ln - sink.n;
                        const uint64_t par = ballot(pos & 1u), rtm = ballot(pos == kRoot);
                        const uint32_t gb = kSG * q;
                        const uint32_t d = (uint32_t)__builtin_ctz((uint32_t)(rtm >> gb) | (1u << kSG));
                        const uint32_t r = __builtin_amdgcn_ubfe((uint32_t)(par >> gb), 0, d) | (1u << d);
                        sink.vrec = q < jf ? r : sink.vrec;
                        __builtin_amdgcn_wave_barrier();
                        sink.n += jf;
                        t += jf;
                    } while (jf == jmax && t < ns);
                    if (jf < jmax) ja = 0;  // (the symbol is looked up again)
                } else {
                    do ja = step(sv, wh, lv);
                    while (ja == kNone && t < ns);
                }
                if (ja != kNone) {  // symbol t: not cached, or a level reported (small: deeper than 4): alone
                    HC_CNT(2);
                    alone(!small, ja, lv, sv, wh);
                    ++t;
                    small = kSmall && fgk.nyt >= kSmallNyt;
                }
            }
        }
    };

    // Table mode (kTab): no path cache. The decoder's level tables (levels 1..8, prefix ->
    // where the walk from the root stops) and pcode[] (position -> the code the tables reached
    // it by) give a symbol's code and whole root path from three reads: where[] -> pcode[] ->
    // one lane-parallel read of the tables (lane k: level 8 - k), exactly the decoder's path
    // read. The level-8 entry read back must name the symbol's own position at the pcode depth;
    // otherwise (deeper than 8, or not in the tables since a split) the symbol is coded from
    // scratch like a cache miss. A symbol's reads go out up to three symbols ahead (where[],
    // pcode[] and the tables change only on the paths that leave the loop).
    const uint32_t psh = lane < 8 ? lane : 8u;
    const uint32_t pbase = lds_off16(&fgk.T.lvl[0]) + 2 * (lane < 8 ? (256u >> lane) - 2 : 0xFFFFFFFEu);
    auto path_read = [&](uint32_t pcw) __attribute__((always_inline)) {
        return opaque(*(const lds_u16 *)(size_t)(pbase + ((pcw & 255u) >> psh) * 2));
    };
    // the root path of position s0 (lane k: level k, kRoot above): climb parent links until a
    // position that pcode[] puts at depth 8 and the tables confirm; the tables give the other 8
    // levels in one read (a 10-bit code: 2 climbs instead of 10). Returns the depth.
    auto chase_tab = [&](uint32_t s0, uint32_t &pv) __attribute__((always_inline)) -> uint32_t {
        uint32_t s = s0, n = 0, td = kRoot;  // td lane j: level n - 1 - j
        for (;;) {
            const uint32_t pc = uni(fgk.T.pcode[s]);
            const uint32_t par = fgk.parent(s);
            if (((pc >> 8) & 7u) == 7u) {
                const uint32_t pr = path_read(pc);
                if (uni(pr) == (s | (8u << 10))) {
                    const uint32_t dn = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((n - 1 - lane) & 63u) * 4), (int)td);
                    const uint32_t tb = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((lane - n) & 63u) * 4), (int)pr);
                    pv = lane < n ? dn : (lane - n < 9 ? (tb & 1023u) : kRoot);
                    return n + 8;
                }
            }
            const uint32_t sh = __builtin_amdgcn_update_dpp(0u, td, 0x138, 0xF, 0xF, true);
            td = lane == 0 ? s : sh;
            ++n;
            if (par == kRoot || n >= 63) {  // the root, or (a bug) a cycle
                fgk.bad |= par ^ kRoot;
                const uint32_t dn = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((n - 1 - lane) & 63u) * 4), (int)td);
                pv = lane < n ? dn : kRoot;
                return n;
            }
            s = par;
        }
    };
    auto miss_tab = [&](uint32_t sv) {
        const uint32_t sym = uni(sv);
        uint32_t s = uni(fgk.T.where[sym]) & 1023u;
        const uint32_t fresh = s == 0;
        if (fresh) s = uni(fgk.split(sym));
        uint32_t pv;
        uint32_t d;
        {
            HC_PROF_BEGIN();
            d = chase_tab(s, pv);
            HC_PROF_END(6);
        }
        const uint64_t bits = ballot(pv & 1u);
        if (!fresh && d <= 8) {  // the tables are short of it (a split since the last build)
            if (++fgk.stale >= kRefresh) fgk.from = 0;
        }
        HC_PROF_BEGIN();
        if (d > kInsertDepth) fgk.walk(s, pv);
        else fgk.update_path(pv);
        HC_PROF_END(7);
        if (fresh) {
            sink.push_bits(bits >> 1, d - 1);
            sink.push((1u << 8) | sym);
        } else {
            sink.push_bits(bits, d);
        }
    };
    auto code_all_tab = [&](uint32_t ns) __attribute__((always_inline)) {
        uint32_t t = 0;
        while (t < ns) {
            if (fgk.from < 9) {
                HC_PROF_BEGIN();
                fgk.build_levels();
                HC_PROF_END(5);
            }
            uint32_t rl = sink.n;
            const uint32_t rend = min(64u, rl + (ns - t));
            const uint32_t x1 = vreg(fgk.T.where[sb[t + 1]]);
            const uint32_t x0 = vreg(fgk.T.where[sb[t]]);
            uint32_t pc0 = vreg(fgk.T.pcode[x0 & 1023u]);   // pcode of t
            uint32_t pr = path_read(pc0);                      // path of t
            uint32_t x0u = x0;
            uint32_t pc1 = vreg(fgk.T.pcode[x1 & 1023u]);   // pcode of t+1
            uint32_t x1u = x1;
            uint32_t x2 = vreg(fgk.T.where[sb[t + 2]]);      // where[] of t+2
            uint32_t sv3 = vreg(sb[t + 3]);                    // byte of t+3
            const lds_u8 *vb = (const lds_u8 *)sb + t + 4;
            asm("" : "+v"(vb));
            uint32_t pv, k, ok;
            int32_t left = (int32_t)(rl - rend);
            do {
                const uint32_t pcu = uni(pc0);
                const uint32_t d = ((pcu >> 8) & 7u) + 1;
                ok = uni(pr) == ((uni(x0u) & 1023u) | (d << 10));
                const uint32_t rec = (1u << d) | ((pcu & 255u) >> (8 - d));
                pv = pr & 1023u;
                uint32_t prn;
                k = fgk.update_fast(pv, [&] {
                    prn = path_read(pc1);
                    const uint32_t pc2 = fgk.T.pcode[x2 & 1023u];
                    const uint32_t x3 = fgk.T.where[sv3];
                    const uint32_t sv4 = *vb;
                    x0u = x1u;
                    x1u = x2;
                    pc0 = pc1;
                    pc1 = pc2;
                    x2 = x3;
                    sv3 = sv4;
                }, ok ? 0u : 0xFFFFFFFFu);
                pr = prn;
                sink.vrec = writelane(sink.vrec, rec, (uint32_t)((int32_t)rend + left));
                ++vb;
                ++left;
            } while ((int32_t)(k & (uint32_t)left) < 0);
            rl = (uint32_t)((int32_t)rend + left);
            t += rl - sink.n;
            if (k != 0xFFFFFFFFu) {
                if (!ok) {  // not in the tables: nothing was stored; code it from scratch
                    --t;
                    sink.n = rl - 1;  // its record lane, overwritten by the miss path
                    HC_PROF_BEGIN();
                    miss_tab(sb[t]);
                    HC_PROF_END(1);
                    ++t;
                    continue;
                }
                HC_PROF_BEGIN();
                fgk.walk(lane_read(pv, k), pv);
                HC_PROF_END(2);
            }
            sink.n = rl;
            if (rl == 64) {
#ifndef HC_PROF_PASS
                HC_PROF_BEGIN();
                sink.pack();
                HC_PROF_END(3);
#else
                sink.pack();
#endif
            }
        }
    };

    uint64_t nsym = 0;
    uint32_t next = buf_load(rin, lane * 4);
    RleCarry cy = {0, 0, 0};
    // Two copies of the chunk loop: streams that fit one window (every batch stream) run without
    // the window bookkeeping, which would otherwise sit in scalar registers across the hot loop,
    // and let the MNP-5 symbols of many chunks gather in syms[] before the FGK loop codes them (a
    // run-heavy stream yields a few symbols per chunk: one coding pass per buffer instead of per
    // chunk; grad -c -m encode 3.77 -> 2.89 ms, photo unchanged).
    auto chunks = [&](auto windowed) __attribute__((always_inline)) {
        constexpr bool kWin = decltype(windowed)::value;
        Prio<uint32_t> prio;
        uint32_t np = 0;       // symbols pending in syms[]
        uint32_t chunk = 0;
        bool redo = false;     // the chunk did not fit the pending symbols: again, after coding them
        // Run-heavy stretches (a 256-byte chunk whose run starts sit in at most kSparseEnter
        // lanes) switch to blocks of kQ KB coded by segments (rle_block; tests/rle_chunk_model.py:
        // rle_blocked) while the blocks stay sparse and a whole block of full chunks remains before
        // the last one; blk holds the block at ci (kQ 16-byte loads per lane, the next block in
        // flight).
        constexpr bool kSparseOn = HC_SPARSE && !kWin && kSrc != SRC_SYMBOLS && !kTab;
        constexpr uint32_t kSparseEnter = 2;
        constexpr uint32_t kQ = HC_SPARSE_KB, kBC = 4 * kQ;  // KB and 256-byte chunks per block
        bool sparse = false;
        u32x4 blk[kQ] = {};
        auto load_blk = [&](uint32_t c0) __attribute__((always_inline)) {
#pragma unroll
            for (uint32_t i = 0; i < kQ; ++i) blk[i] = buf_load4(rin, 256 * c0 + 16 * (kQ * lane + i));
        };
        for (uint32_t ci = 0;;) {
            const bool more = ci < nch && !fgk.bad;
            uint32_t full = 0;
            if (kSparseOn && more && sparse) {
                if (np + 63 > kSymWords * 4) {
                    full = 1;  // room for a block's symbols first
                } else {
                    prio.at(ci, nch);
                    HC_PROF_BEGIN();
                    const uint32_t r = rle_block<kSrc, kQ>(blk, cy, sb_w, np, fgk.T.scratch, lane);
                    HC_PROF_END(4);
                    if (r != kDense) {
                        np = r;
                        ci += kBC;
                        full = np + 63 > kSymWords * 4 ? 1u : 0u;
                    }
                    if (r != kDense && ci + kBC < nch) {
                        load_blk(ci);
                    } else {  // a dense block or the last chunks: 256-byte chunks from ci
                        sparse = false;
                        next = buf_load(rin, 256 * ci + lane * 4);
                        ioff = 256 * ci + 256;
                    }
                }
            } else if (more) {
                const uint32_t m = ci + 1 < nch ? 256u : (uint32_t)(n - 256ull * ci);
                if (!redo) {
                    prio.at(ci, nch);
                    chunk = next;
                    if constexpr (kWin) {
                        if (ioff >= window) {  // slide the input window up to the next chunk
                            const uint64_t at = 256ull * (ci + 1);
                            rin = make_rsrc(bt.in + uni64(bt.in_offs[sid]) + at,
                                            (uint32_t)min((n - min(n, at) + 3u) & ~3ull, (uint64_t)kMaxBufBytes));
                            ioff = 0;
                        }
                        if ((sink.wout - sink.wbase) * 4ull >= window) sink.rebase(bt.out + out_off, cap);
                        next = buf_load(rin, ioff + lane * 4);  // out of range past the end: reads 0
                    } else {
                        next = buf_load(rin, ioff + lane * 4);
                    }
                    ioff += 256;
                }
                if (kSrc == SRC_SYMBOLS) {  // a ready symbol stream (adaptive path)
                    fgk.T.syms[lane] = chunk;
                    __builtin_amdgcn_wave_barrier();
                    np = m;
                    full = 1;  // coded at once
                } else {
                    // transform.cpp:220-229 (diff) + 241-279 (MNP-5 RLE), lane-parallel; symbols
                    // gather in syms[] (windowed streams: coded per chunk)
                    HC_PROF_BEGIN();
                    const uint32_t np0 = np;
                    uint32_t slanes = 64;
                    np = rle_chunk<kSrc>(chunk, m, ci + 1 == nch ? 1u : 0u, cy, sb_w, np, kWin ? 342u : kSymWords * 4,
                                         fgk.scr32(), lane, full, slanes);
                    HC_PROF_END(4);
                    if (kSparseOn && !full && slanes <= kSparseEnter && ci + 1 + kBC < nch) {
                        sparse = true;  // the block at ci + 1 (the chunk loaded ahead is dropped)
                        load_blk(ci + 1);
                    }
                    if (kWin) {
                        full = !full;  // code this chunk's symbols now (the chunk itself always fits)
                        redo = false;
                    } else {
                        redo = full != 0;
                        // code them now, too, when a next chunk like this one would not fit (a
                        // photo's chunk fills half the buffer: no chunk runs twice)
                        full |= np + (np - np0) > kSymWords * 4 ? 1u : 0u;
                    }
                }
                if (!redo) ++ci;
            }
            if (full || (!more && np)) {  // the serial FGK pass over the pending symbols
                if constexpr (kTab) code_all_tab(np);
                else if constexpr (kW <= 1 && HC_ENC_BATCH) {
#ifdef HC_PROF_PASS  // (diagnostic: region 3 times the whole batch pass instead of the record packing)
                    HC_PROF_BEGIN();
                    code_all_batch(np);
                    HC_PROF_END(3);
#else
                    code_all_batch(np);
#endif
                }
                else code_all(np);
                nsym += np;
                np = 0;
            }
            if (!more) break;
        }
    };
    if (n + 512 <= window && cap <= window) chunks(std::false_type{});
    else chunks(std::true_type{});

    const uint64_t total = sink.finish();
    const uint32_t st = fgk.bad ? (uint32_t)HC_ERR_DEVICE : (total <= cap ? 0u : (uint32_t)HC_ERR_CAPACITY);
    // headers.cpp:110-116: u64 little-endian symbol count in words 0-1 (stored after every
    // payload word by program order)
    buf_store(make_rsrc(bt.out + out_off, (uint32_t)min(cap, (uint64_t)8)), lane < 2 ? lane * 4 : kDrop,
              lane ? (uint32_t)(nsym >> 32) : (uint32_t)nsym);
    if (lane == 0) {
        bt.out_lens[sid] = fgk.bad ? 0 : total;
        bt.status[sid] = (int32_t)st;
    }
    trace_wave(sid, t0, lane);
    prof_store(sid, t0, pacc + fgk.pacc, lane);
}

// --------------------------------------------------------------------------- the decoder --

// MSB-first reader over a stream's bytes; words come from a 64-word VGPR chunk, the next chunk
// already loading (its wait falls ~64 refills later).
struct BitSource {
    rsrc_t rs;       // window of the stream at byte ibase
    uint64_t ibase;
    uint32_t lane;
    uint32_t cbase;  // byte offset of chunk lane 0 in the window
    uint32_t chunk;  // big-endian words (byte-swapped once per load, on the lanes)
    uint32_t nxt;    // the following 256 bytes as loaded
    uint32_t ridx;
    uint64_t win;  // upcoming bits, MSB-aligned
    uint32_t nwin; // valid bits in win
#if HC_DEC_NEXTW
    uint32_t nw;  // chunk[ridx], the next unread word, in a scalar register: a peek reads no lane
    __device__ __forceinline__ uint32_t word() const { return nw; }
#else
    __device__ __forceinline__ uint32_t word() const { return lane_read(chunk, ridx); }
#endif

    __device__ __forceinline__ void next_word()
    {
        if (++ridx == 64) {
            cbase += 256;
            chunk = __builtin_bswap32(nxt);
            nxt = buf_load(rs, cbase + 256 + lane * 4);
            ridx = 0;
        }
#if HC_DEC_NEXTW
        nw = lane_read(chunk, ridx);
#endif
    }
    // the window with the bits below its nwin >= 32 valid ones filled from the next unread word:
    // 64 true bits. No state changes: refill() ORs the same word at the same place later.
    __device__ __forceinline__ uint64_t peek() const
    {
        return win | (uint32_t)((uint64_t)word() >> (nwin - 32));
    }
    // a batch step took sj of the n0 valid bits of w (peek()'s value): when sj > n0 the bits past
    // n0 come off the peeked word, which refill() pushes with those bits shifted out (nwin < 0 as
    // a signed value: its shift is 32 - nwin <= 63); 1..31 bits are valid after it, and every
    // call site tests nwin <= 32 before the window is read again
    __device__ __forceinline__ void take_peeked(uint64_t w, uint32_t n0, uint32_t sj)
    {
        win = w << sj;
        nwin = n0 - sj;
        if ((int32_t)nwin < 0) refill();
    }
    // push the next 32 bits (needs nwin <= 32)
    __device__ __forceinline__ void refill()
    {
        const uint32_t w = word();
        win |= (uint64_t)w << (32 - nwin);
        nwin += 32;
        next_word();
    }
    __device__ __forceinline__ uint32_t bit()
    {
        if (nwin == 0) refill();
        const uint32_t b = (uint32_t)(win >> 63);
        win <<= 1;
        --nwin;
        return b;
    }
    __device__ __forceinline__ uint32_t bits8()
    {
        if (nwin < 8) refill();
        const uint32_t b = (uint32_t)(win >> 56);
        win <<= 8;
        nwin -= 8;
        return b;
    }
};

// ------------------------------------------------------- RLE + diff revert (decoder) ------

// transform.cpp:137-159 (RLE revert) then 231-239 (diff revert) for one block of <= 256
// symbols, all lanes at once (model and derivation: tests/revert_block_model.py). The serial
// revert is a 4-state machine on the run counter r: in state 3 a symbol is a count (it emits
// that many copies of the previous symbol, r -> 0), else a literal (r -> r+1 when it repeats the
// previous symbol and r is 1 or 2, otherwise r -> 1). A symbol's transition is one of two
// functions on {0..3}, a 4-byte table (byte x = f(x)), so a composition is one v_perm_b32; a
// wave scan of the compositions gives each symbol's state, scans of output lengths and diff
// sums give each lane's output offset and running byte. Literals write their byte; a lane holds
// at most one count (counts follow three equal literals, so they are >= 4 symbols apart), and
// each count's run (an arithmetic sequence mod 256 with the diff model, a constant without)
// is written by the whole wave, 64 bytes per store.
struct RevCarry {
    uint32_t r;     // machine state after the last symbol
    uint32_t last;  // last symbol
    uint32_t prev;  // last output byte (diff model)
};

constexpr uint32_t kFeq = 1u | 2u << 8 | 3u << 16;  // r: 0->1 1->2 2->3 3->0
constexpr uint32_t kFne = 1u | 1u << 8 | 1u << 16;  // r: 0->1 1->1 2->1 3->0
constexpr uint32_t kFid = 0u | 1u << 8 | 2u << 16 | 3u << 24;

__device__ __forceinline__ uint32_t fsm_compose(uint32_t g, uint32_t f)  // x -> g(f(x))
{
    return __builtin_amdgcn_perm(0u, g, f);  // byte x = byte f(x) of g
}
__device__ __forceinline__ uint32_t fsm_apply(uint32_t f, uint32_t r) { return (f >> (8 * r)) & 255u; }

// lane l holds symbols 4l..4l+3 (m valid); bytes go to the stream's output at pos onwards (the
// buffer range check drops what is past the capacity); returns the bytes produced
__device__ __forceinline__ uint32_t revert_block(uint32_t x4, uint32_t m, RevCarry &cy, uint32_t dmask,
                                                 rsrc_t rs, uint32_t pos, uint32_t *row, uint32_t lane)
{
    const uint32_t xp = (x4 << 8) | (wave_shr1(x4, cy.last << 24) >> 24);  // previous symbols
    const uint32_t i0 = lane * 4;
    uint32_t f[4], F = kFid;
    for (uint32_t b = 0; b < 4; ++b) {
        f[b] = i0 + b < m ? (byte_of(x4, b) == byte_of(xp, b) ? kFeq : kFne) : kFid;
        F = fsm_compose(f[b], F);
    }
    // inclusive scan, lanes 0..l applied in order: DPP row shifts, then row broadcasts 15 and 31;
    // lanes without a source keep the identity
    uint32_t inc = F;
    inc = fsm_compose(inc, __builtin_amdgcn_update_dpp(kFid, inc, 0x111, 0xF, 0xF, false));  // row_shr:1
    inc = fsm_compose(inc, __builtin_amdgcn_update_dpp(kFid, inc, 0x112, 0xF, 0xF, false));  // row_shr:2
    inc = fsm_compose(inc, __builtin_amdgcn_update_dpp(kFid, inc, 0x114, 0xF, 0xF, false));  // row_shr:4
    inc = fsm_compose(inc, __builtin_amdgcn_update_dpp(kFid, inc, 0x118, 0xF, 0xF, false));  // row_shr:8
    inc = fsm_compose(inc, __builtin_amdgcn_update_dpp(kFid, inc, 0x142, 0xA, 0xF, false));  // row_bcast:15
    inc = fsm_compose(inc, __builtin_amdgcn_update_dpp(kFid, inc, 0x143, 0xC, 0xF, false));  // row_bcast:31
    uint32_t r = fsm_apply(wave_shr1(inc, kFid), cy.r);
    uint32_t len[4], c[4], tot = 0, ds = 0, cnt_b = 4;  // cnt_b: the lane's count symbol (4: none)
    for (uint32_t b = 0; b < 4; ++b) {
        const uint32_t sb = byte_of(x4, b), pb = byte_of(xp, b);
        const bool valid = i0 + b < m;
        const bool cnt = r == 3;
        len[b] = valid ? (cnt ? sb : 1u) : 0u;
        c[b] = cnt ? pb : sb;
        ds += valid ? (cnt ? sb * pb : sb) : 0u;
        tot += len[b];
        cnt_b = valid && cnt ? b : cnt_b;
        r = fsm_apply(f[b], r);
    }
    // exclusive scans of (length, diff sum mod 256), packed: both halves stay below 2^16
    const uint32_t mine = tot | ((ds & 255u) << 16);
    const uint32_t acc = RecSink::scan_add(mine);
    const uint32_t exc = acc - mine;
    uint32_t prev = (cy.prev + (exc >> 16)) & 255u;
    uint32_t o = pos + (exc & 0xFFFFu);
    // literals; the count only records its run: output offset, length | base << 8 | step << 16
    // (run byte j = base + step * (j + 1); base = the byte before it, or the repeated byte
    // itself with step 0 without the diff model)
    uint32_t ro = 0, rlen = 0;
    for (uint32_t b = 0; b < 4; ++b) {
        if (b == cnt_b) {
            rlen = dmask ? (len[b] | prev << 8 | c[b] << 16) : (len[b] | c[b] << 8);
            ro = o;
            prev = dmask ? (prev + len[b] * c[b]) & 255u : (len[b] ? c[b] : prev);
        } else {
            prev = ((prev & dmask) + c[b]) & 255u;
            buf_store8(rs, len[b] ? o : kDrop, prev);
        }
        o += len[b];
    }
    // the runs (run byte j = v1 + st1 * j), 16 at a time, four lanes each: a run's 16-byte units
    // (aligned in memory) go four per store, 64 contiguous bytes a run, then the <= 15 + 15 bytes
    // before and after them four per store -- grad -c -m (~54 runs of ~255 bytes per block) takes
    // 4 groups of ~4 + ~8 steps instead of a pass of the whole wave per run and 64 bytes
    // (measured: grad decode 1.30 -> 1.17 ms, C5 383 -> 380, noise 164.5 -> 161; without the run
    // stores at all 0.92 ms; one run per lane, 16-byte units scattered over 64 runs per store,
    // 1.36 ms; whole dwords run by run 1.30 ms: the run loop's instructions, not its stores). A block whose runs reach past the
    // output window (a capacity error) goes run by run, byte by byte, so every byte before the
    // end lands.
    const uint32_t n = rlen & 255u;
    const uint32_t st1 = dmask ? rlen >> 16 : 0u, v1 = (((rlen >> 8) & 255u) + st1) & 255u;
    const uint64_t rm = ballot(n != 0);
    if (rm && !ballot(ro + n > rs.bytes)) {
        // the lanes that hold a run, in order: row[k] = the k-th one
        if (n) row[__builtin_amdgcn_mbcnt_hi((uint32_t)(rm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rm, 0u))] = lane;
        __builtin_amdgcn_wave_barrier();
        const uint32_t nr = (uint32_t)__builtin_popcountll(rm), q = lane & 3u;
        const uint32_t spec = n | st1 << 8 | v1 << 16;
        constexpr uint32_t kL7 = 0x7F7F7F7Fu, kH = 0x80808080u;
        auto add8 = [&](uint32_t a, uint32_t b) __attribute__((always_inline)) {
            return ((a & kL7) + (b & kL7)) ^ ((a ^ b) & kH);
        };
        for (uint32_t g = 0; g < nr; g += 16) {
            const uint32_t r = g + (lane >> 2);
            const uint32_t src = row[r < nr ? r : 0u] * 4;
            // (both permutes on every lane: a source lane outside the exec mask would give 0)
            const uint32_t gs0 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)src, (int)spec);
            const uint32_t go = (uint32_t)__builtin_amdgcn_ds_bpermute((int)src, (int)ro);
            const uint32_t gs = r < nr ? gs0 : 0u;
            const uint32_t gn = gs & 255u, gst = (gs >> 8) & 255u, gv = gs >> 16;
            const uint32_t hb = min((0u - ((uint32_t)rs.base + go)) & 15u, gn);  // bytes before the units
            const uint32_t nu = (gn - hb) >> 4, eb = gn - 16 * nu;                // units; edge bytes
            // bytes j0 .. j0 + 15: a splat of byte j0 plus (0, s, 2 s, 3 s), then + 4 s per byte for
            // each next dword (bytewise adds without carries)
            const uint32_t P = ((gst & 255u) << 8 | ((2 * gst) & 255u) << 16 | ((3 * gst) & 255u) << 24);
            const uint32_t S4 = __builtin_amdgcn_perm(0u, 4u * gst, 0u);
            uint32_t u = q, x = gv + gst * (hb + 16 * q), o = go + hb + 16 * q;
            while (ballot(u < nu)) {
                u32x4 w;
                w[0] = add8(__builtin_amdgcn_perm(0u, x, 0u), P);
                w[1] = add8(w[0], S4);
                w[2] = add8(w[1], S4);
                w[3] = add8(w[2], S4);
                buf_store4(rs, u < nu ? o : kDrop, w);
                u += 4;
                x += 64u * gst;
                o += 64u;
            }
            for (uint32_t e = q; ballot(e < eb); e += 4) {
                const uint32_t j = e < hb ? e : e + 16 * nu;
                buf_store8(rs, e < eb ? go + j : kDrop, gv + gst * j);
            }
        }
        __builtin_amdgcn_wave_barrier();
    } else {
        for (uint64_t runs = ballot(n != 0); runs; runs &= runs - 1) {
            const uint32_t l = (uint32_t)__builtin_ctzll(runs);
            const uint32_t at = lane_read(ro, l), rn = lane_read(n, l), rv = lane_read(v1, l), rs1 = lane_read(st1, l);
            for (uint32_t j0 = 0; j0 < rn; j0 += 64) {
                const uint32_t j = j0 + lane;
                buf_store8(rs, j < rn ? at + j : kDrop, rv + rs1 * j);
            }
        }
    }
    const uint32_t all = lane_read(acc, 63);
    cy.r = fsm_apply(lane_read(inc, 63), cy.r);
    cy.last = byte_of(lane_read(x4, (m - 1) >> 2), (m - 1) & 3u);
    cy.prev = (cy.prev + (all >> 16)) & 255u;
    return all & 0xFFFFu;
}

// One stream's decoder (huffman.cpp:60-93 + transform.cpp:386-406 per symbol, then the RLE and
// diff revert of transform.cpp:137-159 / 231-239 per 256-symbol block; header main.cpp:90-104).
// decode_kernel runs one per wavefront.
// The small-alphabet launch (decode_kernel<0, .., true>, Dec::decode_small) takes the narrow
// streams whose payload averages under 2.5 bits per symbol -- the header's count and the
// stream's length, so the decoder needs no sample of its own (grad -c -m: 1.7; photo -c -m:
// 3.3-3.6; noise, -c photos: ~8). mode (hc_debug_set_dec_small): 0 by the rate, 1 every narrow
// stream, 2 none. Either launch decodes any stream exactly; the rate only picks the faster.
__device__ __forceinline__ bool dec_small_stream(uint64_t count, uint64_t bits, uint32_t mode)
{
    if (mode) return mode == 1;
    return count != 0 && bits * 2 < count * 5;
}

template <int kW, int kDst, bool kSmall = false>
struct Dec {
    // symbol indices: 32-bit below 2^32 symbols (narrow / wide), 64-bit for the huge layout
    using Idx = std::conditional_t<kW == 2, uint64_t, uint32_t>;
    Fgk<kW, true, false, kSmall> fgk;
    BitSource in;
    uint32_t lane, sid, st, dmask;
    uint64_t len, cap, payload_bits;
    uint64_t obase;  // output window at byte obase (slides with the output, like the input's)
    uint64_t pos;    // output bytes produced
    rsrc_t rout;
    RevCarry rc;
    uint8_t *sbuf;  // this block's symbols (LDS)
    Idx n;
    uint32_t bsym = 0, btry = 0;  // this block's batch symbols and batches
    Prio<Idx> prio;
    bool batch_on = true;          // the next block runs batches
    uint64_t pacc = 0;  // HC_PROF regions

    __device__ __forceinline__ Dec(Tree<kW, true, false, kSmall> &t, uint32_t l) : fgk(t, l), lane(l) {}

    // the stream's header; false: nothing to decode here (its error status is written, or another
    // tree layout's launch owns it)
    __device__ __forceinline__ bool open(const Batch &bt, uint32_t s)
    {
        sid = s;
        const uint64_t in_off = uni64(bt.in_offs[sid]);
        len = uni64(bt.in_lens[sid]);
        cap = uni64(bt.out_caps[sid]);
        const uint32_t len32 = (uint32_t)min(len, (uint64_t)kMaxBufBytes);
        const rsrc_t rin = make_rsrc(bt.in + in_off, (len32 + 3u) & ~3u);
        const uint32_t hdr = buf_load(rin, lane * 4);  // words 0..63 of the stream
        st = 0;
        uint64_t count = 0;
        uint32_t flags = 0;
        if (len < 9) {
            st = HC_ERR_HEADER;  // main.cpp:99-104
        } else {
            count = (uint64_t)lane_read(hdr, 0) | ((uint64_t)lane_read(hdr, 1) << 32);
            flags = lane_read(hdr, 2) & 255u;
            const uint64_t avail = (len - 9) * 8;
            // the first symbol costs >= 8 bits and each later one >= 1: a larger count cannot
            // decode, and the reference ends such a stream with status 9 (transform.cpp:394-398)
            if (count > (avail >= 8 ? avail - 7 : 0)) st = HC_ERR_HUFFMAN;
            else if (kDst == DST_RAW && (flags & 0x40u)) st = HC_ERR_UNSUPPORTED;
        }
        if (st == 0 && tree_kind(count, bt.min_tree) != (uint32_t)kW) return false;  // another layout's launch owns it
        // narrow streams under 2.5 payload bits per symbol go to the small-alphabet launch
        // (dec_small_stream), the rest to the regular one
        if (st == 0 && kW == 0 && dec_small_stream(count, (len - 9) * 8, bt.dec_small) != kSmall) return false;
        if (st != 0) {
            if (kW == 0 && !kSmall && lane == 0) {
                bt.status[sid] = (int32_t)st;
                bt.out_lens[sid] = 0;
            }
            return false;
        }
        in.rs = rin;
        in.ibase = 0;
        in.lane = lane;
        in.cbase = 0;
        in.chunk = __builtin_bswap32(hdr);
        in.nxt = buf_load(rin, 256 + lane * 4);
        in.ridx = 2;
#if HC_DEC_NEXTW
        in.nw = lane_read(in.chunk, 2);
#endif
        in.win = 0;
        in.nwin = 0;
        in.refill();  // word 2: flags byte + first payload bits
        in.win <<= 8;
        in.nwin -= 8;
        rout = make_rsrc(bt.out + uni64(bt.out_offs[sid]), (uint32_t)min(cap, (uint64_t)kMaxBufBytes));
        obase = 0;
        pos = 0;
        dmask = kDst == DST_RAW && (flags & 0x80u) ? 255u : 0u;  // diff model
        rc = {0, 0, 0};
        sbuf = reinterpret_cast<uint8_t *>(fgk.T.syms);
        n = (Idx)count;
        payload_bits = (len - 9) * 8;
        return true;
    }
    // input and output fit one buffer window (every batch stream): no window bookkeeping
    __device__ __forceinline__ bool one_window() const
    {
        const uint32_t window = window_bytes();
        return len + 512 <= window && cap <= window;
    }
    // bits read from the stream = words pushed into the window * 32 - bits still in it; the
    // payload starts at bit 72. A stream that ends early decodes zero bits past its end (the
    // range check); the reference stops there with status 9 (transform.cpp:394-398), which is
    // what close() reports.
    __device__ __forceinline__ uint64_t consumed() const { return ((in.ibase + in.cbase) / 4 + in.ridx) * 32 - in.nwin - 72; }
    __device__ __forceinline__ bool stopped() const { return fgk.bad || consumed() > payload_bits + 64; }
    // a block's symbols end at i1
    __device__ __forceinline__ Idx block_end(Idx i0) const
    {
        if constexpr (kW == 2) return n - i0 < 256 ? n : i0 + 256;
        else return min(n, i0 + 256);
    }

    template <bool kWin>
    __device__ __forceinline__ void block_start(const Batch &bt, Idx i0)
    {
        if constexpr (kWin) {
            const uint32_t window = window_bytes();
            if (in.cbase >= window) {  // slide the input window to the current chunk (a block of
                in.ibase += in.cbase;  // 256 symbols reads < 2 KB, so offsets stay below 2^31)
                in.cbase = 0;
                const uint64_t l = uni64(bt.in_lens[sid]);
                in.rs = make_rsrc(bt.in + uni64(bt.in_offs[sid]) + in.ibase,
                                  (uint32_t)min((l - min(l, in.ibase) + 3u) & ~3ull, (uint64_t)kMaxBufBytes));
            }
            if (pos - obase >= window) {  // and the output window to the next byte
                obase = pos;
                rout = make_rsrc(bt.out + uni64(bt.out_offs[sid]) + obase,
                                 obase < cap ? (uint32_t)min(cap - obase, (uint64_t)kMaxBufBytes) : 0u);
            }
        }
        prio.at(i0, n);
    }

    // symbol i - 1 (of the block at i0) left the hot loop with its leaf entry's position x and
    // depth d, the body b read at x, the root path pv and the first level k whose leader test
    // failed (the window stands d bits into its code): finish it
    __device__ __forceinline__ void finish_symbol(uint32_t b, uint32_t pv, uint32_t k, uint32_t d, uint32_t x, Idx i, Idx i0)
    {
        if (!(b & (kInner | kNyt))) {  // a leaf whose update reported level k: walk from there
            HC_PROF_BEGIN();
            fgk.walk(lane_read(pv, k), pv);
            HC_PROF_END(1);
            return;
        }
        // nothing was stored for it
        uint32_t sym = 0;
        bool deep = false;  // a code longer than the cache's 9 levels: a rare symbol
        HC_PROF_BEGIN();
        if (b & kInner) {
            // the code is longer than the tables reach, or they stopped short (a leaf that
            // split since): descend bit by bit, top-down first (depth j at lane 64-j),
            // then turned bottom-up
            uint32_t depth = d;
            fgk.stale += depth < 8 ? 1u : 0u;
            if (fgk.stale >= kRefresh) fgk.from = 0;
            // levels 1..8 of the prefix, lane 64 - j <- level j (lane 8 - j of the path read)
            uint32_t pt = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((lane - 56) & 63u) * 4), (int)pv);
            // the position and its body stay in VGPRs (wave-uniform): per level the child address,
            // one read, a select into lane 63 - depth (a scalar bit mask) and the inner test by a
            // ballot -- no hop through the scalar unit per level (~22 -> ~13 instructions). The
            // tree is the kernel's own (input bits only choose the child), and the depth bound ends
            // the walk down on any inconsistency.
            // The window's bits are taken straight from a copy of it; the refill (and the 63-level
            // bound) is tested once per level against lim, the depth the bits in the window reach.
            const uint32_t bbase = lds_off16(&fgk.T.body[0]);
            uint32_t xv = vreg(x), bv = vreg(b);
            if (in.nwin <= 32) in.refill();
            uint64_t w = in.win;
            uint32_t d0 = depth, lim = min(depth + in.nwin, 63u);
#if HC_DESC_GROUP
            bool ended = false;
            // The first kDescLevels levels in groups (kDescSched: the levels after which the inner
            // test happens; tests/fgk_climb_model.py chooses it), when the window holds that many
            // bits. The bits come from a VGPR copy of the window's high word at compile-time
            // offsets: a level is the bit, the child index, its record into the lane of its depth
            // and the body read, whose word goes into the same lane of bq -- no window shift, depth
            // counter or stop arithmetic per level -- and a group ends with one ballot of bq's
            // inner bits. The first level whose body is not inner ends the code (lanes not written
            // count as inner); the levels below it read only in-range garbage ((body & 255) * 2 +
            // bit <= 511), their lanes fall to kRoot in the turn below, and no bit past that level
            // is consumed. A group of one level tests the body as read and ends in place.
            // (Measured and dropped: streams whose batch steps are off -- flat alphabets, whose long
            // codes are one level below the tables -- kept on the per-level loop by a test of
            // batch_on here: noise decoded 1 % slower with it)
            if (depth + kDescLevels <= lim) {
                const uint32_t wv = vreg((uint32_t)(w >> 32));  // nwin > 32 >= kDescLevels
                uint32_t bq = kInner;
                uint64_t mk = 1ull << (63 - depth);  // the lane of the level reached next
                uint64_t ni = 0;
                uint32_t k = 0, de = depth + kDescLevels;
#pragma unroll
                for (uint32_t g = 0; g < sizeof(kDescSched) / sizeof(kDescSched[0]); ++g) {
                    const bool one = kDescSched[g] == k + 1;  // a one-level group: xv and bv are its end
#pragma unroll
                    for (; k < kDescSched[g]; ++k) {
                        const uint32_t bit = (wv >> (31 - k)) & 1u;
                        xv = ((bv << 1) & 0x1FEu) | bit;  // child pair * 2 + bit
                        pt = sel(mk, xv, pt);
                        bv = opaque(*(const lds_u16 *)(size_t)(bbase + 2 * xv));
                        if (!one) bq = sel(mk, bv, bq);  // (a level that goes on was inner, as bq starts)
                        mk >>= 1;
                    }
                    if (one) {
                        if (!ballot(bv & kInner)) {
                            de = depth + k;
                            ended = true;
                            break;
                        }
                    } else if ((ni = ballot(!(bq & kInner))) != 0) {
                        const uint32_t le = 63u - (uint32_t)__builtin_clzll(ni);  // the highest lane: the first such level
                        de = 64u - le;
                        xv = vreg(lane_read(pt, le));
                        bv = vreg(lane_read(bq, le));
                        ended = true;
                        break;
                    }
                }
                w <<= de - depth;
                depth = de;
            }
#pragma unroll 1
            while (!ended) {
#else
#pragma unroll 1
            for (;;) {
#endif
                uint64_t inner;
#pragma unroll 1
                do {
                    const uint32_t bit = (uint32_t)(w >> 63);
                    w <<= 1;
                    xv = ((bv << 1) & 0x1FEu) | bit;  // child pair * 2 + bit
                    pt = sel(1ull << (63 - depth), xv, pt);
                    ++depth;
                    bv = opaque(*(const lds_u16 *)(size_t)(bbase + 2 * xv));
                    // go on while the body is inner and the window has bits: one compare
                    // (inner bit > stop) the branch takes as it is
                    uint32_t stop = (lim - depth - 1u) >> 31;  // depth >= lim (both < 64)
                    asm("" : "+s"(stop));  // kept an integer (a compare would go through a select)
                    inner = ballot(((bv >> 8) & 1u) > stop);
                } while (inner);
                if (!ballot(bv & kInner) || depth >= 63) break;
                // the window is used up (rare): its next word
                in.win = w;
                in.nwin -= depth - d0;  // 0
                in.refill();
                w = in.win;
                d0 = depth;
                lim = min(depth + in.nwin, 63u);
            }
            in.win = w;
            in.nwin -= depth - d0;
            x = uni(xv);
            b = uni(bv);
            if (depth > 62) fgk.bad = 1;  // beyond the lanes (needs > 2^32 symbols)
            deep = depth > kInsertDepth;
            pv = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((64 - depth + lane) & 63u) * 4), (int)pt);
            pv = lane < depth ? pv : kRoot;
            sym = b & 255u;
        }
        if (b & kNyt) {  // the new leaf below the NYT becomes level 0
            sym = in.bits8();
            // huffman.cpp:95-111 splits only for a symbol without a leaf; a corrupted stream
            // can name a known one, whose own leaf is then updated
            const uint32_t known = fgk.find_leaf(sym);
            if (known == 0xFFFFFFFFu) {
                x = uni(fgk.split(sym));
                pv = __shfl_up(pv, 1, 64);
                pv = lane == 0 ? x : pv;
            } else {
                fgk.chase(known, pv);
            }
        }
        HC_PROF_END(2);
        if (!(b & kInner)) {
            HC_PROF_BEGIN();
            // a rare symbol's leaf nearly always ties with the next position (9 in 10 on
            // the slot-form model): walk from the leaf at once
            if (deep) fgk.walk(lane_read(pv, 0), pv);
            else fgk.update_path(pv);
            HC_PROF_END(3);
        }
        sbuf[i - 1 - i0] = (uint8_t)sym;
    }

#if HC_DEC_BATCH
    // the batch steps of this launch work on 64 true window bits (BitSource::peek)
    static constexpr bool kTopUp = HC_DEC_TOPUP && (!kSmall || HC_DEC_TOPUP_SMALL);
    // Batched hot path (narrow and wide layouts; model: tests/fgk_pack_model.py decode_packed).
    // Between swaps and splits the tree's shape -- and with it every code -- is fixed, and the
    // update of a symbol whose levels all pass the leader test only adds 1 along its root path.
    // So up to kPackMax codes are decoded in a row from the level tables alone, packed by bit
    // offset: lane o stands for bit o of the window, and the d lanes S..S + d - 1 of a d-bit code
    // that starts at bit S read its path from depth 1 down to the leaf (lane o: the level-k entry
    // of the k = o - S + 1 bits S..o, addressed as the one-symbol loop addresses it). No lane
    // pads a short code, so a step takes as many codes as the window holds bits for; lane 63
    // is the root. The step:
    //  0. the depth of a code starting at every bit offset (the level-8 entries), the chain of
    //     code starts S_j+1 = S_j + depth(S_j) on registers -- HC_DEC_CHAIN 2: every second start
    //     from the depths of two codes, the others filled in lane-parallel -- and each lane's code
    //     index and code start from the mask of start bits;
    //  1. every code's path positions get their increment tentatively, one LDS add (the root
    //     one per code, by lane 63), the words of the next positions having been read before;
    //  2. a level fails when that next word is below the position's word after the adds: the
    //     one-symbol loop's test with every batch symbol through the position counted as
    //     earlier (c0 at its largest) and none through the next one (c1 = 0), so it can report
    //     a level falsely, never pass one that fails;
    //  3. the increments of the first failing code and the ones after it are taken back. The
    //     codes before it are decoded; it -- or the first code whose entry is not a leaf (a
    //     code longer than the tables, or the NYT) -- goes to the one-symbol step.
    // Returns whether the batch took every code the window and the block allowed (otherwise the
    // one-symbol step takes the next one).
    __device__ __forceinline__ bool decode_batch(Idx i0, Idx &i, Idx i1)
    {
        constexpr uint32_t kPackMax = HC_DEC_PACK;  // codes per step
        static_assert(kPackMax % 4 == 0 && kPackMax >= 4 && kPackMax <= 24, "chain chunks of four codes");
        constexpr uint64_t kL63 = 1ull << 63;
        const uint32_t n0 = in.nwin;  // >= 32 (32: after a step that took the whole window)
        const uint64_t w0 = kTopUp ? in.peek() : in.win;  // kTopUp: 64 true bits
        const uint32_t lim = kTopUp ? 63u : min(n0, 63u);
        const uint32_t l8 = lds_off16(&fgk.T.lvl[254]);  // level 8
        // lane o: the depth of a code that starts o bits into the window (its level-8 entry)
        const uint32_t dep = opaque(*(const lds_u16 *)(size_t)(l8 + 2 * (uint32_t)((w0 << lane) >> 56))) >> 10;
        uint32_t S = lane_read(dep, 0);
        // a first code of HC_DEC_EXIT_BITS bits or more (most of them on a flat alphabet, e.g. noise,
        // where codes reach past the tables) goes to the one-symbol step at once; so does depth 0 (the
        // tables of a tree that was the NYT alone: every entry the root, no code has a lane)
        if (HC_DEC_EXIT8 ? S - 1 >= HC_DEC_EXIT_BITS - 1 : S == 0) {
            ++btry;
            return false;
        }
        // the chain of code starts: sv lane j = S_j, the bits before code j (255: no such code).
        // Four codes per exit test; a code is taken only if it ends within bit 62 (HC_DEC_TOPUP 0:
        // and within the window's valid bits), so the chain ends once S passes lim. Past bit 63 the depths
        // read are another offset's (the lane select wraps): S still grows, so those starts
        // stay above lim.
        // (measured and dropped on the 7 x 9 layout: the chain by pointer doubling, C5 decode
        // +0.8 %)
        uint32_t sv = lane == 0 ? 0u : 255u;
#if HC_DEC_CHAIN == 1
        sv = writelane(sv, S, 1);
#pragma unroll
        for (uint32_t j = 1; j < kPackMax; ++j) {
            if (j % 4 == 0 && S >= lim) break;
            S += lane_read(dep, S);
            sv = writelane(sv, S, j + 1);
        }
#else
        // HC_DEC_CHAIN 2 / 4: the serial chain visits every second / fourth start only, on the depth
        // map composed with itself (lane o: the bits of the two / four codes from bit o on; a code
        // that ends past bit 63 counts 64 more, so nothing wraps into another offset's depth below
        // bit 64), with the exit tests where the chain of single codes has them. The starts in
        // between come lane-parallel afterwards: lane j of sv takes the start in the lane below it
        // (stride 4: first the one two lanes below, from dep2, then the one below) plus that
        // start's depth. Lanes whose source holds no start (255, or one past bit 63)
        // get a value above 63 and keep their own through the min; the shift stays inside lanes
        // 0..15, so lane 16 and up are never filled. A start at or past lim that the chain of
        // single codes would have left at 255 after an exit is filled with a value above lim:
        // nval, jmax, se and the start mask up to bit lim are the same (tests/fgk_chain_model.py).
        constexpr uint32_t kCh = HC_DEC_CHAIN;
        auto compose = [&](uint32_t d) __attribute__((always_inline)) {
            const uint32_t nx = lane + d;
            const uint32_t dn = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(nx * 4), (int)d);
            return d + (nx < 64 ? dn : 64u);
        };
        const uint32_t dep2 = compose(dep);
        const uint32_t depc = kCh == 4 ? compose(dep2) : dep2;
        uint32_t E = lane_read(depc, 0);
        sv = writelane(sv, E, kCh);
#pragma unroll
        for (uint32_t j = 2; j * kCh <= kPackMax; ++j) {
            if ((j - 1) * kCh % 4 == 0 && E >= lim) break;
            E += lane_read(depc, E);
            sv = writelane(sv, E, j * kCh);
        }
        if constexpr (kCh == 4) {
            const uint32_t pr = (uint32_t)__builtin_amdgcn_update_dpp(255, (int)sv, 0x112, 0x1, 0xF, false);  // row_shr:2, lanes 0..15
            sv = min(sv, pr + (uint32_t)__builtin_amdgcn_ds_bpermute((int)(pr * 4), (int)dep2));
        }
        {
            const uint32_t pr = (uint32_t)__builtin_amdgcn_update_dpp(255, (int)sv, 0x111, 0x1, 0xF, false);  // row_shr:1, lanes 0..15
            sv = min(sv, pr + (uint32_t)__builtin_amdgcn_ds_bpermute((int)(pr * 4), (int)dep));
        }
#endif
        // codes inside the window (S_j+1 <= lim; the starts grow, so these are the first nval)
        // and the block
        const uint32_t nval = (uint32_t)__builtin_popcountll(ballot(sv <= lim)) - 1;
        const uint32_t jmax = min(nval, dec_pack_max(min(kPackMax, (uint32_t)(i1 - i))));
        const uint32_t se = lane_read(sv, jmax);  // the bits of the codes taken, <= 63
        // the start bits as a mask: lane j sends a mark to lane S_j (the lanes without a code and
        // the starts past bit 62 to lane 63, whose bit then only says that some code ends there
        // or later); a code's leaf lane is the one before the next start
        const uint64_t sm = ballot(__builtin_amdgcn_ds_permute((int)(min(sv, 63u) * 4), 1) != 0);
        const uint64_t leaf = sm >> 1;
        const uint64_t act = below_mask(se);  // the lanes of the codes taken
        // the lane's code: the starts in bits 1..o; its start; its level
        const uint32_t jv = __builtin_amdgcn_mbcnt_hi((uint32_t)(leaf >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)leaf, 0u));
        uint32_t so = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(jv * 4), (int)sv);
        so = sel(act, so, lane);  // idle lanes: level 1 of their own bit (a valid entry, not added)
        const uint32_t k = lane + 1 - so;
        // the level-k entry of bits so..o: index ((1 << k) | prefix) - 2
        const uint32_t pre = __builtin_amdgcn_ubfe((uint32_t)(w0 >> (63 - lane)), 0, k);
        const uint32_t ent = opaque(*(const lds_u16 *)(size_t)(lds_off16(&fgk.T.lvl[0]) - 4 + 2 * ((1u << k) + pre)));
        const uint32_t pos = sel(kL63, kRoot, ent & 1023u);
        // the lanes that add: every path position of the codes taken, and the root. An entry of
        // level k <= the code's depth stops at level k in tables built whole, which is what a
        // step reads; a lane where it does not (every lane of a code is a path position here, none
        // pads) ends the batch at its code like a failing level, below.
        const uint64_t actm = ballot((ent >> 10) == k) & act;
        constexpr uint32_t kI = kW ? 1u : 1024u;
        const uint32_t wa = lds_off(&fgk.T.wt[0]) + 4 * pos;
        const uint32_t scr = lds_off(fgk.scr32());
        // a leaf's body is its symbol; bit 15: inner or NYT (read with the weights: a code whose
        // entry is no leaf has its increments taken back like a failing one)
        const uint32_t b = opaque(*(const lds_u16 *)(size_t)(lds_off16(&fgk.T.body[0]) + 2 * pos));
        const uint32_t w1 = *(const lds_u32 *)(size_t)(wa + 4);
        __hip_atomic_fetch_add((uint32_t *)(lds_u32 *)(size_t)sel(actm | kL63, wa, scr), sel(kL63, jmax * kI, kI),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        const uint32_t wn = *(const lds_u32 *)(size_t)wa;
        // the first lane of a failing level or of a leaf lane that holds no leaf: its code ends
        // the batch (the root's next word is a sentinel: lane 63 never fails)
        const uint64_t nl = ballot(b & kNotLeaf) & leaf & act;
        const uint64_t fm = (ballot(w1 < wn) & actm) | nl | (act & ~actm);
        uint32_t jf = jmax, sj = se;
        if (fm) {
            const uint32_t fl = ff1(fm);
            jf = lane_read(jv, fl);
            sj = lane_read(so, fl);
            __hip_atomic_fetch_add((uint32_t *)(lds_u32 *)(size_t)sel((actm & (~0ull << sj)) | kL63, wa, scr),
                                   sel(kL63, (jf - jmax) * kI, 0u - kI), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
        const uint32_t sb0 = (uint32_t)(size_t)(lds_u8 *)sbuf + (uint32_t)(i - i0);
        *(lds_u8 *)(size_t)sel(leaf & below_mask(sj), sb0 + jv, scr) = (uint8_t)b;
        __builtin_amdgcn_wave_barrier();
        HC_CNT(1);
        if (jf < jmax) HC_CNT(2);
        if (nl && ff1(nl) == ff1(fm)) HC_CNT(5);
        if constexpr (kTopUp) {
            in.take_peeked(w0, n0, sj);
        } else {
            in.win = w0 << sj;
            in.nwin = n0 - sj;
        }
        i += jf;
        bsym += jf;
        ++btry;
        return jf == jmax;
    }

    // Small alphabets (the small-alphabet launch, narrow layout, while at most 16 symbols are
    // seen: every position >= kSmallNyt; the encoder's small steps in code_all_batch, whose
    // output this reads back). Up to 15 symbols of depth <= 4 per step, four lanes each (lane
    // 4 j + l: level 4 - l of symbol j's lookup in the level tables); the chain of symbol starts
    // from the level-4 depths at every bit offset (<= 4 bits a symbol: 60 bits at most). The
    // leader tests are exact, as in the encoder: every path position ORs its symbol's bit into a
    // membership mark (smark), and symbol j's test at position a reads the pre-step words of a
    // and a + 1 and the marks of both: with c0 / c1 the earlier symbols through a / a + 1 (c1 = j
    // at the root) the level passes iff weight(a + 1) + c1 >= weight(a) + c0 + 1. The first
    // symbol with a failing level, or whose level-4 entry is no leaf (deeper than 4, or the
    // NYT), ends the step: the ones before it commit with one add (the root by lane 63), it goes
    // to the one-symbol step. Returns whether the step took every symbol the window and the
    // block allowed.
    __device__ __forceinline__ bool decode_small(Idx i0, Idx &i, Idx i1)
    {
        static_assert(kW == 0 && kSmall, "the small-alphabet launch: narrow layout");
        constexpr uint32_t kSG = kSmallG, kSK = kSmallK;
        constexpr uint64_t kL63 = 1ull << 63;
        // (the lane index opaque: these per-lane values are made here, not hoisted beside the
        // regular batch's)
        const uint32_t ln = vreg(lane);
        const uint32_t g = ln < kSK * kSG ? ln >> 2 : kSK;  // the lane's symbol (kSK: idle)
        const uint32_t bl = ln & 3u;                        // its level: 4 - bl
        const uint32_t bvb = lds_off16(&fgk.T.lvl[0]) + 2 * ((16u >> bl) - 2);
        const uint32_t l4 = lds_off16(&fgk.T.lvl[14]);  // level 4
        const uint32_t sscb = lds_off(&fgk.T.scratch[0]) + 4 * ln;
        const uint32_t mkb = lds_off(&fgk.T.smark[0]);
        const uint32_t n0 = in.nwin;  // >= 32: symbols 0..7 always fit
        const uint64_t w0 = kTopUp ? in.peek() : in.win;  // kTopUp: 64 true bits, all 15 symbols (<= 60 bits) fit
        // lane o: the depth of a code that starts o bits into the window (4 when deeper)
        const uint32_t dep = opaque(*(const lds_u16 *)(size_t)(l4 + 2 * (uint32_t)((w0 << ln) >> 60))) >> 10;
        // each lane's own code start by a select per chain step (measured: grad decode 1.172 ->
        // 1.158 ms against one permute after the chain, whose round trip the step waits for)
        uint32_t S = 0, sv = 0, sg = 0;
#pragma unroll
        for (uint32_t j = 0; j < kSK; ++j) {
            sv = writelane(sv, S, j);
            sg = g == j ? S : sg;
            S += lane_read(dep, S);
        }
        sv = writelane(sv, S, kSK);
        const uint32_t nval = kTopUp ? kSK : (uint32_t)__builtin_popcountll(ballot(sv <= n0) & (((1ull << kSK) - 1) << 1));
        const uint32_t jmax = min(nval, (uint32_t)(i1 - i));
        const uint32_t ent = opaque(*(const lds_u16 *)(size_t)(bvb + (((uint32_t)((w0 << sg) >> 32) >> (28 + bl)) << 1)));
        uint32_t pos = ent & 1023u;
        pos = sel(~0ull << (kSK * kSG), kRoot, pos);  // lane 63: the root
        const uint64_t gm = below_mask(kSG * jmax);
        // each path position once (the entry stops at the lane's own level)
        const uint64_t am = ballot((ent >> 10) == 4 - bl) & gm;
        const uint32_t wa = lds_off(&fgk.T.wt[0]) + 4 * pos;
        const uint32_t b = opaque(*(const lds_u16 *)(size_t)(lds_off16(&fgk.T.body[0]) + 2 * pos));
        constexpr uint64_t kLeafLanes = 0x0111111111111111ull;  // level 4: lanes 4 j
        const uint32_t jn = ff1(ballot(b & kNotLeaf) & kLeafLanes) >> 2;
        const uint32_t wl = *(const lds_u32 *)(size_t)wa, wh = *(const lds_u32 *)(size_t)(wa + 4);
        const uint32_t ma = pos - kSmallNyt, odd = ma & 1u;  // (pos >= 480 on the am lanes)
        const uint32_t mda = sel(am, mkb + 4 * (ma >> 1), sscb);
        __hip_atomic_fetch_or((uint32_t *)(lds_u32 *)(size_t)mda, (1u << g) << (odd << 4), __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_WAVEFRONT);
        const uint32_t mlo = *(const lds_u32 *)(size_t)mda;
        const uint32_t mhi = *(const lds_u32 *)(size_t)(mda + 4 * odd);
        const uint32_t c0 = (uint32_t)__builtin_popcount(__builtin_amdgcn_ubfe(mlo, odd << 4, g));
        const uint32_t c1 = pos + 1 == kRoot ? g : (uint32_t)__builtin_popcount(__builtin_amdgcn_ubfe(odd ? mhi : mlo, (odd ^ 1u) << 4, g));
        const uint64_t fm = ballot((wh >> 10) + c1 < (wl >> 10) + c0 + 1) & am;
        const uint32_t jf = min(min(ff1(fm) >> 2, jn), jmax);
        __hip_atomic_fetch_add((uint32_t *)(lds_u32 *)(size_t)sel((am & below_mask(kSG * jf)) | kL63, wa, sscb),
                               sel(kL63, jf << 10, 1u << 10), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        *(lds_u32 *)(size_t)mda = 0u;
        const uint32_t sb0 = (uint32_t)(size_t)(lds_u8 *)sbuf + (uint32_t)(i - i0);
        *(lds_u8 *)(size_t)sel(kLeafLanes & below_mask(kSG * jf), sb0 + g, sscb) = (uint8_t)b;
        __builtin_amdgcn_wave_barrier();
        HC_CNT(1);
        if (jf < jmax) HC_CNT(2);
        const uint32_t sj = lane_read(sv, jf);
        if constexpr (kTopUp) {
            in.take_peeked(w0, n0, sj);
        } else {
            in.win = w0 << sj;
            in.nwin = n0 - sj;
        }
        i += jf;
        bsym += jf;
        ++btry;
        return jf == jmax;
    }
#endif

    // symbols i .. i1 - 1 of the block at i0, one stream
    // kBat: batches first (narrow / wide layouts), the one-symbol step after each batch that
    // stops short; otherwise the one-symbol loop alone
    template <bool kBat = (kW <= 1)>
    __device__ __forceinline__ void decode(Idx i0, Idx &i, Idx i1)
    {
        while (i < i1) {
            // huffman.cpp:60-93: the code's first 8 bits index the level tables: level 8 gives
            // where the walk from the root stops (depth d <= 8), the levels above give the
            // positions the walk passes.
            if (fgk.from < 9) {
                HC_PROF_BEGIN();
                fgk.build_levels();
                HC_PROF_END(5);
            }
            if (in.nwin <= 32) in.refill();
#if HC_DEC_BATCH
            // batches, and the symbol that ends one alone (kOne: the one-symbol step takes one)
            constexpr bool kOne = kBat && kW <= 1;
            if constexpr (kOne) {
                HC_PROF_BEGIN();
                bool whole;
                if constexpr (kSmall) whole = fgk.nyt >= kSmallNyt ? decode_small(i0, i, i1) : decode_batch(i0, i, i1);
                else whole = decode_batch(i0, i, i1);
                HC_PROF_END(6);
                if (whole) continue;
                if (in.nwin <= 32) in.refill();
            }
#else
            constexpr bool kOne = false;
#endif
            // Hot loop: a leaf within the tables' reach whose update needs no walk. Once a
            // symbol's depth is known the next symbol's table entry is read, before this
            // symbol's update (the tables and body[] change only on the paths that leave the
            // loop, and the loop is re-entered after them). Anything else
            // (a longer code or a stale table: body inner; the NYT; a failed leader test) is
            // forced to fail at level 0 so nothing is stored, and is finished outside.
            // lane k reads level 8 - k's entry for the code's 8-bit prefix v, at
            // ((256 | v) >> k) - 2: levels >= d repeat the leaf's entry (position | depth d), so
            // lanes 0..8-d hold the leaf, lanes 9-d..7 its ancestors (level 8-k), lane 8 and up
            // the root pad (lvl_root). One read gives the depth (lane 0) and the whole root path
            // (duplicated lanes store the same word); it depends only on the window, so the next
            // code's read goes out as soon as this code's depth is known.
            // ((256 | v) >> k) - 2 = (v >> k) + (256 >> k) - 2, and v >> k = window bits 56 + k..63:
            // one per-lane shift of the window's high word and one per-lane base; lanes 8 and up
            // shift by 31 and land on lvl_root[-2 + 0/1] (both the root)
            const uint32_t vsh = 24 + min(lane, 7u);
            const uint32_t vbase = lds_off16(&fgk.T.lvl[0]) + 2 * (lane < 8 ? (256u >> lane) - 2 : 0xFFFFFFFEu);
            auto path_read = [&](uint64_t w) __attribute__((always_inline)) {
                return opaque(*(const lds_u16 *)(size_t)(vbase + ((uint32_t)(w >> 32) >> vsh) * 2));
            };
            uint32_t pr = path_read(in.win);
            const uint32_t bbase = lds_off16(&fgk.T.body[0]);
            uint32_t d, x, b, pv, k;
            // loop while no level failed (k = 0xFFFFFFFF) and symbols are left (left < 0):
            // both sign bits set, one scalar AND (after a batch: one symbol)
            int32_t left = kOne ? -1 : (int32_t)(i - i1);
            lds_u8 *so = (lds_u8 *)sbuf + (uint32_t)(i - i0);  // the symbol's byte (LDS address in a VGPR)
            // The leaf's body: every lane reads the body at its own path position; one row_newbcast DPP move gives
            // rows 0 its lane 0's (the leaf's), so the read needs no scalar address. Lanes 16 and up
            // (root padding) read lvl_root instead (kRoot: bit 15 clear, no force) and put their
            // copy of the symbol byte in the landing row, not the block.
            const uint32_t vbb = lane < 16 ? bbase : lds_off16(&fgk.T.lvl_root[0]) - 2 * kRoot;
            so += lane < 16 ? 0 : (uint32_t)((uint8_t *)fgk.T.scratch - sbuf);
            uint32_t e8;
            asm("" : "+v"(so));
            do {
                e8 = uni(pr);  // the leaf's entry
                d = e8 >> 10;
                pv = pr & 1023u;
                b = (uint32_t)__builtin_amdgcn_mov_dpp((int)opaque(*(const lds_u16 *)(size_t)(vbb + 2 * pv)), 0x150, 0xF, 0xF, false);
                in.win <<= d;
                in.nwin -= d;  // >= 25
                uint32_t prn;
                // a leaf's body is its symbol; inner / NYT (bit 15): force the failure
                const uint32_t force = (uint32_t)__builtin_amdgcn_sbfe((int)b, 15, 1);
                k = fgk.update_fast(pv, [&] { prn = path_read(in.win); }, force);  // the next code's
                *so++ = (uint8_t)b;  // the symbol (a leaf's body); rewritten when it leaves
                ++left;
                if (in.nwin <= 32) in.refill();
                pr = prn;
            } while ((int32_t)(k & (uint32_t)left) < 0);
            i = i0 + uni((uint32_t)(so - (lds_u8 *)sbuf));
            if (k == 0xFFFFFFFFu) continue;
            x = e8 & 1023u;
            // symbol i - 1 left the loop: the window stands d bits into its code
            finish_symbol(uni(b), pv, k, uni(d), uni(x), i, i0);
        }
    }

    // the block's symbols [i0, i1) leave: reverted to bytes (transform.cpp:137-159, 231-239) or
    // stored as they are (the adaptive path's symbol stream)
    __device__ __forceinline__ void close_block(Idx i0, Idx i1)
    {
        __builtin_amdgcn_wave_barrier();
        const uint32_t x4 = fgk.T.syms[lane];
        const uint32_t m = (uint32_t)(i1 - i0);
        if (kDst == DST_SYMBOLS) {
            for (uint32_t b = 0; b < 4; ++b)
                buf_store8(rout, lane * 4 + b < m ? (uint32_t)(pos - obase) + lane * 4 + b : kDrop, byte_of(x4, b));
            pos += m;
        } else {
            HC_PROF_BEGIN();
            pos += revert_block(x4, m, rc, dmask, rout, (uint32_t)(pos - obase), fgk.T.scratch, lane);
            HC_PROF_END(4);
        }
    }

    // blocks from i0 on; a block left unfinished at i (i0 <= i < its end) is finished first
    template <bool kWin>
    __device__ __forceinline__ void run(const Batch &bt, Idx i0, Idx i)
    {
        for (; i0 < n; i0 += 256, i = i0) {
            if (stopped()) break;
            block_start<kWin>(bt, i0);
            const Idx i1 = block_end(i0);
#if HC_DEC_BATCH
            // Batches pay where they take several symbols each; on flat alphabets (noise, -c
            // photos: codes at or past the tables' 8 bits) they stop short and the one-symbol
            // loop is faster (measured: C4 decode 2.02 s without batches, 3.52 s with them; a
            // lone wave waits out each batch's table reads). A block runs batches when the last
            // block that ran them took at least kBatchYield / 2 symbols per batch, and every
            // HC_BATCH_PROBE-th block tries them again.
            if constexpr (kW <= 1) {
                if (btry) batch_on = 2 * bsym >= kBatchYield * btry;
                bsym = btry = 0;
                if (batch_on || ((uint32_t)(i0 >> 8) & (HC_BATCH_PROBE - 1u)) == 0) {
                    decode<true>(i0, i, i1);
                    close_block(i0, i1);
                    continue;
                }
            }
            decode<false>(i0, i, i1);
#else
            decode(i0, i, i1);
#endif
            close_block(i0, i1);
        }
    }

    __device__ __forceinline__ void close(const Batch &bt)
    {
        if (consumed() > payload_bits) st = HC_ERR_HUFFMAN;  // ran past the payload
        if (fgk.bad) st = HC_ERR_DEVICE;
        if (st == 0 && pos > cap) st = HC_ERR_CAPACITY;
        if (lane == 0) {
            bt.status[sid] = (int32_t)st;
            bt.out_lens[sid] = (st == 0 || st == HC_ERR_CAPACITY) ? pos : 0;
        }
    }
};

template <int kW, int kDst, bool kSmall = false>
__global__ __launch_bounds__(64 * HC_WAVES) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd<kW>))) void decode_kernel(Batch bt)
{
    __shared__ Tree<kW, true, false, kSmall> trees[kWaves];
    const uint64_t t0 = __builtin_amdgcn_s_memtime();
    const uint32_t lane = lane_id();
    const uint32_t wv = uni(threadIdx.x >> 6);
    const uint32_t sid = blockIdx.x * kWaves + wv;
    if (sid >= bt.n) return;
    Dec<kW, kDst, kSmall> dec(trees[wv], lane);
    if (!dec.open(bt, sid)) return;
    // two copies of the block loop, as in the encoder: without window bookkeeping for streams
    // that fit one window (input and output), with it for the rest
    if (dec.one_window()) dec.template run<false>(bt, 0, 0);
    else dec.template run<true>(bt, 0, 0);
    dec.close(bt);
    trace_wave(sid, t0, lane);
    prof_store(sid, t0, dec.pacc + dec.fgk.pacc, lane);
}

}  // namespace

// streams that the table-mode encoder holds resident at once: 6 waves per SIMD (its LDS)
static uint32_t table_slots()
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        cus = 256;
    return (uint32_t)cus * 24;
}

template <int kSrc>
static hipError_t launch_encode_src(const Batch &b, dim3 grid, dim3 block, hipStream_t st, hipStream_t aux)
{
    // every stream votes for its mode (enc_mode_kernel); the cache-mode launches run on the
    // caller's stream, each skipping the other mode's streams. The table-mode launches follow them
    // on the same stream, or -- when the caller gives a second stream -- run beside them there
    // (forked and joined by events), so that a mixed batch fills the GPU with both at once. The
    // library keeps no stream of its own.
    enc_mode_kernel<kSrc><<<(b.n + 3) / 4, 256, 0, st>>>(b, b.n <= table_slots() ? 1u : 0u, enc_tab());
    hipEvent_t fork = nullptr, join = nullptr;
    if (aux == st) aux = nullptr;
    if (aux && (hipEventCreateWithFlags(&fork, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&join, hipEventDisableTiming) != hipSuccess))
        aux = nullptr;
    hipStream_t ts = st;  // the table-mode launches' stream
    if (aux && hipEventRecord(fork, st) == hipSuccess && hipStreamWaitEvent(aux, fork, 0) == hipSuccess) ts = aux;
    encode_kernel<0, kSrc><<<grid, block, 0, st>>>(b);
    encode_kernel<1, kSrc><<<grid, block, 0, st>>>(b);
    encode_kernel<2, kSrc><<<grid, block, 0, st>>>(b);
    encode_kernel<0, kSrc, true><<<grid, block, 0, ts>>>(b);
    encode_kernel<1, kSrc, true><<<grid, block, 0, ts>>>(b);
    hipError_t e = hipGetLastError();
    if (ts != st) {
        const hipError_t e1 = hipEventRecord(join, ts);
        const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(st, join, 0) : e1;
        if (e2 != hipSuccess) {
            // no join: wait for the side stream here, so that an error return never leaves
            // library work running unordered against the caller's buffers
            (void)hipStreamSynchronize(ts);
            if (e == hipSuccess) e = e2;
        }
    }
    // the small-alphabet streams last, after the join: its batch (grad: 8192 streams, one round of
    // waves) must not share the CUs with the other launches' workgroups while they start and exit
    // (launched first, beside the table launches: grad encode 1.23 -> 2.52 ms; after the cache
    // launches but before the join: 1.6 ms)
    encode_kernel<0, kSrc, false, true><<<grid, block, 0, st>>>(b);
    if (e == hipSuccess) e = hipGetLastError();
    if (fork) (void)hipEventDestroy(fork);  // (released once the recorded work completes)
    if (join) (void)hipEventDestroy(join);
    return e;
}

hipError_t launch_encode(const Batch &b0, EncSrc src, hipStream_t st, hipStream_t aux)
{
    if (b0.n == 0) return hipSuccess;
    Batch b = b0;
    b.min_tree = min_tree();
    const dim3 grid((b.n + kWaves - 1) / kWaves), block(64 * kWaves);
    // enc_mode_kernel marks each stream for the cache or the table launch; then one launch per
    // tree layout and mode, each stream coded by exactly one of them (tree_kind, the mark)
    switch (src) {
    case SRC_RAW: return launch_encode_src<SRC_RAW>(b, grid, block, st, aux);
    case SRC_RAW_DIFF: return launch_encode_src<SRC_RAW_DIFF>(b, grid, block, st, aux);
    default: return launch_encode_src<SRC_SYMBOLS>(b, grid, block, st, aux);
    }
}

hipError_t launch_decode(const Batch &b0, DecDst dst, hipStream_t st)
{
    if (b0.n == 0) return hipSuccess;
    Batch b = b0;
    b.min_tree = min_tree();
    b.dec_small = dec_small();
    const dim3 grid((b.n + kWaves - 1) / kWaves), block(64 * kWaves);
    // one launch per tree layout, then the small-alphabet streams' (dec_small_stream), each
    // stream decoded by exactly one of them
    if (dst == DST_RAW) {
        decode_kernel<0, DST_RAW><<<grid, block, 0, st>>>(b);
        decode_kernel<1, DST_RAW><<<grid, block, 0, st>>>(b);
        decode_kernel<2, DST_RAW><<<grid, block, 0, st>>>(b);
        decode_kernel<0, DST_RAW, true><<<grid, block, 0, st>>>(b);
    } else {
        decode_kernel<0, DST_SYMBOLS><<<grid, block, 0, st>>>(b);
        decode_kernel<1, DST_SYMBOLS><<<grid, block, 0, st>>>(b);
        decode_kernel<2, DST_SYMBOLS><<<grid, block, 0, st>>>(b);
        decode_kernel<0, DST_SYMBOLS, true><<<grid, block, 0, st>>>(b);
    }
    return hipGetLastError();
}

}  // namespace hc

#ifdef HC_DEBUG_HOOKS
extern "C" int hc_debug_set_window(uint32_t bytes)
{
    // a multiple of 256 in [4096, 2^30]: the descriptor windows of every later FGK launch
    uint32_t w = bytes < 4096u ? 4096u : (bytes > (1u << 30) ? (1u << 30) : bytes);
    w &= ~255u;
    return hipMemcpyToSymbol(HIP_SYMBOL(hc::g_window), &w, sizeof(w)) == hipSuccess ? 0 : HC_ERR_DEVICE;
}

extern "C" int hc_debug_set_min_tree(uint32_t kind)
{
    // 0 narrow, 1 wide, 2 huge: the smallest tree layout of every later FGK launch
    hc::g_min_tree = kind > 2 ? 2 : kind;
    return 0;
}

extern "C" int hc_debug_set_dec_small(uint32_t mode)
{
    // 0: by payload rate, 1: the small-alphabet decoder for every narrow stream, 2: for none
    hc::g_dec_small = mode > 2 ? 0 : mode;
    return 0;
}

extern "C" int hc_debug_set_dec_pack(uint32_t max)
{
    // the most codes a decoder batch step takes in every later FGK launch on the current device
    // (a device variable, like the window: other devices keep theirs): 1, 7, or anything else
    // for the build's HC_DEC_PACK
    uint32_t k = max == 1 || max == 7 ? max : (uint32_t)HC_DEC_PACK;
    return hipMemcpyToSymbol(HIP_SYMBOL(hc::g_dec_pack), &k, sizeof(k)) == hipSuccess ? 0 : HC_ERR_DEVICE;
}

extern "C" int hc_debug_set_enc_pack(uint32_t max)
{
    // the most symbols a regular encoder batch step takes in every later FGK launch on the current
    // device (a device variable, like hc_debug_set_dec_pack's): 1, 7, or anything else for the
    // build's HC_ENC_PACK
    uint32_t k = max == 1 || max == 7 ? max : 16u;
    return hipMemcpyToSymbol(HIP_SYMBOL(hc::g_enc_pack), &k, sizeof(k)) == hipSuccess ? 0 : HC_ERR_DEVICE;
}

extern "C" int hc_debug_set_enc_tab(uint32_t mode)
{
    // 0: per stream (sampled alphabet), 1: path cache for every stream, 2: tables for every
    // stream, 3: the small-alphabet kernel for every stream (narrow layout)
    hc::g_enc_tab = mode > 3 ? 0 : mode;
    return 0;
}

extern "C" int hc_debug_enc_votes(const uint8_t *in, const uint64_t *in_offs, const uint64_t *in_lens, uint32_t n,
                                  uint32_t flags, uint32_t low_occ, int32_t *status, void *stream)
{
    // enc_mode_kernel alone: status[i] = the vote (kModeCache -0x7A1 / kModeTables -0x7A0)
    hc::Batch b{};
    b.in = in;
    b.in_offs = in_offs;
    b.in_lens = in_lens;
    b.n = n;
    b.status = status;
    b.flags = flags;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) return 0;
    if (flags & HC_FLAG_DIFF) hc::enc_mode_kernel<hc::SRC_RAW_DIFF><<<(n + 3) / 4, 256, 0, st>>>(b, low_occ, 0u);
    else hc::enc_mode_kernel<hc::SRC_RAW><<<(n + 3) / 4, 256, 0, st>>>(b, low_occ, 0u);
    return hipGetLastError() == hipSuccess ? 0 : HC_ERR_DEVICE;
}

extern "C" int hc_debug_set_trace(void *dev_buf)
{
    uint64_t *p = static_cast<uint64_t *>(dev_buf);
    return hipMemcpyToSymbol(HIP_SYMBOL(hc::g_trace), &p, sizeof(p)) == hipSuccess ? 0 : HC_ERR_DEVICE;
}
#endif  // HC_DEBUG_HOOKS
