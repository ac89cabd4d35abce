// hc_crc.hip — CRC-32 (zlib / IEEE 802.3: reflected polynomial 0xEDB88320, init and final xor
// 0xFFFFFFFF) of many byte ranges in one launch: hc_crc32_batch, and the checksum pass of the
// segmented container (hc_seg.hip).
//
// A CRC state is a polynomial over GF(2) modulo P, bit 31 the coefficient of x^0 (reflected).
// Feeding k zero bits multiplies the state by x^k, and feeding data is linear on top of that:
// state(A || B) = state(A) x^(8 |B|) + raw(B), raw() the CRC with init 0 and no final xor. So a
// range splits into pieces whose raw CRCs are computed side by side and combined by
// multiplications with fixed powers of x:
//
//   a range of more than 64 bytes goes to one wavefront. Its bytes are head (up to the first
//   16-byte boundary) | 16-byte pieces | tail (under 16 bytes). Tiles of 64 pieces, one aligned
//   16-byte load per lane, walk the pieces; the tiles are right-aligned, so the first one is the
//   partial one and lane 63 always ends on the last piece (a raw CRC ignores leading zeros: a lane
//   without a piece adds nothing). Each lane folds acc = acc x^8192 + raw(piece) per tile; the
//   lane that owns piece 0 starts it from the state 0xFFFFFFFF run through the head bytes, which
//   carries the init term along with no power of a variable length anywhere. A six-step
//   shuffle tree with x^128, x^256 ... x^4096 leaves the state after the last piece in lane 63,
//   which runs the tail bytes and stores the result.
//   ranges of up to 64 bytes take one lane each, byte by byte: thousands of tiny segments cost a
//   few wavefronts, not a workgroup each.
//
// The arithmetic is shift / xor in registers. A multiplication by a compile-time constant c
// unrolls to 32 and/xor pairs, bit i of the state selecting the literal c x^i; a 16-byte piece
// is four of those side by side, state(w0 w1 w2 w3) = (s + w0) x^128 + w1 x^96 + w2 x^64 + w3 x^32,
// with no chain between them (feeding the piece bit by bit is a chain of 128 dependent steps:
// 0.093 ms for 256 ranges of 64 KiB against 0.060 ms this way). Only the head,
// tail and short-range bytes go bit by bit. No table in LDS or memory: a byte-indexed table
// lookup is a data-dependent LDS read (64 lanes on random banks), and 16 MiB is tens of
// microseconds of this arithmetic. What bounds it is issue rate: a range is one wavefront, and
// a wavefront alone on its SIMD issues one vector instruction per 4 cycles.
//
// No load touches a byte outside its range: 16-byte loads only on whole aligned pieces inside
// it, single bytes at both ends.
#include "hc_internal.h"

namespace {

constexpr uint32_t kPoly = 0xEDB88320u;
constexpr uint64_t kLaneMax = 64;  // ranges up to this many bytes: one lane each

// one zero bit into the state: times x
__host__ __device__ constexpr uint32_t times_x(uint32_t s) { return (s >> 1) ^ (kPoly & (0u - (s & 1u))); }

// a * b mod P; with a constant b the loop unrolls into and/xor pairs over constants
__host__ __device__ constexpr uint32_t mul_mod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = times_x(b);
    }
    return p;
}

// x^n mod P
constexpr uint32_t x_pow(uint64_t n)
{
    uint32_t v = 0x80000000u, sq = 0x40000000u;  // x^0, x^1
    for (; n; n >>= 1) {
        if (n & 1) v = mul_mod(v, sq);
        sq = mul_mod(sq, sq);
    }
    return v;
}
static_assert(x_pow(1) == 0x40000000u && x_pow(8) == 0x00800000u, "x^8 is eight shifts");
static_assert(x_pow(32) == kPoly, "x^32 = P - x^32 (mod P)");
static_assert(x_pow(96) == mul_mod(x_pow(64), kPoly), "exponents add");

// s x^N: feeding N zero bits at once
template <uint64_t N>
__device__ __forceinline__ uint32_t times_x_pow(uint32_t s)
{
    constexpr uint32_t c = x_pow(N);
    uint32_t p = 0, b = c;
#pragma unroll
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((s >> i) & 1u));
        b = times_x(b);
    }
    return p;
}

__device__ __forceinline__ uint32_t feed_byte(uint32_t s, uint8_t v)
{
    s ^= v;
#pragma unroll
    for (int i = 0; i < 8; ++i) s = times_x(s);
    return s;
}

// sixteen bytes, lowest first: four independent products
__device__ __forceinline__ uint32_t feed_piece(uint32_t s, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3)
{
    return times_x_pow<128>(s ^ w0) ^ times_x_pow<96>(w1) ^ times_x_pow<64>(w2) ^ times_x_pow<32>(w3);
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the whole CRC of p[0 .. len), len > kLaneMax, by one full wavefront; the result is lane 63's
__device__ uint32_t crc_wave(const uint8_t *p, uint64_t len, uint32_t lane)
{
    const uint64_t head = (0 - reinterpret_cast<uintptr_t>(p)) & 15u;  // < len
    const uint64_t pieces = (len - head) / 16;                         // >= 3
    const uint64_t tail = (len - head) & 15u;
    const u32x4 *v = reinterpret_cast<const u32x4 *>(p + head);
    const uint64_t tiles = (pieces + 63) / 64, pad = tiles * 64 - pieces;
    uint32_t acc = 0;
    if (lane >= pad) {  // the first tile, the partial one: lanes below pad have no piece in it
        uint32_t s = 0;
        if (lane == pad) {  // piece 0: the init value through the head bytes
            s = 0xFFFFFFFFu;
            for (uint64_t b = 0; b < head; ++b) s = feed_byte(s, p[b]);
        }
        const u32x4 w = v[lane - pad];
        acc = feed_piece(s, w.x, w.y, w.z, w.w);
    }
    // whole tiles from here on, four loads in flight: one load per tile and wavefront is a
    // memory latency per KiB
    const u32x4 *vt = v + (64 - pad) + lane;
    uint64_t t = 1;
    for (; t + 4 <= tiles; t += 4, vt += 256) {
        const u32x4 w0 = vt[0], w1 = vt[64], w2 = vt[128], w3 = vt[192];
        acc = times_x_pow<8192>(acc) ^ feed_piece(0, w0.x, w0.y, w0.z, w0.w);  // times the tile's 1024 bytes
        acc = times_x_pow<8192>(acc) ^ feed_piece(0, w1.x, w1.y, w1.z, w1.w);
        acc = times_x_pow<8192>(acc) ^ feed_piece(0, w2.x, w2.y, w2.z, w2.w);
        acc = times_x_pow<8192>(acc) ^ feed_piece(0, w3.x, w3.y, w3.z, w3.w);
    }
    for (; t < tiles; ++t, vt += 64) {
        const u32x4 w = *vt;
        acc = times_x_pow<8192>(acc) ^ feed_piece(0, w.x, w.y, w.z, w.w);
    }
    // lanes l - d .. l hold consecutive pieces: the lower half moves up by the upper half's bytes
    uint32_t o;
#define HC_CRC_STEP(D)                                \
    o = __shfl_up(acc, D, 64);                        \
    if (lane >= D) acc ^= times_x_pow<128 * D>(o);
    HC_CRC_STEP(1)
    HC_CRC_STEP(2)
    HC_CRC_STEP(4)
    HC_CRC_STEP(8)
    HC_CRC_STEP(16)
    HC_CRC_STEP(32)
#undef HC_CRC_STEP
    if (lane == 63) {
        const uint8_t *e = p + head + pieces * 16;
        for (uint64_t b = 0; b < tail; ++b) acc = feed_byte(acc, e[b]);
    }
    return ~acc;
}

// gate: the container decoder's conditions (null pointers: every range is taken)
__global__ __launch_bounds__(256) void crc32_kernel(const uint8_t *in, const uint64_t *offs, const uint64_t *lens,
                                                    uint64_t n, uint32_t *crc, hc::CrcGate g)
{
    auto taken = [&](uint64_t i) {
        return !g.status || (g.status[i] == 0 && g.got_lens[i] == lens[i]);
    };
    // short ranges: one lane each
    const uint64_t threads = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += threads) {
        const uint64_t len = lens[i];
        if (len > kLaneMax || !taken(i)) continue;
        const uint8_t *p = in + offs[i];
        uint32_t s = 0xFFFFFFFFu;
        for (uint64_t b = 0; b < len; ++b) s = feed_byte(s, p[b]);
        crc[i] = ~s;
    }
    // the rest: one wavefront each (i is the same in all of a wavefront's lanes)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += waves) {
        const uint64_t len = lens[i];
        if (len <= kLaneMax || !taken(i)) continue;
        const uint32_t c = crc_wave(in + offs[i], len, lane);
        if (lane == 63) crc[i] = c;
    }
}

}  // namespace

namespace hc {

hipError_t launch_crc32(const uint8_t *in, const uint64_t *offs, const uint64_t *lens, uint64_t n, uint32_t *crc,
                        const CrcGate &gate, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 3) / 4;  // a wavefront per range, up to four per SIMD of the chip
    crc32_kernel<<<(uint32_t)(blocks < 1024 ? blocks : 1024), 256, 0, st>>>(in, offs, lens, n, crc, gate);
    return hipGetLastError();
}

}  // namespace hc

extern "C" int hc_crc32_batch(const uint8_t *in, const uint64_t *in_offs, const uint64_t *lens, uint32_t n,
                              uint32_t *crc, void *stream)
{
    if (n == 0) return HC_OK;
    if (!in || !in_offs || !lens || !crc) return HC_ERR_ARG;
    const hc::CrcGate none{nullptr, nullptr};
    return hc::launch_crc32(in, in_offs, lens, n, crc, none, static_cast<hipStream_t>(stream)) == hipSuccess
               ? HC_OK
               : HC_ERR_DEVICE;
}
