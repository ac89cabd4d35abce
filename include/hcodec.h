/*
 * hcodec.h — C ABI of the MI355X-native huffman-codec pipeline (libhcodec.so).
 *
 * Drop-in boundary for dominiksalvet/huffman-codec's codec path. The reference is one C++
 * binary with no library; its replaceable seams are the buffer functions huffCompress /
 * huffDecompress (src/main.cpp:39-87, src/main.cpp:90-128), which main() calls at
 * src/main.cpp:211-215, and the CLI contract around them (src/main.cpp:152-221, reproduced by
 * the `huffman-codec` binary built from huffman-codec_amd/csrc/hc_cli.cpp).
 *
 * Everything here is plain C: pointers and sizes, no torch or HIP types in the signatures
 * (a hipStream_t is passed as void*). Every entry point is re-entrant: no hidden global state.
 * Compute runs on the current HIP device; there is no CPU fallback — without a usable gfx950
 * device every compute entry point returns HC_ERR_DEVICE.
 *
 * Status codes are the reference's process exit codes: the reference calls
 * exit(n) deep inside its library; here n is returned instead, per call or per stream.
 */
#ifndef HCODEC_H
#define HCODEC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum hc_status {
    HC_OK = 0,
    HC_ERR_WIDTH = 4,         /* main.cpp:195-199  width 0 when compressing                  */
    HC_ERR_MATRIX_SIZE = 6,   /* main.cpp:54-58    input size not a multiple of width (-a)   */
    HC_ERR_HEADER = 8,        /* main.cpp:99-104   missing <64b-count><8b-flags> header      */
    HC_ERR_HUFFMAN = 9,       /* transform.cpp:394-398  FGK bits exhausted                   */
    HC_ERR_ADAPT_HEADER = 10, /* headers.cpp:67-71  adaptive header shorter than 24 bytes   */
    HC_ERR_ADAPT_DIRS = 11,   /* headers.cpp:94-98  missing scan-direction bytes             */
    HC_ERR_DIMS = 12,         /* transform.cpp:300-304  width or height < 8 (-a)             */
    HC_ERR_BLOCK_DATA = 13,   /* transform.cpp:178-182  block RLE overshoots its block       */
    HC_ERR_BLOCK_EOF = 14,    /* transform.cpp:170-174  block RLE data ends early            */
    HC_ERR_LEFTOVER = 15,     /* transform.cpp:354-358  bytes left after the last block      */
    /* beyond the reference (it has no equivalent, or crashes) */
    HC_ERR_CAPACITY = 64,     /* output capacity too small; the needed length is reported    */
    HC_ERR_UNSUPPORTED = 65,  /* -a stream given to a non-adaptive entry point or vice versa */
    HC_ERR_BLOCK_SIZE = 66,   /* forged adaptive header, block size 0 (reference: SIGFPE)    */
    HC_ERR_TOO_LARGE = 67,    /* forged adaptive header, W*H > 2^36 (reference: bad_alloc)   */
    HC_ERR_SEG_HEADER = 68,   /* segmented container: bad header, index or length            */
    HC_ERR_SEG_SIZE = 69,     /* segmented container: a segment decodes to another length    */
    HC_ERR_DEVICE = 70,       /* HIP runtime error / no gfx950 device                        */
    HC_ERR_ARG = 71,          /* null pointer, misaligned device buffer, bad flag            */
    HC_ERR_SEG_CHECK = 72     /* segmented container: a segment decodes to its cut's length,
                                 but its checksum differs from the index                    */
};

/* Flags byte of the outer header (headers.cpp:118-122): bit 7 diff model, bit 6 adaptive RLE */
#define HC_FLAG_DIFF 0x80u
#define HC_FLAG_ADAPT 0x40u

/* ---------------------------------------------------------------------------------------
 * Single-buffer API — host buffers, synchronous. Replaces huffCompress (main.cpp:39-87) and
 * huffDecompress (main.cpp:90-128); the input is a byte buffer instead of an ifstream.
 * ------------------------------------------------------------------------------------- */

/* Worst-case compressed size of an in_len-byte input (any mode). */
uint64_t hc_compress_bound(uint64_t in_len, int use_adapt);

/* huffCompress(ifs, useDiffModel, useAdaptRLE, matrixWidth). Writes the whole stream
 * (<u64 LE count><u8 flags><FGK bits>) to out. Returns HC_OK, HC_ERR_WIDTH (width == 0, the
 * CLI check of main.cpp:195-199), HC_ERR_MATRIX_SIZE, HC_ERR_DIMS, HC_ERR_CAPACITY (out_cap <
 * result; *out_len = needed), HC_ERR_DEVICE or HC_ERR_ARG. */
int hc_compress(const uint8_t *in, uint64_t in_len, int use_diff, int use_adapt, uint64_t width,
                uint8_t *out, uint64_t out_cap, uint64_t *out_len);

/* huffDecompress(ifs). Returns HC_OK, 8, 9, 10, 11, 13, 14, 15, HC_ERR_CAPACITY (out_cap too
 * small; *out_len = needed), HC_ERR_BLOCK_SIZE, HC_ERR_TOO_LARGE, HC_ERR_DEVICE or HC_ERR_ARG. */
int hc_decompress(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap,
                  uint64_t *out_len);

/* Same, with the output allocated by the library (release with hc_free). */
int hc_decompress_alloc(const uint8_t *in, uint64_t in_len, uint8_t **out, uint64_t *out_len);
void hc_free(void *p);

/* ---------------------------------------------------------------------------------------
 * Batched device API — many independent streams per call, asynchronous on `stream`
 * (a hipStream_t; NULL = default stream). All pointers are DEVICE pointers. Stream i reads
 * in[in_offs[i] .. +in_lens[i]) and writes out[out_offs[i] .. +out_caps[i]); every
 * in + in_offs[i] and out + out_offs[i] must be 4-byte aligned. Per-stream results land in
 * out_lens[i] (bytes written, or bytes needed on HC_ERR_CAPACITY) and status[i].
 * The return value reports argument / launch errors only.
 * ------------------------------------------------------------------------------------- */

/* Compress n_streams raw streams: [diff model] -> MNP-5 RLE -> FGK -> header, fused in one
 * kernel (one stream per wavefront). flags: 0 or HC_FLAG_DIFF (adaptive streams: the batched
 * adaptive API below). Capacity per stream: hc_compress_bound(in_len, 0) always suffices.
 * The encoder's two modes (see hc_compress_batch_aux) run one after the other on `stream`
 * here: a batch mixing skewed and flat alphabets is faster through hc_compress_batch_aux with
 * a second stream (before round 4 the library ran them on a side stream of its own). */
int hc_compress_batch(const uint8_t *in, const uint64_t *in_offs, const uint64_t *in_lens,
                      uint32_t n_streams, uint32_t flags, uint8_t *out, const uint64_t *out_offs,
                      const uint64_t *out_caps, uint64_t *out_lens, int32_t *status,
                      void *stream);

/* The same, with a second caller-owned HIP stream (or NULL) for the encoder's table-mode
 * launches. Each stream is coded in one of two modes, voted per stream from its alphabet: the
 * path cache (skewed alphabets) or the level tables (flat ones); the two modes are separate
 * launches. With aux_stream they run side by side (forked from and joined back into `stream` by
 * events, also under graph capture), so a batch mixing both kinds fills the GPU with both at once;
 * hc_compress_batch (aux_stream NULL) runs them one after the other on `stream`. The library
 * keeps no stream of its own. */
int hc_compress_batch_aux(const uint8_t *in, const uint64_t *in_offs, const uint64_t *in_lens,
                          uint32_t n_streams, uint32_t flags, uint8_t *out, const uint64_t *out_offs,
                          const uint64_t *out_caps, uint64_t *out_lens, int32_t *status, void *stream,
                          void *aux_stream);

/* Decompress n_streams encoded streams (non-adaptive: a stream whose flags byte has bit 6 set
 * gets HC_ERR_UNSUPPORTED here; use hc_decompress_adapt_batch). FGK -> RLE revert -> [diff revert], fused. */
int hc_decompress_batch(const uint8_t *in, const uint64_t *in_offs, const uint64_t *in_lens,
                        uint32_t n_streams, uint8_t *out, const uint64_t *out_offs,
                        const uint64_t *out_caps, uint64_t *out_lens, int32_t *status,
                        void *stream);

/* ---------------------------------------------------------------------------------------
 * Batched adaptive block RLE (-a) — many W x H matrices per call, asynchronous on `stream`,
 * DEVICE pointers as in the batched API above. huffCompress(ifs, useDiff, true, width)
 * (main.cpp:39-87) for every matrix i = in[in_offs[i] .. +in_lens[i]) of width widths[i]:
 * [diff model] -> adaptive block RLE (transform.cpp:294-328: block-size search, per-block
 * scan order, header) -> FGK -> <u64 count><flags 0x40 | diff> header. Per-stream status:
 * HC_OK, HC_ERR_WIDTH (width 0), HC_ERR_MATRIX_SIZE, HC_ERR_DIMS, HC_ERR_CAPACITY.
 * `work` is device scratch of work_bytes (16-byte aligned), at least
 * hc_adapt_compress_work_bound(sum of in_lens, n_streams); out capacity per stream:
 * hc_compress_bound(in_len, 1) always suffices.
 * ------------------------------------------------------------------------------------- */
uint64_t hc_adapt_compress_work_bound(uint64_t total_in_bytes, uint32_t n_streams);
int hc_compress_adapt_batch(const uint8_t *in, const uint64_t *in_offs, const uint64_t *in_lens,
                            const uint64_t *widths, uint32_t n_streams, uint32_t flags, uint8_t *out,
                            const uint64_t *out_offs, const uint64_t *out_caps, uint64_t *out_lens,
                            int32_t *status, void *work, uint64_t work_bytes, void *stream);

/* huffDecompress (main.cpp:90-128) of adaptive streams (flags bit 6 set; others get
 * HC_ERR_UNSUPPORTED): FGK -> adaptive block revert (transform.cpp:330-361) -> [diff revert].
 * Status: HC_OK, 8, 9, 10, 11, 13, 14, 15, HC_ERR_CAPACITY (out_lens[i] = W * H needed),
 * HC_ERR_BLOCK_SIZE, HC_ERR_TOO_LARGE, HC_ERR_UNSUPPORTED. `work`: at least
 * hc_adapt_decompress_work_bound(sum of in_lens, sum of out_caps, n_streams) bytes. */
uint64_t hc_adapt_decompress_work_bound(uint64_t total_in_bytes, uint64_t total_out_bytes, uint32_t n_streams);
int hc_decompress_adapt_batch(const uint8_t *in, const uint64_t *in_offs, const uint64_t *in_lens,
                              uint32_t n_streams, uint8_t *out, const uint64_t *out_offs,
                              const uint64_t *out_caps, uint64_t *out_lens, int32_t *status, void *work,
                              uint64_t work_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Host-buffer batch API — many independent streams in HOST memory (e.g. files read by the
 * caller), synchronous. Beyond the reference, which codes one file per process
 * (main.cpp:202-220); SURVEY.md §8f-1. The library stages the streams through pinned memory
 * in sub-batches and overlaps each sub-batch's copies and kernels with the next one's (two
 * HIP streams); only produced bytes cross PCIe. Stream i reads in[i][0 .. in_lens[i]) and
 * writes out[i][0 .. out_caps[i]); out_lens[i] / status[i] as in the device batch API
 * (HC_ERR_CAPACITY: out_lens[i] = bytes needed, nothing written). Sub-batch size: the
 * environment variables HC_PIPE_BYTES (input bytes, default 1 GiB) and HC_PIPE_STREAMS
 * (default 8192). The return value reports argument / device errors only.
 * ------------------------------------------------------------------------------------- */

/* flags: 0 or HC_FLAG_DIFF (adaptive: hc_compress_adapt_host_batch). out_caps[i] >=
 * hc_compress_bound(in_lens[i], 0) always suffices. */
int hc_compress_host_batch(const uint8_t *const *in, const uint64_t *in_lens, uint32_t n_streams,
                           uint32_t flags, uint8_t *const *out, const uint64_t *out_caps,
                           uint64_t *out_lens, int32_t *status);

/* The same for adaptive (-a) matrices: huffCompress(ifs, useDiff, true, widths[i]) for every
 * matrix (main.cpp:39-87) through the batched adaptive device API, pipelined in sub-batches
 * like hc_compress_host_batch. Status per stream as hc_compress_adapt_batch. */
int hc_compress_adapt_host_batch(const uint8_t *const *in, const uint64_t *in_lens, const uint64_t *widths,
                                 uint32_t n_streams, uint32_t flags, uint8_t *const *out, const uint64_t *out_caps,
                                 uint64_t *out_lens, int32_t *status);

/* Any streams: adaptive ones (flags bit 6) through the batched adaptive device path, the rest
 * through the FGK -> RLE revert -> [diff revert] path, each kind pipelined in sub-batches. */
int hc_decompress_host_batch(const uint8_t *const *in, const uint64_t *in_lens, uint32_t n_streams,
                             uint8_t *const *out, const uint64_t *out_caps, uint64_t *out_lens,
                             int32_t *status);

/* Device-side packing of many byte ranges into one buffer (e.g. a batch's encoded streams,
 * back to back, before they leave the GPU or cross to rank 0): copies lens[i] bytes from
 * in + in_offs[i] to out + out_offs[i] for every i. Asynchronous on `stream`; ranges must not
 * overlap. Any byte alignment is accepted, of in, out and every offset, and no byte outside the
 * destination ranges is written. No reference counterpart (the reference writes one file per
 * process). */
int hc_pack_batch(const uint8_t *in, const uint64_t *in_offs, const uint64_t *lens, uint32_t n_streams,
                  uint8_t *out, const uint64_t *out_offs, void *stream);

/* ---------------------------------------------------------------------------------------
 * Segmented container (HCSEG1) — one large input coded as many independent segments in one
 * batch launch. A format of this library (the reference has none); opt-in: no other entry point
 * reads or writes it, and a container handed to hc_decompress* gets HC_ERR_HUFFMAN like any
 * stream whose count is above 2^63. All integers little-endian, offsets from the start:
 *
 *   0   8   magic  48 43 53 45 47 31 00 FF ("HCSEG1\0\xFF")
 *   8   1   flags  HC_FLAG_DIFF | HC_FLAG_ADAPT, other bits 0
 *   9   1   check  0 none, 1 CRC-32 per segment; any other value is invalid
 *   10  6   zero
 *   16  8   raw_len     decoded bytes in total
 *   24  8   seg_bytes   the segment size given to the encoder (multiple of 16, >= 16)
 *   32  8   width       adaptive: matrix width; otherwise 0
 *   40  8   n_segments  >= 1
 *   48  8n  enc_len[k]  byte length of segment k's stream
 *   check == 1 only: 4n  crc[k], uint32: the CRC-32 of segment k's raw bytes (the bytes of its
 *               cut, before the diff model) as zlib / IEEE 802.3 define it: reflected polynomial
 *               0xEDB88320, init and final xor 0xFFFFFFFF; of an empty segment, 0
 *   then the segments in order, each at the next multiple of 16 (padding bytes 0); the
 *   container ends with the last byte of the last segment.
 *
 * Segment k is exactly the stream hc_compress writes for segment k's bytes alone with the same
 * options. The cuts are a function of raw_len, seg_bytes, flags and width: plain, segment k is
 * raw bytes [k seg_bytes, min((k+1) seg_bytes, raw_len)), n = max(1, ceil(raw_len / seg_bytes));
 * adaptive, the segments are bands of rows = max(8, floor(seg_bytes / width) & ~3) rows, each
 * coded as its own width x rows matrix, and a band that would leave fewer than 8 rows takes
 * those too.
 *
 * The check is opt-in (HC_SEG_CHECK_CRC32 to the encoders named below): a damaged FGK stream is
 * often still a valid one that decodes to the right length and the wrong bytes. With check == 0
 * the container is what it always was. The decoders take both kinds; in a checked one, a segment
 * that decodes cleanly to its cut's length with another CRC-32 than the index's fails with
 * HC_ERR_SEG_CHECK, by the same lowest-failing-segment rule as every other segment error.
 * ------------------------------------------------------------------------------------- */
#define HC_SEG_DEFAULT_BYTES 65536u
/* Asks the segmented encoders for a checked container. Valid only in the `flags` of
 * hc_seg_compress_bound2, hc_seg_compress_work_bound2, hc_seg_compress2 and hc_seg_compress_dev;
 * hc_seg_info_t.flags reports header byte 9 in bits 8-15, so a checked container has it set. */
#define HC_SEG_CHECK_CRC32 0x100u
typedef struct hc_seg_info_t {
    uint64_t raw_len, seg_bytes, width, n_segments;
    uint32_t flags;
} hc_seg_info_t;

/* Segments of an in_len-byte input (seg_bytes 0: HC_SEG_DEFAULT_BYTES); 0 when the arguments
 * are invalid (seg_bytes not a multiple of 16; adaptive: width 0, in_len not a multiple of
 * width, width or height < 8). */
uint64_t hc_seg_count(uint64_t in_len, uint64_t seg_bytes, int use_adapt, uint64_t width);
/* Worst-case container size (0 when invalid). */
uint64_t hc_seg_compress_bound(uint64_t in_len, uint64_t seg_bytes, int use_adapt, uint64_t width);
/* The same with flags = HC_FLAG_DIFF | HC_FLAG_ADAPT | HC_SEG_CHECK_CRC32 (other bits: 0 is
 * returned); without the check bit, hc_seg_compress_bound's value. */
uint64_t hc_seg_compress_bound2(uint64_t in_len, uint64_t seg_bytes, uint32_t flags, uint64_t width);
/* Host only, no device: parses and checks the 48 header bytes against in_len (every header rule,
 * 48 + 8 n <= in_len (checked: 48 + 12 n), raw_len <= 520 in_len). HC_OK and *info, or
 * HC_ERR_SEG_HEADER. */
int hc_seg_info(const uint8_t *in, uint64_t in_len, hc_seg_info_t *info);

/* Host buffers, synchronous. seg_bytes 0: HC_SEG_DEFAULT_BYTES. Returns HC_ERR_ARG (null
 * pointer, seg_bytes not a multiple of 16), then HC_ERR_WIDTH, HC_ERR_MATRIX_SIZE, HC_ERR_DIMS
 * as hc_compress, HC_ERR_DEVICE, HC_ERR_CAPACITY (*out_len = needed). */
int hc_seg_compress(const uint8_t *in, uint64_t in_len, int use_diff, int use_adapt, uint64_t width,
                    uint64_t seg_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_len);
/* The same with flags = HC_FLAG_DIFF | HC_FLAG_ADAPT | HC_SEG_CHECK_CRC32 (any other bit:
 * HC_ERR_ARG): with the check bit, a checked container. */
int hc_seg_compress2(const uint8_t *in, uint64_t in_len, uint32_t flags, uint64_t width, uint64_t seg_bytes,
                     uint8_t *out, uint64_t out_cap, uint64_t *out_len);
/* HC_ERR_SEG_HEADER (bad container; *out_len = 0), HC_ERR_CAPACITY (*out_len = raw_len), the
 * status of the lowest failing segment with *bad_segment its index (a segment that wants
 * another length than its cut: HC_ERR_SEG_SIZE; in a checked container, one with the right
 * length and another checksum: HC_ERR_SEG_CHECK), or HC_OK. *bad_segment (may be NULL) is
 * UINT64_MAX unless a segment failed. */
int hc_seg_decompress(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap,
                      uint64_t *out_len, uint64_t *bad_segment);
/* Same, with the output allocated by the library (release with hc_free). */
int hc_seg_decompress_alloc(const uint8_t *in, uint64_t in_len, uint8_t **out, uint64_t *out_len,
                            uint64_t *bad_segment);

/* Device buffers, asynchronous on `stream`; in, out and work 16-byte aligned; out_len, status
 * and bad_segment are DEVICE pointers. No allocation, no host synchronisation: every byte of
 * scratch comes from `work`. flags: HC_FLAG_DIFF | HC_FLAG_ADAPT, and for the encoder
 * HC_SEG_CHECK_CRC32 (work_bytes must then reach hc_seg_compress_work_bound2). The return value reports
 * argument / launch errors only (and HC_ERR_WIDTH / _MATRIX_SIZE / _DIMS, decided on the host).
 *
 * The encoder codes every segment into a slot of hc_compress_bound(segment) bytes inside `work`
 * and then gathers the slots into `out`: the slots are bound-sized, not guessed and retried, so
 * the work bound is about 6x the input (plus the adaptive batch workspace for -a). */
uint64_t hc_seg_compress_work_bound(uint64_t in_len, uint64_t seg_bytes, int use_adapt, uint64_t width);
uint64_t hc_seg_compress_work_bound2(uint64_t in_len, uint64_t seg_bytes, uint32_t flags, uint64_t width);
int hc_seg_compress_dev(const uint8_t *in, uint64_t in_len, uint32_t flags, uint64_t width, uint64_t seg_bytes,
                        uint8_t *out, uint64_t out_cap, uint64_t *out_len, int32_t *status,
                        void *work, uint64_t work_bytes, void *stream);
/* The decoder needs the header on the host (hc_seg_info of the first 48 bytes) to size its
 * launches; the device bytes are checked against it. Segments decode in place into `out`. The
 * buffer behind `in` must be readable up to in_len rounded up to a multiple of 4. Both kinds of
 * container go through these two; info must equal the device header, the check kind included. */
uint64_t hc_seg_decompress_work_bound(const hc_seg_info_t *info, uint64_t in_len);
int hc_seg_decompress_dev(const uint8_t *in, uint64_t in_len, const hc_seg_info_t *info,
                          uint8_t *out, uint64_t out_cap, uint64_t *out_len, int32_t *status,
                          uint64_t *bad_segment, void *work, uint64_t work_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Range decode: raw bytes [offset, offset + length) of a container without decoding the rest.
 * The cuts are a function of the header, so the segments that hold a range are known before any
 * payload byte is read; every segment restarts the coder's model, so they decode alone.
 *
 * Covered segments. With n, full and last the container's cuts (segment k is raw bytes
 * [k full, k full + cap_k), cap_k = last for k == n - 1 and full otherwise), a range of
 * length > 0 covers the segments k0 .. k1, k0 = min(offset / full, n - 1) and
 * k1 = min((offset + length - 1) / full, n - 1). (The clamp matters in an adaptive container
 * whose last band took leftover rows: there last > full.) A range of length 0 covers nothing.
 *
 * Range check. The range must lie inside raw_len: offset <= raw_len and length <= raw_len -
 * offset; anything else is HC_ERR_ARG, decided on the host (raw_len is in the host's info). The
 * empty range is valid at every such offset, the empty range of an empty container included.
 *
 * The container-level verdict does not depend on the range: a container that hc_seg_decompress*
 * answers with HC_ERR_SEG_HEADER (the device header against the caller's copy; the index, all
 * 8 n bytes of which are still scanned, must tile [align16(48 + 8 n or 12 n), in_len) exactly)
 * gets that answer for every valid range, the empty one included.
 *
 * Status, in this order:
 *   1  HC_ERR_ARG         null pointers (device call: misaligned buffers)   *out_len, *bad_segment not set
 *   2  HC_ERR_SEG_HEADER  the header fails                                   0, UINT64_MAX
 *   3  HC_ERR_ARG         the range is not inside raw_len                    not set
 *   4  HC_ERR_SEG_HEADER  the index fails                                    0, UINT64_MAX
 *   5  HC_ERR_DEVICE      host call without a device                         0, UINT64_MAX
 *   6  HC_ERR_CAPACITY    out_cap < length                                   length, UINT64_MAX
 *   7  the status of the lowest failing COVERED segment, by hc_seg_decompress's mapping (the
 *      coder's own status; another length than the cut: HC_ERR_SEG_SIZE; in a checked container
 *      the right length with another CRC-32: HC_ERR_SEG_CHECK)               0, its container index
 *   8  HC_OK                                                                 length, UINT64_MAX
 * A damaged segment outside the range is not noticed: that is the contract, not an accident (a
 * ranged read neither reads nor decodes such a segment). Every covered segment is decoded whole,
 * the partially covered first and last ones included, so in a checked container the CRC-32 of
 * every covered segment is verified.
 *
 * Writes. No byte outside out[0 .. length) is written, whatever the status; on a non-zero status
 * the contents of that range are unspecified. out_cap above length is allowed (and need not
 * reach raw_len). The range (0, raw_len) gives exactly what hc_seg_decompress* gives: status,
 * bytes, *out_len and *bad_segment.
 * ------------------------------------------------------------------------------------- */

/* Host only, no device. The segments that hold raw bytes [offset, offset + length) of a container
 * with this info: *first, *count (count 0 when length is 0). HC_OK, or HC_ERR_ARG (null pointer,
 * an info that fails hc_seg_info's rules for in_len, offset > raw_len, length > raw_len - offset). */
int hc_seg_range_segments(const hc_seg_info_t *info, uint64_t in_len, uint64_t offset, uint64_t length,
                          uint64_t *first, uint64_t *count);

/* Host buffers, synchronous: raw bytes [offset, offset + length) of the container into out[0 .. length).
 * The header and the index are checked on the host (HC_ERR_SEG_HEADER needs no device); only the
 * header, the index and the encoded bytes of the covered segments are uploaded, the device buffers
 * are sized by those and by length, and only length bytes come back. bad_segment may be NULL. */
int hc_seg_decompress_range(const uint8_t *in, uint64_t in_len, uint64_t offset, uint64_t length,
                            uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *bad_segment);

/* Device buffers, asynchronous on `stream`, under the rules of hc_seg_decompress_dev: in, out and
 * work 16-byte aligned; out_len, status and bad_segment DEVICE pointers; no allocation, no host
 * synchronisation, no host read of device memory. `in` holds the whole container (of which the
 * header, the index and the covered segments are read). An info that fails hc_seg_info's rules
 * gets HC_ERR_SEG_HEADER as the device status; a range outside raw_len and work_bytes below the
 * bound are HC_ERR_ARG.
 *
 * All covered segments decode in one launch. One that lies wholly inside the range decodes in
 * place at out + (k full - offset) when offset is a multiple of 4 (the coders need a 4-byte
 * aligned output, and full is a multiple of 4). Every other one is staged: it decodes into a slot
 * of align16(max(full, last)) bytes inside `work`, and its covered part is then copied to out at
 * any byte alignment. So the bound holds, for an offset that is a multiple of 4, one slot for each
 * partly covered edge segment (at most two; none when the range starts and ends on cuts), and one
 * slot per covered segment otherwise; plus 44 bytes (checked: 48) per covered segment, not per
 * segment of the container, 24 per slot, and for -a the adaptive batch workspace of the covered
 * segments (hc_adapt_decompress_work_bound(in_len, their raw bytes, their count)). For the range
 * (0, raw_len) of a non-empty container that is hc_seg_decompress_work_bound's value, and the call
 * launches what hc_seg_decompress_dev launches.
 * hc_seg_decompress_range_work_bound: 0 for a null info or a range outside raw_len, 16 for an
 * info that fails the rules (as hc_seg_decompress_work_bound). */
uint64_t hc_seg_decompress_range_work_bound(const hc_seg_info_t *info, uint64_t in_len,
                                            uint64_t offset, uint64_t length);
int hc_seg_decompress_range_dev(const uint8_t *in, uint64_t in_len, const hc_seg_info_t *info,
                                uint64_t offset, uint64_t length, uint8_t *out, uint64_t out_cap,
                                uint64_t *out_len, int32_t *status, uint64_t *bad_segment,
                                void *work, uint64_t work_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Range write: the container with some raw byte ranges overwritten, without recoding the rest.
 * Segment k is the stream hc_compress writes for segment k's bytes alone and the cuts are a
 * function of the header, so a write that keeps raw_len keeps n, the header and the index size:
 * only the segments that the new bytes touch are coded again, and every other stream is carried
 * over byte for byte. raw_len never changes (no truncation; appending is hc_seg_append's).
 *
 * Patches. A call takes a list: patch i makes raw bytes [offset, offset + length) of the container
 * patch_data[src_off .. src_off + length). `patches` is HOST memory, read before the call returns
 * and never after (the list travels as kernel arguments, in chunks, so a call can be captured in a
 * graph). Every patch must lie inside raw_len (offset <= raw_len and length <= raw_len - offset);
 * the patches must be sorted by offset and must not overlap (patches[i+1].offset >=
 * patches[i].offset + patches[i].length); every [src_off, src_off + length) must lie inside
 * patch_data_len. Anything else is HC_ERR_ARG, decided on the host. A patch of length 0 is valid
 * at any offset inside raw_len and touches nothing; n_patches == 0 is valid.
 *
 * Covered and decoded segments. A patch of length > 0 covers the segments that a range read of its
 * bytes covers (the rule above, clamp to n - 1 included); the covered set of a call is the union
 * over its patches. A covered segment whose whole cut lies inside ONE patch is coded from the patch
 * alone: its old stream is neither read nor decoded, so overwriting a damaged segment repairs it.
 * Every other covered segment is decoded whole (and, in a checked container, verified against the
 * index's CRC-32, as the range decoder does), has the patch bytes laid over it and is coded again.
 * The rule is per patch: two adjacent patches that together fill a cut still decode it.
 *
 * Result. On HC_OK out[0 .. *out_len) is the container with the same 48 header bytes; enc_len[k]
 * (checked: and crc[k], the CRC-32 of the segment's new raw bytes, before the diff model) replaced
 * for the covered segments and kept for the others; segment k's stream replaced, for a covered
 * segment, by the stream hc_compress writes for its cut's new bytes with the container's flags and
 * width, and copied verbatim for every other one (a damaged uncovered segment is not noticed, as
 * in a ranged read); every segment at the next multiple of 16 after the one before, with padding 0
 * after the recoded segments. For a container that this library wrote that is byte for byte what
 * hc_seg_compress2 gives for the patched raw input with the same flags (check bit included), width
 * and seg_bytes; with no patch of length > 0 it is the input container.
 *
 * Status, in this order (host call):
 *   1  HC_ERR_ARG         null pointers (device call: in, out or work not 16-byte aligned; [in,
 *                         in + in_len) and [out, out + out_cap) overlap)    *out_len, *bad_segment not set
 *   2  HC_ERR_SEG_HEADER  the header fails                                   0, UINT64_MAX
 *   3  HC_ERR_ARG         the patch list fails its rules (device call: work_bytes below the bound;
 *                         more than 2^31 - 1 covered segments)              not set
 *   4  HC_ERR_SEG_HEADER  the index fails: all n entries are scanned and must tile the container
 *                         exactly, whatever the patches, the empty list included   0, UINT64_MAX
 *   5  HC_ERR_DEVICE      host call without a device                         0, UINT64_MAX
 *   6  the status of the lowest failing DECODED segment, by hc_seg_decompress's mapping (the
 *      coder's own status; another length than the cut: HC_ERR_SEG_SIZE; in a checked container
 *      the right length with another CRC-32: HC_ERR_SEG_CHECK)               0, its container index
 *   7  HC_ERR_CAPACITY    the new container is longer than out_cap           the length needed, UINT64_MAX
 *   8  HC_OK                                                                 the new length, UINT64_MAX
 * Row 6 comes before row 7, unlike the range decoder: the needed length is known only after the
 * covered segments are coded, and means nothing when one of them could not be decoded.
 *
 * Writes. No byte outside out[0 .. out_cap) is written, whatever the status, and on a non-zero
 * status no byte of out is written at all.
 * ------------------------------------------------------------------------------------- */
typedef struct hc_seg_patch_t {
    uint64_t offset, length; /* raw bytes [offset, offset + length) of the container ...        */
    uint64_t src_off;        /* ... become patch_data[src_off .. src_off + length)              */
} hc_seg_patch_t;

/* Host only, no device. *n_covered, *n_decoded: the segments the call codes again, and those among
 * them that it decodes first. HC_OK, or HC_ERR_ARG (a null pointer, an info that fails hc_seg_info's
 * rules for in_len, a patch list that fails the rules above; src_off is not looked at). */
int hc_seg_update_segments(const hc_seg_info_t *info, uint64_t in_len, const hc_seg_patch_t *patches,
                           uint32_t n_patches, uint64_t *n_covered, uint64_t *n_decoded);
/* An out_cap that always suffices: in_len plus the sum over the covered segments of
 * a16(hc_compress_bound(cut, adaptive)). 0 for arguments that the call refuses. */
uint64_t hc_seg_update_bound(const hc_seg_info_t *info, uint64_t in_len, const hc_seg_patch_t *patches,
                             uint32_t n_patches);
/* The device call's workspace. With P = n_patches, C the covered and D the decoded segments, R and
 * W their raw bytes, S the sum of a16(hc_compress_bound(cut, adaptive)) over the covered segments
 * and a16(x) = x rounded up to a multiple of 16:
 *   a16(64 P) + 3 a16(8 P) + 6 a16(8 D) + a16(4 D) + 9 a16(8 C) + a16(4 C) + 3 a16(8 (2 C + 1)) + 32
 *   [+ a16(4 D) + a16(4 C) checked] + a16(R) + S
 *   [+ a16(max(hc_adapt_compress_work_bound(R, C) if C > 0, hc_adapt_decompress_work_bound(in_len,
 *      W, D) if D > 0)) adaptive]
 * It grows with the patches and with the segments they cover, never with n. 0 for a null info, a
 * patch list that fails the rules or more than 2^31 - 1 covered segments; 16 for an info that
 * fails hc_seg_info's rules (as hc_seg_decompress_work_bound). */
uint64_t hc_seg_update_work_bound(const hc_seg_info_t *info, uint64_t in_len, const hc_seg_patch_t *patches,
                                  uint32_t n_patches);

/* Device buffers, asynchronous on `stream`, under the rules of hc_seg_decompress_range_dev: in,
 * out and work 16-byte aligned; out_len, status and bad_segment (may be NULL) DEVICE pointers; no
 * device allocation, no host synchronisation, no host read of device memory, every byte of scratch
 * from `work`. patch_data is a DEVICE pointer of any byte alignment, and so is every src_off. Rows 1
 * and 3 are the return value; an info that fails hc_seg_info's rules gives HC_ERR_SEG_HEADER as the
 * device status with return value HC_OK; everything else is the device status.
 *
 * Covered segment c (in container order) keeps its raw bytes at c full of a staging region in
 * `work`: the decoded ones decode straight into it, one pack launch lays every patch's bytes over
 * it, and one encode launch codes the covered segments into bound-sized slots. The new container
 * is then spliced from the old one's uncovered runs and the slots, 16 bytes per lane. */
int hc_seg_update_dev(const uint8_t *in, uint64_t in_len, const hc_seg_info_t *info,
                      const hc_seg_patch_t *patches, uint32_t n_patches,
                      const uint8_t *patch_data, uint64_t patch_data_len,
                      uint8_t *out, uint64_t out_cap, uint64_t *out_len, int32_t *status,
                      uint64_t *bad_segment, void *work, uint64_t work_bytes, void *stream);

/* Host buffers, synchronous. The header, the patch list and the index are checked on the host
 * (rows 2 - 4 need no device); then the container and the patch bytes are uploaded, the device call
 * runs on the cached scratch of the single calls, and *out_len bytes come back. bad_segment may be
 * NULL. */
int hc_seg_update(const uint8_t *in, uint64_t in_len, const hc_seg_patch_t *patches, uint32_t n_patches,
                  const uint8_t *patch_data, uint64_t patch_data_len,
                  uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *bad_segment);

/* ---------------------------------------------------------------------------------------
 * List read: many raw byte ranges of one container in one call, each covered segment decoded
 * once. The read mirror of the range write: a tile of an image is one read per row, and the rows
 * that share a segment share its one decode, its one CRC-32 and its one place in the workspace.
 *
 * Reads. A call takes a list: read i copies raw bytes [offset, offset + length) of the container to
 * out[dst_off .. dst_off + length). `reads` is HOST memory, read before the call returns and never
 * after (the list travels as kernel arguments, in chunks, so a call can be captured in a graph).
 * Every read must lie inside raw_len (offset <= raw_len and length <= raw_len - offset); the reads
 * must be sorted by offset (reads[i+1].offset >= reads[i].offset); no dst_off + length may wrap.
 * Anything else is HC_ERR_ARG, decided on the host. Source ranges MAY overlap or repeat: this is a
 * read. A read of length 0 is valid at any offset inside raw_len and touches nothing; n_reads == 0 is
 * valid. Destination ranges must not overlap one another: that is the caller's duty, as in
 * hc_pack_batch, and it is not checked. They may come in any order, at any byte alignment, with gaps
 * between them. need is the highest dst_off + length over the reads of length > 0, 0 when there is
 * none.
 *
 * Covered segments. A read of length > 0 covers the segments that hc_seg_range_segments names for its
 * range (clamp to n - 1 included); a call covers the union over its reads, C segments. Each covered
 * segment is decoded whole exactly once, however many reads name it, and in a checked container
 * verified against the index's CRC-32 once. A damaged segment that no read covers is not noticed, as
 * in every ranged read.
 *
 * Status, in this order (the range decoder's):
 *   1  HC_ERR_ARG         null pointers (device call: in, out or work not 16-byte aligned)
 *                                                                            *out_len, *bad_segment not set
 *   2  HC_ERR_SEG_HEADER  the header fails                                   0, UINT64_MAX
 *   3  HC_ERR_ARG         the list fails its rules (device call: work_bytes below the bound; more
 *                         than 2^31 - 1 covered segments)                    not set
 *   4  HC_ERR_SEG_HEADER  the index fails: all n entries are scanned once and must tile the container
 *                         exactly, whatever the list, the empty one included   0, UINT64_MAX
 *   5  HC_ERR_DEVICE      host call without a device                         0, UINT64_MAX
 *   6  HC_ERR_CAPACITY    out_cap < need                                     need, UINT64_MAX
 *   7  the status of the lowest failing COVERED segment in container order, by hc_seg_decompress's
 *      mapping (the coder's own status; another length than the cut: HC_ERR_SEG_SIZE; in a checked
 *      container the right length with another CRC-32: HC_ERR_SEG_CHECK)     0, its container index
 *   8  HC_OK                                                                 need, UINT64_MAX
 *
 * Writes. No byte outside the union of the destination ranges is written, whatever the status; on a
 * non-zero status the contents of those ranges are unspecified. A list of the one read (o, m, 0)
 * gives exactly what hc_seg_decompress_range* gives for (o, m) with the same out_cap: status, bytes,
 * *out_len and *bad_segment (the work bound and the launches may differ).
 * ------------------------------------------------------------------------------------- */
typedef struct hc_seg_read_t {
    uint64_t offset, length; /* raw bytes [offset, offset + length) of the container ...   */
    uint64_t dst_off;        /* ... go to out[dst_off .. dst_off + length)                  */
} hc_seg_read_t;

/* Host only, no device. *n_covered = C, the segments the call decodes; *need as above. HC_OK, or
 * HC_ERR_ARG (a null pointer, an info that fails hc_seg_info's rules for in_len, a list that fails
 * the rules above). */
int hc_seg_reads_segments(const hc_seg_info_t *info, uint64_t in_len, const hc_seg_read_t *reads,
                          uint32_t n_reads, uint64_t *n_covered, uint64_t *need);
/* The device call's workspace. With P = n_reads, C the covered segments, W their raw bytes and
 * a16(x) = x rounded up to a multiple of 16:
 *   a16(48 P) + 3 a16(8 P) + 6 a16(8 C) + a16(4 C) + 16 [+ a16(4 C) checked] + a16(W)
 *   [+ a16(hc_adapt_decompress_work_bound(in_len, W, C)) adaptive, C > 0]
 * It grows with the reads and with the segments they cover, never with n or with how often a
 * segment is named. 0 for a null info, a list that fails the rules or more than 2^31 - 1 covered
 * segments; 16 for an info that fails hc_seg_info's rules (as hc_seg_decompress_work_bound). */
uint64_t hc_seg_decompress_ranges_work_bound(const hc_seg_info_t *info, uint64_t in_len,
                                             const hc_seg_read_t *reads, uint32_t n_reads);

/* Device buffers, asynchronous on `stream`, under the rules of hc_seg_update_dev: in, out and work
 * 16-byte aligned; out_len, status and bad_segment (may be NULL) DEVICE pointers; no device
 * allocation, no host synchronisation, no host read of device memory, every byte of scratch from
 * `work`; capturable in a graph. `in` holds the whole container (of which the header, the index and
 * the covered segments are read). Rows 1 and 3 are the return value; an info that fails
 * hc_seg_info's rules gives HC_ERR_SEG_HEADER as the device status with return value HC_OK;
 * everything else is the device status.
 *
 * Covered segment c (in container order) decodes whole to c full of a staging region in `work`, all
 * of them in one launch. A read's covered segments are consecutive there and only segment n - 1,
 * the last entry when it is covered, has another length than full, so read i's bytes are one run of
 * that region, and one pack launch copies every run to out + dst_off at any byte alignment. The
 * index is scanned by one workgroup, once. */
int hc_seg_decompress_ranges_dev(const uint8_t *in, uint64_t in_len, const hc_seg_info_t *info,
                                 const hc_seg_read_t *reads, uint32_t n_reads, uint8_t *out, uint64_t out_cap,
                                 uint64_t *out_len, int32_t *status, uint64_t *bad_segment,
                                 void *work, uint64_t work_bytes, void *stream);

/* Host buffers, synchronous. The header, the list and the index are checked on the host (rows 2 - 4
 * need no device); the header, the index and the encoded bytes from the first covered segment's
 * stream to the last covered one's are uploaded, never the whole container when the reads cover part
 * of it; the device call runs on the cached scratch of the single calls; the destination bytes
 * [0, need) come down and are copied into out read by read, so no byte outside the destination
 * ranges is written on the host either. bad_segment may be NULL. */
int hc_seg_decompress_ranges(const uint8_t *in, uint64_t in_len, const hc_seg_read_t *reads, uint32_t n_reads,
                             uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *bad_segment);

/* Host only, no device: the rows of a rectangle as a read list. Of a raw buffer of raw_len bytes read
 * as rows of `pitch` bytes, row r of the w x h rectangle at column x, row y is bytes
 * [(y + r) pitch + x, + w), and goes to dst_off r w: reads[r], h entries, sorted. HC_ERR_ARG for a null
 * `reads` with h > 0, pitch == 0, x + w > pitch, any product or sum that wraps, and, when w and h are
 * not 0, (y + h - 1) pitch + x + w > raw_len; HC_OK otherwise. w == 0 gives h empty reads (which the
 * read calls still hold to offset <= raw_len). */
int hc_seg_rect_reads(uint64_t raw_len, uint64_t pitch, uint64_t x, uint64_t y, uint64_t w, uint64_t h,
                      hc_seg_read_t *reads /* h entries */);

/* ---------------------------------------------------------------------------------------
 * Append: the container of X followed by T from the container of X, without recoding the rest. The cuts are
 * a function of raw_len, seg_bytes, flags and width, every segment restarts the coder's model and
 * segment k is the stream hc_compress writes for its cut alone: so when bytes are appended, every
 * segment below the old last one keeps its cut and its stream, at most one old segment (the partly
 * filled last one) is decoded, and only that one and the new ones are coded.
 *
 * Notation. n, full, last: the old container's cuts; R its raw_len; T the appended bytes, A their
 * length; R' = R + A; n', last': the cuts of R' with the same seg_bytes, flags and width (full does
 * not change, and n' >= n).
 *
 * First coded segment K. K = n when A == 0, and when old cut n - 1 equals new cut n - 1, i.e. the
 * last segment was already a complete cut of the shape of one that is not the last (plain: R a
 * non-zero multiple of seg_bytes; adaptive: the last band has exactly `rows` rows and at least 8
 * rows are appended). Otherwise K = n - 1.
 *
 * Segments 0 .. K - 1 are kept: their streams are neither decoded nor checked, so a damaged kept
 * segment is not noticed, as in a ranged read. Segments K .. n' - 1 are coded: they hold raw bytes
 * [K full, R'), the old open tail [K full, R) followed by T. The open tail is empty when K == n. An
 * adaptive open tail can be longer than `full` and end up in two new segments (width 16, seg_bytes
 * 128, 19 rows + 5 rows: the old last band of 11 rows becomes bands of 8 and 8), and it can be the
 * whole container (15 rows + 1 row: one segment becomes two).
 *
 * Decoded segment. When K == n - 1 and last > 0, old segment n - 1 is decoded whole first, and
 * judged by hc_seg_decompress's mapping: the coder's own status; another length than its cut:
 * HC_ERR_SEG_SIZE; in a checked container the right length with another CRC-32: HC_ERR_SEG_CHECK.
 * The empty segment of an empty container (last == 0) is not read or decoded.
 *
 * Arguments decided on the host: R + A wraps: HC_ERR_ARG; an adaptive container and A no multiple
 * of width: HC_ERR_MATRIX_SIZE; more than 2^31 - 1 coded segments (counted once the other two
 * pass): HC_ERR_ARG. A == 0 is valid: the result is the input container, byte for byte.
 *
 * Result. out[0 .. *out_len) is: the 48 header bytes with raw_len = R' and n_segments = n';
 * enc_len[0 .. K) copied and enc_len[K .. n') new; in a checked container crc[0 .. K) copied to
 * their new place at 48 + 8 n' and crc[K .. n') the CRC-32 of the new cuts' raw bytes; zero padding
 * up to align16 of the index end; the old bytes from segment 0's first byte to segment K - 1's
 * last, copied verbatim as one block (old padding between kept segments included; the block moves
 * by a multiple of 16); then every coded segment at the next multiple of 16, with zero padding
 * after the kept block and after every coded segment but the last. For a container that this
 * library wrote from raw bytes X that is byte for byte what hc_seg_compress2 gives for X followed by T with
 * the same flags (check bit included), width and seg_bytes.
 *
 * Status, in this order (host call):
 *   1  HC_ERR_ARG         null pointers (device call: in, out or work not 16-byte aligned; [in,
 *                         in + in_len) and [out, out + out_cap) overlap)    *out_len, *bad_segment not set
 *   2  HC_ERR_SEG_HEADER  the header fails                                   0, UINT64_MAX
 *   3  HC_ERR_ARG, HC_ERR_MATRIX_SIZE  the argument rules above (device call: work_bytes below the
 *                         bound)                                             not set
 *   4  HC_ERR_SEG_HEADER  the index fails: all n entries are scanned and must tile the container
 *                         exactly, for every A, 0 included                   0, UINT64_MAX
 *   5  HC_ERR_DEVICE      host call without a device                         0, UINT64_MAX
 *   6  the decoded segment's failing status, by the mapping above            0, n - 1
 *   7  HC_ERR_CAPACITY    the result is longer than out_cap                  the length needed, UINT64_MAX
 *   8  HC_OK                                                                 the new length, UINT64_MAX
 * Row 6 comes before row 7, as in hc_seg_update, for the same reason.
 *
 * Writes. No byte outside out[0 .. out_cap) is written, whatever the status, and on a non-zero
 * status no byte of out is written at all.
 * ------------------------------------------------------------------------------------- */

/* Host only, no device. *new_info: the header of the result (raw_len and n_segments new);
 * *first_coded = K; *n_decoded: 0 or 1. HC_OK, HC_ERR_ARG (a null pointer, an info that fails
 * hc_seg_info's rules for in_len, R + A wraps) or HC_ERR_MATRIX_SIZE. */
int hc_seg_append_plan(const hc_seg_info_t *info, uint64_t in_len, uint64_t add_len,
                       hc_seg_info_t *new_info, uint64_t *first_coded, uint64_t *n_decoded);
/* An out_cap that always suffices: in_len + a16((8, checked: 12) (n' - n)) + 16 + S, with S the sum
 * of a16(hc_compress_bound(cut, adaptive)) over the coded segments. 0 for arguments that the call
 * refuses. */
uint64_t hc_seg_append_bound(const hc_seg_info_t *info, uint64_t in_len, uint64_t add_len);
/* The device call's workspace. With C = n' - K the coded segments, D the decoded one (0 or 1), S as
 * above and a16(x) = x rounded up to a multiple of 16:
 *   9 a16(8 C) + a16(4 C) + 3 a16(8 (2 C + 1)) + 160 [+ a16(4 C) + 16 checked]
 *   + a16(O + A) + S, O the open tail's bytes (R - K full; 0 when K == n)
 *   [+ a16(max(hc_adapt_compress_work_bound(O + A, C) if C > 0,
 *              hc_adapt_decompress_work_bound(min(in_len, hc_compress_bound(last, 1)), last, 1) if D > 0))
 *      adaptive]
 * It grows with the open tail and with A, never with n or with the kept bytes. (The adaptive
 * decoder's part is sized by the longest stream this library writes for the decoded cut. A forged
 * stream that announces more symbols than fit it fails as HC_ERR_SEG_SIZE.) 0 for a null info or
 * arguments that the call refuses; 16 for an info that fails hc_seg_info's rules (as
 * hc_seg_update_work_bound). */
uint64_t hc_seg_append_work_bound(const hc_seg_info_t *info, uint64_t in_len, uint64_t add_len);

/* Device buffers, asynchronous on `stream`, under the rules of hc_seg_update_dev: in, out and work
 * 16-byte aligned; out_len, status and bad_segment (may be NULL) DEVICE pointers; no device
 * allocation, no host synchronisation, no host read of device memory, every byte of scratch from
 * `work`; capturable in a graph. `add` is a DEVICE pointer of any byte alignment. Rows 1 and 3 are
 * the return value; an info that fails hc_seg_info's rules gives HC_ERR_SEG_HEADER as the device
 * status with return value HC_OK; everything else is the device status.
 *
 * The coded segments' raw bytes lie in a staging region of `work`: the decoded segment decodes to
 * its start, one pack launch lays T behind it (one range per coded segment), and one encode launch
 * codes them into bound-sized slots. The new container is then spliced from the kept block and the
 * slots, 16 bytes per lane, and the new index is written in front of them. */
int hc_seg_append_dev(const uint8_t *in, uint64_t in_len, const hc_seg_info_t *info,
                      const uint8_t *add, uint64_t add_len, uint8_t *out, uint64_t out_cap,
                      uint64_t *out_len, int32_t *status, uint64_t *bad_segment,
                      void *work, uint64_t work_bytes, void *stream);

/* Host buffers, synchronous. The header, the arguments and the index are checked on the host (rows
 * 2 - 4 need no device). The kept bytes never cross to the device: only the header, the index, the
 * decoded segment's stream and T are uploaded; the same stages run on the cached scratch of the
 * single calls; the verdict, the coded segments' index words and their streams, gathered back to
 * back, come down, and the result is put together on the host with the kept block taken from `in`.
 * Device memory and transfers grow with the index, the open tail and A, not with the kept bytes.
 * bad_segment may be NULL. */
int hc_seg_append(const uint8_t *in, uint64_t in_len, const uint8_t *add, uint64_t add_len,
                  uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *bad_segment);

/* ---------------------------------------------------------------------------------------
 * Batches of containers: many inputs, or many (container, range) pairs, in one call whose
 * launches do not grow with the number of items (a directory of mid-sized files; a viewer that
 * fetches many regions of one large image). A launch of the coders takes about as long as its
 * longest segment's serial chain whatever it holds, so n items in one launch cost about one.
 *
 * An encoder item is one input; a decoder item is one container and one range of it, or the whole
 * (length == HC_SEG_WHOLE with offset 0: exactly hc_seg_decompress_dev, an empty container's one
 * empty segment included). The same container may be named by several decoder items. One decode
 * call may mix plain, -m, adaptive, checked and unchecked containers: they describe themselves.
 * The encoder's flags and seg_bytes hold for the whole call; width is per item: 0 is
 * HC_ERR_WIDTH as in every encoder, and any other value is read only with HC_FLAG_ADAPT.
 *
 * The equivalence rule: for every item, the bytes written, out_lens[i], status[i] and
 * bad_segments[i] are exactly what hc_seg_compress_dev, hc_seg_decompress_dev or
 * hc_seg_decompress_range_dev gives for that item alone with the same arguments, by the
 * precedence documented for those calls. What such a call reports through its return value for a
 * reason that belongs to the item goes to status[i] instead: HC_ERR_WIDTH, HC_ERR_MATRIX_SIZE,
 * HC_ERR_DIMS, a range outside raw_len (HC_ERR_ARG), an info that fails the rules
 * (HC_ERR_SEG_HEADER); then out_lens[i] = 0, bad_segments[i] = UINT64_MAX, and the item launches
 * nothing and touches no output byte. Items are independent: a damaged segment, too small an
 * out_cap or a bad header changes nothing about any other item. No byte is written outside
 * out[out_off .. out_off + out_cap) of an item, and for a decoder item none outside its first
 * `length` bytes, whatever the status. Output ranges must not overlap; input ranges may.
 *
 * Memory. `items` is HOST memory, read before the call returns and never after (the descriptors
 * travel as kernel arguments, so a call can be captured in a graph). in, out, work, out_lens,
 * status and bad_segments (may be NULL) are DEVICE pointers; in, out, work and every in_off /
 * out_off are 16-byte aligned. As in the single calls: asynchronous on `stream`, no allocation, no
 * host synchronisation, no host read of device memory, every byte of scratch from `work`.
 *
 * The return value reports call-level errors only, and then nothing is launched or written:
 * HC_ERR_ARG for a null pointer, a misaligned base or offset, a flag outside HC_FLAG_DIFF |
 * HC_FLAG_ADAPT | HC_SEG_CHECK_CRC32, seg_bytes not a multiple of 16, work_bytes below the bound,
 * or more than 2^31 - 1 segments in the call (in any one container, for the decoder);
 * HC_ERR_DEVICE for a launch error. n_items == 0 does nothing and returns HC_OK.
 *
 * Work bounds (0 for arguments that the call refuses), a16(x) = x rounded up to a multiple of 16.
 * Encoder, over the items whose width / length pass hc_compress's checks, with N their segments
 * in total (hc_seg_count), S the sum of a16(hc_compress_bound(segment, adapt)) over those
 * segments and R the sum of their in_len:
 *   7 a16(8 N) + a16(4 N) [+ a16(4 N) checked] + 16 + S
 *   [+ a16(hc_adapt_compress_work_bound(R, N)) adaptive, N > 0]
 *   + a16(112 n_items) + a16(4 N) + a16(8 n_items)
 * Decoder, over the items whose info and range pass, with C their covered segments in total (a
 * whole item: all n), L their staging slots and B the slots' bytes as the range bound above
 * counts them per item, and for the adaptive items E the sum of in_len, W the raw bytes of their
 * covered segments and A their count:
 *   5 a16(8 C) + 2 a16(4 C) + a16(8 n_items) + a16(176 n_items) + 3 a16(8 L) + B
 *   [+ a16(hc_adapt_decompress_work_bound(E, W, A)) when A > 0]
 * Both grow with every item added and are at least the single call's bound for each item.
 * ------------------------------------------------------------------------------------- */
#define HC_SEG_WHOLE UINT64_MAX
typedef struct hc_seg_enc_item_t {
    uint64_t in_off, in_len; /* the input: in[in_off .. in_off + in_len) */
    uint64_t width;          /* the matrix width (HC_FLAG_ADAPT only) */
    uint64_t out_off, out_cap;
} hc_seg_enc_item_t;
typedef struct hc_seg_dec_item_t {
    uint64_t in_off, in_len; /* the container: in[in_off .. in_off + in_len) */
    hc_seg_info_t info;      /* hc_seg_info of its first 48 bytes, from the host */
    uint64_t offset, length; /* the range, or 0 and HC_SEG_WHOLE */
    uint64_t out_off, out_cap;
} hc_seg_dec_item_t;

uint64_t hc_seg_compress_batch_work_bound(const hc_seg_enc_item_t *items, uint32_t n_items, uint32_t flags,
                                          uint64_t seg_bytes);
int hc_seg_compress_batch_dev(const uint8_t *in, uint8_t *out, const hc_seg_enc_item_t *items, uint32_t n_items,
                              uint32_t flags, uint64_t seg_bytes, uint64_t *out_lens, int32_t *status,
                              void *work, uint64_t work_bytes, void *stream);
uint64_t hc_seg_decompress_batch_work_bound(const hc_seg_dec_item_t *items, uint32_t n_items);
int hc_seg_decompress_batch_dev(const uint8_t *in, uint8_t *out, const hc_seg_dec_item_t *items, uint32_t n_items,
                                uint64_t *out_lens, int32_t *status, uint64_t *bad_segments,
                                void *work, uint64_t work_bytes, void *stream);

/* Host buffers, synchronous: item i reads in[i][0 .. in_lens[i]) and writes out[i][0 .. out_caps[i]).
 * The items go to the device in sub-batches of at most HC_PIPE_BYTES uploaded bytes (the host-buffer
 * batch API's variable; an item above it goes alone), one device call per sub-batch on the cached
 * scratch of the single calls. status[i], out_lens[i] and bad_segments[i] (may be NULL) are what
 * hc_seg_compress2, hc_seg_decompress or hc_seg_decompress_range reports for item i alone, its
 * return value as status[i] (HC_ERR_DEVICE without a device included; out_lens[i] is 0 where that
 * call leaves *out_len unset). offsets and lengths both NULL: every item whole; an item with
 * lengths[i] == HC_SEG_WHOLE and offsets[i] == 0 is whole too. A ranged item keeps
 * hc_seg_decompress_range's properties: its index is checked on the host, only the header, the
 * index and the covered segments' bytes are uploaded, and only `length` bytes come back. The
 * return value: HC_ERR_ARG (a null array, one of offsets / lengths alone, a bad flag, seg_bytes
 * not a multiple of 16, too many segments) or HC_ERR_DEVICE (a HIP error), else HC_OK. */
int hc_seg_compress_host_batch(const uint8_t *const *in, const uint64_t *in_lens, const uint64_t *widths,
                               uint32_t n_items, uint32_t flags, uint64_t seg_bytes, uint8_t *const *out,
                               const uint64_t *out_caps, uint64_t *out_lens, int32_t *status);
int hc_seg_decompress_host_batch(const uint8_t *const *in, const uint64_t *in_lens, const uint64_t *offsets,
                                 const uint64_t *lengths, uint32_t n_items, uint8_t *const *out,
                                 const uint64_t *out_caps, uint64_t *out_lens, int32_t *status,
                                 uint64_t *bad_segments);

/* CRC-32 (zlib's crc32: reflected polynomial 0xEDB88320, init and final xor 0xFFFFFFFF) of
 * n_ranges byte ranges, the kernel behind the checked container: crc[i] of in[in_offs[i] ..
 * +lens[i]). DEVICE pointers, asynchronous on `stream`; any alignment, any length (0: crc 0), any
 * n_ranges (0: nothing is done). No byte outside a range is read. */
int hc_crc32_batch(const uint8_t *in, const uint64_t *in_offs, const uint64_t *lens, uint32_t n_ranges,
                   uint32_t *crc, void *stream);

/* Allocation caches. The single-buffer API keeps device scratch between calls (per device,
 * at most 1 GiB each) and the host-buffer batch API keeps its pipeline buffers (per device;
 * above HC_PIPE_KEEP_BYTES, default 8 GiB, of device buffers they are freed at the end of the
 * call). These cache memory only: no result depends on them and concurrent calls never share a
 * buffer. hc_release_cached() frees every cached buffer not in use by a running call (e.g.
 * before handing the memory to another allocator). */
void hc_release_cached(void);

/* Library version string and a device check (1 = a gfx950 device is usable). */
const char *hc_version(void);
int hc_device_ok(void);
/* Human-readable device / runtime description (or the HIP error that prevents one) into buf;
 * returns hc_device_ok(). */
int hc_device_info(char *buf, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* HCODEC_H */
