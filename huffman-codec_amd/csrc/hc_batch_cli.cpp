// hc_batch_cli.cpp — `huffman-codec-batch`: many files per process through the pipelined
// host-batch API of include/hcodec.h (the reference codes one file per
// process, main.cpp:202-220). Each output is byte-identical to what `huffman-codec` (and the
// reference) writes for that file alone.
//
//   huffman-codec-batch [-c | -d [-r OFFSET:LENGTH | -R X:Y:W:H]] [-m] [-a [-w WIDTH]] [-s BYTES [-k]] [-o OUTDIR] [-j THREADS] FILE...
//   huffman-codec-batch -u OFFSET:PATCHFILE [-u ...] [-o OUTDIR] [-j THREADS] FILE...
//   huffman-codec-batch -e TAILFILE [-o OUTDIR] [-j THREADS] FILE...
//
// Compression writes FILE.huf, decompression FILE without its .huf suffix (else FILE.out);
// with -o into OUTDIR under the same base name. Files are read and written by a pool of
// THREADS host threads (default 8). All files go through the pipelined host-batch API in one
// call: hc_compress_host_batch, hc_compress_adapt_host_batch (-a: one matrix of width WIDTH per
// file) or hc_decompress_host_batch (any mix of adaptive and plain streams). A file that fails reports
// "FILE: <the reference's message>"; the exit code is the first failing status (0: all ok).
//
// -s BYTES with -c writes every FILE.huf as a segmented container (HCSEG1, hcodec.h) of BYTES-byte
// segments (0: the default size), all files in one hc_seg_compress_host_batch call; -k (only with
// -s) adds a CRC-32 per segment. -d tells containers from plain streams by their first 8 bytes and
// sends them, all in one call, through hc_seg_decompress_host_batch, which verifies the checksums of
// a container that has them; a failing segment reports "FILE: segment K: <message>".
//
// -r OFFSET:LENGTH with -d writes raw bytes [OFFSET, OFFSET + LENGTH) alone, under the same output
// name, through the same call: only the segments that hold the range are uploaded and
// decoded. Every FILE must then be a container; another one reports "FILE: -r needs a segmented
// container" and counts as HC_ERR_UNSUPPORTED (65). A range outside a container is HC_ERR_ARG (71).
//
// -R X:Y:W:H with -d writes the W x H rectangle at column X, row Y of the raw bytes read as rows of
// PITCH bytes: the W * H bytes of its rows, back to back, under the same output name. PITCH is the
// container's width when it is adaptive, otherwise -w (default 512). The rows are one read list of
// hc_seg_decompress_ranges: each segment that holds rows of the rectangle is uploaded and decoded once.
// Messages and exit codes follow -r: a FILE that is no container reports "FILE: -R needs a
// segmented container" (65), a rectangle outside a container is HC_ERR_ARG (71). -R is given once,
// with -d and without -r.
//
// -u OFFSET:PATCHFILE overwrites the raw bytes from OFFSET on with PATCHFILE's bytes in every FILE,
// each a container, through hc_seg_update: only the segments that the new bytes touch are coded
// again. It writes FILE.upd (with -o OUTDIR/<base name>.upd) and never touches FILE. Several -u are
// sorted by offset before the call; patches that overlap, or that reach past a container's raw
// bytes, are HC_ERR_ARG (71). A FILE that is no container reports "FILE: -u needs a segmented
// container" (65); a segment that must be decoded and fails reports "FILE: segment K: <message>".
// -u goes with none of -c, -d, -m, -a, -s, -k and -r.
//
// -e TAILFILE appends TAILFILE's bytes to the raw bytes of every FILE, each a container, through
// hc_seg_append: only the partly filled last segment and the new ones are coded, and the bytes of
// every other segment never leave the host. It writes FILE.app (with -o OUTDIR/<base name>.app) and
// never touches FILE. Exit codes and messages follow -u: a FILE that is no container reports "FILE:
// -e needs a segmented container" (65); an adaptive container whose width does not divide the tail
// is HC_ERR_MATRIX_SIZE (6); a last segment that must be decoded and fails reports "FILE: segment K:
// <message>". -e is given once and goes with none of -c, -d, -m, -a, -s, -k, -r and -u.
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <thread>
#include <vector>

#include "hc_messages.h"
#include "hcodec.h"

namespace {

const char *const kHelp =
    "USAGE:\n"
    "  huffman-codec-batch [-cm] [-s BYTES [-k]] [-o OUTDIR] [-j THREADS] FILE...\n"
    "  huffman-codec-batch [-cm] -a [-w WIDTH] [-s BYTES [-k]] [-o OUTDIR] [-j THREADS] FILE...\n"
    "  huffman-codec-batch -d [-r OFFSET:LENGTH] [-o OUTDIR] [-j THREADS] FILE... | -h\n"
    "  huffman-codec-batch -d -R X:Y:W:H [-w PITCH] [-o OUTDIR] [-j THREADS] FILE...\n"
    "  huffman-codec-batch -u OFFSET:PATCHFILE [-u ...] [-o OUTDIR] [-j THREADS] FILE...\n"
    "  huffman-codec-batch -e TAILFILE [-o OUTDIR] [-j THREADS] FILE...\n"
    "\n"
    "OPTION:\n"
    "  -c/-d  perform compression/decompression\n"
    "  -m     use differential model for preprocessing\n"
    "  -a     use adaptive block RLE (default: RLE)\n"
    "  -w     width of 2D data (default: 512)\n"
    "  -s     write segmented containers of BYTES-byte segments (0: 65536)\n"
    "  -k     with -s: store a CRC-32 of every segment, verified by -d\n"
    "  -r     with -d: write only raw bytes [OFFSET, OFFSET + LENGTH) of every FILE,\n"
    "         each a segmented container\n"
    "  -R     with -d: write only the W x H rectangle at column X, row Y of every FILE, each a\n"
    "         segmented container; rows of PITCH bytes (an adaptive container's own width, else -w)\n"
    "  -u     overwrite the raw bytes from OFFSET on with PATCHFILE's bytes in every FILE,\n"
    "         each a segmented container; only the segments touched are coded again\n"
    "  -e     append TAILFILE's bytes to the raw bytes of every FILE, each a segmented\n"
    "         container; only the open last segment and the new ones are coded\n"
    "  -o     output directory (default: next to each input)\n"
    "  -j     file I/O threads (default: 8)\n"
    "  -h     show this help\n"
    "OUTPUT:\n"
    "  -c: FILE.huf   -d: FILE without .huf (else FILE.out)   -u: FILE.upd   -e: FILE.app\n";

std::string base_name(const std::string &p)
{
    const size_t k = p.find_last_of('/');
    return k == std::string::npos ? p : p.substr(k + 1);
}

std::string out_path(const std::string &in, bool compress, bool update, bool append, const std::string &dir)
{
    std::string name = dir.empty() ? in : dir + "/" + base_name(in);
    if (update) return name + ".upd";
    if (append) return name + ".app";
    if (compress) return name + ".huf";
    if (name.size() > 4 && name.compare(name.size() - 4, 4, ".huf") == 0) return name.substr(0, name.size() - 4);
    return name + ".out";
}

// run f(i) for i in [0, n) on `threads` host threads
// `count` decimal numbers with ':' between them and nothing else
bool parse_numbers(const char *arg, uint64_t *v, int count)
{
    int k = 0;
    bool digits = false;
    v[0] = 0;
    for (const char *p = arg; *p; ++p) {
        if (*p == ':' && k + 1 < count && digits) {
            v[++k] = 0;
            digits = false;
            continue;
        }
        if (*p < '0' || *p > '9') return false;
        const uint64_t d = (uint64_t)(*p - '0');
        if (v[k] > (UINT64_MAX - d) / 10) return false;
        v[k] = v[k] * 10 + d;
        digits = true;
    }
    return k == count - 1 && digits;
}

// "OFFSET:LENGTH", both decimal and nothing else
bool parse_range(const char *arg, uint64_t &offset, uint64_t &length)
{
    uint64_t v[2];
    if (!parse_numbers(arg, v, 2)) return false;
    offset = v[0];
    length = v[1];
    return true;
}

// "OFFSET:PATCHFILE", the offset decimal and the path not empty
bool parse_patch(const char *arg, uint64_t &offset, std::string &path)
{
    uint64_t v = 0;
    const char *p = arg;
    for (; *p >= '0' && *p <= '9'; ++p) {
        const uint64_t d = (uint64_t)(*p - '0');
        if (v > (UINT64_MAX - d) / 10) return false;
        v = v * 10 + d;
    }
    if (p == arg || *p != ':' || !p[1]) return false;
    offset = v;
    path = p + 1;
    return true;
}

template <class F>
void parallel(size_t n, unsigned threads, F &&f)
{
    std::atomic<size_t> next{0};
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < std::max(1u, threads); ++t)
        pool.emplace_back([&] {
            for (size_t i; (i = next++) < n;) f(i);
        });
    for (auto &th : pool) th.join();
}

}  // namespace

int main(int argc, char *argv[])
{
    bool compress = true, use_diff = false, use_adapt = false, segmented = false, check = false, ranged = false;
    bool update = false, coding_option = false;  // -u; any of -c -d -m -a -s -k -r, which -u goes with none of
    std::vector<std::pair<uint64_t, std::string>> patch_args;  // -u: (offset, patch file)
    bool rect = false;      // -R
    uint64_t rc_xywh[4] = {0, 0, 0, 0};
    bool append = false;    // -e
    std::string tail_path;  // -e: the file whose bytes are appended
    uint64_t seg_bytes = 0, r_offset = 0, r_length = 0;
    std::string dir;
    uint64_t width = 512;
    unsigned threads = 8;
    int opt;
    while ((opt = getopt(argc, argv, ":cdmaw:s:kr:R:u:e:o:j:h")) != -1) {
        switch (opt) {
        case 'c': compress = true; break;
        case 'd': compress = false; break;
        case 'm': use_diff = true; break;
        case 'a': use_adapt = true; break;
        case 'w': width = std::stoull(optarg); break;
        case 's':
            segmented = true;
            seg_bytes = std::stoull(optarg);
            break;
        case 'k': check = true; break;
        case 'r':
            ranged = true;
            if (!parse_range(optarg, r_offset, r_length)) {
                std::cerr << "ERROR: unrecognized option used\n";
                return 2;
            }
            break;
        case 'R':
            if (rect || !parse_numbers(optarg, rc_xywh, 4)) {  // one rectangle
                std::cerr << "ERROR: unrecognized option used\n";
                return 2;
            }
            rect = true;
            break;
        case 'u': {
            update = true;
            uint64_t o = 0;
            std::string path;
            if (!parse_patch(optarg, o, path)) {
                std::cerr << "ERROR: unrecognized option used\n";
                return 2;
            }
            patch_args.emplace_back(o, path);
            break;
        }
        case 'e':
            if (append || !*optarg) {  // one tail, and a path
                std::cerr << "ERROR: unrecognized option used\n";
                return 2;
            }
            append = true;
            tail_path = optarg;
            break;
        case 'o': dir = optarg; break;
        case 'j': threads = (unsigned)std::stoul(optarg); break;
        case 'h': std::cout << kHelp; return 0;
        case ':': std::cerr << "ERROR: missing additional argument\n"; return 1;
        case '?': std::cerr << "ERROR: unrecognized option used\n"; return 2;
        }
        if (opt == 'c' || opt == 'd' || opt == 'm' || opt == 'a' || opt == 's' || opt == 'k' || opt == 'r' || opt == 'R')
            coding_option = true;
    }
    if ((update || append) && (coding_option || (update && append))) {  // a container describes itself: there is nothing to choose
        std::cerr << "ERROR: unrecognized option used\n";
        return 2;
    }
    if (check && !(compress && segmented)) {  // a checksum has nowhere to go but a container's index
        std::cerr << "ERROR: unrecognized option used\n";
        return 2;
    }
    if (ranged && compress) {  // a range is read, never written
        std::cerr << "ERROR: unrecognized option used\n";
        return 2;
    }
    if (rect && (compress || ranged)) {  // so is a rectangle, and it is a range list of its own
        std::cerr << "ERROR: unrecognized option used\n";
        return 2;
    }
    std::vector<std::string> files(argv + optind, argv + argc);
    if (files.empty()) {
        std::cerr << "ERROR: no input file path provided\n";
        return 3;
    }
    if (compress && width == 0) {
        std::cerr << "ERROR: invalid 2D data width\n";
        return 4;
    }
    const size_t n = files.size();
    std::vector<std::vector<uint8_t>> in(n), out(n);
    std::vector<int> status(n, 0);
    std::vector<uint64_t> bad_seg(n, UINT64_MAX);  // the failing segment of a container
    parallel(n, threads, [&](size_t i) {
        std::ifstream ifs(files[i], std::ios::in | std::ios::binary);
        if (ifs.fail()) {
            status[i] = 5;  // main.cpp:205-208
            return;
        }
        in[i].assign(std::istreambuf_iterator<char>(ifs), std::istreambuf_iterator<char>());
    });

    if (update) {
        // the patches sorted by offset, their bytes back to back
        std::stable_sort(patch_args.begin(), patch_args.end(),
                         [](const auto &a, const auto &b) { return a.first < b.first; });
        std::vector<hc_seg_patch_t> patches;
        std::vector<uint8_t> data;
        for (const auto &pa : patch_args) {
            std::ifstream ifs(pa.second, std::ios::in | std::ios::binary);
            if (ifs.fail()) {
                std::cerr << pa.second << ": ERROR: given input file does not exist\n";
                return 5;
            }
            const std::vector<char> bytes((std::istreambuf_iterator<char>(ifs)), std::istreambuf_iterator<char>());
            patches.push_back(hc_seg_patch_t{pa.first, bytes.size(), data.size()});
            data.insert(data.end(), bytes.begin(), bytes.end());
        }
        static const uint8_t kSegMagic[8] = {0x48, 0x43, 0x53, 0x45, 0x47, 0x31, 0x00, 0xFF};
        for (size_t i = 0; i < n; ++i) {
            if (status[i]) continue;
            if (in[i].size() < 8 || !std::equal(kSegMagic, kSegMagic + 8, in[i].begin())) {
                status[i] = -2;  // reported below as HC_ERR_UNSUPPORTED
                continue;
            }
            hc_seg_info_t info;
            uint64_t cap = 0, len = 0;
            if (hc_seg_info(in[i].data(), in[i].size(), &info) == HC_OK)
                cap = hc_seg_update_bound(&info, in[i].size(), patches.data(), (uint32_t)patches.size());
            out[i].resize(cap ? cap : 1);  // (0: the call refuses the header or the patches, and says which)
            status[i] = hc_seg_update(in[i].data(), in[i].size(), patches.data(), (uint32_t)patches.size(), data.data(),
                                      data.size(), out[i].data(), cap, &len, &bad_seg[i]);
            out[i].resize(status[i] ? 0 : len);
        }
    } else if (append) {
        std::ifstream tfs(tail_path, std::ios::in | std::ios::binary);
        if (tfs.fail()) {
            std::cerr << tail_path << ": ERROR: given input file does not exist\n";
            return 5;
        }
        const std::vector<uint8_t> tail((std::istreambuf_iterator<char>(tfs)), std::istreambuf_iterator<char>());
        static const uint8_t kSegMagic[8] = {0x48, 0x43, 0x53, 0x45, 0x47, 0x31, 0x00, 0xFF};
        for (size_t i = 0; i < n; ++i) {
            if (status[i]) continue;
            if (in[i].size() < 8 || !std::equal(kSegMagic, kSegMagic + 8, in[i].begin())) {
                status[i] = -3;  // reported below as HC_ERR_UNSUPPORTED
                continue;
            }
            hc_seg_info_t info;
            uint64_t cap = 0, len = 0;
            if (hc_seg_info(in[i].data(), in[i].size(), &info) == HC_OK) cap = hc_seg_append_bound(&info, in[i].size(), tail.size());
            out[i].resize(cap ? cap : 1);  // (0: the call refuses the header or the tail's length, and says which)
            status[i] = hc_seg_append(in[i].data(), in[i].size(), tail.data(), tail.size(), out[i].data(), cap, &len,
                                      &bad_seg[i]);
            out[i].resize(status[i] ? 0 : len);
        }
    } else if (rect) {
        static const uint8_t kSegMagic[8] = {0x48, 0x43, 0x53, 0x45, 0x47, 0x31, 0x00, 0xFF};
        const uint64_t x = rc_xywh[0], y = rc_xywh[1], w = rc_xywh[2], h = rc_xywh[3];
        for (size_t i = 0; i < n; ++i) {
            if (status[i]) continue;
            if (in[i].size() < 8 || !std::equal(kSegMagic, kSegMagic + 8, in[i].begin())) {
                status[i] = -4;  // reported below as HC_ERR_UNSUPPORTED
                continue;
            }
            hc_seg_info_t info;
            status[i] = hc_seg_info(in[i].data(), in[i].size(), &info);
            if (status[i]) continue;
            // one read per row (none for a rectangle without bytes, once its place is checked)
            const uint64_t pitch = (info.flags & HC_FLAG_ADAPT) ? info.width : width;
            const uint64_t rows = w ? h : 0;
            std::vector<hc_seg_read_t> reads;
            if (rows > UINT32_MAX) status[i] = HC_ERR_ARG;
            else {
                reads.resize(rows);
                status[i] = hc_seg_rect_reads(info.raw_len, pitch, x, y, w, rows, reads.data());
            }
            if (status[i]) continue;
            uint64_t len = 0;
            out[i].resize(std::max<uint64_t>(w * rows, 1));
            status[i] = hc_seg_decompress_ranges(in[i].data(), in[i].size(), reads.data(), (uint32_t)rows, out[i].data(),
                                                 w * rows, &len, &bad_seg[i]);
            out[i].resize(status[i] ? 0 : len);
        }
    } else if (compress && segmented) {  // one container per file, all files in one call
        const uint32_t fl = (use_diff ? HC_FLAG_DIFF : 0u) | (use_adapt ? HC_FLAG_ADAPT : 0u) |
                            (check ? HC_SEG_CHECK_CRC32 : 0u);
        std::vector<size_t> batch;
        for (size_t i = 0; i < n; ++i)
            if (!status[i]) batch.push_back(i);
        const size_t m = batch.size();
        std::vector<const uint8_t *> ip(m);
        std::vector<uint8_t *> op(m);
        std::vector<uint64_t> il(m), oc(m), ol(m, 0), wd(m, width);
        std::vector<int32_t> st(m, 0);
        for (size_t k = 0; k < m; ++k) {
            const size_t i = batch[k];
            out[i].resize(hc_seg_compress_bound2(in[i].size(), seg_bytes, fl, width));
            ip[k] = in[i].data();
            il[k] = in[i].size();
            op[k] = out[i].data();
            oc[k] = out[i].size();
        }
        // a call-level refusal (a segment size that is no multiple of 16) is every file's status
        const int rc = hc_seg_compress_host_batch(ip.data(), il.data(), wd.data(), (uint32_t)m, fl, seg_bytes, op.data(),
                                                  oc.data(), ol.data(), st.data());
        for (size_t k = 0; k < m; ++k) {
            const size_t i = batch[k];
            status[i] = rc ? rc : st[k];
            out[i].resize(status[i] ? 0 : ol[k]);
        }
    } else if (compress) {  // -a: one matrix of width `width` per file
        std::vector<const uint8_t *> ip(n);
        std::vector<uint8_t *> op(n);
        std::vector<uint64_t> il(n), oc(n), ol(n), wd(n, width);
        std::vector<int32_t> st(n, 0);
        for (size_t i = 0; i < n; ++i) {
            ip[i] = in[i].data();
            il[i] = status[i] ? 0 : in[i].size();
            out[i].resize(hc_compress_bound(il[i], use_adapt));
            op[i] = out[i].data();
            oc[i] = out[i].size();
        }
        const uint32_t fl = use_diff ? HC_FLAG_DIFF : 0;
        const int rc = use_adapt ? hc_compress_adapt_host_batch(ip.data(), il.data(), wd.data(), (uint32_t)n, fl,
                                                                op.data(), oc.data(), ol.data(), st.data())
                                 : hc_compress_host_batch(ip.data(), il.data(), (uint32_t)n, fl, op.data(), oc.data(),
                                                          ol.data(), st.data());
        if (rc) {
            std::cerr << hc_status_message(rc);
            return rc;
        }
        for (size_t i = 0; i < n; ++i) {
            if (!status[i]) status[i] = st[i];
            out[i].resize(status[i] ? 0 : ol[i]);
        }
    } else {
        // one batch (adaptive and plain streams alike), whose output sizes are unknown up
        // front: a guess, then the exact size for those that report it
        static const uint8_t kSegMagic[8] = {0x48, 0x43, 0x53, 0x45, 0x47, 0x31, 0x00, 0xFF};
        std::vector<size_t> batch, segs;
        for (size_t i = 0; i < n; ++i) {
            if (status[i]) continue;
            if (in[i].size() < 8 || !std::equal(kSegMagic, kSegMagic + 8, in[i].begin())) {
                if (ranged) status[i] = -1;  // reported below as HC_ERR_UNSUPPORTED
                else batch.push_back(i);
                continue;
            }
            segs.push_back(i);  // a segmented container
        }
        // all containers in one call, each whole or at the range. A whole output is sized like a plain
        // stream's: a guess first, the header's raw_len only for a container whose header and index
        // passed and that reports the guess too small
        for (int pass = 0; pass < 2 && !segs.empty(); ++pass) {
            const size_t m = segs.size();
            std::vector<const uint8_t *> ip(m);
            std::vector<uint8_t *> op(m);
            // (-r 0:2^64-1 is a range outside every container, not the batch call's "whole" item: one
            // byte less is as far outside)
            const uint64_t len = r_length == HC_SEG_WHOLE ? r_length - 1 : r_length;
            std::vector<uint64_t> il(m), oc(m), ol(m, 0), bs(m, UINT64_MAX), ro(m, r_offset), rl(m, len);
            std::vector<int32_t> st(m, 0);
            for (size_t k = 0; k < m; ++k) {
                const size_t i = segs[k];
                hc_seg_info_t info;
                il[k] = in[i].size();
                if (ranged) out[i].resize(std::min<uint64_t>(r_length, 520 * il[k]));  // (no container decodes to more)
                else if (pass == 0 && hc_seg_info(in[i].data(), il[k], &info) == HC_OK)
                    out[i].resize(std::min<uint64_t>(info.raw_len, std::max<uint64_t>(il[k] * 8, 65536)));
                ip[k] = in[i].data();
                op[k] = out[i].data();
                oc[k] = out[i].size();
            }
            const int rc = hc_seg_decompress_host_batch(ip.data(), il.data(), ranged ? ro.data() : nullptr,
                                                        ranged ? rl.data() : nullptr, (uint32_t)m, op.data(), oc.data(),
                                                        ol.data(), st.data(), bs.data());
            std::vector<size_t> again;
            for (size_t k = 0; k < m; ++k) {
                const size_t i = segs[k];
                if (!rc && !ranged && st[k] == HC_ERR_CAPACITY && pass == 0) {
                    out[i].resize(ol[k]);
                    again.push_back(i);
                    continue;
                }
                status[i] = rc ? rc : st[k];
                if (!rc) bad_seg[i] = bs[k];
                out[i].resize(status[i] ? 0 : ol[k]);
            }
            segs.swap(again);
        }
        for (int pass = 0; pass < 2 && !batch.empty(); ++pass) {
            const size_t m = batch.size();
            std::vector<const uint8_t *> ip(m);
            std::vector<uint8_t *> op(m);
            std::vector<uint64_t> il(m), oc(m), ol(m);
            std::vector<int32_t> st(m, 0);
            for (size_t k = 0; k < m; ++k) {
                const size_t i = batch[k];
                ip[k] = in[i].data();
                il[k] = in[i].size();
                if (pass == 0) out[i].resize(std::max<uint64_t>(il[k] * 8, 65536));
                op[k] = out[i].data();
                oc[k] = out[i].size();
            }
            const int rc = hc_decompress_host_batch(ip.data(), il.data(), (uint32_t)m, op.data(), oc.data(), ol.data(),
                                                    st.data());
            if (rc) {
                std::cerr << hc_status_message(rc);
                return rc;
            }
            std::vector<size_t> again;
            for (size_t k = 0; k < m; ++k) {
                const size_t i = batch[k];
                if (st[k] == HC_ERR_CAPACITY && pass == 0) {
                    out[i].resize(ol[k]);
                    again.push_back(i);
                    continue;
                }
                status[i] = st[k];
                out[i].resize(st[k] ? 0 : ol[k]);
            }
            batch.swap(again);
        }
    }

    std::atomic<int> first_fail{0};
    std::vector<std::string> msgs(n);
    parallel(n, threads, [&](size_t i) {
        if (status[i] == 5) {
            msgs[i] = files[i] + ": ERROR: given input file does not exist\n";
            return;
        }
        if (status[i] <= -1 && status[i] >= -4) {
            msgs[i] = files[i] + (status[i] == -1 ? ": -r" : status[i] == -2 ? ": -u" : status[i] == -3 ? ": -e" : ": -R") +
                      " needs a segmented container\n";
            status[i] = HC_ERR_UNSUPPORTED;
            return;
        }
        if (status[i]) {
            msgs[i] = files[i] + ": " + (bad_seg[i] != UINT64_MAX ? "segment " + std::to_string(bad_seg[i]) + ": " : "") +
                      hc_status_message(status[i]);
            return;
        }
        const std::string op = out_path(files[i], compress, update, append, dir);
        std::ofstream ofs(op, std::ios::out | std::ios::binary);
        if (ofs.fail()) {
            status[i] = 7;  // main.cpp:132-144
            msgs[i] = files[i] + ": ERROR: cannot write to " + op + " output file\n";
            return;
        }
        ofs.write(reinterpret_cast<const char *>(out[i].data()), (std::streamsize)out[i].size());
    });
    uint64_t in_bytes = 0, out_bytes = 0, ok = 0;
    for (size_t i = 0; i < n; ++i) {
        if (status[i]) {
            std::cerr << msgs[i];
            int z = 0;
            first_fail.compare_exchange_strong(z, status[i]);
            continue;
        }
        ++ok;
        in_bytes += in[i].size();
        out_bytes += out[i].size();
    }
    std::cerr << "coded " << ok << " of " << n << " files, " << in_bytes << " -> " << out_bytes << " bytes\n";
    return first_fail.load();
}
