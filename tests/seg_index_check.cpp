// seg_index_check — the host's header and index scan of the segmented container
// (huffman-codec_amd/csrc/hc_seg_index.h) as a stand-alone program, so that the parser of
// untrusted lengths can run under the sanitizers (tests/test_seg_range_model.py builds it with
// -fsanitize=address,undefined). No device, no library: the header alone.
//
//   seg_index_check [OFFSET:LENGTH | all] FILE ...
//
// A range argument holds for the files after it ("all", the default: the container's whole
// raw_len). One line per FILE, "name status first count s0 s1": status 0, 68 (header or index) or
// 71 (the range is not inside raw_len), the covered segments and their encoded bytes [s0, s1);
// zeros after a non-zero status. Every file is copied into a heap block of exactly its length,
// so a read past the container's end is a report, not luck.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "hc_seg_index.h"

int main(int argc, char **argv)
{
    bool all = true;
    uint64_t offset = 0, length = 0;
    for (int a = 1; a < argc; ++a) {
        const std::string arg = argv[a];
        const size_t colon = arg.find(':');
        if (arg == "all") {
            all = true;
            continue;
        }
        if (colon != std::string::npos && arg.find_first_not_of("0123456789:") == std::string::npos) {
            all = false;
            offset = strtoull(arg.c_str(), nullptr, 10);
            length = strtoull(arg.c_str() + colon + 1, nullptr, 10);
            continue;
        }
        std::ifstream ifs(arg, std::ios::in | std::ios::binary);
        if (ifs.fail()) {
            fprintf(stderr, "%s: cannot read\n", arg.c_str());
            return 2;
        }
        const std::vector<char> bytes((std::istreambuf_iterator<char>(ifs)), std::istreambuf_iterator<char>());
        const uint64_t n = bytes.size();
        uint8_t *in = static_cast<uint8_t *>(malloc(n ? n : 1));  // exactly the container: no slack behind it
        if (!in) return 2;
        if (n) memcpy(in, bytes.data(), n);
        hc_seg_info_t info;
        int status = hc_seg_index::parse_header(in, n, &info);
        uint64_t first = 0, count = 0, s0 = 0, s1 = 0;
        if (status == HC_OK) {
            const uint64_t off = all ? 0 : offset, len = all ? info.raw_len : length;
            hc_seg_index::Cuts c;
            (void)hc_seg_index::info_ok(info, n, c);
            if (!hc_seg_index::range_ok(info.raw_len, off, len)) {
                status = HC_ERR_ARG;
            } else {
                const hc_seg_index::Cover cv = hc_seg_index::range_cover(c, off, len);
                status = hc_seg_index::index_scan(in, n, c.n, hc_seg_index::checked(info.flags), cv, &s0, &s1);
                first = cv.k0;
                count = cv.count;
            }
            if (status != HC_OK) first = count = s0 = s1 = 0;
        }
        free(in);
        const size_t slash = arg.find_last_of('/');
        printf("%s %d %llu %llu %llu %llu\n", (slash == std::string::npos ? arg : arg.substr(slash + 1)).c_str(), status,
               (unsigned long long)first, (unsigned long long)count, (unsigned long long)s0, (unsigned long long)s1);
    }
    return 0;
}
