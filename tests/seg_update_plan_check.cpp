// seg_update_plan_check — the host's plan of a range write (patches_ok and update_plan of
// huffman-codec_amd/csrc/hc_seg_index.h) as a stand-alone program, so that the walk over an
// untrusted patch list can run under the sanitizers (tests/test_seg_update_model.py builds it
// with -fsanitize=address,undefined). No device, no library: the header alone.
//
//   seg_update_plan_check RAW_LEN SEG_BYTES ADAPT WIDTH DATA_LEN [OFFSET:LENGTH:SRC_OFF ...]
//
// The cuts come from the first four arguments (seg_cuts). Prints "status covered decoded cov_raw
// dec_raw": status 0, or 71 with zeros for cuts or a patch list that fail their rules; then, for
// status 0, one line per patch: "k0 cnt e0 d0 dmask dst". The list and the records live in heap
// blocks of exactly their size, so a read or a write past either is a report, not luck.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hc_seg_index.h"

int main(int argc, char **argv)
{
    if (argc < 6) return 2;
    const uint64_t raw = strtoull(argv[1], nullptr, 10), seg = strtoull(argv[2], nullptr, 10);
    const bool adapt = strtoull(argv[3], nullptr, 10) != 0;
    const uint64_t width = strtoull(argv[4], nullptr, 10), data_len = strtoull(argv[5], nullptr, 10);
    const uint32_t n = (uint32_t)(argc - 6);
    hc_seg_patch_t *p = static_cast<hc_seg_patch_t *>(malloc(n ? n * sizeof(hc_seg_patch_t) : 1));
    hc_seg_index::PatchRec *recs = static_cast<hc_seg_index::PatchRec *>(malloc(n ? n * sizeof(hc_seg_index::PatchRec) : 1));
    if (!p || !recs) return 2;
    for (uint32_t i = 0; i < n; ++i) {
        char *end = nullptr;
        p[i].offset = strtoull(argv[6 + i], &end, 10);
        if (*end != ':') return 2;
        p[i].length = strtoull(end + 1, &end, 10);
        if (*end != ':') return 2;
        p[i].src_off = strtoull(end + 1, &end, 10);
        if (*end) return 2;
    }
    const hc_seg_index::Cuts c = hc_seg_index::seg_cuts(raw, seg, adapt, width);
    if (c.n == 0 || !hc_seg_index::patches_ok(raw, n ? p : nullptr, n, &data_len)) {
        printf("71 0 0 0 0\n");
    } else {
        const hc_seg_index::UpdPlan u = hc_seg_index::update_plan(c, raw, p, n, 16, 16, recs);
        printf("0 %llu %llu %llu %llu\n", (unsigned long long)u.covered, (unsigned long long)u.decoded,
               (unsigned long long)u.cov_raw, (unsigned long long)u.dec_raw);
        if (u.cov_bound != 16 * u.covered) return 3;
        for (uint32_t i = 0; i < n; ++i)
            printf("%llu %llu %llu %llu %llu %llu\n", (unsigned long long)recs[i].k0, (unsigned long long)recs[i].cnt,
                   (unsigned long long)recs[i].e0, (unsigned long long)recs[i].d0, (unsigned long long)recs[i].dmask,
                   (unsigned long long)recs[i].dst);
    }
    free(recs);
    free(p);
    return 0;
}
