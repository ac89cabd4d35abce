// seg_reads_plan_check — the host's plan of a list read (reads_ok, reads_plan, reads_work_base and
// rect_reads of huffman-codec_amd/csrc/hc_seg_index.h) as a stand-alone program, so that the walk
// over an untrusted read list can run under the sanitizers (tests/test_seg_reads_model.py builds it
// with -fsanitize=address,undefined). No device, no library: the header alone.
//
//   seg_reads_plan_check RAW_LEN SEG_BYTES ADAPT WIDTH [OFFSET:LENGTH:DST_OFF ...]
//   seg_reads_plan_check rect RAW_LEN PITCH X Y W H
//
// The cuts come from the first four arguments (seg_cuts). Prints "status covered cov_raw need k_lo
// k_hi base": status 0, or 71 with zeros for cuts or a read list that fail their rules; base is the
// work bound without the adaptive workspace, of an unchecked container. Then, for status 0, one line
// per read: "k0 cnt e0 src length dst_off". The rect form prints "status h", then one line "offset
// length dst_off" per row. The lists and the records live in heap blocks of exactly their size, so a
// read or a write past either is a report, not luck.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hc_seg_index.h"

typedef unsigned long long ull;

static int rect(int argc, char **argv)
{
    if (argc != 8) return 2;
    uint64_t v[6];
    for (int i = 0; i < 6; ++i) v[i] = strtoull(argv[2 + i], nullptr, 10);
    const uint64_t h = v[5];
    if (h > (1u << 20)) {  // (no block of that many reads: the argument rules alone)
        printf("%d 0\n", hc_seg_index::rect_ok(v[0], v[1], v[2], v[3], v[4], h) ? 0 : 71);
        return 0;
    }
    hc_seg_read_t *r = static_cast<hc_seg_read_t *>(malloc(h ? h * sizeof(hc_seg_read_t) : 1));
    if (!r) return 2;
    if (!hc_seg_index::rect_reads(v[0], v[1], v[2], v[3], v[4], h, r)) {
        printf("71 0\n");
    } else {
        printf("0 %llu\n", (ull)h);
        for (uint64_t i = 0; i < h; ++i) printf("%llu %llu %llu\n", (ull)r[i].offset, (ull)r[i].length, (ull)r[i].dst_off);
    }
    free(r);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && strcmp(argv[1], "rect") == 0) return rect(argc, argv);
    if (argc < 5) return 2;
    const uint64_t raw = strtoull(argv[1], nullptr, 10), seg = strtoull(argv[2], nullptr, 10);
    const bool adapt = strtoull(argv[3], nullptr, 10) != 0;
    const uint64_t width = strtoull(argv[4], nullptr, 10);
    const uint32_t n = (uint32_t)(argc - 5);
    hc_seg_read_t *p = static_cast<hc_seg_read_t *>(malloc(n ? n * sizeof(hc_seg_read_t) : 1));
    hc_seg_index::ReadRec *recs = static_cast<hc_seg_index::ReadRec *>(malloc(n ? n * sizeof(hc_seg_index::ReadRec) : 1));
    if (!p || !recs) return 2;
    for (uint32_t i = 0; i < n; ++i) {
        char *end = nullptr;
        p[i].offset = strtoull(argv[5 + i], &end, 10);
        if (*end != ':') return 2;
        p[i].length = strtoull(end + 1, &end, 10);
        if (*end != ':') return 2;
        p[i].dst_off = strtoull(end + 1, &end, 10);
        if (*end) return 2;
    }
    const hc_seg_index::Cuts c = hc_seg_index::seg_cuts(raw, seg, adapt, width);
    uint64_t need = 0;
    if (c.n == 0 || !hc_seg_index::reads_ok(raw, n ? p : nullptr, n, &need)) {
        printf("71 0 0 0 0 0 0\n");
    } else {
        const hc_seg_index::ReadPlan u = hc_seg_index::reads_plan(c, raw, p, n, recs);
        printf("0 %llu %llu %llu %llu %llu %llu\n", (ull)u.covered, (ull)u.cov_raw, (ull)need, (ull)u.k_lo, (ull)u.k_hi,
               (ull)hc_seg_index::reads_work_base(n, u.covered, u.cov_raw, false));
        for (uint32_t i = 0; i < n; ++i)
            printf("%llu %llu %llu %llu %llu %llu\n", (ull)recs[i].k0, (ull)recs[i].cnt, (ull)recs[i].e0, (ull)recs[i].src,
                   (ull)recs[i].length, (ull)recs[i].dst_off);
    }
    free(recs);
    free(p);
    return 0;
}
