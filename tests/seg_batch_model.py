"""The batched segmented coders (hc_seg_*_batch_dev, hc_seg_*_host_batch, include/hcodec.h)
restated in Python. A batch is the existing models applied per item (seg_check_model.build,
seg_check_model.decode, seg_range_model.decode_range) plus one rule: what the single call reports
through its return value for a reason that belongs to the item is the item's status, with
out_len 0 and bad_segment UINT64_MAX. Also the two work bounds in the closed form the header
states. Test infrastructure only."""
import seg_check_model as scm
import seg_model
import seg_range_model as srm
from seg_model import NO_SEGMENT, SEG_HEADER, CAPACITY, align16

WIDTH, MATRIX_SIZE, DIMS, ARG = 4, 6, 12, 71
WHOLE = 2**64 - 1
MAX_SEGS = 2**31 - 1


def host_status(n, use_adapt, width):
    """hc_compress's host-decided statuses, in its order"""
    if width == 0:
        return WIDTH
    if use_adapt and n % width:
        return MATRIX_SIZE
    if use_adapt and (width < 8 or n // width < 8):
        return DIMS
    return 0


def encode_item(raw, width, use_diff, use_adapt, seg_bytes, check, out_cap=None):
    """(status, container, out_len) of one encoder item"""
    hs = host_status(len(raw), use_adapt, width)
    if hs:
        return hs, b"", 0
    c = scm.build(raw, use_diff, use_adapt, width, seg_bytes or seg_model.DEFAULT_BYTES, check=check)
    if out_cap is not None and len(c) > out_cap:
        return CAPACITY, b"", len(c)
    return 0, c, len(c)


def decode_item(container, offset=0, length=WHOLE, out_cap=None):
    """(status, bad_segment, bytes, out_len) of one decoder item; (0, WHOLE) is the whole decoder"""
    if (offset, length) == (0, WHOLE):
        st, bad, got = scm.decode(container, out_cap)
        f = srm.header(container)
        n = len(got) if st == 0 else (f["raw_len"] if st == CAPACITY else 0)
        return st, bad, got, n
    st, bad, got, n = srm.decode_range(container, offset, length, out_cap)
    if st == ARG:  # the single call's return value: the batch's per-item status
        return ARG, NO_SEGMENT, b"", 0
    return st, bad, got, n


def _slots(f, offset, length):
    """(covered segments, staging slots, raw bytes of the covered segments) of a range"""
    k0, count = srm.covered(f, offset, length)
    if count == 0:
        return 0, 0, 0
    cuts = f["cuts"]
    first, end = cuts[k0][0], cuts[k0 + count - 1][0] + cuts[k0 + count - 1][1]
    if offset % 4:
        return count, count, end - first
    head, tail = offset != first, offset + length != end
    return count, (int(head or tail) if count == 1 else int(head) + int(tail)), end - first


def encode_work_bound(hc, items, use_adapt, seg_bytes, check):
    """items: (in_len, width); the closed form of hc_seg_compress_batch_work_bound"""
    L = hc.lib()
    seg_bytes = seg_bytes or seg_model.DEFAULT_BYTES
    N = S = R = 0
    for n, w in items:
        if host_status(n, use_adapt, w):
            continue
        cuts = seg_model.cuts(n, use_adapt, w, seg_bytes)
        N += len(cuts)
        S += sum(align16(hc.compress_bound(m, use_adapt)) for _, m in cuts)
        R += n
    total = 7 * align16(8 * N) + align16(4 * N) + (align16(4 * N) if check else 0) + 16 + S
    if use_adapt and N:
        total += align16(int(L.hc_adapt_compress_work_bound(R, N)))
    return total + align16(112 * len(items)) + align16(4 * N) + align16(8 * len(items))


def decode_work_bound(hc, items):
    """items: (container, offset, length); the closed form of hc_seg_decompress_batch_work_bound"""
    L = hc.lib()
    C = slots = B = E = W = A = 0
    for c, offset, length in items:
        f = srm.header(c)
        if f is None:
            continue
        if (offset, length) == (0, WHOLE):
            count, ns, raw = f["n_segments"], 0, f["raw_len"]
        elif offset > f["raw_len"] or length > f["raw_len"] - offset:
            continue
        else:
            count, ns, raw = _slots(f, offset, length)
        C += count
        slots += ns
        B += ns * align16(max(m for _, m in f["cuts"]))
        if f["flags"] & seg_model.FLAG_ADAPT and count:
            E, W, A = E + len(c), W + raw, A + count
    n = len(items)
    total = 5 * align16(8 * C) + 2 * align16(4 * C) + align16(8 * n) + align16(176 * n) + 3 * align16(8 * slots) + B
    if A:
        total += align16(int(L.hc_adapt_decompress_work_bound(E, W, A)))
    return total
