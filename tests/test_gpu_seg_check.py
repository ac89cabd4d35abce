"""The checked segmented container on the GPU: hc_seg_compress2 / hc_seg_compress_dev with
HC_SEG_CHECK_CRC32 and the decoders against the Python model (tests/seg_check_model.py: the
oracle per segment, zlib.crc32 per cut), byte for byte and round trip; then what the checksum is
for: damaged streams that still decode cleanly."""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import gpu_batch
import seg_check_cases as cases
import seg_check_model as scm
import seg_model

pytestmark = pytest.mark.gpu

NO_SEG = scm.NO_SEGMENT
BIG = 16 * 2049 + 5  # 2050 segments at seg_bytes 16: more than one tile of the index scan
ADAPT_SHAPES = [(16, 19, 128), (16, 15, 128), (9, 32, 80), (64, 200, 4096)]  # (9, 32, 80): bands start 4-byte aligned only

# (raw input, use_adapt, width, seg_bytes, use_diff)
CASES = [(f"rng:256:{n}", False, 512, 16, d) for n in (0, 1, 15, 16, 17) for d in (False, True)]
CASES += [(f"rng:256:{BIG}", False, 512, 16, False)]
CASES += [(f"rng:4:{w * h}", True, w, seg, d) for w, h, seg in ADAPT_SHAPES for d in (False, True)]
CASES += [("photo:64:200", False, 512, 4096, True), ("photo:64:200", True, 64, 4096, True),
          ("photo:64:200", True, 64, 4096, False)]
# segments of 8192 and 1815 bytes; one segment of many tiles of the checksum kernel
CASES += [("rng:256:10007", False, 512, 8192, False), ("rng:4:300000", False, 512, 2**20, True)]

_models = {}


def model(case):
    """(raw, the model's checked container) of a case, built once"""
    if case not in _models:
        name, adapt, w, seg, diff = case
        raw = cases.raw(name)
        _models[case] = (raw, scm.build(raw, diff, adapt, w, seg))
    return _models[case]


def _ids(c):
    return f"{c[0]}-{'a' if c[1] else 'c'}{'m' if c[4] else ''}-w{c[2]}-s{c[3]}"


def dev_compress(hc, torch, raw, diff, adapt, w, seg, out_cap=None, guard=64, check=True):
    """seg_compress_dev -> (status, out_len, the whole output tensor on the host)"""
    inp = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()
    cap = hc.seg_compress_bound(len(raw), seg, adapt, w, check=check) if out_cap is None else out_cap
    out = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    olen = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hc.seg_compress_dev(inp, out, olen, st, use_diff=diff, use_adapt=adapt, width=w, seg_bytes=seg, out_cap=cap,
                        check=check)
    torch.cuda.synchronize()
    return int(st.item()), int(olen.item()), out.cpu().numpy().tobytes()


def dev_decompress(hc, torch, container, out_room, out_cap=None, info=None, guard=64):
    """seg_decompress_dev -> (status, out_len, bad_segment, the whole output tensor on the host)"""
    host = np.zeros(gpu_batch.align(max(len(container), 1)), dtype=np.uint8)
    host[:len(container)] = np.frombuffer(bytes(container), dtype=np.uint8)
    inp = torch.from_numpy(host).cuda()
    cap = out_room if out_cap is None else out_cap
    out = torch.full((out_room + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    olen = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hc.seg_decompress_dev(inp, out, olen, st, bad_segment=bad, info=info, in_len=len(container), out_cap=cap)
    torch.cuda.synchronize()
    return int(st.item()), int(olen.item()), int(bad.item()) % 2**64, out.cpu().numpy().tobytes()


def both_decoders(hc, torch, container, raw_len):
    """(status, bad_segment, bytes) of the host and of the device decoder, which must agree;
    never a byte past the output"""
    st, got, n, bad = hc.seg_decompress(container, full=True)
    dst, dn, dbad, out = dev_decompress(hc, torch, container, raw_len)
    assert out[raw_len:] == b"\xa5" * 64
    assert (dst, dn, dbad) == (st, n, bad)
    assert n == (raw_len if st == 0 else 0) and (got == out[:n] if st == 0 else got == b"")
    return st, bad, got


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_host_matches_model(hc, gpu, case):
    name, adapt, w, seg, diff = case
    raw, want = model(case)
    st, got = hc.seg_compress(raw, diff, adapt, w, seg, check=True)
    assert st == 0 and got == want
    assert hc.seg_info(got)[1].flags & hc.HC_SEG_CHECK_CRC32
    assert hc.seg_decompress(got, full=True) == (0, raw, len(raw), NO_SEG)
    assert hc.decompress(got)[0] == hc.HC_ERR_HUFFMAN


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_device_matches_model(hc, gpu, case):
    name, adapt, w, seg, diff = case
    raw, want = model(case)
    st, n, out = dev_compress(hc, gpu, raw, diff, adapt, w, seg)
    assert (st, n) == (0, len(want)) and out[:n] == want
    st, n, bad, back = dev_decompress(hc, gpu, want, len(raw))
    assert (st, n, bad) == (0, len(raw), NO_SEG) and back[:n] == raw
    assert back[n:] == b"\xa5" * 64  # nothing past the output


def test_unchecked_is_unchanged(hc, gpu):
    """without the bit: hc_seg_compress2 is hc_seg_compress, byte for byte seg_model's container"""
    raw = cases.raw("photo:64:200")
    want = seg_model.build(raw, True, False, 512, 4096)
    L = hc.lib()
    buf = ctypes.create_string_buffer(len(want))
    n = ctypes.c_uint64(0)
    src = ctypes.cast(ctypes.c_char_p(raw), ctypes.c_void_p)
    assert L.hc_seg_compress(src, len(raw), 1, 0, 512, 4096, ctypes.cast(buf, ctypes.c_void_p), len(want),
                             ctypes.byref(n)) == 0
    assert buf.raw[:n.value] == want
    assert hc.seg_compress(raw, True, False, 512, 4096) == (0, want)
    st, n, out = dev_compress(hc, gpu, raw, True, False, 512, 4096, check=False)
    assert (st, n) == (0, len(want)) and out[:n] == want


@pytest.mark.parametrize("case", [("photo:64:200", False, 512, 4096, True), ("photo:64:200", True, 64, 4096, True),
                                  (f"rng:256:{BIG}", False, 512, 16, False), ("rng:256:17", False, 512, 16, False)],
                         ids=_ids)
def test_capacity(hc, gpu, case):
    name, adapt, w, seg, diff = case
    raw, want = model(case)
    # exactly enough room: the container, and not a byte past it
    st, n, out = dev_compress(hc, gpu, raw, diff, adapt, w, seg, out_cap=len(want))
    assert (st, n) == (0, len(want)) and out[:n] == want and out[n:] == b"\xa5" * 64
    assert hc.seg_compress(raw, diff, adapt, w, seg, cap=len(want), check=True) == (0, want)
    # one byte short: the needed length, and nothing written at all
    st, n, out = dev_compress(hc, gpu, raw, diff, adapt, w, seg, out_cap=len(want) - 1)
    assert (st, n) == (hc.HC_ERR_CAPACITY, len(want)) and out == b"\xa5" * len(out)
    assert hc.seg_compress(raw, diff, adapt, w, seg, cap=len(want) - 1, check=True)[0] == hc.HC_ERR_CAPACITY
    # the unchecked container's length is too little for the checked one where the index grew
    plain = seg_model.build(raw, diff, adapt, w, seg)
    if len(plain) < len(want):
        st, n, out = dev_compress(hc, gpu, raw, diff, adapt, w, seg, out_cap=len(plain))
        assert (st, n) == (hc.HC_ERR_CAPACITY, len(want)) and out == b"\xa5" * len(out)
    # decode with one byte too little room: the verdict alone, nothing decoded or checksummed
    st, n, bad, back = dev_decompress(hc, gpu, want, len(raw), out_cap=len(raw) - 1)
    assert (st, n, bad) == (hc.HC_ERR_CAPACITY, len(raw), NO_SEG) and back == b"\xa5" * len(back)


@pytest.mark.parametrize("case", cases.SILENT_FLIPS, ids=cases.FLIP_IDS)
def test_silent_flips_are_caught(hc, gpu, case):
    name, diff, adapt, w, seg, byte, bit = case
    raw, good = model((name, adapt, w, seg, diff))
    plain = seg_model.build(raw, diff, adapt, w, seg)
    # the flipped stream in an unchecked container: status 0 and the model's wrong bytes
    st, bad, wrong = scm.decode(cases.flip(plain, 1, byte, bit))
    assert st == 0 and len(wrong) == len(raw) and wrong != raw
    assert both_decoders(hc, gpu, cases.flip(plain, 1, byte, bit), len(raw)) == (0, NO_SEG, wrong)
    # the same stream in the checked one
    flipped = cases.flip(good, 1, byte, bit)
    assert scm.decode(flipped) == (hc.HC_ERR_SEG_CHECK, 1, b"")
    assert both_decoders(hc, gpu, flipped, len(raw)) == (hc.HC_ERR_SEG_CHECK, 1, b"")


def test_flip_that_changes_nothing(hc, gpu, oracle_mod):
    """a damaged stream that still decodes to the same bytes passes: the checksum is of the data"""
    case = ("photo:64:200", False, 512, 4096, True)
    raw, good = model(case)
    s1 = scm.segments(good)[1]
    o, m = scm.parse(good)[0]["cuts"][1]
    found = None
    for pos in range(len(s1) - 1, 8, -1):
        for bit in (0, 3, 7):
            if oracle_mod.decompress(s1[:pos] + bytes([s1[pos] ^ (1 << bit)]) + s1[pos + 1:]) == (0, raw[o:o + m]):
                found = (pos, bit)
                break
        if found:
            break
    if found is None:
        pytest.skip("no payload flip of this stream decodes to the same bytes")
    same = cases.flip(good, 1, *found)
    assert same != good and scm.decode(same) == (0, NO_SEG, raw)
    assert both_decoders(hc, gpu, same, len(raw)) == (0, NO_SEG, raw)


def _set_crc(c, k, value):
    n = scm.parse(c)[0]["n_segments"]
    at = 48 + 8 * n + 4 * k
    return c[:at] + struct.pack("<I", value) + c[at + 4:]


@pytest.mark.parametrize("case", [("photo:64:200", False, 512, 4096, True), ("photo:64:200", True, 64, 4096, True)],
                         ids=_ids)
def test_precedence_and_index(hc, gpu, case):
    name, adapt, w, seg, diff = case
    raw, good = model(case)
    streams = scm.segments(good)
    crcs = scm.parse(good)[2]
    assert len(streams) == 4
    flip = next(f for f in cases.SILENT_FLIPS if (f[0], f[2]) == (name, adapt))
    flipped1 = cases.flip(good, 1, flip[5], flip[6])
    # a mismatch in segment 1 wins over the coder's error in segment 2
    bad = scm.repack(flipped1, scm.segments(flipped1)[:2] + [streams[2][:len(streams[2]) // 2], streams[3]])
    assert scm.decode(bad) == (hc.HC_ERR_SEG_CHECK, 1, b"")
    assert both_decoders(hc, gpu, bad, len(raw)) == (hc.HC_ERR_SEG_CHECK, 1, b"")
    # and the coder's error in segment 1 over a mismatch in segment 2
    bad = _set_crc(scm.repack(good, [streams[0], streams[1][:len(streams[1]) // 2]] + streams[2:]), 2, crcs[2] ^ 1)
    st, k, _ = scm.decode(bad)
    assert st in (8, 9) and k == 1
    assert both_decoders(hc, gpu, bad, len(raw)) == (st, 1, b"")
    # a wrong crc word alone fails its segment, the lowest of several
    for k in range(4):
        for v in (crcs[k] ^ 1, crcs[k] ^ 0x80000000, 0, crcs[(k + 1) % 4]):
            assert both_decoders(hc, gpu, _set_crc(good, k, v), len(raw)) == (hc.HC_ERR_SEG_CHECK, k, b"")
    two = _set_crc(_set_crc(good, 3, 0), 2, 0)
    assert both_decoders(hc, gpu, two, len(raw)) == (hc.HC_ERR_SEG_CHECK, 2, b"")
    # a segment of another length than its cut is still HC_ERR_SEG_SIZE, not a mismatch
    import oracle
    st, short = oracle.compress(raw[:512], diff, adapt, w)  # 8 rows of 64: a valid stream of either mode
    assert st == 0
    bad = scm.repack(good, [streams[0], short] + streams[2:])
    assert scm.decode(bad) == (hc.HC_ERR_SEG_SIZE, 1, b"")
    assert both_decoders(hc, gpu, bad, len(raw)) == (hc.HC_ERR_SEG_SIZE, 1, b"")


@pytest.mark.parametrize("case", [("rng:256:100", False, 512, 32, True), ("rng:4:560", True, 16, 128, False)], ids=_ids)
def test_container_mutants(hc, gpu, case):
    name, adapt, w, seg, diff = case
    raw, good = model(case)
    plain = seg_model.build(raw, diff, adapt, w, seg)
    f, place, _ = scm.parse(good)
    n = f["n_segments"]
    assert n == 4
    mutants = {}
    for mname, bad in seg_model.header_mutants(plain).items():
        # the same header mutation on the checked container (index_cut: of its own, longer index)
        if mname == "short":
            mutants[mname] = good[:47]
        elif mname == "index_cut":
            mutants[mname] = good[:48 + 12 * n - 1]
        else:
            mutants[mname] = bad[:9] + b"\x01" + bad[10:48] + good[48:]
    mutants["check_2"] = good[:9] + b"\x02" + good[10:]
    mutants["after_check"] = good[:10] + b"\x01" + good[11:]
    mutants["check_dropped"] = good[:9] + b"\x00" + good[10:]  # the crc words then read as part of segment 0's room
    mutants["check_added"] = plain[:9] + b"\x01" + plain[10:]
    mutants["trailing_byte"] = good + b"\x00"
    mutants["last_byte_cut"] = good[:-1]
    mutants["payload_cut"] = good[:place[1][0] + 3]
    for mname, bad in mutants.items():
        assert scm.decode(bad) == (hc.HC_ERR_SEG_HEADER, NO_SEG, b""), mname
        assert hc.seg_decompress(bad, full=True) == (hc.HC_ERR_SEG_HEADER, b"", 0, NO_SEG), mname
        st, m, k, out = dev_decompress(hc, gpu, bad, len(raw))
        assert (st, m, k) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG), mname
        assert out == b"\xa5" * len(out), mname  # and nothing was decoded
    # an info of the other kind than the device bytes: valid for this length, and rejected on the device
    st, info = hc.seg_info(good)
    assert st == 0
    info.flags ^= hc.HC_SEG_CHECK_CRC32
    st, m, k, out = dev_decompress(hc, gpu, good, len(raw), info=info)
    assert (st, m, k) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG) and out == b"\xa5" * len(out)
    st, info = hc.seg_info(plain)
    info.flags |= hc.HC_SEG_CHECK_CRC32
    big = plain + bytes(64)  # room for the index this info claims
    st, m, k, out = dev_decompress(hc, gpu, big, len(raw), info=info)
    assert (st, m, k) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG) and out == b"\xa5" * len(out)


def test_batch_cli(hc, gpu, tmp_path):
    raw = cases.raw("photo:64:200")
    (tmp_path / "a.bin").write_bytes(raw)
    enc = tmp_path / "enc"
    enc.mkdir()
    r = subprocess.run([hc.BATCH_CLI_PATH, "-c", "-m", "-s", "4096", "-k", "-o", str(enc), str(tmp_path / "a.bin")],
                       capture_output=True)
    assert r.returncode == 0, r.stderr
    good = (enc / "a.bin.huf").read_bytes()
    assert good == scm.build(raw, True, False, 512, 4096)
    # -d needs no option: the header says what kind it is
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", str(enc / "a.bin.huf")], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert (enc / "a.bin").read_bytes() == raw
    # the silent flip is named, and nothing is written
    (enc / "bad.huf").write_bytes(cases.flip(good, 1, 9, 0))
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", str(enc / "bad.huf")], capture_output=True)
    assert r.returncode == hc.HC_ERR_SEG_CHECK == 72
    assert b"bad.huf: segment 1: ERROR: segment checksum mismatch\n" in r.stderr
    assert not os.path.exists(enc / "bad")
    # -k belongs to -s -c: anything else is the usage error, before any file is touched
    for args in (["-c", "-k"], ["-d", "-k"], ["-d", "-s", "4096", "-k"]):
        r = subprocess.run([hc.BATCH_CLI_PATH] + args + ["-o", str(tmp_path), str(tmp_path / "a.bin")], capture_output=True)
        assert r.returncode == 2 and b"ERROR: unrecognized option used" in r.stderr
    assert not os.path.exists(tmp_path / "a.bin.huf")
