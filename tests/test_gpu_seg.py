"""The segmented container on the GPU: hc_seg_compress / hc_seg_decompress and their device
entry points against the Python model (tests/seg_model.py, oracle.compress per segment)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import gpu_batch
import seg_model

pytestmark = pytest.mark.gpu

NO_SEG = seg_model.NO_SEGMENT
BIG = 16 * 2049 + 5  # 2050 segments at seg_bytes 16: more than one tile of the index scan
ADAPT_SHAPES = [(16, 19, 128), (16, 15, 128), (9, 32, 80), (64, 200, 4096)]


def _rng(hi, n, seed=1):
    return np.random.default_rng(seed).integers(0, hi, n, dtype=np.uint8).tobytes()


def _photo(w, h, k=3):
    import oracle
    return oracle.synth("photo", k, w, h).tobytes()


def _raw(name):
    kind, *a = name.split(":")
    if kind == "rng":
        return _rng(int(a[0]), int(a[1]))
    if kind == "photo":
        return _photo(int(a[0]), int(a[1]))
    raise KeyError(name)


# (name of the raw input, use_adapt, width, seg_bytes); every one runs with and without -m
PLAIN = [(f"rng:256:{n}", False, 512, 16) for n in (0, 1, 15, 16, 17, BIG)] + [(f"rng:4:{BIG}", False, 512, 16)]
ADAPT = [(f"rng:4:{w * h}", True, w, seg) for w, h, seg in ADAPT_SHAPES] + [("photo:64:200", True, 64, 4096)]
CASES = [c + (d,) for c in PLAIN + ADAPT for d in (False, True)] + [("photo:64:200", False, 512, 4096, True)]

_models = {}


def model(case):
    """(raw, the model's container) of a case, built once"""
    if case not in _models:
        name, adapt, w, seg, diff = case
        raw = _raw(name)
        _models[case] = (raw, seg_model.build(raw, diff, adapt, w, seg))
    return _models[case]


def _ids(c):
    return f"{c[0]}-{'a' if c[1] else 'c'}{'m' if c[4] else ''}-w{c[2]}-s{c[3]}"


def dev_compress(hc, torch, raw, diff, adapt, w, seg, out_cap=None, guard=64):
    """seg_compress_dev -> (status, out_len, the whole output tensor on the host)"""
    inp = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()
    cap = hc.seg_compress_bound(len(raw), seg, adapt, w) if out_cap is None else out_cap
    out = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    olen = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hc.seg_compress_dev(inp, out, olen, st, use_diff=diff, use_adapt=adapt, width=w, seg_bytes=seg, out_cap=cap)
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


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_host_matches_model(hc, gpu, case):
    name, adapt, w, seg, diff = case
    raw, want = model(case)
    if name == f"rng:256:{BIG}":
        # both the padded and the unpadded segment ends are in this case
        _, place = seg_model.parse(want)
        assert len(place) == 2050 and {0, 1, 15} <= {m % 16 for _, m in place}
    st, got = hc.seg_compress(raw, diff, adapt, w, seg)
    assert st == 0 and got == want
    assert hc.seg_decompress(got, full=True) == (0, raw, len(raw), NO_SEG)
    # the existing entry points still answer a container like any stream with a count above 2^63
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


def test_default_segment_size(hc, gpu):
    raw = _photo(64, 200)
    st, got = hc.seg_compress(raw, True, False, 512, 0)
    assert st == 0 and got == seg_model.build(raw, True, False, 512, hc.HC_SEG_DEFAULT_BYTES)
    assert struct.unpack_from("<Q", got, 24)[0] == hc.HC_SEG_DEFAULT_BYTES == 65536
    assert hc.seg_info(got)[1].seg_bytes == 65536


@pytest.mark.parametrize("case", [("photo:64:200", False, 512, 4096, True), ("photo:64:200", True, 64, 4096, True),
                                  (f"rng:256:{BIG}", False, 512, 16, False)], ids=_ids)
def test_device_capacity(hc, gpu, case):
    name, adapt, w, seg, diff = case
    raw, want = model(case)
    # exactly enough room: the container, and not a byte past it
    st, n, out = dev_compress(hc, gpu, raw, diff, adapt, w, seg, out_cap=len(want))
    assert (st, n) == (0, len(want)) and out[:n] == want and out[n:] == b"\xa5" * 64
    # one byte short: the needed length, and nothing written at all
    st, n, out = dev_compress(hc, gpu, raw, diff, adapt, w, seg, out_cap=len(want) - 1)
    assert (st, n) == (hc.HC_ERR_CAPACITY, len(want)) and out == b"\xa5" * len(out)
    assert hc.seg_compress(raw, diff, adapt, w, seg, cap=len(want) - 1)[0] == hc.HC_ERR_CAPACITY
    # decode with one byte too little room
    if len(raw) > 0:
        st, n, bad, back = dev_decompress(hc, gpu, want, len(raw), out_cap=len(raw) - 1)
        assert (st, n, bad) == (hc.HC_ERR_CAPACITY, len(raw), NO_SEG) and back == b"\xa5" * len(back)
        L = hc.lib()
        import ctypes
        buf = ctypes.create_string_buffer(len(raw))
        m = ctypes.c_uint64(0)
        b = ctypes.c_uint64(0)
        src = ctypes.cast(ctypes.c_char_p(want), ctypes.c_void_p)
        rc = L.hc_seg_decompress(src, len(want), ctypes.cast(buf, ctypes.c_void_p), len(raw) - 1, ctypes.byref(m),
                                 ctypes.byref(b))
        assert (rc, m.value, b.value) == (hc.HC_ERR_CAPACITY, len(raw), NO_SEG)
        rc = L.hc_seg_decompress(src, len(want), ctypes.cast(buf, ctypes.c_void_p), len(raw), ctypes.byref(m), None)
        assert (rc, m.value) == (0, len(raw)) and buf.raw == raw


def repack(container, streams):
    """the container with its segments' streams replaced (same header fields)"""
    c = bytes(container)
    out = bytearray(c[:48]) + b"".join(struct.pack("<Q", len(s)) for s in streams)
    for s in streams:
        out += bytes(seg_model.align16(len(out)) - len(out)) + s
    return bytes(out)


def container_mutants(c):
    """every container-level error: those the header decides and those of the index"""
    c = bytes(c)
    f, place = seg_model.parse(c)
    n = f["n_segments"]

    def index(k, v):
        return c[:48 + 8 * k] + struct.pack("<Q", v % 2**64) + c[56 + 8 * k:]

    m = dict(seg_model.header_mutants(c))
    m.update({
        "enc_len_wraps": index(1, 2**64 - 8),
        "enc_len_wraps_first": index(0, 2**64 - 8),
        "enc_len_past_end": index(n - 1, len(c)),
        "enc_len_longer": index(0, place[0][1] + 16),
        "enc_len_shorter": index(n - 1, place[n - 1][1] - 1),
        "trailing_byte": c + b"\x00",
        "last_byte_cut": c[:-1],
        "payload_cut": c[:place[1][0] + 3],
    })
    return m


@pytest.mark.parametrize("case", [("rng:256:100", False, 512, 32, True), ("rng:4:560", True, 16, 128, False)], ids=_ids)
def test_container_mutants(hc, gpu, case):
    raw, good = model(case)
    assert seg_model.parse(good)[0]["n_segments"] == 4
    for name, bad in container_mutants(good).items():
        assert seg_model.decode(bad) == (hc.HC_ERR_SEG_HEADER, NO_SEG, b""), name
        assert hc.seg_decompress(bad, full=True) == (hc.HC_ERR_SEG_HEADER, b"", 0, NO_SEG), name
        st, n, seg, out = dev_decompress(hc, gpu, bad, len(raw))
        assert (st, n, seg) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG), name
        assert out == b"\xa5" * len(out), name  # and nothing was decoded
        assert hc.decompress(bad)[0] in (hc.HC_ERR_HEADER, hc.HC_ERR_HUFFMAN), name
    # an info that is valid for this length but is not what the device bytes say
    st, info = hc.seg_info(good)
    assert st == 0
    info.flags ^= hc.HC_FLAG_DIFF
    st, n, seg, out = dev_decompress(hc, gpu, good, len(raw), info=info)
    assert (st, n, seg) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG) and out == b"\xa5" * len(out)
    # index mutants whose header is intact: the same verdict with the caller's own (valid) info
    st, info = hc.seg_info(good)
    for name in ("enc_len_wraps", "enc_len_longer", "enc_len_shorter"):
        st, n, seg, out = dev_decompress(hc, gpu, container_mutants(good)[name], len(raw), info=info)
        assert (st, n, seg) == (hc.HC_ERR_SEG_HEADER, 0, NO_SEG), name


def _segment_verdict(hc, torch, stream, adapt, want_len):
    """what the existing, unchanged batch decoder says about one segment's bytes with exactly
    its cut's room: (status with 64 and a wrong length mapped to HC_ERR_SEG_SIZE, bytes)"""
    run = gpu_batch.decompress_adapt_batch if adapt else gpu_batch.decompress_batch
    st, outs, lens = run(hc, torch, [stream], [want_len])
    if st[0] == hc.HC_ERR_CAPACITY or (st[0] == 0 and lens[0] != want_len):
        return hc.HC_ERR_SEG_SIZE, b""
    return st[0], outs[0]


@pytest.mark.parametrize("case", [("photo:64:200", False, 512, 4096, True), ("photo:64:200", True, 64, 4096, True)],
                         ids=_ids)
def test_segment_mutants(hc, gpu, case):
    import oracle
    name, adapt, w, seg, diff = case
    raw, good = model(case)
    f, _ = seg_model.parse(good)
    streams = seg_model.segments(good)
    assert len(streams) == 4

    def check(bad, want_st, want_bad, want_bytes=None):
        got = hc.seg_decompress(bad, full=True)
        st, n, seg_k, out = dev_decompress(hc, gpu, bad, len(raw))
        if want_st == 0:
            assert got == (0, want_bytes, len(raw), NO_SEG)
            assert (st, n, seg_k) == (0, len(raw), NO_SEG) and out[:n] == want_bytes
        else:
            assert got == (want_st, b"", 0, want_bad)
            assert (st, n, seg_k) == (want_st, 0, want_bad)
        assert out[len(raw):] == b"\xa5" * 64  # never a byte past the output

    # truncation: the model's verdict (8 or 9 from the oracle), never a length overrun
    s1 = streams[1]
    for cut in (len(s1) - 1, len(s1) // 2, 8):
        bad = repack(good, [streams[0], s1[:cut]] + streams[2:])
        st, k, _ = seg_model.decode(bad)
        assert st in (8, 9) and k == 1
        check(bad, st, 1)
        both = repack(good, [streams[0], s1[:cut], streams[2][:cut], streams[3]])
        assert seg_model.decode(both)[:2] == (st, 1)
        check(both, st, 1)
    # bit flips at eight fixed payload positions of segment 1
    want_len = f["cuts"][1][1]
    for i, pos in enumerate((9, 10, 17, 33, len(s1) // 2, len(s1) // 2 + 7, len(s1) - 2, len(s1) - 1)):
        flipped = s1[:pos] + bytes([s1[pos] ^ (1 << (i % 8))]) + s1[pos + 1:]
        want_st, seg_bytes_out = _segment_verdict(hc, gpu, flipped, adapt, want_len)
        bad = repack(good, [streams[0], flipped] + streams[2:])
        if want_st == 0:
            ost, obytes = oracle.decompress(flipped)
            assert (ost, obytes) == (0, seg_bytes_out)  # the oracle decodes it cleanly to the same length
            o = f["cuts"][1][0]
            check(bad, 0, NO_SEG, raw[:o] + obytes + raw[o + want_len:])
        else:
            check(bad, want_st, 1)
    # a segment of another mode than the container's: the batch decoder's own verdict
    other = oracle.compress(raw[:f["cuts"][1][1]], diff, not adapt, w)[1]
    want_st, _ = _segment_verdict(hc, gpu, other, adapt, want_len)
    assert want_st == hc.HC_ERR_UNSUPPORTED
    check(repack(good, [streams[0], other] + streams[2:]), want_st, 1)


def test_batch_cli(hc, gpu, tmp_path):
    raws = {"a.bin": _photo(64, 200), "b.bin": _rng(256, 10000, seed=2)}
    for fn, r in raws.items():
        (tmp_path / fn).write_bytes(r)
    enc = tmp_path / "enc"
    enc.mkdir()
    r = subprocess.run([hc.BATCH_CLI_PATH, "-c", "-m", "-s", "4096", "-o", str(enc)] + [str(tmp_path / fn) for fn in raws],
                       capture_output=True)
    assert r.returncode == 0, r.stderr
    for fn, raw in raws.items():
        assert (enc / (fn + ".huf")).read_bytes() == seg_model.build(raw, True, False, 512, 4096)
    # -d on a mix: one container, one plain stream
    plain = _rng(4, 5000, seed=3)
    st, stream = hc.compress(plain, True)
    assert st == 0
    mix = tmp_path / "mix"
    mix.mkdir()
    (mix / "a.bin.huf").write_bytes((enc / "a.bin.huf").read_bytes())
    (mix / "p.bin.huf").write_bytes(stream)
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", str(mix / "a.bin.huf"), str(mix / "p.bin.huf")], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert (mix / "a.bin").read_bytes() == raws["a.bin"] and (mix / "p.bin").read_bytes() == plain
    # a failing segment is named
    good = (enc / "a.bin.huf").read_bytes()
    streams = seg_model.segments(good)
    (mix / "bad.huf").write_bytes(repack(good, streams[:2] + [streams[2][:8]] + streams[3:]))
    r = subprocess.run([hc.BATCH_CLI_PATH, "-d", str(mix / "bad.huf")], capture_output=True)
    assert r.returncode == 8 and b"bad.huf: segment 2: ERROR: invalid or missing Huffman coding header" in r.stderr
    assert not os.path.exists(mix / "bad")


def test_one_mebibyte(hc, gpu):
    """the many-waves path: 16 segments of 64 KiB"""
    raw = _photo(1024, 1024, k=1)
    want = seg_model.build(raw, True, False, 512, 65536)
    assert seg_model.parse(want)[0]["n_segments"] == 16
    st, got = hc.seg_compress(raw, True)
    assert st == 0 and got == want
    assert hc.seg_decompress(got) == (0, raw)
    st, n, out = dev_compress(hc, gpu, raw, True, False, 512, 0)
    assert (st, n) == (0, len(want)) and out[:n] == want
