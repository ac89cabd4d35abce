"""GPU tests of what include/hcodec.h promises for the device batch entry points, with the streams
placed by tests/gpu_place.py: starts that are only 4-byte aligned (base address and offsets at
every residue 0, 4, 8, 12 mod 16), slots of exactly the stated size, poison in every byte around
them. Stream i reads in[in_offs[i] .. +in_lens[i]) and writes only out[out_offs[i] .. +out_caps[i]);
`work` need only reach the published bound; hc_pack_batch takes any byte alignment; a base that is
not 4-aligned is HC_ERR_ARG before anything runs.

Every expected byte and status is the oracle's (main.cpp:39-128 restated in oracle/hc_oracle.c),
compared exactly. The paths this reaches: the decoder's run stores, split at absolute 16-byte
boundaries (revert_block), and its byte-wise fallback for a block whose runs cross the capacity;
its input window of (len + 3) & ~3 bytes, which holds up to 3 bytes of the neighbour; the
encoder's 0-4 byte tail store against an exact capacity (RecSink::finish); hc_adapt.hip's plain
pointers (tile_fetch's fast path by (mat | W) & 3, the 16-byte accesses of chunk_sum_kernel and
undiff_kernel at 4-aligned addresses, the partial chunk's last dword); pack_kernel's head / body /
tail split by the destination address."""
import numpy as np
import pytest

import gpu_place as gp
from test_gpu_adapt_batch import _mat

pytestmark = pytest.mark.gpu

OUT_POISON = 0xA5
_cache = {}


def _raws(oracle_mod):
    if "raws" not in _cache:
        lens = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 258, 259, 260]
        raws = [bytes([(31 * n + 9) & 255]) * n for n in lens]
        raws.append(b"".join(bytes([n]) * n for n in range(4, 100)))  # run starts at every residue
        raws += [oracle_mod.synth(kind, 0, w, h).tobytes() for kind, w, h in gp.TRUNC_SET]
        raws += [bytes(range(256)) * 4, b"\x00\xff" * 600]
        # the same shapes with other values and lengths one off, so that the set is about 40
        raws += [bytes([(77 * n + 1) & 255]) * n for n in (6, 9, 14, 18, 62, 66, 254, 261, 300, 515)]
        raws += [oracle_mod.synth(kind, 1, w, h).tobytes() for kind, w, h in (("grad", 33, 31), ("photo", 64, 19))]
        assert 38 <= len(raws) <= 42
        _cache["raws"] = raws
    return _cache["raws"]


def _encs(oracle_mod, use_diff):
    key = ("encs", use_diff)
    if key not in _cache:
        out = []
        for r in _raws(oracle_mod):
            st, e = oracle_mod.compress(r, use_diff, False, 512)
            assert st == 0 and oracle_mod.decompress(e) == (0, r)
            out.append(e)
        _cache[key] = out
    return _cache[key]


def _launch(torch, call, blobs, caps, rot, base_res, in_poison=0x3C, in_lens=None, **kw):
    """place blobs (exact slots, in_poison between them) and an all-poison output with slots of
    exactly caps, run call(in, in_offs, in_lens, out, out_offs, out_caps, out_lens, status, **kw)
    -> (statuses, out_lens, output view, output offsets)"""
    n = len(blobs)
    din, ioffs, ilens = gp.place(torch, blobs, [len(b) for b in blobs], rot, base_res, in_poison)
    if in_lens is not None:
        assert all(a <= len(b) for a, b in zip(in_lens, blobs))
        ilens = gp.dev_i64(torch, in_lens)
    dout, ooffs, _ = gp.place(torch, [b""] * n, caps, rot, base_res, OUT_POISON)
    olens = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    call(din, ioffs, ilens, dout, ooffs, gp.dev_i64(torch, caps), olens, st, **kw)
    torch.cuda.synchronize()
    return st.cpu().tolist(), olens.cpu().tolist(), dout, ooffs.cpu().tolist()


def _check(res, caps, want_st, want, open_slots=()):
    """statuses and lengths as a whole, every slot's bytes (but those of open_slots, whose content
    the header leaves open), and nothing outside the slots touched"""
    st, olens, dout, ooffs = res
    assert st == want_st
    assert olens == [len(w) if isinstance(w, bytes) else w for w in want]
    got = gp.slots(dout, ooffs, [0 if i in open_slots else min(n, c) for i, (n, c) in enumerate(zip(olens, caps))])
    assert [i for i, (g, w) in enumerate(zip(got, want)) if i not in open_slots and g != w] == []
    assert gp.outside_untouched(dout, ooffs, caps, OUT_POISON), gp.touched(dout, ooffs, caps, OUT_POISON)


# ------------------------------------------------------------------ a. exact capacities ----

@pytest.mark.parametrize("use_diff", [False, True])
@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_plain_batch_exact_capacities(gpu, hc, oracle_mod, rot, use_diff):
    torch = gpu
    base_res = 4 * ((rot + 1) % 4)
    raws, encs = _raws(oracle_mod), _encs(oracle_mod, use_diff)
    caps = [len(e) for e in encs]
    _check(_launch(torch, hc.compress_batch, raws, caps, rot, base_res, use_diff=use_diff),
           caps, [0] * len(raws), encs)
    caps = [len(r) for r in raws]
    _check(_launch(torch, hc.decompress_batch, encs, caps, rot, base_res), caps, [0] * len(raws), raws)


# ----------------------------------------------------------------- b. input independence ----

@pytest.mark.parametrize("use_diff", [False, True])
def test_input_gaps_do_not_reach_the_result(gpu, hc, oracle_mod, use_diff):
    """rot = 1 with the input gaps 0x00, 0xFF and random: the same statuses, lengths and bytes"""
    torch = gpu
    raws, encs = _raws(oracle_mod), _encs(oracle_mod, use_diff)
    fills = [0x00, 0xFF, np.random.default_rng(11).integers(0, 256, size=1 << 15, dtype=np.uint8)]
    seen = []
    for fill in fills:
        caps = [len(e) for e in encs]
        enc = _launch(torch, hc.compress_batch, raws, caps, 1, 8, in_poison=fill, use_diff=use_diff)
        _check(enc, caps, [0] * len(raws), encs)
        caps = [len(r) for r in raws]
        dec = _launch(torch, hc.decompress_batch, encs, caps, 1, 8, in_poison=fill)
        _check(dec, caps, [0] * len(raws), raws)
        seen.append((enc[0], enc[1], enc[2].cpu().numpy().tobytes(), dec[0], dec[1], dec[2].cpu().numpy().tobytes()))
    assert seen[0] == seen[1] == seen[2]


# ------------------------------------------------------- c. truncation with a live tail ----

@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_truncated_length_over_whole_stream(gpu, hc, oracle_mod, rot):
    """the whole valid encoding lies in the buffer, in_lens stops 1..8 bytes short of it (or at 0,
    1, 8, 9 bytes): the bytes behind in_lens are the stream's own, and the decoder's window is
    rounded up over as many as 3 of them. Status 9 or 8 like the oracle's for the prefix, never 0;
    good streams in the same launch decode"""
    torch = gpu
    base_res = 4 * ((rot + 1) % 4)
    raws = _raws(oracle_mod)
    good = [(r, e) for r, e in zip(raws, _encs(oracle_mod, False))][8::3] + \
           [(r, e) for r, e in zip(raws, _encs(oracle_mod, True))][9::3]
    blobs, in_lens, caps, want_st, want = [], [], [], [], []
    g = 0
    for name, raw, enc in gp.trunc_streams(oracle_mod):
        for j, n in enumerate([len(enc) - k for k in gp.TRUNC_CUTS] + list(gp.TRUNC_PREFIXES)):
            st, out = oracle_mod.decompress(enc[:n])
            assert st in (8, 9) and out == b"", (name, n)
            blobs.append(enc)
            in_lens.append(n)
            caps.append(len(raw))
            want_st.append(st)
            want.append(out)
            if j % 3 == 1:  # a good stream between them
                r, e = good[g % len(good)]
                g += 1
                blobs.append(e)
                in_lens.append(len(e))
                caps.append(len(r))
                want_st.append(0)
                want.append(r)
    assert want_st.count(9) == 6 * 9 and want_st.count(8) == 6 * 3 and want_st.count(0) == 6 * 4
    _check(_launch(torch, hc.decompress_batch, blobs, caps, rot, base_res, in_lens=in_lens), caps, want_st, want)


# -------------------------------------------------------------- d. capacity at the edge ----

def _edge_streams(oracle_mod):
    s = {name: (raw, enc) for name, raw, enc in gp.trunc_streams(oracle_mod)}
    assert len(s["grad 64x48 -m"][1]) == 63  # long runs: the decoder's run stores
    return [(s["grad 64x48 -m"], True), (s["noise 37x29"], False)], s["photo 41x33"], s["photo 41x33 -m"]


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_decode_capacity_short_by_d(gpu, hc, oracle_mod, rot):
    """out_caps = need - d: HC_ERR_CAPACITY, out_lens = need, no byte behind the short slot
    written, and the good stream in the slot directly behind it is right. What is inside the short
    slot is open (the header does not say)."""
    torch = gpu
    base_res = 4 * ((rot + 1) % 4)
    edge, nb0, nb1 = _edge_streams(oracle_mod)
    blobs, caps, want_st, want, open_slots = [], [], [], [], []
    for (raw, enc), _ in edge:
        for d in (1, 15, 16, 17, 64):
            for nraw, nenc in (nb0, nb1, (raw, enc)):  # every d with each kind of neighbour
                open_slots.append(len(blobs))
                blobs += [enc, nenc]
                caps += [len(raw) - d, len(nraw)]
                want_st += [hc.HC_ERR_CAPACITY, 0]
                want += [len(raw), nraw]
    _check(_launch(torch, hc.decompress_batch, blobs, caps, rot, base_res), caps, want_st, want, set(open_slots))


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_encode_capacity_short_by_d(gpu, hc, oracle_mod, rot):
    torch = gpu
    base_res = 4 * ((rot + 1) % 4)
    edge, nb0, nb1 = _edge_streams(oracle_mod)
    for (raw, enc), use_diff in edge:
        nb = nb1 if use_diff else nb0
        blobs, caps, want_st, want, open_slots = [], [], [], [], []
        for d in (1, 2, 3, 4, 5):
            for nraw, nenc in (nb, (raw, enc)):
                open_slots.append(len(blobs))
                blobs += [raw, nraw]
                caps += [len(enc) - d, len(nenc)]
                want_st += [hc.HC_ERR_CAPACITY, 0]
                want += [len(enc), nenc]
        _check(_launch(torch, hc.compress_batch, blobs, caps, rot, base_res, use_diff=use_diff),
               caps, want_st, want, set(open_slots))


# ------------------------------------------------------------------- e. adaptive batch ----

ADAPT = [("photo", 132, 130), ("photo", 129, 131), ("grad", 257, 40), ("runs", 129, 9), ("photo", 136, 72),
         ("flat", 64, 64), ("photo", 8, 8), ("noise", 12, 10)]


def _adapt(oracle_mod, use_diff):
    key = ("adapt", use_diff)
    if key not in _cache:
        raws = [_mat(oracle_mod, k, w, h, i) for i, (k, w, h) in enumerate(ADAPT)]
        assert len(raws[0]) > 16384 and len(raws[1]) > 16384  # more than one 16 KiB chunk
        encs = []
        for r, (_, w, _) in zip(raws, ADAPT):
            st, e = oracle_mod.compress(r, use_diff, True, w)
            assert st == 0 and oracle_mod.decompress(e) == (0, r)
            encs.append(e)
        _cache[key] = (raws, encs)
    return _cache[key]


def _adapt_launch(torch, hc, encode, blobs, caps, rot, base_res, widths=None, use_diff=False):
    """an adaptive call with the guarded workspace of exactly the published bound"""
    n, total_in = len(blobs), sum(len(b) for b in blobs)
    if encode:
        need = int(hc.lib().hc_adapt_compress_work_bound(total_in, n))
        w = gp.dev_i64(torch, widths)
        call = lambda *a: hc.compress_adapt_batch(*a[:3], w, *a[3:], use_diff=use_diff, work=work)
    else:
        need = int(hc.lib().hc_adapt_decompress_work_bound(total_in, sum(caps), n))
        call = lambda *a: hc.decompress_adapt_batch(*a, work=work)
    whole, work = gp.guarded_work(torch, need)
    assert work.numel() == need and work.data_ptr() % 16 == 0
    res = _launch(torch, call, blobs, caps, rot, base_res)
    assert gp.work_guard_untouched(whole, need), "a write outside the workspace of the published bound"
    return res


@pytest.mark.parametrize("use_diff", [False, True])
@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_adapt_batch_exact_capacities(gpu, hc, oracle_mod, rot, use_diff):
    torch = gpu
    base_res = 4 * ((rot + 1) % 4)
    raws, encs = _adapt(oracle_mod, use_diff)
    caps = [len(e) for e in encs]
    res = _adapt_launch(torch, hc, True, raws, caps, rot, base_res, widths=[w for _, w, _ in ADAPT], use_diff=use_diff)
    _check(res, caps, [0] * len(raws), encs)
    caps = [len(r) for r in raws]  # W * H
    _check(_adapt_launch(torch, hc, False, encs, caps, rot, base_res), caps, [0] * len(raws), raws)


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_adapt_decode_malformed_between_good(gpu, hc, oracle_mod, vectors, rot):
    """the recorded malformed adaptive streams (tests/golden/vectors.json), each between two good
    ones: the recorded statuses, the neighbours' bytes, and both guards"""
    torch = gpu
    base_res = 4 * ((rot + 1) % 4)
    bad = [(bytes.fromhex(v["input"]), v["rc"]) for v in vectors["decompress"]]
    bad = [(b, rc) for b, rc in bad if len(b) >= 9 and (b[8] & 0x40)]
    assert sorted({rc for _, rc in bad}) == [9, 10, 11, 13, 14, 15]
    good = [p for d in (False, True) for p in zip(*_adapt(oracle_mod, d))][2:]  # (the two largest: once is enough)
    blobs, caps, want_st, want, open_slots = [], [], [], [], []
    for j, (b, rc) in enumerate(bad):
        r, e = good[j % len(good)]
        blobs += [e, b]
        caps += [len(r), 1 << 20]
        want_st += [0, rc]
        want += [r, None]
        open_slots.append(len(blobs) - 1)
    blobs.append(good[-1][1])
    caps.append(len(good[-1][0]))
    want_st.append(0)
    want.append(good[-1][0])
    st, olens, dout, ooffs = _adapt_launch(torch, hc, False, blobs, caps, rot, base_res)
    assert st == want_st
    want = [w if w is not None else olens[i] for i, w in enumerate(want)]
    _check((st, olens, dout, ooffs), caps, want_st, want, set(open_slots))


# --------------------------------------------------------------------- f. pack_batch ----

def test_pack_batch_any_byte_alignment(gpu, hc):
    torch = gpu
    rng = np.random.default_rng(5)
    lens = list(range(71)) + [1000, 1023, 4097]
    n = len(lens)
    sres = [(5 * i + 3) % 16 for i in range(n)]
    dres = [(7 * i + i // 16) % 16 for i in range(n)]  # (i // 16: every source - destination shift, too)
    assert set(sres) == set(range(16)) == set(dres) and len({(a - b) % 16 for a, b in zip(sres, dres)}) == 16
    # laid out in a shuffled order, so the offsets of range 0, 1, 2, ... go up and down
    sperm, dperm = rng.permutation(n), rng.permutation(n)
    soffs, doffs = [0] * n, [0] * n
    so, stotal = gp.layout_bytes([lens[i] for i in sperm], [sres[i] for i in sperm])
    do, dtotal = gp.layout_bytes([lens[i] for i in dperm], [dres[i] for i in dperm], gap=1)
    for k in range(n):
        soffs[sperm[k]], doffs[dperm[k]] = so[k], do[k]
    assert soffs != sorted(soffs) and doffs != sorted(doffs)
    assert [o % 16 for o in soffs] == sres and [o % 16 for o in doffs] == dres
    gp.check_disjoint(doffs, lens)
    src_host = rng.integers(0, 256, size=stotal, dtype=np.uint8)  # the gaps hold live bytes, too
    blobs = [src_host[o:o + m].tobytes() for o, m in zip(soffs, lens)]
    for sbase, dbase in ((0, 0), (3, 5), (13, 10)):
        src = gp.fill(torch, blobs, soffs, stotal, sbase, src_host)
        dst = gp.fill(torch, [b""] * n, doffs, dtotal, dbase, OUT_POISON)
        hc.pack_batch(src, gp.dev_i64(torch, soffs), gp.dev_i64(torch, lens), dst, gp.dev_i64(torch, doffs))
        torch.cuda.synchronize()
        assert gp.slots(dst, doffs, lens) == blobs, (sbase, dbase)
        assert gp.outside_untouched(dst, doffs, lens, OUT_POISON), gp.touched(dst, doffs, lens, OUT_POISON)


# ---------------------------------------------------------------- g. rejected arguments ----

@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("which", ["in", "out"])
def test_misaligned_base_is_rejected_on_the_host(gpu, hc, oracle_mod, which, off):
    """a base that is not 4-aligned: HC_ERR_ARG from all four calls, nothing launched -- the status
    and length tensors and the poisoned output are as they were. (Per-stream offsets that are not
    multiples of 4 are outside the contract and none is passed.)"""
    torch = gpu
    raws, encs = _raws(oracle_mod)[10:20], _encs(oracle_mod, False)[10:20]
    araws, aencs = _adapt(oracle_mod, False)
    araws, aencs, widths = araws[3:], aencs[3:], gp.dev_i64(torch, [w for _, w, _ in ADAPT[3:]])
    calls = [
        (raws, [len(e) for e in encs], hc.compress_batch),
        (encs, [len(r) for r in raws], hc.decompress_batch),
        (araws, [len(e) for e in aencs], lambda *a: hc.compress_adapt_batch(*a[:3], widths, *a[3:])),
        (aencs, [len(r) for r in araws], hc.decompress_adapt_batch),
    ]
    for blobs, caps, call in calls:
        n = len(blobs)
        sizes = [len(b) for b in blobs]
        ioffs, itotal = gp.layout(sizes, 1, 0)
        ooffs, ototal = gp.layout(caps, 1, 0)
        din = gp.fill(torch, blobs, ioffs, itotal, off if which == "in" else 4, 0x3C)
        dout = gp.fill(torch, [b""] * n, ooffs, ototal, off if which == "out" else 4, OUT_POISON)
        assert (din if which == "in" else dout).data_ptr() % 4 == off
        olens = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        with pytest.raises(hc.HCodecError, match=str(hc.HC_ERR_ARG)):
            call(din, gp.dev_i64(torch, ioffs), gp.dev_i64(torch, sizes), dout, gp.dev_i64(torch, ooffs),
                 gp.dev_i64(torch, caps), olens, st)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [-1] * n and olens.cpu().tolist() == [-1] * n
        assert gp.outside_untouched(dout, [], [], OUT_POISON), gp.touched(dout, [], [], OUT_POISON)
