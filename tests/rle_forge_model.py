"""Forged MNP-5 symbol streams for the decoders' run revert (hc_fgk.hip: revert_block).

The encoder writes a count only where its input puts one, always maximal, and a run's step and
length are its input's. Here the symbol streams are written by hand, so a test can choose what the
run revert sees: the run's first byte at every address residue mod 16 with every length around
the 16-byte units (align), 1..64 runs in one 256-symbol block with zero counts between them and
the count at each byte of its lane (density), runs and machine states across block boundaries
(carry), and seeded random streams over small alphabets (random). A container is
<u64 LE symbol count><flags> + the FGK code of the symbols (the oracle's encoder); flags 0x00
reverts the RLE alone, 0x80 the diff model behind it, where a run of `v` is an arithmetic
sequence of step `v`.

`blocks(symbols)` reports what a vector reaches, from the reference's serial machine
(transform.cpp:137-159) restated as a loop: per 256-symbol block the state carried in, the runs
as (output offset in the block, length, run byte), the block indices that hold a count, and the
bytes produced. tests/test_rle_forge_model.py asserts the census on the CPU; the GPU side is
tests/test_gpu_rle_forge.py.
"""
import random

ALIGN_COUNTS = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 66, 79, 80, 81, 128, 240, 254, 255)
STEPS = (0, 1, 2, 63, 64, 85, 127, 128, 129, 170, 254, 255)
ALIGN_CROSS = ((5, 255), (0, 64), (15, 17))          # (p, c) that take every v = 0..255
DENSITY_RUNS = (1, 2, 15, 16, 17, 31, 32, 33, 48, 63, 64)
DENSITY_COUNTS = (1, 5, 15, 16, 17, 40, 255)         # the non-zero ones; 0 fills the other slots
DENSITY_GROUPS = 160                                 # 640 symbols: two blocks and a half
CARRY_COUNTS = (0, 1, 255)
EXACT_LENGTHS = (0, 1, 255, 256, 257, 512, 513)
FAMILIES = ("align", "density", "carry", "random")

_cache = {}


def _fill(n, avoid, k=0):
    """n literals that form no run and never equal `avoid`"""
    a, b = (avoid + 1 + k) & 255, (avoid + 3 + k) & 255
    return [a if i & 1 else b for i in range(n)]


def _align():
    out = []
    for p in range(16):
        for ci, c in enumerate(ALIGN_COUNTS):
            v = STEPS[(p * len(ALIGN_COUNTS) + ci) % len(STEPS)]
            out.append(("align/p%d-c%d-v%d" % (p, c, v), _fill(p, v) + [v, v, v, c] + _fill(2, v, 4)))
    for p, c in ALIGN_CROSS:
        for v in range(256):
            out.append(("align/cross-p%d-c%d-v%d" % (p, c, v), _fill(p, v) + [v, v, v, c] + _fill(2, v, 4)))
    return out


def _groups(rng, k, counts_of_block):
    """k literals, DENSITY_GROUPS groups `v v v c` back to back (v changes per group), two literals;
    counts_of_block(block, slots) -> the counts of the groups whose count symbol lies in that block"""
    at = [k + 3 + 4 * g for g in range(DENSITY_GROUPS)]
    counts = []
    for b in range(at[-1] // 256 + 1):
        slots = sum(1 for i in at if i // 256 == b)
        counts += counts_of_block(b, slots)
    sym, v = [], rng.randrange(256)
    first = v
    for c in counts:
        sym += [v, v, v, c]
        v = (v + rng.choice((1, 2, 37, 128, 255))) & 255
    return _fill(k, first) + sym + _fill(2, sym[-4], 4)


def _density():
    out = []
    for runs in DENSITY_RUNS:
        for k in range(4):
            rng = random.Random(1000 * runs + k)

            def counts(block, slots, rng=rng, runs=runs):
                c = [rng.choice(DENSITY_COUNTS) for _ in range(min(runs, slots))] + [0] * max(0, slots - runs)
                rng.shuffle(c)
                return c
            out.append(("density/r%d-k%d" % (runs, k), _groups(rng, k, counts)))
    for k in range(4):
        out.append(("density/all255-k%d" % k, _groups(random.Random(77 + k), k, lambda b, slots: [255] * slots)))
    return out


def _carry():
    out = []
    for edge in (256, 512):
        for s in range(5):
            for c in CARRY_COUNTS:
                v = (40 * s + c + edge) & 255
                head = _fill(edge - s, v)
                if edge == 512:  # block 0 ends in a run: with the diff model its last byte is carried
                    head[252:256] = [7, 7, 7, 200]
                out.append(("carry/edge%d-s%d-c%d" % (edge, s, c), head + [v, v, v, c] + _fill(3, v, 4)))
    for n in (256, 100, 300, 512):  # the stream ends in state 3: at a block end, mid-block
        out.append(("carry/end3-n%d" % n, _fill(n - 3, 50) + [50, 50, 50]))
    for n in EXACT_LENGTHS:
        rng = random.Random(300 + n)
        out.append(("carry/len%d" % n, [rng.choice((0, 3, 255)) for _ in range(n)]))
    for n in range(250, 266):  # count value, run byte and the literal behind it all equal
        out.append(("carry/nines%d" % n, [9] * n))
    return out


def _random():
    alphabets = [list(range(2)), list(range(3)), list(range(5)), list(range(256)), [0, 255], [0, 1, 255]]
    out = []
    for t in range(198):
        rng = random.Random(5000 + t)
        alpha = alphabets[t % len(alphabets)]
        n = rng.randrange(0, 1101)
        out.append(("random/%03d-a%d-n%d" % (t, len(alpha), n), [rng.choice(alpha) for _ in range(n)]))
    for t in range(6):
        rng = random.Random(6000 + t)
        alpha = alphabets[t]
        n = 5000 + rng.randrange(-40, 40)
        out.append(("random/big%d-a%d-n%d" % (t, len(alpha), n), [rng.choice(alpha) for _ in range(n)]))
    return out


def vectors():
    """[(name, symbols)]; the name starts with the family"""
    if "v" not in _cache:
        v = [(name, bytes(sym)) for name, sym in _align() + _density() + _carry() + _random()]
        assert len({name for name, _ in v}) == len(v)
        _cache["v"] = v
    return _cache["v"]


def family(name):
    return name.split("/")[0]


def containers(oracle_mod=None):
    """[(name/00 | name/80, container)]: every vector with flags 0x00 and 0x80"""
    if "c" not in _cache:
        if oracle_mod is None:
            import oracle as oracle_mod
        out = []
        for name, sym in vectors():
            payload, _ = oracle_mod.fgk_encode(sym)
            head = len(sym).to_bytes(8, "little")
            out += [("%s/%02x" % (name, flags), head + bytes([flags]) + payload) for flags in (0x00, 0x80)]
        _cache["c"] = out
    return _cache["c"]


def symbols_of(name):
    """the symbols behind a vector's or a container's name"""
    if "by_name" not in _cache:
        _cache["by_name"] = dict(vectors())
    return _cache["by_name"][name[:-3] if name.endswith(("/00", "/80")) else name]


def blocks(symbols):
    """the serial machine over the stream, reported per block of 256 symbols ->
    [{"state": seen count carried in, "runs": [(output offset in the block, length, run byte)],
      "counts": [block index of every count symbol], "lanes": [the lane (of 64, four symbols
      each) that holds it], "out": bytes produced}]"""
    res = []
    seen, byte = 0, 0
    for i, s in enumerate(symbols):
        if i % 256 == 0:
            res.append({"state": seen, "runs": [], "counts": [], "lanes": [], "out": 0})
        blk = res[-1]
        if seen == 3:
            blk["counts"].append(i % 256)
            blk["lanes"].append(i % 256 // 4)
            blk["runs"].append((blk["out"], s, byte))
            blk["out"] += s
            seen = 0
        else:
            seen = seen + 1 if s == byte else 1
            byte = s
            blk["out"] += 1
    return res


def final_state(symbols):
    """the machine's state behind the last symbol"""
    seen, byte = 0, 0
    for s in symbols:
        if seen == 3:
            seen = 0
        else:
            seen = seen + 1 if s == byte else 1
            byte = s
    return seen


def expand(symbols, diff):
    """the bytes the stream stands for: the same machine, then prefix sums mod 256 with the diff model"""
    out = bytearray()
    seen, byte = 0, 0
    for s in symbols:
        if seen == 3:
            out += bytes([byte]) * s
            seen = 0
        else:
            seen = seen + 1 if s == byte else 1
            byte = s
            out.append(s)
    if diff:
        acc = 0
        for i, d in enumerate(out):
            acc = (acc + d) & 255
            out[i] = acc
    return bytes(out)
