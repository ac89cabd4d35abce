"""A forging FGK encoder: streams that no encoder writes but the reference accepts, on the slot-form
tree of tests/fgk_cache_model.py.

The forged class is the NYT escape for a known symbol: the NYT leaf's code followed by 8 raw bits
that name a symbol which already has a leaf. The reference does not split then
(huffman.cpp:95-128: `symbolNodes[symbol]` is set, so the symbol's own leaf is updated), and the
decoder kernels have code for this case alone (hc_fgk.hip: Fgk::find_leaf and the `chase(known)`
branch of Dec::finish_symbol), which every fast path has to reach in a consistent state.

  forge(symbols, esc)            the bits: symbol i goes through the NYT when it is unseen or
                                 esc[i] is set, by its own code otherwise
  container(symbols, esc, flags) <u64 LE count><u8 flags><bits, zero-padded>
  count_known_escapes(payload, count)
                                 decodes and counts the NYT escapes that named a known symbol
  vectors()                      the test streams (fixed seeds; at most 4096 symbols each)
  truncations(symbols, esc)      one of them cut inside an escape
  forged_containers(), truncated_containers()
                                 the containers the CPU and GPU tests share

Plain Python. Test infrastructure only.
"""
import random

from fgk_cache_model import INNER, NYT, ROOT, Tree

MAX_SYMBOLS = 4096
SMALL_NYT = ROOT - 32  # kSmallNyt: the small-alphabet decoder works while nyt >= this (16 symbols)


def _code(t, x):
    return [p & 1 for p in reversed(t.path(x))]


def forge(symbols, esc, info=None):
    """-> the bits (a list of 0 / 1). info: a list that gets, for every escape of a known symbol,
    (index, nyt position, depth of the symbol's own leaf, depth of the NYT)"""
    t = Tree()
    bits = []
    for i, s in enumerate(symbols):
        seen = t.where[s] != 0
        if not seen or esc[i]:
            code = _code(t, t.nyt)
            if seen and info is not None:
                info.append((i, t.nyt, len(t.path(t.where[s])), len(code)))
            bits += code
            bits += [(s >> k) & 1 for k in range(7, -1, -1)]
            if not seen:
                t.split(s)
        else:
            bits += _code(t, t.where[s])
        t.update(t.where[s])
    return bits


def pack_bits(bits):
    """most significant bit first, zero-padded to a byte"""
    out = bytearray((len(bits) + 7) // 8)
    for i, b in enumerate(bits):
        if b:
            out[i >> 3] |= 0x80 >> (i & 7)
    return bytes(out)


def wrap(count, flags, bits):
    return int(count).to_bytes(8, "little") + bytes([flags]) + pack_bits(bits)


def container(symbols, esc, flags=0):
    return wrap(len(symbols), flags, forge(symbols, esc))


def _bit(payload, pos):
    return (payload[pos >> 3] >> (7 - (pos & 7))) & 1


def decode(payload, count):
    """-> (symbols, known escapes, whole): the first `count` symbols of `payload` by the same tree;
    the decode stops where the bits end (a stream cut short or damaged: whole is False)"""
    nbits = len(payload) * 8
    t = Tree()
    pos = known = 0
    out = []
    for _ in range(count):
        x = ROOT
        while t.body[x] & INNER:
            if pos >= nbits:
                return out, known, False
            x = (t.body[x] & 255) * 2 + _bit(payload, pos)
            pos += 1
        if t.body[x] & NYT:
            if pos + 8 > nbits:
                return out, known, False
            s = 0
            for k in range(8):
                s = (s << 1) | _bit(payload, pos + k)
            pos += 8
            if t.where[s]:
                known += 1
            else:
                t.split(s)
        else:
            s = t.body[x]
        out.append(s)
        t.update(t.where[s])
    return out, known, True


def count_known_escapes(payload, count):
    """how many NYT escapes among the first `count` symbols of `payload` name a known symbol"""
    return decode(payload, count)[1]


# ------------------------------------------------------------------------- the vectors ----

def _fib(n):
    out, a, b = [], 1, 1
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def _known_mask(symbols):
    seen, out = set(), []
    for s in symbols:
        out.append(s in seen)
        seen.add(s)
    return out


def _sprinkle(symbols, rate, seed, only=None):
    """esc with about `rate` of the known occurrences (of the symbols in `only`, if given) set"""
    rng = random.Random(seed)
    return [bool(k and (only is None or s in only) and rng.random() < rate)
            for s, k in zip(symbols, _known_mask(symbols))]


def _weighted(values, weights, n, seed):
    rng = random.Random(seed)
    return rng.choices(values, weights=weights, k=n)


def _skewed(seed, n_sym=16, first=2, step=7):
    """Fibonacci counts in a fixed-seed order: symbol k occurs fib(k) times (the last ones hot)"""
    rng = random.Random(seed)
    out = []
    for k, c in enumerate(_fib(n_sym)):
        out += [(first + k * step) & 255] * c
    rng.shuffle(out)
    return out


def _skewed_esc(symbols, seed, hot_rate=0.08, rare_rate=0.6):
    """escapes on the three hottest symbols (their updates run through the shallow, cached part of
    the tree) and on the rare ones (codes longer than 8 bits)"""
    count = {}
    for s in symbols:
        count[s] = count.get(s, 0) + 1
    by = sorted(count, key=lambda s: -count[s])
    hot, rare = set(by[:3]), {s for s in by if count[s] <= 8}
    rng = random.Random(seed)
    return [bool(k and ((s in hot and rng.random() < hot_rate) or (s in rare and rng.random() < rare_rate)))
            for s, k in zip(symbols, _known_mask(symbols))]


SECOND_AT = (2, 3, 9, 17)  # the first known-symbol escape is this symbol of the stream (1-based)
PHASES = 64
_cache = {}


def vectors():
    """[(name, symbols, esc)], computed once. tests/test_forge_model.py asserts what each holds."""
    if "v" in _cache:
        return _cache["v"]
    out = []
    # -- second symbol: root -> (NYT, s), the code is 0 + 8 bits; then the first known escape as
    # symbol 2, 3, 9 and 17 behind distinct new symbols (17: the NYT stands at kSmallNyt exactly),
    # with a tail of old, new and escaped symbols. The escape leaves the NYT where it is while
    # the small-alphabet decoder's count of symbols seen goes on.
    out.append(("second", [65, 65], [False, True]))
    out.append(("second-control", [65, 65], [False, False]))
    for k in SECOND_AT:
        head = [(40 + 3 * j) & 255 for j in range(k - 1)]
        sym = head + [head[(k - 2) // 2]]
        esc = [False] * (k - 1) + [True]
        rng = random.Random(100 + k)
        pool = head + [201, 202, 203]
        for _ in range(40):
            s = rng.choice(pool)
            sym.append(s)
            esc.append(rng.random() < 0.3)
        out.append(("first@%d" % k, sym, esc))
    # -- small alphabet with escapes: four values, skewed so that the rate stays under 2.5 bits a
    # symbol and the rate rule picks the small-alphabet launch by itself
    sym = _weighted([1, 2, 3, 7], [70, 18, 8, 4], 3000, 11)
    out.append(("small4", sym, _sprinkle(sym, 0.05, 12)))
    # the same, and the alphabet grows past 16 symbols from the middle on (the small decoder
    # hands over to the regular one), escapes on both sides
    sym = _weighted([1, 2, 3, 7], [70, 18, 8, 4], 1500, 13)
    sym += _weighted([1, 2, 3, 7] + list(range(100, 120)), [700, 180, 80, 40] + [1] * 20, 1500, 14)
    out.append(("small-grow", sym, _sprinkle(sym, 0.05, 15)))
    # -- noise: deep codes, the batch steps mostly off
    rng = random.Random(21)
    sym = [rng.randrange(256) for _ in range(3000)]
    out.append(("noise", sym, _sprinkle(sym, 0.05, 22)))
    # -- skewed, the hot symbols escaped (swaps of table levels) and some rare ones (deep -> walk)
    sym = _skewed(31)
    out.append(("skewed", sym, _skewed_esc(sym, 32)))
    sym = _skewed(33, n_sym=15, first=9, step=11)
    out.append(("skewed15", sym, _skewed_esc(sym, 34, hot_rate=0.15)))
    # -- full alphabet: all 256 symbols once, then 1500 with escapes (the NYT at position 0)
    rng = random.Random(41)
    head = list(range(256))
    rng.shuffle(head)
    tail = [rng.randrange(256) if rng.random() < 0.5 else rng.choice((3, 5, 250)) for _ in range(1500)]
    out.append(("full", head + tail, [False] * 256 + [rng.random() < 0.08 for _ in tail]))
    # -- escape runs: 64 escapes in a row, of one symbol and of two in turn
    head = _weighted([5, 6, 9, 12, 40, 77], [40, 25, 15, 10, 6, 4], 60, 51)
    tail = _weighted([5, 6, 9, 12, 40, 77], [40, 25, 15, 10, 6, 4], 60, 52)
    for name, run in (("run-same", [5] * 64), ("run-alt", [5, 6] * 32), ("run-rare", [77] * 64)):
        sym = head + [77] + run + tail
        out.append((name, sym, [False] * (len(head) + 1) + [True] * 64 + [False] * len(tail)))
    # -- window phase: one skewed stream behind 0..63 common symbols (1 bit each after the first),
    # so that the escapes' NYT codes and raw bits start at every bit offset of the 64-bit window
    short = _skewed(61, n_sym=13)
    short_esc = _skewed_esc(short, 62, hot_rate=0.2)
    common = max(set(short), key=short.count)
    for pre in range(PHASES):
        out.append(("phase%d" % pre, [common] * pre + short, [False] * pre + short_esc))
    # -- as MNP-5 symbols (the run-length revert reads these lists): the escaped symbol is the
    # third equal symbol of a run, so that the next one is a count; and the count itself
    for seed, (name, role) in enumerate((("mnp5-third", "third"), ("mnp5-count", "count"), ("mnp5-both", None))):
        rng = random.Random(71 + seed)
        sym, rep, prev = [], 0, -1
        while len(sym) < 1200:
            if rep == 3:
                s, rep = rng.choice((0, 1, 2, 3, 4, 9, 30)), 0  # a count: a symbol seen as a literal, too
                sym.append(s)
                prev = -1
                continue
            s = prev if prev >= 0 and rng.random() < 0.7 else rng.choice((0, 1, 2, 3, 4, 9, 30, 31))
            rep = rep + 1 if s == prev else 1
            sym.append(s)
            prev = s
        roles = mnp5_roles(sym)
        known = _known_mask(sym)
        rate = 0.5 if role else 0.25
        esc = [bool(k and (r == role or role is None) and rng.random() < rate) for k, r in zip(known, roles)]
        out.append((name, sym, esc))
    assert all(len(s) == len(e) and len(s) <= MAX_SYMBOLS for _, s, e in out)
    _cache["v"] = out
    return out


def mnp5_roles(symbols):
    """per symbol what the run-length revert takes it for (transform.cpp:137-159): 'lit', 'third'
    (the third equal literal: a count follows) or 'count'"""
    out, byte, seen = [], None, 0
    for s in symbols:
        if seen == 3:
            out.append("count")
            seen = 0
            continue
        if s == byte:
            seen += 1
        else:
            byte, seen = s, 1
        out.append("third" if seen == 3 else "lit")
    return out


def truncations(symbols, esc):
    """[(tag, count, bits)]: the stream cut inside its middle known-symbol escape, which becomes
    the last symbol (count = its index + 1): after the NYT code, after 1..7 of the raw bits (the
    padding of the last byte then stands for the missing ones, where it reaches), and on the byte
    that ends it with the whole count (the symbols behind it are missing)"""
    info = []
    bits = forge(symbols, esc, info)
    if not info:
        return []
    i = info[len(info) // 2][0]
    start = len(forge(symbols[:i], esc[:i]))
    nyt_len = info[len(info) // 2][3]
    out = [("nyt", i + 1, bits[:start + nyt_len])]
    out += [("raw%d" % r, i + 1, bits[:start + nyt_len + r]) for r in range(1, 8)]
    end = start + nyt_len + 8
    out.append(("byte", len(symbols), bits[:(end + 7) // 8 * 8]))
    out.append(("byte-last", i + 1, bits[:(end + 7) // 8 * 8]))
    return out


def forged_containers():
    """[(name, container)]: every vector with flags 0x00, and with 0x80 all but the phase set"""
    if "c" not in _cache:
        out = []
        for name, sym, esc in vectors():
            bits = forge(sym, esc)
            for flags in (0x00, 0x80) if not name.startswith("phase") else (0x00,):
                out.append(("%s/%02x" % (name, flags), wrap(len(sym), flags, bits)))
        _cache["c"] = out
    return _cache["c"]


def truncated_containers():
    """[("vector:cut", container)] of the cuts inside an escape, flags 0x00"""
    if "t" not in _cache:
        out = []
        for name, sym, esc in vectors():
            for tag, count, bits in truncations(sym, esc):
                out.append(("%s:%s" % (name, tag), wrap(count, 0, bits)))
        _cache["t"] = out
    return _cache["t"]
