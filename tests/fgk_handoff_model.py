"""Model of the encoder's regular batch step with its hand-offs (hc_fgk.hip code_all_batch:
HC_ENC_HANDOFF_MISS, HC_ENC_HANDOFF_LEVEL), on the slot-form tree and path cache of
tests/fgk_cache_model.py and the tentative test of tests/fgk_batch_model.py.

A step takes up to seven symbols, nine lanes each (lane 9 j + l: level l of symbol j's cached
path). Every path position of every step symbol gets its increment first, so symbol j's test at
position a sees all step symbols through a and none through a + 1 (tentative_len's test, here over
every cached group of the step, the ones behind an uncached symbol included, as the kernel's
lanes run it). The first failing lane fl ends the step at symbol jf = fl // 9:

* an uncached symbol (its group's first lane): coded from scratch (miss), its byte and where[]
  word taken from the step's lanes -- nothing the model can see changes;
* a cached symbol whose level l = fl % 9 reported: the increments of its levels below l STAY (they
  passed a test that passes no level that fails), its code comes from the step's row, and the walk
  starts at level l with the row as the known path, repeating the exact leader test there (the
  report is false when the one-symbol loop's test passes the level on the tree as the earlier
  symbols left it).

The kernel ships with the first hand-off on and the second off (it is bit-exact and did not
pay): encode(handoff=False) is the shipped step, which takes the failing
symbol's increments back and tests all its levels again; handoff=True is the kernel built with
-DHC_ENC_HANDOFF_LEVEL=1. Both give the same codes and the same tree.

The symbols before jf commit. encode() runs this in lockstep with the plain Tree.update and
asserts at every symbol that the code about to be sent and the tree are the plain loop's. It also
follows the record lanes (RecSink::n: a step starts with at most 57 records pending, a hand-off's
record may fill lane 63) and the coding passes (`chunk` symbols each: the kernel codes the symbols
of one 256-byte chunk per pass when the stream has no runs), and counts the states steps end in.
"""
from collections import Counter

from fgk_batch_model import BATCH
from fgk_cache_model import ROOT, PathCache, Tree, _word, lanes_update

LANES = 9         # lanes (levels) per step symbol
INSERT_DEPTH = 9  # the deepest path a miss caches (kInsertDepth): every cached path fits a group


def walk(t, s, pv, swaps):
    """Fgk::walk(s, pv) (fgk_cache_model.kernel_walk, keeping the swaps for the path cache): the
    exact level at s, then the climb chased back onto the known path pv (ROOT last) and finished
    lane-parallel; a level reported there is walked in turn"""
    while True:
        f = t.w[s]
        lead = s
        while t.w[lead + 1] == f:
            lead += 1
        if lead != s and lead != t.up[s]:
            a, c = t.body[s], t.body[lead]
            t.body[s], t.body[lead] = c, a
            t.relink(c, s)
            t.relink(a, lead)
            swaps.append((s, lead))
            s = lead
        t.w[s] += 1
        c, td = t.up[s], []
        while c not in pv:
            td.append(c)
            c = t.up[c]
        path = td + pv[pv.index(c):]
        k = lanes_update(t, path)
        if k is None:
            return
        s, pv = path[k], path


def _records(nbits):
    """RecSink::push_bits: records of at most 24 bits"""
    return (nbits + 23) // 24


def same_tree(a, b):
    return a.w == b.w and a.body == b.body and a.up == b.up and a.where == b.where and a.nyt == b.nyt


def encode(symbols, chunk=256, handoff=True, lockstep=True):
    """(codes, tree, states): every symbol's code bits, the final tree, and a Counter of the
    states steps ended in:
      ("miss", j) / ("fresh", j): symbol j uncached with / without a leaf (a split);
      ("level", j, l): cached symbol j, level l reported; ("false", j, l): ... falsely;
      ("fill64",): a level hand-off's record filled lane 63 (pack follows);
      ("short", kind): the step was the last of a pass with fewer than seven symbols left and
      ended at a symbol coded alone (kind "miss" / "fresh" / "level"); ("steps",), ("alone",).
    handoff=False: the symbol that ends a step is coded as the parent kernel did (its increments
    all taken back, every level tested again)."""
    t, ref = Tree(), Tree()
    pc = PathCache()
    codes = []
    st = Counter()
    n = 0  # records pending (sink.n)

    def push(k=1):
        nonlocal n
        filled = False
        for _ in range(k):
            n += 1
            if n == 64:
                n, filled = 0, True
        return filled

    def send(sym, code):
        """the code about to be sent against the plain loop's, which then updates its tree"""
        codes.append(code)
        if not lockstep:
            return
        fresh = ref.where[sym] == 0
        if fresh:
            ref.split(sym)
        x = ref.where[sym]
        want = [p & 1 for p in reversed(ref.path(x))]
        if fresh:
            want = want[:-1] + [(sym >> k) & 1 for k in range(7, -1, -1)]
        assert code == want, (len(codes) - 1, sym, code, want)
        ref.update(x)

    def check(at):
        assert not lockstep or same_tree(t, ref), at

    def after_swaps(swaps):
        for s, lead in swaps:
            pc.on_swap(s, lead)

    def miss(sym):
        fresh = t.where[sym] == 0
        if fresh:
            t.split(sym)
        x = t.where[sym]
        pv = t.path(x)
        d = len(pv)
        if d <= INSERT_DEPTH:
            pc.insert(sym, pv)
        code = [p & 1 for p in reversed(pv)]
        send(sym, code[:-1] + [(sym >> k) & 1 for k in range(7, -1, -1)] if fresh else code)
        swaps = []
        if d > INSERT_DEPTH:
            walk(t, x, pv + [ROOT], swaps)
        else:
            k = lanes_update(t, pv + [ROOT])
            if k is not None:
                walk(t, pv[k], pv + [ROOT], swaps)
        after_swaps(swaps)
        push(_records(d - 1) + 1 if fresh else _records(d))
        return fresh

    for p0 in range(0, len(symbols), chunk):
        syms = symbols[p0:p0 + chunk]
        ns, i = len(syms), 0
        while i < ns:
            if n > 64 - BATCH:
                n = 0  # pack
            st["steps",] += 1
            jmax = min(BATCH, ns - i)
            rows = []
            for s_ in syms[i:i + jmax]:
                e = pc.slot.get(s_) if t.where[s_] else None
                rows.append(None if e is None else pc.ent[e][1])
            cnt = Counter(a for r in rows if r is not None for a in r)
            jf, lf = jmax, None
            for j, r in enumerate(rows):
                if r is None:
                    jf, lf = j, -1
                    break
                for l, a in enumerate(r):
                    if _word(t, a + 1) < _word(t, a) + 1024 * cnt[a]:
                        jf, lf = j, l
                        break
                if lf is not None:
                    break
            for j in range(jf):  # the symbols before jf commit
                send(syms[i + j], [a & 1 for a in reversed(rows[j])])
                for a in rows[j]:
                    t.w[a] += 1
                t.w[ROOT] += 1
                check(p0 + i + j)
            n += jf
            i += jf
            if jf == jmax:
                continue
            st["alone",] += 1
            sym = syms[i]
            if lf < 0:
                kind = "fresh" if miss(sym) else "miss"
                st[kind, jf] += 1
            else:
                kind = "level"
                r = rows[jf]
                pv = r + [ROOT]
                send(sym, [a & 1 for a in reversed(r)])
                st["level", jf, lf] += 1
                if _word(t, r[lf] + 1) >= _word(t, r[lf]) + 1024:
                    st["false", jf, lf] += 1
                swaps = []
                if handoff:
                    for a in r[:lf]:
                        t.w[a] += 1
                    if push():
                        st["fill64",] += 1
                    walk(t, r[lf], pv, swaps)
                else:
                    push()
                    k = lanes_update(t, pv)
                    if k is not None:
                        walk(t, pv[k], pv, swaps)
                after_swaps(swaps)
            if jmax < BATCH:
                st["short", kind] += 1
            check(p0 + i)
            i += 1
    return codes, t, st


# ---- inputs for the GPU test (tests/test_gpu_handoff.py), chosen with the model above

def raw_of(symbols):
    """the raw bytes whose diff-model, MNP-5 coded symbols are `symbols`, given that no two
    neighbours in it are equal (no runs: one symbol per byte, and the kernel codes the 256
    symbols of each 256-byte chunk in a pass of their own)"""
    import numpy as np
    return (np.cumsum(np.asarray(symbols, dtype=np.int64)) & 255).astype(np.uint8).tobytes()


def candidates(length=3072):
    """(name, symbols) of fixed-seed streams without runs, all well inside the path cache's vote
    (the 16 most frequent symbols cover > 60 %). "geo": a geometric alphabet. "chain": one heavy
    symbol before every draw (or every few) from a geometric chain of ten to fourteen symbols --
    the heavy leaf stays within the step's count of the chain's top, so the chain symbol's deep
    level there reports, mostly falsely. "pad": the same behind one to five padding symbols, which
    moves that report from step symbol 1 to symbols 2..6."""
    import numpy as np
    for seed in range(24):
        rng = np.random.default_rng(seed)
        na = int(rng.choice([6, 10, 14, 20, 32, 64, 128]))
        p = float(rng.choice([0.5, 0.6, 0.7, 0.8, 0.9])) ** np.arange(na)
        p /= p.sum()
        vals = rng.permutation(256)[:na]
        c = vals[rng.choice(na, length, p=p)]
        for i in range(1, length):
            while c[i] == c[i - 1]:
                c[i] = vals[rng.choice(na, p=p)]
        yield f"geo{seed}", c.tolist()
    for seed in range(24):
        rng = np.random.default_rng(2000 + seed)
        na = int(rng.choice([10, 12, 14]))
        p = float(rng.choice([0.4, 0.45, 0.5, 0.55, 0.6])) ** np.arange(na)
        p /= p.sum()
        k = int(rng.choice([1, 2, 3, 4, 6]))
        vals = rng.permutation(256)[:na + 1]
        out = []
        while len(out) < length:
            out.append(vals[na])
            out += list(vals[rng.choice(na, k, p=p)])
        c = np.array(out[:length])
        for i in range(1, length):
            while c[i] == c[i - 1]:
                c[i] = vals[rng.integers(0, na)]
        yield f"chain{seed}", c.tolist()
    for seed in range(15):
        # "pad": nf padding symbols, the heavy one, a chain symbol per period, so that the chain
        # symbol is number nf + 1 of the step that follows the one it ended; a preamble sets the
        # padding symbols' weights 40 apart (a separator wherever one would follow itself), so
        # they tie neither with one another nor, for long, with the rest
        rng = np.random.default_rng(4000 + seed)
        nf, na = 1 + seed % 5, 10
        p = float(rng.choice([0.45, 0.5, 0.55])) ** np.arange(na)
        p /= p.sum()
        vals = rng.permutation(256)
        chain, heavy, sep, pad = vals[:na], vals[na], vals[na + 1], list(vals[na + 2:na + 2 + nf])
        out = []
        for rnd in range(40 * nf):
            for i in range(nf):
                if rnd < 40 * (i + 1):
                    if out and out[-1] == pad[i]:
                        out.append(sep)
                    out.append(pad[i])
        while len(out) < 2 * length:
            if out[-1] == pad[0]:
                out.append(sep)
            out += pad + [heavy, chain[rng.choice(na, p=p)]]
        yield f"pad{seed}", [int(x) for x in out[:2 * length]]


def is_state(k):
    return k[0] in ("miss", "fresh", "level", "false", "fill64", "short")


def search():
    """-> (chosen, states): the candidates that add a state no earlier one reached, as (name,
    symbols), and the Counter of every state the chosen streams end a step in"""
    chosen, states = [], Counter()
    for name, syms in candidates():
        st = encode(syms, lockstep=False)[2]
        if any(is_state(k) and k not in states for k in st):
            chosen.append((name, syms))
            states.update({k: v for k, v in st.items() if is_state(k)})
    return chosen, states
