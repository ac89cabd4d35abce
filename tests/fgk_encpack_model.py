"""Model of the encoder's batch step packed by path depth (hc_fgk.hip code_all_batch, HC_ENC_PACK),
on the slot-form tree and path cache of tests/fgk_cache_model.py (paths of up to INSERT_DEPTH
positions are cached) and with the tentative test of tests/fgk_batch_model.py.

A step takes symbols t, t + 1, ... of the pass while fewer than `cap` are taken, each has a cached
row, and the depths of the ones taken sum to at most 63: symbol j's d_j path positions (levels
0 .. d_j - 1) take lanes S_j .. S_j + d_j - 1, S_j the depths before it, and lane 63 is the root.
No lane pads a short path. The depth comes from the row's code record (1 << depth | code bits),
which is also what the record lanes take. The first symbol without a cached row (a miss, or a
symbol not seen yet: a split) ends the step without occupying lanes -- the symbols behind it are
never added, where the 7 x 9 step added them and took them back -- and is coded alone. So is the
first symbol with a reported level: every path position of the symbols taken gets its increment
first, so symbol j's test at position a sees all of them through a and none through a + 1
(tentative_len); its increments and those of the symbols behind it are taken back and all its
levels are tested again (the report may be false). The symbols before it commit.

encode_packed() follows the record lanes (RecSink::n: a step starts with at most 48 records
pending, since it may add 16) and the coding passes (`chunk` symbols each: the kernel codes the
symbols of one 256-byte chunk per pass when the stream has no runs), and counts the states steps
end in. With lockstep=True it runs beside the plain Tree.update and asserts at every symbol that
the code about to be sent and the whole tree are the one-symbol loop's.
"""
import functools
from collections import Counter

from fgk_batch_model import batch_len
from fgk_cache_model import ROOT, PathCache, Tree, _word, lanes_update
from fgk_handoff_model import INSERT_DEPTH, _records, same_tree, walk

PACK = 16    # HC_ENC_PACK: symbols per step (and the record lanes a step needs free)
LANES = 63   # path lanes of a step (lane 63: the root)
CROSS = ((62, 2), (63, 1), (55, 9))  # (lanes taken, depth of the next symbol) the search looks for


def encode_packed(symbols, cap=PACK, chunk=256, lockstep=False):
    """(codes, tree, states): every symbol's code bits, the final tree, and a Counter of
      ("steps",), ("alone",), ("taken",) (symbols committed by steps), ("empty",) (steps whose first
      symbol had no row);
      ("full",): a step took `cap` symbols; ("end63",): its lanes ended at exactly 63;
      ("cross", s, d): the next symbol, d deep, would have crossed lane 63 behind s lanes taken;
      ("deep_first",) / ("deep_last",): a symbol INSERT_DEPTH deep first / last among those taken;
      ("miss", j) / ("fresh", j): step symbol j uncached with / without a leaf (a split);
      ("level", j, l): cached symbol j, level l reported; ("false", j, l): ... falsely;
      ("fill64",): the record of the symbol coded alone went to lane 63 (pack follows);
      ("short", kind): the step was the last of a pass with fewer than PACK symbols left and
      ended at a symbol coded alone (kind "miss" / "fresh" / "level")."""
    t, ref = Tree(), Tree()
    pc = PathCache()
    codes = []
    st = Counter()
    n = 0  # records pending (sink.n)

    def push(k=1):
        nonlocal n
        for _ in range(k):
            n += 1
            if n == 64:
                n = 0

    def send(sym, code):
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
        for s, lead in swaps:
            pc.on_swap(s, lead)
        push(_records(d - 1) + 1 if fresh else _records(d))
        return fresh

    for p0 in range(0, len(symbols), chunk):
        syms = symbols[p0:p0 + chunk]
        ns, i = len(syms), 0
        while i < ns:
            if n > 64 - PACK:
                n = 0  # pack
            st["steps",] += 1
            lim = min(cap, ns - i)
            rows, lanes, uncached = [], 0, False
            for s_ in syms[i:i + lim]:
                e = pc.slot.get(s_) if t.where[s_] else None
                if e is None:
                    uncached = True
                    break
                r = pc.ent[e][1]
                if lanes + len(r) > LANES:
                    if (lanes, len(r)) in CROSS:
                        st["cross", lanes, len(r)] += 1
                    break
                lanes += len(r)
                rows.append(r)
            jmax = len(rows)
            cnt = Counter(a for r in rows for a in r)
            jf, lf = jmax, None
            for j, r in enumerate(rows):
                for l, a in enumerate(r):
                    if _word(t, a + 1) < _word(t, a) + 1024 * cnt[a]:
                        jf, lf = j, l
                        break
                if lf is not None:
                    break
            assert jf <= batch_len(t, [r + [ROOT] for r in rows])  # never passes what the exact test fails
            if jmax:
                st["full",] += jf == cap
                st["end63",] += lanes == LANES
                st["deep_first",] += len(rows[0]) == INSERT_DEPTH
                st["deep_last",] += len(rows[-1]) == INSERT_DEPTH
            else:
                st["empty",] += 1
            for j in range(jf):  # the symbols before jf commit
                send(syms[i + j], [a & 1 for a in reversed(rows[j])])
                for a in rows[j]:
                    t.w[a] += 1
                t.w[ROOT] += 1
                check(p0 + i + j)
            st["taken",] += jf
            n += jf
            i += jf
            if lf is None and not uncached:
                continue  # the cap, the lanes or the pass ended the step
            st["alone",] += 1
            sym = syms[i]
            if n == 63:
                st["fill64",] += 1
            if lf is None:
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
                push()
                swaps = []
                k = lanes_update(t, pv)
                if k is not None:
                    walk(t, pv[k], pv, swaps)
                for s, lead in swaps:
                    pc.on_swap(s, lead)
            if ns - (i - jf) < PACK:
                st["short", kind] += 1
            check(p0 + i)
            i += 1
    return codes, t, st


# ---- inputs for the GPU test (tests/test_gpu_encpack.py), chosen with the model above

def candidates(length=3072):
    """(name, symbols) of fixed-seed streams without runs (fgk_handoff_model.raw_of gives their raw
    bytes), all well inside the path cache's vote. First the families of
    fgk_handoff_model.candidates(), whose steps already end in every state but the crossings.
    "cross": a geometric chain of nine symbols c0..c8 (ratio 0.42 to 0.48, so no leaf ties with the
    rest of the chain below it: depths 1, 2, ..., 9, the NYT's subtree beside c8), long enough that
    the deep leaves' weights stand a few counts apart; then, each behind a symbol not seen before
    (a split: the next step starts at the pattern), runs of deep symbols whose depths sum to 63, 62
    and 55 before a symbol one, two and nine deep."""
    import numpy as np
    from fgk_handoff_model import candidates as handoff_candidates
    yield from handoff_candidates(length)

    for seed in range(3):
        rng = np.random.default_rng(6000 + seed)
        na = 9
        p = float(rng.choice([0.42, 0.45, 0.48])) ** np.arange(na)
        p /= p.sum()
        vals = rng.permutation(256)
        ch, spare = vals[:na], list(vals[na:])
        c = ch[rng.choice(na, 4 * length, p=p)]
        for i in range(1, len(c)):
            while c[i] == c[i - 1]:
                c[i] = ch[rng.choice(na, p=p)]
        out = c.tolist()
        deep = [8, 7, 8, 7, 8, 7]  # 51 lanes
        for rep in range(3):
            for pat in (deep + [8, 2, 0], deep + [6, 3, 1], deep + [3, 8]):
                out += [spare.pop()] + [ch[k] for k in pat] + ch[rng.choice(4, 20, p=p[:4] / p[:4].sum())].tolist()
        for i in range(1, len(out)):
            if out[i] == out[i - 1]:
                out[i] = ch[1] if out[i] == ch[0] else ch[0]
        yield f"cross{seed}", [int(x) for x in out]


def is_state(k):
    return k[0] in ("full", "end63", "cross", "deep_first", "deep_last", "miss", "fresh", "level", "false", "fill64", "short")


@functools.lru_cache(maxsize=None)
def search():
    """(run once per process: the model test and the GPU test share it) -> (chosen, states): the candidates that add a state no earlier one reached, as (name,
    symbols), and the Counter of every state the chosen streams end a step in"""
    chosen, states = [], Counter()
    for name, syms in candidates():
        st = encode_packed(syms)[2]
        new = {k: v for k, v in st.items() if is_state(k) and v}
        if any(k not in states for k in new):
            chosen.append((name, syms))
            states.update(new)
    return chosen, states
