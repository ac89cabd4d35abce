"""Model of the encoder's miss run (hc_fgk.hip code_all_batch, HC_ENC_MISS_RUN), on the packed batch
step of tests/fgk_encpack_model.py.

A regular step reads the bytes and where[] words of up to 16 symbols and forms mm, the mask of those
without a cache row (within the step's cap and the pass). When a symbol ends the step and is coded
alone, the symbols right behind it whose mm bits are set -- up to run_cap of them -- are coded alone
as well, one after the other, each looked up afresh (so one that became cached meanwhile, by
equalling a symbol just inserted, is coded from its row), instead of starting a step that would take
nothing. Only the count crosses the miss path. run_cap 0 is the encoder without the rule
(fgk_encpack_model.encode_packed: same steps, same symbols alone).

encode_missrun() follows the record lanes and the coding passes as encode_packed does; with
lockstep=True it runs beside the plain Tree.update and asserts at every symbol that the code about
to be sent and the whole tree are the one-symbol loop's.
"""
import functools
from collections import Counter

from fgk_cache_model import ROOT, PathCache, Tree, _word, lanes_update
from fgk_handoff_model import INSERT_DEPTH, _records, same_tree, walk

PACK = 16    # HC_ENC_PACK
LANES = 63
RUN_MAX = 15  # HC_ENC_MISS_RUN_MAX as shipped


def encode_missrun(symbols, run_cap=RUN_MAX, cap=PACK, chunk=256, lockstep=False):
    """(codes, tree, states). states: ("steps",), ("empty",) (steps whose first symbol had no row),
    ("alone",) (symbols coded alone, the runs' among them), ("direct",) (symbols coded in a run),
    ("taken",);
      ("run", n, taken): a run of n symbols behind a step that took `taken` symbols;
      ("run_last",): a run that reached the step's last read lane (symbol 15 of the step);
      ("run_pass",): a run cut by the end of the pass (the symbol behind it, in the next pass,
        has no row either);
      ("run_fresh",): a run symbol not seen before (a split);
      ("run_repeat", d): a run symbol cached by the time it is coded, equal to the symbol d before;
      ("run_fill",): the record lanes filled (sink.n == 64: pack) while a run symbol was coded;
      ("run_level",): the run followed a cached symbol with a reported level."""
    t, ref = Tree(), Tree()
    pc = PathCache()
    codes = []
    st = Counter()
    n = 0  # records pending (sink.n)
    filled = False

    def push(k=1):
        nonlocal n, filled
        for _ in range(k):
            n += 1
            if n == 64:
                n = 0
                filled = True

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

    def row_of(sym):
        e = pc.slot.get(sym) if t.where[sym] else None
        return None if e is None else pc.ent[e][1]

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

    def cached(sym, r):
        """a cached symbol coded alone: its row's code, every level tested again"""
        pv = r + [ROOT]
        send(sym, [a & 1 for a in reversed(r)])
        push()
        swaps = []
        k = lanes_update(t, pv)
        if k is not None:
            walk(t, pv[k], pv, swaps)
        for s, lead in swaps:
            pc.on_swap(s, lead)

    for p0 in range(0, len(symbols), chunk):
        syms = symbols[p0:p0 + chunk]
        ns, i = len(syms), 0
        while i < ns:
            if n > 64 - PACK:
                n = 0  # pack
            st["steps",] += 1
            lim = min(cap, ns - i)
            # mm: what the step's 16 lanes read, before anything of the step changes the cache
            mm = [row_of(s_) is None for s_ in syms[i:i + lim]]
            rows, lanes = [], 0
            for s_ in syms[i:i + lim]:
                r = row_of(s_)
                if r is None or lanes + len(r) > LANES:
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
            st["empty",] += jmax == 0
            for j in range(jf):
                send(syms[i + j], [a & 1 for a in reversed(rows[j])])
                for a in rows[j]:
                    t.w[a] += 1
                t.w[ROOT] += 1
                check(p0 + i + j)
            st["taken",] += jf
            n += jf
            i0, i = i, i + jf
            if lf is None and not (jf < lim and mm[jf]):
                continue  # the cap, the lanes or the pass ended the step
            st["alone",] += 1
            if lf is None:
                miss(syms[i])
            else:
                cached(syms[i], rows[jf])
            check(p0 + i)
            i += 1
            # the run: the set bits of mm above jf, at most run_cap
            run = 0
            while run < run_cap and jf + 1 + run < lim and mm[jf + 1 + run]:
                run += 1
            if not run:
                continue
            st["run", run, jf] += 1
            st["run_level",] += lf is not None
            st["run_last",] += jf + run == PACK - 1
            nxt = p0 + i + run
            if jf + 1 + run == lim and lim < cap and run < run_cap and nxt < len(symbols):
                s_ = symbols[nxt]
                st["run_pass",] += (pc.slot.get(s_) if t.where[s_] else None) is None
            for q in range(run):
                sym = syms[i]
                st["alone",] += 1
                st["direct",] += 1
                filled = False
                r = row_of(sym)
                if r is None:
                    st["run_fresh",] += miss(sym)
                else:
                    back = [d for d in range(1, q + 2) if syms[i - d] == sym]
                    assert back, "a run symbol is cached only by equalling one coded alone before it"
                    st["run_repeat", back[0]] += 1
                    cached(sym, r)
                st["run_fill",] += filled
                check(p0 + i)
                i += 1
    return codes, t, st


# ---- inputs for the GPU test (tests/test_gpu_missrun.py), chosen with the model above

def candidates(length=1536):
    """(name, symbols) of fixed-seed streams of at most 4096 symbols. A few common symbols (cached
    rows, steps that take many) and, planted behind steps of chosen lengths, runs of rare or unseen
    symbols: runs of 2, 3 and 15, runs to the step's last lane and over a pass's end, repeats
    (A A: a two-byte run, which MNP-5 codes as two symbols; A B A)."""
    import numpy as np
    for seed in range(6):
        rng = np.random.default_rng(9100 + seed)
        vals = [int(v) for v in rng.permutation(256)]
        common, rare = vals[:6], vals[6:]
        p = np.array([0.4, 0.25, 0.15, 0.1, 0.06, 0.04])
        out = []

        def fill(k):
            while k > 0:
                c = common[int(rng.choice(6, p=p))]
                if not out or out[-1] != c:
                    out.append(c)
                    k -= 1

        fill(length // 4)
        ri = 0
        while len(out) < length and ri + 40 < len(rare):
            kind = int(rng.integers(0, 6))
            fill(int(rng.choice([0, 1, 1, 15, 15, 3, 7, 30])))
            if kind == 0:    # a run of 2..4 distinct rare symbols, some not seen before
                k = int(rng.integers(2, 5))
                out += rare[ri:ri + k]
                ri += k - 1
            elif kind == 1:  # sixteen in a row: a run of 15 behind the first
                out += rare[ri:ri + 16]
                ri += 5
            elif kind == 2:  # A A (a two-byte run) and A B A
                a, b = rare[ri], rare[ri + 1]
                out += [a, a, b] if seed & 1 else [a, b, a]
                ri += 1
            elif kind == 3:  # rare symbols seen before: misses without splits
                k = int(rng.integers(2, 5))
                out += [rare[j] for j in rng.choice(max(ri, 4), k, replace=False)]
            elif kind == 4:  # up to the pass's end and over it
                pad = (-len(out) - 2) % 256
                if pad < 60:
                    fill(pad)
                    out += rare[ri:ri + 5]
                    ri += 2
            else:            # many records pending: long codes of rare symbols seen before
                out += [rare[j] for j in rng.choice(max(ri, 8), 8, replace=False)]
        # no run of three or more equal symbols, no A A A (MNP-5 would add a count)
        for k in range(2, len(out)):
            if out[k] == out[k - 1] == out[k - 2]:
                out[k] = common[0] if out[k] != common[0] else common[1]
        yield "plant%d" % seed, out[:4096]


def is_state(k):
    return k[0].startswith("run")


@functools.lru_cache(maxsize=None)
def search(caps=(1, 7, 16)):
    """-> (chosen, states): the candidates that add a run state no earlier one reached under some
    step cap of `caps` (hc_debug_set_enc_pack), as (name, symbols), and per cap the Counter of the
    run states the chosen streams reach"""
    chosen, states = [], {c: Counter() for c in caps}
    for name, syms in candidates():
        add = False
        new = {}
        for c in caps:
            st = encode_missrun(syms, cap=c)[2]
            new[c] = {k: v for k, v in st.items() if is_state(k) and v}
            add = add or any(k not in states[c] for k in new[c])
        if add:
            chosen.append((name, syms))
            for c in caps:
                states[c].update(new[c])
    return chosen, states
