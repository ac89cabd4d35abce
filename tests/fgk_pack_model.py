"""Model of the FGK batch steps' second-generation lane layouts (hc_fgk.hip), on the slot-form
tree of fgk_cache_model.py and with the tentative leader test of fgk_batch_model.py, whose
7 x 9 layout (seven symbols, nine lanes each) both kernels used before.

decode_packed -- Dec::decode_batch, one lane per code bit: lane o stands for bit o of the 64-bit
window, the d lanes of a d-bit code read its path from depth 1 down to the leaf, lane 63 is the
root. No lane pads a short code, so a step takes up to PACK_MAX codes: as many as end within the
window's valid bits (and within bit 62), the block of 256 symbols, and the first code that fails
the tentative test or is no leaf of the level tables (longer than 8 bits, or the NYT's), which
is decoded alone. The window: 64 bits, refilled by 32 whenever at most 32 are valid.

encode_hyst -- the encoder's code_all_batch with two layouts chosen by hysteresis, no depth
lookup: deep = 7 symbols x 9 lanes as before; shallow = 9 symbols x 7 lanes (levels 0..6, a
symbol fits when its level-6 lane holds the root: a cached path of at most 6 positions). In
shallow mode a cached symbol deeper than that ends the step like a failure but is not coded
alone: the mode becomes deep and the next step takes it. After a deep step that took all seven
symbols, every one of them fit for the shallow layout, the mode becomes shallow.
"""
from fgk_batch_model import batch_len, tentative_len
from fgk_cache_model import ROOT, PathCache, Tree

PACK_MAX = 16     # decoder: codes per step
TABLE_DEPTH = 8   # the level tables reach codes of up to 8 bits
EXIT_BITS = 7     # decoder: a first code of this many bits or more is left to the one-symbol step
BLOCK = 256       # decoder: symbols per block (a step never crosses a block's end)
DEEP = (7, 9)     # encoder layouts: symbols per step, deepest cached path taken
SHALLOW = (9, 6)


def decode_packed(symbols, cap=PACK_MAX, window=True, exit8=True, exit_bits=EXIT_BITS):
    """(tree, stats): decode `symbols` (the model knows them; the kernel reads them from the
    tables) with packed steps of up to `cap` codes. window=False: no bit window (every code fits).
    stats: steps, alone (symbols decoded by the one-symbol step), sent (first codes of >= exit_bits
    bits sent to the one-symbol step before the chain: the kernel's HC_DEC_EXIT_BITS; exit8=False:
    none), capped (steps that ended at `cap`). The gate only chooses which path decodes a symbol:
    the tree is the same for every setting."""
    t = Tree()
    st = {"steps": 0, "alone": 0, "sent": 0, "capped": 0}
    nwin = 24  # after the header: the flags byte taken from the first payload word

    def refill(need=33):
        nonlocal nwin
        while nwin < need:
            nwin += 32

    def code_bits(sym):
        x = t.where[sym]
        return len(t.path(x)) if x else len(t.path(t.nyt)) + 8

    def alone(sym):
        nonlocal nwin
        refill()
        d = code_bits(sym)
        refill(d)  # (a code longer than the window refills on its way down)
        nwin -= d
        if t.where[sym] == 0:
            t.split(sym)
        t.update(t.where[sym])

    i, n = 0, len(symbols)
    while i < n:
        refill()
        if exit8 and code_bits(symbols[i]) >= exit_bits:
            st["sent"] += 1
            alone(symbols[i])
            i += 1
            continue
        i1 = min(n, i - i % BLOCK + BLOCK)
        lim = min(nwin, 63) if window else 1 << 30
        paths, s = [], 0
        for sym in symbols[i:min(i1, i + cap)]:
            x = t.where[sym]
            p = t.path(x) if x else None
            if p is None or len(p) > TABLE_DEPTH:
                # no leaf in the tables: the entry stops at depth <= 8 and fails the leaf test,
                # if it lies inside the window
                if s + min(code_bits(sym), TABLE_DEPTH) <= lim:
                    paths.append(None)
                break
            if s + len(p) > lim:
                break
            s += len(p)
            paths.append(p + [ROOT])
        jf = tentative_len(t, paths)
        assert jf <= batch_len(t, paths)  # never passes what the exact test fails
        st["steps"] += 1
        st["capped"] += jf == cap
        for p in paths[:jf]:
            nwin -= len(p) - 1
            for a in p:
                t.w[a] += 1
        i += jf
        if jf < len(paths):
            st["alone"] += 1
            alone(symbols[i])
            i += 1
    return t, st


def encode_hyst(symbols, layout=0):
    """(codes, tree, stats): the encoder's batch steps with the layout chosen by hysteresis
    (layout 0), the deep layout only (1), or shallow from the start and again after every deep
    step (2: the kernel's test hook). stats: steps, alone, shallow (steps in the shallow layout),
    empty (shallow steps that took nothing: their first symbol was too deep), switches."""
    t = Tree()
    pc = PathCache()
    codes = []
    st = {"steps": 0, "alone": 0, "shallow": 0, "empty": 0, "switches": 0}
    shallow = layout == 2

    def alone(sym):
        fresh = t.where[sym] == 0
        if fresh:
            t.split(sym)
        x = t.where[sym]
        pv = pc.lookup(sym)
        if pv is None:
            pv = t.path(x)
            pc.insert(sym, pv)
        code = [p & 1 for p in reversed(pv)]
        codes.append(code[:-1] + [(sym >> k) & 1 for k in range(7, -1, -1)] if fresh else code)
        t.update(x)
        for s, lead in t.swaps:
            pc.on_swap(s, lead)

    def cached(sym):
        e = pc.slot.get(sym)
        return None if t.where[sym] == 0 or e is None else pc.ent[e][1]

    i, n = 0, len(symbols)
    while i < n:
        cap, depth = SHALLOW if shallow else DEEP
        paths, too_deep = [], False
        for sym in symbols[i:i + cap]:
            p = cached(sym)
            if p is not None and len(p) > depth:
                too_deep = True  # (in the deep layout it is coded alone, as a miss is)
                p = None
            paths.append(None if p is None else p + [ROOT])
            if p is None:
                break
        jf = tentative_len(t, paths)
        assert jf <= batch_len(t, paths)
        st["steps"] += 1
        st["shallow"] += shallow
        for p in paths[:jf]:
            codes.append([a & 1 for a in reversed(p[:-1])])
            for a in p:
                t.w[a] += 1
        i += jf
        if shallow and too_deep and jf == len(paths) - 1:
            # the step ended at the symbol too deep for seven lanes: deep mode takes it next
            st["empty"] += jf == 0
            st["switches"] += 1
            shallow = False
            continue
        if not shallow and layout != 1:
            if layout == 2 or (jf == cap and all(len(p) - 1 <= SHALLOW[1] for p in paths)):
                st["switches"] += 1
                shallow = True
        if jf < len(paths):
            st["alone"] += 1
            alone(symbols[i])
            i += 1
    return codes, t, st
