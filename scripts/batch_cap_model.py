"""How often the FGK batches stop at their lane cap, and what a second lane layout would buy
(DESIGN.md §8 item 1), on the slot-form model (tests/fgk_batch_model.py, fgk_cache_model.py).

Both kernels batch seven symbols per step, nine lanes each (lane 9 j + l: level l of symbol j's
path; levels 0..8). A step ends at the first symbol that fails the tentative leader test, has no
cached path (encoder) / no leaf in the level tables (decoder), or at the cap. The alternative
counted here: ten symbols of six lanes (depth <= 5) whenever the step's next ten symbols all fit
that depth, else the present layout.

    python scripts/batch_cap_model.py [--stream 0] [--symbols 60000]

--policy pack / hyst: the two layouts the kernels can realise without an oracle
(tests/fgk_pack_model.py) on streams 0..3 -- the decoder packed by bit offset (one lane per code
bit, up to 16 or 12 codes per step, the 64-bit window refilled by 32 at <= 32 valid bits), the
encoder's 9 x 7 / 7 x 9 layouts chosen by hysteresis -- against the 7 x 9 steps: steps, symbols per
step, symbols coded alone.

    python scripts/batch_cap_model.py --policy pack
    python scripts/batch_cap_model.py --policy hyst

--policy encpack: the encoder's step packed by path depth (tests/fgk_encpack_model.py: up to 16 or
12 cached symbols a step, one lane per path position while the depths sum to at most 63) against
the 7 x 9 steps on streams 0..3.

    python scripts/batch_cap_model.py --policy encpack
"""
import argparse
import os
import sys

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT_DIR, "oracle"))
sys.path.insert(0, os.path.join(ROOT_DIR, "tests"))

import numpy as np  # noqa: E402
import oracle  # noqa: E402
import fgk_batch_model as M  # noqa: E402
from fgk_cache_model import ROOT, PathCache, Tree  # noqa: E402


def run(symbols, encoder, layout):
    """layout(path_of, symbols, i) -> (cap, deepest path length); path_of(sym, depth) is the
    symbol's batch path (ROOT last) or None"""
    t, pc = Tree(), PathCache()
    st = {"steps": 0, "alone": 0, "full": 0}

    def alone(sym):
        if t.where[sym] == 0:
            t.split(sym)
        x = t.where[sym]
        if encoder and pc.lookup(sym) is None:
            pc.insert(sym, t.path(x))
        t.update(x)
        for s, lead in t.swaps:
            pc.on_swap(s, lead)

    def path_of(sym, depth):
        if t.where[sym] == 0:
            return None
        if encoder:
            e = pc.slot.get(sym)
            p = pc.ent[e][1] if e is not None else None
        else:
            p = t.path(t.where[sym])
        return p + [ROOT] if p is not None and len(p) <= depth else None

    i, n = 0, len(symbols)
    while i < n:
        cap, depth = layout(path_of, symbols, i)
        paths = []
        for s in symbols[i:i + cap]:
            paths.append(path_of(s, depth))
            if paths[-1] is None:
                break
        jf = M.tentative_len(t, paths)
        st["steps"] += 1
        st["full"] += jf == cap
        for p in paths[:jf]:
            for a in p:
                t.w[a] += 1
        i += jf
        if jf < len(paths) and i < n:
            st["alone"] += 1
            alone(symbols[i])
            i += 1
    return st


def realisable(policy, n_sym):
    import fgk_pack_model as P

    def line(name, n, steps, alone, base=None):
        rel = f" ({(steps / base - 1) * 100:+.1f} %)" if base else ""
        print(f"  {name}: {steps} steps{rel}, {n / steps:.2f} symbols a step, {alone} alone")

    for k in range(4):
        syms = np.frombuffer(oracle.rle(oracle.diff(oracle.synth("photo", k))), np.uint8)[:n_sym].tolist()
        n = len(syms)
        print(f"photo -c -m stream {k}, first {n} symbols")
        if policy == "pack":
            t0, s0 = P.decode_packed(syms, cap=7, window=False, exit8=False)
            line("decoder 7 x 9", n, s0["steps"], s0["alone"])
            for cap in (16, 12):
                t1, s1 = P.decode_packed(syms, cap=cap, exit8=False)
                assert t1.w == t0.w and t1.body == t0.body
                line(f"decoder packed, <= {cap} codes", n, s1["steps"], s1["alone"], s0["steps"])
            t1, s1 = P.decode_packed(syms, cap=16, window=False, exit8=False)
            line("decoder packed, <= 16 codes, no window limit", n, s1["steps"], s1["alone"], s0["steps"])
        elif policy == "encpack":
            import fgk_encpack_model as E
            c0, t0, s0 = P.encode_hyst(syms, 1)
            line("encoder 7 x 9", n, s0["steps"], s0["alone"])
            for cap in (16, 12):
                c1, t1, s1 = E.encode_packed(syms, cap=cap)
                assert c1 == c0 and t1.w == t0.w
                line(f"encoder packed by depth, <= {cap} symbols", n, s1["steps",], s1["alone",], s0["steps"])
                print(f"    {s1['empty',]} steps that took nothing (their first symbol had no row), "
                      f"{s1['full',]} at the cap, {s1['end63',]} with all 63 lanes")
        else:
            c0, t0, s0 = P.encode_hyst(syms, 1)
            line("encoder 7 x 9", n, s0["steps"], s0["alone"])
            c1, t1, s1 = P.encode_hyst(syms, 0)
            assert c1 == c0 and t1.w == t0.w
            line("encoder 9 x 7 / 7 x 9 by hysteresis", n, s1["steps"], s1["alone"], s0["steps"])
            print(f"    {s1['shallow']} shallow steps, {s1['switches']} switches, {s1['empty']} steps that took nothing")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream", type=int, default=0)
    ap.add_argument("--symbols", type=int, default=60000)
    ap.add_argument("--policy", choices=("oracle", "pack", "hyst", "encpack"), default="oracle")
    a = ap.parse_args()
    if a.policy != "oracle":
        return realisable(a.policy, a.symbols)
    syms = np.frombuffer(oracle.rle(oracle.diff(oracle.synth("photo", a.stream))), np.uint8)[: a.symbols].tolist()
    for name, enc in (("encoder (path cache)", True), ("decoder (level tables)", False)):
        # the deepest batch path: the encoder's cached rows (insert depth 9), the decoder's tables
        # (codes of up to 8 bits)
        deep = 9 if enc else 8
        now = lambda path_of, s, i, deep=deep: (7, deep)  # noqa: E731

        def hybrid(path_of, s, i, deep=deep):
            return (10, 5) if all(path_of(x, 5) is not None for x in s[i:i + 10]) else (7, deep)

        a0, a1 = run(syms, enc, now), run(syms, enc, hybrid)
        print(f"{name}: 7 x 9 lanes: {a0['steps']} steps, {a0['full'] / a0['steps'] * 100:.0f} % full, "
              f"{len(syms) / a0['steps']:.2f} symbols a step, {a0['alone']} alone; "
              f"+ 10 x 6 when the next ten fit: {a1['steps']} steps ({(a1['steps'] / a0['steps'] - 1) * 100:+.1f} %), "
              f"{len(syms) / a1['steps']:.2f} a step, {a1['alone']} alone")


if __name__ == "__main__":
    main()
