"""Model of the chain of code starts in the decoder's packed batch step (hc_fgk.hip
Dec::decode_batch, HC_DEC_CHAIN), as a pure function of the step's depth map and window limit.

chain(dep, lim, stride) -- dep[o], o = 0..63: the depth of a code that starts o bits into the
window (the level-8 entry of the eight bits from o on, 1..8); lim: a code is taken if it ends
within bit lim (63 on 64 true window bits, else min(valid bits, 63)). Returns the 64 lanes of sv
(lane j: the bits before code j, 255: no such code) with the links run and the exit tests made.

stride 1 is the chain of single codes as the kernel has had it: S_j+1 = S_j + dep[S_j & 63] (the
lane select wraps past bit 63, S still grows), sixteen links, an exit test before links 5, 9 and
13 (S >= lim). Stride 2 / 4 compose the depth map with itself once / twice,
    dep2[o] = dep[o] + (o + dep[o] < 64 ? dep[o + dep[o]] : 64),
run the same chain over every second / fourth start with the tests at the same starts, and fill
the starts in between lane-parallel: lane j of sv, 0 <= j < 16, takes min(sv[j], p + d[p & 63])
with p = sv[j - sh] (255 for j < sh), sh = 2 with d = dep2, then sh = 1 with d = dep.

What the rest of the step reads (derive): nval = the codes that end within lim, jmax = the codes
taken (the cap and the block's end bind too), se = sv[jmax], sm = the mask of start bits (lane j
marks bit min(sv[j], 63)), and each lane's code start so on the lanes below se. The strides agree
on all of them and on sv wherever it is at most 63; they differ in two ways that nothing reads:
  * a start past bit 63 is S + another offset's depth at stride 1 and at least 64 more than a
    start at stride 2 / 4: every such lane marks bit 63 of sm, which lanes 17..63 (255) mark anyway;
  * after an exit at S_4k >= lim stride 1 leaves lanes 4k + 1.. at 255, the fill gives lanes 4k + 1
    (.. 4k + 3) a start above S_4k >= lim: with lim < 63 that can mark a bit of sm above lim,
    beyond every code taken (se <= lim; the step masks sm with the lanes below se).
same_step asserts exactly this.

decode_chain(bits, n, ...) decodes a stream from its bits the way the kernel does -- the depth map
from the level tables at every bit offset, the chain, the tentative test of fgk_batch_model over
the codes found -- with the window of fgk_topup_model. Run beside fgk_pack_model.decode_packed
and fgk_topup_model.decode_topup on the same streams it leaves their tree and restores every
symbol; its step counts are close to theirs, not equal: those models know the symbols and give a
step the true paths of the ones to come, while the kernel -- and this model -- parse the window
with the tree as it is at the step's start, so the codes after a symbol whose update changes the
tree's shape (the step ends at or before it) are read differently and count differently in the
tentative test; and their gate sends a first code that is the NYT's to the one-symbol step by its
whole length, the kernel's by the table depth.

Instructions, from the ISA of decode_kernel<0, 0, false>: a link is v_readlane_b32, s_add_i32,
v_writelane_b32 (3 VALU + SALU; the first has no add) and two s_nop; an exit test s_cmp + s_cbranch;
a composition v_add, v_lshlrev, ds_bpermute, v_cmp, v_cndmask, v_add (6); a fill v_mov, v_mov_dpp,
v_lshlrev, ds_bpermute, v_add, v_min (6).
"""
import numpy as np

from fgk_batch_model import encode, tentative_len
from fgk_cache_model import INNER, NYT, ROOT, LevelTables, Tree
from fgk_pack_model import BLOCK, EXIT_BITS, PACK_MAX
from fgk_topup_model import Window

STRIDES = (1, 2, 4)
_IDLE = [255] * 47
LINK, LINK_NOPS, TEST, COMPOSE, FILL = 3, 2, 2, 6, 6


def compose(d):
    return [d[o] + (d[(o + d[o]) & 63] if o + d[o] < 64 else 64) for o in range(64)]


def chain(dep, lim, stride=1, pack=PACK_MAX):
    """(sv, links, tests)"""
    sv = [0] + [255] * 63
    links, tests = 1, 0
    if stride == 1:
        s = dep[0]
        sv[1] = s
        for j in range(1, pack):
            if j % 4 == 0:
                tests += 1
                if s >= lim:
                    break
            s += dep[s & 63]
            sv[j + 1] = s
            links += 1
        return sv, links, tests
    d2 = compose(dep)
    dc = compose(d2) if stride == 4 else d2
    e = dc[0]
    sv[stride] = e
    for j in range(2, pack // stride + 1):
        if (j - 1) * stride % 4 == 0:
            tests += 1
            if e >= lim:
                break
        e += dc[e & 63]
        sv[j * stride] = e
        links += 1

    def fill(sv, sh, d):  # the DPP row shift reaches lanes 0..15 only, lanes without a source read 255
        pr = [sv[l - sh] if sh <= l < 16 else 255 for l in range(64)]
        return [min(sv[l], pr[l] + d[pr[l] & 63]) for l in range(64)]

    if stride == 4:
        sv = fill(sv, 2, d2)
    return fill(sv, 1, dep), links, tests


def instructions(stride, links, tests):
    """(VALU + SALU + LDS instructions, s_nop) of the chain by the count above"""
    levels = {1: 0, 2: 1, 4: 2}[stride]
    return LINK * links - 1 + TEST * tests + (COMPOSE + FILL) * levels, LINK_NOPS * links


def derive(sv, lim, cap=PACK_MAX, left=1 << 30):
    """(nval, jmax, se, sm, so): what the step reads of the chain; so on the lanes below se"""
    assert sv[17:] == _IDLE  # lanes 17..63 hold no start: above every lim, and they mark bit 63
    nval = sum(v <= lim for v in sv[:17]) - 1
    jmax = min(nval, cap, left)
    se = sv[jmax]
    sm = 1 << 63
    for v in sv[:17]:
        sm |= 1 << min(v, 63)
    so, j = [], 0
    for o in range(se):  # lane o: the starts in bits 1..o
        j += o > 0 and sm >> o & 1
        so.append(sv[j])
    return nval, jmax, se, sm, so


def same_step(dep, lim, cap=PACK_MAX, left=1 << 30, strides=(2, 4)):
    """assert that the strided chains give the step what stride 1 gives it; returns stride 1's
    (sv, nval, jmax, se)"""
    sv1, l1, _ = chain(dep, lim, 1)
    n1, j1, se1, sm1, so1 = derive(sv1, lim, cap, left)
    assert se1 <= lim and l1 in (4, 8, 12, 16)
    for st in strides:
        sv, links, _ = chain(dep, lim, st)
        assert links * st == l1, (st, dep, lim)
        n, j, se, sm, so = derive(sv, lim, cap, left)
        assert (n, j, se, so) == (n1, j1, se1, so1), (st, dep, lim)
        for a, b in zip(sv1[:17], sv[:17]):
            assert a == b if a <= lim else b > lim, (st, dep, lim, sv1[:17], sv[:17])
            assert a == b or a > 63 or (a == 255 and b > lim), (st, dep, lim, sv1[:17], sv[:17])
        below = (1 << (lim + 1)) - 1
        assert sm & below == sm1 & below and sm >> 63 == sm1 >> 63 == 1, (st, dep, lim)
        assert lim < 63 or sm == sm1, (st, dep, lim)
    return sv1, n1, j1, se1


EDGES = ("start_62", "start_63", "start_64", "start_past_64", "jump_past_63", "odd_last", "one_bit_16",
         "six_bit_cross", "nonleaf_mid", "stale_entry", "block_end", "peeked_used", "exit_4", "exit_8", "exit_12")


def stream_bits(symbols):
    """the one-symbol encoder's bits of `symbols`"""
    codes, _, _ = encode(list(symbols), batched=False)
    return [b for c in codes for b in c]


def decode_chain(bits, n, stride=1, cap=PACK_MAX, topup=True, on_step=None):
    """(symbols, stats, edges, tree): decode n symbols from `bits` with packed steps whose chain runs at
    `stride`. The level tables are the kernel's (fgk_cache_model.LevelTables: rebuilt when a swap moves
    a position some walk passes through; an entry may stop at a position that has become inner).
    stats: steps, alone, sent, capped as fgk_topup_model's, nyt_first (steps whose first code was
    the NYT's below the gate), links[k] (steps that ran k links), instr / nops (the chain's);
    edges: steps per name in EDGES. on_step(dep, lim, left) sees every step."""
    t, pt, win = Tree(), LevelTables(), Window()
    pad = list(bits) + [0] * 136
    b = np.array(pad, dtype=np.int64)
    v8 = np.zeros(len(pad) - 7, dtype=np.int64)
    for k in range(8):
        v8 = (v8 << 1) | b[k:len(pad) - 7 + k]
    st = {"steps": 0, "alone": 0, "sent": 0, "capped": 0, "nyt_first": 0, "links": {}, "instr": 0, "nops": 0}
    ed = {e: 0 for e in EDGES}
    out, pos = [], 0
    l8, built = None, -1

    def alone():
        nonlocal pos
        win.top_up()
        x, d, _ = pt.lookup(t, pad, pos)
        dt = pt.L[8][int(v8[pos])][1]
        win.nwin -= dt
        win.top_up()
        win.take(d - dt)
        pos += d
        fresh = bool(t.body[x] & NYT)
        if fresh:
            sym = int(v8[pos])
            pos += 8
            if win.nwin < 8:
                win.refill()
            win.nwin -= 8
            t.split(sym)
        else:
            sym = t.body[x]
        out.append(sym)
        t.update(t.where[sym])
        for s, lead in t.swaps:
            pt.on_swap(s, lead)

    while len(out) < n:
        i = len(out)
        win.top_up()
        if pt.frm < 9:
            pt.build(t)
        if built != pt.rebuilds:
            l8, built = np.array([d for _, d in pt.L[8]]), pt.rebuilds
        dep = l8[v8[pos:pos + 64]].tolist()
        if dep[0] == 0 or dep[0] >= EXIT_BITS:
            st["sent"] += 1
            alone()
            continue
        left = min(n, i - i % BLOCK + BLOCK) - i
        n0 = win.nwin
        assert 32 <= n0 <= 64
        lim = 63 if topup else min(n0, 63)
        if on_step:
            on_step(dep, lim, left)
        sv, links, tests = chain(dep, lim, stride)
        nval, jmax, se, _, _ = derive(sv, lim, cap, left)
        paths = []
        for j in range(jmax):
            x, d = ROOT, 0
            while t.body[x] & INNER and d < sv[j + 1] - sv[j]:
                x = (t.body[x] & 255) * 2 + pad[pos + sv[j] + d]
                d += 1
            if t.body[x] & (INNER | NYT):
                ed["nonleaf_mid"] += j > 0
                ed["stale_entry"] += d < 8 and bool(t.body[x] & INNER)
                paths.append(None)
                break
            paths.append(t.path(x) + [ROOT])
        jf = tentative_len(t, paths)
        sj = sv[jf]
        st["steps"] += 1
        st["capped"] += jf == cap
        st["nyt_first"] += paths[:1] == [None] and not t.body[x] & INNER
        st["links"][links] = st["links"].get(links, 0) + 1
        ins, nops = instructions(stride, links, tests)
        st["instr"] += ins
        st["nops"] += nops
        s1 = chain(dep, lim, 1)[0] if stride != 1 else sv
        real = [v for v in s1[1:17] if v != 255]
        ed["start_62"] += 62 in real
        ed["start_63"] += 63 in real
        ed["start_64"] += 64 in real
        ed["start_past_64"] += any(v > 64 for v in real)
        ed["jump_past_63"] += any(v <= 63 and v + dep[v] > 63 for v in [0] + real)
        ed["odd_last"] += jmax % 2 == 1 and jf == jmax
        ed["one_bit_16"] += s1[16] == 16
        ed["six_bit_cross"] += any(j % 4 and s1[j - 1] <= 62 < s1[j] != 255 and dep[s1[j - 1]] == 6 for j in range(1, 17))
        ed["block_end"] += left < PACK_MAX and jmax == left < nval
        ed["peeked_used"] += topup and sj > n0
        for k in (4, 8, 12):
            ed[f"exit_{k}"] += s1[k] != 255 and s1[k + 1] == 255
        for p in paths[:jf]:
            out.append(t.body[p[0]])
            for a in p:
                t.w[a] += 1
        win.nwin = n0 - sj
        if win.nwin < 0:
            win.refill()
        pos += sj
        if jf < len(paths):
            st["alone"] += 1
            alone()
    assert win.consumed() == pos
    return out, st, ed, t


def report(oracle_mod, n=60000):
    """the text of profiles/r13_chain_model.txt"""
    from fgk_topup_model import bench_streams, decode_topup
    lines = ["# chain of code starts in the decoder's packed step (tests/fgk_chain_model.py), first %d symbols, -c -m," % n,
             "# 64 true window bits, cap 16: steps, links per step and the share of steps running 4 / 8 / 12 / 16 links at",
             "# stride 1, then per stride the chain's VALU + SALU + LDS instructions and s_nop per step and per symbol",
             "# (link 3 + 2 s_nop, exit test 2, composition 6, fill 6: the ISA of decode_kernel<0, 0, false>)"]
    for name, syms in bench_streams(oracle_mod, n):
        bits = stream_bits(syms)
        ref = decode_topup(syms)[1]
        line = None
        for stride in STRIDES:
            out, st, _, _ = decode_chain(bits, len(syms), stride)
            assert out == syms and abs(st["steps"] - ref["steps"]) <= 0.02 * ref["steps"] + 32
            steps = max(st["steps"], 1)
            if stride == 1:
                share = [100.0 * st["links"].get(k, 0) / steps for k in (4, 8, 12, 16)]
                line = "%-8s steps %5d  links/step %5.2f  share 4/8/12/16 %4.1f %4.1f %4.1f %4.1f %%" % (
                    name, st["steps"], sum(k * v for k, v in st["links"].items()) / steps, *share)
            line += "  | stride %d: %5.1f + %4.1f nop /step, %5.2f + %4.2f /sym" % (
                stride, st["instr"] / steps, st["nops"] / steps, st["instr"] / len(syms), st["nops"] / len(syms))
        lines.append(line)
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    import oracle
    sys.stdout.write(report(oracle))
