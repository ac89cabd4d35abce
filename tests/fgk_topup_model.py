"""Model of the decoder's packed batch step on a window of 64 true bits (hc_fgk.hip
Dec::decode_batch with HC_DEC_TOPUP 1; BitSource::peek, BitSource::take_peeked), on the slot-form
tree of fgk_cache_model.py and with the step of fgk_pack_model.decode_packed.

The window holds nwin valid bits and is refilled by one 32-bit word whenever a call site finds at
most 32 valid, so a step starts with n0 = 32..64 of them (32 only after a step that took the whole
window: 0 bits left, one refill). Before the step the top 64 - n0 bits of the next unread word are
ORed below them (a peek: no state changes; one word is enough from 32 valid bits on), and the step
takes codes up to bit 62 whatever n0 was. A step that took sj > n0 bits used sj - n0 bits of the
peeked word: nwin = n0 - sj is negative, and the one refill that follows pushes that word with
those bits shifted out (a shift of 32 - nwin <= 63; 1..31 valid bits after it, which the next call
site's refill brings to 33 or more).

The model tracks what the kernel's BitSource tracks: nwin (signed) and the index of the next
unread word (the kernel's ridx is that index mod 64: the 256-byte chunk rolls over when it reaches
64), refilling exactly where the kernel's call sites do. The bits read are then
32 * words pushed - nwin - 72 (Dec::consumed), which must be the sum of the code lengths.

topup=False is the shipped window of fgk_pack_model.decode_packed (lim = min(n0, 63)), with the
same bookkeeping.
"""
from fgk_batch_model import batch_len, tentative_len
from fgk_cache_model import ROOT, Tree
from fgk_pack_model import BLOCK, EXIT_BITS, PACK_MAX, TABLE_DEPTH

EVENTS = ("sj_eq_n0", "sj_eq_n0_plus_1", "sj_past_n0_by_24", "neg_refill_rolls_chunk", "peek_last_word", "use_last_word")


class Window:
    """BitSource's counters: nwin valid bits, word = index of the next unread 32-bit word of the
    stream (the header is words 0, 1 and the first byte of word 2)"""

    def __init__(self):
        self.word = 3
        self.nwin = 24

    def refill(self):
        assert self.nwin <= 32
        self.nwin += 32
        self.word += 1

    def top_up(self):  # the call sites' `if (in.nwin <= 32) in.refill();`
        assert self.nwin >= 0
        if self.nwin <= 32:
            self.refill()

    def take(self, d):
        """a code's bits one after the other (the descent: a refill only once the window is empty)"""
        while d > self.nwin:
            d -= self.nwin
            self.nwin = 0
            self.refill()
        self.nwin -= d

    def consumed(self):
        return self.word * 32 - self.nwin - 72


def decode_topup(symbols, cap=PACK_MAX, topup=True, exit_bits=EXIT_BITS, lockstep=False, last_word=None):
    """(tree, stats, window): decode `symbols` with packed steps of up to `cap` codes.
    stats: steps, alone, sent, capped as decode_packed's, ended_window (steps that the window's
    bits ended: the next code did not fit), and one count per name in EVENTS:
      sj_eq_n0, sj_eq_n0_plus_1, sj_past_n0_by_24: steps that took sj = n0, n0 + 1, >= n0 + 24 bits;
      neg_refill_rolls_chunk: a refill at negative nwin that read word 63 of its chunk;
      peek_last_word / use_last_word: steps whose peeked word was word `last_word` of the stream
      (its last), and those of them that took bits from it.
    lockstep: a second tree takes the one-symbol update symbol by symbol and is compared after
    every step and every symbol decoded alone."""
    t = Tree()
    ref = Tree() if lockstep else None
    st = {"steps": 0, "alone": 0, "sent": 0, "capped": 0, "ended_window": 0}
    st.update({e: 0 for e in EVENTS})
    win = Window()
    bits = 0  # the code lengths' sum

    def table_depth(sym):
        """the depth at which the level tables' entry for sym's code stops: its leaf, the NYT, or
        level 8"""
        x = t.where[sym]
        return min(len(t.path(x if x else t.nyt)), TABLE_DEPTH)

    def code_bits(sym):
        x = t.where[sym]
        return len(t.path(x)) if x else len(t.path(t.nyt)) + 8

    def follow(syms):
        if ref is None:
            return
        for s in syms:
            if ref.where[s] == 0:
                ref.split(s)
            ref.update(ref.where[s])
        assert t.w == ref.w and t.body == ref.body and t.up == ref.up

    def alone(sym):
        """the one-symbol step: the table entry's bits in the hot loop, the rest of a longer code
        in the descent, the eight bits of a new symbol after the NYT"""
        nonlocal bits
        win.top_up()
        fresh = t.where[sym] == 0
        total = code_bits(sym) - (8 if fresh else 0)
        d = table_depth(sym)
        win.nwin -= d
        win.top_up()
        win.take(total - d)
        if fresh:
            if win.nwin < 8:
                win.refill()
            win.nwin -= 8
            t.split(sym)
        t.update(t.where[sym])
        bits += total + (8 if fresh else 0)
        follow([sym])

    i, n = 0, len(symbols)
    while i < n:
        win.top_up()
        if code_bits(symbols[i]) >= exit_bits:
            st["sent"] += 1
            alone(symbols[i])
            i += 1
            continue
        i1 = min(n, i - i % BLOCK + BLOCK)
        n0 = win.nwin
        assert 32 <= n0 <= 64, (n0, i)
        lim = 63 if topup else min(n0, 63)
        paths, s, full = [], 0, False
        for sym in symbols[i:min(i1, i + cap)]:
            x = t.where[sym]
            p = t.path(x) if x else None
            if p is None or len(p) > TABLE_DEPTH:
                if s + table_depth(sym) <= lim:
                    paths.append(None)
                else:
                    full = True
                break
            if s + len(p) > lim:
                full = True
                break
            s += len(p)
            paths.append(p + [ROOT])
        jf = tentative_len(t, paths)
        assert jf <= batch_len(t, paths)
        sj = sum(len(p) - 1 for p in paths[:jf])
        assert sj <= 63
        st["steps"] += 1
        st["capped"] += jf == cap
        st["ended_window"] += full and jf == len(paths)
        if topup:
            st["sj_eq_n0"] += sj == n0
            st["sj_eq_n0_plus_1"] += sj == n0 + 1
            st["sj_past_n0_by_24"] += sj - n0 >= 24
            if last_word is not None and win.word == last_word:
                st["peek_last_word"] += 1
                st["use_last_word"] += sj > n0
        else:
            assert sj <= n0
        for p in paths[:jf]:
            for a in p:
                t.w[a] += 1
        win.nwin = n0 - sj
        if win.nwin < 0:  # BitSource::take_peeked
            assert topup and 32 - win.nwin <= 63  # the refill's shift
            st["neg_refill_rolls_chunk"] += win.word % 64 == 63
            win.refill()
            assert 1 <= win.nwin <= 31
        bits += sj
        follow(symbols[i:i + jf])
        i += jf
        if jf < len(paths):
            st["alone"] += 1
            alone(symbols[i])
            i += 1
    assert win.nwin >= 0 and win.consumed() == bits
    return t, st, win


def bench_streams(oracle_mod, n=60000):
    """(name, symbols): the first n symbols of the benchmark's photo streams 0-3, grad and noise
    (512 x 512, -c -m)"""
    out = []
    for kind, ks in (("photo", range(4)), ("grad", [0]), ("noise", [0])):
        for k in ks:
            raw = oracle_mod.synth(kind, k, 512, 512).tobytes()
            out.append((f"{kind} {k}", list(oracle_mod.rle(oracle_mod.diff(raw)))[:n]))
    return out


if __name__ == "__main__":  # the step counts (profiles/r10_topup_model.txt)
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    import oracle
    print("# packed decoder steps per stream (first 60000 symbols, -c -m, gate 7 bits): the window's own 32..64 bits")
    print("# (HC_DEC_TOPUP 0) against 64 true bits (HC_DEC_TOPUP 1) at caps 16 / 20 / 24; steps, symbols alone, steps at the cap,")
    print("# steps the window ended")
    for name, syms in bench_streams(oracle):
        line = f"{name:8}"
        for topup, cap in ((False, 16), (True, 16), (True, 20), (True, 24)):
            st = decode_topup(syms, cap=cap, topup=topup)[1]
            line += f" | {'topup' if topup else 'own  '} cap {cap}: {st['steps']:5} {st['alone']:5} {st['capped']:5} {st['ended_window']:5}"
        print(line)
