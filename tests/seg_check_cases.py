"""Inputs shared by the checked-container tests: the raw inputs by name, and the three payload
flips that decode cleanly, to the cut's length, to other bytes (found with the oracle by flipping
bits 0, 3 and 7 of every payload byte of segment 1). Test infrastructure only."""
import numpy as np

import seg_check_model as scm

_raws = {}


def raw(name):
    """'rng:HI:N': N bytes below HI from default_rng(1); 'photo:W:H': oracle.synth('photo', 3, W, H)"""
    if name not in _raws:
        kind, a, b = name.split(":")
        if kind == "rng":
            _raws[name] = np.random.default_rng(1).integers(0, int(a), int(b), dtype=np.uint8).tobytes()
        else:
            import oracle
            _raws[name] = oracle.synth(kind, 3, int(a), int(b)).tobytes()
    return _raws[name]


# (raw input, use_diff, use_adapt, width, seg_bytes, byte of segment 1's stream, bit)
SILENT_FLIPS = [
    ("photo:64:200", True, False, 512, 4096, 9, 0),
    ("photo:64:200", True, True, 64, 4096, 15, 0),
    ("rng:256:100", True, False, 512, 32, 9, 0),
]
FLIP_IDS = ["photo-cm-s4096", "photo-am-w64-s4096", "rng100-cm-s32"]


def flip(container, seg, byte, bit):
    """the container with one bit of one segment's stream flipped (index and crc words kept)"""
    streams = scm.segments(container)
    s = streams[seg]
    streams[seg] = s[:byte] + bytes([s[byte] ^ (1 << bit)]) + s[byte + 1:]
    return scm.repack(container, streams)
