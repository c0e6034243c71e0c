"""The lane-parallel inflate's window rule in pure Python over ``png_decode_model``'s bit reader: what
``inflate_lanes_kernel`` and ``cgan_png_inflate_lanes_host`` do, lane by lane and pass by pass.

A window starts at a committed bit ``P`` inside a block of Huffman codes and is ``64 * S`` bits long; lane i owns the bits
``[P + i * S, P + (i + 1) * S)`` and decodes the tokens that begin there -- first from its own first bit, a guess, then from
the exit bit of lane i - 1 whenever that changes.  After pass k lanes 0 .. k - 1 hold what a serial decode gives, so the
passes end after at most 64.  The lanes up to the first one that stopped for another reason than its range's end are
committed; the checks that need the output position are made then.  Block headers, stored blocks and the trailer are read
serially.  The committed tokens are ``png_decode_model.inflate``'s token list (tests/test_png_lanes_host.py)."""
import zlib

import png_decode_model as pm

LANES = 64
NONE, EOB, BAD, FULL = 0, 1, 2, 3


def decode_subseq(data, e, lt, dt, end, cap):
    """The tokens that begin in [e, end) -> (exit bit, flag, tokens).  Nothing here knows the output position."""
    b, tokens = pm._Bits(data, e), []
    while True:
        at = b.pos
        if at >= end:
            return at, NONE, tokens
        if len(tokens) >= cap:
            return at, FULL, tokens
        try:
            s = b.symbol(*lt)
            if s < 256:
                tokens.append(("lit", s))
                continue
            if s == 256:
                return b.pos, EOB, tokens
            if s > 285:
                return at, BAD, tokens
            n = pm.LENGTH_BASE[s - 257] + b.take(pm.LENGTH_EXTRA[s - 257])
            ds = b.symbol(*dt)
            if ds > 29:
                return at, BAD, tokens
            tokens.append(("match", n, pm.DIST_BASE[ds] + b.take(pm.DIST_EXTRA[ds])))
        except pm.Corrupt:
            return at, BAD, tokens


def window(data, P, S, cap, lt, dt):
    """One window -> (passes, the last committed lane, per lane (entry, exit bit, flag, tokens))."""
    entry = [P] + [P + i * S for i in range(1, LANES)]
    changed, res, passes = [True] * LANES, [None] * LANES, 0
    while any(changed):
        passes += 1
        assert passes <= LANES
        for i in range(LANES):
            if changed[i]:
                end = P + (i + 1) * S
                res[i] = (entry[i], NONE, []) if entry[i] >= end else decode_subseq(data, entry[i], lt, dt, end, cap)
        changed = [False] * LANES
        for i in range(1, LANES):
            if res[i - 1][1] == NONE and res[i - 1][0] != entry[i]:
                entry[i], changed[i] = res[i - 1][0], True
    last = next((i for i in range(LANES) if res[i][1] != NONE), LANES - 1)
    return passes, last, [(entry[i],) + tuple(res[i]) for i in range(LANES)]


def _header(b, stream):
    """A block's header at the reader's place -> (last, kind, lt, dt, stored bytes); ``png_decode_model.inflate``'s rules."""
    last, kind = b.take(1), b.take(2)
    if kind == 3:
        raise pm.Corrupt("block type 3")
    if kind == 0:
        b.pos = (b.pos + 7) & ~7
        n, nn = b.take(16), b.take(16)
        if n ^ nn != 0xFFFF:
            raise pm.Corrupt("LEN and NLEN disagree")
        at = b.pos >> 3
        if at + n > len(stream):
            raise pm.Corrupt("the stream ends early")
        b.pos += 8 * n
        return last, "stored", None, None, stream[at:at + n]
    if kind == 1:
        return last, "fixed", pm._table(pm.FIXED_LIT), pm._table(pm.FIXED_DIST), None
    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    if hlit > 286 or hdist > 30:
        raise pm.Corrupt("too many symbols")
    cl = [0] * 19
    for k in range(hclen):
        cl[pm.CL_ORDER[k]] = b.take(3)
    if sum(1 for v in cl if v) == 0 or sum(2 ** (15 - v) for v in cl if v) != 2 ** 15:
        raise pm.Corrupt("the code-length code is not complete")
    ct, lens = pm._table(cl), []
    while len(lens) < hlit + hdist:
        s = b.symbol(*ct)
        if s < 16:
            lens.append(s)
            continue
        if s == 16 and not lens:
            raise pm.Corrupt("nothing to repeat")
        v, rep = (lens[-1], 3 + b.take(2)) if s == 16 else ((0, 3 + b.take(3)) if s == 17 else (0, 11 + b.take(7)))
        if len(lens) + rep > hlit + hdist:
            raise pm.Corrupt("a repeat runs past the lengths")
        lens += [v] * rep
    if lens[256] == 0:
        raise pm.Corrupt("no end-of-block code")
    return last, "dynamic", pm._table(lens[:hlit]), pm._table(lens[hlit:]), None


def inflate_lanes(stream, S, cap, limit):
    """A zlib stream -> (bytes, tokens, stats, windows, blocks).  tokens as ``png_decode_model.inflate`` lists them.  stats: windows,
    passes (in all), max_passes (in one window), full_windows (ended by a lane's cap), tokens (committed from windows).
    windows: per window a dict -- start, passes, lanes (committed), flag (of the last committed lane), exit, empty (committed
    lanes that held no token because their entry lay behind their range), block (its index), crosses_end.  blocks: kinds."""
    assert S % 32 == 0 and S > 0 and cap >= 1
    b, out, tokens, windows, blocks = pm._Bits(stream, 16), bytearray(), [], [], []
    stats = {"windows": 0, "passes": 0, "max_passes": 0, "full_windows": 0, "tokens": 0}
    while True:
        last, kind, lt, dt, stored = _header(b, stream)
        blocks.append(kind)
        if kind == "stored":
            if len(out) + len(stored) > limit:
                raise pm.Corrupt("more output than the image has")
            out += stored
            tokens.append(("stored", len(stored)))
        else:
            P = b.pos
            while True:
                passes, c, lanes = window(stream, P, S, cap, lt, dt)
                committed = [t for lane in lanes[:c + 1] for t in lane[3]]
                _, exit_bit, flag, _ = lanes[c]
                stats["windows"] += 1
                stats["passes"] += passes
                stats["max_passes"] = max(stats["max_passes"], passes)
                stats["full_windows"] += flag == FULL
                stats["tokens"] += len(committed)
                windows.append({"start": P, "passes": passes, "lanes": c + 1, "flag": flag, "exit": exit_bit, "S": S,
                                "empty": sum(1 for i, lane in enumerate(lanes[:c + 1]) if lane[0] >= P + (i + 1) * S),
                                "block": len(blocks) - 1, "crosses_end": P + LANES * S > 8 * len(stream),
                                "counts": [len(lane[3]) for lane in lanes[:c + 1]]})
                for t in committed:                      # the checks that need the output position
                    n = 1 if t[0] == "lit" else t[1]
                    if t[0] == "match" and t[2] > len(out):
                        raise pm.Corrupt("a distance in front of the output's start")
                    if len(out) + n > limit:
                        raise pm.Corrupt("more output than the image has")
                    if t[0] == "lit":
                        out.append(t[1])
                    else:
                        for _ in range(n):
                            out.append(out[-t[2]])
                    tokens.append(t)
                if flag == BAD:
                    raise pm.Corrupt("an invalid symbol or the stream's end in a committed lane")
                P = exit_bit
                if flag == EOB:
                    break
            b.pos = P
        if last:
            break
    b.pos = (b.pos + 7) & ~7
    adler = 0
    for _ in range(4):
        adler = (adler << 8) | b.take(8)
    if len(out) != limit:
        raise pm.Corrupt("less output than the image has")
    if adler != zlib.adler32(bytes(out)):
        raise pm.Corrupt("Adler-32 mismatch")
    return bytes(out), tokens, stats, windows, blocks
