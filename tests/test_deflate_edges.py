"""The shared deflate (ndt_amd/csrc/ndt_deflate.hpp) at the edges its other tests never reach: the Huffman limiter at 15 and at 7
bits, the header's run-length coder, the HLIT / HDIST / HCLEN trims, the bit a non-final chunk ends on, short last chunks and
checksums that pass their modulus many times -- through encode_png, encode_png16 (grey) and encode_exr (half), nothing else.

Two yardsticks, neither of them the device's own output:
  * Python's zlib inside the sinks' existing readers (it refuses over-subscribed and incomplete codes and checks the Adler-32);
  * the block reader below, written from RFC 1951: it inflates a raw deflate stream block by block and says what each block's
    header held, so that a test can show from the file that the edge it is named for was reached.
Every case starts from the bytes the deflate is to see.  The sink's front end is inverted to get an image (PNG: the bytes
themselves behind filter 0, or their running sum at the pixel stride behind filter 1; OpenEXR half: the running sum of the deltas
split into the low and the high bytes of the samples), and a CPU test shows that the models of the front ends give those bytes
back and that the bytes have the property the case is named for -- computed from them with the token rule the header comment of
ndt_deflate.hpp states (a run at distance D is one literal and matches in pieces of 258, a last piece under 3 bytes is literals)
and a plain heapq Huffman.
"""
import functools
import heapq
import struct
import zlib

import numpy as np
import pytest

import test_exr_device as ex
import test_png16_device as p16
import test_png_device as p8

from ndt_amd import hip as nh

CHUNK = 32768

# ---------------------------------------------------------------- RFC 1951: the block reader

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k // 2 - 1 for k in range(4, 30)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30


class Block(object):
    """one block of a deflate stream: kind 0 stored / 1 fixed / 2 dynamic, final, the bit offsets start and end, hlit / hdist /
    hclen (counts, not the fields), cl_lens [19], tokens [(symbol, extra)], ll_lens, d_lens, hist [286], data"""


def _canonical(lens):
    """{(length, code): symbol} of the canonical code RFC 1951 3.2.2 assigns to the lengths"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    table = {}
    for sym, l in enumerate(lens):
        if l:
            table[(l, nxt[l])] = sym
            nxt[l] += 1
    return table


class _Bits(object):
    def __init__(self, data):
        self.d, self.pos = data, 0

    def bit(self):
        b = (self.d[self.pos >> 3] >> (self.pos & 7)) & 1
        self.pos += 1
        return b

    def take(self, n):
        v = 0
        for k in range(n):
            v |= self.bit() << k
        return v

    def symbol(self, table):
        code = 0
        for l in range(1, 16):
            code = (code << 1) | self.bit()
            if (l, code) in table:
                return table[(l, code)]
        raise AssertionError("no code of up to 15 bits at bit %d" % self.pos)


def inflate_blocks(data):
    """(blocks, the bytes, the bit offset behind the final block) of the raw deflate stream that starts `data`"""
    rd, out, blocks = _Bits(data), bytearray(), []
    while True:
        b = Block()
        b.start = rd.pos
        b.final, b.kind = bool(rd.bit()), rd.take(2)
        b.hlit = b.hdist = b.hclen = 0
        b.cl_lens, b.tokens, b.ll_lens, b.d_lens = [], [], [], []
        b.hist = np.zeros(286, dtype=np.int64)
        first = len(out)
        assert b.kind != 3, "block type 3 at bit %d" % b.start
        if b.kind == 0:
            rd.pos = (rd.pos + 7) & ~7
            n, inv = rd.take(16), rd.take(16)
            assert n ^ inv == 0xffff, "LEN / NLEN at bit %d" % rd.pos
            at = rd.pos >> 3
            assert at + n <= len(data)
            out += data[at:at + n]
            rd.pos += 8 * n
        else:
            if b.kind == 1:
                b.ll_lens, b.d_lens = list(FIXED_LL), list(FIXED_D)
            else:
                b.hlit, b.hdist, b.hclen = rd.take(5) + 257, rd.take(5) + 1, rd.take(4) + 4
                assert b.hlit <= 286 and b.hdist <= 30
                b.cl_lens = [0] * 19
                for k in range(b.hclen):
                    b.cl_lens[CL_ORDER[k]] = rd.take(3)
                cl, lens = _canonical(b.cl_lens), []
                while len(lens) < b.hlit + b.hdist:
                    sym = rd.symbol(cl)
                    if sym < 16:
                        b.tokens.append((sym, 0))
                        lens.append(sym)
                    elif sym == 16:
                        assert lens, "a repeat with nothing in front of it"
                        extra = rd.take(2)
                        b.tokens.append((16, extra))
                        lens += [lens[-1]] * (3 + extra)
                    else:
                        extra = rd.take(3 if sym == 17 else 7)
                        b.tokens.append((sym, extra))
                        lens += [0] * ((3 if sym == 17 else 11) + extra)
                assert len(lens) == b.hlit + b.hdist, "a run leaves the header's lengths"
                b.ll_lens, b.d_lens = lens[:b.hlit], lens[b.hlit:]
            ll, dd = _canonical(b.ll_lens), _canonical(b.d_lens)
            while True:
                sym = rd.symbol(ll)
                b.hist[sym] += 1
                if sym < 256:
                    out.append(sym)
                elif sym == 256:
                    break
                else:
                    n = LEN_BASE[sym - 257] + rd.take(LEN_EXTRA[sym - 257])
                    ds = rd.symbol(dd)
                    dist = DIST_BASE[ds] + rd.take(DIST_EXTRA[ds])
                    assert dist <= len(out)
                    for _ in range(n):
                        out.append(out[-dist])
        b.end = rd.pos
        b.data = bytes(out[first:])
        blocks.append(b)
        if b.final:
            return blocks, bytes(out), rd.pos


# ---------------------------------------------------------------- the models the preconditions are computed with

def length_symbol(n):
    return 285 if n == 258 else 257 + max(k for k in range(28) if LEN_BASE[k] <= n)


def model_hist(chunk, dist):
    """The literal / length histogram (end-of-block included) of one chunk under the stated token rule: byte i heads a run when it
    differs from the byte `dist` before it (the chunk's first `dist` bytes always do); a run of k bytes is its head as a literal
    and the other k - 1 as matches in pieces of 258, a last piece under 3 bytes as literals.  Returns (hist [286], matches)."""
    s = np.frombuffer(bytes(chunk), dtype=np.uint8)
    head = np.ones(s.size, dtype=bool)
    head[dist:] = s[dist:] != s[:-dist]
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], s.size)
    hist = np.bincount(s[starts], minlength=286).astype(np.int64)
    matches = 0
    for a, e in zip(starts[ends - starts > 1], ends[ends - starts > 1]):
        at, m = a + 1, e - a - 1
        while m > 0:
            piece = min(m, 258)
            if piece < 3:
                np.add.at(hist, s[at:at + piece], 1)
            else:
                hist[length_symbol(piece)] += 1
                matches += 1
            at, m = at + piece, m - piece
    hist[256] += 1
    return hist, matches


def huffman_lengths(freq):
    """Code lengths of an unlimited Huffman code, equal weights merged shallowest first: its depth is the least any tie-breaking
    gives.  One used symbol gets length 1."""
    used = [s for s, f in enumerate(freq) if f]
    lens = [0] * len(freq)
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    heap = [(int(freq[s]), 0, [s]) for s in used]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            lens[s] += 1
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, a[2] + b[2]))
    return lens


def unlimited_depth(freq):
    return max(huffman_lengths(freq))


def header_tokens(lens):
    """RFC 1951 3.2.7, the usual greedy way: zeros in runs of up to 138 (18 from 11, 17 from 3), a length equal to the one in front
    of it in runs of up to 6 (16 from 3)"""
    out, i = [], 0
    while i < len(lens):
        v, run = lens[i], 1
        while i + run < len(lens) and lens[i + run] == v and run < 138:
            run += 1
        if v == 0 and run >= 11:
            out.append((18, run - 11))
        elif v == 0 and run >= 3:
            out.append((17, run - 3))
        elif v and i and lens[i - 1] == v and run >= 3:
            run = min(run, 6)
            out.append((16, run - 3))
        else:
            out.append((v, 0))
            run = 1
        i += run
    return out


def token_hist(tokens):
    return np.bincount([s for s, _ in tokens], minlength=19)


def runs_of(lens):
    """{(value is zero, run length)} of the maximal runs of equal values"""
    a = np.asarray(lens)
    edges = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1], [True])))
    return set((bool(a[e] == 0), int(n)) for e, n in zip(edges[:-1], np.diff(edges)))


def model_header(chunk, dist):
    """what any exact Huffman coder makes of a chunk whose frequencies fix the lengths: (hlit, lengths the header lists, tokens)"""
    hist, matches = model_hist(chunk, dist)
    lens = huffman_lengths(hist)
    hlit = max(s for s in range(286) if lens[s]) + 1
    listed = lens[:hlit] + [0] * (dist - 1) + [1 if matches else 0]
    return hlit, listed, header_tokens(listed)


# ---------------------------------------------------------------- the sinks' front ends, inverted

SMALL = [0, 1, 255, 2, 254, 3, 253, 4, 252, 5, 251, 6, 250, 7, 249, 8, 248, 9, 247, 10, 246, 11, 245, 12, 244]     # near 0 as int8


def png_image(stream, rows, bpp):
    """The image whose filtered stream is `stream` ([rows, 1 + bpp w] flattened; every row's first byte is its filter, 0 or 1):
    (rows, w, 4) uint8 for bpp 4, (rows, w) uint16 for bpp 2."""
    s = np.asarray(stream, dtype=np.uint8).reshape(rows, -1)
    assert (s.shape[1] - 1) % bpp == 0 and (s[:, 0] <= 1).all()
    raw = s[:, 1:].copy()
    for r in range(rows):
        if s[r, 0] == 1:
            raw[r] = np.cumsum(raw[r].reshape(-1, bpp), axis=0, dtype=np.uint8).reshape(-1)
    if bpp == 4:
        return raw.reshape(rows, -1, 4)
    return np.ascontiguousarray(raw).view(">u2").astype(np.uint16)


def exr_image(stream, lines, width):
    """The (lines, width, 4) doubles whose half RGBA block is `stream` after the byte planes and the predictor: the running sum of
    the deltas gives the low bytes (first half) and the high bytes (second half) of the samples, which must not be NaN or
    infinite; the doubles are those halves exactly."""
    d = np.asarray(stream, dtype=np.int64).copy()
    assert d.size == 8 * lines * width
    d[1:] -= 128
    t = np.cumsum(d) % 256
    low, high = t[:d.size // 2], t[d.size // 2:]
    assert ((high & 0x7c) != 0x7c).all(), "a sample that is not finite"
    halves = (high << 8 | low).astype(np.uint16).view(np.float16).astype(np.float64).reshape(lines, 4, width)
    fb = np.empty((lines, width, 4))
    for c, (_, _, src) in enumerate(ex.channel_list(ex.HALF, False)):
        fb[:, :, src] = halves[:, c, :]
    return fb


def exr_tail(first_half, high=0x3c):
    """the block's stream when every sample's high byte is `high`: the wanted deltas, the step to the high plane, 128s"""
    c = np.asarray(first_half, dtype=np.int64)
    last = (c[0] + (c[1:] - 128).sum()) % 256
    return np.concatenate([c, [(high - last + 128) % 256], np.full(c.size - 1, 128)]).astype(np.uint8)


class Case(object):
    """sink: png / png16 / exr; image; streams: what each of the file's deflate streams is to inflate to; dist; expect: what the
    case is named for"""

    def __init__(self, sink, image, streams, **expect):
        self.sink, self.image, self.expect = sink, image, expect
        self.streams = [np.asarray(s, dtype=np.uint8).tobytes() for s in streams]
        self.dist = 2 if sink == "exr" else 1


def png_case(sink, stream, rows=1, **expect):
    bpp = 4 if sink == "png" else 2
    return Case(sink, png_image(stream, rows, bpp), [stream], **expect)


def exr_case(stream, lines, width, **expect):
    return Case("exr", exr_image(stream, lines, width), [stream], **expect)


def front_end(case):
    """the models of the sinks' front ends: the byte streams the deflate sees"""
    if case.sink == "png":
        return [p8.filter_rows(case.image)[1].tobytes()]
    if case.sink == "png16":
        return [p16.filter_rows(case.image)[1].tobytes()]
    return [pre for _, pre in ex.model_blocks(case.image, None, ex.HALF)]


def chunks_of(stream):
    return [stream[k:k + CHUNK] for k in range(0, len(stream), CHUNK)]


# ---------------------------------------------------------------- stream builders

def arrange(freq, dist, seed, pinned=None):
    """The values of {value: count} in an order in which no three bytes in a row equal the byte `dist` before them, so that the
    token rule finds no match; pinned {position: value} (counted in freq) stay where they are."""
    pinned = dict(pinned or {})
    n = int(sum(freq.values()))
    pinned = dict((p % n, v) for p, v in pinned.items())
    left = dict(freq)
    for v in pinned.values():
        left[v] -= 1
    assert min(left.values()) >= 0
    for attempt in range(64):
        rng = np.random.default_rng(seed + 1000 * attempt)
        pool = rng.permutation(np.repeat(list(left.keys()), list(left.values()))).tolist()
        s, free = [0] * n, [p for p in range(n) if p not in pinned]
        for p, v in pinned.items():
            s[p] = v
        for p, v in zip(free, pool):
            s[p] = v
        for k, p in enumerate(free):
            if p >= 3 * dist and all(s[p - j] == s[p - j - dist] for j in range(3)):
                for q in free[k + 1:]:
                    if s[q] != s[p]:
                        s[p], s[q] = s[q], s[p]
                        break
        s = np.array(s, dtype=np.uint8)
        if model_hist(s, dist)[1] == 0:
            return s
    raise AssertionError("no order without a match")


def chain_weights(n_sym, forced=()):
    """n_sym ascending weights, the first (the end-of-block symbol) and the second 1, each later one more than the sum of all
    weights two or more places below it: the merge then never has a choice that changes a depth, and the code's depth is
    n_sym - 1.  The smallest such weights (1 1 2 3 5 8 ...), but for the forced ones, taken as late as they still fit."""
    w, pending = [1], sorted(forced)
    for k in range(1, n_sym):
        need = max(sum(w[:k - 1]) + 1, w[-1])
        if pending and need <= pending[0] <= sum(w[:k]):
            w.append(pending.pop(0))
        else:
            w.append(need)
    assert not pending, "a forced weight that fits nowhere"
    return w


def limiter15_png(sink, n_sym):
    """A one-row stream behind filter 1 whose literals and end-of-block have chain weights: every byte a literal, value 0 the
    commonest (raised until the row is full), then 1, 255, 2, ... so that Sub's cost stays small."""
    bpp = 4 if sink == "png" else 2
    w = chain_weights(n_sym)
    width = -(-(sum(w) - 2) // bpp)
    w[-1] += 1 + bpp * width - (sum(w) - 1)
    freq = dict(zip(SMALL, w[:0:-1]))
    return png_case(sink, arrange(freq, 1, n_sym, {0: 1}), depth15=n_sym - 1)


def limiter15_exr(n_sym):
    """The same for a one-line half block of width w.  Behind the 4 w wanted bytes come the step to the high plane -- a value
    used nowhere else, the chain's second 1 -- two 128s and a run of 4 w - 3 bytes: q matches of 258 and one more 128, with
    4 w = 258 q + 4.  Symbol 285's weight q is one of the chain's; 128 is the commonest value."""
    for q in range(2, 200, 2):
        w = chain_weights(n_sym, [q])
        n = 258 * q + 4
        rest = list(w[2:])
        rest.remove(q)
        if sum(rest) > n:
            continue
        rest[-1] += n - sum(rest)
        for shift in range(64):
            values = [128] + [(130 + shift + k) % 256 for k in range(len(rest) - 1)]
            freq = dict(zip(values, rest[::-1]))
            first = arrange(freq, 2, n_sym + shift, {-1: values[1], -2: values[1]})
            stream = exr_tail(first)
            if int(stream[n]) not in values:
                assert stream.size <= CHUNK
                return exr_case(stream, 1, n // 4, depth15=n_sym - 1)
    raise AssertionError("no width fits")


def limiter15_exr_deep(n_sym):
    """The chain of 19 literals needs 17 709 bytes, and a half block whose high-byte plane is one run spends as many again on
    that run: too much for one chunk.  So here the high bytes carry literals too.  Behind the step to the high plane stand k
    times 128 128 130 128 128 126 -- the high byte goes from 0x3c to 0x3e and back, and at distance 2 never two bytes in a row
    equal theirs -- then the run: a 128 that ends a run of two, its head, 8 matches of 258 (symbol 285 takes the chain's weight 8)
    and r 128s more.  128, 130 and 126 are the chain's three commonest values; the 4 w wanted bytes hold what is left of
    them and all of the others."""
    q = 8
    w = chain_weights(n_sym, [q])
    others = list(w[2:-3])
    others.remove(q)
    for k in range(1, w[-3]):
        for r in range(3):
            n = 1 + 6 * k + 258 * q + 2 + r
            top = n - (w[-2] - k) - (w[-3] - k) - sum(others) + 4 * k + 2 + r
            if n % 4 or top < w[-1]:
                continue
            for shift in range(64):
                values = [(131 + shift + j) % 256 for j in range(len(others))]
                freq = dict(zip(values, others[::-1]))
                freq.update({128: top - (4 * k + 2 + r), 130: w[-2] - k, 126: w[-3] - k})
                first = arrange(freq, 2, n_sym + shift, {-1: values[0], -2: values[0]})
                step = int(exr_tail(first)[n])
                if step in freq:
                    continue
                stream = np.concatenate([first, [step], np.tile([128, 128, 130, 128, 128, 126], k), np.full(258 * q + 2 + r, 128)])
                assert stream.size == 2 * n <= CHUNK
                return exr_case(stream, 1, n // 4, depth15=n_sym - 1)
    raise AssertionError("no width fits")


def limiter15(sink, n_sym):
    if sink == "exr":
        return limiter15_exr(n_sym) if n_sym < 20 else limiter15_exr_deep(n_sym)
    return limiter15_png(sink, n_sym)


def dyadic_lengths_7bit():
    """Code lengths for the byte values 0 .. 255 (0: unused), 78 of them used: 8 of length 5, 34 of 6, 21 of 7, 13 of 8, one of 9
    and one of 10 (the end-of-block symbol is the other 10).  A value of length l is given 2^(10 - l) bytes of the 1 023, so any
    Huffman coder finds these lengths.  The gaps are three of 3 zeros and five of 11 or more, no four equal lengths stand side
    by side, and the distance length behind the end-of-block symbol is the one single zero: the header's tokens are 34 sixes,
    21 sevens, 13 eights, 8 fives, 5 of symbol 18, 3 of symbol 17, 2 tens, a nine and a zero -- chain weights, depth 8."""
    common = arrange({5: 8, 6: 34, 7: 21}, 1, 7).tolist()       # no four equal lengths in a row
    common.insert(40, 8)                                        # the thirteenth 8
    low, high = common[:38], common[38:]
    blocks = [low[:10], [0] * 3, low[10:20], [0] * 3, low[20:29], [0] * 3, low[29:], [0] * 12, [8, 8, 9, 8], [0] * 11, [8, 8, 10, 8],
              [0] * 124, [8, 8, 8], [0] * 11, [8, 8, 8], [0] * 11, high]
    lens = [l for b in blocks for l in b]
    assert len(lens) == 256
    return lens


def dyadic_lengths_7bit_deeper():
    """The same with 128 values used -- 8 of length 5, 13 of 6, 34 of 7, 71 of 8, one of 9, one of 10 -- and symbol 16 in the
    header: three runs of 7, 7 and 5 eights are an 8 and a repeat each, so 55 eights are listed.  21 gaps of 3 zeros, 5 of 13.
    The tokens: 55 eights, 34 sevens, 21 of symbol 17, 13 sixes, 8 fives, 5 of symbol 18, 3 of symbol 16, 2 tens, a nine and
    the distance length's zero -- depth 9."""
    common = arrange({5: 8, 6: 13}, 1, 8).tolist()
    rest = arrange({7: 34, 8: 52}, 1, 9).tolist()
    rest.insert(30, 9)
    rest.insert(60, 10)
    blocks = [common, [8] * 7, [8] * 7, [8] * 5] + [rest[4 * k:4 * k + 4] for k in range(19)] + [rest[76 + 3 * k:79 + 3 * k] for k in range(4)]
    lens = []
    for k, b in enumerate(blocks):
        lens += b + ([] if k == len(blocks) - 1 else [0] * (13 if k % 5 == 4 else 3))
    assert len(lens) == 256
    return lens


def dyadic_case(sink, lens, deepest, **expect):
    """2^deepest - 1 bytes, every one a literal, the value v 2^(deepest - lens[v]) times: 3 rows of RGBA pixels or one row of grey
    samples, behind whichever of filters 0 and 1 the row heuristic then picks"""
    freq = dict((v, 1 << (deepest - l)) for v, l in enumerate(lens) if l)
    n = (1 << deepest) - 1
    assert sum(freq.values()) == n
    rows = 3 if sink == "png" else 1
    for f in (1, 0):
        case = png_case(sink, arrange(freq, 1, 77, dict((r * (n // rows), f) for r in range(rows))), rows, values=lens, **expect)
        if front_end(case) == case.streams:
            break
    return case


def short_header_lengths():
    """11 values of 6 bits, 105 of 7, one of 8 like the end-of-block symbol: of the code-length code's symbols only 16, 18, 0, 8,
    7 and 6 are used, the first eight in the header's order"""
    return [6] * 11 + [7] * 105 + [8] + [0] * 139


def run_lengths_a():
    """lengths of the byte values for the header-run stream: equal runs of 10, 9, 8, 7, 3, 6, 4 and 5 (5 and 6 bits, neighbours
    differ), zero runs of 2, 3, 10, 138, 40 and 11"""
    blocks = [[6] * 10, [0] * 2, [6] * 9, [0] * 3, [6] * 8, [0] * 10, [5] * 7, [0] * 138, [6] * 3, [0] * 40, [6] * 6, [5] * 4, [6] * 5, [0] * 11]
    return [l for b in blocks for l in b]


def run_lengths_b():
    """9 values of 6 bits, 50 of 7, a zero run of 139 (symbol 18 with 127, then a single zero), 58 of 7"""
    return [6] * 9 + [7] * 50 + [0] * 139 + [7] * 58


def header_runs(lens, required_tokens, required_runs):
    """A PNG row behind filter 1 for 256 byte-value lengths of 5 .. 7 bits: a value of length l stands 2^(8 - l) times among 252
    literals, the last of them heads a run of 522 bytes -- two matches of 258 (symbol 285, 7 bits) and one of 5 (symbol 259,
    8 bits, like the end-of-block symbol).  The frequencies are powers of two that sum to 256, so the lengths are fixed."""
    assert len(lens) == 256
    freq = dict((v, 1 << (8 - l)) for v, l in enumerate(lens) if l)
    assert sum(freq.values()) == 252
    lit = arrange(freq, 1, 5, {0: 1, -1: 3, -2: 5})
    stream = np.concatenate([lit, np.full(521, 3, dtype=np.uint8)])
    want = list(lens) + [8, 0, 0, 8] + [0] * 25 + [7, 1]
    return png_case("png", stream, lengths=want, tokens=required_tokens, runs=required_runs, hlit=286, dist_used=True)


def no_match(sink):
    """compressible without a single match: two values in turn at distance 1, three at distance 2 (deltas -2, 0, +2 from a first
    byte of 130: low and high bytes stay on 128 and 130)"""
    if sink == "exr":
        return exr_case(np.tile([130, 126, 128], 8 * 96 // 3), 1, 96, hlit=257, dist_used=False)
    bpp = 4 if sink == "png" else 2
    return png_case(sink, np.concatenate([[1], np.tile([0, 2], 64 * bpp // 2)]), hlit=257, dist_used=False)


def long_run(sink):
    """a run of 300 bytes -- symbol 285 -- among bytes that repeat with period 3"""
    if sink == "exr":
        return exr_case(exr_tail(np.tile([131, 126, 127], 100)), 1, 75, hlit=286, dist_used=True)
    bpp = 4 if sink == "png" else 2
    stream = np.concatenate([[1], np.tile([3, 5, 9], 40), np.full(300, 7), np.tile([3, 5, 9], 20)])[:1 + 480]
    assert (stream.size - 1) % bpp == 0
    return png_case(sink, stream, hlit=286, dist_used=True)


def one_value(sink):
    """Nothing but one value: a literal, two matches of 258 and the end-of-block symbol (PNG: 517 zeros behind filter 0); the
    all-zero half block of 520 bytes is a 0, three 128s and the two matches."""
    if sink == "exr":
        return Case("exr", np.zeros((1, 65, 4)), [np.concatenate([[0], np.full(519, 128)])], hlit=286, dist_used=True, used=4)
    bpp = 4 if sink == "png" else 2
    return png_case(sink, np.zeros(1 + 516, dtype=np.uint8), hlit=286, dist_used=True, used=3)


def literals_then_run(n_literals, n, seed, dist, run_value):
    """n_literals bytes of a skewed alphabet of small values, none equal to either of the two before it, then `run_value`"""
    rng = np.random.default_rng(seed)
    values = np.array([v for v in SMALL[3:] if v != run_value])
    p = 0.75 ** np.arange(values.size)
    draw = values[rng.choice(values.size, size=3 * n_literals, p=p / p.sum())]
    out = []
    for v in draw:
        if len(out) == n_literals:
            break
        if v not in out[-2:]:
            out.append(int(v))
    assert len(out) == n_literals
    return np.concatenate([out, np.full(n - n_literals, run_value)]).astype(np.uint8)


SWEEP = 32


def residue_variant(sink, k):
    """Two chunks.  Chunk 0: 600 + k literals (the first 600 the same in every variant, so each step adds one code) and a run to
    its end and beyond."""
    if sink == "exr":
        return exr_case(exr_tail(literals_then_run(600 + k, 16448, 11, 2, 127)), 16, 257, chunks=2)
    bpp = 4 if sink == "png" else 2
    body = literals_then_run(600 + k, CHUNK, 11, 1, 1)
    return png_case(sink, np.concatenate([[1], body]), chunks=2)


def short_tail(sink, tail, crossing):
    """A last chunk of `tail` bytes behind full ones, and a run of 300 bytes in front of the last boundary that goes on to the
    stream's end (crossing) or stops at the boundary."""
    if sink == "exr":
        first = literals_then_run(3000, 16388, 13, 2, 127)
        stream = exr_tail(first)
        if not crossing:
            stream[CHUNK] = 129          # the high bytes step from 0x3c to 0x3d at the boundary
        return exr_case(stream, 1, 4097, chunks=2, tail=8)
    bpp = 4 if sink == "png" else 2
    width, rows = {(4, 1): (8192, 1), (4, 2): (4096, 2), (4, 3): (8192, 3), (2, 1): (16384, 1), (2, 2): (8192, 2), (2, 3): (16385, 1)}[(bpp, tail)]
    n = rows * (1 + bpp * width)
    rng = np.random.default_rng(100 * tail + bpp)
    stream = np.array(SMALL[:7], dtype=np.uint8)[rng.choice(7, size=n, p=[0.4, 0.2, 0.2, 0.05, 0.05, 0.05, 0.05])]
    edge = n - tail
    stream[edge - 300:] = 9
    if not crossing:
        stream[edge:] = [2, 4, 6][:tail]
    stream[::1 + bpp * width] = 1
    return png_case(sink, stream, rows, chunks=n // CHUNK + 1, tail=tail)


def high_sums(sink):
    """at least three chunks of bytes of 200 and more: each chunk's sums pass 65521 hundreds of times"""
    rng = np.random.default_rng(200)
    if sink == "png":
        stream = rng.integers(224, 256, 1 + 4 * 24577).astype(np.uint8)
        stream[0] = 1
        return png_case("png", stream, chunks=4, mean=200)
    n = 8 * 16 * 513
    stream, t = rng.integers(200, 256, n), 0
    for i in range(n):
        t = (t + stream[i] - (128 if i else 0)) % 256
        if i >= n // 2 and (t & 0x7c) == 0x7c:      # the high byte of a NaN or an infinity: step 8 less (or more)
            step = -8 if stream[i] >= 208 else 8
            stream[i] += step
            t = (t + step) % 256
    return exr_case(stream, 16, 513, chunks=3, mean=200)


STARRED = ("png", "png16", "exr")
BUILDERS = {}
for _sink in STARRED:
    for _n in (17, 18, 20):
        BUILDERS["limiter15_depth%d-%s" % (_n - 1, _sink)] = functools.partial(limiter15, _sink, _n)
    BUILDERS["no_match-" + _sink] = functools.partial(no_match, _sink)
    BUILDERS["long_run-" + _sink] = functools.partial(long_run, _sink)
    BUILDERS["one_value-" + _sink] = functools.partial(one_value, _sink)
    for _tail in (1, 2, 3) if _sink != "exr" else (8,):
        for _crossing in (True, False):
            BUILDERS["tail%d_%s-%s" % (_tail, "crossing" if _crossing else "exact", _sink)] = functools.partial(short_tail, _sink, _tail, _crossing)
for _sink in ("png", "png16"):
    BUILDERS["limiter7_depth8-" + _sink] = functools.partial(dyadic_case, _sink, dyadic_lengths_7bit(), 10, depth7=8)
    BUILDERS["limiter7_depth9-" + _sink] = functools.partial(dyadic_case, _sink, dyadic_lengths_7bit_deeper(), 10, depth7=9)
    BUILDERS["short_header-" + _sink] = functools.partial(dyadic_case, _sink, short_header_lengths(), 8, hclen=8, hlit=257, dist_used=False)
BUILDERS["header_runs_a-png"] = functools.partial(
    header_runs, run_lengths_a(), [(16, 0), (16, 1), (16, 2), (16, 3), (17, 0), (17, 7), (18, 0), (18, 127)],
    [(True, 2), (True, 3), (True, 10), (True, 11), (True, 138)] + [(False, n) for n in (3, 4, 5, 6, 7, 8, 9, 10)])
BUILDERS["header_runs_b-png"] = functools.partial(header_runs, run_lengths_b(), [(18, 127), (0, 0), (16, 3)], [(True, 139), (True, 2)])
BUILDERS["high_sums-png"] = functools.partial(high_sums, "png")
BUILDERS["high_sums-exr"] = functools.partial(high_sums, "exr")
CASES = sorted(BUILDERS)


@functools.lru_cache(maxsize=None)
def case_of(name):
    return BUILDERS[name]()


# ---------------------------------------------------------------- CPU: the reader

ZLIB_SETTINGS = [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
                 (6, zlib.Z_RLE), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_FIXED)]


@pytest.mark.parametrize("kind", ["zero", "gradient", "noise", "noise_row", "runs"])
def test_the_block_reader_inflates_what_zlib_inflates(kind):
    """Raw deflate streams zlib makes of the five synthetic kinds at levels 0, 1, 6 and 9, with Z_RLE, Z_HUFFMAN_ONLY and Z_FIXED,
    and with a sync flush in the middle: the reader's bytes are zlib.decompress's, its blocks tile the stream, their bytes add
    up, and the flush is the empty stored block it looks for behind the device's non-final chunks."""
    data = p8.filter_rows(p8.synthetic(kind, 264, 7))[1].tobytes()
    seen = set()
    for level, strategy in ZLIB_SETTINGS:
        for flush_at in (None, len(data) // 2):
            c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
            if flush_at is None:
                z = c.compress(data) + c.flush()
            else:
                z = c.compress(data[:flush_at]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(data[flush_at:]) + c.flush()
            blocks, out, end = inflate_blocks(z)
            assert out == zlib.decompress(z, -15) == data
            assert (end + 7) // 8 == len(z) and b"".join(b.data for b in blocks) == data
            assert blocks[0].start == 0 and all(a.end == b.start for a, b in zip(blocks, blocks[1:]))
            assert [b.final for b in blocks] == [False] * (len(blocks) - 1) + [True]
            for b in blocks:
                seen.add(b.kind)
                if b.kind:
                    assert b.hist[256] == 1 and b.hist[:256].sum() <= len(b.data)
                if b.kind == 2:
                    assert len(b.ll_lens) == b.hlit and len(b.d_lens) == b.hdist and len(b.cl_lens) == 19
                    listed = b.ll_lens + b.d_lens
                    again = []
                    for sym, extra in b.tokens:
                        again += [sym] if sym < 16 else [again[-1]] * (3 + extra) if sym == 16 else [0] * ((3 if sym == 17 else 11) + extra)
                    assert again == listed
            if flush_at is not None:
                empty = [k for k, b in enumerate(blocks) if b.kind == 0 and not b.data and not b.final]
                assert empty and all(blocks[k].end % 8 == 0 for k in empty)
                assert len(b"".join(b.data for b in blocks[:empty[0]])) == flush_at
            if strategy == zlib.Z_FIXED:
                assert all(b.kind != 2 for b in blocks)              # fixed codes, or stored where that is shorter
            if level == 0:
                assert all(b.kind == 0 for b in blocks if b.data)
    assert seen == {0, 1, 2} or kind in ("zero", "noise")


def test_the_models_of_the_preconditions_on_known_answers():
    assert [length_symbol(n) for n in (3, 10, 11, 12, 13, 257, 258)] == [257, 264, 265, 265, 266, 284, 285]
    # a run of 1 + 258 + 258 + 2 bytes at distance 1: a literal, two matches, two literals; the same bytes at distance 2
    hist, matches = model_hist(bytes([5]) * 519 + bytes([6, 6, 6, 6]), 1)
    assert (hist[5], hist[6], hist[285], hist[257], hist[256], matches) == (3, 1, 2, 1, 1, 3)
    hist, matches = model_hist(bytes([1, 2] * 4), 2)
    assert (hist[1], hist[2], hist[260], matches) == (1, 1, 1, 1)
    assert model_hist(bytes([1, 1, 1, 2, 2, 2, 3]), 1)[1] == 0          # runs of up to 3 are literals
    # Fibonacci weights chain; with a third 1 the ties break the chain
    assert unlimited_depth([1, 1, 2, 3, 5, 8, 13, 21]) == 7 and unlimited_depth([1, 1, 1, 2, 3, 5, 8, 13]) < 7
    assert chain_weights(9) == [1, 1, 2, 3, 5, 8, 13, 21, 34] and unlimited_depth(chain_weights(9, [16])) == 8
    assert huffman_lengths([4, 2, 1, 1, 0]) == [1, 2, 3, 3, 0]
    assert header_tokens([0] * 139 + [7] * 10 + [0, 0] + [3] * 4) == [(18, 127), (0, 0), (7, 0), (16, 3), (16, 0), (0, 0), (0, 0), (3, 0), (16, 0)]
    assert runs_of([0, 0, 5, 5, 5, 0]) == {(True, 2), (False, 3), (True, 1)}


# ---------------------------------------------------------------- CPU: every builder's precondition

def check_preconditions(case):
    """the models of the front end give the wanted streams back, and the streams have what the case is named for"""
    got = front_end(case)
    assert [len(s) for s in got] == [len(s) for s in case.streams]
    assert got == case.streams, "the front end's model makes other bytes of the image"
    e = case.expect
    first = chunks_of(case.streams[0])[0]
    hist, matches = model_hist(first, case.dist)
    if "depth15" in e:
        assert matches == (0 if case.dist == 1 else hist[285]) and unlimited_depth(hist) == e["depth15"] > 15
        assert len(first) == len(case.streams[0])               # one chunk
    if "depth7" in e:
        assert matches == 0
        hlit, listed, tokens = model_header(first, case.dist)
        assert hlit == 257 and listed[256:] == [10, 0]
        assert unlimited_depth(token_hist(tokens)) == e["depth7"] > 7
    if "values" in e:
        assert model_header(first, case.dist)[1][:256] == e["values"]
    if "hclen" in e:
        used = token_hist(model_header(first, case.dist)[2])
        assert max(k for k in range(19) if used[CL_ORDER[k]]) + 1 == e["hclen"]
    if "lengths" in e:
        hlit, listed, tokens = model_header(first, case.dist)
        assert hlit == e["hlit"] and listed == e["lengths"]
        assert set(e["tokens"]) <= set(tokens) and set(e["runs"]) <= runs_of(listed)
    if "hlit" in e:
        assert max(s for s in range(286) if hist[s]) + 1 == e["hlit"] and (matches > 0) == e["dist_used"]
    if "used" in e:
        assert int((hist > 0).sum()) == e["used"]
    if "chunks" in e:
        assert [len(chunks_of(s)) for s in case.streams] == [e["chunks"]]
    if "tail" in e:
        assert len(case.streams[0]) % CHUNK == e["tail"]
    if "mean" in e:
        for c in chunks_of(case.streams[0]):
            assert np.frombuffer(c, dtype=np.uint8).mean() >= e["mean"]
        assert len(chunks_of(case.streams[0])) >= 3


@pytest.mark.parametrize("name", CASES)
def test_the_image_gives_the_wanted_stream_and_the_stream_its_edge(name):
    check_preconditions(case_of(name))


@pytest.mark.parametrize("sink", STARRED)
def test_the_sweep_gives_the_wanted_streams(sink):
    for k in range(SWEEP):
        check_preconditions(residue_variant(sink, k))


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    ctx = nh.NdtHip(0)
    yield ctx
    ctx.close()


def encode(gpu, case):
    """(the file, the raw deflate stream of each of its zlib streams, chunks by the stats or None, the Z_RLE model's size)"""
    if case.sink == "exr":
        data = gpu.encode_exr(case.image, None, "half")
        sizes, raw_flags = ex.assert_decodes_to(data, case.image, None, ex.HALF)          # the model's sample bits
        assert not any(raw_flags), "a block fell back to raw bytes: there is no deflate to look at"
        rows, width = case.image.shape[:2]
        at = len(ex.model_header(width, rows, ex.HALF, False))
        offsets = struct.unpack("<%dQ" % len(sizes), data[at:at + 8 * len(sizes)])
        zstreams = [data[o + 8:o + 8 + n] for o, n in zip(offsets, sizes)]
        model = 0
        for s in case.streams:
            model += 6
            for c in chunks_of(s):
                z = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
                model += len(z.compress(c) + z.flush(zlib.Z_SYNC_FLUSH))
        return data, zstreams, None, model
    if case.sink == "png":
        data = gpu.encode_png(case.image)
        pixels, filters, idat = p8.read_png(data)
        want_filters, model = p8.filter_rows(case.image)[0], p8.model_sizes(case.image)[1]
    else:
        data = gpu.encode_png16(case.image)
        pixels, filters, idat = p16.read_png16(data, 1)
        want_filters, model = p16.filter_rows(case.image)[0], p16.model_sizes(case.image)[1]
    assert np.array_equal(pixels, case.image) and np.array_equal(filters, want_filters)
    assert gpu.png_stats.idat_bytes == len(idat)
    return data, [idat], gpu.png_stats.chunks, model


def monotone(hist, lens):
    """of two used symbols the more frequent one has no longer a code"""
    used = sorted((-int(f), l) for f, l in zip(hist, lens) if f)
    longest = 0
    for k, (f, l) in enumerate(used):
        if k and f != used[k - 1][0]:
            longest = max(x for y, x in used[:k])
        if l < longest:
            return False
    return True


def check_stream(z, want, dist):
    """Assertions 2, 3, 4, 6 and 7 on one zlib stream of a file; returns [(the chunk's block, its bytes in the file)]."""
    assert z[0] & 15 == 8 and ((z[0] << 8) | z[1]) % 31 == 0
    blocks, out, end = inflate_blocks(z[2:])
    assert out == want, "the block reader's bytes are not the model's stream"
    assert (end + 7) // 8 == len(z) - 6 and struct.unpack(">I", z[-4:])[0] == zlib.adler32(want)
    assert [b.final for b in blocks] == [False] * (len(blocks) - 1) + [True]
    chunks, k = [], 0
    while k < len(blocks):
        b = blocks[k]
        assert b.start % 8 == 0 and b.kind in (0, 2) and len(b.data) > 0
        stop = b.end
        if b.kind == 2 and not b.final:
            sync = blocks[k + 1]
            assert sync.kind == 0 and not sync.data and not sync.final and sync.end % 8 == 0
            stop = sync.end
            k += 1
        assert stop % 8 == 0 or b.final
        chunks.append((b, (stop + 7) // 8 - b.start // 8))
        k += 1
    assert [len(b.data) for b, _ in chunks] == [len(c) for c in chunks_of(want)]
    for b, size in chunks:
        if b.kind == 0:
            assert size == 5 + len(b.data)
            continue
        assert size < 5 + len(b.data), "a dynamic block of %d bytes for %d" % (size, len(b.data))
        assert max(b.ll_lens) <= 15 and max(b.cl_lens) <= 7
        assert sum(1 << (15 - l) for l in b.ll_lens if l) == 1 << 15, "the literal / length code is not complete"
        assert sum(1 << (7 - l) for l in b.cl_lens if l) == 1 << 7, "the code-length code is not complete"
        assert b.hdist == dist and b.d_lens in ([0] * dist, [0] * (dist - 1) + [1])
        assert (b.d_lens[-1] == 1) == bool(b.hist[257:].sum())
        assert all((f > 0) <= (l > 0) for f, l in zip(b.hist, b.ll_lens))
        assert monotone(b.hist, b.ll_lens), "a more frequent literal / length symbol has the longer code"
        assert monotone(token_hist(b.tokens), b.cl_lens), "a more frequent code-length symbol has the longer code"
    return chunks


def describe(name, case, data, chunks, model):
    for b, size in chunks:
        if b.kind == 2:
            print("%s: chunk of %d bytes in %d: HLIT %d HDIST %d HCLEN %d, longest literal/length code %d, longest code-length code %d, "
                  "%d symbols used, ends on bit %d" % (name, len(b.data), size, b.hlit, b.hdist, b.hclen, max(b.ll_lens), max(b.cl_lens),
                                                       int((b.hist > 0).sum()), b.end % 8))
        else:
            print("%s: chunk of %d bytes stored" % (name, len(b.data)))
    streams = sum(len(s) for s in case.streams)
    print("%s: stream %d bytes, file %d bytes, deflate %d bytes against %d of the Z_RLE model" % (
        name, streams, len(data), sum(s for _, s in chunks) + 6 * len(case.streams), model))


def run_case(gpu, name, case):
    data, zstreams, stat_chunks, model = encode(gpu, case)                 # assertion 1 inside
    assert len(zstreams) == len(case.streams)
    chunks = []
    for z, want in zip(zstreams, case.streams):
        chunks += check_stream(z, want, case.dist)
    if stat_chunks is not None:
        assert stat_chunks == len(chunks)
    describe(name, case, data, chunks, model)
    assert encode(gpu, case)[0] == data                                     # the same input, the same bytes
    return chunks


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_the_device_file_at_the_edge(gpu, name):
    """Assertions for every case, all from the file the device wrote: the sink's reader gives the image back, the block reader
    the model stream; a chunk is one dynamic or one stored block, on a byte boundary, a non-final dynamic one followed by an empty
    stored block, BFINAL on the last block alone, as many chunks as the stats say; both codes of a dynamic block complete (Kraft
    sum exactly 1) within 15 and 7 bits, the distance code empty or one length 1 in the last of DIST entries; lengths monotone in
    frequency in both alphabets; a dynamic chunk shorter than its stored form; two encodes the same bytes.  Then the proof that
    the edge the case is named for was reached."""
    case = case_of(name)
    e = case.expect
    chunks = run_case(gpu, name, case)
    first = chunks[0][0]
    if "depth15" in e:
        assert first.kind == 2 and max(first.ll_lens) == 15 and unlimited_depth(first.hist) == e["depth15"] > 15
        assert first.hclen == 19
    if "depth7" in e:
        assert first.kind == 2 and max(first.cl_lens) == 7 and unlimited_depth(token_hist(first.tokens)) == e["depth7"] > 7
    if "values" in e:
        assert first.kind == 2 and first.ll_lens[:256] == e["values"]
    if "hclen" in e:
        assert first.hclen == e["hclen"]
    if "lengths" in e:
        assert first.kind == 2 and first.ll_lens + first.d_lens == e["lengths"]
        assert set(e["tokens"]) <= set(first.tokens) and set(e["runs"]) <= runs_of(first.ll_lens + first.d_lens)
    if "hlit" in e:
        assert first.kind == 2 and first.hlit == e["hlit"] and first.hdist == case.dist and (first.d_lens[-1] == 1) == e["dist_used"]
    if "used" in e:
        assert int((first.hist > 0).sum()) == e["used"]
    if "chunks" in e:
        assert len(chunks) == e["chunks"]
    if "tail" in e:
        assert len(chunks[-1][0].data) == e["tail"]
    if "mean" in e:
        assert all(b.kind == 2 for b, _ in chunks[:-1])


@pytest.mark.gpu
@pytest.mark.parametrize("sink", STARRED)
def test_non_final_chunks_end_on_every_bit_of_a_byte(gpu, sink):
    """32 variants of a two-chunk stream, one literal more in chunk 0 each: every file decodes, and over the sweep the dynamic
    block of chunk 0 ends on all eight residues, so the empty stored block has stood behind each."""
    seen = {}
    for k in range(SWEEP):
        case = residue_variant(sink, k)
        data, zstreams, stat_chunks, _ = encode(gpu, case)
        chunks = check_stream(zstreams[0], case.streams[0], case.dist)
        assert len(chunks) == 2 and stat_chunks in (None, 2) and chunks[0][0].kind == 2
        seen[k] = chunks[0][0].end % 8
    print("%s: chunk 0 ends on bit %s" % (sink, " ".join("%d" % seen[k] for k in range(SWEEP))))
    assert set(seen.values()) == set(range(8))
