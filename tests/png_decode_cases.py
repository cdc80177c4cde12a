"""The pictures, zlib streams and PNG files of the PNG decoder's tests (test_png_decode_cpu.py: csrc/png_inflate.h on the CPU under the
sanitizers; test_png_decode_gpu.py: the same text on the device), written with zlib and struct alone.

A case is (name, H, W, C, stream, want): want is the bytes H rows of 1 + W C that the stream has to inflate to, or None for a stream
that has to be refused.  zlib.decompress is the judge of which is which: it returns `want` for the former and, except where the case
says otherwise (a picture one row short or long, a filter byte of 5: streams that are fine and pictures that are not), raises for
the latter."""
import collections
import functools
import struct
import zlib

import numpy as np

SIG = b'\x89PNG\r\n\x1a\n'
COLOUR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}
SHAPES = [(1, 1), (1, 70), (70, 1), (5, 3), (33, 7), (63, 67), (64, 67), (65, 67), (129, 67), (9, 63), (9, 64), (9, 65)]      # H x W
FILTER_MODES = (0, 1, 2, 3, 4, 'mix', 'min')
BIG = (130, 130, 4)          # 67,730 raw bytes: more than one stored block, more than 32 KiB
HAND = (200, 200, 1)         # the hand-assembled streams' picture: 40,200 raw bytes


def pixels(H, W, C, seed):
    """uint8 [H, W, C]: seeded noise in the first half of the bytes, a smooth ramp in the second"""
    n = H * W * C
    flat = np.arange(n)
    noise = np.random.default_rng(seed).integers(0, 256, n)
    return np.where(flat < n // 2, noise, (flat // max(1, C)) * 3 // 2 % 256).astype(np.uint8).reshape(H, W, C)


def residuals(img):
    """[5, H, W C] uint8: every row under every filter type, the PNG specification's arithmetic"""
    H, W, C = img.shape
    x = img.reshape(H, W * C).astype(np.int32)
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, C:] = x[:, :-C]
    b[1:] = x[:-1]
    c[1:, C:] = x[:-1, :-C]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]).astype(np.uint8)


def row_choice(img, mode, seed=0):
    H = img.shape[0]
    if mode == 'mix':
        return np.random.default_rng(1000 + seed).integers(0, 5, H)
    if mode == 'min':
        return np.argmin(np.abs(residuals(img).astype(np.int8).astype(np.int64)).sum(-1), 0)
    return np.full(H, int(mode))


def filtered(img, mode, seed=0):
    """the bytes a PNG compresses: H rows of filter type, residuals"""
    H = img.shape[0]
    choice = row_choice(img, mode, seed)
    rows = residuals(img)[choice, np.arange(H)]
    return np.concatenate([choice.astype(np.uint8)[:, None], rows], 1).tobytes()


def chunk(tag, body):
    return struct.pack('>I', len(body)) + tag + body + struct.pack('>I', zlib.crc32(tag + body) & 0xffffffff)


def png_file(H, W, C, stream, idat_bytes=None, before=(), depth=8, colour=None, interlace=0):
    """a PNG file around a zlib stream; idat_bytes cuts the stream into IDAT chunks of that size; `before`: chunks in front of them"""
    out = SIG + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, depth, COLOUR_TYPE[C] if colour is None else colour, 0, 0, interlace))
    for tag, body in before:
        out += chunk(tag, body)
    step = idat_bytes or max(1, len(stream))
    for i in range(0, max(1, len(stream)), step):
        out += chunk(b'IDAT', stream[i:i + step])
    return out + chunk(b'IEND', b'')


def compress(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush=None, every=1000):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    if flush is None:
        return co.compress(raw) + co.flush()
    out = b''
    for i in range(0, len(raw), every):
        out += co.compress(raw[i:i + every]) + co.flush(flush)
    return out + co.flush()


# ---- a deflate bit writer: fixed-Huffman blocks, and dynamic blocks from given code lengths ----
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30


def canonical(lens):
    """{symbol: (code, bits)} of RFC 1951 3.2.2"""
    code, out = 0, {}
    for bits in range(1, 16):
        for s, l in enumerate(lens):
            if l == bits:
                out[s] = (code, bits)
                code += 1
        code <<= 1
    return out


class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):                 # n bits, lowest first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):                   # a Huffman code: highest bit first
        v, n = c
        self.put(int(format(v, f'0{n}b')[::-1], 2), n)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b'')


def spelled(s):
    """a match as (length symbol, extra value, distance symbol, extra value), the symbols counted from 0: a (length, distance) pair
    gets the last symbol whose base is not above it; one that is spelled out already (227 + 31 for a length of 258) stays"""
    if len(s) == 4:
        return s
    length, dist = s
    i = max(k for k in range(29) if LEN_BASE[k] <= length) if length < 258 else 28
    j = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, length - LEN_BASE[i], j, dist - DIST_BASE[j]


def pair(s):
    """(length, distance) of a match in either spelling"""
    return s if len(s) == 2 else (LEN_BASE[s[0]] + s[1], DIST_BASE[s[2]] + s[3])


def put_symbols(bw, ll, dd, symbols):
    """symbols: ints (literals) and matches ((length, distance), or spelled()'s four); then end of block"""
    for s in symbols:
        if isinstance(s, tuple):
            i, le, j, de = spelled(s)
            bw.code(ll[257 + i])
            bw.put(le, LEN_EXTRA[i])
            bw.code(dd[j])
            bw.put(de, DIST_EXTRA[j])
        else:
            bw.code(ll[s])
    bw.code(ll[256])


def fixed_stream(symbols):
    bw = Bits()
    bw.put(1, 1), bw.put(1, 2)
    put_symbols(bw, canonical(FIXED_LL), canonical(FIXED_D), symbols)
    return b'\x78\x9c' + bw.bytes()


def run_length(lens):
    """[(code-length symbol, extra value, extra bits, first index, count)]: the longest repeats, greedily, over the whole list"""
    out, i = [], 0
    while i < len(lens):
        v, n = lens[i], 1
        while i + n < len(lens) and lens[i + n] == v:
            n += 1
        if v == 0 and n >= 3:
            n = min(n, 138)
            out.append((17, n - 3, 3, i, n) if n <= 10 else (18, n - 11, 7, i, n))
        elif v and n >= 4:
            n = min(n - 1, 6)
            out += [(v, 0, 0, i, 1), (16, n - 3, 2, i + 1, n)]
            n += 1
        else:
            n = 1
            out.append((v, 0, 0, i, 1))
        i += n
    return out


CL_LENS = [4] * 13 + [5] * 6             # a complete code-length code: 13 / 16 + 6 / 32


def dynamic_header(bw, ll_lens, d_lens, final=1):
    """BFINAL, BTYPE = 2 and the code lengths; returns the run-length items (run_length's)"""
    bw.put(final, 1), bw.put(2, 2)
    bw.put(len(ll_lens) - 257, 5), bw.put(len(d_lens) - 1, 5), bw.put(19 - 4, 4)
    for s in CL_ORDER:
        bw.put(CL_LENS[s], 3)
    cl = canonical(CL_LENS)
    items = run_length(list(ll_lens) + list(d_lens))
    for s, extra, bits, _, _ in items:
        bw.code(cl[s])
        bw.put(extra, bits)
    return items


def dynamic_stream(ll_lens, d_lens, symbols):
    bw = Bits()
    items = dynamic_header(bw, ll_lens, d_lens)
    put_symbols(bw, canonical(ll_lens), canonical(d_lens), symbols)
    return b'\x78\x9c' + bw.bytes(), items


def with_adler(body, raw):
    return body + struct.pack('>I', zlib.adler32(raw) & 0xffffffff)


def expand(symbols, before=b''):
    """the bytes of the symbols; `before`: the output in front of them, which their matches may reach into"""
    out = bytearray(before)
    for s in symbols:
        if isinstance(s, tuple):
            length, dist = pair(s)
            assert 1 <= dist <= len(out)
            for _ in range(length):
                out.append(out[-dist])
        else:
            out.append(s)
    return bytes(out)


def hand_streams():
    """{name: (stream, raw, note)} for the HAND picture; every byte is a valid filter type, so any row start may fall anywhere"""
    H, W, C = HAND
    n = H * (W * C + 1)
    lit = np.random.default_rng(77).integers(0, 5, n).tolist()
    out = {}
    for name, head, match in (('len258-dist32768', 32768, (258, 32768)), ('len258-dist1', 1, (258, 1)), ('len3-dist2', 2, (3, 2))):
        symbols = lit[:head] + [match] + lit[:n - head - match[0]]
        raw = expand(symbols)
        out[name] = (with_adler(fixed_stream(symbols), raw), raw, None)
    rng = np.random.default_rng(78)
    # literals 0 .. 2, end of block and length 3; 262 literal / length lengths whose last four are 0, then the distance lengths 0 0 0 1 1:
    # one run of seven zeros that starts among the former and ends among the latter
    ll = [2, 2, 2] + [0] * 253 + [3, 3] + [0] * 4
    dd = [0, 0, 0, 1, 1]
    symbols, size = [0, 1, 2, 1, 0, 2, 2, 1], 8
    while size < n:
        if n - size >= 3 and rng.random() < 0.5:
            symbols.append((3, int(rng.integers(4, 7))))
            size += 3
        else:
            symbols.append(int(rng.integers(0, 3)))
            size += 1
    raw = expand(symbols)
    body, items = dynamic_stream(ll, dd, symbols)
    crossing = [it for it in items if it[3] < len(ll) < it[3] + it[4]]
    out['dynamic-crossing-run'] = (with_adler(body, raw), raw, crossing)
    # a single distance code, of one bit: distance 1 alone (an incomplete code, and the one kind that is allowed)
    ll = [2, 2, 2] + [0] * 253 + [3, 3]
    symbols, size = [2, 0, 1], 3
    while size < n:
        if n - size >= 3 and rng.random() < 0.3:
            symbols.append((3, 1))
            size += 3
        else:
            symbols.append(int(rng.integers(0, 3)))
            size += 1
    raw = expand(symbols)
    body, _ = dynamic_stream(ll, [1], symbols)
    out['dynamic-one-distance'] = (with_adler(body, raw), raw, None)
    return out


def deflate_streams():
    """{name: stream} of the BIG picture's filtered bytes (min-sum rows) and the bytes themselves"""
    H, W, C = BIG
    raw = filtered(pixels(H, W, C, 5), 'min')
    out = {f'level{lv}': compress(raw, lv) for lv in (0, 1, 6, 9)}
    out.update(fixed=compress(raw, 6, zlib.Z_FIXED), huffman=compress(raw, 6, zlib.Z_HUFFMAN_ONLY), rle=compress(raw, 6, zlib.Z_RLE),
               wbits9=compress(raw, 6, wbits=9), fullflush=compress(raw, 6, flush=zlib.Z_FULL_FLUSH), syncflush=compress(raw, 6, flush=zlib.Z_SYNC_FLUSH))
    return out, raw


def broken_streams():
    """{name: (H, W, C, stream, zlib_accepts)}: each one has to be refused"""
    H, W, C = 33, 7, 4
    raw = filtered(pixels(H, W, C, 9), 'mix')
    good = compress(raw)
    rb = W * C + 1
    out = {}
    cuts = sorted(set(np.random.default_rng(3).choice(np.arange(2, len(good) - 1), 16, replace=False).tolist()))
    for k in cuts:
        out[f'cut-{k}'] = (H, W, C, good[:k], False)
    out['cut-header'] = (H, W, C, good[:1], False)
    out['adler'] = (H, W, C, good[:-1] + bytes([good[-1] ^ 1]), False)
    out['block-type-3'] = (H, W, C, b'\x78\x9c\x07' + good[3:], False)
    stored = b'\x78\x01\x01' + struct.pack('<HH', len(raw), (len(raw) ^ 0xffff) ^ 0x10) + raw
    out['stored-nlen'] = (H, W, C, with_adler(stored, raw), False)
    out['far-distance'] = (H, W, C, with_adler(fixed_stream([1, 2, (3, 3)] + [0] * (len(raw) - 5)), raw), False)
    for name, ll in (('oversubscribed', [1, 1, 1] + [0] * 253 + [2]), ('incomplete', [2, 2] + [0] * 254 + [3])):
        bw = Bits()
        dynamic_header(bw, ll, [1])
        out[name] = (H, W, C, b'\x78\x9c' + bw.bytes() + bytes(8), False)
    out['row-short'] = (H, W, C, compress(raw[:-rb]), True)
    out['row-long'] = (H, W, C, compress(raw + raw[-rb:]), True)
    five = bytearray(raw)
    five[2 * rb] = 5
    out['filter-5'] = (H, W, C, compress(bytes(five)), True)
    out['fdict'] = (H, W, C, bytes([0x78, 0xbb]) + good[2:], False)
    return out, good, raw


# ---- streams laid out on purpose: the long codes, the ring, the refill, the refusals.  What each group reaches is computed from its
# symbols by the *_coverage functions below, and the tests assert it, so that an edit of a case cannot empty it silently ----
PNG_LBITS, PNG_DBITS = 10, 9              # csrc/png_inflate.h's: the bits that index the two lookup tables; longer codes are walked
PNG_FLUSH = 16384                         # ... the waiting bytes at which the ring goes to memory
PNG_WIN = 65536                           # ... the ring
PNG_INW_BYTES = 8192                      # ... the bytes of the stream that are fetched at a time
CHAIN = list(range(1, 15)) + [15, 15]     # a complete code of 16 members with one of every length (zlib takes it for both alphabets)
RING = (400, 511, 1)                      # 204,800 filtered bytes: 3.125 rings
REFILL = (100, 199, 1)                    # 20,000 filtered bytes: in fixed-code literals, a stream of more than two fetches
SMALL = (3, 4, 1)                         # 15 filtered bytes: the picture of the refusals
STATUS_WORDS = ('OK', 'TRUNCATED', 'BAD_HEADER', 'BAD_BLOCK', 'BAD_STORED', 'OVERSUBSCRIBED', 'INCOMPLETE', 'BAD_LENGTHS', 'BAD_CODE',
                'FAR_DISTANCE', 'TOO_LONG', 'TOO_SHORT', 'BAD_FILTER', 'BAD_ADLER', 'BAD_OFFSETS')      # r2l_png_status, include/r2l_hip.h


def chain_lens(members):
    """the code lengths that give CHAIN to `members`, in that order, and 0 to every symbol between them"""
    lens = [0] * (max(members) + 1)
    for s, bits in zip(members, CHAIN):
        lens[s] = bits
    return lens


def blocks_stream(blocks):
    """a zlib stream without its Adler-32 of ('stored', bytes), ('fixed', symbols) and ('dynamic', ll_lens, d_lens, symbols) blocks"""
    bw = Bits()
    for k, blk in enumerate(blocks):
        final = int(k == len(blocks) - 1)
        if blk[0] == 'stored':
            bw.put(final, 1), bw.put(0, 2), bw.put(0, -bw.n % 8)
            bw.put(len(blk[1]), 16), bw.put(len(blk[1]) ^ 0xffff, 16)
            bw.out += blk[1]
        elif blk[0] == 'fixed':
            bw.put(final, 1), bw.put(1, 2)
            put_symbols(bw, canonical(FIXED_LL), canonical(FIXED_D), blk[1])
        else:
            dynamic_header(bw, blk[1], blk[2], final)
            put_symbols(bw, canonical(blk[1]), canonical(blk[2]), blk[3])
    return b'\x78\x9c' + bw.bytes()


def blocks_bytes(blocks):
    raw = b''
    for blk in blocks:
        raw = raw + blk[1] if blk[0] == 'stored' else expand(blk[-1], raw)
    return raw


# -- 1. codes longer than the lookup tables, and all 29 + 30 symbols with their extra bits all 0 and all 1 --
def long_code_blocks():
    """three dynamic blocks over the HAND picture.  Each one's literal / length code is CHAIN over the literals 0 .. 4, end of block
    and ten length symbols, and its distance code is CHAIN over sixteen distance symbols, in a seeded order; a block uses every member
    of both, the length and distance symbols once with their extra bits all 0 and once all 1."""
    H, W, C = HAND
    n = H * (W * C + 1)
    rng = np.random.default_rng(79)
    len_sets = [list(range(19, 29)), list(range(9, 19)), list(range(0, 9)) + [28]]
    dist_sets = [list(range(0, 16)), list(range(14, 30)), list(range(0, 30, 2)) + [29]]
    blocks, op = [], 0
    for b in range(3):
        members = [0, 1, 2, 3, 4, 256] + [257 + i for i in len_sets[b]]
        ll = chain_lens([members[k] for k in rng.permutation(16)])
        dd = chain_lens([dist_sets[b][k] for k in rng.permutation(16)])
        weight = np.array([2. ** -ll[v] for v in range(5)])
        draw = lambda count: rng.choice(5, count, p=weight / weight.sum()).tolist()
        symbols = [0, 1, 2, 3, 4]
        op += 5
        len_uses = [(i, e) for i in len_sets[b] for e in (0, (1 << LEN_EXTRA[i]) - 1)]
        dist_uses = sorted(((j, e) for j in dist_sets[b] for e in (0, (1 << DIST_EXTRA[j]) - 1)), key=lambda u: DIST_BASE[u[0]] + u[1])
        order = rng.permutation(len(len_uses)).tolist()
        for k, (j, de) in enumerate(dist_uses):
            i, le = len_uses[order[k % len(order)]]
            dist = DIST_BASE[j] + de
            some = draw(max(dist - op, int(rng.integers(1, 4))))          # literals up to where the distance lies inside the output
            symbols += some + [(i, le, j, de)]
            op += len(some) + LEN_BASE[i] + le
        if b == 2:
            assert op <= n
            symbols += draw(n - op)
        blocks.append(('dynamic', ll, dd, symbols))
    return blocks


def code_coverage(blocks):
    """of the dynamic blocks: (bits of the literal / length codes they use, bits of the distance codes, how often they use each (length
    symbol, extra value), each (distance symbol, extra value))"""
    ll_bits, d_bits, len_uses, dist_uses = set(), set(), collections.Counter(), collections.Counter()
    for blk in blocks:
        if blk[0] != 'dynamic':
            continue
        _, ll, dd, symbols = blk
        ll_bits.add(ll[256])
        for s in symbols:
            if isinstance(s, tuple):
                i, le, j, de = spelled(s)
                ll_bits.add(ll[257 + i]), d_bits.add(dd[j])
                len_uses[(i, le)] += 1
                dist_uses[(j, de)] += 1
            else:
                ll_bits.add(ll[s])
    assert 0 not in ll_bits and 0 not in d_bits
    return ll_bits, d_bits, len_uses, dist_uses


# -- 2. the ring, several times round --
class Layout:
    """symbols placed by output position, with the decoder's flush rule mirrored (flush_sizes)"""

    def __init__(self, op, seed, dists, any_length=True):
        self.symbols, self.op, self.start = [], op, op
        self.rng, self.dists, self.turn, self.any_length = np.random.default_rng(seed), dists, 0, any_length

    def waiting(self):
        sizes = flush_sizes(self.symbols, self.start)
        return self.op - self.start - sum(sizes)

    def lit(self, count=1):
        self.symbols += self.rng.integers(0, 5, count).tolist()
        self.op += count

    def match(self, length, dist):
        assert 1 <= dist <= self.op and 3 <= length <= 258
        self.symbols.append((length, dist))
        self.op += length

    def fill(self, to):
        """up to position `to`: matches of 258 at the distances in turn with two literals behind each, then a shorter match, then literals"""
        assert to >= self.op
        while self.op < to:
            room = to - self.op
            dist = self.dists[self.turn % len(self.dists)]
            self.turn += 1
            if dist > self.op:
                self.lit()
            elif room >= 260:
                self.match(258, dist), self.lit(2)
            elif room in (3, 258) or (3 < room < 258 and self.any_length):
                self.match(room, dist)
            elif room >= 6:
                self.match(3, dist)
            else:
                self.lit()

    def fill_waiting(self, want):
        """up to where `want` bytes wait for the next flush"""
        w = self.waiting()
        if w > want:
            self.fill(self.op + PNG_FLUSH - w)
            self.match(3, 300)
            w = self.waiting()
            assert w <= 258 + 3
        self.fill(self.op + want - w)
        assert self.waiting() == want


def flush_sizes(symbols, start=0):
    """the bytes of each flush of the ring while these symbols are decoded, without the last one at the end of the stream.
    png_inflate's rule: the ring is flushed when PNG_FLUSH or more bytes wait after a symbol that went down its general path.  Every
    match does; a literal whose code the lookup table holds goes down the literal loop instead, which stops where PNG_FLUSH bytes wait
    and does not flush, so that literal is flushed together with the symbol behind it."""
    return [size for size, _ in flushes(symbols, start)]


def flushes(symbols, start=0):
    """flush_sizes' flushes as (bytes, the symbol that brought the flush about)"""
    out, op, flushed = [], start, start
    for s in symbols:
        general = isinstance(s, tuple) or op - flushed >= PNG_FLUSH
        op += pair(s)[0] if isinstance(s, tuple) else 1
        if general and op - flushed >= PNG_FLUSH:
            out.append((op - flushed, s))
            flushed = op
    return out


RING_MARKS = (PNG_WIN, 2 * PNG_WIN, 3 * PNG_WIN)
RING_CLASSES = ('one', 'overlap', '32768', '32767')


def distance_class(length, dist):
    return 'one' if dist == 1 else 'overlap' if dist < length else str(dist) if dist in (32768, 32767) else 'other'


def ring_symbols(variant):
    """one fixed block over the RING picture.  At every multiple of the ring's size: variant 0 a match of 3 that ends on it and one of
    258 that starts on it, variant 1 the two lengths exchanged, variants 2 and 3 a match of 3 / 258 that lies across it; behind it
    matches of 3 and 258 whose SOURCE lies across it, near and (the first two multiples: the picture ends 8192 bytes behind the third)
    at distance 32768 / 32767.  In between, matches of 258 at distance 32768 where exactly PNG_FLUSH, PNG_FLUSH + 257 and
    PNG_FLUSH + 258 bytes come to wait."""
    H, W, C = RING
    n = H * (W * C + 1)
    lay = Layout(0, 80 + variant, (32768, 300, 32767, 4097, 259, 1000))
    lay.lit(700)
    turn = variant

    def dist_for(length):
        nonlocal turn
        turn += 1
        return (1, 2 if length == 3 else 100, 32768, 32767)[turn % 4]

    lay.fill(32768 + 700)
    lay.fill_waiting(PNG_FLUSH - 258)
    lay.match(258, 32768)                                    # a flush of exactly PNG_FLUSH
    for m, mark in enumerate(RING_MARKS):
        if variant < 2:
            first, second = (3, 258) if variant == 0 else (258, 3)
            lay.fill(mark - first)
            lay.match(first, dist_for(first))
            assert lay.op == mark
            lay.match(second, dist_for(second))
        else:
            length = 3 if variant == 2 else 258
            lay.fill(mark - (1 if length == 3 else 100))
            lay.match(length, dist_for(length))
        lay.match(3, lay.op - (mark - 2))                    # the source across the mark, near
        lay.fill(max(lay.op, mark + 130))
        lay.match(258, lay.op - (mark - 129))
        if m == 2:
            break
        if m == 0:
            lay.fill_waiting(PNG_FLUSH - 1)                  # the match begins one byte short of the threshold
        else:
            lay.fill_waiting(PNG_FLUSH - 4)
            lay.lit(4)                                       # ... and on it: the literal loop stops here and does not flush
            assert lay.waiting() == PNG_FLUSH
        lay.match(258, 32768)
        length, dist = (258 if variant < 2 else 3), (32768 if variant % 2 == 0 else 32767)
        src = mark - (100 if length == 258 else 1)           # the source across the mark, far
        lay.fill(src + dist)
        lay.match(length, dist)
    lay.fill(n)
    return lay.symbols


def ring_coverage(symbols, start=0):
    """({(mark, how, length)}, {how: {distance class}}) of the matches of 3 and of 258 that touch a multiple of the ring's size:
    'dest-across', 'source-across' (a source that the match itself does not run into), 'ends-on', 'starts-on'"""
    hits, classes = set(), {}
    op = start
    for s in symbols:
        if not isinstance(s, tuple):
            op += 1
            continue
        length, dist = pair(s)
        src = op - dist
        for mark in RING_MARKS:
            for how, yes in (('dest-across', op < mark < op + length), ('source-across', dist >= length and src < mark < src + length),
                             ('ends-on', op + length == mark), ('starts-on', op == mark)):
                if yes and length in (3, 258):
                    hits.add((mark, how, length))
                    classes.setdefault(how, set()).add(distance_class(length, dist))
        op += length
    return hits, classes


MIXED_STORED = 40000
MIXED_EDGES = (MIXED_STORED, PNG_WIN + 464, 140000)          # where the fixed block, the first and the second dynamic block begin


def mixed_blocks():
    """the RING picture as a stored block, a fixed block that reaches back into the stored bytes and across the first turn of the ring,
    a dynamic block with codes of up to 15 bits that reaches into both, and a dynamic block whose longest code has 3"""
    H, W, C = RING
    n = H * (W * C + 1)
    dists = (32768, 300, 32767, 4097, 259)
    stored = bytes(np.random.default_rng(90).integers(0, 5, MIXED_STORED).tolist())
    fixed = Layout(MIXED_EDGES[0], 91, dists)
    fixed.match(258, 32768)
    fixed.fill(PNG_WIN - 100)
    fixed.match(258, 32768)                                  # out of the stored bytes, across the turn of the ring
    fixed.fill(MIXED_EDGES[1])
    # 258 and 3 have the shortest codes, end of block and length symbol 8 the two of 15 bits
    ll = chain_lens([285, 257, 0, 1, 2, 3, 4, 258, 259, 260, 261, 262, 263, 264, 265, 256])
    dd = chain_lens([29, 16, 24, 0, 1, 2, 3, 5, 8, 10, 12, 14, 18, 20, 22, 26])
    first = Layout(MIXED_EDGES[1], 92, dists, any_length=False)
    first.match(258, 32768)                                  # from the stored bytes
    first.match(3, 24577)                                    # from the fixed block's
    first.fill(MIXED_EDGES[2])
    ll2 = [3] * 5 + [0] * 251 + [3, 3] + [0] * 27 + [3]
    dd2 = [2] + [0] * 15 + [2] + [0] * 7 + [2] + [0] * 4 + [2]
    second = Layout(MIXED_EDGES[2], 93, dists + (1,), any_length=False)
    second.fill(n)
    return [('stored', stored), ('fixed', fixed.symbols), ('dynamic', ll, dd, first.symbols), ('dynamic', ll2, dd2, second.symbols)]


def sources(symbols, start):
    """[(position, length, distance)] of the matches"""
    out, op = [], start
    for s in symbols:
        if isinstance(s, tuple):
            out.append((op,) + tuple(pair(s)))
        op += pair(s)[0] if isinstance(s, tuple) else 1
    return out


@functools.lru_cache(maxsize=None)
def built_streams():
    """{name: (H, W, C, stream, raw, blocks)}: the long codes (HAND), the four ring layouts and the mixed blocks (RING)"""
    out = {}
    blocks = long_code_blocks()
    raw = blocks_bytes(blocks)
    out['long-codes'] = HAND + (with_adler(blocks_stream(blocks), raw), raw, blocks)
    for v in range(4):
        blocks = [('fixed', ring_symbols(v))]
        raw = blocks_bytes(blocks)
        out[f'ring-{v}'] = RING + (with_adler(blocks_stream(blocks), raw), raw, blocks)
    blocks = mixed_blocks()
    raw = blocks_bytes(blocks)
    out['mixed-blocks'] = RING + (with_adler(blocks_stream(blocks), raw), raw, blocks)
    return out


# -- 3. the fetches of PNG_INW_BYTES bytes of the stream --
def refill_symbols(literals, n, seed=94):
    """`literals` literals (a byte of the stream each in the fixed code), then matches of up to 258 at distance 1 to the end"""
    symbols = np.random.default_rng(seed).integers(0, 5, literals).tolist()
    left = n - literals
    while left:
        if left < 3:
            symbols += [symbols[literals - 1]] * left
            break
        step = 258 if left >= 261 or left == 258 else min(left, 255)
        symbols.append((step, 1))
        left -= step
    return symbols


@functools.lru_cache(maxsize=None)
def refill_streams():
    """({total length: (stream, raw)}, {name: (stream, status word)}): good streams of the REFILL picture whose lengths are
    PNG_INW_BYTES k + r for k = 1, 2 and r = -4 .. 5, so that the four Adler-32 bytes lie before, across and behind a fetch; and what
    has to be refused behind the first fetch"""
    H, W, C = REFILL
    n = H * (W * C + 1)
    good = {}
    for k in (1, 2):
        for x in range(PNG_INW_BYTES * k - 120, PNG_INW_BYTES * k + 6):
            tail = Bits()
            put_symbols(tail, canonical(FIXED_LL), canonical(FIXED_D), refill_symbols(x, n)[x:])
            total = 2 + (3 + 8 * x + 8 * len(tail.out) + tail.n + 7) // 8 + 4
            if total not in good and -4 <= total - PNG_INW_BYTES * k <= 5:
                symbols = refill_symbols(x, n)
                raw = expand(symbols)
                good[total] = (with_adler(fixed_stream(symbols), raw), raw)
                assert len(good[total][0]) == total
    base = good[2 * PNG_INW_BYTES + 5][0]
    bad = {f'cut-{k}': (base[:k], 'TRUNCATED') for k in (8190, 8191, 8192, 8193, 8194, 16384)}
    bad['adler-bit'] = (base[:-3] + bytes([base[-3] ^ 0x10]) + base[-2:], 'BAD_ADLER')
    far = np.random.default_rng(95).integers(0, 5, 8300).tolist() + [(3, 32768)]
    far_body = fixed_stream(far + [0] * (n - 8303))
    bad['far-distance'] = (far_body + bytes(4), 'FAR_DISTANCE')
    return good, bad


# -- 5. the branches of the Paeth and Average filters --
BRANCHES = ('paeth-a', 'paeth-b', 'paeth-c', 'tie-ab', 'tie-bc', 'avg-odd', 'avg-carry')
PLACES = ('row-0', 'first-pixel', 'band-first', 'anywhere')      # behind the first pixel of row 0; of a later row; of rows 64 and 128; all


def branch_masks(a, b, c):
    """{branch: where it is taken} for left, up and up-left bytes (ints or int arrays), residuals()' arithmetic: the predictor Paeth
    chooses, its two ties (pa = pb <= pc goes to a, pb = pc < pa to b), and an Average whose sum is odd or does not fit a byte"""
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    is_a = (pa <= pb) & (pa <= pc)
    is_b = ~is_a & (pb <= pc)
    return {'paeth-a': is_a, 'paeth-b': is_b, 'paeth-c': ~is_a & ~is_b, 'tie-ab': (pa == pb) & (pb <= pc), 'tie-bc': (pb == pc) & (pc < pa),
            'avg-odd': (a + b) % 2 == 1, 'avg-carry': a + b >= 256}


def reachable_branches():
    """{place: the branches that some bytes reach there}.  On row 0 up and up-left are 0, on a first pixel left and up-left are: all 256
    values of the byte that is left are tried.  Elsewhere each branch has a witness."""
    v = np.arange(256)
    zero = np.zeros(256, np.int64)
    row0, first = branch_masks(v, zero, zero), branch_masks(zero, v, zero)
    witness = {'paeth-a': (9, 1, 1), 'paeth-b': (1, 9, 1), 'paeth-c': (10, 12, 11), 'tie-ab': (3, 3, 1), 'tie-bc': (4, 1, 3),
               'avg-odd': (2, 3, 0), 'avg-carry': (200, 100, 0)}
    for name, (a, b, c) in witness.items():
        assert bool(branch_masks(np.int64(a), np.int64(b), np.int64(c))[name]), name
    out = {'row-0': {k for k in BRANCHES if row0[k].any()}, 'first-pixel': {k for k in BRANCHES if first[k].any()}}
    out['band-first'] = out['anywhere'] = set(BRANCHES)
    return out


def filter_branches(img, types):
    """{(branch, place)} that a picture reaches under its rows' filter types: Paeth's on rows of type 4, Average's on rows of type 3"""
    H, W, C = img.shape
    x = img.reshape(H, W * C).astype(np.int64)
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, C:] = x[:, :-C]
    b[1:] = x[:-1]
    c[1:, C:] = x[:-1, :-C]
    rows, cols = np.arange(H)[:, None], np.arange(W * C)[None, :]
    types = np.asarray(types)[:, None]
    places = {'row-0': (rows == 0) & (cols >= C), 'first-pixel': (rows > 0) & (cols < C), 'band-first': ((rows == 64) | (rows == 128)) & (cols >= C),
              'anywhere': rows >= 0}
    out = set()
    for name, mask in branch_masks(a, b, c).items():
        mask = mask & (types == (4 if name in BRANCHES[:5] else 3))
        out |= {(name, place) for place, where in places.items() if (mask & where).any()}
    return out


# -- 4. the refusals the header comment of png_inflate.h promises, one small stream each, and what has to pass next to them --
PROMISED = {                              # name: the status the decoder has to give
    'hlit-30': 'BAD_LENGTHS', 'hlit-31': 'BAD_LENGTHS', 'hdist-30': 'BAD_LENGTHS', 'hdist-31': 'BAD_LENGTHS',
    'repeat-first': 'BAD_LENGTHS', 'repeat-16-past-end': 'BAD_LENGTHS', 'repeat-17-past-end': 'BAD_LENGTHS', 'repeat-18-past-end': 'BAD_LENGTHS',
    'no-end-of-block': 'BAD_LENGTHS',
    'cl-oversubscribed': 'OVERSUBSCRIBED', 'cl-incomplete': 'INCOMPLETE', 'cl-single-code': 'INCOMPLETE',
    'dist-oversubscribed': 'OVERSUBSCRIBED', 'dist-incomplete-two': 'INCOMPLETE', 'dist-single-two-bits': 'INCOMPLETE',
    'symbol-286': 'BAD_CODE', 'symbol-287': 'BAD_CODE', 'distance-30': 'BAD_CODE', 'distance-31': 'BAD_CODE',
    'cinfo-8': 'BAD_HEADER', 'cm-7': 'BAD_HEADER', 'fcheck': 'BAD_HEADER',
    'stored-overrun': 'TOO_LONG', 'match-overrun-by-one': 'TOO_LONG', 'stored-past-stream': 'TRUNCATED',
    # an empty distance code and then a length symbol: png_symbol finds no code in 15 bits (BAD_CODE), or fewer than 15 are left
    'empty-distance-used': 'BAD_CODE', 'empty-distance-used-at-end': 'TRUNCATED',
    'empty-distance-unused': 'OK', 'stray-bytes': 'OK',
}
ZLIB_TAKES = ('stored-overrun', 'match-overrun-by-one')      # streams that are fine for a picture that is not


def raw_dynamic(hlit, hdist, cl_lens=None, items=(), pad=8):
    """a zlib stream that ends in a dynamic block's header: HLIT, HDIST, all 19 lengths of the code-length code, then `items`, (symbol
    of that code, extra value) each, then `pad` zero bytes"""
    cl_lens = CL_LENS if cl_lens is None else cl_lens
    bw = Bits()
    bw.put(1, 1), bw.put(2, 2), bw.put(hlit, 5), bw.put(hdist, 5), bw.put(19 - 4, 4)
    for s in CL_ORDER:
        bw.put(cl_lens[s], 3)
    cl = canonical(cl_lens)
    for s, extra in items:
        bw.code(cl[s])
        bw.put(extra, {16: 2, 17: 3, 18: 7}.get(s, 0))
    return b'\x78\x9c' + bw.bytes() + bytes(pad)


@functools.lru_cache(maxsize=None)
def promised_streams():
    """({name: stream} with PROMISED's names, the picture's filtered bytes): the SMALL picture"""
    H, W, C = SMALL
    n = H * (W * C + 1)
    raw = bytes(np.random.default_rng(96).integers(0, 5, n).tolist())
    lits = list(raw)
    good = with_adler(fixed_stream(lits), raw)
    out = {}
    for v in (30, 31):
        out[f'hlit-{v}'] = raw_dynamic(v, 0)
        out[f'hdist-{v}'] = raw_dynamic(0, v)
    out['repeat-first'] = raw_dynamic(0, 0, items=[(16, 0)])
    # 257 + 1 lengths: 138 + 116 zeros and a 2, then three more than are left; 138 + 117 zeros and four; 138 zeros and 121
    out['repeat-16-past-end'] = raw_dynamic(0, 0, items=[(18, 127), (18, 105), (2, 0), (16, 1)])
    out['repeat-17-past-end'] = raw_dynamic(0, 0, items=[(18, 127), (18, 106), (17, 1)])
    out['repeat-18-past-end'] = raw_dynamic(0, 0, items=[(18, 127), (18, 110)])
    one = [1] + [0] * 255 + [1]                              # a literal and end of block, a bit each
    for name, ll, dd in (('no-end-of-block', [1, 1] + [0] * 255, [1]), ('dist-oversubscribed', one, [1, 1, 1]),
                         ('dist-incomplete-two', one, [2, 2]), ('dist-single-two-bits', one, [2])):
        bw = Bits()
        dynamic_header(bw, ll, dd)
        out[name] = b'\x78\x9c' + bw.bytes() + bytes(8)
    out['cl-oversubscribed'] = raw_dynamic(0, 0, [1, 1, 1] + [0] * 16)
    out['cl-incomplete'] = raw_dynamic(0, 0, [2, 2, 2] + [0] * 16)
    out['cl-single-code'] = raw_dynamic(0, 0, [1] + [0] * 18)
    fixed_ll, fixed_d = canonical(FIXED_LL), canonical(FIXED_D)
    for v in (286, 287):
        bw = Bits()
        bw.put(1, 1), bw.put(1, 2)
        for s in lits[:4] + [v]:
            bw.code(fixed_ll[s])
        out[f'symbol-{v}'] = b'\x78\x9c' + bw.bytes() + bytes(8)
    for v in (30, 31):
        bw = Bits()
        bw.put(1, 1), bw.put(1, 2)
        for s in lits[:4] + [257]:
            bw.code(fixed_ll[s])
        bw.put(int(format(v, '05b')[::-1], 2), 5)            # the fixed distance code: five bits, highest first
        out[f'distance-{v}'] = b'\x78\x9c' + bw.bytes() + bytes(8)
    out['cinfo-8'] = bytes([0x88, 31 - 0x8800 % 31]) + good[2:]
    out['cm-7'] = bytes([0x77, 31 - 0x7700 % 31]) + good[2:]
    out['fcheck'] = bytes([0x78, 0x9d]) + good[2:]
    assert all(out[k][1] & 32 == 0 and (out[k][0] << 8 | out[k][1]) % 31 == 0 for k in ('cinfo-8', 'cm-7'))
    more = raw + b'\x02'
    out['stored-overrun'] = with_adler(blocks_stream([('stored', more)]), more)
    more = expand(lits[:n - 2] + [(3, 1)])
    out['match-overrun-by-one'] = with_adler(fixed_stream(lits[:n - 2] + [(3, 1)]), more)
    out['stored-past-stream'] = blocks_stream([('stored', raw)])[:-1]
    # literals 0 .. 4 and end of block (and, for the twins, length symbol 0) in a complete code; HDIST = 0 and that one length 0
    ll = [2, 2, 2, 3, 4] + [0] * 251 + [4]
    bw = Bits()
    dynamic_header(bw, ll, [0])
    put_symbols(bw, canonical(ll), {}, lits)
    out['empty-distance-unused'] = with_adler(b'\x78\x9c' + bw.bytes(), raw)
    ll = [2, 2, 2, 3, 4] + [0] * 251 + [5, 5]
    bw = Bits()
    dynamic_header(bw, ll, [0])
    for s in lits[:4] + [257]:
        bw.code(canonical(ll)[s])
    out['empty-distance-used'] = b'\x78\x9c' + bw.bytes() + bytes(8)
    out['empty-distance-used-at-end'] = b'\x78\x9c' + bw.bytes()
    out['stray-bytes'] = good + b'\x05\xfa'
    assert sorted(out) == sorted(PROMISED)
    return out, good, raw


# -- 6. more workgroups than a card runs at once --
CARD = (5, 3, 3)
CARD_FILES = 600
CARD_BREAKS = ('TRUNCATED', 'BAD_ADLER', 'BAD_HEADER', 'TOO_SHORT')


@functools.lru_cache(maxsize=None)
def card_streams():
    """[(good stream, picture, broken stream or None, its status word)], CARD_FILES of them: every picture is another one, its rows
    under one of FILTER_MODES in turn; every 7th has a broken twin: cut in the middle, an Adler-32 bit, FDICT set, a row short"""
    H, W, C = CARD
    out = []
    for k in range(CARD_FILES):
        img = pixels(H, W, C, 5000 + k)
        raw = filtered(img, FILTER_MODES[k % 7], k)
        good = compress(raw, (1, 6, 9)[k % 3])
        broken, word = None, None
        if k % 7 == 3:
            word = CARD_BREAKS[k // 7 % 4]
            broken = {'TRUNCATED': good[:len(good) // 2], 'BAD_ADLER': good[:-1] + bytes([good[-1] ^ (1 << k % 8)]),
                      'BAD_HEADER': bytes([0x78, 0xbb]) + good[2:], 'TOO_SHORT': compress(raw[:-(W * C + 1)])}[word]
        out.append((good, img, broken, word))
    return out
