"""The pictures, zlib streams and PNG files of the PNG decoder's tests (test_png_decode_cpu.py: csrc/png_inflate.h on the CPU under the
sanitizers; test_png_decode_gpu.py: the same text on the device), written with zlib and struct alone.

A case is (name, H, W, C, stream, want): want is the bytes H rows of 1 + W C that the stream has to inflate to, or None for a stream
that has to be refused.  zlib.decompress is the judge of which is which: it returns `want` for the former and, except where the case
says otherwise (a picture one row short or long, a filter byte of 5: streams that are fine and pictures that are not), raises for
the latter."""
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


def put_symbols(bw, ll, dd, symbols):
    """symbols: ints (literals) and (length, distance) pairs; then end of block"""
    for s in symbols:
        if isinstance(s, tuple):
            length, dist = s
            i = max(k for k in range(29) if LEN_BASE[k] <= length) if length < 258 else 28
            bw.code(ll[257 + i])
            bw.put(length - LEN_BASE[i], LEN_EXTRA[i])
            j = max(k for k in range(30) if DIST_BASE[k] <= dist)
            bw.code(dd[j])
            bw.put(dist - DIST_BASE[j], DIST_EXTRA[j])
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


def expand(symbols):
    out = bytearray()
    for s in symbols:
        if isinstance(s, tuple):
            for _ in range(s[0]):
                out.append(out[-s[1]])
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
