"""What the Motion-JPEG tests hold the encoder to, written from ITU-T T.81 alone (no library code is used): the arithmetic of a
baseline 4:4:4 encoder in float64 (`reference_coefficients`) and a baseline decoder of the entropy-coded scan (`decode`, T.81 F.2.2) that
takes every table from the file's own DQT / DHT / SOF0 / SOS segments."""
import struct

import numpy as np


def zigzag():
    """zig-zag position -> natural index, walked along the anti-diagonals (T.81 figure A.6)"""
    order = []
    for s in range(15):
        diag = [(r, s - r) for r in range(8) if 0 <= s - r < 8]
        order += diag if s % 2 else diag[::-1]
    return [r * 8 + c for r, c in order]


ZZ = np.array(zigzag())


def to_bytes(frames):
    """p = floor(255 clamp(x, 0, 1)) in float32, as frontend.to8b computes it; NaN = 0"""
    x = np.asarray(frames, dtype=np.float32)
    x = np.where(np.isnan(x), np.float32(0), x)
    return np.floor(np.float32(255) * np.clip(x, np.float32(0), np.float32(1))).astype(np.float64)


def reference_coefficients(frames, luma_zz, chroma_zz):
    """frames [n, H, W, 3] -> F / Q before rounding, float64 [n, n_blocks, 3, 64] in zig-zag order (blocks in raster order): bytes,
    replicate padding to multiples of 8, JFIF YCbCr with the level shift on Y, the FDCT of T.81 A.3.3, the division by the quantiser"""
    p = to_bytes(frames)
    n, H, W, _ = p.shape
    p = np.pad(p, ((0, 0), (0, -H % 8), (0, -W % 8), (0, 0)), mode='edge')
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    ycc = np.stack([0.299 * R + 0.587 * G + 0.114 * B - 128., -0.168736 * R - 0.331264 * G + 0.5 * B, 0.5 * R - 0.418688 * G - 0.081312 * B], 1)
    bh, bw = p.shape[1] // 8, p.shape[2] // 8
    blocks = ycc.reshape(n, 3, bh, 8, bw, 8).transpose(0, 2, 4, 1, 3, 5).reshape(n, bh * bw, 3, 8, 8)       # [.., y, x]
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    c = 0.5 * np.where(u == 0, np.sqrt(0.5), 1.0) * np.cos((2 * x + 1) * u * np.pi / 16)                    # [u, x]
    F = np.einsum('vy,nbcyx,ux->nbcvu', c, blocks, c).reshape(n, bh * bw, 3, 64)                            # natural index v * 8 + u
    q_nat = np.empty((3, 64))
    q_nat[0, ZZ], q_nat[1, ZZ] = luma_zz, chroma_zz
    q_nat[2] = q_nat[1]
    return (F / q_nat[None, None])[..., ZZ]


def quantise(pre):
    """round to nearest, the AC coefficients clamped to +-1023"""
    q = np.rint(pre)
    q[..., 1:] = np.clip(q[..., 1:], -1023, 1023)
    return q.astype(np.int64)


def tie_distance(pre):
    """how far F / Q is from the nearest half-integer"""
    return np.abs(pre - np.floor(pre) - 0.5)


class Jpeg:
    pass


def parse(data):
    """The segments of a baseline file: quantisers, frame header, Huffman tables, scan header; where the scan starts"""
    assert data[:2] == b'\xff\xd8', 'no SOI'
    j = Jpeg()
    j.qt, j.huff, j.markers = {}, {}, []
    at = 2
    while True:
        assert data[at] == 0xFF and data[at + 1] not in (0x00, 0xFF), f'no marker at {at}'
        marker = data[at + 1]
        n = struct.unpack('>H', data[at + 2:at + 4])[0]
        body = data[at + 4:at + 2 + n]
        j.markers.append(marker)
        if marker == 0xDB:
            assert len(body) == 65 and body[0] >> 4 == 0, '8-bit tables, one per segment'
            j.qt[body[0] & 15] = list(body[1:])
        elif marker == 0xC0:
            prec, j.H, j.W, nc = struct.unpack('>BHHB', body[:6])
            assert prec == 8 and len(body) == 6 + 3 * nc
            j.comps = [(body[6 + 3 * k], body[7 + 3 * k], body[8 + 3 * k]) for k in range(nc)]            # id, sampling, quantiser
        elif marker == 0xC4:
            bits, vals = list(body[1:17]), list(body[17:])
            assert sum(bits) == len(vals)
            j.huff[body[0]] = (bits, vals)
        elif marker == 0xDA:
            ns = body[0]
            j.scan = [(body[1 + 2 * k], body[2 + 2 * k] >> 4, body[2 + 2 * k] & 15) for k in range(ns)]      # id, DC table, AC table
            assert tuple(body[1 + 2 * ns:]) == (0, 63, 0), 'one sequential scan of all 64 coefficients'
            j.scan_at = at + 2 + n
            return j
        else:
            assert 0xE0 <= marker <= 0xEF or marker == 0xFE, f'unexpected marker {marker:02x}'
        at += 2 + n


def _lookup(bits, vals):
    """16-bit prefix -> (length, symbol) of a table given as BITS / HUFFVAL (T.81 Annex C); length 0 where no code starts"""
    length, symbol = np.zeros(65536, np.int64), np.zeros(65536, np.int64)
    code, k = 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            lo = code << (16 - n)
            length[lo:lo + (1 << (16 - n))] = n
            symbol[lo:lo + (1 << (16 - n))] = vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return length.tolist(), symbol.tolist()


def decode(data):
    """A complete baseline 4:4:4 file -> dict(H, W, qt, coef int64 [n_blocks, 3, 64] in zig-zag order with the DC prediction undone,
    zrl: ZRL symbols met, eob: EOB symbols met, stuffed: 0x00 bytes removed, end: the position after FF D9).  Asserts what T.81 asks of
    the scan: a 0x00 after every 0xFF, no other marker before EOI, one-bits as padding, nothing between the last unit and EOI."""
    j = parse(data)
    assert len(j.comps) == 3 and all(s == 0x11 for _, s, _ in j.comps), '4:4:4'
    assert [c[0] for c in j.scan] == [c[0] for c in j.comps], 'one interleaved scan'
    eoi = data.index(b'\xff\xd9', j.scan_at)
    raw = data[j.scan_at:eoi]
    k = raw.find(b'\xff')
    while k >= 0:
        assert k + 1 < len(raw) and raw[k + 1] == 0, f'0xFF at scan byte {k} is followed by {raw[k + 1:k + 2].hex() or "the end"}'
        k = raw.find(b'\xff', k + 2)
    clean = raw.replace(b'\xff\x00', b'\xff')
    bits = ''.join(f'{b:08b}' for b in clean) + '1' * 32
    tables = {key: _lookup(*t) for key, t in j.huff.items()}
    n_blocks = ((j.H + 7) // 8) * ((j.W + 7) // 8)
    coef = np.zeros((n_blocks, 3, 64), np.int64)
    pos, zrl, eob = 0, 0, 0

    def receive(n):                       # T.81 F.2.2.1 EXTEND on n bits
        nonlocal pos
        if n == 0:
            return 0
        v = int(bits[pos:pos + n], 2)
        pos += n
        return v if v >> (n - 1) else v - (1 << n) + 1

    def symbol(table):
        nonlocal pos
        peek = int(bits[pos:pos + 16], 2)
        n = table[0][peek]
        assert n, f'no Huffman code at bit {pos}'
        pos += n
        return table[1][peek]
    pred = [0, 0, 0]
    for b in range(n_blocks):
        for c, (_, td, ta) in enumerate(j.scan):
            dc, ac = tables[td], tables[0x10 | ta]
            pred[c] += receive(symbol(dc))
            out = [pred[c]] + [0] * 63
            k = 1
            while k < 64:
                rs = symbol(ac)
                r, s = rs >> 4, rs & 15
                if s == 0:
                    if r != 15:
                        assert r == 0, f'symbol {rs:02x}'
                        eob += 1
                        break
                    zrl += 1
                    k += 16
                    continue
                k += r
                assert k < 64, 'a run past coefficient 63'
                out[k] = receive(s)
                k += 1
            coef[b, c] = out
    assert pos <= 8 * len(clean), 'the scan ends inside a unit'
    assert 8 * len(clean) - pos < 8 and set(bits[pos:8 * len(clean)]) <= {'1'}, 'padding: fewer than 8 bits, all ones'
    return dict(H=j.H, W=j.W, qt=j.qt, coef=coef, zrl=zrl, eob=eob, stuffed=len(raw) - len(clean), end=eoi + 2, markers=j.markers)

