// PNG on the way in: a zlib stream (RFC 1950: header, deflate blocks of RFC 1951, Adler-32) to the filtered rows of an 8-bit image, and
// the five row filters of the PNG specification undone.  Plain integer C++, marked __host__ __device__: the text that runs in
// csrc/r2l_png_decode.hip is the text tools/png_decode_asan_main.cpp runs under the sanitizers on the CPU.
//
// The decoder is written for `width` co-operating lanes (Co: 64 lanes of one wave on the device, 1 on the host).  Every lane decodes
// the same bits; the lanes share the work of building the lookup tables, of match and stored-block copies, of flushing the window and
// of the Adler-32 sums.  The last 64 KiB of output live in a ring (png_inflate_mem::win, LDS on the device): literals and matches are
// written there, a match reads there, and the ring goes to `out` PNG_FLUSH bytes at a time.  Co::sync() stands between a write by one
// lane and a read by another; nothing relies on the order in which instructions issue.
//
// Nothing here trusts the stream: every read is checked against its end, every write against `expect` = H * row_bytes, every loop is
// bounded by one of the two, and whatever is wrong comes back as an r2l_png_status (include/r2l_hip.h).  What zlib's inflate refuses is
// refused: FDICT, block type 3, LEN / NLEN, more than 286 / 30 code lengths, a repeat without a previous length or past the end,
// over-subscribed codes, incomplete codes other than a single code of one bit, a missing end-of-block code, symbols 286 / 287 and
// distance codes 30 / 31, a distance before the first byte, a wrong Adler-32.
#pragma once
#include <stdint.h>

#include "../../include/r2l_hip.h"

#if defined(__HIPCC__)
#define PNG_HD __host__ __device__
#else
#define PNG_HD
#endif

typedef unsigned long long png_u64;

constexpr unsigned PNG_WIN = 65536;           // ring of the newest output bytes: a power of two above 32768 + 258 + PNG_FLUSH
constexpr unsigned PNG_WIN_MASK = PNG_WIN - 1;
constexpr unsigned PNG_FLUSH = 16384;         // the ring goes to memory once this much is waiting
constexpr int PNG_LBITS = 10;                 // bits that index the literal / length table; longer codes walk the canonical counts
constexpr int PNG_DBITS = 9;                  // ... the distance table (and, with 7 of them, the code-length table)
constexpr unsigned PNG_INW = 2048;             // 32-bit words of the stream held at a time (8 KiB): the lanes fetch them together
constexpr int PNG_MAX_LANES = 64;
constexpr uint32_t PNG_ADLER_MOD = 65521u;

struct png_inflate_mem {
    unsigned char win[PNG_WIN];
    uint32_t inw[PNG_INW];                    // words w of the stream, w in [fw - PNG_INW, fw), at inw[w mod PNG_INW]; bytes past the end are 0
    png_u64 red[2 * PNG_MAX_LANES];           // the lanes' partial sums
    uint16_t lfast[1 << PNG_LBITS], dfast[1 << PNG_DBITS];      // symbol << 4 | bits, 0 = not here
    uint16_t lsym[288], dsym[32];             // symbols in canonical order
    uint16_t lcnt[16], dcnt[16];              // codes of each length
    uint16_t first[16], start[16], next[16];  // while a table is built: first code, first index and running index of each length
    unsigned char lens[320];                  // literal / length lengths, then the distance lengths
    unsigned char clens[32];                  // the code-length code's
};

// one lane, nothing to wait for: the host
struct png_serial {
    PNG_HD unsigned lane() const { return 0; }
    PNG_HD unsigned width() const { return 1; }
    PNG_HD void sync() const {}
    PNG_HD unsigned uniform(unsigned v) const { return v; }      // a value every lane holds alike
};

struct png_bits {
    const unsigned char* in;
    unsigned n;               // bytes of the stream
    unsigned w, fw;           // next word to take from inw; words [w, fw) are there
    png_u64 hold;             // bits not yet used, the next one lowest; zero above `avail`
    unsigned avail;           // bits of the STREAM in hold: the zeros that stand for bytes past its end are not counted
};

// 33 bits or more, or all that is left of the stream.  A word comes from inw; when inw is used up, the lanes fetch the next PNG_INW
// words together, a byte at a time and each byte only if it lies inside the stream.
template <class Co>
PNG_HD inline void png_refill(const Co& co, png_inflate_mem* m, png_bits& b) {
    if (b.avail > 32) return;
    if (b.w == b.fw) {
        co.sync();      // every lane has read the words that are overwritten now
        for (unsigned k = b.w + co.lane(); k < b.w + PNG_INW; k += co.width()) {
            uint32_t v = 0;
            for (unsigned j = 0; j < 4; ++j) {      // without a branch, so that the four loads are in flight together: past the end the last
                const unsigned i = 4 * k + j;       // byte of the stream (there are two at least) is read again, and dropped
                const uint32_t c = b.in[i < b.n ? i : b.n - 1];
                v |= (i < b.n ? c : 0u) << (8 * j);
            }
            m->inw[k & (PNG_INW - 1)] = v;
        }
        b.fw = b.w + PNG_INW;
        co.sync();
    }
    const unsigned first = 4 * b.w;      // below 2^31 + 4 PNG_INW refills past the end; every refill past the end is followed by a refusal
    const unsigned real = first >= b.n ? 0u : b.n - first >= 4 ? 32u : 8 * (b.n - first);
    b.hold |= (png_u64)co.uniform(m->inw[b.w & (PNG_INW - 1)]) << b.avail;
    b.avail += real;
    ++b.w;
}
// Every lane holds the same reader; saying so (a first-lane read on the device) keeps it in scalar registers and its branches scalar
template <class Co>
PNG_HD inline void png_settle(const Co& co, png_bits& b) {
    b.hold = (png_u64)co.uniform((unsigned)b.hold) | (png_u64)co.uniform((unsigned)(b.hold >> 32)) << 32;
    b.avail = co.uniform(b.avail), b.w = co.uniform(b.w), b.fw = co.uniform(b.fw);
}
// the next bit to come is bit 0 of byte `pos` of the stream
template <class Co>
PNG_HD inline void png_seek(const Co& co, png_inflate_mem* m, png_bits& b, unsigned pos) {
    b.w = b.fw = pos >> 2;
    b.hold = 0, b.avail = 0;
    png_refill(co, m, b);
    const unsigned drop = 8 * (pos & 3u) < b.avail ? 8 * (pos & 3u) : b.avail;
    b.hold >>= drop;
    b.avail -= drop;
}
// the byte the next bit lies in (the stream is at a byte boundary, or the bits before it in that byte are used)
PNG_HD inline unsigned png_byte_pos(const png_bits& b) {
    const unsigned loaded = 4 * b.w < b.n ? 4 * b.w : b.n;
    return loaded - ((b.avail + 7) >> 3);
}
PNG_HD inline bool png_take(png_bits& b, unsigned n, unsigned& v) {      // n <= 16 bits; false past the end of the stream
    if (n > b.avail) return false;
    v = (unsigned)b.hold & ((1u << n) - 1u);
    b.hold >>= n;
    b.avail -= n;
    return true;
}

PNG_HD inline unsigned png_bit_reverse(unsigned code, unsigned len) {
    unsigned r = 0;
    for (unsigned i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// One symbol of a code: the table for codes of up to fb bits, the canonical counts bit by bit for longer ones
template <class Co>
PNG_HD inline int png_symbol(const Co& co, png_bits& b, const uint16_t* fast, int fb, const uint16_t* cnt, const uint16_t* sym, unsigned& out) {
    const unsigned e = co.uniform(fast[(unsigned)b.hold & ((1u << fb) - 1u)]);
    if (e) {
        const unsigned l = e & 15u;
        if (l > b.avail) return R2L_PNG_TRUNCATED;
        b.hold >>= l;
        b.avail -= l;
        out = e >> 4;
        return R2L_PNG_OK;
    }
    int code = 0, first = 0, index = 0;
    for (unsigned len = 1; len <= 15; ++len) {
        code |= (int)((b.hold >> (len - 1)) & 1u);
        const int count = (int)co.uniform(cnt[len]);
        if (code - count < first) {
            if (len > b.avail) return R2L_PNG_TRUNCATED;
            b.hold >>= len;
            b.avail -= len;
            out = co.uniform(sym[index + (code - first)]);
            return R2L_PNG_OK;
        }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return b.avail < 15 ? R2L_PNG_TRUNCATED : R2L_PNG_BAD_CODE;
}

// The tables of n code lengths.  strict: an incomplete code is refused outright (the code-length code); otherwise a single code of one
// bit passes, as in zlib.  No code at all passes either way and fails at its first use.
template <class Co>
PNG_HD inline int png_build(const Co& co, png_inflate_mem* m, const unsigned char* lens, unsigned n, uint16_t* fast, int fb, uint16_t* cnt,
                            uint16_t* sym, bool strict) {
    co.sync();      // the lengths are one lane's writes; the tables may still be read by a lane that is behind
    if (co.lane() == 0) {
        for (unsigned l = 0; l < 16; ++l) cnt[l] = 0;
        for (unsigned s = 0; s < n; ++s) cnt[lens[s] & 15u] = (uint16_t)(cnt[lens[s] & 15u] + 1);
    }
    for (unsigned i = co.lane(); i < (1u << fb); i += co.width()) fast[i] = 0;
    co.sync();
    int left = 1;
    unsigned longest = 0, total = 0;
    for (unsigned l = 1; l <= 15; ++l) {
        const unsigned c = co.uniform(cnt[l]);
        left = (left << 1) - (int)c;
        if (left < 0) return R2L_PNG_OVERSUBSCRIBED;
        if (c) longest = l;
        total += c;
    }
    if (left > 0 && longest != 0 && (strict || longest != 1)) return R2L_PNG_INCOMPLETE;
    if (co.lane() == 0) {
        unsigned code = 0, offs = 0;
        for (unsigned l = 1; l <= 15; ++l) {
            code = (code + (l > 1 ? cnt[l - 1] : 0u)) << 1;
            m->first[l] = (uint16_t)code;
            m->start[l] = m->next[l] = (uint16_t)offs;
            offs += cnt[l];
        }
        for (unsigned s = 0; s < n; ++s) {
            const unsigned l = lens[s] & 15u;
            if (l) {
                sym[m->next[l]] = (uint16_t)s;
                m->next[l] = (uint16_t)(m->next[l] + 1);
            }
        }
    }
    co.sync();
    for (unsigned i = co.lane(); i < total; i += co.width()) {      // total <= n: every symbol has its own place
        const unsigned s = sym[i], l = lens[s] & 15u;
        if (l <= (unsigned)fb) {
            const unsigned code = m->first[l] + (i - m->start[l]);
            for (unsigned k = png_bit_reverse(code, l); k < (1u << fb); k += 1u << l) fast[k] = (uint16_t)(s << 4 | l);
        }
    }
    co.sync();
    return R2L_PNG_OK;
}

// win[from, to) to out and into the Adler-32 pair (a, b)
template <class Co>
PNG_HD inline void png_flush(const Co& co, png_inflate_mem* m, unsigned char* out, unsigned from, unsigned to, uint32_t& a, uint32_t& b) {
    co.sync();
    const unsigned L = to - from;      // at most PNG_FLUSH + 258 + PNG_FLUSH
    png_u64 s1 = 0, s2 = 0;
    for (unsigned j = co.lane(); j < L; j += co.width()) {
        const unsigned d = m->win[(from + j) & PNG_WIN_MASK];
        out[from + j] = (unsigned char)d;
        s1 += d;
        s2 += (png_u64)(L - j) * d;
    }
    m->red[2 * co.lane()] = s1;
    m->red[2 * co.lane() + 1] = s2;
    co.sync();
    png_u64 t1 = 0, t2 = 0;
    for (unsigned k = 0; k < co.width(); ++k) t1 += m->red[2 * k], t2 += m->red[2 * k + 1];
    co.sync();
    b = (uint32_t)((b + (png_u64)L * a + t2) % PNG_ADLER_MOD);
    a = (uint32_t)((a + t1) % PNG_ADLER_MOD);
}

// in[0, n_in), a zlib stream, to out[0, H * row_bytes).  Returns an r2l_png_status, the same in every lane; *adler (may be NULL) gets the
// Adler-32 of what was written.  On a status other than OK the bytes of out are unspecified, and none outside it is touched.
template <class Co>
PNG_HD inline int png_inflate(const Co& co, png_inflate_mem* m, const unsigned char* in, unsigned n_in, unsigned char* out, unsigned H,
                              unsigned row_bytes, uint32_t* adler) {
    const unsigned expect = H * row_bytes;
    if (adler) *adler = 1;
    if (n_in < 2) return R2L_PNG_TRUNCATED;
    const unsigned cmf = in[0], flg = in[1];
    if ((cmf & 15u) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31u != 0 || (flg & 32u)) return R2L_PNG_BAD_HEADER;
    png_bits bs = {in, n_in, 0, 0, 0, 0};
    png_seek(co, m, bs, 2);
    unsigned op = 0, flushed = 0;      // bytes produced, bytes of them in out
    uint32_t a = 1, b = 0;
    unsigned final_block = 0;
    do {
        unsigned type = 0;
        png_settle(co, bs);
        op = co.uniform(op), flushed = co.uniform(flushed);
        png_refill(co, m, bs);
        if (!png_take(bs, 1, final_block) || !png_take(bs, 2, type)) return R2L_PNG_TRUNCATED;
        if (type == 3) return R2L_PNG_BAD_BLOCK;
        if (type == 0) {
            unsigned skip, len, nlen;
            png_take(bs, bs.avail & 7u, skip);
            png_refill(co, m, bs);
            if (!png_take(bs, 16, len)) return R2L_PNG_TRUNCATED;
            png_refill(co, m, bs);
            if (!png_take(bs, 16, nlen)) return R2L_PNG_TRUNCATED;
            if ((len ^ 0xffffu) != nlen) return R2L_PNG_BAD_STORED;
            unsigned pos = png_byte_pos(bs);      // the bytes of the block go from the stream itself to the window
            if (len > bs.n - pos) return R2L_PNG_TRUNCATED;
            if (len > expect - op) return R2L_PNG_TOO_LONG;
            while (len) {
                const unsigned piece = len < PNG_FLUSH ? len : PNG_FLUSH;
                for (unsigned j = co.lane(); j < piece; j += co.width()) m->win[(op + j) & PNG_WIN_MASK] = bs.in[pos + j];
                op += piece, pos += piece, len -= piece;
                if (op - flushed >= PNG_FLUSH) png_flush(co, m, out, flushed, op, a, b), flushed = op;
            }
            png_seek(co, m, bs, pos);
            continue;
        }
        unsigned nlen = 288, ndist = 32;
        if (type == 1) {
            co.sync();
            if (co.lane() == 0) {
                for (unsigned s = 0; s < 288; ++s) m->lens[s] = (unsigned char)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
                for (unsigned s = 0; s < 32; ++s) m->lens[288 + s] = 5;      // 30 and 31 complete the code and are refused when met
            }
        } else {
            unsigned hlit, hdist, hclen;
            if (!png_take(bs, 5, hlit) || !png_take(bs, 5, hdist) || !png_take(bs, 4, hclen)) return R2L_PNG_TRUNCATED;
            nlen = hlit + 257, ndist = hdist + 1, hclen += 4;
            if (nlen > 286 || ndist > 30) return R2L_PNG_BAD_LENGTHS;
            co.sync();
            for (unsigned i = 0; i < 19; ++i) {
                unsigned v = 0;
                png_refill(co, m, bs);
                if (i < hclen && !png_take(bs, 3, v)) return R2L_PNG_TRUNCATED;
                const unsigned order = i < 3 ? 16 + i : i == 3 ? 0 : i & 1u ? 7 - ((i - 5) >> 1) : 6 + (i >> 1);      // 16 17 18 0 8 7 9 6 10 5 ...
                if (co.lane() == 0) m->clens[order] = (unsigned char)v;
            }
            int e = png_build(co, m, m->clens, 19, m->dfast, 7, m->dcnt, m->dsym, true);
            if (e) return e;
            unsigned prev = 0;
            for (unsigned i = 0; i < nlen + ndist;) {
                unsigned s, rep = 1, v;
                png_settle(co, bs);
                i = co.uniform(i), prev = co.uniform(prev);
                png_refill(co, m, bs);
                e = png_symbol(co, bs, m->dfast, 7, m->dcnt, m->dsym, s);
                if (e) return e;
                if (s < 16) {
                    v = prev = s;
                } else if (s == 16) {
                    if (i == 0) return R2L_PNG_BAD_LENGTHS;
                    if (!png_take(bs, 2, rep)) return R2L_PNG_TRUNCATED;
                    rep += 3, v = prev;
                } else {
                    if (!png_take(bs, s == 17 ? 3 : 7, rep)) return R2L_PNG_TRUNCATED;
                    rep += s == 17 ? 3 : 11, v = prev = 0;
                }
                if (rep > nlen + ndist - i) return R2L_PNG_BAD_LENGTHS;
                if (co.lane() == 0)      // the distance lengths sit behind room for 288 literal / length ones
                    for (unsigned k = 0; k < rep; ++k) m->lens[i + k < nlen ? i + k : 288 + (i + k - nlen)] = (unsigned char)v;
                i += rep;
            }
            co.sync();
            if (co.uniform(m->lens[256]) == 0) return R2L_PNG_BAD_LENGTHS;      // no end-of-block code
        }
        int e = png_build(co, m, m->lens, nlen, m->lfast, PNG_LBITS, m->lcnt, m->lsym, false);
        if (!e) e = png_build(co, m, m->lens + 288, ndist, m->dfast, PNG_DBITS, m->dcnt, m->dsym, false);
        if (e) return e;
        for (;;) {      // every turn uses at least one bit of the stream or returns
            unsigned s;
            png_settle(co, bs);
            op = co.uniform(op), flushed = co.uniform(flushed);
            // literals whose code the table holds, one after the other with one test each: up to where the window wants flushing, the
            // image ends, or the stream runs low; whatever ends the run (a length, a long code, an error) is the general path's below
            const unsigned stop = expect - flushed < PNG_FLUSH ? expect : flushed + PNG_FLUSH;
            for (;;) {
                png_refill(co, m, bs);
                const unsigned e = co.uniform(m->lfast[(unsigned)bs.hold & ((1u << PNG_LBITS) - 1u)]);
                if (e == 0 || e >= (256u << 4) || bs.avail < 16 || op >= stop) break;
                bs.hold >>= e & 15u;
                bs.avail -= e & 15u;
                if (co.lane() == 0) m->win[op & PNG_WIN_MASK] = (unsigned char)(e >> 4);
                ++op;
            }
            png_refill(co, m, bs);      // 33 bits or the rest: a literal / length code and its extra bits take 20 at most
            e = png_symbol(co, bs, m->lfast, PNG_LBITS, m->lcnt, m->lsym, s);
            if (e) return e;
            if (s < 256) {
                if (op >= expect) return R2L_PNG_TOO_LONG;
                if (co.lane() == 0) m->win[op & PNG_WIN_MASK] = (unsigned char)s;
                ++op;
            } else if (s == 256) {
                break;
            } else {
                if (s > 285) return R2L_PNG_BAD_CODE;
                unsigned len, dist, ds, extra = 0;
                s -= 257;
                if (s < 8) {
                    len = 3 + s;
                } else if (s == 28) {
                    len = 258;
                } else {
                    const unsigned eb = (s - 4) >> 2;
                    if (!png_take(bs, eb, extra)) return R2L_PNG_TRUNCATED;
                    len = 3 + ((4 + (s & 3u)) << eb) + extra;
                }
                png_refill(co, m, bs);      // ... a distance code and its extra bits 28
                e = png_symbol(co, bs, m->dfast, PNG_DBITS, m->dcnt, m->dsym, ds);
                if (e) return e;
                if (ds > 29) return R2L_PNG_BAD_CODE;
                if (ds < 4) {
                    dist = ds + 1;
                } else {
                    const unsigned eb = (ds >> 1) - 1;
                    if (!png_take(bs, eb, extra)) return R2L_PNG_TRUNCATED;
                    dist = 1 + ((2 + (ds & 1u)) << eb) + extra;
                }
                if (dist > op) return R2L_PNG_FAR_DISTANCE;
                if (len > expect - op) return R2L_PNG_TOO_LONG;
                // byte j of the match is byte j mod dist of the dist bytes before it: every read lies before op, so the lanes may
                // take the bytes in any order and a match that overlaps itself still gives what a byte-by-byte copy gives
                co.sync();
                const unsigned src = op - dist;
                for (unsigned j = co.lane(); j < len; j += co.width())
                    m->win[(op + j) & PNG_WIN_MASK] = m->win[(src + (dist >= len ? j : j % dist)) & PNG_WIN_MASK];
                op += len;
            }
            if (op - flushed >= PNG_FLUSH) png_flush(co, m, out, flushed, op, a, b), flushed = op;
        }
    } while (!final_block);
    png_flush(co, m, out, flushed, op, a, b);
    if (adler) *adler = b << 16 | a;
    if (op != expect) return R2L_PNG_TOO_SHORT;
    unsigned skip, stored = 0;
    png_take(bs, bs.avail & 7u, skip);
    png_refill(co, m, bs);
    for (int i = 0; i < 4; ++i) {
        unsigned v;
        if (!png_take(bs, 8, v)) return R2L_PNG_TRUNCATED;
        stored = stored << 8 | v;
    }
    if (stored != (b << 16 | a)) return R2L_PNG_BAD_ADLER;
    co.sync();      // out is read by other lanes than wrote it
    png_u64 bad = 0;
    for (unsigned r = co.lane(); r < H; r += co.width()) bad |= out[r * row_bytes] > 4;
    m->red[co.lane()] = bad;
    co.sync();
    bad = 0;
    for (unsigned k = 0; k < co.width(); ++k) bad |= m->red[k];
    co.sync();
    return bad ? R2L_PNG_BAD_FILTER : R2L_PNG_OK;
}

// ---- the filters ----
// One byte: x as stored, a left, b up, c up-left (PNG 1.2, 6.6 / 9.2-9.4).  A type above 4 never gets here (png_inflate refuses it).
PNG_HD inline unsigned png_recon(unsigned ft, unsigned x, unsigned a, unsigned b, unsigned c) {
    unsigned pred = 0;
    if (ft == 1) {
        pred = a;
    } else if (ft == 2) {
        pred = b;
    } else if (ft == 3) {
        pred = (a + b) >> 1;
    } else if (ft == 4) {
        const int p = (int)a + (int)b - (int)c;
        const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p, pc = p > (int)c ? p - (int)c : (int)c - p;
        pred = (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;
    }
    return (x + pred) & 255u;
}

// raw [H, 1 + W C] to px [H, W C], one byte after the other: what the skewed wavefront of the device kernel has to equal
PNG_HD inline void png_unfilter_serial(const unsigned char* raw, unsigned H, unsigned W, unsigned C, unsigned char* px) {
    const unsigned stride = W * C;
    for (unsigned y = 0; y < H; ++y) {
        const unsigned char* row = raw + (png_u64)y * (stride + 1);
        unsigned char* cur = px + (png_u64)y * stride;
        const unsigned char* up = y ? cur - stride : nullptr;
        const unsigned ft = row[0];
        for (unsigned i = 0; i < stride; ++i) {
            const unsigned a = i >= C ? cur[i - C] : 0u, b = up ? up[i] : 0u, c = (up && i >= C) ? up[i - C] : 0u;
            cur[i] = (unsigned char)png_recon(ft, row[1 + i], a, b, c);
        }
    }
}
