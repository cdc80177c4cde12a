// PNG: rendered frames to finished .png files on the device (PNG 1.2: 8-bit RGB, colour type 2, non-interlaced; zlib stream of RFC 1950,
// deflate blocks of RFC 1951), one C-ABI call per stack of frames.  The host side is png.py.
//
// A frame's filtered stream, H rows of 1 + 3 W bytes, is cut into segments of whole rows (PNG_SEG_TARGET bytes or one row, whichever is
// more) that are compressed independently and become one IDAT chunk each.  Per call, every launch covering all frames:
//   filter    one wave per row: to8b's bytes, the five residual rows of the specification, the type with the smallest sum of
//             |residual as int8| (or the forced one), the filtered row into the workspace
//   deflate   one workgroup per segment: every thread takes a contiguous piece of the segment; runs of equal bytes become matches at
//             distance 1 (a literal, then lengths of 258, then the rest if it is 3 or more), a histogram in LDS, code lengths by one
//             lane (Huffman over a rank sort, limited to 15 / 7 bits), the dynamic-block header, an exclusive sum of the pieces' bits,
//             the codes OR-ed into the cleared slot of the segment; stored instead where that is no longer; Adler-32 pair of the segment
//   offsets   one workgroup per frame: exclusive sum of the chunk sizes, the segments' Adler pairs combined in order, signature,
//             IHDR, IEND and the frame's size
//   assemble  one workgroup per segment: length, 'IDAT', the zlib header in the first, the slot's bytes, the Adler-32 in the last, and
//             the CRC-32 of the chunk from the threads' pieces (crc(A B) = crc(A) x^(8 |B|) + crc(B) over GF(2))
// OR into cleared words and integer adds in LDS are the only atomics, and both commute: the same input gives the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/r2l_hip.h"
#include "r2l_host_util.h"
#include "r2l_to8b.h"

namespace {

typedef unsigned long long u64;

constexpr int PNG_MAX_DIM = 16384;            // a row of 1 + 3 W bytes then fits one stored block (65,535) with room to spare
constexpr int PNG_SEG_TARGET = 16384;         // filtered bytes of a segment: as many whole rows as fit, at least one
constexpr int PNG_THREADS = 256;
constexpr int PNG_NLL = 286;                  // literal / length symbols
constexpr int PNG_NCL = 19;                   // symbols of the code-length code
constexpr int PNG_NSYM = 288;                 // room in the tables
constexpr int PNG_HEAD_BYTES = 33;            // signature, IHDR
constexpr uint32_t PNG_ADLER = 65521u;
constexpr uint32_t PNG_POLY = 0xedb88320u;    // CRC-32, reflected: bit 31 is x^0

// ---- CRC-32 over GF(2): the byte table, and x^(2^k) mod P for the shift by a number of bytes ----
struct CrcTables {
    uint32_t byte[256];
    uint32_t x2n[32];
};
constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {      // a(x) b(x) mod P
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ PNG_POLY : b >> 1;
    }
    return p;
}
constexpr CrcTables crc_tables() {
    CrcTables t = {};
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ PNG_POLY : c >> 1;
        t.byte[i] = c;
    }
    uint32_t p = 1u << 30;      // x^1
    t.x2n[0] = p;
    for (int k = 1; k < 32; ++k) t.x2n[k] = p = crc_mul(p, p);
    return t;
}
__constant__ CrcTables d_crc = crc_tables();

// sizes of one frame, and where a stack's buffers lie in the workspace (bytes; every part 16-byte aligned)
struct Layout {
    int S, R, n_seg;                 // bytes of a filtered row, rows of a segment, segments of a frame
    long long frame_bytes, slot;     // H S; room of a segment's compressed bytes
    long long filt, slots, meta, off, adler, total;
};
struct SegMeta {
    uint32_t size, a, b, pad;        // compressed bytes; Adler pair of the segment's bytes from (0, 0)
};
long long up16(long long v) { return (v + 15) & ~15ll; }
Layout png_layout(int n_img, int H, int W) {
    Layout L;
    L.S = 1 + 3 * W;
    L.R = PNG_SEG_TARGET / L.S;
    if (L.R < 1) L.R = 1;
    if (L.R > H) L.R = H;
    L.n_seg = (H + L.R - 1) / L.R;
    L.frame_bytes = (long long)H * L.S;
    L.slot = up16((long long)L.R * L.S + 5) + 16;      // a segment is never written longer than stored; the last OR reaches 3 bytes further
    long long at = 0;
    auto take = [&at](long long bytes) {
        const long long here = at;
        at += up16(bytes);
        return here;
    };
    L.filt = take(n_img * L.frame_bytes);
    L.slots = take((long long)n_img * L.n_seg * L.slot);
    L.meta = take((long long)n_img * L.n_seg * (long long)sizeof(SegMeta));
    L.off = take((long long)n_img * L.n_seg * 8);
    L.adler = take(n_img * 4ll);
    L.total = at;
    return L;
}
// signature + IHDR + per segment (chunk 12 + stored header 5) + zlib header 2 + Adler 4 + IEND 12, and the filtered bytes themselves
long long png_max_frame(const Layout& L) { return PNG_HEAD_BYTES + 17ll * L.n_seg + 6 + 12 + L.frame_bytes; }

// ---------------------------------------------------------------------------------------------------------------------------------
__device__ inline int png_paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// x: the byte, a: the one a pixel to the left, b: above, c: above left (0 outside the image)
__device__ inline int png_residual(int type, int x, int a, int b, int c) {
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? ((a + b) >> 1) : png_paeth(a, b, c);
    return (x - pred) & 255;
}

__global__ __launch_bounds__(PNG_THREADS) void png_filter_kernel(const float* __restrict__ rgb, int H, int W, int filter,
                                                                 unsigned char* __restrict__ filt) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y = blockIdx.x * 4 + wave, n = 3 * W;
    const long long frame = blockIdx.y;
    if (y >= H) return;
    const float* row = rgb + (frame * H + y) * (long long)n;
    const float* up = y ? row - n : row;      // row 0 has zeros above, in every frame
    int type = filter;
    if (filter < 0) {
        uint32_t s[5] = {0, 0, 0, 0, 0};
        for (int i = lane; i < n; i += 64) {
            const int x = (int)r2l_to8b(row[i]), a = i >= 3 ? (int)r2l_to8b(row[i - 3]) : 0;
            const int b = y ? (int)r2l_to8b(up[i]) : 0, c = (y && i >= 3) ? (int)r2l_to8b(up[i - 3]) : 0;
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                const int r = png_residual(t, x, a, b, c);
                s[t] += (uint32_t)(r < 128 ? r : 256 - r);
            }
        }
        type = 0;
        uint32_t best = 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            uint32_t v = s[t];
#pragma unroll
            for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
            if (t == 0 || v < best) best = v, type = t;      // ties go to the lowest type
        }
    }
    unsigned char* o = filt + (frame * H + y) * (long long)(n + 1);
    if (lane == 0) o[0] = (unsigned char)type;
    for (int i = lane; i < n; i += 64) {
        const int x = (int)r2l_to8b(row[i]), a = i >= 3 ? (int)r2l_to8b(row[i - 3]) : 0;
        const int b = y ? (int)r2l_to8b(up[i]) : 0, c = (y && i >= 3) ? (int)r2l_to8b(up[i - 3]) : 0;
        o[1 + i] = (unsigned char)png_residual(type, x, a, b, c);
    }
}

// ---- deflate ----
// RFC 1951 3.2.5: the symbol of a match length 3 .. 258, and its extra bits
__device__ inline void png_length_symbol(int len, int& sym, int& ebits, int& eval) {
    const int l = len - 3;
    if (len == 258) {
        sym = 285, ebits = 0, eval = 0;
    } else if (l < 8) {
        sym = 257 + l, ebits = 0, eval = 0;
    } else {
        const int k = 31 - __clz(l);
        ebits = k - 2;
        sym = 257 + 4 * (k - 1) + ((l >> ebits) & 3);
        eval = l & ((1 << ebits) - 1);
    }
}
__device__ inline int png_length_extra_bits(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }

// The tokens of d[0 .. n) that start in [c0, c1), in order, into a sink.  A maximal run [s, e) of equal bytes is: a literal, then with
// M = e - s - 1 bytes left, M / 258 matches of 258 and, of the rest, one match if it is 3 or more, else literals.  first[t] / last[t]:
// the first / last position in thread t's piece where a run starts (n / -1: none); position 0 starts one.
template <class Sink>
__device__ inline void png_tokens(const unsigned char* d, int n, int c0, int c1, const int* first, const int* last, int tid, Sink& sink) {
    if (c0 >= c1) return;
    int s = c0;
    if (c0 > 0 && d[c0] == d[c0 - 1]) {
        int t = tid - 1;
        while (last[t] < 0) --t;      // ends at thread 0 at the latest
        s = last[t];
    }
    int i = c0;
    while (i < c1) {
        int e = i + 1;
        while (e < c1 && d[e] == d[e - 1]) ++e;
        if (e == c1 && c1 < n) {
            int t = tid + 1;
            while (t < PNG_THREADS && first[t] >= n) ++t;
            e = t < PNG_THREADS ? first[t] : n;
        }
        const int stop = e < c1 ? e : c1;
        const int M = e - s - 1, q = M / 258, r = M - q * 258;
        int p = i;
        while (p < stop) {
            if (p == s || M < 3) {
                sink.literal(d[p]);
                ++p;
                continue;
            }
            const int j = p - s - 1, blk = j / 258, within = j - blk * 258;
            if (blk < q) {
                if (within == 0) sink.match(258);
                p += 258 - within;
            } else if (r >= 3) {
                if (within == 0) sink.match(r);
                p += r - within;
            } else {
                sink.literal(d[p]);
                ++p;
            }
        }
        i = stop;
        s = e;
    }
}

struct HistSink {
    uint32_t* freq;      // [PNG_NLL] literal / length symbols, [PNG_NLL] the matches
    __device__ void literal(int b) { atomicAdd(freq + b, 1u); }
    __device__ void match(int len) {
        int sym, eb, ev;
        png_length_symbol(len, sym, eb, ev);
        atomicAdd(freq + sym, 1u);
        atomicAdd(freq + PNG_NLL, 1u);
    }
};
struct CountSink {
    const unsigned char* len;
    uint32_t bits = 0;
    __device__ void literal(int b) { bits += len[b]; }
    __device__ void match(int l) {
        int sym, eb, ev;
        png_length_symbol(l, sym, eb, ev);
        bits += (uint32_t)(len[sym] + eb + 1);      // the distance code is one bit
    }
};
// OR-s bits into a cleared buffer of little-endian 32-bit words, least significant bit first (RFC 1951 3.1.1); at most 16 bits per put
struct BitSink {
    uint32_t* buf;
    u64 acc = 0;
    int nb;
    uint32_t w;
    __device__ BitSink(uint32_t* b, uint32_t bitpos) : buf(b), nb((int)(bitpos & 31u)), w(bitpos >> 5) {}
    __device__ void put(uint32_t v, int bits) {
        acc |= (u64)v << nb;
        nb += bits;
        if (nb >= 32) {
            atomicOr(buf + w, (uint32_t)acc);
            ++w;
            acc >>= 32;
            nb -= 32;
        }
    }
    __device__ void finish() {
        if (nb && acc) atomicOr(buf + w, (uint32_t)acc);
    }
};
struct EmitSink {
    BitSink bits;
    const unsigned char* len;
    const uint16_t* code;      // bit-reversed: Huffman codes go most significant bit first
    __device__ EmitSink(uint32_t* b, uint32_t bitpos, const unsigned char* l, const uint16_t* c) : bits(b, bitpos), len(l), code(c) {}
    __device__ void literal(int b) { bits.put(code[b], len[b]); }
    __device__ void match(int l) {
        int sym, eb, ev;
        png_length_symbol(l, sym, eb, ev);
        bits.put(code[sym], len[sym]);
        bits.put((uint32_t)ev, eb + 1);      // the extra bits, then distance symbol 0: the one-bit code 0
    }
};

struct HuffScratch {
    uint32_t f[2 * PNG_NSYM];               // weights: leaves in ascending order, then the inner nodes as they are made
    uint16_t parent[2 * PNG_NSYM];
    uint16_t order[PNG_NSYM];               // the used symbols in ascending order of (frequency, symbol)
    uint16_t depth[2 * PNG_NSYM];
};

// Code lengths of the used symbols of freq[0 .. n), at most maxbits each, into len (0: unused); called by the whole workgroup.  The
// sort is a rank sort by all threads; one lane builds the Huffman tree from two queues, shortens what is deeper than maxbits until
// the Kraft sum is 1 again, and hands the lengths out by frequency.  Two or more used symbols give a complete code.
__device__ void png_code_lengths(const uint32_t* freq, int n, int maxbits, unsigned char* len, HuffScratch& h, int tid) {
    for (int s = tid; s < n; s += PNG_THREADS) {
        const uint32_t fs = freq[s];
        len[s] = 0;
        if (fs) {
            int rank = 0;
            for (int k = 0; k < n; ++k) {
                const uint32_t fk = freq[k];
                rank += (fk != 0u) && (fk < fs || (fk == fs && k < s));
            }
            h.order[rank] = (uint16_t)s;
            h.f[rank] = fs;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int m = 0;
        for (int k = 0; k < n; ++k) m += freq[k] != 0u;
        if (m == 1) {
            len[h.order[0]] = 1;
        } else if (m > 1) {
            int li = 0, ni = m;      // the next leaf, the next inner node not yet under a parent
            for (int nn = m; nn < 2 * m - 1; ++nn) {
                uint32_t sum = 0;
                for (int k = 0; k < 2; ++k) {
                    const bool leaf = li < m && (ni >= nn || h.f[li] <= h.f[ni]);
                    const int c = leaf ? li++ : ni++;
                    sum += h.f[c];
                    h.parent[c] = (uint16_t)nn;
                }
                h.f[nn] = sum;
            }
            int cnt[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            h.depth[2 * m - 2] = 0;
            for (int k = 2 * m - 3; k >= 0; --k) {      // a parent is made after its children
                const int dk = h.depth[h.parent[k]] + 1;
                h.depth[k] = (uint16_t)dk;
                if (k < m) ++cnt[dk < maxbits ? dk : maxbits];
            }
            uint32_t total = 0;
            for (int i = 1; i <= maxbits; ++i) total += (uint32_t)cnt[i] << (maxbits - i);
            while (total > (1u << maxbits)) {      // one code less at maxbits, its sibling-to-be moved down from the deepest shorter length
                --cnt[maxbits];
                for (int i = maxbits - 1; i > 0; --i)
                    if (cnt[i]) {
                        --cnt[i];
                        cnt[i + 1] += 2;
                        break;
                    }
                --total;
            }
            int j = m;      // the most frequent symbols take the shortest codes
            for (int i = 1; i <= maxbits; ++i)
                for (int l = cnt[i]; l > 0; --l) len[h.order[--j]] = (unsigned char)i;
        }
    }
    __syncthreads();
}

// canonical codes (RFC 1951 3.2.2), bit-reversed for the writer; one lane
__device__ void png_canonical(const unsigned char* len, int n, uint16_t* code) {
    int count[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < n; ++s) ++count[len[s]];
    count[0] = 0;
    uint32_t next[16];
    uint32_t c = 0;
    for (int b = 1; b < 16; ++b) next[b] = c = (c + (uint32_t)count[b - 1]) << 1;
    for (int s = 0; s < n; ++s) {
        const int l = len[s];
        code[s] = l ? (uint16_t)(__brev(next[l]++) >> (32 - l)) : (uint16_t)0;
    }
}

__constant__ unsigned char d_cl_order[PNG_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__global__ __launch_bounds__(PNG_THREADS) void png_deflate_kernel(const unsigned char* __restrict__ filt, int H, int S, int R, int n_seg,
                                                                  long long slot, unsigned char* __restrict__ slots, SegMeta* __restrict__ meta) {
    __shared__ __attribute__((aligned(16))) unsigned char s_data[PNG_SEG_TARGET];
    __shared__ uint32_t s_freq[PNG_NSYM];
    __shared__ unsigned char s_len[PNG_NSYM];
    __shared__ uint16_t s_code[PNG_NSYM];
    __shared__ uint32_t s_clfreq[PNG_NCL];
    __shared__ unsigned char s_cllen[PNG_NCL];
    __shared__ uint16_t s_clcode[PNG_NCL];
    __shared__ uint16_t s_cls[PNG_NSYM];      // the code lengths as symbols of the code-length code: symbol | extra value << 8
    __shared__ int s_first[PNG_THREADS], s_last[PNG_THREADS];
    __shared__ uint32_t s_a[PNG_THREADS], s_b[PNG_THREADS];
    __shared__ HuffScratch s_h;
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_ncls, s_nl, s_ncl, s_hdr_bits, s_all_bits, s_dynamic;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int seg = blockIdx.x;
    const long long frame = blockIdx.y;
    const int row0 = seg * R, rows = (H - row0 < R) ? H - row0 : R, n = rows * S;
    const bool final_seg = seg == n_seg - 1;
    const unsigned char* src = filt + (frame * H + row0) * (long long)S;
    const unsigned char* d = src;
    if (n <= PNG_SEG_TARGET) {
        for (int i = tid; i < n; i += PNG_THREADS) s_data[i] = src[i];
        d = s_data;
    }
    for (int s = tid; s < PNG_NSYM; s += PNG_THREADS) s_freq[s] = 0;
    if (tid < PNG_NCL) s_clfreq[tid] = 0;
    __syncthreads();

    // a thread's piece: ceil(n / 256) bytes, made an odd number of 32-bit words so that the threads of a wave start in different LDS banks
    const int piece = 4 * ((((n + PNG_THREADS - 1) / PNG_THREADS + 3) / 4) | 1);
    const int c0 = (long long)tid * piece < n ? tid * piece : n, c1 = c0 + piece < n ? c0 + piece : n;
    {
        int first = n, last = -1;
        uint32_t a = 0, b = 0;
        for (int i = c0; i < c1; ++i) {
            const uint32_t v = d[i];
            if (i == 0 || d[i - 1] != v) {
                if (first == n) first = i;
                last = i;
            }
            a += v;
            b += (uint32_t)(c1 - i) * v;      // a piece is at most 196 bytes: under 2^23
        }
        s_first[tid] = first, s_last[tid] = last, s_a[tid] = a, s_b[tid] = b;
    }
    __syncthreads();
    uint32_t* out = reinterpret_cast<uint32_t*>(slots + (frame * n_seg + seg) * slot);
    SegMeta* mt = meta + frame * n_seg + seg;
    if (tid == 64) {      // Adler-32 pair of the segment from (0, 0): the pieces in order, reduced at every step
        uint32_t A = 0, B = 0;
        for (int t = 0; t < PNG_THREADS; ++t) {
            const int t0 = (long long)t * piece < n ? t * piece : n, t1 = t0 + piece < n ? t0 + piece : n;
            B = (B + (uint32_t)(t1 - t0) * A + s_b[t]) % PNG_ADLER;
            A = (A + s_a[t]) % PNG_ADLER;
        }
        mt->a = A, mt->b = B, mt->pad = 0;
    }
    {
        HistSink hist{s_freq};
        png_tokens(d, n, c0, c1, s_first, s_last, tid, hist);
    }
    if (tid == 0) s_freq[256] = 1;      // end of block
    __syncthreads();
    const uint32_t n_match = s_freq[PNG_NLL];
    png_code_lengths(s_freq, PNG_NLL, 15, s_len, s_h, tid);
    if (tid == 0) {
        // HLIT code lengths and the one distance code (length 1, used or not: a complete-enough code for every decoder), as code-length
        // symbols: 0 .. 15 a length, 16 repeat the last 3 .. 6 times, 17 / 18 zeros 3 .. 10 / 11 .. 138 times
        int nl = PNG_NLL;
        while (nl > 257 && s_len[nl - 1] == 0) --nl;
        const int nc = nl + 1;
        int k = 0, i = 0;
        auto emit = [&](int sym, int extra) {
            s_cls[k++] = (uint16_t)(sym | (extra << 8));
            ++s_clfreq[sym];
        };
        while (i < nc) {
            const int v = i < nl ? s_len[i] : 1;
            int run = 1;
            while (i + run < nc && (i + run < nl ? s_len[i + run] : 1) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 3) {
                    const int r = run < 138 ? run : 138;
                    if (r <= 10) emit(17, r - 3);
                    else emit(18, r - 11);
                    run -= r;
                }
            } else {
                emit(v, 0);
                --run;
                while (run >= 3) {
                    const int r = run < 6 ? run : 6;
                    emit(16, r - 3);
                    run -= r;
                }
            }
            while (run-- > 0) emit(v, 0);
        }
        s_ncls = (uint32_t)k, s_nl = (uint32_t)nl;
    }
    __syncthreads();
    png_code_lengths(s_clfreq, PNG_NCL, 7, s_cllen, s_h, tid);
    if (tid == 0) {
        png_canonical(s_len, PNG_NLL, s_code);
        png_canonical(s_cllen, PNG_NCL, s_clcode);
        int ncl = PNG_NCL;
        while (ncl > 4 && s_cllen[d_cl_order[ncl - 1]] == 0) --ncl;
        uint32_t hdr = 3 + 5 + 5 + 4 + 3 * (uint32_t)ncl;
        for (int s = 0; s < PNG_NCL; ++s) hdr += s_clfreq[s] * (uint32_t)(s_cllen[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0));
        uint32_t body = n_match;      // the distance codes
        for (int s = 0; s < PNG_NLL; ++s) body += s_freq[s] * (uint32_t)(s_len[s] + (s > 256 ? png_length_extra_bits(s) : 0));
        const uint32_t all = hdr + body;      // at most 49,153 x 15 + the header: under 2^20
        // behind a block that is not the last: an empty stored block (3 bits, to the byte, 00 00 FF FF), so that the next segment starts on a byte
        const uint32_t bytes = final_seg ? (all + 7) / 8 : (all + 3 + 7) / 8 + 4;
        s_ncl = (uint32_t)ncl, s_hdr_bits = hdr, s_all_bits = all;
        s_dynamic = bytes < 5u + (uint32_t)n;
        mt->size = s_dynamic ? bytes : 5u + (uint32_t)n;
    }
    __syncthreads();
    if (!s_dynamic) {      // one stored block: n is under 65,536 (PNG_MAX_DIM)
        unsigned char* o = reinterpret_cast<unsigned char*>(out);
        if (tid == 0) {
            o[0] = final_seg ? 1 : 0;
            o[1] = (unsigned char)(n & 255), o[2] = (unsigned char)(n >> 8);
            o[3] = (unsigned char)(~n & 255), o[4] = (unsigned char)((~n >> 8) & 255);
        }
        for (int i = tid; i < n; i += PNG_THREADS) o[5 + i] = d[i];
        return;
    }
    const uint32_t all_bits = s_all_bits, hdr_bits = s_hdr_bits;
    const uint32_t n_bytes = final_seg ? (all_bits + 7) / 8 : (all_bits + 3 + 7) / 8 + 4;
    for (uint32_t wd = tid; wd < n_bytes / 4 + 2; wd += PNG_THREADS) out[wd] = 0u;      // the slot has 16 bytes beyond the stored size
    __threadfence();
    __syncthreads();
    // where each piece's bits start
    CountSink count{s_len};
    png_tokens(d, n, c0, c1, s_first, s_last, tid, count);
    uint32_t x = count.bits;
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) {
        const uint32_t yv = __shfl_up(x, dd, 64);
        if (lane >= dd) x += yv;
    }
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    uint32_t before = 0;
    for (int k = 0; k < wave; ++k) before += s_wave[k];
    const uint32_t at = hdr_bits + before + x - count.bits;
    if (tid == 0) {
        BitSink hb(out, 0);
        hb.put(final_seg ? 1u : 0u, 1);
        hb.put(2u, 2);
        hb.put(s_nl - 257u, 5);
        hb.put(0u, 5);
        hb.put(s_ncl - 4u, 4);
        for (uint32_t k = 0; k < s_ncl; ++k) hb.put(s_cllen[d_cl_order[k]], 3);
        for (uint32_t k = 0; k < s_ncls; ++k) {
            const int sym = s_cls[k] & 255, extra = s_cls[k] >> 8;
            hb.put(s_clcode[sym], s_cllen[sym]);
            if (sym >= 16) hb.put((uint32_t)extra, sym == 16 ? 2 : sym == 17 ? 3 : 7);
        }
        hb.finish();
        BitSink eob(out, all_bits - s_len[256]);
        eob.put(s_code[256], s_len[256]);
        eob.finish();
        if (!final_seg) {
            const uint32_t bp = (all_bits + 3 + 7) / 8 + 2;      // the FF FF of the empty stored block
            atomicOr(out + (bp >> 2), 0xFFu << (8 * (bp & 3)));
            atomicOr(out + ((bp + 1) >> 2), 0xFFu << (8 * ((bp + 1) & 3)));
        }
    }
    EmitSink em(out, at, s_len, s_code);
    png_tokens(d, n, c0, c1, s_first, s_last, tid, em);
    em.bits.finish();
}

__device__ inline uint32_t png_crc_bytes(const uint32_t* tab, uint32_t crc, unsigned char b) { return tab[(crc ^ b) & 255u] ^ (crc >> 8); }
__device__ inline uint32_t png_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ PNG_POLY : b >> 1;
    }
    return p;
}
// crc moved in front of n_bytes more bytes: times x^(8 n_bytes) mod P
__device__ inline uint32_t png_crc_shift(uint32_t crc, uint32_t n_bytes) {
    uint32_t p = 1u << 31;
    for (int k = 3; n_bytes; n_bytes >>= 1, ++k)
        if (n_bytes & 1u) p = png_crc_mul(d_crc.x2n[k & 31], p);
    return png_crc_mul(p, crc);
}
__device__ inline void png_put_be32(unsigned char* o, uint32_t v) {
    o[0] = (unsigned char)(v >> 24), o[1] = (unsigned char)(v >> 16), o[2] = (unsigned char)(v >> 8), o[3] = (unsigned char)v;
}
// bytes of the data of segment seg's IDAT chunk
__device__ inline long long png_chunk_data(const SegMeta* m, int seg, int n_seg) { return (seg == 0 ? 2 : 0) + (long long)m[seg].size + (seg == n_seg - 1 ? 4 : 0); }

// One workgroup per frame: where every IDAT chunk starts (exclusive sum of 12 + data bytes, a tile of 256 per round with a carry),
// Adler-32 of the frame, signature, IHDR, IEND, the size of the file.
__global__ __launch_bounds__(PNG_THREADS) void png_offsets_kernel(const SegMeta* __restrict__ meta, int H, int W, int S, int R, int n_seg,
                                                                  u64* __restrict__ off, uint32_t* __restrict__ adler,
                                                                  unsigned char* __restrict__ out, long long pitch, long long* __restrict__ sizes) {
    __shared__ u64 s_w[4];
    const long long frame = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const SegMeta* m = meta + frame * n_seg;
    u64 carry = PNG_HEAD_BYTES;
    for (int base = 0; base < n_seg; base += PNG_THREADS) {
        const int j = base + tid;
        const u64 v = j < n_seg ? (u64)(12 + png_chunk_data(m, j, n_seg)) : 0ull;
        u64 x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        u64 before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < wave) before += s_w[k];
            all += s_w[k];
        }
        if (j < n_seg) off[frame * n_seg + j] = carry + before + x - v;
        carry += all;
        __syncthreads();
    }
    unsigned char* o = out + frame * pitch;
    if (tid == 0) {
        const unsigned char head[PNG_HEAD_BYTES - 4] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R',
                                                        (unsigned char)(W >> 24), (unsigned char)(W >> 16), (unsigned char)(W >> 8), (unsigned char)W,
                                                        (unsigned char)(H >> 24), (unsigned char)(H >> 16), (unsigned char)(H >> 8), (unsigned char)H,
                                                        8, 2, 0, 0, 0};
        uint32_t crc = 0xFFFFFFFFu;
        for (int i = 0; i < PNG_HEAD_BYTES - 4; ++i) {
            o[i] = head[i];
            if (i >= 12) crc = png_crc_bytes(d_crc.byte, crc, head[i]);
        }
        png_put_be32(o + PNG_HEAD_BYTES - 4, ~crc);
        unsigned char* e = o + carry;
        const unsigned char iend[8] = {0, 0, 0, 0, 'I', 'E', 'N', 'D'};
        crc = 0xFFFFFFFFu;
        for (int i = 0; i < 8; ++i) {
            e[i] = iend[i];
            if (i >= 4) crc = png_crc_bytes(d_crc.byte, crc, iend[i]);
        }
        png_put_be32(e + 8, ~crc);
        sizes[frame] = (long long)carry + 12;
    }
    if (tid == 64) {      // the segments' pairs in order, from (1, 0): B' = B + n A + b, A' = A + a (mod 65,521)
        u64 A = 1, B = 0;
        for (int j = 0; j < n_seg; ++j) {
            const int rows = (H - j * R < R) ? H - j * R : R;
            B = (B + (u64)rows * S * A + m[j].b) % PNG_ADLER;
            A = (A + m[j].a) % PNG_ADLER;
        }
        adler[frame] = (uint32_t)(B << 16 | A);
    }
}

// One workgroup per segment: its IDAT chunk into the file.  The bytes under the CRC are 'IDAT' and the data; thread t copies and sums
// its piece of them, the sums are moved to the end of the chunk and added.
__global__ __launch_bounds__(PNG_THREADS) void png_assemble_kernel(const SegMeta* __restrict__ meta, int n_seg, long long slot,
                                                                   const unsigned char* __restrict__ slots, const u64* __restrict__ off,
                                                                   const uint32_t* __restrict__ adler, unsigned char* __restrict__ out, long long pitch) {
    __shared__ uint32_t s_tab[256];
    __shared__ uint32_t s_w[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int seg = blockIdx.x;
    const long long frame = blockIdx.y;
    s_tab[tid] = d_crc.byte[tid];
    __syncthreads();
    const SegMeta* m = meta + frame * n_seg;
    const unsigned char* src = slots + (frame * n_seg + seg) * slot;
    const uint32_t size = m[seg].size, lead = seg == 0 ? 2u : 0u, ad = adler[frame];
    const uint32_t n_data = (uint32_t)png_chunk_data(m, seg, n_seg), n_crc = n_data + 4;
    unsigned char* o = out + frame * pitch + off[frame * n_seg + seg];
    if (tid == 0) png_put_be32(o, n_data);
    const uint32_t piece = (n_crc + PNG_THREADS - 1) / PNG_THREADS;
    const uint32_t i0 = tid * piece < n_crc ? tid * piece : n_crc, i1 = i0 + piece < n_crc ? i0 + piece : n_crc;
    uint32_t crc = 0xFFFFFFFFu;
    for (uint32_t i = i0; i < i1; ++i) {
        unsigned char b;
        if (i < 4) b = (unsigned char)("IDAT"[i]);
        else if (i < 4 + lead) b = i == 4 ? 0x78 : 0x01;      // deflate, 32 KiB window; FCHECK makes 0x7801 a multiple of 31
        else if (i < 4 + lead + size) b = src[i - 4 - lead];
        else b = (unsigned char)(ad >> (8 * (3 - (i - 4 - lead - size))));
        o[4 + i] = b;
        crc = png_crc_bytes(s_tab, crc, b);
    }
    uint32_t part = i1 > i0 ? png_crc_shift(~crc, n_crc - i1) : 0u;
#pragma unroll
    for (int d = 32; d; d >>= 1) part ^= __shfl_xor(part, d, 64);
    if (lane == 0) s_w[wave] = part;
    __syncthreads();
    if (tid == 0) png_put_be32(o + 4 + n_crc, s_w[0] ^ s_w[1] ^ s_w[2] ^ s_w[3]);
}

int png_check_dims(const char* who, int H, int W) {
    if (H < 1 || W < 1 || H > PNG_MAX_DIM || W > PNG_MAX_DIM)
        return r2l_set_error(R2L_EINVAL, "%s: H=%d W=%d (1 .. %d each)", who, H, W, PNG_MAX_DIM);
    return R2L_OK;
}
int png_check_n(const char* who, int n_img) {
    if (n_img < 0 || n_img > 65535) return r2l_set_error(R2L_EINVAL, "%s: n_img = %d (0 .. 65535)", who, n_img);
    return R2L_OK;
}

}  // namespace

extern "C" {

long long r2l_png_max_frame_bytes(int H, int W) {
    int e = png_check_dims("r2l_png_max_frame_bytes", H, W);
    if (e) return e;
    return png_max_frame(png_layout(1, H, W));
}

long long r2l_png_workspace_bytes(int n_img, int H, int W) {
    int e = png_check_n("r2l_png_workspace_bytes", n_img);
    if (!e) e = png_check_dims("r2l_png_workspace_bytes", H, W);
    if (e) return e;
    return png_layout(n_img, H, W).total;
}

int r2l_png_layout(int H, int W, int* rows_per_segment, int* n_segments) {
    if (!rows_per_segment || !n_segments) return r2l_set_error(R2L_EINVAL, "r2l_png_layout: NULL argument");
    int e = png_check_dims("r2l_png_layout", H, W);
    if (e) return e;
    const Layout L = png_layout(1, H, W);
    *rows_per_segment = L.R, *n_segments = L.n_seg;
    return R2L_OK;
}

int r2l_png_encode(const float* rgb_dev, int n_img, int H, int W, int filter, void* workspace_dev, long long workspace_bytes,
                   unsigned char* out_dev, long long pitch, long long* sizes_dev, void* stream) {
    int e = png_check_n("r2l_png_encode", n_img);
    if (!e) e = png_check_dims("r2l_png_encode", H, W);
    if (e) return e;
    if (filter < -1 || filter > 4) return r2l_set_error(R2L_EINVAL, "r2l_png_encode: filter = %d (-1 adaptive, 0 .. 4 that type on every row)", filter);
    if (n_img == 0) return R2L_OK;
    if (!rgb_dev) return r2l_set_error(R2L_EINVAL, "r2l_png_encode: the frame stack is NULL");
    if (!workspace_dev || !out_dev || !sizes_dev) return r2l_set_error(R2L_EINVAL, "r2l_png_encode: workspace / out / sizes is NULL");
    const Layout L = png_layout(n_img, H, W);
    if (pitch < png_max_frame(L))
        return r2l_set_error(R2L_EINVAL, "r2l_png_encode: a pitch of %lld bytes, a %d x %d frame can take %lld (r2l_png_max_frame_bytes)", pitch, H, W,
                             png_max_frame(L));
    if (workspace_bytes < L.total)
        return r2l_set_error(R2L_EINVAL, "r2l_png_encode: a workspace of %lld bytes, %d frames of %d x %d need %lld (r2l_png_workspace_bytes)",
                             workspace_bytes, n_img, H, W, L.total);
    if (((uintptr_t)rgb_dev & 3) || ((uintptr_t)workspace_dev & 15) || ((uintptr_t)sizes_dev & 7))
        return r2l_set_error(R2L_EINVAL, "r2l_png_encode: alignment (frames 4, sizes 8, workspace 16 bytes)");
    e = r2l_require_gfx950(nullptr);
    if (e) return e;

    char* ws = (char*)workspace_dev;
    unsigned char* filt = (unsigned char*)(ws + L.filt);
    unsigned char* slots = (unsigned char*)(ws + L.slots);
    SegMeta* meta = (SegMeta*)(ws + L.meta);
    u64* off = (u64*)(ws + L.off);
    uint32_t* adler = (uint32_t*)(ws + L.adler);
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(PNG_THREADS), g_seg(L.n_seg, n_img);
    hipLaunchKernelGGL(png_filter_kernel, dim3((H + 3) / 4, n_img), blk, 0, s, rgb_dev, H, W, filter, filt);
    hipLaunchKernelGGL(png_deflate_kernel, g_seg, blk, 0, s, (const unsigned char*)filt, H, L.S, L.R, L.n_seg, L.slot, slots, meta);
    hipLaunchKernelGGL(png_offsets_kernel, dim3(n_img), blk, 0, s, (const SegMeta*)meta, H, W, L.S, L.R, L.n_seg, off, adler, out_dev, pitch, sizes_dev);
    hipLaunchKernelGGL(png_assemble_kernel, g_seg, blk, 0, s, (const SegMeta*)meta, L.n_seg, L.slot, (const unsigned char*)slots, (const u64*)off,
                       (const uint32_t*)adler, out_dev, pitch);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return r2l_set_error(R2L_EHIP, "r2l_png_encode launch: %s", hipGetErrorString(err));
    return R2L_OK;
}

}  // extern "C"
