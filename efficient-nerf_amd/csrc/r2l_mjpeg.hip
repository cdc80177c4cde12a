// Motion-JPEG: rendered frames to baseline JPEG files on the device (ITU-T T.81: sequential DCT, 8 bit, Huffman; JFIF colour space,
// 4:4:4, one interleaved scan, no restart markers), one C-ABI call per stack of frames.  The host side (video.py) wraps the files in
// an AVI container.
//
// Per call, every launch covering all frames (grid.y or grid.x = frame):
//   header   the file header, built on the host and passed by value, to the front of every frame's slot
//   dct      one wave per 8 x 8 block, one lane per pixel: to8b's byte, YCbCr, two 1-D DCT passes through LDS, quantiser, zig-zag
//   len      one thread per unit (block, component): the bits its Huffman code takes
//   scan     one workgroup per frame: exclusive sum of the units' bits, tile after tile with a carry
//   zero     clears the bytes of the raw scan that will be written
//   bits     one thread per unit: its code, OR-ed into the raw scan at its offset, most significant bit first
//   count    one thread per 16 bytes of the raw scan: how many are 0xFF
//   scan     the same kernel over those counts
//   stuff    one thread per 16 bytes: copies them behind the header with a 0x00 after every 0xFF; EOI and the frame's size
// OR into cleared words is the only atomic, and OR commutes: the same input gives the same bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/r2l_hip.h"
#include "r2l_host_util.h"
#include "r2l_to8b.h"

namespace {

typedef unsigned long long u64;

constexpr int MJPEG_MAX_DIM = 65535;          // SOF0 holds 16 bits each
constexpr int MJPEG_HEADER_BYTES = 623;       // SOI APP0 DQT DQT SOF0 DHT x 4 SOS
constexpr int MJPEG_UNIT_BYTES = 208;         // a unit's code is at most 22 (DC) + 63 x 26 (AC) = 1,660 bits
constexpr int MJPEG_SCAN_TILE = 1024;         // elements a workgroup of the scan takes per round (256 threads x 4)
constexpr int MJPEG_BLOCKS_PER_WG = 4;        // dct: one wave each

// T.81 Annex K.1 / K.2, natural (row-major) order
constexpr unsigned char kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                         69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
                                         81, 104, 113, 92, 49, 64, 78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
constexpr unsigned char kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                           99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                           99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// zig-zag position -> natural index (T.81 figure A.6)
constexpr unsigned char kZigZag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T.81 Annex K.3.3: BITS (codes per length 1 .. 16) and HUFFVAL of the four typical tables
constexpr unsigned char kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr unsigned char kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr unsigned char kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr unsigned char kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr unsigned char kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
constexpr unsigned char kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr unsigned char kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

// code tables the kernels read: entry[symbol] = code << 5 | length (T.81 Annex C: codes count up within a length, doubled between
// lengths).  Four tables of 256: DC luma, AC luma, DC chroma, AC chroma.
struct HuffCodes {
    uint32_t e[4][256];
};
constexpr void huff_fill(uint32_t* e, const unsigned char* bits, const unsigned char* vals) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) e[vals[k++]] = (code++ << 5) | (unsigned)len;
        code <<= 1;
    }
}
constexpr HuffCodes huff_codes() {
    HuffCodes h = {};
    huff_fill(h.e[0], kDcLumaBits, kDcVals);
    huff_fill(h.e[1], kAcLumaBits, kAcLumaVals);
    huff_fill(h.e[2], kDcChromaBits, kDcVals);
    huff_fill(h.e[3], kAcChromaBits, kAcChromaVals);
    return h;
}
__constant__ HuffCodes d_huff = huff_codes();
// natural index -> zig-zag position
struct ZigInv {
    unsigned char p[64];
};
constexpr ZigInv zig_inv() {
    ZigInv z = {};
    for (int i = 0; i < 64; ++i) z.p[kZigZag[i]] = (unsigned char)i;
    return z;
}
__constant__ ZigInv d_zig = zig_inv();

// what the dct kernel takes by value: c[u * 8 + x] = 1/2 C(u) cos((2x + 1) u pi / 16), so that F(u, v) = sum_y sum_x c[v][y] c[u][x] f(x, y)
// (T.81 A.3.3), and the two quantisers in natural order
struct DctParams {
    float c[64];
    float q[2][64];
};
struct HeaderBytes {
    unsigned char b[MJPEG_HEADER_BYTES + 1];
};

// libjpeg's quality rule on the Annex K tables, zig-zag order as DQT stores them
void mjpeg_tables(int quality, unsigned char* luma64, unsigned char* chroma64) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int l = (kBaseLuma[kZigZag[i]] * s + 50) / 100, c = (kBaseChroma[kZigZag[i]] * s + 50) / 100;
        luma64[i] = (unsigned char)(l < 1 ? 1 : l > 255 ? 255 : l);
        chroma64[i] = (unsigned char)(c < 1 ? 1 : c > 255 ? 255 : c);
    }
}

int mjpeg_header(int H, int W, int quality, unsigned char* out) {
    unsigned char* p = out;
    auto put = [&p](std::initializer_list<int> v) {
        for (int x : v) *p++ = (unsigned char)x;
    };
    unsigned char ql[64], qc[64];
    mjpeg_tables(quality, ql, qc);
    put({0xFF, 0xD8});
    put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});      // JFIF 1.01, aspect 1:1, no thumbnail
    for (int t = 0; t < 2; ++t) {
        put({0xFF, 0xDB, 0, 67, t});
        memcpy(p, t ? qc : ql, 64);
        p += 64;
    }
    put({0xFF, 0xC0, 0, 17, 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    const unsigned char* bits[4] = {kDcLumaBits, kAcLumaBits, kDcChromaBits, kAcChromaBits};
    const unsigned char* vals[4] = {kDcVals, kAcLumaVals, kDcVals, kAcChromaVals};
    const int ids[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; ++t) {
        const int n = (t & 1) ? 162 : 12;
        put({0xFF, 0xC4, (19 + n) >> 8, (19 + n) & 255, ids[t]});
        memcpy(p, bits[t], 16);
        memcpy(p + 16, vals[t], n);
        p += 16 + n;
    }
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return (int)(p - out);
}

// sizes of one frame, and where a stack's buffers lie in the workspace (bytes; every part 16-byte aligned)
struct Layout {
    long long n_blocks, n_units, raw_cap, n16;      // raw_cap: bytes of the raw (unstuffed) scan's slot; n16 = raw_cap / 16
    long long coef, len, off, raw, cnt, ffoff, bits, ffs, total;
};
long long up16(long long v) { return (v + 15) & ~15ll; }
Layout mjpeg_layout(int n_img, int H, int W) {
    Layout L;
    L.n_blocks = (long long)((H + 7) / 8) * ((W + 7) / 8);
    L.n_units = 3 * L.n_blocks;
    L.raw_cap = up16(L.n_units * MJPEG_UNIT_BYTES) + 16;
    L.n16 = L.raw_cap / 16;
    long long at = 0;
    auto take = [&at](long long bytes) {
        const long long here = at;
        at += up16(bytes);
        return here;
    };
    L.coef = take(n_img * L.n_units * 128);
    L.len = take(n_img * L.n_units * 4);
    L.off = take(n_img * L.n_units * 8);
    L.raw = take(n_img * L.raw_cap);
    L.cnt = take(n_img * L.n16 * 4);
    L.ffoff = take(n_img * L.n16 * 8);
    L.bits = take(n_img * 8ll);
    L.ffs = take(n_img * 8ll);
    L.total = at;
    return L;
}
long long mjpeg_max_frame(const Layout& L) { return MJPEG_HEADER_BYTES + 2 * L.n_units * MJPEG_UNIT_BYTES + 2; }

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mjpeg_header_kernel(HeaderBytes hb, unsigned char* out, long long pitch) {
    unsigned char* o = out + blockIdx.x * pitch;
    for (int i = threadIdx.x; i < MJPEG_HEADER_BYTES; i += 256) o[i] = hb.b[i];
}

__global__ __launch_bounds__(256) void mjpeg_dct_kernel(const float* __restrict__ rgb, int H, int W, int bw, long long n_blocks, DctParams P,
                                                        short* __restrict__ coef) {
    __shared__ float s_c[64], s_q[2][64];
    __shared__ float s_f[MJPEG_BLOCKS_PER_WG][3][64], s_t[MJPEG_BLOCKS_PER_WG][3][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < 64) s_c[tid] = P.c[tid];
    else if (tid < 192) s_q[(tid - 64) >> 6][tid & 63] = P.q[(tid - 64) >> 6][tid & 63];
    const long long frame = blockIdx.y, b = (long long)blockIdx.x * MJPEG_BLOCKS_PER_WG + wave;
    const bool valid = b < n_blocks;
    const int r8 = lane >> 3, c8 = lane & 7;
    if (valid) {
        const int by = (int)(b / bw), bx = (int)(b % bw);
        const int y = min(by * 8 + r8, H - 1), x = min(bx * 8 + c8, W - 1);      // replicate the last row and column
        const float* p = rgb + ((frame * H + y) * W + x) * 3;
        const float R = r2l_to8b(p[0]), G = r2l_to8b(p[1]), B = r2l_to8b(p[2]);
        s_f[wave][0][lane] = 0.299f * R + 0.587f * G + 0.114f * B - 128.0f;
        s_f[wave][1][lane] = -0.168736f * R - 0.331264f * G + 0.5f * B;
        s_f[wave][2][lane] = 0.5f * R - 0.418688f * G - 0.081312f * B;
    }
    __syncthreads();
    if (valid) {      // along x: lane (y, u)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float t = 0.0f;
#pragma unroll
            for (int x = 0; x < 8; ++x) t = fmaf(s_c[c8 * 8 + x], s_f[wave][c][r8 * 8 + x], t);
            s_t[wave][c][lane] = t;
        }
    }
    __syncthreads();
    if (valid) {      // along y: lane (v, u) = natural index v * 8 + u
        const int zz = d_zig.p[lane];
        short* o = coef + ((frame * n_blocks + b) * 3) * 64;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float F = 0.0f;
#pragma unroll
            for (int y = 0; y < 8; ++y) F = fmaf(s_c[r8 * 8 + y], s_t[wave][c][y * 8 + c8], F);
            float v = rintf(F / s_q[c ? 1 : 0][lane]);
            if (lane) v = fminf(fmaxf(v, -1023.0f), 1023.0f);
            o[c * 64 + zz] = (short)(int)v;
        }
    }
}

// A unit's Huffman code, symbol after symbol, into a sink: T.81 F.1.2.  The 64 coefficients stream through eight 16-byte loads;
// nothing is indexed by a run-time value but the code tables.
template <class Sink>
__device__ inline void mjpeg_code_unit(const short* __restrict__ c, int pred, int chroma, Sink& sink) {
    const uint32_t* dc = d_huff.e[chroma ? 2 : 0];
    const uint32_t* ac = d_huff.e[chroma ? 3 : 1];
    int run = 0;
    const uint4* q = reinterpret_cast<const uint4*>(c);
#pragma unroll 1
    for (int j = 0; j < 8; ++j) {
        const uint4 w = q[j];
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int v = (int)(short)(ws[i >> 1] >> ((i & 1) * 16));
            const bool is_dc = (j == 0 && i == 0);
            if (is_dc) v -= pred;
            if (v == 0 && !is_dc) {
                ++run;
                continue;
            }
            const int a = v < 0 ? -v : v;
            const int cat = a ? 32 - __clz(a) : 0;
            const uint32_t extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u);
            uint32_t e;
            if (is_dc) {
                e = dc[cat];
            } else {
                while (run >= 16) {
                    const uint32_t z = ac[0xF0];
                    sink.put(z >> 5, (int)(z & 31));
                    run -= 16;
                }
                e = ac[(run << 4) | cat];
                run = 0;
            }
            sink.put(((e >> 5) << cat) | extra, (int)(e & 31) + cat);
        }
    }
    if (run) {
        const uint32_t z = ac[0x00];
        sink.put(z >> 5, (int)(z & 31));
    }
}

struct LenSink {
    uint32_t n = 0;
    __device__ void put(uint32_t, int bits) { n += (uint32_t)bits; }
};
// OR-s bits into a cleared buffer of big-endian 32-bit words; at most 26 bits per put
struct BitSink {
    uint32_t* buf;
    u64 w, acc;
    int nb;
    __device__ BitSink(uint32_t* b, u64 bitpos) : buf(b), w(bitpos >> 5), acc(0), nb((int)(bitpos & 31)) {}
    __device__ void put(uint32_t v, int bits) {
        acc = (acc << bits) | v;
        nb += bits;
        if (nb >= 32) {
            nb -= 32;
            atomicOr(buf + w, __builtin_bswap32((uint32_t)(acc >> nb)));
            ++w;
            acc &= (1ull << nb) - 1ull;
        }
    }
    __device__ void finish() {
        if (nb) atomicOr(buf + w, __builtin_bswap32((uint32_t)(acc << (32 - nb))));
    }
};

__device__ inline int mjpeg_pred(const short* coef_frame, long long u) { return u >= 3 ? coef_frame[(u - 3) * 64] : 0; }

__global__ __launch_bounds__(256) void mjpeg_len_kernel(const short* __restrict__ coef, long long n_units, uint32_t* __restrict__ len) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x, frame = blockIdx.y;
    if (u >= n_units) return;
    const short* cf = coef + frame * n_units * 64;
    LenSink s;
    mjpeg_code_unit(cf + u * 64, mjpeg_pred(cf, u), (int)(u % 3) != 0, s);
    len[frame * n_units + u] = s.n;
}

// Exclusive sums of in[frame * stride + 0 .. n) into out, the sum of all into total[frame]; one workgroup per frame, a tile of
// MJPEG_SCAN_TILE per round.  n = n_fixed, or with bits_dev the 16-byte groups of a raw scan of bits_dev[frame] bits.
__global__ __launch_bounds__(256) void mjpeg_scan_kernel(const uint32_t* __restrict__ in, u64* __restrict__ out, long long stride, long long n_fixed,
                                                         const u64* __restrict__ bits_dev, u64* __restrict__ total) {
    __shared__ u64 s_w[4];
    const long long frame = blockIdx.x;
    in += frame * stride;
    out += frame * stride;
    const long long n = bits_dev ? (long long)((((bits_dev[frame] + 7) >> 3) + 15) >> 4) : n_fixed;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    u64 carry = 0;
    for (long long base = 0; base < n; base += MJPEG_SCAN_TILE) {
        const long long i0 = base + tid * 4;
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i0 + j < n ? in[i0 + j] : 0u;
        const u64 s = (u64)v[0] + v[1] + v[2] + v[3];
        u64 x = s;
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
        u64 e = carry + before + x - s;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j < n) out[i0 + j] = e;
            e += v[j];
        }
        carry += all;
        __syncthreads();
    }
    if (tid == 0) total[frame] = carry;
}

// clears the 16-byte groups of the raw scan that the bits kernel can reach: those of ceil(bits / 8) bytes, and one more
__global__ __launch_bounds__(256) void mjpeg_zero_kernel(unsigned char* __restrict__ raw, long long raw_cap, const u64* __restrict__ bits_dev) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x, frame = blockIdx.y;
    const long long n = (long long)((((bits_dev[frame] + 7) >> 3) + 15) >> 4) + 1;
    if (t < n && (t + 1) * 16 <= raw_cap) reinterpret_cast<uint4*>(raw + frame * raw_cap)[t] = make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(256) void mjpeg_bits_kernel(const short* __restrict__ coef, long long n_units, const uint32_t* __restrict__ len,
                                                         const u64* __restrict__ off, unsigned char* __restrict__ raw, long long raw_cap) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x, frame = blockIdx.y;
    if (u >= n_units) return;
    const short* cf = coef + frame * n_units * 64;
    const u64 at = off[frame * n_units + u];
    BitSink s(reinterpret_cast<uint32_t*>(raw + frame * raw_cap), at);
    mjpeg_code_unit(cf + u * 64, mjpeg_pred(cf, u), (int)(u % 3) != 0, s);
    if (u == n_units - 1) {      // the last byte is filled up with ones
        const int pad = (int)((8 - ((at + len[frame * n_units + u]) & 7)) & 7);
        if (pad) s.put((1u << pad) - 1u, pad);
    }
    s.finish();
}

__global__ __launch_bounds__(256) void mjpeg_count_kernel(const unsigned char* __restrict__ raw, long long raw_cap, const u64* __restrict__ bits_dev,
                                                          uint32_t* __restrict__ cnt) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x, frame = blockIdx.y;
    const long long n_bytes = (long long)((bits_dev[frame] + 7) >> 3);
    if (t * 16 >= n_bytes) return;
    const uint4 w = reinterpret_cast<const uint4*>(raw + frame * raw_cap)[t];      // bytes past n_bytes in this group are 0
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) c += ((ws[i >> 2] >> ((i & 3) * 8)) & 255u) == 255u;
    cnt[frame * (raw_cap / 16) + t] = c;
}

__global__ __launch_bounds__(256) void mjpeg_stuff_kernel(const unsigned char* __restrict__ raw, long long raw_cap, const u64* __restrict__ bits_dev,
                                                          const u64* __restrict__ ffoff, const u64* __restrict__ ffs, unsigned char* __restrict__ out,
                                                          long long pitch, long long* __restrict__ sizes) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x, frame = blockIdx.y;
    const long long n_bytes = (long long)((bits_dev[frame] + 7) >> 3);
    unsigned char* o = out + frame * pitch + MJPEG_HEADER_BYTES;
    if (t == 0) {
        const long long end = n_bytes + (long long)ffs[frame];
        o[end] = 0xFF;
        o[end + 1] = 0xD9;
        sizes[frame] = MJPEG_HEADER_BYTES + end + 2;
    }
    if (t * 16 >= n_bytes) return;
    const uint4 w = reinterpret_cast<const uint4*>(raw + frame * raw_cap)[t];
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
    long long at = t * 16 + (long long)ffoff[frame * (raw_cap / 16) + t];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (t * 16 + i < n_bytes) {
            const unsigned char b = (unsigned char)(ws[i >> 2] >> ((i & 3) * 8));
            o[at++] = b;
            if (b == 0xFF) o[at++] = 0;
        }
    }
}

int mjpeg_check_dims(const char* who, int H, int W) {
    if (H < 1 || W < 1 || H > MJPEG_MAX_DIM || W > MJPEG_MAX_DIM)
        return r2l_set_error(R2L_EINVAL, "%s: H=%d W=%d (1 .. %d each)", who, H, W, MJPEG_MAX_DIM);
    return R2L_OK;
}
int mjpeg_check_quality(const char* who, int quality) {
    if (quality < 1 || quality > 100) return r2l_set_error(R2L_EINVAL, "%s: quality = %d (1 .. 100)", who, quality);
    return R2L_OK;
}

}  // namespace

extern "C" {

int r2l_mjpeg_tables(int quality, unsigned char* luma64, unsigned char* chroma64) {
    if (!luma64 || !chroma64) return r2l_set_error(R2L_EINVAL, "r2l_mjpeg_tables: NULL argument");
    int e = mjpeg_check_quality("r2l_mjpeg_tables", quality);
    if (e) return e;
    mjpeg_tables(quality, luma64, chroma64);
    return R2L_OK;
}

long long r2l_mjpeg_header(int H, int W, int quality, unsigned char* out_host, long long cap) {
    if (!out_host) return r2l_set_error(R2L_EINVAL, "r2l_mjpeg_header: NULL argument");
    int e = mjpeg_check_dims("r2l_mjpeg_header", H, W);
    if (!e) e = mjpeg_check_quality("r2l_mjpeg_header", quality);
    if (e) return e;
    if (cap < MJPEG_HEADER_BYTES) return r2l_set_error(R2L_EINVAL, "r2l_mjpeg_header: room for %lld bytes, the header takes %d", cap, MJPEG_HEADER_BYTES);
    return mjpeg_header(H, W, quality, out_host);
}

long long r2l_mjpeg_workspace_bytes(int n_img, int H, int W) {
    if (n_img < 0 || n_img > 65535) return r2l_set_error(R2L_EINVAL, "r2l_mjpeg_workspace_bytes: n_img = %d (0 .. 65535)", n_img);
    int e = mjpeg_check_dims("r2l_mjpeg_workspace_bytes", H, W);
    if (e) return e;
    return mjpeg_layout(n_img, H, W).total;
}

long long r2l_mjpeg_max_frame_bytes(int H, int W) {
    int e = mjpeg_check_dims("r2l_mjpeg_max_frame_bytes", H, W);
    if (e) return e;
    return mjpeg_max_frame(mjpeg_layout(1, H, W));
}

int r2l_mjpeg_encode(const float* rgb_dev, int n_img, int H, int W, int quality, void* workspace_dev, long long workspace_bytes,
                     unsigned char* out_dev, long long out_pitch, long long* sizes_dev, short* coef_dev, void* stream) {
    if (n_img < 0 || n_img > 65535) return r2l_set_error(R2L_EINVAL, "r2l_mjpeg_encode: n_img = %d (0 .. 65535)", n_img);
    int e = mjpeg_check_dims("r2l_mjpeg_encode", H, W);
    if (!e) e = mjpeg_check_quality("r2l_mjpeg_encode", quality);
    if (e) return e;
    if (n_img == 0) return R2L_OK;
    if (!rgb_dev) return r2l_set_error(R2L_EINVAL, "r2l_mjpeg_encode: the frame stack is NULL");
    if (!workspace_dev || !out_dev || !sizes_dev) return r2l_set_error(R2L_EINVAL, "r2l_mjpeg_encode: workspace / out / sizes is NULL");
    const Layout L = mjpeg_layout(n_img, H, W);
    if (out_pitch < mjpeg_max_frame(L))
        return r2l_set_error(R2L_EINVAL, "r2l_mjpeg_encode: a pitch of %lld bytes, a %d x %d frame can take %lld (r2l_mjpeg_max_frame_bytes)", out_pitch,
                             H, W, mjpeg_max_frame(L));
    if (workspace_bytes < L.total)
        return r2l_set_error(R2L_EINVAL, "r2l_mjpeg_encode: a workspace of %lld bytes, %d frames of %d x %d need %lld (r2l_mjpeg_workspace_bytes)",
                             workspace_bytes, n_img, H, W, L.total);
    if (((uintptr_t)rgb_dev & 3) || ((uintptr_t)workspace_dev & 15) || ((uintptr_t)sizes_dev & 7) || ((uintptr_t)coef_dev & 15))
        return r2l_set_error(R2L_EINVAL, "r2l_mjpeg_encode: alignment (frames 4, sizes 8, workspace and coefficients 16 bytes)");
    e = r2l_require_gfx950(nullptr);
    if (e) return e;

    DctParams P;
    const double pi = 3.14159265358979323846;
    for (int u = 0; u < 8; ++u)
        for (int x = 0; x < 8; ++x) P.c[u * 8 + x] = (float)(0.5 * (u ? 1.0 : sqrt(0.5)) * cos((2 * x + 1) * u * pi / 16.0));
    unsigned char ql[64], qc[64];
    mjpeg_tables(quality, ql, qc);
    for (int i = 0; i < 64; ++i) P.q[0][kZigZag[i]] = ql[i], P.q[1][kZigZag[i]] = qc[i];
    HeaderBytes hb;
    mjpeg_header(H, W, quality, hb.b);

    char* ws = (char*)workspace_dev;
    short* coef = coef_dev ? coef_dev : (short*)(ws + L.coef);
    uint32_t* len = (uint32_t*)(ws + L.len);
    u64* off = (u64*)(ws + L.off);
    unsigned char* raw = (unsigned char*)(ws + L.raw);
    uint32_t* cnt = (uint32_t*)(ws + L.cnt);
    u64* ffoff = (u64*)(ws + L.ffoff);
    u64* bits = (u64*)(ws + L.bits);
    u64* ffs = (u64*)(ws + L.ffs);
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(256);
    const dim3 g_units((unsigned)((L.n_units + 255) / 256), n_img), g_raw((unsigned)((L.n16 + 255) / 256), n_img);
    hipLaunchKernelGGL(mjpeg_header_kernel, dim3(n_img), blk, 0, s, hb, out_dev, out_pitch);
    hipLaunchKernelGGL(mjpeg_dct_kernel, dim3((unsigned)((L.n_blocks + MJPEG_BLOCKS_PER_WG - 1) / MJPEG_BLOCKS_PER_WG), n_img), blk, 0, s, rgb_dev, H, W,
                       (W + 7) / 8, L.n_blocks, P, coef);
    hipLaunchKernelGGL(mjpeg_len_kernel, g_units, blk, 0, s, (const short*)coef, L.n_units, len);
    hipLaunchKernelGGL(mjpeg_scan_kernel, dim3(n_img), blk, 0, s, (const uint32_t*)len, off, L.n_units, L.n_units, (const u64*)nullptr, bits);
    hipLaunchKernelGGL(mjpeg_zero_kernel, g_raw, blk, 0, s, raw, L.raw_cap, (const u64*)bits);
    hipLaunchKernelGGL(mjpeg_bits_kernel, g_units, blk, 0, s, (const short*)coef, L.n_units, (const uint32_t*)len, (const u64*)off, raw, L.raw_cap);
    hipLaunchKernelGGL(mjpeg_count_kernel, g_raw, blk, 0, s, (const unsigned char*)raw, L.raw_cap, (const u64*)bits, cnt);
    hipLaunchKernelGGL(mjpeg_scan_kernel, dim3(n_img), blk, 0, s, (const uint32_t*)cnt, ffoff, L.n16, 0ll, (const u64*)bits, ffs);
    hipLaunchKernelGGL(mjpeg_stuff_kernel, g_raw, blk, 0, s, (const unsigned char*)raw, L.raw_cap, (const u64*)bits, (const u64*)ffoff, (const u64*)ffs,
                       out_dev, out_pitch, sizes_dev);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return r2l_set_error(R2L_EHIP, "r2l_mjpeg_encode launch: %s", hipGetErrorString(err));
    return R2L_OK;
}

}  // extern "C"
