// FLIP (Andersson et al., HPG 2020) of image pairs: FLIP.compute_flip of the reference's utils/flip_loss.py:70-130, the TestFLIP of
// its [TEST] lines, as three kernels per frame pair.  The reference applies fourteen dense 2-D filters (21 x 21 and 19 x 19 at the
// default viewing geometry, about 5.5 k MAC per pixel); every one of them is separable or a sum of two separable ones
// (efficient-nerf_amd/flip_taps.py says how), so the work here is two 1-D passes, about 0.6 k MAC per pixel:
//
//   flip_rows_kernel     one block = 2 rows x 128 pixels of ONE image (grid.z = a / b).  Loads the pixels with a halo of the CSF radius
//                        (columns clamped: replicate padding), maps them v = mul * (x - lo) + add, sRGB -> linear RGB -> XYZ -> YCxCz in
//                        registers, leaves Y, Cx, Cz and (Y + 16) / 116 in LDS, and writes the seven row-filtered planes
//                        A(Y), RG(Cx), BY1(Cz), BY2(Cz), D(yn), G(yn), P(yn) to the workspace.  The opponent image never reaches memory.
//   flip_cols_kernel     one block = a 64 x 32 tile of the pair.  Plane by plane it stages tile + halo rows (rows clamped) in one 16 KiB
//                        LDS buffer; a thread owns 8 consecutive rows of one column and slides down it, so an LDS read feeds 8 (or 16)
//                        FMAs: taps come from the kernel arguments through the scalar unit, padded with 7 zeros on both sides so that
//                        the slide needs no bounds test (sums that come out NaN are taken again over their own rows: 0 * NaN would
//                        carry a NaN pixel further than the reference's filters do).  Then the colour pipeline (clamped linear RGB ->
//                        L*a*b* -> Hunt -> HyAB ->
//                        redistribution), the feature pipeline and dE_c ^ (1 - dE_f) per pixel; a plain store into the map and one
//                        partial sum per block (fixed-order tree).
//   flip_mean_kernel     one block per frame adds the partials in a fixed order in float64: frame_mean.
//
// No atomics anywhere: the same inputs give the same bits, with or without a map.  Built with -ffp-contract=off like the rest of the
// library: every fusion is an explicit fmaf() (the filter sums), the colour arithmetic rounds once per operation of the reference.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/r2l_hip.h"
#include "r2l_host_util.h"

#define FLIP_MAX_R 16                    // the largest filter radius the tiles hold (efficient-nerf_amd/flip_taps.py MAX_RADIUS)
#define FLIP_PAD 7                       // zeros on both sides of a tap row: a thread's 8 outputs slide over it
#define FLIP_TAPS (2 * FLIP_MAX_R + 1 + 2 * FLIP_PAD + 1)      // 48
#define FLIP_ROW_W 128                   // flip_rows_kernel: pixels of a row per block ...
#define FLIP_ROW_H 2                     // ... and rows per block
#define FLIP_TILE_W 64                   // flip_cols_kernel: tile width ...
#define FLIP_TILE_H 32                   // ... and height = 4 thread rows x FLIP_PER_THREAD
#define FLIP_PER_THREAD 8
#define FLIP_MAX_DIM 32768

namespace {

enum { T_A = 0, T_RG, T_BY1, T_BY2, T_G, T_D, T_P, T_COUNT };     // tap rows; also the order of r2l_flip_taps' output
enum { P_A = 0, P_RG, P_BY1, P_BY2, P_D, P_G, P_P, P_COUNT };     // row-filtered planes of one image in the workspace

struct FlipParams {
    float taps[T_COUNT][FLIP_TAPS];      // row k: FLIP_PAD zeros, 2 r + 1 taps, zeros
    int rc, rf;                          // CSF radius, feature radius (rf <= rc)
    float m[9], minv[9], ill[3];         // linear RGB -> XYZ, its inverse, the reference illuminant (the matrix's row sums)
    float lo[2], mul[2], add[2];         // the affine map of image a / b
    float pccmax, k_lo, c_span, one_m_pt, pt;      // redistribute_errors
};

// torch.clamp(v, 0, 1): a NaN stays a NaN
__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

__device__ __forceinline__ void mat3(const float* __restrict__ m, float r, float g, float b, float& x, float& y, float& z) {
    x = m[0] * r + m[1] * g + m[2] * b;
    y = m[3] * r + m[4] * g + m[5] * b;
    z = m[6] * r + m[7] * g + m[8] * b;
}

__device__ __forceinline__ float srgb2lin(float c) {       // :305-311
    c = clamp01(c);
    return c > 0.04045f ? powf((c + 0.055f) / 1.055f, 2.4f) : c / 12.92f;
}

__device__ __forceinline__ float lab_f(float v) {          // :369-375
    return v > 0.00885f ? powf(v, (float)(1.0 / 3.0)) : v / (float)(3.0 * (6.0 / 29.0) * (6.0 / 29.0)) + (float)(4.0 / 29.0);
}

__global__ void __launch_bounds__(FLIP_ROW_W* FLIP_ROW_H)
    flip_rows_kernel(const float* __restrict__ img_a, const float* __restrict__ img_b, int H, int W, const FlipParams P, float* __restrict__ ws) {
    __shared__ float s_y[FLIP_ROW_H][FLIP_ROW_W + 2 * FLIP_MAX_R], s_cx[FLIP_ROW_H][FLIP_ROW_W + 2 * FLIP_MAX_R],
        s_cz[FLIP_ROW_H][FLIP_ROW_W + 2 * FLIP_MAX_R], s_yn[FLIP_ROW_H][FLIP_ROW_W + 2 * FLIP_MAX_R];
    const int which = blockIdx.z, ty = threadIdx.y, tx = threadIdx.x;
    const float* __restrict__ img = which ? img_b : img_a;
    const float lo = P.lo[which], mul = P.mul[which], add = P.add[which];
    const int rc = P.rc, rf = P.rf;
    const int x0 = blockIdx.x * FLIP_ROW_W, y = blockIdx.y * FLIP_ROW_H + ty;
    const int yy = y < H ? y : H - 1;
    for (int i = tx; i < FLIP_ROW_W + 2 * rc; i += FLIP_ROW_W) {
        int xx = x0 - rc + i;
        xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx);
        const float* __restrict__ p = img + ((size_t)yy * W + xx) * 3;
        const float r = srgb2lin(mul * (p[0] - lo) + add), g = srgb2lin(mul * (p[1] - lo) + add), b = srgb2lin(mul * (p[2] - lo) + add);
        float X, Y, Z;
        mat3(P.m, r, g, b, X, Y, Z);
        X = X / P.ill[0], Y = Y / P.ill[1], Z = Z / P.ill[2];      // :343-350
        const float yc = 116.0f * Y - 16.0f;
        s_y[ty][i] = yc;
        s_cx[ty][i] = 500.0f * (X - Y);
        s_cz[ty][i] = 200.0f * (Y - Z);
        s_yn[ty][i] = (yc + 16.0f) / 116.0f;                       // :108
    }
    __syncthreads();
    const int x = x0 + tx;
    if (x >= W || y >= H) return;
    float a = 0.f, rg = 0.f, by1 = 0.f, by2 = 0.f;
    for (int k = 0; k <= 2 * rc; ++k) {
        a = fmaf(P.taps[T_A][FLIP_PAD + k], s_y[ty][tx + k], a);
        rg = fmaf(P.taps[T_RG][FLIP_PAD + k], s_cx[ty][tx + k], rg);
        const float cz = s_cz[ty][tx + k];
        by1 = fmaf(P.taps[T_BY1][FLIP_PAD + k], cz, by1);
        by2 = fmaf(P.taps[T_BY2][FLIP_PAD + k], cz, by2);
    }
    float d = 0.f, g = 0.f, p = 0.f;
    const int off = tx + rc - rf;
    for (int k = 0; k <= 2 * rf; ++k) {
        const float v = s_yn[ty][off + k];
        d = fmaf(P.taps[T_D][FLIP_PAD + k], v, d);
        g = fmaf(P.taps[T_G][FLIP_PAD + k], v, g);
        p = fmaf(P.taps[T_P][FLIP_PAD + k], v, p);
    }
    const size_t hw = (size_t)H * W, at = (size_t)y * W + x;
    float* __restrict__ o = ws + (size_t)which * P_COUNT * hw + at;
    o[P_A * hw] = a;
    o[P_RG * hw] = rg;
    o[P_BY1 * hw] = by1;
    o[P_BY2 * hw] = by2;
    o[P_D * hw] = d;
    o[P_G * hw] = g;
    o[P_P * hw] = p;
}

// Column filter of one plane for the thread's FLIP_PER_THREAD rows: the tile and its halo rows go through LDS, then the thread slides
// down its column: row j of its window meets output o with tap j - o (zero outside the filter, by the padding).
template <int NF>
__device__ __forceinline__ void filter_column(float (*tile)[FLIP_TILE_W], const float* __restrict__ plane, int H, int W, int x0, int y0, int R,
                                              const float* __restrict__ t0, const float* __restrict__ t1, float (&acc0)[FLIP_PER_THREAD],
                                              float (&acc1)[FLIP_PER_THREAD]) {
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int xx = x0 + tx < W ? x0 + tx : W - 1;
    __syncthreads();                     // the previous plane's readers are through
    for (int l = ty; l < FLIP_TILE_H + 2 * R; l += 4) {
        int yy = y0 - R + l;
        yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
        tile[l][tx] = plane[(size_t)yy * W + xx];
    }
    __syncthreads();
#pragma unroll
    for (int o = 0; o < FLIP_PER_THREAD; ++o) acc0[o] = acc1[o] = 0.f;
    const int l0 = ty * FLIP_PER_THREAD;
    for (int j = 0; j < FLIP_PER_THREAD + 2 * R; ++j) {
        const float v = tile[l0 + j][tx];
#pragma unroll
        for (int o = 0; o < FLIP_PER_THREAD; ++o) {
            acc0[o] = fmaf(t0[FLIP_PAD + j - o], v, acc0[o]);
            if (NF == 2) acc1[o] = fmaf(t1[FLIP_PAD + j - o], v, acc1[o]);
        }
    }
    // 0 * NaN is NaN: a NaN in any row of the window has gone into all eight sums through the padding, also into those whose filter
    // does not reach that row, where the reference's dense filter leaves the pixel finite.  A sum that came out NaN is taken again
    // over its own rows o .. o + 2 R alone, in the same order.  Every row of the window meets every sum (with a tap or a zero), so
    // one sum is NaN exactly when all are: frames without a NaN pay one comparison per plane.
    if (acc0[0] != acc0[0]) {
#pragma unroll
        for (int o = 0; o < FLIP_PER_THREAD; ++o) {
            float s0 = 0.f, s1 = 0.f;
            for (int j = o; j <= o + 2 * R; ++j) {
                const float v = tile[l0 + j][tx];
                s0 = fmaf(t0[FLIP_PAD + j - o], v, s0);
                if (NF == 2) s1 = fmaf(t1[FLIP_PAD + j - o], v, s1);
            }
            acc0[o] = s0;
            if (NF == 2) acc1[o] = s1;
        }
    }
}

// what the metric needs of one image at the thread's pixels: Hunt-adjusted L*a*b* of the filtered colour, edge and point strength
struct FlipSide {
    float L[FLIP_PER_THREAD], a[FLIP_PER_THREAD], b[FLIP_PER_THREAD], edge[FLIP_PER_THREAD], point[FLIP_PER_THREAD];
};

__device__ __forceinline__ void flip_side(float (*tile)[FLIP_TILE_W], const float* __restrict__ planes, size_t hw, int H, int W, int x0, int y0,
                                          const FlipParams& P, FlipSide& s) {
    float A[FLIP_PER_THREAD], RG[FLIP_PER_THREAD], B1[FLIP_PER_THREAD], B2[FLIP_PER_THREAD], none[FLIP_PER_THREAD];
    filter_column<1>(tile, planes + P_A * hw, H, W, x0, y0, P.rc, P.taps[T_A], nullptr, A, none);
    filter_column<1>(tile, planes + P_RG * hw, H, W, x0, y0, P.rc, P.taps[T_RG], nullptr, RG, none);
    filter_column<1>(tile, planes + P_BY1 * hw, H, W, x0, y0, P.rc, P.taps[T_BY1], nullptr, B1, none);
    filter_column<1>(tile, planes + P_BY2 * hw, H, W, x0, y0, P.rc, P.taps[T_BY2], nullptr, B2, none);
#pragma unroll
    for (int o = 0; o < FLIP_PER_THREAD; ++o) {
        // ycxcz2linrgb, clamp to the RGB box (:216-221), linrgb2lab, Hunt (:224-236)
        const float y = (A[o] + 16.0f) / 116.0f, cx = RG[o] / 500.0f, cz = (B1[o] + B2[o]) / 200.0f;
        float r, g, b, X, Y, Z;
        mat3(P.minv, (y + cx) * P.ill[0], y * P.ill[1], (y - cz) * P.ill[2], r, g, b);
        mat3(P.m, clamp01(r), clamp01(g), clamp01(b), X, Y, Z);
        const float fx = lab_f(X / P.ill[0]), fy = lab_f(Y / P.ill[1]), fz = lab_f(Z / P.ill[2]);
        const float L = 116.0f * fy - 16.0f;
        s.L[o] = L;
        s.a[o] = (0.01f * L) * (500.0f * (fx - fy));
        s.b[o] = (0.01f * L) * (200.0f * (fy - fz));
    }
    // edge filter along x = d (x) g: D rows, G columns; along y: G rows, D columns.  The point filter likewise with p.
    float ex[FLIP_PER_THREAD], ey[FLIP_PER_THREAD], px[FLIP_PER_THREAD], py[FLIP_PER_THREAD];
    filter_column<1>(tile, planes + P_D * hw, H, W, x0, y0, P.rf, P.taps[T_G], nullptr, ex, none);
    filter_column<2>(tile, planes + P_G * hw, H, W, x0, y0, P.rf, P.taps[T_D], P.taps[T_P], ey, py);
    filter_column<1>(tile, planes + P_P * hw, H, W, x0, y0, P.rf, P.taps[T_G], nullptr, px, none);
#pragma unroll
    for (int o = 0; o < FLIP_PER_THREAD; ++o) {
        s.edge[o] = sqrtf(ex[o] * ex[o] + ey[o] * ey[o]);
        s.point[o] = sqrtf(px[o] * px[o] + py[o] * py[o]);
    }
}

__global__ void __launch_bounds__(256)
    flip_cols_kernel(const float* __restrict__ ws, int H, int W, const FlipParams P, float* __restrict__ map, float* __restrict__ partial) {
    __shared__ float tile[FLIP_TILE_H + 2 * FLIP_MAX_R][FLIP_TILE_W];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int x0 = blockIdx.x * FLIP_TILE_W, y0 = blockIdx.y * FLIP_TILE_H;
    const size_t hw = (size_t)H * W;
    FlipSide sa, sb;
    flip_side(tile, ws, hw, H, W, x0, y0, P, sa);
    flip_side(tile, ws + P_COUNT * hw, hw, H, W, x0, y0, P, sb);
    const int x = x0 + tx;
    float sum = 0.f;
#pragma unroll
    for (int o = 0; o < FLIP_PER_THREAD; ++o) {
        const int y = y0 + ty * FLIP_PER_THREAD + o;
        const float da = sa.a[o] - sb.a[o], db = sa.b[o] - sb.b[o];
        const float hyab = fabsf(sa.L[o] - sb.L[o]) + sqrtf(da * da + db * db);                      // :239-243
        const float pw = powf(hyab, 0.7f);
        const float dEc = pw < P.pccmax ? P.k_lo * pw : P.pt + ((pw - P.pccmax) / P.c_span) * P.one_m_pt;      // :246-256
        float dEf = fmaxf(fabsf(sa.edge[o] - sb.edge[o]), fabsf(sb.point[o] - sa.point[o]));        // :118-126
        dEf = clamp01(sqrtf((float)(1.0 / 1.4142135623730951) * dEf));
        const float v = powf(dEc, 1.0f - dEf);
        if (x < W && y < H) {
            if (map) map[(size_t)y * W + x] = v;
            sum += v;
        }
    }
    // the block's sum: a fixed tree over its 256 threads
    __syncthreads();
    float* red = &tile[0][0];
    const int t = ty * FLIP_TILE_W + tx;
    red[t] = sum;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if (t < step) red[t] += red[t + step];
        __syncthreads();
    }
    if (t == 0) partial[blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(256) flip_mean_kernel(const float* __restrict__ partial, int n, double count, float* __restrict__ out) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < n; i += 256) s += (double)partial[i];
    red[t] = s;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if (t < step) red[t] += red[t + step];
        __syncthreads();
    }
    if (t == 0) *out = (float)(red[0] / count);
}

// ---- host: radii, taps and constants, float64 throughout, rounded to float32 once ----
const double kPi = 3.14159265358979323846;

void flip_radii(double ppd, int* rc, int* rf) {
    // :167-170 (the largest scale parameter of the three CSFs is b1 of BY, 0.04) and :267-268 (w = 0.082)
    const double c = ceil(3.0 * sqrt(0.04 / (2.0 * kPi * kPi)) * ppd), f = ceil(3.0 * (0.5 * 0.082 * ppd));
    *rc = c > 1e6 ? 1000000 : (int)c;
    *rf = f > 1e6 ? 1000000 : (int)f;
}

// the 1-D factors of the five filters (efficient-nerf_amd/flip_taps.py restates this in numpy): out[k][i], i <= 2 r
void flip_build_taps(double ppd, int rc, int rf, double out[T_COUNT][2 * FLIP_MAX_R + 1]) {
    memset(out, 0, sizeof(double) * T_COUNT * (2 * FLIP_MAX_R + 1));
    const double a1[3] = {1.0, 1.0, 34.1}, b1[3] = {0.0047, 0.0053, 0.04}, a2 = 13.5, b2 = 0.025;      // A, RG, BY (:138-149); a2 of A, RG = 0
    double e1[2 * FLIP_MAX_R + 1], e2[2 * FLIP_MAX_R + 1];
    for (int c = 0; c < 3; ++c) {
        double s1 = 0.0, s2 = 0.0;
        for (int i = 0; i <= 2 * rc; ++i) {
            const double x = (i - rc) / ppd, z = x * x;
            e1[i] = exp(-kPi * kPi * z / b1[c]);
            e2[i] = exp(-kPi * kPi * z / b2);
            s1 += e1[i];
            s2 += e2[i];
        }
        if (c < 2) {
            for (int i = 0; i <= 2 * rc; ++i) out[c == 0 ? T_A : T_RG][i] = e1[i] / s1;
        } else {      // (w1 e1 (x) e1 + w2 e2 (x) e2) / S = t1 (x) t1 + t2 (x) t2
            const double w1 = a1[c] * sqrt(kPi / b1[c]), w2 = a2 * sqrt(kPi / b2), S = w1 * s1 * s1 + w2 * s2 * s2;
            for (int i = 0; i <= 2 * rc; ++i) {
                out[T_BY1][i] = sqrt(w1 / S) * e1[i];
                out[T_BY2][i] = sqrt(w2 / S) * e2[i];
            }
        }
    }
    const double sd = 0.5 * 0.082 * ppd;
    double sg = 0.0, dpos = 0.0, dneg = 0.0, ppos = 0.0, pneg = 0.0;
    double g[2 * FLIP_MAX_R + 1], d[2 * FLIP_MAX_R + 1], p[2 * FLIP_MAX_R + 1];
    for (int i = 0; i <= 2 * rf; ++i) {
        const double x = i - rf;
        g[i] = exp(-(x * x) / (2.0 * sd * sd));
        d[i] = -x * g[i];
        p[i] = (x * x / (sd * sd) - 1.0) * g[i];
        sg += g[i];
        if (d[i] > 0) dpos += d[i]; else if (d[i] < 0) dneg -= d[i];
        if (p[i] > 0) ppos += p[i]; else if (p[i] < 0) pneg -= p[i];
    }
    for (int i = 0; i <= 2 * rf; ++i) {      // positive weights sum to 1, negative ones to -1 (:282-287); the sign depends on x alone
        out[T_G][i] = g[i] / sg;
        out[T_D][i] = d[i] < 0 ? d[i] / dneg : d[i] / dpos;
        out[T_P][i] = p[i] < 0 ? p[i] / pneg : p[i] / ppos;
    }
}

void mat3d(const double* m, const double* v, double* o) {
    for (int r = 0; r < 3; ++r) o[r] = m[3 * r] * v[0] + m[3 * r + 1] * v[1] + m[3 * r + 2] * v[2];
}

double lab_fd(double v) { return v > 0.00885 ? pow(v, 1.0 / 3.0) : v / (3.0 * (6.0 / 29.0) * (6.0 / 29.0)) + 4.0 / 29.0; }

void hunt_lab(const double* m, const double* ill, const double* rgb, double* o) {
    double xyz[3];
    mat3d(m, rgb, xyz);
    const double fx = lab_fd(xyz[0] / ill[0]), fy = lab_fd(xyz[1] / ill[1]), fz = lab_fd(xyz[2] / ill[2]);
    o[0] = 116.0 * fy - 16.0;
    o[1] = 0.01 * o[0] * (500.0 * (fx - fy));
    o[2] = 0.01 * o[0] * (200.0 * (fy - fz));
}

void flip_fill_params(double ppd, int rc, int rf, FlipParams* P) {
    memset(P, 0, sizeof(*P));
    double taps[T_COUNT][2 * FLIP_MAX_R + 1];
    flip_build_taps(ppd, rc, rf, taps);
    for (int k = 0; k < T_COUNT; ++k)
        for (int i = 0; i <= 2 * (k < T_G ? rc : rf); ++i) P->taps[k][FLIP_PAD + i] = (float)taps[k][i];
    P->rc = rc;
    P->rf = rf;
    // :321-333, D65
    const double m[9] = {10135552.0 / 24577794.0, 8788810.0 / 24577794.0, 4435075.0 / 24577794.0, 2613072.0 / 12288897.0, 8788810.0 / 12288897.0,
                         887015.0 / 12288897.0,   1425312.0 / 73733382.0, 8788810.0 / 73733382.0, 70074185.0 / 73733382.0};
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    const double inv[9] = {(m[4] * m[8] - m[5] * m[7]) / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
                           (m[5] * m[6] - m[3] * m[8]) / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
                           (m[3] * m[7] - m[4] * m[6]) / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det};
    const double one[3] = {1.0, 1.0, 1.0}, green[3] = {0.0, 1.0, 0.0}, blue[3] = {0.0, 0.0, 1.0};
    double ill[3], lg[3], lb[3];
    mat3d(m, one, ill);
    for (int i = 0; i < 9; ++i) P->m[i] = (float)m[i], P->minv[i] = (float)inv[i];
    for (int i = 0; i < 3; ++i) P->ill[i] = (float)ill[i];
    // cmax: HyAB of Hunt-adjusted green against blue, to the power q_c (:93-102); p_c = 0.4, p_t = 0.95
    hunt_lab(m, ill, green, lg);
    hunt_lab(m, ill, blue, lb);
    const double cmax = pow(fabs(lg[0] - lb[0]) + sqrt((lg[1] - lb[1]) * (lg[1] - lb[1]) + (lg[2] - lb[2]) * (lg[2] - lb[2])), 0.7);
    const double pc = 0.4, pt = 0.95, pccmax = pc * cmax;
    P->pccmax = (float)pccmax;
    P->k_lo = (float)(pt / pccmax);
    P->c_span = (float)(cmax - pccmax);
    P->one_m_pt = (float)(1.0 - pt);
    P->pt = (float)pt;
}

int flip_check_ppd(double ppd, int* rc, int* rf) {
    if (!(ppd > 0.0) || !(ppd < 1e9)) return r2l_set_error(R2L_EINVAL, "r2l_flip: pixels_per_degree = %g", ppd);
    flip_radii(ppd, rc, rf);
    if (*rc > FLIP_MAX_R)
        return r2l_set_error(R2L_EINVAL, "r2l_flip: pixels_per_degree = %g needs a filter radius of %d, the kernels hold up to %d (pixels_per_degree <= %.2f)",
                             ppd, *rc, FLIP_MAX_R, floor(100.0 * FLIP_MAX_R / (3.0 * sqrt(0.04 / (2.0 * kPi * kPi)))) / 100.0);
    return R2L_OK;
}

long long flip_partials(int H, int W) {
    return (long long)((W + FLIP_TILE_W - 1) / FLIP_TILE_W) * ((H + FLIP_TILE_H - 1) / FLIP_TILE_H);
}

}  // namespace

extern "C" {

int r2l_flip_taps(double pixels_per_degree, float* taps_host, int* radius_csf, int* radius_feature) {
    int rc, rf;
    if (!taps_host || !radius_csf || !radius_feature) return r2l_set_error(R2L_EINVAL, "r2l_flip_taps: NULL argument");
    int e = flip_check_ppd(pixels_per_degree, &rc, &rf);
    if (e) return e;
    FlipParams P;
    flip_fill_params(pixels_per_degree, rc, rf, &P);
    for (int k = 0; k < T_COUNT; ++k)
        for (int i = 0; i < 2 * FLIP_MAX_R + 1; ++i) taps_host[k * (2 * FLIP_MAX_R + 1) + i] = P.taps[k][FLIP_PAD + i];
    *radius_csf = rc;
    *radius_feature = rf;
    return R2L_OK;
}

long long r2l_flip_workspace_floats(int H, int W, double pixels_per_degree) {
    int rc, rf;
    if (H < 1 || W < 1 || H > FLIP_MAX_DIM || W > FLIP_MAX_DIM)
        return r2l_set_error(R2L_EINVAL, "r2l_flip_workspace_floats: H=%d W=%d (1 .. %d each)", H, W, FLIP_MAX_DIM);
    int e = flip_check_ppd(pixels_per_degree, &rc, &rf);
    if (e) return e;
    return 2ll * P_COUNT * H * W + flip_partials(H, W);
}

int r2l_flip(const float* a_dev, const float* b_dev, int n_img, int H, int W, float a_lo, float a_mul, float a_add, float b_lo, float b_mul,
             float b_add, double pixels_per_degree, float* map_dev, float* frame_mean_dev, float* workspace_dev, long long workspace_floats,
             void* stream) {
    if (n_img < 0 || H < 1 || W < 1 || H > FLIP_MAX_DIM || W > FLIP_MAX_DIM)
        return r2l_set_error(R2L_EINVAL, "bad argument to r2l_flip (n_img=%d H=%d W=%d; H, W in 1 .. %d)", n_img, H, W, FLIP_MAX_DIM);
    int rc, rf;
    int e = flip_check_ppd(pixels_per_degree, &rc, &rf);
    if (e) return e;
    if (n_img == 0) return R2L_OK;
    if (!a_dev || !b_dev) return r2l_set_error(R2L_EINVAL, "r2l_flip: an image stack is NULL");
    if (!frame_mean_dev || !workspace_dev) return r2l_set_error(R2L_EINVAL, "r2l_flip: frame_mean / workspace is NULL");
    const long long need = 2ll * P_COUNT * H * W + flip_partials(H, W);
    if (workspace_floats < need)
        return r2l_set_error(R2L_EINVAL, "r2l_flip: a workspace of %lld floats, %d x %d needs %lld (r2l_flip_workspace_floats)", workspace_floats, H,
                             W, need);
    if (((uintptr_t)a_dev & 3) || ((uintptr_t)b_dev & 3) || ((uintptr_t)map_dev & 3) || ((uintptr_t)frame_mean_dev & 3) || ((uintptr_t)workspace_dev & 3))
        return r2l_set_error(R2L_EINVAL, "r2l_flip: every buffer must be 4-byte aligned");
    e = r2l_require_gfx950(nullptr);
    if (e) return e;
    FlipParams P;
    flip_fill_params(pixels_per_degree, rc, rf, &P);
    P.lo[0] = a_lo, P.mul[0] = a_mul, P.add[0] = a_add;
    P.lo[1] = b_lo, P.mul[1] = b_mul, P.add[1] = b_add;
    const size_t hw = (size_t)H * W;
    const int n_part = (int)flip_partials(H, W);
    float* partial = workspace_dev + 2 * P_COUNT * hw;
    const dim3 rows_grid((W + FLIP_ROW_W - 1) / FLIP_ROW_W, (H + FLIP_ROW_H - 1) / FLIP_ROW_H, 2), rows_block(FLIP_ROW_W, FLIP_ROW_H);
    const dim3 cols_grid((W + FLIP_TILE_W - 1) / FLIP_TILE_W, (H + FLIP_TILE_H - 1) / FLIP_TILE_H), cols_block(FLIP_TILE_W, 4);
    for (int k = 0; k < n_img; ++k) {      // frame after frame through one workspace: the stream orders them
        hipLaunchKernelGGL(flip_rows_kernel, rows_grid, rows_block, 0, (hipStream_t)stream, a_dev + k * hw * 3, b_dev + k * hw * 3, H, W, P, workspace_dev);
        hipLaunchKernelGGL(flip_cols_kernel, cols_grid, cols_block, 0, (hipStream_t)stream, (const float*)workspace_dev, H, W, P,
                           map_dev ? map_dev + k * hw : nullptr, partial);
        hipLaunchKernelGGL(flip_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, n_part, (double)hw, frame_mean_dev + k);
        hipError_t err = hipGetLastError();
        if (err != hipSuccess) return r2l_set_error(R2L_EHIP, "r2l_flip launch: %s", hipGetErrorString(err));
    }
    return R2L_OK;
}

}  // extern "C"
