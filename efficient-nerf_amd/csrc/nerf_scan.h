// The arithmetic of the teacher's volume-rendering scan, stated once (device code only): raw2outputs (main.py:556-621),
// sample_pdf (utils/run_nerf_raybased_helpers.py:283-330) and the sort of cat(z, samples) (main.py:730-732) as functions of ONE
// wave that owns ONE ray.  The stand-alone kernels, the fused coarse launch (nerf_kernels.hip) and the backward pass of the scan
// (nerf_train.hip) are the per-ray pointer set-up plus calls of these, so the fused launch equals the three launches and the
// backward recomputes the forward's alpha by construction.  Row pointers may be HBM or LDS: every function is inlined and the
// address space is the caller's.  The float / double orders are the reference's (torch on the CPU for sample_pdf); the build's
// -ffp-contract=off keeps one rounding per operation.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- wave helpers (64 lanes) -----------------------------------------------------------------------------------------------------
// a double through a 32-bit shuffle, half by half
template <class Shfl>
__device__ __forceinline__ double wave_shfl_f64(double v, Shfl shfl) {
    const int lo = shfl(__double2loint(v)), hi = shfl(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double shfl_up_f64(double v, int delta) { return wave_shfl_f64(v, [=](int x) { return __shfl_up(x, delta, 64); }); }
__device__ __forceinline__ double shfl_down_f64(double v, int delta) { return wave_shfl_f64(v, [=](int x) { return __shfl_down(x, delta, 64); }); }
__device__ __forceinline__ double shfl_xor_f64(double v, int mask) { return wave_shfl_f64(v, [=](int x) { return __shfl_xor(x, mask, 64); }); }
__device__ __forceinline__ double shfl_f64(double v, int src) { return wave_shfl_f64(v, [=](int x) { return __shfl(x, src, 64); }); }
// inclusive product / sum scans across the wave in double precision (torch's CPU cumprod / cumsum accumulate float tensors in
// double and round each output to float)
__device__ __forceinline__ double wave_scan_mul(double v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        double u = shfl_up_f64(v, d);
        if (lane >= d) v *= u;
    }
    return v;
}
__device__ __forceinline__ double wave_scan_add(double v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        double u = shfl_up_f64(v, d);
        if (lane >= d) v += u;
    }
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += shfl_xor_f64(v, m);
    return v;
}
// what one lane wrote to an LDS row, every lane of the wave may read behind this
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// ---- raw2outputs -----------------------------------------------------------------------------------------------------------------
// torch.norm(rays_d, dim=-1)
__device__ __forceinline__ float ray_norm(const float* __restrict__ rays_d, int ray) {
    const float dx = rays_d[(size_t)ray * 3 + 0], dy = rays_d[(size_t)ray * 3 + 1], dz = rays_d[(size_t)ray * 3 + 2];
    return sqrtf(__fadd_rn(__fadd_rn(dx * dx, dy * dy), dz * dz));
}

__device__ __forceinline__ float scan_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }  // torch.sigmoid

// sample i (i < S) of a ray: raw2alpha(raw[..., 3] + noise, dists), noise = randn * raw_noise_std drawn by the caller
// (main.py:592-600).  zr / noise_r: the ray's rows (noise_r may be null).  The forward kernels use alpha alone.
struct ScanSample {
    float alpha, dalpha;  // dalpha = d alpha / d raw_sigma = dist exp(-s dist) (0 where the relu is closed)
    bool closed;          // raw_sigma + noise <= 0 (false for a NaN)
};
__device__ __forceinline__ ScanSample scan_sample(const float* __restrict__ zr, const float* __restrict__ noise_r, float raw_sigma, int i,
                                                  int S, float norm) {
    float dist = (i < S - 1) ? (zr[i + 1] - zr[i]) : 1e10f;   // dists = cat(z[1:] - z[:-1], 1e10)
    dist = dist * norm;
    const float pre = noise_r ? raw_sigma + noise_r[i] : raw_sigma;
    const float sig = (pre != pre) ? pre : fmaxf(pre, 0.0f);  // F.relu: a NaN stays a NaN (fmaxf alone returns the 0)
    const float e = expf(-sig * dist);
    ScanSample o;
    o.alpha = 1.0f - e;                                       // 1 - exp(-relu(raw) * dists)
    o.closed = pre <= 0.0f;                                   // threshold_backward: 0 where x <= 0, the gradient elsewhere (NaN included)
    o.dalpha = o.closed ? 0.0f : dist * e;                    // NaN where pre is
    return o;
}

// The composite of one ray: lane l owns the C consecutive samples l C .. l C + C - 1 (S <= 64 C).  raw_r [S, 4], zr [S] and
// noise_r [S] (or null) are the ray's rows; w_row / z_row (null or [S]) take the weights and a copy of z; the maps are whole
// arrays indexed by ray, each optional.
template <int C>
__device__ __forceinline__ void scan_composite(const float* __restrict__ raw_r, const float* __restrict__ zr,
                                               const float* __restrict__ noise_r, int S, float norm, int white_bkgd, int lane, int ray,
                                               float* w_row, float* z_row, float* rgb_map, float* disp_map, float* acc_map,
                                               float* depth_map) {
    float alpha[C], zi[C], cr[C], cg[C], cb[C];
    double lp[C];
    double prod = 1.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int i = lane * C + c;
        const bool ok = i < S;
        const int ii = ok ? i : S - 1;
        const f32x4 r4 = *reinterpret_cast<const f32x4*>(raw_r + (size_t)ii * 4);
        float a = scan_sample(zr, noise_r, r4[3], ii, S, norm).alpha;
        if (!ok) a = 0.0f;
        alpha[c] = a;
        zi[c] = zr[ii];
        cr[c] = scan_sigmoid(r4[0]);
        cg[c] = scan_sigmoid(r4[1]);
        cb[c] = scan_sigmoid(r4[2]);
        lp[c] = prod;                                           // exclusive product inside the lane
        const float pterm = ok ? ((1.0f - a) + 1e-10f) : 1.0f;  // 1 - alpha + 1e-10, float ops
        prod *= (double)pterm;
    }
    const double incl = wave_scan_mul(prod, lane);
    double excl = shfl_up_f64(incl, 1);
    if (lane == 0) excl = 1.0;
    float sr = 0.f, sg = 0.f, sb = 0.f, sd = 0.f, sa = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int i = lane * C + c;
        const float T = (float)(excl * lp[c]);  // cumprod accumulated in double, rounded per element
        const float w = alpha[c] * T;
        if (i < S) {
            if (w_row) w_row[i] = w;
            if (z_row) z_row[i] = zi[c];
            sr += w * cr[c];
            sg += w * cg[c];
            sb += w * cb[c];
            sd += w * zi[c];
            sa += w;
        }
    }
    sr = wave_sum(sr);
    sg = wave_sum(sg);
    sb = wave_sum(sb);
    sd = wave_sum(sd);
    sa = wave_sum(sa);
    if (lane == 0) {
        if (white_bkgd) {
            const float bg = 1.0f - sa;
            sr += bg;
            sg += bg;
            sb += bg;
        }
        if (rgb_map) {
            rgb_map[(size_t)ray * 3 + 0] = sr;
            rgb_map[(size_t)ray * 3 + 1] = sg;
            rgb_map[(size_t)ray * 3 + 2] = sb;
        }
        if (depth_map) depth_map[ray] = sd;
        if (acc_map) acc_map[ray] = sa;
        if (disp_map) {
            const float q = sd / sa;
            // torch.max(1e-10, q) propagates NaN (0/0 for empty rays), fmaxf would not
            const float m = (q != q) ? q : fmaxf(1e-10f, q);
            disp_map[ray] = 1.0f / m;
        }
    }
}

// ---- sample_pdf (the reference runs it on the CPU, main.py:723-728, so the float accumulation orders are ATen's CPU orders) ------
// torch.sum(x, -1) of a contiguous float row on the CPU (ATen SumKernel, vectorized_inner_sum): 8-lane vectors,
// 4 interleaved vector accumulators over groups of 4 vectors, the remaining whole vectors into accumulator 0,
// ((a0 + a1) + a2) + a3 per lane, then a scalar chain: the row's tail elements first, then the 8 lane sums.
// Verified bit for bit against torch.sum on rows of 30 .. 190 floats (tools/torch_sum_order.py).
__device__ __forceinline__ float torch_cpu_row_sum(const float* row /* LDS, zero padded to 64 */, float* cols /* LDS [8] */,
                                                   int nw, int lane) {
    const int nv = nw >> 3, full = (nv >> 2) << 2;
    if (lane < 8) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int v = 0; v < full; v += 4) {
            a0 = __fadd_rn(a0, row[(v + 0) * 8 + lane]);
            a1 = __fadd_rn(a1, row[(v + 1) * 8 + lane]);
            a2 = __fadd_rn(a2, row[(v + 2) * 8 + lane]);
            a3 = __fadd_rn(a3, row[(v + 3) * 8 + lane]);
        }
        for (int v = full; v < nv; ++v) a0 = __fadd_rn(a0, row[v * 8 + lane]);
        cols[lane] = __fadd_rn(__fadd_rn(__fadd_rn(a0, a1), a2), a3);
    }
    wave_sync();
    float fin = 0.f;
    for (int k = nv * 8; k < nw; ++k) fin = __fadd_rn(fin, row[k]);
    for (int k = 0; k < 8; ++k) fin = __fadd_rn(fin, cols[k]);
    return fin;
}

// The tables of one ray, n_bins <= 64, into the LDS rows s_cdf [64] = cat(0, cumsum(pdf)) and s_bins [64]; s_w [64] and s_col [8]
// are scratch.  w_src: the n_bins - 1 weights.  bins_src: the n_bins bins, or with bins_are_z n_bins + 1 depths whose midpoints
// .5 * (z[1:] + z[:-1]) are the bins (main.py:722).  Synchronised on return.
__device__ __forceinline__ void pdf_tables(const float* w_src, const float* bins_src, int bins_are_z, int n_bins, float* s_w, float* s_col,
                                           float* s_cdf, float* s_bins, int lane) {
    const int nw = n_bins - 1;
    float w = 0.0f;
    if (lane < nw) w = w_src[lane] + 1e-5f;  // weights + 1e-5
    s_w[lane] = w;
    wave_sync();
    const float total = torch_cpu_row_sum(s_w, s_col, nw, lane);  // torch.sum(weights, -1)
    const float pdf = (lane < nw) ? w / total : 0.0f;
    const double cs = wave_scan_add((double)pdf, lane);           // cumsum (double accumulate)
    if (lane < nw) s_cdf[lane + 1] = (float)cs;
    if (lane == 63) s_cdf[0] = 0.0f;                              // cat(zeros, cdf)
    if (lane < n_bins) s_bins[lane] = bins_are_z ? 0.5f * __fadd_rn(bins_src[lane + 1], bins_src[lane]) : bins_src[lane];
    wave_sync();
}

// element k of torch.linspace(0, 1, N), by its scalar formula
__device__ __forceinline__ float linspace_u(int k, int N) {
    const float step = N > 1 ? 1.0f / (float)(N - 1) : 0.0f;
    return (k < N / 2 || N == 1) ? __fmul_rn(step, (float)k) : __fsub_rn(1.0f, __fmul_rn(step, (float)(N - k - 1)));
}

// one draw: lo = searchsorted(cdf, u, right=True) in ATen's form (a NaN on either side goes right), then the interpolation
__device__ __forceinline__ float pdf_draw(const float* s_cdf, const float* s_bins, int n_bins, float u, int& lo) {
    int hi = n_bins;
    lo = 0;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (!(s_cdf[mid] > u)) lo = mid + 1; else hi = mid;
    }
    const int below = lo - 1 > 0 ? lo - 1 : 0;
    const int above = lo < n_bins - 1 ? lo : n_bins - 1;
    const float c0 = s_cdf[below], c1 = s_cdf[above];
    const float b0 = s_bins[below], b1 = s_bins[above];
    float denom = c1 - c0;
    if (denom < 1e-5f) denom = 1.0f;
    const float t = (u - c0) / denom;
    return b0 + t * (b1 - b0);
}

// ---- sort / merge ----------------------------------------------------------------------------------------------------------------
// torch.sort's order of floats: ascending, every NaN behind every number (+inf included), NaNs equal among themselves; -0 == 0.
// A total preorder, which the bitonic network and the rank searches of the merge need: with a plain < every comparison against
// a NaN is false, the network no longer sorts the numbers and two ranks of the merge coincide (a slot stays unwritten).
__device__ __forceinline__ bool nerf_before(float a, float b) { return a < b || (a == a && b != b); }

// two ascending LDS rows into o [na + nb] (the reference sorts the concatenation)
__device__ __forceinline__ void merge_rows(const float* s_a, int na, const float* s_b, int nb, float* o, int lane) {
    for (int i = lane; i < na; i += 64) {  // rank of a[i] = i + #{b before a[i]}
        const float v = s_a[i];
        int lo = 0, hi = nb;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (nerf_before(s_b[mid], v)) lo = mid + 1; else hi = mid;
        }
        o[i + lo] = v;
    }
    for (int j = lane; j < nb; j += 64) {  // rank of b[j] = j + #{a not behind b[j]}: on a tie a's element first, as a stable sort of cat(a, b)
        const float v = s_b[j];
        int lo = 0, hi = na;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (!nerf_before(v, s_a[mid])) lo = mid + 1; else hi = mid;
        }
        o[j + lo] = v;
    }
}
