// Training of the NeRF teacher (main.py:624-756, 1353-1406) in exact fp32: the one stage of a teacher step the student's
// training kernels (r2l_train.hip) do not cover, the backward pass of the volume-rendering scan raw2outputs (main.py:556-621),
// and, further down, the rays of a step of the use_batching loop straight from the images (nerf_train_batch_rays_kernel).
// The host mirror composes the step (efficient-nerf_amd/train_teacher.py).
//
// Forward (scan_composite, nerf_scan.h): c = sigmoid(raw_rgb), s = relu(raw_sigma + noise), alpha = 1 - exp(-s dist),
// p = 1 - alpha + 1e-10, T_i = prod_{j<i} p_j, w = alpha T, rgb_map = sum_i w_i c_i (+ 1 - sum_i w_i on a white background).
// The loss reaches rgb_map alone (z_samples is detached, main.py:728), so with g = g_rgb_map and
//   q_i = g . c_i - (white_bkgd ? g_r + g_g + g_b : 0)                      (= dL/dw_i)
//   g_c_i     = w_i g                                                       through c (1 - c)
//   g_alpha_i = T_i (q_i - B_i),   B_i = alpha_{i+1} q_{i+1} + p_{i+1} B_{i+1},  B_{S-1} = 0
//   g_s_i     = g_alpha_i * (dist_i exp(-s_i dist_i))                       through relu' (0 at 0, as torch)
// B is the division-free form of cumprod's backward: autograd's reverse_cumsum(grad * out) / in divides by p = 1e-10 on a
// saturated sample.
//
// Layout as the forward scan: a wave owns a ray, lane l of chunk k owns sample 64 k + l (a coalesced float4 of raw per lane), any
// S >= 1.  Pass 1 walks the chunks front to back: T (cumprod accumulated in double and rounded per element, by the forward's
// wave_scan_mul) is parked in the density slot of the sample's own g_raw element.  Pass 2 walks them back to front: the forward quantities
// are recomputed in registers by the forward's own functions (scan_sample, scan_sigmoid, ray_norm), B is a suffix scan of the affine maps E -> alpha q + p E across the wave (in double) with the carry
// E of the chunk behind, and every g_raw element is written once, whole.  No atomics, no reduction across rays: the same
// inputs give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/r2l_hip.h"
#include "nerf_scan.h"
#include "r2l_host_util.h"
#include "r2l_ray_math.h"

__global__ __launch_bounds__(256) void nerf_raw2outputs_backward_kernel(const float* __restrict__ raw, const float* __restrict__ z,
                                                                        const float* __restrict__ rays_d,
                                                                        const float* __restrict__ noise, int n, int S, int white_bkgd,
                                                                        const float* __restrict__ g_rgb_map, float* g_raw) {
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (ray >= n) return;
    const float* zr = z + (size_t)ray * S;
    const float* nr = noise ? noise + (size_t)ray * S : nullptr;
    const float* rr = raw + (size_t)ray * S * 4;
    float* gr = g_raw + (size_t)ray * S * 4;
    const float norm = ray_norm(rays_d, ray);
    const float g0 = g_rgb_map[(size_t)ray * 3 + 0], g1 = g_rgb_map[(size_t)ray * 3 + 1], g2 = g_rgb_map[(size_t)ray * 3 + 2];
    const float gsum = white_bkgd ? (g0 + g1) + g2 : 0.0f;
    const int n_chunk = (S + 63) >> 6;

    // pass 1: T_i into g_raw[i][3]
    double carry = 1.0;
    for (int k = 0; k < n_chunk; ++k) {
        const int i = k * 64 + lane;
        const bool ok = i < S;
        double pterm = 1.0;
        if (ok) {
            const ScanSample sm = scan_sample(zr, nr, rr[(size_t)i * 4 + 3], i, S, norm);
            pterm = (double)((1.0f - sm.alpha) + 1e-10f);
        }
        const double incl = wave_scan_mul(pterm, lane);
        double excl = shfl_up_f64(incl, 1);
        if (lane == 0) excl = 1.0;
        if (ok) gr[(size_t)i * 4 + 3] = (float)(carry * excl);
        carry *= shfl_f64(incl, 63);
    }

    // pass 2: E_i = alpha_i q_i + p_i E_{i+1}, E_S = 0; B_i = E_{i+1}
    double e_behind = 0.0;
    for (int k = n_chunk - 1; k >= 0; --k) {
        const int i = k * 64 + lane;
        const bool ok = i < S;
        f32x4 r4 = {0.f, 0.f, 0.f, 0.f};
        ScanSample sm = {0.f, 0.f, true};
        float T = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f, q = 0.f;
        double a = 0.0, p = 1.0;               // the identity map on the lanes behind the ray's end
        if (ok) {
            r4 = *reinterpret_cast<const f32x4*>(rr + (size_t)i * 4);
            sm = scan_sample(zr, nr, r4[3], i, S, norm);
            T = gr[(size_t)i * 4 + 3];         // this lane's own store of pass 1
            c0 = scan_sigmoid(r4[0]);
            c1 = scan_sigmoid(r4[1]);
            c2 = scan_sigmoid(r4[2]);
            q = ((g0 * c0 + g1 * c1) + g2 * c2) - gsum;
            a = (double)sm.alpha * (double)q;
            p = (double)((1.0f - sm.alpha) + 1e-10f);
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {     // (a, p) of lane l := the map of samples l .. min(l + 2d - 1, 63) of the chunk
            const double a2 = shfl_down_f64(a, d), p2 = shfl_down_f64(p, d);
            if (lane + d < 64) {
                a = a + p * a2;
                p = p * p2;
            }
        }
        const double E = a + p * e_behind;
        double B = shfl_down_f64(E, 1);
        if (lane == 63) B = e_behind;
        e_behind = shfl_f64(E, 0);
        if (ok) {
            const float w = sm.alpha * T;
            const float g_alpha = T * (float)((double)q - B);
            f32x4 o;
            o[0] = (w * g0) * (c0 * (1.0f - c0));
            o[1] = (w * g1) * (c1 * (1.0f - c1));
            o[2] = (w * g2) * (c2 * (1.0f - c2));
            // a closed relu gives 0 whatever arrives; an open one with dist exp(-s dist) = 0 gives 0 (not -0) to a finite g_alpha and,
            // as autograd's product, NaN to a NaN or infinite one
            const float g_s = g_alpha * sm.dalpha;
            o[3] = (sm.closed || (sm.dalpha == 0.0f && g_s == g_s)) ? 0.0f : g_s;
            *reinterpret_cast<f32x4*>(gr + (size_t)i * 4) = o;
        }
    }
}

// ---- a step's rays straight from the images (the reference's use_batching loop, main.py:1137-1162, 1199-1210) -----------------
// The reference keeps rays_rgb [n_train H W, 3, 3] (get_rays_np of every training pose beside the images) and slices N_rand rows of
// it per step.  That bank is a function of the image bytes, the poses and a permutation, so those stay on the device and a step's
// rows are computed: thread t of a block owns output ray k = 256 block + t, src = order[k] names image src / (H W) and pixel
// (row, column) of its grid.  Colour and world ray are r2l_rays_from_images_kernel's (three channels, full resolution), the view
// direction and the NDC projection nerf_ndc_rays_kernel's: the device code is shared (r2l_ray_math.h), not restated.
// Reads: 8 bytes of order (coalesced), then a random 3-byte pixel and a 48-byte pose (a handful of poses: cache hits).  Stores: the
// block's 256 rows of each output are 768 consecutive floats, staged in LDS and written as consecutive dwords by consecutive
// lanes, 256 bytes per wave instruction, whatever the alignment of the four arrays.  No atomics: a pure function of the inputs.
// An index outside [0, n_img H W) reads nothing and gives NaN in all four rows.
__global__ void __launch_bounds__(256) nerf_train_batch_rays_kernel(const unsigned char* __restrict__ images, long long n_img, int H, int W,
                                                                     const float* __restrict__ poses, float half_w, float half_h, float focal,
                                                                     const long long* __restrict__ order, long long rows, int ndc, RayNdc kn,
                                                                     float* __restrict__ rays_o, float* __restrict__ rays_d,
                                                                     float* __restrict__ viewdirs, float* __restrict__ target) {
    __shared__ float stage[4][768];
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * 256;
    const long long k = base + t;
    if (k < rows) {
        const float nan = __builtin_nanf("");
        float o[3] = {nan, nan, nan}, d[3] = {nan, nan, nan}, v[3] = {nan, nan, nan}, c[3] = {nan, nan, nan};
        const long long per_img = (long long)H * W;
        const long long src = order[k];
        if (src >= 0 && src < n_img * per_img) {
            const long long img = src / per_img;
            const int pix = (int)(src - img * per_img);
            const int j = pix / W, i = pix - j * W;
            ray_load_pixel<3>(images + ((size_t)img * per_img + pix) * 3, c);
            ray_from_pixel(poses + img * 12, i, j, half_w, half_h, focal, o, d);
            ray_viewdir(d, v);                        // of the WORLD direction, before the projection (main.py:148-162)
            if (ndc) ray_ndc_project(kn, o, d, o, d);
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            stage[0][3 * t + r] = o[r];
            stage[1][3 * t + r] = d[r];
            stage[2][3 * t + r] = v[r];
            stage[3][3 * t + r] = c[r];
        }
    }
    __syncthreads();
    const long long left = rows - base;
    const int count = 3 * (int)(left < 256 ? left : 256);     // floats of this block per output
    float* const outs[4] = {rays_o, rays_d, viewdirs, target};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (!outs[a]) continue;                               // viewdirs may be NULL
        float* __restrict__ dst = outs[a] + base * 3;
#pragma unroll
        for (int e = t; e < 768; e += 256)
            if (e < count) dst[e] = stage[a][e];
    }
}

extern "C" {

int nerf_train_raw2outputs_backward(const float* raw_dev, const float* z_dev, const float* rays_d_dev, const float* noise_dev, int n,
                                    int S, int white_bkgd, const float* g_rgb_map_dev, float* g_raw_dev, void* stream) {
    if ((n != 0 && (!raw_dev || !z_dev || !rays_d_dev || !g_rgb_map_dev || !g_raw_dev)) || n < 0 || S < 1 ||
        (long long)n * S > (1LL << 40))
        return r2l_set_error(R2L_EINVAL, "bad argument to nerf_train_raw2outputs_backward (n=%d S=%d)", n, S);
    if (((uintptr_t)raw_dev | (uintptr_t)g_raw_dev) & 15)
        return r2l_set_error(R2L_EINVAL, "nerf_train_raw2outputs_backward: raw and g_raw must be 16-byte aligned");
    if (n > 0 && raw_dev == g_raw_dev) return r2l_set_error(R2L_EINVAL, "nerf_train_raw2outputs_backward: g_raw must not be raw");
    int rc = r2l_require_gfx950(nullptr);
    if (rc) return rc;
    if (n == 0) return R2L_OK;
    hipLaunchKernelGGL(nerf_raw2outputs_backward_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, raw_dev, z_dev,
                       rays_d_dev, noise_dev, n, S, white_bkgd ? 1 : 0, g_rgb_map_dev, g_raw_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return r2l_set_error(R2L_EHIP, "nerf_train_raw2outputs_backward launch: %s", hipGetErrorString(e));
    return R2L_OK;
}

int nerf_train_batch_rays(const unsigned char* images_dev, int n_img, int H, int W, const float* poses_dev, double focal,
                          const long long* order_dev, long long rows, int ndc, float near_, float* rays_o_dev, float* rays_d_dev,
                          float* viewdirs_dev, float* target_dev, void* stream) {
    if (!images_dev || !poses_dev || n_img <= 0 || H <= 0 || W <= 0 || rows < 0 ||
        (rows != 0 && (!order_dev || !rays_o_dev || !rays_d_dev || !target_dev)))
        return r2l_set_error(R2L_EINVAL, "bad argument to nerf_train_batch_rays (n_img=%d H=%d W=%d rows=%lld)", n_img, H, W, rows);
    if (!(focal > 0.0)) return r2l_set_error(R2L_EINVAL, "nerf_train_batch_rays: focal = %g", focal);
    if (ndc && !(near_ == near_)) return r2l_set_error(R2L_EINVAL, "nerf_train_batch_rays: near = %g", (double)near_);
    if (((uintptr_t)poses_dev & 3) || ((uintptr_t)rays_o_dev & 3) || ((uintptr_t)rays_d_dev & 3) || ((uintptr_t)viewdirs_dev & 3) ||
        ((uintptr_t)target_dev & 3) || ((uintptr_t)order_dev & 7))
        return r2l_set_error(R2L_EINVAL, "nerf_train_batch_rays: poses and the four outputs must be 4-byte aligned, order 8-byte aligned");
    if ((rows + 255) / 256 > 0x7fffffffll) return r2l_set_error(R2L_EINVAL, "nerf_train_batch_rays: rows = %lld", rows);
    int rc = r2l_require_gfx950(nullptr);
    if (rc) return rc;
    if (rows == 0) return R2L_OK;
    const float half_w = (float)(W * .5), half_h = (float)(H * .5);
    hipLaunchKernelGGL(nerf_train_batch_rays_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, images_dev,
                       (long long)n_img, H, W, poses_dev, half_w, half_h, (float)focal, order_dev, rows, ndc ? 1 : 0,
                       ray_ndc_constants(H, W, focal, near_), rays_o_dev, rays_d_dev, viewdirs_dev, target_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return r2l_set_error(R2L_EHIP, "nerf_train_batch_rays launch: %s", hipGetErrorString(e));
    return R2L_OK;
}

}  // extern "C"
