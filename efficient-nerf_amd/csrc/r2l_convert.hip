// Real images -> ray rows [rays_o | rays_d | rgb] in a given row order: the arithmetic of the reference's
// utils/convert_original_data_to_rays_blender.py (:142-223) as one gather.  One thread computes one output row:
//   src = order[k]              which image and which pixel of the (possibly halved) grid the row comes from
//   pixel                       bytes / 255 (:142); under half_res the mean of the 2 x 2 block, ((a + b) + (c + d)) * 0.25, what
//                               cv2.INTER_AREA computes for a factor of two (:171-175; efficient-nerf_amd/blender.py half_res_area);
//                               with four channels rgb * a + (1 - a) (:178-182), with three the colours as they are
//   ray                         get_rays (:69-86): d = ((i - W/2) / focal, -(j - H/2) / focal, -1) rotated by the pose, the three
//                               products added in x, y, z order; the origin is the pose's last column
// One rounding per operation of the reference (the library is built with -ffp-contract=off; the intrinsics say so in place).
// The reads are a random gather (4 to 16 bytes per row out of a cache line each) and dominate the traffic; the rows go out as
// plain vector stores, adjacent threads to adjacent 36-byte rows.  No atomics: the output is a pure function of the inputs.
// An index outside [0, n_img * H * W) reads nothing and leaves a row of NaN.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/r2l_hip.h"
#include "r2l_host_util.h"
#include "r2l_ray_math.h"

namespace {

template <int C>
__global__ void __launch_bounds__(256) r2l_rays_from_images_kernel(const unsigned char* __restrict__ images, long long n_img, int H0, int W0,
                                                                    const float* __restrict__ poses, int H, int W, float half_w, float half_h,
                                                                    float focal, int half_res, const long long* __restrict__ order,
                                                                    long long rows, float* __restrict__ out) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= rows) return;
    float* __restrict__ o = out + k * 9;
    const long long per_img = (long long)H * W;
    const long long src = order[k];
    if (src < 0 || src >= n_img * per_img) {
#pragma unroll
        for (int c = 0; c < 9; ++c) o[c] = __builtin_nanf("");
        return;
    }
    const long long img = src / per_img;
    const int pix = (int)(src - img * per_img);
    const int j = pix / W, i = pix - j * W;
    // colour
    const unsigned char* __restrict__ im = images + (size_t)img * H0 * W0 * C;
    float v[C];
    if (half_res) {
        float a[C], b[C], c_[C], d[C];
        const size_t at = ((size_t)(2 * j) * W0 + 2 * i) * C;
        ray_load_pixel<C>(im + at, a);
        ray_load_pixel<C>(im + at + C, b);
        ray_load_pixel<C>(im + at + (size_t)W0 * C, c_);
        ray_load_pixel<C>(im + at + (size_t)W0 * C + C, d);
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = __fmul_rn(__fadd_rn(__fadd_rn(a[c], b[c]), __fadd_rn(c_[c], d[c])), 0.25f);
    } else {
        ray_load_pixel<C>(im + ((size_t)j * W0 + i) * C, v);
    }
    if constexpr (C == 4) {
        const float one_minus_a = __fsub_rn(1.0f, v[3]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = __fadd_rn(__fmul_rn(v[c], v[3]), one_minus_a);
    }
    // ray
    const float* __restrict__ p = poses + img * 12;
    float ro[3], rd[3];
    ray_from_pixel(p, i, j, half_w, half_h, focal, ro, rd);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        o[r] = ro[r];
        o[3 + r] = rd[r];
        o[6 + r] = v[r];
    }
}

}  // namespace

extern "C" {

int r2l_rays_from_images(const unsigned char* images_dev, int n_img, int H0, int W0, int channels, const float* poses_dev, double focal,
                         int half_res, const long long* order_dev, long long rows, float* out_dev, void* stream) {
    if (!images_dev || !poses_dev || n_img <= 0 || H0 <= 0 || W0 <= 0 || rows < 0 || (rows != 0 && (!order_dev || !out_dev)))
        return r2l_set_error(R2L_EINVAL, "bad argument to r2l_rays_from_images (n_img=%d H0=%d W0=%d rows=%lld)", n_img, H0, W0, rows);
    if (channels != 3 && channels != 4) return r2l_set_error(R2L_EINVAL, "r2l_rays_from_images: %d channels (3 = RGB or 4 = RGBA)", channels);
    if (!(focal > 0.0)) return r2l_set_error(R2L_EINVAL, "r2l_rays_from_images: focal = %g", focal);
    const int H = half_res ? H0 / 2 : H0, W = half_res ? W0 / 2 : W0;
    if (H < 1 || W < 1) return r2l_set_error(R2L_EINVAL, "r2l_rays_from_images: a %d x %d image has no half resolution", H0, W0);
    if (((uintptr_t)images_dev & 3) || ((uintptr_t)poses_dev & 3) || ((uintptr_t)out_dev & 3) || ((uintptr_t)order_dev & 7))
        return r2l_set_error(R2L_EINVAL, "r2l_rays_from_images: images / poses / out must be 4-byte aligned, order 8-byte aligned");
    if ((rows + 255) / 256 > 0x7fffffffll) return r2l_set_error(R2L_EINVAL, "r2l_rays_from_images: rows = %lld", rows);
    int rc = r2l_require_gfx950(nullptr);
    if (rc) return rc;
    if (rows == 0) return R2L_OK;
    const dim3 grid((unsigned)((rows + 255) / 256)), block(256);
    const float half_w = (float)(W * .5), half_h = (float)(H * .5);
    if (channels == 4)
        hipLaunchKernelGGL(r2l_rays_from_images_kernel<4>, grid, block, 0, (hipStream_t)stream, images_dev, (long long)n_img, H0, W0, poses_dev, H,
                           W, half_w, half_h, (float)focal, half_res ? 1 : 0, order_dev, rows, out_dev);
    else
        hipLaunchKernelGGL(r2l_rays_from_images_kernel<3>, grid, block, 0, (hipStream_t)stream, images_dev, (long long)n_img, H0, W0, poses_dev, H,
                           W, half_w, half_h, (float)focal, half_res ? 1 : 0, order_dev, rows, out_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return r2l_set_error(R2L_EHIP, "r2l_rays_from_images launch: %s", hipGetErrorString(e));
    return R2L_OK;
}

}  // extern "C"
