// Rays for online distillation: n random pixels of n_pose cameras per launch, ready for the teacher to render and the student to
// learn from in the same step (efficient-nerf_amd/online.py).  One thread computes one ray k:
//   pose    k % n_pose: a batch mixes every pose of the step evenly, as a save group of create_data rand mixes its poses
//   pixel   mulhi32(x, H * W), x = word 0 of Philox4x32-10 (Salmon et al., SC'11) with counter (k_lo, k_hi, step_lo, step_hi) and
//           key (seed_lo, seed_hi), in integer arithmetic only.  mulhi32(x, m) = floor(x m / 2^32) maps the 2^32 values of x onto
//           [0, m) in runs of floor(2^32 / m) or one more: a pixel's probability differs from 1 / m by less than 2^-32, a relative
//           bias of at most m / 2^32 = H W / 2^32 (3.7e-5 for 400 x 400; H W < 2^31 is required).
//   ray     get_rays (utils/run_nerf_raybased_helpers.py:231-257) for that pixel, pose and that pose's focal, with the operations
//           and roundings of r2l_rays_from_images_kernel / nerf_get_rays_kernel: d = ((i - W/2) / focal, -(j - H/2) / focal, -1)
//           rotated by the pose, the three products added in x, y, z order; the origin is the pose's last column
// The output is a pure function of the arguments: no atomics, no generator state, nothing read back.
// Store shape: a thread writes its own two 12-byte rows with three dword stores each, adjacent threads to adjacent rows, so a
// wave's three store instructions together cover 768 contiguous bytes and the L2 merges them into whole lines.  Staging the rows
// in LDS and writing coalesced runs was worth 6 % on r2l_rays_from_images' 576 MB (DESIGN, "Converting real images"); a step's
// launch here writes 2.6 MB (81,920 rays x 32 bytes with the pixel indices) and is paced by the launch, not the stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/r2l_hip.h"
#include "r2l_host_util.h"

namespace {

// word 0 of Philox4x32-10(counter c0..c3, key k0, k1): ten rounds of
//   (c0, c1, c2, c3) <- (mulhi(M1, c2) ^ c1 ^ k0, mullo(M1, c2), mulhi(M0, c0) ^ c3 ^ k1, mullo(M0, c0)),  key += (W0, W1)
__device__ __forceinline__ uint32_t philox4x32_10_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    return c0;
}

__global__ void __launch_bounds__(256) r2l_rand_rays_kernel(const float* __restrict__ poses, const float* __restrict__ focals, int n_pose,
                                                             int W, uint32_t n_pix, float half_w, float half_h, uint32_t seed_lo,
                                                             uint32_t seed_hi, uint32_t step_lo, uint32_t step_hi, long long n,
                                                             float* __restrict__ rays_o, float* __restrict__ rays_d,
                                                             long long* __restrict__ pixel) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int pose = (int)(k % n_pose);
    const uint32_t x = philox4x32_10_word0((uint32_t)k, (uint32_t)((unsigned long long)k >> 32), step_lo, step_hi, seed_lo, seed_hi);
    const int pix = (int)__umulhi(x, n_pix);             // < n_pix < 2^31
    const int j = pix / W, i = pix - j * W;
    const float* __restrict__ p = poses + (size_t)pose * 12;
    const float focal = focals[pose];
    const float dx = __fdiv_rn(__fsub_rn((float)i, half_w), focal);
    const float dy = -__fdiv_rn(__fsub_rn((float)j, half_h), focal);
    float* __restrict__ o = rays_o + k * 3;
    float* __restrict__ d = rays_d + k * 3;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float s = __fadd_rn(__fmul_rn(dx, p[4 * r + 0]), __fmul_rn(dy, p[4 * r + 1]));
        o[r] = p[4 * r + 3];
        d[r] = __fadd_rn(s, __fmul_rn(-1.0f, p[4 * r + 2]));
    }
    if (pixel) pixel[k] = pix;
}

}  // namespace

extern "C" {

int r2l_rand_rays(const float* poses_dev, const float* focal_dev, int n_pose, int H, int W, unsigned long long seed, long long step,
                  long long n, float* rays_o_dev, float* rays_d_dev, long long* pixel_dev, void* stream) {
    const long long n_pix = (long long)H * W;
    if (!poses_dev || !focal_dev || n_pose < 1 || H < 1 || W < 1 || n_pix < 1 || n_pix >= (1ll << 31) || n < 0 ||
        (n != 0 && (!rays_o_dev || !rays_d_dev)))
        return r2l_set_error(R2L_EINVAL, "bad argument to r2l_rand_rays (n_pose=%d H=%d W=%d n=%lld; poses / focal / rays_o / rays_d must "
                             "not be NULL, 1 <= H * W < 2^31)", n_pose, H, W, n);
    if (((uintptr_t)poses_dev & 3) || ((uintptr_t)focal_dev & 3) || ((uintptr_t)rays_o_dev & 3) || ((uintptr_t)rays_d_dev & 3) ||
        ((uintptr_t)pixel_dev & 7))
        return r2l_set_error(R2L_EINVAL, "r2l_rand_rays: poses / focal / rays_o / rays_d must be 4-byte aligned, pixel 8-byte aligned");
    if ((n + 255) / 256 > 0x7fffffffll) return r2l_set_error(R2L_EINVAL, "r2l_rand_rays: n = %lld", n);
    int rc = r2l_require_gfx950(nullptr);
    if (rc) return rc;
    if (n == 0) return R2L_OK;
    const unsigned long long st = (unsigned long long)step;
    hipLaunchKernelGGL(r2l_rand_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, poses_dev, focal_dev,
                       n_pose, W, (uint32_t)n_pix, (float)(W * .5), (float)(H * .5), (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)st,
                       (uint32_t)(st >> 32), n, rays_o_dev, rays_d_dev, pixel_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return r2l_set_error(R2L_EHIP, "r2l_rand_rays launch: %s", hipGetErrorString(e));
    return R2L_OK;
}

}  // extern "C"
