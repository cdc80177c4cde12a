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
// On an LLFF scene the poses themselves are built on the device first (r2l_llff_rand_poses_kernel below, one thread per pose, from
// the step's uniform draws), so that a step's host work is one RandomState.rand call and its upload.
// Store shape: a thread writes its own two 12-byte rows with three dword stores each, adjacent threads to adjacent rows, so a
// wave's three store instructions together cover 768 contiguous bytes and the L2 merges them into whole lines.  Staging the rows
// in LDS and writing coalesced runs was worth 6 % on r2l_rays_from_images' 576 MB (DESIGN, "Converting real images"); a step's
// launch here writes 2.6 MB (81,920 rays x 32 bytes with the pixel indices) and is paced by the launch, not the stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

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

// The poses of an LLFF step (llff.pose_in_boxes, the reference's get_rand_pose_v2 with its draws given): a position and a viewing
// axis drawn in the two widened boxes of the scene, both carried through the average pose M (the translation is added to the
// viewing axis too, as the reference does), then view_matrix.  box: M row-major [12], up [3], the position box left [3], right [3],
// the viewing-axis box left [3], right [3] (llff.pose_box).  One thread builds one pose in binary64, one rounding per operation in
// the order written here, and rounds the twelve entries to float32 once; a zero-length vector gives NaN rows, as numpy does.
struct LLFFPoseBox {
    double m[12], up[3], o_left[3], o_right[3], d_left[3], d_right[3];
};
static_assert(sizeof(LLFFPoseBox) == 27 * sizeof(double), "LLFFPoseBox is the 27 doubles of llff.pose_box");

__device__ __forceinline__ void llff_normalise(double* v) {
    const double n = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(v[0], v[0]), __dmul_rn(v[1], v[1])), __dmul_rn(v[2], v[2])));
#pragma unroll
    for (int r = 0; r < 3; ++r) v[r] = __ddiv_rn(v[r], n);
}

__device__ __forceinline__ void llff_cross(const double* a, const double* b, double* out) {
    out[0] = __dsub_rn(__dmul_rn(a[1], b[2]), __dmul_rn(a[2], b[1]));
    out[1] = __dsub_rn(__dmul_rn(a[2], b[0]), __dmul_rn(a[0], b[2]));
    out[2] = __dsub_rn(__dmul_rn(a[0], b[1]), __dmul_rn(a[1], b[0]));
}

// M[:3, :4] . (p, 1), the three products added left to right and the translation last
__device__ __forceinline__ void llff_through_pose(const double* m, const double* p, double* out) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
        out[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[4 * r + 0], p[0]), __dmul_rn(m[4 * r + 1], p[1])), __dmul_rn(m[4 * r + 2], p[2])),
                           m[4 * r + 3]);
}

__global__ void __launch_bounds__(256) r2l_llff_rand_poses_kernel(const double* __restrict__ u, int n_pose, int n_u, LLFFPoseBox box,
                                                                   double focal, float* __restrict__ poses, float* __restrict__ focals) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_pose) return;
    const double* __restrict__ uk = u + (size_t)k * n_u;
    double po[3], pd[3], c[3], v0[3], v1[3], v2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        po[r] = __dadd_rn(__dmul_rn(uk[r], __dsub_rn(box.o_right[r], box.o_left[r])), box.o_left[r]);
        pd[r] = __dadd_rn(__dmul_rn(uk[3 + r], __dsub_rn(box.d_right[r], box.d_left[r])), box.d_left[r]);
    }
    llff_through_pose(box.m, po, c);
    llff_through_pose(box.m, pd, v2);
    llff_normalise(v2);                                  // pose_in_boxes' _normalize(z) ...
    llff_normalise(v2);                                  // ... and view_matrix's own
    llff_cross(box.up, v2, v0);
    llff_normalise(v0);
    llff_cross(v2, v0, v1);
    llff_normalise(v1);
    float* __restrict__ p = poses + (size_t)k * 12;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        p[4 * r + 0] = (float)v0[r];
        p[4 * r + 1] = (float)v1[r];
        p[4 * r + 2] = (float)v2[r];
        p[4 * r + 3] = (float)c[r];
    }
    focals[k] = (float)(n_u == 7 ? __dmul_rn(focal, __dadd_rn(uk[6], 1.0)) : focal);
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

int r2l_llff_rand_poses(const double* u_dev, int n_pose, int n_u, const double* box_host, double focal, float* poses_dev, float* focal_dev,
                        void* stream) {
    if (!u_dev || !box_host || !poses_dev || !focal_dev)
        return r2l_set_error(R2L_EINVAL, "r2l_llff_rand_poses: u / box / poses / focal must not be NULL");
    if (n_pose < 1) return r2l_set_error(R2L_EINVAL, "r2l_llff_rand_poses: n_pose = %d, at least one pose", n_pose);
    if (n_u != 6 && n_u != 7)
        return r2l_set_error(R2L_EINVAL, "r2l_llff_rand_poses: n_u = %d draws per pose, 7 (with the focal scale) or 6", n_u);
    if (((uintptr_t)u_dev & 7) || ((uintptr_t)poses_dev & 3) || ((uintptr_t)focal_dev & 3))
        return r2l_set_error(R2L_EINVAL, "r2l_llff_rand_poses: u must be 8-byte aligned, poses / focal 4-byte aligned");
    if (!std::isfinite(focal) || !(focal > 0)) return r2l_set_error(R2L_EINVAL, "r2l_llff_rand_poses: focal = %g is not finite and positive", focal);
    LLFFPoseBox box;
    memcpy(&box, box_host, sizeof(box));
    for (int i = 0; i < 27; ++i)
        if (!std::isfinite(box_host[i])) return r2l_set_error(R2L_EINVAL, "r2l_llff_rand_poses: box entry %d = %g is not finite", i, box_host[i]);
    for (int r = 0; r < 3; ++r)
        if (!(box.o_right[r] > box.o_left[r]) || !(box.d_right[r] > box.d_left[r]))
            return r2l_set_error(R2L_EINVAL, "r2l_llff_rand_poses: axis %d of a box is empty (position [%g, %g], viewing axis [%g, %g]; right must "
                                 "exceed left)", r, box.o_left[r], box.o_right[r], box.d_left[r], box.d_right[r]);
    int rc = r2l_require_gfx950(nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(r2l_llff_rand_poses_kernel, dim3((unsigned)(((long long)n_pose + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u_dev, n_pose, n_u,
                       box, focal, poses_dev, focal_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return r2l_set_error(R2L_EHIP, "r2l_llff_rand_poses launch: %s", hipGetErrorString(e));
    return R2L_OK;
}

}  // extern "C"
