// Per-ray arithmetic that more than one kernel states: a pixel's colour and world ray from image bytes and a pose
// (r2l_rays_from_images_kernel, nerf_train_batch_rays_kernel), the unit view direction and the NDC projection
// (nerf_ndc_rays_kernel, nerf_train_batch_rays_kernel).  One rounding per operation of the reference; every kernel that includes
// this is built with -ffp-contract=off, so the callers agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// one pixel's channels as bytes / 255
template <int C>
__device__ __forceinline__ void ray_load_pixel(const unsigned char* __restrict__ p, float (&v)[C]) {
    if constexpr (C == 4) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p);       // 4-byte aligned: the base is, and a pixel is 4 bytes
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = __fdiv_rn((float)((w >> (8 * c)) & 0xffu), 255.0f);
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = __fdiv_rn((float)p[c], 255.0f);
    }
}

// get_rays of pixel (row j, column i) under the pose p [3, 4]: d = ((i - W/2) / focal, -(j - H/2) / focal, -1) rotated by the
// pose, the three products added in x, y, z order; the origin is the pose's last column
__device__ __forceinline__ void ray_from_pixel(const float* __restrict__ p, int i, int j, float half_w, float half_h, float focal,
                                               float (&o)[3], float (&d)[3]) {
    const float dx = __fdiv_rn(__fsub_rn((float)i, half_w), focal);
    const float dy = -__fdiv_rn(__fsub_rn((float)j, half_h), focal);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float s = __fadd_rn(__fmul_rn(dx, p[4 * r + 0]), __fmul_rn(dy, p[4 * r + 1]));
        o[r] = p[4 * r + 3];
        d[r] = __fadd_rn(s, __fmul_rn(-1.0f, p[4 * r + 2]));
    }
}

// rays_d / ||rays_d|| (main.py:148-157; same arithmetic as nerf_mlp_kernel)
__device__ __forceinline__ void ray_viewdir(const float (&d)[3], float (&v)[3]) {
    const float nrm = sqrtf(__fadd_rn(__fadd_rn(d[0] * d[0], d[1] * d[1]), d[2] * d[2]));
    v[0] = __fdiv_rn(d[0], nrm);
    v[1] = __fdiv_rn(d[1], nrm);
    v[2] = __fdiv_rn(d[2], nrm);
}

// the constants of ndc_rays (utils/run_nerf_raybased_helpers.py:260-279), rounded once on the host:
//   c0 = fl32(-1/(W/(2 focal))), c1 = fl32(-1/(H/(2 focal))), two_near = fl32(2 near), mtwo_near = fl32(-2 near)
struct RayNdc {
    float c0, c1, near_, two_near, mtwo_near;
};
inline RayNdc ray_ndc_constants(int H, int W, double focal, float near_) {
    return RayNdc{(float)(-1. / (W / (2. * focal))), (float)(-1. / (H / (2. * focal))), near_, (float)(2. * near_), (float)(-2. * near_)};
}

// ndc_rays of one ray, the reference's operation order; o / d may be the outputs themselves
__device__ __forceinline__ void ray_ndc_project(const RayNdc& k, const float (&o)[3], const float (&d)[3], float (&out_o)[3],
                                                float (&out_d)[3]) {
    const float ox = o[0], oy = o[1], oz = o[2], dx = d[0], dy = d[1], dz = d[2];
    const float t = __fdiv_rn(-__fadd_rn(k.near_, oz), dz);      // -(near + o_z) / d_z
    const float px = __fadd_rn(ox, __fmul_rn(t, dx));            // origin moved to the near plane
    const float py = __fadd_rn(oy, __fmul_rn(t, dy));
    const float pz = __fadd_rn(oz, __fmul_rn(t, dz));
    const float rx = __fdiv_rn(px, pz), ry = __fdiv_rn(py, pz);  // used by the d0 / d1 terms
    out_o[0] = __fdiv_rn(__fmul_rn(k.c0, px), pz);               // (c0 * o_x) / o_z
    out_o[1] = __fdiv_rn(__fmul_rn(k.c1, py), pz);
    out_o[2] = __fadd_rn(1.0f, __fdiv_rn(k.two_near, pz));
    out_d[0] = __fmul_rn(k.c0, __fadd_rn(__fdiv_rn(dx, dz), -rx));
    out_d[1] = __fmul_rn(k.c1, __fadd_rn(__fdiv_rn(dy, dz), -ry));
    out_d[2] = __fdiv_rn(k.mtwo_near, pz);
}
