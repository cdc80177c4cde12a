// Training of the R2L student (NeRF_v3_2, model/nerf_raybased.py:480-544) in exact fp32: the backward pass of the generic layer path
// (r2l_generic.hip), the rgb loss, Adam and the jittered depths of PointSampler.sample_train.  One launch per layer and direction,
// activations and gradients through HBM in caller buffers; the host mirror composes them (efficient-nerf_amd/train.py).
//
// A layer computes y = post + act(u), u = s (x W^T + b) + res.  Given g_y:
//   r2l_train_act_backward   g_post (+)= g_y;  g_u = g_y * act'(a), a = y - post;  g_res (+)= g_u;  g_z = s g_u
//                            (ReLU selects as torch's threshold_backward: 0 where a <= 0 whatever g_y holds, g_y elsewhere, at a NaN too)
//   r2l_train_grad_input     g_x [n, in] (+)= g_z [n, out] W [out, in]
//   r2l_train_grad_weight    g_W [out, in] = g_z^T x,  g_b = sum over rays of g_z
// Both GEMMs run on v_mfma_f32_32x32x2_f32 like the forward kernel (fp32 products, fp32 accumulation in k order).  g_W reduces over
// the rays: the rays are cut into slabs (their number is a function of n alone: r2l_train_grad_weight_slabs), each slab's partial
// [out, in] product goes to a caller workspace, and a second kernel adds the slabs in slab order.  No float atomics anywhere: a
// step is bit-identical from run to run.
//
//   r2l_train_mse_loss       img2mse (utils/run_nerf_raybased_helpers.py) + its gradient (through the tail's sigmoid on request)
//                            + the per-ray error the hard-ray pool sorts (main.py:1410-1413)
//   r2l_train_adam           torch.optim.Adam's update (no weight decay, no amsgrad) over flat buffers, one launch
//   r2l_train_jitter_z       main.py:684-699 / model/nerf_raybased.py:117-123: stratified jitter of the sample depths
//   r2l_train_sum_parts      the ranks' gradients of a ray-sharded step, weighted and added in rank order (flat_trainer.py)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/r2l_hip.h"
#include "r2l_host_util.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define TT_M 128      // rows of the output tile per workgroup (4 waves x 32)
#define TT_N 64       // columns of the output tile (2 MFMA column tiles per wave)
#define TT_K 32       // reduction elements per LDS stage
#define TT_PN 96      // LDS pitch of a k-major [TT_K][TT_N] tile: lanes 32..63 read row k + 1, 96 % 64 = 32 puts them on the other banks
#define TT_PM 160     // ... of a k-major [TT_K][TT_M] tile (160 % 64 = 32)

#define GW_SLAB_RAYS 512      // rays per slab of the g_W reduction ...
#define GW_MAX_SLABS 128      // ... until this many slabs, then the slabs grow

__device__ __forceinline__ float r2l_act_grad(float a, int act) {
    switch (act) {
        case R2L_ACT_LRELU: return a > 0.0f ? 1.0f : 0.01f;
        case R2L_ACT_SIGMOID: return a * (1.0f - a);
        default: return 1.0f;
    }
}

__global__ void r2l_act_backward_kernel(const float* g_y, long long ldg, const float* __restrict__ y, long long ldy,
                                        const float* __restrict__ post, long long ldp, long long n, int width, int act, float scale,
                                        float* g_z, long long ldz, float* g_res, long long ldr, int res_acc, float* g_post,
                                        long long ldq, int post_acc) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n * width) return;
    const long long r = gid / width;
    const int c = (int)(gid - r * width);
    const float gy = g_y[r * ldg + c];
    float a = y[r * ldy + c];
    if (post) a = a - post[r * ldp + c];
    // ReLU selects as torch's threshold_backward does (0 at a closed unit whatever g_y holds, g_y itself elsewhere); the others multiply
    const float gu = act == R2L_ACT_RELU ? (a <= 0.0f ? 0.0f : gy) : gy * r2l_act_grad(a, act);
    // g_post first: g_res may be the same buffer (a one-block body under --use_residual), and then holds g_y + g_u
    if (g_post) g_post[r * ldq + c] = post_acc ? g_post[r * ldq + c] + gy : gy;
    if (g_res) g_res[r * ldr + c] = res_acc ? g_res[r * ldr + c] + gu : gu;
    g_z[r * ldz + c] = scale * gu;
}

// g_x = g_z W: A lane l = g_z[ray l % 32][o l / 32], B lane l = W[o l / 32][i l % 32], D as in r2l_linear_kernel
__global__ __launch_bounds__(256) void r2l_grad_input_kernel(const float* __restrict__ gz, long long ldz, int n,
                                                             const float* __restrict__ w, int out_dim, int in_dim, float* gx,
                                                             long long ldgx, int accumulate) {
    __shared__ float zs[TT_M][TT_K + 1];
    __shared__ float ws[TT_K][TT_PN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long ray0 = (long long)blockIdx.x * TT_M;
    const int i0 = blockIdx.y * TT_N;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
    const int lc = tid & 31, lr = tid >> 5;      // g_z loader: 8 rays of 32 consecutive o per pass
    const int wc = tid & 63, wr = tid >> 6;      // W loader: 4 rows o of 64 consecutive i per pass
    float zv[TT_M / 8], wv[TT_K / 4];
    unsigned okz = 0, okw = 0;
    auto load_stage = [&](int k0) {
        okz = okw = 0;
        const int kz = k0 + lc;
#pragma unroll
        for (int i = 0; i < TT_M / 8; ++i) {
            const long long ray = ray0 + lr + 8 * i;
            const bool ok = kz < out_dim && ray < n;
            zv[i] = gz[ok ? ray * ldz + kz : 0];
            okz |= (ok ? 1u : 0u) << i;
        }
#pragma unroll
        for (int i = 0; i < TT_K / 4; ++i) {
            const int o = k0 + wr + 4 * i;
            const bool ok = o < out_dim && i0 + wc < in_dim;
            wv[i] = w[ok ? (long long)o * in_dim + i0 + wc : 0];
            okw |= (ok ? 1u : 0u) << i;
        }
    };
    load_stage(0);
    for (int k0 = 0; k0 < out_dim; k0 += TT_K) {
#pragma unroll
        for (int i = 0; i < TT_M / 8; ++i) zs[lr + 8 * i][lc] = ((okz >> i) & 1) ? zv[i] : 0.0f;
#pragma unroll
        for (int i = 0; i < TT_K / 4; ++i) ws[wr + 4 * i][wc] = ((okw >> i) & 1) ? wv[i] : 0.0f;
        __syncthreads();
        if (k0 + TT_K < out_dim) load_stage(k0 + TT_K);
#pragma unroll
        for (int kk = 0; kk < TT_K; kk += 2) {
            const int kq = kk + (lane >> 5);
            const float a = zs[wave * 32 + (lane & 31)][kq];
            const float b0 = ws[kq][lane & 31], b1 = ws[kq][32 + (lane & 31)];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int i = i0 + 32 * t + (lane & 31);
        if (i >= in_dim) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long ray = ray0 + wave * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
            if (ray >= n) continue;
            float v = t ? acc1[r] : acc0[r];
            if (accumulate) v = gx[ray * ldgx + i] + v;       // the gradients that meet on a residual stream add up
            gx[ray * ldgx + i] = v;
        }
    }
}

// One slab of g_W = g_z^T x: A lane l = g_z[ray l / 32][o l % 32], B lane l = x[ray l / 32][i l % 32]; D register r of lane l =
// g_W[o 8 (r / 4) + 4 (l / 32) + r % 4][i l % 32].  The workgroups of column tile 0 also add up g_z's columns (g_b).
__global__ __launch_bounds__(256) void r2l_grad_weight_kernel(const float* __restrict__ gz, long long ldz, const float* __restrict__ x,
                                                              long long ldx, int n, int out_dim, int in_dim, int slab_rays,
                                                              float* __restrict__ ws_w, float* __restrict__ ws_b) {
    __shared__ float as[TT_K][TT_PM];
    __shared__ float bs[TT_K][TT_PN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o0 = blockIdx.x * TT_M, i0 = blockIdx.y * TT_N, slab = blockIdx.z;
    const long long r_begin = (long long)slab * slab_rays;
    const long long r_end = r_begin + slab_rays < n ? r_begin + slab_rays : n;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
    const int ac = tid & 127, ar = tid >> 7;     // g_z loader: 2 rays of 128 consecutive o per pass
    const int bc = tid & 63, br = tid >> 6;      // x loader: 4 rays of 64 consecutive i per pass
    float av[TT_K / 2], bv[TT_K / 4];
    unsigned oka = 0, okb = 0;
    float bsum = 0.0f;
    auto load_stage = [&](long long r0) {
        oka = okb = 0;
#pragma unroll
        for (int i = 0; i < TT_K / 2; ++i) {
            const long long ray = r0 + ar + 2 * i;
            const bool ok = ray < r_end && o0 + ac < out_dim;
            av[i] = gz[ok ? ray * ldz + o0 + ac : 0];
            oka |= (ok ? 1u : 0u) << i;
        }
#pragma unroll
        for (int i = 0; i < TT_K / 4; ++i) {
            const long long ray = r0 + br + 4 * i;
            const bool ok = ray < r_end && i0 + bc < in_dim;
            bv[i] = x[ok ? ray * ldx + i0 + bc : 0];
            okb |= (ok ? 1u : 0u) << i;
        }
    };
    load_stage(r_begin);
    for (long long r0 = r_begin; r0 < r_end; r0 += TT_K) {
#pragma unroll
        for (int i = 0; i < TT_K / 2; ++i) {
            const float v = ((oka >> i) & 1) ? av[i] : 0.0f;
            as[ar + 2 * i][ac] = v;
            bsum = bsum + v;
        }
#pragma unroll
        for (int i = 0; i < TT_K / 4; ++i) bs[br + 4 * i][bc] = ((okb >> i) & 1) ? bv[i] : 0.0f;
        __syncthreads();
        if (r0 + TT_K < r_end) load_stage(r0 + TT_K);
#pragma unroll
        for (int kk = 0; kk < TT_K; kk += 2) {
            const int kq = kk + (lane >> 5);
            const float a = as[kq][wave * 32 + (lane & 31)];
            const float b0 = bs[kq][lane & 31], b1 = bs[kq][32 + (lane & 31)];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
        }
        __syncthreads();
    }
    float* slab_w = ws_w + (size_t)slab * out_dim * in_dim;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int i = i0 + 32 * t + (lane & 31);
        if (i >= in_dim) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = o0 + wave * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
            if (o < out_dim) slab_w[(size_t)o * in_dim + i] = t ? acc1[r] : acc0[r];
        }
    }
    if (blockIdx.y == 0) {       // every thread's column sum over its rays, then the two threads of a column in a fixed order
        as[ar][ac] = bsum;
        __syncthreads();
        if (tid < TT_M && o0 + tid < out_dim) ws_b[(size_t)slab * out_dim + o0 + tid] = as[0][tid] + as[1][tid];
    }
}

// the second pass: the slabs added in slab order, for [g_W | g_b]
__global__ void r2l_grad_weight_reduce_kernel(const float* __restrict__ ws_w, const float* __restrict__ ws_b, int n_slab,
                                              long long wn, int out_dim, float* __restrict__ g_w, float* __restrict__ g_b) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= wn + out_dim) return;
    const bool is_w = gid < wn;
    const float* src = is_w ? ws_w + gid : ws_b + (gid - wn);
    const long long pitch = is_w ? wn : out_dim;
    float s = 0.0f;
    for (int k = 0; k < n_slab; ++k) s = s + src[(long long)k * pitch];
    if (is_w) g_w[gid] = s;
    else if (g_b) g_b[gid - wn] = s;
}

#define LOSS_BLOCK 256
// fixed-order tree over a workgroup's LOSS_BLOCK values in LDS
__device__ __forceinline__ float r2l_block_sum(float v, float* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = LOSS_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(LOSS_BLOCK) void r2l_mse_loss_kernel(const float* __restrict__ rgb, const float* __restrict__ target,
                                                                   long long n, float inv_count, int through_sigmoid,
                                                                   float* __restrict__ g_out, float* __restrict__ err,
                                                                   float* __restrict__ partial) {
    __shared__ float sh[LOSS_BLOCK];
    const long long r = (long long)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    float sq = 0.0f;
    if (r < n) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float y = rgb[r * 3 + c];
            const float d = y - target[r * 3 + c];
            sq = sq + d * d;
            float g = (2.0f * d) * inv_count;                 // mean backward, then pow backward
            if (through_sigmoid) g = g * (y * (1.0f - y));      // the tail's sigmoid from its saved output
            g_out[r * 3 + c] = g;
        }
        if (err) err[r] = sq / 3.0f;
    }
    const float s = r2l_block_sum(sq, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(LOSS_BLOCK) void r2l_mse_loss_final_kernel(const float* __restrict__ partial, int n_partial,
                                                                         float inv_count, float* __restrict__ loss) {
    __shared__ float sh[LOSS_BLOCK];
    float s = 0.0f;
    for (int k = threadIdx.x; k < n_partial; k += LOSS_BLOCK) s = s + partial[k];
    s = r2l_block_sum(s, sh);
    if (threadIdx.x == 0) loss[0] = s * inv_count;
}

// torch.optim.Adam (no weight decay, no amsgrad): exp_avg.mul_(b1).add_(g, alpha = 1 - b1); exp_avg_sq.mul_(b2).addcmul_(g, g,
// value = 1 - b2); denom = (exp_avg_sq.sqrt() / sqrt(1 - b2^t)).add_(eps); p.addcdiv_(exp_avg, denom, value = -lr / (1 - b1^t))
__global__ void r2l_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                long long count, float b1, float one_b1, float b2, float one_b2, float neg_step, float bc2_sqrt,
                                float eps) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float gi = g[i];
    const float m0 = m[i], dm = gi - m0;
    // torch steps exp_avg by lerp_(g, 1 - b1) = m + (1 - b1) (g - m).  Where g - m is not a number that form and the two products
    // part: inf - inf is NaN (an infinite gradient on an infinite moment of its sign), a finite gradient on an infinite moment
    // gives inf + -inf = NaN, a difference that overflows gives inf.  There the kernel takes lerp's form; a finite g - m keeps the
    // products', as before.
    const float mi = (fabsf(dm) <= 3.402823466e+38f) ? m0 * b1 + one_b1 * gi : m0 + one_b1 * dm;
    const float vi = v[i] * b2 + (one_b2 * gi) * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = p[i] + (neg_step * mi) / denom;
}

// mids = .5 * (z[1:] + z[:-1]); upper = cat(mids, z[-1:]); lower = cat(z[:1], mids); z = lower + (upper - lower) * t_rand: one
// rounding per torch op
__global__ void r2l_jitter_z_kernel(const float* __restrict__ z_vals, const float* __restrict__ t_rand, long long n, int n_sample,
                                    float* __restrict__ z_out) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n * n_sample) return;
    const int s = (int)(gid % n_sample);
    const float z = z_vals[s];
    const float upper = s + 1 < n_sample ? __fmul_rn(0.5f, __fadd_rn(z_vals[s + 1], z)) : z;
    const float lower = s > 0 ? __fmul_rn(0.5f, __fadd_rn(z, z_vals[s - 1])) : z;
    z_out[gid] = __fadd_rn(lower, __fmul_rn(__fsub_rn(upper, lower), t_rand[gid]));
}

// out[i] = (...((w0 p0[i]) + w1 p1[i]) + ...) + w_{P-1} p_{P-1}[i]: every product and every sum rounded to fp32 on its own (the file
// is built without contraction; the intrinsics say so again), in part order -- what torch's mul and add give, and what one process
// gives that holds all the parts.  A streaming pass: 16-byte loads and stores over the first n_vec * 4 elements where the pointers
// and the pitch allow them (n_vec = 0 otherwise), one element per thread behind them, grid-stride over both.  `out` may be part 0:
// a thread has read every part's element(s) before it writes its own.
#define SUM_MAX_PARTS 64
#define SUM_BLOCK 256
#define SUM_MAX_BLOCKS 2048
struct r2l_sum_weights {
    float w[SUM_MAX_PARTS];
};

__global__ __launch_bounds__(SUM_BLOCK) void r2l_sum_parts_kernel(const float* parts, long long pitch, int n_part, r2l_sum_weights wt,
                                                                  long long count, long long n_vec, float* out) {
    const long long n_item = n_vec + (count - 4 * n_vec);
    const long long stride = (long long)gridDim.x * SUM_BLOCK;
    for (long long it = (long long)blockIdx.x * SUM_BLOCK + threadIdx.x; it < n_item; it += stride) {
        if (it < n_vec) {
            const float4 p0 = *reinterpret_cast<const float4*>(parts + 4 * it);
            float4 acc;
            acc.x = __fmul_rn(p0.x, wt.w[0]);
            acc.y = __fmul_rn(p0.y, wt.w[0]);
            acc.z = __fmul_rn(p0.z, wt.w[0]);
            acc.w = __fmul_rn(p0.w, wt.w[0]);
            for (int k = 1; k < n_part; ++k) {
                const float4 p = *reinterpret_cast<const float4*>(parts + k * pitch + 4 * it);
                const float w = wt.w[k];
                acc.x = __fadd_rn(acc.x, __fmul_rn(p.x, w));
                acc.y = __fadd_rn(acc.y, __fmul_rn(p.y, w));
                acc.z = __fadd_rn(acc.z, __fmul_rn(p.z, w));
                acc.w = __fadd_rn(acc.w, __fmul_rn(p.w, w));
            }
            *reinterpret_cast<float4*>(out + 4 * it) = acc;
        } else {
            const long long i = 4 * n_vec + (it - n_vec);
            float acc = __fmul_rn(parts[i], wt.w[0]);
            for (int k = 1; k < n_part; ++k) acc = __fadd_rn(acc, __fmul_rn(parts[k * pitch + i], wt.w[k]));
            out[i] = acc;
        }
    }
}

static int launch_status(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return r2l_set_error(R2L_EHIP, "%s launch: %s", what, hipGetErrorString(e));
    return R2L_OK;
}

static int gw_slabs(int n) {
    if (n <= 0) return 0;
    const int s = (n + GW_SLAB_RAYS - 1) / GW_SLAB_RAYS;
    return s < GW_MAX_SLABS ? s : GW_MAX_SLABS;
}

extern "C" {

int r2l_train_act_backward(const float* g_y_dev, long long ldg, const float* y_dev, long long ldy, const float* post_dev,
                           long long ldp, int n, int width, int act, float scale, float* g_z_dev, long long ldz, float* g_res_dev,
                           long long ldr, int res_accumulate, float* g_post_dev, long long ldq, int post_accumulate, void* stream) {
    if ((n != 0 && (!g_y_dev || !y_dev || !g_z_dev)) || n < 0 || width <= 0 || ldg < width || ldy < width || ldz < width ||
        (post_dev && ldp < width) || (g_res_dev && ldr < width) || (g_post_dev && ldq < width) || act < R2L_ACT_NONE ||
        act > R2L_ACT_SIGMOID)
        return r2l_set_error(R2L_EINVAL, "bad argument to r2l_train_act_backward (n=%d width=%d act=%d ldg=%lld ldy=%lld ldz=%lld)", n,
                             width, act, ldg, ldy, ldz);
    int rc = r2l_require_gfx950(nullptr);
    if (rc) return rc;
    if (n == 0) return R2L_OK;
    const long long total = (long long)n * width;
    hipLaunchKernelGGL(r2l_act_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g_y_dev, ldg,
                       y_dev, ldy, post_dev, ldp, (long long)n, width, act, scale, g_z_dev, ldz, g_res_dev, ldr, res_accumulate ? 1 : 0,
                       g_post_dev, ldq, post_accumulate ? 1 : 0);
    return launch_status("r2l_train_act_backward");
}

int r2l_train_grad_input(const float* g_z_dev, long long ldz, int n, const float* w_dev, int out_dim, int in_dim, float* g_x_dev,
                         long long ldgx, int accumulate, void* stream) {
    if ((n != 0 && (!g_z_dev || !g_x_dev)) || !w_dev || n < 0 || out_dim <= 0 || in_dim <= 0 || out_dim > (1 << 16) || in_dim > (1 << 16) ||
        ldz < out_dim || ldgx < in_dim)
        return r2l_set_error(R2L_EINVAL, "bad argument to r2l_train_grad_input (n=%d ldz=%lld ldgx=%lld; layer %d -> %d)", n, ldz, ldgx,
                             in_dim, out_dim);
    const float* z_end = g_z_dev + (size_t)(n > 0 ? n - 1 : 0) * ldz + out_dim;
    const float* x_end = g_x_dev + (size_t)(n > 0 ? n - 1 : 0) * ldgx + in_dim;
    if (n > 0 && g_z_dev < x_end && g_x_dev < z_end) return r2l_set_error(R2L_EINVAL, "r2l_train_grad_input: g_z and g_x overlap");
    int rc = r2l_require_gfx950(nullptr);
    if (rc) return rc;
    if (n == 0) return R2L_OK;
    dim3 grid((unsigned)((n + TT_M - 1) / TT_M), (unsigned)((in_dim + TT_N - 1) / TT_N));
    hipLaunchKernelGGL(r2l_grad_input_kernel, grid, dim3(256), 0, (hipStream_t)stream, g_z_dev, ldz, n, w_dev, out_dim, in_dim, g_x_dev,
                       ldgx, accumulate ? 1 : 0);
    return launch_status("r2l_train_grad_input");
}

int r2l_train_grad_weight_slabs(int n) { return gw_slabs(n); }

int r2l_train_grad_weight(const float* g_z_dev, long long ldz, const float* x_dev, long long ldx, int n, int out_dim, int in_dim,
                          float* g_w_dev, float* g_b_dev, float* workspace_dev, long long workspace_floats, void* stream) {
    if ((n != 0 && (!g_z_dev || !x_dev)) || !g_w_dev || n < 0 || out_dim <= 0 || in_dim <= 0 || out_dim > (1 << 16) || in_dim > (1 << 16) ||
        ldz < out_dim || ldx < in_dim)
        return r2l_set_error(R2L_EINVAL, "bad argument to r2l_train_grad_weight (n=%d ldz=%lld ldx=%lld; layer %d -> %d)", n, ldz, ldx,
                             in_dim, out_dim);
    const int n_slab = gw_slabs(n);
    const long long wn = (long long)out_dim * in_dim;
    const long long need = (long long)n_slab * (wn + out_dim);
    if (n_slab > 0 && (!workspace_dev || workspace_floats < need))
        return r2l_set_error(R2L_EINVAL, "r2l_train_grad_weight: the workspace holds %lld floats, %d slabs of a %d x %d layer need %lld",
                             workspace_dev ? workspace_floats : 0LL, n_slab, out_dim, in_dim, need);
    int rc = r2l_require_gfx950(nullptr);
    if (rc) return rc;
    float* ws_w = workspace_dev;
    float* ws_b = workspace_dev ? workspace_dev + (size_t)n_slab * wn : nullptr;
    if (n_slab > 0) {
        int slab_rays = (n + n_slab - 1) / n_slab;
        slab_rays = (slab_rays + TT_K - 1) / TT_K * TT_K;
        dim3 grid((unsigned)((out_dim + TT_M - 1) / TT_M), (unsigned)((in_dim + TT_N - 1) / TT_N), (unsigned)n_slab);
        hipLaunchKernelGGL(r2l_grad_weight_kernel, grid, dim3(256), 0, (hipStream_t)stream, g_z_dev, ldz, x_dev, ldx, n, out_dim, in_dim,
                           slab_rays, ws_w, ws_b);
        rc = launch_status("r2l_train_grad_weight");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(r2l_grad_weight_reduce_kernel, dim3((unsigned)((wn + out_dim + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       ws_w, ws_b, n_slab, wn, out_dim, g_w_dev, g_b_dev);
    return launch_status("r2l_train_grad_weight (slab pass)");
}

int r2l_train_mse_loss(const float* rgb_dev, const float* target_dev, int n, int through_sigmoid, float* g_out_dev, float* err_dev,
                       float* loss_dev, float* workspace_dev, long long workspace_floats, void* stream) {
    const long long n_partial = ((long long)n + LOSS_BLOCK - 1) / LOSS_BLOCK;
    if ((n != 0 && (!rgb_dev || !target_dev || !g_out_dev)) || !loss_dev || n < 0 || (n > 0 && (!workspace_dev || workspace_floats < n_partial)))
        return r2l_set_error(R2L_EINVAL, "bad argument to r2l_train_mse_loss (n=%d; the workspace holds %lld floats, %lld needed)", n,
                             workspace_dev ? workspace_floats : 0LL, n_partial);
    int rc = r2l_require_gfx950(nullptr);
    if (rc) return rc;
    const float inv_count = n > 0 ? 1.0f / (3.0f * (float)n) : 0.0f;
    if (n > 0) {
        hipLaunchKernelGGL(r2l_mse_loss_kernel, dim3((unsigned)n_partial), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, rgb_dev, target_dev,
                           (long long)n, inv_count, through_sigmoid ? 1 : 0, g_out_dev, err_dev, workspace_dev);
        rc = launch_status("r2l_train_mse_loss");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(r2l_mse_loss_final_kernel, dim3(1), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, workspace_dev, (int)n_partial,
                       inv_count, loss_dev);
    return launch_status("r2l_train_mse_loss (final pass)");
}

int r2l_train_adam(float* param_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, long long count, double lr,
                   long long step, void* stream) {
    if (!param_dev || !grad_dev || !exp_avg_dev || !exp_avg_sq_dev || count < 0 || step < 1 || !(lr >= 0.0))
        return r2l_set_error(R2L_EINVAL, "bad argument to r2l_train_adam (count=%lld step=%lld lr=%g)", count, step, lr);
    int rc = r2l_require_gfx950(nullptr);
    if (rc) return rc;
    if (count == 0) return R2L_OK;
    const double b1 = 0.9, b2 = 0.999, eps = 1e-8;          // torch.optim.Adam's scalars are Python doubles, rounded once per op
    const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    hipLaunchKernelGGL(r2l_adam_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param_dev, grad_dev,
                       exp_avg_dev, exp_avg_sq_dev, count, (float)b1, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)(-(lr / bc1)),
                       (float)sqrt(bc2), (float)eps);
    return launch_status("r2l_train_adam");
}

int r2l_train_jitter_z(const float* z_vals_dev, const float* t_rand_dev, int n, int n_sample, float* z_out_dev, void* stream) {
    if (!z_vals_dev || (n != 0 && (!t_rand_dev || !z_out_dev)) || n < 0 || n_sample <= 0)
        return r2l_set_error(R2L_EINVAL, "bad argument to r2l_train_jitter_z (n=%d n_sample=%d)", n, n_sample);
    int rc = r2l_require_gfx950(nullptr);
    if (rc) return rc;
    if (n == 0) return R2L_OK;
    const long long total = (long long)n * n_sample;
    hipLaunchKernelGGL(r2l_jitter_z_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, z_vals_dev,
                       t_rand_dev, (long long)n, n_sample, z_out_dev);
    return launch_status("r2l_train_jitter_z");
}

int r2l_train_sum_parts(const float* parts_dev, long long pitch_floats, int n_part, const float* weights, long long count,
                        float* out_dev, void* stream) {
    if (n_part < 1 || n_part > SUM_MAX_PARTS || !weights || count < 0 || (count != 0 && (!parts_dev || !out_dev)) ||
        (n_part > 1 && pitch_floats < count))
        return r2l_set_error(R2L_EINVAL, "bad argument to r2l_train_sum_parts (n_part=%d, 1 .. %d; count=%lld pitch=%lld)", n_part,
                             SUM_MAX_PARTS, count, pitch_floats);
    // out may be part 0 exactly; any other overlap with the parts would be read after it was written
    if (count > 0 && out_dev != parts_dev) {
        const float* p_end = parts_dev + (size_t)(n_part - 1) * pitch_floats + count;
        if (out_dev < p_end && parts_dev < out_dev + count)
            return r2l_set_error(R2L_EINVAL, "r2l_train_sum_parts: out overlaps the parts (it may be part 0 itself, nothing else)");
    }
    int rc = r2l_require_gfx950(nullptr);
    if (rc) return rc;
    if (count == 0) return R2L_OK;
    r2l_sum_weights wt;
    for (int k = 0; k < SUM_MAX_PARTS; ++k) wt.w[k] = k < n_part ? weights[k] : 0.0f;
    const bool aligned = (((uintptr_t)parts_dev | (uintptr_t)out_dev) & 15) == 0 && (n_part == 1 || pitch_floats % 4 == 0);
    const long long n_vec = aligned ? count / 4 : 0;
    const long long n_item = n_vec + (count - 4 * n_vec);
    long long blocks = (n_item + SUM_BLOCK - 1) / SUM_BLOCK;
    if (blocks > SUM_MAX_BLOCKS) blocks = SUM_MAX_BLOCKS;
    hipLaunchKernelGGL(r2l_sum_parts_kernel, dim3((unsigned)blocks), dim3(SUM_BLOCK), 0, (hipStream_t)stream, parts_dev, pitch_floats,
                       n_part, wt, count, n_vec, out_dev);
    return launch_status("r2l_train_sum_parts");
}

}  // extern "C"
