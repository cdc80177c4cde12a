// LPIPS v0.1 with the AlexNet trunk (Zhang et al., CVPR 2018; the reference's default --lpips_net alex), the TestLPIPS of its [TEST]
// lines (main.py:359-369), of image pairs.  Features live as [pixels, channels] rows, image after image (a of pair 0, b of pair 0, a of
// pair 1, ...), so a convolution is one patch gather and one product with the weight as [out, kh kw in]:
//
//   lpips_gather_kernel   one block = one output pixel of one image: writes its row of the patch matrix [images P, kh kw C], column
//                         (ky kw + kx) C + c -- a window row is one contiguous run of the source, so loads and stores coalesce;
//                         r2l_lpips_create reorders the state_dict's [out, in, kh, kw] once on the host to match -- zeros where the
//                         window leaves the image.  The first layer's gather also applies v = mul (x - lo) + add and the scaling
//                         layer (v - shift) / scale.
//   r2l_linear_forward_dev  the library's fp32 MFMA layer (csrc/r2l_generic.hip): patches x weight^T + bias, ReLU (a NaN stays a NaN, as
//                         in nn.ReLU).  A row's sum does not depend on where the row stands, so a pair's value does not depend on its
//                         place in the stack, and a NaN pixel reaches its own pair alone.
//   lpips_pool_kernel     max over 3 x 3 windows, stride 2, no padding, floor mode; one block = one output pixel.
//   lpips_dist_kernel     one wave = one pixel at a time: both images' feature vectors are normalised over the channels,
//                         n = f / (sqrt(sum f^2) + 1e-10), and sum_c lin[c] (n_a[c] - n_b[c])^2 is taken; the sums run in float64
//                         over a butterfly of the 64 lanes.  A block adds its 32 pixels in a fixed order into one partial.
//   lpips_mean_kernel     adds a layer's partials in a fixed order in float64: d_k.  lpips_total_kernel: d = sum_k d_k.
//
// No atomics: the same inputs give the same bits.  (n_a - n_b)^2 = (n_b - n_a)^2 bit for bit and both images run through the same
// code, so d(a, b) = d(b, a); an identical pair gives 0 and an all-zero feature vector normalises to 0, never NaN.  The pairs go
// through one workspace in groups whose size follows from H and W alone (up to 8 pairs of small frames, so that the deep layers'
// few hundred pixels per image still fill the card; 1 pair of large ones); no sum crosses a pair, so a pair's value does not depend
// on its group.  Every launch is on the caller's stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/r2l_hip.h"
#include "r2l_host_util.h"

#define LPIPS_LAYERS 5
#define LPIPS_MIN_DIM 31                 // 31 -> 7 -> 3 -> 1: the second pool needs 3 rows and columns
#define LPIPS_MAX_DIM 32768
#define LPIPS_DIST_PIX 32                // pixels per block of lpips_dist_kernel: 4 waves x 8
#define LPIPS_MAX_PER_LANE 6             // 384 channels over 64 lanes
#define LPIPS_MAX_GROUP 8                // pairs per pass through the workspace, at the most
#define LPIPS_GROUP_PIXELS 4096          // ... as many as bring conv 3 .. 5 to this many pixels per side of the pairs (64 row tiles)

struct r2l_lpips_ctx {
    DevBuf<float> dev;                   // one allocation: weights, biases, lin vectors; the rest are views into it
    const float* w[LPIPS_LAYERS] = {};   // [out][kh kw in]: the state_dict's [out][in][kh][kw] reordered
    const float* b[LPIPS_LAYERS] = {};
    const float* lin[LPIPS_LAYERS] = {};
};

namespace {

// torchvision's AlexNet features 0, 3, 6, 8, 10
const int kCin[LPIPS_LAYERS] = {3, 64, 192, 384, 256}, kCout[LPIPS_LAYERS] = {64, 192, 384, 256, 256}, kSize[LPIPS_LAYERS] = {11, 5, 3, 3, 3},
          kStride[LPIPS_LAYERS] = {4, 1, 1, 1, 1}, kPad[LPIPS_LAYERS] = {2, 2, 1, 1, 1};

struct LpipsMap {                        // the first gather's affine map and scaling layer, image a / b
    float lo[2], mul[2], add[2], shift[3], scale[3];
};

template <bool FIRST>
__global__ void __launch_bounds__(256)
    lpips_gather_kernel(const float* __restrict__ src_a, const float* __restrict__ src_b, int h, int w, int C, int ksize, int stride, int pad,
                        int oh, int ow, const LpipsMap M, float* __restrict__ patch) {
    // image j of the group: FIRST: pair j / 2 of the stacks src_a (j even) / src_b (j odd); else feature map j behind src_a
    const int P = oh * ow, row = blockIdx.x;             // row < images P
    const int j = row / P, p = row - j * P;
    const int oy = p / ow, ox = p - oy * ow;
    const int y0 = oy * stride - pad, x0 = ox * stride - pad;
    const int K = C * ksize * ksize, side = j & 1;
    const float* __restrict__ src = FIRST ? ((side ? src_b : src_a) + (size_t)(j >> 1) * h * w * C) : src_a + (size_t)j * h * w * C;
    float* __restrict__ out = patch + (size_t)row * K;
    for (int col = threadIdx.x; col < K; col += 256) {
        const int t = col / C, c = col - t * C;
        const int ky = t / ksize, kx = t - ky * ksize;
        const int y = y0 + ky, x = x0 + kx;
        float v = 0.0f;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            v = src[((size_t)y * w + x) * C + c];
            if (FIRST) v = ((M.mul[side] * (v - M.lo[side]) + M.add[side]) - M.shift[c]) / M.scale[c];
        }
        out[col] = v;
    }
}

// F.max_pool2d(x, 3, 2): a NaN stays a NaN
__global__ void __launch_bounds__(64)
    lpips_pool_kernel(const float* __restrict__ src, int h, int w, int C, int oh, int ow, float* __restrict__ dst) {
    const int P = oh * ow, row = blockIdx.x;             // row < images P
    const int img = row / P, p = row - img * P;
    const int oy = p / ow, ox = p - oy * ow;
    const float* __restrict__ in = src + ((size_t)img * h * w + (size_t)(2 * oy) * w + 2 * ox) * C;
    for (int c = threadIdx.x; c < C; c += 64) {
        float m = in[c];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float v = in[((size_t)j * w + i) * C + c];
                m = (v > m || v != v) ? v : m;
            }
        dst[(size_t)row * C + c] = m;
    }
}

__device__ __forceinline__ double wave_sum(double v) {    // a butterfly: every lane ends with the same sum, in a fixed order
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__global__ void __launch_bounds__(256)
    lpips_dist_kernel(const float* __restrict__ feat, int P, int C, const float* __restrict__ lin, float* __restrict__ partial) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* __restrict__ fa = feat + (size_t)(2 * blockIdx.y) * P * C;      // blockIdx.y: the pair of the group
    const float* __restrict__ fb = fa + (size_t)P * C;
    float lw[LPIPS_MAX_PER_LANE];
#pragma unroll
    for (int i = 0; i < LPIPS_MAX_PER_LANE; ++i) lw[i] = lane + 64 * i < C ? lin[lane + 64 * i] : 0.0f;
    double sum = 0.0;
    for (int j = 0; j < LPIPS_DIST_PIX / 4; ++j) {
        const int p = blockIdx.x * LPIPS_DIST_PIX + wave * (LPIPS_DIST_PIX / 4) + j;      // the same for every lane of the wave
        if (p >= P) break;
        float va[LPIPS_MAX_PER_LANE], vb[LPIPS_MAX_PER_LANE];
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int i = 0; i < LPIPS_MAX_PER_LANE; ++i) {
            const int c = lane + 64 * i;
            va[i] = c < C ? fa[(size_t)p * C + c] : 0.0f;
            vb[i] = c < C ? fb[(size_t)p * C + c] : 0.0f;
            sa += (double)va[i] * (double)va[i];
            sb += (double)vb[i] * (double)vb[i];
        }
        const float den_a = sqrtf((float)wave_sum(sa)) + 1e-10f, den_b = sqrtf((float)wave_sum(sb)) + 1e-10f;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < LPIPS_MAX_PER_LANE; ++i) {
            const float d = va[i] / den_a - vb[i] / den_b;
            acc += (double)lw[i] * ((double)d * (double)d);
        }
        sum += wave_sum(acc);
    }
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.y * gridDim.x + blockIdx.x] = (float)(((red[0] + red[1]) + red[2]) + red[3]);
}

__global__ void __launch_bounds__(256) lpips_mean_kernel(const float* __restrict__ partial, int n, double count, float* __restrict__ out) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    partial += (size_t)blockIdx.x * n;                    // blockIdx.x: the pair of the group
    out += blockIdx.x * 8;
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

__global__ void lpips_total_kernel(const float* __restrict__ dk, float* __restrict__ d, float* __restrict__ layers) {
    if (threadIdx.x != 0) return;
    const int g = blockIdx.x;                             // the pair of the group
    double s = 0.0;
    for (int k = 0; k < LPIPS_LAYERS; ++k) {
        s += (double)dk[g * 8 + k];
        if (layers) layers[g * LPIPS_LAYERS + k] = dk[g * 8 + k];
    }
    d[g] = (float)s;
}

// sizes, pairs per group and workspace offsets (in floats) for H x W pairs
struct LpipsPlan {
    int group;
    int in_h[LPIPS_LAYERS], in_w[LPIPS_LAYERS];          // what conv k reads ...
    int h[LPIPS_LAYERS], w[LPIPS_LAYERS];                // ... and writes
    long long off_f[LPIPS_LAYERS], off_pool[2], off_patch, off_partial, off_dk, total;
};

void lpips_plan(int H, int W, LpipsPlan* pl) {
    int h = H, w = W;
    for (int k = 0; k < LPIPS_LAYERS; ++k) {
        if (k == 1 || k == 2) h = (h - 3) / 2 + 1, w = (w - 3) / 2 + 1;      // the pools in front of conv 2 and conv 3
        pl->in_h[k] = h, pl->in_w[k] = w;
        h = (h + 2 * kPad[k] - kSize[k]) / kStride[k] + 1;
        w = (w + 2 * kPad[k] - kSize[k]) / kStride[k] + 1;
        pl->h[k] = h, pl->w[k] = w;
    }
    const long long deep = (long long)pl->h[4] * pl->w[4];
    const long long want = (LPIPS_GROUP_PIXELS + deep - 1) / deep;
    pl->group = want < 1 ? 1 : (want > LPIPS_MAX_GROUP ? LPIPS_MAX_GROUP : (int)want);
    const long long images = 2ll * pl->group;
    long long at = 0, patch = 0;
    for (int k = 0; k < LPIPS_LAYERS; ++k) {
        const long long P = (long long)pl->h[k] * pl->w[k];
        pl->off_f[k] = at;
        at += images * P * kCout[k];
        const long long need = images * P * kCin[k] * kSize[k] * kSize[k];
        if (need > patch) patch = need;
    }
    for (int k = 0; k < 2; ++k) {
        pl->off_pool[k] = at;
        at += images * pl->in_h[k + 1] * pl->in_w[k + 1] * kCout[k];
    }
    pl->off_patch = at;
    at += patch;
    pl->off_partial = at;
    at += pl->group * (((long long)pl->h[0] * pl->w[0] + LPIPS_DIST_PIX - 1) / LPIPS_DIST_PIX);
    pl->off_dk = at;
    at += pl->group * 8;
    pl->total = at;
}

int lpips_check_size(const char* who, int H, int W) {
    if (H < LPIPS_MIN_DIM || W < LPIPS_MIN_DIM || H > LPIPS_MAX_DIM || W > LPIPS_MAX_DIM)
        return r2l_set_error(R2L_EINVAL, "%s: H=%d W=%d (%d .. %d each: the trunk's second pool needs 3 rows and columns)", who, H, W, LPIPS_MIN_DIM,
                             LPIPS_MAX_DIM);
    return R2L_OK;
}

}  // namespace

extern "C" {

int r2l_lpips_create(r2l_lpips_ctx** out, const float* const* tensors_host, int n_tensors) {
    if (!out || !tensors_host || n_tensors != 3 * LPIPS_LAYERS)
        return r2l_set_error(R2L_EINVAL, "r2l_lpips_create: %d tensors (5 conv weights, 5 biases, 5 lin vectors = 15), out or tensors NULL", n_tensors);
    for (int i = 0; i < n_tensors; ++i)
        if (!tensors_host[i]) return r2l_set_error(R2L_EINVAL, "r2l_lpips_create: tensor %d is NULL", i);
    int e = r2l_require_gfx950(nullptr);
    if (e) return e;
    size_t off[3 * LPIPS_LAYERS + 1];
    off[0] = 0;
    for (int i = 0; i < 3 * LPIPS_LAYERS; ++i) {
        const int k = i % LPIPS_LAYERS;
        off[i + 1] = off[i] + (i < LPIPS_LAYERS ? (size_t)kCout[k] * kCin[k] * kSize[k] * kSize[k] : (size_t)kCout[k]);
    }
    std::vector<float> host(off[3 * LPIPS_LAYERS]);
    for (int i = 0; i < 3 * LPIPS_LAYERS; ++i) {
        if (i >= LPIPS_LAYERS) {
            for (size_t j = 0; j < off[i + 1] - off[i]; ++j) host[off[i] + j] = tensors_host[i][j];
            continue;
        }
        const int C = kCin[i], kk = kSize[i] * kSize[i];          // [out][c][tap] -> [out][tap][c]: the gather's column order
        for (int o = 0; o < kCout[i]; ++o)
            for (int c = 0; c < C; ++c)
                for (int t = 0; t < kk; ++t) host[off[i] + ((size_t)o * kk + t) * C + c] = tensors_host[i][((size_t)o * C + c) * kk + t];
    }
    r2l_lpips_ctx* l = new r2l_lpips_ctx();
    e = l->dev.upload(host.data(), host.size(), "r2l_lpips_create");
    if (e) {
        delete l;
        return e;
    }
    for (int k = 0; k < LPIPS_LAYERS; ++k) {
        l->w[k] = l->dev + off[k];
        l->b[k] = l->dev + off[LPIPS_LAYERS + k];
        l->lin[k] = l->dev + off[2 * LPIPS_LAYERS + k];
    }
    *out = l;
    return R2L_OK;
}

void r2l_lpips_destroy(r2l_lpips_ctx* l) {
    if (l) delete l;
}

long long r2l_lpips_workspace_floats(int H, int W) {
    int e = lpips_check_size("r2l_lpips_workspace_floats", H, W);
    if (e) return e;
    LpipsPlan pl;
    lpips_plan(H, W, &pl);
    return pl.total;
}

int r2l_lpips(const r2l_lpips_ctx* l, const float* a_dev, const float* b_dev, int n_img, int H, int W, float a_lo, float a_mul, float a_add, float b_lo,
              float b_mul, float b_add, float* d_dev, float* layers_dev, float* workspace_dev, long long workspace_floats, void* stream) {
    if (n_img < 0) return r2l_set_error(R2L_EINVAL, "bad argument to r2l_lpips (n_img=%d)", n_img);
    int e = lpips_check_size("r2l_lpips", H, W);
    if (e) return e;
    if (n_img == 0) return R2L_OK;
    if (!l) return r2l_set_error(R2L_EINVAL, "r2l_lpips: the context is NULL (r2l_lpips_create)");
    if (!a_dev || !b_dev) return r2l_set_error(R2L_EINVAL, "r2l_lpips: an image stack is NULL");
    if (!d_dev || !workspace_dev) return r2l_set_error(R2L_EINVAL, "r2l_lpips: d / workspace is NULL");
    LpipsPlan pl;
    lpips_plan(H, W, &pl);
    if (workspace_floats < pl.total)
        return r2l_set_error(R2L_EINVAL, "r2l_lpips: a workspace of %lld floats, %d x %d needs %lld (r2l_lpips_workspace_floats)", workspace_floats, H, W,
                             pl.total);
    if (((uintptr_t)a_dev & 3) || ((uintptr_t)b_dev & 3) || ((uintptr_t)d_dev & 3) || ((uintptr_t)layers_dev & 3) || ((uintptr_t)workspace_dev & 3))
        return r2l_set_error(R2L_EINVAL, "r2l_lpips: every buffer must be 4-byte aligned");
    e = r2l_require_gfx950(nullptr);
    if (e) return e;
    LpipsMap M;
    M.lo[0] = a_lo, M.mul[0] = a_mul, M.add[0] = a_add;
    M.lo[1] = b_lo, M.mul[1] = b_mul, M.add[1] = b_add;
    M.shift[0] = -0.030f, M.shift[1] = -0.088f, M.shift[2] = -0.188f;
    M.scale[0] = 0.458f, M.scale[1] = 0.448f, M.scale[2] = 0.450f;
    hipStream_t s = (hipStream_t)stream;
    float* const ws = workspace_dev;
    float* const patch = ws + pl.off_patch;
    float* const partial = ws + pl.off_partial;
    float* const dk = ws + pl.off_dk;
    const size_t hw3 = (size_t)H * W * 3;
    for (int n0 = 0; n0 < n_img; n0 += pl.group) {      // group after group through one workspace: the stream orders them
        const int pairs = n_img - n0 < pl.group ? n_img - n0 : pl.group, images = 2 * pairs;
        for (int k = 0; k < LPIPS_LAYERS; ++k) {
            const int P = pl.h[k] * pl.w[k], K = kCin[k] * kSize[k] * kSize[k];
            float* const f = ws + pl.off_f[k];
            if (k == 0) {
                hipLaunchKernelGGL(lpips_gather_kernel<true>, dim3(images * P), dim3(256), 0, s, a_dev + n0 * hw3, b_dev + n0 * hw3, H, W, 3, kSize[k],
                                   kStride[k], kPad[k], pl.h[k], pl.w[k], M, patch);
            } else {
                const float* src = ws + pl.off_f[k - 1];
                if (k <= 2) {              // the pool in front of conv 2 and conv 3
                    float* const pooled = ws + pl.off_pool[k - 1];
                    hipLaunchKernelGGL(lpips_pool_kernel, dim3(images * pl.in_h[k] * pl.in_w[k]), dim3(64), 0, s, src, pl.h[k - 1], pl.w[k - 1], kCin[k],
                                       pl.in_h[k], pl.in_w[k], pooled);
                    src = pooled;
                }
                hipLaunchKernelGGL(lpips_gather_kernel<false>, dim3(images * P), dim3(256), 0, s, src, src, pl.in_h[k], pl.in_w[k], kCin[k], kSize[k],
                                   kStride[k], kPad[k], pl.h[k], pl.w[k], M, patch);
            }
            e = r2l_linear_forward_dev(l->w[k], l->b[k], kCout[k], K, patch, K, images * P, f, kCout[k], nullptr, 0, 1.0f, R2L_ACT_RELU, nullptr, 0,
                                       stream);
            if (e) return e;
            const int n_part = (P + LPIPS_DIST_PIX - 1) / LPIPS_DIST_PIX;
            hipLaunchKernelGGL(lpips_dist_kernel, dim3(n_part, pairs), dim3(256), 0, s, (const float*)f, P, kCout[k], l->lin[k], partial);
            hipLaunchKernelGGL(lpips_mean_kernel, dim3(pairs), dim3(256), 0, s, (const float*)partial, n_part, (double)P, dk + k);
        }
        hipLaunchKernelGGL(lpips_total_kernel, dim3(pairs), dim3(64), 0, s, (const float*)dk, d_dev + n0,
                           layers_dev ? layers_dev + (size_t)n0 * LPIPS_LAYERS : nullptr);
        hipError_t err = hipGetLastError();
        if (err != hipSuccess) return r2l_set_error(R2L_EHIP, "r2l_lpips launch: %s", hipGetErrorString(err));
    }
    return R2L_OK;
}

}  // extern "C"
