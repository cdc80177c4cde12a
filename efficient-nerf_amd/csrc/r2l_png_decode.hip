// PNG on the way in: the zlib streams of a batch of 8-bit PNG files of one shape to pixels on the device, one C-ABI call per batch.  The
// host side is png.decode_pngs; the decoder itself is png_inflate.h, the text the CPU runs under the sanitizers.  Two launches:
//   inflate   one workgroup of ONE wave per stream (deflate is serial along a stream; the parallelism is across the files).  The wave's
//             lanes decode the same bits and share the table building, the match and stored copies, the flushes of the 64 KiB window
//             in LDS to the workspace and the Adler-32 sums (png_inflate.h).  The stream's status goes to status[k].
//   unfilter  one workgroup of four waves per picture whose status is 0, 64 rows at a time.  Lane k of wave 0 reconstructs row r0 + k
//             one pixel behind lane k - 1: left and up-left are the lane's own registers, up arrives from lane k - 1 by one cross-lane
//             move per step, so the W x 64 dependent steps of a band become W + 63.  The four waves stage the skewed tile of 64 steps
//             through LDS (coalesced byte loads of the filtered rows, coalesced stores of the pixels); row r0 - 1, which the previous
//             band stored, is staged with it for lane 0.
// No atomics; the same streams give the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/r2l_hip.h"
#include "png_inflate.h"
#include "r2l_host_util.h"

namespace {

constexpr int PNGD_MAX_DIM = 16384;       // H (W C + 1) stays below 2^31
constexpr int PNGD_ROWS = 64;             // rows of a band: the lanes of the wave that walks it
constexpr int PNGD_STEPS = 64;            // steps of a tile
constexpr int PNGD_PITCH = PNGD_STEPS * 4 + 4;      // bytes of a tile row: 65 words, so that the lanes' rows start on different banks
constexpr int PNGD_THREADS = 256;

struct png_wave {      // the 64 lanes of the workgroup's only wave
    __device__ unsigned lane() const { return threadIdx.x; }
    __device__ unsigned width() const { return 64; }
    __device__ void sync() const { __syncthreads(); }      // barrier and workgroup-scope fence: LDS and global writes before it are visible after it
    __device__ unsigned uniform(unsigned v) const { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }
};

__global__ __launch_bounds__(64) void png_inflate_kernel(const unsigned char* __restrict__ z, const long long* __restrict__ offsets, int H,
                                                         int row_bytes, long long raw_pitch, unsigned char* __restrict__ raw,
                                                         int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char png_lds[];
    png_inflate_mem* m = reinterpret_cast<png_inflate_mem*>(png_lds);
    const int img = blockIdx.x;
    const long long o0 = offsets[img], o1 = offsets[img + 1];
    int st = R2L_PNG_BAD_OFFSETS;
    if (o0 >= 0 && o1 >= o0 && o1 - o0 < 0x7fffffffll) {
        png_wave co;
        st = png_inflate(co, m, z + o0, (unsigned)(o1 - o0), raw + img * raw_pitch, (unsigned)H, (unsigned)row_bytes, (uint32_t*)nullptr);
    }
    if (threadIdx.x == 0) status[img] = st;
}

__device__ inline unsigned pngd_pack(const unsigned char* p, int C) {
    unsigned v = 0;
    for (int ch = 0; ch < C; ++ch) v |= (unsigned)p[ch] << (8 * ch);
    return v;
}

__global__ __launch_bounds__(PNGD_THREADS) void png_unfilter_kernel(const unsigned char* __restrict__ raw, long long raw_pitch, int H, int W,
                                                                    int C, const int* __restrict__ status, unsigned char* out) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[PNGD_ROWS][PNGD_PITCH];
    __shared__ __attribute__((aligned(16))) unsigned char above[PNGD_STEPS * 4];
    const int img = blockIdx.x;
    if (status[img] != 0) return;      // the whole workgroup alike
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stride = W * C, row_bytes = stride + 1, tile_bytes = PNGD_STEPS * C;
    const unsigned char* src = raw + img * raw_pitch;
    unsigned char* dst = out + (long long)img * H * stride;
    for (int r0 = 0; r0 < H; r0 += PNGD_ROWS) {
        const int rows = H - r0 < PNGD_ROWS ? H - r0 : PNGD_ROWS;
        const unsigned ft = (wave == 0 && lane < rows) ? src[(long long)(r0 + lane) * row_bytes] : 0u;
        unsigned left = 0, upleft = 0;      // the lane's last pixel (0 outside the row), and what was above it
        for (int t0 = 0; t0 < W + rows - 1; t0 += PNGD_STEPS) {
            // in: row k takes the pixels t0 - k .. t0 - k + 63 of its row, where they exist
            for (int k = wave; k < rows; k += PNGD_THREADS / 64) {
                const long long row = (long long)(r0 + k) * row_bytes + 1;
                for (int j = lane; j < tile_bytes; j += 64) {
                    const int bx = (t0 - k) * C + j;
                    if (bx >= 0 && bx < stride) tile[k][j] = src[row + bx];
                }
            }
            if (r0 > 0)
                for (int j = tid; j < tile_bytes; j += PNGD_THREADS) {
                    const int bx = t0 * C + j;
                    if (bx < stride) above[j] = dst[(long long)(r0 - 1) * stride + bx];
                }
            __syncthreads();
            if (wave == 0) {
                for (int i = 0; i < PNGD_STEPS; ++i) {
                    const int x = t0 + i - lane;
                    unsigned up = __shfl_up(left, 1, 64);      // lane k - 1 was at pixel x of its row one step ago
                    if (lane == 0) up = (r0 > 0 && t0 + i < W) ? pngd_pack(&above[i * C], C) : 0u;
                    unsigned cur = 0;
                    if (lane < rows && x >= 0 && x < W) {
                        unsigned char* p = &tile[lane][i * C];
                        for (int ch = 0; ch < C; ++ch) {
                            const int sh = 8 * ch;
                            const unsigned v = png_recon(ft, p[ch], (left >> sh) & 255u, (up >> sh) & 255u, (upleft >> sh) & 255u);
                            p[ch] = (unsigned char)v;
                            cur |= v << sh;
                        }
                    }
                    upleft = up;
                    left = cur;
                }
            }
            __syncthreads();
            // out: the same bytes of the tile
            for (int k = wave; k < rows; k += PNGD_THREADS / 64) {
                const long long row = (long long)(r0 + k) * stride;
                for (int j = lane; j < tile_bytes; j += 64) {
                    const int bx = (t0 - k) * C + j;
                    if (bx >= 0 && bx < stride) dst[row + bx] = tile[k][j];
                }
            }
            __syncthreads();      // the tile is free again, and row r0 + 63 is visible to the band that reads it as `above`
        }
    }
}

int pngd_check(const char* who, int n_img, int H, int W, int C) {
    if (n_img < 0 || n_img > 65535) return r2l_set_error(R2L_EINVAL, "%s: n_img = %d (0 .. 65535)", who, n_img);
    if (H < 1 || W < 1 || H > PNGD_MAX_DIM || W > PNGD_MAX_DIM)
        return r2l_set_error(R2L_EINVAL, "%s: H=%d W=%d (1 .. %d each)", who, H, W, PNGD_MAX_DIM);
    if (C < 1 || C > 4) return r2l_set_error(R2L_EINVAL, "%s: C = %d bytes per pixel (1 gray, 2 gray + alpha, 3 RGB, 4 RGBA)", who, C);
    return R2L_OK;
}
long long pngd_raw_pitch(int H, int W, int C) { return ((long long)H * ((long long)W * C + 1) + 15) & ~15ll; }

}  // namespace

extern "C" {

long long r2l_png_decode_workspace_bytes(int n_img, int H, int W, int C) {
    int e = pngd_check("r2l_png_decode_workspace_bytes", n_img, H, W, C);
    if (e) return e;
    return n_img * pngd_raw_pitch(H, W, C);
}

int r2l_png_decode(const unsigned char* zstreams_dev, const long long* offsets_dev, int n_img, int H, int W, int C, void* workspace_dev,
                   long long workspace_bytes, unsigned char* out_dev, int* status_dev, void* stream) {
    int e = pngd_check("r2l_png_decode", n_img, H, W, C);
    if (e) return e;
    if (n_img == 0) return R2L_OK;
    if (!zstreams_dev || !offsets_dev) return r2l_set_error(R2L_EINVAL, "r2l_png_decode: streams / offsets is NULL");
    if (!workspace_dev || !out_dev || !status_dev) return r2l_set_error(R2L_EINVAL, "r2l_png_decode: workspace / out / status is NULL");
    const long long pitch = pngd_raw_pitch(H, W, C);
    if (workspace_bytes < n_img * pitch)
        return r2l_set_error(R2L_EINVAL, "r2l_png_decode: a workspace of %lld bytes, %d images of %d x %d x %d need %lld (r2l_png_decode_workspace_bytes)",
                             workspace_bytes, n_img, H, W, C, n_img * pitch);
    if (((uintptr_t)offsets_dev & 7) || ((uintptr_t)workspace_dev & 15) || ((uintptr_t)status_dev & 3))
        return r2l_set_error(R2L_EINVAL, "r2l_png_decode: alignment (offsets 8, status 4, workspace 16 bytes)");
    e = r2l_require_gfx950(nullptr);
    if (e) return e;

    static std::atomic<bool> attr_set[64];      // zero-initialised; the opt-in to more than 64 KiB of LDS is per device and idempotent
    int dev = 0;
    HIPCHK(hipGetDevice(&dev), "r2l_png_decode: hipGetDevice");
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&png_inflate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)sizeof(png_inflate_mem)),
               "r2l_png_decode: LDS opt-in");
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    hipStream_t s = (hipStream_t)stream;
    unsigned char* raw = (unsigned char*)workspace_dev;
    hipLaunchKernelGGL(png_inflate_kernel, dim3(n_img), dim3(64), sizeof(png_inflate_mem), s, zstreams_dev, offsets_dev, H, W * C + 1, pitch, raw,
                       status_dev);
    hipLaunchKernelGGL(png_unfilter_kernel, dim3(n_img), dim3(PNGD_THREADS), 0, s, (const unsigned char*)raw, pitch, H, W, C,
                       (const int*)status_dev, out_dev);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return r2l_set_error(R2L_EHIP, "r2l_png_decode launch: %s", hipGetErrorString(err));
    return R2L_OK;
}

}  // extern "C"
