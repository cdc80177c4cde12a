// Host-only driver of the r2l_png_* entry points for an AddressSanitizer / UBSan build (make -C efficient-nerf_amd/csrc asan_png): the
// layout arithmetic over the whole range of sizes and every refusal of r2l_png_encode.  No call here reaches a device.
#include <stdio.h>
#include <string.h>

#include "../include/r2l_hip.h"

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAILED line %d: %s\n", __LINE__, #c);         \
            ++fails;                                              \
        }                                                         \
    } while (0)

int main() {
    const int dims[] = {1, 2, 3, 7, 85, 86, 87, 173, 504, 800, 5461, 5462, 16383, 16384};
    const int n_dims = (int)(sizeof(dims) / sizeof(dims[0]));
    for (int i = 0; i < n_dims; ++i)
        for (int j = 0; j < n_dims; ++j) {
            const int H = dims[i], W = dims[j];
            int rows = -1, segs = -1;
            CHECK(r2l_png_layout(H, W, &rows, &segs) == R2L_OK);
            const long long S = 1 + 3ll * W;
            CHECK(rows >= 1 && rows <= H && segs == (H + rows - 1) / rows);
            CHECK(rows * S <= 16384 || rows == 1);
            CHECK(rows * S <= 65535);
            CHECK(r2l_png_max_frame_bytes(H, W) == 51 + 17ll * segs + H * S);
            const long long one = r2l_png_workspace_bytes(1, H, W), many = r2l_png_workspace_bytes(65535, H, W);
            CHECK(one >= H * S + segs * (rows * S + 5) && many > one && many <= 65535 * one);
            CHECK(r2l_png_workspace_bytes(0, H, W) == 0);
        }
    int rows = 0, segs = 0;
    CHECK(r2l_png_layout(0, 8, &rows, &segs) == R2L_EINVAL && strstr(r2l_last_error(), "H=0"));
    CHECK(r2l_png_layout(8, 16385, &rows, &segs) == R2L_EINVAL && strstr(r2l_last_error(), "W=16385"));
    CHECK(r2l_png_layout(8, 8, nullptr, &segs) == R2L_EINVAL);
    CHECK(r2l_png_max_frame_bytes(-1, 8) == R2L_EINVAL && r2l_png_workspace_bytes(65536, 8, 8) == R2L_EINVAL);
    const long long pitch = r2l_png_max_frame_bytes(16, 24), need = r2l_png_workspace_bytes(2, 16, 24);
    float* rgb = (float*)(1 << 20);
    unsigned char* out = (unsigned char*)(1 << 21);
    long long* sizes = (long long*)(1 << 22);
    void* ws = (void*)(1 << 23);
    CHECK(r2l_png_encode(rgb, 2, 0, 24, -1, ws, need, out, pitch, sizes, nullptr) == R2L_EINVAL && strstr(r2l_last_error(), "H=0"));
    CHECK(r2l_png_encode(rgb, 2, 16, 0, -1, ws, need, out, pitch, sizes, nullptr) == R2L_EINVAL && strstr(r2l_last_error(), "W=0"));
    CHECK(r2l_png_encode(rgb, -1, 16, 24, -1, ws, need, out, pitch, sizes, nullptr) == R2L_EINVAL && strstr(r2l_last_error(), "n_img"));
    CHECK(r2l_png_encode(rgb, 2, 16, 24, 5, ws, need, out, pitch, sizes, nullptr) == R2L_EINVAL && strstr(r2l_last_error(), "filter = 5"));
    CHECK(r2l_png_encode(rgb, 2, 16, 24, -1, ws, need, out, pitch - 1, sizes, nullptr) == R2L_EINVAL && strstr(r2l_last_error(), "pitch"));
    CHECK(r2l_png_encode(rgb, 2, 16, 24, -1, ws, need - 1, out, pitch, sizes, nullptr) == R2L_EINVAL && strstr(r2l_last_error(), "workspace"));
    CHECK(r2l_png_encode(nullptr, 2, 16, 24, -1, ws, need, out, pitch, sizes, nullptr) == R2L_EINVAL);
    CHECK(r2l_png_encode(rgb, 2, 16, 24, -1, (char*)ws + 8, need, out, pitch, sizes, nullptr) == R2L_EINVAL && strstr(r2l_last_error(), "alignment"));
    CHECK(r2l_png_encode(nullptr, 0, 16, 24, -1, nullptr, 0, nullptr, 0, nullptr, nullptr) == R2L_OK);
    printf(fails ? "png_asan: %d check(s) failed\n" : "png_asan: all checks passed\n", fails);
    return fails ? 1 : 0;
}
