// The byte every image writer here makes of a rendered value, stated once for the encoders (r2l_mjpeg.hip, r2l_png.hip).
#pragma once
#include <hip/hip_runtime.h>

// frontend.to8b: floor(255 clamp(x, 0, 1)); fmaxf returns the other operand for a NaN, so a NaN is 0
__device__ inline float r2l_to8b(float x) { return floorf(255.0f * fminf(fmaxf(x, 0.0f), 1.0f)); }
