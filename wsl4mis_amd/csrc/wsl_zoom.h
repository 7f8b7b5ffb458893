// The nearest-neighbour index arithmetic of scipy.ndimage shared by the data-path kernels (wsl_data.hip, wsl_s2l.hip).
// Coordinates are computed in double without contraction, in the order that reproduces scipy bit for bit on the tests.
#pragma once
#include <math.h>

#include "wsl_rt.h"

namespace wsl {

#ifdef WSL_HOST_EMUL
static inline double dmul(double a, double b) { return a * b; }   // emulator TU is built with -ffp-contract=off
static inline double dadd(double a, double b) { return a + b; }
#else
__device__ __forceinline__ double dmul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double dadd(double a, double b) { return __dadd_rn(a, b); }
#endif

// scipy.ndimage.zoom(order 0) from `in` to `out` samples along one axis: scale = (in - 1) / (out - 1) (0 when out == 1)
__host__ __device__ __forceinline__ double zoom0_scale(int in, int out) { return out > 1 ? (double)(in - 1) / (double)(out - 1) : 0.0; }
// ... and the input index output sample o reads: floor(o * scale + 0.5), kept inside the array
__device__ __forceinline__ int zoom0_index(int o, double scale, int in) {
  const int i = (int)floor(dadd(dmul((double)o, scale), 0.5));
  return i < 0 ? 0 : (i > in - 1 ? in - 1 : i);
}

// scipy maps the coordinate o * scale with mode='constant' before it rounds: a coordinate above in - 1 is OUTSIDE and reads cval.
// (out - 1) * ((in - 1) / (out - 1)) exceeds in - 1 by one ulp for some (in, out) -- 26 -> 12, 105 <- 256, ... -- and the last row /
// column of such a zoom is the fill value, not the edge pixel.  The Scribble2Label kernels reproduce that (wsl_s2l.hip).
__device__ __forceinline__ bool zoom0_outside(int o, double scale, int in) { return dmul((double)o, scale) > (double)(in - 1); }

}  // namespace wsl
