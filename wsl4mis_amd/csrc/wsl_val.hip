// On-device validation (ref: code/val_2D.py:18-50 test_single_volume, :90-124 test_single_volume_cct) -- the two host stages around the
// eval forward as device gathers:
//   wsl_val_zoom_in    scipy.ndimage.zoom(slice, (Ho / h, Wo / w), order=0) of up to 64 native slices of any sizes per launch, to the
//                      network size, with scipy's fill: where the coordinate of the last row / column lands above the array, 0.0f
//   wsl_val_labelmap   per native pixel: argmax over the C logits at the zoomed-back position (first maximum, like np.argmax), the label
//                      byte, and |pred == c|, |label == c|, |pred == c & label == c| per (volume, class) for Dice
// Both are launch- and HBM-bound gathers.  A lane owns four consecutive output bytes / floats (one 32-bit or 128-bit store where the
// address allows it); the C logits of a pixel stay in registers.  The counts are integers: lane -> wave (shuffles) -> workgroup (LDS)
// -> ONE 64-bit integer atomic per counter and workgroup, so the sums do not depend on the order (no float atomics, no workspace).
#include <math.h>
#include <stdint.h>

#include "wsl_rt.h"
#include "wsl_zoom.h"

namespace wsl {

constexpr int kValMaxC = 8;
constexpr int kValSlices = 64;     // slices per launch: the table travels as a kernel argument (64 * 16 + 8 B, 64 * 32 + 8 B)
constexpr int kValBlocksX = 16;    // workgroups per slice at most: each ends in 3 * C atomics, so a lane takes several pixel groups

struct ValSrcTable {
  int n;
  WslValSrc s[kValSlices];
};
struct ValDstTable {
  int n;
  WslValDst s[kValSlices];
};

// the value output sample (oy, ox) of the zoom from [h, w] reads: the nearest input sample, or scipy's fill
__device__ __forceinline__ float zoom_in_px(const float* img, int h, int w, int oy, int ox, double sy, double sx) {
  const bool outside = zoom0_outside(oy, sy, h) || zoom0_outside(ox, sx, w);
  const float v = img[(int64_t)zoom0_index(oy, sy, h) * w + zoom0_index(ox, sx, w)];     // (the index is clamped: always a valid read)
  return outside ? 0.f : v;
}

// VEC: Wo % 4 == 0 and a 16-byte aligned output -- a lane writes four samples of one row as one float4
template <bool VEC>
__global__ __launch_bounds__(256) void val_zoom_in_kernel(ValSrcTable t, float* out, int Ho, int Wo) {
  const WslValSrc& s = t.s[blockIdx.y];
  const int h = s.h, w = s.w;
  const double sy = zoom0_scale(h, Ho), sx = zoom0_scale(w, Wo);
  float* o = out + (int64_t)blockIdx.y * Ho * Wo;
  if constexpr (VEC) {
    const int G = (Ho * Wo) >> 2;
    for (int g = blockIdx.x * kThreads + threadIdx.x; g < G; g += gridDim.x * kThreads) {
      const int p = g * 4, oy = p / Wo, ox = p - oy * Wo;
      *reinterpret_cast<float4*>(o + p) = make_float4(zoom_in_px(s.img, h, w, oy, ox, sy, sx), zoom_in_px(s.img, h, w, oy, ox + 1, sy, sx),
                                                      zoom_in_px(s.img, h, w, oy, ox + 2, sy, sx), zoom_in_px(s.img, h, w, oy, ox + 3, sy, sx));
    }
  } else {
    for (int p = blockIdx.x * kThreads + threadIdx.x; p < Ho * Wo; p += gridDim.x * kThreads) {
      const int oy = p / Wo, ox = p - oy * Wo;
      o[p] = zoom_in_px(s.img, h, w, oy, ox, sy, sx);
    }
  }
}

// 64-bit integer add to global memory (the emulator runs the workgroups of a launch on several host threads)
__device__ __forceinline__ void val_count_add(int64_t* p, int64_t v) {
#ifdef WSL_HOST_EMUL
  __atomic_fetch_add(p, v, __ATOMIC_RELAXED);
#else
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
#endif
}

__device__ __forceinline__ int val_wave_sum(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// CT > 0: class count fixed at compile time; CT == 0: generic (C <= 8).  blockIdx.y = slice; a lane takes groups of four consecutive
// BYTES of the prediction, counted from the 4-byte boundary at or below s.pred: a group that lies inside the slice leaves as one
// aligned 32-bit store, the (at most two) groups that straddle its ends as single bytes -- nothing outside [pred, pred + h * w).
template <int CT>
__global__ __launch_bounds__(256) void val_labelmap_kernel(ValDstTable t, const float* z, int C_, int Hn, int Wn, int64_t* counts) {
  constexpr int KC = CT > 0 ? CT : kValMaxC;
  const int C = CT > 0 ? CT : C_;
  __shared__ int red[4][3 * kValMaxC];
  const WslValDst& s = t.s[blockIdx.y];
  const int h = s.h, w = s.w, hw = h * w;
  const int64_t plane = (int64_t)Hn * Wn;
  const float* zi = z + (int64_t)blockIdx.y * C * plane;
  const double sy = zoom0_scale(Hn, h), sx = zoom0_scale(Wn, w);     // zoom(label map, (h / Hn, w / Wn), order=0): network size -> native
  const int lead = (int)((size_t)s.pred & 3);                         // bytes between the boundary and the slice's first pixel
  uint8_t* const base = s.pred - lead;                                // 4-byte aligned
  const bool count = counts != nullptr && s.label != nullptr;
  int n_p[KC], n_l[KC], n_i[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) n_p[c] = n_l[c] = n_i[c] = 0;
  const int G = (lead + hw + 3) >> 2;
  for (int g = blockIdx.x * kThreads + threadIdx.x; g < G; g += gridDim.x * kThreads) {
    uint32_t word = 0;
    const int o0 = g * 4 - lead;     // pixel of the group's first byte (negative / >= hw: outside the slice)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = o0 + j;
      if (o < 0 || o >= hw) continue;
      const int y = o / w, x = o - y * w;
      const int64_t src = (int64_t)zoom0_index(y, sy, Hn) * Wn + zoom0_index(x, sx, Wn);
      const bool outside = zoom0_outside(y, sy, Hn) || zoom0_outside(x, sx, Wn);     // scipy's fill: label 0 there
      float zz[KC];
#pragma unroll
      for (int c = 0; c < KC; ++c) zz[c] = c < C ? zi[(int64_t)c * plane + src] : 0.f;
      int p = 0;
      float m = zz[0];
#pragma unroll
      for (int c = 1; c < KC; ++c)
        if (c < C && zz[c] > m) m = zz[c], p = c;     // strictly greater: the FIRST maximum wins a tie
      p = outside ? 0 : p;
      word |= (uint32_t)p << (8 * j);
      if (count) {
        const int l = s.label[o];
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          n_p[c] += p == c ? 1 : 0;
          n_l[c] += l == c ? 1 : 0;
          n_i[c] += (p == c && l == c) ? 1 : 0;
        }
      }
    }
    if (o0 >= 0 && o0 + 4 <= hw) {
      *reinterpret_cast<uint32_t*>(base + (int64_t)g * 4) = word;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (o0 + j >= 0 && o0 + j < hw) s.pred[o0 + j] = (uint8_t)(word >> (8 * j));
    }
  }
  if (!count) return;     // (uniform over the workgroup: nobody waits at the barrier below)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    const int a = val_wave_sum(n_p[c]), b = val_wave_sum(n_l[c]), d = val_wave_sum(n_i[c]);
    if (lane == 0) red[wave][3 * c] = a, red[wave][3 * c + 1] = b, red[wave][3 * c + 2] = d;
  }
  __syncthreads();
  if ((int)threadIdx.x < 3 * C) {
    const int64_t v = (int64_t)red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (v) val_count_add(counts + (int64_t)s.group * C * 3 + threadIdx.x, v);
  }
}

static bool val_aligned(const void* p, size_t a) { return ((size_t)p & (a - 1)) == 0; }
static int val_grid_x(int64_t groups) {
  const int64_t b = (groups + kThreads - 1) / kThreads;
  return (int)(b < 1 ? 1 : (b > kValBlocksX ? kValBlocksX : b));
}

}  // namespace wsl

using namespace wsl;

extern "C" int wsl_val_zoom_in(const WslValSrc* slices, int n, float* out, int Ho, int Wo, void* stream) {
  WSL_REQUIRE(slices && out && n > 0 && Ho > 0 && Wo > 0 && (int64_t)Ho * Wo < (int64_t)1 << 30, "val_zoom_in: bad arguments");
  for (int k = 0; k < n; ++k)     // every slice is checked before the first launch: a refused call has written nothing
    WSL_REQUIRE(slices[k].img && slices[k].h > 0 && slices[k].w > 0 && (int64_t)slices[k].h * slices[k].w < (int64_t)1 << 30,
                "val_zoom_in: slice %d is malformed", k);
  const int64_t opx = (int64_t)Ho * Wo;
  const bool vec = Wo % 4 == 0 && val_aligned(out, 16);
  for (int b0 = 0; b0 < n; b0 += kValSlices) {
    ValSrcTable t;
    t.n = n - b0 < kValSlices ? n - b0 : kValSlices;
    for (int k = 0; k < t.n; ++k) t.s[k] = slices[b0 + k];
    const dim3 grid(val_grid_x(vec ? opx >> 2 : opx), t.n);
    if (vec) WSL_LAUNCH((val_zoom_in_kernel<true>), grid, dim3(kThreads), 0, stream, t, out + b0 * opx, Ho, Wo);
    else WSL_LAUNCH((val_zoom_in_kernel<false>), grid, dim3(kThreads), 0, stream, t, out + b0 * opx, Ho, Wo);
  }
  return check_launch("val_zoom_in_kernel");
}

extern "C" int wsl_val_labelmap(const float* z, const WslValDst* slices, int n, int C, int Hn, int Wn, int64_t* counts, int n_groups,
                                void* stream) {
  WSL_REQUIRE(z && slices && n > 0 && Hn > 0 && Wn > 0 && (int64_t)Hn * Wn < (int64_t)1 << 30, "val_labelmap: bad arguments");
  WSL_REQUIRE(C >= 1 && C <= kValMaxC, "val_labelmap: %d classes (1 <= C <= %d)", C, kValMaxC);
  for (int k = 0; k < n; ++k) {
    const WslValDst& s = slices[k];
    WSL_REQUIRE(s.pred && s.h > 0 && s.w > 0 && (int64_t)s.h * s.w < (int64_t)1 << 30, "val_labelmap: slice %d is malformed", k);
    WSL_REQUIRE(!counts || (s.group >= 0 && s.group < n_groups), "val_labelmap: slice %d has group %d outside [0, %d)", k, s.group, n_groups);
  }
  for (int b0 = 0; b0 < n; b0 += kValSlices) {
    ValDstTable t;
    t.n = n - b0 < kValSlices ? n - b0 : kValSlices;
    int64_t px = 1;
    for (int k = 0; k < t.n; ++k) {
      t.s[k] = slices[b0 + k];
      px = (int64_t)t.s[k].h * t.s[k].w > px ? (int64_t)t.s[k].h * t.s[k].w : px;
    }
    const dim3 grid(val_grid_x((px + 6) >> 2), t.n);
    const float* zb = z + (int64_t)b0 * C * Hn * Wn;
    if (C == 4) WSL_LAUNCH((val_labelmap_kernel<4>), grid, dim3(kThreads), 0, stream, t, zb, C, Hn, Wn, counts);
    else WSL_LAUNCH((val_labelmap_kernel<0>), grid, dim3(kThreads), 0, stream, t, zb, C, Hn, Wn, counts);
  }
  return check_launch("val_labelmap_kernel");
}
