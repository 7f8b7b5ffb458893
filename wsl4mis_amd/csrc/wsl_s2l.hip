// Scribble2Label (ref: code/train_s2l.py, code/dataloaders/dataset_s2l.py) -- the three device pieces the recipe adds to pCE:
//   wsl_s2l_head_fwd_bwd      scribble CE + w_u * CE on thresholded pseudo labels read from the running prediction average
//                             (train_s2l.py:123-147), value and logit gradient
//   wsl_s2l_ensemble_update   that running average, per training slice at native resolution: softmax of the network-size logits,
//                             zoomed back with order 0, mixed in with an fp32 EMA (train_s2l.py:228-243)
//   wsl_augment_batch_s2l     RandomGenerator_s2l: the gather of wsl_augment_batch for image, mask, scribble and the [h,w,C] weight map
// All three are HBM-bound scans.  The weight map is channels-last, so with C == 4 a pixel's weights are ONE 16-byte access; the
// 4-class head also walks the logits four pixels per lane (float4 per class plane, one 32-bit word of labels).
// Reductions: per-workgroup partials, then a single-workgroup finalize that merges them in a fixed order in fp64 (no float atomics).
#include <math.h>
#include <stdint.h>

#include "wsl_rt.h"
#include "wsl_zoom.h"

namespace wsl {

constexpr int kS2lMaxC = 8;
constexpr int kS2lMaxBlocks = 1024;
constexpr int kS2lK = 4;              // partial columns per workgroup: nll_scribble, n_scribble, nll_pseudo, n_pseudo
constexpr int kS2lHeadFloats = kS2lMaxBlocks * kS2lK + 64;   // partials + the two gradient coefficients, in front of the target bytes
// target byte the first pass leaves per pixel for the second: class | kS2lPseudo (a pseudo label), or kS2lNone (no loss here)
constexpr uint32_t kS2lPseudo = 0x10, kS2lNone = 0xff;

struct S2lP {
  const float* z;
  const uint8_t* scr;
  const float* weight;
  int ignore, C, HW;
  int64_t P;
  float thr;
};

// a lane's four running sums (named members, not an array: an array handed to the block reduction is indexed at run time there and
// lands in scratch memory)
struct S2lAcc {
  float nll_s = 0.f, n_s = 0.f, nll_u = 0.f, n_u = 0.f;
};

__device__ __forceinline__ float f4_get(const float4& a, int j) { return j == 0 ? a.x : j == 1 ? a.y : j == 2 ? a.z : a.w; }

// exp(z - max) per class, their sum and the maximum: softmax = e / sum, log-sum-exp = m + log(sum)  (same arithmetic as the loss
// heads of wsl_loss.hip).  KC = array length (compile time), C <= KC the live classes: constant indices only, so the arrays stay in
// registers for a run-time C as well.
template <int KC>
__device__ __forceinline__ void exp_col(const float (&z)[KC], int C, float (&e)[KC], float& m, float& sum) {
  m = z[0];
#pragma unroll
  for (int c = 1; c < KC; ++c)
    if (c < C) m = fmaxf(m, z[c]);
  sum = 0.f;
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    e[c] = c < C ? expf(z[c] - m) : 0.f;
    sum += e[c];
  }
}

// One pixel of the first pass: the pseudo label u (highest class whose weight exceeds thr, only where the scribble is `ignore`:
// the reference writes the classes in ascending order, train_s2l.py:141-145), the target byte, and the pixel's NLL into v.
template <int KC>
__device__ __forceinline__ uint32_t s2l_pixel(const float (&z)[KC], const float (&w)[KC], int C, int l, int ignore, float thr,
                                              S2lAcc& v, uint32_t& u_out) {
  const bool scrib = l != ignore && l < C;
  int u = -1;
  if (l == ignore) {
#pragma unroll
    for (int c = 0; c < KC; ++c)
      if (c < C && w[c] > thr) u = c;
    if (u == ignore) u = -1;     // (only when a real class is the ignore index: CE ignores a pseudo label of that class as well)
  }
  u_out = u >= 0 ? (uint32_t)u : (uint32_t)ignore;
  const int t = scrib ? l : u;
  float nll = 0.f;
  if (t >= 0) {
    float e[KC], m, sum, zt = 0.f;
    exp_col<KC>(z, C, e, m, sum);
#pragma unroll
    for (int c = 0; c < KC; ++c)
      if (c == t) zt = z[c];
    nll = (m + logf(sum)) - zt;
  }
  // (selects, not `if (scrib) v.a += ... else v.b += ...`: the compiler turns that into a select of the ADDRESS and the sums into scratch)
  const bool pseudo = t >= 0 && !scrib;
  v.nll_s += scrib ? nll : 0.f, v.n_s += scrib ? 1.f : 0.f;
  v.nll_u += pseudo ? nll : 0.f, v.n_u += pseudo ? 1.f : 0.f;
  return t < 0 ? kS2lNone : ((uint32_t)t | (scrib ? 0u : kS2lPseudo));
}

__device__ __forceinline__ void s2l_write_partials(const S2lAcc& v, float* part, float* red) {
  const float a = block_sum(v.nll_s, red), b = block_sum(v.n_s, red), c = block_sum(v.nll_u, red), d = block_sum(v.n_u, red);
  if (threadIdx.x == 0) {
    float* p = part + (int64_t)blockIdx.x * kS2lK;
    p[0] = a, p[1] = b, p[2] = c, p[3] = d;
  }
}

// CT > 0: class count fixed at compile time; CT == 0: generic (C <= 8)
template <int CT>
__global__ __launch_bounds__(256) void s2l_reduce_kernel(S2lP h, uint8_t* tgt, uint8_t* u_labels, float* part) {
  constexpr int KC = CT > 0 ? CT : kS2lMaxC;
  const int C = CT > 0 ? CT : h.C;
  __shared__ float red[4];
  S2lAcc v;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < h.P; i += (int64_t)gridDim.x * kThreads) {
    const int64_t n = i / h.HW, p = i - n * h.HW, base = n * C * h.HW + p;
    float z[KC], w[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      z[c] = c < C ? h.z[base + (int64_t)c * h.HW] : 0.f;
      w[c] = c < C ? h.weight[i * C + c] : 0.f;
    }
    uint32_t u;
    tgt[i] = (uint8_t)s2l_pixel<KC>(z, w, C, h.scr[i], h.ignore, h.thr, v, u);
    if (u_labels) u_labels[i] = (uint8_t)u;
  }
  s2l_write_partials(v, part, red);
}

// C == 4, HW % 4 == 0, 16-byte aligned tensors: four consecutive pixels per lane -- one float4 per class plane, one 32-bit word of
// scribble bytes, one float4 of weights per pixel; the target bytes (and u_labels) leave as one 32-bit word
__global__ __launch_bounds__(256) void s2l_reduce4_kernel(S2lP h, uint8_t* tgt, uint8_t* u_labels, float* part) {
  __shared__ float red[4];
  S2lAcc v;
  const int64_t G = h.P >> 2;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < G; g += (int64_t)gridDim.x * kThreads) {
    const int64_t i = g * 4, n = i / h.HW, p = i - n * h.HW, base = n * 4 * h.HW + p;
    const uint32_t l4 = *reinterpret_cast<const uint32_t*>(h.scr + i);
    float4 zc[4], wp[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) zc[c] = *reinterpret_cast<const float4*>(h.z + base + (int64_t)c * h.HW);
#pragma unroll
    for (int j = 0; j < 4; ++j) wp[j] = *reinterpret_cast<const float4*>(h.weight + (i + j) * 4);
    uint32_t t4 = 0, u4 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float z[4] = {f4_get(zc[0], j), f4_get(zc[1], j), f4_get(zc[2], j), f4_get(zc[3], j)};
      const float w[4] = {wp[j].x, wp[j].y, wp[j].z, wp[j].w};
      uint32_t u;
      const uint32_t t = s2l_pixel<4>(z, w, 4, (int)((l4 >> (8 * j)) & 0xffu), h.ignore, h.thr, v, u);
      t4 |= t << (8 * j), u4 |= (u & 0xffu) << (8 * j);
    }
    *reinterpret_cast<uint32_t*>(tgt + i) = t4;
    if (u_labels) *reinterpret_cast<uint32_t*>(u_labels + i) = u4;
  }
  s2l_write_partials(v, part, red);
}

// out = {loss, ce, ce_u, n_valid, n_u}; scal = {gradient coefficient of scribble pixels 1 / n_valid, of pseudo pixels w_u / n_u}
__global__ __launch_bounds__(256) void s2l_finalize_kernel(const float* part, int nblk, float w_u, float* out, float* scal) {
  __shared__ double red[kThreads];
  const int k = threadIdx.x & 3, g = threadIdx.x >> 2;     // 64 row groups x 4 columns; every merge below has a fixed order
  double a = 0.0;
  for (int b = g; b < nblk; b += kThreads / kS2lK) a += (double)part[(int64_t)b * kS2lK + k];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = kThreads / 2; s >= kS2lK; s >>= 1) {        // s stays a multiple of 4: a thread only ever adds its own column
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double nll_s = red[0], n_s = red[1], nll_u = red[2], n_u = red[3];
    const float ce = (float)(nll_s / n_s), ce_u = (float)(nll_u / n_u);     // 0/0 -> NaN like torch when a CE has no valid pixel
    out[0] = __fadd_rn(ce, __fmul_rn(w_u, ce_u));
    out[1] = ce;
    out[2] = ce_u;
    out[3] = (float)n_s;
    out[4] = (float)n_u;
    scal[0] = n_s > 0 ? (float)(1.0 / n_s) : 0.f;
    scal[1] = n_u > 0 ? w_u * (float)(1.0 / n_u) : 0.f;
  }
}

template <int KC>
__device__ __forceinline__ void s2l_pixel_bwd(const float (&z)[KC], int C, uint32_t t, float ks, float ku, float (&g)[KC]) {
  if (t == kS2lNone) {
#pragma unroll
    for (int c = 0; c < KC; ++c) g[c] = 0.f;
    return;
  }
  const int cls = (int)(t & 0xfu);
  const float k = (t & kS2lPseudo) ? ku : ks;
  float e[KC], m, sum;
  exp_col<KC>(z, C, e, m, sum);
  const float inv = 1.f / sum;
#pragma unroll
  for (int c = 0; c < KC; ++c) g[c] = k * (e[c] * inv - (c == cls ? 1.f : 0.f));
}

template <int CT>
__global__ __launch_bounds__(256) void s2l_bwd_kernel(const float* zp, const uint8_t* tgt, const float* scal, float gscale, float* dz,
                                                      int C_, int HW, int64_t P) {
  constexpr int KC = CT > 0 ? CT : kS2lMaxC;
  const int C = CT > 0 ? CT : C_;
  const float ks = scal[0] * gscale, ku = scal[1] * gscale;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < P; i += (int64_t)gridDim.x * kThreads) {
    const int64_t n = i / HW, p = i - n * HW, base = n * C * HW + p;
    const uint32_t t = tgt[i];
    float z[KC], g[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) z[c] = (c < C && t != kS2lNone) ? zp[base + (int64_t)c * HW] : 0.f;
    s2l_pixel_bwd<KC>(z, C, t, ks, ku, g);
#pragma unroll
    for (int c = 0; c < KC; ++c)
      if (c < C) dz[base + (int64_t)c * HW] = g[c];
  }
}

__global__ __launch_bounds__(256) void s2l_bwd4_kernel(const float* zp, const uint8_t* tgt, const float* scal, float gscale, float* dz,
                                                       int HW, int64_t P) {
  const float ks = scal[0] * gscale, ku = scal[1] * gscale;
  const int64_t G = P >> 2;
  for (int64_t gi = (int64_t)blockIdx.x * kThreads + threadIdx.x; gi < G; gi += (int64_t)gridDim.x * kThreads) {
    const int64_t i = gi * 4, n = i / HW, p = i - n * HW, base = n * 4 * HW + p;
    const uint32_t t4 = *reinterpret_cast<const uint32_t*>(tgt + i);
    float o[4][4];   // [class][pixel]
    if (t4 == 0xffffffffu) {     // no loss at any of the four pixels (most of a scribble batch before the store fills): no logit read
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[c][j] = 0.f;
    } else {
      float4 zc[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) zc[c] = *reinterpret_cast<const float4*>(zp + base + (int64_t)c * HW);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float z[4] = {f4_get(zc[0], j), f4_get(zc[1], j), f4_get(zc[2], j), f4_get(zc[3], j)};
        float g[4];
        s2l_pixel_bwd<4>(z, 4, (t4 >> (8 * j)) & 0xffu, ks, ku, g);
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c][j] = g[c];
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      *reinterpret_cast<float4*>(dz + base + (int64_t)c * HW) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
  }
}

// ------------------------------------------------------------------------------------------------ ensemble update
constexpr int kSlotMax = 64;   // slices per launch: the slot table travels as a kernel argument (64 * 16 + 8 B)
struct SlotTable {
  int n;
  WslS2lSlot s[kSlotMax];
};

// VEC: C == 4 and every store 16-byte aligned -- a pixel's four averages are one float4 load and one float4 store
template <int CT, bool VEC>
__global__ __launch_bounds__(256) void s2l_ensemble_kernel(SlotTable t, const float* z, int C_, int Hn, int Wn, float a, float oma) {
  constexpr int KC = CT > 0 ? CT : kS2lMaxC;
  const int C = CT > 0 ? CT : C_;
  const WslS2lSlot& s = t.s[blockIdx.y];
  const int h = s.h, w = s.w;
  const int64_t plane = (int64_t)Hn * Wn;
  const float* zi = z + (int64_t)blockIdx.y * C * plane;
  const double sy = zoom0_scale(Hn, h), sx = zoom0_scale(Wn, w);     // zoom(pred, (1, h / Hn, w / Wn), order=0): network size -> native
  for (int o = blockIdx.x * kThreads + threadIdx.x; o < h * w; o += gridDim.x * kThreads) {
    const int y = o / w, x = o - y * w;
    const int64_t src = (int64_t)zoom0_index(y, sy, Hn) * Wn + zoom0_index(x, sx, Wn);
    const bool outside = zoom0_outside(y, sy, Hn) || zoom0_outside(x, sx, Wn);     // scipy's fill: pred = 0 in every class there
    float zz[KC], e[KC], m, sum;
#pragma unroll
    for (int c = 0; c < KC; ++c) zz[c] = c < C ? zi[(int64_t)c * plane + src] : 0.f;
    exp_col<KC>(zz, C, e, m, sum);
    const float inv = outside ? 0.f : 1.f / sum;
    float* wp = s.weight + (int64_t)o * C;
    if constexpr (VEC) {
      const float4 old = *reinterpret_cast<const float4*>(wp);
      *reinterpret_cast<float4*>(wp) = make_float4(__fadd_rn(__fmul_rn(a, e[0] * inv), __fmul_rn(oma, old.x)),
                                                   __fadd_rn(__fmul_rn(a, e[1] * inv), __fmul_rn(oma, old.y)),
                                                   __fadd_rn(__fmul_rn(a, e[2] * inv), __fmul_rn(oma, old.z)),
                                                   __fadd_rn(__fmul_rn(a, e[3] * inv), __fmul_rn(oma, old.w)));
    } else {
#pragma unroll
      for (int c = 0; c < KC; ++c)
        if (c < C) wp[c] = __fadd_rn(__fmul_rn(a, e[c] * inv), __fmul_rn(oma, wp[c]));
    }
  }
}

// ------------------------------------------------------------------------------------------------ augmentation
constexpr int kAugS2lMax = 32;   // samples per launch (32 * 104 + 8 B of kernel arguments)
struct AugS2lTable {
  int n;
  WslAugSampleS2l s[kAugS2lMax];
};

// the index map of augment_kernel (wsl_data.hip) applied to four arrays; every fill is 0 (ndimage.rotate without cval)
template <bool VEC>
__global__ __launch_bounds__(256) void augment_s2l_kernel(AugS2lTable t, int C, float* out_img, uint8_t* out_mask, uint8_t* out_scr,
                                                          float* out_weight, int Ho, int Wo) {
  const WslAugSampleS2l& s = t.s[blockIdx.y];
  const int h = s.h, w = s.w;
  const bool swap = s.op == 1 && (s.k & 1);     // shape after step 1 (rot90 by an odd k swaps the axes)
  const int R = swap ? w : h, Cc = swap ? h : w;
  const double sy = zoom0_scale(R, Ho), sx = zoom0_scale(Cc, Wo);
  const int64_t ob = (int64_t)blockIdx.y * Ho * Wo;
  for (int o = blockIdx.x * kThreads + threadIdx.x; o < Ho * Wo; o += gridDim.x * kThreads) {
    const int oy = o / Wo, ox = o - oy * Wo;
    int i = zoom0_index(oy, sy, R), j = zoom0_index(ox, sx, Cc);
    int y = i, x = j;
    bool inside = !(zoom0_outside(oy, sy, R) || zoom0_outside(ox, sx, Cc));     // zoom's own fill (0 as well)
    if (s.op == 1) {
      if (s.axis == 0) i = R - 1 - i; else j = Cc - 1 - j;          // undo np.flip
      switch (s.k & 3) {                                            // undo np.rot90(m, k): r[i][j] = m[y][x]
        case 0: y = i, x = j; break;
        case 1: y = j, x = w - 1 - i; break;
        case 2: y = h - 1 - i, x = w - 1 - j; break;
        default: y = h - 1 - j, x = i; break;
      }
    } else if (s.op == 2) {
      const double cy = dadd(dadd(dmul(s.m00, (double)i), dmul(s.m01, (double)j)), s.off0);
      const double cx = dadd(dadd(dmul(s.m10, (double)i), dmul(s.m11, (double)j)), s.off1);
      inside = inside && cy >= 0.0 && cy <= (double)(h - 1) && cx >= 0.0 && cx <= (double)(w - 1);
      y = (int)floor(dadd(cy, 0.5)), x = (int)floor(dadd(cx, 0.5));
    }
    const int64_t src = inside ? (int64_t)y * w + x : 0;
    out_img[ob + o] = inside ? s.img[src] : 0.f;
    if (out_scr) out_scr[ob + o] = inside ? s.scr[src] : (uint8_t)0;
    if (out_mask) out_mask[ob + o] = (inside && s.mask) ? s.mask[src] : (uint8_t)0;
    if (!out_weight) continue;
    float* ow = out_weight + (ob + o) * C;
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(ow) = inside ? *reinterpret_cast<const float4*>(s.weight + src * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int c = 0; c < C; ++c) ow[c] = inside ? s.weight[src * C + c] : 0.f;
    }
  }
}

static int s2l_grid(int64_t n) {
  const int64_t b = (n + kThreads - 1) / kThreads;
  return (int)(b < 1 ? 1 : (b > kS2lMaxBlocks ? kS2lMaxBlocks : b));
}
static bool aligned(const void* p, size_t a) { return ((size_t)p & (a - 1)) == 0; }

}  // namespace wsl

using namespace wsl;

extern "C" size_t wsl_s2l_head_ws_bytes(int N, int C, int HW) {
  if (N <= 0 || C <= 0 || HW <= 0) return 0;
  // [partials: kS2lMaxBlocks * 4][coefficients: 64][target bytes: N * HW, rounded up to whole floats]
  return sizeof(float) * ((size_t)kS2lHeadFloats + ((size_t)N * HW + 3) / 4);
}

extern "C" int wsl_s2l_head_fwd_bwd(const float* z, const uint8_t* scribble, const float* weight, int ignore, float thr_conf, float w_u,
                                    float gscale, float* out, uint8_t* u_labels, float* dz, int N, int C, int HW, void* ws,
                                    size_t ws_bytes, void* stream) {
  WSL_REQUIRE(z && scribble && weight && out && N > 0 && HW > 0 && C > 0 && C <= kS2lMaxC, "s2l_head_fwd_bwd: bad args (C <= %d)", kS2lMaxC);
  WSL_REQUIRE(ignore >= 0 && ignore < 255, "s2l_head_fwd_bwd: ignore %d does not fit a label byte", ignore);
  if (!ws || ws_bytes < wsl_s2l_head_ws_bytes(N, C, HW)) {
    set_error("s2l_head_fwd_bwd: workspace %zu < %zu", ws_bytes, wsl_s2l_head_ws_bytes(N, C, HW));
    return WSL_EWORKSPACE;
  }
  const int64_t P = (int64_t)N * HW;
  S2lP h{z, scribble, weight, ignore, C, HW, P, thr_conf};
  float* part = static_cast<float*>(ws);
  float* scal = part + (size_t)kS2lMaxBlocks * kS2lK;
  uint8_t* tgt = reinterpret_cast<uint8_t*>(part + kS2lHeadFloats);
  // forward: logits + 1 B scribble + C weights in, 1 B target out (+ 1 B u_labels); backward: 1 B target + logits in, gradients out
  ProfScope ps(PF_LOSS_HEAD, 0.0, (double)P * (8.0 * C + 2.0 + (u_labels ? 1.0 : 0.0) + (dz ? 8.0 * C + 1.0 : 0.0)), stream);
  const bool v4 = C == 4 && HW % 4 == 0 && aligned(z, 16) && aligned(weight, 16) && aligned(scribble, 4) && aligned(u_labels, 4) &&
                  aligned(dz, 16) && aligned(ws, 16);
  if (v4) {
    const int nb = s2l_grid(P >> 2);
    WSL_LAUNCH(s2l_reduce4_kernel, dim3(nb), dim3(kThreads), 0, stream, h, tgt, u_labels, part);
    WSL_LAUNCH(s2l_finalize_kernel, dim3(1), dim3(kThreads), 0, stream, part, nb, w_u, out, scal);
    if (dz) WSL_LAUNCH(s2l_bwd4_kernel, dim3(nb), dim3(kThreads), 0, stream, z, tgt, scal, gscale, dz, HW, P);
  } else {
    const int nb = s2l_grid(P);
    if (C == 4) WSL_LAUNCH((s2l_reduce_kernel<4>), dim3(nb), dim3(kThreads), 0, stream, h, tgt, u_labels, part);
    else WSL_LAUNCH((s2l_reduce_kernel<0>), dim3(nb), dim3(kThreads), 0, stream, h, tgt, u_labels, part);
    WSL_LAUNCH(s2l_finalize_kernel, dim3(1), dim3(kThreads), 0, stream, part, nb, w_u, out, scal);
    if (dz) {
      if (C == 4) WSL_LAUNCH((s2l_bwd_kernel<4>), dim3(nb), dim3(kThreads), 0, stream, z, tgt, scal, gscale, dz, C, HW, P);
      else WSL_LAUNCH((s2l_bwd_kernel<0>), dim3(nb), dim3(kThreads), 0, stream, z, tgt, scal, gscale, dz, C, HW, P);
    }
  }
  return check_launch("s2l_head_fwd_bwd");
}

extern "C" int wsl_s2l_ensemble_update(const float* z, const WslS2lSlot* slots, int n, int C, int Hn, int Wn, double alpha, void* stream) {
  WSL_REQUIRE(z && slots && n > 0 && C > 0 && C <= kS2lMaxC && Hn > 0 && Wn > 0, "s2l_ensemble_update: bad args (C <= %d)", kS2lMaxC);
  const float a = (float)alpha, oma = (float)(1.0 - alpha);      // the python doubles alpha and 1 - alpha, each rounded to fp32
  for (int base = 0; base < n; base += kSlotMax) {
    SlotTable t;
    t.n = n - base < kSlotMax ? n - base : kSlotMax;
    bool vec = C == 4;
    int64_t px = 1;
    for (int k = 0; k < t.n; ++k) {
      const WslS2lSlot& s = slots[base + k];
      WSL_REQUIRE(s.weight && s.h > 0 && s.w > 0 && (int64_t)s.h * s.w < (int64_t)1 << 30, "s2l_ensemble_update: slot %d is malformed", base + k);
      t.s[k] = s;
      vec = vec && aligned(s.weight, 16);
      px = (int64_t)s.h * s.w > px ? (int64_t)s.h * s.w : px;
    }
    const dim3 grid(cdiv((int)px, kThreads * 2), t.n);
    const float* zb = z + (int64_t)base * C * Hn * Wn;
    if (vec) WSL_LAUNCH((s2l_ensemble_kernel<4, true>), grid, dim3(kThreads), 0, stream, t, zb, C, Hn, Wn, a, oma);
    else WSL_LAUNCH((s2l_ensemble_kernel<0, false>), grid, dim3(kThreads), 0, stream, t, zb, C, Hn, Wn, a, oma);
  }
  return check_launch("s2l_ensemble_kernel");
}

extern "C" int wsl_augment_batch_s2l(const WslAugSampleS2l* samples, int n, int C, float* out_img, uint8_t* out_mask, uint8_t* out_scr,
                                     float* out_weight, int Ho, int Wo, void* stream) {
  WSL_REQUIRE(samples && out_img && n > 0 && C > 0 && C <= kS2lMaxC && Ho > 0 && Wo > 0, "augment_batch_s2l: bad arguments (C <= %d)",
              kS2lMaxC);
  const int64_t opx = (int64_t)Ho * Wo;
  for (int base = 0; base < n; base += kAugS2lMax) {
    AugS2lTable t;
    t.n = n - base < kAugS2lMax ? n - base : kAugS2lMax;
    bool vec = C == 4 && out_weight && aligned(out_weight, 16);
    for (int k = 0; k < t.n; ++k) {
      const WslAugSampleS2l& s = samples[base + k];
      WSL_REQUIRE(s.img && (s.scr || !out_scr) && (s.weight || !out_weight) && s.h > 0 && s.w > 0 && s.op >= 0 && s.op <= 2,
                  "augment_batch_s2l: sample %d is malformed", base + k);
      t.s[k] = s;
      vec = vec && aligned(s.weight, 16);
    }
    const dim3 grid(cdiv(Ho * Wo, kThreads * 4), t.n);
    uint8_t* om = out_mask ? out_mask + base * opx : nullptr;
    uint8_t* os = out_scr ? out_scr + base * opx : nullptr;
    float* ow = out_weight ? out_weight + base * opx * C : nullptr;
    if (vec) WSL_LAUNCH((augment_s2l_kernel<true>), grid, dim3(kThreads), 0, stream, t, C, out_img + base * opx, om, os, ow, Ho, Wo);
    else WSL_LAUNCH((augment_s2l_kernel<false>), grid, dim3(kThreads), 0, stream, t, C, out_img + base * opx, om, os, ow, Ho, Wo);
  }
  return check_launch("augment_s2l_kernel");
}
