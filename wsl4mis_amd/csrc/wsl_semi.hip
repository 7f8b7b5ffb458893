// Semi-supervised trainers (ref: code/train_mean_teacher_2D.py, code/train_uncertainty_aware_mean_teacher_2D.py,
// code/train_entropy_minimization_2D.py) -- the two loss heads their step adds, both straight from logits:
//   wsl_sup_head_fwd_bwd         w_ce * CE(z, label; ignore) + w_dice * DiceLoss(C)(softmax(z), label)   (the labeled half:
//                                train_mean_teacher_2D.py:161-163, utils/losses.py:156-192), value and logit gradient
//   wsl_entropy_logits_fwd_bwd   entropy_loss(softmax(z), norm_classes)   (the unlabeled half of the entropy-minimisation trainer:
//                                train_entropy_minimization_2D.py:140-142, utils/losses.py:30-36), value and logit gradient in one pass
// Both are HBM-bound scans over [N,C,HW] logits.  A workgroup walks contiguous chunks of kSemiChunk pixels of the flattened [N*HW]
// pixel axis; with HW % 4 == 0 and 16-byte aligned tensors a lane takes four consecutive pixels (one float4 per class plane, one
// 32-bit word of labels), otherwise one pixel at a time.  The class count is a template argument (1 .. 8): every per-class array is
// indexed with constants only and lives in registers -- no private segment.
// Reductions: per-workgroup partials, then a single-workgroup merge in a fixed order in fp64 (no float atomics): bit-reproducible.
#include <math.h>
#include <stdint.h>

#include "wsl_rt.h"

namespace wsl {

constexpr int kSemiMaxC = 8;
constexpr int kSemiMaxBlocks = 1024;
constexpr int kSemiChunk = 2048;                 // pixels per workgroup and grid step: 8 per lane
constexpr int kSemiK = 2 + 3 * kSemiMaxC;        // partial columns of the supervised head: nll, n_valid, I[c], Z[c], Y[c] (row stride)
// the coefficients of the second pass live behind the partials region every loss entry point shares (wsl_loss.hip: kMaxBlocks * kMaxK
// floats of partials, then 64 floats): wsl_loss_ws_bytes() >= (1024 * 48 + 64) floats for every shape
constexpr size_t kSemiScalOff = (size_t)1024 * 48;
static_assert((size_t)kSemiMaxBlocks * kSemiK <= kSemiScalOff, "the partials stay in front of the coefficients");
static_assert(1 + 2 * kSemiMaxC <= 64, "the coefficients fit the 64 floats");

__device__ __forceinline__ float semi_f4(const float4& a, int j) { return j == 0 ? a.x : j == 1 ? a.y : j == 2 ? a.z : a.w; }

// softmax of C logits held in registers; returns the log-sum-exp (max-subtracted: finite for any finite logits)
template <int C>
__device__ __forceinline__ float semi_softmax(const float (&z)[C], float (&s)[C]) {
  float m = z[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    s[c] = expf(z[c] - m);
    sum += s[c];
  }
  const float inv = 1.f / sum;
#pragma unroll
  for (int c = 0; c < C; ++c) s[c] *= inv;
  return m + logf(sum);
}

// the same softmax, returning the maximum and log(sum) apart: log p_c = (z_c - m) - lsum keeps its precision for large |z|
template <int C>
__device__ __forceinline__ void semi_softmax_parts(const float (&z)[C], float (&s)[C], float& m, float& lsum) {
  m = z[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    s[c] = expf(z[c] - m);
    sum += s[c];
  }
  const float inv = 1.f / sum;
#pragma unroll
  for (int c = 0; c < C; ++c) s[c] *= inv;
  lsum = logf(sum);
}

// ------------------------------------------------------------------------------------------------ supervised head, first pass
// v: 0 nll sum, 1 valid count, 2 + c I_c = sum s_c [l == c], 2 + C + c Z_c = sum s_c^2, 2 + 2C + c Y_c = sum [l == c].
// DiceLoss one-hot encodes over range(C): a label outside 0 .. C-1 (the ignore value) is zero in every class and still adds to Z.
template <int C>
__device__ __forceinline__ void sup_pixel(const float (&z)[C], int l, int ignore, float (&v)[2 + 3 * C]) {
  float s[C], m, lsum;
  semi_softmax_parts<C>(z, s, m, lsum);
  const bool valid = l != ignore && l < C;
  float zl = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const bool hit = l == c;
    zl = hit ? z[c] : zl;
    v[2 + c] += hit ? s[c] : 0.f;
    v[2 + C + c] = fmaf(s[c], s[c], v[2 + C + c]);
    v[2 + 2 * C + c] += hit ? 1.f : 0.f;
  }
  v[0] += valid ? (m - zl) + lsum : 0.f;      // -log softmax(z)[l], the maximum taken out before the small term is added
  v[1] += valid ? 1.f : 0.f;
}

template <int C, bool VEC>
__global__ __launch_bounds__(256) void sup_reduce_kernel(const float* zp, const uint8_t* label, int ignore, int HW, int64_t P,
                                                         float* part) {
  __shared__ float red[4];
  float v[2 + 3 * C];
#pragma unroll
  for (int k = 0; k < 2 + 3 * C; ++k) v[k] = 0.f;
  const int64_t nchunk = (P + kSemiChunk - 1) / kSemiChunk;
  for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    if (VEC) {
      for (int g = threadIdx.x; g < kSemiChunk / 4; g += kThreads) {
        const int64_t i = ch * kSemiChunk + 4 * (int64_t)g;
        if (i >= P) break;
        const int64_t n = i / HW, p = i - n * HW, base = n * C * HW + p;
        const uint32_t l4 = *reinterpret_cast<const uint32_t*>(label + i);
        float4 zc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) zc[c] = *reinterpret_cast<const float4*>(zp + base + (int64_t)c * HW);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float z[C];
#pragma unroll
          for (int c = 0; c < C; ++c) z[c] = semi_f4(zc[c], j);
          sup_pixel<C>(z, (int)((l4 >> (8 * j)) & 0xffu), ignore, v);
        }
      }
    } else {
      for (int g = threadIdx.x; g < kSemiChunk; g += kThreads) {
        const int64_t i = ch * kSemiChunk + g;
        if (i >= P) break;
        const int64_t n = i / HW, p = i - n * HW, base = n * C * HW + p;
        float z[C];
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = zp[base + (int64_t)c * HW];
        sup_pixel<C>(z, (int)label[i], ignore, v);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 2 + 3 * C; ++k) {
    const float s = block_sum(v[k], red);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.x * kSemiK + k] = s;
  }
}

// Column sums of part[nblk][kSemiK] in one sweep: thread (row group g of 8, column k of 32) adds every eighth row in fp64, four rows
// in flight; the eight groups are merged in a fixed order.  Then the scalar arithmetic of the two losses (DiceLoss in fp32 as
// pdice_finalize_kernel does it) and the coefficients of the second pass:
//   scal[0] = w_ce / n_valid (0 without a valid pixel: CE is NaN then, like torch, and its gradient 0 -- wsl_head_fwd_bwd's convention)
//   scal[1 + c] = -2 / D_c * w_dice / C            (d dice / d s through I_c, on pixels with l == c)
//   scal[1 + C + c] = 2 (2 I_c + eps) / D_c^2 * w_dice / C     (through Z_c, times s_c)          D_c = Z_c + Y_c + eps, eps = 1e-5
__global__ __launch_bounds__(256) void sup_finalize_kernel(const float* part, int nblk, int C, float w_ce, float w_dice, float* out,
                                                           float* scal) {
  __shared__ double red8[8][32];
  __shared__ double tot[32];
  const int g = threadIdx.x >> 5, k = threadIdx.x & 31;
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  if (k < 2 + 3 * C) {
    int b = g;
    for (; b + 24 < nblk; b += 32) {
      const float v0 = part[(int64_t)b * kSemiK + k], v1 = part[(int64_t)(b + 8) * kSemiK + k], v2 = part[(int64_t)(b + 16) * kSemiK + k],
                  v3 = part[(int64_t)(b + 24) * kSemiK + k];
      a0 += (double)v0, a1 += (double)v1, a2 += (double)v2, a3 += (double)v3;
    }
    for (; b < nblk; b += 8) a0 += (double)part[(int64_t)b * kSemiK + k];
  }
  red8[g][k] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (threadIdx.x < 32)
    tot[k] = ((red8[0][k] + red8[1][k]) + (red8[2][k] + red8[3][k])) + ((red8[4][k] + red8[5][k]) + (red8[6][k] + red8[7][k]));
  __syncthreads();
  if (threadIdx.x == 0) {
    const double nll = tot[0], cnt = tot[1];
    const float ce = (float)(nll / cnt);      // 0 / 0 -> NaN like torch when every pixel is ignored
    double acc = 0;
    const float kd = w_dice / (float)C;
    for (int c = 0; c < C; ++c) {
      const float I = (float)tot[2 + c], Z = (float)tot[2 + C + c], Y = (float)tot[2 + 2 * C + c];
      const float D = Z + Y + 1e-5f;
      acc += 1.0 - (double)((2.f * I + 1e-5f) / D);
      scal[1 + c] = -2.f / D * kd;
      scal[1 + C + c] = 2.f * (2.f * I + 1e-5f) / (D * D) * kd;
    }
    const float dice = (float)(acc / C);
    out[0] = w_ce * ce + w_dice * dice;
    out[1] = ce;
    out[2] = dice;
    out[3] = (float)cnt;
    scal[0] = cnt > 0 ? w_ce * (float)(1.0 / cnt) : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ supervised head, second pass
template <int C>
__device__ __forceinline__ void sup_pixel_bwd(const float (&z)[C], int l, int ignore, float kce, const float (&ca)[C],
                                              const float (&cb)[C], float gscale, float (&g)[C]) {
  float s[C], ds[C], dot = 0.f;
  semi_softmax<C>(z, s);
  const bool valid = l != ignore && l < C;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    ds[c] = (l == c ? ca[c] : 0.f) + cb[c] * s[c];
    dot = fmaf(ds[c], s[c], dot);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float d = s[c] * (ds[c] - dot);
    if (valid) d += kce * (s[c] - (l == c ? 1.f : 0.f));
    g[c] = d * gscale;
  }
}

template <int C, bool VEC>
__global__ __launch_bounds__(256) void sup_bwd_kernel(const float* zp, const uint8_t* label, int ignore, int HW, int64_t P,
                                                      const float* scal, float gscale, float* dz) {
  const float kce = scal[0];
  float ca[C], cb[C];
#pragma unroll
  for (int c = 0; c < C; ++c) ca[c] = scal[1 + c], cb[c] = scal[1 + C + c];
  const int64_t nchunk = (P + kSemiChunk - 1) / kSemiChunk;
  for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    if (VEC) {
      for (int gi = threadIdx.x; gi < kSemiChunk / 4; gi += kThreads) {
        const int64_t i = ch * kSemiChunk + 4 * (int64_t)gi;
        if (i >= P) break;
        const int64_t n = i / HW, p = i - n * HW, base = n * C * HW + p;
        const uint32_t l4 = *reinterpret_cast<const uint32_t*>(label + i);
        float4 zc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) zc[c] = *reinterpret_cast<const float4*>(zp + base + (int64_t)c * HW);
        float o[C][4];   // [class][pixel]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float z[C], g[C];
#pragma unroll
          for (int c = 0; c < C; ++c) z[c] = semi_f4(zc[c], j);
          sup_pixel_bwd<C>(z, (int)((l4 >> (8 * j)) & 0xffu), ignore, kce, ca, cb, gscale, g);
#pragma unroll
          for (int c = 0; c < C; ++c) o[c][j] = g[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c)
          *reinterpret_cast<float4*>(dz + base + (int64_t)c * HW) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
      }
    } else {
      for (int gi = threadIdx.x; gi < kSemiChunk; gi += kThreads) {
        const int64_t i = ch * kSemiChunk + gi;
        if (i >= P) break;
        const int64_t n = i / HW, p = i - n * HW, base = n * C * HW + p;
        float z[C], g[C];
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = zp[base + (int64_t)c * HW];
        sup_pixel_bwd<C>(z, (int)label[i], ignore, kce, ca, cb, gscale, g);
#pragma unroll
        for (int c = 0; c < C; ++c) dz[base + (int64_t)c * HW] = g[c];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ entropy head
// Per pixel, p = softmax(z):  e = -sum_c p_c log(p_c + 1e-6);  d e / d p_c = -(log(p_c + 1e-6) + p_c / (p_c + 1e-6));
// dz_c = k * p_c * (de_c - sum_j de_j p_j),  k = gscale / (N * HW * log(norm_classes)) -- known before the launch, so the gradient
// leaves in the same pass that sums e.  Returns e of the pixel.
// log(p_c + 1e-6): the sum p_c + 1e-6 rounds to a multiple of 6e-8 near p_c = 1, which is 5 % of the whole term of a confident pixel
// (-log(1 + 1e-6) = -1e-6), so from p_c >= 0.5 on the same quantity is taken as log p_c + log1p(1e-6 / p_c) with log p_c from the
// logits ((z_c - max) - log sum); below 0.5 the plain form is exact to an ulp of the logarithm.
template <int C>
__device__ __forceinline__ float ent_pixel(const float (&z)[C], float k, float (&g)[C]) {
  float s[C], de[C], e = 0.f, dot = 0.f;
  float m, lsum;
  semi_softmax_parts<C>(z, s, m, lsum);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float xe = s[c] + 1e-6f;
    const float lg = s[c] >= 0.5f ? ((z[c] - m) - lsum) + log1pf(1e-6f / s[c]) : logf(xe);
    e = fmaf(-s[c], lg, e);
    de[c] = -(lg + s[c] / xe);
    dot = fmaf(de[c], s[c], dot);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) g[c] = k * s[c] * (de[c] - dot);
  return e;
}

template <int C, bool VEC>
__global__ __launch_bounds__(256) void ent_logits_kernel(const float* zp, int HW, int64_t P, float k, float* dz, float* part) {
  __shared__ float red[4];
  float v = 0.f;
  const int64_t nchunk = (P + kSemiChunk - 1) / kSemiChunk;
  for (int64_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    if (VEC) {
      for (int gi = threadIdx.x; gi < kSemiChunk / 4; gi += kThreads) {
        const int64_t i = ch * kSemiChunk + 4 * (int64_t)gi;
        if (i >= P) break;
        const int64_t n = i / HW, p = i - n * HW, base = n * C * HW + p;
        float4 zc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) zc[c] = *reinterpret_cast<const float4*>(zp + base + (int64_t)c * HW);
        float o[C][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float z[C], g[C];
#pragma unroll
          for (int c = 0; c < C; ++c) z[c] = semi_f4(zc[c], j);
          v += ent_pixel<C>(z, k, g);
#pragma unroll
          for (int c = 0; c < C; ++c) o[c][j] = g[c];
        }
        if (dz) {
#pragma unroll
          for (int c = 0; c < C; ++c)
            *reinterpret_cast<float4*>(dz + base + (int64_t)c * HW) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
        }
      }
    } else {
      for (int gi = threadIdx.x; gi < kSemiChunk; gi += kThreads) {
        const int64_t i = ch * kSemiChunk + gi;
        if (i >= P) break;
        const int64_t n = i / HW, p = i - n * HW, base = n * C * HW + p;
        float z[C], g[C];
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = zp[base + (int64_t)c * HW];
        v += ent_pixel<C>(z, k, g);
        if (dz) {
#pragma unroll
          for (int c = 0; c < C; ++c) dz[base + (int64_t)c * HW] = g[c];
        }
      }
    }
  }
  const float s = block_sum(v, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// loss = norm * sum of the workgroup partials: fp64, every thread its rows in order, then a fixed-order tree
__global__ __launch_bounds__(256) void ent_finalize_kernel(const float* part, int nblk, double norm, float* loss) {
  __shared__ double red[kThreads];
  double a = 0;
  for (int b = threadIdx.x; b < nblk; b += kThreads) a += (double)part[b];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(red[0] * norm);
}

static int semi_grid(int64_t P) {
  const int64_t b = (P + kSemiChunk - 1) / kSemiChunk;
  return (int)(b < 1 ? 1 : (b > kSemiMaxBlocks ? kSemiMaxBlocks : b));
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

template <int C>
static void sup_launch(const float* z, const uint8_t* label, int ignore, float w_ce, float w_dice, float gscale, float* out, float* dz,
                       int HW, int64_t P, float* part, float* scal, void* stream) {
  const int nb = semi_grid(P);
  const bool vec = HW % 4 == 0 && aligned16(z) && aligned4(label) && (!dz || aligned16(dz));
  if (vec) WSL_LAUNCH((sup_reduce_kernel<C, true>), dim3(nb), dim3(kThreads), 0, stream, z, label, ignore, HW, P, part);
  else WSL_LAUNCH((sup_reduce_kernel<C, false>), dim3(nb), dim3(kThreads), 0, stream, z, label, ignore, HW, P, part);
  WSL_LAUNCH(sup_finalize_kernel, dim3(1), dim3(kThreads), 0, stream, part, nb, C, w_ce, w_dice, out, scal);
  if (!dz) return;
  if (vec) WSL_LAUNCH((sup_bwd_kernel<C, true>), dim3(nb), dim3(kThreads), 0, stream, z, label, ignore, HW, P, scal, gscale, dz);
  else WSL_LAUNCH((sup_bwd_kernel<C, false>), dim3(nb), dim3(kThreads), 0, stream, z, label, ignore, HW, P, scal, gscale, dz);
}

template <int C>
static void ent_launch(const float* z, float* loss, float* dz, float k, double norm, int HW, int64_t P, float* part, void* stream) {
  const int nb = semi_grid(P);
  const bool vec = HW % 4 == 0 && aligned16(z) && (!dz || aligned16(dz));
  if (vec) WSL_LAUNCH((ent_logits_kernel<C, true>), dim3(nb), dim3(kThreads), 0, stream, z, HW, P, k, dz, part);
  else WSL_LAUNCH((ent_logits_kernel<C, false>), dim3(nb), dim3(kThreads), 0, stream, z, HW, P, k, dz, part);
  WSL_LAUNCH(ent_finalize_kernel, dim3(1), dim3(kThreads), 0, stream, part, nb, norm, loss);
}

}  // namespace wsl

using namespace wsl;

#define WSL_SEMI_BY_C(C, CALL)  \
  switch (C) {                  \
    case 1: CALL(1); break;     \
    case 2: CALL(2); break;     \
    case 3: CALL(3); break;     \
    case 4: CALL(4); break;     \
    case 5: CALL(5); break;     \
    case 6: CALL(6); break;     \
    case 7: CALL(7); break;     \
    default: CALL(8); break;    \
  }

extern "C" int wsl_sup_head_fwd_bwd(const float* z, const uint8_t* label, int ignore, float w_ce, float w_dice, float gscale,
                                    float* out, float* dz, int N, int C, int HW, void* ws, size_t ws_bytes, void* stream) {
  WSL_REQUIRE(z && label && out && N > 0 && HW > 0 && C > 0 && C <= kSemiMaxC, "sup_head_fwd_bwd: bad args (1 <= C <= %d)", kSemiMaxC);
  const size_t need = wsl_loss_ws_bytes(N, C, HW);
  if (!ws || ws_bytes < need) {
    set_error("sup_head_fwd_bwd: workspace %zu < %zu", ws_bytes, need);
    return WSL_EWORKSPACE;
  }
  const int64_t P = (int64_t)N * HW;
  // the reduction pass reads logits + 1 B label; the gradient pass reads them again and writes the logit gradient
  ProfScope ps(PF_LOSS_HEAD, 0.0, (double)P * ((dz ? 2.0 : 1.0) * (4.0 * C + 1.0) + (dz ? 4.0 * C : 0.0)), stream);
  float* part = static_cast<float*>(ws);
  float* scal = part + kSemiScalOff;
#define WSL_SEMI_SUP(K) sup_launch<K>(z, label, ignore, w_ce, w_dice, gscale, out, dz, HW, P, part, scal, stream)
  WSL_SEMI_BY_C(C, WSL_SEMI_SUP)
#undef WSL_SEMI_SUP
  return check_launch("sup_head_fwd_bwd");
}

extern "C" int wsl_entropy_logits_fwd_bwd(const float* z, float* loss, float* dz, float gscale, int N, int C, int HW, int norm_classes,
                                          void* ws, size_t ws_bytes, void* stream) {
  WSL_REQUIRE(z && loss && N > 0 && HW > 0 && C > 0 && C <= kSemiMaxC && norm_classes > 1,
              "entropy_logits_fwd_bwd: bad args (1 <= C <= %d, norm_classes >= 2)", kSemiMaxC);
  const size_t need = wsl_loss_ws_bytes(N, C, HW);
  if (!ws || ws_bytes < need) {
    set_error("entropy_logits_fwd_bwd: workspace %zu < %zu", ws_bytes, need);
    return WSL_EWORKSPACE;
  }
  const int64_t P = (int64_t)N * HW;
  const double norm = 1.0 / ((double)P * log((double)norm_classes));   // losses.py:32-33: the class count is only the log(C) normaliser
  ProfScope ps(PF_LOSS_HEAD, 0.0, (double)P * 4.0 * C * (dz ? 2.0 : 1.0), stream);
  float* part = static_cast<float*>(ws);
#define WSL_SEMI_ENT(K) ent_launch<K>(z, loss, dz, (float)(gscale * norm), norm, HW, P, part, stream)
  WSL_SEMI_BY_C(C, WSL_SEMI_ENT)
#undef WSL_SEMI_ENT
  return check_launch("entropy_logits_fwd_bwd");
}
