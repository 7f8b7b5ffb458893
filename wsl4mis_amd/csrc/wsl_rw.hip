// Random-walker pseudo labels (ref: code/dataloaders/acdc_pseudo_label_random_walker.py:9-26, dataloaders/dataset_scribblevc.py:20-36;
// skimage.segmentation.random_walker(data, markers, beta=100, mode='bf') as those call it) for a batch of N equal-sized slices:
//   rw_stats_kernel     per slice: std of the rescaled image d (two passes, fp64 sums merged in a fixed order) -> the exponent scale
//                       beta / (10 std), and which seed classes are present -> the class-rule flag
//   rw_setup_kernel     per pixel: the edge weights to the right and down, the diagonal of L_uu and its inverse (0 on seeded pixels),
//                       and per class the right-hand side b_k = sum of the weights to neighbours seeded with k
//   rw_pcg_kernel       ONE persistent workgroup per (slice, class) system: Jacobi-preconditioned conjugate gradients in fp32 on the
//                       5-point stencil.  The vectors (x, r, p, q) do not fit in LDS -- they live in the caller's workspace, each
//                       thread owns the pixels tid, tid + 256, ... of all four, and only p is read across threads (after a
//                       barrier).  Three passes and three fixed-order reductions per iteration; the loop ends at max_iter at the latest.
//   rw_finish_kernel    argmax over the classes (ties to the lowest), seeds kept, zeros for slices that fail the class rule
// Seeded pixels stay in the index space with x = r = p = 0 and 1 / diag = 0, so L_uu is the full stencil with no index compaction.
#include <math.h>
#include <stdint.h>

#include "wsl_rt.h"

namespace wsl {

constexpr int kRwMaxC = 8;
constexpr int kRwMaxPixels = 1 << 20;
constexpr int kRwMaxIter = 100000;
constexpr int kRwSlicePlanes = 4;     // wr, wd, diag, 1 / diag
constexpr int kRwSysPlanes = 4;       // x, r, p, q

// [scale: N floats][ok: N ints] rounded up to 64 words, then the planes
static size_t rw_head_words(int N) { return ((size_t)2 * N + 63) / 64 * 64; }

__device__ __forceinline__ float rw_rescale(float v) {
  const float c = fminf(fmaxf(v, -0.35f), 1.35f);
  return 2.f * (c + 0.35f) / 1.7f - 1.f;
}

// sum over the workgroup in fp64, fixed order; valid in every thread
__device__ __forceinline__ double rw_block_sum_f64(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kThreads / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(256) void rw_stats_kernel(const float* img, const uint8_t* seed, int HW, int K, float beta, float* scale,
                                                       int* ok) {
  __shared__ double red[kThreads];
  __shared__ uint32_t present[4];
  const int n = blockIdx.x;
  const float* im = img + (int64_t)n * HW;
  const uint8_t* sd = seed + (int64_t)n * HW;
  double s = 0.0;
  uint32_t mask = 0;
  for (int i = threadIdx.x; i < HW; i += kThreads) {
    s += (double)rw_rescale(im[i]);
    const uint32_t c = sd[i];
    mask |= c < (uint32_t)K ? 1u << c : 0u;
  }
  const double mean = rw_block_sum_f64(s, red) / (double)HW;
  double q = 0.0;
  for (int i = threadIdx.x; i < HW; i += kThreads) {
    const double d = (double)rw_rescale(im[i]) - mean;
    q += d * d;
  }
  const double var = rw_block_sum_f64(q, red) / (double)HW;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) mask |= (uint32_t)__shfl_xor((int)mask, m);
  if ((threadIdx.x & 63) == 0) present[threadIdx.x >> 6] = mask;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t all = present[0] | present[1] | present[2] | present[3], fg = ((1u << K) - 1u) & ~1u;
    const double sd_ = sqrt(var);
    scale[n] = sd_ > 0.0 ? (float)((double)beta / (10.0 * sd_)) : 0.f;      // std == 0: every weight is exp(0) + 1e-6 (see wsl_hip.h)
    ok[n] = (all & fg) == fg ? 1 : 0;
  }
}

struct RwP {
  const float* scale;
  const int* ok;
  float *wr, *wd, *diag, *invd;      // [N][HW]
  float* sys;                        // [N][K][4][HW]: x, r, p, q
  int H, W, HW, K;
};

__device__ __forceinline__ float rw_weight(float a, float b, float scale) {
  const float g = a - b;
  return expf(-scale * (g * g)) + 1e-6f;
}

__global__ __launch_bounds__(256) void rw_setup_kernel(RwP a, const float* img, const uint8_t* seed) {
  const int n = blockIdx.y;
  if (!a.ok[n]) return;                                   // nothing of this slice is read later
  const float sc = a.scale[n];
  const int64_t sb = (int64_t)n * a.HW;
  const float* im = img + sb;
  const uint8_t* sd = seed + sb;
  const int W = a.W, H = a.H, K = a.K;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < a.HW; i += gridDim.x * kThreads) {
    const int y = i / W, x = i - y * W;
    const float d = rw_rescale(im[i]);
    // (a - b)^2 == (b - a)^2 bit for bit: the weight of an edge is the same from either end
    const float wl = x > 0 ? rw_weight(d, rw_rescale(im[i - 1]), sc) : 0.f;
    const float wr = x + 1 < W ? rw_weight(d, rw_rescale(im[i + 1]), sc) : 0.f;
    const float wu = y > 0 ? rw_weight(d, rw_rescale(im[i - W]), sc) : 0.f;
    const float wd = y + 1 < H ? rw_weight(d, rw_rescale(im[i + W]), sc) : 0.f;
    const bool seeded = sd[i] < K;
    const float dg = (wl + wr) + (wu + wd);
    a.wr[sb + i] = wr, a.wd[sb + i] = wd;
    a.diag[sb + i] = seeded ? 0.f : dg;
    a.invd[sb + i] = seeded ? 0.f : 1.f / dg;
    const int sl = x > 0 ? sd[i - 1] : 255, sr = x + 1 < W ? sd[i + 1] : 255, su = y > 0 ? sd[i - W] : 255, sdn = y + 1 < H ? sd[i + W] : 255;
    for (int k = 0; k < K; ++k) {
      const float b = ((sl == k ? wl : 0.f) + (sr == k ? wr : 0.f)) + ((su == k ? wu : 0.f) + (sdn == k ? wd : 0.f));
      a.sys[(((int64_t)n * K + k) * kRwSysPlanes + 1) * a.HW + i] = seeded ? 0.f : b;      // r = b (x = 0)
    }
  }
}

__global__ __launch_bounds__(256) void rw_pcg_kernel(RwP a, float tol, int max_iter, int* iters, float* resid) {
  __shared__ float red[4];
  const int k = blockIdx.x, n = blockIdx.y, HW = a.HW, W = a.W, tid = threadIdx.x;
  const int sysi = n * a.K + k;
  if (!a.ok[n]) {
    if (tid == 0) iters[sysi] = 0, resid[sysi] = 0.f;
    return;
  }
  const int64_t sb = (int64_t)n * HW;
  const float *wr = a.wr + sb, *wd = a.wd + sb, *diag = a.diag + sb, *invd = a.invd + sb;
  float* xv = a.sys + (int64_t)sysi * kRwSysPlanes * HW;
  float *rv = xv + HW, *pv = rv + HW, *qv = pv + HW;

  float bb = 0.f, rz = 0.f;
  for (int i = tid; i < HW; i += kThreads) {
    const float r = rv[i], z = r * invd[i];
    xv[i] = 0.f, pv[i] = z;
    bb += r * r, rz += r * z;
  }
  bb = block_sum(bb, red), rz = block_sum(rz, red);
  if (!(bb > 0.f)) {                                       // b == 0: x = 0 after zero iterations
    if (tid == 0) iters[sysi] = 0, resid[sysi] = 0.f;
    return;
  }
  const float bnorm = sqrtf(bb), stop = tol * bnorm;
  float rr = bb;
  int it = 0;
  // every value the loop condition reads is the same in all threads (block_sum results): the barriers inside are uniform.
  // HARD BOUND: it < max_iter (max_iter <= kRwMaxIter, checked by the entry point)
  while (it < max_iter && !(sqrtf(rr) <= stop)) {
    __syncthreads();                                       // p of the previous iteration (or the start) is complete
    float pq = 0.f;
    for (int i = tid; i < HW; i += kThreads) {
      const float dg = diag[i], pc = pv[i];
      const float pl = i > 0 ? pv[i - 1] : 0.f, wl = i > 0 ? wr[i - 1] : 0.f;          // wr is 0 in the last column: no row wrap
      const float pu = i >= W ? pv[i - W] : 0.f, wu = i >= W ? wd[i - W] : 0.f;
      const float pr = i + 1 < HW ? pv[i + 1] : 0.f, pd = i + W < HW ? pv[i + W] : 0.f;   // wd is 0 in the last row
      const float nb = (wl * pl + wr[i] * pr) + (wu * pu + wd[i] * pd);
      const float q = dg > 0.f ? dg * pc - nb : 0.f;
      qv[i] = q;
      pq += pc * q;
    }
    pq = block_sum(pq, red);
    if (!(pq > 0.f)) break;                                // (L_uu is positive definite: only a breakdown in fp32 gets here)
    const float alpha = rz / pq;
    float rr_n = 0.f, rz_n = 0.f;
    for (int i = tid; i < HW; i += kThreads) {
      xv[i] += alpha * pv[i];
      const float r = rv[i] - alpha * qv[i], z = r * invd[i];
      rv[i] = r;
      rr_n += r * r, rz_n += r * z;
    }
    rr = block_sum(rr_n, red), rz_n = block_sum(rz_n, red);
    const float beta = rz_n / rz;
    rz = rz_n;
    for (int i = tid; i < HW; i += kThreads) pv[i] = rv[i] * invd[i] + beta * pv[i];
    ++it;
  }
  if (tid == 0) iters[sysi] = it, resid[sysi] = sqrtf(rr) / bnorm;
}

__global__ __launch_bounds__(256) void rw_finish_kernel(RwP a, const uint8_t* seed, uint8_t* label, float* prob) {
  const int n = blockIdx.y, K = a.K, HW = a.HW;
  const bool ok = a.ok[n] != 0;
  const int64_t sb = (int64_t)n * HW;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < HW; i += gridDim.x * kThreads) {
    const int s = seed[sb + i];
    const bool seeded = s < K;
    int best = 0;
    float bv = 0.f;
    for (int k = 0; k < K; ++k) {
      float v = 0.f;
      if (ok) v = seeded ? (s == k ? 1.f : 0.f) : a.sys[((int64_t)n * K + k) * kRwSysPlanes * HW + i];
      if (prob) prob[((int64_t)n * K + k) * HW + i] = v;
      if (k == 0 || v > bv) best = k, bv = v;              // strict: a tie keeps the lowest class
    }
    label[sb + i] = (uint8_t)(ok ? (seeded ? s : best) : 0);
  }
}

}  // namespace wsl

using namespace wsl;

static bool rw_supported(int N, int H, int W, int K) {
  return N > 0 && H >= 2 && W >= 2 && (int64_t)H * W <= kRwMaxPixels && K >= 2 && K <= kRwMaxC && N <= 65535;
}

extern "C" size_t wsl_random_walker_ws_bytes(int N, int H, int W, int n_class) {
  if (!rw_supported(N, H, W, n_class)) return 0;
  return sizeof(float) * (rw_head_words(N) + (size_t)N * H * W * (kRwSlicePlanes + (size_t)kRwSysPlanes * n_class));
}

extern "C" int wsl_random_walker(const float* img, const uint8_t* seed, uint8_t* label_out, float* prob_out, int* iters_out,
                                 float* resid_out, int N, int H, int W, int n_class, float beta, float tol, int max_iter, void* ws,
                                 size_t ws_bytes, void* stream) {
  WSL_REQUIRE(img && seed && label_out && iters_out && resid_out, "random_walker: null argument");
  WSL_REQUIRE(beta >= 0.f && tol >= 0.f, "random_walker: beta %g / tol %g must not be negative", (double)beta, (double)tol);
  if (!rw_supported(N, H, W, n_class) || max_iter < 0 || max_iter > kRwMaxIter) {
    set_error("random_walker: unsupported N %d, H %d, W %d, n_class %d, max_iter %d (1 <= N <= 65535, H, W >= 2, H * W <= %d, 2 <= n_class "
              "<= %d, 0 <= max_iter <= %d)", N, H, W, n_class, max_iter, kRwMaxPixels, kRwMaxC, kRwMaxIter);
    return WSL_EUNSUPPORTED;
  }
  const size_t need = wsl_random_walker_ws_bytes(N, H, W, n_class);
  if (!ws || ws_bytes < need) {
    set_error("random_walker: workspace %zu < %zu", ws_bytes, need);
    return WSL_EWORKSPACE;
  }
  const int HW = H * W;
  float* base = static_cast<float*>(ws);
  float* planes = base + rw_head_words(N);
  const size_t sp = (size_t)N * HW;
  RwP a{base, reinterpret_cast<int*>(base + N), planes, planes + sp, planes + 2 * sp, planes + 3 * sp, planes + kRwSlicePlanes * sp,
        H, W, HW, n_class};
  ProfScope ps(PF_OTHER, 0.0, (double)sp * (5.0 + 4.0 * (kRwSlicePlanes + kRwSysPlanes * n_class)), stream);
  const dim3 px(cdiv(HW, kThreads * 4), N);
  WSL_LAUNCH(rw_stats_kernel, dim3(N), dim3(kThreads), 0, stream, img, seed, HW, n_class, beta, base, reinterpret_cast<int*>(base + N));
  WSL_LAUNCH(rw_setup_kernel, px, dim3(kThreads), 0, stream, a, img, seed);
  WSL_LAUNCH(rw_pcg_kernel, dim3(n_class, N), dim3(kThreads), 0, stream, a, tol, max_iter, iters_out, resid_out);
  WSL_LAUNCH(rw_finish_kernel, px, dim3(kThreads), 0, stream, a, seed, label_out, prob_out);
  return check_launch("random_walker");
}
