// The adversary of the semi-supervised DAN trainer (ref: networks/discriminator.py FCDiscriminator; trainer
// train_deep_adversarial_network_2D.py): 4x4 stride-2 padding-1 convolutions as fp32-MFMA implicit GEMMs for gfx950, the pooled
// 2-class head, Adam, and the host-side sequencing of one discriminator forward / backward over flat arenas.
//
//   forward        M = 16 consecutive output pixels of a row, N = 16 output channels, K = 4 input channels of one of the 16 taps per
//                  v_mfma_f32_16x16x4_f32.  A workgroup owns 8 x 16 output pixels x CO_T channels; its input tile is 18 rows x 34
//                  columns per channel, staged with the columns DE-INTERLEAVED (even columns, then odd ones): tap kx of pixel m reads
//                  column 2m + kx, which is index m + (kx >> 1) of half (kx & 1) -- contiguous over the 16 lanes of an operand row, so
//                  the stride-2 walk costs no LDS bank conflict.  Up to two sources (conv0(map) + conv1(image) as ONE pass with bias
//                  b0 + b1); the loader applies LeakyReLU(0.2) and the Dropout2d channel multiplier of the producing layer; the
//                  epilogue adds the bias and stores the pre-activation.
//   data gradient  the transposed convolution by output parity: input row iy = 2j + py receives taps ky = 1 - py + 2a from output
//                  rows oy = j + py - a (a = 0, 1), likewise for columns -- each of the four phases is a 2x2-tap stride-1 convolution
//                  of dy with K = Co x 4.  The loader forms dy = g * cmask * leaky'(z) from the incoming gradient, the saved
//                  pre-activation and the mask.  Every element of dx is written exactly once; nothing is scattered.
//   weight gradient M = 16 output channels, N = 16 input channels, K = 4 pixels, sixteen accumulators per channel pair; partials
//                  [nsplit][16][Co][Ci] (+ [nsplit][Co]) reduced by wsl_wgrad_reduce_batch (wsl_conv.hip) in a fixed order.
//
// Any N, Ci, Co >= 1 and H, W >= 2 is correct (Ho = H / 2; halo, ragged tiles and channel tails are masked); alignment only selects
// vector loads / stores.  No atomics anywhere: two calls give the same bits.
#include "wsl_seq.h"

namespace wsl {
namespace {

constexpr float kSlope = WSL_DAN_LEAKY_SLOPE;
__device__ __forceinline__ float dan_leaky(float z) { return z > 0.f ? z : kSlope * z; }

// the activation a convolution reads: source a [N][Ca][H][W] (optionally LeakyReLU(0.2), then the channel multiplier) and a raw
// source b [N][Cb][H][W] behind it on the channel axis
struct C4In {
  const float* xa;
  const float* xb;
  const float* cmask;   // [N][Ca] or null
  int Ca, Cb, act, H, W;
};
__device__ __forceinline__ float c4_in(const C4In& t, int n, int c, int gy, int gx) {
  if (gy < 0 || gy >= t.H || gx < 0 || gx >= t.W) return 0.f;
  const int64_t hw = (int64_t)t.H * t.W, off = (int64_t)gy * t.W + gx;
  if (c < t.Ca) {
    float v = t.xa[((int64_t)n * t.Ca + c) * hw + off];
    if (t.act) v = dan_leaky(v);
    if (t.cmask) v *= t.cmask[(int64_t)n * t.Ca + c];
    return v;
  }
  c -= t.Ca;
  return c < t.Cb ? t.xb[((int64_t)n * t.Cb + c) * hw + off] : 0.f;
}

// the gradient at a convolution's output: dy = g * cmask[n, co] * leaky'(z)  (z null: g is already d/d(pre-activation))
struct C4Dy {
  const float* g;
  const float* z;
  const float* cmask;   // [N][Co] or null
  int Co, Ho, Wo;
};
__device__ __forceinline__ float c4_dy(const C4Dy& t, int n, int co, int oy, int ox) {
  if (co >= t.Co || oy < 0 || oy >= t.Ho || ox < 0 || ox >= t.Wo) return 0.f;
  const int64_t i = (((int64_t)n * t.Co + co) * t.Ho + oy) * t.Wo + ox;
  float v = t.g[i];
  if (t.cmask) v *= t.cmask[(int64_t)n * t.Co + co];
  if (t.z) v = t.z[i] > 0.f ? v : v * kSlope;
  return v;
}

constexpr int kTH = 8, kTW = 16;              // output tile of the forward / phase tile of the data gradient
constexpr size_t kMaxSmem = 160 * 1024;       // LDS of one gfx950 CU

static int pick_co_t(int64_t tiles, int Cn) {
  int co_t = Cn <= 16 ? 16 : (Cn <= 32 ? 32 : 64);
  const int64_t enough = 2 * (int64_t)device_cu_count();
  while (co_t > 16 && tiles * cdiv(Cn, co_t) < enough) co_t >>= 1;
  return co_t;
}

// ------------------------------------------------------------------------------------------------ forward
struct C4FwdP {
  C4In in;
  const float* wa;   // [Co][Ca][4][4]
  const float* wb;   // [Co][Cb][4][4]
  const float* ba;
  const float* bb;
  float* y;          // [N][Co][Ho][Wo]
  int N, Co, Ho, Wo, tiles_y, tiles_x, vec_w, vec_y;
};

template <int CO_T>
struct C4FwdCfg {
  static constexpr int KC = 8, ROWS = 2 * kTH + 2, HALF = kTW + 1, ROWP = 2 * HALF;
  static constexpr int PLANE = ((ROWS * ROWP - 16 + 31) / 32) * 32 + 16;   // == 16 (mod 32)
  static constexpr int CSTR = (CO_T % 32 == 0) ? CO_T + 16 : CO_T;
  static constexpr int MT = kTH / 4, NT = CO_T / 16;
  static constexpr size_t SMEM = sizeof(float) * (KC * PLANE + 16 * KC * CSTR);
};

template <int CO_T>
__global__ __launch_bounds__(256) void c4_fwd_kernel(C4FwdP p) {
  using C = C4FwdCfg<CO_T>;
  WSL_DYN_SMEM(smem);
  float* in_t = reinterpret_cast<float*>(smem);
  float* w_t = in_t + C::KC * C::PLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int item = blockIdx.x;
  const int tx_i = item % p.tiles_x;
  item /= p.tiles_x;
  const int ty_i = item % p.tiles_y, n = item / p.tiles_y;
  const int oy0 = ty_i * kTH, ox0 = tx_i * kTW, co0 = blockIdx.y * CO_T;
  const int Ca = p.in.Ca, Ci = p.in.Ca + p.in.Cb;
  constexpr int TILE = C::ROWS * C::ROWP;

  v4f acc[C::MT][C::NT];
#pragma unroll
  for (int i = 0; i < C::MT; ++i)
#pragma unroll
    for (int j = 0; j < C::NT; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
  int abase[C::MT];
#pragma unroll
  for (int i = 0; i < C::MT; ++i) abase[i] = (lane >> 4) * C::PLANE + 2 * (wave * C::MT + i) * C::ROWP + (lane & 15);
  const int bbase = (lane >> 4) * C::CSTR + (lane & 15);

  for (int c0 = 0; c0 < Ci; c0 += C::KC) {
    // ---- input tile of channels [c0, c0 + KC): rows 2 oy0 - 1 + ty, columns 2 ox0 - 1 + t, even t first
    for (int e = tid; e < C::KC * TILE; e += kThreads) {
      const int c = e / TILE, rem = e - c * TILE;
      const int ty = rem / C::ROWP, tx = rem - ty * C::ROWP;
      const int t = tx < C::HALF ? 2 * tx : 2 * (tx - C::HALF) + 1;
      in_t[c * C::PLANE + rem] = c4_in(p.in, n, c0 + c, 2 * oy0 - 1 + ty, 2 * ox0 - 1 + t);
    }
    // ---- weights of this chunk as w_t[tap][c][co]
    if (p.vec_w) {
      for (int e = tid; e < CO_T * C::KC * 4; e += kThreads) {
        const int co = e % CO_T, q = e / CO_T, t4 = q & 3, c = q >> 2;
        const int cog = co0 + co, cg = c0 + c;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (cog < p.Co && cg < Ci) {
          const float* src = cg < Ca ? p.wa + ((int64_t)cog * Ca + cg) * 16 : p.wb + ((int64_t)cog * p.in.Cb + (cg - Ca)) * 16;
          v = *reinterpret_cast<const float4*>(src + t4 * 4);
        }
        float* dst = w_t + ((t4 * 4) * C::KC + c) * C::CSTR + co;
        dst[0] = v.x, dst[C::KC * C::CSTR] = v.y, dst[2 * C::KC * C::CSTR] = v.z, dst[3 * C::KC * C::CSTR] = v.w;
      }
    } else {
      for (int e = tid; e < CO_T * C::KC * 16; e += kThreads) {
        const int co = e % CO_T, q = e / CO_T, tap = q & 15, c = q >> 4;
        const int cog = co0 + co, cg = c0 + c;
        float v = 0.f;
        if (cog < p.Co && cg < Ci)
          v = cg < Ca ? p.wa[((int64_t)cog * Ca + cg) * 16 + tap] : p.wb[((int64_t)cog * p.in.Cb + (cg - Ca)) * 16 + tap];
        w_t[(tap * C::KC + c) * C::CSTR + co] = v;
      }
    }
    __syncthreads();
    const int ngroups = (Ci - c0 >= C::KC) ? C::KC / 4 : (Ci - c0 + 3) / 4;
#pragma unroll
    for (int tap = 0; tap < 16; ++tap) {
      const int toff = (tap >> 2) * C::ROWP + (tap & 1) * C::HALF + ((tap & 3) >> 1);
#pragma unroll
      for (int cg = 0; cg < C::KC / 4; ++cg) {
        if (cg < ngroups) {
          float bv[C::NT];
#pragma unroll
          for (int j = 0; j < C::NT; ++j) bv[j] = w_t[(tap * C::KC + cg * 4) * C::CSTR + j * 16 + bbase];
#pragma unroll
          for (int i = 0; i < C::MT; ++i) {
            const float av = in_t[cg * 4 * C::PLANE + toff + abase[i]];
#pragma unroll
            for (int j = 0; j < C::NT; ++j) acc[i][j] = WSL_MFMA16(av, bv[j], acc[i][j]);
          }
        }
      }
    }
    __syncthreads();
  }

  // ---- epilogue: bias (b0 + b1 of a merged layer), pre-activation store
  const int64_t HWo = (int64_t)p.Ho * p.Wo;
#pragma unroll
  for (int j = 0; j < C::NT; ++j) {
    const int co = co0 + j * 16 + (lane & 15);
    float bias = 0.f;
    if (co < p.Co) {
      if (p.ba) bias = p.ba[co];
      if (p.bb) bias += p.bb[co];
    }
#pragma unroll
    for (int i = 0; i < C::MT; ++i) {
      const int oy = oy0 + wave * C::MT + i, ox = ox0 + (lane >> 4) * 4;
      if (co < p.Co && oy < p.Ho) {
        const v4f v = acc[i][j];
        float* dst = p.y + ((int64_t)n * p.Co + co) * HWo + (int64_t)oy * p.Wo + ox;
        if (p.vec_y && ox + 3 < p.Wo) {
          *reinterpret_cast<float4*>(dst) = make_float4(v[0] + bias, v[1] + bias, v[2] + bias, v[3] + bias);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (ox + r < p.Wo) dst[r] = v[r] + bias;
        }
      }
    }
  }
}

template <int CO_T>
static int launch_c4_fwd(const C4FwdP& p, void* stream) {
  using C = C4FwdCfg<CO_T>;
  auto kern = c4_fwd_kernel<CO_T>;
  static_assert(C::SMEM <= kMaxSmem, "forward tile exceeds the LDS");
  static bool attr_done = false;
  if (!attr_done) {
    (void)WSL_SET_MAX_DYN_SMEM(kern, C::SMEM);
    attr_done = true;
  }
  const dim3 grid((unsigned)(p.N * p.tiles_y * p.tiles_x), cdiv(p.Co, CO_T));
  const double px = (double)p.N * p.Ho * p.Wo, Ci = p.in.Ca + p.in.Cb;
  void* tok = prof_begin(PF_CONV_FWD, 2.0 * px * p.Co * Ci * 16, 4.0 * px * (p.Co + 4.0 * Ci), stream);
  WSL_LAUNCH(kern, grid, dim3(kThreads), C::SMEM, stream, p);
  prof_end(tok, stream);
  return check_launch("c4_fwd_kernel");
}

// ------------------------------------------------------------------------------------------------ data gradient
struct C4DgP {
  C4Dy dy;
  const float* w;   // [Co][Ci][4][4]
  float* dx;        // [N][Ci][H][W]
  int N, Ci, H, W, tiles_y, tiles_x;
};

template <int CI_T>
struct C4DgCfg {
  static constexpr int KC = 32, ROWS = kTH + 1, ROWP = kTW + 1;
  static constexpr int PLANE = ((ROWS * ROWP - 16 + 31) / 32) * 32 + 16;
  static constexpr int CSTR = (CI_T % 32 == 0) ? CI_T + 16 : CI_T;
  static constexpr int MT = kTH / 4, NT = CI_T / 16;
  static constexpr size_t SMEM = sizeof(float) * (KC * PLANE + 4 * KC * CSTR);
};

template <int CI_T>
__global__ __launch_bounds__(256) void c4_dgrad_kernel(C4DgP p) {
  using C = C4DgCfg<CI_T>;
  WSL_DYN_SMEM(smem);
  float* dy_t = reinterpret_cast<float*>(smem);
  float* w_t = dy_t + C::KC * C::PLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int item = blockIdx.x;
  const int tx_i = item % p.tiles_x;
  item /= p.tiles_x;
  const int ty_i = item % p.tiles_y;
  item /= p.tiles_y;
  const int ph = item & 3, n = item >> 2;
  const int py = ph >> 1, px = ph & 1;
  const int j0 = ty_i * kTH, i0 = tx_i * kTW, ci0 = blockIdx.y * CI_T;
  const int Co = p.dy.Co;
  constexpr int TILE = C::ROWS * C::ROWP;

  v4f acc[C::MT][C::NT];
#pragma unroll
  for (int i = 0; i < C::MT; ++i)
#pragma unroll
    for (int j = 0; j < C::NT; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
  int abase[C::MT];
#pragma unroll
  for (int i = 0; i < C::MT; ++i) abase[i] = (lane >> 4) * C::PLANE + (wave * C::MT + i) * C::ROWP + (lane & 15);
  const int bbase = (lane >> 4) * C::CSTR + (lane & 15);

  for (int c0 = 0; c0 < Co; c0 += C::KC) {
    // ---- dy tile of output channels [c0, c0 + KC): rows j0 + py - 1 + tr, columns i0 + px - 1 + tc, transformed
    for (int e = tid; e < C::KC * TILE; e += kThreads) {
      const int c = e / TILE, rem = e - c * TILE;
      const int tr = rem / C::ROWP, tc = rem - tr * C::ROWP;
      dy_t[c * C::PLANE + rem] = c4_dy(p.dy, n, c0 + c, j0 + py - 1 + tr, i0 + px - 1 + tc);
    }
    // ---- the phase's four taps as w_t[2a + b][c][ci] = w[co][ci][1 - py + 2a][1 - px + 2b]
    for (int e = tid; e < CI_T * C::KC * 4; e += kThreads) {
      const int ci = e % CI_T, q = e / CI_T, tap = q & 3, c = q >> 2;
      const int cig = ci0 + ci, cog = c0 + c;
      const int ky = 1 - py + 2 * (tap >> 1), kx = 1 - px + 2 * (tap & 1);
      float v = 0.f;
      if (cig < p.Ci && cog < Co) v = p.w[((int64_t)cog * p.Ci + cig) * 16 + ky * 4 + kx];
      w_t[(tap * C::KC + c) * C::CSTR + ci] = v;
    }
    __syncthreads();
    const int ngroups = (Co - c0 >= C::KC) ? C::KC / 4 : (Co - c0 + 3) / 4;
#pragma unroll
    for (int tap = 0; tap < 4; ++tap) {
      const int toff = (1 - (tap >> 1)) * C::ROWP + (1 - (tap & 1));
#pragma unroll 2
      for (int cg = 0; cg < C::KC / 4; ++cg) {
        if (cg < ngroups) {
          float bv[C::NT];
#pragma unroll
          for (int j = 0; j < C::NT; ++j) bv[j] = w_t[(tap * C::KC + cg * 4) * C::CSTR + j * 16 + bbase];
#pragma unroll
          for (int i = 0; i < C::MT; ++i) {
            const float av = dy_t[cg * 4 * C::PLANE + toff + abase[i]];
#pragma unroll
            for (int j = 0; j < C::NT; ++j) acc[i][j] = WSL_MFMA16(av, bv[j], acc[i][j]);
          }
        }
      }
    }
    __syncthreads();
  }

  const int64_t HW = (int64_t)p.H * p.W;
#pragma unroll
  for (int j = 0; j < C::NT; ++j) {
    const int ci = ci0 + j * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < C::MT; ++i) {
      const int iy = 2 * (j0 + wave * C::MT + i) + py;
      if (ci < p.Ci && iy < p.H) {
        float* dst = p.dx + ((int64_t)n * p.Ci + ci) * HW + (int64_t)iy * p.W;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ix = 2 * (i0 + (lane >> 4) * 4 + r) + px;
          if (ix < p.W) dst[ix] = acc[i][j][r];
        }
      }
    }
  }
}

template <int CI_T>
static int launch_c4_dgrad(const C4DgP& p, void* stream) {
  using C = C4DgCfg<CI_T>;
  auto kern = c4_dgrad_kernel<CI_T>;
  static_assert(C::SMEM <= kMaxSmem, "data-gradient tile exceeds the LDS");
  static bool attr_done = false;
  if (!attr_done) {
    (void)WSL_SET_MAX_DYN_SMEM(kern, C::SMEM);
    attr_done = true;
  }
  const dim3 grid((unsigned)(p.N * 4 * p.tiles_y * p.tiles_x), cdiv(p.Ci, CI_T));
  const double px = (double)p.N * p.dy.Ho * p.dy.Wo;
  void* tok = prof_begin(PF_CONV_DGRAD, 2.0 * px * p.dy.Co * p.Ci * 16, 4.0 * px * (p.dy.Co + 4.0 * p.Ci), stream);
  WSL_LAUNCH(kern, grid, dim3(kThreads), C::SMEM, stream, p);
  prof_end(tok, stream);
  return check_launch("c4_dgrad_kernel");
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct C4WgP {
  C4In in;          // one source (xa)
  C4Dy dy;
  float* part_dw;   // [nsplit][16][Co][Ci]
  float* part_db;   // [nsplit][Co]
  int N, items, nsplit, co_blocks, tiles_y, tiles_x;
};

constexpr int kWgTH = 4;

template <int CB, int WK>
struct C4WgCfg {
  static constexpr int IB = CB, ROWS = 2 * kWgTH + 2, HALF = kTW + 1, ROWP = 2 * HALF, S = kWgTH * kTW;
  static constexpr int PLD = ((S - 2 + 31) / 32) * 32 + 2;               // == 2 (mod 32)
  static constexpr int PLA = ((ROWS * ROWP - 2 + 31) / 32) * 32 + 2;     // == 2 (mod 32)
  static constexpr int CBT = CB / 16, PAIRS = CBT * CBT, WP = 4 / WK, PP = PAIRS / WP;
  static constexpr int TILE_FLOATS = CB * PLD + IB * PLA;
  static constexpr int PER = PP * 17 * 4;
  static constexpr int RED_FLOATS = (WK > 1) ? 4 * 64 * PER : 0;
  static constexpr size_t SMEM = sizeof(float) * (TILE_FLOATS > RED_FLOATS ? TILE_FLOATS : RED_FLOATS);
  static_assert(PAIRS % WP == 0 && kWgTH % WK == 0, "wgrad tile shape");
};

template <int CB, int WK>
__global__ __launch_bounds__(256) void c4_wgrad_kernel(C4WgP p) {
  using C = C4WgCfg<CB, WK>;
  WSL_DYN_SMEM(smem);
  float* dy_t = reinterpret_cast<float*>(smem);
  float* a_t = dy_t + CB * C::PLD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cb = blockIdx.x % p.co_blocks, ib = blockIdx.x / p.co_blocks, split = blockIdx.y;
  const int co0 = cb * CB, ci0 = ib * C::IB;
  const int wp = wave % C::WP, wk = wave / C::WP;
  const int Co = p.dy.Co, Ci = p.in.Ca;
  constexpr int ATILE = C::ROWS * C::ROWP;

  v4f acc[C::PP][16];
  v4f accb[C::PP];
#pragma unroll
  for (int j = 0; j < C::PP; ++j) {
    accb[j] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[j][t] = v4f{0.f, 0.f, 0.f, 0.f};
  }
  const bool want_db = (ib == 0) && (p.part_db != nullptr);
  const int it0 = (int)((int64_t)split * p.items / p.nsplit), it1 = (int)((int64_t)(split + 1) * p.items / p.nsplit);
  for (int item = it0; item < it1; ++item) {
    int q = item;
    const int tx_i = q % p.tiles_x;
    q /= p.tiles_x;
    const int ty_i = q % p.tiles_y, n = q / p.tiles_y;
    const int oy0 = ty_i * kWgTH, ox0 = tx_i * kTW;
    for (int e = tid; e < CB * C::S; e += kThreads) {
      const int c = e / C::S, rem = e - c * C::S;
      dy_t[c * C::PLD + rem] = c4_dy(p.dy, n, co0 + c, oy0 + rem / kTW, ox0 + rem % kTW);
    }
    for (int e = tid; e < C::IB * ATILE; e += kThreads) {
      const int c = e / ATILE, rem = e - c * ATILE;
      const int ty = rem / C::ROWP, tx = rem - ty * C::ROWP;
      const int t = tx < C::HALF ? 2 * tx : 2 * (tx - C::HALF) + 1;
      a_t[c * C::PLA + rem] = c4_in(p.in, n, ci0 + c, 2 * oy0 - 1 + ty, 2 * ox0 - 1 + t);
    }
    __syncthreads();
    constexpr int RW = kWgTH / WK;
#pragma unroll 1
    for (int r = wk * RW; r < wk * RW + RW; ++r) {
#pragma unroll 1
      for (int x4 = 0; x4 < kTW / 4; ++x4) {
        const int pix = r * kTW + x4 * 4 + (lane >> 4);
        const int apix = 2 * r * C::ROWP + x4 * 4 + (lane >> 4);
#pragma unroll
        for (int j = 0; j < C::PP; ++j) {
          const int pr = wp * C::PP + j, cot = pr / C::CBT, cit = pr % C::CBT;
          const float av = dy_t[(cot * 16 + (lane & 15)) * C::PLD + pix];
          if (want_db && cit == 0) accb[j] = WSL_MFMA16(av, 1.0f, accb[j]);
#pragma unroll
          for (int t = 0; t < 16; ++t) {
            const float bv = a_t[(cit * 16 + (lane & 15)) * C::PLA + apix + (t >> 2) * C::ROWP + (t & 1) * C::HALF + ((t & 3) >> 1)];
            acc[j][t] = WSL_MFMA16(av, bv, acc[j][t]);
          }
        }
      }
    }
    __syncthreads();
  }
  // ---- merge the WK row groups (fixed order) and store partials
  if (WK > 1) {
    float* red = reinterpret_cast<float*>(smem);
    float* mine = red + (wave * 64 + lane) * C::PER;
#pragma unroll
    for (int j = 0; j < C::PP; ++j) {
#pragma unroll
      for (int t = 0; t < 16; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) mine[(j * 17 + t) * 4 + r] = acc[j][t][r];
#pragma unroll
      for (int r = 0; r < 4; ++r) mine[(j * 17 + 16) * 4 + r] = accb[j][r];
    }
    __syncthreads();
    if (wk == 0) {
#pragma unroll
      for (int j = 0; j < C::PP; ++j) {
#pragma unroll
        for (int t = 0; t <= 16; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float s = 0.f;
            for (int k = 0; k < WK; ++k) s += red[((k * C::WP + wp) * 64 + lane) * C::PER + (j * 17 + t) * 4 + r];
            if (t < 16) acc[j][t][r] = s; else accb[j][r] = s;
          }
      }
    }
  }
  if (wk == 0) {
#pragma unroll
    for (int j = 0; j < C::PP; ++j) {
      const int pr = wp * C::PP + j, cot = pr / C::CBT, cit = pr % C::CBT;
      const int ci = ci0 + cit * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + cot * 16 + (lane >> 4) * 4 + r;
        if (co < Co && ci < Ci) {
#pragma unroll
          for (int t = 0; t < 16; ++t) p.part_dw[(((int64_t)split * 16 + t) * Co + co) * Ci + ci] = acc[j][t][r];
        }
        if (want_db && cit == 0 && (lane & 15) == 0 && co < Co) p.part_db[(int64_t)split * Co + co] = accb[j][r];
      }
    }
  }
}

struct C4WgPlan { int cb, nsplit, items, tiles_y, tiles_x, co_blocks, ci_blocks; };

static C4WgPlan c4_wgrad_plan(int N, int H, int W, int Ci, int Co) {
  C4WgPlan g;
  g.cb = (Co <= 16 || Ci <= 16) ? 16 : 32;
  g.tiles_y = cdiv(H / 2, kWgTH), g.tiles_x = cdiv(W / 2, kTW);
  g.items = N * g.tiles_y * g.tiles_x;
  g.co_blocks = cdiv(Co, g.cb), g.ci_blocks = cdiv(Ci, g.cb);
  int want = 768 / (g.co_blocks * g.ci_blocks);   // pixel splits of the whole launch: three rounds over the 256 CUs
  if (want < 1) want = 1;
  g.nsplit = g.items < want ? g.items : want;
  return g;
}

template <int CB, int WK>
static int launch_c4_wgrad(const C4WgP& p, const C4WgPlan& g, void* stream) {
  using C = C4WgCfg<CB, WK>;
  auto kern = c4_wgrad_kernel<CB, WK>;
  static_assert(C::SMEM <= kMaxSmem, "weight-gradient tile exceeds the LDS");
  static bool attr_done = false;
  if (!attr_done) {
    (void)WSL_SET_MAX_DYN_SMEM(kern, C::SMEM);
    attr_done = true;
  }
  const dim3 grid(g.co_blocks * g.ci_blocks, g.nsplit);
  const double px = (double)p.N * p.dy.Ho * p.dy.Wo;
  void* tok = prof_begin(PF_WGRAD_DIRECT, 2.0 * px * p.dy.Co * p.in.Ca * 16, 4.0 * px * (p.dy.Co + 4.0 * p.in.Ca), stream);
  WSL_LAUNCH(kern, grid, dim3(kThreads), C::SMEM, stream, p);
  prof_end(tok, stream);
  return check_launch("c4_wgrad_kernel");
}

// ------------------------------------------------------------------------------------------------ head
// feat[n][c*4 + pos] = mean over the pool x pool window `pos` of leaky(z4);  logits = Wc feat + bc;  2-class cross entropy (mean over N)
struct HeadP {
  const float* z;        // [N][C][H][W] pre-activation of conv4
  const float* Wc;       // [2][4C]
  const float* bc;       // [2]
  const int32_t* target; // [N] in {0, 1} or null (logits only)
  float* feat;           // [N][4C]
  float* dlg;            // [N][2]
  float* lossn;          // [N]
  float* logits;         // [N][2]
  int N, C, H, W, pool, wp;
  float gscale;
};

__global__ __launch_bounds__(256) void dan_head_fwd_kernel(HeadP p) {
  __shared__ float red[4];
  const int n = blockIdx.x, tid = threadIdx.x, F = 4 * p.C;
  const float inv = 1.f / (float)(p.pool * p.pool);
  for (int f = tid; f < F; f += kThreads) {
    const int c = f >> 2, pos = f & 3, y0 = (pos / p.wp) * p.pool, x0 = (pos % p.wp) * p.pool;
    const float* src = p.z + (((int64_t)n * p.C + c) * p.H + y0) * p.W + x0;
    float s = 0.f;
    for (int yy = 0; yy < p.pool; ++yy)
      for (int xx = 0; xx < p.pool; ++xx) s += dan_leaky(src[(int64_t)yy * p.W + xx]);
    p.feat[(int64_t)n * F + f] = s * inv;
  }
  __syncthreads();
  float lg[2];
  for (int k = 0; k < 2; ++k) {
    float s = 0.f;
    for (int f = tid; f < F; f += kThreads) s = fmaf(p.Wc[(int64_t)k * F + f], p.feat[(int64_t)n * F + f], s);
    lg[k] = block_sum(s, red) + p.bc[k];
  }
  if (tid == 0) {
    p.logits[2 * n] = lg[0], p.logits[2 * n + 1] = lg[1];
    if (p.target) {
      const float m = fmaxf(lg[0], lg[1]);
      const float lse = m + logf(expf(lg[0] - m) + expf(lg[1] - m));
      const int t = p.target[n] != 0;
      p.lossn[n] = lse - lg[t];
      const float k = p.gscale / (float)p.N;
      p.dlg[2 * n] = (expf(lg[0] - lse) - (t == 0 ? 1.f : 0.f)) * k;
      p.dlg[2 * n + 1] = (expf(lg[1] - lse) - (t == 1 ? 1.f : 0.f)) * k;
    }
  }
}

__global__ __launch_bounds__(256) void dan_loss_kernel(const float* lossn, int N, float* loss) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += lossn[n];
    loss[0] = s / (float)N;
  }
}

// dz4 = (W^T dlogits)[c*4 + pos] / pool^2 * leaky'(z4) inside the pooled windows, 0 in the rows / columns the floor drops
__global__ __launch_bounds__(256) void dan_head_bwd_kernel(HeadP p, const float* dlg, float* dz) {
  const int64_t HW = (int64_t)p.H * p.W, total = (int64_t)p.N * p.C * HW;
  const int F = 4 * p.C, hp = 4 / p.wp;
  const float inv = 1.f / (float)(p.pool * p.pool);
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t nc = i / HW, rem = i - nc * HW;
    const int n = (int)(nc / p.C), c = (int)(nc - (int64_t)n * p.C);
    const int y = (int)(rem / p.W), x = (int)(rem - (int64_t)y * p.W);
    float v = 0.f;
    if (y < hp * p.pool && x < p.wp * p.pool) {
      const int f = c * 4 + (y / p.pool) * p.wp + x / p.pool;
      const float df = fmaf(dlg[2 * n + 1], p.Wc[F + f], dlg[2 * n] * p.Wc[f]) * inv;
      v = p.z[i] > 0.f ? df : df * kSlope;
    }
    dz[i] = v;
  }
}

// classifier gradients: dW[k][f] = sum_n dlogits[n][k] feat[n][f], db[k] = sum_n dlogits[n][k]  (n ascending)
__global__ __launch_bounds__(256) void dan_head_param_kernel(const float* feat, const float* dlg, int N, int F, float* dW, float* db) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < 2 * F) {
    const int k = i / F, f = i - k * F;
    float s = 0.f;
    for (int n = 0; n < N; ++n) s = fmaf(dlg[2 * n + k], feat[(int64_t)n * F + f], s);
    dW[i] = s;
  } else if (i < 2 * F + 2) {
    const int k = i - 2 * F;
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += dlg[2 * n + k];
    db[k] = s;
  }
}

static unsigned ew_grid(int64_t total) {
  int64_t b = (total + kThreads - 1) / kThreads;
  const int64_t cap = 16 * (int64_t)device_cu_count();
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

static int head_shape(int H, int W, int pool, int* wp) {
  WSL_REQUIRE(pool >= 1, "dan_head: pool %d", pool);
  const int hp = H / pool, w = W / pool;
  WSL_REQUIRE(hp * w == 4, "dan_head: the %dx%d map pools (%d) to %dx%d; Linear(ndf*32, 2) needs exactly 4 positions", H, W, pool, hp, w);
  *wp = w;
  return WSL_OK;
}

struct HeadWs { size_t feat, dlg, lossn, total; };
static HeadWs head_ws(int N, int C) {
  Bump B;
  HeadWs h;
  h.feat = B.take((size_t)N * 4 * C), h.dlg = B.take((size_t)N * 2), h.lossn = B.take((size_t)N), h.total = B.off;
  return h;
}

static int head_fwd(HeadP& p, float* loss, void* stream) {
  ProfScope ps(PF_LOSS_HEAD, 0.0, 4.0 * (double)p.N * p.C * p.H * p.W, stream);
  WSL_LAUNCH(dan_head_fwd_kernel, dim3(p.N), dim3(kThreads), 0, stream, p);
  WSL_TRY(check_launch("dan_head_fwd_kernel"));
  if (p.target && loss) {
    WSL_LAUNCH(dan_loss_kernel, dim3(1), dim3(kThreads), 0, stream, p.lossn, p.N, loss);
    WSL_TRY(check_launch("dan_loss_kernel"));
  }
  return WSL_OK;
}
static int head_bwd(const HeadP& p, const float* dlg, float* dz, float* dW, float* db, void* stream) {
  ProfScope ps(PF_LOSS_HEAD, 0.0, 8.0 * (double)p.N * p.C * p.H * p.W, stream);
  WSL_LAUNCH(dan_head_bwd_kernel, dim3(ew_grid((int64_t)p.N * p.C * p.H * p.W)), dim3(kThreads), 0, stream, p, dlg, dz);
  WSL_TRY(check_launch("dan_head_bwd_kernel"));
  if (dW) {
    WSL_LAUNCH(dan_head_param_kernel, dim3(cdiv(8 * p.C + 2, kThreads)), dim3(kThreads), 0, stream, p.feat, dlg, p.N, 4 * p.C, dW, db);
    WSL_TRY(check_launch("dan_head_param_kernel"));
  }
  return WSL_OK;
}

// ------------------------------------------------------------------------------------------------ Adam
__global__ __launch_bounds__(256) void adam_kernel(float* p, const float* g, float* m, float* v, int64_t n, float step_size, float b1,
                                                   float b2, float inv_bc2_sqrt, float eps, float gs) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const float gi = g[i] * gs;
    const float mi = fmaf(1.f - b1, gi - m[i], m[i]);
    const float vi = fmaf(1.f - b2, gi * gi, b2 * v[i]);
    m[i] = mi, v[i] = vi;
    const float denom = sqrtf(vi) * inv_bc2_sqrt + eps;
    p[i] = fmaf(-step_size, mi / denom, p[i]);
  }
}

// ------------------------------------------------------------------------------------------------ the network
struct DanPlan {
  WslDanDesc d;
  ConvRef c0, c1, c2, c3, c4;
  int64_t cls_w, cls_b, n_param;
  int h[5], w[5];   // h[0] x w[0] the input, h[k] x w[k] the output of level k (conv0 + conv1, conv2, conv3, conv4)
  int wp;
  size_t z[5], head, gA, gB, wg, total_floats;
  HeadWs hw;
  size_t wg_bytes;
};

static int dan_layout(const WslDanDesc* d, DanPlan& P) {
  WSL_REQUIRE(d, "dan: null descriptor");
  WSL_REQUIRE(d->num_classes > 0 && d->n_channel > 0 && d->ndf > 0 && d->pool > 0, "dan: bad descriptor (classes %d, channels %d, ndf %d, pool %d)",
              d->num_classes, d->n_channel, d->ndf, d->pool);
  P.d = *d;
  int64_t po = 0;
  const int f = d->ndf;
  plan_conv(P.c0, d->num_classes, f, 4, po);
  plan_conv(P.c1, d->n_channel, f, 4, po);
  plan_conv(P.c2, f, 2 * f, 4, po);
  plan_conv(P.c3, 2 * f, 4 * f, 4, po);
  plan_conv(P.c4, 4 * f, 8 * f, 4, po);
  P.cls_w = po, po += 2 * (int64_t)32 * f;
  P.cls_b = po, po += 2;
  P.n_param = po;
  return WSL_OK;
}

static int dan_plan(const WslDanDesc* d, DanPlan& P) {
  WSL_TRY(dan_layout(d, P));
  WSL_REQUIRE(d->N > 0, "dan: N=%d", d->N);
  P.h[0] = d->H, P.w[0] = d->W;
  for (int k = 1; k <= 4; ++k) {
    WSL_REQUIRE(P.h[k - 1] >= 2 && P.w[k - 1] >= 2, "dan: input %dx%d is too small for four stride-2 levels", d->H, d->W);
    P.h[k] = P.h[k - 1] / 2, P.w[k] = P.w[k - 1] / 2;
  }
  WSL_TRY(head_shape(P.h[4], P.w[4], d->pool, &P.wp));
  const int N = d->N, f = d->ndf;
  Bump B;
  const int ch[5] = {0, f, 2 * f, 4 * f, 8 * f};
  for (int k = 1; k <= 4; ++k) P.z[k] = B.take((size_t)N * ch[k] * P.h[k] * P.w[k]);
  P.hw = head_ws(N, 8 * f);
  P.head = B.take(P.hw.total);
  const size_t z1 = (size_t)N * f * P.h[1] * P.w[1];
  P.gA = B.take(z1), P.gB = B.take(z1);
  auto r256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
  size_t wgb = 0;
  const ConvRef* cv[5] = {&P.c0, &P.c1, &P.c2, &P.c3, &P.c4};
  const int lvl[5] = {0, 0, 1, 2, 3};
  for (int i = 0; i < 5; ++i) {
    const size_t b = r256(wsl_conv4s2_wgrad_ws_bytes(N, P.h[lvl[i]], P.w[lvl[i]], cv[i]->Ci, cv[i]->Co));
    wgb = b > wgb ? b : wgb;
  }
  P.wg_bytes = wgb;
  P.wg = B.take(wgb / sizeof(float) + 64);
  P.total_floats = B.off;
  return WSL_OK;
}

static int dan_entries(const DanPlan& P, int want, WslNetEntry* out) {
  EntryWalk e{want, out};
  e.conv("conv0", "", P.c0), e.conv("conv1", "", P.c1), e.conv("conv2", "", P.c2), e.conv("conv3", "", P.c3), e.conv("conv4", "", P.c4);
  e.put("classifier", "", "weight", 0, 2, 2, 32 * (int64_t)P.d.ndf, 0, 0, P.cls_w);
  e.put("classifier", "", "bias", 0, 1, 2, 0, 0, 0, P.cls_b);
  return e.idx;
}

}  // namespace
}  // namespace wsl

using namespace wsl;

// ================================================================================================ C ABI: kernels
extern "C" int wsl_conv4s2_fwd(const float* xa, int Ca, const float* xb, int Cb, int act, const float* cmask, const float* wa,
                               const float* wb, const float* ba, const float* bb, float* y, int N, int H, int W, int Co, void* stream) {
  WSL_REQUIRE(xa && wa && y, "conv4s2_fwd: null argument");
  WSL_REQUIRE(N > 0 && Ca > 0 && Cb >= 0 && Co > 0, "conv4s2_fwd: bad shape N=%d Ca=%d Cb=%d Co=%d", N, Ca, Cb, Co);
  WSL_REQUIRE(H >= 2 && W >= 2, "conv4s2_fwd: H=%d W=%d (a 4x4 stride-2 padding-1 convolution needs H, W >= 2)", H, W);
  WSL_REQUIRE(Cb == 0 || (xb && wb), "conv4s2_fwd: second source without data or weights");
  C4FwdP p;
  p.in = C4In{xa, Cb ? xb : nullptr, cmask, Ca, Cb, act, H, W};
  p.wa = wa, p.wb = Cb ? wb : nullptr, p.ba = ba, p.bb = Cb ? bb : nullptr, p.y = y;
  p.N = N, p.Co = Co, p.Ho = H / 2, p.Wo = W / 2;
  p.tiles_y = cdiv(p.Ho, kTH), p.tiles_x = cdiv(p.Wo, kTW);
  const int64_t tiles = (int64_t)N * p.tiles_y * p.tiles_x;
  WSL_REQUIRE(tiles < (int64_t)1 << 31, "conv4s2_fwd: %lld tiles", (long long)tiles);
  auto al = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  p.vec_w = al(wa) && (!p.wb || al(wb));
  p.vec_y = (p.Wo % 4 == 0) && al(y);
  switch (pick_co_t(tiles, Co)) {
    case 16: return launch_c4_fwd<16>(p, stream);
    case 32: return launch_c4_fwd<32>(p, stream);
    default: return launch_c4_fwd<64>(p, stream);
  }
}

extern "C" int wsl_conv4s2_dgrad(const float* g, const float* z, const float* cmask, const float* w, float* dx, int N, int Ci, int H,
                                 int W, int Co, void* stream) {
  WSL_REQUIRE(g && w && dx, "conv4s2_dgrad: null argument");
  WSL_REQUIRE(N > 0 && Ci > 0 && Co > 0, "conv4s2_dgrad: bad shape N=%d Ci=%d Co=%d", N, Ci, Co);
  WSL_REQUIRE(H >= 2 && W >= 2, "conv4s2_dgrad: H=%d W=%d", H, W);
  C4DgP p;
  p.dy = C4Dy{g, z, cmask, Co, H / 2, W / 2};
  p.w = w, p.dx = dx, p.N = N, p.Ci = Ci, p.H = H, p.W = W;
  p.tiles_y = cdiv(cdiv(H, 2), kTH), p.tiles_x = cdiv(cdiv(W, 2), kTW);
  const int64_t tiles = (int64_t)N * 4 * p.tiles_y * p.tiles_x;
  WSL_REQUIRE(tiles < (int64_t)1 << 31, "conv4s2_dgrad: %lld tiles", (long long)tiles);
  switch (pick_co_t(tiles, Ci)) {
    case 16: return launch_c4_dgrad<16>(p, stream);
    case 32: return launch_c4_dgrad<32>(p, stream);
    default: return launch_c4_dgrad<64>(p, stream);
  }
}

extern "C" size_t wsl_conv4s2_wgrad_ws_bytes(int N, int H, int W, int Ci, int Co) {
  if (N <= 0 || H < 2 || W < 2 || Ci <= 0 || Co <= 0) return 0;
  const C4WgPlan g = c4_wgrad_plan(N, H, W, Ci, Co);
  return sizeof(float) * ((size_t)g.nsplit * 16 * Co * Ci + (size_t)g.nsplit * Co) + 256;
}

extern "C" int wsl_conv4s2_wgrad(const float* x, int act, const float* cmask_in, const float* g, const float* z, const float* cmask_out,
                                 float* dw, float* db, int N, int Ci, int H, int W, int Co, void* ws, size_t ws_bytes, void* stream) {
  WSL_REQUIRE(x && g && dw && ws, "conv4s2_wgrad: null argument");
  WSL_REQUIRE(N > 0 && Ci > 0 && Co > 0, "conv4s2_wgrad: bad shape N=%d Ci=%d Co=%d", N, Ci, Co);
  WSL_REQUIRE(H >= 2 && W >= 2, "conv4s2_wgrad: H=%d W=%d", H, W);
  WSL_TRY(check_ws("conv4s2_wgrad", ws_bytes, wsl_conv4s2_wgrad_ws_bytes(N, H, W, Ci, Co)));
  const C4WgPlan pl = c4_wgrad_plan(N, H, W, Ci, Co);
  C4WgP p;
  p.in = C4In{x, nullptr, cmask_in, Ci, 0, act, H, W};
  p.dy = C4Dy{g, z, cmask_out, Co, H / 2, W / 2};
  p.part_dw = static_cast<float*>(ws);
  p.part_db = db ? p.part_dw + (size_t)pl.nsplit * 16 * Co * Ci : nullptr;
  p.N = N, p.items = pl.items, p.nsplit = pl.nsplit, p.co_blocks = pl.co_blocks, p.tiles_y = pl.tiles_y, p.tiles_x = pl.tiles_x;
  if (pl.cb == 16) WSL_TRY((launch_c4_wgrad<16, 4>(p, pl, stream)));
  else WSL_TRY((launch_c4_wgrad<32, 1>(p, pl, stream)));
  WslWgradPending q;
  q.part_dw = p.part_dw, q.part_db = p.part_db, q.dw = dw, q.db = db, q.Co = Co, q.Ci = Ci, q.KK = 16, q.nsplit = pl.nsplit;
  return wsl_wgrad_reduce_batch(&q, 1, stream);
}

extern "C" size_t wsl_dan_head_ws_bytes(int N, int C) {
  if (N <= 0 || C <= 0) return 0;
  return head_ws(N, C).total * sizeof(float);
}

extern "C" int wsl_dan_head_fwd_bwd(const float* z, const int32_t* target, const float* Wc, const float* bc, int pool, float gscale,
                                    float* loss, float* logits, float* dz, float* dW, float* db, int N, int C, int H, int W, void* ws,
                                    size_t ws_bytes, void* stream) {
  WSL_REQUIRE(z && target && Wc && bc && loss && logits && ws, "dan_head: null argument");
  WSL_REQUIRE((dW == nullptr) == (db == nullptr), "dan_head: dW and db come together");
  WSL_REQUIRE(dz || !dW, "dan_head: parameter gradients without dz");
  WSL_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "dan_head: bad shape");
  int wp;
  WSL_TRY(head_shape(H, W, pool, &wp));
  const HeadWs h = head_ws(N, C);
  WSL_TRY(check_ws("dan_head", ws_bytes, h.total * sizeof(float)));
  float* f = static_cast<float*>(ws);
  HeadP p{z, Wc, bc, target, f + h.feat, f + h.dlg, f + h.lossn, logits, N, C, H, W, pool, wp, gscale};
  WSL_TRY(head_fwd(p, loss, stream));
  if (dz) WSL_TRY(head_bwd(p, p.dlg, dz, dW, db, stream));
  return WSL_OK;
}

extern "C" int wsl_adam_step(float* p, const float* grad, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                             int step, float grad_scale, void* stream) {
  WSL_REQUIRE(p && grad && m && v && n > 0, "adam_step: bad args");
  WSL_REQUIRE(step >= 1 && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "adam_step: step %d betas (%g, %g)", step,
              (double)beta1, (double)beta2);
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  const float step_size = (float)((double)lr / bc1), inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
  ProfScope ps(PF_SGD, 0.0, 28.0 * (double)n, stream);
  int64_t blocks = (n + kThreads - 1) / kThreads;
  if (blocks > 2048) blocks = 2048;
  WSL_LAUNCH(adam_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, p, grad, m, v, n, step_size, beta1, beta2, inv_bc2_sqrt, eps,
             grad_scale);
  return check_launch("adam_kernel");
}

// ================================================================================================ C ABI: the network
extern "C" int wsl_dan_num_entries(const WslDanDesc* d) {
  DanPlan P;
  if (dan_layout(d, P)) return -1;
  return dan_entries(P, -1, nullptr);
}
extern "C" int wsl_dan_entry(const WslDanDesc* d, int i, WslNetEntry* out) {
  DanPlan P;
  WSL_TRY(dan_layout(d, P));
  WSL_REQUIRE(out && i >= 0, "dan_entry: bad args");
  const int n = dan_entries(P, i, out);
  WSL_REQUIRE(i < n, "dan_entry: index %d out of %d", i, n);
  return WSL_OK;
}
extern "C" int64_t wsl_dan_param_count(const WslDanDesc* d) {
  DanPlan P;
  return dan_layout(d, P) ? -1 : P.n_param;
}
extern "C" int64_t wsl_dan_buffer_count(const WslDanDesc* d) {
  DanPlan P;
  return dan_layout(d, P) ? -1 : 0;
}
extern "C" size_t wsl_dan_ws_bytes(const WslDanDesc* d) {
  DanPlan P;
  return dan_plan(d, P) ? 0 : P.total_floats * sizeof(float);
}

extern "C" int wsl_dan_forward(const WslDanDesc* d, const float* params, const float* map, const float* feature, const float* const* cmasks,
                               int training, const int32_t* target, float gscale, float* logits, float* loss, void* ws, size_t ws_bytes,
                               void* stream) {
  DanPlan P;
  WSL_TRY(dan_plan(d, P));
  WSL_REQUIRE(params && map && feature && logits && ws, "dan_forward: null argument");
  WSL_REQUIRE(!target || loss, "dan_forward: target without a place for the loss");
  WSL_REQUIRE(!training || (cmasks && cmasks[0] && cmasks[1]), "dan_forward: a training forward needs the two Dropout2d multipliers");
  WSL_TRY(check_ws("dan_forward", ws_bytes, P.total_floats * sizeof(float)));
  float* f = static_cast<float*>(ws);
  const int N = d->N;
  const float* cm2 = training ? cmasks[0] : nullptr;
  const float* cm3 = training ? cmasks[1] : nullptr;
  WSL_TRY(wsl_conv4s2_fwd(map, P.c0.Ci, feature, P.c1.Ci, 0, nullptr, params + P.c0.w, params + P.c1.w, params + P.c0.b, params + P.c1.b,
                          f + P.z[1], N, P.h[0], P.w[0], P.c0.Co, stream));
  WSL_TRY(wsl_conv4s2_fwd(f + P.z[1], P.c2.Ci, nullptr, 0, 0, nullptr, params + P.c2.w, nullptr, params + P.c2.b, nullptr, f + P.z[2], N,
                          P.h[1], P.w[1], P.c2.Co, stream));
  WSL_TRY(wsl_conv4s2_fwd(f + P.z[2], P.c3.Ci, nullptr, 0, 1, cm2, params + P.c3.w, nullptr, params + P.c3.b, nullptr, f + P.z[3], N,
                          P.h[2], P.w[2], P.c3.Co, stream));
  WSL_TRY(wsl_conv4s2_fwd(f + P.z[3], P.c4.Ci, nullptr, 0, 1, cm3, params + P.c4.w, nullptr, params + P.c4.b, nullptr, f + P.z[4], N,
                          P.h[3], P.w[3], P.c4.Co, stream));
  float* hw = f + P.head;
  HeadP p{f + P.z[4], params + P.cls_w, params + P.cls_b, target, hw + P.hw.feat, hw + P.hw.dlg, hw + P.hw.lossn, logits,
          N, P.c4.Co, P.h[4], P.w[4], d->pool, P.wp, gscale};
  return head_fwd(p, loss, stream);
}

extern "C" int wsl_dan_backward(const WslDanDesc* d, const float* params, const float* map, const float* feature, const float* const* cmasks,
                                const float* dlogits, int flags, float* dmap, float* grads, void* ws, size_t ws_bytes, void* stream) {
  DanPlan P;
  WSL_TRY(dan_plan(d, P));
  WSL_REQUIRE(params && map && feature && ws, "dan_backward: null argument");
  const bool want_map = (flags & WSL_DAN_GRAD_MAP) != 0, want_par = (flags & WSL_DAN_GRAD_PARAMS) != 0;
  WSL_REQUIRE((flags & ~3) == 0 && (want_map || want_par), "dan_backward: flags %d", flags);
  WSL_REQUIRE(!want_map || dmap, "dan_backward: gradient to the map asked for without a place for it");
  WSL_REQUIRE(!want_par || grads, "dan_backward: parameter gradients asked for without an arena");
  WSL_TRY(check_ws("dan_backward", ws_bytes, P.total_floats * sizeof(float)));
  float* f = static_cast<float*>(ws);
  const int N = d->N;
  const float* cm2 = cmasks ? cmasks[0] : nullptr;
  const float* cm3 = cmasks ? cmasks[1] : nullptr;
  float *A = f + P.gA, *Bf = f + P.gB, *wg = f + P.wg;
  float* hw = f + P.head;
  HeadP hp{f + P.z[4], params + P.cls_w, params + P.cls_b, nullptr, hw + P.hw.feat, hw + P.hw.dlg, hw + P.hw.lossn, nullptr,
           N, P.c4.Co, P.h[4], P.w[4], d->pool, P.wp, 1.f};
  WSL_TRY(head_bwd(hp, dlogits ? dlogits : hp.dlg, A, want_par ? grads + P.cls_w : nullptr, want_par ? grads + P.cls_b : nullptr, stream));
  // conv4: dy = A (already d/d pre-activation); input leaky(z3) * cm3
  if (want_par)
    WSL_TRY(wsl_conv4s2_wgrad(f + P.z[3], 1, cm3, A, nullptr, nullptr, grads + P.c4.w, grads + P.c4.b, N, P.c4.Ci, P.h[3], P.w[3], P.c4.Co, wg,
                              P.wg_bytes, stream));
  WSL_TRY(wsl_conv4s2_dgrad(A, nullptr, nullptr, params + P.c4.w, Bf, N, P.c4.Ci, P.h[3], P.w[3], P.c4.Co, stream));
  // conv3: dy = Bf * cm3 * leaky'(z3); input leaky(z2) * cm2
  if (want_par)
    WSL_TRY(wsl_conv4s2_wgrad(f + P.z[2], 1, cm2, Bf, f + P.z[3], cm3, grads + P.c3.w, grads + P.c3.b, N, P.c3.Ci, P.h[2], P.w[2], P.c3.Co, wg,
                              P.wg_bytes, stream));
  WSL_TRY(wsl_conv4s2_dgrad(Bf, f + P.z[3], cm3, params + P.c3.w, A, N, P.c3.Ci, P.h[2], P.w[2], P.c3.Co, stream));
  // conv2: dy = A * cm2 * leaky'(z2); input z1 as it is (the reference's 2-D class has no activation after conv0 + conv1)
  if (want_par)
    WSL_TRY(wsl_conv4s2_wgrad(f + P.z[1], 0, nullptr, A, f + P.z[2], cm2, grads + P.c2.w, grads + P.c2.b, N, P.c2.Ci, P.h[1], P.w[1], P.c2.Co,
                              wg, P.wg_bytes, stream));
  WSL_TRY(wsl_conv4s2_dgrad(A, f + P.z[2], cm2, params + P.c2.w, Bf, N, P.c2.Ci, P.h[1], P.w[1], P.c2.Co, stream));
  // conv0 + conv1: dy = Bf; db0 = db1
  if (want_par) {
    WSL_TRY(wsl_conv4s2_wgrad(map, 0, nullptr, Bf, nullptr, nullptr, grads + P.c0.w, grads + P.c0.b, N, P.c0.Ci, P.h[0], P.w[0], P.c0.Co, wg,
                              P.wg_bytes, stream));
    WSL_TRY(wsl_conv4s2_wgrad(feature, 0, nullptr, Bf, nullptr, nullptr, grads + P.c1.w, grads + P.c1.b, N, P.c1.Ci, P.h[0], P.w[0], P.c1.Co,
                              wg, P.wg_bytes, stream));
  }
  if (want_map) WSL_TRY(wsl_conv4s2_dgrad(Bf, nullptr, nullptr, params + P.c0.w, dmap, N, P.c0.Ci, P.h[0], P.w[0], P.c0.Co, stream));
  return WSL_OK;
}
