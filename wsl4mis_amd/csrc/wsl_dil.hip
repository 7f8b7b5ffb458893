// Dilated 3x3 convolutions of PNet2D (ref: networks/pnet.py PNetBlock: Conv2d 3x3, dilation d, padding d) as fp32-MFMA implicit
// GEMMs for gfx950 -- the same operand mapping as conv_mfma_kernel / wgrad_mfma_kernel (wsl_conv.hip), on ROW-PHASE tiles:
//
//   a workgroup owns TH output rows spaced d apart (rows ph + d*(rg*TH + i), i < TH: one row phase ph = row mod d) x TW contiguous
//   columns.  Every tap of that tile reads input rows of the same phase, so its input tile is TH + 2 rows (also d apart) x TW + 2d
//   contiguous columns: the row count of the d = 1 tile whatever d, and the column offset d*(kx-1) of a tap is a contiguous LDS read.
//   (A plain TH x TW tile would need TH + 2d halo rows: 40 rows for TH 8 at d = 16.)
//
//   forward / data-gradient:  M = 16 consecutive pixels of a row, N = 16 output channels, K = 4 input channels of one tap per
//       v_mfma_f32_16x16x4_f32; the loader transform of WslSrc (BatchNorm apply + LeakyReLU, emask, cmask, batch stride) while
//       staging; epilogue: bias, batch-strided store, per-tile (sum, M2) per channel in wsl_bn_stats_finalize's layout.
//       wmode 1 is the data gradient: a dilation-d conv with the flipped, transposed filter and the same padding d.
//   weight-gradient:  M = 16 output channels, N = 16 input channels, K = 4 pixels, nine accumulators per channel pair; partials
//       [nsplit][9][Co][Ci] (+ [nsplit][Co] for the bias) reduced by wsl_wgrad_reduce_batch (wsl_conv.hip) in a fixed order.
//
// Any shape and dilation is correct (halo, ragged tiles and row phases without rows are masked); W % 4 == 0 with a 16-byte aligned
// output only selects float4 stores.  Column layout of a staged row: for d <= TW the TW + 2d contiguous columns (tap kx at LDS column
// offset kx*d); for d > TW three windows of TW columns, one per kx (source columns x0 + (kx-1)*d + t, LDS offset kx*TW) -- so the tile
// never exceeds its d = TW size and every dilation fits the LDS.  In both cases LDS column t holds source column
//     x0 - d + t + seg*(d - kstep),  kstep = min(d, TW), seg = min(t / kstep, 2).
#include <stdio.h>
#include <stdlib.h>

#include "wsl_seq.h"

namespace wsl {

namespace {

struct DilTile {
  WslSrc a, b;
  int H, W, Ci;
};

// source column of LDS column t of a staged row (see the header comment)
__device__ __forceinline__ int dil_col(int x0, int d, int kstep, int t) {
  int seg = t / kstep;
  seg = seg > 2 ? 2 : seg;
  return x0 - d + t + seg * (d - kstep);
}

__device__ __forceinline__ float dil_value(const DilTile& t, int n, int c, int gy, int gx) {
  if (c >= t.Ci || gy < 0 || gy >= t.H || gx < 0 || gx >= t.W) return 0.f;
  const int64_t hw = (int64_t)t.H * t.W;
  const int64_t off = (int64_t)gy * t.W + gx;
  if (c < t.a.C) return src_value(t.a, n, c, n * t.a.bs + c * hw + off, ((int64_t)n * t.a.C + c) * hw + off);
  c -= t.a.C;
  return src_value(t.b, n, c, n * t.b.bs + c * hw + off, ((int64_t)n * t.b.C + c) * hw + off);
}

// tile walk shared by both kernels: item -> (n, phase, row group, column tile); column tiles fastest, then the row groups of
// one phase, so consecutive workgroups share input rows
struct DilWalk {
  int d, rgroups, tiles_x;
  __device__ __forceinline__ void at(int item, int& n, int& ph, int& rg, int& tx) const {
    tx = item % tiles_x;
    item /= tiles_x;
    rg = item % rgroups;
    item /= rgroups;
    ph = item % d;
    n = item / d;
  }
};

static int plane16(int floats) { return ((floats - 16 + 31) / 32) * 32 + 16; }   // >= floats, == 16 (mod 32)
static int plane2(int floats) { return ((floats - 2 + 31) / 32) * 32 + 2; }      // >= floats, == 2 (mod 32)

// ------------------------------------------------------------------------------------------------ forward / data gradient
struct DilP {
  DilTile in;
  DilWalk walk;
  const float* w;
  const float* bias;
  float* y;
  int64_t y_bs;
  int N, Co, wmode, vec_ok, rowp, plane, kstep;
  float* stat_part;
  float* stat_cnt;
};

constexpr int kDilKC = 8;

template <int TH, int TW, int CO_T>
struct DilCfg {
  static constexpr int KC = kDilKC, ROWS = TH + 2;
  static constexpr int CSTR = (CO_T % 32 == 0) ? CO_T + 16 : CO_T;
  static constexpr int SEGS = TW / 16, MT_TOTAL = TH * SEGS, MT = MT_TOTAL / 4, NT = CO_T / 16;
  static constexpr int W_FLOATS = 9 * KC * CSTR, RED_FLOATS = 8 * CO_T;
  static size_t smem(int plane) {
    const int f = KC * plane + W_FLOATS;
    return sizeof(float) * (f > RED_FLOATS ? f : RED_FLOATS);
  }
  static_assert(MT_TOTAL % 4 == 0 && TW % 16 == 0 && CO_T % 16 == 0, "tile shape");
};

template <int TH, int TW, int CO_T>
__global__ __launch_bounds__(256) void dil_conv_kernel(DilP p) {
  using C = DilCfg<TH, TW, CO_T>;
  WSL_DYN_SMEM(smem);
  float* in_t = reinterpret_cast<float*>(smem);
  float* w_t = in_t + C::KC * p.plane;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n, ph, rg, tx_i;
  p.walk.at(blockIdx.x, n, ph, rg, tx_i);
  const int d = p.walk.d, rowp = p.rowp, plane = p.plane, kstep = p.kstep;
  const int co0 = blockIdx.y * CO_T;
  const int r0 = rg * TH;              // first row of the tile inside its phase
  const int x0 = tx_i * TW;
  const int H = p.in.H, W = p.in.W, Ci = p.in.Ci;
  const int tile = C::ROWS * rowp;

  v4f acc[C::MT][C::NT];
#pragma unroll
  for (int i = 0; i < C::MT; ++i)
#pragma unroll
    for (int j = 0; j < C::NT; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
  int abase[C::MT];
#pragma unroll
  for (int i = 0; i < C::MT; ++i) {
    const int mt = wave * C::MT + i;
    abase[i] = (lane >> 4) * plane + (mt / C::SEGS) * rowp + (mt % C::SEGS) * 16 + (lane & 15);
  }
  const int bbase = (lane >> 4) * C::CSTR + (lane & 15);

  for (int c0 = 0; c0 < Ci; c0 += C::KC) {
    // ---- input tile of channels [c0, c0+KC): TH + 2 rows of this phase x TW + 2d columns, transformed, zero padded
    for (int e = tid; e < C::KC * tile; e += kThreads) {
      const int c = e / tile, rem = e - c * tile;
      const int ty = rem / rowp, tx = rem - ty * rowp;
      in_t[c * plane + rem] = dil_value(p.in, n, c0 + c, ph + d * (r0 + ty - 1), dil_col(x0, d, kstep, tx));
    }
    // ---- weights of this channel chunk as w_t[tap][c][co]
    for (int e = tid; e < CO_T * C::KC * 9; e += kThreads) {
      const int co = e / (C::KC * 9), rem = e - co * (C::KC * 9);
      const int c = rem / 9, tap = rem - c * 9;
      const int cog = co0 + co, cg = c0 + c;
      float v = 0.f;
      if (cog < p.Co && cg < Ci)
        v = p.wmode == 0 ? p.w[((int64_t)cog * Ci + cg) * 9 + tap] : p.w[((int64_t)cg * p.Co + cog) * 9 + (8 - tap)];
      w_t[(tap * C::KC + c) * C::CSTR + co] = v;
    }
    __syncthreads();
    const int ngroups = (Ci - c0 >= C::KC) ? C::KC / 4 : (Ci - c0 + 3) / 4;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int toff = (tap / 3) * rowp + (tap % 3) * kstep;
#pragma unroll
      for (int cg = 0; cg < C::KC / 4; ++cg) {
        if (cg < ngroups) {
          float bv[C::NT];
#pragma unroll
          for (int j = 0; j < C::NT; ++j) bv[j] = w_t[(tap * C::KC + cg * 4) * C::CSTR + j * 16 + bbase];
#pragma unroll
          for (int i = 0; i < C::MT; ++i) {
            const float av = in_t[cg * 4 * plane + toff + abase[i]];
#pragma unroll
            for (int j = 0; j < C::NT; ++j) acc[i][j] = WSL_MFMA16(av, bv[j], acc[i][j]);
          }
        }
      }
    }
    __syncthreads();
  }

  // ---- epilogue: bias, store, BatchNorm partial statistics of the tile's valid pixels
  const int64_t HW = (int64_t)H * W;
  float bsum[C::NT];
#pragma unroll
  for (int j = 0; j < C::NT; ++j) {
    const int co = co0 + j * 16 + (lane & 15);
    const float bias = (p.bias && co < p.Co) ? p.bias[co] : 0.f;
    bsum[j] = 0.f;
#pragma unroll
    for (int i = 0; i < C::MT; ++i) {
      const int mt = wave * C::MT + i;
      const int gy = ph + d * (r0 + mt / C::SEGS), gx = x0 + (mt % C::SEGS) * 16 + (lane >> 4) * 4;
      v4f v = acc[i][j];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] += bias;
      acc[i][j] = v;
      if (co < p.Co && gy < H) {
        float* dst = p.y + n * p.y_bs + co * HW + (int64_t)gy * W + gx;
        if (p.vec_ok && gx + 3 < W) {
          *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (gx + r < W) dst[r] = v[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (gx + r < W) bsum[j] += v[r];
      }
    }
  }
  if (p.stat_part) {  // uniform branch
    int vh = 0;   // rows of this tile inside the image: rows ph + d*(r0 + i) < H
    if (ph < H) {
      const int rows_ph = (H - ph + d - 1) / d;
      vh = rows_ph - r0;
      vh = vh < 0 ? 0 : (vh > TH ? TH : vh);
    }
    const int vw = (W - x0 < TW) ? W - x0 : TW;
    const float cnt = (float)(vh * vw);
    auto sqdev = [=](int j, float mean_q) __attribute__((always_inline)) {
      const int co = co0 + j * 16 + (lane & 15);
      const float mean_b = cnt > 0.f ? mean_q : 0.f;   // a tile past the last row of its phase has no valid pixel: sum / cnt is 0 / 0 there
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < C::MT; ++i) {
        const int mt = wave * C::MT + i;
        const int gy = ph + d * (r0 + mt / C::SEGS), gx = x0 + (mt % C::SEGS) * 16 + (lane >> 4) * 4;
        if (co < p.Co && gy < H) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (gx + r < W) {
              const float df = acc[i][j][r] - mean_b;
              q = fmaf(df, df, q);
            }
        }
      }
      return q;
    };
    __syncthreads();   // (the helper's scratch aliases the staging tile: every wave is past its last read)
    // [Co][nblk][2]: one slot per tile
    bn_stat_store<C::NT, CO_T>(bsum, cnt, sqdev, in_t, co0, p.Co, (int)blockIdx.x, (int)gridDim.x, 1, p.stat_part, p.stat_cnt, blockIdx.y == 0);
  }
}

struct DilPlan {
  int th, tw, co_t, rgroups, tiles_x, rowp, plane, kstep;
  int64_t tiles;
};

static DilPlan dil_plan(int N, int H, int W, int Co, int d) {
  DilPlan f;
  f.th = 8;
  if (Co <= 16) {
    f.co_t = 16;
    f.tw = W >= 64 ? 64 : (W >= 32 ? 32 : 16);
  } else {
    f.tw = W >= 32 ? 32 : 16;
    f.co_t = Co <= 32 ? 32 : 64;
  }
  f.rgroups = cdiv(cdiv(H, d), f.th);
  f.tiles_x = cdiv(W, f.tw);
  f.tiles = (int64_t)N * d * f.rgroups * f.tiles_x;
  if (Co > 16) {
    const int64_t enough = 2 * (int64_t)device_cu_count();
    while (f.co_t > 16 && f.tiles * cdiv(Co, f.co_t) < enough) f.co_t >>= 1;
  }
  f.kstep = d < f.tw ? d : f.tw;
  f.rowp = f.tw + 2 * f.kstep;
  f.plane = plane16((f.th + 2) * f.rowp);
  return f;
}

constexpr size_t kDilMaxSmem = 160 * 1024;   // LDS of one gfx950 CU

template <int TH, int TW, int CO_T>
static int launch_dil(DilP& p, const DilPlan& f, void* stream) {
  using C = DilCfg<TH, TW, CO_T>;
  auto kern = dil_conv_kernel<TH, TW, CO_T>;
  const size_t smem = C::smem(f.plane);
  if (smem > kDilMaxSmem) {
    set_error("conv2d_dil: dilation %d needs %zu bytes of LDS per workgroup (%zu available)", p.walk.d, smem, kDilMaxSmem);
    return WSL_EUNSUPPORTED;
  }
  static bool attr_done = false;
  if (!attr_done) {
    (void)WSL_SET_MAX_DYN_SMEM(kern, kDilMaxSmem);
    attr_done = true;
  }
  dim3 grid((unsigned)f.tiles, cdiv(p.Co, CO_T));
  const double px = (double)p.N * p.in.H * p.in.W;
  void* tok = prof_begin(p.wmode ? PF_CONV_DGRAD : PF_CONV_FWD, 2.0 * px * p.Co * p.in.Ci * 9, 4.0 * px * (p.Co + p.in.Ci), stream);
  WSL_LAUNCH(kern, grid, dim3(kThreads), smem, stream, p);
  prof_end(tok, stream);
  return check_launch("dil_conv_kernel");
}

static int dispatch_dil(DilP& p, const DilPlan& f, void* stream) {
#define WSL_CASE(TW_, CO_) \
  if (f.tw == TW_ && f.co_t == CO_) return launch_dil<8, TW_, CO_>(p, f, stream);
  WSL_CASE(64, 16)
  WSL_CASE(32, 16)
  WSL_CASE(32, 32)
  WSL_CASE(32, 64)
  WSL_CASE(16, 16)
  WSL_CASE(16, 32)
  WSL_CASE(16, 64)
#undef WSL_CASE
  set_error("conv2d_dil: no kernel for tile %dx%d co_t %d", f.th, f.tw, f.co_t);
  return WSL_EUNSUPPORTED;
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct DilWgP {
  DilTile in;
  DilWalk walk;
  const float* dy;
  int64_t dy_bs;
  float* part_dw;   // [nsplit][9][Co][Ci]
  float* part_db;   // [nsplit][Co]
  int N, Co, items, nsplit, co_blocks, rowp, pla, kstep;
};

template <int TH, int TW, int CB, int IB, int WK>
struct DilWgCfg {
  static constexpr int ROWS = TH + 2, S = TH * TW;
  static constexpr int PLD = ((S - 2 + 31) / 32) * 32 + 2;   // == 2 (mod 32)
  static constexpr int CBT = CB / 16, IBT = IB / 16, PAIRS = CBT * IBT, WP = 4 / WK, PP = PAIRS / WP;
  static constexpr int DY_FLOATS = CB * PLD;
  static constexpr int RED_FLOATS = (WK > 1) ? 4 * 64 * (PP * 10 * 4) : 0;
  static size_t smem(int pla) {
    const int f = DY_FLOATS + IB * pla;
    return sizeof(float) * (f > RED_FLOATS ? f : RED_FLOATS);
  }
  static_assert(PAIRS % WP == 0 && TH % WK == 0 && TW % 4 == 0, "wgrad tile shape");
};

template <int TH, int TW, int CB, int IB, int WK>
__global__ __launch_bounds__(256) void dil_wgrad_kernel(DilWgP p) {
  using C = DilWgCfg<TH, TW, CB, IB, WK>;
  WSL_DYN_SMEM(smem);
  float* dy_t = reinterpret_cast<float*>(smem);
  float* a_t = dy_t + C::DY_FLOATS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cb = blockIdx.x % p.co_blocks, ib = blockIdx.x / p.co_blocks, split = blockIdx.y;
  const int co0 = cb * CB, ci0 = ib * IB;
  const int wp = wave % C::WP, wk = wave / C::WP;
  const int H = p.in.H, W = p.in.W, Ci = p.in.Ci, d = p.walk.d, rowp = p.rowp, pla = p.pla, kstep = p.kstep;
  const int atile = C::ROWS * rowp;
  const int64_t HW = (int64_t)H * W;

  v4f acc[C::PP][9];
  v4f accb[C::PP];
#pragma unroll
  for (int j = 0; j < C::PP; ++j) {
    accb[j] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[j][t] = v4f{0.f, 0.f, 0.f, 0.f};
  }
  const bool want_db = (ib == 0) && (p.part_db != nullptr);
  const int it0 = (int)((int64_t)split * p.items / p.nsplit), it1 = (int)((int64_t)(split + 1) * p.items / p.nsplit);
  for (int item = it0; item < it1; ++item) {
    int n, ph, rg, tx_i;
    p.walk.at(item, n, ph, rg, tx_i);
    const int r0 = rg * TH, x0 = tx_i * TW;
    // ---- dy tile [CB][TH*TW] of this phase (zero outside image / channel range)
    for (int e = tid; e < CB * C::S; e += kThreads) {
      const int c = e / C::S, rem = e - c * C::S;
      const int ty = rem / TW, tx = rem - ty * TW;
      const int gy = ph + d * (r0 + ty), gx = x0 + tx, co = co0 + c;
      float v = 0.f;
      if (co < p.Co && gy < H && gx < W) v = p.dy[n * p.dy_bs + co * HW + (int64_t)gy * W + gx];
      dy_t[c * C::PLD + rem] = v;
    }
    // ---- input tile [IB][TH+2 rows of the phase x TW+2d columns], transformed
    for (int e = tid; e < IB * atile; e += kThreads) {
      const int c = e / atile, rem = e - c * atile;
      const int ty = rem / rowp, tx = rem - ty * rowp;
      a_t[c * pla + rem] = dil_value(p.in, n, ci0 + c, ph + d * (r0 + ty - 1), dil_col(x0, d, kstep, tx));
    }
    __syncthreads();
    constexpr int RW = TH / WK;
#pragma unroll 1
    for (int r = wk * RW; r < wk * RW + RW; ++r) {
#pragma unroll 2
      for (int x4 = 0; x4 < TW / 4; ++x4) {
        const int pix = r * TW + x4 * 4 + (lane >> 4);
        const int apix = r * rowp + x4 * 4 + (lane >> 4);
#pragma unroll
        for (int j = 0; j < C::PP; ++j) {
          const int pr = wp * C::PP + j, cot = pr / C::IBT, cit = pr % C::IBT;
          const float av = dy_t[(cot * 16 + (lane & 15)) * C::PLD + pix];
          if (want_db && cit == 0) accb[j] = WSL_MFMA16(av, 1.0f, accb[j]);
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            const float bv = a_t[(cit * 16 + (lane & 15)) * pla + apix + (t / 3) * rowp + (t % 3) * kstep];
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
    constexpr int PER = C::PP * 10 * 4;
    float* mine = red + (wave * 64 + lane) * PER;
#pragma unroll
    for (int j = 0; j < C::PP; ++j) {
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) mine[(j * 10 + t) * 4 + r] = acc[j][t][r];
#pragma unroll
      for (int r = 0; r < 4; ++r) mine[(j * 10 + 9) * 4 + r] = accb[j][r];
    }
    __syncthreads();
    if (wk == 0) {
#pragma unroll
      for (int j = 0; j < C::PP; ++j) {
#pragma unroll
        for (int t = 0; t <= 9; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float s = 0.f;
            for (int k = 0; k < WK; ++k) s += red[((k * C::WP + wp) * 64 + lane) * PER + (j * 10 + t) * 4 + r];
            if (t < 9) acc[j][t][r] = s; else accb[j][r] = s;
          }
      }
    }
  }
  if (wk == 0) {
#pragma unroll
    for (int j = 0; j < C::PP; ++j) {
      const int pr = wp * C::PP + j, cot = pr / C::IBT, cit = pr % C::IBT;
      const int ci = ci0 + cit * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + cot * 16 + (lane >> 4) * 4 + r;
        if (co < p.Co && ci < Ci) {
#pragma unroll
          for (int t = 0; t < 9; ++t) p.part_dw[(((int64_t)split * 9 + t) * p.Co + co) * Ci + ci] = acc[j][t][r];
        }
        if (want_db && cit == 0 && (lane & 15) == 0 && co < p.Co) p.part_db[(int64_t)split * p.Co + co] = accb[j][r];
      }
    }
  }
}

struct DilWgPlan {
  int th, tw, cb, wk, nsplit, items, rgroups, tiles_x, co_blocks, ci_blocks, rowp, pla, kstep;
};

static DilWgPlan dil_wgrad_plan(int N, int H, int W, int Ci, int Co, int d) {
  DilWgPlan g;
  if (Co <= 16 || Ci <= 16) {
    g.cb = 16, g.wk = 4, g.th = 8;
    g.tw = W >= 64 ? 64 : (W >= 32 ? 32 : 16);
  } else {
    g.cb = 32, g.wk = 1, g.th = 8;
    g.tw = W >= 32 ? 32 : 16;
  }
  g.rgroups = cdiv(cdiv(H, d), g.th);
  g.tiles_x = cdiv(W, g.tw);
  g.items = N * d * g.rgroups * g.tiles_x;
  g.co_blocks = cdiv(Co, g.cb), g.ci_blocks = cdiv(Ci, g.cb);
  // 768 pixel splits of the whole launch, the direct kernel's setting.  (Not a residency count: at CB 32 the staged tiles take
  // 76.5 KiB of LDS at d = 1 and 80.5 / 84.5 / 92.5 / 112.5 / 152.5 KiB at d = 2 / 4 / 8 / 16 / >= 32, so from d = 2 on one workgroup
  // fits a 160 KiB CU and the 768 workgroups run as three rounds over the 256 CUs -- DESIGN.md section 8.)
  int want = (forced_wgrad_wgs() > 0 ? forced_wgrad_wgs() : 768) / (g.co_blocks * g.ci_blocks);
  if (want < 1) want = 1;
  g.nsplit = g.items < want ? g.items : want;
  g.kstep = d < g.tw ? d : g.tw;
  g.rowp = g.tw + 2 * g.kstep;
  g.pla = plane2((g.th + 2) * g.rowp);
  return g;
}

template <int TH, int TW, int CB, int WK>
static int launch_dil_wgrad(DilWgP& p, const DilWgPlan& g, void* stream) {
  using C = DilWgCfg<TH, TW, CB, CB, WK>;
  auto kern = dil_wgrad_kernel<TH, TW, CB, CB, WK>;
  const size_t smem = C::smem(g.pla);
  if (smem > kDilMaxSmem) {
    set_error("conv2d_dil_wgrad: dilation %d needs %zu bytes of LDS per workgroup (%zu available)", p.walk.d, smem, kDilMaxSmem);
    return WSL_EUNSUPPORTED;
  }
  static bool attr_done = false;
  if (!attr_done) {
    (void)WSL_SET_MAX_DYN_SMEM(kern, kDilMaxSmem);
    attr_done = true;
  }
  dim3 grid(g.co_blocks * g.ci_blocks, g.nsplit);
  const double px = (double)p.N * p.in.H * p.in.W;
  void* tok = prof_begin(PF_WGRAD_DIRECT, 2.0 * px * p.Co * p.in.Ci * 9, 4.0 * px * (p.Co + p.in.Ci), stream);
  WSL_LAUNCH(kern, grid, dim3(kThreads), smem, stream, p);
  prof_end(tok, stream);
  return check_launch("dil_wgrad_kernel");
}

static int dispatch_dil_wgrad(DilWgP& p, const DilWgPlan& g, void* stream) {
#define WSL_CASE(TW_, CB_, WK_) \
  if (g.tw == TW_ && g.cb == CB_) return launch_dil_wgrad<8, TW_, CB_, WK_>(p, g, stream);
  WSL_CASE(64, 16, 4)
  WSL_CASE(32, 16, 4)
  WSL_CASE(16, 16, 4)
  WSL_CASE(32, 32, 1)
  WSL_CASE(16, 32, 1)
#undef WSL_CASE
  set_error("conv2d_dil_wgrad: no kernel for tile %dx%d cb %d", g.th, g.tw, g.cb);
  return WSL_EUNSUPPORTED;
}

static int dil_check_src(const WslSrc* s, int HW, const char* who) {
  WSL_REQUIRE(s->x != nullptr && s->C > 0, "%s: source has no data", who);
  WSL_REQUIRE(s->bs >= (int64_t)s->C * HW, "%s: batch stride %lld < C*H*W", who, (long long)s->bs);
  WSL_REQUIRE((s->scale == nullptr) == (s->shift == nullptr), "%s: scale and shift must come together", who);
  return WSL_OK;
}

static int dil_tile(DilTile& t, const WslSrc* a, const WslSrc* b, int H, int W, const char* who) {
  WSL_REQUIRE(a != nullptr, "%s: null source", who);
  if (int rc = dil_check_src(a, H * W, who)) return rc;
  t.a = *a;
  if (b && b->C > 0) {
    if (int rc = dil_check_src(b, H * W, who)) return rc;
    t.b = *b;
  } else {
    t.b = WslSrc{};
  }
  t.H = H, t.W = W, t.Ci = a->C + t.b.C;
  return WSL_OK;
}

}  // namespace
}  // namespace wsl

using namespace wsl;

extern "C" int wsl_conv2d_dil_stat_blocks(int N, int H, int W, int Ci, int Co, int dil) {
  (void)Ci;
  if (N <= 0 || H <= 0 || W <= 0 || Co <= 0 || dil <= 0) return 0;
  return (int)dil_plan(N, H, W, Co, dil).tiles;
}

extern "C" int wsl_conv2d_dil_fwd(const WslSrc* a, const WslSrc* b, const float* w, const float* bias, float* y, int64_t y_bs,
                                  int N, int H, int W, int Co, int ks, int dil, int wmode, float* stat_part, float* stat_cnt,
                                  void* stream) {
  WSL_REQUIRE(w && y, "conv2d_dil_fwd: null argument");
  WSL_REQUIRE(N > 0 && H > 0 && W > 0 && Co > 0, "conv2d_dil_fwd: bad shape N=%d H=%d W=%d Co=%d", N, H, W, Co);
  WSL_REQUIRE(ks == 3, "conv2d_dil_fwd: kernel size %d (the dilated kernels are 3x3)", ks);
  WSL_REQUIRE(dil >= 1, "conv2d_dil_fwd: dilation %d", dil);
  WSL_REQUIRE(wmode == 0 || wmode == 1, "conv2d_dil_fwd: wmode %d (0 forward, 1 data gradient)", wmode);
  WSL_REQUIRE((stat_part == nullptr) == (stat_cnt == nullptr), "conv2d_dil_fwd: stat_part and stat_cnt come together");
  WSL_REQUIRE(y_bs >= (int64_t)Co * H * W, "conv2d_dil_fwd: y batch stride too small");
  DilP p;
  WSL_TRY(dil_tile(p.in, a, b, H, W, "conv2d_dil_fwd"));
  const DilPlan f = dil_plan(N, H, W, Co, dil);
  WSL_REQUIRE(f.tiles < (int64_t)1 << 31, "conv2d_dil_fwd: %lld tiles", (long long)f.tiles);
  p.walk.d = dil, p.walk.rgroups = f.rgroups, p.walk.tiles_x = f.tiles_x;
  p.w = w, p.bias = bias, p.y = y, p.y_bs = y_bs, p.N = N, p.Co = Co, p.wmode = wmode;
  p.vec_ok = (W % 4 == 0) && (y_bs % 4 == 0) && ((reinterpret_cast<uintptr_t>(y) & 15) == 0);
  p.rowp = f.rowp, p.plane = f.plane, p.kstep = f.kstep;
  p.stat_part = stat_part, p.stat_cnt = stat_cnt;
  return dispatch_dil(p, f, stream);
}

extern "C" size_t wsl_conv2d_dil_wgrad_ws_bytes(int N, int H, int W, int Ci, int Co, int ks, int dil) {
  if (N <= 0 || H <= 0 || W <= 0 || Ci <= 0 || Co <= 0 || ks != 3 || dil <= 0) return 0;
  const DilWgPlan g = dil_wgrad_plan(N, H, W, Ci, Co, dil);
  return sizeof(float) * ((size_t)g.nsplit * 9 * Co * Ci + (size_t)g.nsplit * Co) + 256;
}

extern "C" int wsl_conv2d_dil_wgrad_partial(const WslSrc* a, const WslSrc* b, const float* dy, int64_t dy_bs, float* dw, float* db,
                                            int N, int H, int W, int Co, int ks, int dil, void* ws, size_t ws_bytes,
                                            WslWgradPending* pending, void* stream) {
  WSL_REQUIRE(dy && dw && ws && pending, "conv2d_dil_wgrad: null argument");
  WSL_REQUIRE(N > 0 && H > 0 && W > 0 && Co > 0, "conv2d_dil_wgrad: bad shape");
  WSL_REQUIRE(ks == 3, "conv2d_dil_wgrad: kernel size %d (the dilated kernels are 3x3)", ks);
  WSL_REQUIRE(dil >= 1, "conv2d_dil_wgrad: dilation %d", dil);
  WSL_REQUIRE(dy_bs >= (int64_t)Co * H * W, "conv2d_dil_wgrad: dy batch stride too small");
  DilWgP p;
  WSL_TRY(dil_tile(p.in, a, b, H, W, "conv2d_dil_wgrad"));
  const int Ci = p.in.Ci;
  const size_t need = wsl_conv2d_dil_wgrad_ws_bytes(N, H, W, Ci, Co, ks, dil);
  if (ws_bytes < need) {
    set_error("conv2d_dil_wgrad: workspace %zu < %zu bytes", ws_bytes, need);
    return WSL_EWORKSPACE;
  }
  const DilWgPlan g = dil_wgrad_plan(N, H, W, Ci, Co, dil);
  p.walk.d = dil, p.walk.rgroups = g.rgroups, p.walk.tiles_x = g.tiles_x;
  p.dy = dy, p.dy_bs = dy_bs, p.N = N, p.Co = Co;
  p.items = g.items, p.nsplit = g.nsplit, p.co_blocks = g.co_blocks, p.rowp = g.rowp, p.pla = g.pla, p.kstep = g.kstep;
  p.part_dw = reinterpret_cast<float*>(ws);
  p.part_db = db ? p.part_dw + (size_t)g.nsplit * 9 * Co * Ci : nullptr;
  WSL_TRY(dispatch_dil_wgrad(p, g, stream));
  pending->part_dw = p.part_dw, pending->part_db = p.part_db, pending->dw = dw, pending->db = db;
  pending->Co = Co, pending->Ci = Ci, pending->KK = 9, pending->nsplit = g.nsplit;
  return WSL_OK;
}

extern "C" int wsl_conv2d_dil_wgrad(const WslSrc* a, const WslSrc* b, const float* dy, int64_t dy_bs, float* dw, float* db, int N,
                                    int H, int W, int Co, int ks, int dil, void* ws, size_t ws_bytes, void* stream) {
  WslWgradPending pend;
  WSL_TRY(wsl_conv2d_dil_wgrad_partial(a, b, dy, dy_bs, dw, db, N, H, W, Co, ks, dil, ws, ws_bytes, &pend, stream));
  return wsl_wgrad_reduce_batch(&pend, 1, stream);
}
