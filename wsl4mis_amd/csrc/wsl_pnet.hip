// PNet2D forward + backward over flat arenas (ref: networks/pnet.py PNet2D / PNetBlock / ConcatBlock / OutPutBlock; factory
// networks/net_factory.py: PNet2D(in_chns, class_num, 64, [1, 2, 4, 8, 16])).  Host-side sequencing of this library's kernels on the
// caller's stream, as wsl_net.hip does for the UNet; nothing here allocates or synchronises.
//
// The concat is free: block k's conv2 writes its raw output into channel slice k of one [N,5F,H,W] buffer (y_bs = 5F*H*W), block
// k+1's conv1 reads that slice through the loader with block k's in2 scale / shift, and catblock.conv1 reads all 5F channels as one
// source whose BatchNorm tables are the five in2 tables laid end to end.  No BatchNorm / LeakyReLU output is materialised: the
// LeakyReLU-only sites (catblock and out.conv1 outputs) go through the loader with unit scale and zero shift, the two Dropout2d sites
// as its channel multiplier.
#include "wsl_seq.h"

namespace wsl {
namespace {

struct PBlock { ConvRef c1, c2; BnRef b1, b2; int dil; };

struct PPlan {
  WslPNetDesc d;
  int F;
  int64_t HW, NHW;
  PBlock blk[5];
  ConvRef cb1, cb2, o1, o2;
  int64_t n_param, n_block_param, n_buf;
  // workspace (float offsets)
  size_t cat, y1[5], st1[5], st2, zc1, zc2, zo1, unit, stat_part, stat_cnt, bufA, bufB, ycopy, bn_ws, wg_ws;
  size_t bn_bytes, wg_bytes[2], total_floats;
};

static int make_plan(const WslPNetDesc* d, PPlan& P) {
  WSL_REQUIRE(d, "pnet: null descriptor");
  WSL_REQUIRE(d->in_chns > 0 && d->n_class > 0 && d->n_class <= 8 && d->num_filters > 0, "pnet: bad channel counts");
  for (int k = 0; k < 5; ++k) WSL_REQUIRE(d->ratios[k] >= 1, "pnet: ratio %d of block %d", d->ratios[k], k + 1);
  WSL_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0, "pnet: N=%d H=%d W=%d", d->N, d->H, d->W);
  P.d = *d;
  const int F = d->num_filters;
  P.F = F;
  P.HW = (int64_t)d->H * d->W, P.NHW = (int64_t)d->N * P.HW;
  // parameters() order: per block conv1, conv2, in1, in2 (registration order of PNetBlock), then catblock, then out
  int64_t po = 0, bo = 0, nbn = 0;
  for (int k = 0; k < 5; ++k) {
    PBlock& b = P.blk[k];
    b.dil = d->ratios[k];
    plan_conv(b.c1, k == 0 ? d->in_chns : F, F, 3, po);
    plan_conv(b.c2, F, F, 3, po);
    plan_bn(b.b1, F, po, bo, nbn);   // (num_batches_tracked slots 2k, 2k + 1)
    plan_bn(b.b2, F, po, bo, nbn);
  }
  P.n_block_param = po;
  plan_conv(P.cb1, 5 * F, 5 * F, 1, po);
  plan_conv(P.cb2, 5 * F, 2 * F, 1, po);
  plan_conv(P.o1, 2 * F, F, 1, po);
  plan_conv(P.o2, F, d->n_class, 1, po);
  P.n_param = po, P.n_buf = bo;

  const int N = d->N, H = d->H, W = d->W;
  const size_t u = (size_t)P.NHW * F;   // one [N,F,H,W] tensor
  Bump B;
  P.cat = B.take(5 * u);
  for (int k = 0; k < 5; ++k) P.y1[k] = B.take(u);
  for (int k = 0; k < 5; ++k) P.st1[k] = B.take(4 * (size_t)F);
  P.st2 = B.take(20 * (size_t)F);   // mean[5F] | invstd[5F] | scale[5F] | shift[5F]: block k's table at k*F of each
  P.zc1 = B.take(5 * u);
  P.zc2 = B.take(2 * u);
  P.zo1 = B.take(u);
  P.unit = B.take(10 * (size_t)F);  // ones[5F] | zeros[5F]
  int nblk = 1;
  for (int k = 0; k < 5; ++k) {
    const int nb = wsl_conv2d_dil_stat_blocks(N, H, W, F, F, P.blk[k].dil);
    nblk = nb > nblk ? nb : nblk;
  }
  P.stat_part = B.take((size_t)F * nblk * 2);
  P.stat_cnt = B.take((size_t)nblk);
  P.bufA = B.take(5 * u);
  P.bufB = B.take(5 * u);
  P.ycopy = B.take(u);
  P.bn_bytes = (wsl_bnact_bwd_ws_bytes(N, F, H, W) + 255) & ~(size_t)255;
  P.bn_ws = B.take(P.bn_bytes / sizeof(float));
  // weight-gradient partials of every layer of a phase (their second stages run as one launch per phase)
  auto r256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
  P.wg_bytes[0] = r256(wsl_conv2d_wgrad_ws_bytes(N, H, W, P.cb1.Ci, P.cb1.Co, 1)) + r256(wsl_conv2d_wgrad_ws_bytes(N, H, W, P.cb2.Ci, P.cb2.Co, 1)) +
                  r256(wsl_conv2d_wgrad_ws_bytes(N, H, W, P.o1.Ci, P.o1.Co, 1)) + r256(wsl_conv2d_wgrad_ws_bytes(N, H, W, P.o2.Ci, P.o2.Co, 1));
  P.wg_bytes[1] = 0;
  for (int k = 0; k < 5; ++k) {
    const PBlock& b = P.blk[k];
    P.wg_bytes[1] += r256(wsl_conv2d_dil_wgrad_ws_bytes(N, H, W, b.c1.Ci, F, 3, b.dil)) + r256(wsl_conv2d_dil_wgrad_ws_bytes(N, H, W, F, F, 3, b.dil));
  }
  const size_t wgb = P.wg_bytes[0] > P.wg_bytes[1] ? P.wg_bytes[0] : P.wg_bytes[1];
  P.wg_ws = B.take(wgb / sizeof(float) + 64);
  P.total_floats = B.off;
  return WSL_OK;
}

// ------------------------------------------------------------------------------------------------ elementwise kernels
__global__ __launch_bounds__(256) void pnet_unit_kernel(float* t, int n) {   // ones[n] | zeros[n]
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < 2 * n; i += gridDim.x * kThreads) t[i] = i < n ? 1.f : 0.f;
}

// backward of out = cmask[n,c] * leaky(z) given g = dL/d(out), in place: g <- (g * cmask) * leaky'(z)   (dense [N,C,HW])
__global__ __launch_bounds__(256) void pnet_leaky_bwd_kernel(float* g, const float* z, const float* cmask, int C, int64_t HW, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    float t = g[i];
    if (cmask) t *= cmask[i / HW];
    g[i] = z[i] > 0.f ? t : t * WSL_LEAKY_SLOPE;
  }
}

// g = ga (batch stride ga_bs) [+ gb (dense)], ycopy = y (batch stride y_bs): the gradient reaching a block output from the concat and
// from the next block, and a dense copy of the block's raw conv2 output (its slice of the concat) for the BatchNorm backward
__global__ __launch_bounds__(256) void pnet_gather_kernel(const float* ga, int64_t ga_bs, const float* gb, float* g, const float* y,
                                                          int64_t y_bs, float* ycopy, int64_t CHW, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t n = i / CHW, r = i - n * CHW;
    float v = ga[n * ga_bs + r];
    if (gb) v += gb[i];
    g[i] = v;
    ycopy[i] = y[n * y_bs + r];
  }
}

static unsigned ew_grid(int64_t total) {
  int64_t b = (total + kThreads - 1) / kThreads;
  const int64_t cap = 16 * (int64_t)device_cu_count();
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ------------------------------------------------------------------------------------------------ sequencing
struct PCtx {
  const PPlan& P;
  const float* params;
  float* buffers;
  int64_t* nbt;
  float* grads;
  float* ws;
  void* stream;
  int training;
  WgBatch* wb;
};

// (no element mask anywhere in this network: its two dropout sites are Dropout2d, the loader's channel multiplier)
// virtual tensor leaky(z) [* cmask] of a dense [N,C,H,W] tensor
static WslSrc leaky_src(const PCtx& c, size_t z, int C, const float* cmask) {
  const int F5 = 5 * c.P.F;
  return act_src(c.ws + z, C, (int64_t)C * c.P.HW, c.ws + c.P.unit, c.ws + c.P.unit + F5, nullptr, 1.f, cmask);
}
// block k's output f_k = leaky(in2(y2_k)): slice k of the concat buffer
static WslSrc block_out_src(const PCtx& c, int k) {
  const PPlan& P = c.P;
  const int F = P.F;
  return act_src(c.ws + P.cat + (size_t)k * F * P.HW, F, 5 * F * P.HW, c.ws + P.st2 + 10 * F + k * F, c.ws + P.st2 + 15 * F + k * F,
                 nullptr, 1.f, nullptr);
}
static WslSrc block_mid_src(const PCtx& c, int k) {
  const PPlan& P = c.P;
  const int F = P.F;
  return act_src(c.ws + P.y1[k], F, F * P.HW, c.ws + P.st1[k] + 2 * F, c.ws + P.st1[k] + 3 * F, nullptr, 1.f, nullptr);
}

static int bn_fwd(const PCtx& c, const BnRef& bn, int nblk, float* mean, float* invstd, float* scale, float* shift) {
  return wsl::bn_fwd(c.training, c.ws + c.P.stat_part, c.ws + c.P.stat_cnt, nblk, bn, c.params, c.buffers, c.nbt, mean, invstd, scale, shift,
                c.stream);
}

static int pnet_fwd(const PCtx& c, const float* x, const float* const* cmasks, float* logits) {
  const PPlan& P = c.P;
  const int N = P.d.N, H = P.d.H, W = P.d.W, F = P.F;
  const int64_t HW = P.HW;
  WSL_LAUNCH(pnet_unit_kernel, dim3(cdiv(10 * F, kThreads)), dim3(kThreads), 0, c.stream, c.ws + P.unit, 5 * F);
  WSL_TRY(check_launch("pnet_unit_kernel"));
  float* stp = c.training ? c.ws + P.stat_part : nullptr;
  float* stc = c.training ? c.ws + P.stat_cnt : nullptr;
  for (int k = 0; k < 5; ++k) {
    const PBlock& b = P.blk[k];
    const WslSrc in = k == 0 ? raw_src(x, P.d.in_chns, (int64_t)P.d.in_chns * HW) : block_out_src(c, k - 1);
    const int nblk = wsl_conv2d_dil_stat_blocks(N, H, W, F, F, b.dil);
    float* s1 = c.ws + P.st1[k];
    WSL_TRY(wsl_conv2d_dil_fwd(&in, nullptr, c.params + b.c1.w, c.params + b.c1.b, c.ws + P.y1[k], F * HW, N, H, W, F, 3, b.dil, 0, stp,
                               stc, c.stream));
    WSL_TRY(bn_fwd(c, b.b1, nblk, s1, s1 + F, s1 + 2 * F, s1 + 3 * F));
    const WslSrc mid = block_mid_src(c, k);
    WSL_TRY(wsl_conv2d_dil_fwd(&mid, nullptr, c.params + b.c2.w, c.params + b.c2.b, c.ws + P.cat + (size_t)k * F * HW, 5 * F * HW, N, H,
                               W, F, 3, b.dil, 0, stp, stc, c.stream));
    float* s2 = c.ws + P.st2;
    WSL_TRY(bn_fwd(c, b.b2, nblk, s2 + k * F, s2 + 5 * F + k * F, s2 + 10 * F + k * F, s2 + 15 * F + k * F));
  }
  const float* cm1 = c.training && cmasks ? cmasks[0] : nullptr;
  const float* cm2 = c.training && cmasks ? cmasks[1] : nullptr;
  const WslSrc cat = act_src(c.ws + P.cat, 5 * F, 5 * F * HW, c.ws + P.st2 + 10 * F, c.ws + P.st2 + 15 * F, nullptr, 1.f, nullptr);
  WSL_TRY(wsl_conv2d_fwd(&cat, nullptr, c.params + P.cb1.w, c.params + P.cb1.b, c.ws + P.zc1, 5 * F * HW, N, H, W, 5 * F, 1, 0, nullptr,
                         nullptr, c.stream));
  const WslSrc a1 = leaky_src(c, P.zc1, 5 * F, nullptr);
  WSL_TRY(wsl_conv2d_fwd(&a1, nullptr, c.params + P.cb2.w, c.params + P.cb2.b, c.ws + P.zc2, 2 * F * HW, N, H, W, 2 * F, 1, 0, nullptr,
                         nullptr, c.stream));
  const WslSrc a2 = leaky_src(c, P.zc2, 2 * F, cm1);
  WSL_TRY(wsl_conv2d_fwd(&a2, nullptr, c.params + P.o1.w, c.params + P.o1.b, c.ws + P.zo1, F * HW, N, H, W, F, 1, 0, nullptr, nullptr,
                         c.stream));
  const WslSrc a3 = leaky_src(c, P.zo1, F, cm2);
  return wsl_conv2d_fwd(&a3, nullptr, c.params + P.o2.w, c.params + P.o2.b, logits, (int64_t)P.d.n_class * HW, N, H, W, P.d.n_class, 1,
                        0, nullptr, nullptr, c.stream);
}

static int wgrad_layer(const PCtx& c, const WslSrc* a, const float* dy, int64_t dy_bs, const ConvRef& cv, int dil) {
  const PPlan& P = c.P;
  const int N = P.d.N, H = P.d.H, W = P.d.W;
  const size_t need = ((dil > 0 ? wsl_conv2d_dil_wgrad_ws_bytes(N, H, W, cv.Ci, cv.Co, 3, dil)
                                : wsl_conv2d_wgrad_ws_bytes(N, H, W, cv.Ci, cv.Co, cv.ks)) + 255) & ~(size_t)255;
  float *dw = c.grads + cv.w, *db = c.grads + cv.b;
  return wgrad_push(c.wb, "pnet", c.ws + P.wg_ws, need, [&](void* ws, size_t n, WslWgradPending* q) {
    return dil > 0 ? wsl_conv2d_dil_wgrad_partial(a, nullptr, dy, dy_bs, dw, db, N, H, W, cv.Co, 3, dil, ws, n, q, c.stream)
                   : wsl_conv2d_wgrad_partial(a, nullptr, dy, dy_bs, dw, db, N, H, W, cv.Co, cv.ks, ws, n, q, c.stream);
  });
}

static int leaky_bwd(const PCtx& c, float* g, size_t z, const float* cmask, int C) {
  const int64_t total = c.P.NHW * C;
  WSL_LAUNCH(pnet_leaky_bwd_kernel, dim3(ew_grid(total)), dim3(kThreads), 0, c.stream, g, c.ws + z, cmask, C, c.P.HW, total);
  return check_launch("pnet_leaky_bwd_kernel");
}

// 1x1 data gradient: g [N,Ci,H,W] = conv1x1^T(dy)
static int dgrad_1x1(const PCtx& c, const float* dy, const ConvRef& cv, float* g) {
  const PPlan& P = c.P;
  const WslSrc s = raw_src(dy, cv.Co, (int64_t)cv.Co * P.HW);
  return wsl_conv2d_fwd(&s, nullptr, c.params + cv.w, nullptr, g, (int64_t)cv.Ci * P.HW, P.d.N, P.d.H, P.d.W, cv.Ci, 1, 1, nullptr,
                        nullptr, c.stream);
}

// catblock + out: their gradients are final when it returns; leaves d(concat) [N,5F,H,W] in bufB
static int tail_bwd(const PCtx& c, const float* const* cmasks, const float* dlogits) {
  const PPlan& P = c.P;
  const int F = P.F;
  const int64_t HW = P.HW;
  const float* cm1 = cmasks ? cmasks[0] : nullptr;
  const float* cm2 = cmasks ? cmasks[1] : nullptr;
  float* A = c.ws + P.bufA;
  float* Bf = c.ws + P.bufB;
  // out.conv2
  const WslSrc a3 = leaky_src(c, P.zo1, F, cm2);
  WSL_TRY(wgrad_layer(c, &a3, dlogits, (int64_t)P.d.n_class * HW, P.o2, 0));
  WSL_TRY(dgrad_1x1(c, dlogits, P.o2, A));
  WSL_TRY(leaky_bwd(c, A, P.zo1, cm2, F));
  // out.conv1
  const WslSrc a2 = leaky_src(c, P.zc2, 2 * F, cm1);
  WSL_TRY(wgrad_layer(c, &a2, A, F * HW, P.o1, 0));
  WSL_TRY(dgrad_1x1(c, A, P.o1, Bf));
  WSL_TRY(leaky_bwd(c, Bf, P.zc2, cm1, 2 * F));
  // catblock.conv2
  const WslSrc a1 = leaky_src(c, P.zc1, 5 * F, nullptr);
  WSL_TRY(wgrad_layer(c, &a1, Bf, 2 * F * HW, P.cb2, 0));
  WSL_TRY(dgrad_1x1(c, Bf, P.cb2, A));
  WSL_TRY(leaky_bwd(c, A, P.zc1, nullptr, 5 * F));
  // catblock.conv1: its data gradient is d(cat) for all five blocks at once
  const WslSrc cat = act_src(c.ws + P.cat, 5 * F, 5 * F * HW, c.ws + P.st2 + 10 * F, c.ws + P.st2 + 15 * F, nullptr, 1.f, nullptr);
  WSL_TRY(wgrad_layer(c, &cat, A, 5 * F * HW, P.cb1, 0));
  WSL_TRY(dgrad_1x1(c, A, P.cb1, Bf));
  return wgrad_flush(c.wb, c.stream);
}

// the five blocks, last first; d(cat) in bufB (left by tail_bwd), scratch in bufA
static int blocks_bwd(const PCtx& c, const float* x) {
  const PPlan& P = c.P;
  const int N = P.d.N, H = P.d.H, W = P.d.W, F = P.F;
  const int64_t HW = P.HW, CHW = F * HW, total = P.NHW * F;
  const float* dcat = c.ws + P.bufB;
  float* g = c.ws + P.bufA;
  float* dy2 = g + (size_t)P.NHW * F;
  float* g1 = dy2 + (size_t)P.NHW * F;
  float* dy1 = g1 + (size_t)P.NHW * F;
  float* gnext = dy1 + (size_t)P.NHW * F;   // d(block k output) from block k+1's conv1
  float* ycopy = c.ws + P.ycopy;
  char* bnws = reinterpret_cast<char*>(c.ws + P.bn_ws);
  for (int k = 4; k >= 0; --k) {
    const PBlock& b = P.blk[k];
    const float* s1 = c.ws + P.st1[k];
    const float* s2 = c.ws + P.st2;
    WSL_LAUNCH(pnet_gather_kernel, dim3(ew_grid(total)), dim3(kThreads), 0, c.stream, dcat + (size_t)k * CHW, 5 * CHW,
               k < 4 ? (const float*)gnext : nullptr, g, c.ws + P.cat + (size_t)k * CHW, 5 * CHW, ycopy, CHW, total);
    WSL_TRY(check_launch("pnet_gather_kernel"));
    // in2 + LeakyReLU
    WSL_TRY(wsl_bnact_bwd(g, CHW, ycopy, s2 + k * F, s2 + 5 * F + k * F, c.params + b.b2.gamma, c.params + b.b2.beta, nullptr, 1.f, dy2,
                          c.grads + b.b2.gamma, c.grads + b.b2.beta, N, F, H, W, bnws, P.bn_bytes, c.stream));
    const WslSrc mid = block_mid_src(c, k);
    WSL_TRY(wgrad_layer(c, &mid, dy2, CHW, b.c2, b.dil));
    const WslSrc d2 = raw_src(dy2, F, CHW);
    WSL_TRY(wsl_conv2d_dil_fwd(&d2, nullptr, c.params + b.c2.w, nullptr, g1, CHW, N, H, W, F, 3, b.dil, 1, nullptr, nullptr, c.stream));
    // in1 + LeakyReLU
    WSL_TRY(wsl_bnact_bwd(g1, CHW, c.ws + P.y1[k], s1, s1 + F, c.params + b.b1.gamma, c.params + b.b1.beta, nullptr, 1.f, dy1,
                          c.grads + b.b1.gamma, c.grads + b.b1.beta, N, F, H, W, bnws, P.bn_bytes, c.stream));
    const WslSrc in = k == 0 ? raw_src(x, P.d.in_chns, (int64_t)P.d.in_chns * HW) : block_out_src(c, k - 1);
    WSL_TRY(wgrad_layer(c, &in, dy1, CHW, b.c1, b.dil));
    if (k > 0) {   // (no gradient with respect to the input image)
      const WslSrc d1 = raw_src(dy1, F, CHW);
      WSL_TRY(wsl_conv2d_dil_fwd(&d1, nullptr, c.params + b.c1.w, nullptr, gnext, CHW, N, H, W, F, 3, b.dil, 1, nullptr, nullptr,
                                 c.stream));
    }
  }
  return wgrad_flush(c.wb, c.stream);
}

// state_dict order of the reference module: block{k}.conv1, conv2, in1, in2 (BatchNorm: weight, bias, running_mean, running_var,
// num_batches_tracked), catblock.conv1, conv2, out.conv1, conv2
int enumerate_entries(const PPlan& P, int want, WslNetEntry* out) {
  EntryWalk e{want, out};
  char pre[32];
  for (int k = 0; k < 5; ++k) {
    const PBlock& b = P.blk[k];
    snprintf(pre, sizeof(pre), "block%d", k + 1);
    e.conv(pre, ".conv1", b.c1), e.conv(pre, ".conv2", b.c2), e.bn(pre, ".in1", b.b1), e.bn(pre, ".in2", b.b2);
  }
  e.conv("catblock", ".conv1", P.cb1), e.conv("catblock", ".conv2", P.cb2);
  e.conv("out", ".conv1", P.o1), e.conv("out", ".conv2", P.o2);
  return e.idx;
}

}  // namespace
}  // namespace wsl

using namespace wsl;

extern "C" int wsl_pnet_num_entries(const WslPNetDesc* d) {
  PPlan P;
  if (make_plan(d, P)) return -1;
  return enumerate_entries(P, -1, nullptr);
}
extern "C" int wsl_pnet_entry(const WslPNetDesc* d, int i, WslNetEntry* out) {
  PPlan P;
  WSL_TRY(make_plan(d, P));
  WSL_REQUIRE(out && i >= 0, "pnet_entry: bad args");
  const int n = enumerate_entries(P, i, out);
  WSL_REQUIRE(i < n, "pnet_entry: index %d out of %d", i, n);
  return WSL_OK;
}
extern "C" int64_t wsl_pnet_param_count(const WslPNetDesc* d) {
  PPlan P;
  return make_plan(d, P) ? -1 : P.n_param;
}
extern "C" int64_t wsl_pnet_block_param_count(const WslPNetDesc* d) {
  PPlan P;
  return make_plan(d, P) ? -1 : P.n_block_param;
}
extern "C" int64_t wsl_pnet_buffer_count(const WslPNetDesc* d) {
  PPlan P;
  return make_plan(d, P) ? -1 : P.n_buf;
}
extern "C" size_t wsl_pnet_ws_bytes(const WslPNetDesc* d) {
  PPlan P;
  return make_plan(d, P) ? 0 : P.total_floats * sizeof(float);
}

extern "C" int wsl_pnet_forward(const WslPNetDesc* d, const float* params, float* buffers, int64_t* nbt, const float* x,
                                const float* const* cmasks, int training, float* logits, void* ws, size_t ws_bytes, void* stream) {
  PPlan P;
  WSL_TRY(make_plan(d, P));
  WSL_REQUIRE(params && buffers && x && logits && ws, "pnet_forward: null argument");
  WSL_TRY(check_ws("pnet_forward", ws_bytes, P.total_floats * sizeof(float)));
  PCtx c{P, params, buffers, nbt, nullptr, static_cast<float*>(ws), stream, training, nullptr};
  return pnet_fwd(c, x, cmasks, logits);
}

extern "C" int wsl_pnet_backward(const WslPNetDesc* d, const float* params, const float* x, const float* const* cmasks,
                                 const float* dlogits, float* grads, void* ws, size_t ws_bytes, int phase, void* stream) {
  PPlan P;
  WSL_TRY(make_plan(d, P));
  WSL_REQUIRE(params && x && grads && ws, "pnet_backward: null argument");
  WSL_REQUIRE(phase >= 0 && phase <= 2, "pnet_backward: phase %d", phase);
  WSL_REQUIRE(phase == 2 || dlogits, "pnet_backward: missing dlogits");
  WSL_TRY(check_ws("pnet_backward", ws_bytes, P.total_floats * sizeof(float)));
  WgBatch wb;
  wb.cap = (P.wg_bytes[0] > P.wg_bytes[1] ? P.wg_bytes[0] : P.wg_bytes[1]) + 256;
  PCtx c{P, params, nullptr, nullptr, grads, static_cast<float*>(ws), stream, 1, &wb};
  if (phase == 0 || phase == 1) WSL_TRY(tail_bwd(c, cmasks, dlogits));
  if (phase == 0 || phase == 2) WSL_TRY(blocks_bwd(c, x));
  return WSL_OK;
}
