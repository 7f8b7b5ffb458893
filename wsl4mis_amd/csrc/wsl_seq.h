/* PRIVATE header of libwslhip.so: the host-side sequencing toolkit shared by the network drivers (wsl_net.hip: UNet / UNet_CCT /
 * UpBlock, wsl_pnet.hip: PNet2D; wsl_dil.hip takes WSL_TRY).  One definition of what every driver needs to lay out its arenas and
 * workspace, describe a virtual source tensor, batch the second stages of a phase's weight gradients, finish a BatchNorm forward,
 * enumerate its state_dict and refuse a short workspace.  Nothing here is specific to one network, launches a kernel of its own,
 * allocates or synchronises. */
#pragma once
#include <stdio.h>
#include <string.h>

#include "wsl_rt.h"

#define WSL_TRY(expr)                 \
  do {                                \
    if (int rc_ = (expr)) return rc_; \
  } while (0)

namespace wsl {
namespace {   // (internal linkage for the member functions too: the library exports nothing from here)

constexpr float kEps = 1e-5f, kMom = 0.1f;   // nn.BatchNorm2d defaults

// ------------------------------------------------------------------------------------------------ planning
struct Bump {   // float offsets into a workspace, every region 64-float aligned
  size_t off = 0;
  size_t take(size_t n, const char* = "") {
    const size_t o = off;
    off += (n + 63) & ~(size_t)63;
    return o;
  }
};

struct ConvRef { int64_t w, b; int Ci, Co, ks; int li; };   // li: index in the pack table (UNet)
struct BnRef { int64_t gamma, beta, rmean, rvar; int nbt, C; };

// po / bo / nbn: running offsets into the parameter arena, the buffer arena and the num_batches_tracked array
static inline void plan_conv(ConvRef& c, int Ci, int Co, int ks, int64_t& po) {
  c.Ci = Ci, c.Co = Co, c.ks = ks;
  c.w = po, po += (int64_t)Co * Ci * ks * ks;
  c.b = po, po += Co;
}
static inline void plan_bn(BnRef& b, int C, int64_t& po, int64_t& bo, int64_t& nbn) {
  b.C = C;
  b.gamma = po, po += C;
  b.beta = po, po += C;
  b.rmean = bo, bo += C;
  b.rvar = bo, bo += C;
  b.nbt = (int)nbn++;
}

static inline int check_ws(const char* who, size_t ws_bytes, size_t need) {
  if (ws_bytes >= need) return WSL_OK;
  set_error("%s: workspace %zu < %zu", who, ws_bytes, need);
  return WSL_EWORKSPACE;
}

// ------------------------------------------------------------------------------------------------ virtual source tensors
static inline WslSrc raw_src(const float* x, int C, int64_t bs) {
  WslSrc s{};
  s.x = x, s.C = C, s.bs = bs, s.emask_scale = 1.f;
  return s;
}
// leaky(y * scale + shift) [* emask * es] [* cmask], rebuilt by the consumer's loader
static inline WslSrc act_src(const float* y, int C, int64_t bs, const float* scale, const float* shift, const uint8_t* emask, float es,
                             const float* cmask) {
  WslSrc s = raw_src(y, C, bs);
  s.scale = scale, s.shift = shift;
  s.emask = emask, s.emask_scale = es, s.cmask = cmask;
  return s;
}

// ------------------------------------------------------------------------------------------------ BatchNorm forward
// training: batch statistics from the producing convolution's per-tile partials -> coefficients + running statistics;
// else: coefficients from the running statistics.  The four tables may be strided (PNet2D's concatenated in2 tables).
static inline int bn_fwd(int training, const float* stat_part, const float* stat_cnt, int nblk, const BnRef& bn, const float* params,
                         float* buffers, int64_t* nbt, float* mean, float* invstd, float* scale, float* shift, void* stream) {
  if (training)
    return wsl_bn_stats_finalize(stat_part, stat_cnt, nblk, bn.C, params + bn.gamma, params + bn.beta, kEps, kMom, buffers + bn.rmean,
                                 buffers + bn.rvar, nbt ? nbt + bn.nbt : nullptr, mean, invstd, scale, shift, stream);
  return wsl_bn_eval_affine(params + bn.gamma, params + bn.beta, buffers + bn.rmean, buffers + bn.rvar, kEps, bn.C, scale, shift, stream);
}

// ------------------------------------------------------------------------------------------------ weight-gradient batches
// pending second stages of a phase (a decoder's backward, the encoder's, PNet2D's head / blocks): every layer's stage 1 gets its own
// region of the phase's partials area, one wsl_wgrad_reduce_batch launch finishes them all
struct WgBatch {
  WslWgradPending items[24];
  int n = 0;
  size_t off = 0, cap = 0;   // bytes used / available
};

// stage 1 of one layer: stage1(region, need, pending) is the f32 / split / dilated wsl_*_wgrad_partial call; `need` in bytes (256-aligned)
template <class Stage1>
static inline int wgrad_push(WgBatch* wb, const char* who, void* area, size_t need, Stage1 stage1) {
  if (!wb || wb->n >= 24 || wb->off + need > wb->cap) {
    set_error("%s: weight-gradient batch overflow (%d pending, %zu + %zu of %zu bytes)", who, wb ? wb->n : -1, wb ? wb->off : 0, need,
              wb ? wb->cap : 0);
    return WSL_EWORKSPACE;
  }
  WSL_TRY(stage1(static_cast<char*>(area) + wb->off, need, &wb->items[wb->n]));
  wb->n += 1, wb->off += need;
  return WSL_OK;
}
static inline int wgrad_flush(WgBatch* wb, void* stream) {
  if (!wb || wb->n == 0) return WSL_OK;
  const int rc = wsl_wgrad_reduce_batch(wb->items, wb->n, stream);
  wb->n = 0, wb->off = 0;
  return rc;
}

// ------------------------------------------------------------------------------------------------ state_dict enumeration
static inline void entry_set(WslNetEntry* e, const char* name, int kind, int ndim, int64_t s0, int64_t s1, int64_t s2, int64_t s3,
                             int64_t off) {
  memset(e, 0, sizeof(*e));
  snprintf(e->name, sizeof(e->name), "%s", name);
  e->kind = kind, e->ndim = ndim, e->offset = off;
  e->shape[0] = s0, e->shape[1] = s1, e->shape[2] = s2, e->shape[3] = s3;
}
// walks a module's entries in the reference's state_dict order; fills `out` at entry number `want`, idx ends as the entry count
struct EntryWalk {
  int want;
  WslNetEntry* out;
  int idx = 0;
  void put(const char* pre, const char* sfx, const char* field, int kind, int ndim, int64_t s0, int64_t s1, int64_t s2, int64_t s3,
           int64_t off) {
    if (idx++ != want) return;
    char nm[128];
    snprintf(nm, sizeof(nm), "%s%s.%s", pre, sfx, field);
    entry_set(out, nm, kind, ndim, s0, s1, s2, s3, off);
  }
  void conv(const char* pre, const char* sfx, const ConvRef& c) {
    put(pre, sfx, "weight", 0, 4, c.Co, c.Ci, c.ks, c.ks, c.w);
    put(pre, sfx, "bias", 0, 1, c.Co, 0, 0, 0, c.b);
  }
  void bn(const char* pre, const char* sfx, const BnRef& b) {
    put(pre, sfx, "weight", 0, 1, b.C, 0, 0, 0, b.gamma);
    put(pre, sfx, "bias", 0, 1, b.C, 0, 0, 0, b.beta);
    put(pre, sfx, "running_mean", 1, 1, b.C, 0, 0, 0, b.rmean);
    put(pre, sfx, "running_var", 1, 1, b.C, 0, 0, 0, b.rvar);
    put(pre, sfx, "num_batches_tracked", 2, 0, 0, 0, 0, 0, b.nbt);
  }
};

}  // namespace
}  // namespace wsl
