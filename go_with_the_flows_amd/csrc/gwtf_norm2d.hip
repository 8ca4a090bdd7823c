// gwtf_norm2d.hip -- train-mode BatchNorm2d fused with what follows it in the image encoder (ResNet-18, contiguous NCHW fp32):
//   none            y = g * xhat + b                                  (the downsample branch)
//   relu            y = relu(g * xhat + b)
//   relu + residual y = relu(g * xhat + b + r)                        (the BasicBlock tail)
//   relu + pool     y = maxpool3x3/2/1(relu(g * xhat + b))            (the stem; the full-size activation is never written)
// Record, semantics and refusals: include/gwtf.h (GwtfNorm2dArgs).
//
// Forward, three launches
//   stats      grid (C, S) x 256: block (c, s) sums x and x * x of its share of channel c in float64 (the exact product of two
//              floats; no cancellation to speak of in E[x^2] - mean^2 at 53 bits), a fixed-order LDS tree, one partial per block
//   finalise   one thread per channel adds the S partials in order, writes mean (as a float and the float of what the rounding
//              lost), rstd, and the running statistics
//   apply      grid (tiles of an image, N) x 256: normalise (+ r) (relu); with pool one thread per POOLED element, which
//              evaluates its <= 9 inputs, keeps the first maximum in row-major order and stores the value and the window offset
// Backward, three launches of the same shapes: partial sums of dy' and dy' * xhat, finalise (dgamma, dbeta), apply
//   dx = g * rstd * (dy' - mean(dy') - xhat * mean(dy' * xhat)),  d_residual = dy'
// with dy' = dy * [y > 0] read from the saved output, or with pool gathered from the pooled gradient and the offset image:
// position (h, w) lies in at most four windows, each contributes when its offset points at (h, w); y is recomputed from x by the
// forward's own expression (norm_affine, uncontracted) so that its sign is the forward's.
//
// A thread takes four consecutive floats as one 16-byte access when planes are a multiple of four floats and every base address is
// 16-byte aligned; otherwise (7 x 7 planes) one float at a time.  One 32-bit division per access finds the plane.
// No atomics, no scratch, no device-side allocation: two runs give the same bits.
//
// Statistics over several ranks (SyncBatchNorm): each direction as two calls around the caller's sum over the ranks.  *_sums runs the
// partial-sum launch and folds the S partials into this rank's float64 (C, 2) sums; *_apply finalises from the totals and the global
// count and runs the same applying launch.  The kernels of the one-rank calls are launched unchanged; three one-thread-per-channel
// launches are new (fold, finalise from sums, the totals as floats for the backward's applying launch).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/gwtf.h"

namespace {

constexpr int kThreads = 256;
constexpr int kQuads = 4;                      // accesses per thread of an apply tile
constexpr int kMaxSplit = 64;                  // S <= kMaxSplit
constexpr int kWantBlocks = 2048;              // blocks of a (C, S) grid aimed at: 8 per compute unit
constexpr unsigned kMinShare = 8192;           // elements a split is worth

typedef float quad_t __attribute__((ext_vector_type(4)));

enum { kPlain = 0, kMask = 1, kPool = 2 };     // dy' of the backward: dy, dy * [y > 0], the pooled gather

// ---- the forward's arithmetic, shared with the recomputation in the pooled backward --------------------------------------------
__device__ __forceinline__ float centred(float x, float m, float ml) { return (x - m) - ml; }
__device__ __forceinline__ float norm_affine(float x, float m, float ml, float a, float b) { return centred(x, m, ml) * a + b; }

struct Channel { float m, ml, rstd, a, b; };
__device__ __forceinline__ Channel channel(const GwtfNorm2dArgs& p, int c) {
  Channel k;
  k.m = p.stats[c]; k.rstd = p.stats[p.C + c]; k.ml = p.stats[2 * p.C + c];
  k.a = k.rstd * p.gamma[c]; k.b = p.beta ? p.beta[c] : 0.f;
  return k;
}

__host__ __device__ inline int pooled(int n) { return (n - 1) / 2 + 1; }      // kernel 3, stride 2, padding 1

// Sum of the pooled gradients whose window maximum sits at (h, w); g / off: the (n, c) plane of the pooled images.
__device__ __forceinline__ float pool_gather(const float* g, const unsigned char* off, int h, int w, int Ho, int Wo) {
  const int i0 = h >> 1, i1 = (h + 1) >> 1, j0 = w >> 1, j1 = (w + 1) >> 1;
  float acc = 0.f;
#pragma unroll
  for (int ii = 0; ii < 2; ++ii) {
    const int i = ii ? i1 : i0;
    if ((ii && i1 == i0) || i >= Ho) continue;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = jj ? j1 : j0;
      if ((jj && j1 == j0) || j >= Wo) continue;
      const int o = off[i * Wo + j], oy = o / 3, ox = o - 3 * oy;
      if (2 * i - 1 + oy == h && 2 * j - 1 + ox == w) acc += g[i * Wo + j];
    }
  }
  return acc;
}

// Fixed-order tree over the block: thread 0 returns the two sums.
__device__ __forceinline__ void block_sum2(double& s1, double& s2) {
  __shared__ double red[2][kThreads];
  const int t = threadIdx.x;
  red[0][t] = s1; red[1][t] = s2;
  __syncthreads();
#pragma unroll
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (t < w) { red[0][t] += red[0][t + w]; red[1][t] += red[1][t + w]; }
    __syncthreads();
  }
  s1 = red[0][0]; s2 = red[1][0];
}

// ---- partial sums over a (C, S) grid -----------------------------------------------------------------------------------------
// Forward (BWD = false): x and x * x.  Backward: dy' and dy' * xhat, dy' by MODE.
template <bool VEC, bool BWD, int MODE>
__global__ __launch_bounds__(kThreads) void partials_kernel(GwtfNorm2dArgs p, unsigned nhw, unsigned per) {
  const int c = blockIdx.x, s = blockIdx.y, S = gridDim.y;
  const int C = p.C, HW = p.H * p.W;
  const unsigned begin = (unsigned)s * per, end = begin + per < nhw ? begin + per : nhw;
  constexpr int step = VEC ? 4 : 1;
  Channel k = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (BWD) k = channel(p, c);
  const int Ho = pooled(p.H), Wo = pooled(p.W);
  double s1 = 0.0, s2 = 0.0;
  for (unsigned e = begin + threadIdx.x * step; e < end; e += kThreads * step) {
    const unsigned n = e / (unsigned)HW, i = e - n * (unsigned)HW;
    const size_t at = ((size_t)n * C + c) * HW + i;
    float xv[4], dv[4] = {0.f, 0.f, 0.f, 0.f}, yv[4] = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
      const quad_t q = *reinterpret_cast<const quad_t*>(p.x + at);
      xv[0] = q[0]; xv[1] = q[1]; xv[2] = q[2]; xv[3] = q[3];
      if (BWD && MODE != kPool) {
        const quad_t d = *reinterpret_cast<const quad_t*>(p.dy + at);
        dv[0] = d[0]; dv[1] = d[1]; dv[2] = d[2]; dv[3] = d[3];
      }
      if (BWD && MODE == kMask) {
        const quad_t y = *reinterpret_cast<const quad_t*>(p.y + at);
        yv[0] = y[0]; yv[1] = y[1]; yv[2] = y[2]; yv[3] = y[3];
      }
    } else {
      xv[0] = p.x[at];
      if (BWD && MODE != kPool) dv[0] = p.dy[at];
      if (BWD && MODE == kMask) yv[0] = p.y[at];
    }
    int h = 0, w = 0;
    size_t pplane = 0;
    if (BWD && MODE == kPool) { h = (int)(i / (unsigned)p.W); w = (int)i - h * p.W; pplane = ((size_t)n * C + c) * Ho * Wo; }
#pragma unroll
    for (int j = 0; j < step; ++j) {
      if (!BWD) {
        const double v = (double)xv[j];
        s1 += v; s2 += v * v;
      } else {
        float d;
        if (MODE == kPool) {
          int hh = h, ww = w + j;
          if (ww >= p.W) { ww -= p.W; ++hh; }            // a quad runs over one row end at most: the host takes this path for W >= 4
          d = norm_affine(xv[j], k.m, k.ml, k.a, k.b) > 0.f ? pool_gather(p.dy + pplane, p.offsets + pplane, hh, ww, Ho, Wo) : 0.f;
        } else if (MODE == kMask) {
          d = yv[j] > 0.f ? dv[j] : 0.f;
        } else {
          d = dv[j];
        }
        const float xh = centred(xv[j], k.m, k.ml) * k.rstd;
        s1 += (double)d; s2 += (double)d * (double)xh;
      }
    }
  }
  block_sum2(s1, s2);
  if (threadIdx.x == 0) {
    p.partials[((size_t)c * S + s) * 2] = s1;
    p.partials[((size_t)c * S + s) * 2 + 1] = s2;
  }
}

// Channel c's statistics from its sums over `count` values: stats and the running statistics.
__device__ __forceinline__ void finalize_channel(const GwtfNorm2dArgs& p, int c, double s1, double s2, double count) {
  const double mean = s1 / count;
  double var = s2 / count - mean * mean;
  if (var < 0.0) var = 0.0;
  const float mf = (float)mean;
  p.stats[c] = mf;
  p.stats[p.C + c] = (float)(1.0 / sqrt(var + (double)p.eps));
  p.stats[2 * p.C + c] = (float)(mean - (double)mf);
  const double mom = (double)p.momentum;
  if (p.running_mean) p.running_mean[c] = (float)((1.0 - mom) * (double)p.running_mean[c] + mom * mean);
  if (p.running_var) p.running_var[c] = (float)((1.0 - mom) * (double)p.running_var[c] + mom * (var * count / (count - 1.0)));
}

__global__ __launch_bounds__(kThreads) void finalize_forward_kernel(GwtfNorm2dArgs p, int S, double count) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= p.C) return;
  double s1 = 0.0, s2 = 0.0;
  for (int s = 0; s < S; ++s) { s1 += p.partials[((size_t)c * S + s) * 2]; s2 += p.partials[((size_t)c * S + s) * 2 + 1]; }
  finalize_channel(p, c, s1, s2, count);
}

// ---- statistics over several ranks: the finalising launches split where the caller sums over the ranks ----------------------------
// This rank's sums of channel c, the S partials added in the order of the finalising kernels above.  BWD: also the rank-local
// parameter gradients, as finalize_backward_kernel writes them.
template <bool BWD>
__global__ __launch_bounds__(kThreads) void fold_sums_kernel(GwtfNorm2dArgs p, int S, double* sums) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= p.C) return;
  double s1 = 0.0, s2 = 0.0;
  for (int s = 0; s < S; ++s) { s1 += p.partials[((size_t)c * S + s) * 2]; s2 += p.partials[((size_t)c * S + s) * 2 + 1]; }
  sums[2 * c] = s1;
  sums[2 * c + 1] = s2;
  if (BWD) { p.dbeta[c] = (float)s1; p.dgamma[c] = (float)s2; }
}

__global__ __launch_bounds__(kThreads) void finalize_from_sums_kernel(GwtfNorm2dArgs p, const double* sums, double count) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= p.C) return;
  finalize_channel(p, c, sums[2 * c], sums[2 * c + 1], count);
}

// The totals as floats, [2][C]: what apply_backward_kernel reads through dbeta / dgamma.
__global__ __launch_bounds__(kThreads) void float_sums_kernel(const double* sums, float* out, int C) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= C) return;
  out[c] = (float)sums[2 * c];
  out[C + c] = (float)sums[2 * c + 1];
}

__global__ __launch_bounds__(kThreads) void finalize_backward_kernel(GwtfNorm2dArgs p, int S) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= p.C) return;
  double s1 = 0.0, s2 = 0.0;
  for (int s = 0; s < S; ++s) { s1 += p.partials[((size_t)c * S + s) * 2]; s2 += p.partials[((size_t)c * S + s) * 2 + 1]; }
  p.dbeta[c] = (float)s1;
  p.dgamma[c] = (float)s2;
}

// ---- apply, forward ----------------------------------------------------------------------------------------------------------
template <bool VEC, bool RELU, bool RES>
__global__ __launch_bounds__(kThreads) void apply_forward_kernel(GwtfNorm2dArgs p, unsigned chw) {
  constexpr int step = VEC ? 4 : 1;
  const size_t img = (size_t)blockIdx.y * chw;
  const unsigned base = blockIdx.x * (unsigned)(kThreads * kQuads * step);
  const unsigned HW = (unsigned)(p.H * p.W);
#pragma unroll
  for (int q = 0; q < kQuads; ++q) {
    const unsigned e = base + (unsigned)(q * kThreads + threadIdx.x) * step;
    if (e >= chw) continue;
    const Channel k = channel(p, (int)(e / HW));
    float v[4], r[4] = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
      const quad_t t = *reinterpret_cast<const quad_t*>(p.x + img + e);
      v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
      if (RES) { const quad_t u = *reinterpret_cast<const quad_t*>(p.residual + img + e); r[0] = u[0]; r[1] = u[1]; r[2] = u[2]; r[3] = u[3]; }
    } else {
      v[0] = p.x[img + e];
      if (RES) r[0] = p.residual[img + e];
    }
#pragma unroll
    for (int j = 0; j < step; ++j) {
      float o = norm_affine(v[j], k.m, k.ml, k.a, k.b);
      if (RES) o = o + r[j];
      if (RELU) o = o > 0.f ? o : 0.f;
      v[j] = o;
    }
    if (VEC) {
      const quad_t t = {v[0], v[1], v[2], v[3]};
      *reinterpret_cast<quad_t*>(p.y + img + e) = t;
    } else {
      p.y[img + e] = v[0];
    }
  }
}

// One thread per pooled element: relu(norm) of the window, first maximum in row-major order, padding = -inf.
__global__ __launch_bounds__(kThreads) void apply_forward_pool_kernel(GwtfNorm2dArgs p, unsigned cpool) {
  const unsigned e = blockIdx.x * (unsigned)kThreads + threadIdx.x;
  if (e >= cpool) return;
  const int H = p.H, W = p.W, Ho = pooled(H), Wo = pooled(W);
  const unsigned c = e / (unsigned)(Ho * Wo), rem = e - c * (unsigned)(Ho * Wo);
  const int i = (int)(rem / (unsigned)Wo), j = (int)rem - i * Wo;
  const Channel k = channel(p, (int)c);
  const float* xp = p.x + ((size_t)blockIdx.y * p.C + c) * H * W;
  float best = -INFINITY;
  int at = 0;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int h = 2 * i - 1 + dy;
    if (h < 0 || h >= H) continue;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int w = 2 * j - 1 + dx;
      if (w < 0 || w >= W) continue;
      float v = norm_affine(xp[h * W + w], k.m, k.ml, k.a, k.b);
      v = v > 0.f ? v : 0.f;
      if (v > best) { best = v; at = dy * 3 + dx; }
    }
  }
  const size_t o = (size_t)blockIdx.y * cpool + e;
  p.y[o] = best;
  p.offsets[o] = (unsigned char)at;
}

// ---- apply, backward ---------------------------------------------------------------------------------------------------------
template <bool VEC, int MODE, bool RES>
__global__ __launch_bounds__(kThreads) void apply_backward_kernel(GwtfNorm2dArgs p, unsigned chw, float inv_count) {
  constexpr int step = VEC ? 4 : 1;
  const size_t img = (size_t)blockIdx.y * chw;
  const unsigned base = blockIdx.x * (unsigned)(kThreads * kQuads * step);
  const unsigned HW = (unsigned)(p.H * p.W);
  const int Ho = pooled(p.H), Wo = pooled(p.W);
#pragma unroll
  for (int q = 0; q < kQuads; ++q) {
    const unsigned e = base + (unsigned)(q * kThreads + threadIdx.x) * step;
    if (e >= chw) continue;
    const unsigned c = e / HW, i = e - c * HW;
    const Channel k = channel(p, (int)c);
    const float m1 = p.dbeta[c] * inv_count, m2 = p.dgamma[c] * inv_count;
    float xv[4], dv[4] = {0.f, 0.f, 0.f, 0.f}, yv[4] = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
      const quad_t t = *reinterpret_cast<const quad_t*>(p.x + img + e);
      xv[0] = t[0]; xv[1] = t[1]; xv[2] = t[2]; xv[3] = t[3];
      if (MODE != kPool) { const quad_t d = *reinterpret_cast<const quad_t*>(p.dy + img + e); dv[0] = d[0]; dv[1] = d[1]; dv[2] = d[2]; dv[3] = d[3]; }
      if (MODE == kMask) { const quad_t y = *reinterpret_cast<const quad_t*>(p.y + img + e); yv[0] = y[0]; yv[1] = y[1]; yv[2] = y[2]; yv[3] = y[3]; }
    } else {
      xv[0] = p.x[img + e];
      if (MODE != kPool) dv[0] = p.dy[img + e];
      if (MODE == kMask) yv[0] = p.y[img + e];
    }
    int h = 0, w = 0;
    size_t pplane = 0;
    if (MODE == kPool) { h = (int)(i / (unsigned)p.W); w = (int)i - h * p.W; pplane = ((size_t)blockIdx.y * p.C + c) * Ho * Wo; }
    float dr[4];
#pragma unroll
    for (int j = 0; j < step; ++j) {
      float d;
      if (MODE == kPool) {
        int hh = h, ww = w + j;
        if (ww >= p.W) { ww -= p.W; ++hh; }
        d = norm_affine(xv[j], k.m, k.ml, k.a, k.b) > 0.f ? pool_gather(p.dy + pplane, p.offsets + pplane, hh, ww, Ho, Wo) : 0.f;
      } else if (MODE == kMask) {
        d = yv[j] > 0.f ? dv[j] : 0.f;
      } else {
        d = dv[j];
      }
      const float xh = centred(xv[j], k.m, k.ml) * k.rstd;
      dr[j] = d;
      xv[j] = k.a * ((d - m1) - xh * m2);
    }
    if (VEC) {
      const quad_t t = {xv[0], xv[1], xv[2], xv[3]};
      *reinterpret_cast<quad_t*>(p.dx + img + e) = t;
      if (RES) { const quad_t u = {dr[0], dr[1], dr[2], dr[3]}; *reinterpret_cast<quad_t*>(p.d_residual + img + e) = u; }
    } else {
      p.dx[img + e] = xv[0];
      if (RES) p.d_residual[img + e] = dr[0];
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
int split_of(long long nhw, int C) {
  long long want = (kWantBlocks + C - 1) / C, cap = (nhw + kMinShare - 1) / kMinShare;
  long long s = want < cap ? want : cap;
  if (s > kMaxSplit) s = kMaxSplit;
  return s < 1 ? 1 : (int)s;
}

// least: the values per channel this rank must hold (2; 1 when the statistics cover other ranks' images as well)
int check_sizes(int N, int C, int H, int W, long long least = 2) {
  if (N < 1 || C < 1 || H < 1 || W < 1 || N > 65535) return GWTF_E_BADARG;
  const long long hw = (long long)H * W, nhw = (long long)N * hw, chw = (long long)C * hw;
  if (nhw >= (1LL << 31) - 4LL * kMaxSplit - kThreads * 4 || chw >= (1LL << 31) - kThreads * kQuads * 4) return GWTF_E_BADARG;
  if (nhw < least) return GWTF_E_FEW_VALUES;
  return 0;
}

int check_common(const GwtfNorm2dArgs* pa, long long least = 2) {
  if (!pa) return GWTF_E_BADARG;
  const GwtfNorm2dArgs& a = *pa;
  const int e = check_sizes(a.N, a.C, a.H, a.W, least);
  if (e) return e;
  if (!a.x || !a.gamma || !a.stats || !a.partials) return GWTF_E_BADARG;
  if (a.pool && (!a.relu || a.residual || a.d_residual || !a.offsets)) return GWTF_E_BADARG;
  if (!(a.eps >= 0.f) || !(a.momentum >= 0.f && a.momentum <= 1.f)) return GWTF_E_BADARG;
  return 0;
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15u) == 0; }

// What the launches of one call share: the stream, the sizes, the split of the partial sums.
struct Work {
  hipStream_t st;
  unsigned hw, nhw, chw, per;
  int S;
};

Work work_of(const GwtfNorm2dArgs& a) {
  Work w;
  w.st = (hipStream_t)a.stream;
  w.hw = (unsigned)(a.H * a.W); w.nhw = (unsigned)a.N * w.hw; w.chw = (unsigned)a.C * w.hw;
  w.S = split_of(w.nhw, a.C);
  w.per = ((w.nhw + w.S - 1) / w.S + 3u) & ~3u;
  return w;
}

dim3 channel_grid(int C) { return dim3((C + kThreads - 1) / kThreads); }

// The totals over the ranks and the number of values they cover.
int check_totals(const double* sums, double count, const Work& w) {
  if (!sums) return GWTF_E_BADARG;
  if (!(count >= 2.0)) return GWTF_E_FEW_VALUES;
  if (count < (double)w.nhw) return GWTF_E_BADARG;
  return 0;
}

void launch_forward_partials(const GwtfNorm2dArgs& a, const Work& w) {
  const bool vec_x = w.hw % 4 == 0 && aligned16(a.x);
  if (vec_x) hipLaunchKernelGGL((partials_kernel<true, false, kPlain>), dim3(a.C, w.S), dim3(kThreads), 0, w.st, a, w.nhw, w.per);
  else hipLaunchKernelGGL((partials_kernel<false, false, kPlain>), dim3(a.C, w.S), dim3(kThreads), 0, w.st, a, w.nhw, w.per);
}

void launch_forward_apply(const GwtfNorm2dArgs& a, const Work& w) {
  hipStream_t st = w.st;
  const unsigned chw = w.chw;
  if (a.pool) {
    const unsigned cpool = (unsigned)a.C * pooled(a.H) * pooled(a.W);
    hipLaunchKernelGGL(apply_forward_pool_kernel, dim3((cpool + kThreads - 1) / kThreads, a.N), dim3(kThreads), 0, st, a, cpool);
    return;
  }
  const bool vec = w.hw % 4 == 0 && aligned16(a.x) && aligned16(a.y) && (!a.residual || aligned16(a.residual));
  const unsigned tile = kThreads * kQuads * (vec ? 4 : 1);
  const dim3 grid((chw + tile - 1) / tile, a.N), block(kThreads);
#define GWTF_NORM2D_FWD(V, R, S_) hipLaunchKernelGGL((apply_forward_kernel<V, R, S_>), grid, block, 0, st, a, chw)
  const bool relu = a.relu != 0, res = a.residual != nullptr;
  if (vec) {
    if (relu) { if (res) GWTF_NORM2D_FWD(true, true, true); else GWTF_NORM2D_FWD(true, true, false); }
    else { if (res) GWTF_NORM2D_FWD(true, false, true); else GWTF_NORM2D_FWD(true, false, false); }
  } else {
    if (relu) { if (res) GWTF_NORM2D_FWD(false, true, true); else GWTF_NORM2D_FWD(false, true, false); }
    else { if (res) GWTF_NORM2D_FWD(false, false, true); else GWTF_NORM2D_FWD(false, false, false); }
  }
#undef GWTF_NORM2D_FWD
}

int backward_mode(const GwtfNorm2dArgs& a) { return a.pool ? kPool : (a.relu ? kMask : kPlain); }

// What either backward launch reads besides x, gamma and stats.
bool backward_reads_ok(const GwtfNorm2dArgs& a) {
  if (!a.dy) return false;
  if (a.relu && !a.pool && !a.y) return false;                      // the mask is read from the saved output
  if (a.pool && !a.beta) return false;                              // the recomputation needs the forward's shift
  return true;
}

// One access width for both backward launches (a NULL dx counts as aligned: the split entry points pass one record to both calls).
bool backward_vec(const GwtfNorm2dArgs& a, const Work& w) {
  const int mode = backward_mode(a);
  // with pool a quad may run over a row's end into the next row (handled) but never over two: W >= 4
  bool vec = w.hw % 4 == 0 && aligned16(a.x) && aligned16(a.dx) && (!a.d_residual || aligned16(a.d_residual));
  if (mode == kPool) vec = vec && a.W >= 4;
  else vec = vec && aligned16(a.dy) && (mode != kMask || aligned16(a.y));
  return vec;
}

void launch_backward_partials(const GwtfNorm2dArgs& a, const Work& w) {
  const int mode = backward_mode(a);
  const dim3 pgrid(a.C, w.S), block(kThreads);
#define GWTF_NORM2D_PART(V, M) hipLaunchKernelGGL((partials_kernel<V, true, M>), pgrid, block, 0, w.st, a, w.nhw, w.per)
  if (backward_vec(a, w)) { if (mode == kPool) GWTF_NORM2D_PART(true, kPool); else if (mode == kMask) GWTF_NORM2D_PART(true, kMask); else GWTF_NORM2D_PART(true, kPlain); }
  else { if (mode == kPool) GWTF_NORM2D_PART(false, kPool); else if (mode == kMask) GWTF_NORM2D_PART(false, kMask); else GWTF_NORM2D_PART(false, kPlain); }
#undef GWTF_NORM2D_PART
}

// dbeta / dgamma of the record: the two sums over all `1 / inv_count` values, as floats.
void launch_backward_apply(const GwtfNorm2dArgs& a, const Work& w, float inv_count) {
  const int mode = backward_mode(a);
  const bool vec = backward_vec(a, w);
  hipStream_t st = w.st;
  const unsigned chw = w.chw;
  const unsigned tile = kThreads * kQuads * (vec ? 4 : 1);
  const dim3 grid((chw + tile - 1) / tile, a.N), block(kThreads);
  const bool res = a.d_residual != nullptr;
#define GWTF_NORM2D_BWD(V, M, R) hipLaunchKernelGGL((apply_backward_kernel<V, M, R>), grid, block, 0, st, a, chw, inv_count)
  if (vec) {
    if (mode == kPool) GWTF_NORM2D_BWD(true, kPool, false);
    else if (mode == kMask) { if (res) GWTF_NORM2D_BWD(true, kMask, true); else GWTF_NORM2D_BWD(true, kMask, false); }
    else { if (res) GWTF_NORM2D_BWD(true, kPlain, true); else GWTF_NORM2D_BWD(true, kPlain, false); }
  } else {
    if (mode == kPool) GWTF_NORM2D_BWD(false, kPool, false);
    else if (mode == kMask) { if (res) GWTF_NORM2D_BWD(false, kMask, true); else GWTF_NORM2D_BWD(false, kMask, false); }
    else { if (res) GWTF_NORM2D_BWD(false, kPlain, true); else GWTF_NORM2D_BWD(false, kPlain, false); }
  }
#undef GWTF_NORM2D_BWD
}

}  // namespace

extern "C" int gwtf_norm2d_partials(int N, int C, int H, int W) {
  if (check_sizes(N, C, H, W)) return 0;
  return split_of((long long)N * H * W, C);
}

extern "C" int gwtf_norm2d_forward(const GwtfNorm2dArgs* pa) {
  const int bad = check_common(pa);
  if (bad) return bad;
  const GwtfNorm2dArgs& a = *pa;
  if (!a.beta || !a.y) return GWTF_E_BADARG;
  const Work w = work_of(a);
  launch_forward_partials(a, w);
  hipLaunchKernelGGL(finalize_forward_kernel, channel_grid(a.C), dim3(kThreads), 0, w.st, a, w.S, (double)w.nhw);
  launch_forward_apply(a, w);
  return (int)hipGetLastError();
}

extern "C" int gwtf_norm2d_forward_sums(const GwtfNorm2dArgs* pa, double* sums) {
  const int bad = check_common(pa, 1);
  if (bad) return bad;
  if (!sums) return GWTF_E_BADARG;
  const GwtfNorm2dArgs& a = *pa;
  const Work w = work_of(a);
  launch_forward_partials(a, w);
  hipLaunchKernelGGL(fold_sums_kernel<false>, channel_grid(a.C), dim3(kThreads), 0, w.st, a, w.S, sums);
  return (int)hipGetLastError();
}

extern "C" int gwtf_norm2d_forward_apply(const GwtfNorm2dArgs* pa, const double* sums, double count) {
  int bad = check_common(pa, 1);
  if (bad) return bad;
  const GwtfNorm2dArgs& a = *pa;
  if (!a.beta || !a.y) return GWTF_E_BADARG;
  const Work w = work_of(a);
  if ((bad = check_totals(sums, count, w))) return bad;
  hipLaunchKernelGGL(finalize_from_sums_kernel, channel_grid(a.C), dim3(kThreads), 0, w.st, a, sums, count);
  launch_forward_apply(a, w);
  return (int)hipGetLastError();
}

extern "C" int gwtf_norm2d_backward(const GwtfNorm2dArgs* pa) {
  const int bad = check_common(pa);
  if (bad) return bad;
  const GwtfNorm2dArgs& a = *pa;
  if (!a.dx || !a.dgamma || !a.dbeta) return GWTF_E_BADARG;
  if (!backward_reads_ok(a)) return GWTF_E_BADARG;
  const Work w = work_of(a);
  launch_backward_partials(a, w);
  hipLaunchKernelGGL(finalize_backward_kernel, channel_grid(a.C), dim3(kThreads), 0, w.st, a, w.S);
  launch_backward_apply(a, w, (float)(1.0 / (double)w.nhw));
  return (int)hipGetLastError();
}

extern "C" int gwtf_norm2d_backward_sums(const GwtfNorm2dArgs* pa, double* sums) {
  const int bad = check_common(pa, 1);
  if (bad) return bad;
  const GwtfNorm2dArgs& a = *pa;
  if (!sums || !a.dgamma || !a.dbeta || !backward_reads_ok(a)) return GWTF_E_BADARG;
  const Work w = work_of(a);
  launch_backward_partials(a, w);
  hipLaunchKernelGGL(fold_sums_kernel<true>, channel_grid(a.C), dim3(kThreads), 0, w.st, a, w.S, sums);
  return (int)hipGetLastError();
}

extern "C" int gwtf_norm2d_backward_apply(const GwtfNorm2dArgs* pa, const double* sums, double count) {
  int bad = check_common(pa, 1);
  if (bad) return bad;
  if (!pa->dx || !backward_reads_ok(*pa)) return GWTF_E_BADARG;
  const Work w = work_of(*pa);
  if ((bad = check_totals(sums, count, w))) return bad;
  // the applying launch reads the two sums through dbeta / dgamma: the totals, as floats, in the partials' space ([C][S][2] doubles
  // hold 2 C floats for every S >= 1); this rank's dbeta / dgamma stay as backward_sums left them
  GwtfNorm2dArgs a = *pa;
  a.dbeta = reinterpret_cast<float*>(a.partials);
  a.dgamma = a.dbeta + a.C;
  hipLaunchKernelGGL(float_sums_kernel, channel_grid(a.C), dim3(kThreads), 0, w.st, sums, a.dbeta, a.C);
  launch_backward_apply(a, w, (float)(1.0 / count));
  return (int)hipGetLastError();
}
