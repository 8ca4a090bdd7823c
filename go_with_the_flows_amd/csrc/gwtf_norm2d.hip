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

__global__ __launch_bounds__(kThreads) void finalize_forward_kernel(GwtfNorm2dArgs p, int S, double count) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= p.C) return;
  double s1 = 0.0, s2 = 0.0;
  for (int s = 0; s < S; ++s) { s1 += p.partials[((size_t)c * S + s) * 2]; s2 += p.partials[((size_t)c * S + s) * 2 + 1]; }
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

int check_sizes(int N, int C, int H, int W) {
  if (N < 1 || C < 1 || H < 1 || W < 1 || N > 65535) return GWTF_E_BADARG;
  const long long hw = (long long)H * W, nhw = (long long)N * hw, chw = (long long)C * hw;
  if (nhw >= (1LL << 31) - 4LL * kMaxSplit - kThreads * 4 || chw >= (1LL << 31) - kThreads * kQuads * 4) return GWTF_E_BADARG;
  if (nhw < 2) return GWTF_E_FEW_VALUES;
  return 0;
}

int check_common(const GwtfNorm2dArgs* pa) {
  if (!pa) return GWTF_E_BADARG;
  const GwtfNorm2dArgs& a = *pa;
  const int e = check_sizes(a.N, a.C, a.H, a.W);
  if (e) return e;
  if (!a.x || !a.gamma || !a.stats || !a.partials) return GWTF_E_BADARG;
  if (a.pool && (!a.relu || a.residual || a.d_residual || !a.offsets)) return GWTF_E_BADARG;
  if (!(a.eps >= 0.f) || !(a.momentum >= 0.f && a.momentum <= 1.f)) return GWTF_E_BADARG;
  return 0;
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15u) == 0; }

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
  hipStream_t st = (hipStream_t)a.stream;
  const unsigned hw = (unsigned)(a.H * a.W), nhw = (unsigned)a.N * hw, chw = (unsigned)a.C * hw;
  const int S = split_of(nhw, a.C);
  const unsigned per = ((nhw + S - 1) / S + 3u) & ~3u;
  const bool vec_x = hw % 4 == 0 && aligned16(a.x);
  const bool vec = vec_x && aligned16(a.y) && (!a.residual || aligned16(a.residual));
  if (vec_x) hipLaunchKernelGGL((partials_kernel<true, false, kPlain>), dim3(a.C, S), dim3(kThreads), 0, st, a, nhw, per);
  else hipLaunchKernelGGL((partials_kernel<false, false, kPlain>), dim3(a.C, S), dim3(kThreads), 0, st, a, nhw, per);
  hipLaunchKernelGGL(finalize_forward_kernel, dim3((a.C + kThreads - 1) / kThreads), dim3(kThreads), 0, st, a, S, (double)nhw);
  if (a.pool) {
    const unsigned cpool = (unsigned)a.C * pooled(a.H) * pooled(a.W);
    hipLaunchKernelGGL(apply_forward_pool_kernel, dim3((cpool + kThreads - 1) / kThreads, a.N), dim3(kThreads), 0, st, a, cpool);
    return (int)hipGetLastError();
  }
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
  return (int)hipGetLastError();
}

extern "C" int gwtf_norm2d_backward(const GwtfNorm2dArgs* pa) {
  const int bad = check_common(pa);
  if (bad) return bad;
  const GwtfNorm2dArgs& a = *pa;
  if (!a.dy || !a.dx || !a.dgamma || !a.dbeta) return GWTF_E_BADARG;
  if (a.relu && !a.pool && !a.y) return GWTF_E_BADARG;              // the mask is read from the saved output
  if (a.pool && !a.beta) return GWTF_E_BADARG;                      // the recomputation needs the forward's shift
  hipStream_t st = (hipStream_t)a.stream;
  const unsigned hw = (unsigned)(a.H * a.W), nhw = (unsigned)a.N * hw, chw = (unsigned)a.C * hw;
  const int S = split_of(nhw, a.C);
  const unsigned per = ((nhw + S - 1) / S + 3u) & ~3u;
  const int mode = a.pool ? kPool : (a.relu ? kMask : kPlain);
  // with pool a quad may run over a row's end into the next row (handled) but never over two: W >= 4
  bool vec = hw % 4 == 0 && aligned16(a.x) && aligned16(a.dx) && (!a.d_residual || aligned16(a.d_residual));
  if (mode == kPool) vec = vec && a.W >= 4;
  else vec = vec && aligned16(a.dy) && (mode != kMask || aligned16(a.y));
  const dim3 pgrid(a.C, S), block(kThreads);
#define GWTF_NORM2D_PART(V, M) hipLaunchKernelGGL((partials_kernel<V, true, M>), pgrid, block, 0, st, a, nhw, per)
  if (vec) { if (mode == kPool) GWTF_NORM2D_PART(true, kPool); else if (mode == kMask) GWTF_NORM2D_PART(true, kMask); else GWTF_NORM2D_PART(true, kPlain); }
  else { if (mode == kPool) GWTF_NORM2D_PART(false, kPool); else if (mode == kMask) GWTF_NORM2D_PART(false, kMask); else GWTF_NORM2D_PART(false, kPlain); }
#undef GWTF_NORM2D_PART
  hipLaunchKernelGGL(finalize_backward_kernel, dim3((a.C + kThreads - 1) / kThreads), block, 0, st, a, S);
  const unsigned tile = kThreads * kQuads * (vec ? 4 : 1);
  const dim3 grid((chw + tile - 1) / tile, a.N);
  const float inv_count = (float)(1.0 / (double)nhw);
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
  return (int)hipGetLastError();
}
