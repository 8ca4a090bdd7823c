// gwtf_assign.hip -- the inference direction of the mixture at the level of a point: for every observed point the responsibility
// r_k(n) = softmax_k(log w_k + log p_k(x_n | z)) of every component, and what follows from it (label, confidence, log-density,
// per-shape component counts, the contingency table against ground-truth parts).  Record and rules: include/gwtf.h (GwtfAssignArgs).
//
// Reference: the per-component body of FlowMixtureNLL.forward, lib/networks/losses.py:101-122 -- the lp_k of nll_kernel
// (gwtf_nll.hip), in the same expression and order, with its `log(exp(logit)) - logsumexp` weight:
//     lp_k = -0.5 * sum_d [ lv0 + logdet + (z - mu0)^2 / exp(lv0) ] - 0.5 * 3 * log(2 pi) + log w_bk
//
// assign_kernel: one workgroup of kThreads per (shape, kPtsPerBlock points), streaming: 24 K bytes per point read, coalesced along N.
//   load      N a multiple of 4 and every per-point base 16-byte aligned: one thread takes 4 consecutive points and reads each of the
//             6 K rows as one 16-byte load (every row then starts on a 16-byte boundary and no row has a tail); otherwise one thread
//             takes one point per round, float by float.  Both run the same arithmetic per point: the same values give the same bits
//   reduce    an online log-sum-exp over k that also carries the running best (lp, k): a strictly greater lp replaces the best, so an
//             exact tie stays with the lowest k.  NaN and -inf as in nll_kernel (read its comment): a component at -inf is skipped, a
//             NaN is caught on the bits of lp.  The point is INVALID (label -1) when its log-density is not finite -- a NaN anywhere in
//             its lp_k, every component at -inf, or an lp of +inf -- which is again told by the bits
//   resp      only when asked for: a second pass over k recomputes lp_k (the same expression: resp of the label IS the confidence, bit
//             for bit) and writes exp(lp_k - log_density); without it z and logdet are read exactly once
//   count     one LDS atomic per point into the workgroup's K bins and, with parts, into its K x P table (<= 4096 ints)
//   flush     every non-zero LDS bin: one INTEGER global atomic (int32 for counts / invalid, 64-bit for table / skipped)
// No float atomics anywhere: the same inputs give the same bits on every call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/gwtf.h"

namespace {

constexpr int kMaxK = 64;
constexpr int kMaxP = 64;
constexpr int kThreads = 128;
constexpr int kPtsPerBlock = 512;     // 4 points per thread; 64 x 2048 points are 256 workgroups, one per CU

struct AssignParams {
  const float* z;
  const float* logdet;
  const float* mu0;
  const float* lv0;
  const float* logits;
  const int* parts;
  float* log_density;
  int* labels;
  float* confidence;
  float* resp;
  int* counts;
  int* invalid;
  unsigned long long* table;
  unsigned long long* skipped;
  int K, B, N, P;
  int blocks_per_shape;
};

struct Shared {
  float logw[kMaxK];
  float mu[kMaxK][3], lv[kMaxK][3], iv[kMaxK][3];
  int counts[kMaxK];
  int invalid, skipped;
  int table[kMaxK * kMaxP];
};

template <int V> __device__ inline void load_f(const float* p, float (&v)[V]);
template <> __device__ inline void load_f<1>(const float* p, float (&v)[1]) { v[0] = *p; }
template <> __device__ inline void load_f<4>(const float* p, float (&v)[4]) {
  const float4 q = *reinterpret_cast<const float4*>(p);
  v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
template <int V> __device__ inline void load_i(const int* p, int (&v)[V]);
template <> __device__ inline void load_i<1>(const int* p, int (&v)[1]) { v[0] = *p; }
template <> __device__ inline void load_i<4>(const int* p, int (&v)[4]) {
  const int4 q = *reinterpret_cast<const int4*>(p);
  v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
template <int V> __device__ inline void store_f(float* p, const float (&v)[V]);
template <> __device__ inline void store_f<1>(float* p, const float (&v)[1]) { *p = v[0]; }
template <> __device__ inline void store_f<4>(float* p, const float (&v)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <int V> __device__ inline void store_i(int* p, const int (&v)[V]);
template <> __device__ inline void store_i<1>(int* p, const int (&v)[1]) { *p = v[0]; }
template <> __device__ inline void store_i<4>(int* p, const int (&v)[4]) {
  *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]);
}

// lp_k of V consecutive points of shape b starting at n: nll_kernel's expression, term by term.
template <int V>
__device__ inline void component_lp(const AssignParams& a, const Shared& sh, int k, int b, int n, float (&lp)[V]) {
  float qsum[V];
#pragma unroll
  for (int i = 0; i < V; ++i) qsum[i] = 0.f;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const size_t o = (((size_t)k * a.B + b) * 3 + d) * a.N + n;
    float zv[V], ld[V];
    load_f<V>(a.z + o, zv);
    load_f<V>(a.logdet + o, ld);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float diff = zv[i] - sh.mu[k][d];
      qsum[i] += (sh.lv[k][d] + ld[i]) + diff * diff * sh.iv[k][d];
    }
  }
  const float half_log2pi3 = 0.5f * 3.0f * 1.8378770664093453f;
#pragma unroll
  for (int i = 0; i < V; ++i) lp[i] = -0.5f * qsum[i] - half_log2pi3 + sh.logw[k];
}

template <int V>
__device__ inline void assign_points(const AssignParams& a, Shared& sh, int b, int n) {
  const int K = a.K;
  // The library is built with -fno-honor-nans: infinities are honoured, NaN is not, and a test on the bits of a value that comes out
  // of no-NaN arithmetic would be folded away -- the empty statement below emits no instruction, it only makes the value opaque to
  // the optimiser (nll_kernel's comment, gwtf_nll.hip).
  float m[V], s[V];
  int best[V];
  bool nan_seen[V];
#pragma unroll
  for (int i = 0; i < V; ++i) { m[i] = -INFINITY; s[i] = 0.f; best[i] = 0; nan_seen[i] = false; }
  for (int k = 0; k < K; ++k) {
    float lp[V];
    component_lp<V>(a, sh, k, b, n, lp);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float v = lp[i];
      asm volatile("" : "+v"(v));
      nan_seen[i] |= (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u;
      if (v == -INFINITY) continue;
      if (v > m[i] || k == 0) {                      // strictly greater: an exact tie keeps the lower k
        s[i] = s[i] * expf(m[i] - v) + 1.0f;
        m[i] = v;
        best[i] = k;
      } else {
        s[i] += expf(v - m[i]);
      }
    }
  }
  float lse[V], conf[V];
  int label[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    float l = m[i] + logf(s[i]);
    asm volatile("" : "+v"(l));
    const bool finite = (__float_as_uint(l) & 0x7f800000u) != 0x7f800000u;
    const bool valid = finite && !nan_seen[i];
    lse[i] = nan_seen[i] ? __uint_as_float(0x7fc00000u) : l;
    label[i] = valid ? best[i] : -1;
    conf[i] = valid ? expf(m[i] - l) : 0.f;
  }
  const size_t at = (size_t)b * a.N + n;
  store_f<V>(a.log_density + at, lse);
  store_i<V>(a.labels + at, label);
  if (a.confidence) store_f<V>(a.confidence + at, conf);
  if (a.resp) {
    for (int k = 0; k < K; ++k) {
      float lp[V], r[V];
      component_lp<V>(a, sh, k, b, n, lp);
#pragma unroll
      for (int i = 0; i < V; ++i) r[i] = label[i] < 0 ? __uint_as_float(0x7fc00000u) : expf(lp[i] - lse[i]);
      store_f<V>(a.resp + ((size_t)b * K + k) * a.N + n, r);
    }
  }
  int part[V];
  if (a.parts) load_i<V>(a.parts + at, part);
#pragma unroll
  for (int i = 0; i < V; ++i) {
    if (label[i] < 0) {
      atomicAdd(&sh.invalid, 1);
    } else if (a.counts) {
      atomicAdd(&sh.counts[label[i]], 1);
    }
    if (a.parts) {
      if (label[i] >= 0 && part[i] >= 0 && part[i] < a.P) atomicAdd(&sh.table[label[i] * a.P + part[i]], 1);
      else atomicAdd(&sh.skipped, 1);
    }
  }
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void assign_kernel(AssignParams a) {
  __shared__ Shared sh;
  const int K = a.K, B = a.B, N = a.N;
  const int b = blockIdx.x / a.blocks_per_shape;
  const int chunk = blockIdx.x - b * a.blocks_per_shape;
  const int tid = threadIdx.x;
  if (tid < 64) {
    // log w = log(exp(logit)) - logsumexp(logits)   (losses.py:101-104)
    float mx = -INFINITY;
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, a.logits[(size_t)b * K + k]);
    float sum = 0.f;
    for (int k = 0; k < K; ++k) sum += expf(a.logits[(size_t)b * K + k] - mx);
    const float lse = mx + logf(sum);
    for (int k = tid; k < K; k += 64) sh.logw[k] = logf(expf(a.logits[(size_t)b * K + k])) - lse;
  }
  for (int t = tid; t < K * 3; t += kThreads) {
    const int k = t / 3, d = t % 3;
    const float l = a.lv0[((size_t)k * B + b) * 3 + d];
    sh.mu[k][d] = a.mu0[((size_t)k * B + b) * 3 + d];
    sh.lv[k][d] = l;
    sh.iv[k][d] = 1.0f / expf(l);       // the points multiply by 1/exp(lv0), as in nll_kernel
  }
  for (int t = tid; t < K; t += kThreads) sh.counts[t] = 0;
  if (tid == 0) { sh.invalid = 0; sh.skipped = 0; }
  if (a.parts)
    for (int t = tid; t < K * a.P; t += kThreads) sh.table[t] = 0;
  __syncthreads();

  const int n_begin = chunk * kPtsPerBlock;
  const int n_end = min(N, n_begin + kPtsPerBlock);
  if (kVec) {                                                  // N % 4 == 0: a group of 4 is inside [0, N) whole or not at all
    const int n = n_begin + 4 * tid;
    if (n < n_end) assign_points<4>(a, sh, b, n);
  } else {
    for (int n = n_begin + tid; n < n_end; n += kThreads) assign_points<1>(a, sh, b, n);
  }
  __syncthreads();

  if (a.counts)
    for (int t = tid; t < K; t += kThreads)
      if (sh.counts[t]) atomicAdd(&a.counts[(size_t)b * K + t], sh.counts[t]);
  if (a.parts)
    for (int t = tid; t < K * a.P; t += kThreads)
      if (sh.table[t]) atomicAdd(&a.table[t], (unsigned long long)sh.table[t]);
  if (tid == 0) {
    if (a.invalid && sh.invalid) atomicAdd(&a.invalid[b], sh.invalid);
    if (a.skipped && sh.skipped) atomicAdd(a.skipped, (unsigned long long)sh.skipped);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int gwtf_mixture_assign(const GwtfAssignArgs* pa) {
  if (!pa) return GWTF_E_BADARG;
  const GwtfAssignArgs& g = *pa;
  if (!g.z || !g.logdet || !g.mu0 || !g.lv0 || !g.logits || !g.log_density || !g.labels) return GWTF_E_BADARG;
  if (g.K < 1 || g.K > kMaxK || g.B < 1 || g.N < 1) return GWTF_E_BADARG;
  if (g.parts && (g.P < 1 || g.P > kMaxP || !g.table)) return GWTF_E_BADARG;
  const long long per_shape = ((long long)g.N + kPtsPerBlock - 1) / kPtsPerBlock;
  if (per_shape * g.B > 0x7fffffffll) return GWTF_E_UNSUPPORTED;
  AssignParams a;
  a.z = g.z; a.logdet = g.logdet; a.mu0 = g.mu0; a.lv0 = g.lv0; a.logits = g.logits;
  a.parts = g.parts;
  a.log_density = g.log_density; a.labels = g.labels; a.confidence = g.confidence; a.resp = g.resp;
  a.counts = g.counts; a.invalid = g.invalid;
  a.table = g.parts ? reinterpret_cast<unsigned long long*>(g.table) : nullptr;
  a.skipped = g.parts ? reinterpret_cast<unsigned long long*>(g.skipped) : nullptr;
  a.K = g.K; a.B = g.B; a.N = g.N; a.P = g.parts ? g.P : 0;
  a.blocks_per_shape = (int)per_shape;
  hipStream_t st = (hipStream_t)g.stream;
  hipError_t e = hipSuccess;
  if (g.counts) e = hipMemsetAsync(g.counts, 0, sizeof(int) * (size_t)g.B * g.K, st);
  if (e == hipSuccess && g.invalid) e = hipMemsetAsync(g.invalid, 0, sizeof(int) * (size_t)g.B, st);
  if (e != hipSuccess) return (int)e;
  // rows of z / logdet / resp start at multiples of N floats behind their bases, the per-point outputs at multiples of N
  const bool vec = g.N % 4 == 0 && aligned16(g.z) && aligned16(g.logdet) && aligned16(g.log_density) && aligned16(g.labels) &&
                   aligned16(g.confidence) && aligned16(g.resp) && aligned16(g.parts);
  const dim3 grid((unsigned)(per_shape * g.B));
  if (vec) hipLaunchKernelGGL(assign_kernel<true>, grid, dim3(kThreads), 0, st, a);
  else hipLaunchKernelGGL(assign_kernel<false>, grid, dim3(kThreads), 0, st, a);
  return (int)hipGetLastError();
}
