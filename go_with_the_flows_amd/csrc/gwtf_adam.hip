// gwtf_adam.hip -- fused optimiser step of the reference's custom Adam / AMSGrad (lib/networks/optimizers.py:15-76):
//     m = b1 m + (1-b1) g        v = b2 v + (1-b2) g^2        [vmax = max(vmax, v)]
//     p -= wd * p + lr * (m / (1 - b1^t)) / (sqrt(v or vmax) / sqrt(1 - b2^t) + eps)      (decay NOT scaled by lr: :69-72)
// The reference loops over parameters in Python (~12 tiny launches per tensor, ~1500 tensors per model).  Here one
// launch updates up to 48 tensors: their pointers ride in the kernel arguments (no allocation, no table upload), each
// workgroup owns a 4096-element chunk, float4 streams.  Pure HBM streaming: 28 (Adam) / 36 (AMSGrad) bytes per element.
#include <hip/hip_runtime.h>
#include "../../include/gwtf.h"

namespace {

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));     // 16 bytes at any dword address

constexpr int kMaxT = 48;
constexpr int kChunk = 4096;

struct AdamTable {
  float* p[kMaxT];
  const float* g[kMaxT];
  float* m[kMaxT];
  float* v[kMaxT];
  float* vmax[kMaxT];
  unsigned long long n[kMaxT];
  int chunk_start[kMaxT + 1];   // prefix sum of chunks per tensor
  int count;
};

// One 4096-element chunk of one tensor: the update every kernel of this file runs, written ONCE.  A macro and not an inlined
// function: the pointer-argument and the table kernel must keep the code the compiler gave them before the device-driven launch
// existed, and only the same tokens in the same place guarantee that (a force-inlined function moved adam_kernel's blocks).
// It reads, from the scope it is expanded in: AMS; p, g, m, v, vm; n, base; lr, b1, b2, omb1, omb2, eps, wd, bc1, bc2s.
//   - 1-beta is computed in double on the host, like the reference's Python scalars
//   - 16-byte accesses need p / m / v / vmax on 16-byte boundaries (torch allocations: always).  The GRADIENT does not: the decoders'
//     .grad tensors are views of one flat arena gradient at odd float offsets (flows._ArenaCat, dist.OverlappedGradients.finish), and
//     a global_load_dwordx4 only needs dword alignment -- g is read through a 4-byte-aligned vector type (with g in this
//     test ~3.7 M of the airplane model's 4.8 M parameters took the scalar path)
#define GWTF_ADAM_CHUNK()                                                                                                              \
  auto upd = [&](float& pp, float gg, float& mm, float& vv, float& vx) {                                                               \
    mm = mm * b1 + omb1 * gg;                                                                                                          \
    vv = vv * b2 + omb2 * gg * gg;                                                                                                     \
    float den;                                                                                                                         \
    if (AMS) {                                                                                                                         \
      vx = fmaxf(vx, vv);                                                                                                              \
      den = sqrtf(vx);                                                                                                                 \
    } else {                                                                                                                           \
      den = sqrtf(vv);                                                                                                                 \
    }                                                                                                                                  \
    const float step = (mm / bc1) / (den / bc2s + eps);                                                                                \
    pp = pp - (pp * wd + lr * step);                                                                                                   \
  };                                                                                                                                   \
  const bool vec = (((size_t)p | (size_t)m | (size_t)v | (size_t)(AMS ? vm : p)) & 15) == 0;                                           \
  for (size_t i = base + (size_t)threadIdx.x * 4; i < base + kChunk && i < n; i += 256 * 4) {                                          \
    if (vec && i + 4 <= n) {                                                                                                           \
      float4 pp = *reinterpret_cast<float4*>(p + i), mm = *reinterpret_cast<float4*>(m + i), vv = *reinterpret_cast<float4*>(v + i);   \
      const f4u gg = *reinterpret_cast<const f4u*>(g + i);                                                                             \
      float4 vx = AMS ? *reinterpret_cast<float4*>(vm + i) : make_float4(0.f, 0.f, 0.f, 0.f);                                          \
      upd(pp.x, gg.x, mm.x, vv.x, vx.x);                                                                                               \
      upd(pp.y, gg.y, mm.y, vv.y, vx.y);                                                                                               \
      upd(pp.z, gg.z, mm.z, vv.z, vx.z);                                                                                               \
      upd(pp.w, gg.w, mm.w, vv.w, vx.w);                                                                                               \
      *reinterpret_cast<float4*>(p + i) = pp;                                                                                          \
      *reinterpret_cast<float4*>(m + i) = mm;                                                                                          \
      *reinterpret_cast<float4*>(v + i) = vv;                                                                                          \
      if (AMS) *reinterpret_cast<float4*>(vm + i) = vx;                                                                                \
    } else {                                                                                                                           \
      for (size_t k = i; k < i + 4 && k < n; ++k) {                                                                                    \
        float pp = p[k], mm = m[k], vv = v[k], vx = AMS ? vm[k] : 0.f;                                                                 \
        upd(pp, g[k], mm, vv, vx);                                                                                                     \
        p[k] = pp; m[k] = mm; v[k] = vv;                                                                                               \
        if (AMS) vm[k] = vx;                                                                                                           \
      }                                                                                                                                \
    }                                                                                                                                  \
  }

template <bool AMS>
__global__ __launch_bounds__(256) void adam_kernel(const AdamTable t, float lr, float b1, float b2, float omb1, float omb2,
                                                   float eps, float wd, float bc1, float bc2s) {
  int ti = 0;
  while (ti + 1 < t.count && (int)blockIdx.x >= t.chunk_start[ti + 1]) ++ti;
  const size_t base = (size_t)(blockIdx.x - t.chunk_start[ti]) * kChunk;
  const size_t n = t.n[ti];
  float* __restrict__ p = t.p[ti];
  const float* __restrict__ g = t.g[ti];
  float* __restrict__ m = t.m[ti];
  float* __restrict__ v = t.v[ti];
  float* __restrict__ vm = t.vmax[ti];
  GWTF_ADAM_CHUNK()
}

// Any number of tensors in ONE launch: the pointer table lives in device memory (a model has ~1200 parameter tensors, most
// of them a few dozen floats: 25 dependent 48-tensor launches cost 13 us each, one table launch streams at HBM rate).
//   table [n_tensors][5] u64 = {param, exp_avg, exp_avg_sq, max_exp_avg_sq or 0, numel}     grads [n_tensors] u64
//   chunk_map [n_chunks][2] i32 = {tensor index, chunk index within the tensor}
template <bool AMS>
__global__ __launch_bounds__(256) void adam_table_kernel(const unsigned long long* __restrict__ table,
                                                         const unsigned long long* __restrict__ grads,
                                                         const int* __restrict__ chunk_map, float lr, float b1, float b2,
                                                         float omb1, float omb2, float eps, float wd, float bc1, float bc2s) {
  const int ti = chunk_map[2 * blockIdx.x];
  const size_t base = (size_t)chunk_map[2 * blockIdx.x + 1] * kChunk;
  const unsigned long long* row = table + (size_t)ti * 5;
  float* __restrict__ p = reinterpret_cast<float*>(row[0]);
  float* __restrict__ m = reinterpret_cast<float*>(row[1]);
  float* __restrict__ v = reinterpret_cast<float*>(row[2]);
  float* __restrict__ vm = reinterpret_cast<float*>(row[3]);
  const size_t n = row[4];
  const float* __restrict__ g = reinterpret_cast<const float*>(grads[ti]);
  GWTF_ADAM_CHUNK()
}

// The table kernel driven from device memory (the resident training loop, gwtf_loop.hip): the seven scalars of the update come from
// the record `hyper` (gwtf_adam_hyper's layout), and a set `*skip` ends every workgroup before it touches anything -- the NaN guard
// and the end of an epoch inside a captured graph.
template <bool AMS>
__global__ __launch_bounds__(256) void adam_table_dev_kernel(const unsigned long long* __restrict__ table,
                                                             const unsigned long long* __restrict__ grads,
                                                             const int* __restrict__ chunk_map, const float* __restrict__ hyper,
                                                             const int* __restrict__ skip, float eps, float wd) {
  if (*skip != 0) return;
  const int ti = chunk_map[2 * blockIdx.x];
  const size_t base = (size_t)chunk_map[2 * blockIdx.x + 1] * kChunk;
  const unsigned long long* row = table + (size_t)ti * 5;
  float* __restrict__ p = reinterpret_cast<float*>(row[0]);
  float* __restrict__ m = reinterpret_cast<float*>(row[1]);
  float* __restrict__ v = reinterpret_cast<float*>(row[2]);
  float* __restrict__ vm = reinterpret_cast<float*>(row[3]);
  const size_t n = row[4];
  const float* __restrict__ g = reinterpret_cast<const float*>(grads[ti]);
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], omb1 = hyper[3], omb2 = hyper[4], bc1 = hyper[5], bc2s = hyper[6];
  GWTF_ADAM_CHUNK()
}

// The scalars of the update with step count `step`, each formed in double and cast to float once (the reference's Python scalars).
struct AdamHyper { float lr, b1, b2, omb1, omb2, bc1, bc2s; };
static AdamHyper adam_hyper(double lr, double beta1, double beta2, int step) {
  AdamHyper h;
  h.lr = (float)lr; h.b1 = (float)beta1; h.b2 = (float)beta2;
  h.omb1 = (float)(1.0 - (double)beta1); h.omb2 = (float)(1.0 - (double)beta2);
  h.bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  h.bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  return h;
}

}  // namespace

// Table variant of gwtf_adam_step (layouts above; all three arrays in DEVICE memory, built by the caller once per set of
// tensors -- only `grads` changes from step to step).  gwtf_adam_chunk_elems() is the chunk size the map must use.
extern "C" int gwtf_adam_chunk_elems(void) { return kChunk; }

extern "C" int gwtf_adam_step_table(const unsigned long long* table, const unsigned long long* grads, const int* chunk_map,
                                    int n_chunks, float lr, double beta1, double beta2, float eps, float weight_decay,
                                    int step, int amsgrad, void* stream) {
  if (!table || !grads || !chunk_map || n_chunks < 0 || step < 1) return GWTF_E_BADARG;
  if (n_chunks == 0) return 0;
  const AdamHyper h = adam_hyper((double)lr, beta1, beta2, step);
  hipStream_t st = (hipStream_t)stream;
  if (amsgrad) hipLaunchKernelGGL(adam_table_kernel<true>, dim3(n_chunks), dim3(256), 0, st, table, grads, chunk_map, h.lr, h.b1, h.b2, h.omb1, h.omb2, eps, weight_decay, h.bc1, h.bc2s);
  else hipLaunchKernelGGL(adam_table_kernel<false>, dim3(n_chunks), dim3(256), 0, st, table, grads, chunk_map, h.lr, h.b1, h.b2, h.omb1, h.omb2, eps, weight_decay, h.bc1, h.bc2s);
  return (int)hipGetLastError();
}

extern "C" int gwtf_adam_hyper(double lr, double beta1, double beta2, int step, float* out8) {
  if (!out8 || step < 1) return GWTF_E_BADARG;
  const AdamHyper h = adam_hyper(lr, beta1, beta2, step);
  out8[0] = h.lr; out8[1] = h.b1; out8[2] = h.b2; out8[3] = h.omb1; out8[4] = h.omb2; out8[5] = h.bc1; out8[6] = h.bc2s; out8[7] = 0.f;
  return 0;
}

extern "C" int gwtf_adam_step_table_dev(const unsigned long long* table, const unsigned long long* grads, const int* chunk_map,
                                        int n_chunks, const float* hyper, const int* skip, float eps, float weight_decay,
                                        int amsgrad, void* stream) {
  if (!table || !grads || !chunk_map || !hyper || !skip || n_chunks < 0) return GWTF_E_BADARG;
  if (n_chunks == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (amsgrad) hipLaunchKernelGGL(adam_table_dev_kernel<true>, dim3(n_chunks), dim3(256), 0, st, table, grads, chunk_map, hyper, skip, eps, weight_decay);
  else hipLaunchKernelGGL(adam_table_dev_kernel<false>, dim3(n_chunks), dim3(256), 0, st, table, grads, chunk_map, hyper, skip, eps, weight_decay);
  return (int)hipGetLastError();
}

// Host arrays of n_tensors device pointers (max_exp_avg_sq may be NULL when amsgrad == 0).  `step` is the 1-based step
// count AFTER this update (the reference increments before using it, optimizers.py:47).
extern "C" int gwtf_adam_step(float* const* params, const float* const* grads, float* const* exp_avg,
                              float* const* exp_avg_sq, float* const* max_exp_avg_sq, const size_t* numel, int n_tensors,
                              float lr, double beta1, double beta2, float eps, float weight_decay, int step, int amsgrad,
                              void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !numel || n_tensors < 0 || step < 1 || (amsgrad && !max_exp_avg_sq))
    return GWTF_E_BADARG;
  const AdamHyper h = adam_hyper((double)lr, beta1, beta2, step);
  hipStream_t st = (hipStream_t)stream;
  int i = 0;
  while (i < n_tensors) {
    AdamTable t;
    t.count = 0;
    t.chunk_start[0] = 0;
    while (i < n_tensors && t.count < kMaxT) {
      if (numel[i] > 0) {
        if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || (amsgrad && !max_exp_avg_sq[i])) return GWTF_E_BADARG;
        const int k = t.count++;
        t.p[k] = params[i]; t.g[k] = grads[i]; t.m[k] = exp_avg[i]; t.v[k] = exp_avg_sq[i];
        t.vmax[k] = amsgrad ? max_exp_avg_sq[i] : nullptr;
        t.n[k] = numel[i];
        t.chunk_start[k + 1] = t.chunk_start[k] + (int)((numel[i] + kChunk - 1) / kChunk);
      }
      ++i;
    }
    if (t.count == 0) continue;
    const dim3 grid((unsigned)t.chunk_start[t.count]);
    if (amsgrad) hipLaunchKernelGGL(adam_kernel<true>, grid, dim3(256), 0, st, t, h.lr, h.b1, h.b2, h.omb1, h.omb2, eps, weight_decay, h.bc1, h.bc2s);
    else hipLaunchKernelGGL(adam_kernel<false>, grid, dim3(256), 0, st, t, h.lr, h.b1, h.b2, h.omb1, h.omb2, eps, weight_decay, h.bc1, h.bc2s);
  }
  return (int)hipGetLastError();
}
