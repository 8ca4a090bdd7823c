// gwtf_clouds.hip -- training batches drawn on the device: area-weighted points on the faces of packed triangle meshes, the cloud
// transformations fused behind them (reference lib/datasets/cloud_sampling.py:4-32, cloud_transformations.py:6-103, and the loader
// around them, lib/datasets/datasets.py:69-106).
//
// One sampling launch, grid (point chunks, B) x 256 threads: the threads of a workgroup share one shape.  Per point
//   face   = #{k < n : T[k] <= w}      the 32-bit word w against the shape's integer thresholds T[k] = ceil(cdf[k] * 2^32); n counts
//                                      the thresholds below 2^32, so the count never passes the last face with area (include/gwtf.h)
//   point  = (v0 + s1 (v1 - v0)) + s2 (v2 - v0)    float32, in this order, uncontracted (-ffp-contract=off): the reference's bits
// The search is a chain of dependent loads.  Its top levels run in LDS: every 2^ls-th threshold of the shape (at most kTop of
// them) is staged once per workgroup, the remaining ls levels are read through L2.
// Sums for CenterCloud are taken per TILE of 256 consecutive points in a fixed tree (wave butterfly, then the four waves in order)
// and stored, never added atomically; the finishing launch sums a row's tiles in a fixed order and subtracts.  A tile is 256 points
// whatever the chunk a workgroup walks, so the result does not depend on the tuning word.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/gwtf.h"
#include "gwtf_philox.h"

namespace {

using namespace gwtf_rng;

constexpr int kThreads = 256;      // one tile of points
constexpr int kTop = 1024;         // staged thresholds (4 KiB of LDS)
constexpr int kChunkDefault = 1024, kChunkMax = 8192;

constexpr uint32_t kNanBits = 0x7fc00000u;

__global__ __launch_bounds__(kThreads) void cloud_sample_kernel(GwtfCloudArgs a, int chunk, int tiles) {
  __shared__ uint32_t top[kTop];
  __shared__ float wave_sums[4][6];
  const int r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = a.M, N = a.eval_cloud ? M / 2 : M;
  const int shape = a.rows[r];
  const bool known = shape >= 0 && shape < a.n_shapes;       // a row outside the store: NaN points, nothing is read
  const long long fb = known ? a.faces_bounds[shape] : 0, vb = known ? a.vertices_bounds[shape] : 0;
  const int n = known ? a.search_len[shape] : 0;
  int ls = 0;
  while ((n >> ls) > kTop) ++ls;
  const int nc = n >> ls;                                     // staged: the last threshold of every full block of 2^ls
  const uint32_t* __restrict__ T = a.thresholds + fb;
  for (int i = tid; i < nc; i += kThreads) top[i] = T[(((long long)i + 1) << ls) - 1];
  __syncthreads();

  const unsigned long long seed = a.state[0], call = a.state[1];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), c2 = (uint32_t)call, c3 = (uint32_t)(call >> 32);
  float os = 1.f, oc[3] = {0.f, 0.f, 0.f};
  if (known && a.rescale) os = a.orig_s[shape];
  if (known && a.recenter) { oc[0] = a.orig_c[shape * 3]; oc[1] = a.orig_c[shape * 3 + 1]; oc[2] = a.orig_c[shape * 3 + 2]; }

  const int j0 = blockIdx.x * chunk;
  for (int jt = j0; jt < j0 + chunk && jt < M; jt += kThreads) {
    const int j = jt + tid;
    const bool live = j < M;
    float p[3] = {0.f, 0.f, 0.f};
    if (live) {
      const size_t e = (size_t)r * M + j;
      uint32_t w;
      float s1, s2;
      if (a.words) {
        w = a.words[e]; s1 = a.s1[e]; s2 = a.s2[e];
      } else {
        const Philox4 d = philox4x32_10((uint32_t)j, (uint32_t)r, c2, c3, k0, k1);
        w = d.x; s1 = (float)(d.y >> 8) * 0x1p-24f; s2 = (float)(d.z >> 8) * 0x1p-24f;
      }
      if (known) {
        int lo = 0, hi = nc;
        while (lo < hi) {                                     // LDS levels
          const int mid = (lo + hi) >> 1;
          if (top[mid] <= w) lo = mid + 1; else hi = mid;
        }
        // blocks [0, lo) lie at or below w; block lo ends above it (or is the short tail)
        lo <<= ls;
        hi = min(lo + (1 << ls) - (lo < (nc << ls) ? 1 : 0), n);
        while (lo < hi) {                                     // L2 levels
          const int mid = (lo + hi) >> 1;
          if (T[mid] <= w) lo = mid + 1; else hi = mid;
        }
        const int* fv = a.faces + (fb + lo) * 3;
        const float* v0 = a.vertices + (vb + fv[0]) * 3;
        const float* v1 = a.vertices + (vb + fv[1]) * 3;
        const float* v2 = a.vertices + (vb + fv[2]) * 3;
        if (s1 + s2 > 1.0f) { s1 = 1.0f - s1; s2 = 1.0f - s2; }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float e1 = v1[c] - v0[c], e2 = v2[c] - v0[c];
          p[c] = (v0[c] + s1 * e1) + s2 * e2;
        }
      }
      if (a.rescale) { p[0] = os * p[0]; p[1] = os * p[1]; p[2] = os * p[2]; }
      if (a.recenter) { p[0] = p[0] + oc[0]; p[1] = p[1] + oc[1]; p[2] = p[2] + oc[2]; }
      if (a.translate) { p[0] = p[0] - a.shift[0]; p[1] = p[1] - a.shift[1]; p[2] = p[2] - a.shift[2]; }
      if (a.scale) { p[0] = p[0] / a.scale_div; p[1] = p[1] / a.scale_div; p[2] = p[2] / a.scale_div; }
      if (a.noise) {
        float z[4];
        if (a.words) {
          const size_t eb = (size_t)r * 3 * M + j;
          z[0] = a.normals[eb]; z[1] = a.normals[eb + M]; z[2] = a.normals[eb + 2 * (size_t)M];
        } else {
          const Philox4 d = philox4x32_10((uint32_t)j, (uint32_t)r, c2, c3 | (1u << 28), k0, k1);
          box_muller(d.x, d.y, z[0], z[1]);
          box_muller(d.z, d.w, z[2], z[3]);
        }
        p[0] = p[0] + a.noise_scale * z[0]; p[1] = p[1] + a.noise_scale * z[1]; p[2] = p[2] + a.noise_scale * z[2];
      }
      float* dst = a.cloud;
      int col = j;
      if (a.eval_cloud) { dst = (j & 1) ? a.eval_cloud : a.cloud; col = j >> 1; }
      dst += (size_t)r * 3 * N + col;
      if (known) {
        dst[0] = p[0]; dst[N] = p[1]; dst[2 * (size_t)N] = p[2];
      } else {                                                // as bits: the library is built to assume NaN-free arithmetic
        uint32_t* bits = reinterpret_cast<uint32_t*>(dst);
        bits[0] = kNanBits; bits[N] = kNanBits; bits[2 * (size_t)N] = kNanBits;
      }
    }
    if (a.center) {                                           // uniform: every lane takes part, a dead lane adds 0
      float s[3] = {p[0], p[1], p[2]};
#pragma unroll
      for (int off = 32; off >= 2; off >>= 1) {
        s[0] += __shfl_xor(s[0], off); s[1] += __shfl_xor(s[1], off); s[2] += __shfl_xor(s[2], off);
      }
      // lane 0: the even points, lane 1: the odd ones.  Without an eval cloud both belong to `cloud`.
      const float o0 = __shfl_xor(s[0], 1), o1 = __shfl_xor(s[1], 1), o2 = __shfl_xor(s[2], 1);
      if (!a.eval_cloud) { s[0] += o0; s[1] += o1; s[2] += o2; }
      if (lane < 2 && (lane == 0 || a.eval_cloud)) {
        wave_sums[wave][lane * 3] = s[0]; wave_sums[wave][lane * 3 + 1] = s[1]; wave_sums[wave][lane * 3 + 2] = s[2];
      } else if (lane == 1) {
        wave_sums[wave][3] = 0.f; wave_sums[wave][4] = 0.f; wave_sums[wave][5] = 0.f;
      }
      __syncthreads();
      if (tid < 6)
        a.partials[((size_t)r * tiles + jt / kThreads) * 6 + tid] =
            ((wave_sums[0][tid] + wave_sums[1][tid]) + wave_sums[2][tid]) + wave_sums[3][tid];
      __syncthreads();
    }
  }
}

// Finishing launch: subtracts each cloud's mean (CenterCloud) and advances the call word.  grid (slices of the columns, B); with
// centring off it is one thread.  Every workgroup of a row sums the row's tiles itself, in the same fixed order.
__global__ __launch_bounds__(kThreads) void cloud_finish_kernel(GwtfCloudArgs a, int tiles) {
  __shared__ float mean[6];
  const int r = blockIdx.y, tid = threadIdx.x;
  const int shape = a.rows[r];
  if (a.center && shape >= 0 && shape < a.n_shapes) {       // a row outside the store keeps its NaN bits
    const int N = a.eval_cloud ? a.M / 2 : a.M;
    if (tid < 64) {
      float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int t = tid; t < tiles; t += 64) {
        const float* q = a.partials + ((size_t)r * tiles + t) * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] += q[k];
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] += __shfl_xor(s[k], off);
      }
      if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) mean[k] = s[k] / (float)N;
      }
    }
    __syncthreads();
    const int clouds = a.eval_cloud ? 2 : 1;
    for (int col = blockIdx.x * kThreads + tid; col < N; col += gridDim.x * kThreads) {
      for (int h = 0; h < clouds; ++h) {
        float* dst = (h ? a.eval_cloud : a.cloud) + (size_t)r * 3 * N + col;
        dst[0] = dst[0] - mean[h * 3]; dst[N] = dst[N] - mean[h * 3 + 1]; dst[2 * (size_t)N] = dst[2 * (size_t)N] - mean[h * 3 + 2];
      }
    }
  }
  // every sampling workgroup has finished reading the state (this launch follows it on the stream): the next call, or the next
  // replay of a captured graph, draws fresh points
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) a.state[1] = a.state[1] + 1ull;
}

int chunk_of(int tune) {
  int c = tune & 0xffff;
  if (c == 0) c = kChunkDefault;
  c = (c + kThreads - 1) / kThreads * kThreads;
  return c > kChunkMax ? kChunkMax : c;
}

}  // namespace

extern "C" int gwtf_cloud_partials(int M) { return M < 1 ? 0 : (M + kThreads - 1) / kThreads; }

extern "C" int gwtf_sample_clouds(const GwtfCloudArgs* pa) {
  if (!pa) return GWTF_E_BADARG;
  const GwtfCloudArgs& a = *pa;
  if (!a.rows || !a.vertices || !a.faces || !a.thresholds || !a.vertices_bounds || !a.faces_bounds || !a.search_len || !a.cloud ||
      !a.state)
    return GWTF_E_BADARG;
  if (a.B < 1 || a.B > 65535 || a.M < 1 || a.n_shapes < 1) return GWTF_E_BADARG;
  if (a.eval_cloud && (a.M & 1)) return GWTF_E_BADARG;
  if ((a.rescale && !a.orig_s) || (a.recenter && !a.orig_c) || (a.center && !a.partials)) return GWTF_E_BADARG;
  if (a.scale && !(a.scale_div > 0.f)) return GWTF_E_BADARG;
  if (a.noise && !(a.noise_scale > 0.f)) return GWTF_E_BADARG;
  if (a.words ? (!a.s1 || !a.s2 || (a.noise && !a.normals)) : (a.s1 || a.s2 || a.normals)) return GWTF_E_BADARG;
  const int chunk = chunk_of(a.tune), tiles = gwtf_cloud_partials(a.M);
  hipStream_t st = (hipStream_t)a.stream;
  hipLaunchKernelGGL(cloud_sample_kernel, dim3((a.M + chunk - 1) / chunk, a.B), dim3(kThreads), 0, st, a, chunk, tiles);
  const int N = a.eval_cloud ? a.M / 2 : a.M;
  const dim3 fg = a.center ? dim3(min((N + 4 * kThreads - 1) / (4 * kThreads), 64), a.B) : dim3(1, 1);
  hipLaunchKernelGGL(cloud_finish_kernel, fg, dim3(kThreads), 0, st, a, tiles);
  return (int)hipGetLastError();
}
