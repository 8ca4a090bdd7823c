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
#include "gwtf_perm.h"

namespace {

using namespace gwtf_rng;

constexpr int kThreads = 256;      // one tile of points
constexpr int kTop = 1024;         // staged thresholds (4 KiB of LDS)
constexpr int kChunkDefault = 1024, kChunkMax = 8192;

constexpr uint32_t kNanBits = 0x7fc00000u;

// Everything behind a sampled point, one body for both samplers (Args: GwtfCloudArgs or GwtfStoredCloudArgs, whose fields of these
// names mean the same): the transformations in ComposeCloudTransformation's order, each an uncontracted float32 statement, then the
// channel-major store -- even j to cloud, odd j to eval_cloud when there is one.  !known: the NaN bits, p keeps its value.
template <class Args>
__device__ __forceinline__ void transform_and_store(const Args& a, bool explicit_draws, bool known, int r, int j, int M, int N, float os,
                                                    const float (&oc)[3], uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                    float (&p)[3]) {
  if (a.rescale) { p[0] = os * p[0]; p[1] = os * p[1]; p[2] = os * p[2]; }
  if (a.recenter) { p[0] = p[0] + oc[0]; p[1] = p[1] + oc[1]; p[2] = p[2] + oc[2]; }
  if (a.translate) { p[0] = p[0] - a.shift[0]; p[1] = p[1] - a.shift[1]; p[2] = p[2] - a.shift[2]; }
  if (a.scale) { p[0] = p[0] / a.scale_div; p[1] = p[1] / a.scale_div; p[2] = p[2] / a.scale_div; }
  if (a.noise) {
    float z[4];
    if (explicit_draws) {
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
  } else {                                                    // as bits: the library is built to assume NaN-free arithmetic
    uint32_t* bits = reinterpret_cast<uint32_t*>(dst);
    bits[0] = kNanBits; bits[N] = kNanBits; bits[2 * (size_t)N] = kNanBits;
  }
}

// The sums of one tile of 256 points for CenterCloud, in a fixed tree (wave butterfly, then the four waves in order) -> tile[6]:
// the even points' sums, then the odd points' (zero without an eval cloud, where all belong to `cloud`).  Uniform: every thread of
// the workgroup calls it, a dead lane with p = 0.
__device__ __forceinline__ void tile_sums(const float (&p)[3], float (*wave_sums)[6], bool eval_cloud, float* tile, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  float s[3] = {p[0], p[1], p[2]};
#pragma unroll
  for (int off = 32; off >= 2; off >>= 1) {
    s[0] += __shfl_xor(s[0], off); s[1] += __shfl_xor(s[1], off); s[2] += __shfl_xor(s[2], off);
  }
  // lane 0: the even points, lane 1: the odd ones.  Without an eval cloud both belong to `cloud`.
  const float o0 = __shfl_xor(s[0], 1), o1 = __shfl_xor(s[1], 1), o2 = __shfl_xor(s[2], 1);
  if (!eval_cloud) { s[0] += o0; s[1] += o1; s[2] += o2; }
  if (lane < 2 && (lane == 0 || eval_cloud)) {
    wave_sums[wave][lane * 3] = s[0]; wave_sums[wave][lane * 3 + 1] = s[1]; wave_sums[wave][lane * 3 + 2] = s[2];
  } else if (lane == 1) {
    wave_sums[wave][3] = 0.f; wave_sums[wave][4] = 0.f; wave_sums[wave][5] = 0.f;
  }
  __syncthreads();
  if (tid < 6) tile[tid] = ((wave_sums[0][tid] + wave_sums[1][tid]) + wave_sums[2][tid]) + wave_sums[3][tid];
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void cloud_sample_kernel(GwtfCloudArgs a, int chunk, int tiles) {
  __shared__ uint32_t top[kTop];
  __shared__ float wave_sums[4][6];
  const int r = blockIdx.y, tid = threadIdx.x;
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
      transform_and_store(a, a.words != nullptr, known, r, j, M, N, os, oc, c2, c3, k0, k1, p);
    }
    if (a.center) tile_sums(p, wave_sums, a.eval_cloud != nullptr, a.partials + ((size_t)r * tiles + jt / kThreads) * 6, tid);
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

// Stored clouds (GwtfStoredCloudArgs): the same grid and the same code behind the point, but the point is a 12-byte gather at an
// index that a keyed bijection on [0, P) gives (gwtf_perm.h) -- no table, no LDS beyond the round keys.  Draw j of a row lies in
// round q = j / P at slot t = j % P.  A cloud of P >= 256 points puts at most two rounds into a tile of 256 draws: their keys are
// derived once per workgroup and round (four threads, one Philox block each) and kept in LDS, slot q & 1.  A smaller cloud wraps
// within the tile, and each thread derives the keys of its own round.
__global__ __launch_bounds__(kThreads) void cloud_gather_kernel(GwtfStoredCloudArgs a, int chunk, int tiles) {
  __shared__ uint32_t keys[2][8];
  __shared__ float wave_sums[4][6];
  const int r = blockIdx.y, tid = threadIdx.x;
  const int M = a.M, N = a.eval_cloud ? M / 2 : M;
  const int shape = a.rows[r];
  const bool known = shape >= 0 && shape < a.n_shapes;       // a row outside the store: NaN points, nothing is read
  const long long pb = known ? a.bounds[shape] : 0;
  const uint32_t P = known ? (uint32_t)(a.bounds[shape + 1] - pb) : 1u;      // the host refuses P < 1 and P >= 2^31
  const bool keyed = known && !a.index && a.permute;
  const bool shared_keys = P >= (uint32_t)kThreads;

  const unsigned long long seed = a.state[0], call = a.state[1];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), c2 = (uint32_t)call, c3 = (uint32_t)(call >> 32);
  float os = 1.f, oc[3] = {0.f, 0.f, 0.f};
  if (known && a.rescale) os = a.orig_s[shape];
  if (known && a.recenter) { oc[0] = a.orig_c[shape * 3]; oc[1] = a.orig_c[shape * 3 + 1]; oc[2] = a.orig_c[shape * 3 + 2]; }

  long long have = -1;                                        // the last round whose keys LDS holds
  const int j0 = blockIdx.x * chunk;
  for (int jt = j0; jt < j0 + chunk && jt < M; jt += kThreads) {
    const int j = jt + tid;
    const bool live = j < M;
    if (keyed && shared_keys) {                               // uniform
      const long long q1 = (uint32_t)min(jt + kThreads - 1, M - 1) / P;
      const long long from = max(have + 1, (long long)((uint32_t)jt / P));
      if (from <= q1) {
        __syncthreads();                                      // the slower waves have read the slot this overwrites
        const long long q = from + (tid >> 1);
        if (tid < 4 && q <= q1) {
          const Philox4 d = philox4x32_10((uint32_t)(2 * q + (tid & 1)), (uint32_t)r, c2, c3 | (2u << 28), k0, k1);
          uint32_t* k = keys[q & 1] + (tid & 1) * 4;          // K0..K3 from block 2q, K4 K5 from block 2q + 1
          k[0] = d.x; k[1] = d.y; k[2] = d.z; k[3] = d.w;
        }
        __syncthreads();
        have = q1;
      }
    }
    float p[3] = {0.f, 0.f, 0.f};
    bool valid = false;
    if (live) {
      uint32_t idx = gwtf_perm::kNoIndex;
      if (known) {
        const uint32_t q = (uint32_t)j / P, t = (uint32_t)j % P;
        if (a.index) {
          idx = (uint32_t)a.index[(size_t)r * M + j];         // a negative index is one above P
        } else if (!a.permute) {
          idx = t;
        } else {
          uint32_t own[6];
          if (shared_keys) {
#pragma unroll
            for (int i = 0; i < 6; ++i) own[i] = keys[q & 1][i];
          } else {
            const Philox4 d0 = philox4x32_10(2u * q, (uint32_t)r, c2, c3 | (2u << 28), k0, k1);
            const Philox4 d1 = philox4x32_10(2u * q + 1u, (uint32_t)r, c2, c3 | (2u << 28), k0, k1);
            own[0] = d0.x; own[1] = d0.y; own[2] = d0.z; own[3] = d0.w; own[4] = d1.x; own[5] = d1.y;
          }
          idx = gwtf_perm::feistel_index(own, t, P);
        }
        valid = idx < P;                                      // the walk's cap and a foreign explicit index: NaN bits, no read
      }
      if (valid) {
        const float* src = a.points + (pb + (long long)idx) * 3;
        p[0] = src[0]; p[1] = src[1]; p[2] = src[2];
      }
      transform_and_store(a, a.index != nullptr, valid, r, j, M, N, os, oc, c2, c3, k0, k1, p);
    }
    if (a.center) {
      if (!valid) { p[0] = 0.f; p[1] = 0.f; p[2] = 0.f; }     // a NaN point adds nothing to its tile
      tile_sums(p, wave_sums, a.eval_cloud != nullptr, a.partials + ((size_t)r * tiles + jt / kThreads) * 6, tid);
    }
  }
}

int chunk_of(int tune) {
  int c = tune & 0xffff;
  if (c == 0) c = kChunkDefault;
  c = (c + kThreads - 1) / kThreads * kThreads;
  return c > kChunkMax ? kChunkMax : c;
}

int launch_finish(const GwtfCloudArgs& a, int tiles, hipStream_t st) {
  const int N = a.eval_cloud ? a.M / 2 : a.M;
  const dim3 fg = a.center ? dim3(min((N + 4 * kThreads - 1) / (4 * kThreads), 64), a.B) : dim3(1, 1);
  hipLaunchKernelGGL(cloud_finish_kernel, fg, dim3(kThreads), 0, st, a, tiles);
  return (int)hipGetLastError();
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
  return launch_finish(a, tiles, st);
}

extern "C" unsigned gwtf_perm_index(const unsigned* keys6, unsigned t, unsigned P) {
  return keys6 ? gwtf_perm::feistel_index(keys6, t, P) : gwtf_perm::kNoIndex;
}

extern "C" int gwtf_sample_stored_clouds(const GwtfStoredCloudArgs* pa) {
  if (!pa) return GWTF_E_BADARG;
  const GwtfStoredCloudArgs& a = *pa;
  if (!a.rows || !a.points || !a.bounds || !a.cloud || !a.state) return GWTF_E_BADARG;
  if (a.B < 1 || a.B > 65535 || a.M < 1 || a.n_shapes < 1) return GWTF_E_BADARG;
  if (a.eval_cloud && (a.M & 1)) return GWTF_E_BADARG;
  if ((a.rescale && !a.orig_s) || (a.recenter && !a.orig_c) || (a.center && !a.partials)) return GWTF_E_BADARG;
  if (a.scale && !(a.scale_div > 0.f)) return GWTF_E_BADARG;
  if (a.noise && !(a.noise_scale > 0.f)) return GWTF_E_BADARG;
  if (a.index ? (a.noise && !a.normals) : (a.normals != nullptr)) return GWTF_E_BADARG;
  const int chunk = chunk_of(a.tune), tiles = gwtf_cloud_partials(a.M);
  hipStream_t st = (hipStream_t)a.stream;
  hipLaunchKernelGGL(cloud_gather_kernel, dim3((a.M + chunk - 1) / chunk, a.B), dim3(kThreads), 0, st, a, chunk, tiles);
  GwtfCloudArgs f = {};                                       // what the finishing launch reads, and nothing else
  f.rows = a.rows; f.cloud = a.cloud; f.eval_cloud = a.eval_cloud; f.partials = a.partials; f.state = a.state;
  f.B = a.B; f.M = a.M; f.n_shapes = a.n_shapes; f.center = a.center;
  return launch_finish(f, tiles, st);
}
