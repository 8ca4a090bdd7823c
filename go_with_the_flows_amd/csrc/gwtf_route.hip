// gwtf_route.hip -- device-resident generation, the step in front of the routed stack launch (gwtf_stack.hip, ROUTED): every point of
// S generated clouds draws its mixture component and its base sample, and the points of a shape are laid out component by component
// in whole tiles of the stack kernel (reference lib/networks/flow_mixture.py:146-177: np.random.choice over the normalised weights,
// models.py:99-109 reparameterize, the scatter by mask; include/gwtf.h has the contract).
//
// One launch, one workgroup of 256 threads per shape, two passes over the shape's n points in chunks of 256 (n is not bounded by LDS):
//   pass 1  label of every point (thresholds against its 32-bit word, or read) -> labels; per-component counts in LDS
//   pass 2  position of every point: a stable counting sort -- rank among the equal labels of its wavefront by ballot, plus the
//           earlier wavefronts' counts of the chunk, plus the component's running offset -- then perm / zp at that position
// and the padding behind every component's last point is filled (perm -1, zp 0).  Thread i handles point chunk * 256 + i in both
// passes and reads back only labels it wrote itself.  Counts are integer LDS atomics, nothing is added in global memory: the
// outputs are a function of the labels alone.  A one-thread finishing launch stores call + 1, as the cloud sampler's does.
// The same body serves latent sweeps (gwtf_mixture_route_sweep): rows that share the draws of one shape in groups, each with its own
// logits and, per component, its own base Gaussian.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/gwtf.h"
#include "gwtf_layout.h"
#include "gwtf_philox.h"

namespace {

using namespace gwtf_rng;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxK = GWTF_MAX_COMPONENTS;
constexpr uint32_t kStreamLabel = 2u, kStreamNormal = 3u;      // Philox streams (the cloud sampler uses 0 and 1)

// SWEEP (gwtf_mixture_route_sweep, Args = GwtfRouteSweepArgs): row r of R = a.S rows draws what shape r / group draws -- the Philox shape
// coordinate and the row of every explicit array are r / group -- while its logits, its base Gaussians and its outputs are its own; the
// base of a point is that of ITS component, K tables a.mu0_stride_k floats apart, read from LDS by the label in pass 2.
// route_kernel<false, GwtfRouteArgs> is the routing launch as it always was, instruction for instruction.
template <bool SWEEP, class Args>
__global__ __launch_bounds__(kThreads) void route_kernel(Args a, int tiles) {
  __shared__ double cdf[kMaxK];
  __shared__ uint32_t thr[kMaxK];
  __shared__ int count[kMaxK], next_slot[kMaxK], tile_start[kMaxK + 1], wave_count[kWaves][kMaxK];
  __shared__ float mu_k[SWEEP ? kMaxK : 1][3], sd_k[SWEEP ? kMaxK : 1][3];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int sdraw = s;                                               // whose draws this row takes
  if constexpr (SWEEP) sdraw = s / a.group;
  const int n = a.n, K = a.K, P = a.P;
  const size_t NP = (size_t)tiles * P;
  const int* words = a.words ? a.words + (size_t)sdraw * n : nullptr;
  const int* labels_in = a.labels_in ? a.labels_in + (size_t)sdraw * n : nullptr;
  int* labels = a.labels + (size_t)s * n;
  int* perm = a.perm + (size_t)s * NP;
  float* zp = a.zp + (size_t)s * 3 * NP;

  if (!labels_in && tid == 0) {                                // K <= 64 values: one thread, numpy's order of additions
    const float* l = a.logits + (size_t)s * K;
    float mx = l[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, l[k]);
    double run = 0.0;
    for (int k = 0; k < K; ++k) {
      run += exp((double)l[k] - (double)mx);
      cdf[k] = run;
    }
    for (int k = 0; k < K; ++k) {
      const double t = ceil(cdf[k] / run * 4294967296.0);
      thr[k] = t < 4294967295.0 ? (uint32_t)t : 0xffffffffu;
    }
  }
  for (int k = tid; k < K; k += kThreads) {
    count[k] = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) wave_count[w][k] = 0;
  }
  if constexpr (SWEEP) {
    if (!a.z0_in) {
      for (int j = tid; j < 3 * K; j += kThreads) {            // read in pass 2, behind the barriers below
        const int k = j / 3, d = j - 3 * k;
        mu_k[k][d] = a.mu0[(size_t)s * a.mu0_stride + (size_t)k * a.mu0_stride_k + d];
        sd_k[k][d] = expf(0.5f * a.lv0[(size_t)s * a.lv0_stride + (size_t)k * a.lv0_stride_k + d]);
      }
    }
  }
  __syncthreads();
  if (!labels_in && a.thresholds && tid < K) a.thresholds[(size_t)s * K + tid] = (int)thr[tid];

  uint32_t k0 = 0, k1 = 0, c2 = 0, c3 = 0;
  if (a.state) {
    const unsigned long long seed = (unsigned long long)a.state[0], call = (unsigned long long)a.state[1];
    k0 = (uint32_t)seed; k1 = (uint32_t)(seed >> 32); c2 = (uint32_t)call; c3 = (uint32_t)(call >> 32);
  }

  // ---- pass 1: labels and counts
  for (int i0 = 0; i0 < n; i0 += kThreads) {
    const int i = i0 + tid;
    const bool live = i < n;
    int lab = -1;
    if (live) {
      if (labels_in) {
        lab = min(max(labels_in[i], 0), K - 1);                // every position computed below stays inside the shape's slots
      } else {
        const uint32_t w = words ? (uint32_t)words[i] : philox4x32_10((uint32_t)i, (uint32_t)sdraw, c2, c3 | (kStreamLabel << 28), k0, k1).x;
        lab = 0;
        for (int k = 0; k + 1 < K; ++k) lab += thr[k] <= w ? 1 : 0;
      }
      labels[i] = lab;
    }
    unsigned long long todo = __ballot(live);                  // wave-uniform: one round per distinct label of the wavefront
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int L = __shfl(lab, leader);
      const unsigned long long same = __ballot(lab == L);
      if (lane == leader) atomicAdd(&count[L], __popcll(same));
      todo &= ~same;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int t = 0;
    for (int k = 0; k < K; ++k) {
      tile_start[k] = t;
      next_slot[k] = t * P;
      t += (count[k] + P - 1) / P;
    }
    tile_start[K] = t;                                         // <= tiles: sum_k ceil(c_k / P) <= floor((n + K (P - 1)) / P)
  }
  __syncthreads();
  for (int t = tid; t < tiles; t += kThreads) {
    int comp = -1;
    for (int k = 0; k < K; ++k) comp = (t >= tile_start[k] && t < tile_start[k + 1]) ? k : comp;
    a.tile_comp[(size_t)s * tiles + t] = comp;
  }

  float mu[3] = {0.f, 0.f, 0.f}, sd[3] = {1.f, 1.f, 1.f};
  if (!SWEEP && !a.z0_in) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      mu[d] = a.mu0[(size_t)s * a.mu0_stride + d];
      sd[d] = expf(0.5f * a.lv0[(size_t)s * a.lv0_stride + d]);
    }
  }

  // ---- pass 2: positions, perm and the base samples
  for (int i0 = 0; i0 < n; i0 += kThreads) {
    const int i = i0 + tid;
    const bool live = i < n;
    const int lab = live ? labels[i] : -1;
    int rank = 0;
    unsigned long long todo = __ballot(live);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int L = __shfl(lab, leader);
      const unsigned long long same = __ballot(lab == L);
      if (lab == L) rank = __popcll(same & ((1ull << lane) - 1ull));
      if (lane == leader) wave_count[wave][L] = __popcll(same);
      todo &= ~same;
    }
    __syncthreads();
    int slot = -1;
    if (live) {
      slot = next_slot[lab] + rank;
      for (int w = 0; w < wave; ++w) slot += wave_count[w][lab];
    }
    __syncthreads();
    for (int k = tid; k < K; k += kThreads) {
      int c = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) { c += wave_count[w][k]; wave_count[w][k] = 0; }
      next_slot[k] += c;
    }
    __syncthreads();
    if (live && slot >= 0 && (size_t)slot < NP) {
      float z[3];
      if (a.z0_in) {
        const float* src = a.z0_in + (size_t)sdraw * 3 * n + i;
        z[0] = src[0]; z[1] = src[n]; z[2] = src[2 * (size_t)n];
      } else {
        float e[4];
        if (a.normals) {
          const float* src = a.normals + (size_t)sdraw * 3 * n + i;
          e[0] = src[0]; e[1] = src[n]; e[2] = src[2 * (size_t)n];
        } else {
          const Philox4 d = philox4x32_10((uint32_t)i, (uint32_t)sdraw, c2, c3 | (kStreamNormal << 28), k0, k1);
          box_muller(d.x, d.y, e[0], e[1]);
          box_muller(d.z, d.w, e[2], e[3]);
        }
        if constexpr (SWEEP) {
#pragma unroll
          for (int d = 0; d < 3; ++d) { mu[d] = mu_k[lab][d]; sd[d] = sd_k[lab][d]; }
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) z[d] = e[d] * sd[d] + mu[d];  // reparameterize's order (the library is built -ffp-contract=off)
      }
      perm[slot] = i;
      zp[slot] = z[0]; zp[NP + slot] = z[1]; zp[2 * NP + slot] = z[2];
    }
  }

  // ---- padding: behind each component's last point up to the end of its last tile, then the unused slots
  for (int k = 0; k <= K; ++k) {
    const size_t from = k < K ? (size_t)tile_start[k] * P + count[k] : (size_t)tile_start[K] * P;
    const size_t to = k < K ? (size_t)tile_start[k + 1] * P : NP;
    for (size_t j = from + tid; j < to; j += kThreads) {
      perm[j] = -1;
      zp[j] = 0.f; zp[NP + j] = 0.f; zp[2 * NP + j] = 0.f;
    }
  }
}

// every workgroup of the routing launch has read the state (this launch follows it on the stream): the next call, or the next replay of
// a captured graph, draws fresh clouds
__global__ void route_finish_kernel(long long* state) { state[1] = state[1] + 1; }

}  // namespace

extern "C" int gwtf_route_tiles(int n, int K, int P) {
  if (n < 1 || n > (1 << 30) || K < 1 || K > kMaxK || (P != 64 && P != 128 && P != 256)) return 0;
  return (int)(((long long)n + (long long)K * (P - 1)) / P);
}

// what both entry points refuse
template <class Args>
static bool route_args_ok(const Args& a) {
  if (a.S < 1 || a.n < 1 || a.K < 1 || a.K > kMaxK || (a.P != 64 && a.P != 128 && a.P != 256)) return false;
  if (!a.tile_comp || !a.perm || !a.zp || !a.labels) return false;
  if (!a.labels_in && (!a.logits || (!a.words && !a.state))) return false;
  if (!a.z0_in && (!a.mu0 || !a.lv0 || a.mu0_stride < 0 || a.lv0_stride < 0 || (!a.normals && !a.state))) return false;
  const int tiles = gwtf_route_tiles(a.n, a.K, a.P);
  return tiles >= 1 && (long long)a.S * tiles <= 0x7fffffffLL / a.P;
}

extern "C" int gwtf_mixture_route(const GwtfRouteArgs* pa) {
  if (!pa || !route_args_ok(*pa)) return GWTF_E_BADARG;
  const GwtfRouteArgs& a = *pa;
  const int tiles = gwtf_route_tiles(a.n, a.K, a.P);
  hipStream_t st = (hipStream_t)a.stream;
  hipLaunchKernelGGL((route_kernel<false, GwtfRouteArgs>), dim3((unsigned)a.S), dim3(kThreads), 0, st, a, tiles);
  if (a.state) hipLaunchKernelGGL(route_finish_kernel, dim3(1), dim3(1), 0, st, a.state);
  return (int)hipGetLastError();
}

extern "C" int gwtf_mixture_route_sweep(const GwtfRouteSweepArgs* pa) {
  if (!pa || !route_args_ok(*pa)) return GWTF_E_BADARG;
  const GwtfRouteSweepArgs& a = *pa;
  if (a.group < 1 || a.S % a.group != 0 || a.mu0_stride_k < 0 || a.lv0_stride_k < 0) return GWTF_E_BADARG;
  const int tiles = gwtf_route_tiles(a.n, a.K, a.P);
  hipStream_t st = (hipStream_t)a.stream;
  hipLaunchKernelGGL((route_kernel<true, GwtfRouteSweepArgs>), dim3((unsigned)a.S), dim3(kThreads), 0, st, a, tiles);
  if (a.state) hipLaunchKernelGGL(route_finish_kernel, dim3(1), dim3(1), 0, st, a.state);
  return (int)hipGetLastError();
}
