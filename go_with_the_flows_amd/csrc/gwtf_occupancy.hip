// gwtf_occupancy.hip -- the Jensen-Shannon divergence of the generation evaluation on the device: the occupancy histogram of a set of
// clouds over a res^3 grid of [-0.5, 0.5)^3 (reference lib/networks/utils.py:45-79) and the divergence of two such histograms
// (:82-86, scipy.stats.entropy).  Records and rules: include/gwtf.h (GwtfOccupancyArgs).
//
// voxel_occupancy_kernel: one persistent grid of kThreads, at most one workgroup per CU and one per kPointsPerGroup points (a 200-point
// call clears and flushes ONE histogram); a workgroup walks tiles of kTilePoints points with a grid stride.
//   load     the tile's 3 * kTilePoints floats as 16-byte loads, lane after lane (three per thread): never three floats at stride 12.
//            A tensor that starts off a 16-byte boundary is read from the boundary below it; a 16-byte piece that is not wholly
//            inside the tensor (the first and the last one at most) is read float by float, so nothing outside the tensor is touched
//   bin      per VALUE, not per point: the float widened to double, a floor guess corrected against the edge table (LDS copy) until
//            edges[k] <= x < edges[k+1] holds in double -- the table is the rule, the guess only where the search starts.  NaN and
//            +-inf are told by their bits (this library is built with -fno-honor-nans).  The bin (or 0xff: none) is one byte in an LDS
//            staging row; |x| > bound and NaN are counted here, per value
//   count    per point: its three bytes from the staging row, one LDS atomic add into the workgroup's private uint32 histogram
//   flush    every non-zero LDS bin: one 64-bit global atomic add; the two stats: one 64-bit global atomic add per workgroup each
// Integer atomics only: the result does not depend on the order, two calls give the same bits.  LDS: 4 res^3 + 264 (edges) + 12,304
// (staging) + 8 bytes: 100,384 B at res 28, 143,648 B at res 32 -- beyond the 64 KiB a launch gets without asking, so the launcher
// raises the kernel's dynamic-LDS limit once per device and process (the only state this file keeps; it changes no result).
// 12 bytes are read per point and nothing else moves but the flush: the kernel is bound by bytes, not by its atomics, as long as the
// points do not pile into a few bins (an LDS atomic on one address serialises its lanes); see DESIGN.md.
//
// jsd_counts_kernel: one workgroup, float64, fixed order (strided partial sums per thread, then a tree over LDS).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/gwtf.h"

namespace {

constexpr int kThreads = 1024;                      // 16 waves on the CU: the one workgroup is all that hides its own latencies
constexpr int kTilePoints = 4096;                   // 12288 floats = 3072 16-byte pieces: three per thread
constexpr int kTilePieces = 3 * kTilePoints / 4;
constexpr int kPointsPerGroup = 8192;               // metrics.OCC_POINTS_PER_WORKGROUP: the grid has ceil(M / this) workgroups, CUs at most
constexpr int kMaxRes = 32;
constexpr int kJsdThreads = 1024;
constexpr int kMaxDevices = 64;
constexpr uint32_t kNoBin = 0xffu;
constexpr size_t kStageBytes = 4 * (kTilePieces + 1) + 12;     // the tile's pieces + the one more a misaligned tensor needs, one byte per
                                                               // float, rounded to 16

struct Edges { double e[kMaxRes + 1]; };

__host__ __device__ inline size_t occupancy_lds_bytes(int res) {
  return (((size_t)res * res * res * 4 + 15) & ~(size_t)15) + kStageBytes + (kMaxRes + 1) * 8 + 8;
}

// Bin of one value, or kNoBin.  `edges` is the LDS copy of the table, e_first / e_last its two outer entries.
__device__ inline uint32_t bin_of(float xf, const double* edges, int res, double e_first, double e_last, uint32_t& n_out, uint32_t& n_nan,
                                  float bound) {
  const uint32_t mag = __float_as_uint(xf) & 0x7fffffffu;
  if (mag > 0x7f800000u) { ++n_nan; return kNoBin; }                 // NaN: |x| > bound is false for it, as in numpy
  if (__uint_as_float(mag) > bound) ++n_out;                         // +-inf included
  if (mag == 0x7f800000u) return kNoBin;
  const double x = (double)xf;
  if (!(x >= e_first && x < e_last)) return kNoBin;
  int k0 = (int)((x + 0.5) * (double)res);                           // where the search starts; x is finite and inside the table
  k0 = k0 < 0 ? 0 : (k0 > res - 1 ? res - 1 : k0);
  const double lo = edges[k0], hi = edges[k0 + 1];
  int k = k0 + (x >= hi ? 1 : 0) - (x < lo ? 1 : 0);                 // the guess is a bin off at most (a float64 rounding of an edge)
  if (k != k0) {                                                     // rare; the table decides, however far the guess was off
    while (k > 0 && x < edges[k]) --k;
    while (k < res - 1 && x >= edges[k + 1]) ++k;
  }
  return (uint32_t)k;
}

__global__ __launch_bounds__(kThreads) void voxel_occupancy_kernel(const float* __restrict__ points, size_t n_points, int res, Edges table,
                                                                   float bound, unsigned long long* __restrict__ counts,
                                                                   unsigned long long* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int bins = res * res * res;
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem);                                   // [bins]
  uint32_t* stage = reinterpret_cast<uint32_t*>(smem + (((size_t)bins * 4 + 15) & ~(size_t)15));      // [kTilePieces + 1] x 4 bytes
  double* edges = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(stage) + kStageBytes);   // [res + 1]
  uint32_t* totals = reinterpret_cast<uint32_t*>(edges + kMaxRes + 1);                  // {out of bound, NaN}

  for (int i = tid; i < bins; i += kThreads) hist[i] = 0u;
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i <= kMaxRes; ++i) edges[i] = table.e[i];
    totals[0] = 0u;
    totals[1] = 0u;
  }
  __syncthreads();

  // The tensor as a stream of floats F[0 .. 3M); F[j] sits at base[j + shift], base the 16-byte boundary at or below `points`.
  const int shift = (int)((reinterpret_cast<uintptr_t>(points) & 15u) >> 2);
  const float* base = points - shift;
  const long long n_floats = 3ll * (long long)n_points;
  const size_t n_tiles = (n_points + kTilePoints - 1) / kTilePoints;
  const int pieces = kTilePieces + (shift ? 1 : 0);
  const unsigned char* stage_bytes = reinterpret_cast<const unsigned char*>(stage);
  const double e_first = edges[0], e_last = edges[res];
  uint32_t n_out = 0u, n_nan = 0u;

  for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long f_lo = (long long)tile * (3 * kTilePoints);                          // the tile's floats: F[f_lo .. f_hi)
    const long long f_hi = f_lo + 3 * kTilePoints < n_floats ? f_lo + 3 * kTilePoints : n_floats;
    for (int i = tid; i < pieces; i += kThreads) {
      const long long j0 = f_lo + 4ll * i - shift;                                        // F index of the piece's first float
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (j0 >= 0 && j0 + 3 < n_floats) {
        const float4 q = *reinterpret_cast<const float4*>(base + (j0 + shift));
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (j0 + c >= 0 && j0 + c < n_floats) v[c] = points[j0 + c];
      }
      uint32_t packed = 0u;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        uint32_t b = kNoBin;
        if (j0 + c >= f_lo && j0 + c < f_hi) b = bin_of(v[c], edges, res, e_first, e_last, n_out, n_nan, bound);       // a neighbour tile's float: not ours
        packed |= b << (8 * c);
      }
      stage[i] = packed;
    }
    __syncthreads();
    const size_t p0 = tile * kTilePoints;
#pragma unroll
    for (int r = 0; r < kTilePoints / kThreads; ++r) {
      const int p = tid + r * kThreads;
      if (p0 + p < n_points) {
        const unsigned char* s = stage_bytes + 3 * p + shift;
        const uint32_t bx = s[0], by = s[1], bz = s[2];
        if ((bx | by | bz) < (uint32_t)kMaxRes) atomicAdd(&hist[(bx * res + by) * res + bz], 1u);
      }
    }
    __syncthreads();                                                                      // the staging row is rewritten next
  }

  if (stats) {
    if (n_out) atomicAdd(&totals[0], n_out);
    if (n_nan) atomicAdd(&totals[1], n_nan);
  }
  __syncthreads();
  for (int i = tid; i < bins; i += kThreads) {
    const uint32_t c = hist[i];
    if (c) atomicAdd(&counts[i], (unsigned long long)c);
  }
  if (stats && tid < 2 && totals[tid]) atomicAdd(&stats[tid], (unsigned long long)totals[tid]);
}

// -x ln x of a probability: 0 at 0 (scipy.special.entr).
__device__ inline double entr(double p) { return p > 0.0 ? -p * log(p) : 0.0; }

__global__ __launch_bounds__(kJsdThreads) void jsd_counts_kernel(const long long* __restrict__ c1, const long long* __restrict__ c2, int bins,
                                                              double* __restrict__ out) {
  __shared__ double red[3][kJsdThreads];
  __shared__ long long tot[2][kJsdThreads];
  const int tid = threadIdx.x;
  long long t1 = 0, t2 = 0;
  for (int i = tid; i < bins; i += kJsdThreads) { t1 += c1[i]; t2 += c2[i]; }
  tot[0][tid] = t1;
  tot[1][tid] = t2;
  __syncthreads();
  for (int s = kJsdThreads / 2; s > 0; s >>= 1) {
    if (tid < s) { tot[0][tid] += tot[0][tid + s]; tot[1][tid] += tot[1][tid + s]; }
    __syncthreads();
  }
  t1 = tot[0][0];
  t2 = tot[1][0];
  if (t1 == 0 || t2 == 0) {                                   // 0 / 0 in the reference: NaN (by its bits: built with -fno-honor-nans)
    if (tid == 0) *reinterpret_cast<unsigned long long*>(out) = 0x7ff8000000000000ull;
    return;
  }
  const double d1 = (double)t1, d2 = (double)t2;
  double h1 = 0.0, h2 = 0.0, hm = 0.0;
  for (int i = tid; i < bins; i += kJsdThreads) {
    const double p1 = (double)c1[i] / d1, p2 = (double)c2[i] / d2;
    h1 += entr(p1);
    h2 += entr(p2);
    hm += entr((p1 + p2) / 2.0);
  }
  red[0][tid] = h1;
  red[1][tid] = h2;
  red[2][tid] = hm;
  __syncthreads();
  for (int s = kJsdThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
      red[2][tid] += red[2][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double ln2 = 0.693147180559945309417232121458;
    out[0] = red[2][0] / ln2 - 0.5 * (red[0][0] / ln2 + red[1][0] / ln2);
  }
}

// Per device: the CU count, and whether the kernel's dynamic-LDS limit has been raised (0 not asked yet, 1 granted, -1 refused).
struct DeviceNote { int cus; int large_lds; };
DeviceNote g_notes[kMaxDevices];

}  // namespace

extern "C" int gwtf_voxel_occupancy(const GwtfOccupancyArgs* pa) {
  if (!pa) return GWTF_E_BADARG;
  const GwtfOccupancyArgs& a = *pa;
  if (!a.points || !a.counts || a.n_points < 1 || a.n_points > 0xffffffffull) return GWTF_E_BADARG;
  if (a.res < 1 || a.res > kMaxRes || !(a.bound >= 0.f)) return GWTF_E_BADARG;
  if (reinterpret_cast<uintptr_t>(a.points) & 3u) return GWTF_E_BADARG;
  for (int i = 0; i < a.res; ++i)
    if (!(a.edges[i] < a.edges[i + 1])) return GWTF_E_BADARG;
  int dev = 0;
  hipError_t err = hipGetDevice(&dev);
  if (err != hipSuccess) return (int)err;
  if (dev < 0 || dev >= kMaxDevices) return GWTF_E_UNSUPPORTED;
  DeviceNote& note = g_notes[dev];
  if (note.large_lds == 0) {
    int cus = 0;
    err = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (err != hipSuccess) return (int)err;
    note.cus = cus < 1 ? 1 : cus;
    err = hipFuncSetAttribute(reinterpret_cast<const void*>(&voxel_occupancy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)occupancy_lds_bytes(kMaxRes));
    if (err != hipSuccess) (void)hipGetLastError();           // refused: remembered, and the error does not stick to the next call
    note.large_lds = err == hipSuccess ? 1 : -1;
  }
  if (note.large_lds < 0) return GWTF_E_UNSUPPORTED;
  Edges table;
  for (int i = 0; i <= kMaxRes; ++i) table.e[i] = i <= a.res ? a.edges[i] : 0.0;
  const size_t groups = (a.n_points + kPointsPerGroup - 1) / kPointsPerGroup;
  const unsigned grid = (unsigned)(groups < (size_t)note.cus ? groups : (size_t)note.cus);
  hipLaunchKernelGGL(voxel_occupancy_kernel, dim3(grid), dim3(kThreads), occupancy_lds_bytes(a.res), (hipStream_t)a.stream, a.points,
                     a.n_points, a.res, table, a.bound, reinterpret_cast<unsigned long long*>(a.counts),
                     reinterpret_cast<unsigned long long*>(a.stats));
  return (int)hipGetLastError();
}

extern "C" int gwtf_jsd_counts(const long long* c1, const long long* c2, int bins, double* out, void* stream) {
  if (!c1 || !c2 || !out || bins < 1) return GWTF_E_BADARG;
  hipLaunchKernelGGL(jsd_counts_kernel, dim3(1), dim3(kJsdThreads), 0, (hipStream_t)stream, c1, c2, bins, out);
  return (int)hipGetLastError();
}
