// gwtf_metrics.hip -- structural losses between point sets: nearest-neighbour (Chamfer) distances and the approximate
// earth-mover matching.  These are the reference's ONLY native code (CUDA extension
// lib/metrics/pytorch_structural_losses/src/{nndistance.cu,approxmatch.cu}, bound in structural_loss.cpp:22-123 and
// pybind/bind.cpp:9-15); evaluate_ae.py cannot run on ROCm without them.  Same results (first-minimum tie rule, the
// nine-level auction schedule, clamp constants), different decomposition: the reference caps every launch at 32
// workgroups (one V100-era choice); here the grid covers (batch x tiles) and both directions run in one launch.
// Layout of the point sets is the reference's: [b][n][3] point-major.
#include <hip/hip_runtime.h>
#include "../../include/gwtf.h"

namespace {

constexpr int kTile = 1024;   // points of the "other" set staged in LDS per step (16 KiB as float4)

// |b - a|^2 as every Chamfer kernel of this file evaluates it: b - a per coordinate, (dx dx + dy dy) + dz dz, no FMA (the library is
// built with -ffp-contract=off).  T = float, or a 2-vector of floats (two query points per packed instruction): elementwise, so
// the bits of a lane do not depend on T.
typedef float float2v __attribute__((ext_vector_type(2)));
template <class T>
__device__ inline T sqdist3(T bx, T by, T bz, T ax, T ay, T az) {
  const T dx = bx - ax, dy = by - ay, dz = bz - az;
  return (dx * dx + dy * dy) + dz * dz;
}

// dist[i][j] = min_k |a_j - b_k|^2, idx = first minimiser (reference nndistance.cu:2-124: strict '<' inside a tile,
// strict '>' across tiles).  grid = (query tiles, batch, 2 directions); 256 threads x 2 query points each.
__global__ __launch_bounds__(256) void nnd_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                  float* __restrict__ dist1, int* __restrict__ idx1,
                                                  float* __restrict__ dist2, int* __restrict__ idx2, int b, int n, int m) {
  __shared__ float4 buf[kTile];
  const bool rev = blockIdx.z == 1;
  const float* A = rev ? xyz2 : xyz1;
  const float* Bp = rev ? xyz1 : xyz2;
  const int na = rev ? m : n, nb = rev ? n : m;
  float* dist = rev ? dist2 : dist1;
  int* idx = rev ? idx2 : idx1;
  const int i = blockIdx.y;
  const int j0 = blockIdx.x * 512 + threadIdx.x, j1 = j0 + 256;
  if (blockIdx.x * 512 >= na) return;
  const bool v0 = j0 < na, v1 = j1 < na;
  const float ax0 = v0 ? A[((size_t)i * na + j0) * 3 + 0] : 0.f, ay0 = v0 ? A[((size_t)i * na + j0) * 3 + 1] : 0.f,
              az0 = v0 ? A[((size_t)i * na + j0) * 3 + 2] : 0.f;
  const float ax1 = v1 ? A[((size_t)i * na + j1) * 3 + 0] : 0.f, ay1 = v1 ? A[((size_t)i * na + j1) * 3 + 1] : 0.f,
              az1 = v1 ? A[((size_t)i * na + j1) * 3 + 2] : 0.f;
  float best0 = 3.4e38f, best1 = 3.4e38f;
  int bi0 = 0, bi1 = 0;
  for (int k0 = 0; k0 < nb; k0 += kTile) {
    const int cnt = min(kTile, nb - k0);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt; t += blockDim.x) {
      const float* q = Bp + ((size_t)i * nb + k0 + t) * 3;
      buf[t] = make_float4(q[0], q[1], q[2], 0.f);
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < cnt; ++k) {
      const float4 q = buf[k];   // same address in every lane: LDS broadcast
      const float d0 = sqdist3(q.x, q.y, q.z, ax0, ay0, az0);
      const float d1 = sqdist3(q.x, q.y, q.z, ax1, ay1, az1);
      if (d0 < best0) { best0 = d0; bi0 = k0 + k; }
      if (d1 < best1) { best1 = d1; bi1 = k0 + k; }
    }
  }
  if (v0) { dist[(size_t)i * na + j0] = best0; idx[(size_t)i * na + j0] = bi0; }
  if (v1) { dist[(size_t)i * na + j1] = best1; idx[(size_t)i * na + j1] = bi1; }
}

// Directed Chamfer reduction over ALL ordered pairs of two sets of clouds: sum[i][j] = sum_{a in q_i} min_{b in t_j} |a - b|^2 and
// cnt[h][i][j] = #{a in q_i : min < thr[h]} (float32 compare).  The per-point minimum is nnd_kernel's dist1 bit for bit (same
// sqdist3, min instead of compare-and-select: no index is kept).  One workgroup = one query cloud x one GROUP of kCdGroup target
// clouds: the query points sit in registers (256 threads x 8 points = 2048 per chunk, longer clouds in chunks of that), the
// targets stream through the LDS tile, so one broadcast LDS read serves 8 evaluations and the query load is paid once per group.
// Reductions are per pair and inside the workgroup -- lane (points in order), wave (shuffle tree), waves in order, chunks in
// order -- so a result does not depend on the launch; no float atomics.  grid.x = nq * ceil(nt / kCdGroup).
constexpr int kCdGroup = 8;      // target clouds per workgroup
constexpr int kCdPts = 8;        // query points per thread
constexpr int kCdChunk = 256 * kCdPts;
constexpr int kCdMaxThr = 8;
struct CdThr { float v[kCdMaxThr]; };

__global__ __launch_bounds__(256) void chamfer_directed_kernel(const float* __restrict__ q, const float* __restrict__ t,
                                                               float* __restrict__ sum, int* __restrict__ cnt, CdThr thr,
                                                               int n_thr, int nq, int nt, int n, int m) {
  __shared__ float4 buf[kTile];
  __shared__ float wsum[4];
  __shared__ int wcnt[4][kCdMaxThr];
  __shared__ float acc_sum[kCdGroup];
  __shared__ int acc_cnt[kCdGroup][kCdMaxThr];
  const int groups = (nt + kCdGroup - 1) / kCdGroup;
  const int i = blockIdx.x / groups, j0 = (blockIdx.x % groups) * kCdGroup;
  const int nj = min(kCdGroup, nt - j0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < kCdGroup) {
    acc_sum[tid] = 0.f;
#pragma unroll
    for (int h = 0; h < kCdMaxThr; ++h) acc_cnt[tid][h] = 0;
  }
  const float* Q = q + (size_t)i * n * 3;
  for (int c0 = 0; c0 < n; c0 += kCdChunk) {
    float2v ax[kCdPts / 2], ay[kCdPts / 2], az[kCdPts / 2];
#pragma unroll
    for (int p = 0; p < kCdPts; ++p) {     // point c0 + p * 256 + tid: consecutive lanes read consecutive points
      const int k = c0 + p * 256 + tid;
      const bool v = k < n;
      ax[p / 2][p % 2] = v ? Q[(size_t)k * 3 + 0] : 0.f;
      ay[p / 2][p % 2] = v ? Q[(size_t)k * 3 + 1] : 0.f;
      az[p / 2][p % 2] = v ? Q[(size_t)k * 3 + 2] : 0.f;
    }
    for (int jj = 0; jj < nj; ++jj) {
      const float* T = t + (size_t)(j0 + jj) * m * 3;
      float2v best[kCdPts / 2];
#pragma unroll
      for (int p = 0; p < kCdPts / 2; ++p) best[p] = float2v{3.4e38f, 3.4e38f};
      for (int k0 = 0; k0 < m; k0 += kTile) {
        const int cn = min(kTile, m - k0);
        __syncthreads();
        for (int s = tid; s < cn; s += 256) {
          const float* b = T + (size_t)(k0 + s) * 3;
          buf[s] = make_float4(b[0], b[1], b[2], 0.f);
        }
        __syncthreads();
#pragma unroll 2
        for (int k = 0; k < cn; ++k) {
          const float4 b = buf[k];   // same address in every lane: LDS broadcast
          const float2v bx = {b.x, b.x}, by = {b.y, b.y}, bz = {b.z, b.z};
#pragma unroll
          for (int p = 0; p < kCdPts / 2; ++p) {
            const float2v d = sqdist3(bx, by, bz, ax[p], ay[p], az[p]);
            best[p] = float2v{fminf(best[p][0], d[0]), fminf(best[p][1], d[1])};
          }
        }
      }
      // this chunk's share of pair (i, j0 + jj)
      float s = 0.f;
      int c[kCdMaxThr];
#pragma unroll
      for (int h = 0; h < kCdMaxThr; ++h) c[h] = 0;
#pragma unroll
      for (int p = 0; p < kCdPts; ++p) {
        const float d = best[p / 2][p % 2];
        if (c0 + p * 256 + tid < n) {
          s += d;
#pragma unroll
          for (int h = 0; h < kCdMaxThr; ++h) c[h] += (h < n_thr && d < thr.v[h]) ? 1 : 0;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
#pragma unroll
      for (int h = 0; h < kCdMaxThr; ++h) {
        if (h < n_thr) {             // uniform
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) c[h] += __shfl_down(c[h], off);
        }
      }
      if (lane == 0) {
        wsum[wave] = s;
#pragma unroll
        for (int h = 0; h < kCdMaxThr; ++h) wcnt[wave][h] = c[h];
      }
      __syncthreads();
      if (tid == 0) {
        acc_sum[jj] += ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
#pragma unroll
        for (int h = 0; h < kCdMaxThr; ++h) acc_cnt[jj][h] += ((wcnt[0][h] + wcnt[1][h]) + wcnt[2][h]) + wcnt[3][h];
      }
      // the next tile's first barrier orders thread 0's reads of wsum / wcnt before they are written again
    }
  }
  __syncthreads();
  if (tid < nj) {
    sum[(size_t)i * nt + j0 + tid] = acc_sum[tid];
    for (int h = 0; h < n_thr; ++h) cnt[((size_t)h * nq + i) * nt + j0 + tid] = acc_cnt[tid][h];
  }
}

// The rescaling chain of the reference's evaluate (evaluating.py:100-120) fused with the layout change its metrics need: channel-major
// (B,3,cnt) in, point-major (B,cnt,3) out, both sets in one launch (z = set).  One thread = one point: consecutive lanes read
// consecutive floats of each channel row and a wave's 12-byte stores are one contiguous run.  Every statement of the reference is one
// IEEE operation here, in its order (include/gwtf.h); the translation is added in double and rounded once, as torch rounds
// float32 += float64.  Lanes past the end clamp their index (they load a valid point) and skip the store.
__global__ __launch_bounds__(256) void eval_frame_kernel(GwtfEvalFrameArgs a) {
  const bool second = blockIdx.z == 1;
  const int cnt = second ? a.m : a.n;
  if ((int)(blockIdx.x * 256) >= cnt) return;
  const float* src = second ? a.ref : a.gen;
  float* dst = second ? a.ref_out : a.gen_out;
  const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x, k = min(j, cnt - 1);
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = src[((size_t)i * 3 + c) * cnt + k];
  for (int s = 0; s < a.n_scale; ++s) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = v[c] * a.scale;
  }
  if (a.translate) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (float)((double)v[c] + a.shift[c]);
  }
  if (a.row_scale) {
    const float s = a.orig_s[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = v[c] * s;
  }
  if (a.row_shift) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = v[c] + a.orig_c[(size_t)i * 3 + c];
  }
  if (j < cnt) {
    float* o = dst + ((size_t)i * cnt + j) * 3;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
  }
}

// Cloud i against cloud i, both directions: grid = (query chunks, pairs, 2 directions).  chamfer_directed_kernel's structure with one
// target cloud per workgroup: PTS query points per thread in registers (chunk = 256 * PTS), the other cloud streamed through the LDS
// tile and read by broadcast, minimum by fminf on the same sqdist3 -- each per-point minimum is nnd_kernel's dist1 / dist2 bit for
// bit.  The workgroup reduces its chunk (lane: points in order; wave: shuffle tree; waves in order) and writes ONE partial of
// kPairWords words -- float32 sum, kCdMaxThr int32 counts -- with plain stores; nothing is accumulated across workgroups.
// PTS = 8 keeps the 8 evaluations per LDS read of the all-pairs kernel; PTS = 2 is for batches that would leave the device empty at
// that chunk (B = 1 at 2500 points: 2 x 2 workgroups against 2 x 5).  Lanes past the end clamp their index and are left out of the sums.
constexpr int kPairWords = 1 + kCdMaxThr;
constexpr int kPairSmallChunk = 512;     // 256 threads x 2 points: the chunk the partial buffer is laid out for
constexpr int kPairFillGroups = 256;     // PTS = 8 when its grid has at least this many workgroups (one per compute unit)

template <int PTS>
__global__ __launch_bounds__(256) void chamfer_paired_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                             float* __restrict__ partials, CdThr thr, int n_thr, int B, int n,
                                                             int m, int P) {
  __shared__ float4 buf[kTile];
  __shared__ float wsum[4];
  __shared__ int wcnt[4][kCdMaxThr];
  const bool rev = blockIdx.z == 1;
  const int nq = rev ? m : n, nt = rev ? n : m;
  const int c0 = blockIdx.x * (256 * PTS);
  if (c0 >= nq) return;                                   // uniform: the grid is sized for the longer of the two sets
  const int i = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* Q = (rev ? xb : xa) + (size_t)i * nq * 3;
  const float* T = (rev ? xa : xb) + (size_t)i * nt * 3;
  float2v ax[PTS / 2], ay[PTS / 2], az[PTS / 2], best[PTS / 2];
#pragma unroll
  for (int p = 0; p < PTS; ++p) {                         // point c0 + p * 256 + tid: consecutive lanes read consecutive points
    const int k = min(c0 + p * 256 + tid, nq - 1);
    ax[p / 2][p % 2] = Q[(size_t)k * 3 + 0];
    ay[p / 2][p % 2] = Q[(size_t)k * 3 + 1];
    az[p / 2][p % 2] = Q[(size_t)k * 3 + 2];
  }
#pragma unroll
  for (int p = 0; p < PTS / 2; ++p) best[p] = float2v{3.4e38f, 3.4e38f};
  for (int k0 = 0; k0 < nt; k0 += kTile) {
    const int cn = min(kTile, nt - k0);
    __syncthreads();
    for (int s = tid; s < cn; s += 256) {
      const float* b = T + (size_t)(k0 + s) * 3;
      buf[s] = make_float4(b[0], b[1], b[2], 0.f);
    }
    __syncthreads();
#pragma unroll 2
    for (int k = 0; k < cn; ++k) {
      const float4 b = buf[k];   // same address in every lane: LDS broadcast
      const float2v bx = {b.x, b.x}, by = {b.y, b.y}, bz = {b.z, b.z};
#pragma unroll
      for (int p = 0; p < PTS / 2; ++p) {
        const float2v d = sqdist3(bx, by, bz, ax[p], ay[p], az[p]);
        best[p] = float2v{fminf(best[p][0], d[0]), fminf(best[p][1], d[1])};
      }
    }
  }
  float s = 0.f;
  int c[kCdMaxThr];
#pragma unroll
  for (int h = 0; h < kCdMaxThr; ++h) c[h] = 0;
#pragma unroll
  for (int p = 0; p < PTS; ++p) {
    const float d = best[p / 2][p % 2];
    if (c0 + p * 256 + tid < nq) {
      s += d;
#pragma unroll
      for (int h = 0; h < kCdMaxThr; ++h) c[h] += (h < n_thr && d < thr.v[h]) ? 1 : 0;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
#pragma unroll
  for (int h = 0; h < kCdMaxThr; ++h) {
    if (h < n_thr) {             // uniform
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) c[h] += __shfl_down(c[h], off);
    }
  }
  if (lane == 0) {
    wsum[wave] = s;
#pragma unroll
    for (int h = 0; h < kCdMaxThr; ++h) wcnt[wave][h] = c[h];
  }
  __syncthreads();
  if (tid == 0) {
    float* out = partials + (((size_t)blockIdx.z * B + i) * P + blockIdx.x) * kPairWords;
    out[0] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
#pragma unroll
    for (int h = 0; h < kCdMaxThr; ++h) out[1 + h] = __int_as_float(((wcnt[0][h] + wcnt[1][h]) + wcnt[2][h]) + wcnt[3][h]);
  }
}

// Per-pair values from the partials (include/gwtf.h), one wave: lane l owns pairs l, l + 64, ...; each adds its pair's partials in
// chunk order, evaluates the reference's float32 expressions, and keeps float64 running sums that a shuffle tree folds into the meter.
__global__ __launch_bounds__(64) void paired_finalise_kernel(const float* __restrict__ partials, const float* __restrict__ emd_cost,
                                                             float* __restrict__ cd, float* __restrict__ cdl, float* __restrict__ cdr,
                                                             float* __restrict__ emd, float* __restrict__ f1, double* __restrict__ meter,
                                                             int meter_head, int n_thr, int B, int n, int m, int P, int chunks_l,
                                                             int chunks_r, float inv_n) {
  const int lane = threadIdx.x;
  double m_cd = 0.0, m_emd = 0.0, m_f1[kCdMaxThr];
#pragma unroll
  for (int h = 0; h < kCdMaxThr; ++h) m_f1[h] = 0.0;
  for (int i = lane; i < B; i += 64) {
    const float* L = partials + (size_t)i * P * kPairWords;
    const float* R = partials + ((size_t)B + i) * P * kPairWords;
    float sl = 0.f, sr = 0.f;
    int cl[kCdMaxThr], cr[kCdMaxThr];
#pragma unroll
    for (int h = 0; h < kCdMaxThr; ++h) cl[h] = cr[h] = 0;
    for (int k = 0; k < chunks_l; ++k) {
      sl += L[(size_t)k * kPairWords];
#pragma unroll
      for (int h = 0; h < kCdMaxThr; ++h) cl[h] += __float_as_int(L[(size_t)k * kPairWords + 1 + h]);
    }
    for (int k = 0; k < chunks_r; ++k) {
      sr += R[(size_t)k * kPairWords];
#pragma unroll
      for (int h = 0; h < kCdMaxThr; ++h) cr[h] += __float_as_int(R[(size_t)k * kPairWords + 1 + h]);
    }
    const float vl = sl / (float)n, vr = sr / (float)m, v = vl + vr;
    if (cdl) cdl[i] = vl;
    if (cdr) cdr[i] = vr;
    if (cd) { cd[i] = v; m_cd += (double)v; }
#pragma unroll
    for (int h = 0; h < kCdMaxThr; ++h) {
      if (h < n_thr) {
        const float recall = 100.f * ((float)cl[h] / (float)n), precision = 100.f * ((float)cr[h] / (float)m);
        const float f = ((2.f * precision) * recall) / ((precision + recall) + 1e-7f);
        if (f1) f1[(size_t)h * B + i] = f;
        m_f1[h] += (double)f;
      }
    }
    if (emd_cost) {
      const float e = emd_cost[i] * inv_n;
      if (emd) emd[i] = e;
      m_emd += (double)e;
    }
  }
  if (!meter) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    m_cd += __shfl_down(m_cd, off);
    m_emd += __shfl_down(m_emd, off);
#pragma unroll
    for (int h = 0; h < kCdMaxThr; ++h) m_f1[h] += __shfl_down(m_f1[h], off);
  }
  if (lane == 0) {
    if (meter_head) {
      meter[0] += (double)B;
      if (cd) meter[1] += m_cd;
      if (emd_cost) meter[2] += m_emd;
    }
#pragma unroll
    for (int h = 0; h < kCdMaxThr; ++h) {
      if (h < n_thr) meter[3 + h] += m_f1[h];
    }
  }
}

// reference nndistance.cu:129-148: grad_a[j] += 2 g_j (a_j - b_idx[j]); grad_b[idx[j]] -= the same.  z = direction.
__global__ __launch_bounds__(256) void nnd_grad_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                       const float* __restrict__ gd1, const int* __restrict__ idx1,
                                                       const float* __restrict__ gd2, const int* __restrict__ idx2,
                                                       float* __restrict__ g1, float* __restrict__ g2, int b, int n, int m) {
  const bool rev = blockIdx.z == 1;
  const float* A = rev ? xyz2 : xyz1;
  const float* Bp = rev ? xyz1 : xyz2;
  const int na = rev ? m : n, nb = rev ? n : m;
  const float* gd = rev ? gd2 : gd1;
  const int* idx = rev ? idx2 : idx1;
  float* ga = rev ? g2 : g1;
  float* gb = rev ? g1 : g2;
  const int i = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= na) return;
  const int k = idx[(size_t)i * na + j];
  const float g = gd[(size_t)i * na + j] * 2.0f;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float diff = g * (A[((size_t)i * na + j) * 3 + d] - Bp[((size_t)i * nb + k) * 3 + d]);
    atomicAdd(&ga[((size_t)i * na + j) * 3 + d], diff);
    atomicAdd(&gb[((size_t)i * nb + k) * 3 + d], -diff);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Approximate EMD matching (reference approxmatch.cu:3-182): nine temperature levels -4^j, j = 7..-1; per level
//   (L) ratioL[k] = remainL[k] / (1e-9 + sum_l e_kl remainR[l])
//   (R) sumr = remainR[l] sum_k e_kl ratioL[k];  ratioR[l] = min(remainR[l]/(sumr+1e-9), 1) remainR[l];
//       remainR[l] = max(0, remainR[l] - sumr)
//   (M) w = e_kl ratioL[k] ratioR[l];  match[l][k] += w;  remainL[k] = max(0, remainL[k] - sum_l w)
// with e_kl = exp(level |a_k - b_l|^2).  The reference runs the whole schedule inside one workgroup per cloud pair (at
// most 32 workgroups on the device); here every sweep is its own launch over (tiles of 256 points) x (cloud pairs), so a
// batch of 64 pairs of 2048 points puts 512 workgroups on the 256 CUs, and the stream order is the barrier between
// sweeps.  exp(level d) is evaluated as exp2((level log2 e) d) with the bare v_exp_f32 (results below 2^-126 flush to 0).
// temp: [b][2(n+m)] = remainL[n] | remainR[m] | ratioL[n] | ratioR[m]
// Pair index i (blockIdx.y) owns temp / match / out slot i.  GRID = false: it is also the cloud index on both sides (cloud i of xyz1
// against cloud i of xyz2).  GRID = true (gwtf_emd_cost_pairs): the pairs are a rows x nb grid, A-cloud row0 + i / nb of xyz1 against
// B-cloud i % nb of xyz2 -- no expanded copy of either set.
constexpr int kEmdThreads = 256;
constexpr int kEmdTile = 1024;

struct EmdPair {
  const float* A; const float* Bp; float* M; float* remainL; float* remainR; float* ratioL; float* ratioR;
};
template <bool GRID>
__device__ inline EmdPair emd_pair(const float* xyz1, const float* xyz2, float* match, float* temp, int i, int n, int m, int nb,
                                   int row0) {
  EmdPair p;
  p.A = xyz1 + (size_t)(GRID ? row0 + i / nb : i) * n * 3;
  p.Bp = xyz2 + (size_t)(GRID ? i % nb : i) * m * 3;
  p.M = match + (size_t)i * n * m;
  p.remainL = temp + (size_t)i * (n + m) * 2;
  p.remainR = p.remainL + n;
  p.ratioL = p.remainR + m;
  p.ratioR = p.ratioL + n;
  return p;
}

__global__ __launch_bounds__(256) void emd_init_kernel(float* __restrict__ temp, int n, int m) {
  float* remainL = temp + (size_t)blockIdx.y * (n + m) * 2;
  const float multiL = n >= m ? 1.f : (float)(m / n), multiR = n >= m ? (float)(n / m) : 1.f;   // integer ratios (:6-12)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) remainL[t] = multiL;
  else if (t < n + m) remainL[t] = multiR;
}

// sum over the OTHER set of exp2(lvl2 |p - q|^2) * weight(q), q staged through LDS as (x,y,z,weight); p per thread.
//   MODE 0: plain sum (sweeps L and R)
//   MODE 1: sweep M, materialising match[q][p] += w (w = e * wp * weight(q); `pitch` = row length of match); lanes
//           whose w is exactly 0 skip the read-modify-write -- at the sharp early levels that is almost all of them
//   MODE 2: sweep M without the matrix: also returns sum_q w * |p - q| in `cost` (ApproxMatch + MatchCost fused)
template <int MODE>
__device__ inline float emd_sweep(const float* __restrict__ other, const float* __restrict__ weight, int cnt_other,
                                  float px, float py, float pz, float lvl2, float4* buf, float wp, float* __restrict__ Mcol,
                                  int pitch, bool valid, float& cost) {
  float acc = 0.f, c = 0.f;
  for (int l0 = 0; l0 < cnt_other; l0 += kEmdTile) {
    const int cnt = min(kEmdTile, cnt_other - l0);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt; t += kEmdThreads)
      buf[t] = make_float4(other[(l0 + t) * 3 + 0], other[(l0 + t) * 3 + 1], other[(l0 + t) * 3 + 2], weight[l0 + t]);
    __syncthreads();
    if (MODE == 1) {
      if (valid) {
#pragma unroll 4
        for (int l = 0; l < cnt; ++l) {
          const float4 q = buf[l];
          const float dx = q.x - px, dy = q.y - py, dz = q.z - pz;
          const float w = __builtin_amdgcn_exp2f(lvl2 * (dx * dx + dy * dy + dz * dz)) * wp * q.w;
          if (w != 0.f) Mcol[(size_t)(l0 + l) * pitch] += w;
          acc += w;
        }
      }
    } else if (MODE == 2) {
#pragma unroll 4
      for (int l = 0; l < cnt; ++l) {
        const float4 q = buf[l];
        const float dx = q.x - px, dy = q.y - py, dz = q.z - pz;
        const float d2 = dx * dx + dy * dy + dz * dz;
        const float w = __builtin_amdgcn_exp2f(lvl2 * d2) * wp * q.w;
        c += w * __builtin_amdgcn_sqrtf(d2);
        acc += w;
      }
    } else {
#pragma unroll 4
      for (int l = 0; l < cnt; ++l) {
        const float4 q = buf[l];
        const float dx = q.x - px, dy = q.y - py, dz = q.z - pz;
        acc += __builtin_amdgcn_exp2f(lvl2 * (dx * dx + dy * dy + dz * dz)) * q.w;
      }
    }
  }
  cost = c;
  return acc;
}

template <bool GRID>
__global__ __launch_bounds__(kEmdThreads) void emd_left_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                               float* __restrict__ temp, int n, int m, float lvl2, int nb,
                                                               int row0) {
  __shared__ float4 buf[kEmdTile];
  const EmdPair P = emd_pair<GRID>(xyz1, xyz2, nullptr, temp, blockIdx.y, n, m, nb, row0);
  const int k = blockIdx.x * kEmdThreads + threadIdx.x;
  const bool v = k < n;
  const float x1 = v ? P.A[k * 3] : 0.f, y1 = v ? P.A[k * 3 + 1] : 0.f, z1 = v ? P.A[k * 3 + 2] : 0.f;
  float unused;
  const float s = emd_sweep<0>(P.Bp, P.remainR, m, x1, y1, z1, lvl2, buf, 0.f, nullptr, 0, v, unused);
  if (v) P.ratioL[k] = P.remainL[k] / (1e-9f + s);
}

template <bool GRID>
__global__ __launch_bounds__(kEmdThreads) void emd_right_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                                float* __restrict__ temp, int n, int m, float lvl2, int nb,
                                                                int row0) {
  __shared__ float4 buf[kEmdTile];
  const EmdPair P = emd_pair<GRID>(xyz1, xyz2, nullptr, temp, blockIdx.y, n, m, nb, row0);
  const int l = blockIdx.x * kEmdThreads + threadIdx.x;
  const bool v = l < m;
  const float x2 = v ? P.Bp[l * 3] : 0.f, y2 = v ? P.Bp[l * 3 + 1] : 0.f, z2 = v ? P.Bp[l * 3 + 2] : 0.f;
  float unused;
  float sumr = emd_sweep<0>(P.A, P.ratioL, n, x2, y2, z2, lvl2, buf, 0.f, nullptr, 0, v, unused);
  if (v) {
    const float rr = P.remainR[l];
    sumr *= rr;
    P.ratioR[l] = fminf(rr / (sumr + 1e-9f), 1.0f) * rr;
    P.remainR[l] = fmaxf(0.0f, rr - sumr);
  }
}

template <bool FUSED, bool GRID>
__global__ __launch_bounds__(kEmdThreads) void emd_match_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                                float* __restrict__ match, float* __restrict__ temp,
                                                                float* __restrict__ out, int n, int m, float lvl2, int nb,
                                                                int row0) {
  __shared__ float4 buf[kEmdTile];
  __shared__ float part[kEmdThreads / 64];
  const EmdPair P = emd_pair<GRID>(xyz1, xyz2, match, temp, blockIdx.y, n, m, nb, row0);
  const int k = blockIdx.x * kEmdThreads + threadIdx.x;
  const bool v = k < n;
  const float x1 = v ? P.A[k * 3] : 0.f, y1 = v ? P.A[k * 3 + 1] : 0.f, z1 = v ? P.A[k * 3 + 2] : 0.f;
  const float rl = v ? P.ratioL[k] : 0.f;      // 0 for the padding lanes: they add nothing to the fused cost
  float c;
  const float s = emd_sweep<FUSED ? 2 : 1>(P.Bp, P.ratioR, m, x1, y1, z1, lvl2, buf, rl, FUSED ? nullptr : P.M + k, n, v, c);
  if (v) P.remainL[k] = fmaxf(0.0f, P.remainL[k] - s);
  if (FUSED) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < kEmdThreads / 64; ++w) t += part[w];
      atomicAdd(&out[blockIdx.y], t);
    }
  }
}

// out[i] = sum_{l,k} match[l][k] |a_k - b_l|   (reference approxmatch.cu:184-224).  grid = (column tiles, batch).
__global__ __launch_bounds__(256) void matchcost_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                        const float* __restrict__ match, float* __restrict__ out, int b,
                                                        int n, int m) {
  __shared__ float part[4];
  const int i = blockIdx.y;
  const float* A = xyz1 + (size_t)i * n * 3;
  const float* Bp = xyz2 + (size_t)i * m * 3;
  const float* M = match + (size_t)i * n * m;
  float sub = 0.f;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    const float x1 = A[k * 3], y1 = A[k * 3 + 1], z1 = A[k * 3 + 2];
    for (int l = 0; l < m; ++l) {
      const float dx = Bp[l * 3] - x1, dy = Bp[l * 3 + 1] - y1, dz = Bp[l * 3 + 2] - z1;   // wave-uniform loads
      sub += M[(size_t)l * n + k] * sqrtf(dx * dx + dy * dy + dz * dz);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sub += __shfl_down(sub, off);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sub;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&out[i], part[0] + part[1] + part[2] + part[3]);
}

// grad1[k] = sum_l match[l][k] (a_k - b_l) / max(|a_k - b_l|, 1e-10)      (reference :270-291)
__global__ __launch_bounds__(256) void matchcost_grad1_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                              const float* __restrict__ match, float* __restrict__ grad1,
                                                              int b, int n, int m) {
  const int i = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const float* A = xyz1 + (size_t)i * n * 3;
  const float* Bp = xyz2 + (size_t)i * m * 3;
  const float* M = match + (size_t)i * n * m;
  const float x1 = A[k * 3], y1 = A[k * 3 + 1], z1 = A[k * 3 + 2];
  float gx = 0.f, gy = 0.f, gz = 0.f;
  for (int l = 0; l < m; ++l) {
    const float dx = x1 - Bp[l * 3], dy = y1 - Bp[l * 3 + 1], dz = z1 - Bp[l * 3 + 2];
    const float d = M[(size_t)l * n + k] * rsqrtf(fmaxf(dx * dx + dy * dy + dz * dz, 1e-20f));
    gx += dx * d; gy += dy * d; gz += dz * d;
  }
  grad1[((size_t)i * n + k) * 3 + 0] = gx;
  grad1[((size_t)i * n + k) * 3 + 1] = gy;
  grad1[((size_t)i * n + k) * 3 + 2] = gz;
}

// grad2[l] = sum_k match[l][k] (b_l - a_k) / max(|b_l - a_k|, 1e-10)      (reference :229-269); one wave per l
__global__ __launch_bounds__(256) void matchcost_grad2_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                              const float* __restrict__ match, float* __restrict__ grad2,
                                                              int b, int n, int m) {
  const int i = blockIdx.y, l = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (l >= m) return;
  const float* A = xyz1 + (size_t)i * n * 3;
  const float* Bp = xyz2 + (size_t)i * m * 3;
  const float* M = match + ((size_t)i * m + l) * n;
  const float x2 = Bp[l * 3], y2 = Bp[l * 3 + 1], z2 = Bp[l * 3 + 2];
  float gx = 0.f, gy = 0.f, gz = 0.f;
  for (int k = lane; k < n; k += 64) {
    const float dx = x2 - A[k * 3], dy = y2 - A[k * 3 + 1], dz = z2 - A[k * 3 + 2];
    const float d = M[k] * rsqrtf(fmaxf(dx * dx + dy * dy + dz * dz, 1e-20f));
    gx += dx * d; gy += dy * d; gz += dz * d;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    gx += __shfl_down(gx, off); gy += __shfl_down(gy, off); gz += __shfl_down(gz, off);
  }
  if (lane == 0) {
    grad2[((size_t)i * m + l) * 3 + 0] = gx;
    grad2[((size_t)i * m + l) * 3 + 1] = gy;
    grad2[((size_t)i * m + l) * 3 + 2] = gz;
  }
}

}  // namespace

extern "C" int gwtf_nn_distance(const float* xyz1, const float* xyz2, float* dist1, int* idx1, float* dist2, int* idx2,
                                int b, int n, int m, void* stream) {
  if (!xyz1 || !xyz2 || !dist1 || !idx1 || !dist2 || !idx2 || b <= 0 || n <= 0 || m <= 0) return GWTF_E_BADARG;
  const int tiles = (max(n, m) + 511) / 512;
  hipLaunchKernelGGL(nnd_kernel, dim3(tiles, b, 2), dim3(256), 0, (hipStream_t)stream, xyz1, xyz2, dist1, idx1, dist2, idx2, b,
                     n, m);
  return (int)hipGetLastError();
}

extern "C" int gwtf_chamfer_directed(const float* q, const float* t, float* sum, int* cnt, const float* thr, int n_thr, int nq,
                                     int nt, int n, int m, void* stream) {
  if (!q || !t || !sum || nq <= 0 || nt <= 0 || n <= 0 || m <= 0 || n_thr < 0 || n_thr > kCdMaxThr) return GWTF_E_BADARG;
  if (n_thr > 0 && (!cnt || !thr)) return GWTF_E_BADARG;
  const long long groups = (nt + kCdGroup - 1) / kCdGroup;
  if (groups * nq > 0x7fffffffLL) return GWTF_E_BADARG;
  CdThr th;
  for (int h = 0; h < kCdMaxThr; ++h) th.v[h] = h < n_thr ? thr[h] : 0.f;
  hipLaunchKernelGGL(chamfer_directed_kernel, dim3((unsigned)(groups * nq)), dim3(256), 0, (hipStream_t)stream, q, t, sum, cnt, th,
                     n_thr, nq, nt, n, m);
  return (int)hipGetLastError();
}

extern "C" int gwtf_eval_frame(const GwtfEvalFrameArgs* pa) {
  if (!pa) return GWTF_E_BADARG;
  const GwtfEvalFrameArgs& a = *pa;
  if (!a.gen || !a.ref || !a.gen_out || !a.ref_out || a.B < 1 || a.B > 65535 || a.n < 1 || a.m < 1 || a.n_scale < 0 ||
      a.n_scale > 2 || (a.row_scale && !a.orig_s) || (a.row_shift && !a.orig_c))
    return GWTF_E_BADARG;
  hipLaunchKernelGGL(eval_frame_kernel, dim3((max(a.n, a.m) + 255) / 256, a.B, 2), dim3(256), 0, (hipStream_t)a.stream, a);
  return (int)hipGetLastError();
}

extern "C" int gwtf_chamfer_paired_partials(int n, int m) {
  return (n < 1 || m < 1) ? 0 : (max(n, m) + kPairSmallChunk - 1) / kPairSmallChunk;
}

// Query points per thread of a paired launch: a function of (B, n, m) alone, so gwtf_paired_finalise finds the chunks that were written.
static int paired_points_per_thread(int B, int n, int m) {
  const long long groups = (long long)((max(n, m) + kCdChunk - 1) / kCdChunk) * B * 2;
  return groups >= kPairFillGroups ? kCdPts : kPairSmallChunk / 256;
}

extern "C" int gwtf_chamfer_paired(const float* a, const float* b, float* partials, const float* thr, int n_thr, int B, int n, int m,
                                   void* stream) {
  if (!a || !b || !partials || B < 1 || B > 65535 || n < 1 || m < 1 || n_thr < 0 || n_thr > kCdMaxThr || (n_thr > 0 && !thr))
    return GWTF_E_BADARG;
  CdThr th;
  for (int h = 0; h < kCdMaxThr; ++h) th.v[h] = h < n_thr ? thr[h] : 0.f;
  const int P = gwtf_chamfer_paired_partials(n, m), pts = paired_points_per_thread(B, n, m);
  const dim3 grid((max(n, m) + 256 * pts - 1) / (256 * pts), B, 2);
  if (pts == kCdPts)
    hipLaunchKernelGGL(chamfer_paired_kernel<kCdPts>, grid, dim3(256), 0, (hipStream_t)stream, a, b, partials, th, n_thr, B, n, m, P);
  else
    hipLaunchKernelGGL(chamfer_paired_kernel<kPairSmallChunk / 256>, grid, dim3(256), 0, (hipStream_t)stream, a, b, partials, th, n_thr,
                       B, n, m, P);
  return (int)hipGetLastError();
}

extern "C" int gwtf_paired_finalise(const float* partials, const float* emd_cost, float* cd, float* cdl, float* cdr, float* emd,
                                    float* f1, double* meter, int meter_head, int n_thr, int B, int n, int m, void* stream) {
  if (!partials || B < 1 || B > 65535 || n < 1 || m < 1 || n_thr < 0 || n_thr > kCdMaxThr || (n_thr > 0 && !f1 && !meter) ||
      (emd && !emd_cost))
    return GWTF_E_BADARG;
  const int chunk = 256 * paired_points_per_thread(B, n, m);
  const float inv_n = (float)(1.0 / (double)n);
  hipLaunchKernelGGL(paired_finalise_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partials, emd_cost, cd, cdl, cdr, emd, f1,
                     meter, meter_head, n_thr, B, n, m, gwtf_chamfer_paired_partials(n, m), (n + chunk - 1) / chunk,
                     (m + chunk - 1) / chunk, inv_n);
  return (int)hipGetLastError();
}

extern "C" int gwtf_nn_distance_grad(const float* xyz1, const float* xyz2, const float* grad_dist1, const int* idx1,
                                     const float* grad_dist2, const int* idx2, float* grad_xyz1, float* grad_xyz2, int b,
                                     int n, int m, void* stream) {
  if (!xyz1 || !xyz2 || !grad_dist1 || !idx1 || !grad_dist2 || !idx2 || !grad_xyz1 || !grad_xyz2 || b <= 0 || n <= 0 || m <= 0)
    return GWTF_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(grad_xyz1, 0, sizeof(float) * (size_t)b * n * 3, st);
  if (e == hipSuccess) e = hipMemsetAsync(grad_xyz2, 0, sizeof(float) * (size_t)b * m * 3, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(nnd_grad_kernel, dim3((max(n, m) + 255) / 256, b, 2), dim3(256), 0, st, xyz1, xyz2, grad_dist1, idx1,
                     grad_dist2, idx2, grad_xyz1, grad_xyz2, b, n, m);
  return (int)hipGetLastError();
}

// b pairs; GRID: they are the rows x nb grid starting at A-cloud row0 (b = rows * nb), see emd_pair.
template <bool GRID>
static int emd_schedule(const float* xyz1, const float* xyz2, float* match, float* temp, float* out, int b, int n, int m,
                        hipStream_t st, int nb = 0, int row0 = 0) {
  hipError_t e = match ? hipMemsetAsync(match, 0, sizeof(float) * (size_t)b * n * m, st)
                       : hipMemsetAsync(out, 0, sizeof(float) * (size_t)b, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(emd_init_kernel, dim3((n + m + 255) / 256, b), dim3(256), 0, st, temp, n, m);
  const dim3 gl((n + kEmdThreads - 1) / kEmdThreads, b), gr((m + kEmdThreads - 1) / kEmdThreads, b);
  for (int j = 7; j > -2; --j) {   // approxmatch.cu:31-32
    const float lvl2 = -powf(4.0f, (float)j) * 1.4426950408889634f;
    hipLaunchKernelGGL(emd_left_kernel<GRID>, gl, dim3(kEmdThreads), 0, st, xyz1, xyz2, temp, n, m, lvl2, nb, row0);
    hipLaunchKernelGGL(emd_right_kernel<GRID>, gr, dim3(kEmdThreads), 0, st, xyz1, xyz2, temp, n, m, lvl2, nb, row0);
    if (match)
      hipLaunchKernelGGL((emd_match_kernel<false, GRID>), gl, dim3(kEmdThreads), 0, st, xyz1, xyz2, match, temp, out, n, m, lvl2,
                         nb, row0);
    else
      hipLaunchKernelGGL((emd_match_kernel<true, GRID>), gl, dim3(kEmdThreads), 0, st, xyz1, xyz2, match, temp, out, n, m, lvl2,
                         nb, row0);
  }
  return (int)hipGetLastError();
}

extern "C" int gwtf_approx_match(const float* xyz1, const float* xyz2, float* match, float* temp, int b, int n, int m,
                                 void* stream) {
  if (!xyz1 || !xyz2 || !match || !temp || b <= 0 || n <= 0 || m <= 0) return GWTF_E_BADARG;
  return emd_schedule<false>(xyz1, xyz2, match, temp, nullptr, b, n, m, (hipStream_t)stream);
}

extern "C" int gwtf_emd_cost(const float* xyz1, const float* xyz2, float* temp, float* out, int b, int n, int m,
                             void* stream) {
  if (!xyz1 || !xyz2 || !temp || !out || b <= 0 || n <= 0 || m <= 0) return GWTF_E_BADARG;
  return emd_schedule<false>(xyz1, xyz2, nullptr, temp, out, b, n, m, (hipStream_t)stream);
}

extern "C" int gwtf_emd_cost_pairs(const float* a, const float* b, float* temp, float* out, int na, int nb, int n, int m,
                                   int row0, int rows, void* stream) {
  if (!a || !b || !temp || !out || na <= 0 || nb <= 0 || n <= 0 || m <= 0 || row0 < 0 || rows <= 0 || rows > na - row0)
    return GWTF_E_BADARG;
  if ((long long)rows * nb > 65535) return GWTF_E_BADARG;   // the pair index is grid.y
  return emd_schedule<true>(a, b, nullptr, temp, out, rows * nb, n, m, (hipStream_t)stream, nb, row0);
}

extern "C" int gwtf_match_cost(const float* xyz1, const float* xyz2, const float* match, float* out, int b, int n, int m,
                               void* stream) {
  if (!xyz1 || !xyz2 || !match || !out || b <= 0 || n <= 0 || m <= 0) return GWTF_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(out, 0, sizeof(float) * (size_t)b, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(matchcost_kernel, dim3((n + 255) / 256, b), dim3(256), 0, st, xyz1, xyz2, match, out, b, n, m);
  return (int)hipGetLastError();
}

extern "C" int gwtf_match_cost_grad(const float* xyz1, const float* xyz2, const float* match, float* grad1, float* grad2,
                                    int b, int n, int m, void* stream) {
  if (!xyz1 || !xyz2 || !match || !grad1 || !grad2 || b <= 0 || n <= 0 || m <= 0) return GWTF_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(matchcost_grad1_kernel, dim3((n + 255) / 256, b), dim3(256), 0, st, xyz1, xyz2, match, grad1, b, n, m);
  hipLaunchKernelGGL(matchcost_grad2_kernel, dim3((m + 3) / 4, b), dim3(256), 0, st, xyz1, xyz2, match, grad2, b, n, m);
  return (int)hipGetLastError();
}
