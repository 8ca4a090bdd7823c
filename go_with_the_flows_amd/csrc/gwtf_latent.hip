// gwtf_latent.hip -- the latent-space loss terms of the training step and their combination with the point NLL, two small launches forward and
// one backward (reference lib/networks/losses.py:24-33 GaussianFlowNLL, :36-41 GaussianEntropy, :159-170 Flow_Mixture_Loss.forward):
//     gnll = 0.5 ( sum_{b,j} [ lv0_j + sum_l flow_lv[l][b][j] + (z_bj - mu0_j)^2 / exp(lv0_j) ] / B + G log 2 pi )
//     gent = 0.5 ( G (1 + log 2 pi) + sum_{b,j} post_lv_bj / B )
//     pnll = sum_b nll_b / B            loss = pw pnll + gw gnll - ew gent
// As torch ops these are ~25 elementwise / reduction launches forward and ~30 backward on (B, G) tensors of a few thousand elements:
// 0.15 ms of a 9 ms step spent on launch latency.
// One record (include/gwtf.h GwtfLatentLossArgs), two families by its `rows` field: the base Gaussian shared by the batch (mu0, lv0
// [G]: the generative / autoencoding models' learned parameters) and one base Gaussian per row (mu0, lv0 [B][G]: the single-view
// reconstruction model's g0_prior(img_encoder(images))); the per-row family reads mu0[e] / lv0[e] where the shared one reads
// mu0[e % G], and its backward has no column sums.
#include <hip/hip_runtime.h>
#include "../../include/gwtf.h"

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float block_sum(float v, float* red, int tid) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  float s = 0.f;
  for (int w = 0; w < kThreads / 64; ++w) s += red[w];      // every thread: the same order
  __syncthreads();
  return s;
}

// stage 1: one element per thread (the n2 flow_lv loads of a thread are independent and coalesced across the wave);
// part[blk] = {sum of the gnll integrand, sum of post_lv} of the block's 256 elements
template <bool kRows>
__global__ __launch_bounds__(kThreads) void latent_part_kernel(const float* __restrict__ z, const float* __restrict__ mu0,
                                                               const float* __restrict__ lv0, const float* __restrict__ flow_lv,
                                                               const float* __restrict__ post_lv, float2* __restrict__ part, int B,
                                                               int G, int n2) {
  __shared__ float red[kThreads / 64];
  const int tid = threadIdx.x, n = B * G, e = blockIdx.x * kThreads + tid;
  float sg = 0.f, se = 0.f;
  if (e < n) {
    const int j = kRows ? e : e % G;                   // the element's base Gaussian: its own, or its column's
    const float d = z[e] - mu0[j], l0 = lv0[j];
    float s0 = 0.f, s1 = 0.f;
    int l = 0;
    for (; l + 1 < n2; l += 2) {
      s0 += flow_lv[(size_t)l * n + e];
      s1 += flow_lv[(size_t)(l + 1) * n + e];
    }
    if (l < n2) s0 += flow_lv[(size_t)l * n + e];
    sg = l0 + d * d * __expf(-l0) + (s0 + s1);
    se = post_lv[e];
  }
  sg = block_sum(sg, red, tid);
  se = block_sum(se, red, tid);
  if (tid == 0) part[blockIdx.x] = make_float2(sg, se);
}

// stage 2 (one workgroup): the partials in block order + the per-shape point NLL -> out[4] = {loss, pnll, gnll, gent}
__global__ __launch_bounds__(kThreads) void latent_finish_kernel(const float* __restrict__ nll, const float2* __restrict__ part,
                                                                 float* __restrict__ out, int B, int G, int nb, float pw, float gw,
                                                                 float ew) {
  __shared__ float red[kThreads / 64];
  const int tid = threadIdx.x;
  float sg = 0.f, se = 0.f, sp = 0.f;
  for (int i = tid; i < nb; i += kThreads) {
    const float2 v = part[i];
    sg += v.x;
    se += v.y;
  }
  for (int b = tid; b < B; b += kThreads) sp += nll[b];
  sg = block_sum(sg, red, tid);
  se = block_sum(se, red, tid);
  sp = block_sum(sp, red, tid);
  if (tid == 0) {
    const float log2pi = 1.8378770664093453f;
    const float gnll = 0.5f * (sg / (float)B + log2pi * (float)G);
    const float gent = 0.5f * ((float)G * (1.0f + log2pi) + se / (float)B);
    const float pnll = sp / (float)B;
    out[0] = pw * pnll + gw * gnll - ew * gent;
    out[1] = pnll;
    out[2] = gnll;
    out[3] = gent;
  }
}

// g_out[4] = upstream of {loss, pnll, gnll, gent}.  Blocks [0, nb_e): elementwise part; the rest: the column sums of mu0 / lv0.
__global__ __launch_bounds__(kThreads) void latent_bwd_kernel(const float* __restrict__ g_out, const float* __restrict__ z,
                                                         const float* __restrict__ mu0, const float* __restrict__ lv0,
                                                         float* __restrict__ g_nll, float* __restrict__ g_z, float* __restrict__ g_mu0,
                                                         float* __restrict__ g_lv0, float* __restrict__ g_flow, float* __restrict__ g_post,
                                                         int B, int G, int n2, float pw, float gw, float ew, int nb_e) {
  const float gl = g_out[0];
  const float cp = (gl * pw + g_out[1]) / (float)B, cg = (gl * gw + g_out[2]) / (float)B, ce = (g_out[3] - gl * ew) / (float)B;
  const int n = B * G;
  if ((int)blockIdx.x < nb_e) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e < B) g_nll[e] = cp;
    if (e >= n) return;
    const int j = e % G;
    g_z[e] = cg * (z[e] - mu0[j]) * __expf(-lv0[j]);
    g_post[e] = 0.5f * ce;
    const float c = 0.5f * cg;
    for (int l = 0; l < n2; ++l) g_flow[(size_t)l * n + e] = c;
    return;
  }
  const int j = ((int)blockIdx.x - nb_e) * kThreads + threadIdx.x;
  if (j >= G) return;
  const float m = mu0[j], r = __expf(-lv0[j]);
  float sm = 0.f, sl = 0.f;
  for (int b = 0; b < B; ++b) {
    const float d = z[(size_t)b * G + j] - m;
    sm += d;
    sl = fmaf(d, d, sl);
  }
  g_mu0[j] = -cg * r * sm;
  g_lv0[j] = 0.5f * cg * ((float)B - r * sl);
}

// per-row base: every gradient is elementwise (mu0 / lv0 have the shape of z), one element per thread
__global__ __launch_bounds__(kThreads) void latent_rows_bwd_kernel(const float* __restrict__ g_out, const float* __restrict__ z,
                                                              const float* __restrict__ mu0, const float* __restrict__ lv0,
                                                              float* __restrict__ g_nll, float* __restrict__ g_z,
                                                              float* __restrict__ g_mu0, float* __restrict__ g_lv0,
                                                              float* __restrict__ g_flow, float* __restrict__ g_post, int B, int G,
                                                              int n2, float pw, float gw, float ew) {
  const float gl = g_out[0];
  const float cp = (gl * pw + g_out[1]) / (float)B, cg = (gl * gw + g_out[2]) / (float)B, ce = (g_out[3] - gl * ew) / (float)B;
  const int n = B * G, e = blockIdx.x * kThreads + threadIdx.x;
  if (e < B) g_nll[e] = cp;
  if (e >= n) return;
  const float d = z[e] - mu0[e], r = __expf(-lv0[e]);
  const float gz = cg * d * r;
  g_z[e] = gz;
  g_mu0[e] = -gz;
  g_lv0[e] = 0.5f * cg * (1.0f - r * d * d);
  g_post[e] = 0.5f * ce;
  const float c = 0.5f * cg;
  for (int l = 0; l < n2; ++l) g_flow[(size_t)l * n + e] = c;
}

// B * G elements in blocks of kThreads: 0 when there are none or the product does not fit an int (the element index of the kernels)
int latent_blocks(int B, int G) {
  const long long n = (long long)B * G;
  return B <= 0 || G <= 0 || n > 0x7fffffffLL - kThreads ? 0 : (int)((n + kThreads - 1) / kThreads);
}

// the sizes and the family of a record, before its pointers: 0 blocks = refused
int latent_blocks(const GwtfLatentLossArgs* a) { return !a || a->n2 <= 0 || a->rows < 0 || a->rows > 1 ? 0 : latent_blocks(a->B, a->G); }

}  // namespace

extern "C" int gwtf_latent_loss_workspace_floats(int B, int G) { return 2 * latent_blocks(B, G); }

extern "C" int gwtf_latent_loss_forward(const GwtfLatentLossArgs* a) {
  const int nb = latent_blocks(a);
  if (nb == 0 || !a->nll || !a->z || !a->mu0 || !a->lv0 || !a->flow_lv || !a->post_lv || !a->workspace || !a->out4) return GWTF_E_BADARG;
  hipStream_t st = (hipStream_t)a->stream;
  float2* part = (float2*)a->workspace;
  hipLaunchKernelGGL(a->rows == 0 ? latent_part_kernel<false> : latent_part_kernel<true>, dim3(nb), dim3(kThreads), 0, st, a->z, a->mu0, a->lv0,
                     a->flow_lv, a->post_lv, part, a->B, a->G, a->n2);
  hipLaunchKernelGGL(latent_finish_kernel, dim3(1), dim3(kThreads), 0, st, a->nll, (const float2*)part, a->out4, a->B, a->G, nb, a->pw,
                     a->gw, a->ew);
  return (int)hipGetLastError();
}

extern "C" int gwtf_latent_loss_backward(const GwtfLatentLossArgs* a) {
  const int nb = latent_blocks(a);
  if (nb == 0 || !a->g_out4 || !a->z || !a->mu0 || !a->lv0 || !a->g_nll || !a->g_z || !a->g_mu0 || !a->g_lv0 || !a->g_flow_lv ||
      !a->g_post_lv)
    return GWTF_E_BADARG;
  hipStream_t st = (hipStream_t)a->stream;
  if (a->rows) {
    hipLaunchKernelGGL(latent_rows_bwd_kernel, dim3(nb), dim3(kThreads), 0, st, a->g_out4, a->z, a->mu0, a->lv0, a->g_nll, a->g_z,
                       a->g_mu0, a->g_lv0, a->g_flow_lv, a->g_post_lv, a->B, a->G, a->n2, a->pw, a->gw, a->ew);
  } else {
    const int nb_c = (a->G + kThreads - 1) / kThreads;      // the column sums of mu0 / lv0 behind the elementwise blocks
    hipLaunchKernelGGL(latent_bwd_kernel, dim3(nb + nb_c), dim3(kThreads), 0, st, a->g_out4, a->z, a->mu0, a->lv0, a->g_nll, a->g_z,
                       a->g_mu0, a->g_lv0, a->g_flow_lv, a->g_post_lv, a->B, a->G, a->n2, a->pw, a->gw, a->ew, nb);
  }
  return (int)hipGetLastError();
}
