// gwtf_film.hip -- per-shape FiLM conditioning vectors for every coupling of the stack (eval-mode BatchNorm).
//
// For coupling c and branch X in {logvar, mu} the reference evaluates two small MLPs on the latent g
// (lib/networks/flows.py:33-45 / 68-80, used at :100-101,105-106):
//     w = Linear_f->f( Swish( BN( Linear_G->f(g) ) ) ),   b = same structure, other weights
//     h <- (eps + exp(w)) * BN1(sd1(.)) + b
// This kernel produces, per (shape, coupling, branch, feature j), what the fused stack kernel consumes:
// c = c1 + b/a (start value of the sd1 accumulators), W2[0][j]*a, W2[1][j]*a, with a = eps + exp(w) > 0 and
// c1 the (eval-mode) sd1_bn shift -- relu(a*(y+c1)+b) = a*relu(y+c) -- plus the sd2 biases.  The train-mode heads (batch
// statistics over the latent rows) are csrc/gwtf_film_train.hip.
#include <hip/hip_runtime.h>
#include "gwtf_layout.h"
#include "../../include/gwtf.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Eval mode has no cross-shape dependency (BatchNorm is folded), so the grid also tiles B:
// one workgroup per (coupling, branch, tile of 16 shapes).  Both Linear layers of both heads run on
// v_mfma_f32_16x16x4_f32 (exact fp32, bitwise an fmaf chain) with the 16 shapes on M:
//     layer 1:  H[16 x FP]  = g_tile[16 x G] . L0T[G x FP]      per head, K = G
//     layer 2:  O[16 x FP]  = swish(bn(H))   . L1T[FP x FP]     per head, K = FP
// Wave w owns feature block w (16 output features) of BOTH heads, so the final a = eps + exp(w-head),
// c = c1 + b-head / a is computed in-lane from its two accumulators.  The contraction index is free to be
// renamed, so k-slot (step 4*kg + t, quarter q) is mapped to column 16*kg + 4*q + t: a lane's A operands
// of four consecutive MFMAs are four consecutive floats.  (History: a VALU version with operands read from
// L2 inside the dot-product loop took 89 us for 66 workgroups; VALU from LDS 24 us; MFMA with LDS-staged
// operands and a barrier per chunk 15-18 us -- every phase was a dependent load->sync->compute step.)
constexpr int kBTe = 16;   // shapes per workgroup = one MFMA M tile

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The whole kernel is one dependent chain (load -> 2 GEMMs -> exp), so it is written for latency: all
// operands of a K chunk are fetched straight from L2 into registers with independent, unpredicated loads
// issued back to back (no LDS staging, no barrier; L0T is zero-padded to a multiple of 16 rows by the packer
// and out-of-range latent columns / shapes are clamped, their products land on zero weights or discarded
// rows), the layer-2 weights are prefetched before layer 1 starts, and the only LDS traffic is the 16 x FP
// transpose of the hidden activations between the two layers.
// kGCH = latent columns per register-resident chunk: 128 keeps a G = 128 head in ONE load round (shortest chain; 150 VGPRs,
// 3 workgroups per CU), 64 takes two rounds but 4-5 workgroups fit a CU -- chosen when the grid exceeds one round of the
// former (the K x C couplings of a mixture: 19.8 -> 17.1 us on the airplane grid of 1056 workgroups).
// PerK: empty (gwtf_film_forward; the kernel as it always was, instruction for instruction), or (int Cper, long long g_stride_k) of
// gwtf_film_forward_k: coupling c reads the latent rows of ITS component -- K tables of B rows, g_stride_k floats apart, the couplings
// laid out component by component, Cper per component.
__device__ __forceinline__ size_t film_table_offset(int c, int Cper, long long g_stride_k) { return (size_t)(c / Cper) * (size_t)g_stride_k; }

template <int MB, int kGCH, class... PerK>
__global__ __launch_bounds__(MB > 4 ? 512 : 256) void film_eval_kernel(const float* __restrict__ g, const float* __restrict__ pf,
                                                        float* __restrict__ out, int B, int G, int C, int f, float eps, PerK... per_k) {
  constexpr int FP = 16 * MB;
  __shared__ __align__(16) float hb[2][16][FP + 4];   // [head][shape][feature]
  const int c = blockIdx.x, br = blockIdx.y, b0 = blockIdx.z * kBTe;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, i16 = lane & 15;
  const GwtfPackF P(FP, G);
  const int GP = P.GP();
  const float* w = pf + ((size_t)c * 2 + br) * P.branch_size();
  const size_t FS = gwtf_film_out_size(FP);
  const bool own = wave < MB;                        // this wave's feature block exists
  const int ft = 16 * wave + i16;                    // output feature owned by this lane (both heads)
  const int brow = b0 + i16;                         // shape whose latent row this lane feeds to the A operand
  const float* table = g;
  if constexpr (sizeof...(PerK) != 0) table += film_table_offset(c, per_k...);
  const float* grow = table + (size_t)(brow < B ? brow : B - 1) * G;
  const float* l0 = w + P.l0t(0) + 4 * ft;           // L0Q[col/4][ft][col%4] (gwtf_layout.h)
  const float* l1 = w + P.l0t(1) + 4 * ft;
  const bool gvec = (G & 3) == 0;                    // latent rows are 16-byte aligned and whole quads

  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  f32x4 w1[2][MB];                                   // layer-2 B operands (prefetched)
  if (own) {
#pragma unroll
    for (int kg = 0; kg < MB; ++kg)
#pragma unroll
      for (int which = 0; which < 2; ++which)
#pragma unroll
        for (int t = 0; t < 4; ++t) w1[which][kg][t] = w[P.l1t(which) + ((size_t)(4 * kg + q) * FP + ft) * 4 + t];   // L1Q: one dwordx4
    for (int i0 = 0; i0 < GP; i0 += kGCH) {
      f32x4 a4[kGCH / 16], b4[2][kGCH / 16];
#pragma unroll
      for (int kg = 0; kg < kGCH / 16; ++kg) {
        if (i0 + 16 * kg < GP) {                     // wave-uniform
          const int col = i0 + 16 * kg + 4 * q;      // k-slot (4*kg + t, q) <-> latent column col + t
          if (gvec) {
            a4[kg] = *reinterpret_cast<const f32x4*>(grow + (col < G ? col : G - 4));
          } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) a4[kg][t] = grow[col + t < G ? col + t : G - 1];
          }
          b4[0][kg] = *reinterpret_cast<const f32x4*>(l0 + (size_t)col * FP);   // (col/4) * FP * 4
          b4[1][kg] = *reinterpret_cast<const f32x4*>(l1 + (size_t)col * FP);
        }
      }
#pragma unroll
      for (int kg = 0; kg < kGCH / 16; ++kg) {
        if (i0 + 16 * kg < GP) {
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[kg][t], b4[0][kg][t], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[kg][t], b4[1][kg][t], acc[1], 0, 0, 0);
          }
        }
      }
    }
    // BatchNorm (folded) + Swish; hidden activations -> LDS for the layer-2 A operand
#pragma unroll
    for (int which = 0; which < 2; ++which) {
      const float sc = w[P.s(which) + ft], sh = w[P.t(which) + ft];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float h = fmaf(acc[which][r], sc, sh);
        hb[which][4 * q + r][ft] = h / (1.0f + expf(-h));
      }
    }
  }
  __syncthreads();
  if (!own) return;
  f32x4 o[2];
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    const float bias = w[P.l1b(which) + ft];
    o[which] = f32x4{bias, bias, bias, bias};
  }
#pragma unroll
  for (int kg = 0; kg < MB; ++kg) {
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(&hb[0][i16][16 * kg + 4 * q]);
    const f32x4 a1 = *reinterpret_cast<const f32x4*>(&hb[1][i16][16 * kg + 4 * q]);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      o[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[t], w1[0][kg][t], o[0], 0, 0, 0);
      o[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[t], w1[1][kg][t], o[1], 0, 0, 0);
    }
  }
  const float c1 = w[P.c1() + ft], w20 = w[P.w2() + ft], w21 = w[P.w2() + FP + ft];
  // NaN / Inf must reach the outputs (the reference aborts on a non-finite loss, training.py:43-46) although the stack
  // kernel's ReLU is a v_max that returns 0 for a NaN accumulator: a non-finite head output (non-finite latent or FiLM
  // weight) turns the whole record entry into NaN -- u = NaN survives the ReLU as relu(acc) * NaN -- and POISON (NaN when
  // any weight of the coupling is non-finite, gwtf_pack.hip) is added to the sd2 biases.  Bit tests: -fno-honor-nans.
  const float qnan = __builtin_bit_cast(float, 0x7fc00000u);
  const float poison = w[P.poison()];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = b0 + 4 * q + r;
    if (b < B) {
      float cv = 0.f, u0 = 0.f, u1 = 0.f;
      if (ft < f) {
        const float a = eps + expf(o[0][r]);
        cv = c1 + o[1][r] / a;
        u0 = w20 * a;
        u1 = w21 * a;
        if (gwtf_nonfinite(o[0][r]) || gwtf_nonfinite(o[1][r])) cv = u0 = u1 = qnan;
      }
      float* ob = out + ((size_t)b * C + c) * FS + (size_t)br * 3 * FP + ft;
      ob[0] = cv;
      ob[FP] = u0;
      ob[2 * FP] = u1;
      if (ft < 2) out[((size_t)b * C + c) * FS + 6 * FP + 2 * br + ft] = w[P.b2() + ft] + poison;
    }
  }
}

}  // namespace

extern "C" int gwtf_film_forward(const float* g, const float* packed_film, float* film_out, int B, int G, int C, int f, float eps,
                                 void* stream) {
  if (B <= 0 || G <= 0 || C <= 0 || f <= 0 || f > GWTF_MAX_FP || !g || !packed_film || !film_out) return GWTF_E_BADARG;
  const int FP = gwtf_padded_width(f);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(C, 2, (B + kBTe - 1) / kBTe);
  const bool many = (long)grid.x * grid.y * grid.z > 768;   // more than one round of 256 CUs x 3 resident workgroups
  // one wavefront per block of 16 output features: 4 wavefronts up to f = 64, 8 beyond (f <= 128)
#define GWTF_FILM_EVAL(MB_)                                                                                                  \
  if (many) hipLaunchKernelGGL((film_eval_kernel<MB_, 64>), grid, dim3(MB_ > 4 ? 512 : 256), 0, st, g, packed_film, film_out, B, G, C, f, eps); \
  else hipLaunchKernelGGL((film_eval_kernel<MB_, 128>), grid, dim3(MB_ > 4 ? 512 : 256), 0, st, g, packed_film, film_out, B, G, C, f, eps)
  switch (FP / 16) {
    case 1: GWTF_FILM_EVAL(1); break;
    case 2: GWTF_FILM_EVAL(2); break;
    case 3: GWTF_FILM_EVAL(3); break;
    case 4: GWTF_FILM_EVAL(4); break;
    case 5: GWTF_FILM_EVAL(5); break;
    case 6: GWTF_FILM_EVAL(6); break;
    case 7: GWTF_FILM_EVAL(7); break;
    default: GWTF_FILM_EVAL(8); break;
  }
#undef GWTF_FILM_EVAL
  return (int)hipGetLastError();
}

extern "C" int gwtf_film_forward_k(const float* g, const float* packed_film, float* film_out, int B, int G, int K, int Cper, int f, float eps,
                                   long long g_stride_k, void* stream) {
  if (B <= 0 || G <= 0 || K <= 0 || Cper <= 0 || (long long)K * Cper > 0x7fffffffLL || g_stride_k < 0 || f <= 0 || f > GWTF_MAX_FP || !g ||
      !packed_film || !film_out)
    return GWTF_E_BADARG;
  const int FP = gwtf_padded_width(f), C = K * Cper;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(C, 2, (B + kBTe - 1) / kBTe);
  const bool many = (long)grid.x * grid.y * grid.z > 768;   // the choice of gwtf_film_forward at the same grid
#define GWTF_FILM_EVAL_K(MB_)                                                                                                \
  if (many) hipLaunchKernelGGL((film_eval_kernel<MB_, 64, int, long long>), grid, dim3(MB_ > 4 ? 512 : 256), 0, st, g, packed_film, film_out, B, G, C, f, eps, Cper, g_stride_k); \
  else hipLaunchKernelGGL((film_eval_kernel<MB_, 128, int, long long>), grid, dim3(MB_ > 4 ? 512 : 256), 0, st, g, packed_film, film_out, B, G, C, f, eps, Cper, g_stride_k)
  switch (FP / 16) {
    case 1: GWTF_FILM_EVAL_K(1); break;
    case 2: GWTF_FILM_EVAL_K(2); break;
    case 3: GWTF_FILM_EVAL_K(3); break;
    case 4: GWTF_FILM_EVAL_K(4); break;
    case 5: GWTF_FILM_EVAL_K(5); break;
    case 6: GWTF_FILM_EVAL_K(6); break;
    case 7: GWTF_FILM_EVAL_K(7); break;
    default: GWTF_FILM_EVAL_K(8); break;
  }
#undef GWTF_FILM_EVAL_K
  return (int)hipGetLastError();
}
