// gwtf_conv2d.hip -- the three passes of a bias-free, dilation-1, groups-1 2-D convolution on contiguous NCHW float32: the
// convolutions of the image encoder in train mode (go_with_the_flows_amd/conv2d.py; include/gwtf.h GwtfConv2dArgs).
//
// All three are ONE implicit-GEMM kernel, D[row][col] = sum_k A[row][k] * B[k][col], on v_mfma_f32_16x16x4_f32 (exact fp32
// products, as gwtf_resnet.hip and gwtf_gemm.h), with the pass deciding what the operands are:
//
//   pass              rows        cols (fastest in memory)     k                    A (rows x k)             B (k x cols)
//   forward           Cout        output pixel (n, oy, ox)     (ci, ky, kx)         w, as torch stores it    x, gathered
//   backward_input    Cin         input pixel (n, iy, ix)      (co, ky, kx)         w transposed (pre-pass)  dy, gathered
//   backward_weight   Cout        (ci, ky, kx)                 pixel (n, oy, ox)    dy                       x, gathered
//
// The COLUMN index is the one that is contiguous in the output tensor, and the MFMA's D layout puts 16 consecutive columns in
// 16 consecutive lanes (lane = 16 q + r holds D[4 q + e][r], e = 0..3): every store instruction writes 64-byte runs.  For the
// same reason the gathered operand is read with r along the pixels of an image row (forward, backward_input).
//
// Lane (r, q) holds, of a 16-wide K step, the four k values 4 q .. 4 q + 3 of row r (A) and of column r (B); MFMA e of the step
// consumes element e of both (the same k order on both sides is all a contraction needs).  With A dense, [rows][K] and K a
// multiple of 4, that is one 16-byte load.  Operands come straight from L2 into registers, no LDS; a workgroup's four waves
// each own a 32 x 32 output tile.
//
// Memory safety: every address is clamped into its tensor BEFORE the load -- rows and columns beyond the matrix, k beyond K,
// padding taps, and (backward_input) the output positions that a stride-2 grid does not have -- and the loaded value is zeroed
// afterwards where the clamp moved it; there is no exec-masked branch per load.  Stores are masked to the matrix.
//
// Accumulation: step u of a pass (kU = 4 steps whose loads are issued together) goes into accumulator set u, four independent
// chains per output tile that are combined pairwise at the end (AccSets of gwtf_resnet.hip: a k-ordered fma chain's rounding
// error grows with its length -- K = 4608 at layer4, hundreds of thousands of pixels for dw).  backward_weight additionally
// splits the pixels over blockIdx.z; each split writes its partial dw to the workspace and reduce_splits adds them in the
// FIXED order 0 .. S-1.  No float atomics anywhere: two launches give the same bits.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <algorithm>
#include "../../include/gwtf.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kU = 4;            // K steps (16 k each) whose loads are issued together; also the number of accumulator sets
constexpr int kT = 2;            // 16 x 16 tiles per wave along rows and along columns: a wave owns 32 x 32, a workgroup 64 x 64
constexpr int kBlock = 32 * kT;
constexpr int kMaxSplit = 64;

enum { FWD = GWTF_CONV2D_FORWARD, DX = GWTF_CONV2D_BACKWARD_INPUT, DW = GWTF_CONV2D_BACKWARD_WEIGHT };

struct Gemm {
  const float* a;                // FWD: w [Cout][K]; DX: w transposed [Cin][K]; DW: dy [N][Cout][Ho][Wo]
  const float* b;                // FWD, DW: x [N][Cin][H][W]; DX: dy
  float* out;                    // FWD: y; DX: dx; DW: dw (S = 1)
  float* part;                   // DW, S > 1: [S][rows][cols]
  int N, Cin, H, W, Cout, Ho, Wo;
  int shift, pad;                // stride = 1 << shift
  int rows, cols, K;
  int steps_per_split;
};

// (ky, kx) of tap t of a KS x KS window
template <int KS>
__device__ __forceinline__ void tap_of(int t, int& ky, int& kx) {
  ky = t / KS;
  kx = t - ky * KS;
}

template <int MODE, int KS>
__global__ __launch_bounds__(kThreads) void conv_gemm(Gemm g) {
  constexpr int KK = KS * KS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int col_base = blockIdx.x * kBlock + (wave & 1) * (16 * kT);
  const int row_base = blockIdx.y * kBlock + (wave >> 1) * (16 * kT);
  const int HW = g.H * g.W, HoWo = g.Ho * g.Wo;
  const int stride = 1 << g.shift;

  // ---- what this lane's rows and columns are (fixed for the whole contraction) ----
  int arow[kT];                  // clamped row of the A operand
#pragma unroll
  for (int i = 0; i < kT; ++i) arow[i] = min(row_base + 16 * i + r16, g.rows - 1);

  // FWD / DX: column = pixel (n, py, px) of the output tensor; cb = the image's first plane in the gathered tensor, (y0, x0) the
  // window origin.  DW: column = (ci, ky, kx); cb = the plane offset of ci inside an image, (y0, x0) the tap's shift.
  size_t cb[kT];
  int y0[kT], x0[kT];
  size_t ostore[kT];             // FWD / DX: offset of (n, row 0, py, px) in the output tensor
#pragma unroll
  for (int j = 0; j < kT; ++j) {
    const int col = min(col_base + 16 * j + r16, g.cols - 1);
    if (MODE == DW) {
      const int ci = col / KK;
      int ky, kx;
      tap_of<KS>(col - ci * KK, ky, kx);
      cb[j] = (size_t)ci * HW;
      y0[j] = ky - g.pad;
      x0[j] = kx - g.pad;
      ostore[j] = 0;
    } else {
      const int plane = MODE == FWD ? HoWo : HW, width = MODE == FWD ? g.Wo : g.W;
      const int n = col / plane, rem = col - n * plane;
      const int py = rem / width, px = rem - py * width;
      if (MODE == FWD) {
        cb[j] = (size_t)n * g.Cin * HW;
        y0[j] = py * stride - g.pad;
        x0[j] = px * stride - g.pad;
      } else {
        cb[j] = (size_t)n * g.Cout * HoWo;
        y0[j] = py + g.pad;
        x0[j] = px + g.pad;
      }
      ostore[j] = (size_t)n * g.rows * plane + rem;
    }
  }

  f32x4 sets[kU][kT][kT];
#pragma unroll
  for (int u = 0; u < kU; ++u)
#pragma unroll
    for (int i = 0; i < kT; ++i)
#pragma unroll
      for (int j = 0; j < kT; ++j) sets[u][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int total_steps = (g.K + 15) / 16;
  const int t_begin = blockIdx.z * g.steps_per_split;
  const int t_end = min(t_begin + g.steps_per_split, total_steps);
  const int k_end = min(t_end * 16, g.K);          // k >= k_end: clamped address, both operands zeroed
  const int Hm = g.H - 1, Wm = g.W - 1, Hom = g.Ho - 1, Wom = g.Wo - 1;

  for (int t = t_begin; t < t_end; t += kU) {
    f32x4 av[kU][kT], bv[kU][kT];
    bool aok[kU][4], bok[kU][kT][4];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int k0 = (t + u) * 16 + 4 * q;           // this lane's four k values: k0 .. k0 + 3
      if (MODE != DW) {
        // A: one 16-byte load from the dense [rows][K] matrix (K is a multiple of 4: the four k are inside K together or not at all)
        const int ka = min(k0, g.K - 4);
#pragma unroll
        for (int i = 0; i < kT; ++i) av[u][i] = *reinterpret_cast<const f32x4*>(g.a + (size_t)arow[i] * g.K + ka);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = k0 + e;
          aok[u][e] = k < k_end;
          const int kc = min(k, g.K - 1);
          const int c = kc / KK;                       // FWD: ci; DX: co
          int ky, kx;
          tap_of<KS>(kc - c * KK, ky, kx);
#pragma unroll
          for (int j = 0; j < kT; ++j) {
            if (MODE == FWD) {
              const int iy = y0[j] + ky, ix = x0[j] + kx;
              bok[u][j][e] = aok[u][e] && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
              bv[u][j][e] = g.b[cb[j] + (size_t)c * HW + (size_t)min(max(iy, 0), Hm) * g.W + min(max(ix, 0), Wm)];
            } else {
              // dy[n][co][ty / stride][tx / stride] where the division is exact and the position exists
              const int ty = y0[j] - ky, tx = x0[j] - kx;
              const int oy = max(ty, 0) >> g.shift, ox = max(tx, 0) >> g.shift;
              bok[u][j][e] = aok[u][e] && ty >= 0 && tx >= 0 && ((ty | tx) & (stride - 1)) == 0 && oy < g.Ho && ox < g.Wo;
              bv[u][j][e] = g.b[cb[j] + (size_t)c * HoWo + (size_t)min(oy, Hom) * g.Wo + min(ox, Wom)];
            }
          }
        }
      } else {
        // k = pixel (n, oy, ox) of dy: one division per step, then the four k walk along the row
        const int kc = min(k0, g.K - 1);
        int n = kc / HoWo;
        const int rem = kc - n * HoWo;
        int oy = rem / g.Wo, ox = rem - oy * g.Wo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          aok[u][e] = k0 + e < k_end;
          const size_t pix = (size_t)oy * g.Wo + ox;
#pragma unroll
          for (int i = 0; i < kT; ++i) av[u][i][e] = g.a[((size_t)n * g.Cout + arow[i]) * HoWo + pix];
          const size_t img = (size_t)n * g.Cin * HW;
#pragma unroll
          for (int j = 0; j < kT; ++j) {
            const int iy = oy * stride + y0[j], ix = ox * stride + x0[j];
            bok[u][j][e] = aok[u][e] && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
            bv[u][j][e] = g.b[img + cb[j] + (size_t)min(max(iy, 0), Hm) * g.W + min(max(ix, 0), Wm)];
          }
          if (k0 + e + 1 < g.K) {                      // the next pixel; the last one stays where it is (clamped, zeroed)
            if (++ox == g.Wo) {
              ox = 0;
              if (++oy == g.Ho) { oy = 0; ++n; }
            }
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int i = 0; i < kT; ++i)
          if (!aok[u][e]) av[u][i][e] = 0.f;
#pragma unroll
        for (int j = 0; j < kT; ++j)
          if (!bok[u][j][e]) bv[u][j][e] = 0.f;
      }
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < kT; ++i)
#pragma unroll
          for (int j = 0; j < kT; ++j)
            sets[u][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][i][e], bv[u][j][e], sets[u][i][j], 0, 0, 0);
  }

  // ---- the four chains combined pairwise in a fixed order; masked stores ----
  float* part = MODE == DW && gridDim.z > 1 ? g.part + (size_t)blockIdx.z * g.rows * g.cols : g.out;
#pragma unroll
  for (int j = 0; j < kT; ++j) {
    const int col = col_base + 16 * j + r16;
#pragma unroll
    for (int i = 0; i < kT; ++i) {
      const f32x4 acc = (sets[0][i][j] + sets[1][i][j]) + (sets[2][i][j] + sets[3][i][j]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = row_base + 16 * i + 4 * q + e;
        if (row < g.rows && col < g.cols) {
          if (MODE == DW) part[(size_t)row * g.cols + col] = acc[e];
          else g.out[ostore[j] + (size_t)row * (MODE == FWD ? HoWo : HW)] = acc[e];
        }
      }
    }
  }
}

// wt[ci][co * KK + tap] = w[co][ci * KK + tap]: the dense A operand of backward_input.
__global__ __launch_bounds__(kThreads) void transpose_w(const float* __restrict__ w, float* __restrict__ wt, int Cout, int Cin,
                                                        int KK) {
  const size_t total = (size_t)Cout * Cin * KK;
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int tap = (int)(i % KK);
  const size_t r = i / KK;
  const int ci = (int)(r % Cin), co = (int)(r / Cin);
  wt[((size_t)ci * Cout + co) * KK + tap] = w[i];
}

// dw = the S partial matrices added in split order, four values per thread (total is a multiple of 4).
__global__ __launch_bounds__(kThreads) void reduce_splits(const float* __restrict__ part, int S, size_t total4,
                                                          float* __restrict__ out) {
  const size_t i4 = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i4 >= total4) return;
  const f32x4* p = reinterpret_cast<const f32x4*>(part) + i4;
  f32x4 v = p[0];
  for (int s = 1; s < S; ++s) v += p[(size_t)s * total4];
  reinterpret_cast<f32x4*>(out)[i4] = v;
}

// ---- host side: validation, the GEMM each pass is, the split rule ---------------------------------------------------------------

struct Plan {
  int Ho, Wo, shift;
  int rows, cols, K;
  int S, steps_per_split;
  size_t work_floats;
};

constexpr long long kIndexLimit = (1LL << 31) - 256;     // room for the K steps a pass issues beyond the last one

int make_plan(const GwtfConv2dArgs* a, int pass, Plan& P) {
  if (!a) return GWTF_E_BADARG;
  if (pass != FWD && pass != DX && pass != DW) return GWTF_E_BADARG;
  if (a->N < 1 || a->Cin < 1 || a->H < 1 || a->W < 1 || a->Cout < 1 || a->k < 1 || a->stride < 1 || a->pad < 0) return GWTF_E_BADARG;
  if (a->N > 65535) return GWTF_E_BADARG;
  if (a->k != 1 && a->k != 3 && a->k != 7) return GWTF_E_UNSUPPORTED;
  if (a->stride != 1 && a->stride != 2) return GWTF_E_UNSUPPORTED;
  if (a->pad != a->k / 2) return GWTF_E_UNSUPPORTED;
  if (a->Cout % 16) return GWTF_E_UNSUPPORTED;
  if (a->Cin % 16 && !(a->Cin == 4 && a->k == 7)) return GWTF_E_UNSUPPORTED;
  P.Ho = (a->H + 2 * a->pad - a->k) / a->stride + 1;
  P.Wo = (a->W + 2 * a->pad - a->k) / a->stride + 1;
  P.shift = a->stride - 1;
  const long long KK = (long long)a->k * a->k;
  const long long xn = (long long)a->N * a->Cin * a->H * a->W, yn = (long long)a->N * a->Cout * P.Ho * P.Wo;
  const long long wn = (long long)a->Cout * a->Cin * KK;
  if (xn >= kIndexLimit || yn >= kIndexLimit || wn >= kIndexLimit) return GWTF_E_BADARG;   // every index fits an int
  long long rows, cols, K;
  if (pass == FWD) { rows = a->Cout; cols = (long long)a->N * P.Ho * P.Wo; K = a->Cin * KK; }
  else if (pass == DX) { rows = a->Cin; cols = (long long)a->N * a->H * a->W; K = a->Cout * KK; }
  else { rows = a->Cout; cols = a->Cin * KK; K = (long long)a->N * P.Ho * P.Wo; }
  P.rows = (int)rows; P.cols = (int)cols; P.K = (int)K;
  const int steps = (P.K + 15) / 16;
  int S = 1;
  if (pass == DW) {
    // enough workgroups to fill the device twice over, every split at least 16 steps (256 pixels) long
    const long long tiles = ((rows + kBlock - 1) / kBlock) * ((cols + kBlock - 1) / kBlock);
    S = (int)std::min<long long>((512 + tiles - 1) / tiles, std::min(kMaxSplit, steps / 16));
    S = std::max(S, 1);
  }
  P.steps_per_split = (steps + S - 1) / S;
  P.S = (steps + P.steps_per_split - 1) / P.steps_per_split;      // no empty split
  P.work_floats = pass == DX ? (size_t)wn : pass == DW && P.S > 1 ? (size_t)P.S * rows * cols : 0;
  return 0;
}

template <int MODE>
void launch(const Gemm& g, int k, int S, hipStream_t stream) {
  const dim3 grid((g.cols + kBlock - 1) / kBlock, (g.rows + kBlock - 1) / kBlock, S);
  if (k == 1) hipLaunchKernelGGL((conv_gemm<MODE, 1>), grid, dim3(kThreads), 0, stream, g);
  else if (k == 3) hipLaunchKernelGGL((conv_gemm<MODE, 3>), grid, dim3(kThreads), 0, stream, g);
  else hipLaunchKernelGGL((conv_gemm<MODE, 7>), grid, dim3(kThreads), 0, stream, g);
}

Gemm gemm_of(const GwtfConv2dArgs* a, const Plan& P) {
  Gemm g{};
  g.N = a->N; g.Cin = a->Cin; g.H = a->H; g.W = a->W; g.Cout = a->Cout; g.Ho = P.Ho; g.Wo = P.Wo;
  g.shift = P.shift; g.pad = a->pad;
  g.rows = P.rows; g.cols = P.cols; g.K = P.K;
  g.steps_per_split = P.steps_per_split;
  return g;
}

}  // namespace

extern "C" int gwtf_conv2d_plan(const GwtfConv2dArgs* args, int pass, int* splits, size_t* work_floats) {
  Plan P;
  if (int e = make_plan(args, pass, P)) return e;
  if (splits) *splits = P.S;
  if (work_floats) *work_floats = P.work_floats;
  return 0;
}

extern "C" int gwtf_conv2d_forward(const GwtfConv2dArgs* a) {
  Plan P;
  if (int e = make_plan(a, FWD, P)) return e;
  if (!a->x || !a->w || !a->y || ((size_t)a->w & 15)) return GWTF_E_BADARG;       // w rows are read 16 bytes at a time
  Gemm g = gemm_of(a, P);
  g.a = a->w; g.b = a->x; g.out = a->y;
  launch<FWD>(g, a->k, 1, (hipStream_t)a->stream);
  return (int)hipGetLastError();
}

extern "C" int gwtf_conv2d_backward_input(const GwtfConv2dArgs* a) {
  Plan P;
  if (int e = make_plan(a, DX, P)) return e;
  if (!a->dy || !a->w || !a->dx || !a->work || ((size_t)a->work & 15)) return GWTF_E_BADARG;
  hipStream_t stream = (hipStream_t)a->stream;
  const size_t total = P.work_floats;
  hipLaunchKernelGGL(transpose_w, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, a->w, a->work,
                     a->Cout, a->Cin, a->k * a->k);
  Gemm g = gemm_of(a, P);
  g.a = a->work; g.b = a->dy; g.out = a->dx;
  launch<DX>(g, a->k, 1, stream);
  return (int)hipGetLastError();
}

extern "C" int gwtf_conv2d_backward_weight(const GwtfConv2dArgs* a) {
  Plan P;
  if (int e = make_plan(a, DW, P)) return e;
  if (!a->dy || !a->x || !a->dw || (P.S > 1 && (!a->work || ((size_t)a->work & 15) || ((size_t)a->dw & 15)))) return GWTF_E_BADARG;
  hipStream_t stream = (hipStream_t)a->stream;
  Gemm g = gemm_of(a, P);
  g.a = a->dy; g.b = a->x; g.out = a->dw; g.part = a->work;
  launch<DW>(g, a->k, P.S, stream);
  if (P.S > 1) {
    const size_t total4 = (size_t)P.rows * P.cols / 4;
    hipLaunchKernelGGL(reduce_splits, dim3((unsigned)((total4 + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, a->work, P.S,
                       total4, a->dw);
  }
  return (int)hipGetLastError();
}
