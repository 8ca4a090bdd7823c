// gwtf_images.hip -- image batches transformed on the device: the composed image transformations of the reference
// (lib/datasets/image_transformations.py:7-95) behind the image read of ShapeNetAllDataset.__getitem__ (lib/datasets/datasets.py:
// 201-214), for B raw uint8 renderings in one launch.  Stage order and arithmetic: include/gwtf.h (GwtfImageArgs).
//
// Grid (tiles of kRows output rows, B) x 256 threads; the threads of a workgroup share one source image.
//   staging  the two source rows each of the tile's output rows reads, after ToNumpy (byte / 255, channels 0 and 1 times channel 2),
//            as floats in LDS, with the column table beside them: every source byte is loaded and divided once per workgroup
//   compute  a thread takes four consecutive output x of one row and ALL output channels: both bilinear passes from LDS, grayscale,
//            normalisation, noise, each in the reference's order, uncontracted (-ffp-contract=off)
//   store    one 16-byte store per channel (rows of a width that is no multiple of four are only dword-aligned: the store's type
//            says so); the W_out % 4 last columns of a row take dword stores
// The source is 1 / 15 of the bytes written (137 x 137 x 3 uint8 -> 4 x 224 x 224 float32).  Measured at B = 128: 1.98 TB/s of
// written bytes, a third of the streaming rate -- the launch is bound by its divisions and LDS reads, not yet by its stores.
// No atomics, no scratch, no device-side allocation.  Philox noise advances the call word in a one-thread launch of its own, which
// follows the transforming launch on the stream: every workgroup has read the state by then.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/gwtf.h"
#include "gwtf_philox.h"

namespace {

using namespace gwtf_rng;

constexpr int kThreads = 256;
constexpr int kRows = 4;                       // output rows of a tile
constexpr int kSlots = 2 * kRows;              // staged source rows with resize (two per output row; kRows without)
constexpr int kMaxC = 5;                       // output channels: grayscale + RGBA
constexpr size_t kMaxLds = 65536;
constexpr uint32_t kNanBits = 0x7fc00000u;

typedef uint32_t quad_t __attribute__((ext_vector_type(4), aligned(4)));

// Source channels the outputs need: 0..2 always (grayscale, and channel 2 scales 0 and 1); alpha only when an output carries it.
__host__ __device__ inline int read_channels(int C, int grayscale, int c_out) { return (C == 4 && c_out - (grayscale ? 1 : 0) > 3) ? 4 : 3; }
__host__ __device__ inline int stage_channels(const GwtfImageArgs& a) { return a.C + (a.grayscale ? 1 : 0); }
__host__ __device__ inline int out_channels(const GwtfImageArgs& a) {
  const int cs = stage_channels(a);
  return (a.remove_alpha && cs > 4) ? 4 : cs;
}

__global__ __launch_bounds__(kThreads) void image_transform_kernel(GwtfImageArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, b = blockIdx.y, y0 = blockIdx.x * kRows;
  const int W = a.W, H = a.H, Wr = a.W_r, Hr = a.H_r;
  const int Wo = Wr + 2 * a.pad_x, Ho = Hr + 2 * a.pad_y;
  const int Cs = stage_channels(a), Co = out_channels(a), Cr = read_channels(a.C, a.grayscale, Co);
  const int img = a.rows ? a.rows[b] : b;
  const bool known = img >= 0 && img < a.n_images;            // an image outside the store: NaN bits, nothing is read
  const int slots = a.resize ? kSlots : kRows;                // without resize an output row reads one source row
  float* stage = lds;                                         // [slots][Cr][W]
  int* txs = reinterpret_cast<int*>(lds + (size_t)slots * Cr * W);      // [Wr], with resize
  float* txf = reinterpret_cast<float*>(txs + Wr);

  if (known) {
    const unsigned char* src = a.images + (size_t)img * a.C * H * W;
    const size_t plane = (size_t)H * W;
    for (int i = tid; i < slots * W; i += kThreads) {
      const int slot = i / W, x = i - slot * W;
      const int ry = a.resize ? slot >> 1 : slot, tap = a.resize ? slot & 1 : 0;
      const int yr = y0 + ry - a.pad_y;
      if (yr < 0 || yr >= Hr) continue;                       // a padding row, or past the image: never read below
      int sy = yr;
      if (a.resize) { sy = a.ys[yr] + tap; sy = sy > H - 1 ? H - 1 : (sy < 0 ? 0 : sy); }     // the second tap: min(s + 1, H - 1)
      const unsigned char* p = src + (size_t)sy * W + x;
      const float v2 = __fdiv_rn((float)p[2 * plane], 255.f);
      float* dst = stage + ((size_t)slot * Cr) * W + x;
      dst[0] = v2 * __fdiv_rn((float)p[0], 255.f);
      dst[W] = v2 * __fdiv_rn((float)p[plane], 255.f);
      dst[2 * W] = v2;
      if (Cr == 4) dst[3 * W] = __fdiv_rn((float)p[3 * plane], 255.f);
    }
    if (a.resize)
      for (int i = tid; i < Wr; i += kThreads) { txs[i] = a.xs[i]; txf[i] = a.xf[i]; }
  }
  __syncthreads();

  unsigned long long seed = 0, call = 0;
  const bool philox = a.add_noise && !a.noise;
  if (philox) { seed = a.state[0]; call = a.state[1]; }
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), c2 = (uint32_t)call, c3 = (uint32_t)(call >> 32);

  const int W4 = (Wo + 3) >> 2;
  for (int it = tid; it < kRows * W4; it += kThreads) {
    const int ry = it / W4, x0 = (it - ry * W4) * 4, yo = y0 + ry;
    if (yo >= Ho) continue;
    uint32_t o[kMaxC][4];
    if (!known) {
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) { o[c][0] = kNanBits; o[c][1] = kNanBits; o[c][2] = kNanBits; o[c][3] = kNanBits; }
    } else {
      const int yr = yo - a.pad_y;
      const bool row_in = yr >= 0 && yr < Hr;
      float wy1 = 0.f;
      if (a.resize && row_in) wy1 = a.yf[yr];
      const float wy0 = 1.f - wy1;
      const float* s0 = stage + (size_t)(a.resize ? 2 * ry : ry) * Cr * W;
      const float* s1 = s0 + (size_t)Cr * W;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int xo = x0 + k, xr = xo - a.pad_x;
        float v[4] = {0.f, 0.f, 0.f, 0.f};                    // the source channels at this pixel; zeros in the padding
        if (xo < Wo && row_in && xr >= 0 && xr < Wr) {
          if (a.resize) {
            const int xa = min(max(txs[xr], 0), W - 1), xb = min(xa + 1, W - 1);
            const float wx1 = txf[xr], wx0 = 1.f - wx1;
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (c < Cr) {
                const float r0 = s0[c * W + xa] * wx0 + s0[c * W + xb] * wx1;
                const float r1 = s1[c * W + xa] * wx0 + s1[c * W + xb] * wx1;
                v[c] = r0 * wy0 + r1 * wy1;
              }
          } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (c < Cr) v[c] = s0[c * W + xr];
          }
        }
        float t[kMaxC];                                       // the channels after AddGrayscale
        if (a.grayscale) {
          t[0] = (a.gray[0] * v[0] + a.gray[1] * v[1]) + a.gray[2] * v[2];
          t[1] = v[0]; t[2] = v[1]; t[3] = v[2]; t[4] = v[3];
        } else {
          t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3]; t[4] = 0.f;
        }
        if (a.normalize) {
#pragma unroll
          for (int c = 0; c < kMaxC; ++c)
            if (c < Co) t[c] = __fdiv_rn(t[c] - a.mean[c], a.stdev[c]);
        }
        if (a.add_noise && xo < Wo) {
          float n[kMaxC] = {0.f, 0.f, 0.f, 0.f, 0.f};
          if (a.noise) {
            const size_t e = (((size_t)b * Cs) * Ho + yo) * Wo + xo;
#pragma unroll
            for (int c = 0; c < kMaxC; ++c)
              if (c < Co) n[c] = a.noise[e + (size_t)c * Ho * Wo];
          } else {
            const uint32_t pix = (uint32_t)(yo * Wo + xo);
            const Philox4 d = philox4x32_10(pix, (uint32_t)b, c2, c3 | (4u << 28), k0, k1);
            box_muller(d.x, d.y, n[0], n[1]);
            box_muller(d.z, d.w, n[2], n[3]);
            if (Co > 4) {
              const Philox4 d5 = philox4x32_10(pix, (uint32_t)b, c2, c3 | (5u << 28), k0, k1);
              float unused;
              box_muller(d5.x, d5.y, n[4], unused);
            }
#pragma unroll
            for (int c = 0; c < kMaxC; ++c) n[c] = a.noise_scale * n[c];
          }
#pragma unroll
          for (int c = 0; c < kMaxC; ++c)
            if (c < Co) t[c] = fminf(fmaxf(t[c] + n[c], 0.f), 1.f);
        }
#pragma unroll
        for (int c = 0; c < kMaxC; ++c) o[c][k] = __float_as_uint(t[c]);
      }
    }
    const size_t row = (((size_t)b * Co) * Ho + yo) * Wo + x0;
    uint32_t* out = reinterpret_cast<uint32_t*>(a.out);
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < Co) {
        uint32_t* dst = out + row + (size_t)c * Ho * Wo;
        if (x0 + 3 < Wo) {
          quad_t q = {o[c][0], o[c][1], o[c][2], o[c][3]};
          *reinterpret_cast<quad_t*>(dst) = q;
        } else {                                              // the row's tail
          dst[0] = o[c][0];
          if (x0 + 1 < Wo) dst[1] = o[c][1];
          if (x0 + 2 < Wo) dst[2] = o[c][2];
        }
      }
  }
}

// Follows the transforming launch on the stream: the next call, or the next replay of a captured graph, draws fresh noise.
__global__ void image_tick_kernel(unsigned long long* state) { state[1] = state[1] + 1ull; }

}  // namespace

extern "C" int gwtf_transform_images(const GwtfImageArgs* pa) {
  if (!pa) return GWTF_E_BADARG;
  const GwtfImageArgs& a = *pa;
  if (!a.images || !a.out) return GWTF_E_BADARG;
  if (a.B < 1 || a.B > 65535 || a.n_images < 1 || (a.C != 3 && a.C != 4) || a.H < 1 || a.W < 1 || a.H_r < 1 || a.W_r < 1) return GWTF_E_BADARG;
  if (a.pad_y < 0 || a.pad_x < 0) return GWTF_E_BADARG;
  if (a.resize ? (!a.xs || !a.xf || !a.ys || !a.yf) : (a.H_r != a.H || a.W_r != a.W)) return GWTF_E_BADARG;
  const int co = out_channels(a);
  if (a.normalize)
    for (int c = 0; c < co; ++c)
      if (!(a.stdev[c] > 0.f)) return GWTF_E_BADARG;
  if (a.add_noise && !a.noise && (!a.state || !(a.noise_scale > 0.f))) return GWTF_E_BADARG;
  const long long ho = (long long)a.H_r + 2LL * a.pad_y, wo = (long long)a.W_r + 2LL * a.pad_x;
  if (ho * wo >= (1LL << 31) || (long long)a.H * a.W >= (1LL << 31)) return GWTF_E_BADARG;
  const int cr = read_channels(a.C, a.grayscale, co);
  const size_t lds = ((size_t)(a.resize ? kSlots : kRows) * cr * a.W + (a.resize ? 2 * (size_t)a.W_r : 0)) * sizeof(float);
  if (lds > kMaxLds) return GWTF_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)a.stream;
  const unsigned tiles = (unsigned)((ho + kRows - 1) / kRows);
  hipLaunchKernelGGL(image_transform_kernel, dim3(tiles, a.B), dim3(kThreads), lds, st, a);
  if (a.add_noise && !a.noise) hipLaunchKernelGGL(image_tick_kernel, dim3(1), dim3(1), 0, st, a.state);
  return (int)hipGetLastError();
}
