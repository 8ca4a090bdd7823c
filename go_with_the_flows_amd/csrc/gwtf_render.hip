// gwtf_render.hip -- B labelled point clouds drawn into the cells of a contact sheet: opaque, depth-tested discs coloured by mixture
// component, as a uint8 CHW image.  Record and rules: include/gwtf.h (GwtfRenderArgs) -- every rounding of the projection and every
// integer step behind it is fixed there, and tests/render_ref.py restates them bit for bit.
//
// Reference: the qualitative output of eval(), lib/visualization/utils.py:41-61 (rotate by (25, 135, 0) degrees, one matplotlib scatter
// per panel, coloured by COLORS_PLT[label - 1]), called from lib/networks/training.py:147-167.  The rotation arrives here inside the
// view matrix (render.py view_matrix / fit_views); the scatter is this kernel.
//
// render_kernel: one workgroup of kThreads per (tile of kTile x kTile pixels, image), one launch, no scratch, no global atomic.
//   clear     the tile's kTile^2 64-bit keys in LDS (32 KB) are set to all ones: "nothing drawn"
//   scan      every thread walks the image's N points with stride kThreads (12 B per point, coalesced along N): projection with
//             __fmul_rn / __fadd_rn; a non-finite coordinate is told on the BITS (opaque_bits below) and counted by the image's tile 0
//             alone; the float32 test against the cell grown by the radius comes before any conversion to int, so no conversion
//             overflows; then the integer footprint clipped to the tile and one LDS ds_min_u64 (atomicMin on unsigned long long) per
//             covered pixel with the key (ord(d) << 32) | n
//   resolve   every thread takes 4 consecutive pixels of a tile row: key -> (n, d) -> label -> palette -> depth cue, and writes rgb,
//             index and depth ONCE each: as one 4-byte / 16-byte store where the 4 pixels are inside the cell and the address is
//             aligned, pixel by pixel otherwise (the same values either way)
// Integer minimum only: the same inputs give the same bits on every call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/gwtf.h"

namespace {

constexpr int kTile = 64;              // 64 x 64 keys of 8 bytes: 32 KB of LDS, 5 workgroups per CU
constexpr int kThreads = 256;
constexpr int kMaxRadiusQ = 16 * 64;
constexpr int kMaxCell = 1 << 20;      // 16 * (W + radius + 2) stays far inside an int
constexpr unsigned long long kEmpty = ~0ull;

struct RenderParams {
  const float* clouds;
  const int* labels;
  const unsigned char* palette;
  const float* view;
  unsigned char* rgb;
  int* index;
  float* depth;
  int* skipped;
  int N, P, label_base, view_stride, H, W, radius_q, fog;
  int sheet_h, sheet_w, cols, cell0, cell_step;
  int tiles_x, tiles_per_image;
  float near, inv_range;
  unsigned char invalid_rgb[3], background_rgb[3];
};

// The library is built with -fno-honor-nans (see gwtf_nll.hip): a test on a float, and even the exponent test on its bits, is rewritten
// into a float comparison that takes NaN for a number.  The empty statement emits no instruction; it makes the BITS opaque, so that
// what follows is integer arithmetic on a value the optimiser knows nothing about.
__device__ inline unsigned opaque_bits(float v) {
  unsigned bits = __float_as_uint(v);
  asm volatile("" : "+v"(bits));
  return bits;
}
__device__ inline bool finite_bits(float v) { return (opaque_bits(v) & 0x7f800000u) != 0x7f800000u; }

__device__ inline unsigned ord_of(unsigned bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
__device__ inline unsigned bits_of(unsigned ord) { return (ord & 0x80000000u) ? (ord & 0x7fffffffu) : ~ord; }

__device__ inline float project_row(const float* m, float x, float y, float z) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z)), m[3]);
}

// The colour of the pixel whose key is `key` (not kEmpty), the winning point and its depth.
__device__ inline void shade(const RenderParams& a, int b, unsigned long long key, unsigned char (&c)[3], int& n, float& d) {
  n = (int)(unsigned)(key & 0xffffffffull);
  d = __uint_as_float(bits_of((unsigned)(key >> 32)));
  long long l = 0;
  if (a.labels) l = (long long)a.labels[(size_t)b * a.N + n] - (long long)a.label_base;
  const unsigned char* src = a.palette + 3 * (int)(l < 0 ? 0 : l % a.P);
  const float f = floorf(__fmul_rn(__fmul_rn(__fadd_rn(d, -a.near), a.inv_range), 256.0f));
  const bool number = (opaque_bits(f) & 0x7fffffffu) <= 0x7f800000u;      // not NaN (inf * 0)
  int q = 0;
  if (number && f > 0.0f) q = f >= 255.0f ? 255 : (int)f;
  const int w = 256 - ((a.fog * q) >> 8);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) c[ch] = (unsigned char)(((int)(l < 0 ? a.invalid_rgb[ch] : src[ch]) * w) >> 8);
}

__global__ __launch_bounds__(kThreads) void render_kernel(RenderParams a) {
  __shared__ unsigned long long keys[kTile * kTile];              // all of the workgroup's LDS: a 33rd KB would cost the 5th workgroup of a CU
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.tiles_per_image;
  const int tile = blockIdx.x - b * a.tiles_per_image;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int x0 = tx * kTile, y0 = ty * kTile;                       // the tile inside the cell
  const int x1 = min(a.W, x0 + kTile), y1 = min(a.H, y0 + kTile);   // (exclusive)
  for (int t = tid; t < kTile * kTile; t += kThreads) keys[t] = kEmpty;
  __syncthreads();

  const float* m = a.view + (size_t)b * a.view_stride;
  float mv[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) mv[i] = m[i];
  const float* px = a.clouds + (size_t)b * 3 * a.N;
  const int rq = a.radius_q;
  const int rq2 = rq * rq;
  const float grow = (float)(rq / 16 + 2);                          // whole pixels, more than the radius
  const float u_hi = (float)a.W + grow, v_hi = (float)a.H + grow;
  int n_bad = 0;
  for (int n = tid; n < a.N; n += kThreads) {
    const float x = px[n], y = px[a.N + n], z = px[2 * (size_t)a.N + n];
    const float u = project_row(mv, x, y, z), v = project_row(mv + 4, x, y, z), t2 = project_row(mv + 8, x, y, z);
    if (!(finite_bits(u) && finite_bits(v) && finite_bits(t2))) { ++n_bad; continue; }
    if (!(u > -grow && u < u_hi && v > -grow && v < v_hi)) continue;  // the disc cannot touch the cell; |16 u| < 2^25 from here on
    unsigned dbits = __float_as_uint(t2);
    if (dbits == 0x80000000u) dbits = 0u;                           // d = t_2 + 0.0f: -0 becomes +0, nothing else changes
    const int U = (int)floorf(__fmul_rn(u, 16.0f)), V = (int)floorf(__fmul_rn(v, 16.0f));
    const int j_lo = max(x0, (U - rq) >> 4), j_hi = min(x1 - 1, (U + rq) >> 4);      // a superset of the disc's columns / rows
    const int i_lo = max(y0, (V - rq) >> 4), i_hi = min(y1 - 1, (V + rq) >> 4);
    if (j_lo > j_hi || i_lo > i_hi) continue;
    const unsigned long long key = ((unsigned long long)ord_of(dbits) << 32) | (unsigned)n;
    const int jc = U >> 4, ic = V >> 4;
    for (int i = i_lo; i <= i_hi; ++i) {
      const int dy = 16 * i + 8 - V;
      for (int j = j_lo; j <= j_hi; ++j) {
        const int dx = 16 * j + 8 - U;
        if ((i == ic && j == jc) || dx * dx + dy * dy <= rq2) atomicMin(&keys[(i - y0) * kTile + (j - x0)], key);
      }
    }
  }
  __syncthreads();

  const long long cell = (long long)a.cell0 + (long long)b * a.cell_step;
  const size_t oy = (size_t)(cell / a.cols) * a.H, ox = (size_t)(cell % a.cols) * a.W;
  const size_t plane = (size_t)a.sheet_h * a.sheet_w;
  for (int t = tid; t < kTile * kTile / 4; t += kThreads) {
    const int i = y0 + t / (kTile / 4), j = x0 + 4 * (t % (kTile / 4));
    if (i >= y1 || j >= x1) continue;
    const int count = min(4, x1 - j);
    unsigned char c[4][3];
    int idx[4];
    float dep[4];
    for (int e = 0; e < count; ++e) {
      const unsigned long long key = keys[(i - y0) * kTile + (j - x0) + e];
      if (key == kEmpty) {
        c[e][0] = a.background_rgb[0]; c[e][1] = a.background_rgb[1]; c[e][2] = a.background_rgb[2];
        idx[e] = -1;
        dep[e] = INFINITY;
      } else {
        shade(a, b, key, c[e], idx[e], dep[e]);
      }
    }
    const size_t at_sheet = (oy + i) * a.sheet_w + ox + j;
    const size_t at_cell = ((size_t)b * a.H + i) * a.W + j;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      unsigned char* dst = a.rgb + ch * plane + at_sheet;
      if (count == 4 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
        *reinterpret_cast<unsigned*>(dst) = (unsigned)c[0][ch] | ((unsigned)c[1][ch] << 8) | ((unsigned)c[2][ch] << 16) | ((unsigned)c[3][ch] << 24);
      } else {
        for (int e = 0; e < count; ++e) dst[e] = c[e][ch];
      }
    }
    if (a.index) {
      int* dst = a.index + at_cell;
      if (count == 4 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) *reinterpret_cast<int4*>(dst) = make_int4(idx[0], idx[1], idx[2], idx[3]);
      else for (int e = 0; e < count; ++e) dst[e] = idx[e];
    }
    if (a.depth) {
      float* dst = a.depth + at_cell;
      if (count == 4 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) *reinterpret_cast<float4*>(dst) = make_float4(dep[0], dep[1], dep[2], dep[3]);
      else for (int e = 0; e < count; ++e) dst[e] = dep[e];
    }
  }
  if (tile == 0 && a.skipped) {                                    // uniform over the workgroup; the keys are done with
    int* count = reinterpret_cast<int*>(keys);
    __syncthreads();
    if (tid == 0) *count = 0;
    __syncthreads();
    if (n_bad) atomicAdd(count, n_bad);
    __syncthreads();
    if (tid == 0) a.skipped[b] = *count;
  }
}

}  // namespace

extern "C" int gwtf_render_splats(const GwtfRenderArgs* pa) {
  if (!pa) return GWTF_E_BADARG;
  const GwtfRenderArgs& g = *pa;
  if (!g.clouds || !g.palette || !g.view || !g.rgb) return GWTF_E_BADARG;
  if (g.B < 1 || g.N < 1 || g.H < 1 || g.W < 1) return GWTF_E_BADARG;
  if (g.P < 1 || g.P > 256) return GWTF_E_BADARG;
  if (g.view_stride != 0 && g.view_stride != 12) return GWTF_E_BADARG;
  if (g.radius_q < 0 || g.radius_q > kMaxRadiusQ) return GWTF_E_BADARG;
  if (g.fog < 0 || g.fog > 256) return GWTF_E_BADARG;
  if (g.cols < 1 || g.cell0 < 0 || g.cell_step < 0 || g.sheet_h < 1 || g.sheet_w < 1) return GWTF_E_BADARG;
  if (g.B > 1 && g.cell_step < 1) return GWTF_E_BADARG;           // two images in one cell: two workgroups would write the same pixels
  // the cells are visited in rising order: the last one is the farthest down, and every cell of a row of `cols` lies inside the width
  const long long last = (long long)g.cell0 + (long long)(g.B - 1) * g.cell_step;
  if ((long long)g.cols * g.W > g.sheet_w || (last / g.cols + 1) * g.H > g.sheet_h) return GWTF_E_BADARG;
  if (g.H > kMaxCell || g.W > kMaxCell) return GWTF_E_UNSUPPORTED;
  const long long tiles_x = (g.W + kTile - 1) / kTile, tiles_y = (g.H + kTile - 1) / kTile;
  if (tiles_x * tiles_y * g.B > 0x7fffffffll) return GWTF_E_UNSUPPORTED;
  RenderParams a;
  a.clouds = g.clouds; a.labels = g.labels; a.palette = g.palette; a.view = g.view;
  a.rgb = g.rgb; a.index = g.index; a.depth = g.depth; a.skipped = g.skipped;
  a.N = g.N; a.P = g.P; a.label_base = g.label_base; a.view_stride = g.view_stride; a.H = g.H; a.W = g.W;
  a.radius_q = g.radius_q; a.fog = g.fog;
  a.sheet_h = g.sheet_h; a.sheet_w = g.sheet_w; a.cols = g.cols; a.cell0 = g.cell0; a.cell_step = g.cell_step;
  a.tiles_x = (int)tiles_x; a.tiles_per_image = (int)(tiles_x * tiles_y);
  a.near = g.near; a.inv_range = g.inv_range;
  for (int ch = 0; ch < 3; ++ch) { a.invalid_rgb[ch] = g.invalid_rgb[ch]; a.background_rgb[ch] = g.background_rgb[ch]; }
  hipLaunchKernelGGL(render_kernel, dim3((unsigned)(tiles_x * tiles_y * g.B)), dim3(kThreads), 0, (hipStream_t)g.stream, a);
  return (int)hipGetLastError();
}
