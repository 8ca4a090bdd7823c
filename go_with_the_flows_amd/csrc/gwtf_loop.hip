// gwtf_loop.hip -- the state of the training loop on the device (GwtfLoopState / GwtfLoopArgs of include/gwtf.h).  The reference's
// train() / train_svr() (lib/networks/training.py:12-100, 188-303) keeps the iteration count, the schedule, the NaN test and the four
// AverageMeters on the host, and pays a synchronisation per .item().  Here they are three one-workgroup launches around the captured
// forward / backward, so that one graph replay is one whole iteration and the host only replays:
//   begin  : this iteration's rows of the epoch plan -> the static index buffers the batch kernels read
//   detect : the guard's verdict on the loss -> state->flag (data-parallel runs MAX-reduce it before the commit)
//   commit : poisoned / exhausted: skip the optimiser; otherwise the schedule row, the meters and the counters
// The validation pass (eval(), training.py:103-184) keeps a record of its own and replaces the commit by
//   eval_commit : poisoned / exhausted: nothing; a NaN or infinite loss poisons; otherwise the meters and the cursor
// Nothing here is hot: every kernel is one workgroup and a handful of words.  All stores are plain global stores.
#include <hip/hip_runtime.h>
#include "../../include/gwtf.h"

namespace {

constexpr int kPoisoned = 1, kExhausted = 2;

// NaN by its bits: the library is built with -fno-honor-nans, under which isnan(x) / x != x may be folded to false.  Any sign, quiet
// or signalling: exponent all ones and a non-zero mantissa.  or_inf: an infinity counts too (the reference's eval(), stop on inf).
__device__ __forceinline__ bool non_finite(float x, bool or_inf) {
  const unsigned mag = __float_as_uint(x) & 0x7fffffffu;
  return or_inf ? mag >= 0x7f800000u : mag > 0x7f800000u;
}

__device__ __forceinline__ bool runnable(const GwtfLoopState* s, const GwtfLoopArgs& a) {
  const int c = s->cursor;
  return c >= 0 && c < s->n_iters && c < a.table_rows && (long long)(c + 1) * a.B <= (long long)a.plan_len;
}

// AverageMeter.update(v.item(), B) of the four meters: val = v; sum += val * n; count += n  (float64, like the host's Python floats)
__device__ __forceinline__ void feed_meters(GwtfLoopState* s, float pnll, float gnll, float gent, int B) {
  const float lb = (pnll + gnll) - gent;                      // training.py:53 / :127, float32 in this order
  const float vals[4] = {lb, pnll, gnll, gent};
  const double n = (double)B;
  for (int k = 0; k < 4; ++k) {
    const double v = (double)vals[k];
    s->meters[3 * k] = v;
    s->meters[3 * k + 1] += v * n;
    s->meters[3 * k + 2] += n;
  }
}

__global__ __launch_bounds__(64) void loop_begin_kernel(const GwtfLoopArgs a) {
  GwtfLoopState* s = reinterpret_cast<GwtfLoopState*>(a.state);
  const bool in_epoch = runnable(s, a);
  const int status = s->status, cursor = s->cursor;
  __syncthreads();                                   // every thread has read the state before thread 0 writes it
  if (in_epoch && !(status & kPoisoned)) {
    for (int i = threadIdx.x; i < a.B; i += blockDim.x) {
      const int r = a.plan[(size_t)cursor * a.B + i];
      a.rows[i] = r;
      if (a.mesh_rows) a.mesh_rows[i] = r / a.views;
    }
    if (threadIdx.x == 0) s->status = status & ~kExhausted;
  } else if (threadIdx.x == 0) {
    s->skip = 1;
    s->status = in_epoch ? status : (status | kExhausted);
  }
}

__global__ __launch_bounds__(64) void loop_detect_kernel(const GwtfLoopArgs a) {
  if (threadIdx.x == 0) reinterpret_cast<GwtfLoopState*>(a.state)->flag = non_finite(*a.terms[0], a.stop_on_inf != 0) ? 1 : 0;
}

__global__ __launch_bounds__(64) void loop_commit_kernel(const GwtfLoopArgs a) {
  if (threadIdx.x != 0) return;
  GwtfLoopState* s = reinterpret_cast<GwtfLoopState*>(a.state);
  if (!runnable(s, a) || (s->status & kPoisoned)) {           // beyond the epoch, or after a poisoned step: a no-op replay
    s->skip = 1;
    return;
  }
  const float loss = *a.terms[0], pnll = *a.terms[1], gnll = *a.terms[2], gent = *a.terms[3];
  const bool bad = a.use_flag ? s->flag != 0 : non_finite(loss, a.stop_on_inf != 0);
  const int cursor = s->cursor;
  if (bad) {                                                  // "Stopping without updating the net" (training.py:48-50)
    s->status |= kPoisoned;
    s->poisoned_at = cursor;
    s->skip = 1;
    return;
  }
  const float* row = a.table + (size_t)cursor * 8;
  for (int i = 0; i < 8; ++i) s->hyper[i] = row[i];
  feed_meters(s, pnll, gnll, gent, a.B);
  s->adam_step += 1;
  s->cursor = cursor + 1;
  s->skip = 0;
}

// The validation pass: eval() stops on NaN and on an infinity alike (training.py:130-135), whatever stop_on_inf says; no schedule row,
// no optimiser: hyper, adam_step and skip stay as they are.
__global__ __launch_bounds__(64) void loop_eval_commit_kernel(const GwtfLoopArgs a) {
  if (threadIdx.x != 0) return;
  GwtfLoopState* s = reinterpret_cast<GwtfLoopState*>(a.state);
  if (!runnable(s, a) || (s->status & kPoisoned)) return;     // beyond the pass, or after a poisoned batch: nothing moves
  const float loss = *a.terms[0], pnll = *a.terms[1], gnll = *a.terms[2], gent = *a.terms[3];
  const int cursor = s->cursor;
  if (non_finite(loss, true)) {
    s->status |= kPoisoned;
    s->poisoned_at = cursor;
    return;
  }
  feed_meters(s, pnll, gnll, gent, a.B);
  s->cursor = cursor + 1;
}

bool args_ok(const GwtfLoopArgs* a) {
  return a && a->state && a->B >= 1 && a->views >= 1 && a->plan_len >= 0 && a->table_rows >= 0;
}

}  // namespace

extern "C" int gwtf_loop_begin(const GwtfLoopArgs* args) {
  if (!args_ok(args) || !args->plan || !args->rows) return GWTF_E_BADARG;
  hipLaunchKernelGGL(loop_begin_kernel, dim3(1), dim3(64), 0, (hipStream_t)args->stream, *args);
  return (int)hipGetLastError();
}

extern "C" int gwtf_loop_detect(const GwtfLoopArgs* args) {
  if (!args_ok(args) || !args->terms[0]) return GWTF_E_BADARG;
  hipLaunchKernelGGL(loop_detect_kernel, dim3(1), dim3(64), 0, (hipStream_t)args->stream, *args);
  return (int)hipGetLastError();
}

extern "C" int gwtf_loop_commit(const GwtfLoopArgs* args) {
  if (!args_ok(args) || !args->table) return GWTF_E_BADARG;
  for (int k = 0; k < 4; ++k)
    if (!args->terms[k]) return GWTF_E_BADARG;
  hipLaunchKernelGGL(loop_commit_kernel, dim3(1), dim3(64), 0, (hipStream_t)args->stream, *args);
  return (int)hipGetLastError();
}

extern "C" int gwtf_loop_eval_commit(const GwtfLoopArgs* args) {
  if (!args_ok(args)) return GWTF_E_BADARG;
  for (int k = 0; k < 4; ++k)
    if (!args->terms[k]) return GWTF_E_BADARG;
  hipLaunchKernelGGL(loop_eval_commit_kernel, dim3(1), dim3(64), 0, (hipStream_t)args->stream, *args);
  return (int)hipGetLastError();
}
