/* gwtf.h -- C ABI of libgwtf_hip.so: the MI355X (gfx950) implementation of the discrete
 * point-flow decoder hot path of janisgp/go_with_the_flows.
 *
 * The reference has no native code on this path; each entry point below replaces a span of
 * Python/torch code, cited as reference file:line.  Conventions for every function:
 *   - returns 0 on success, otherwise a hipError_t value (or GWTF_E_* below); never throws;
 *   - all pointers are DEVICE pointers to contiguous fp32 (int32 where stated) buffers owned by
 *     the caller; the library allocates nothing and keeps NO mutable global state (no tuning switches, no environment
 *     variables: what a call does is a function of its arguments -- see GWTF_TUNE_* for the per-call tuning word; the one thing
 *     remembered between calls changes no result: gwtf_voxel_occupancy notes per device that its kernel's LDS limit is raised);
 *   - work is enqueued on `stream` (a hipStream_t passed as void*) and returns immediately:
 *     no internal streams, events or synchronisation (same convention as the reference's own
 *     native ops, lib/metrics/pytorch_structural_losses/src/structural_loss.cpp:35);
 *   - callable from one host thread per process (one process per GPU).
 * Buffer layouts are specified in go_with_the_flows_amd/csrc/gwtf_layout.h.
 */
#ifndef GWTF_H
#define GWTF_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GWTF_ABI_VERSION 12
#define GWTF_E_BADARG 10001   /* shape / mode / width outside what the kernels support */
#define GWTF_E_UNSUPPORTED 10002   /* a layer-width list no kernel instantiation was built for */
#define GWTF_E_FEW_VALUES 10003   /* batch statistics over fewer than 2 values per channel */
#define GWTF_MODE_DIRECT 0    /* sampling direction  base -> data (reference models.py:202) */
#define GWTF_MODE_INVERSE 1   /* density direction   data -> base (reference models.py:197) */

/* Per-call tuning word (`tune` arguments; 0 = the library's own choices).  Tests and the tile-calibration tools pass it; results
 * never depend on it beyond fp32 rounding of a different summation order (tests/test_gpu_parity.py pins that). */
#define GWTF_TUNE_DEFAULT 0
#define GWTF_TUNE_POINTS_PER_WAVE(n) ((n) & 0xffff)   /* force 16, 32 or 64 points per wavefront in the forward-sized kernels */
#define GWTF_TUNE_GENERIC_BODY (1 << 30)              /* the run-time-width coupling body instead of the software-pipelined one */
#define GWTF_TUNE_SMALL_LIGHT_TILE (1 << 29)          /* train backward, light pass: 128-point tiles even on large grids */
#define GWTF_TUNE_SINGLE_TILE (1 << 28)               /* no mixed launch (large tiles + a small-tile tail): one tile size per launch */

int gwtf_abi_version(void);
/* Human-readable text for a non-zero return value (static storage). */
const char* gwtf_error_string(int code);
/* Diagnostic: a one-thread kernel on `stream` writes wall_clock64() (100 MHz) to *slot -- a time stamp inside a captured hipGraph. */
int gwtf_diag_stamp(unsigned long long* slot, void* stream);

/* Sizes (in floats) of the buffers the caller must provide. FP = f rounded up to 16. */
int    gwtf_padded_width(int f);
size_t gwtf_raw_coupling_floats(int f, int G);        /* one coupling record of the raw arena   */
size_t gwtf_packed_w_coupling_floats(int f);          /* one coupling of packed stack weights   */
size_t gwtf_packed_film_coupling_floats(int f, int G);/* one coupling of packed FiLM weights    */
size_t gwtf_film_out_floats(int f);                   /* FiLM output per (shape, coupling)      */

/* Weight packer.  Folds eval-mode BatchNorm into the adjacent SharedDot / Linear weights, pads
 * f to FP and lays the weights out in MFMA-fragment / coalesced order.
 * Replaces the per-call parameter reads of nn.BatchNorm1d + SharedDot in
 * lib/networks/flows.py:25-50,60-85 (module construction) as consumed by :95-107.
 *   raw          [K*Cper][gwtf_raw_coupling_floats]   parameters + running statistics, direct order
 *   pattern0     warp pattern index of coupling 0 (the raw record stores sd0.weight as the module does, [f][k] with
 *                k = 1 or 2 kept coordinates: the packer needs each coupling's k)
 *   packed_w     [K*Cper][gwtf_packed_w_coupling_floats]
 *   packed_film  [K*Cper][gwtf_packed_film_coupling_floats]
 *   training     0: fold running statistics (model.eval()); 1: the train pipeline's packing (model.train()) -- packed_w only, in
 *                train form (sd1 un-scaled, sd0 records left to the pipeline's fold0); packed_film may be NULL: the pipeline's
 *                FiLM heads read the raw arena in place (gwtf_film_heads_forward). */
/* K concatenated stacks of Cper couplings each (the components of a mixture; K = 1: one stack, C = Cper): raw [K][Cper][...],
 * every stack starts again at warp pattern `pattern0`. */
int gwtf_pack_weights_k(const float* raw, float* packed_w, float* packed_film,
                        int K, int Cper, int f, int G, int pattern0, int training, void* stream);

/* Per-shape FiLM conditioning for all C couplings, eval-mode BatchNorm (the train-mode heads: gwtf_film_heads_forward): the four
 * Linear->BN->Swish->Linear heads of each coupling applied to the latent g, then a = eps + exp(w(g)), b' = a*c1 + b(g).
 * Replaces T_{mu,logvar}_0_cond_{w,b}(g) and torch.add(eps, torch.exp(.)) in
 * lib/networks/flows.py:100-101,105-106 (modules built at :33-45,68-80).
 *   g        [B][G]
 *   film_out [B][C][gwtf_film_out_floats]
 *   eps      the coupling's `eps` buffer (reference flows.py:21, 1e-6) */
int gwtf_film_forward(const float* g, const float* packed_film, float* film_out, int B, int G, int C, int f, float eps,
                      void* stream);
/* gwtf_film_forward over the C = K*Cper concatenated couplings of K components, every component conditioned on latent rows of its
 * own (added without a version change): coupling c reads its B rows at g + (c / Cper) * g_stride_k, g_stride_k >= 0 floats from
 * one component's [B][G] table to the next.  Stride 0 is gwtf_film_forward(C = K*Cper).  Same kernel body, instantiations, grid
 * and arithmetic per (coupling, row): component k's part of film_out equals, bit for bit, what gwtf_film_forward writes there when
 * it is run on table k.  GWTF_E_BADARG as for gwtf_film_forward, and for K < 1, Cper < 1 or a negative stride. */
int gwtf_film_forward_k(const float* g, const float* packed_film, float* film_out, int B, int G, int K, int Cper, int f, float eps,
                        long long g_stride_k, void* stream);

/* Fused coupling stack: all C elementary couplings applied to every point, with the log-det
 * accumulation.  Replaces LocalCondRNVPDecoder.forward (lib/networks/decoders.py:61-79) ->
 * CondRealNVPFlow3DTriple.forward (flows.py:150-160) -> CondRealNVPFlow3D.forward (flows.py:95-117)
 * and the `sum(logvars)` of lib/networks/losses.py:14,115 -- for K flow components in ONE launch (the loop over
 * `self.pc_decoder[i]` in Flow_Mixture_Model.decode, lib/networks/flow_mixture.py:163-166; K = 1: one decoder).
 * Everything a stack launch takes is one record, read by both entry points below. */
#define GWTF_WORKLIST_CAP 2048
#define GWTF_WORKLIST_INTS (2 + 2 * GWTF_WORKLIST_CAP)
typedef struct GwtfStackArgs {
  const float* p;            /* [B][3][N]  input coordinates (data for INVERSE, base samples for DIRECT); component k reads p + k*p_stride_k */
  const float* weights;      /* [K][C][...]  the K components' records, concatenated: packed_w (gwtf_pack_weights_k) for gwtf_stack_forward,
                              * packed_x (gwtf_pack_weights_exact of the same raw arena, [K*C][gwtf_packed_x_coupling_floats]) for
                              * gwtf_stack_forward_exact */
  const float* film;         /* [B][K*C][...]  gwtf_film_forward run once on the concatenated FiLM weights with C' = K*C; both entry
                              * points read the SAME records */
  float* out;                /* [B][3][N]  coordinates after the whole stack (ps[0] for INVERSE, ps[-1] for DIRECT); component k writes
                              * out + k*out_stride_k */
  float* logdet;             /* [B][3][N]  sum over the C couplings of logvar (per coordinate; the reference's definition of the log-det,
                              * NOT including the base logvar0); component k writes logdet + k*out_stride_k */
  float* ps;                 /* optional (all three NULL, or all three non-NULL): the per-coupling lists the reference returns, slot j =
                              * direct-order coupling j; [K][C][B][3][N] when out_stride_k != 0 else [C][B][3][N] */
  float* mus;
  float* logvars;
  const int* segments;       /* HOST array of 2K ints, or NULL: component k takes the points [segments[2k], segments[2k+1]) of every shape
                              * (NULL: every component takes all N points);  K <= 64 */
  int* worklist;             /* NULL, or GWTF_WORKLIST_INTS ints of device memory, zero before the FIRST use, owned by one stream at a time
                              * (the pair below keeps it zero between uses): the flagged-tile list between a split launch and its re-run */
  size_t p_stride_k;         /* floats; 0: all components read the same clouds */
  size_t out_stride_k;       /* floats; B*3*N for the density path -> [K][B][3][N], the layout gwtf_mixture_nll reads; 0 for the sampling
                              * path where the segments partition N */
  int K, B, N, C, f;
  int pattern0;              /* warp pattern index of coupling 0 (0 for a decoder / pattern-0 Triple; see gwtf_layout.h) */
  int mode;                  /* GWTF_MODE_DIRECT / GWTF_MODE_INVERSE */
  int tune;                  /* GWTF_TUNE_* word; gwtf_stack_forward_exact reads GWTF_TUNE_POINTS_PER_WAVE(16 | 32) only */
  float eps;                 /* the coupling's `eps` buffer (reference flows.py:21, 1e-6) */
  void* stream;
} GwtfStackArgs;
/* The split-f16 body (csrc/gwtf_stack.hip).  A point whose coordinate left the f16-safe range (|x| > 3e4) is flagged with NaN; with
 * worklist != NULL a wave that flags a point also appends {component * B + shape, first point} to worklist[2 + 2 i], i = atomic
 * increment of worklist[0]. */
int gwtf_stack_forward(const GwtfStackArgs* args);
/* The same stack with the f x f contraction on the EXACT-fp32 matrix instruction (v_mfma_f32_16x16x4_f32, unsplit operands):
 * the arithmetic of the reference's torch.matmul in SharedDot (lib/networks/layers.py:40-45 as called by flows.py:95-117), no
 * operand range limit (csrc/gwtf_stack_exact.hip).
 *   rerun = 0: every tile is computed (on-device A/B of the split-f16 contraction; the fp32-MFMA comparison point).
 *   rerun = 1: RE-RUN after gwtf_stack_forward with the same record (weights = packed_x) -- tiles whose out / logdet are all finite are
 *              left alone, the others are recomputed (all list slots included): points the split kernel flagged with NaN come back
 *              with the reference's finite fp32 values; genuinely non-finite inputs / parameters stay NaN.
 *              worklist != NULL: the launch walks the list the split launch left (all tiles when worklist[0] > GWTF_WORKLIST_CAP) and
 *              its last workgroup clears worklist[0..1] -- the re-run behind a clean pass costs the dispatch of 64 idle workgroups
 *              (2.8 us per forward pass of the airplane config).  worklist == NULL: a scan of every tile's flags (7 us). */
size_t gwtf_packed_x_coupling_floats(int f);
int gwtf_pack_weights_exact(const float* raw, const float* packed_film /*eval packing of the same arena: its range exponents*/,
                            float* packed_x, int K, int Cper, int f, int G, int pattern0, void* stream);
int gwtf_stack_forward_exact(const GwtfStackArgs* args, int rerun);
/* Latent-space loss terms of the training step and their combination with the point NLL (reference lib/networks/losses.py:24-33
 * GaussianFlowNLL, :36-41 GaussianEntropy, :159-170 Flow_Mixture_Loss.forward), two launches forward and one backward
 * (csrc/gwtf_latent.hip).  The base Gaussian of the prior flow is shared by the batch (rows = 0: mu0, lv0 and their gradients [G], the
 * generative / autoencoding models' learned parameters) or there is one per row (rows = 1: [B][G], single-view reconstruction:
 * g0_prior(img_encoder(images)); its backward is elementwise throughout).  The forward is a two-stage block-ordered reduction (no
 * float atomics: same inputs, same bits). */
typedef struct GwtfLatentLossArgs {
  const float* nll;                  /* [B] per-shape point NLL (gwtf_mixture_nll) */
  const float* z;                    /* [B][G] = g_prior_samples[0] */
  const float* mu0;                  /* [G] (rows = 0) or [B][G] (rows = 1) */
  const float* lv0;                  /* as mu0 */
  const float* flow_lv;              /* [n2][B][G] = the prior flow's stacked logvars (g_prior_logvars[1:]) */
  const float* post_lv;              /* [B][G] = g_posterior_logvars */
  float* workspace;                  /* forward: gwtf_latent_loss_workspace_floats(B, G) floats (block partials; 8-byte aligned) */
  float* out4;                       /* forward: {loss = pw pnll + gw gnll - ew gent, pnll, gnll, gent} */
  const float* g_out4;               /* backward: upstream of the four outputs */
  float* g_nll;                      /* backward outputs, each of the shape of its forward operand */
  float* g_z;
  float* g_mu0;
  float* g_lv0;
  float* g_flow_lv;
  float* g_post_lv;
  int B, G, n2;
  int rows;                          /* 0: one base Gaussian for the batch, 1: one per row */
  float pw, gw, ew;
  void* stream;
} GwtfLatentLossArgs;
/* Both validate on the host before any launch.  GWTF_E_BADARG: a NULL record, a NULL pointer among those the direction uses
 * (forward: nll .. out4; backward: g_out4, z, mu0, lv0 and the six outputs), B, G or n2 < 1, rows outside 0..1, B * G beyond the
 * kernels' int element index.  gwtf_latent_loss_workspace_floats returns 0 for sizes the launches refuse. */
int gwtf_latent_loss_workspace_floats(int B, int G);
int gwtf_latent_loss_forward(const GwtfLatentLossArgs* args);
int gwtf_latent_loss_backward(const GwtfLatentLossArgs* args);
/* Tile plan of a forward launch (what stack_dispatch decides; diagnostic + tests): out[0] = points per wavefront of the main
 * launch, out[1] = its workgroups, out[2] = points per wavefront of the tail launch (0: none), out[3] = its workgroups.
 * The choice minimises resident rounds x the cost of a round of that tile (calibrated, csrc/gwtf_stack.hip tile_cost). */
int gwtf_stack_plan(const int* segments, int K, int B, int N, int f, int tune, int* out4);
/* The passes of the coupling backward, by the kernels' own values. */
#define GWTF_BWD_PASS_DIRECT 0   /* the coupling's whole backward (gwtf_coupling_backward_lists) */
#define GWTF_BWD_PASS_LIGHT 2    /* train pipeline, phase BWD_A: FiLM-record and bias sums only */
#define GWTF_BWD_PASS_MERGED 3   /* train pipeline, phase BWD_B: g_in, dW1 partials, sd0 sums */
/* Launch plan of one backward pass (GWTF_BWD_PASS_*) of a coupling (what csrc/gwtf_bwd.hip bwd_plan decides; diagnostic + tests,
 * launches nothing): out8 = {MB, NB, MG, K2, FULL, tpw, grid_x, grid_y} -- the kernel variant (MB = padded width / 16, NB = 64-point
 * blocks per workgroup tile, MG / K2 / FULL as in the kernel's template), the tiles of one shape a workgroup walks, and the grid.
 * The direct and merged passes' grid_x is gwtf_dw1_partials(B, N).  pattern = (pattern0 + c) % 6.
 * GWTF_E_BADARG: NULL out8, unknown pass, f outside 1..96, B, N or K <= 0, K > 64, pattern outside 0..5, a grid beyond an int
 * (gwtf_dw1_partials and gwtf_dw1_workspace_floats return 0 for such a shape, gwtf_dw1_reduce refuses it). */
int gwtf_bwd_plan(int pass, int f, int B, int N, int K, int pattern, int tune, int* out8);

/* ---- backward (both directions, BatchNorm as a fixed affine) --------------------------------------------------
 * Autograd of CondRealNVPFlow3D.forward (reference flows.py:95-117 as differentiated by loss.backward(),
 * training.py:54), one coupling per call, in the FOLDED parameters the forward kernel consumes:
 *   W1p [C][2][f][f] = sd1.weight with sd1_bn's scale folded, W0f [C][2][f][2] / c0f [C][2][f] = sd0 with sd0_bn folded,
 *   FiLM record [B][C][6FP+4] = {c, u0, u1} x 2 branches + biases (gwtf_layout.h).
 * gwtf_pack_folded builds the forward record (packed_w) and the backward record (packed_b) from them.
 * gwtf_coupling_backward_lists: x_in = the coupling's input saved by the forward, g_out/g_ld = dL/d(out), dL/d(logdet);
 *   g_ps_c = dL/d ps[c], g_lvs_c = dL/d logvars[c], each [B][3][N] or NULL: gradients that enter through the coupling's own list
 *   slots (the reference's forward returns differentiable per-coupling lists, decoders.py:61-79);
 *   -> g_in [B][3][N]; dw1_ws: per-workgroup partials of dW1p = sum_p dL/dacc(p) relu(sd0)(p)^T, gwtf_dw1_workspace_floats(f,B,N)
 *   floats, summed by gwtf_dw1_reduce; g_film [B][C][2][3][FP] += {dc, du0, du1}; g_sd0 [64][2][3][FP] += {dW0f[:,0], dW0f[:,1], dc0f};
 *   g_bias [64][4] += {db_lv0, db_lv1, db_mu0, db_mu1}   (64 = GWTF_STAT_REPLICAS copies, sum them; all pre-zeroed). */
size_t gwtf_packed_b_coupling_floats(int f);
int gwtf_pack_folded(const float* W1p, const float* W0f, const float* c0f, float* packed_w, float* packed_b,
                     int C, int f, void* stream);
int gwtf_coupling_backward_lists(const float* x_in, const float* g_out, const float* g_ld, const float* g_ps_c,
                                 const float* g_lvs_c, const float* packed_w_c, const float* packed_b_c, const float* film,
                                 float* g_in, float* dw1_ws, float* g_film, float* g_sd0, float* g_bias, int c, int B, int N,
                                 int C, int f, int pattern0, float eps, int mode, void* stream);

/* Backward records of the train pipeline: W1T sections from the un-scaled sd1 weights (sd0 sections: the pipeline's fold0). */
int gwtf_pack_w1t(const float* raw, float* packed_b, int C, int f, int G, void* stream);
/* ---- FiLM conditioning heads under autograd (csrc/gwtf_film_train.hip) -----------------------------------------------------
 * Replaces T_*_0_cond_w / T_*_0_cond_b of every coupling (reference lib/networks/flows.py:33-45, 68-80, evaluated at :100-101,
 * 105-106): Linear(G -> f) -> BatchNorm1d over the latent rows -> Swish -> Linear(f -> f); a = eps + exp(scale head), b = shift head.
 * H = 4 KC heads (KC couplings in all: K stacks x C), one workgroup per head, parameters read in place from the raw arena
 * [KC][raw coupling record]; training = 1: batch statistics over the B_all rows (any number <= 65536, walked 128 at a time; all ranks' rows when data parallel),
 * 0: the arena's running statistics.
 *   g [B_all][G]; poison [KC][2] (0 or NaN, added to the scale a: diverged weights reach every output) or NULL
 *   hraw, hn [B_all][H][f] (pre-BatchNorm / post-Swish activations, kept for the backward); stats [3][H][f] = mean, biased var, rstd
 *   film_raw [B][KC][2][2][FP] (rows row0 .. row0 + B of g): {a, b} per branch, the train pipeline's GwtfTrainCtx.film_raw; only the
 *   f valid columns are written (zero the buffer first).
 * Backward: g_film_raw = dL/d film_raw -> g_raw: every FiLM parameter's gradient written (=) at its arena offset (other slots
 * untouched); dhraw [B_all][H][f] scratch; dg_part [gwtf_film_heads_slices(KC, G)][B_all][G]: partial dL/dg, summed by the caller. */
int gwtf_film_heads_slices(int KC, int G);
int gwtf_film_heads_forward(const float* raw, const float* g, const float* poison, float* hraw, float* hn, float* stats,
                            float* film_raw, int KC, int f, int G, int B_all, int row0, int B, float eps, int training,
                            void* stream);
int gwtf_film_heads_backward(const float* raw, const float* g, const float* hraw, const float* hn, const float* stats,
                             const float* film_raw, const float* g_film_raw, float* g_raw, float* dhraw, float* dg_part,
                             int KC, int f, int G, int B_all, int row0, int B, float eps, int training, void* stream);

/* ---- K-batched, phase-split train pipeline (round 2) -------------------------------------------------------------------
 * All K components of a flow mixture (reference flow_mixture.py:163-166: a Python loop over self.pc_decoder) run through
 * every kernel of the train-mode chain together, and the chain is cut exactly where a data-parallel run sums BatchNorm
 * statistics over the ranks (SyncBatchNorm, reference train_ae.py:152): two collectives per depth level and direction.
 * A rank that owns the whole batch calls gwtf_mtrain_forward / gwtf_mtrain_backward; a sharded run calls
 * gwtf_mtrain_phase level by level and all-reduces (sum) the named slab between the phases:
 *     FWD_INIT -> moments[0] (64*16 floats) | per step: FWD_A -> ystats[c] (K*64*2*FP*2) | FWD_B -> moments[step+1] (K*64*16)
 *     per backward step: BWD_A (light pass, fold1) -> g_stats[c] (K*2*2*FP) | BWD_B (merged pass, fold0) -> g_mom[c] (K*48 DOUBLES) | BWD_C
 * with c = step (DIRECT) or C-1-step (INVERSE) going forward, and c = step (INVERSE) or C-1-step (DIRECT) going backward.
 * Every buffer is caller-owned; "zero" = must be zero on entry.  FP = gwtf_padded_width(f), R = 64 statistic replicas. */
#define GWTF_PHASE_FWD_INIT 0
#define GWTF_PHASE_FWD_A 1
#define GWTF_PHASE_FWD_B 2
#define GWTF_PHASE_BWD_A 3
#define GWTF_PHASE_BWD_B 4
#define GWTF_PHASE_BWD_C 5
typedef struct GwtfTrainCtx {
  int K, B, N, C, f, G, pattern0, mode;
  int tune;                  /* GWTF_TUNE_* word for every launch of the pipeline (0 = default) */
  float eps;
  double n_total;            /* points the statistics cover: B*N summed over all ranks */
  const float* p;            /* [B][3][N]            input clouds, shared by the K components */
  const float* raw;          /* [K][C][raw record]   parameters + buffers (gwtf_layout.h GwtfRaw) */
  float* packed_w;           /* [K][C][packed_w]     from gwtf_pack_weights_k(training=1); fold0 fills the sd0 records */
  float* packed_b;           /* [K][C][packed_b]     from gwtf_pack_w1t; fold0 fills the sd0 sections; NULL: no backward */
  const float* film_raw;     /* [B][K*C][2][2][FP]   raw FiLM {a, b} per shape (batch-statistic FiLM BatchNorm applied) */
  float* film_rec;           /* [B][K*C][gwtf_film_out_floats]  written by fold1, read by apply and the backward */
  float* moments;            /* [C+1][K][R*16]       zero: the R = 64 copies the passes' statistic atomics are spread over */
  float* ystats;             /* [C][K][R*2*FP*2]     zero */
  float* mom_c;              /* [C+1][K][16] or NULL COMPACT moments (9 used) of every level's input: data-parallel runs -- each forward
                              *                       phase then ends with one launch that sums the copies into it, the caller all-reduces
                              *                       it, and every consumer (folds, backward) reads it instead of the copies.
                              *                       Level 0 (the shared input clouds): record [0][0] only */
  float* ys_c;               /* [C][K][2*FP*2] or NULL (both or neither): COMPACT {sum y, sum y^2} per branch and feature, likewise */
  float* bn_batch;           /* [K][C][2][4][2][f]   batch {mean, unbiased var} of sd0_bn (kind 0) and sd1_bn (kind 1) */
  float* xbuf;               /* [2][K][B][3][N]      ping-pong coordinates; result in half gwtf_mtrain_final_forward_half(C) */
  float* logdet;             /* [K][B][3][N] */
  float* ps; float* mus; float* logvars;   /* [K][C][B][3][N] each, or all NULL, or ps alone (required for the backward: ps) */
  /* backward only */
  const float* g_out;        /* [K][B][3][N]  dL/d out */
  const float* g_ld;         /* [K][B][3][N]  dL/d logdet */
  const float* g_ps;         /* [K][C][B][3][N] or NULL: dL/d ps[c], gradients entering through the per-coupling list slots */
  const float* g_lvs;        /* [K][C][B][3][N] or NULL: dL/d logvars[c] */
  float* g_bufs;             /* [2][K][B][3][N]  dL/dp per component ends in half gwtf_mtrain_final_backward_half(C, mode) */
  float* g_xa; float* g_xb;  /* unused (the gradient combine runs inside the next level's passes); kept for layout stability, may be NULL */
  float* dw1_ws;             /* [K][gwtf_mtrain_dw1_floats(f, B, N)] scratch */
  float* g_film;             /* [B][K*C][2][3][FP]   zero */
  float* g_sd0;              /* [C][K][R*2*3*FP]     zero */
  float* g_bias;             /* [C][K][R*4]          zero */
  float* g_stats;            /* [C][K][2*2*FP] */
  float* g_mom;              /* [C][K][16]  zero: the nine moment gradients gM of every level (summed by atomics; all-reduced when data parallel) */
  float* g_film_raw;         /* [B][K*C][2][2][FP]   dL/d film_raw */
  float* g_raw;              /* [K][C][raw record]   zero; receives dW0, dgamma0, dbeta0, dW1, dW2, db2 */
  void* stream;
} GwtfTrainCtx;
/* running = (1 - m) running + m batch for n BatchNorm modules in one launch (torch.nn.BatchNorm1d's train-mode buffer update):
 * table [n][3] = device pointers {running_mean [f], running_var [f], num_batches_tracked (int64, += 1) or 0}; src [n][2][f] =
 * batch {mean, unbiased var} (bn_batch of the train pipeline); momentum [n]. */
int gwtf_bn_running_update(const unsigned long long* table, const float* src, const float* momentum, int n, int f, void* stream);
/* dst[offset_i .. + numel_i) = src_i for n small tensors in one launch: table [n][3] = {src device pointer, offset, numel}
 * (floats).  Builds a stack's raw arena from its parameter / buffer tensors (the host mirror's torch.cat, one launch). */
int gwtf_gather_table(const unsigned long long* table, float* dst, int n, void* stream);
size_t gwtf_mtrain_dw1_floats(int f, int B, int N);
int gwtf_mtrain_phase(const GwtfTrainCtx* ctx, int phase, int step);
int gwtf_mtrain_forward(const GwtfTrainCtx* ctx);
int gwtf_mtrain_backward(const GwtfTrainCtx* ctx);
int gwtf_mtrain_final_forward_half(int C);
int gwtf_mtrain_final_backward_half(int C, int mode);

/* The sd1 weight gradient dW1[br][j][i] = sum_p dL/dacc[br][j](p) * h[br][i](p) is accumulated INSIDE the backward kernels
 * (points on the MFMA K axis, csrc/gwtf_bwd.hip); every workgroup leaves a compact [2][f][f] partial in the workspace.
 *   gwtf_dw1_partials(B, N)             partials one backward pass writes
 *   gwtf_dw1_workspace_floats(f, B, N)  floats of one pass's workspace region
 *   gwtf_dw1_reduce_scratch_floats(f)   floats of scratch the reduction needs AFTER the last region of the same buffer
 *   gwtf_dw1_reduce                     fixed-order (deterministic) two-stage sum over `passes` consecutive regions; branch br
 *                                       is written as an [f][f] block at dW1 + br * branch_stride (f*f for a dense [2][f][f];
 *                                       the raw-arena branch size to write a gradient record in place) */
int gwtf_dw1_partials(int B, int N);
size_t gwtf_dw1_workspace_floats(int f, int B, int N);
size_t gwtf_dw1_reduce_scratch_floats(int f);
int gwtf_dw1_reduce(float* workspace, int passes, float* dW1, size_t branch_stride, int f, int B, int N, void* stream);

/* Mixture negative log-likelihood over K flow components.
 * Replaces FlowMixtureNLL.forward (lib/networks/losses.py:88-137; per-component body :112-122 is
 * PointFlowNLL, :11-20).
 *   z, logdet [K][B][3][N]  outputs of gwtf_stack_forward(INVERSE) per component
 *   mu0, lv0  [K][B][3]     base Gaussian of each component (reference models.py:169-193)
 *   logits    [B][K]        un-normalised mixture log-weights
 *   point_lse [B][N]        optional: per-point logsumexp_k(log w_k + log p_k)
 *   nll_shape [B]           per-shape  -sum_n point_lse   (zeroed by the call)
 * The batch mean of nll_shape is the reference's pnll. */
int gwtf_mixture_nll(const float* z, const float* logdet, const float* mu0, const float* lv0,
                     const float* logits, float* point_lse, float* nll_shape,
                     int K, int B, int N, void* stream);

/* Backward of gwtf_mixture_nll: g_nll [B] = dL/d nll_shape; point_lse as returned by the forward.
 * Writes g_z, g_logdet [K][B][3][N]; g_mu0, g_lv0 [K][B][3]; g_logits [B][K] (the last three zeroed by the call). */
int gwtf_mixture_nll_backward(const float* z, const float* logdet, const float* mu0, const float* lv0,
                              const float* logits, const float* point_lse, const float* g_nll, float* g_z,
                              float* g_logdet, float* g_mu0, float* g_lv0, float* g_logits, int K, int B, int N,
                              void* stream);

/* Fused step of the reference's custom Adam / AMSGrad (lib/networks/optimizers.py:15-76; un-scaled decoupled decay
 * p -= wd*p + lr*m_hat/(sqrt(v_hat)+eps), :69-72) over many tensors per launch.  HOST arrays of n_tensors DEVICE
 * pointers; max_exp_avg_sq may be NULL when amsgrad == 0; `step` = 1-based count including this update. */
int gwtf_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                   float* const* max_exp_avg_sq, const size_t* numel, int n_tensors, float lr, double beta1, double beta2,
                   float eps, float weight_decay, int step, int amsgrad, void* stream);

/* The same update for ANY number of tensors in one launch, the pointer table in DEVICE memory (a model has ~1200 tensors):
 *   table [n_tensors][5] u64 = {param, exp_avg, exp_avg_sq, max_exp_avg_sq or 0, numel}    grads [n_tensors] u64
 *   chunk_map [n_chunks][2] i32 = {tensor index, chunk index within that tensor}, chunks of gwtf_adam_chunk_elems() elements
 * Only `grads` changes from step to step. */
int gwtf_adam_chunk_elems(void);
int gwtf_adam_step_table(const unsigned long long* table, const unsigned long long* grads, const int* chunk_map, int n_chunks,
                         float lr, double beta1, double beta2, float eps, float weight_decay, int step, int amsgrad,
                         void* stream);
/* The scalars of one update, on the host (launches nothing): out8 = {(float)lr, (float)beta1, (float)beta2, 1-beta1, 1-beta2,
 * bc1 = 1 - beta1^step, bc2s = sqrt(1 - beta2^step), 0}, each formed in double and cast to float once -- the very values
 * gwtf_adam_step and gwtf_adam_step_table hand their kernels (all three call one helper).  GWTF_E_BADARG: NULL out8, step < 1. */
int gwtf_adam_hyper(double lr, double beta1, double beta2, int step, float* out8);
/* gwtf_adam_step_table driven from DEVICE memory: the seven scalars are read from hyper[0..6] (a record of gwtf_adam_hyper), and every
 * workgroup returns before it touches anything when *skip != 0.  The update of an element is the one of the two launches above.
 * GWTF_E_BADARG without a launch: a NULL pointer, n_chunks < 0. */
int gwtf_adam_step_table_dev(const unsigned long long* table, const unsigned long long* grads, const int* chunk_map, int n_chunks,
                             const float* hyper, const int* skip, float eps, float weight_decay, int amsgrad, void* stream);

/* The training loop's state ON THE DEVICE (csrc/gwtf_loop.hip): one replay of a captured graph is one iteration of the reference's
 * train() (lib/networks/training.py:12-100) -- batch draw, forward, loss, backward, NaN guard, schedule, optimiser, meters -- and
 * the host reads this record when it wants to log.  160 bytes, no padding.
 *   meters: {val, sum, count} of LB, PNLL, GNLL, GENT, AverageMeter.update(v.item(), B) in float64
 *   hyper:  the gwtf_adam_hyper record of the update in flight (what gwtf_adam_step_table_dev reads)
 *   cursor: iteration within the epoch; n_iters: iterations of the epoch; adam_step: updates applied so far
 *   status: bit 0 = poisoned (sticky: a non-finite loss was seen), bit 1 = exhausted (cursor >= n_iters at the last begin)
 *   poisoned_at: cursor of the poisoned iteration (-1: none); skip: non-zero = the optimiser launches of this replay do nothing
 *   flag: the guard's verdict on this replay's loss, between gwtf_loop_detect and gwtf_loop_commit (MAX-reduced over ranks) */
typedef struct GwtfLoopState {
  double meters[12];
  float hyper[8];
  int cursor, n_iters, adam_step, status, poisoned_at, skip, flag, reserved;
} GwtfLoopState;
/* The launches' arguments.  state: a GwtfLoopState in device memory.  plan [plan_len] int32: the epoch's item indices, uploaded once
 * per epoch; rows [B] (and mesh_rows [B], or NULL: rows / views) the static index buffers the batch kernels read.  table
 * [table_rows][8]: row i = the gwtf_adam_hyper record of iteration i of the epoch.  terms: the four float32 loss terms {loss, pnll,
 * gnll, gent} of the replay.  use_flag: gwtf_loop_commit takes state->flag (written by gwtf_loop_detect, reduced by the caller)
 * instead of testing the loss itself. */
typedef struct GwtfLoopArgs {
  void* state;
  const int* plan;
  int* rows;
  int* mesh_rows;
  const float* table;
  const float* terms[4];
  int B, views, plan_len, table_rows, stop_on_inf, use_flag;
  void* stream;
} GwtfLoopArgs;
/* One workgroup each, plain stores only.
 * gwtf_loop_begin: cursor < n_iters, (cursor + 1) B <= plan_len, cursor < table_rows and not poisoned: rows = plan[cursor B ..
 *   (cursor + 1) B), mesh_rows = rows / views, the exhausted bit cleared.  Otherwise skip = 1, the exhausted bit set where the cursor
 *   is the reason, and rows / mesh_rows left as they were (valid indices of the last batch).
 * gwtf_loop_detect: flag = 1 when the loss is NaN -- bit test (bits & 0x7fffffff) > 0x7f800000, the library is built with
 *   -fno-honor-nans -- or, with stop_on_inf, infinite (>=); else 0.
 * gwtf_loop_commit: exhausted or already poisoned: skip = 1, nothing else moves.  A non-finite loss (use_flag: flag != 0): status |= 1,
 *   poisoned_at = cursor, skip = 1, nothing else moves.  Otherwise hyper = table[cursor]; the four meters take val = the term
 *   (LB: (pnll + gnll) - gent in float32, in that order, then widened), sum += val * B, count += B in float64; ++adam_step; ++cursor;
 *   skip = 0.
 * gwtf_loop_eval_commit: the commit of the VALIDATION pass (eval(), lib/networks/training.py:103-184), on a record of its own (state)
 *   that gwtf_loop_begin advances as it does the training loop's; table may be NULL, table_rows = n_iters.  Exhausted or already
 *   poisoned: nothing moves.  A NaN or infinite loss -- (bits & 0x7fffffff) >= 0x7f800000, eval() stops on both, stop_on_inf and
 *   use_flag are not read -- : status |= 1, poisoned_at = cursor, nothing else moves.  Otherwise the four meters take gwtf_loop_commit's
 *   arithmetic, then ++cursor.  adam_step, hyper and skip are never written.
 * GWTF_E_BADARG without a launch: a NULL record, state, plan, rows (begin), table (commit) or term (commit, eval_commit), loss term
 * (detect), B < 1, views < 1, plan_len < 0, table_rows < 0. */
int gwtf_loop_begin(const GwtfLoopArgs* args);
int gwtf_loop_detect(const GwtfLoopArgs* args);
int gwtf_loop_commit(const GwtfLoopArgs* args);
int gwtf_loop_eval_commit(const GwtfLoopArgs* args);

/* Structural losses between point sets -- the reference's only native code (CUDA extension
 * lib/metrics/pytorch_structural_losses, bound in pybind/bind.cpp:9-15).  Point sets are [b][n][3] / [b][m][3].
 *
 * gwtf_nn_distance replaces nn_distance (src/structural_loss.cpp:82-104, nndistance.cu:2-124): squared distance to the
 * nearest point of the other set and the index of the FIRST minimiser, both directions in one launch. */
int gwtf_nn_distance(const float* xyz1, const float* xyz2, float* dist1, int* idx1, float* dist2, int* idx2,
                     int b, int n, int m, void* stream);
/* Replaces nn_distance_grad (structural_loss.cpp:106-123, nndistance.cu:129-169); grad_xyz1/2 are zeroed by the call. */
int gwtf_nn_distance_grad(const float* xyz1, const float* xyz2, const float* grad_dist1, const int* idx1,
                          const float* grad_dist2, const int* idx2, float* grad_xyz1, float* grad_xyz2, int b,
                          int n, int m, void* stream);
/* Replaces ApproxMatch (structural_loss.cpp:22-37, approxmatch.cu:3-182): match [b][m][n] (zeroed by the call),
 * temp [b][2(n+m)] scratch. */
int gwtf_approx_match(const float* xyz1, const float* xyz2, float* match, float* temp, int b, int n, int m,
                      void* stream);
/* ApproxMatch + MatchCost in one schedule that never materialises the (b,m,n) matching: out [b] (zeroed by the call)
 * accumulates sum w * distance level by level.  What match_cost.py:10-23 computes when no gradient is wanted
 * (evaluation_metrics.py:25-30 is its only caller); temp as for gwtf_approx_match. */
int gwtf_emd_cost(const float* xyz1, const float* xyz2, float* temp, float* out, int b, int n, int m, void* stream);
/* The fused cost over a GRID of pairs, without expanded copies: a [na][n][3], b [nb][m][3]; out[r][c] (rows x nb, zeroed by the
 * call) is what gwtf_emd_cost gives for the pair (a[row0 + r], b[c]) -- same nine levels, same sweeps.  temp holds at least
 * rows * nb * 2(n+m) floats; rows * nb <= 65535 (the caller walks row0 in blocks). */
int gwtf_emd_cost_pairs(const float* a, const float* b, float* temp, float* out, int na, int nb, int n, int m, int row0,
                        int rows, void* stream);
/* Directed Chamfer reduction over all ordered pairs of two sets of clouds (the all-pairs matrices of evaluation_metrics.py:110-181
 * without its host loop): q [nq][n][3], t [nt][m][3];
 *   sum[i][j]    = sum over the points a of q_i of min_{b in t_j} |a - b|^2      (the minimum is dist1 of gwtf_nn_distance, bit for bit)
 *   cnt[h][i][j] = number of points of q_i whose minimum is < thr[h], compared in float32
 * thr: HOST array of n_thr <= 8 values, read during the call; with n_thr == 0 cnt and thr may be NULL.  Reductions are in a fixed
 * order inside one workgroup per pair: repeated calls give identical bits. */
int gwtf_chamfer_directed(const float* q, const float* t, float* sum, int* cnt, const float* thr, int n_thr, int nq, int nt,
                          int n, int m, void* stream);
/* Replaces MatchCost (structural_loss.cpp:39-55, approxmatch.cu:184-224): out [b] = sum match * distance. */
int gwtf_match_cost(const float* xyz1, const float* xyz2, const float* match, float* out, int b, int n, int m,
                    void* stream);
/* Replaces MatchCostGrad (structural_loss.cpp:57-75, approxmatch.cu:229-297): d out / d xyz1, d out / d xyz2 (un-scaled
 * by the upstream gradient, as in the reference; match_cost.py:38-45 applies it). */
int gwtf_match_cost_grad(const float* xyz1, const float* xyz2, const float* match, float* grad1, float* grad2,
                         int b, int n, int m, void* stream);

/* PointNet cloud encoder, eval-mode BatchNorm (lib/networks/encoders.py:9-28) fused with the max-pool its caller applies
 * (lib/networks/models.py:127-128).  widths = {3, C0, C1, ..., C_last} (n_widths entries); built instantiations:
 * {3,64,128,256,512} (every shipped config) and {3,64,128,64,128}; others return GWTF_E_UNSUPPORTED / size 0.
 *   raw     per layer l: weight[C_l][C_{l-1}] | bn.weight | bn.bias | bn.running_mean | bn.running_var   (C_l each)
 *   x       [B][3][N];  features [B][C_last][N] or NULL;  pooled [B][C_last] or NULL (zeroed by the call) */
size_t gwtf_encoder_raw_floats(const int* widths, int n_widths);
size_t gwtf_encoder_packed_floats(const int* widths, int n_widths);
int gwtf_encoder_pack(const float* raw, float* packed, const int* widths, int n_widths, void* stream);
int gwtf_encoder_forward(const float* x, const float* packed, float* features, float* pooled, int B, int N,
                         const int* widths, int n_widths, void* stream);

/* PointNet cloud encoder 3-64-128-256-512 under model.train() (batch-statistic BatchNorm1d; SyncBatchNorm = sum the
 * statistic arrays over the ranks between a kernel and its fold), max-pooled, forward AND backward, layer at a time.
 * Replaces, for lib/networks/encoders.py:9-28 + models.py:127-128 inside the training step (training.py:43-54), the chain of
 * library GEMM / batch-norm / elementwise calls and their autograd.  Channel counts C = {3, 64, 128, 256, 512}: layer l maps
 * C[l] -> C[l+1] channels with weight W_l [C[l+1]][C[l]]; kernels exist for layer = 1..3 (layer 0, 3 -> 64, is three FMAs
 * folded into layer 1's prologue).  x is the reference's (B, 3, N) fp32 tensor; the stored activations y_1, y_2 and gradients dA_2, dA_1 are
 * fp32 in tiles of 32 points, [B][ceil(N/32)][C][32] (gwtf_enc_train_act_floats): written and read by these entry points only.
 *   aff     [4][C]  = s, t, mean, rstd of a layer's BatchNorm (a = relu(s y + t));  table0 [64][4] = (s W_0 row, t)
 *   sums    replicated accumulators, zero on entry: a phase sums the 64 replicas, the caller the ranks, before the fold
 *   bconst  [3][C] + 4: dy = s gm + Q y + R per channel, then {up, down} = the power-of-two scale of the f16-split operand
 * gwtf_enc_train_supported(widths, n) -> 1 when this width list has kernels. */
int gwtf_enc_train_supported(const int* widths, int n_widths);
size_t gwtf_enc_train_units_floats(int layer);
/* floats of one stored activation / gradient array of `channels` channels.  y_1, y_2, dA_2, dA_1 are internal to the pipeline and live in
 * tiles of 32 points, [B][ceil(N / 32)][channels][32] + one spare tile (a wave / a k-step takes 32 points x all channels: one contiguous block), NOT in the
 * reference's (B, C, N); only x (B, 3, N) and the pooled (B, 512) outputs keep the reference's layouts. */
size_t gwtf_enc_train_act_floats(int B, int channels, int N);
/* floats of the scratch the weight-gradient kernels of `layer` = 1..3 leave their per-slice partials in (layer 3: the Gram matrix). */
size_t gwtf_enc_train_dw_partial_floats(int layer, int B, int N);
/* Everything the pipeline's launches take, one record for both directions (as GwtfTrainCtx is for the decoder stacks).  Every buffer
 * is caller-owned; "zero" = must be zero on entry; R = 64 statistic replicas; C = {3, 64, 128, 256, 512}; a per-layer array is
 * indexed by the layer l = 0..3 (BatchNorm l normalises y_l, C[l+1] channels) unless its comment says otherwise.
 * Data parallel (SyncBatchNorm): a phase leaves this rank's COMPACT sums in the *_c record, the caller sums a copy of it over the
 * ranks between the phases (the cuts of gwtf_enc_train_phase), and the *_fold / *_r pointer names that copy; on one rank it names the
 * *_c record itself.  bn.weight / bn.bias gradients and dW_0's moments are always this rank's (*_c). */
typedef struct GwtfEncTrainCtx {
  int B, N;                  /* x is (B, 3, N); N % 4 == 0 and N <= 12288 (the arg-max row table of top_scatter lives in LDS) */
  double n_total;            /* points the statistics cover: B*N summed over all ranks */
  float momentum[4];         /* of BatchNorm l: running = (1 - m) running + m batch (unbiased var) */
  const float* x;            /* [B][3][N]  the reference's input tensor */
  const float* W[4];         /* [C[l+1]][C[l]]  SharedDot weights */
  const float* gamma[4];     /* [C[l+1]]  bn.weight */
  const float* beta[4];      /* [C[l+1]]  bn.bias */
  float* running_mean[4];    /* [C[l+1]]  updated by the fold of layer l; NULL (both): skip */
  float* running_var[4];
  float* mom;                /* [R][12]  zero: += {sum x (3), sum x x^T (xx xy xz yy yz zz), -} over this rank's points (FWD_INIT) */
  float* mom_c;              /* [12]  the R copies summed (FWD_INIT); read by dw0_finish (this rank's moments) */
  const float* mom_fold;     /* [12]  what fold0 reads: mom_c, or its copy summed over the ranks */
  float* sums[3];            /* index l-1, l = 1..3: [R][2][C[l+1]]  zero: += {sum y_l, sum y_l^2} by the forward kernel of layer l */
  float* sums_c[3];          /* index l-1: [2][C[l+1]]  the R copies summed, behind that kernel */
  const float* sums_fold[3]; /* index l-1: what the fold of layer l reads: sums_c, or its copy summed over the ranks */
  float* ymax;               /* [4]  zero: ymax[l] = max |y_l|, l = 1..3 (bit pattern max; the backward's operand scale) */
  unsigned long long* kmax;  /* [B][512]  zero: 64-bit arg-max key of y_3 per (shape, channel), channels with gamma[3] >= 0 -- layer 3 stores */
  unsigned long long* kmin;  /* [B][512]  zero: arg-min key, channels with gamma[3] < 0 -- no y: BatchNorm + ReLU is monotone in y per channel */
  float* aff[4];             /* [4][C[l+1]] = s, t, mean, rstd of BatchNorm l (a = relu(s y + t)), written by its fold; non-finite
                              * statistics in aff[l-1] or here poison all of aff[l] with NaN */
  float* table0;             /* [64][4] = (s W_0 row, t): layer 0 folded into layer 1's prologue (fold0) */
  float* units_f[3];         /* index l-1: gwtf_enc_train_units_floats(l)  MFMA fragment images of W_l (forward) ... */
  float* units_b[3];         /* ... and of W_l^T (backward), all six from one launch */
  float* y[2];               /* index l-1, l = 1, 2: gwtf_enc_train_act_floats(B, C[l+1], N)  y_l = W_l . relu(s in + t), tiled */
  float* pooled;             /* [B][512] = max_n relu(s y_3 + t) from the keys; NaN where a statistic or the extreme is not finite */
  int* amax;                 /* [B][512]  its first arg-max */
  float* ystar;              /* [B][512]  y_3 there */
  /* backward only */
  const float* g_pooled;     /* [B][512]  dL/d pooled */
  float* gp;                 /* [B][512] = g_pooled where pooled > 0 (BWD_TOP) */
  float* gmax;               /* [4]  zero: gmax[l] = max |dL/da_l| masked, l = 1..3 (gmax[3]: max |gp|) */
  float* g_sums[3];          /* index l = 0..2: [R][5][64], [R][2][128], [R][3][256]  zero: += {sum gm_l, sum gm_l yhat_l} (then l = 0: sum gm x_d,
                              * 3 rows; l = 2: sum a_2) by the backward kernel of layer l + 1 */
  float* g_sums_c[4];        /* l = 0..2: [5][64], [2][128], [3][256]  the R copies summed, behind that kernel; l = 3: [2][512] = {sum gp,
                              * sum gp yhat*} written by BWD_TOP.  Rows 1 / 0 are this rank's bn.weight / bn.bias gradients */
  const float* g_sums_r[4];  /* [2][C[l+1]]  what the consts kernel of layer l reads: g_sums_c[l], or a copy of its first two rows summed over the ranks */
  float* bconst[4];          /* [3][C[l+1]] + 4: dy = s gm + Q y + R per channel, then {up, down} = the power-of-two operand scale */
  float* units_m;            /* gwtf_enc_train_units_floats(3) / 2  fragment images of M 2^k (gwtf_enc_train_mform) */
  float* mconst;             /* [256 + 4] = {W_3^T R, 2^-k, 0, 0, 0} */
  float* mform_ws;           /* gwtf_enc_train_mform_workspace_floats(256) scratch */
  float* extra;              /* [B][512][256]  row r of shape b = sum of gp[b][c] s[c] W_3[c][:] over the channels whose arg-max is that point
                              * (only the used rows are written) */
  int* slot_of;              /* [B][N]  row of a point, or -1 */
  int* tables;               /* [B (2 * 512 + 2)] scratch of top_scatter */
  float* a2rows;             /* [B][512][256]  row slot_of[b][n] of shape b = a_2(b, :, n) of every arg-max point n (other rows not written) */
  float* dA[2];              /* index l-1, l = 1, 2: gwtf_enc_train_act_floats(B, C[l+1], N)  dL/da_l masked by a_l > 0, tiled; dA[1] =
                              * (M a_2 + v + extra) by the top layer, dA[0] = W_2^T dy_2 by layer 2 (layer 1 stores none) */
  float* partials;           /* max over l = 1..3 of gwtf_enc_train_dw_partial_floats(l, B, N) scratch */
  float* gram;               /* [256][256] = sum_p a_2 a_2^T over this rank's points */
  float* S;                  /* [512][256]  S[c] = sum_b gp[b][c] a_2(b, amax[b][c]) */
  float* dW[4];              /* [C[l+1]][C[l]]  the weight gradients over this rank's points */
  void* stream;
} GwtfEncTrainCtx;
/* The chain is cut where a data-parallel run sums the statistics over the ranks: the record named behind a phase goes into what *_fold / *_r names:
 *   FWD_INIT      xmoments, compact                                                     -> mom_c
 *   FWD_LAYER l   l = 0: fold0, pack_all; l = 1..3: fold of layer l; then l < 3: forward kernel of layer l + 1, compact
 *                 -> sums_c[l]; l = 3: pool
 *   BWD_TOP       top                                                                   -> g_sums_c[3]
 *   BWD_LAYER l   consts of layer l, then  l = 3: mform, top_scatter, backward_top (M form: dL/da_2 = M a_2 + v + extra, M = W_3^T diag(Q)
 *                 W_3, v = W_3^T R), compact, dw3 (Gram form), dw3_finish;  l = 2, 1: backward, dw, compact;  l = 0: dw0_finish
 *                 -> g_sums_c[l - 1][0..2)
 * gwtf_enc_train_forward / _backward are the loops over the phases.  GWTF_E_BADARG without a launch: a NULL record, B or N <= 0,
 * N % 4 != 0, N * sizeof(int) > 48 KiB, n_total <= 0, a NULL field other than running_mean / running_var (the backward fields only
 * for a backward phase), a phase or layer out of range. */
#define GWTF_ENC_PHASE_FWD_INIT 0
#define GWTF_ENC_PHASE_FWD_LAYER 1
#define GWTF_ENC_PHASE_BWD_TOP 2
#define GWTF_ENC_PHASE_BWD_LAYER 3
int gwtf_enc_train_phase(const GwtfEncTrainCtx* ctx, int phase, int layer);
int gwtf_enc_train_forward(const GwtfEncTrainCtx* ctx);
int gwtf_enc_train_backward(const GwtfEncTrainCtx* ctx);
/* The small dense algebra between those kernels (csrc/gwtf_encoder_glue.hip), a launch or two each instead of chains of library calls:
 *   gwtf_stat_compact          out [n] = sum of the `replicas` copies of slab [replicas][n], fixed order
 *   gwtf_enc_train_mform       bconst3 = {s, Q, R} [3][C4] of layer 3 -> units_m = fragment images of M 2^k (M = W_3^T diag(Q) W_3,
 *                              k = 8 - floor(log2 max|M|)), mconst [C3 + 4] = {W_3^T R, 2^-k, 0, 0, 0}: what the top layer's backward kernel
 *                              reads.  workspace: gwtf_enc_train_mform_workspace_floats(C3) floats.  C3 % 32 == 0, C4 % 64 == 0.
 *   gwtf_enc_train_dw3_finish  dW_3 [C4][C3] = s (.) S + Q (.) (W_3 gram) + R (x) a2sum   (a2sum [C3] = sum_p a_2)
 *   gwtf_enc_train_dw0_finish  dW_0 [C1][3] = s (.) red5[2:5]^T + Q (.) (W_0 Mxx) + R (x) m[:3]; bconst0 = {s, Q, R} [3][C1] of layer 0,
 *                              red5 [5][C1] = the compact sums the backward kernel of layer 1 leaves (g_sums_c[0]), mom12 = this rank's coordinate
 *                              moments (mom_c) */
int gwtf_stat_compact(const float* slab, float* out, int replicas, int n, void* stream);
size_t gwtf_enc_train_mform_workspace_floats(int C3);
int gwtf_enc_train_mform(const float* W3, const float* bconst3, float* workspace, float* units_m, float* mconst, int C3, int C4,
                         void* stream);
int gwtf_enc_train_dw3_finish(const float* bconst3, const float* S, const float* W3, const float* gram, const float* a2sum, float* dW3,
                              int C3, int C4, void* stream);
int gwtf_enc_train_dw0_finish(const float* bconst0, const float* red5, const float* W0, const float* mom12, float* dW0, int C1,
                              void* stream);

/* Global prior flow on the shape latent: the whole GlobalRNVPDecoder (lib/networks/decoders.py:7-38; RealNVPFlowCouple /
 * RealNVPFlow, flows.py:163-243) as ONE launch per direction -- forward (the lists the reference returns) and backward
 * (every parameter, the input, gradients entering through any gs[j] / logvars[j] slot), eval- or train-mode BatchNorm.
 *   raw       gwtf_prior_raw_floats(n_flows, G, F) floats: per elementary flow j (2 per couple), branch mu then logvar:
 *             mlp0.weight[F][Gk] | bn.weight[F] | bn.bias[F] | bn.running_mean[F] | bn.running_var[F] | mlp1.weight[Gw][F] |
 *             mlp1.bias[Gw]     (record j starts at gwtf_prior_raw_offset(n_flows, G, F, j))
 *   g         [B][G], B <= 128;   gs, mus, logvars  [2 n_flows][B][G] direct-ordered lists (decoders.py:24-36)
 *   workspace gwtf_prior_workspace_floats(B, G, F) floats of scratch
 *   bn_stats  [2 n_flows][2 branches][2][F] = batch {mean, biased var} of every BatchNorm (train; may be NULL)
 *   backward: g_gs / g_logvars [2 n_flows][B][G] = dL/d gs[j], dL/d logvars[j] (either may be NULL); g_raw (zero on entry)
 *             receives the parameter gradients in the raw layout; g_g [B][G] = dL/d g. */
size_t gwtf_prior_raw_floats(int n_flows, int G, int F);
size_t gwtf_prior_raw_offset(int n_flows, int G, int F, int j);
size_t gwtf_prior_workspace_floats(int B, int G, int F);
int gwtf_prior_forward(const float* g, const float* raw, float* gs, float* mus, float* logvars, float* workspace,
                       float* bn_stats, int n_flows, int B, int G, int F, float eps, int mode, int training, void* stream);
int gwtf_prior_backward(const float* g, const float* raw, const float* gs, const float* mus, const float* logvars,
                        const float* g_gs, const float* g_logvars, float* workspace, float* g_raw, float* g_g,
                        int n_flows, int B, int G, int F, float eps, int mode, int training, void* stream);

/* Per-shape MLP heads: FeatureEncoder / WeightsEncoder (lib/networks/encoders.py:31-89) = n_layers x [Linear(no bias) ->
 * BatchNorm1d -> Swish], then Linear(bias) heads (mu, logvar), the mixture-weight head ending in log_softmax (:87-91) -- the
 * modules g_posterior, p_prior and mixture_weights_encoder of the model (models.py:51-59, flow_mixture.py:28-32).  One launch runs
 * `n_heads` (1 or 2) LAYERS ON THE SAME INPUT x, forward and backward: one layer of a trunk, or the mu and logvar heads of a
 * FeatureEncoder (encoders.py:55-60) together.  A workgroup owns 16 output columns of one head and all B rows, so BatchNorm's column
 * statistics are local; the workgroups of head 0 come first, then head 1's.  Per-head fields are arrays of two (entry 1 is not read
 * when n_heads = 1).
 *   x [B][Din], W [Dout][Din], bias / gamma / beta [Dout] (each may be NULL), out [B][Dout]
 *   bn_mode  0: no BatchNorm   1: batch statistics; running_mean / running_var (may be NULL) get the momentum update with the
 *            unbiased batch variance applied `bn_updates` times, *num_batches_tracked += bn_updates   2: running statistics
 *   act      0: none   1: swish   2: log_softmax over the columns (Dout <= 16)
 *   ypre [B][Dout] = x W^T (the backward's input), stats [3][Dout] = mean, biased variance, 1/sqrt(var + bn_eps) used
 * backward: g_out [B][Dout] -> g_y [B][Dout] (scratch: dL/d(x W^T)), g_W [Dout][Din], g_bias / g_gamma / g_beta [Dout] (each may be
 *   NULL), g_x [B][Din] (NULL: not wanted) = the sum of the heads' input gradients: always overwritten, head 1's product accumulates
 *   onto head 0's inside the kernel. */
typedef struct GwtfHeadArgs {
  const float* x;
  float* g_x;
  int n_heads, B, Din;
  int bn_updates;                    /* >= 1 */
  const float* W[2];
  const float* bias[2];
  const float* gamma[2];
  const float* beta[2];
  float* running_mean[2];
  float* running_var[2];
  long long* num_batches_tracked[2]; /* may be NULL */
  float* ypre[2];                    /* forward outputs (read by the backward) */
  float* stats[2];                   /* NULL with bn_mode 0 */
  float* out[2];
  const float* g_out[2];             /* backward */
  float* g_y[2];
  float* g_W[2];
  float* g_bias[2];
  float* g_gamma[2];
  float* g_beta[2];
  int Dout[2], bn_mode[2], act[2];
  float momentum[2], bn_eps[2];
  void* stream;
} GwtfHeadArgs;
/* Both validate on the host before any launch.  GWTF_E_BADARG: a NULL record, n_heads outside 1..2, bn_updates < 1, a NULL x, and per
 * head: a NULL W, ypre or out (backward also g_out or g_y), sizes gwtf_head_layer_supported refuses (B outside 1..65536, Din or Dout
 * outside 1..4096, act 2 with Dout > 16), bn_mode or act outside 0..2, bn_mode != 0 without stats, bn_mode 2 without running
 * statistics, bn_mode 1 with B < 2.  gwtf_head_layer_supported -> 1 when the kernels cover (B, Din, Dout, act). */
int gwtf_head_layer_supported(int B, int Din, int Dout, int act);
int gwtf_heads_forward(const GwtfHeadArgs* args);
int gwtf_heads_backward(const GwtfHeadArgs* args);

/* Image encoder of the single-view-reconstruction model (go_with_the_flows_amd/resnet.py): the 4-channel ResNet-18 of the
 * reference's lib/networks/resnet.py:9-224 (BasicBlock x [2,2,2,2], fc -> fc_bn -> ReLU head), EVAL-MODE forward only
 * (csrc/gwtf_resnet.hip).  Replaces img_encoder(images) in flow_mixture.py:212 for model.eval().
 *   image   [B][4][H][W] NCHW fp32, H, W >= 32
 *   packed  [gwtf_resnet_packed_floats(num_classes)], BatchNorm folded by the caller (float64 on the host, rounded once):
 *           for each convolution in network order -- stem; then per block conv1, conv2 -- W [Cout][Kp] then shift [Cout], with
 *           W[n][k] = weight[n][ci][kh][kw] * s[n], k = (kh * KW + kw) * Cin + ci, columns K..Kp-1 zero (Kp = K rounded up to
 *           16; only the stem, K = 196, pads), s = gamma / sqrt(running_var + eps), shift = beta - running_mean * s.  The first
 *           block of layer2..4 appends its downsample to conv2's rows: Kp = 9 * Cout + Cin, columns 9 Cout + ci = downsample
 *           weight[n][ci] * s_ds[n], shift = shift_conv2 + shift_ds.  Then the head: W [num_classes][512] = fc.weight * s_fc,
 *           bias [num_classes] = (fc.bias - running_mean) * s_fc + beta (fc_bn).
 *   out     [B][num_classes]
 *   work    [gwtf_resnet_work_floats(B, H, W, tune)] scratch (NHWC activations, split-K partial sums)
 *   tune    GWTF_TUNE_RESNET_TILE(1: 64x64, 2: 32x32, 3: 64x32 output tile; 0: by shape) | GWTF_TUNE_RESNET_SPLIT(n: K split
 *           in n parts, 1: none; 0: by shape).  Splits are summed in a fixed order: a launch is bit-identical to the last.
 * gwtf_resnet_work_floats returns 0 for arguments gwtf_resnet_forward rejects (GWTF_E_BADARG). */
#define GWTF_TUNE_RESNET_TILE(t) ((t) & 0xf)
#define GWTF_TUNE_RESNET_SPLIT(n) (((n) & 0xff) << 4)
#define GWTF_TUNE_RESNET_TILE_OF(w) ((w) & 0xf)
#define GWTF_TUNE_RESNET_SPLIT_OF(w) (((w) >> 4) & 0xff)
size_t gwtf_resnet_packed_floats(int num_classes);
size_t gwtf_resnet_work_floats(int B, int H, int W, int tune);
int gwtf_resnet_forward(const float* image, const float* packed, float* out, float* work, int B, int H, int W, int num_classes,
                        int tune, void* stream);

/* Training batches drawn on the device (csrc/gwtf_clouds.hip): what ShapeNetCoreDataset.__getitem__ (lib/datasets/datasets.py:69-106)
 * does per item on the host -- sample_cloud (lib/datasets/cloud_sampling.py:4-32) and the composed cloud transformations
 * (lib/datasets/cloud_transformations.py:6-64,79-103, Random3DRotation excluded) -- for B shapes of a store of packed meshes (the
 * datasets of meshes.h5, preprocess_ShapeNetCore.py:55-69) in one launch plus a finishing launch.
 *   Face of a point: #{k < search_len : thresholds[k] <= w} for a 32-bit word w, thresholds[k] = ceil(cdf[k] * 2^32) of the float64
 *   CDF RandomState.choice builds -- np.searchsorted(cdf, w * 2^-32, 'right') for every w.  search_len counts the shape's thresholds
 *   below 2^32 (the others can never be reached and are not read; store them as 0xffffffff), so the count stays at or below the last
 *   face with area, and leading zero-area faces (threshold 0) are always counted past.
 *   Point: (v0 + s1 (v1 - v0)) + s2 (v2 - v0) in float32, (s1, s2) folded to 1 - s when s1 + s2 > 1.  Point j of row r goes to
 *   cloud[r][:][j] -- with an eval cloud (M even) to cloud[r][:][j/2] for even j, eval_cloud[r][:][j/2] for odd j.
 *   Randomness: Philox4x32-10, key (seed lo, seed hi), counter (j, r, call lo, call hi | stream << 28), call < 2^60; stream 0 gives
 *   w = word 0, s1 = (word 1 >> 8) 2^-24, s2 = (word 2 >> 8) 2^-24; stream 1 Box-Muller normals from (word 0, word 1) -> x, y and
 *   (word 2, word 3) -> z.  With `words` non-NULL the draws are read instead (tests, fixtures).
 *   The finishing launch subtracts the per-cloud means (fixed summation order, no float atomics) and stores call + 1 into state[1].
 * A row index outside [0, n_shapes) yields NaN points and reads nothing. */
typedef struct GwtfCloudArgs {
  const int* rows;                   /* [B] shape indices, repeats allowed */
  const float* vertices;             /* [V][3] all shapes' vertices */
  const int* faces;                  /* [F][3] vertex indices LOCAL to the shape's vertex slice */
  const unsigned* thresholds;        /* [F] */
  const long long* vertices_bounds;  /* [n_shapes + 1] */
  const long long* faces_bounds;     /* [n_shapes + 1] */
  const int* search_len;             /* [n_shapes] */
  const float* orig_c;               /* [n_shapes][3], read when recenter */
  const float* orig_s;               /* [n_shapes], read when rescale */
  float* cloud;                      /* [B][3][N], N = M / 2 with an eval cloud, else M */
  float* eval_cloud;                 /* [B][3][N] or NULL */
  float* partials;                   /* [B][gwtf_cloud_partials(M)][6] scratch, written and read when center */
  unsigned long long* state;         /* {seed, call} */
  const unsigned* words;             /* explicit draws: [B][M] face words, or NULL (Philox) */
  const float* s1;                   /* [B][M] in [0, 1) */
  const float* s2;                   /* [B][M] */
  const float* normals;              /* [B][3][M] standard normals, read when noise */
  int B, M, n_shapes;
  int rescale, recenter, translate, scale, noise, center;   /* cloud_transformations.py:79-96, applied in this order */
  int tune;                          /* low 16 bits: points a workgroup walks (a multiple of 256; 0: 1024); results do not depend on it */
  float shift[3];                    /* TranslateCloud: x - shift */
  float scale_div;                   /* ScaleCloud: x / scale_div, > 0 */
  float noise_scale;                 /* AddNoise2Cloud: x + noise_scale * z, > 0 */
  void* stream;
} GwtfCloudArgs;
/* Tiles of 256 points whose partial sums one row leaves in `partials` (reference cloud_transformations.py:56-64). */
int gwtf_cloud_partials(int M);
/* GWTF_E_BADARG without a launch: a NULL record or required pointer, B < 1, M < 1, odd M with an eval cloud, scale_div / noise_scale
 * <= 0 where enabled, explicit draws given in part (reference cloud_sampling.py:4-32). */
int gwtf_sample_clouds(const GwtfCloudArgs* args);

/* Batches drawn from STORED clouds (csrc/gwtf_clouds.hip, cloud_gather_kernel; added without a version change: no existing entry or
 * record moved).  A store holds n_shapes clouds packed as points [T][3] with bounds [n_shapes + 1]; cloud s has
 * P = bounds[s + 1] - bounds[s] points, 1 <= P < 2^31.  Draw j in [0, M) of batch row r, shape s = rows[r], takes the stored point
 * at an INDEX in [0, P):
 *   Round and slot: q = j / P, t = j % P.  Within a round distinct j give distinct points -- the draw is without replacement while
 *   M <= P, so cloud and eval_cloud are disjoint; past P it wraps into a new permutation, and every point is used floor(M / P) or
 *   ceil(M / P) times.
 *   Index: a keyed bijection on [0, P).  b = max(1, ceil(log2 P)), h = (b + 1) / 2, domain 2^(2h) (P <= domain < 4P for P > 1).  Six
 *   round keys: K0..K3 the four words of the Philox4x32-10 block with key (seed lo, seed hi) and counter
 *   (2q, r, call lo, call hi | 2 << 28), K4 K5 the first two words of the block with counter (2q + 1, r, call lo, call hi | 2 << 28)
 *   -- stream 2; streams 0 and 1 keep the meaning they have in gwtf_sample_clouds.  Start x = t and repeat until x < P:
 *   L = x >> h, R = x & (2^h - 1); for i = 0..5: (L, R) = (R, L ^ (fmix32(R ^ K_i) >> (32 - h))); x = (L << h) | R.  fmix32 is
 *   murmur3's finaliser: x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16.  The walk follows the cycle of
 *   t in a permutation of the domain, so it returns to [0, P); it is cut at 1024 steps all the same, and then yields a NaN point.
 *   permute = 0: index = t, the stored order (fixed sets).
 *   With `index` non-NULL the indices are read instead (tests, fixtures); one outside [0, P) yields a NaN point and reads nothing.
 * Everything behind the index is gwtf_sample_clouds': even j to cloud[r][:][j/2] and odd j to eval_cloud with an eval cloud, the six
 * transformations in the same order and the same float32 statements, noise from stream 1 with counter (j, r, ...) or from
 * `normals` with explicit indices, per-tile sums of 256 points in the same fixed tree, the same finishing launch (centring, call + 1).
 * A NaN point adds nothing to its tile's sums.  A row index outside [0, n_shapes) yields NaN points and reads nothing.  Results do
 * not depend on the tuning word. */
typedef struct GwtfStoredCloudArgs {
  const int* rows;                   /* [B] shape indices, repeats allowed */
  const float* points;               /* [T][3] all shapes' points */
  const long long* bounds;           /* [n_shapes + 1] */
  const float* orig_c;               /* [n_shapes][3], read when recenter */
  const float* orig_s;               /* [n_shapes], read when rescale */
  float* cloud;                      /* [B][3][N], N = M / 2 with an eval cloud, else M */
  float* eval_cloud;                 /* [B][3][N] or NULL */
  float* partials;                   /* [B][gwtf_cloud_partials(M)][6] scratch, written and read when center */
  unsigned long long* state;         /* {seed, call} */
  const int* index;                  /* explicit draws: [B][M] point indices, or NULL (the rule above) */
  const float* normals;              /* [B][3][M] standard normals, read when noise and index */
  int B, M, n_shapes;
  int rescale, recenter, translate, scale, noise, center;   /* as in GwtfCloudArgs */
  int permute;                       /* 0: the stored order */
  int tune;                          /* as in GwtfCloudArgs */
  float shift[3];
  float scale_div;
  float noise_scale;
  void* stream;
} GwtfStoredCloudArgs;
/* GWTF_E_BADARG without a launch: a NULL record or required pointer, B outside 1..65535, M < 1, odd M with an eval cloud, scale_div /
 * noise_scale <= 0 where enabled, normals without index, index without normals when noise. */
int gwtf_sample_stored_clouds(const GwtfStoredCloudArgs* args);
/* The index rule above on the host: the image of t under the permutation of [0, P) keyed by keys6[0..5]; 0xffffffff for a NULL
 * keys6, t >= P, P outside [1, 2^31) and at the 1024-step cap. */
unsigned gwtf_perm_index(const unsigned* keys6, unsigned t, unsigned P);

/* Device-resident generation (ABI 10 gained these entry points; no existing record or signature changed): every point of S generated
 * clouds draws its mixture component and its base sample on the device and is laid out so that ONE stack launch sends it through its
 * own component -- the sampling branch of Flow_Mixture_Model.decode (lib/networks/flow_mixture.py:146-177: np.random.choice over the
 * normalised weights, reparameterize of models.py:99-109, the K decoder passes, the scatter by mask) without a host round trip.
 *
 * gwtf_mixture_route (csrc/gwtf_route.hip): one workgroup per shape, then a one-thread launch that stores call + 1 into state[1].
 *   Thresholds of shape s from its K float32 logits, in float64: e_k = exp(l_k - max l), cdf = cumsum(e),
 *   T[k] = min(ceil(cdf[k] / cdf[K-1] * 2^32), 2^32 - 1) -- RandomState.choice's cdf and searchsorted(cdf, w 2^-32, 'right') at 32-bit
 *   resolution, the construction of the cloud sampler's face thresholds.  Component of point i: #{k < K-1 : T[k] <= w_i}.
 *   Base sample: z = eps * expf(0.5f * lv0) + mu0 per coordinate, float32, uncontracted; mu0 / lv0 of shape s are the three floats at
 *   mu0 + s * mu0_stride (stride 0: one base Gaussian for all shapes).
 *   Randomness: Philox4x32-10, key (seed lo, seed hi), counter (i, s, call lo, call hi | stream << 28), call < 2^60, with the streams
 *   the cloud sampler leaves free: stream 2 gives w_i = word 0; stream 3 Box-Muller normals from (word 0, word 1) -> eps 0, eps 1 and
 *   (word 2, word 3) -> eps 2.  Explicit draws replace either stream: labels_in (taken as they are, clamped to [0, K); no thresholds
 *   are built) or words; z0_in (the base samples themselves) or normals.  state may be NULL when neither stream is drawn.
 *   Layout, P = points per tile of the stack launch (64, 128 or 256): a shape owns tiles = gwtf_route_tiles(n, K, P) =
 *   floor((n + K (P - 1)) / P) tile slots, an upper bound of sum_k ceil(c_k / P) for any counts c_k that sum to n; component k takes
 *   ceil(c_k / P) consecutive slots, in component order, its points in their original order (a stable counting sort: the outputs are a
 *   function of the labels alone and bit-reproducible -- no atomics on global memory).
 *     tile_comp [S][tiles]        component of each slot, -1: unused
 *     perm      [S][tiles * P]    original index of the point in each position, -1: padding
 *     zp        [S][3][tiles * P] base samples in that order, padding 0
 *     labels    [S][n]            component of each point
 *     thresholds [S][K]           the bits of the uint32 thresholds (may be NULL; not written with labels_in)
 * gwtf_stack_forward_routed (csrc/gwtf_stack.hip): the split-f16 stack, DIRECT, on that layout -- slot (s, t) runs component
 *   tile_comp[s][t] on its P positions of zp and stores each point at perm's index of out / logdet [S][3][n] (logdet may be NULL);
 *   unused slots exit at once.  weights / film as for gwtf_stack_forward with K components; P must be the routing call's (f > 64:
 *   P <= 128, else GWTF_E_UNSUPPORTED).  No work list and no exact re-run: a point that leaves the f16-safe range comes back NaN.
 *   tune: GWTF_TUNE_GENERIC_BODY only (the caller chooses P, e.g. from gwtf_stack_plan over K equal segments). */
typedef struct GwtfRouteArgs {
  const float* logits;               /* [S][K]; NULL with labels_in */
  const float* mu0;                  /* base mean / log-variance; NULL with z0_in */
  const float* lv0;
  long long* state;                  /* {seed, call} */
  const int* words;                  /* explicit: [S][n] bits of the uint32 label words, or NULL */
  const int* labels_in;              /* explicit: [S][n] components; takes precedence over words */
  const float* normals;              /* explicit: [S][3][n] standard normals, or NULL */
  const float* z0_in;                /* explicit: [S][3][n] base samples; takes precedence over normals */
  int* thresholds;
  int* tile_comp;
  int* perm;
  float* zp;
  int* labels;
  int S, n, K, P;
  int mu0_stride, lv0_stride;        /* floats from one shape's values to the next: 3, or 0 for shared values */
  void* stream;
} GwtfRouteArgs;
typedef struct GwtfRoutedStackArgs {
  const float* zp;
  const float* weights;              /* [K][C][gwtf_packed_w_coupling_floats] */
  const float* film;                 /* [S][K*C][gwtf_film_out_floats] */
  const int* tile_comp;
  const int* perm;
  float* out;                        /* [S][3][n] */
  float* logdet;                     /* [S][3][n] or NULL */
  int K, S, n, P, C, f;
  int pattern0;
  int tune;
  float eps;
  void* stream;
} GwtfRoutedStackArgs;
/* Tile slots per shape of the routed layout; 0 for arguments the two entry points reject.  Host only. */
int gwtf_route_tiles(int n, int K, int P);
/* Both return GWTF_E_BADARG without a launch for a NULL record or required pointer, K outside 1..64, S < 1, n < 1, P not in
 * {64, 128, 256}, a draw that is neither explicit nor given a state; the stack launch GWTF_E_UNSUPPORTED for a width outside 1..128
 * or P = 256 beyond f = 64. */
int gwtf_mixture_route(const GwtfRouteArgs* args);
int gwtf_stack_forward_routed(const GwtfRoutedStackArgs* args);

/* Latent sweeps (added without a version change; no existing record, signature or kernel changed): R = S rows are decoded, row r
 * taking the DRAWS of shape r / group -- T = group steps of a sweep between two latent codes share their label words and normals,
 * so every step is a sample of the model at its own code and point i moves continuously along the sweep -- and, per component, a
 * base Gaussian of its own, so that chosen components can follow the sweep while the others stay at one code.
 *
 * gwtf_mixture_route_sweep (csrc/gwtf_route.hip, the body of gwtf_mixture_route): one workgroup per ROW, then the same one-thread
 * launch that stores call + 1 into state[1] (one advance per call, whatever R).
 *   Draws: the Philox counter is (i, r / group, call lo, call hi | stream << 28), and words / labels_in / normals / z0_in hold
 *   [S / group][...]: row r reads row r / group of each.  group = 1 draws what gwtf_mixture_route draws.
 *   Per row: logits [R][K] -> thresholds and the component of every point by the rule above, from the row's own logits.
 *   Base sample: z = eps * expf(0.5f * lv0) + mu0 with the three floats at mu0 + r * mu0_stride + k * mu0_stride_k for the point's
 *   OWN component k (its label is known before the sample is formed; the K x 3 means and deviations of a row sit in LDS);
 *   mu0_stride_k = 0: one base for all components, and with group = 1 every output bit is gwtf_mixture_route's.
 *   Outputs: tile_comp, perm, zp, labels, thresholds as above for R rows; gwtf_stack_forward_routed takes them with S = R. */
typedef struct GwtfRouteSweepArgs {
  const float* logits;               /* [R][K]; NULL with labels_in */
  const float* mu0;                  /* base mean / log-variance tables; NULL with z0_in */
  const float* lv0;
  long long* state;                  /* {seed, call} */
  const int* words;                  /* explicit: [R / group][n] bits of the uint32 label words, or NULL */
  const int* labels_in;              /* explicit: [R / group][n] components; takes precedence over words */
  const float* normals;              /* explicit: [R / group][3][n] standard normals, or NULL */
  const float* z0_in;                /* explicit: [R / group][3][n] base samples; takes precedence over normals */
  int* thresholds;                   /* [R][K] or NULL */
  int* tile_comp;                    /* [R][tiles] */
  int* perm;                         /* [R][tiles * P] */
  float* zp;                         /* [R][3][tiles * P] */
  int* labels;                       /* [R][n] */
  int S, n, K, P;                    /* S: the R rows */
  int mu0_stride, lv0_stride;        /* floats from one row's values to the next: 3, or 0 for shared values */
  int group;                         /* >= 1, divides S: rows per shape of draws */
  int mu0_stride_k, lv0_stride_k;    /* floats from one component's table to the next, or 0: one base for all components */
  void* stream;
} GwtfRouteSweepArgs;
/* GWTF_E_BADARG without a launch for everything gwtf_mixture_route refuses, group < 1, S % group != 0 and a negative stride. */
int gwtf_mixture_route_sweep(const GwtfRouteSweepArgs* args);

/* Image batches transformed on the device (csrc/gwtf_images.hip; added without a version change, no existing record or signature
 * moved): what ShapeNetAllDataset.__getitem__ (lib/datasets/datasets.py:173-222) and ComposeImageTransformation
 * (lib/datasets/image_transformations.py:7-95) do per item on the host, for B images of a store of raw uint8 renderings
 * [n_images][C][H][W], C in {3, 4}, in ONE launch.  Stage order and arithmetic, all float32 and uncontracted:
 *   ToNumpy     v_c = (float)byte / 255.f, correctly rounded (the bits of np.float32(byte / 255.) for all 256 bytes); then
 *               v_0 = v_2 * v_0, v_1 = v_2 * v_1 (channel 2, not alpha: image_transformations.py:13)
 *   Resize      cv2's INTER_LINEAR from per-axis tables the HOST computes in float64 and rounds: column x of the resized image reads
 *               source columns xs[x] and min(xs[x] + 1, W - 1) with weights 1.f - xf[x] and xf[x], rows likewise from ys / yf;
 *               r = S[s0] * a0 + S[s1] * a1 along x first, then out = r0 * b0 + r1 * b1 along y
 *   Pad         pad_y zero rows above and below, pad_x zero columns left and right (before grayscale and normalisation)
 *   Grayscale   a new channel 0 = (gray[0] * v_0 + gray[1] * v_1) + gray[2] * v_2; the others move up by one
 *   Normalize   (v_c - mean[c]) / stdev[c], correctly rounded, c the channel at this stage
 *   Noise       min(max(v_c + n_c, 0), 1): n from `noise` ([B][C_stage][H_out][W_out], already scaled) or, when that is NULL,
 *               noise_scale * z with z from Philox4x32-10, key (seed lo, seed hi), counter (y * W_out + x, b, call lo,
 *               call hi | stream << 28): stream 4 Box-Muller normals from (word 0, word 1) -> channels 0, 1 and (word 2, word 3) ->
 *               channels 2, 3; stream 5 (word 0, word 1) -> channel 4.  A second, one-thread launch then stores call + 1 into state[1]
 *   RemoveAlpha keeps the first four channels
 * C_stage = C + gray, C_out = remove_alpha ? min(C_stage, 4) : C_stage; H_out = H_r + 2 pad_y, W_out = W_r + 2 pad_x with
 * (H_r, W_r) the resized size (the source's without resize).  A source channel no output channel needs is never loaded.
 * rows[b] names the source image of output b (NULL: image b); an index outside [0, n_images) yields an all-NaN image and reads
 * nothing.  Each thread stores four consecutive x of every channel as one 16-byte store; W_out % 4 columns take scalar stores. */
typedef struct GwtfImageArgs {
  const unsigned char* images;       /* [n_images][C][H][W] */
  const int* rows;                   /* [B] or NULL */
  const int* xs;                     /* [W_r], read when resize */
  const float* xf;                   /* [W_r] */
  const int* ys;                     /* [H_r] */
  const float* yf;                   /* [H_r] */
  const float* noise;                /* explicit noise or NULL */
  unsigned long long* state;         /* {seed, call}; required when noise is on and `noise` is NULL */
  float* out;                        /* [B][C_out][H_out][W_out] */
  int B, n_images, C, H, W;
  int H_r, W_r;
  int pad_y, pad_x;
  int resize, grayscale, normalize, add_noise, remove_alpha;
  float gray[3];
  float mean[5], stdev[5];           /* per channel at the normalisation stage */
  float noise_scale;                 /* > 0 when Philox noise is drawn */
  void* stream;
} GwtfImageArgs;
/* GWTF_E_BADARG without a launch: a NULL record or required pointer, B outside 1..65535, C outside {3, 4}, sizes < 1, negative
 * padding, H_r / W_r other than H / W without resize, a stdev <= 0 with normalize, Philox noise without a state or with
 * noise_scale <= 0.  GWTF_E_UNSUPPORTED: source rows too wide for the staging buffer (8 rows with
 * resize, 4 without, of the channels read, W floats each, plus the column table with resize, beyond 64 KiB). */
int gwtf_transform_images(const GwtfImageArgs* args);

/* Train-mode BatchNorm2d fused with what follows it in the image encoder (csrc/gwtf_norm2d.hip; added without a version change, no
 * existing record or signature moved).  Contiguous NCHW float32; batch statistics over N * H * W values per channel: biased variance
 * for the normalisation, eps inside the square root, running_mean / running_var updated in place with `momentum` (the unbiased
 * variance goes into running_var).  xhat = (x - mean) * rstd, and
 *   relu = 0                    y = gamma * xhat + beta
 *   relu = 1                    y = relu(gamma * xhat + beta + residual)     (residual may be NULL)
 *   relu = 1, pool = 1          y = MaxPool2d(3, stride 2, padding 1) of relu(gamma * xhat + beta): y and offsets are
 *                               [N][C][Ho][Wo], Ho = (H - 1) / 2 + 1; offsets holds 3 * dy + dx (0..8) of the first maximum of the
 *                               window in row-major order, padding counting as -inf (torch's rule); no residual
 * Forward: partial sums (float64, a (C, S) grid, S = gwtf_norm2d_partials), a finalising launch that adds them in a fixed order
 * and writes stats = [3][C] {mean, rstd, mean - (float)mean} and the running statistics, the applying launch.  Backward, with
 * dy' = dy * [y > 0] (relu; y the saved output), = dy (no relu), or gathered from the pooled gradient through `offsets` with y
 * recomputed from x by the forward's arithmetic (pool): dgamma = sum dy' * xhat, dbeta = sum dy',
 * dx = gamma * rstd * (dy' - mean(dy') - xhat * mean(dy' * xhat)), d_residual = dy' when asked for.  No atomics: two calls give
 * the same bits.  Any H * W >= 1 and any alignment are taken (16-byte accesses when planes and addresses allow, else 4-byte). */
typedef struct GwtfNorm2dArgs {
  const float* x;                    /* [N][C][H][W] */
  const float* residual;             /* as x, or NULL */
  const float* gamma;                /* [C] */
  const float* beta;                 /* [C]; the backward reads it with pool only */
  float* running_mean;               /* [C], forward; NULL: not updated */
  float* running_var;
  float* y;                          /* forward: the output; backward: the saved output (read when relu and not pool) */
  unsigned char* offsets;            /* [N][C][Ho][Wo] with pool */
  float* stats;                      /* [3][C]: written by the forward, read by the backward */
  double* partials;                  /* [C][S][2] */
  const float* dy;                   /* backward: the gradient of y */
  float* dx;
  float* d_residual;                 /* or NULL */
  float* dgamma;                     /* [C] */
  float* dbeta;                      /* [C] */
  int N, C, H, W;
  int relu, pool;
  float eps, momentum;
  void* stream;
} GwtfNorm2dArgs;
/* All three validate on the host before any launch.  GWTF_E_BADARG: a NULL record or required pointer, a size < 1, N > 65535,
 * N * H * W or C * H * W near 2^31, pool without relu or with a residual, eps < 0, momentum outside [0, 1].  GWTF_E_FEW_VALUES:
 * N * H * W < 2 (torch refuses the same).  gwtf_norm2d_partials returns S (1..64), or 0 for sizes the launches reject. */
int gwtf_norm2d_partials(int N, int C, int H, int W);
int gwtf_norm2d_forward(const GwtfNorm2dArgs* args);
int gwtf_norm2d_backward(const GwtfNorm2dArgs* args);

/* The same layer with batch statistics over the images of SEVERAL ranks (SyncBatchNorm; added without a version change, no existing
 * record or signature moved).  Each direction is split where the statistics become global: *_sums leaves this rank's float64 sums in
 * sums = [C][2] -- the caller adds them up over the ranks -- and *_apply takes the totals and `count`, the number of values per
 * channel over all ranks.  Pass the same record to both calls of a direction.
 *   forward_sums    the partial-sum launch of gwtf_norm2d_forward over this rank's N images, then one thread per channel adds the S
 *                   partials in that call's order: sums[c] = {sum x, sum x * x}.  Nothing else is written.
 *   forward_apply   stats, running_mean and running_var from the totals by gwtf_norm2d_forward's arithmetic (the unbiased variance
 *                   takes the global count), then its applying launch on the local images.
 *   backward_sums   the backward's partial-sum launch, folded: sums[c] = {sum dy', sum dy' * xhat}, and the rank-local dbeta /
 *                   dgamma (the floats of those sums): parameter gradients stay local, as torch's SyncBatchNorm leaves them.
 *   backward_apply  dx = gamma * rstd * (dy' - sums[c][0] / count - xhat * sums[c][1] / count) and d_residual = dy' by
 *                   gwtf_norm2d_backward's applying launch; the first 2 * C floats of `partials` are overwritten (the totals as floats,
 *                   which that launch reads in place of dbeta / dgamma; those two are not touched).
 * One rank, count = N * H * W: the bits of gwtf_norm2d_forward / _backward.  Validation as there, on the host before any launch, except
 * that a local N * H * W of 1 is taken; further GWTF_E_BADARG: sums NULL, count < N * H * W; GWTF_E_FEW_VALUES: count < 2.  *_sums read
 * no y (forward), beta (unless pool) or running statistics; backward_apply needs no dgamma / dbeta. */
int gwtf_norm2d_forward_sums(const GwtfNorm2dArgs* args, double* sums);
int gwtf_norm2d_forward_apply(const GwtfNorm2dArgs* args, const double* sums, double count);
int gwtf_norm2d_backward_sums(const GwtfNorm2dArgs* args, double* sums);
int gwtf_norm2d_backward_apply(const GwtfNorm2dArgs* args, const double* sums, double count);

/* The convolutions of the image encoder in train mode, all three passes (csrc/gwtf_conv2d.hip; added without a version change, no
 * existing record or signature moved).  Bias-free, dilation 1, groups 1, contiguous NCHW float32, w in torch's parameter layout:
 *   forward          y[n][co][oy][ox]  = sum over (ci, ky, kx) of x[n][ci][oy * stride - pad + ky][ox * stride - pad + kx] * w[co][ci][ky][kx]
 *   backward_input   dx[n][ci][iy][ix] = sum over (co, ky, kx) of dy[n][co][oy][ox] * w[co][ci][ky][kx] where that output position
 *                    exists (gather form).  EVERY element of dx is written, the zeros at positions no output reads included; `work`
 *                    receives w transposed to [Cin][Cout][k][k] first.
 *   backward_weight  dw[co][ci][ky][kx] = sum over (n, oy, ox) of dy * x.  The pixels are split into `splits` ranges; with more than
 *                    one, each writes a partial dw to `work` and a second launch adds them in the order 0 .. splits-1.
 * Products are exact fp32 (v_mfma_f32_16x16x4_f32); a contraction runs as four independent chains combined pairwise.  No atomics:
 * two calls give the same bits.  Ho = (H + 2 * pad - k) / stride + 1, Wo likewise.
 * Accepted: k in {1, 3, 7}, stride in {1, 2}, pad = k / 2, Cout a multiple of 16, Cin a multiple of 16 or Cin = 4 with k = 7 (the
 * stem); any N >= 1, H >= 1, W >= 1.  Everything else: GWTF_E_UNSUPPORTED. */
#define GWTF_CONV2D_FORWARD 0
#define GWTF_CONV2D_BACKWARD_INPUT 1
#define GWTF_CONV2D_BACKWARD_WEIGHT 2
typedef struct GwtfConv2dArgs {
  const float* x;                    /* [N][Cin][H][W]: forward, backward_weight */
  const float* w;                    /* [Cout][Cin][k][k]: forward, backward_input; 16-byte aligned */
  float* y;                          /* [N][Cout][Ho][Wo]: forward */
  const float* dy;                   /* as y: both backward passes */
  float* dx;                         /* as x: backward_input */
  float* dw;                         /* as w: backward_weight */
  float* work;                       /* the planner's work_floats for the pass (16-byte aligned); may be NULL when that is 0 */
  int N, Cin, H, W, Cout, k, stride, pad;
  void* stream;
} GwtfConv2dArgs;
/* All validate on the host before any launch.  GWTF_E_BADARG: a NULL record, a NULL or misaligned pointer among those the pass uses,
 * a size < 1, N > 65535, an element count of x, y or w near 2^31, an unknown pass.  The planner launches nothing and reads no
 * pointer of the record: it returns the status the pass would give a record with its pointers set, and on success the number of
 * splits (1 for forward and backward_input) and the floats of `work` the pass needs (0: none); either output may be NULL. */
int gwtf_conv2d_plan(const GwtfConv2dArgs* args, int pass, int* splits, size_t* work_floats);
int gwtf_conv2d_forward(const GwtfConv2dArgs* args);
int gwtf_conv2d_backward_input(const GwtfConv2dArgs* args);
int gwtf_conv2d_backward_weight(const GwtfConv2dArgs* args);

/* Occupancy histogram and Jensen-Shannon divergence of the generation evaluation (csrc/gwtf_occupancy.hip; added without a version
 * change, no existing record or signature moved): get_voxel_occ_dist and JSD of lib/networks/utils.py:45-86 without the copy of both
 * cloud sets to the host.
 * Binning rule, the reference's (utils.py:56-75), exactly: coordinate x (float32, widened to double) falls in bin k iff
 * edges[k] <= x < edges[k + 1], compared in double; a point counts iff all three of its coordinates have a bin, and then adds one to
 * counts[(kx * res + ky) * res + kz].  NaN, +-inf, x >= edges[res] and x < edges[0] have no bin.  The caller fills `edges` with the
 * reference's table, -0.5 + arange(res + 1) * (1. / res) in float64: the table is the only statement of where a bin ends (a floor of
 * (x + 0.5) * res is NOT the rule: most edges are no float32 value, and the float32 neighbours of an edge fall on the other side).
 * stats counts VALUES, not points: stats[0] += #{|x| > bound} (NaN is not; +-inf is), stats[1] += #{NaN}: what the reference turns
 * into its two warnings.  counts and stats are ADDED TO, never cleared: a set may be folded in call by call.  Integer atomics only:
 * repeated calls give identical bits.  One persistent grid, one workgroup per 8192 points and one per CU at most, each with a private
 * uint32 histogram of res^3 bins in LDS (131,072 B at res 32): the launcher raises the kernel's dynamic-LDS limit once per device and
 * process -- the one piece of state this library keeps, it changes no result -- and returns GWTF_E_UNSUPPORTED without a launch when
 * the runtime refuses that. */
typedef struct GwtfOccupancyArgs {
  const float* points;               /* [n_points][3], row-contiguous */
  size_t n_points;
  int res;                           /* 1..32 */
  double edges[33];                  /* edges[0..res], strictly increasing */
  float bound;
  long long* counts;                 /* [res][res][res], added to */
  long long* stats;                  /* [2] {values beyond bound, NaN values}, added to; or NULL */
  void* stream;
} GwtfOccupancyArgs;
/* GWTF_E_BADARG without a launch: a NULL record, points or counts, n_points outside 1..2^32-1, res outside 1..32, a bound that is
 * negative or NaN, edges[0..res] not strictly increasing. */
int gwtf_voxel_occupancy(const GwtfOccupancyArgs* args);
/* out[0] = H((p1 + p2) / 2) - (H(p1) + H(p2)) / 2 in bits (base 2), p = counts / sum(counts), H(p) = -sum p log2 p with a zero bin
 * contributing zero (scipy.stats.entropy): one workgroup, float64 throughout, a fixed summation order.  A histogram whose sum is 0
 * gives NaN, which is what the reference's 0 / 0 turns into.  GWTF_E_BADARG: a NULL pointer, bins < 1. */
int gwtf_jsd_counts(const long long* c1, const long long* c2, int bins, double* out, void* stream);

/* Paired evaluation of the autoencoding and reconstruction branches (csrc/gwtf_metrics.hip; added without a version change, no
 * existing record or signature moved): the rescaling chain of lib/networks/evaluating.py:100-120 fused with the layout change its
 * metrics need, cloud i against cloud i in one Chamfer launch, and the per-pair values and running sums in one small launch.
 *
 * The frame.  gen [B][3][n] and ref [B][3][m] channel-major (what the model and the loaders produce) -> gen_out [B][n][3] and ref_out
 * [B][m][3] point-major (what every metric kernel takes); one launch for both.  Every value goes through the reference's in-place
 * statements in the reference's order, each rounded on its own as torch rounds it:
 *   n_scale times   x = x * scale                       float32              (:103 and :107: one per evaluation flag that is on)
 *   translate       x = float(double(x) + shift[c])     ONE rounding          (:111-113: the shift is a float64 tensor, torch adds in
 *                                                                              float64 and rounds the sum to float32)
 *   row_scale       x = x * orig_s[b]                   float32              (:116)
 *   row_shift       x = x + orig_c[b][c]                float32              (:119)
 * With every flag off the launch is a pure layout change; NaN and inf pass through like any other value. */
typedef struct GwtfEvalFrameArgs {
  const float* gen;                  /* [B][3][n] */
  const float* ref;                  /* [B][3][m] */
  const float* orig_s;               /* [B], read when row_scale */
  const float* orig_c;               /* [B][3], read when row_shift */
  float* gen_out;                    /* [B][n][3] */
  float* ref_out;                    /* [B][m][3] */
  int B, n, m;
  int n_scale;                       /* 0..2 multiplications by `scale` */
  int translate, row_scale, row_shift;
  float scale;
  double shift[3];
  void* stream;
} GwtfEvalFrameArgs;
/* GWTF_E_BADARG without a launch: a NULL record, a NULL cloud pointer, B outside 1..65535, n or m < 1, n_scale outside 0..2,
 * row_scale with a NULL orig_s, row_shift with a NULL orig_c. */
int gwtf_eval_frame(const GwtfEvalFrameArgs* args);
/* Chunks per (direction, pair) the partial buffer of gwtf_chamfer_paired is laid out for: ceil(max(n, m) / 512); 0 for sizes < 1. */
int gwtf_chamfer_paired_partials(int n, int m);
/* Cloud i of a [B][n][3] against cloud i of b [B][m][3], both directions in one launch, grid (query chunks, B, 2).  Direction 0: the
 * points of a against b; direction 1: the points of b against a.  The per-point minimum is dist1 / dist2 of gwtf_nn_distance bit for
 * bit.  Every workgroup writes ONE partial of 9 words at partials[((d * B + i) * P + chunk) * 9], P = gwtf_chamfer_paired_partials(n, m):
 * word 0 the float32 sum of its chunk's minima, words 1..8 int32 counts of minima < thr[h], compared in float32 (thr: HOST array of
 * n_thr <= 8 values read during the call, NULL allowed when n_thr == 0).  The chunk is 2048 query points when that fills the device
 * and 512 otherwise, a function of (B, n, m) alone that gwtf_paired_finalise repeats; the order of every sum is fixed -- lane, wave
 * shuffle tree, waves in order -- and nothing is accumulated across workgroups: the same call gives the same bits.
 * GWTF_E_BADARG without a launch: a NULL pointer, B outside 1..65535, n or m < 1, n_thr outside 0..8. */
int gwtf_chamfer_paired(const float* a, const float* b, float* partials, const float* thr, int n_thr, int B, int n, int m,
                        void* stream);
/* The per-pair values from the partials of gwtf_chamfer_paired on the same (B, n, m, n_thr), in float32 and in the reference's
 * expressions; one wave, one thread per pair adding that pair's partials in chunk order.  Every output pointer may be NULL:
 *   cdl[i] = sum_l / n, cdr[i] = sum_r / m, cd[i] = cdl + cdr                                  (evaluation_metrics.py:73-78)
 *   f1[h][i] = 2 P R / (P + R + 1e-7), R = 100 (cnt_l[h] / n), P = 100 (cnt_r[h] / m)          (utils.py:38-42)
 *   emd[i] = emd_cost[i] * float(1 / double(n))   -- what `match_cost(...) / float(n)` evaluates to on the device (the division by a
 *            host scalar is carried out as a multiplication by its reciprocal); emd_cost: the [B] output of gwtf_emd_cost, or NULL
 * meter (or NULL): float64 running sums ON THE DEVICE, added to and never cleared: meter[3 + h] += sum_i f1[h][i] for h < n_thr, and
 * when meter_head is non-zero meter[0] += B, meter[1] += sum_i cd[i] (when cd is given), meter[2] += sum_i emd[i] (when emd_cost is
 * given).  The float32 per-pair values are widened and added in float64: every lane its pairs in pair order, then a shuffle tree.
 * GWTF_E_BADARG without a launch: NULL partials, B outside 1..65535, n or m < 1, n_thr outside 0..8, f1 NULL with n_thr > 0 and no
 * meter, emd given without emd_cost. */
int gwtf_paired_finalise(const float* partials, const float* emd_cost, float* cd, float* cdl, float* cdr, float* emd, float* f1,
                         double* meter, int meter_head, int n_thr, int B, int n, int m, void* stream);

/* Per-point component posteriors of observed clouds (csrc/gwtf_assign.hip; added without a version change, no existing record or
 * signature moved): the inference direction of the mixture.  Inputs are exactly what gwtf_mixture_nll reads, and per shape b, point n,
 * component k the same quantity in the same float32 expression (lib/networks/losses.py:101-122, its log(exp(logit)) - logsumexp weight
 * included):
 *   lp_k = -0.5 * sum_d [ lv0 + logdet + (z - mu0)^2 / exp(lv0) ] - 1.5 * log(2 pi) + log w_bk
 *   log_density = logsumexp_k lp_k                 (what point_lse of gwtf_mixture_nll holds)
 *   labels      = argmax_k lp_k in [0, K), the LOWEST k on an exact tie; -1 (invalid) when log_density is not finite: a NaN anywhere in
 *                 the point's lp_k (log_density is then NaN), every component at -inf (log_density -inf), an lp of +inf
 *   confidence  = exp(lp_label - log_density), 0 where the label is -1
 *   resp[k]     = exp(lp_k - log_density), NaN in every k where the label is -1; resp of the label equals confidence bit for bit.
 *                 With resp NULL z and logdet are read exactly once, with it twice
 *   counts      = points per (shape, component), invalid = points labelled -1 per shape: WRITTEN by the call (cleared on the stream,
 *                 then added to with integer atomics)
 *   table       = the contingency of (label, part) over every point with a label >= 0 and a part in [0, P), ADDED TO and never cleared
 *                 (a set is folded in batch by batch, as counts of gwtf_voxel_occupancy is); skipped += the points left out
 * Integer atomics only, no float atomic anywhere: the same inputs give the same bits in every output on every call.  16-byte loads when
 * N is a multiple of 4 and z, logdet, parts and the per-point outputs are 16-byte aligned, float by float otherwise -- the same
 * arithmetic per point, hence the same bits.  Everything is enqueued on `stream`; no allocation, no synchronisation. */
typedef struct GwtfAssignArgs {
  const float* z;                    /* [K][B][3][N] */
  const float* logdet;               /* [K][B][3][N] */
  const float* mu0;                  /* [K][B][3] */
  const float* lv0;                  /* [K][B][3] */
  const float* logits;               /* [B][K] */
  const int* parts;                  /* [B][N] ground-truth part of every point, or NULL */
  float* log_density;                /* [B][N] */
  int* labels;                       /* [B][N]; int32 is what labels_in of GwtfRouteArgs takes */
  float* confidence;                 /* [B][N], or NULL */
  float* resp;                       /* [B][K][N], or NULL */
  int* counts;                       /* [B][K], written; or NULL */
  int* invalid;                      /* [B], written; or NULL */
  long long* table;                  /* [K][P], added to; read only with parts */
  long long* skipped;                /* [1], added to; or NULL; read only with parts */
  int K, B, N;
  int P;                             /* 1..64 with parts */
  void* stream;
} GwtfAssignArgs;
/* GWTF_E_BADARG without a launch: a NULL record or required pointer (the five inputs, log_density, labels), K outside 1..64, B or N
 * below 1, with parts a P outside 1..64 or a NULL table.  GWTF_E_UNSUPPORTED: B * ceil(N / 512) beyond an int. */
int gwtf_mixture_assign(const GwtfAssignArgs* args);

/* Labelled point clouds drawn into the cells of a contact sheet (csrc/gwtf_render.hip; added without a version change, no existing
 * record or signature moved): B clouds, one cell of H x W pixels each, opaque depth-tested discs coloured by label.  Every step is
 * integer arithmetic behind a float32 projection whose roundings are fixed, so that a restatement reproduces every output bit:
 *   projection  row r of the image's view M (view + b * view_stride): t_r = ((M[r][0]*x + M[r][1]*y) + M[r][2]*z) + M[r][3], every
 *               product and sum rounded to float32 on its own (no fused multiply-add).  u = t_0, v = t_1 in pixels of the cell: pixel
 *               (i, j) covers [j, j+1) x [i, i+1), row 0 at the top.  d = t_2 + 0.0f (so -0 is +0); a smaller d is nearer
 *   rejected    a point with a non-finite u, v or d draws nothing and is counted in skipped[b]; a point whose disc cannot touch the
 *               cell draws nothing and is not counted (told in float32, before any conversion to an integer)
 *   footprint   U = (int)floorf(u * 16.0f), V likewise.  Pixel (V >> 4, U >> 4) is always covered; pixel (i, j) is also covered when
 *               (16 j + 8 - U)^2 + (16 i + 8 - V)^2 <= radius_q^2.  The depth is flat over the disc
 *   winner      per pixel the smallest 64-bit key (ord(d) << 32) | n, ord the order-preserving map of float32 bits to uint32 (all bits
 *               of a negative value flipped, the sign bit of a non-negative one): the nearest point, the lowest n on equal depth
 *   colour      l = labels[b][n] - label_base: invalid_rgb when l < 0, else palette[l % P]; palette[0] with labels NULL.  Depth cue:
 *               f = floorf(((d - near) * inv_range) * 256.0f) (unfused), q = 0 for f <= 0 or NaN, 255 for f >= 255, else (int)f;
 *               w = 256 - ((fog * q) >> 8); every channel is (c * w) >> 8 -- unchanged with fog = 0
 *   cell        image b goes to cell c = cell0 + b * cell_step of the sheet, origin ((c / cols) * H, (c % cols) * W)
 *   rgb         EVERY pixel of the B cells is written (background_rgb where nothing was drawn): no clear is needed.  Pixels of the
 *               sheet outside these cells are not touched
 *   index       the winning n, -1 for background;  depth: its d, +inf for background;  skipped: WRITTEN by the call
 * One launch, no scratch buffer, no global atomic, no float atomic: the same inputs give the same bits on every call.  Everything is
 * enqueued on `stream`; no allocation, no synchronisation. */
typedef struct GwtfRenderArgs {
  const float* clouds;               /* [B][3][N] */
  const int* labels;                 /* [B][N], or NULL */
  const unsigned char* palette;      /* [P][3] */
  const float* view;                 /* [B][3][4] (view_stride 12) or [3][4] (view_stride 0) */
  unsigned char* rgb;                /* [3][sheet_h][sheet_w] */
  int* index;                        /* [B][H][W], or NULL */
  float* depth;                      /* [B][H][W], or NULL */
  int* skipped;                      /* [B], written; or NULL */
  int B, N, P;
  int label_base;                    /* 1 for the generators' labels, 0 for those of gwtf_mixture_assign */
  int view_stride;                   /* 0 or 12 floats */
  int H, W;                          /* the cell */
  int radius_q;                      /* disc radius in 1/16 pixel, 0..1024 */
  int fog;                           /* 0..256 */
  int sheet_h, sheet_w, cols, cell0, cell_step;
  float near, inv_range;
  unsigned char invalid_rgb[3], background_rgb[3];
  void* stream;
} GwtfRenderArgs;
/* GWTF_E_BADARG without a launch: a NULL record or required pointer (clouds, palette, view, rgb), B, N, H or W below 1, P outside
 * 1..256, view_stride not 0 or 12, radius_q outside 0..1024, fog outside 0..256, cols below 1, a cell that does not lie inside the
 * sheet (cell0 or cell_step negative included), cell_step 0 with B above 1 (two images in one cell).  GWTF_E_UNSUPPORTED: H or W
 * above 2^20, B * ceil(H / 64) * ceil(W / 64) beyond an int. */
int gwtf_render_splats(const GwtfRenderArgs* args);

#ifdef __cplusplus
}
#endif
#endif /* GWTF_H */
