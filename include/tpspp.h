/*
 * tpspp.h -- C ABI of libtpspp_hip.so: the TPS++ rectification hot path on MI355X (gfx950).
 *
 * This is the drop-in boundary.  The reference has no native code and no FFI:
 * its "operator API" for this path is a handful of PyTorch calls inside two nn.Modules.  Each entry
 * point below replaces the call sites cited next to it (paths relative to the reference tree,
 * mmocr/models/textrecog/...); tps_pp_amd/ binds them with ctypes and INTEGRATION.md shows the
 * few lines a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to densely packed row-major fp32 (int32 for indices); tensors
 *     are NCHW like the reference's.  No allocation (one exception: tpspp_warp_plan_create's small host
 *     structure, freed by tpspp_warp_plan_destroy), no ownership transfer, no host synchronisation:
 *     work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default stream) and
 *     the call returns immediately.  Re-entrant per stream.
 *   - return value: 0 on success, a negative TPSPP_E* code otherwise; tpspp_last_error() returns a
 *     thread-local human-readable message for the last failure on the calling thread.
 *   - arithmetic contract (what makes the result equal the reference's, not merely close):
 *       T-solve and grid:  zero-initialised, k-ascending fp32 FMA chains -- bit-identical to the
 *                          reference's torch.bmm on the CPU;
 *       sampler:           ATen bilinear / border / align_corners=True with the CPU kernel's weight
 *                          form and FMA order -- bit-identical to F.grid_sample on the CPU.
 */
#ifndef TPSPP_H_
#define TPSPP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPSPP_ABI_VERSION 12  /* 2 (round 4): tpspp_warp_bwd and tpspp_nrtr_decoder_fwd carry the sizes of their workspace / pointer table;
                               3: tpspp_down_fused_bf16_fwd / _x3_fwd / _f32_fwd, tpspp_token_gemm_bf16_fwd, tpspp_front_fwd and tpspp_front_bf16_fwd takes feat0 = feat1 = NULL;
                               4 (round 6): tpspp_nrtr_decoder_fwd takes status_out, tpspp_resize_normalize_fwd takes interpolation;
                               5 (round 6): tpspp_warp_plan_create / _run / _run_on / _destroy;
                               6: tpspp_conv2d_bwd_data / _bwd_weight / _bwd_weight_workspace_floats, tpspp_conv2d_prep_weight;
                               7: the regressor's training kernels: tpspp_mm_f32, tpspp_linear_bwd_weight (+ _workspace_floats),
                                  tpspp_act_bwd, tpspp_plane_ln_fwd / _bwd (+ _workspace_floats), tpspp_dgab_pool_fwd / _bwd,
                                  tpspp_dgab_gate_fwd / _bwd, tpspp_cbam_train_fwd, tpspp_cbam_bwd (+ _workspace_floats);
                               8: the backbone's BatchNorm training kernels: tpspp_bn_train_stats (+ _workspace_floats as
                                  tpspp_bn_stats_workspace_floats), tpspp_bn_eval_stats, tpspp_bn_apply_fwd, tpspp_bn_bwd_reduce
                                  (+ _workspace_floats), tpspp_bn_bwd_data;
                               9: the encoder's attention training kernels, declared in tpspp_train_attn.h: tpspp_attn_train_fwd,
                                  tpspp_attn_train_bwd, tpspp_attn_dropout_mask;
                               10: the decoder's and the loss's training kernels, declared in tpspp_train_dec.h:
                                  tpspp_attn_train_fwd_ex / _bwd_ex, tpspp_embed_pos_fwd, tpspp_embed_bwd (+ _workspace_floats),
                                  tpspp_seq_ce_fwd / _bwd;
                               11: the train pipeline's augmentation kernel, declared in tpspp_augment.h:
                                  tpspp_augment_normalize_fwd;
                               12: no new entry point: tpspp_warp_fwd / tpspp_warp_plan_* accept TPSPP_IO_BF16 on a classic
                                  call with the prepared table (bf16 images in and out on the in-place kernel);
                               (still 12): the CRNN recogniser's entry points, declared in tpspp_crnn.h, tpspp_crnn_train.h and
                                  tpspp_crnn_bf16.h, are bound by name; they change nothing declared here;
                               (still 12): the classic rectifier's training kernels tpspp_bn_pool2x2_fwd / _bwd_reduce
                                  (+ _workspace_floats) / _bwd_data and tpspp_global_avgpool_bwd, bound by name;
                               (still 12): the CRNN decoder's reduced-precision kernels tpspp_crnn_lstm_bf16_fwd and tpspp_mm_bf16,
                                  bound by name;
                               (still 12): their training counterparts tpspp_crnn_lstm_bf16_train_fwd, tpspp_crnn_lstm_bf16_bwd and
                                  tpspp_linear_bwd_weight_bf16 (+ _workspace_floats), bound by name;
                               (still 12): the VGG's training kernel tpspp_crnn_maxpool_bwd, bound by name */

#define TPSPP_OK        0
#define TPSPP_EINVAL  (-22)  /* bad argument (null pointer, non-positive size, unsupported shape) */
#define TPSPP_ENODEV  (-19)  /* no HIP device / wrong architecture */
#define TPSPP_EIO      (-5)  /* the HIP runtime reported a launch error */

typedef void* tpspp_stream_t; /* hipStream_t */

/* ABI version of the loaded library (== TPSPP_ABI_VERSION it was built with). */
int tpspp_abi_version(void);

/* Message for the last non-zero return on this thread ("" if none). */
const char* tpspp_last_error(void);

/*
 * T[b] = inv_delta_c (F+3 x F+3) @ [ctrl[b] (F x 2); 0 (3 x 2)]          -> T (N, F+3, 2)
 * replaces: torch.bmm(batch_inv_delta_C, batch_C_prime_with_zeros)
 *           preprocessor/tps_preprocessor.py:273-280, backbones/tps_pp/tps_pp.py:484,489-494
 */
int tpspp_solve_T(const float* inv_delta_c, const float* ctrl, int N, int F, float* T,
                  tpspp_stream_t stream);

/*
 * grid[b,p,:] = [1, P.x, P.y, m_0..m_{F-1}] @ T[b]                         -> grid (N, n, 2)
 *   p_xy == NULL: p_hat is (n, F+3), leading dimension p_hat_ld, rows [1, P.x, P.y, rbf_0..]
 *                 (GridGenerator.P_hat, tps_preprocessor.py:255-268)
 *   p_xy != NULL: p_hat is (n, F) rbf only (Attention_Enhanced_TPS.P_hat) and p_xy is (n, 2)
 *   score (N, n, F) or NULL: m_k = rbf_k * (score_k * 0.5 + 1)   (tps_pp.py:474, thela = 0.5)
 * replaces: torch.bmm(batch_P_hat, batch_T)   tps_preprocessor.py:281, tps_pp.py:467-479,495
 */
int tpspp_build_grid(const float* p_hat, int p_hat_ld, const float* p_xy, const float* score,
                     const float* T, int N, int n, int F, float* grid, tpspp_stream_t stream);

/*
 * out = grid_sample(in, grid, mode='bilinear', padding_mode='border', align_corners=True)
 *   in (N,C,H,W), grid (N,Ho,Wo,2) -> out (N,C,Ho,Wo); idx_or_null (N,Ho*Wo,2) int32 receives the
 *   north-west corner (ix_nw, iy_nw) of every output pixel.
 * replaces: F.grid_sample   tps_preprocessor.py:79-83, tps_pp.py:606-615
 */
int tpspp_grid_sample(const float* in, const float* grid, int N, int C, int H, int W, int Ho,
                      int Wo, float* out, int32_t* idx_or_null, tpspp_stream_t stream);

/*
 * p_hat_t[c, p] = p_hat[p, c]: the batch-shared RBF table transposed to (cols, n) so that a wavefront
 * whose lanes own consecutive output pixels reads it fully coalesced.  One-off preparation (the
 * table is a module buffer); cols = F+3 (classic layout) or F (TPS_PP layout).
 */
int tpspp_transpose_p_hat(const float* p_hat, int p_hat_ld, int n, int cols, float* p_hat_t,
                          tpspp_stream_t stream);

/*
 * Does the HOST copy of a classic-layout table (n = Ho*Wo rows of [1, P.x, P.y, rbf_0..rbf_{F-1}])
 * have the exact (bitwise) 4-fold mirror symmetry of the reference's constants?  Returns 1 / 0.
 * When 1, pass TPSPP_TABLE_MIRROR4 to tpspp_warp_fwd: one table row then serves four output pixels.
 * (GridGenerator's table always has it: fiducials on the top/bottom edges at mirrored abscissae,
 * tps_preprocessor.py:197-211, pixel centres mirrored about the image centre, :242-253.)
 */
int tpspp_table_mirror_symmetry(const float* p_hat_host, int p_hat_ld, int Ho, int Wo, int F);

/*
 * The prepared form of a mirror-symmetric classic table that the image-pair and in-place kernels read: the (F+3, n)
 * transposed table of tpspp_transpose_p_hat followed by a packed copy in those kernels' thread order (a thread's F+3
 * values per quadrant pixel as 16-byte pieces, [wavefront][quadrant pixels per thread][(F+3+3)/4][lane][4]; thread ->
 * pixel: a half-wavefront owns a block of 32 pixels -- 4 columns x 8 rows, 8 x 4 or 32 x 1 by the row pitch -- of the left
 * half of the upper half-image, a thread 1 - 4 such row groups depending on the geometry); for the large geometries (more
 * than two row groups per thread in that copy) a third section follows: the same packing with ONE row group per thread,
 * read by the span-staging kernel (tpspp_warp_span.h).  tpspp_prepared_table_floats:
 * buffer size in floats, 0 when the geometry has no prepared form (needs Ho % 16 == 0, Wo % 4 == 0).  One-off
 * preparation, like the transposition.  Pass the buffer
 * as p_hat_t together with TPSPP_TABLE_PACKED | TPSPP_TABLE_SPAN (and TPSPP_TABLE_MIRROR4 once the symmetry has been verified).
 * The buffer's size grew in round 5 (the third section): size it with THIS function, never with a remembered formula.
 * replaces nothing in the reference (its table is a module buffer, tps_preprocessor.py:187-188); see tpspp_warp_fwd.
 */
size_t tpspp_prepared_table_floats(int Ho, int Wo, int F);
int tpspp_prepare_mirror_table(const float* p_hat, int p_hat_ld, int Ho, int Wo, int F, float* prepared,
                               tpspp_stream_t stream);

#define TPSPP_TABLE_MIRROR4 1      /* table_flags bit: symmetry verified by the caller */
#define TPSPP_TABLE_PACKED 8       /* table_flags bit: p_hat_t is a tpspp_prepare_mirror_table buffer (the packed copy
                                      follows the transposed table).  Never changes results. */
#define TPSPP_TABLE_SPAN 32        /* table_flags bit, with TPSPP_TABLE_PACKED: the buffer was sized by THIS library's
                                      tpspp_prepared_table_floats and filled by its tpspp_prepare_mirror_table, i.e. it carries the
                                      third section (round 5) that the span-staging kernel of the large geometries reads.  A
                                      caller still holding a two-section buffer of an earlier build omits the bit and gets the
                                      kernels that do not read behind the second section.  Never changes results. */
#define TPSPP_SCORE_TRANSPOSED 2   /* table_flags bit: `score` is laid out (N, F, n) instead of the
                                      reference's (N, n, F): lanes that own consecutive pixels then read
                                      it coalesced.  Same values, same results. */
#define TPSPP_BWD_FIXED_POINT 16   /* table_flags bit of tpspp_warp_bwd only: accumulate dL/d input in 64-bit fixed point (bitwise
                                    * reproducible from run to run) instead of the default fp64 LDS atomics; per call, any stream */
#define TPSPP_BWD_TWO_KERNELS 64   /* table_flags bit of tpspp_warp_bwd only: never the one-launch form of the classic rectifier's call
                                    * (A/B runs, tests); per call. */
#define TPSPP_IO_BF16 4            /* table_flags bit: in0 / in1 / out0 / out1 hold bfloat16 (the pointers are
                                      reinterpreted; everything else stays fp32).  The bf16 configuration
                                      (BASELINE.json configs[2]): T, grid and interpolation in fp32 exactly as
                                      without the flag, one round-to-nearest-even at the store.  Accepted for
                                      (a) a classic call with the prepared table: one input, no score / p_xy,
                                      H0 == Ho, W0 == Wo, C0 in {1, 3}, F = 20, p_hat_t from
                                      tpspp_prepare_mirror_table with TPSPP_TABLE_MIRROR4 | TPSPP_TABLE_PACKED,
                                      in0 / out0 16-byte aligned, a bf16 image that fits the LDS (every geometry
                                      with a prepared table up to 64x256x3); grid_or_null / idx_or_null keep the
                                      bits they have without the flag;
                                      (b) shapes the plane-streaming kernel takes (TPS_PP geometry).
                                      Anything else: TPSPP_EINVAL, and tpspp_last_error names the condition that
                                      is not met (a classic call without p_hat_t, without the two table bits or
                                      without mirror symmetry included).  tpspp_warp_set_tuning's kernel_choice /
                                      bands are not consulted when the bit is set.
                                      tpspp_warp_bwd honours the bit too: g_out0 / g_out1 / in0 / in1 / g_in0 / g_in1
                                      hold bfloat16; grid, T, the tables, score, g_ctrl, g_score, the workspace and
                                      all accumulation stay as without it.  Served and refused forms: see
                                      tpspp_warp_bwd. */

/*
 * The fused hot path: T-solve -> grid -> bilinear warp of in0 (and in1 when non-NULL) in ONE kernel;
 * T lives in LDS and the grid in registers, neither touches HBM unless grid_or_null is given.
 *   in0 (N,C0,H0,W0) -> out0 (N,C0,Ho,Wo);  in1 (N,C1,H1,W1) -> out1 (N,C1,Ho,Wo)  [optional]
 *   ctrl (N,F,2); score (N,Ho*Wo,F) or NULL; inv_delta_c (F+3,F+3); p_hat / p_hat_ld / p_xy as in
 *   tpspp_build_grid; p_hat_t_or_null = tpspp_transpose_p_hat(p_hat) (same values, enables the
 *   coalesced / LDS-staged fast kernels; NULL selects the generic kernel -- identical results);
 *   table_flags: OR of TPSPP_TABLE_MIRROR4, TPSPP_TABLE_PACKED, TPSPP_TABLE_SPAN (only meaningful with p_hat_t),
 *   TPSPP_SCORE_TRANSPOSED (none of them changes results) and TPSPP_IO_BF16 (bf16 images in and out);
 *   with TPSPP_IO_BF16 the classic rectifier (prepared table required) and the TPS_PP geometry are served, see the bit;
 *   grid_or_null (N,Ho*Wo,2); idx_or_null (N,Ho*Wo,2) int32 = NW corner in in0.
 * replaces: GridGenerator.build_P_prime + F.grid_sample   tps_preprocessor.py:71-83
 *           Attention_Enhanced_TPS.build_P_prime + 2x F.grid_sample   tps_pp.py:597-615
 */
int tpspp_warp_fwd(const float* in0, int C0, int H0, int W0,
                   const float* in1, int C1, int H1, int W1,
                   const float* ctrl, const float* score,
                   const float* inv_delta_c, const float* p_hat, int p_hat_ld, const float* p_xy,
                   const float* p_hat_t_or_null, int table_flags, int N, int F, int Ho, int Wo,
                   float* out0, float* out1, float* grid_or_null, int32_t* idx_or_null,
                   tpspp_stream_t stream);

/*
 * Prepared calls of tpspp_warp_fwd (round 6; ABI 5).  A caller that rectifies batch after batch into the same buffers -- a
 * serving loop, bench.py -- hands the 25 arguments over ONCE: tpspp_warp_plan_run(plan) is tpspp_warp_fwd with the stored
 * arguments (same checks, same dispatch, same kernel, same results), tpspp_warp_plan_run_on the same on another stream.  What it
 * saves is the caller's foreign-function marshalling per launch (ctypes: 1.6 of ~4.3 us), which matters when the device needs
 * ~8 us per batch and, at the start of a burst, waits for the host.  The plan holds POINTERS, not copies: the buffers must
 * outlive it.  tpspp_warp_plan_create allocates a small host structure (the only entry point that allocates);
 * tpspp_warp_plan_destroy(NULL) is a no-op.  Thread safety: a plan is immutable after creation.
 * replaces: the same call sites as tpspp_warp_fwd (tps_preprocessor.py:71-83, tps_pp.py:597-615).
 */
typedef struct tpspp_warp_plan tpspp_warp_plan_t;
int tpspp_warp_plan_create(const float* in0, int C0, int H0, int W0,
                           const float* in1, int C1, int H1, int W1,
                           const float* ctrl, const float* score,
                           const float* inv_delta_c, const float* p_hat, int p_hat_ld, const float* p_xy,
                           const float* p_hat_t_or_null, int table_flags, int N, int F, int Ho, int Wo,
                           float* out0, float* out1, float* grid_or_null, int32_t* idx_or_null,
                           tpspp_stream_t stream, tpspp_warp_plan_t** plan_out);
int tpspp_warp_plan_run(const tpspp_warp_plan_t* plan);
int tpspp_warp_plan_run_on(const tpspp_warp_plan_t* plan, tpspp_stream_t stream);
void tpspp_warp_plan_destroy(tpspp_warp_plan_t* plan);

/*
 * Backward of tpspp_warp_fwd: given dL/d out0 [, dL/d out1] returns
 *   g_in0 (N, C0, H0, W0), g_in1 (N, C1, H1, W1)  dL/d input (zeroed here, then accumulated with float
 *                                                  atomics); either may be NULL (not wanted)
 *   g_ctrl (N, F, 2)                                dL/d control points
 *   g_score                                         dL/d score in the layout of `score` ((N, n, F), or
 *                                                  (N, F, n) with TPSPP_SCORE_TRANSPOSED), or NULL
 *   g_grid_ws, g_grid_ws_floats                     scratch and its size in floats, at least
 *                                                  tpspp_warp_bwd_workspace_floats(N, Ho, Wo) (checked: TPSPP_EINVAL
 *                                                  otherwise; the size grew in round 3); on return its first
 *                                                  N * Ho*Wo * 2 floats hold dL/d grid
 * grid (N, Ho*Wo, 2) is the sampling grid the forward produced (its grid_or_null output) and
 * T (N, F+3, 2) = tpspp_solve_T(inv_delta_c, ctrl) (only dL/d score reads it: may be NULL when score is NULL); the tables
 * are the forward's.  Gradients follow
 * ATen's CPU grid_sampler_2d_backward (bilinear, border, align_corners=True: zero coordinate gradient
 * where the coordinate was clamped) and the transposes of the two products of build_P_prime.
 * The classic rectifier's call (one input of <= 3 channels, no score, transposed table given, 1024 < Ho*Wo <= 4096, the
 * fp64 accumulator) is ONE launch; every other call a sampling + a parameter kernel.  Same sampling arithmetic either way;
 * dL/d control points of the one-launch form sums 8-term fp32 chains in fp64 (the two-kernel form: ~12-term chains), the
 * two agree within 5e-5 of the largest entry.  Which form runs depends on these arguments only: in1 == NULL, score == NULL,
 * p_xy == NULL (p_xy means the TPS_PP table layout, whose p_hat lacks the [1, x, y] columns the one-launch form reads from the
 * transposed classic table), p_hat_t given and 16-byte aligned, C0 <= 3, F <= 21, Ho*Wo in (1024, 4096] and a multiple of 4,
 * the fp64 accumulator, and the TPSPP_BWD_TWO_KERNELS flag bit unset.
 * TPSPP_IO_BF16 in `table_flags`: g_out0, g_out1, in0, in1, g_in0 and g_in1 hold bfloat16 (the pointers are reinterpreted, as in
 * the forward).  Everything else keeps its type: grid, T, the tables, score, g_ctrl, g_score, the workspace (dL/d grid in its
 * first N * Ho*Wo * 2 floats included) and all accumulation.  bf16 is widened exactly to fp32 as it is read; every product,
 * chain and accumulator is the fp32 kernel's; g_in0 / g_in1 are the fp32 kernel's values on the widened inputs, rounded once
 * to nearest even when the finished LDS plane is stored; NaN and Inf behave as without the bit.  g_ctrl, g_score and dL/d grid
 * have the bits of the fp32 call on the widened inputs.  Served: (a) the one-launch form, under its conditions above with the
 * image staged at two bytes per pixel (8 C0 H0 W0 bytes of LDS <= 78 KB); (b) the sampling + parameter kernels where
 * dL/d input is finished in LDS: Ho*Wo <= 4096, input planes of at most 4096 pixels, one or two inputs, with or without a
 * score; both accumulators; TPSPP_BWD_TWO_KERNELS keeps its meaning.  Both need H0*W0 (and H1*W1) to be a multiple of 8 (bf16
 * planes of whole 16-byte pieces) and in0 / in1 / g_in0 / g_in1 16-byte aligned.  Refused with TPSPP_EINVAL before any launch
 * or memset, tpspp_last_error naming the condition: every shape that without the bit accumulates dL/d input in HBM (more than
 * 4096 output pixels, a plane of more than 4096 pixels) -- a bf16 sum cannot be accumulated there -- and misaligned planes.
 * These conditions are checked before the N == 0 return: a call with N = 0 tells whether a geometry is served.
 * replaces: autograd through backbones/tps_pp/tps_pp.py:467-496,597-615;
 *           preprocessor/tps_preprocessor.py:71-83,270-282
 */
size_t tpspp_warp_bwd_workspace_floats(int N, int Ho, int Wo);
/* How dL/d input is accumulated in LDS when whole planes fit.  Default = fp64 LDS atomics: every term's fp32 bits are kept
 * whatever the spread of magnitudes (a non-finite gradient poisons the four taps it touches, as ATen does), but the fp64 sum
 * depends on the order in which the atomics arrive (2^-53 relative per add), so g_in0 / g_in1 are NOT bitwise reproducible
 * from run to run: after the rounding to fp32 two runs differ by at most one fp32 ulp, and only where the fp64 sum lies
 * within ~2^-50 of an fp32 rounding tie (tests/test_gpu_backward.py bounds it).  TPSPP_BWD_FIXED_POINT in `table_flags`
 * selects, for that call only, round 3's 64-bit fixed point: order-independent, hence bitwise reproducible, exact within
 * 2^-50 of a pass's largest |g| (a non-finite gradient turns the whole plane NaN).  g_ctrl / g_score are computed in a fixed
 * order in either mode.  tpspp_warp_bwd_set_accumulator(1) makes the fixed point the process-wide default of calls that do
 * not pass the flag (kept for scripts/bench_backward.py; prefer the flag: it is per call and per stream). */
int tpspp_warp_bwd_set_accumulator(int fixed_point);
int tpspp_warp_bwd(const float* g_out0, const float* in0, int C0, int H0, int W0,
                   const float* g_out1, const float* in1, int C1, int H1, int W1,
                   const float* grid, const float* T, const float* inv_delta_c,
                   const float* p_hat, int p_hat_ld, const float* p_xy, const float* score,
                   const float* p_hat_t_or_null, int table_flags, int N, int F, int Ho, int Wo,
                   float* g_in0, float* g_in1, float* g_ctrl, float* g_score,
                   float* g_grid_ws, size_t g_grid_ws_floats, tpspp_stream_t stream);

/*
 * The kernels tpspp_warp_bwd launches for these arguments (a host-side query: touches no device, works without one, launches
 * nothing).  Takes tpspp_warp_bwd's arguments without the stream; a pointer is only compared with NULL and read for its
 * alignment, never dereferenced, so any address with the alignment of the real buffer will do.  Both functions decide through
 * one planner (warp_bwd_plan, tpspp_warp_bwd.hip): whatever tpspp_warp_bwd refuses -- null pointers, bad sizes, a workspace
 * that is too small, N > 65535, the TPSPP_IO_BF16 shapes -- is refused here with the same TPSPP_EINVAL and the same
 * tpspp_last_error text; honours tpspp_warp_bwd_set_accumulator.  On TPSPP_OK `route` (at least TPSPP_WARP_BWD_ROUTE_INTS
 * ints, checked) holds:
 *   [0]  sampling family: 0 the one-launch classic kernel, 1 its bf16 form, 2 kernel A'' ("lds2": 8-byte LDS accumulators,
 *        per-workgroup slices of dL/d grid), 3 kernel A' ("lds": fp32 LDS atomics), 4 kernel A ("atomics": fp32 global
 *        atomics, dL/d input zeroed by memsets); -1 with N = 0 (accepted, nothing to launch; every other entry is 0)
 *   [1] [2]  kernel A'': output pixels per thread (1, 2, 4) and threads per workgroup (256, 1024)
 *   [3]  1 = dL/d input accumulated in fp64, 0 = 64-bit fixed point (families 0, 1, 2)      [4]  1 = bf16 images and gradients
 *   [5]  G, sampling workgroups per (image, input) (families 2, 3; at most 8)
 *   [6] [7]  channels per chunk of input 0 / 1        [8] [9]  channel chunks of input 0 / 1 (families 2, 3, 4)
 *   [10] slices of dL/d grid the parameter kernel adds, in ascending order (G x inputs for families 2 and 3; the channel
 *        chunks of both inputs, at most 16, for family 4; 0 for the one-launch forms): dL/d grid never goes through atomics
 *   [11] 1 = warp_bwd_params_kernel follows (families 2, 3, 4); then its instantiation and grid:
 *   [12] KMAX (24, 36, 64: the smallest that holds F + 3)   [13] TABLE (0 classic [1, x, y, rbf], 1 TPS_PP: p_xy given)
 *   [14] TRANSPOSED (p_hat_t given)   [15] SCORE (0 none, 1 (N, n, F), 2 (N, F, n))   [16] GSCORE (g_score wanted)
 *   [17] S, workgroups per image (1..8), each over ceil(Ho*Wo / S) pixels
 */
#define TPSPP_WARP_BWD_ROUTE_INTS 18
int tpspp_warp_bwd_route(const float* g_out0, const float* in0, int C0, int H0, int W0,
                         const float* g_out1, const float* in1, int C1, int H1, int W1,
                         const float* grid, const float* T, const float* inv_delta_c,
                         const float* p_hat, int p_hat_ld, const float* p_xy, const float* score,
                         const float* p_hat_t_or_null, int table_flags, int N, int F, int Ho, int Wo,
                         const float* g_in0, const float* g_in1, const float* g_ctrl, const float* g_score,
                         const float* g_grid_ws, size_t g_grid_ws_floats, int* route, int route_ints);

/*
 * out = act(conv2d(cat_c(up(src_0), up(src_1), up(src_2)), W) + bias [+ residual]) [+ residual]
 *       [* post_scale + post_shift]
 * fp32, NCHW, 1x1 or 3x3 kernel with "same" padding ((K-1)/2), stride (sh, sw), on the fp32 matrix
 * cores (exact fp32 products, fp32 accumulation).
 *   src_ptrs[i]   (N, C_i, H_i, W_i); src_dims + 5*i = {C_i, H_i, W_i, uh_i, uw_i}: source i is
 *                 nearest-upsampled by (uh_i, uw_i) on the fly; all sources share the logical size;
 *                 with nsrc > 1 every C_i must be a multiple of tpspp_conv_chunk_channels(K), 32 (1x1) / 4 (3x3):
 *                 no kernel's channel chunk straddles two sources (the generic 3x3 kernel takes 8 channels per chunk
 *                 where every source but the last holds a multiple of 8, and 4 per chunk otherwise)
 *   weight_t      (Cin*KH*KW, Cout) = the PyTorch weight (Cout, Cin, KH, KW) flattened and
 *                 transposed once by the caller (BatchNorm, if any, folded in): generic kernel
 *   weight_tiled  the same values arranged (chunk, tap, channel-in-chunk, cout) with
 *                 KC = tpspp_conv_chunk_channels(K) channels per chunk, zero-padded to whole
 *                 chunks: [ceil(Cin/KC)][KH*KW][KC][Cout]; enables the tiled kernel (either pointer
 *                 may be NULL; results agree to fp32 rounding, the summation order differs)
 *   bias          (Cout) or NULL;  residual (N, Cout, Ho, Wo) or NULL
 *   res_mode      0 none, 1 act(conv + bias) + residual, 2 act(conv + bias + residual)
 *   relu          activation code: 0 none, 1 ReLU, 2 GELU in its exact erf form (nn.GELU / mmcv.GELU,
 *                 common/modules/transformer_module.py:116,121)
 *   post_scale/post_shift (Cout) or NULL: per-channel affine applied last (an eval-mode BatchNorm that
 *                 FOLLOWS the activation: backbones/nrtr_modality_transformer.py:42-48)
 * replaces: mmcv ConvModule / nn.Conv2d (+ nn.Upsample, torch.cat, skip additions)
 *           backbones/tps_pp/tps_pp.py:126-131,149-154,156-169,538-552,560-562;
 *           preprocessor/tps_preprocessor.py:101-128; backbones/resnet_v2_large.py:131-135;
 *           layers/conv_layer.py:12-33; backbones/nrtr_modality_transformer.py:19-48
 */
int tpspp_conv2d_fwd(const float* const* src_ptrs, const int* src_dims, int nsrc,
                     const float* weight_t, const float* weight_tiled, const float* bias,
                     const float* residual, const float* post_scale, const float* post_shift,
                     int res_mode, int relu, int N, int Cout, int KH, int KW, int sh, int sw,
                     float* out, int Ho, int Wo, tpspp_stream_t stream);

/*
 * The kernel tpspp_conv2d_fwd launches for these sizes (a host-side query: touches no device, works without one).
 * Takes what the choice depends on: src_dims and nsrc as above, whether weight_t / weight_tiled are given (0 | 1), and
 * the sizes; honours bit 0 of tpspp_conv_set_tuning.  Sizes the forward refuses are refused with the same negative code
 * and the same tpspp_last_error text.  Otherwise a non-negative packed code:
 *   bits 0-3   family: 0 generic (im2col chunks), 1 tiled, 2 wide (1x1, 128x128 tiles), 3 skinny (1x1, split K)
 *   bits 4-7   kernel size, 1 or 3
 *   generic:   bits 8-15  input channels per chunk (32 for 1x1; 8 for 3x3, or 4: see src_dims above)
 *   skinny:    bits 8-15  wavefronts that split K (4, or 16 for Cin >= 256)
 *   tiled:     bits 8-11 stride h, 12-15 stride w, 16-19 tile rows TH, 20-27 tile columns TW,
 *              bit 28 images per tile - 1 (two images share a tile on maps of at most 4x16), bit 29 accumulators per
 *              wavefront - 1 (one for Cout <= 32, two otherwise)
 * (N = 0 launches nothing; the code is then the one a non-empty batch of these sizes would be judged by.)
 */
int tpspp_conv2d_route(const int* src_dims, int nsrc, int has_weight_t, int has_weight_tiled,
                       int N, int Cout, int KH, int KW, int sh, int sw, int Ho, int Wo);

/*
 * Backward of tpspp_conv2d_fwd with res_mode = 0 and no post-affine, i.e. of
 *     y = act(conv2d(cat_c(up(src_0), up(src_1), up(src_2)), W) + bias),   act: relu = 0 none, 1 ReLU,
 * on the fp32 matrix cores (exact fp32 products, fp32 accumulation).  Sizes and source descriptions as
 * tpspp_conv2d_fwd takes them (src_dims + 5*i = {C_i, H_i, W_i, uh_i, uw_i}, 1x1 or 3x3 "same" padding), with the
 * stride restricted to sh, sw in {1, 2}.  The gradient reaching the convolution is dz = dy * [y > 0] for ReLU
 * (PyTorch's threshold_backward on the in-place ReLU's output: no gradient where y == 0), dz = dy otherwise; it is
 * formed as dy is read and never stored.  `y` is the forward's output (read only with relu = 1, may be NULL otherwise).
 *
 * Data gradient: dsrc_ptrs[i] (N, C_i, H_i, W_i) receives source i's gradient, NULL skips that source (at least one
 * must be given).  An upsampled source's gradient is the sum over its uh x uw footprint; source pixels no output reads
 * (1x1 kernel at stride 2) get exact zeros.  Every element of a requested gradient is written.
 *   weight (Cout, Cin_total, KH, KW): PyTorch's layout, read as it is.
 */
int tpspp_conv2d_bwd_data(float* const* dsrc_ptrs, const int* src_dims, int nsrc, const float* weight,
                          const float* dy, const float* y, int relu, int N, int Cout, int KH, int KW, int sh, int sw,
                          int Ho, int Wo, tpspp_stream_t stream);

/*
 * Floats of workspace tpspp_conv2d_bwd_weight needs for these sizes (0 for N == 0 or invalid sizes).
 */
size_t tpspp_conv2d_bwd_weight_workspace_floats(const int* src_dims, int nsrc, int N, int Cout, int KH, int KW,
                                                int Ho, int Wo);

/*
 * Weight and bias gradient: dweight (Cout, Cin_total, KH, KW) in PyTorch's layout and dbias (Cout); either may be
 * NULL (not both); with dweight NULL only the bias reduction runs (no GEMM), in the same order and to the same bits.  The sources are read as the forward read them (concatenated, upsampled on the fly).
 * The reduction over N*Ho*Wo is a FIXED split-K: the terms are cut into slices whose number depends on the sizes only,
 * each slice writes its partial sums to `ws` (ws_floats >= tpspp_conv2d_bwd_weight_workspace_floats(...), checked) and
 * a second launch adds the slices in a fixed order.  No atomics: the result is bitwise reproducible from run to run and
 * from stream to stream (a property the library backward-weights solvers do not promise).
 * replaces: the autograd of nn.Conv2d (mmcv ConvModule, + nn.Upsample, torch.cat) at
 *           backbones/tps_pp/tps_pp.py:126-131,149-169,537-562
 */
int tpspp_conv2d_bwd_weight(const float* const* src_ptrs, const int* src_dims, int nsrc, const float* dy,
                            const float* y, int relu, int N, int Cout, int KH, int KW, int sh, int sw, int Ho, int Wo,
                            float* dweight, float* dbias, float* ws, size_t ws_floats, tpspp_stream_t stream);

/*
 * The forward's weight layouts built on the device from PyTorch's (Cout, Cin, KH, KW) weight (a training step changes
 * the weights every step): weight_t (Cin*KH*KW, Cout) and/or weight_tiled as tpspp_conv2d_fwd takes them (either may
 * be NULL, not both).
 */
int tpspp_conv2d_prep_weight(const float* weight, int Cout, int Cin, int KH, int KW, float* weight_t,
                             float* weight_tiled, tpspp_stream_t stream);

/*
 * Training kernels of the control-point regressor's other layers (ABI 7; train backend "hip_all", tpspp_regressor_bwd.hip).
 * The autograd functions of tps_pp_amd/ops.py (dgab_autograd, score_autograd, cbam_autograd, tpe_points_autograd) compose
 * DGAB, the score, CBAM and the localization FCs, forward and backward, from the entry points below.  fp32 throughout.
 * REPRODUCIBLE: no atomics; every reduction over rows is a fixed split (slice count a function of the sizes alone) whose
 * slices write slabs into the caller's workspace, added in slice order by a second launch: gradients are bitwise identical
 * across calls and streams.  Host arrays (`*_strides`, `x_layout`) are read during the call only.
 */

/*
 * Strided batched matrix product on the fp32 matrix cores (v_mfma_f32_32x32x2_f32; fp32 accumulation in four k chains
 * interleaved by pairs of k, added pairwise at the end):
 *   C[b][i][j] = epi(alpha * sum_{k < K_b} A[b][i][k] * B[b][j][k] + bias[j])  (+ R[b][i][j] when R != NULL)
 * for b < batch, i < M, j < N.  Element (b, i, k) of A is A[b*a_strides[0] + i*a_strides[1] + k*a_strides[2]] (B and C / R
 * likewise with b_strides, c_strides), in elements: tokens can be read from and written to NCHW maps in place.
 * epilogue: 0 none, 1 ReLU, 2 GELU (erf form), 3 tanh.  bias (N) or NULL.  k_total > 0 splits one long reduction over the
 * batch (K_b = min(K, k_total - b*K); k_total <= batch * K), <= 0: K_b = K.  A trailing entry with K_b <= 0 is an empty
 * sum, C[b] = epi(bias) (+ R[b]), and reads neither A nor B; no entry reads k >= K_b.  batch, M or N of 0: success, nothing
 * written.  Only the addressed elements of C are written.  C must not alias A, B or R.
 * replaces: nn.Linear (+ ReLU / GELU) and the score's einsum + tanh in the autograd graph of backbones/tps_pp/DGAB.py:7-23,55,
 *           backbones/tps_pp/tps_pp.py:293-323
 */
int tpspp_mm_f32(int batch, int M, int N, int K, const float* A, const long long* a_strides, const float* B,
                 const long long* b_strides, float* C, const long long* c_strides, const float* bias, const float* R,
                 int epilogue, float alpha, int k_total, tpspp_stream_t stream);

/*
 * Floats of workspace tpspp_linear_bwd_weight needs: S * O * (K + 1), S = ceil(M / L), L = max(256, ceil(M / 512))
 * rounded up to a multiple of 16 (0 for non-positive sizes).
 */
size_t tpspp_linear_bwd_weight_workspace_floats(long long M, int O, int K);

/*
 * Weight and bias gradient of a Linear layer y = x W^T + b over M rows:
 *   dweight (O, K) = sum_r dy[r][:]^T x[r][:],   dbias (O) = sum_r dy[r][:]    (either may be NULL, not both)
 * dy (M, O) dense.  x row r = (q, i), q = r / x_layout[0], i = r % x_layout[0]: x[q*x_layout[1] + i*x_layout[2] + k*x_layout[3]]
 * (dense rows: {M, 0, K, 1}; NCHW tokens: {H*W, C*H*W, 1, H*W}); x_act 2: the layer's input is GELU(x) (x = the previous
 * layer's pre-activation, applied as x is staged), 0: x itself.  M < 2^31.  Fixed split-K into slices of L rows (see the
 * workspace query), matrix cores for dweight, then the ordered slab sum.
 * replaces: the autograd of nn.Linear (weight, bias) at backbones/tps_pp/DGAB.py:7-23,32-34, backbones/tps_pp/tps_pp.py:240-287
 */
int tpspp_linear_bwd_weight(const float* dy, const float* x, const long long* x_layout, int x_act, long long M, int O,
                            int K, float* dweight, float* dbias, float* ws, size_t ws_floats, tpspp_stream_t stream);

/*
 * Pointwise backward of an activation over n elements: out = grad * f'(.), from t:
 *   op 0 ReLU (t = its output: grad where t > 0), op 1 GELU, erf form (t = its input), op 2 tanh(scale * u)
 *   (t = its output: grad * (1 - t^2) * scale, the gradient with respect to u).  out may alias grad.
 * replaces: threshold_backward, GeluBackward, TanhBackward + MulBackward in the autograd graph of tps_pp.py:293-323, DGAB.py:7-23
 */
int tpspp_act_bwd(int op, long long n, const float* grad, const float* t, float scale, float* out, tpspp_stream_t stream);

/*
 * LayerNorm over planes: x (rows, P) -> y = (x - mean) * rstd * w + b, w / b (P), rstd = 1 / sqrt(biased var + eps);
 * mean, rstd (rows) saved for the backward.  One workgroup per plane, fixed reduction tree.
 * replaces: nn.LayerNorm([high, width]) (norm1, norm2) at backbones/tps_pp/DGAB.py:58-77
 */
int tpspp_plane_ln_fwd(const float* x, const float* w, const float* b, long long rows, int P, float eps, float* y,
                       float* mean, float* rstd, tpspp_stream_t stream);

/*
 * Floats of workspace tpspp_plane_ln_bwd needs when it forms parameter gradients: S * 2 * P, S = ceil(rows / L),
 * L = max(16, ceil(rows / 512)) rounded up to a multiple of 16.
 */
size_t tpspp_plane_ln_bwd_workspace_floats(long long rows, int P);

/*
 * Backward of tpspp_plane_ln_fwd from the saved mean / rstd: dx (rows, P) = the input gradient (added to dx's contents when
 * accumulate = 1), or NULL; dweight, dbias (P) = sum over planes of dy * xhat and of dy (fixed split over planes), or NULL.
 * replaces: the autograd of norm1 / norm2, backbones/tps_pp/DGAB.py:58-77
 */
int tpspp_plane_ln_bwd(const float* dy, const float* x, const float* w, const float* mean, const float* rstd, long long rows,
                       int P, float* dx, int accumulate, float* dweight, float* dbias, float* ws, size_t ws_floats,
                       tpspp_stream_t stream);

/*
 * DGAB's pooled gate inputs: xn (N, C, H, W) (the norm1 output), y (N, C, T) the point map (en_feat, T = its H*W) ->
 *   catw (N, C, W + T) = [mean over H of xn, y],  cath (N, C, H + T) = [mean over W of xn, y].
 * H, W <= 256, H * W <= 4096.  One workgroup per (n, c) plane.
 * replaces: torch.cat([x.mean(2), y], 2), torch.cat([x.mean(3), y], 2)   backbones/tps_pp/DGAB.py:37-41
 */
int tpspp_dgab_pool_fwd(const float* xn, const float* y, int N, int C, int H, int W, int T, float* catw, float* cath,
                        tpspp_stream_t stream);

/*
 * Backward of tpspp_dgab_pool_fwd: dxn[n][c][i][j] += dcatw[n][c][j] / H + dcath[n][c][i] / W (accumulates);
 * dy (N, C, T) = dcatw[.., W:] + dcath[.., H:] (written; NULL: not formed).
 * replaces: the autograd of backbones/tps_pp/DGAB.py:36-41
 */
int tpspp_dgab_pool_bwd(const float* dcatw, const float* dcath, int N, int C, int H, int W, int T, float* dxn, float* dy,
                        tpspp_stream_t stream);

/*
 * DGAB's gating: w (N, C, W + 1) = mlp_w output, h (N, C, H + 1) = mlp_h output, xn (N, C, H, W) ->
 *   A[n][c][i][j] = softmax(h[n][c][:H])[i] * xn * h[n][c][H] + softmax(w[n][c][:W])[j] * xn * w[n][c][W].
 * replaces: backbones/tps_pp/DGAB.py:40-45 (softmaxes, gates, the two products and their sum; proj follows on tpspp_mm_f32)
 */
int tpspp_dgab_gate_fwd(const float* xn, const float* w, const float* h, int N, int C, int H, int W, float* A,
                        tpspp_stream_t stream);

/*
 * Backward of tpspp_dgab_gate_fwd: dxn = dA * (vh[i] gh + vw[j] gw) (written), dw (N, C, W + 1) and dh (N, C, H + 1) =
 * the gradients of the pre-softmax gate vectors (softmax backward included).
 * replaces: the autograd of backbones/tps_pp/DGAB.py:40-45
 */
int tpspp_dgab_gate_bwd(const float* dA, const float* xn, const float* w, const float* h, int N, int C, int H, int W,
                        float* dxn, float* dw, float* dh, tpspp_stream_t stream);

/*
 * CBAM forward for training: x (N, C, H, W), shared_MLP weights w1 (Cr, C), w2 (C, Cr) (bias-free 1x1 convolutions),
 * spatial conv cw (1, 2, 3, 3), cb (1) -> out (N, C, H, W), and the gates ca (N, C), sa (N, H*W).  C <= 256, Cr <= 64,
 * H*W <= 256, C*H*W <= 4096.  One workgroup per image.
 * replaces: backbones/tps_pp/tps_pp.py:27-82 as called at :163, in the training graph
 */
int tpspp_cbam_train_fwd(const float* x, const float* w1, const float* w2, const float* cw, const float* cb, int N, int C,
                         int Cr, int H, int W, float* out, float* ca, float* sa, tpspp_stream_t stream);

/* Floats of workspace tpspp_cbam_bwd needs: N * (2 * C * Cr + 19) (per-image slabs). */
size_t tpspp_cbam_bwd_workspace_floats(int N, int C, int Cr);

/*
 * Backward of CBAM (recomputes the forward's gates from x): dx (N, C, H, W) written; dw1 (Cr, C), dw2 (C, Cr), dcw (18),
 * dcb (1) = per-image slabs summed in image order, each NULL when not wanted.  The maxima route their gradient to the
 * first maximal element (torch.max's choice on ties).
 * replaces: the autograd of backbones/tps_pp/tps_pp.py:27-82
 */
int tpspp_cbam_bwd(const float* dout, const float* x, const float* w1, const float* w2, const float* cw, const float* cb,
                   int N, int C, int Cr, int H, int W, float* dx, float* dw1, float* dw2, float* dcw, float* dcb, float* ws,
                   size_t ws_floats, tpspp_stream_t stream);

/*
 * BatchNorm in training mode, fused with the residual add and the ReLU that follow it (ABI 8; the backbone's train backend
 * "hip", tpspp_bn_train.hip).  The autograd functions of tps_pp_amd/ops.py (bn_stem_autograd, bn_block_autograd) compose
 * ResNetABI_v2_large's stem and BasicBlocks from tpspp_conv2d_fwd (relu = 0, weights from tpspp_conv2d_prep_weight), the
 * entry points below, and tpspp_conv2d_bwd_data / _bwd_weight (relu = 0, dz given as dy).  fp32, NCHW, statistics per
 * channel over M = N*H*W; N*C*H*W < 2^31, C <= 65535.  REPRODUCIBLE: no atomics; every per-channel reduction is a fixed
 * split into S = ceil(M / 4096) slices (a function of the sizes alone) whose partials go to the caller's workspace and are
 * combined in slice order (fp64) by a second launch: results are bitwise identical across calls and streams.
 */

/* Floats of workspace tpspp_bn_train_stats needs: S * C * 3, S = ceil(N*HW / 4096) (0 for non-positive sizes). */
size_t tpspp_bn_stats_workspace_floats(int N, int C, int HW);

/*
 * Batch statistics of z (N, C, HW): mean (C) and rstd (C) = 1 / sqrt(biased var + eps).  Per slice (count, mean, M2), the
 * slice's mean first and the squared deviations from it second, merged with Chan's formula: no E[z^2] - E[z]^2.
 * running_mean / running_var (C) or both NULL: updated on the device with PyTorch's rule,
 *   running_mean = (1 - f) running_mean + f mean,  running_var = (1 - f) running_var + f var M / (M - 1),
 * f = momentum if momentum >= 0, else 1 / (num_batches_tracked + 1) (momentum=None: the cumulative average); then
 * num_batches_tracked (one int64, or NULL) += 1 by a launch of its own.  An update needs M >= 2.
 * replaces: the batch statistics and running-statistics update of nn.BatchNorm2d in .train() (F.batch_norm, training=True)
 *           at backbones/resnet_v2_large.py:131-135,160-196, layers/conv_layer.py:12-33
 */
int tpspp_bn_train_stats(const float* z, int N, int C, int HW, float eps, float momentum, long long* num_batches_tracked,
                         float* running_mean, float* running_var, float* mean, float* rstd, float* ws, size_t ws_floats,
                         tpspp_stream_t stream);

/*
 * The statistics an eval-mode BatchNorm normalises with: mean (C) = running_mean, rstd (C) = 1 / sqrt(running_var + eps).
 * replaces: nn.BatchNorm2d in .eval() inside a training graph (frozen-BatchNorm fine-tuning)
 */
int tpspp_bn_eval_stats(const float* running_mean, const float* running_var, int C, float eps, float* mean, float* rstd,
                        tpspp_stream_t stream);

/*
 * y (N, C, HW) = act(gamma_a (za - mean_a) rstd_a + beta_a + r), act = ReLU (relu = 1) or none (0), r by res_mode:
 *   0 nothing; 1 the tensor `residual` (N, C, HW) (identity shortcut); 2 a second normalised branch
 *   gamma_b (zb - mean_b) rstd_b + beta_b (downsample shortcut).  Per-channel vectors (C).  One pass.
 * replaces: relu(bn1(conv1 x)), relu(bn2(conv2 .) + x), relu(bn2(conv2 .) + bn_d(conv_d x)) and the stem's relu(bn(conv x))
 *           at backbones/resnet_v2_large.py:181-186, layers/conv_layer.py:12-33
 */
int tpspp_bn_apply_fwd(const float* za, const float* mean_a, const float* rstd_a, const float* gamma_a, const float* beta_a,
                       int res_mode, const float* residual, const float* zb, const float* mean_b, const float* rstd_b,
                       const float* gamma_b, const float* beta_b, int relu, int N, int C, int HW, float* y,
                       tpspp_stream_t stream);

/* Floats of workspace tpspp_bn_bwd_reduce needs: S * C * 3, S = ceil(N*HW / 4096) (0 for non-positive sizes). */
size_t tpspp_bn_bwd_reduce_workspace_floats(int N, int C, int HW);

/*
 * dr = dy [y > 0] (relu = 1; y = the forward's output, as tpspp_conv2d_bwd_data reads it) or dy (relu = 0), and per channel
 *   sum_dr = sum dr,  sum_dr_xa = sum dr xhat_a,  sum_dr_xb = sum dr xhat_b  (xhat = (z - mean) rstd)
 * in one pass over dr: the beta gradient and the gamma gradients of branch a and, with zb != NULL, branch b.  Fixed split
 * as tpspp_bn_train_stats (ws_floats >= tpspp_bn_bwd_reduce_workspace_floats(...), checked).
 * replaces: the autograd of nn.BatchNorm2d (weight, bias), the residual add and nn.ReLU at backbones/resnet_v2_large.py
 */
int tpspp_bn_bwd_reduce(const float* dy, const float* y, int relu, const float* za, const float* mean_a, const float* rstd_a,
                        const float* zb, const float* mean_b, const float* rstd_b, int N, int C, int HW, float* sum_dr,
                        float* sum_dr_xa, float* sum_dr_xb, float* ws, size_t ws_floats, tpspp_stream_t stream);

/*
 * Input gradients of the normalised branches from dr (as tpspp_bn_bwd_reduce forms it) and its sums:
 *   train_x = 1 (batch statistics):  dz_x = gamma_x rstd_x (dr - sum_dr / M - xhat_x sum_dr_xx / M)
 *   train_x = 0 (running statistics): dz_x = gamma_x rstd_x dr
 * for x = a (dza, or NULL) and x = b (dzb, or NULL); xhat recomputed from z, mean, rstd.  sum_dr and sum_dr_xx are read
 * only for a requested branch with train_x = 1 (required there, checked) and may be NULL when no such branch is asked
 * for: an eval-mode BatchNorm whose gamma and beta are frozen needs no reduction.  The shortcut's gradient:
 * dres_mode 1 writes dr to dres, 2 adds it (dres = dres + dr, in that order), 0 leaves dres alone.  With dza = dzb = NULL
 * and relu = 0 the call is the ordered sum dres + dy.
 * replaces: the autograd of nn.BatchNorm2d (input), the residual add and nn.ReLU at backbones/resnet_v2_large.py
 */
int tpspp_bn_bwd_data(const float* dy, const float* y, int relu, const float* za, const float* mean_a, const float* rstd_a,
                      const float* gamma_a, const float* sum_dr_xa, int train_a, float* dza, const float* zb,
                      const float* mean_b, const float* rstd_b, const float* gamma_b, const float* sum_dr_xb, int train_b,
                      float* dzb, const float* sum_dr, float* dres, int dres_mode, int N, int C, int HW,
                      tpspp_stream_t stream);

/*
 * BatchNorm + ReLU + MaxPool2d(2, 2) in one pass, forward and backward, and the backward of AdaptiveAvgPool2d(1) (still ABI
 * 12, bound by name; the classic rectifier's train backend "hip", tpspp_bn_pool_train.hip).  ops.bn_pool_autograd composes
 * a pooled layer of the localisation network from tpspp_conv2d_fwd (relu = 0), tpspp_bn_train_stats / _eval_stats, the
 * entry points below and tpspp_conv2d_bwd_weight / _bwd_data (relu = 0).  Conventions of the block above: fp32 NCHW,
 * N*C*H*W < 2^31, C <= 65535, every argument checked before any launch, N == 0 returns 0 and launches nothing, no
 * allocation, no host synchronisation, no atomics.
 *   a(v) = relu((v - mean_c) (gamma_c rstd_c) + beta_c), tpspp_bn_apply_fwd's expression bit for bit.
 *   A 2x2 window is scanned row by row from its first element with ATen's rule (v replaces m if v > m or v != v); the
 *   selected element is the last one that replaced m: the first of equal maxima wins, a NaN wins.
 * No selector and no activated full-resolution map is stored: both backward passes read z anyway and repeat the scan.
 */

/*
 * p (N, C, H/2, W/2) = the scan of a(z) over each window; H, W >= 2, an odd last row / column belongs to no window.  The
 * bits of tpspp_maxpool2x2_fwd(tpspp_bn_apply_fwd(z, ..., relu = 1)).
 * replaces: nn.BatchNorm2d + nn.ReLU(True) + nn.MaxPool2d(2, 2)   preprocessor/tps_preprocessor.py:101-128
 */
int tpspp_bn_pool2x2_fwd(const float* z, const float* mean, const float* rstd, const float* gamma, const float* beta, int N,
                         int C, int H, int W, float* p, tpspp_stream_t stream);

/* Floats of workspace tpspp_bn_pool2x2_bwd_reduce needs: S * C * 2, S = ceil(N*H*W / 4096) (0 for non-positive sizes). */
size_t tpspp_bn_pool2x2_bwd_reduce_workspace_floats(int N, int C, int H, int W);

/*
 * dr[n][c][y][x] = dp[n][c][y/2][x/2] where (y, x) is its window's selected element and a(z) > 0 there, +0 elsewhere (the
 * uncovered odd row / column included); per channel over all M = N*H*W positions
 *   sum_dr = sum dr,  sum_dr_x = sum dr xhat   (xhat = (z - mean) rstd): the beta and gamma gradients.
 * Fixed split as tpspp_bn_bwd_reduce: S slices from the sizes alone (slice s holds the channel's windows 1024 s .. 1024 s +
 * 1023), partials in ws (ws_floats >= tpspp_bn_pool2x2_bwd_reduce_workspace_floats(...), checked), added in slice order
 * in fp64 by a second launch.
 * replaces: the autograd of nn.MaxPool2d, nn.ReLU and nn.BatchNorm2d (weight, bias)   preprocessor/tps_preprocessor.py:101-128
 */
int tpspp_bn_pool2x2_bwd_reduce(const float* dp, const float* z, const float* mean, const float* rstd, const float* gamma,
                                const float* beta, int N, int C, int H, int W, float* sum_dr, float* sum_dr_x, float* ws,
                                size_t ws_floats, tpspp_stream_t stream);

/*
 * dz (N, C, H, W), every element written:
 *   train = 1 (batch statistics):   dz = gamma rstd (dr - sum_dr / M - xhat sum_dr_x / M)
 *   train = 0 (running statistics): dz = gamma rstd dr; sum_dr and sum_dr_x may be NULL (required with train = 1, checked)
 * A zero dp gives dz == +0 bit for bit in both modes.
 * replaces: the autograd of nn.MaxPool2d, nn.ReLU and nn.BatchNorm2d (input)   preprocessor/tps_preprocessor.py:101-128
 */
int tpspp_bn_pool2x2_bwd_data(const float* dp, const float* z, const float* mean, const float* rstd, const float* gamma,
                              const float* beta, const float* sum_dr, const float* sum_dr_x, int train, int N, int C, int H,
                              int W, float* dz, tpspp_stream_t stream);

/*
 * dx[n][c][:][:] = g[n][c] / (float)(H*W)   (g (N, C), dx (N, C, H, W))
 * replaces: the autograd of nn.AdaptiveAvgPool2d(1)   preprocessor/tps_preprocessor.py:101-128
 */
int tpspp_global_avgpool_bwd(const float* g, int N, int C, int H, int W, float* dx, tpspp_stream_t stream);

/*
 * VeryDeepVgg's training graph (VeryDeepVgg.set_vgg_train_backend("hip"); tpspp_crnn_pool_train.hip): the backward of
 * tpspp_crnn_maxpool_fwd (tpspp_crnn.h), with the backward of the in-place ReLU in front of the pool folded in.
 *   y  (N, C, H, W):   the pool's input (the convolution's ReLU output);
 *   dp (N, C, Ho, Wo): the gradient of the pool's output;
 *   dy (N, C, H, W):   the gradient of y, every element written.
 * Geometry and argument rules are tpspp_crnn_maxpool_fwd's (kh, kw, sh, sw >= 1; 0 <= ph <= kh / 2, 0 <= pw <= kw / 2; Ho, Wo
 * must equal the formula; -22 otherwise), and N C H W <= 2^31 - 1.  No index map is read: each window of y is scanned again
 * with the forward's rule, row by row from -inf, `v > m || v != v` replaces m, and the window SELECTS the last element
 * that did: the first of equal maxima, the last of several NaNs, never padding; a window in which nothing replaced m (all
 * of it -inf) selects its first element inside the map.  This is the routing of ATen's max_pool2d backward.
 *   dy[h][w] = sum of dp[oh][ow] over the windows (oh, ow) that contain (h, w) and selected it,
 * gathered by the element's own lane in ascending (oh, ow), starting from +0: no atomics, no workspace, bitwise
 * reproducible.  relu_mask = 1: an element with !(y > 0) -- zero, negative or NaN -- receives +0 (the ReLU's backward;
 * the convolution backward then runs with relu = 0 and does not read y); relu_mask = 0: the pool's backward alone.  An
 * element that no window covers (an odd last row or column at 2x2 / stride 2) receives +0.
 * Two forms: kernel 2x2, stride 2, no padding, W % 4 == 0, y and dy 16-byte and dp 8-byte aligned: a lane owns two windows
 * side by side (16-byte loads and stores); anything else: one lane per element of y.  Both give the same bits.
 * N == 0 returns 0 and launches nothing.
 * replaces: the autograd of nn.MaxPool2d and of the nn.ReLU(True) in front of it   backbones/very_deep_vgg.py:39-60
 */
int tpspp_crnn_maxpool_bwd(const float* dp, const float* y, int relu_mask, int N, int C, int H, int W, int kh, int kw, int sh,
                           int sw, int ph, int pw, float* dy, int Ho, int Wo, tpspp_stream_t stream);



/*
 * DGAB block of the TPS++ regressor on a (N, C, 16, 64) feature map x with the point features
 * y (N, C, 32) [= en_feat (N, C, 2, 16) viewed per channel]:
 *     xn = LayerNorm_(16,64)(x);  A = gated attention(xn, y);  x1 = x + proj(A);
 *     out = x1 + fc2(gelu(fc1(LayerNorm_(16,64)(x1))))          (proj / fc1 / fc2 act along W)
 *   ln*_w/b (16,64); mlp_w_t (96,65) and mlp_h_t (48,17) = the bias-free Linear weights transposed;
 *   proj_slab [64][64], fc1_slab [4][64][64], fc2_slab [4][64][64]: Linear weights permuted into the
 *   MFMA k-slot order (slot 2*ks+half holds input feature 32*(ks>>4)+(ks&3)+8*((ks&15)>>2)+4*half);
 *   fc1 split into 4 blocks of 64 hidden units; biases in natural order; scratch (N,C,16,64).
 * replaces: backbones/tps_pp/DGAB.py:25-77 as called at backbones/tps_pp/tps_pp.py:318-319
 */
int tpspp_dgab_fwd(const float* x, const float* y, const float* ln1_w, const float* ln1_b,
                   const float* mlp_w_t, const float* mlp_h_t, const float* proj_slab,
                   const float* proj_b, const float* ln2_w, const float* ln2_b,
                   const float* fc1_slab, const float* fc1_b, const float* fc2_slab,
                   const float* fc2_b, float* scratch, float* out, int N, int C,
                   tpspp_stream_t stream);

/*
 * tpspp_dgab_fwd with the three Linear layers of the chain on the bf16 matrix cores (the bf16 configuration):
 * x, LayerNorms, gates, softmaxes, GELU and both residual sums in fp32; the gated map, the normalised x1 and the
 * GELU output are rounded to bf16 once each as matrix operands; erf by Abramowitz-Stegun 7.1.26 (|err| < 1.5e-7).
 *   proj_slab [4 k-steps][2][64 out][8] bf16 = Wp[out][16 j + 8 h + e];
 *   fc1_slab  [4 blocks][4][2][64][8] = W1[64 b + m][16 j + perm[8 h + e]];
 *   fc2_slab  [4 blocks][4][2][64][8] = W2[m][64 b + 16 j + perm[8 h + e]];  perm as in tpspp_front_bf16_fwd;
 *   scratch   (N,C,16,64) bf16;  everything else as tpspp_dgab_fwd.
 *   split3: the three-term "bf16x3" split (see tpspp_conv2d_bf16_fwd): scratch is then fp32 and every slab holds its hi
 *   and lo halves back to back ([..][hi|lo][4 k-steps][2][64][8]); results within ~1e-5 of tpspp_dgab_fwd.
 * replaces: backbones/tps_pp/DGAB.py:25-77
 */
int tpspp_dgab_bf16_fwd(const float* x, const float* y, const float* ln1_w, const float* ln1_b,
                        const float* mlp_w_t, const float* mlp_h_t, const void* proj_slab,
                        const float* proj_b, const float* ln2_w, const float* ln2_b,
                        const void* fc1_slab, const float* fc1_b, const void* fc2_slab,
                        const float* fc2_b, void* scratch, float* out, int N, int C, int split3,
                        tpspp_stream_t stream);

/*
 * The pointwise front of TPS_PP (ResNet45v2 wiring) fused: feat0 = relu(W0 outs0 + b0),
 * feat1 = relu(W1 outs1 + b1) at (H, W); feat2 = relu(W2 x + b2) at (H/2, W/2);
 * feat_grid = relu(Wg cat(feat0, feat1, Upsample2(feat2)) + bg).
 *   outs0/outs1 (N,32,H,W), x (N,64,H/2,W/2); w0/w1_slab [32][64], w2_slab [64][64] = the 1x1 weights
 *   transposed; wg_slab [3][64 k-slots (MFMA order, see tpspp_dgab_fwd)][64]; outputs (N,64,...).
 * replaces: backbones/tps_pp/tps_pp.py:560-562,581-585 (down0, down1, down2, up_sample + cat + down_feat)
 */
int tpspp_front_fwd(const float* outs0, const float* outs1, const float* x,
                    const float* w0_slab, const float* b0, const float* w1_slab, const float* b1,
                    const float* w2_slab, const float* b2, const float* wg_slab, const float* bg,
                    float* feat0, float* feat1, float* feat2, float* feat_grid,
                    int N, int H, int W, tpspp_stream_t stream);

/*
 * Attention score: score_t[b, pt, px] = tanh(scale * sum_j f[b, j, px] * p[b, pt, j]) with
 *   f = W2 (W1 de_feat[b, :, px] + b1) + b2   (feat_linear: Linear 64->32, Linear 32->128, no activation)
 *   de_feat (N, 64, n); w1_slab [64][32] = W1 transposed; w2_slab [32 k-slots][128] = W2 columns in
 *   the MFMA order (slot 2*ks+half <- input feature (ks&3) + 8*(ks>>2) + 4*half), transposed;
 *   p (N, 32, 128) = p_linear(point features); score_t (N, 32, n) -- the (N, F, n) layout that
 *   tpspp_warp_fwd takes with TPSPP_SCORE_TRANSPOSED.
 * replaces: backbones/tps_pp/tps_pp.py:293-312 (get_score / atten_score)
 */
int tpspp_score_fwd(const float* de_feat, const float* w1_slab, const float* b1, const float* w2_slab,
                    const float* b2, const float* p, float scale, float* score_t, int N, int n,
                    tpspp_stream_t stream);

/*
 * tpspp_score_fwd with the three-term "bf16x3" split (see tpspp_conv2d_bf16_fwd) in its three matrix products: fp32
 * tensors in and out, ~5e-6 of scale before the tanh.
 *   w1_slab [hi|lo][4 k-steps][2][32 out][8] bf16 = W1[out][16 j + 8 h + e];
 *   w2_slab [hi|lo][2 k-steps][2][128 out][8]     = W2[out][16 j + perm[8 h + e]]  (perm as in tpspp_front_bf16_fwd)
 * replaces: backbones/tps_pp/tps_pp.py:293-312
 */
int tpspp_score_x3_fwd(const float* de_feat, const void* w1_slab, const float* b1,
                       const void* w2_slab, const float* b2, const float* p, float scale,
                       float* score_t, int N, int n, tpspp_stream_t stream);

/*
 * CBAM(64, ratio 16) on the (N, 64, 2, 16) bottleneck map: mlp0_w (4,64), mlp2_w (64,4) = the
 * bias-free shared 1x1 MLP; sp_w (1,2,3,3), sp_b (1) = the spatial-attention conv.
 * replaces: backbones/tps_pp/tps_pp.py:27-82 as called at :163
 */
int tpspp_cbam_fwd(const float* x, const float* mlp0_w, const float* mlp2_w, const float* sp_w,
                   const float* sp_b, float* out, int N, tpspp_stream_t stream);

/*
 * Per-point stages on en_feat (N, 64, 2, 16) [point t = flattened (2,16) index]:
 *   ctrl (N,32,2) = fc2( relu(fc1b( relu(fc1a(en[:, t])) )) flattened )     fc1a (256,64) fc1b (2,256) fc2 (64,64)
 *   p    (N,32,128) = pl1( pl0(en[:, t]) )                                   pl0 (32,64)   pl1 (128,32)
 * weights / biases in nn.Linear layout.
 * replaces: backbones/tps_pp/tps_pp.py:321-323 (localization_fc1/fc2) and :305 (p_linear)
 */
int tpspp_tpe_points_fwd(const float* en_feat, const float* fc1a_w, const float* fc1a_b,
                         const float* fc1b_w, const float* fc1b_b, const float* fc2_w,
                         const float* fc2_b, const float* pl0_w, const float* pl0_b,
                         const float* pl1_w, const float* pl1_b, float* ctrl, float* p, int N,
                         tpspp_stream_t stream);

/*
 * out (N, C, H/2, W/2) = MaxPool2d(kernel 2, stride 2)(in);  out (N, C) = AdaptiveAvgPool2d(1)(in)
 * replaces: preprocessor/tps_preprocessor.py:110,114,118,126 (LocalizationNetwork.conv)
 */
int tpspp_maxpool2x2_fwd(const float* in, int N, int C, int H, int W, float* out, tpspp_stream_t stream);
int tpspp_global_avgpool_fwd(const float* in, int N, int C, int H, int W, float* out,
                             tpspp_stream_t stream);

/* Channels per K-chunk of the tiled conv kernel for a 1x1 / 3x3 kernel (layout of weight_tiled). */
int tpspp_conv_chunk_channels(int kernel_size);

/*
 * tpspp_front_fwd on the bf16 matrix cores (the bf16 configuration): inputs and feat0 / feat1 / feat2 are bf16,
 * feat_grid bf16 or fp32 (feat_grid_f32 bit 0); accumulation, bias and ReLU in fp32; feat_grid is computed from the
 * bf16-rounded feat0 / feat1 / feat2 (what the separate convolutions would read back).  feat_grid_f32 bit 1 (value 2):
 * feat0 / feat1 / feat2 are written in the BLOCKED layout (N, 8, H, W, 8) -- the eight channels of a group next to
 * each other per pixel -- that tpspp_conv2d_bf16_fwd takes with layout code 2 (same values; feat_grid stays NCHW).
 *   w0 / w1  [2 k-steps][2 halves][64 cout][8] bf16 with value W[cout][16 j + 8 h + e];  w2 the same with 4 k-steps;
 *   wg       [12][2][64][8] with value Wg[cout][16 j + perm[8 h + e]], perm = {0,1,2,3,8,9,10,11,4,5,6,7,12,13,14,15}
 *            (the order in which the matrix core's result registers come back as the next operand);
 *   b0 / b1 / b2 / bg (64) fp32.  Needs H even and W a multiple of 32.
 *   split3: the three-term "bf16x3" split on fp32 tensors -- inputs and all four outputs fp32, every slab holds its hi
 *   and lo halves ([hi|lo][k-steps][2][64][8]), feat0 / feat1 / feat2 are chained without an intermediate rounding;
 *   feat_grid_f32 bit 1 then means the fp32 blocked layout (N, 8, H, W, 8) (tpspp_conv2d_bf16_fwd's code 3).
 * Non-finite values: the ReLU of the bf16 form is a signed 16-bit max on the rounded pair (identical bits for every finite
 * value and for +-inf; a NaN with the sign bit clear propagates like torch.relu's, a NaN with the sign bit set becomes +0);
 * the fp32 / three-term forms and tpspp_down_fused_* use fmaxf(x, 0), which sends every NaN to 0.  NaN inputs are outside
 * the parity contract of all of them (tests/test_gpu_conv_bf16.py pins this behaviour so that a change is noticed).
 * replaces: backbones/tps_pp/tps_pp.py:560-562,581-585
 */
int tpspp_front_bf16_fwd(const void* outs0, const void* outs1, const void* x,
                         const void* w0, const float* b0, const void* w1, const float* b1,
                         const void* w2, const float* b2, const void* wg, const float* bg,
                         void* feat0, void* feat1, void* feat2, void* feat_grid, int feat_grid_f32,
                         int N, int H, int W, int split3, tpspp_stream_t stream);

/*
 * A Linear layer over channel-major tokens on the bf16 matrix cores:  out (Co, M) = act(W^T X + bias) [+ res]
 *   X (K, M) fp32 (rounded to bf16 -- split3: split into hi + lo -- as it is staged), M = images x tokens;
 *   w_arranged: the (Co, K, 1, 1) weight arranged as tpspp_conv2d_bf16_fwd takes a 1x1 kernel (split3: with hi and lo slabs);
 *   bias (Co) or NULL; res (Co, M) fp32 or NULL (added after the activation); act 0 none, 2 GELU (erf);
 *   out (Co, M) fp32 (out_f32 != 0) or bf16.  K % 32 == 0, Co % 128 == 0, M % 4 == 0; fp32 accumulation over k ascending.
 * The recogniser head's encoder projections and the decoder's one-off key / value projections in the bf16 / bf16x3
 * configurations go through this kernel (tpspp_nrtr_encoder_fwd / tpspp_nrtr_decoder_fwd with TPSPP_HEAD_BF16 / _BF16X3).
 * replaces: nn.Linear inside MultiHeadAttention / PositionwiseFeedForward, common/layers/transformer_layers.py:36-75
 */
int tpspp_token_gemm_bf16_fwd(const float* X, const void* w_arranged, const float* bias, const float* res,
                              void* out, int out_f32, int K, int Co, int M, int act, int split3,
                              tpspp_stream_t stream);

/*
 * CRNNDecoder's reduced-precision eval path (opt-in; tpspp_crnn_dec_bf16.hip): the LSTM input projection and the
 * recurrence on the bf16 matrix cores (v_mfma_f32_16x16x32_bf16).  Both take their weight W (rows, K) fp32 ARRANGED on the
 * host side (ops.arrange_mfma16) into the lane order of the instruction's B operand:
 *   [hi | lo][rows / 16][K / 32][64 lanes][8] bf16,  lane l of tile (ct, ks) holds W[16 ct + (l & 15)][32 ks + 8 (l >> 4) + j],
 * j = 0..7: a lane's fragment is one 16-byte load, a wavefront's 1 KB contiguous.  Without split3 there is one slab,
 * bf16(W), round to nearest even; with split3 two, hi = bf16(W) and lo = bf16(W - hi), the lo slab rows * K elements behind
 * the hi slab.  16-byte aligned.
 *
 * Arithmetic of a product sum_k a[k] w[k] (a: the fp32 activation, w: the weight), both kernels:
 *   split3 == 0: sum_k bf16(a[k]) * bf16(w[k]);
 *   split3 == 1: with a_hi = bf16(a), a_lo = bf16(a - a_hi), per k step of 32 the three terms in tpspp_conv2d_bf16_fwd's
 *                order  w_hi a_hi,  w_hi a_lo,  w_lo a_hi  (the lo lo term is dropped);
 * every term one v_mfma_f32_16x16x32_bf16 with fp32 accumulation, k steps ascending: the order is fixed by the layout alone.
 *
 * tpspp_mm_bf16:   C[b][i][j] = sum_{k < K} A[b][i][k] * W[j][k] + bias[j]     b < batch, i < M, j < N
 * A and C fp32, addressed through element strides as tpspp_mm_f32 takes them ((batch, row, k) and (batch, row, column), all
 * >= 0); A is rounded -- split3: split -- while it is staged; B_arranged: W (N, K) arranged as above; bias (N) fp32, added
 * to the finished fp32 sum, or NULL.  K % 32 == 0 and N % 128 == 0 (-22 otherwise); batch * M <= 2^30.  A is staged
 * coalesced along whichever of its strides is 1: k (dense rows), the row, or the batch -- tokens (t, n, c) = feat[n, c, 0, t]
 * of an NCHW map are (batch t: stride 1, row n, k c), and are then taken in the order t fastest.  A row's result does not
 * depend on batch, M or its position.  Only the addressed elements of C are written.  batch, M or N of 0: success, nothing
 * written.
 *
 * tpspp_crnn_lstm_bf16_fwd: tpspp_crnn_lstm_fwd (tpspp_crnn.h) with the recurrent product on the bf16 matrix cores.  xg, out,
 * the directions, the gate order, the cell update and the activations are tpspp_crnn_lstm_fwd's, unchanged:
 *   a_q = xg[t][n][d][q hidden + u] + sum_k h[n][k] w_hh[d][q hidden + u][k]     accumulated ON xg's value, k steps b = 0..7,
 *   c = sigma(a_f) c + sigma(a_i) tanh(a_g),   h = sigma(a_o) tanh(c)            (two multiplies and one add, not fused)
 * xg, c, the activations and the stored out are fp32.  The h that is stored is unrounded; the copy that feeds the next step
 * is bf16(h), round to nearest even (split3: h_hi = bf16(h), h_lo = bf16(h - h_hi), split every step).
 *   w_hh_arranged: [2 directions][hi | lo][64][8][64][8] bf16 -- each direction's (4 hidden, hidden) matrix arranged as above.
 * An image's output depends on its own xg rows alone: not on N, on its position in the batch or on images_per_group, bit
 * for bit.  Work division as tpspp_crnn_lstm_fwd: one workgroup of 512 threads per (direction, block of images_per_group
 * images) for all T steps, planned by tpspp_crnn_lstm_plan; rows past the block stay zero; h in LDS as bf16 (two copies of
 * 16 x 256, hi and lo with split3, swapped at the one barrier per step), c in registers, w_hh read again through L2 every
 * step (512 KB per direction, 1 MB with split3).  No communication between workgroups, no spin-wait, no grid barrier:
 * every loop is bounded by T.  hidden must be 256; T >= 1; T * N <= 2^30; images_per_group 0, 4, 8 or 16; split3 0 or 1
 * (-22 otherwise, before any launch).  N == 0 returns 0 and launches nothing.
 * replaces (opt-in): nn.LSTM(nIn, 256, bidirectional=True), layers/lstm_layer.py:10,14
 */
int tpspp_mm_bf16(int batch, int M, int N, int K, const float* A, const long long* a_strides, const void* B_arranged,
                  float* C, const long long* c_strides, const float* bias, int split3, tpspp_stream_t stream);
int tpspp_crnn_lstm_bf16_fwd(const float* xg, const void* w_hh_arranged, float* out, int T, int N, int hidden,
                             int images_per_group, int split3, tpspp_stream_t stream);

/*
 * CRNNDecoder's training graph on the bf16 matrix cores (opt-in: CRNNDecoder.set_train_compute_dtype("bf16x3");
 * tpspp_crnn_dec_bf16.hip).  The arranged weights, split3 and the arithmetic of a product are those stated above
 * tpspp_mm_bf16; the input projection and dx of a layer run on tpspp_mm_bf16 itself.  No atomics; every loop is bounded by T;
 * no communication between workgroups, no spin-wait, no grid barrier.  Every argument is checked before any launch.
 *
 * tpspp_crnn_lstm_bf16_train_fwd: tpspp_crnn_lstm_bf16_fwd -- one kernel body with a compile-time switch, `out` has the same
 * bits -- that also stores, fp32, what the backward reads, laid out as tpspp_crnn_lstm_train_fwd (tpspp_crnn_train.h) stores
 * it: gates (T, N, 2, 4 hidden) after their activations, cell (T, N, 2, hidden).  Limits as tpspp_crnn_lstm_bf16_fwd.
 *
 * tpspp_crnn_lstm_bf16_bwd: tpspp_crnn_lstm_bwd's recursion (tpspp_crnn_train.h), unchanged: the `+ 0.0f`, tanh from the
 * stored cell, dc and dh_rec in registers, d_xg the unrounded fp32 da.  The one change is the product
 *   dh_rec[n][k] = sum_j da[n][j] w_hh[d][j][k]
 * on v_mfma_f32_16x16x32_bf16: da is rounded (split3: split into hi / lo) as it is written to LDS, the B operand is
 *   w_hh_t_arranged: [2 directions][hi | lo][16][32][64][8] bf16 -- each direction's TRANSPOSE (hidden rows, K = 4 hidden)
 *   arranged as above (ops.arrange_mfma16(w_hh.transpose(1, 2))),
 * per k step of 32 the terms w_hi da_hi, w_hi da_lo, w_lo da_hi, fp32 accumulation from 0, k steps ascending, one chain.
 * Work division and lane <-> (image, unit) map of tpspp_crnn_lstm_bwd: one workgroup of 512 threads per (direction, block of
 * 4, 8 or 16 images); a wavefront's two 16 x 16 tiles are the dh_rec of its own pairs.  An image's d_xg does not depend on
 * N, its position or images_per_group, bit for bit; d_out == 0 gives d_xg == +0.  da in LDS: [hi | lo] x 16 x (1024 + 8)
 * bf16, 66048 bytes with split3 (one workgroup per CU), 33024 without.  There is no direction-major copy.
 * hidden must be 256; T >= 1; T * N <= 2^30; images_per_group 0, 4, 8 or 16; split3 0 or 1.  N == 0 launches nothing.
 *
 * tpspp_linear_bwd_weight_bf16:   dW[i][j] = sum_{b < batch, r < M} DY[b][r][i] * X[b][r][j]     i < O, j < K
 * DY and X fp32, read through (batch, row, column) element strides >= 0 (the NCHW token view and shifted views included);
 * dW dense (O, K) fp32, every element written.  Both operands are rounded -- split3: split -- while they are staged into
 * LDS; the rows (b, r) in the order b M + r are the instruction's k: per k step of 32 rows the terms dy_hi x_hi, dy_hi x_lo,
 * dy_lo x_hi, fp32 accumulation from 0, k steps ascending; rows past batch * M count as zeros.  An operand whose column
 * stride is 1 is staged coalesced along its columns, any other along its rows; both are transposed in LDS into the
 * fragment order.  One workgroup of 256 threads per 128 x 128 tile of dW and slice of the rows.  The split over rows is
 * fixed by (batch, M, O, K) alone:  R = batch M, steps = ceil(R / 32), tiles = (O / 128)(K / 128),
 *   per = ceil(steps / max(1, 512 / tiles)),  slices = ceil(steps / per),  workspace = slices > 1 ? slices O K : 0 floats;
 * with more than one slice each writes its partial to ws and a second launch adds them in ascending order: the result is
 * bitwise reproducible from call to call and from stream to stream, and depends on batch and M through R alone.
 * O % 128 == 0 and K % 128 == 0 (-22 otherwise); batch, M >= 0, R <= 2^30.  R == 0: dW is all +0, no workspace.
 * replaces (opt-in): the autograd of nn.LSTM(nIn, 256, bidirectional=True), layers/lstm_layer.py:10,14
 */
int tpspp_crnn_lstm_bf16_train_fwd(const float* xg, const void* w_hh_arranged, float* out, float* gates, float* cell, int T,
                                   int N, int hidden, int images_per_group, int split3, tpspp_stream_t stream);
int tpspp_crnn_lstm_bf16_bwd(const float* d_out, const float* gates, const float* cell, const void* w_hh_t_arranged,
                             float* d_xg, int T, int N, int hidden, int images_per_group, int split3, tpspp_stream_t stream);
size_t tpspp_linear_bwd_weight_bf16_workspace_floats(int batch, int M, int O, int K);
int tpspp_linear_bwd_weight_bf16(int batch, int M, int O, int K, const float* DY, const long long* dy_strides, const float* X,
                                 const long long* x_strides, float* dW, float* ws, size_t ws_floats, int split3,
                                 tpspp_stream_t stream);

/*
 * down0 + down0_1 (or down1 + down1_1) of the ResNet45v2 wiring in one kernel (bf16 configuration):
 *     out = bf16(relu(conv3x3 stride 2 pad 1 (bf16(relu(W0 in + b0))) + bd))
 * without the intermediate (N, 64, H, W) map in HBM; bit for bit what tpspp_front_bf16_fwd's feat0 / feat1 followed by
 * tpspp_conv2d_bf16_fwd (3x3, stride 2, blocked output) give.
 *   in (N, 32, H, W) bf16, W = 128, H even;  w0 / b0 as tpspp_front_bf16_fwd takes them;  wd = the (64, 64, 3, 3) weight
 *   arranged as tpspp_conv2d_bf16_fwd takes it ([4 chunks][9 taps][2][64 cout][8] bf16), bd (64) fp32;
 *   out: the blocked layout (N, 8, H/2, 64, 8) bf16 (tpspp_conv2d_bf16_fwd's layout code 2).
 * tpspp_front_bf16_fwd may then be called with feat0 = feat1 = NULL (blocked mode): it keeps computing them as operands of
 * feat_grid and stores neither.
 * replaces: backbones/tps_pp/tps_pp.py:560-563 (self.down0_1(self.down0(outs[0])), self.down1_1(self.down1(outs[1])))
 */
int tpspp_down_fused_bf16_fwd(const void* in, const void* w0, const float* b0, const void* wd, const float* bd,
                              void* out, int N, int H, int W, int relu, tpspp_stream_t stream);

/*
 * The same for the three-term "bf16x3" split: in (N, 32, H, 128) fp32, w0 / wd with their hi and lo slabs (as
 * tpspp_front_bf16_fwd / tpspp_conv2d_bf16_fwd take them with split3), out the fp32 blocked layout (N, 8, H/2, 64, 8)
 * (layout code 3); bit for bit tpspp_front_bf16_fwd(split3)'s feat0 / feat1 followed by the three-term 3x3 stride-2
 * convolution.  tpspp_front_bf16_fwd(split3, blocked) accepts feat0 = feat1 = NULL as well.
 * replaces: backbones/tps_pp/tps_pp.py:560-563
 */
int tpspp_down_fused_x3_fwd(const float* in, const void* w0, const float* b0, const void* wd, const float* bd,
                            float* out, int N, int H, int W, int relu, tpspp_stream_t stream);

/*
 * The same for the exact-fp32 configuration: in (N, 32, H, 128) fp32, w0_slab [32][64] (tpspp_front_fwd's), wd_tiled the
 * (64, 64, 3, 3) weight as tpspp_conv2d_fwd's weight_tiled ([16 chunks][9 taps][4][64]), out (N, 64, H/2, 64) fp32 NCHW; bit for
 * bit tpspp_front_fwd's feat0 / feat1 followed by tpspp_conv2d_fwd (3x3, stride 2).  tpspp_front_fwd accepts
 * feat0 = feat1 = NULL.
 * replaces: backbones/tps_pp/tps_pp.py:560-563
 */
int tpspp_down_fused_f32_fwd(const float* in, const float* w0_slab, const float* b0, const float* wd_tiled,
                             const float* bd, float* out, int N, int H, int W, int relu, tpspp_stream_t stream);

/*
 * The same fused convolution on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16: bf16 operands, fp32
 * accumulation; bias / residual / activation / affine in fp32) for the bf16 configurations
 * (BASELINE.json configs[2], configs[4]).  Every tensor is independently bf16 NCHW (layout code 0), fp32 NCHW (1) or
 * bf16 BLOCKED (2): (N, C/8, H, W, 8), the eight channels of a group next to each other per pixel -- a 16-byte unit
 * of that layout IS a unit of the kernel's channel-innermost LDS patch, so a blocked source is staged with 16-byte
 * loads and no transposition, and a blocked output leaves as 8-byte pieces straight from the result registers
 * (layers that only feed other convolutions use it; C a multiple of 8; not with split3); with split3 there is code 3,
 * the same blocked shape in fp32 (sources, residual, output: a patch position's 8 channels are two 16-byte loads).
 * Same values in every layout.
 *   src_ptrs[i]      (N, C_i, H_i, W_i); src_dims + 6*i = {C_i, H_i, W_i, uh_i, uw_i, layout code}; uh, uw in
 *                    {1, 2, 4}; with nsrc > 1 every C_i must be a multiple of
 *                    KC = tpspp_conv_bf16_chunk_channels(K)
 *   weight_arranged  bf16, the PyTorch weight (Cout, Cin, KH, KW) (BatchNorm folded) zero-padded to
 *                    Cout % 64 == 0 and Cin % KC == 0 and laid out
 *                    [Cout/64][Cin/KC][KH*KW][KC/8][64 cout][8 cin]  (the LDS image of each K-chunk)
 *   bias, post_scale, post_shift   (Cout) fp32 or NULL
 *   residual         (N, Cout, Ho, Wo), layout code residual_f32, or NULL; res_mode as above
 *   relu             0 none, 1 ReLU, 2 GELU (exact erf form)
 *   out              (N, Cout, Ho, Wo), layout code out_f32 (bf16: round to nearest even)
 *   split3           "bf16x3": every fp32 operand is split into bf16 halves (hi = bf16(x), lo = bf16(x - hi)) and a
 *                    product is hi*hi + hi*lo + lo*hi in fp32: ~5e-6 relative error per layer (fp32: 3e-7, bf16:
 *                    2.5e-3) at three bf16 matrix instructions.  weight_arranged then holds TWO slabs per chunk,
 *                    [Cout/64][Cin/KC][hi|lo][KH*KW][KC/8][64][8]; fp32 sources are split as they are staged
 * replaces: the call sites listed for tpspp_conv2d_fwd when the module runs in bf16.
 */
int tpspp_conv2d_bf16_fwd(const void* const* src_ptrs, const int* src_dims, int nsrc,
                          const void* weight_arranged, const float* bias,
                          const void* residual, int residual_f32,
                          const float* post_scale, const float* post_shift,
                          int res_mode, int relu, int N, int Cout, int KH, int KW, int sh, int sw,
                          void* out, int out_f32, int Ho, int Wo, int split3, tpspp_stream_t stream);

/*
 * The kernel tpspp_conv2d_bf16_fwd launches for these arguments (a host-side query: touches no device, works without one).
 * Takes what the forward takes, minus the stream; the pointers only for being NULL or not and for their alignment (the
 * choice depends on the 16-byte alignment of sources, output and weight) -- none is dereferenced.  Honours bits 1 and 2 of
 * tpspp_conv_set_tuning.  What the forward refuses is refused with the same negative code and the same tpspp_last_error
 * text.  Otherwise a non-negative packed code:
 *   bits 0-2   family: 0 tiled (plain bf16), 1 tiled-x3 (three-term split), 2 wide3 (3x3, 128 x 64 wavefront tiles),
 *              3 wide1 (the same kernel's 1x1 form), 4 stem, 5 persist (persistent blocked 3x3), 6 blk1 (blocked 1x1)
 *   bit 3      kernel size: 0 1x1, 1 3x3
 *   bits 4-5   stride h, bits 6-7 stride w
 *   every family but blk1:
 *     bits 8-12  output tile rows TH, bits 13-21 tile columns TW, bits 22-24 images per tile (1, 2 or 4),
 *     bits 25-26 32-pixel fragments per wavefront NF - 1 (tiled: NF 1 = 128-pixel workgroup tiles, 2 = 256; persist: 1 | 2;
 *                wide3, wide1 and stem: 4)
 *   tiled, tiled-x3: bit 27 wide staging (16-byte pieces of bf16 NCHW rows brought into patch order in LDS; needs a 3x3
 *              stride-1 layer, a tile of a multiple of 16 columns and every source bf16 NCHW at full resolution with W a
 *              multiple of 8 and a 16-byte aligned pointer; never with split3), bit 28 accumulators per fragment - 1 (one
 *              32-channel accumulator for split3 with Cout <= 32, two otherwise)
 *   persist:   bit 27 WRES (the whole weight resident in LDS: Cin <= 64), bits 28-29 EPI (0 blocked output, 1 blocked output
 *              + blocked residual, 2 fp32 NCHW output), bit 30 CPB - 1 (two 16-channel chunks per ring slot: WRES, an even
 *              chunk count and room for a ring of three such slots)
 *   wide3, wide1: bits 27-28 epilogue (0 blocked output, 1 blocked + blocked residual, 2 fp32 NCHW, 3 fp32 NCHW + blocked
 *              residual)
 *   stem:      bit 27 output form (0 bf16 NCHW, 1 blocked)
 *   blk1:      bits 8-11 NT (32-channel output tiles per launch), bits 12-16 NKS (16-channel k steps = Cin / 16),
 *              bits 17-18 slices (launches, each owning NT x 32 output channels: 2 for 256 -> 512), bits 19-22 NW
 *              (wavefronts per workgroup, 4 | 8)
 * Some routes depend on N: blk1 wants N * Ho * Wo to be a multiple of 32 NW pixels, and every grid has its limit.  N = 0
 * launches nothing; the code is then the one a batch of N = 8 would be judged by (a whole number of tiles of every kernel).
 * A route, once named, is launched or the forward fails: a refused LDS opt-in or a failed CU-count query (which sizes the
 * persistent kernels' grids, never the route) is an error that names the route, not a silent change of kernel.
 */
int tpspp_conv2d_bf16_route(const void* const* src_ptrs, const int* src_dims, int nsrc,
                            const void* weight_arranged, const float* bias,
                            const void* residual, int residual_f32,
                            const float* post_scale, const float* post_shift,
                            int res_mode, int relu, int N, int Cout, int KH, int KW, int sh, int sw,
                            void* out, int out_f32, int Ho, int Wo, int split3);

/* Channels per K-chunk of the bf16 conv kernel for a 1x1 / 3x3 kernel (layout of weight_arranged). */
int tpspp_conv_bf16_chunk_channels(int kernel_size);

/* Tuning / testing (results do not depend on it).  Bit 0: tpspp_conv2d_fwd uses its generic kernel even when
 * weight_tiled is given.  Bit 1: tpspp_conv2d_bf16_fwd does not use the persistent kernel for blocked 3x3 layers.
 * Bit 2: ... nor the wide-tile kernel (tpspp_conv3_wide.hip) for the blocked 3x3 layers with >= 128 output channels. */
int tpspp_conv_set_tuning(int flags);

/*
 * Launch-shape override for tpspp_warp_fwd (tuning / benchmarking only; results do not depend on
 * it): images per workgroup and threads per workgroup of the gather kernel (0 = heuristic), and
 * kernel choice: 0 = automatic, 1 = force the gather kernel, 2 = require the LDS-staged kernel
 * (TPSPP_EINVAL if the shape does not qualify), 3 = as 2 but ignore TPSPP_TABLE_MIRROR4,
 * 4 = require the plane-streaming kernel, 5 = require the image-pair kernel (classic 32x100 geometry with a
 * tpspp_prepare_mirror_table buffer), 6 = require the in-place kernel (32x100, 32x128, 48x160, 32x64 with C = 1 or 3,
 * same buffer), 7 = require a run-time-geometry kernel (C = 1, 3 or 4, F = 20, same buffer): the in-place kernel where one
 * workgroup covers the image, else row bands with span staging, 8 = require the span-staging kernel (geometries whose
 * prepared table has the third section: tpspp_prepared_table_floats), 9 = require the in-place kernel with run-time
 * geometry in its banded form as well (every band stages the whole image: round 4's kernel, kept for comparisons);
 * bands = workgroups per image pair in the LDS-staged kernel, 0..8 (0 = heuristic); with kernel_choice 7 / 9: bits 0-2 =
 * workgroups per image (0 = heuristic), bit 3 = never an image pair per workgroup; with kernel_choice 8: bits 0-5 =
 * workgroups per image (0 = heuristic), bit 6 = every workgroup on its global-memory path, bit 7 = measure each band's
 * row span before staging it (the first form) instead of requesting the band's rows +- 2 at launch, bits 8-15 = LDS budget
 * per workgroup in KB (0 = 38 / 40: four workgroups per CU).
 */
int tpspp_warp_set_tuning(int images_per_group, int threads_per_group, int kernel_choice, int bands);

/*
 * Diagnostics: when device_buf is non-NULL the LDS-staged kernel writes 8 int64 shader-clock stamps
 * per workgroup (start, T ready, grid expanded, images in LDS, stores retired, DMA issued, DMA
 * landed, unused) into device_buf[workgroup * 8 + i]; the image-pair kernel writes ticks since kernel entry
 * of (T ready, tap descriptors done, image A landed, A staged, image B landed, B staged, stores retired) and
 * the 100 MHz wall clock at entry.  NULL (default) disables it.
 */
int tpspp_warp_set_trace(long long* device_buf);
/* Diagnostics of the persistent decoder step (tpspp_nrtr_decoder_fwd, reduced-precision heads): when non-NULL every workgroup
 * writes the 100 MHz wall clock at the end of each of its phases, device_buf[(step * workgroups + workgroup) * 64 + phase]
 * (phase 0 = entry; 8 phases per layer, then the classifier); the buffer must hold steps x workgroups x 64 int64.  NULL
 * (default) disables it. */
int tpspp_head_set_trace(long long* device_buf);
/* Lab / test hook: occupies the device for a while -- `workgroups` workgroups of one wavefront, each holding `lds_bytes` of LDS
 * (>= 64 KB keeps a workgroup of the persistent decoder, ~103 KB, off that CU), spin for `milliseconds` of wall-clock time
 * (<= 2000) on `stream`.  tests/test_gpu_head.py uses it to decode on a partly occupied device. */
int tpspp_lab_occupy(int workgroups, int lds_bytes, int milliseconds, tpspp_stream_t stream);

/* ===== Recogniser head after TPS++: NRTR encoder / decoder ==========
 *
 * Layout convention of the head: activations are CHANNEL-MAJOR matrices X[c][m] (row = feature,
 * column = token; m = image * T + token), fp32, dense.  Linear weights are passed K-MAJOR: the
 * PyTorch weight (out_features, in_features) transposed once by the caller to (in_features,
 * out_features).  d_k = d_v = 64 (n_head = d_model / 64), dropout is the identity (inference).
 */

/* out (cols, rows) = in (rows, cols) transposed. */
int tpspp_transpose2d(const float* in, int rows, int cols, float* out, tpspp_stream_t stream);

/*
 * y[c][m] = (x[c][m] - mean_m) / sqrt(var_m + eps) * gamma[c] + beta[c], statistics over the C rows of
 * column m (biased variance): nn.LayerNorm(C) applied to every token of a channel-major (C, M) matrix.
 * replaces: common/layers/transformer_layers.py:44,46,103-105; encoders/nrtr_encoder.py:49;
 *           decoders/nrtr_decoder.py:77
 */
int tpspp_layernorm_cm_fwd(const float* x, const float* gamma, const float* beta, int C, int M, float eps,
                           float* y, tpspp_stream_t stream);

/*
 * Multi-head self-attention of the encoder on already projected q/k/v:
 *   qkv (3C, N*T) channel-major: rows [0,C) = q, [C,2C) = k, [2C,3C) = v; head h = rows [64h, 64h+64)
 *   out (C, N*T):  softmax_j(q_i . k_j / 8  masked to j < valid_len[b]) . v_j   per image b and head
 *   valid_len (N) device int32 or NULL (no mask); T <= 256.  1 <= valid_len[b]; values above T mean T.  The columns of k
 *   and v at or beyond valid_len[b] are never used: whatever they hold, NaN included, reaches no output (the columns of
 *   q there are queries like any other, and their outputs are written).
 * replaces: common/modules/transformer_module.py:24-33,82-93 (ScaledDotProductAttention inside
 *           MultiHeadAttention) with the key mask of encoders/nrtr_encoder.py:51-65
 */
int tpspp_attn_enc_fwd(const float* qkv, int N, int C, int T, const int* valid_len, float* out,
                       tpspp_stream_t stream);

/*
 * Fused LayerNorm -> Linear on a channel-major activation x (K, M), made for the few hundred columns of one
 * decoder step (any size is accepted; large M is better served by the two separate calls):
 *   token_major == 0:  out (Cout, M) = act(W^T LN(x) + bias) [+ residual]     act: 0 none, 1 ReLU, 2 GELU(erf)
 *   token_major != 0:  out (M, Cout) = LN(x)^T W + bias                       (no activation / residual)
 * The LayerNorm's affine is folded into the weight by the caller, once:
 *   w_gamma (K, Cout) = diag(gamma) W_kmajor,   w_colsum (Cout) = column sums of w_gamma,
 *   bias_eff (Cout)   = beta^T W_kmajor (+ bias)  or NULL when that is zero,
 * so that  W^T LN(x)[:, m] = rstd_m (w_gamma^T x[:, m] - mean_m w_colsum) + bias_eff  and the kernel multiplies
 * the activation as it loads it (mean / rstd of every column are accumulated from the same loads, biased variance, eps).
 * Every column is shifted by the median of three of its values (features 0, K/2 and K-1) before it enters the products
 * and the sums, which leaves the identity as it is; both differences then lose digits as |mean - shift| / std of the
 * column grows, not as |mean| / std does.  Measured on an MI355X against float64 (tests/test_gpu_head_primitives.py,
 * K = 127 .. 513, both layouts): at |mean| / std = 16 and 64 of every column the relative L2 error is 1.2e-7 .. 2.7e-7 and
 * 1.2e-7 .. 3.0e-7, next to 3.5e-7 .. 5.4e-7 and 1.1e-6 .. 1.9e-6 of PyTorch's fp32 LayerNorm -> Linear (the same formula
 * on the unshifted values, in fp32 on the CPU: 5.3e-6 .. 1.3e-5 and 9.0e-5 .. 2.0e-4); with one feature 64 or 1000 away
 * from the rest, in a sampled row or not, 1.1e-7 .. 3.2e-7.  The worst case is a shift that is itself an outlier: features
 * 0 and K-1 both 64 or 1000 above the rest give 9.8e-7 .. 1.3e-6 at K = 128 and 5.5e-6 .. 1.1e-5 at K = 512 / 513
 * (PyTorch and the unshifted formula: 1.2e-7 .. 3.7e-7).
 * replaces: `norm` followed by a projection, common/layers/transformer_layers.py:150-163
 */
int tpspp_linear_ln_fwd(const float* x, int K, int M, float eps, const float* w_gamma,
                        const float* w_colsum, int Cout, const float* bias_eff, int act,
                        const float* residual, int token_major, float* out, tpspp_stream_t stream);

/*
 * ResizeOCR + ToTensorOCR + NormalizeOCR on the GPU: N uint8 HWC crops of different
 * sizes, packed in one device buffer, -> out (N, C, H, W) fp32.  Image n (src_h[n] x src_w[n] x C at
 * src_packed + src_offsets[n]) is resized to H x resize_w[n], columns >= resize_w[n] hold pad_value, and every
 * byte v of channel c becomes lut[c*256 + v] (the caller tabulates (v/255 - mean[c]) / std[c] in fp32).
 * The widths come from the host logic of ResizeOCR.__call__ (tps_pp_amd/ocr_transforms.py).
 *   interpolation   ResizeOCR's `backend` (ocr_transforms.py:34-36,46,65 -> mmcv.imresize(..., backend=)):
 *     TPSPP_RESIZE_CV2 (0)     backend None / 'cv2': OpenCV's 8-bit INTER_LINEAR arithmetic (11-bit fixed-point weights;
 *                              INTER_AREA for an exact 2x2 shrink).  PARITY UNPINNED against OpenCV (absent at build time);
 *                              bit-exact against oracle/resize_oracle.py.
 *     TPSPP_RESIZE_PILLOW (1)  backend 'pillow': Image.resize(size, Image.BILINEAR) on uint8 -- Pillow's Resample.c (double
 *                              coefficients of the support-scaled triangle filter, 22-bit fixed point, horizontal pass into
 *                              uint8, then the vertical pass).  PINNED: bit-exact against the installed Pillow's outputs
 *                              (tests/golden/resize_pillow.npz, written by tests/golden/make_resize_golden.py).
 * replaces: mmocr/datasets/pipelines/ocr_transforms.py:67-156 (mmcv.imresize + mmcv.impad, TF.to_tensor, TF.normalize)
 */
#define TPSPP_RESIZE_CV2    0
#define TPSPP_RESIZE_PILLOW 1
int tpspp_resize_normalize_fwd(const unsigned char* src_packed, const long long* src_offsets,
                               const int* src_h, const int* src_w, const int* resize_w,
                               const float* lut, int pad_value, int N, int C, int H, int W,
                               float* out, int interpolation, tpspp_stream_t stream);

/*
 * flags bit of tpspp_nrtr_encoder_fwd / tpspp_nrtr_decoder_fwd (the bf16 configuration, BASELINE.json configs[4]):
 * the wide projections run on the bf16 matrix cores -- encoder: wqkv / fc / w1 / w2; decoder: the one-off key / value
 * projections of the encoder output -- and their entries of layer_ptrs then point to bf16 weights arranged as
 * tpspp_conv2d_bf16_fwd wants a 1x1 kernel; the decoder keeps the encoder keys / values as bf16 (they are the only
 * HBM-bound operand of a decoding step).  Residual stream, LayerNorms, softmaxes, the per-step projections and the
 * classifier stay fp32.
 */
#define TPSPP_HEAD_BF16 1
/* The same projections with the "bf16x3" split of tpspp_conv2d_bf16_fwd (fp32 tensors, ~5e-6 per layer): encoder wqkv / fc /
 * w1 / w2 and the decoder's key projection of the encoder output; their layer_ptrs entries point to hi+lo arranged weights.
 * Keys / values stay fp32. */
#define TPSPP_HEAD_BF16X3 2

/* Scratch sizes (bytes) for the two calls below; 0 on bad arguments. */
size_t tpspp_nrtr_encoder_workspace(int N, int C, int T, int d_inner);
size_t tpspp_nrtr_decoder_workspace(int N, int C, int T, int d_inner, int n_layers, int max_seq_len,
                                    int num_out);

/*
 * NRTREncoder.forward: feat (N, C, H, W) viewed as (N, C, T = H*W) -> LayerNorm(layer_stack(tokens)).
 *   layer_ptrs   n_layers x 12 device pointers, per layer in this order (K-major weights, NULL = absent bias):
 *                norm1.weight, norm1.bias, [linear_q|linear_k|linear_v].weight^T concatenated (C, 3C),
 *                its bias (3C) | NULL, fc.weight^T (C, C), fc.bias | NULL, norm2.weight, norm2.bias,
 *                mlp.w_1.weight^T (C, d_inner), mlp.w_1.bias, mlp.w_2.weight^T (d_inner, C), mlp.w_2.bias
 *   ln_g, ln_b   the encoder's final layer_norm
 *   valid_len    (N) int32 device or NULL: number of valid tokens per image = min(T, ceil(T * valid_ratio))
 *   out_cm       (C, N*T) channel-major result or NULL;  out_ntc (N, T, C) (the reference's return) or NULL
 * Layer order ('norm','self_attn','norm','ffn'), activation GELU (erf).
 * replaces: textrecog/encoders/nrtr_encoder.py:67-87, common/layers/transformer_layers.py:57-75
 */
int tpspp_nrtr_encoder_fwd(const float* feat, int N, int C, int T, int d_inner, int n_layers,
                           const float* const* layer_ptrs, const float* ln_g, const float* ln_b,
                           const int* valid_len, void* workspace, size_t workspace_bytes,
                           float* out_cm, float* out_ntc, int flags, tpspp_stream_t stream);

/*
 * NRTRDecoder.forward_test (greedy, forced_tokens == NULL) / forward_train (teacher forcing):
 *   enc_cm       (C, N*T) channel-major encoder output (tpspp_nrtr_encoder_fwd's out_cm)
 *   layer_ptrs, layer_ptrs_len   the table and its length in pointers, which must be n_layers x 24 + 1 (checked: a
 *                table in the 12- or 18-pointer layout of earlier rounds is refused, not read out of bounds);
 *                per layer (every LayerNorm folded into the projection that
 *                follows it, see tpspp_linear_ln_fwd: w_gamma = diag(norm.weight) W^T-k-major, colsum its
 *                column sums, bias_eff = norm.bias^T W (+ bias)):
 *                  self_attn q|k|v fused (C, 3C): w_gamma, colsum (3C), bias_eff (3C);
 *                  self_attn.fc.weight^T (C, C), its bias | NULL;
 *                  enc_attn.linear_q (C, C): w_gamma, colsum (C), bias_eff (C);
 *                  enc_attn.linear_k.weight^T, its bias | NULL;  enc_attn.linear_v.weight^T (no bias);
 *                  enc_attn.fc.weight^T, its bias | NULL;
 *                  mlp.w_1 (C, d_inner): w_gamma, colsum (d_inner), bias_eff (d_inner);
 *                  mlp.w_2.weight^T (d_inner, C), mlp.w_2.bias;
 *                  then six entries (or NULL: the round-2 channel-major step kernels are used) with the six per-step
 *                  projections (q|k|v with norm1 folded, self fc, enc q with norm2 folded, enc fc, w_1 with norm3 folded,
 *                  w_2) arranged in MFMA fragment order for the token-major step GEMM, Co zero-padded to a multiple of 32:
 *                  exact fp32 (no flag):  [Co/32][K/8][2 k halves][32 outputs][4 k] fp32, k = 8 u + 4 half + e;
 *                  TPSPP_HEAD_BF16 / _BF16X3: hi = bf16(w), lo = bf16(w - hi),
 *                  [Co/32][K/16][hi|lo][2 k halves][32 outputs][8 k] bf16 (products hi*hi + hi*lo + lo*hi, fp32
 *                  accumulation: inside the fp32 tolerance);
 *                one more pointer follows the last layer: the classifier (final layer_norm folded) arranged the same way
 *   emb (num_classes, C) trg_word_emb.weight;  pos_table (n_position, C) position_enc.position_table;
 *   w_cls (C, num_out), cls_colsum (num_out), b_cls (num_out): the classifier with the final layer_norm
 *                (eps 1e-6) folded in the same way;  max_seq_len <= 64;  valid_len as above (cross-attention
 *                key mask) or NULL
 *   forced_tokens NULL: greedy decoding from start_idx; out (N, max_seq_len, num_out) = per-step softmax
 *                scores, tokens_out (N, max_seq_len + 1) int32 (or NULL) = <BOS> followed by the arg-max
 *                of every step.
 *                non-NULL (N, max_seq_len) int32 padded targets: out = raw logits of every position
 *                (keys holding padding_idx are masked out of the self-attention).
 * One position per step against cached keys/values: same results as the reference's full re-run of the
 * padded sequence at every step, up to fp32 summation order.  Nothing synchronises with the host.
 *
 * How the steps run, and what that asks of the caller.  With d_model 512, 8 heads, num_out <= 128, <= 8 layers and the
 * arranged per-step weights present, the max_seq_len steps of up to 512 images run as ONE persistent launch: 16 workgroups
 * (one per CU, 512 threads, ~103 KB of LDS) per 32 images synchronise among themselves through device counters
 * (tpspp_head_persist.h).  That form has two requirements, both ENFORCED by this entry point rather than left to the caller:
 *   (1) co-residency: a group of 8 such clusters (128 workgroups) must be resident together.  The call queries the device's
 *       CU count and the kernel's occupancy; a device (or CU-masked / CPX partition) that cannot hold 128 workgroups gets the
 *       launch-per-phase pipeline instead (same scores: bit-identical for the exact-fp32 head, within 2e-5 with identical
 *       tokens for the reduced-precision heads), one that holds 128..255 gets 256 images per launch.  Under stream capture
 *       the launch pipeline is used as well.
 *   (2) one persistent decode in flight per device and process: every such call makes `stream` wait (hipStreamWaitEvent, no
 *       host synchronisation) for the previous persistent decode issued by this process on the same device, whatever stream
 *       that one ran on.  Decodes issued from several streams / threads are therefore safe and simply run one after the
 *       other; kernels of other streams may overlap a decode (its clusters wait for their CUs).  Decodes issued by ANOTHER
 *       PROCESS on the same device are not seen by this guard: one process per GPU, as everywhere in this library.
 * Failure is loud, never silent: if a cluster's barrier is not completed within TPSPP_HEAD_TIMEOUT_MS (environment,
 * wall-clock milliseconds, default 4000; only possible when (2) is violated from outside the process, or the device is held
 * by another kernel for that long), the scores of that cluster's images are NaN for EVERY step from the failing one to
 * max_seq_len - 1, and *status_out = 1; no step of `out` is left uninitialised and the call itself has long returned
 * TPSPP_OK (it is asynchronous).
 *   status_out   device int32 (or NULL): written on `stream` behind the decode -- 0 = every step completed, 1 = a barrier
 *                timed out (scores NaN as described).  Read it with the copy that fetches the scores / tokens; the Python
 *                wrapper (tps_pp_amd.nrtr_head) does and raises TpsppError.  TPSPP_HEAD_NO_PERSIST=1 (environment) forces
 *                the launch pipeline, which has no such failure mode (status 0).
 * replaces: textrecog/decoders/nrtr_decoder.py:95-113,131-177, common/layers/transformer_layers.py:133-163
 */
int tpspp_nrtr_decoder_fwd(const float* enc_cm, int N, int C, int T, int d_inner, int n_layers,
                           const float* const* layer_ptrs, int layer_ptrs_len,
                           const float* emb, const float* pos_table, int n_position,
                           const float* w_cls, const float* cls_colsum, const float* b_cls, int num_out,
                           int max_seq_len,
                           int start_idx, int padding_idx, const int* valid_len,
                           const int* forced_tokens, void* workspace, size_t workspace_bytes,
                           float* out, int* tokens_out, int* status_out, int flags, tpspp_stream_t stream);

/*
 * Which pipeline and which kernels tpspp_nrtr_decoder_fwd takes for these sizes, flags and this table (same arguments, same
 * meaning; of the HOST array layer_ptrs only which entries are NULL is read).  A host-side query: nothing is launched, no
 * device is needed; it is the function the entry point itself dispatches on.  Returns TPSPP_EINVAL on bad arguments, else
 *   bits 0-1   pipeline: 0 plain (channel-major steps on tpspp_linear_ln_fwd), 1 arranged (token-major steps on the step
 *              GEMM, a launch per phase), 2 persistent-eligible (ONE launch per decode where the device holds a group of
 *              clusters, the stream is not capturing and TPSPP_HEAD_NO_PERSIST is unset; else as 1)
 *   bit 2      keys / values and the self-attention caches are bf16 (TPSPP_HEAD_BF16), else fp32
 *   bit 3      the per-step products and the key projection are exact fp32, else the three-term bf16 split
 *   bit 4      (pipeline 1 and 2's launch form) cross-attention with two heads per wavefront, else one
 *   bits 8-11  pipeline 2: 1 + the persistent kernel's instantiation 0..11 (6 x (T > 64) + 2 x {0 three-term, 1 bf16
 *              keys / values, 2 exact fp32} + (d_inner == 512)); 0 otherwise
 * replaces nothing in the reference (it has one path).
 */
int tpspp_nrtr_decoder_route(int C, int T, int d_inner, int n_layers, const float* const* layer_ptrs, int layer_ptrs_len,
                             int num_out, int flags);

/*
 * Layout change between bf16 convolutions and the sampler: in_blocked (N, C/8, HW, 8) bf16 (tpspp_conv2d_bf16_fwd's layout
 * code 2) -> out_nchw (N, C, HW) bf16.  C % 8 == 0, HW % 64 == 0, 16-byte aligned tensors.  Same values.
 * (The bf16 backbone's second stage ends on the persistent blocked kernel; the warp reads channel planes.)
 * replaces nothing in the reference (its maps are NCHW throughout).
 */
int tpspp_blocked_to_nchw_bf16(const void* in_blocked, int N, int C, int HW, void* out_nchw, tpspp_stream_t stream);

/*
 * AttnConvertor.tensor2idx on the device: scores (N, L, C) fp32 (the decoder's per-step soft-max scores, or any tensor of
 * that shape) -> per position the maximum (val_out (N, L)) and its first index, torch.max's tie and NaN rules; idx_out (N, L)
 * int32 holds that index where the reference's scan KEEPS the character -- position before the image's first end_idx and
 * index != padding_idx -- and -1 elsewhere.  The host then needs one copy of 2 x N x L words per batch.
 * replaces: textrecog/convertors/attn.py:124-140 (torch.max per image, two device->host copies per image, the Python scan)
 */
int tpspp_attn_tensor2idx_fwd(const float* scores, int N, int L, int C, int end_idx, int padding_idx,
                              int* idx_out, float* val_out, tpspp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TPSPP_H_ */
