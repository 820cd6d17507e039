/* =============================================================================================
 * panoflow.h -- C ABI of the MI355X-native bidirectional optical-flow blending path.
 *
 * Drop-in boundary for MungoMeng/Panorama-OpticalFlow (reference paths are relative to
 * /root/reference/).  Everything here is plain pointers + sizes; no C++/torch/OpenCV types.  The
 * C++ mirror of the reference's OpticalFlow.hpp / StitchTool.hpp / PixFlow.hpp classes
 * (panorama-opticalflow_amd/include/) is a thin layer over these entry points; INTEGRATION.md shows
 * the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - return 0 on success, negative pf_status on failure; pf_last_error() gives the message.
 *     No exceptions cross this ABI (the C++ wrapper rethrows util::VrCamException).
 *   - images: 8-bit BGRA interleaved, row-major, `step` = bytes per row  (CV_8UC4)
 *     flow  : float (dx,dy) interleaved, pixels of the full-res image      (CV_32FC2)
 *     blend : float in [0,1] = weight of the RIGHT image                   (CV_32FC1)
 *     map   : uint8 region codes 0/50/100/150                              (CV_8UC1)
 *   - every call is synchronous on return; a context is owned by one host thread and one GPU.
 *   - row steps (host-buffer entry points): a step is the distance in bytes between the starts of two rows of the caller's plane, at
 *     least the row's width (cols x 4 for BGRA and float planes, x 8 for flows, x 1 for the map, x 3 / x 12 for the colour wheel / a
 *     panel) and a multiple of the element's size; bytes of a row beyond its width are never read and never written.  A step below
 *     the row width is PF_ERR_ARG "row step too small", checked before any work; the step of an optional plane that is NULL is
 *     not looked at (0 will do).  Planes that share ONE step argument share the step: L and R (and the merged image of pf_stitch_gather,
 *     the images of a batch, a rig's top and left images), the two flows, the outputs of a batch, the two panels of pf_stitch_visualize;
 *     pf_stitch_prepare / pf_stitch_match write overlapped_l / overlapped_r at the INPUT step (step_bytes), and merged_dis is packed.
 *   - device pointers (the _dev entry points): packed planes at their element's natural alignment -- 4 bytes for BGRA, blend and
 *     other float planes, 8 bytes for flows ((dx, dy) pairs are read and written whole) -- anywhere inside an allocation; nothing
 *     wider is ever required (DESIGN.md 8.9 lists the kernels).  No output of a call may overlap an input or another output of the
 *     same call (inputs may repeat or overlap each other): outputs are written while inputs are still gathered from.  Both are
 *     PF_ERR_ARG before any work ("... is not 4-byte aligned", "... overlaps ...").
 *   - there is NO CPU fallback: without a usable gfx950 device pf_create() fails.
 * ============================================================================================= */
#ifndef PANOFLOW_H_
#define PANOFLOW_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pf_ctx pf_ctx;

typedef enum pf_status {
  PF_OK = 0,
  PF_ERR_ARG = -1,      /* bad argument (null pointer, size out of range, unknown algorithm) */
  PF_ERR_DEVICE = -2,   /* HIP runtime / launch failure */
  PF_ERR_NOMEM = -3,    /* device allocation failed */
  PF_ERR_TIMEOUT = -4   /* a sweep band gave up waiting for its predecessor (never expected) */
} pf_status;

/* OpticalFlowInterface::DirectionHint, CPU/PixFlow.hpp:19 */
typedef enum pf_hint { PF_HINT_UNKNOWN = 0, PF_HINT_RIGHT = 1, PF_HINT_DOWN = 2, PF_HINT_LEFT = 3, PF_HINT_UP = 4 } pf_hint;

/* ---- lifetime -------------------------------------------------------------------------------
 * Replaces the reference's runtime device probe (GPU/OpticalFlow.cpp:132-189, GPU/StitchTool.cpp:33-60). */
int pf_device_count(void);
/* max_cols x max_rows > 0: every device buffer a bidirectional solve / a stitch step of that size needs is allocated
 * now (the first call then pays no allocation); 0 x 0: allocate lazily.  The arena only ever grows, so larger images
 * are still accepted later.  NULL on failure; pf_last_error(NULL) explains. */
pf_ctx* pf_create(int device, int max_cols, int max_rows);
/* The same with the scheduling knobs exposed.  None of them changes a result (tests hold every setting to the same bits);
 * they exist so that a deployment can tune for its image sizes without environment variables.  pf_config_init() fills
 * in the defaults (= what pf_create uses); set struct_size = sizeof(pf_config). */
typedef struct pf_config {
  int struct_size;
  int device, max_cols, max_rows;   /* as pf_create */
  int stagger_levels;       /* direction R->L starts this many coarse levels behind L->R (-1: 2, or 3 for >= 5 Mpix half-res) */
  int64_t fuse_small_level_px; /* levels up to this many pixels fold the upsample / second median into the neighbouring Gaussian
                               launches (-1: 0 for a lone pair, 262144 for the lanes of the throughput mode) */
  int fine_gradient_blocks; /* width of the launch that computes the gradients of the 4 finest levels beside the coarse sweeps (64) */
  int pyramid_chaining;     /* 1: small pyramid levels are built two or three per launch, 0: one launch per level (1) */
  int sweep_window;         /* 1: a sweep covers the bounding box of the gated pixels only, 0: the whole level (1) */
  int sparse_sweep;         /* -1: pick the sweep variant that skips ungated anti-diagonals from the gate density, 0 / 1: force (-1) */
  int batch_pairs;          /* throughput mode (pf_novel_view_batch_dev): pairs that go through ONE set of launches (1..16; in_flight =
                               lanes x batch_pairs, at most 32).  -1: in_flight itself up to 16 (one lane), half of it (two lanes) beyond */
  int sweep_wide;           /* form of the sweep launches.  0 = latency form: 8 lanes per pixel evaluate a step's six energies at once, bands of 8 rows,
                               ONE compute wave per SIMD -- the shortest step, what a lone pair wants.  2 = throughput form: 2 lanes per pixel, the
                               reference's own order without speculation (two gather rounds per step), bands of 32 rows -- less than half the VALU
                               instructions per pixel, what a batch that oversubscribes the chip wants.  -1 (default) = throughput form for the launches of a
                               batch that oversubscribe the chip (sweep_wide_threshold), latency form otherwise.  Same bits in every form.
                               (1 = the latency step with two compute waves per SIMD: measured and rejected, lab build only -- libpanoflow.so answers
                               PF_ERR_ARG.  The throughput form's loader-staged and fused-prepass record paths of rounds 4 / 5 are gone: profiles/.) */
  int sweep_wide_threshold; /* sweep_wide = -1: a launch takes the throughput form when (sweeps running at the same time: pairs of the batch x 2
                               directions x lanes) x (its latency-form workgroups) exceeds this (512: two rounds of the chip) */
  int sweep_throughput_transposed; /* sweep_wide = -1: sweeps whose bands step along y (windows taller than wide, e.g. 2000x4000 strips) may take the
                               throughput form too (1: +17 % on 16 strips in flight; 0 keeps them in the latency form) */
  int full_width_batch_gradients; /* 1: in a batched solve the finest levels' gradients are one full-width launch (nothing to hide them
                               behind: the batch keeps every CU busy anyway), 0: the narrow launch of a lone pair (1) */
  /* Cross-check implementation -- only in libpanoflow_exp.so (the -DPF_EXPERIMENTS build used by the test-suite);
   * libpanoflow.so rejects anything but the default with PF_ERR_ARG. */
  int sweep_impl;           /* 2: wavefront sweep (k_sweep_prep + k_sweep2); 1: the independent 64-rows-per-wave kernel; any other value: PF_ERR_ARG in every build */
} pf_config;
void pf_config_init(pf_config* cfg);
/* Self-test that pf_create already ran once for the context's device: the sweep's asm-block packed-fp32 chains against the
 * compiler-scheduled forms of the same arithmetic, and (round 6) the step's partial DPP writes issued back to back against the same
 * sequence with wait states (the two hardware assumptions of the scheduled sweep TU).  0 = identical bits (or a
 * -DPF_SAFE_PK build, which has no such blocks); > 0 = threads whose results differed (pf_create would have refused the device);
 * < 0 = error code. */
int pf_selftest_packed_chains(pf_ctx* ctx);
pf_ctx* pf_create_cfg(const pf_config* cfg);
void pf_destroy(pf_ctx* ctx);
const char* pf_last_error(const pf_ctx* ctx);  /* ctx may be NULL (creation errors) */
/* Conditions that cost PERFORMANCE, never results: the last warning raised on this context ("" if none) and how many were raised.
 * Today there is one: a call that drives more HIP streams than the HIP runtime has hardware queues (pf_novel_view_batch_dev needs
 * 3 x lanes + 2, pf_stitch_step 5; the runtime sizes its pool from GPU_MAX_HW_QUEUES -- default 4 -- when the process makes its first
 * HIP call) runs correctly but with streams sharing queues.  The library reads GPU_MAX_HW_QUEUES only to report this; it reads no
 * other environment variable (once per process).  A context raises the warning once per condition, not once per call. */
const char* pf_last_warning(const pf_ctx* ctx);
int pf_warning_count(const pf_ctx* ctx);
const char* pf_version(void);

/* makeOpticalFlowByName, CPU/PixFlow.hpp:459-500: "pixflow_low" -> 0, "pixflow_search_20" -> 20,
 * anything else -> PF_ERR_ARG (the reference throws VrCamException). */
int pf_max_percentage_by_name(const char* flow_alg_name);

/* The constructor arguments of the reference's PixFlow<P> (CPU/PixFlow.hpp:46-68).  Its factory only ever passes the values
 * pf_solver_params_init() fills in (:459-497, both presets), but the class accepts any: so does this library (round 6).  The
 * parameters belong to the context and apply to every later solve on it (pf_flow*, pf_novel_view*, pf_stitch_step, the lanes of
 * pf_novel_view_batch_dev).  Results are bit-identical to the reference's arithmetic for every accepted set.  Coefficients large
 * enough to overflow an energy are accepted (the reference computes with them, too); from there on "bit-identical" means: every
 * element of a flow is of the reference's class -- finite, +inf, -inf or NaN -- and a finite element has the reference's bits.  A
 * NaN's sign and payload are not part of the promise (IEEE 754 leaves open which operand's an operation hands on).
 *   pyr_scale_factor  in [0.25, 0.98]: level sizes int(w * s + 0.5f) while both > 24 (:137-151), inter-level flow scale 1.0f / s (:124);
 *                     at most 96 levels (PF_ERR_ARG from the solve otherwise, naming the count, before the solve sizes or launches anything).  0.98f itself is
 *                     accepted here and refused by every solve whose half-resolution sides exceed 25: int(25 * 0.98f + 0.5f) is 25, so
 *                     the reference's pyramid never ends and runs to its limit of 1000 levels (and solves each).  The largest usable
 *                     value is the float below, nextafterf(0.98f, 0);
 *   smoothness_coef, vertical_/horizontal_regularization_coef: finite and >= 0 (errorFunction :450-453; a negative coefficient could
 *                     make an energy negative, which the sweep's "keep" sentinel excludes);
 *   gradient_step_size: finite and >= 0 (:321,334).  A power of two in [2^-16, 2^16] (the presets' 0.5 is one) runs at full speed; any
 *                     other value is computed with the IEEE multiply + subtract in every step of the sweeps (same bits as the reference,
 *                     about 2-3x the sweep time);
 *   downscale_factor: must be 0.5 (the 8-bit half-resolution path, :81-83, is built for it): anything else is PF_ERR_ARG;
 *   directional_regularization_coef: stored and ignored, as in the reference (no code there reads it). */
typedef struct pf_solver_params {
  float pyr_scale_factor, smoothness_coef, vertical_regularization_coef, horizontal_regularization_coef, gradient_step_size, downscale_factor,
      directional_regularization_coef;
} pf_solver_params;
void pf_solver_params_init(pf_solver_params* p);   /* 0.9, 0.001, 0.01, 0.01, 0.5, 0.5, 0 */
int pf_set_solver_params(pf_ctx* ctx, const pf_solver_params* p);   /* p == NULL: back to the presets */
int pf_get_solver_params(const pf_ctx* ctx, pf_solver_params* out);

/* ---- host-buffer entry points (the drop-in boundary) --------------------------------------- */

/* PixFlow<P>::computeOpticalFlow, CPU/PixFlow.hpp:72-135.  flow = I0 -> I1, cols x rows. */
int pf_flow(pf_ctx* ctx, const uint8_t* i0_bgra, const uint8_t* i1_bgra, int cols, int rows, size_t step_bytes,
            int max_percentage, int hint, float* flow_xy, size_t flow_step_bytes);

/* NovelViewGeneratorAsymmetricFlow::prepare, CPU/OpticalFlow.cpp:102-145: wrap-pad by cols/20,
 * L->R solve (hint LEFT) and R->L solve (hint RIGHT) concurrently, crop.  Either output may be NULL. */
int pf_flow_bidir(pf_ctx* ctx, const uint8_t* l_bgra, const uint8_t* r_bgra, int cols, int rows, size_t step_bytes,
                  int max_percentage, float* flow_l2r, float* flow_r2l, size_t flow_step_bytes);

/* NovelViewUtil::combineNovelViews, CPU/OpticalFlow.cpp:30-92 (+ generateNovelViewPoint :9-28). */
int pf_blend(pf_ctx* ctx, const uint8_t* l_bgra, const uint8_t* r_bgra, size_t step_bytes, const float* flow_l2r,
             const float* flow_r2l, size_t flow_step_bytes, const float* blend, size_t blend_step_bytes, int cols, int rows,
             uint8_t* out_bgra, size_t out_step_bytes);

/* prepare() + setBlend() + generateNovelView() in one call with the flows kept in HBM
 * (CPU/main.cpp:82-90).  flow outputs may be NULL. */
int pf_novel_view(pf_ctx* ctx, const uint8_t* l_bgra, const uint8_t* r_bgra, int cols, int rows, size_t step_bytes,
                  int max_percentage, const float* blend, size_t blend_step_bytes, uint8_t* out_bgra, size_t out_step_bytes,
                  float* flow_l2r, float* flow_r2l, size_t flow_step_bytes);

/* Canvas sizes of the stitch entry points that build the blend ramp (pf_stitch_prepare, pf_stitch_generate_blend, pf_stitch_step,
 * pf_stitch_step_batch*): any size the image checks accept.  The tile smoothing of GenerateBlend (CPU/StitchTool.cpp:130-143) works on
 * one tile's window, (step + k - 1)^2 floats + (step + k - 1) x step doubles with step = min(cols, rows) / 200 and k = rows / 130.  Where
 * that fits the 160 KiB (163,840 B) of LDS of a CU (24000x12000 does, 24500x12250 does not) the window stays resident; larger windows
 * (a 30000x15000 equirectangular panorama: ~250 KiB; a 400x26200 strip) are streamed through the LDS in pieces, with the same
 * bits and a per-block scratch area in the context's arena (pre-sized by pf_create).  The one exception: a window that reaches across
 * the whole canvas (k/2 >= min(cols, rows): canvases more than ~260 times taller than wide) returns PF_ERR_ARG. */
/* Stitchtools::prepare, CPU/StitchTool.cpp:7-36 (MatchImages :38-50, GenerateBlend :98-146,
 * countblend :148-191).  Every output may be NULL.  All planes cols x rows; overlapped_l / overlapped_r have the inputs' step_bytes. */
int pf_stitch_prepare(pf_ctx* ctx, const uint8_t* l_bgra, const uint8_t* r_bgra, int cols, int rows, size_t step_bytes,
                      uint8_t* map_out, size_t map_step_bytes, uint8_t* overlapped_l, uint8_t* overlapped_r,
                      float* blend_out, size_t blend_step_bytes, float* merged_dis /* packed, nullable */);

/* The two halves of prepare() as the reference exposes them: Stitchtools::MatchImages (CPU/StitchTool.cpp:38-50) with the overlap
 * masking of :17-33, and Stitchtools::GenerateBlend (:98-146) computed from a GIVEN map -- the reference reads its public `Map`
 * member there, so a caller that edits Map between the two calls gets the ramp of the edited map.  Outputs may be NULL. */
int pf_stitch_match(pf_ctx* ctx, const uint8_t* l_bgra, const uint8_t* r_bgra, int cols, int rows, size_t step_bytes, uint8_t* map_out,
                    size_t map_step_bytes, uint8_t* overlapped_l, uint8_t* overlapped_r);
int pf_stitch_generate_blend(pf_ctx* ctx, const uint8_t* map, size_t map_step_bytes, int cols, int rows, float* blend_out,
                             size_t blend_step_bytes, float* merged_dis /* packed, nullable */);

/* GenerateBlend's per-pixel loop alone, CPU/StitchTool.cpp:113-125: 0 / 1 / 0.5 by map code and, in the overlap,
 * Stitchtools::countblend(x, y) (:148-191) = minLdis / (minRdis + minLdis) -- the ramp BEFORE the smoothing of
 * :130-143 -- plus MergedDis (:185-188, nullable, packed). */
int pf_stitch_raw_blend(pf_ctx* ctx, const uint8_t* l_bgra, const uint8_t* r_bgra, int cols, int rows, size_t step_bytes,
                        float* raw_blend_out, size_t blend_step_bytes, float* merged_dis);

/* Stitchtools::Gather, CPU/StitchTool.cpp:52-96. */
int pf_stitch_gather(pf_ctx* ctx, const uint8_t* l_bgra, const uint8_t* r_bgra, const uint8_t* merged_bgra, size_t step_bytes,
                     const uint8_t* map, size_t map_step_bytes, int cols, int rows, uint8_t* out_bgra, size_t out_step_bytes);

/* One whole iteration of the stitch loop of CPU/main.cpp:70-95 on the device: Stitchtools::prepare ->
 * NovelViewGeneratorAsymmetricFlow::prepare + generateNovelView -> Stitchtools::Gather.  Only the inputs go up
 * and only the composite comes down.  r_bgra == NULL chains on the previous call's result, which stays in HBM
 * (main.cpp:64-65: R_i = FinalResult_{i-1}).  out_bgra may be NULL (intermediate steps). */
int pf_stitch_step(pf_ctx* ctx, const uint8_t* l_bgra, const uint8_t* r_bgra, int cols, int rows, size_t step_bytes,
                   int max_percentage, uint8_t* out_bgra, size_t out_step_bytes);

/* Hint, given BEFORE step i: the l_bgra of step i+1.  Step i then issues that host->device upload after its own kernels are
 * enqueued, so it overlaps the compute (CPU/main.cpp:66-69 reads image i+1 only after step i).  One-shot: step i consumes the
 * hint, step i+1 consumes (or, if it is called with anything else, drops) the uploaded copy.  CONTRACT: the buffer must stay valid
 * and UNCHANGED until step i+1 has returned.  The library guards against the common slip (a buffer reused for another image at the
 * same address) with a content signature over 16 evenly spaced rows taken at upload time -- a sample, not a hash of the whole image:
 * a partial overwrite that misses those rows is not detected and the stale device copy would be used.  NULL cancels.  With the
 * contract kept it is purely an optimisation: results are identical. */
int pf_stitch_prefetch(pf_ctx* ctx, const uint8_t* next_l_bgra, int cols, int rows, size_t step_bytes);

/* Batched stitch step: n_frames independent canvases of one size, each one pf_stitch_step of its own chain, `in_flight` (1..32,
 * clamped like pf_novel_view_batch_dev; pf_config::batch_pairs applies) of them on this GPU at a time.  Groups of frames share every
 * launch (match, blend ramp with ONE tile-smoothing launch per group, solve, blend, gather) on one or more lanes of streams.  Frame k
 * gets exactly the bytes pf_stitch_step would give for frame k's own sequence of calls.  n_frames == 0 does nothing; a negative count,
 * NULL arrays or a NULL l entry are PF_ERR_ARG, as is anything pf_stitch_step refuses (checked before any work).  Synchronous on return.
 * Host form: r_bgra == NULL, or r_bgra[k] == NULL, chains frame k on its own composite of the previous pf_stitch_step_batch call on this
 * context (kept in HBM, one slot per frame index; that call must have had the same cols x rows and more than k frames, else
 * PF_ERR_ARG).  out_bgra == NULL, or out_bgra[k] == NULL, skips frame k's download.  The slots are separate from pf_stitch_step's
 * chained result and pf_stitch_prefetch's records: interleaving the two APIs changes neither one's results.
 * HBM: ~33 B/px of StitchTool planes + 16 B/px of flows + one solver slab per frame in flight, and 12 B/px per frame slot of the host
 * form (left, right, composite).  Needs GPU_MAX_HW_QUEUES >= 3 x lanes + 2, like pf_novel_view_batch_dev. */
int pf_stitch_step_batch(pf_ctx* ctx, int n_frames, const uint8_t* const* l_bgra, const uint8_t* const* r_bgra, int cols, int rows,
                         size_t step_bytes, int max_percentage, uint8_t* const* out_bgra, size_t out_step_bytes, int in_flight);
/* Device form: packed device buffers; no chain state -- every d_r[k] must be non-NULL (the caller chains by ping-ponging its
 * buffers).  A d_out[k] that overlaps any input of the call or another d_out is PF_ERR_ARG; repeated input pointers are allowed. */
int pf_stitch_step_batch_dev(pf_ctx* ctx, int n_frames, const uint8_t* const* d_l, const uint8_t* const* d_r, int cols, int rows,
                             int max_percentage, uint8_t* const* d_out, int in_flight);

/* ---- stitch plans: one rig's overlap map and blend ramp, reused across frames ----------------
 * Stitchtools::prepare derives Map (MatchImages, CPU/StitchTool.cpp:38-50) and the blend ramp (GenerateBlend, :98-146) from the two
 * alpha masks alone, and Gather (:52-96) gives the composite an alpha that is > 0 exactly where L's or R's is -- so for a fixed camera
 * rig every frame of a step has the same map and ramp.  A plan holds them in HBM (5 B/px: map 1, ramp 4) with cols, rows and the
 * overlap pixel count; a planned step uses them instead of recomputing them: no countblend, tile-smoothing or box-blur launch, no
 * blend-ramp stream, and 12 B/px of StitchTool planes per frame in flight (two overlap images and the novel view) instead of 33.
 * A planned step VERIFIES: its match kernel derives every pixel's region code (100 = L only, 50 = R only, 150 = both, 0 = none) from
 * the frame's alphas and compares it with the plan's.  The bytes of a planned call are those of the unplanned call on the same
 * inputs; a call in which any frame differs from the plan in even one pixel's code (alpha 255 -> 0 or 0 -> 1 does, 255 -> 1 does not)
 * fails as a whole with PF_ERR_ARG -- pf_last_error names the first such frame and its pixel count --, delivers no composite (the host
 * forms download nothing, the device form zero-fills every d_out of the call) and leaves nothing to chain on.
 * A plan belongs to the context that made it: passing it to another context (hence another device), after pf_stitch_plan_destroy, or
 * with another cols x rows is PF_ERR_ARG before any work (a handle is looked up in the context's list, never dereferenced first).
 * Creation runs the kernels of pf_stitch_prepare, accepts and refuses the canvases pf_stitch_step does, and leaves the chain state,
 * the prefetch records and pf_stitch_visualize's inputs alone.  r_bgra == NULL takes the R mask from the composite pf_stitch_step /
 * pf_stitch_step_planned left in HBM (PF_ERR_ARG if there is none of this size).  pf_destroy frees the plans still alive. */
typedef struct pf_stitch_plan pf_stitch_plan;
int pf_stitch_plan_create(pf_ctx* ctx, const uint8_t* l_bgra, const uint8_t* r_bgra, int cols, int rows, size_t step_bytes,
                          pf_stitch_plan** plan_out);
int pf_stitch_plan_create_dev(pf_ctx* ctx, const uint8_t* d_l, const uint8_t* d_r, int cols, int rows, pf_stitch_plan** plan_out);
int pf_stitch_plan_destroy(pf_ctx* ctx, pf_stitch_plan* plan);
/* geometry of a LIVE plan (outputs may be NULL) */
int pf_stitch_plan_info(const pf_stitch_plan* plan, int* cols, int* rows, long long* overlap_px);
/* the plan's Map (1 B/px) and finished ramp (4 B/px, what pf_stitch_prepare gives as blend_out); either output may be NULL */
int pf_stitch_plan_download(pf_ctx* ctx, const pf_stitch_plan* plan, uint8_t* map_out, size_t map_step_bytes, float* blend_out,
                            size_t blend_step_bytes);
/* pf_stitch_step with a plan: the same arguments, chain state ("r_bgra == NULL" chains on the last composite whichever of the two
 * calls made it), pf_stitch_prefetch records and pf_stitch_visualize inputs; the same bytes. */
int pf_stitch_step_planned(pf_ctx* ctx, const pf_stitch_plan* plan, const uint8_t* l_bgra, const uint8_t* r_bgra, int cols, int rows,
                           size_t step_bytes, int max_percentage, uint8_t* out_bgra, size_t out_step_bytes);
/* pf_stitch_step_batch / _dev with ONE plan for all frames; the host form shares the unplanned one's frame slots, so the two may be
 * interleaved step by step.  HBM per frame in flight: 12 B/px of StitchTool planes + 16 B/px of flows + the solver slab. */
int pf_stitch_step_batch_planned(pf_ctx* ctx, const pf_stitch_plan* plan, int n_frames, const uint8_t* const* l_bgra,
                                 const uint8_t* const* r_bgra, int cols, int rows, size_t step_bytes, int max_percentage,
                                 uint8_t* const* out_bgra, size_t out_step_bytes, int in_flight);
int pf_stitch_step_batch_planned_dev(pf_ctx* ctx, const pf_stitch_plan* plan, int n_frames, const uint8_t* const* d_l,
                                     const uint8_t* const* d_r, int cols, int rows, int max_percentage, uint8_t* const* d_out,
                                     int in_flight);

/* ---- rig plans: the plans of a whole stitch chain from its input masks, and the chain in one call ----
 * The composite of a step has alpha > 0 exactly where its L or its R has, so the R mask of step i of the chain of CPU/main.cpp:60-101 is
 * top | L_1 | .. | L_{i-1}: every step's Map and ramp follow from the n + 1 input masks before a single flow is solved.  A rig plan makes
 * them all at once: ONE kernel pass over the n + 1 images writes the n maps and counts their overlaps, and the n ramps are smoothed as
 * one group (one countblend, one tile-smoothing and one box-blur launch).  n_steps is 1..16; l_bgra holds the n_steps left images in
 * chain order; only alphas are read.  The canvases accepted and refused are pf_stitch_plan_create's, as is everything said there about
 * contexts, handles after destroy (PF_ERR_ARG, looked up before they are dereferenced) and the state creation leaves alone.  A step
 * whose masks do not overlap gets the plan pf_stitch_plan_create makes for those masks (overlap count 0).  5 B/px per step.
 * pf_rig_plan_step hands out step `step` (0-based) as an ordinary pf_stitch_plan for pf_stitch_step_planned, pf_stitch_step_batch_planned*,
 * pf_stitch_plan_info and pf_stitch_plan_download; the rig owns it: pf_stitch_plan_destroy on it is PF_ERR_ARG, pf_rig_plan_destroy (or
 * pf_destroy) frees it.  NULL, with pf_last_error set, for a handle that is not a live rig plan of the context or a step outside it. */
typedef struct pf_rig_plan pf_rig_plan;
int pf_rig_plan_create(pf_ctx* ctx, int n_steps, const uint8_t* top_bgra, const uint8_t* const* l_bgra, int cols, int rows,
                       size_t step_bytes, pf_rig_plan** rig_out);
int pf_rig_plan_create_dev(pf_ctx* ctx, int n_steps, const uint8_t* d_top, const uint8_t* const* d_l, int cols, int rows,
                           pf_rig_plan** rig_out);
int pf_rig_plan_destroy(pf_ctx* ctx, pf_rig_plan* rig);
/* geometry of a LIVE rig plan (outputs may be NULL) */
int pf_rig_plan_info(const pf_rig_plan* rig, int* n_steps, int* cols, int* rows);
const pf_stitch_plan* pf_rig_plan_step(pf_ctx* ctx, const pf_rig_plan* rig, int step);
/* The whole chain of n_frames frames of the rig in one call.  top_bgra[k] and l_bgra[k * n_steps + i] are frame k's inputs (frame-major);
 * out_bgra[k * n_steps + i] receives the bytes pf_stitch_step gives for step i + 1 of frame k's own chain.  out_bgra == NULL or a NULL
 * entry skips that download.
 * Verification first: before any solve every frame's region codes of every step are derived from its n_steps + 1 alphas and compared
 * with the rig's maps.  If any frame is off the rig the call fails with PF_ERR_ARG, pf_last_error names the first such frame, its first
 * differing step (1-based) and the pixel count, nothing is solved, the host form downloads nothing and the device form zero-fills its
 * non-NULL d_out entries.  (The device form verifies all frames in one launch; the host form, whose images pass through the slots of
 * the frames in flight, in one launch per wave.  It keeps two waves' images, so a call of up to 2 x in_flight frames uploads every
 * image once; a longer call uploads the images of its third and later waves twice, the second time on the copy stream while the wave
 * before computes -- pf_rig_set_upload_overlap(ctx, 0) issues that upload between the waves instead; results never depend on it.)
 * Execution: frames go through in waves of `in_flight` (clamped as in pf_stitch_step_batch); a wave runs its steps one after the other
 * as planned batched steps (the launches, lanes and groups of pf_stitch_step_batch_planned).  Synchronous on return.  The call leaves
 * pf_stitch_step's chain state, pf_stitch_prefetch's records and the frame slots of pf_stitch_step_batch alone (pf_stitch_visualize's
 * inputs are invalidated, as by any batched call).
 * HBM is bounded by in_flight, not by n_frames.  Per frame in flight: two composites (8 B/px) + the planned step's 12 B/px of StitchTool
 * planes + 16 B/px of flows + the solver slab; the host form adds the frame's n_steps + 1 inputs (4 (n_steps + 1) B/px), twice that
 * where the call has more than in_flight frames.
 * Device form: only a frame's LAST d_out entry must be non-NULL; a NULL entry keeps that composite in an internal plane (two per frame in
 * flight, ping-ponged: a composite is never written over an input of its own step).  A non-NULL d_out that overlaps any input of the
 * call or another d_out is PF_ERR_ARG; repeated input pointers are allowed.
 * pf_rig_stitch / pf_rig_stitch_dev are these calls with one frame (l and out hold n_steps entries). */
int pf_rig_stitch_batch(pf_ctx* ctx, const pf_rig_plan* rig, int n_frames, const uint8_t* const* top_bgra, const uint8_t* const* l_bgra,
                        int cols, int rows, size_t step_bytes, int max_percentage, uint8_t* const* out_bgra, size_t out_step_bytes,
                        int in_flight);
int pf_rig_stitch_batch_dev(pf_ctx* ctx, const pf_rig_plan* rig, int n_frames, const uint8_t* const* d_top, const uint8_t* const* d_l,
                            int cols, int rows, int max_percentage, uint8_t* const* d_out, int in_flight);
int pf_rig_set_upload_overlap(pf_ctx* ctx, int on);   /* default 1 */
int pf_rig_stitch(pf_ctx* ctx, const pf_rig_plan* rig, const uint8_t* top_bgra, const uint8_t* const* l_bgra, int cols, int rows,
                  size_t step_bytes, int max_percentage, uint8_t* const* out_bgra, size_t out_step_bytes);
int pf_rig_stitch_dev(pf_ctx* ctx, const pf_rig_plan* rig, const uint8_t* d_top, const uint8_t* const* d_l, int cols, int rows,
                      int max_percentage, uint8_t* const* d_out);

/* ---- device-resident entry points (packed buffers already in this context's HBM) -----------
 * Same semantics as above, alignment and aliasing as under "Conventions" (d_out inside d_l, say, is refused: the blend gathers from
 * the images it would be overwriting); used by bench.py (inputs resident when the clock starts) and by the
 * multi-GPU driver.  Pointers are device pointers on the context's device.  The calls are synchronous on
 * return, but they run on the context's own non-blocking streams and do NOT wait for work the caller has
 * in flight on other streams: inputs produced there (e.g. by a framework's kernels) must be complete --
 * synchronise that stream or the device -- before the call. */
void* pf_dev_alloc(pf_ctx* ctx, size_t bytes);
void pf_dev_free(pf_ctx* ctx, void* dptr);
/* Page-locked host memory for images handed to / received from the host-buffer entry points (optional: any host memory works,
 * pinned memory is copied at the link's DMA rate instead of through the runtime's bounce buffers). */
void* pf_host_alloc(pf_ctx* ctx, size_t bytes);
void pf_host_free(pf_ctx* ctx, void* hptr);
int pf_upload(pf_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int pf_download(pf_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int pf_sync(pf_ctx* ctx);
/* 64-bit content checksum of a device buffer (8-byte aligned), computed on the device: compares or verifies results that stay in
 * HBM (e.g. a strip at its producer and after the gather to rank 0) without moving them through the host. */
int pf_checksum_dev(pf_ctx* ctx, const void* d_ptr, size_t bytes, uint64_t* checksum_out);

int pf_flow_bidir_dev(pf_ctx* ctx, const uint8_t* d_l, const uint8_t* d_r, int cols, int rows, int max_percentage,
                      float* d_flow_l2r, float* d_flow_r2l);
int pf_blend_dev(pf_ctx* ctx, const uint8_t* d_l, const uint8_t* d_r, const float* d_flow_l2r, const float* d_flow_r2l,
                 const float* d_blend, int cols, int rows, uint8_t* d_out);
/* flow + blend; the per-pair unit the benchmark times.  d_flow_* may be NULL (flows stay internal). */
int pf_novel_view_dev(pf_ctx* ctx, const uint8_t* d_l, const uint8_t* d_r, int cols, int rows, int max_percentage,
                      const float* d_blend, uint8_t* d_out, float* d_flow_l2r, float* d_flow_r2l);

/* Throughput mode: n_pairs independent pairs of one size, `in_flight` (1..32) of them on this GPU at a time (the exact sweeps of one
 * pair are a dependency chain that occupies ~1/4 of the CUs): batches of pairs that share every kernel launch, on one or more
 * lanes of streams (pf_config::batch_pairs).  Arrays of n_pairs device pointers; d_flow_* may be NULL (or hold NULL entries).
 * Same results as n_pairs calls of pf_novel_view_dev.  Needs GPU_MAX_HW_QUEUES >= 3 * lanes + 2 in the environment before the
 * first HIP call, or the lanes' streams share hardware queues (then pf_last_warning says so). */
int pf_novel_view_batch_dev(pf_ctx* ctx, int n_pairs, const uint8_t* const* d_l, const uint8_t* const* d_r, int cols, int rows,
                            int max_percentage, const float* const* d_blend, uint8_t* const* d_out, float* const* d_flow_l2r,
                            float* const* d_flow_r2l, int in_flight);

/* ---- multi-GPU: the path's only exchange ---------------------------------
 * Overlap pairs are independent units (no state shared between the reference's Stitchtools / NovelViewGenerator objects,
 * CPU/main.cpp:70,82): one rank (process or host thread) + one pf_ctx per GPU, pair i on rank i % world, NO collective
 * on the data path.  What remains is the final gather of the results into rank 0's HBM: grouped ncclSend/ncclRecv over
 * RCCL/xGMI on a stream of its own, so that the gather of pair k overlaps the compute of pair k+1.  RCCL is bound at run
 * time (dlopen): single-GPU users carry no dependency on it.  The reference has no counterpart (it is single-device). */
typedef struct pf_dist pf_dist;
int pf_dist_unique_id(void* id128);                                   /* rank 0: 128-byte ncclUniqueId to hand to every rank */
pf_dist* pf_dist_init(int device, const void* id128, int rank, int world);   /* NULL on failure; pf_dist_last_error(NULL) */
void pf_dist_destroy(pf_dist* d);
const char* pf_dist_last_error(const pf_dist* d);
/* every rank sends `bytes` from d_send; rank 0 receives rank r's block at d_recv_all + r*bytes (d_recv_all ignored elsewhere).
 * Asynchronous; at most one gather in flight (a second call first waits for the previous one). */
int pf_dist_gather_async(pf_dist* d, const void* d_send, void* d_recv_all, size_t bytes);
int pf_dist_wait(pf_dist* d);                                         /* host-blocking: the last gather has completed */
int pf_dist_max(pf_dist* d, double* value_inout);                     /* max over ranks (the job's time is the slowest rank's) */
int pf_dist_barrier(pf_dist* d);

/* ---- stage-level entry points (host buffers, packed) ---------------------------------------
 * One per reference step, so that tests can check every HIP kernel family against the oracle in
 * isolation.  They run the very kernels the entry points above chain together. */
int pf_stage_preprocess(pf_ctx* ctx, const uint8_t* bgra, int cols, int rows, int pad,
                        float* gray_half, float* alpha_half);                         /* PixFlow.hpp:78-103 (+ OpticalFlow.cpp:113-126 when pad>0) */
int pf_stage_pyr_down(pf_ctx* ctx, const float* src, int sw, int sh, float* dst, int dw, int dh);   /* PixFlow.hpp:146-148 */
int pf_stage_gradients(pf_ctx* ctx, const float* img, int w, int h, float* gxy /* (Ix,Iy) interleaved */); /* PixFlow.hpp:281-294 */
int pf_stage_gauss(pf_ctx* ctx, const float* src, int w, int h, int cn, int ksize, double sigma, float* dst); /* GaussianBlur call sites */
int pf_stage_median5(pf_ctx* ctx, const float* flow, int w, int h, float* out);        /* PixFlow.hpp:325,338 */
int pf_stage_sweep(pf_ctx* ctx, const float* g0xy, const float* g1xy, const float* blurred, const float* alpha0,
                   const float* alpha1, float* flow_inout, int w, int h, int forward);  /* PixFlow.hpp:315-324 / :328-337 */
int pf_stage_diffusion(pf_ctx* ctx, const float* alpha0, const float* alpha1, float* flow_inout, int w, int h); /* PixFlow.hpp:388-405 */
int pf_stage_upsample_cubic(pf_ctx* ctx, const float* flow, int sw, int sh, float* out, int dw, int dh, float scale); /* PixFlow.hpp:122-125 */
                                                                      /* PF_ERR_ARG when sh / dh > 1.1875: the kernel upsamples, as every pyramid does */
int pf_stage_final(pf_ctx* ctx, const float* flow, int sw, int sh, int pad_cols, int rows, int pad, float scale,
                   float* out /* (pad_cols-2*pad) x rows */);                          /* PixFlow.hpp:128-134 + OpticalFlow.cpp:143-144 */
int pf_stage_adjust_initial_flow(pf_ctx* ctx, const float* i0, const float* i1, const float* a0, const float* a1, int w, int h,
                                 int hint, int max_percentage, float* flow_out);       /* PixFlow.hpp:226-270 */
int pf_stage_level(pf_ctx* ctx, const float* i0, const float* i1, const float* a0, const float* a1, int w, int h,
                   const float* flow_in /* nullable */, int hint, int max_percentage, float* flow_out); /* PixFlow.hpp:272-340 */
int pf_stage_blend_smooth(pf_ctx* ctx, float* blend_inout, const float* merged_dis, int cols, int rows); /* StitchTool.cpp:130-143 */
/* The tile pass of that smoothing alone (StitchTool.cpp:134-141, without the final rows/400 blur), tile size `step` and window `k` given
 * explicitly: the kernel the stitch entry points run.  form: -1 = the form the library would choose, 0 = window resident in LDS
 * (PF_ERR_ARG if it does not fit), 1 = streamed (any geometry whose window row, step + k - 1 floats, fits that LDS).  PF_ERR_ARG for
 * step < 1, k < 1, step >= min(cols, rows) (no tile), max(k/2, k-1-k/2) >= min(cols, rows), null pointers. */
int pf_stage_tile_blur(pf_ctx* ctx, float* blend_inout, const float* merged_dis, int cols, int rows, int step, int k, int form);
/* The final box blur of that smoothing alone (StitchTool.cpp:142-143: blur(blend, blend, Size(k, k)) with k = rows / 400) with the
 * kernel width k given explicitly, through the launcher the stitch entry points use, on n_batch (1..3) planes laid out as the frames of a
 * batched stitch step are.  src / dst hold n_batch packed cols x rows planes one after the other.  k <= 32 runs the row pass staged
 * through LDS, k > 32 the one that reads straight from memory; k may exceed cols or rows (BORDER_REFLECT_101, reflected as often as
 * needed).  The device planes are filled with 0xFF bytes first: a value read outside a plane comes back as a NaN.
 * PF_ERR_ARG for k < 1, n_batch outside 1..3, cols or rows < 1, null pointers. */
int pf_stage_box_blur(pf_ctx* ctx, int n_batch, const float* src, int cols, int rows, int k, float* dst);
/* Every form of the fused Gaussian 15 (PixFlow.hpp:306-311, :389-403) through the launcher a solve uses, on n_batch (1..3) planes laid
 * out as the slabs of a batched solve are.  Host arrays hold n_batch packed planes one after the other.
 *   PF_G15_PLAIN:       src w x h float2                                  -> dst = GaussianBlur 15, sigma 8
 *   PF_G15_MIX:         src w x h float2, alpha0 / alpha1 w x h           -> dst = lowAlphaFlowDiffusion
 *   PF_G15_UPSAMPLE:    src sw x sh float2 (the coarser level), mul       -> up_out = cubic upsample * mul (w x h), dst = its GaussianBlur
 *   PF_G15_MEDIAN_MIX:  src w x h float2, alpha0 / alpha1                 -> dst = lowAlphaFlowDiffusion of medianBlur 5 of src
 * max_blocks > 0 caps the persistent blocks per plane (a block then walks several tiles); 0 = the library's choice.
 * sw, sh, mul and up_out are only read by PF_G15_UPSAMPLE, the alphas only by the two MIX forms. */
typedef enum pf_gauss15_form { PF_G15_PLAIN = 0, PF_G15_MIX = 1, PF_G15_UPSAMPLE = 2, PF_G15_MEDIAN_MIX = 3 } pf_gauss15_form;
int pf_stage_gauss15_form(pf_ctx* ctx, int form, int n_batch, int max_blocks, const float* src, int sw, int sh, float mul,
                          const float* alpha0, const float* alpha1, int w, int h, float* dst, float* up_out);
/* Gradients (PixFlow.hpp:281-294) and gate + bounding boxes + level-0 count (PixFlow.hpp:317,330) of a whole level table in one launch
 * each, as a solve runs them, for n_batch (1..3) pairs.  ws / hs: n_levels level sizes (each at least 2 x 2, at most 96 levels).  The host
 * inputs hold, per pair, the levels back to back without padding; on the device they lie as in a solve's pyramid plane, level l at
 * off[l], every offset rounded up to 64 elements.  off_out receives off[0..n_levels-1] and the plane size P.
 * The gradients cover plane elements [first, total) (multiples of 4; total 0 = P) with at most max_blocks blocks per image (0 = no cap).
 * Outputs per pair: g0 / g1 = the whole gradient planes (P x float2), gate = the whole gate plane (P bytes) -- what no kernel wrote reads
 * 0xFF bytes -- boxes = (min x, min y, max x, max y) per level as the kernel published them (max < min: nothing gated), count0 = gated
 * pixels of level 0.  One pair uses the context's own work area of the gate kernel, several use slab areas as a batched solve does. */
int pf_stage_level_table(pf_ctx* ctx, int n_levels, const int* ws, const int* hs, int n_batch, const float* img0, const float* img1,
                         const float* alpha0, const float* alpha1, long long first, long long total, int max_blocks, long long* off_out,
                         float* g0, float* g1, uint8_t* gate, int* boxes, int* count0);

/* The head of the pipeline in the forms a solve runs it (tests/test_gpu_front_forms.py): n_batch (1..3) pairs in slabs as a batched solve
 * lays them out (n_batch = 1: the lone form), the slabs filled with 0xFF bytes before the inputs go in.  Host arrays hold the pairs one
 * after the other.  pf_stage_preprocess and pf_stage_preprocess_batch return PF_ERR_ARG for pad < 0 or pad > cols (the kernel wraps a tap
 * of the virtually padded image once) before anything is launched.
 *   preprocess_batch: n_batch BGRA images of one size, each in a device buffer of its own (a caller's, to the kernel) -> per pair the grey
 *     and the alpha half-resolution plane, each as ((w0 * h0 + 63) & ~63) floats: the plane and its padding inside the slab.
 *   pyramid: level0 = per pair the four level-0 planes I0, I1, alpha0, alpha1 (w0 x h0 each) -> the solver's own pyramid loop.
 *     mode 0: one level per launch; 1: the product's rule (by level size); 2 / 3: two / three levels per launch wherever that many are left.
 *     Out: n_levels, ws / hs [n_levels], off [n_levels + 1] (level offsets in a plane and the plane size P, elements), ks [n_launches] =
 *     levels written by each launch, planes = per pair four whole planes of P floats.  cap_levels / cap_plane: what ws / hs / off / ks
 *     and a plane of `planes` hold (PF_ERR_ARG if the pyramid needs more).
 *   adjust_initial_flow_batch: per pair the four planes of one w x h level, flows zero-filled, the ratio scratch in the slab ->
 *     per pair the flow plane as ((2 * w * h + 63) & ~63) floats.
 *   intensity_ratio: k_intensity_ratio (PixFlow.hpp:190-205) on n elements per pair -> one ratio per pair. */
int pf_stage_preprocess_batch(pf_ctx* ctx, int n_batch, const uint8_t* bgra, int cols, int rows, int pad, float* gray_half, float* alpha_half);
int pf_stage_pyramid(pf_ctx* ctx, int n_batch, int mode, const float* level0, int w0, int h0, int cap_levels, long long cap_plane,
                     int* n_levels, int* ws, int* hs, long long* off, int* ks, int* n_launches, float* planes);
int pf_stage_adjust_initial_flow_batch(pf_ctx* ctx, int n_batch, const float* i0, const float* i1, const float* a0, const float* a1,
                                       int w, int h, int hint, int max_percentage, float* flow_out);
int pf_stage_intensity_ratio(pf_ctx* ctx, int n_batch, const float* i0, const float* i1, const float* a0, const float* a1, int n, float* ratio_out);

/* ---- flow visualisation ---------------------------------------------------------------------
 * The reference's debugging views of a flow (CPU/OpticalFlow.cpp:147-204, declared in CPU/OpticalFlow.hpp:72-76), byte for byte,
 * on the device.  The reference computes them with OpenCV 3.2 on the host; here they are restated kernels:
 *   grey disparity  visualizeFlowAsGreyDisparity (:147-158): flow.x through normalize(0, 255, NORM_MINMAX) and convertTo(CV_8U);
 *   colour wheel    visualizeFlowColorWheel (:185-204): hue = flow direction, value = magnitude / (max(cols, rows) / 20), HSV2BGR;
 *   vector field    visualizeFlowAsVectorField (:160-183): a copy of the image with an anti-aliased black arrow line (LineAA) from
 *                   every grid point 12 <= x < cols - 12, 12 <= y < rows - 12, x, y multiples of 12, drawn in row-major order;
 *   panel           the strip buildvisualizations (CPU/main.cpp:20-45) writes per direction: [GRAY2BGRA(grey) | BGR2BGRA(wheel) |
 *                   vector field], BGRA, 3 * cols x rows.
 * A flow with a non-finite component is PF_ERR_ARG (the reference's result there depends on OpenCV's SIMD internals and on undefined
 * float -> uchar conversions); a zero vector is finite (hue byte 0, the reference's x86-64 result for its 0 / 0 direction). */
int pf_vis_grey_disparity(pf_ctx* ctx, const float* flow, size_t flow_step, int cols, int rows, uint8_t* out, size_t out_step);        /* CV_8UC1 */
int pf_vis_color_wheel(pf_ctx* ctx, const float* flow, size_t flow_step, int cols, int rows, uint8_t* out_bgr, size_t out_step);       /* CV_8UC3 */
int pf_vis_vector_field(pf_ctx* ctx, const float* flow, size_t flow_step, const uint8_t* image_bgra, size_t image_step,
                        int cols, int rows, uint8_t* out_bgra, size_t out_step);                                                  /* CV_8UC4 */
int pf_vis_panel(pf_ctx* ctx, const float* flow, size_t flow_step, const uint8_t* image_bgra, size_t image_step,
                 int cols, int rows, uint8_t* out_bgra /* 3*cols x rows */, size_t out_step);
/* the same on device pointers of this context's device, all packed (d_out: 3 * cols * 4 bytes per row) */
int pf_vis_panel_dev(pf_ctx* ctx, const float* d_flow, const uint8_t* d_image, int cols, int rows, uint8_t* d_out);
/* The two panels (L->R over the step's L input, R->L over its R input: the arguments of the reference's commented-out
 * buildvisualizations call, CPU/main.cpp:85) of the LAST pf_stitch_step on this context, from the flows and inputs still in HBM;
 * either output may be NULL.  pf_stitch_step itself does no extra work for this.  PF_ERR_ARG if no step has run or a later call
 * has reused those buffers (any solve: pf_flow*, pf_novel_view*, the throughput mode, a failed step). */
int pf_stitch_visualize(pf_ctx* ctx, uint8_t* l2r_panel, uint8_t* r2l_panel, size_t step);

/* ---- PNG files made on the device -------------------------------------------------------------
 * An 8-bit RGBA PNG (colour type 6, no interlace) of a packed BGRA image, of any size pf_blend accepts and any width (the
 * 3 * cols panels of pf_vis_panel_dev included).  Scanline filtering (per row the filter type with the smallest sum of absolute
 * residuals), deflate and compaction run in kernels on the device; only the finished stream crosses the link, into its place in
 * png_out (HOST memory), where the library frames it (its own CRC-32 and Adler-32: no zlib).  Opt-in: no other entry point's
 * behaviour depends on these.  The deflate stream: the filtered scanlines in segments of pf_png_segment_bytes()
 * bytes, each compressed on its own into dynamic-Huffman blocks with run matches (the byte 1 or 4 back, lengths up to 258) or, where
 * that would not shrink it, a stored block; each segment ends on a byte boundary with an empty stored block.  The bytes are a
 * function of the image alone.
 *   cap       bytes png_out holds.  A file larger than cap is PF_ERR_ARG: nothing is written and *size_out receives the size
 *             needed (the batch form: cap_each per file, every sizes_out[k] set).  pf_png_bound(cols, rows) always suffices.
 *   _dev      d_bgra: device pointers of this context's device, packed rows, 4-byte aligned.
 *   batch     n same-size images -> the bytes of n single calls, their kernels enqueued together.
 * pf_stitch_result_png encodes the composite the last pf_stitch_step / pf_stitch_step_planned left in HBM (the one a step with
 * r_bgra == NULL chains on), pf_stitch_batch_result_png frame slot `frame` of the last host-form pf_stitch_step_batch* call; both
 * return PF_ERR_ARG where there is none, and neither changes the chain, the prefetch records, the frame slots or what
 * pf_stitch_visualize reads.  A step may therefore pass out_bgra == NULL and bring down only the file. */
size_t pf_png_bound(int cols, int rows);
size_t pf_png_segment_bytes(void);
int pf_png_encode_dev(pf_ctx* ctx, const uint8_t* d_bgra, int cols, int rows, uint8_t* png_out, size_t cap, size_t* size_out);
int pf_png_encode(pf_ctx* ctx, const uint8_t* bgra, size_t step_bytes, int cols, int rows, uint8_t* png_out, size_t cap, size_t* size_out);
int pf_png_encode_batch_dev(pf_ctx* ctx, int n, const uint8_t* const* d_bgra, int cols, int rows, uint8_t* const* png_out, size_t cap_each,
                            size_t* sizes_out);
int pf_stitch_result_png(pf_ctx* ctx, uint8_t* png_out, size_t cap, size_t* size_out);
int pf_stitch_batch_result_png(pf_ctx* ctx, int frame, uint8_t* png_out, size_t cap, size_t* size_out);

/* ---- JPEG files made on the device ------------------------------------------------------------
 * A baseline sequential JPEG (SOF0, 8 bits, Y Cb Cr, JFIF 1.01, Annex K's Huffman tables) of a packed BGRA image; alpha is dropped
 * and the colour bytes are encoded as stored.  Any size pf_png_encode_dev accepts up to the format's 65535 a side, any width (the
 * 3 * cols panels included).  The colour transform, libjpeg's integer DCT, quantisation and the entropy coder run in kernels on the
 * device; only the finished entropy-coded segment crosses the link, into its place in jpg_out (HOST memory) behind
 * the header the library writes.  Opt-in: no other entry point's behaviour depends on these.  The bytes are a function of the image
 * and the three parameters alone, and with gpano == 0 they are the file libjpeg writes for that image at that quality and
 * subsampling with a restart interval of pf_jpeg_restart_interval(subsampling) MCUs.
 *   params    NULL: the defaults pf_jpeg_params_init sets.  quality 1..100 (default 90); subsampling 0 = 4:4:4, 1 = 4:2:0
 *             (default); gpano 1: an APP1 segment directly behind APP0 holds an XMP packet that declares the image a full
 *             equirectangular sphere (GPano:ProjectionType, UsePanoramaViewer, the full and cropped sizes = the image's, left and top
 *             0), for which the image must be 2:1 -- removing that segment gives the gpano == 0 file exactly.  Anything else is
 *             PF_ERR_ARG, as is a side above 65535.
 *   cap       bytes jpg_out holds.  A file larger than cap is PF_ERR_ARG: nothing is written and *size_out receives the size
 *             needed (the batch form: cap_each per file, every sizes_out[k] set).  pf_jpeg_bound(cols, rows, params) always suffices
 *             (it is a worst case, about 20 bytes per pixel at 4:4:4; 0 for a shape or subsampling the encoder refuses).
 *   _dev, batch, pf_stitch_result_jpeg, pf_stitch_batch_result_jpeg: as the PNG family's. */
typedef struct pf_jpeg_params {
  int struct_size;   /* sizeof(pf_jpeg_params), set by pf_jpeg_params_init */
  int quality;
  int subsampling;
  int gpano;
} pf_jpeg_params;
void pf_jpeg_params_init(pf_jpeg_params* params);
size_t pf_jpeg_bound(int cols, int rows, const pf_jpeg_params* params);
int pf_jpeg_restart_interval(int subsampling);   /* MCUs per restart interval; 0 for an unknown subsampling */
int pf_jpeg_encode_dev(pf_ctx* ctx, const uint8_t* d_bgra, int cols, int rows, const pf_jpeg_params* params, uint8_t* jpg_out, size_t cap, size_t* size_out);
int pf_jpeg_encode(pf_ctx* ctx, const uint8_t* bgra, size_t step_bytes, int cols, int rows, const pf_jpeg_params* params, uint8_t* jpg_out, size_t cap,
                   size_t* size_out);
int pf_jpeg_encode_batch_dev(pf_ctx* ctx, int n, const uint8_t* const* d_bgra, int cols, int rows, const pf_jpeg_params* params, uint8_t* const* jpg_out,
                             size_t cap_each, size_t* sizes_out);
int pf_stitch_result_jpeg(pf_ctx* ctx, const pf_jpeg_params* params, uint8_t* jpg_out, size_t cap, size_t* size_out);
int pf_stitch_batch_result_jpeg(pf_ctx* ctx, int frame, const pf_jpeg_params* params, uint8_t* jpg_out, size_t cap, size_t* size_out);

/* ---- TIFF files decoded on the device ----------------------------------------------------------
 * The counterpart of the PNG encoder: the bytes of a TIFF file (HOST memory) go up as they are, the strips decode in parallel on the
 * device (one workgroup per strip: LZW -- compression 5 -- and PackBits -- 32773 --; uncompressed strips are read in place), the
 * predictor (2 = horizontal differencing) is undone per row and the pixels are stored as packed BGRA, alpha 255 for RGB files: what
 * cv::imread(-1) + BGR->BGRA delivers.  Opt-in: no other entry point's behaviour depends on these.
 * Accepted: the first IFD of a little- or big-endian classic TIFF with 8-bit chunky RGB / RGBA strips.  Tiles, 16-bit, palette and
 * planar files, FillOrder 2, an inconsistent strip table, a strip that does not lie inside the file and images over 4e9 pixels are
 * refused with a message; a hostile IFD cannot cause a read outside `file`.
 *   pf_tiff_probe   host only, needs no device; ctx may be NULL (pf_last_error(ctx) / pf_last_error(NULL) explains a refusal).
 *                   out->struct_size must be set to sizeof(pf_tiff_info).  device_decodable means "with default settings": it
 *                   is 0 for deflate files (compression 8 / 32946), which the decode calls refuse with PF_ERR_ARG by default:
 *                   use a host reader for them, or the switch below.
 *   pf_tiff_set_inflate   on != 0: this context's decode calls also take deflate files -- every strip one zlib stream, stored,
 *                   fixed and dynamic blocks, predictor 1 or 2 -- alone or mixed with the other classes in a batch.  Default 0:
 *                   deflate files are refused as before.  A deflate strip is accepted exactly when zlib's own
 *                   uncompress(dst, expected bytes, strip) returns Z_OK or Z_BUF_ERROR with all expected bytes delivered (an
 *                   over-long stream is clipped; a wrong Adler-32 or any malformed block refuses the file, as below).
 *   pf_tiff_device_decodable   1 / 0: would this context's decode calls take the probed file?  ctx == NULL: the defaults, i.e.
 *                   the probe's own field.  Host only.
 *   cols, rows      what the caller expects, as learned from the probe; a file of another size is PF_ERR_ARG before any work.
 *   _dev            d_out_bgra: device memory of this context's device, cols * rows * 4 bytes, packed rows, 4-byte aligned.
 *   pf_tiff_decode  delivers to HOST memory with a row step of out_step bytes; bytes of a row beyond cols * 4 are left untouched.
 *   batch           n same-size files -> the bytes of n single calls, their kernels enqueued together before one drain.
 * A strip whose stream is malformed or ends before the strip's rows are filled fails the call with PF_ERR_ARG; pf_last_error names
 * the first such strip and how many of its bytes decoded.  The device forms then zero-fill their outputs (all of them, in the batch
 * form) and the host form writes nothing.  This differs from the drop-in CLI's host reader (tools/image_io.hpp read_tiff), which
 * zero-fills the rest of a short strip silently and returns the image: the device path refuses the file.
 * The scratch is the decoder's own: these calls leave alone the chain state, the prefetch records, the frame slots, the plans and
 * what pf_stitch_visualize reads.  Kernel families in pf_profile_*: tiff_lzw, tiff_packbits, tiff_inflate, tiff_finish. */
typedef struct pf_tiff_info {
  int struct_size, cols, rows, samples, compression, predictor, rows_per_strip, n_strips, big_endian, device_decodable;
} pf_tiff_info;
int pf_tiff_probe(pf_ctx* ctx, const uint8_t* file, size_t bytes, pf_tiff_info* out);
int pf_tiff_set_inflate(pf_ctx* ctx, int on);            /* default 0 */
int pf_tiff_device_decodable(const pf_ctx* ctx, const pf_tiff_info* info);   /* 1 / 0; ctx == NULL: the defaults */
int pf_tiff_decode_dev(pf_ctx* ctx, const uint8_t* file, size_t bytes, int cols, int rows, uint8_t* d_out_bgra);
int pf_tiff_decode(pf_ctx* ctx, const uint8_t* file, size_t bytes, int cols, int rows, uint8_t* out_bgra, size_t out_step);
int pf_tiff_decode_batch_dev(pf_ctx* ctx, int n, const uint8_t* const* files, const size_t* bytes, int cols, int rows,
                             uint8_t* const* d_out_bgra);

/* ---- JPEG files decoded on the device -------------------------------------------------------
 * The counterpart of the JPEG encoder: the bytes of a baseline JPEG file (HOST memory) go up as they are and come out as packed
 * BGRA, alpha 255, byte for byte Pillow's Image.open(file).convert("RGB") (libjpeg-turbo's integer IDCT, fancy upsampling and colour
 * transform); grey files give B = G = R = Y.  The scan's one Huffman stream is decoded in parallel by self-synchronising lanes over
 * subsequences of the entropy segment, so files without restart markers decode in parallel, too.  Opt-in: no other
 * entry point's behaviour depends on these.
 * Accepted, checked on the host before any device work: baseline SOF0, 8-bit samples, 8-bit quantisation tables, Huffman tables 0..3,
 * one component or Y Cb Cr with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1, one interleaved scan, any restart interval, sides up to
 * 65535.  APPn and COM segments are skipped; EXIF orientation and ICC profiles are ignored.  Everything else -- progressive, extended,
 * lossless and arithmetic frames, 12-bit samples, four components, other samplings, several scans, DNL, a file libjpeg would read as
 * RGB, a Huffman table libjpeg refuses, a missing table, another size than the caller expects -- is PF_ERR_ARG with the reason.
 *   pf_jpeg_probe   host only, needs no device; ctx may be NULL.  out->struct_size must be set to sizeof(pf_jpeg_info).  PF_OK for
 *                   anything that begins as a JPEG: device_decodable says whether the decode calls take it, `reason` why not (cols,
 *                   rows and components are then what the frame header gave, 0 where it was not reached).  subsampling: 0 grey,
 *                   444, 422 or 420.
 *   cols, rows      what the caller expects, as learned from the probe; a file of another size is PF_ERR_ARG before any work.
 *   _dev            d_out_bgra: device memory of this context's device, cols * rows * 4 bytes, packed rows, 4-byte aligned.
 *   pf_jpeg_decode  delivers to HOST memory with a row step of out_step bytes; bytes of a row beyond cols * 4 are left untouched.
 *   batch           n same-size files, which may differ in tables, subsampling and interval -> the bytes of n single calls; every
 *                   step's kernels of all files are enqueued before the step's one drain.  Outputs must not overlap.
 * A scan is accepted exactly when its decode meets no event: every code valid, every run inside its block, every restart interval
 * holding exactly its MCUs and followed by its own RSTn, the last by EOI after at most 7 pad bits.  libjpeg tolerates such events
 * with a warning; the device path refuses the file with PF_ERR_ARG, pf_last_error names the file and the MCU where decoding stopped,
 * the device forms zero-fill their outputs (all of them, in the batch form) and the host form writes nothing.  IDCT outputs beyond
 * libjpeg's range table are clamped to 0..255.  A synchronisation that does not settle within its bound of launches (never expected) is
 * PF_ERR_DEVICE and zero-fills the device outputs, too.
 *   pf_stage_jpeg_decode   the stage hook for the tests: one file decoded as above; states_out receives every subsequence's final
 *                   exit state (4 words each: bit, block in MCU | zigzag index << 8, blocks completed, markers crossed; subsequence
 *                   i enters where i - 1 left), coef_out the coefficient plane (64 int16 per block in MCU order, zigzag order, DC
 *                   summed), planes_out the component planes (Y, then Cb and Cr, at their block-padded sizes); the caps are in bytes.
 *                   counts_out: [0] subsequences, [1] rounds, [2] launches to the fixed point, [3] the subsequence size,
 *                   [4] subsequences whose exit state changed after their first walk (one that changed in two launches counts twice).
 * The scratch is the decoder's own: these calls leave alone the chain state, the prefetch records, the frame slots, the plans and
 * every other family's scratch.  Kernel families in pf_profile_*: jpegd_sync, jpegd_write, jpegd_pixels. */
typedef struct pf_jpeg_info {
  int struct_size, cols, rows, components, subsampling, restart_interval, device_decodable;
  char reason[128];
} pf_jpeg_info;
int pf_jpeg_probe(pf_ctx* ctx, const uint8_t* file, size_t bytes, pf_jpeg_info* out);
int pf_jpeg_decode_dev(pf_ctx* ctx, const uint8_t* file, size_t bytes, int cols, int rows, uint8_t* d_out_bgra);
int pf_jpeg_decode(pf_ctx* ctx, const uint8_t* file, size_t bytes, int cols, int rows, uint8_t* out_bgra, size_t out_step);
int pf_jpeg_decode_batch_dev(pf_ctx* ctx, int n, const uint8_t* const* files, const size_t* bytes, int cols, int rows,
                             uint8_t* const* d_out_bgra);
int pf_stage_jpeg_decode(pf_ctx* ctx, const uint8_t* file, size_t bytes, uint32_t* states_out, size_t states_cap, int16_t* coef_out,
                         size_t coef_cap, uint8_t* planes_out, size_t planes_cap, int* counts_out);

/* ---- Resize on the device --------------------------------------------------------------------
 * A packed BGRA image at another size, byte for byte what Pillow's Image.resize(size, filter) gives for the same bytes as an RGBA
 * image (the three colour channels are treated alike, so the channel order does not matter): an antialiased separable resample --
 * horizontal pass, then vertical -- in 22-bit fixed point, over colour premultiplied by alpha and divided by it again at the end,
 * so that transparent pixels do not bleed their colour into their neighbours.  An axis whose size stays runs no
 * pass; out_cols == cols && out_rows == rows is a plain copy.  The coefficient tables are made on the host in double (HAMMING and
 * LANCZOS through the host's sin / cos: their bytes are scoped to this libm, as the blend's are), kept in the context per (in, out,
 * filter) and uploaded; the kernels are integer only.  Opt-in: no other entry point's behaviour depends on these.  A result stays
 * in HBM between the stitch and pf_png_encode_dev / pf_jpeg_encode_dev: chain them.
 *   filter    one of PF_RESIZE_* (Pillow's numbering); anything else is PF_ERR_ARG.
 *   _dev      d_src_bgra: cols * rows * 4 bytes, d_dst_bgra: out_cols * out_rows * 4 bytes of this context's device, packed rows,
 *             4-byte aligned.  A destination that overlaps a source is PF_ERR_ARG.
 *   pf_resize HOST memory on both sides, row steps in bytes; bytes of a destination row beyond out_cols * 4 are left untouched.
 *   batch     n same-size images -> the bytes of n single calls, their kernels enqueued together before one drain.
 *   pf_stitch_result_resized_dev, pf_stitch_batch_result_resized_dev: from the composite the last pf_stitch_step left in HBM, or
 *             frame slot `frame` of the last pf_stitch_step_batch; PF_ERR_ARG when none is resident, as pf_stitch_result_png.
 * PF_ERR_ARG with a message also for: null pointers; sizes <= 0; more than 2e9 pixels on either side (or in the intermediate
 * out_cols x rows plane); an axis whose table exceeds 16 777 216 coefficients, where the table of an axis holds
 * (2 * ceil(support * max(in / out, 1)) + 1) * out of them (support: 3, 1, 2, 0.5, 1 in the order below) -- every axis up to 2.7
 * million source or 2.3 million output samples fits.
 * The scratch is the resize's own: these calls leave alone the chain state, the prefetch records, the frame slots, the plans and
 * what pf_stitch_visualize reads.  Kernel families in pf_profile_*: resize_h, resize_v. */
enum { PF_RESIZE_LANCZOS = 1, PF_RESIZE_BILINEAR = 2, PF_RESIZE_BICUBIC = 3, PF_RESIZE_BOX = 4, PF_RESIZE_HAMMING = 5 };
int pf_resize_dev(pf_ctx* ctx, const uint8_t* d_src_bgra, int cols, int rows, uint8_t* d_dst_bgra, int out_cols, int out_rows, int filter);
int pf_resize(pf_ctx* ctx, const uint8_t* src_bgra, size_t src_step, int cols, int rows, uint8_t* dst_bgra, size_t dst_step, int out_cols, int out_rows,
              int filter);
int pf_resize_batch_dev(pf_ctx* ctx, int n, const uint8_t* const* d_src_bgra, int cols, int rows, uint8_t* const* d_dst_bgra, int out_cols, int out_rows,
                        int filter);
int pf_stitch_result_resized_dev(pf_ctx* ctx, int out_cols, int out_rows, int filter, uint8_t* d_dst_bgra);
int pf_stitch_batch_result_resized_dev(pf_ctx* ctx, int frame, int out_cols, int out_rows, int filter, uint8_t* d_dst_bgra);
/* Stage entry (tests): ONE pass of the resize on packed HOST images, exactly one launch of the horizontal (axis 0: cols -> n_out
 * columns, dst n_out x rows) or the vertical kernel (axis 1: rows -> n_out rows, dst cols x n_out) with the library's own table of
 * that axis and the two fusions as given: premul != 0 premultiplies what the pass loads, unpremul != 0 divides what it stores.
 * An n_out equal to the axis still runs the pass.  Refuses what pf_resize refuses, and an axis other than 0 or 1. */
int pf_stage_resize_pass(pf_ctx* ctx, const uint8_t* src_bgra, int cols, int rows, int axis, int n_out, int filter, int premul, int unpremul,
                         uint8_t* dst_bgra);

/* ---- Reprojection on the device --------------------------------------------------------------
 * A packed BGRA equirectangular sphere in HBM -> a cube face, a rectilinear view, or the sphere turned (re-levelled), without the
 * image leaving the device.  For every output pixel: a ray, rotated by `rot`, its longitude and latitude, the source
 * position, quantised to 1/256 pixel, and a bilinear (2 x 2) or Catmull-Rom (4 x 4) sample in integer arithmetic over colour
 * premultiplied by alpha (as pf_resize premultiplies) and divided by it again.  The geometry is fp64 add, subtract, multiply, divide
 * and sqrt with a polynomial arctangent, in a fixed order: the bytes are a function of the image, the sizes and the parameters.
 *   frame     right-handed: x forward (the source's centre column), y to the right (increasing columns), z up.
 *   source    cols x rows, 360 degrees across with square angular pixels, centred on the horizon: rows * 360 / cols degrees tall.
 *             Columns wrap, rows clamp; a ray beyond half a pixel past the first or last row gives four zero bytes.
 *   PF_PROJ_CUBE         out_cols == out_rows; face = PF_FACE_*.  The up face's bottom edge and the down face's top edge meet the front face.
 *   PF_PROJ_RECTILINEAR  a view along +x of hfov_deg degrees across (0 < hfov_deg < 180), square pixels.
 *   PF_PROJ_EQUIRECT     a sphere of out_cols x out_rows with the source's conventions: with a rotation, the source re-levelled.
 *   rot       s = rot * d, row-major, passed as it is (it need not be a rotation).  pf_reproject_rotation makes
 *             Rz(yaw) Ry(-pitch) Rx(roll) with the host's sin / cos: yaw turns the view to the right, pitch up, roll lifts its right side.
 *   _dev      d_src_bgra: cols * rows * 4 bytes, d_dst_bgra: out_cols * out_rows * 4 bytes of this context's device, packed rows,
 *             4-byte aligned.
 *   pf_reproject  HOST memory on both sides, row steps in bytes; bytes of a destination row beyond out_cols * 4 are left untouched.
 *   batch     n same-size images, one set of parameters -> the bytes of n single calls, their kernels enqueued together before one drain.
 *   pf_reproject_cube_dev  the six faces (PF_FACE_* order) of face_size x face_size into six destinations, one launch; params'
 *             projection and face are not read.
 *   pf_stitch_result_reprojected_dev, pf_stitch_batch_result_reprojected_dev: from the composite the last pf_stitch_step left in
 *             HBM, or frame slot `frame` of the last pf_stitch_step_batch; PF_ERR_ARG when none is resident, as pf_stitch_result_png.
 *   pf_stage_reproject_coords  the quantised source coordinates (256 * position, rounded) of every output pixel as the device
 *             computes them: two int32 planes of out_cols x out_rows in host memory.
 * There is no antialiasing: an output that samples the source more coarsely than about one source pixel per output pixel aliases.
 * Make a face of about cols / 4 (or any view near the source's scale) and shrink it with pf_resize_dev.  A result stays in HBM for
 * pf_resize_dev, pf_png_encode_dev and pf_jpeg_encode_dev: chain them.  Opt-in: no other entry point's behaviour depends on these.
 * PF_ERR_ARG with a message, before any device work, for: null pointers; sizes <= 0 or a side above 65535; more than 2e9 pixels
 * on either side; an unknown projection, face (cube) or filter; a cube with out_cols != out_rows; hfov_deg outside (0, 180)
 * (rectilinear); a non-finite entry of rot; a destination that overlaps a source.
 * The scratch is the reprojection's own: these calls leave alone the chain state, the prefetch records, the frame slots, the plans
 * and what pf_stitch_visualize reads.  Kernel family in pf_profile_*: reproject. */
enum { PF_PROJ_CUBE = 0, PF_PROJ_RECTILINEAR = 1, PF_PROJ_EQUIRECT = 2 };
enum { PF_FACE_FRONT = 0, PF_FACE_RIGHT = 1, PF_FACE_BACK = 2, PF_FACE_LEFT = 3, PF_FACE_UP = 4, PF_FACE_DOWN = 5 };
enum { PF_REPROJECT_BILINEAR = 2, PF_REPROJECT_BICUBIC = 3 };   /* PF_RESIZE_*'s numbers */
typedef struct pf_reproject_params {
  int projection;   /* PF_PROJ_* */
  int face;         /* cube only */
  int filter;       /* PF_REPROJECT_* */
  double hfov_deg;  /* rectilinear only */
  double rot[9];
} pf_reproject_params;
void pf_reproject_params_init(pf_reproject_params* params);   /* the front face, bicubic, hfov 90, the identity rotation */
void pf_reproject_rotation(double yaw_deg, double pitch_deg, double roll_deg, double* rot_out /* 9 */);   /* host only */
int pf_reproject_dev(pf_ctx* ctx, const uint8_t* d_src_bgra, int cols, int rows, uint8_t* d_dst_bgra, int out_cols, int out_rows,
                     const pf_reproject_params* params);
int pf_reproject(pf_ctx* ctx, const uint8_t* src_bgra, size_t src_step, int cols, int rows, uint8_t* dst_bgra, size_t dst_step, int out_cols, int out_rows,
                 const pf_reproject_params* params);
int pf_reproject_batch_dev(pf_ctx* ctx, int n, const uint8_t* const* d_src_bgra, int cols, int rows, uint8_t* const* d_dst_bgra, int out_cols, int out_rows,
                           const pf_reproject_params* params);
int pf_reproject_cube_dev(pf_ctx* ctx, const uint8_t* d_src_bgra, int cols, int rows, uint8_t* const* d_faces_bgra /* 6 */, int face_size,
                          const pf_reproject_params* params);
int pf_stitch_result_reprojected_dev(pf_ctx* ctx, int out_cols, int out_rows, const pf_reproject_params* params, uint8_t* d_dst_bgra);
int pf_stitch_batch_result_reprojected_dev(pf_ctx* ctx, int frame, int out_cols, int out_rows, const pf_reproject_params* params, uint8_t* d_dst_bgra);
int pf_stage_reproject_coords(pf_ctx* ctx, int cols, int rows, int out_cols, int out_rows, const pf_reproject_params* params, int32_t* fx_out, int32_t* fy_out);

/* ---- Lens remap on the device ------------------------------------------------------------------
 * Raw photos of a camera rig in HBM -> each camera's equirectangular canvas, the warp the stitcher's inputs have been through
 * (DESIGN.md 8.7): the inverse of the reprojection above.  For every canvas pixel: its ray, rotated into the camera by `rot`, the
 * lens model's radius, the radial polynomial, the position in the photo, quantised to 1/256 pixel, and the reprojection's bilinear
 * or Catmull-Rom sample over premultiplied colour (a photo's alpha channel, its mask, is kept).  The geometry is fp64 add, subtract,
 * multiply, divide and sqrt with the reprojection's polynomial arctangent, in a fixed order: the bytes are a function of the photo,
 * the sizes and the lens.
 *   canvas    cols x rows BGRA with the reprojection's source conventions: 360 degrees across, square angular pixels, centred on
 *             the horizon; frame x forward, y right, z up.
 *   camera    c = rot * d, row-major, used as passed.  The optical axis is +x, image right +y, image up +z.  A camera posed by
 *             pf_reproject_rotation(yaw, pitch, roll) = R takes rot = R transposed: pf_lens_rotation writes that.
 *   outside   four zero bytes: |c| == 0; c.x <= min_cos * |c| (pf_lens_init: 0 for rectilinear, -0.5 for the fisheyes); for the
 *             stereographic and equisolid models |c| + c.x <= 0; a position that is no number within +-1e9; a position more than
 *             half a pixel off the photo; with crop_r256 > 0 a position outside the circle (crop_cx256, crop_cy256, crop_r256),
 *             integers in 1/256 pixel: the image circle of a circular fisheye.  Taps clamp to the photo in both axes.
 *   model     the ideal radius r = focal_px * g with rho = sqrt(c.y^2 + c.z^2), n = |c|:
 *             PF_LENS_RECTILINEAR rho / c.x;  PF_LENS_FISHEYE_EQUIDISTANT atan2(rho, c.x);
 *             PF_LENS_FISHEYE_STEREOGRAPHIC 2 rho / (n + c.x);  PF_LENS_FISHEYE_EQUISOLID 2 rho / sqrt(2 n (n + c.x)).
 *             pf_lens_focal makes focal_px from the photo's width and its horizontal field of view in degrees (host libm).
 *   polynomial  the panotools convention, applied canvas -> photo: rn = r / (min(photo_cols, photo_rows) / 2),
 *             r_src = r * (((a rn + b) rn + c) rn + dd); pf_lens_init sets a = b = c = 0 and dd = 1.
 *   position  px = photo_cols / 2 - 1/2 + shift_x + (r_src / rho) c.y,  py = photo_rows / 2 - 1/2 + shift_y - (r_src / rho) c.z.
 *   _dev      d_photo: photo_cols * photo_rows * 4 bytes, d_canvas: cols * rows * 4 bytes of this context's device, packed rows,
 *             4-byte aligned.
 *   pf_lens_remap  HOST memory on both sides, row steps in bytes; bytes of a canvas row beyond cols * 4 are left untouched.
 *   batch     n same-size photos -> n same-size canvases, image k under lenses[k] (its filter included): the bytes of n single
 *             calls, up to 16 images per launch, one drain.  A rig's photos become its canvases in one launch.
 *   pf_stage_lens_coords  the quantised photo coordinates (256 * position, rounded) of every canvas pixel as the device computes
 *             them, two int32 planes of cols x rows in host memory; a pixel with no position has fx = 0, fy = INT32_MIN.
 * There is no antialiasing: use a canvas near the photo's angular resolution.  No vignetting, exposure or white-balance correction,
 * no tangential or shear terms.  Opt-in: no other entry point's behaviour depends on these.
 * PF_ERR_ARG with a message, before any device work, for: null pointers; sizes <= 0 or a side above 65535; more than 2e9 pixels on
 * either side; an unknown model or filter; a focal_px, polynomial coefficient, shift, min_cos or rot entry that is not finite;
 * focal_px <= 0; min_cos outside [-1, 1), or below 0 for rectilinear; a negative crop_r256; a canvas that overlaps a photo; device
 * pointers that are not 4-byte aligned.
 * The scratch is the remap's own: these calls leave alone the chain state, the frame slots, the plans and the reprojection's
 * scratch.  Kernel family in pf_profile_*: lens. */
enum { PF_LENS_RECTILINEAR = 0, PF_LENS_FISHEYE_EQUIDISTANT = 1, PF_LENS_FISHEYE_STEREOGRAPHIC = 2, PF_LENS_FISHEYE_EQUISOLID = 3 };
typedef struct pf_lens {
  int model;    /* PF_LENS_* */
  int filter;   /* PF_REPROJECT_* */
  double focal_px, a, b, c, dd, shift_x, shift_y, min_cos;
  int crop_cx256, crop_cy256, crop_r256;
  double rot[9];
} pf_lens;
void pf_lens_init(pf_lens* lens, int model);   /* bicubic, dd = 1, the model's min_cos, the identity rotation; focal_px = 0: set it (pf_lens_focal) */
double pf_lens_focal(int model, int photo_cols, double hfov_deg);   /* host only; 0 for an unknown model */
void pf_lens_rotation(double yaw_deg, double pitch_deg, double roll_deg, double* rot_out /* 9 */);   /* host only */
int pf_lens_remap_dev(pf_ctx* ctx, const uint8_t* d_photo_bgra, int photo_cols, int photo_rows, uint8_t* d_canvas_bgra, int cols, int rows, const pf_lens* lens);
int pf_lens_remap(pf_ctx* ctx, const uint8_t* photo_bgra, size_t photo_step, int photo_cols, int photo_rows, uint8_t* canvas_bgra, size_t canvas_step, int cols, int rows,
                  const pf_lens* lens);
int pf_lens_remap_batch_dev(pf_ctx* ctx, int n, const uint8_t* const* d_photos_bgra, int photo_cols, int photo_rows, uint8_t* const* d_canvases_bgra, int cols, int rows,
                            const pf_lens* lenses /* n */);
int pf_stage_lens_coords(pf_ctx* ctx, int photo_cols, int photo_rows, int cols, int rows, const pf_lens* lens, int32_t* fx_out, int32_t* fy_out);

/* ---- per-kernel-family timing (HIP events on the streams the kernels run on) ---------------- */
int pf_profile_enable(pf_ctx* ctx, int on);   /* 0 off, 1 all kernel families, 2 only the sweep kernels */
int pf_profile_reset(pf_ctx* ctx);
int pf_profile_count(pf_ctx* ctx);                                       /* number of kernel families seen */
int pf_profile_get(pf_ctx* ctx, int idx, char* name, int name_cap, double* total_ms, int* launches);
/* algorithmic HBM bytes of one pf_novel_view on cols x rows (SURVEY.md section 8(d) model) */
double pf_algorithmic_bytes(int cols, int rows);
long long pf_level_pixels(int cols, int rows, int* n_levels, long long* sweep_steps);
/* dependent wavefront steps of ONE direction of the last solve: sum over levels and both sweeps of (w + h - 1) of the
 * window of gated pixels -- the length of the exact Gauss-Seidel dependency chain (SURVEY.md 8(d) "honest bound") */
long long pf_last_swept_steps(pf_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* PANOFLOW_H_ */
