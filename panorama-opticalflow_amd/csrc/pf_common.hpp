// Shared host/device declarations for the panoflow HIP library (gfx950 only).
// All kernels are built with -ffp-contract=off: the solver makes strict '<' decisions on nearly
// equal floats, so every expression keeps the reference's evaluation order without FMA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tile_stream_plan.hpp"
#include "reproject_math.hpp"
#include "lens_math.hpp"

namespace pf {

// ---- constants of the solver (reference: CPU/PixFlow.hpp:32-44 and the factory :459-497) ----
constexpr int kPyrMinImageSize = 24;
constexpr int kPyrMaxLevels = 1000;
constexpr float kGradEpsilon = 0.001f;
constexpr float kUpdateAlphaThreshold = 0.9f;
constexpr float kPyrScaleFactor = 0.9f;
constexpr float kSmoothnessCoef = 0.001f;
constexpr float kVerticalRegularizationCoef = 0.01f;
constexpr float kHorizontalRegularizationCoef = 0.01f;
constexpr float kGradientStepSize = 0.5f;
constexpr float kDownscaleFactor = 0.5f;
// The reference's PixFlow takes these as constructor arguments (CPU/PixFlow.hpp:46-68); its factory only ever passes the values above
// (:459-497).  The sweep kernels take them as scalar kernel arguments (round 6, pf_set_solver_params): a multiply by a coefficient costs
// the same from an SGPR as from a literal.  `step`: the fast step folds `flow - step * g` into ONE fused multiply-add, which is the
// reference's two roundings only when the product is exact, i.e. when step is a power of two; for any other step size the host sets
// `guard_min` above every exponent, so that the range guard sends EVERY step of an updated pixel through the IEEE sequence
// (select_step<false>, which multiplies and subtracts): no second kernel variant, bit-exact, slower.
struct SolverCoef {
  float smooth = kSmoothnessCoef, vreg = kVerticalRegularizationCoef, hreg = kHorizontalRegularizationCoef, step = kGradientStepSize;
  int guard_min = -94;   // an operand whose frexp exponent lies below this (and is not zero) leaves the exact forms' range; INT_MAX = always
};

// sentinel for "boundary flow not published yet" (a NaN payload arithmetic cannot produce)
constexpr unsigned long long kNotReady = 0x7FFFDEAD7FFFDEADull;

struct Gauss {  // separable kernel taps (host-computed, [OpenCV] getGaussianKernel CV_32F)
  float k[15];
  int ksize;
};

// ---- device helpers ----
__device__ __forceinline__ int d_reflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) { if (p < 0) p = -p; else p = 2 * n - 2 - p; }
  return p;
}
__device__ __forceinline__ int d_replicate(int p, int n) { return p < 0 ? 0 : (p >= n ? n - 1 : p); }
__device__ __forceinline__ int d_floor(float v) { int i = (int)v; return i - (v < (float)i); }

// [OpenCV imgwarp.cpp] interpolateCubic, A = -0.75, float arithmetic in this exact order
__device__ __forceinline__ void d_cubic_coeffs(float x, float* c) {
  const float A = -0.75f;
  c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
  c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
  c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
  c[3] = 1.f - c[0] - c[1] - c[2];
}
// source coordinate of destination index d: (float)((d+0.5)*scale-0.5), floor and fraction
__device__ __forceinline__ void d_src_coord(int d, double scale, int& s, float& f) {
  f = (float)((d + 0.5) * scale - 0.5);
  s = d_floor(f);
  f -= s;
}

// [OpenCV imgwarp.cpp] INTER_LINEAR float: HResizeLinear (fx forced to 0 at the borders, tail pixels
// copy S[sx]*1) then VResizeLinear (rows clipped per tap, weights untouched).
template <int CN>
__device__ __forceinline__ void d_resize_linear_px(const float* __restrict__ src, int sw, int sh, int dw, int dh, double scale_x,
                                                   double scale_y, int dx, int dy, float* out) {
  int sx, sy; float fx, fy;
  d_src_coord(dx, scale_x, sx, fx);
  d_src_coord(dy, scale_y, sy, fy);
  if (sx < 0) { fx = 0; sx = 0; }
  const bool tail = (sx + 1 >= sw);
  if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
  const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
  const float* r0 = src + size_t(d_replicate(sy, sh)) * sw * CN;
  const float* r1 = src + size_t(d_replicate(sy + 1, sh)) * sw * CN;
#pragma unroll
  for (int c = 0; c < CN; ++c) {
    float h0, h1;
    if (tail) { h0 = r0[sx * CN + c] * 1.0f; h1 = r1[sx * CN + c] * 1.0f; }
    else { h0 = r0[sx * CN + c] * a0 + r0[(sx + 1) * CN + c] * a1; h1 = r1[sx * CN + c] * a0 + r1[(sx + 1) * CN + c] * a1; }
    out[c] = h0 * b0 + h1 * b1;
  }
}

// ---- batch dimension -------------------------------------------------------------------------------------------------------
// A launch may cover `n` same-size pairs at once (throughput mode: one kernel boundary for n pairs instead of n).  The pairs'
// working buffers lie in identically laid-out slabs `stride` bytes apart, so a kernel reaches pair z's copy of ANY internal buffer
// by adding z * stride to the pointer it was given for pair 0 (blockIdx.z = pair; kernels that already use z for planes keep the
// plane in its low bits).  Caller-owned buffers (input images, blend ramp, outputs) come as per-pair pointer tables instead.
constexpr int kMaxBatch = 16;
struct Batch { int n = 1; size_t stride = 0; };
struct ExtPtrs { const void* p[kMaxBatch]; };   // caller-owned buffers of the pairs of a batch (read-only or written, by use)
// (pointer arithmetic on bytes, NOT a round trip through uintptr_t: an inttoptr hides the kernel argument from the compiler's address-space
// inference and every access through the pointer becomes a FLAT instruction -- counted in lgkmcnt as well, completion order unknown, so
// each wait on one is s_waitcnt vmcnt(0) lgkmcnt(0).  Rounds 3-4 shipped that: found in round 4, tests/micro/isa_flat_count.sh)
#define PF_BOFF(ptr, off) (ptr = (decltype(ptr))((char*)(ptr) + (off)))

// ---- launch wrappers (defined in the kernels_*.hip files) ----
// preprocessing
void launch_downscale_gray(hipStream_t st, const uint8_t* bgra, int cols, int rows, int pad, float* gray, float* alpha, int dw, int dh, Batch bt = Batch(),
                           const ExtPtrs* imgs = nullptr /* batched: the pairs' input images instead of bgra */);
void launch_gauss_small(hipStream_t st, const float* src, float* dst, int w, int h, int cn, const Gauss& g, Batch bt = Batch());
void launch_pyr_down4(hipStream_t st, const float* s0, const float* s1, const float* s2, const float* s3, int sw, int sh, float* d0,
                      float* d1, float* d2, float* d3, int dw, int dh, Batch bt = Batch(), int nplanes = 4 /* 1..4 of the planes */);
void launch_pyr_chain4(hipStream_t st, float* p0, float* p1, float* p2, float* p3, const int* ws, const int* hs, const size_t* off, int first, int k,
                       Batch bt = Batch());
// offsets/sizes of the pyramid levels inside one pyramid plane, passed by value to kernels that cover all levels at once
constexpr int kLevelTableMax = 96;
struct LevelTable { int n; int w[kLevelTableMax]; int h[kLevelTableMax]; unsigned off[kLevelTableMax]; };
// elements [first, total) of the pyramid planes (levels lie back to back, level 0 first); pyr1 == nullptr: one image
void launch_gradients_all(hipStream_t st, const float* pyr0, const float* pyr1, float* grad0, float* grad1, const LevelTable& t, size_t first,
                          size_t total, const Gauss& g3, int max_blocks = 0, Batch bt = Batch());
// gate + per-level bounding boxes + level-0 count in one launch, published to mapped pinned host memory behind an epoch flag
// (work: 4*kLevelTableMax + 2 ints, initialised once to (INT_MAX, INT_MAX, -1, -1)*, 0, 0; host_mapped: same size);
// work[4*l..]: min x, min y, max x, max y of level l
void launch_gate_bbox_all(hipStream_t st, const float* a0, const float* a1, uint8_t* gate, const LevelTable& t, size_t total, int* work, int* host_mapped,
                          int epoch, Batch bt = Batch(), size_t host_stride = 0 /* bytes between the pairs' mapped host areas */);
void launch_gauss15(hipStream_t st, const float* src, float* dst, int w, int h, const Gauss& g15, Batch bt = Batch(), int max_blocks = 0 /* cap on the persistent blocks per plane; 0 = the launcher's choice */);
void launch_median_gauss15_mix(hipStream_t st, const float* flow, const float* a0, const float* a1, int w, int h, const Gauss& g15, float* out, Batch bt = Batch(), int max_blocks = 0 /* cap on the persistent blocks per plane; 0 = the launcher's choice */);
void launch_gauss15_upsample(hipStream_t st, const float* coarse, int sw, int sh, float mul, float* up, float* dst, int w, int h, const Gauss& g15, Batch bt = Batch(), int max_blocks = 0 /* cap on the persistent blocks per plane; 0 = the launcher's choice */);
void launch_gauss15_mix(hipStream_t st, float* flow, const float* a0, const float* a1, int w, int h, const Gauss& g15, float* out, Batch bt = Batch(), int max_blocks = 0 /* cap on the persistent blocks per plane; 0 = the launcher's choice */);
void launch_median5(hipStream_t st, const float* src, float* dst, int w, int h, Batch bt = Batch());   // direct form below 3 Mpix, LDS-tiled form above
void launch_median5_form(hipStream_t st, const float* src, float* dst, int w, int h, bool tiled, Batch bt = Batch());   // a given form at any size (tests)
void launch_upsample_cubic(hipStream_t st, const float* src, int sw, int sh, float* dst, int dw, int dh, float mul, Batch bt = Batch());
bool upsample_cubic_fits(int sh, int dh);   // the scale launch_upsample_cubic covers: sh / dh <= 1.1875 (every pyramid: sh <= dh); it aborts on any other
void launch_final_flow(hipStream_t st, const float* flow0, int sw, int sh, int pad_cols, int rows, int pad, float mul, const Gauss& g3,
                       float* out, Batch bt = Batch(), const ExtPtrs* outs = nullptr /* batched: the pairs' output planes instead of out */);
// sweep
struct SweepArgs {
  const float2* g0;       // (I0x,I0y) at the pixel
  const float2* g1;       // (I1x,I1y) gathered bilinearly
  const float2* blurred;  // frozen blurred flow
  const uint8_t* gate;    // alpha0>thr && alpha1>thr
  float2* flow;           // in/out
  unsigned long long* boundary;  // [nbands][W] hand-off rows, pre-filled with kNotReady
  int* ctrl;              // [0] ticket, [1] abort/timeout flag
  int W, H, forward;
  int sparse;             // few pixels gated (full-canvas inputs): use the kernel variant that skips ungated anti-diagonals
  // optional timing events (v2 sweep): attached to the launches themselves (hipExtLaunchKernel: start of the prepass / end of the
  // sweep kernel come from the dispatch packets' own timestamps), so that timing a sweep puts no marker packets on its stream
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  Batch bt;               // v2 sweep: bt.n same-size pairs in one launch (every pointer above is pair 0's; pair z's lies z * bt.stride bytes on)
  int ax0 = 0, ay0 = 0, ax1 = 1 << 30, ay1 = 1 << 30;   // bounding box [ax0,ax1) x [ay0,ay1) of the gated pixels (default: everything); v2 sweep only
  int wide = 0;           // v2 sweep form: 0 = latency form (8 lanes per pixel, 4 bands of 8 rows per workgroup, one compute wave per SIMD), 1 = the same step
                          // with 8 bands per workgroup (two compute waves per SIMD), 2 = throughput form (2 lanes per pixel, bands of 32 rows,
                          // kernels_sweep_t.inl), -1 = throughput form when the launch oversubscribes the chip (dense, bands along x), else latency
  int wide_threshold_wgs = 512;   // wide = -1: "oversubscribed" means more latency-form workgroups x concurrent_sweeps than this
  int wide_tr = 0;                // wide = -1: transposed sweeps (bands along y) may take the throughput form too (its window loads do not coalesce there)
  int concurrent_sweeps = 2;      // sweeps that run on the chip at the same time as this launch's (this launch's pairs x 2 directions x lanes)
  SolverCoef cf;                  // the energy's coefficients and the gradient step size (defaults = the reference factory's presets)
};
size_t sweep_boundary_elems(int W, int H);   // hand-off granules needed per sweep launch (covers every sweep kernel of this build)
size_t sweep1_boundary_elems(int W, int H);                     // lab build only (-DPF_EXPERIMENTS)
void launch_sweep(hipStream_t st, const SweepArgs& a);          // lab build only: v1, 64 rows per wave, the independent cross-check (pf_config::sweep_impl = 1)
int sweep2_num_wgs(int H);
size_t sweep2_boundary_elems(int W, int H);   // granules one sweep launch may need (either band orientation)
size_t sweep2_rec_bytes(int W, int H);
int sweep_pk_probe(hipStream_t st, unsigned* d_scratch);   // 0 = the sweep's asm-block packed chains give the compiler forms' bits on this device; > 0 mismatching threads; < 0 HIP error
bool launch_sweep2(hipStream_t st, const SweepArgs& a, float* rec);  // v2: prepass + 8 lanes/pixel + helper waves; false = empty window, nothing launched
// coarsest-level search
void launch_adjust_initial_flow(hipStream_t st, const float* i0, const float* i1, const float* a0, const float* a1, int w, int h, int hint,
                                int max_pct, float* i1eq_tmp, float* flow, Batch bt = Batch());
void launch_intensity_ratio(hipStream_t st, const float* i0, const float* i1, const float* a0, const float* a1, int n, float* ratio, Batch bt = Batch());   // computeIntensityRatio of n elements
// blend
void launch_blend_tables(hipStream_t st);   // once per device before the first blend (create_ctx)
struct BlendPtrs { const uint8_t* L[kMaxBatch]; const uint8_t* R[kMaxBatch]; const float* fLR[kMaxBatch]; const float* fRL[kMaxBatch]; const float* blend[kMaxBatch]; uint8_t* out[kMaxBatch]; };
void launch_blend(hipStream_t st, const BlendPtrs& p, int n, int cols, int rows);   // n pairs, blockIdx.z = pair
void launch_blend(hipStream_t st, const uint8_t* L, const uint8_t* R, const float* flowLR, const float* flowRL, const float* blend, int cols,
                  int rows, uint8_t* out);   // one pair: fills a one-pair table
// stitch (K12-K15): per-frame pointer tables, blockIdx.z = frame, nf <= kMaxBatch same-size frames per launch; a lone canvas is nf = 1
struct StitchPtrs {
  const uint8_t* L[kMaxBatch]; const uint8_t* R[kMaxBatch];     // input images
  uint8_t* map[kMaxBatch]; uint8_t* ovL[kMaxBatch]; uint8_t* ovR[kMaxBatch];
  float* blend[kMaxBatch]; float* md[kMaxBatch];                // ramp (smoothed in place by the tile pass) and MergedDis
  double* rs[kMaxBatch]; float* tmp[kMaxBatch];                 // box blur: fp64 row sums, result
  uint8_t* merged[kMaxBatch]; uint8_t* out[kMaxBatch];          // novel view, composite
};
void launch_match_images(hipStream_t st, const StitchPtrs& p, int nf, int cols, int rows);   // L, R -> map, ovL, ovR
// against a stitch plan: p.map = the plan's map (read only); L, R -> ovL, ovR by the plan's code, and per frame the number of pixels whose
// own code differs from it, added to diff_mapped[frame] (mapped host words, zeroed by the caller)
void launch_match_verify(hipStream_t st, const StitchPtrs& p, int nf, int cols, int rows, unsigned* diff_mapped);
void launch_count_code(hipStream_t st, const uint8_t* map, int cols, int rows, int code, unsigned* count /* device word, zeroed by the caller */);
void launch_countblend(hipStream_t st, const StitchPtrs& p, int nf, int cols, int rows);     // map -> blend, md
// K12 for a whole chain (rig plans): img = a DEVICE table of nf x (n_steps + 1) image pointers, frame-major (top, L_1 .. L_n); the region
// code of step i is derived from L_i's alpha and the running union of top's and L_1 .. L_{i-1}'s.  make: nf = 1, the codes are stored into
// maps.m[i] and each step's overlap pixels (code 150) are added to count[i] (device words, zeroed by the caller).  verify: nothing is stored,
// pixels whose code differs from maps.m[i] are added to diff_mapped[frame * n_steps + i] (mapped host words, zeroed by the caller).
struct RigMaps { uint8_t* m[kMaxBatch]; };
void launch_rig_maps_make(hipStream_t st, const uint8_t* const* img, bool aligned16, const RigMaps& maps, int n_steps, int cols, int rows, unsigned* count);
void launch_rig_maps_verify(hipStream_t st, const uint8_t* const* img, bool aligned16, const RigMaps& maps, int n_steps, int nf, int cols, int rows,
                            unsigned* diff_mapped);
void launch_tile_blur(hipStream_t st, const StitchPtrs& p, int nf, int cols, int rows, int step, int k, void* work, bool streamed = false,
                      void* scratch = nullptr);                                                // blend in place, by md
void launch_box_blur(hipStream_t st, const StitchPtrs& p, int nf, int cols, int rows, int k); // blend -> tmp (rs: scratch)
void launch_gather(hipStream_t st, const StitchPtrs& p, int nf, int cols, int rows);         // L, R, merged, map -> out
// a canvas's blend-ramp geometry (StitchTool.cpp:130-143): the probe stride / tile size, the tile pass's window k1 and its form, the
// final box blur's window k2 (0 = none)
struct RampGeom {
  int step = 0, k1 = 0, k2 = 0;
  bool tiles = false;      // there is a tile pass (step > 0 && k1 > 0)
  bool streamed = false;   // ... in the streamed form: its window exceeds the LDS of a CU
  bool ok = true;          // false = neither form smooths this canvas (the window reaches across all of it): the entry points refuse it
};
RampGeom ramp_geom(int cols, int rows);
int countblend_step(int cols, int rows);   // the probe stride of countblend (StitchTool.cpp:151), at least 1
int tile_blur_reach(int k);                // how far a k-wide window (anchor k/2) reaches beyond its own pixel: max(k/2, k-1-k/2)
size_t tile_blur_work_bytes(int cols, int rows, int step, int k);   // device scratch of launch_tile_blur (diagonal counts + barrier word)
size_t tile_blur_lds_bytes(int step, int k);           // dynamic LDS of the resident form (whole window + all row sums)
bool tile_blur_resident_fits(int step, int k);          // ... within the 160 KB of a CU: the launcher's callers pick the form by this
bool tile_blur_stream_ok(int step, int k);              // the streamed form has a plan (one window row fits its LDS piece)
size_t tile_blur_stream_scratch_bytes(int step, int k); // device scratch of the streamed form (row sums of every block's tile)
void launch_fill_u64(hipStream_t st, unsigned long long* p, size_t n, unsigned long long v, Batch bt = Batch());
void launch_fill_u32(hipStream_t st, unsigned* p, size_t n, unsigned v, Batch bt = Batch());   // memset that knows the batch dimension
void launch_checksum64(hipStream_t st, const void* p, size_t bytes, unsigned long long* acc /* zeroed by the caller */);
void launch_count_diff_u32(hipStream_t st, const uint32_t* a, const uint32_t* b, size_t n, int* count /* zeroed by the caller */);
void launch_collect_status(hipStream_t st, const int* ctrl, int nwords, int* status_mapped, int bit, Batch bt = Batch());

// ---- flow visualisers (kernels_vis.hip; CPU/OpticalFlow.cpp:147-204, CPU/main.cpp:20-45).  Flows / images packed. ----
struct VisParams {   // written on the device: the grey disparity's float scale / shift, and the non-finite flow components seen
  float scale, shift;
  int nonfinite;     // zeroed by the caller
  int pad_;
};
void vis_grid(int cols, int rows, int* nax, int* nay);   // arrows per axis of the 12-px grid
size_t vis_part_bytes();
size_t vis_arrow_bytes(int cols, int rows);
void launch_vis_reduce(hipStream_t st, const float* flow, int cols, int rows, float* part, VisParams* par);   // min / max -> scale, shift, count
void launch_vis_arrows(hipStream_t st, const float* flow, int cols, int rows, void* arrows);                   // LineAA set-up per arrow
void launch_vis_grey(hipStream_t st, const float* flow, int cols, int rows, const VisParams* par, uint8_t* out);   // 16-byte aligned buffers
void launch_vis_wheel(hipStream_t st, const float* flow, int cols, int rows, VisParams* par, uint8_t* out);       // counts non-finite too
void launch_vis_field(hipStream_t st, const uint8_t* img, int cols, int rows, const void* arrows, uint8_t* out);
void launch_vis_panel(hipStream_t st, const float* flow, const uint8_t* img, int cols, int rows, const VisParams* par, const void* arrows,
                      uint8_t* out /* 3 cols x rows BGRA */);

// ---- PNG encoder (kernels_png.hip): filter, deflate of independent segments, compaction; the host frames (png_frame.hpp) ----
struct PngWork {
  uint8_t* stream;            // filtered scanlines, png_stream_alloc_bytes()
  uint8_t* slots;             // png_frame::kSegSlot bytes per segment
  unsigned* sizes;            // per segment: bytes of its deflate blocks
  unsigned* adler;            // per segment: Adler-32 of its bytes (from 1), combined on the host
  unsigned long long* offs;   // segments + 1: exclusive prefix sum of sizes; the last entry is the deflate stream's length
  uint8_t* packed;            // the deflate stream, png_frame::deflate_bound() bytes
};
size_t png_stream_alloc_bytes(int cols, int rows);
void launch_png_filter(hipStream_t st, const uint8_t* bgra /* packed, 4-byte aligned */, int cols, int rows, const PngWork& w);   // bgra -> stream
void launch_png_deflate(hipStream_t st, int cols, int rows, const PngWork& w);   // stream -> slots, sizes, adler
void launch_png_pack(hipStream_t st, int cols, int rows, const PngWork& w);      // sizes -> offs; slots -> packed

// ---- JPEG encoder (kernels_jpeg.hip): blocks, the entropy coder's size pass, a scan, its write pass; the host frames (jpeg_frame.hpp) ----
struct JpegWork {
  int16_t* coef;              // jpeg_frame::coef_bytes(): 64 int16 per block in MCU order
  const void* tables;         // a jpeg_frame::Tables in device memory
  unsigned* sizes;            // per restart interval: its bytes, stuffing and marker included
  unsigned long long* offs;   // intervals + 1: exclusive prefix sums of sizes; the last is the segment's length
};
bool jpeg_restart_fits(int subsampling, int restart);   // can the entropy kernel's workgroup hold an interval of `restart` MCUs?
void launch_jpeg_blocks(hipStream_t st, const uint8_t* bgra /* packed, 4-byte aligned */, int cols, int rows, int subsampling, const JpegWork& w);   // bgra -> coef
void launch_jpeg_sizes(hipStream_t st, int cols, int rows, int subsampling, int restart, const JpegWork& w);                                          // coef -> sizes, offs
void launch_jpeg_write(hipStream_t st, int cols, int rows, int subsampling, int restart, const JpegWork& w, uint8_t* packed /* offs[intervals] bytes */);

// ---- resize (kernels_resize.hip): Pillow's antialiased resample of an RGBA image, a horizontal and a vertical pass; the host makes the tables ----
struct ResizePtrs { const uint32_t* src[kMaxBatch]; uint32_t* dst[kMaxBatch]; };   // blockIdx.z = image, n <= kMaxBatch same-size images per launch
// bounds: per output index {first source index, taps}; k: 22-bit fixed-point coefficients, tap-major (k[t * out + index])
void launch_resize_h(hipStream_t st, int n, const ResizePtrs& io, int cols, int rows, int out_cols, const int* bounds, const int* k, bool premul, bool unpremul);   // cols x rows -> out_cols x rows
void launch_resize_v(hipStream_t st, int n, const ResizePtrs& io, int cols, int rows, int out_rows, const int* bounds, const int* k, bool premul, bool unpremul);   // cols x rows -> cols x out_rows

// ---- reprojection (kernels_reproject.hip): an equirectangular sphere -> cube faces, a rectilinear view, a turned sphere; the host makes the tables ----
struct ReprojectArgs {
  const uint32_t* src[kMaxBatch]; uint32_t* dst[kMaxBatch];   // blockIdx.z = image, n <= kMaxBatch per launch; dst null: coordinates only
  int face[kMaxBatch];                                        // cube: the face of image z
  reproject::Geometry g;
  const double* eq;      // equirect output: cos lon, sin lon (out_cols each), cos lat, sin lat (out_rows each)
  const int* cubic;      // bicubic: 256 phases x 4 taps (reproject::make_cubic_table)
  int* fx_out; int* fy_out;   // null, or out_cols x out_rows planes that take the quantised coordinates (pf_stage_reproject_coords, n = 1)
};
void launch_reproject(hipStream_t st, int n, const ReprojectArgs& a);

// ---- lens remap (kernels_lens.hip): raw photos of a camera rig -> the equirectangular canvas, the inverse of the reprojection; the host makes the tables ----
struct LensArgs {
  const uint32_t* src[kMaxBatch]; uint32_t* dst[kMaxBatch];   // blockIdx.z = image, n <= kMaxBatch per launch; dst null: coordinates only
  lens::Lens lens[kMaxBatch];                                 // the camera of image z
  lens::Geometry g;
  const double* eq;      // the canvas's tables: cos lon, sin lon (cols each), cos lat, sin lat (rows each)
  const int* cubic;      // bicubic: 256 phases x 4 taps (reproject::make_cubic_table)
  int* fx_out; int* fy_out;   // null, or cols x rows planes that take the quantised coordinates (pf_stage_lens_coords, n = 1)
};
void launch_lens_remap(hipStream_t st, int n, const LensArgs& a);

// ---- TIFF decoder (kernels_tiff.hip): strips in parallel (LZW, PackBits, deflate), then predictor + RGB(A) -> BGRA per row ----
// A strip's status word: the bytes it produced in the low half, a reason in the high half (0 = the stream ended by itself or filled
// the strip; the strip is good when the low half equals its expected bytes).
constexpr unsigned kTiffBadCode = 1;        // LZW: a code above the table's next entry, or a non-literal first code after a Clear
constexpr unsigned kTiffBadTableFull = 2;   // LZW: code == next with the table full
constexpr unsigned kTiffCutPacket = 3;      // PackBits: a packet runs past the strip's bytes
// deflate strips (opt-in, pf_tiff_set_inflate): the classes of zlib's own refusals.  A deflate strip is good when the low half equals
// its expected bytes AND the reason is 0 (a wrong Adler-32 is full and wrong).
constexpr unsigned kTiffZlibHeader = 4;     // CM, CINFO, FCHECK, a preset dictionary
constexpr unsigned kTiffBlockHeader = 5;    // block type 3, stored LEN != ~NLEN
constexpr unsigned kTiffCodeLengths = 6;    // too many symbols, a bad repeat, an over-subscribed or incomplete set, no end-of-block code
constexpr unsigned kTiffInvalidSymbol = 7;  // literal/length 286-287, distance 30-31, bits no code of an incomplete set spells
constexpr unsigned kTiffFarBack = 8;        // a distance that reaches before the strip's first byte
constexpr unsigned kTiffDataCheck = 9;      // the Adler-32 does not match the bytes written
struct TiffWork {
  const uint8_t* file;         // the uploaded file bytes
  unsigned long long bytes;    // ... and how many
  const uint32_t* offsets;     // per strip: file offset
  const uint32_t* counts;      // per strip: compressed bytes
  int n_strips, cols, rows, samples, rows_per_strip, predictor;
  uint8_t* plane;              // decoded samples, rows * cols * samples bytes (unused for compression 1)
  unsigned long long* status;  // per strip
};
void launch_tiff_lzw(hipStream_t st, const TiffWork& w);        // file -> plane, status
void launch_tiff_packbits(hipStream_t st, const TiffWork& w);   // file -> plane, status
void launch_tiff_inflate(hipStream_t st, const TiffWork& w);    // file -> plane, status
void launch_tiff_finish(hipStream_t st, const TiffWork& w, bool from_file /* compression 1: samples read from the file */, uint8_t* bgra /* packed, 4-byte aligned */);

// ---- JPEG decoder (kernels_jpegd.hip): self-synchronising Huffman decode over subsequences, DC sums, IDCT, upsampling and colour ----
constexpr unsigned kJpegdSubseq = 64;       // the product's subsequence size S in bytes: measured, DESIGN.md 8.10, profiles/jpeg_decode_ab.txt
constexpr unsigned kJpegdSubseqMin = 32, kJpegdSubseqMax = 1024;   // what the lab build's PANOFLOW_JPEGD_SUBSEQ may choose (powers of two)
constexpr unsigned kJpegdLanes = 256;       // subsequences per workgroup of the entropy kernels
struct JpegdWork {
  const uint8_t* seg;          // the entropy segment inside the uploaded file
  unsigned seg_bytes, S, nsub; // ... its bytes, the subsequence size, ceil(seg_bytes / S) (at least 1)
  int ncomp, hs, vs;           // 1 or 3 components; luma sampling (chroma is 1 x 1)
  unsigned restart, cols, rows;
  const void* tables;          // a jpeg_parse::Tables in device memory
  void* states[2];             // nsub x 16 bytes each: the lanes' exit states, read from one and written to the other
  unsigned* words;             // [0] changed, [1] rounds of the launch, [2] the MCU of the true path's first event (0xFFFFFFFF: none);
                               // [3] lanes whose record changed after their first walk, summed over the launches
  void* first;                 // nsub x 8 bytes: blocks and markers before each subsequence
  int16_t* coef;               // 64 int16 per block in MCU order, zigzag order; zeroed before the write pass
  uint8_t* planes;             // Y, then Cb and Cr, at their block-padded sizes
  unsigned* dcsum;             // intervals x components x jpegd_dc_chunks() words: the DC pass's chunk sums
};
unsigned jpegd_dc_chunks(int ncomp, int hs, int vs, unsigned restart, unsigned nmcu);   // workgroups per (interval, component) of the DC pass
void launch_jpegd_sync(hipStream_t st, const JpegdWork& w, int first /* the first launch: lanes guess */, int from /* states[from] -> states[1 - from] */);
void launch_jpegd_write(hipStream_t st, const JpegdWork& w, int from);   // states[from] -> first, coef, words[2]
void launch_jpegd_pixels(hipStream_t st, const JpegdWork& w, uint8_t* bgra /* packed, 4-byte aligned; null: planes only */);   // coef -> planes -> bgra

}  // namespace pf
