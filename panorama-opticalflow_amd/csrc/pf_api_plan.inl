// Part of pf_api.hip (one translation unit): stitch plans, rig plans and the rig chain in one call, on the batched step of pf_api_stitch.inl.

// ---- stitch plans ----
// Creation: MatchImages into the plan's map, then the blend ramp by blend_ramp_dev with ramp_geom()'s geometry and form, finishing in
// the plan's ramp plane (the box blur's result plane, or the in-place ramp where the canvas has no box blur); the working planes are the
// lone entry points' ("st_*"), the inputs go through "h_img0/1": the chain ("ch_*"), the prefetch records and the visualiser's inputs stay.
static int stitch_plan_make(pf_ctx* c, const uint8_t* dl, const uint8_t* dr, int cols, int rows, const RampGeom& g, pf_stitch_plan** plan_out) {
  StitchPtrs p{};
  if (int e = stitch_planes(c, SP_OV | SP_RAMP, cols, rows, p)) return e;
  unsigned* dcount = (unsigned*)ensure(c, "plan_count", 256);
  if (!dcount) return PF_ERR_NOMEM;
  RampWork w;
  if (int e = ramp_planes(c, kRampLone, 1, cols, rows, g, p, w, false)) return e;
  pf_stitch_plan* pl = plan_new(cols, rows, false);
  if (!pl) return fail(c, PF_ERR_NOMEM, "hipMalloc of a %dx%d stitch plan (5 B/px) failed", cols, rows);
  PlanDrop drop; drop.pl = pl;
  hipStream_t sm = c->s_main;
  p.L[0] = dl; p.R[0] = dr; p.map[0] = pl->map;
  if (g.k2 > 0) p.tmp[0] = pl->ramp; else p.blend[0] = pl->ramp;
  { PROF(c, sm, "match_images"); launch_match_images(sm, p, 1, cols, rows); }
  const float* ramp = nullptr;
  if (int e = blend_ramp_dev(c, sm, p, 1, cols, rows, g, w, true, &ramp)) return e;
  HIPCHK(c, hipMemsetAsync(dcount, 0, 4, sm));
  launch_count_code(sm, pl->map, cols, rows, 150, dcount);
  unsigned overlap = 0;
  HIPCHK(c, hipMemcpyAsync(&overlap, dcount, 4, hipMemcpyDeviceToHost, sm));
  HIPCHK(c, hipGetLastError());
  if (int e = finish(c)) return e;
  if (int e = check_sweeps(c)) return e;
  pl->overlap_px = overlap;
  c->plans.push_back(pl);
  drop.pl = nullptr;
  *plan_out = pl;
  return 0;
}
int pf_stitch_plan_create(pf_ctx* c, const uint8_t* l, const uint8_t* r, int cols, int rows, size_t step, pf_stitch_plan** plan_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!l || !plan_out) return fail(c, PF_ERR_ARG, "null pointer");
  *plan_out = nullptr;
  if (int e = check_dims(c, cols, rows, cols / 20)) return e;
  if (step < size_t(cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  const RampGeom g = ramp_geom(cols, rows);
  if (int e = check_blend_ramp(c, cols, rows, g)) return e;
  const size_t n = size_t(cols) * rows;
  uint8_t* dl = (uint8_t*)ensure(c, "h_img0", n * 4);
  if (!dl) return PF_ERR_NOMEM;
  const uint8_t* dr = nullptr;
  if (r) {
    uint8_t* up = (uint8_t*)ensure(c, "h_img1", n * 4);
    if (!up) return PF_ERR_NOMEM;
    if (int e = up_plane(c, up, r, step, cols, rows, 4)) return e;
    dr = up;
  } else {
    if (c->chain_cols != cols || c->chain_rows != rows) return fail(c, PF_ERR_ARG, "pf_stitch_plan_create: no previous result of this size to take the R mask from");
    dr = (const uint8_t*)ensure(c, "ch_final", n * 4);   // read in place
    if (!dr) return PF_ERR_NOMEM;
  }
  if (int e = up_plane(c, dl, l, step, cols, rows, 4)) return e;
  return stitch_plan_make(c, dl, dr, cols, rows, g, plan_out);
}
int pf_stitch_plan_create_dev(pf_ctx* c, const uint8_t* d_l, const uint8_t* d_r, int cols, int rows, pf_stitch_plan** plan_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!d_l || !d_r || !plan_out) return fail(c, PF_ERR_ARG, "null pointer");
  *plan_out = nullptr;
  if (int e = check_dims(c, cols, rows, cols / 20)) return e;
  const RampGeom g = ramp_geom(cols, rows);
  if (int e = check_blend_ramp(c, cols, rows, g)) return e;
  const uint8_t* const imgs[2] = {d_l, d_r};
  if (int e = check_dev_align(c, "pf_stitch_plan_create_dev", "image", imgs, 2)) return e;
  return stitch_plan_make(c, d_l, d_r, cols, rows, g, plan_out);
}
int pf_stitch_plan_destroy(pf_ctx* c, pf_stitch_plan* plan) {
  if (int e = use(c)) return e;
  if (!plan_is_live(c, plan)) return fail(c, PF_ERR_ARG, "pf_stitch_plan_destroy: not a live stitch plan of this context");
  if (plan->rig_owned) return fail(c, PF_ERR_ARG, "pf_stitch_plan_destroy: the plan is a step of a rig plan (pf_rig_plan_destroy frees it)");
  c->plans.erase(std::find(c->plans.begin(), c->plans.end(), plan));
  plan_free(plan);
  return 0;
}
int pf_stitch_plan_info(const pf_stitch_plan* plan, int* cols, int* rows, long long* overlap_px) {
  if (!plan) return fail(nullptr, PF_ERR_ARG, "null plan");
  if (cols) *cols = plan->cols;
  if (rows) *rows = plan->rows;
  if (overlap_px) *overlap_px = plan->overlap_px;
  return 0;
}
int pf_stitch_plan_download(pf_ctx* c, const pf_stitch_plan* plan, uint8_t* map_out, size_t mstep, float* blend_out, size_t bstep) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!plan_is_live(c, plan)) return fail(c, PF_ERR_ARG, "pf_stitch_plan_download: not a live stitch plan of this context");
  const int cols = plan->cols, rows = plan->rows;
  if ((map_out && mstep < size_t(cols)) || (blend_out && bstep < size_t(cols) * 4)) return fail(c, PF_ERR_ARG, "row step too small");
  if (map_out) if (int e = down_plane(c, map_out, mstep, plan->map, cols, rows, 1)) return e;
  if (blend_out) if (int e = down_plane(c, blend_out, bstep, plan->ramp, cols, rows, 4)) return e;
  return finish(c);
}

// ---- rig plans: the plans of a whole chain from its n + 1 input masks, and the chain in one call ----
// A composite's alpha is > 0 exactly where L's or R's is, so the R mask of step i is top | L_1 | .. | L_{i-1}: k_rig_maps (kernels_misc.hip)
// derives every step's map in one pass over the inputs, and the n ramps go through blend_ramp_dev as ONE group of n frames.
namespace {
// a handle is valid if the context lists it (never dereferenced before that, as with stitch plans)
int check_rig(pf_ctx* c, const pf_rig_plan* rig, int cols, int rows, const char* what) {
  if (std::find(c->rigs.begin(), c->rigs.end(), rig) == c->rigs.end()) return fail(c, PF_ERR_ARG, "%s: not a live rig plan of this context", what);
  if (cols > 0 && (rig->cols != cols || rig->rows != rows)) return fail(c, PF_ERR_ARG, "%s: the rig plan is %dx%d, the canvas %dx%d", what, rig->cols, rig->rows, cols, rows);
  return 0;
}
// the mapped words k_rig_maps (verify) counts into, zeroed: frames x steps of one call
int rig_diff_words(pf_ctx* c, size_t words) {
  if (c->rig_diff_cap < words) {
    if (c->h_rig_diff) hipHostFree(c->h_rig_diff);
    c->h_rig_diff = c->d_rig_diff = nullptr; c->rig_diff_cap = 0;
    const size_t cap = std::max(words, size_t(kMaxBatch) * kMaxBatch);
    if (hipHostMalloc((void**)&c->h_rig_diff, cap * sizeof(unsigned), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&c->d_rig_diff, c->h_rig_diff, 0) != hipSuccess) {
      if (c->h_rig_diff) hipHostFree(c->h_rig_diff);
      c->h_rig_diff = c->d_rig_diff = nullptr;
      return fail(c, PF_ERR_NOMEM, "hipHostMalloc of %zu mapped words failed", cap);
    }
    c->rig_diff_cap = cap;
  }
  memset(c->h_rig_diff, 0, words * sizeof(unsigned));
  return 0;
}
// after the sync that followed the verifying launches: the first frame off the rig, its first differing step and the pixel count
// (tools/pano_stitch.cpp reads the frame index out of this message: keep "frame %d differs from the rig plan")
int report_rig_diff(pf_ctx* c, const char* what, int n_frames, int n_steps) {
  for (int k = 0; k < n_frames; ++k)
    for (int i = 0; i < n_steps; ++i) {
      const unsigned d = __atomic_load_n(c->h_rig_diff + size_t(k) * n_steps + i, __ATOMIC_ACQUIRE);
      if (d) return fail(c, PF_ERR_ARG, "%s: frame %d differs from the rig plan at step %d in %u pixels' region codes (alpha masks are not the rig's)", what, k, i + 1, d);
    }
  return 0;
}
uint8_t* rig_slot(pf_ctx* c, const char* kind, int w, int j, size_t bytes) {
  char name[40];
  snprintf(name, sizeof name, "rg_%s%d_%d", kind, w, j);
  return (uint8_t*)ensure(c, name, bytes);
}
bool all_aligned16(const uint8_t* const* p, size_t count) {
  uintptr_t bits = 0;
  for (size_t i = 0; i < count; ++i) bits |= (uintptr_t)p[i];
  return (bits & 15) == 0;
}
RigMaps rig_maps(const pf_rig_plan* rig) {
  RigMaps m{};
  for (int i = 0; i < rig->n_steps; ++i) m.m[i] = rig->steps[i]->map;
  return m;
}
// d_img: n_steps + 1 device images (top, L_1 .. L_n) of this context's device, complete on s_main's timeline
int rig_plan_make(pf_ctx* c, int n_steps, const uint8_t* const* d_img, int cols, int rows, const RampGeom& g, pf_rig_plan** out) {
  const size_t n = size_t(cols) * rows;
  const uint8_t** tbl = (const uint8_t**)ensure(c, "rg_tbl", size_t(n_steps + 1) * sizeof(void*));
  unsigned* dcount = (unsigned*)ensure(c, "plan_count", 256);
  size_t s4 = 0;
  float* blend = frame_planes<float>(c, "sb_blend", n_steps, n * 4, s4); float* md = frame_planes<float>(c, "sb_md", n_steps, n * 4, s4);
  if (!tbl || !dcount || !blend || !md) return PF_ERR_NOMEM;
  StitchPtrs p{};
  RampWork w;
  if (int e = ramp_planes(c, kRampBatch, n_steps, cols, rows, g, p, w, false)) return e;
  pf_rig_plan* rig = new pf_rig_plan();
  rig->n_steps = n_steps; rig->cols = cols; rig->rows = rows;
  PlanDrop drop; drop.rig = rig;
  for (int i = 0; i < n_steps; ++i) {
    pf_stitch_plan* pl = plan_new(cols, rows, true);
    if (!pl) return fail(c, PF_ERR_NOMEM, "hipMalloc of a %dx%d rig plan (5 B/px per step, %d steps) failed", cols, rows, n_steps);
    rig->steps.push_back(pl);
  }
  hipStream_t sm = c->s_main;
  HIPCHK(c, hipMemcpyAsync(tbl, d_img, size_t(n_steps + 1) * sizeof(void*), hipMemcpyHostToDevice, sm));
  HIPCHK(c, hipMemsetAsync(dcount, 0, kMaxBatch * sizeof(unsigned), sm));
  { PROF(c, sm, "rig_maps"); launch_rig_maps_make(sm, tbl, all_aligned16(d_img, n_steps + 1), rig_maps(rig), n_steps, cols, rows, dcount); }
  for (int i = 0; i < n_steps; ++i) {
    p.map[i] = rig->steps[i]->map; p.md[i] = (float*)((char*)md + i * s4);
    float* work = (float*)((char*)blend + i * s4);
    if (g.k2 > 0) { p.blend[i] = work; p.tmp[i] = rig->steps[i]->ramp; } else p.blend[i] = rig->steps[i]->ramp;
  }
  const float* ramp[kMaxBatch];
  if (int e = blend_ramp_dev(c, sm, p, n_steps, cols, rows, g, w, true, ramp)) return e;
  unsigned overlap[kMaxBatch] = {0};
  HIPCHK(c, hipMemcpyAsync(overlap, dcount, kMaxBatch * sizeof(unsigned), hipMemcpyDeviceToHost, sm));
  HIPCHK(c, hipGetLastError());
  if (int e = finish(c)) return e;
  if (int e = check_sweeps(c)) return e;
  for (int i = 0; i < n_steps; ++i) { rig->steps[i]->overlap_px = overlap[i]; c->plans.push_back(rig->steps[i]); }
  c->rigs.push_back(rig);
  drop.rig = nullptr;
  *out = rig;
  return 0;
}
int check_rig_create(pf_ctx* c, int n_steps, const void* top, const void* l, int cols, int rows, pf_rig_plan** out, RampGeom& g) {
  if (!top || !l || !out) return fail(c, PF_ERR_ARG, "null pointer");
  *out = nullptr;
  if (n_steps < 1 || n_steps > kMaxBatch) return fail(c, PF_ERR_ARG, "a rig plan has 1..%d steps (n_steps = %d)", kMaxBatch, n_steps);
  if (int e = check_dims(c, cols, rows, cols / 20)) return e;
  g = ramp_geom(cols, rows);
  return check_blend_ramp(c, cols, rows, g);
}
}  // namespace

int pf_rig_plan_create(pf_ctx* c, int n_steps, const uint8_t* top, const uint8_t* const* l, int cols, int rows, size_t step, pf_rig_plan** out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  RampGeom g;
  if (int e = check_rig_create(c, n_steps, top, l, cols, rows, out, g)) return e;
  for (int i = 0; i < n_steps; ++i) if (!l[i]) return fail(c, PF_ERR_ARG, "null pointer (step %d)", i + 1);
  if (step < size_t(cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  const size_t n = size_t(cols) * rows;
  const uint8_t* d_img[kMaxBatch + 1];
  for (int j = 0; j <= n_steps; ++j) {
    uint8_t* d = rig_slot(c, "in", 0, j, n * 4);
    if (!d) return PF_ERR_NOMEM;
    if (int e = up_plane(c, d, j == 0 ? top : l[j - 1], step, cols, rows, 4)) return e;
    d_img[j] = d;
  }
  return rig_plan_make(c, n_steps, d_img, cols, rows, g, out);
}
int pf_rig_plan_create_dev(pf_ctx* c, int n_steps, const uint8_t* d_top, const uint8_t* const* d_l, int cols, int rows, pf_rig_plan** out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  RampGeom g;
  if (int e = check_rig_create(c, n_steps, d_top, d_l, cols, rows, out, g)) return e;
  const uint8_t* d_img[kMaxBatch + 1];
  d_img[0] = d_top;
  for (int i = 0; i < n_steps; ++i) { if (!d_l[i]) return fail(c, PF_ERR_ARG, "null device pointer (step %d)", i + 1); d_img[i + 1] = d_l[i]; }
  if (int e = check_dev_align(c, "pf_rig_plan_create_dev", "image", d_img, size_t(n_steps) + 1)) return e;
  return rig_plan_make(c, n_steps, d_img, cols, rows, g, out);
}
int pf_rig_plan_destroy(pf_ctx* c, pf_rig_plan* rig) {
  if (int e = use(c)) return e;
  auto it = std::find(c->rigs.begin(), c->rigs.end(), rig);
  if (it == c->rigs.end()) return fail(c, PF_ERR_ARG, "pf_rig_plan_destroy: not a live rig plan of this context");
  c->rigs.erase(it);
  for (pf_stitch_plan* pl : rig->steps) {
    c->plans.erase(std::remove(c->plans.begin(), c->plans.end(), pl), c->plans.end());
    plan_free(pl);
  }
  delete rig;
  return 0;
}
int pf_rig_plan_info(const pf_rig_plan* rig, int* n_steps, int* cols, int* rows) {
  if (!rig) return fail(nullptr, PF_ERR_ARG, "null rig plan");
  if (n_steps) *n_steps = rig->n_steps;
  if (cols) *cols = rig->cols;
  if (rows) *rows = rig->rows;
  return 0;
}
const pf_stitch_plan* pf_rig_plan_step(pf_ctx* c, const pf_rig_plan* rig, int step) {
  if (!c) { fail(nullptr, PF_ERR_ARG, "null context"); return nullptr; }
  if (check_rig(c, rig, 0, 0, "pf_rig_plan_step")) return nullptr;
  if (step < 0 || step >= rig->n_steps) { fail(c, PF_ERR_ARG, "pf_rig_plan_step: step %d of a rig plan of %d steps (0-based)", step, rig->n_steps); return nullptr; }
  return rig->steps[step];
}

// The chain in one call.  Frames go through in waves of `in_flight`; a wave runs its steps one after the other through stitch_group with
// step i's plan (run_lanes' lanes and groups), R of step i + 1 = the composite of step i, which ping-pongs between two internal planes
// per frame in flight (or lies in the caller's buffer, device form).  Every frame is verified against the rig's maps before any solve.
namespace {
// one step of one wave: `count` frames, arrays indexed by the frame's place in the wave
int rig_wave_step(pf_ctx* c, const pf_rig_plan* rig, int i, int count, const uint8_t* const* dl, const uint8_t* const* dr, uint8_t* const* dout, int cols, int rows,
                  int max_pct, int in_flight, const char* what) {
  std::vector<unsigned> diff(count, 0u);
  if (int e = run_lanes(c, count, in_flight, cols, rows, 3, what, [&](pf_ctx* lane, int first, int cnt) {
        return stitch_group(lane, first, cnt, dl, dr, cols, rows, max_pct, dout, rig->steps[i], diff.data());
      })) return e;
  for (int k = 0; k < count; ++k)
    if (diff[k]) return fail(c, PF_ERR_DEVICE, "%s: internal error: step %d's match found %u pixels off the plan in a frame that passed the rig's verification", what, i + 1, diff[k]);
  return 0;
}
}  // namespace

int pf_rig_stitch_batch(pf_ctx* c, const pf_rig_plan* rig, int n_frames, const uint8_t* const* top, const uint8_t* const* l, int cols, int rows, size_t step,
                        int max_pct, uint8_t* const* out, size_t ostep, int in_flight) {
  const char* const what = "pf_rig_stitch_batch";
  if (int e = use(c)) return e;
  c->vis_step_valid = false;   // lane 0 solves in this context's arena
  if (n_frames < 0 || !top || !l) return fail(c, PF_ERR_ARG, "bad argument");
  if (int e = check_rig(c, rig, cols, rows, what)) return e;
  if (n_frames == 0) return 0;
  const int ns = rig->n_steps;
  for (int k = 0; k < n_frames; ++k) {
    if (!top[k]) return fail(c, PF_ERR_ARG, "null pointer (frame %d)", k);
    for (int i = 0; i < ns; ++i) if (!l[size_t(k) * ns + i]) return fail(c, PF_ERR_ARG, "null pointer (frame %d, step %d)", k, i + 1);
  }
  if (int e = check_stitch_canvas(c, cols, rows, max_pct)) return e;
  if (step < size_t(cols) * 4 || (out && ostep < size_t(cols) * 4)) return fail(c, PF_ERR_ARG, "row step too small");
  const int W = clamp_in_flight(in_flight, n_frames), nwaves = (n_frames + W - 1) / W;
  const size_t n = size_t(cols) * rows;
  // per frame in flight: the n + 1 inputs -- two sets of them where the call has several waves, wave wv in set wv & 1 -- and two composites
  const int nsets = nwaves > 1 ? 2 : 1;
  const size_t set_len = size_t(W) * (ns + 1);
  std::vector<const uint8_t*> in(nsets * set_len);
  std::vector<uint8_t*> comp(size_t(W) * 2);
  for (int w = 0; w < nsets * W; ++w)
    for (int j = 0; j <= ns; ++j) if (!(in[size_t(w) * (ns + 1) + j] = rig_slot(c, "in", w, j, n * 4))) return PF_ERR_NOMEM;
  for (int w = 0; w < W; ++w)
    for (int j = 0; j < 2; ++j) if (!(comp[w * 2 + j] = rig_slot(c, "c", w, j, n * 4))) return PF_ERR_NOMEM;
  const uint8_t** tbl = (const uint8_t**)ensure(c, "rg_tbl", in.size() * sizeof(void*));
  if (!tbl) return PF_ERR_NOMEM;
  if (int e = rig_diff_words(c, size_t(n_frames) * ns)) return e;
  // image j (0 = top) of frame w of wave wv: its slot in set wv & 1 and the caller's source, through copy(slot, source) until one fails
  auto wave_images = [&](int wv, auto copy) {
    const int first = wv * W, count = std::min(W, n_frames - first);
    const uint8_t* const* slot = in.data() + (wv & 1) * set_len;
    for (int w = 0; w < count; ++w)
      for (int j = 0; j <= ns; ++j)
        if (!copy((void*)slot[size_t(w) * (ns + 1) + j], j == 0 ? top[first + w] : l[size_t(first + w) * ns + j - 1])) return;
  };
  auto upload_wave = [&](int wv) -> int {
    int e = 0;
    wave_images(wv, [&](void* d, const uint8_t* src) { return (e = up_plane(c, d, src, step, cols, rows, 4)) == 0; });
    return e;
  };
  // The overlapped form of a later wave's second upload: while wave wv - 1 computes, a host thread of its own copies wave wv (>= 2) into
  // the set wave wv - 2 has left, on the copy stream.  (A thread, because the copy of a pageable source blocks its caller while it is
  // staged: issued from the calling thread it would hold back the launches it is meant to run beside.)
  struct Prefetch {
    std::thread th; hipError_t err = hipSuccess;
    int join() { if (th.joinable()) th.join(); return err == hipSuccess ? 0 : 1; }
    ~Prefetch() { if (th.joinable()) th.join(); }
  } pre;
  auto prefetch_wave = [&](int wv) {
    pre.err = hipSuccess;
    pre.th = std::thread([&, wv]() {
      hipError_t e = hipSetDevice(c->device);
      if (e == hipSuccess) wave_images(wv, [&](void* d, const uint8_t* src) { return (e = up_plane_on(c->s_copy, d, src, step, cols, rows, 4)) == hipSuccess; });
      if (e == hipSuccess) e = hipStreamSynchronize(c->s_copy);
      pre.err = e;
    });
  };
  const bool overlap = c->rig_overlap_uploads && nwaves > 2;
  if (overlap && !c->s_copy) HIPCHK(c, hipStreamCreateWithFlags(&c->s_copy, hipStreamNonBlocking));
  {
    // verification: every wave's images go through its set of slots and one verifying launch, the last wave first, so that waves 0 and 1
    // are resident when the solves begin (a call of up to two waves uploads nothing twice)
    CallGuard guard_(c);
    HIPCHK(c, hipMemcpyAsync(tbl, in.data(), in.size() * sizeof(void*), hipMemcpyHostToDevice, c->s_main));
    for (int wv = nwaves - 1; wv >= 0; --wv) {
      const int first = wv * W, count = std::min(W, n_frames - first);
      if (int e = upload_wave(wv)) return e;
      PROF(c, c->s_main, "rig_verify");
      launch_rig_maps_verify(c->s_main, tbl + (wv & 1) * set_len, true, rig_maps(rig), ns, count, cols, rows, c->d_rig_diff + size_t(first) * ns);
    }
    HIPCHK(c, hipGetLastError());
    if (int e = finish(c)) return e;
  }
  if (int e = report_rig_diff(c, what, n_frames, ns)) return e;   // nothing is solved, nothing downloaded
  std::vector<const uint8_t*> dl(W), dr(W);
  std::vector<uint8_t*> dout(W);
  for (int wv = 0; wv < nwaves; ++wv) {
    const int first = wv * W, count = std::min(W, n_frames - first);
    if (wv > 1) {   // into the set wave wv - 2 has left
      if (overlap) {
        if (pre.join()) return fail(c, PF_ERR_DEVICE, "%s: the upload of wave %d beside wave %d's compute failed: %s", what, wv, wv - 1, hipGetErrorString(pre.err));
      } else {
        CallGuard guard_(c);
        if (int e = upload_wave(wv)) return e;
        if (int e = finish(c)) return e;   // the lanes' streams start from complete inputs
      }
    }
    if (overlap && wv >= 1 && wv + 1 < nwaves) prefetch_wave(wv + 1);
    const uint8_t* const* slot = in.data() + (wv & 1) * set_len;
    for (int i = 0; i < ns; ++i) {
      for (int w = 0; w < count; ++w) {
        dl[w] = slot[size_t(w) * (ns + 1) + i + 1];
        dr[w] = i == 0 ? slot[size_t(w) * (ns + 1)] : comp[w * 2 + ((i - 1) & 1)];
        dout[w] = comp[w * 2 + (i & 1)];
      }
      if (int e = rig_wave_step(c, rig, i, count, dl.data(), dr.data(), dout.data(), cols, rows, max_pct, in_flight, what)) return e;
      bool any = false;
      for (int w = 0; out && w < count; ++w) any = any || out[size_t(first + w) * ns + i];
      if (!any) continue;
      CallGuard guard_(c);
      for (int w = 0; w < count; ++w)
        if (uint8_t* o = out[size_t(first + w) * ns + i]) if (int e = down_plane(c, o, ostep, dout[w], cols, rows, 4)) return e;
      HIPCHK(c, hipGetLastError());
      if (int e = finish(c)) return e;
    }
  }
  return 0;
}

int pf_rig_stitch_batch_dev(pf_ctx* c, const pf_rig_plan* rig, int n_frames, const uint8_t* const* d_top, const uint8_t* const* d_l, int cols, int rows,
                            int max_pct, uint8_t* const* d_out, int in_flight) {
  const char* const what = "pf_rig_stitch_batch_dev";
  if (int e = use(c)) return e;
  c->vis_step_valid = false;
  if (n_frames < 0 || !d_top || !d_l || !d_out) return fail(c, PF_ERR_ARG, "bad argument");
  if (int e = check_rig(c, rig, cols, rows, what)) return e;
  if (n_frames == 0) return 0;
  const int ns = rig->n_steps;
  if (int e = check_stitch_canvas(c, cols, rows, max_pct)) return e;
  const size_t n = size_t(cols) * rows, bytes = n * 4;
  std::vector<const uint8_t*> img(size_t(n_frames) * (ns + 1));   // the verifying launch's table: frame-major (top, L_1 .. L_n)
  std::vector<uint8_t*> outs;                                     // the caller's composites
  for (int k = 0; k < n_frames; ++k) {
    if (!d_top[k]) return fail(c, PF_ERR_ARG, "null device pointer (frame %d)", k);
    img[size_t(k) * (ns + 1)] = d_top[k];
    for (int i = 0; i < ns; ++i) {
      if (!d_l[size_t(k) * ns + i]) return fail(c, PF_ERR_ARG, "null device pointer (frame %d, step %d)", k, i + 1);
      img[size_t(k) * (ns + 1) + i + 1] = d_l[size_t(k) * ns + i];
      if (uint8_t* o = d_out[size_t(k) * ns + i]) outs.push_back(o);
    }
    if (!d_out[size_t(k) * ns + ns - 1]) return fail(c, PF_ERR_ARG, "frame %d: the last step's d_out must not be NULL", k);
  }
  if (int e = check_dev_align(c, what, "image", img.data(), img.size())) return e;
  if (int e = check_dev_align(c, what, "d_out", outs.data(), outs.size())) return e;
  // a composite is written while inputs of the call are still read: no aliasing (the rules of pf_stitch_step_batch_dev)
  for (size_t a = 0; a < outs.size(); ++a) {
    for (size_t j = 0; j < img.size(); ++j)
      if (overlaps(outs[a], img[j], bytes)) return fail(c, PF_ERR_ARG, "a d_out of the call overlaps an input of the call (frame %d)", (int)(j / (ns + 1)));
    for (size_t b = a + 1; b < outs.size(); ++b)
      if (overlaps(outs[a], outs[b], bytes)) return fail(c, PF_ERR_ARG, "two d_out entries of the call overlap");
  }
  const int W = clamp_in_flight(in_flight, n_frames), nwaves = (n_frames + W - 1) / W;
  std::vector<uint8_t*> comp(size_t(W) * 2);
  for (int w = 0; w < W; ++w)
    for (int j = 0; j < 2; ++j) if (!(comp[w * 2 + j] = rig_slot(c, "c", w, j, bytes))) return PF_ERR_NOMEM;
  const uint8_t** tbl = (const uint8_t**)ensure(c, "rg_tbl", img.size() * sizeof(void*));
  if (!tbl) return PF_ERR_NOMEM;
  if (int e = rig_diff_words(c, size_t(n_frames) * ns)) return e;
  {
    CallGuard guard_(c);
    HIPCHK(c, hipMemcpyAsync(tbl, img.data(), img.size() * sizeof(void*), hipMemcpyHostToDevice, c->s_main));
    const bool vec = all_aligned16(img.data(), img.size());
    for (int first = 0; first < n_frames; first += 32768) {   // (one launch for any call below the grid's z limit)
      PROF(c, c->s_main, "rig_verify");
      launch_rig_maps_verify(c->s_main, tbl + size_t(first) * (ns + 1), vec, rig_maps(rig), ns, std::min(32768, n_frames - first), cols, rows,
                             c->d_rig_diff + size_t(first) * ns);
    }
    HIPCHK(c, hipGetLastError());
    if (int e = finish(c)) return e;
  }
  // the call fails as a whole before any solve; the caller's buffers are cleared, as the planned device form clears them
  if (int e = report_rig_diff(c, what, n_frames, ns)) return clear_outputs(c, e, outs.data(), outs.size(), bytes);
  std::vector<const uint8_t*> dl(W), dr(W);
  std::vector<uint8_t*> dout(W);
  for (int wv = 0; wv < nwaves; ++wv) {
    const int first = wv * W, count = std::min(W, n_frames - first);
    std::vector<int> tog(count, 0);
    for (int i = 0; i < ns; ++i) {
      for (int w = 0; w < count; ++w) {
        const size_t k = size_t(first + w);
        dl[w] = d_l[k * ns + i];
        dr[w] = i == 0 ? d_top[k] : dout[w];   // the previous step's composite, wherever it went
        uint8_t* o = d_out[k * ns + i];
        if (!o) { o = comp[w * 2 + tog[w]]; tog[w] ^= 1; }   // never the plane the previous step wrote
        dout[w] = o;
      }
      if (int e = rig_wave_step(c, rig, i, count, dl.data(), dr.data(), dout.data(), cols, rows, max_pct, in_flight, what)) return e;
    }
  }
  return 0;
}
int pf_rig_set_upload_overlap(pf_ctx* c, int on) {
  if (!c) return fail(nullptr, PF_ERR_ARG, "null context");
  c->rig_overlap_uploads = on != 0;
  return 0;
}
int pf_rig_stitch(pf_ctx* c, const pf_rig_plan* rig, const uint8_t* top, const uint8_t* const* l, int cols, int rows, size_t step, int max_pct, uint8_t* const* out,
                  size_t ostep) {
  return pf_rig_stitch_batch(c, rig, 1, top ? &top : nullptr, l, cols, rows, step, max_pct, out, ostep, 1);
}
int pf_rig_stitch_dev(pf_ctx* c, const pf_rig_plan* rig, const uint8_t* d_top, const uint8_t* const* d_l, int cols, int rows, int max_pct, uint8_t* const* d_out) {
  return pf_rig_stitch_batch_dev(c, rig, 1, d_top ? &d_top : nullptr, d_l, cols, rows, max_pct, d_out, 1);
}
