// Baseline JPEG decoded on the device: the file's bytes in HBM -> packed BGRA, byte for byte libjpeg's own output.
// A baseline scan is one serial Huffman stream, so the entropy segment is cut into subsequences of S bytes, one lane each:
//   k_jpegd_sync    self-synchronising decode.  A lane walks its subsequence from a guessed state (block 0 of an MCU, coefficient 0) and
//                   records where and in which state it leaves it; in the next rounds it walks again from its predecessor's exit state,
//                   until no exit state changes.  Subsequence 0 is true from the start and every RSTn a lane meets makes it true, so the
//                   fixed point is the serial decode.  Rounds inside a workgroup use barriers; no workgroup waits for another: states
//                   cross workgroups between launches (two state arrays, read one, write the other), and the host launches again while
//                   the "changed" word is set.
//   k_jpegd_place   exclusive prefix sums of the lanes' completed blocks and crossed markers: every lane's first block and interval
//   k_jpegd_write   every lane walks once more from its now true entry state and stores the coefficients, 64 int16 per block in MCU
//                   order (k_jpeg_blocks's layout), zigzag order, DC as differences; the first event of the true path goes to a status word
//   k_jpegd_dc      segmented prefix sum of the DC differences per component, the segments being the restart intervals; chunks of 2048
//                   differences, two passes (chunk sums, then values) where an interval holds more than one
//   k_jpegd_idct    dequantisation and jidctint, 8 lanes per block, into component planes at their block-padded sizes
//   k_jpegd_pixels  libjpeg's fancy upsampling over the real samples (edges replicate), the colour transform, BGRA dwords
// The RSTn markers need no pass of their own: a lane that stands at an MCU boundary with fewer than 8 bits before a marker steps over it,
// and the write pass checks every marker against the interval the prefix sums give it.
// Every loop is bounded by the segment's bytes (a code word consumes a bit, or the walk steps over a marker, or it ends); reads are
// clamped to the segment, writes to the block count the header implies.  A lane's reader lives in its registers across the barriers.
// Plain C++ throughout: the host-run test (tests/cpp/jpegd_kernels_host.cpp) compiles this file as it is.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pf_common.hpp"
#include "jpeg_parse.hpp"

namespace pf {
namespace {

using jpeg_parse::DTab;
using jpeg_parse::Tables;

constexpr int kJdThreads = (int)kJpegdLanes;            // lanes (subsequences) per workgroup of the entropy kernels
constexpr unsigned kJdInfinite = 0xFFFFFFFFu;

struct JdState { uint32_t bp, st, nblk, nmark; };   // exit bit, block in MCU | zigzag index << 8, blocks completed, markers crossed

struct JdGeom {
  uint32_t seg_bytes, S, nsub;
  int ncomp, hs, vs, bpm;
  uint32_t restart, nmcu, nint, nblocks, mcu_cols, mcu_rows, cols, rows;
};

__device__ __forceinline__ JdGeom jd_geom(const JpegdWork& w) {
  JdGeom g;
  g.seg_bytes = w.seg_bytes; g.S = w.S; g.nsub = w.nsub; g.ncomp = w.ncomp; g.hs = w.hs; g.vs = w.vs; g.bpm = w.ncomp == 3 ? w.hs * w.vs + 2 : 1;
  g.restart = w.restart; g.cols = w.cols; g.rows = w.rows;
  g.mcu_cols = (w.cols + 8 * w.hs - 1) / (8 * w.hs); g.mcu_rows = (w.rows + 8 * w.vs - 1) / (8 * w.vs);
  g.nmcu = g.mcu_cols * g.mcu_rows; g.nblocks = g.nmcu * g.bpm; g.nint = w.restart ? (g.nmcu + w.restart - 1) / w.restart : 1;
  return g;
}

// ---- the bit reader: 64 bits at the top of acc, the file's bytes below it.  sacc marks, at the last bit of an 0xFF data byte, that a
// stuffing byte follows it: the raw bit position of the next unread bit is then pos * 8 - nbits - 8 * popcount(sacc). ----
struct JdReader {
  const uint8_t* d; uint32_t lim, pos; uint64_t acc, sacc; int nbits; bool mark;   // mark: the next byte is a marker, or the segment's end
};

__device__ __forceinline__ void jd_fill(JdReader& r) {
  while (r.nbits <= 56 && !r.mark) {
    if (r.pos >= r.lim) { r.mark = true; break; }
    const uint32_t b = r.d[r.pos];
    if (b == 0xFF) {
      const uint32_t nb = r.pos + 1 < r.lim ? r.d[r.pos + 1] : 0xD9u;
      if (nb != 0) { r.mark = true; break; }
      r.pos += 2; r.sacc |= uint64_t(1) << (56 - r.nbits);
    } else {
      r.pos += 1;
    }
    r.acc |= uint64_t(b) << (56 - r.nbits); r.nbits += 8;
  }
}
__device__ __forceinline__ void jd_skip(JdReader& r, int n) { r.acc <<= n; r.sacc <<= n; r.nbits -= n; }
__device__ __forceinline__ uint32_t jd_bit(const JdReader& r) { return r.pos * 8u - (uint32_t)r.nbits - 8u * (uint32_t)__popcll(r.sacc); }
__device__ __forceinline__ void jd_open(JdReader& r, const uint8_t* seg, uint32_t lim, uint32_t bp) {
  r.d = seg; r.lim = lim; r.pos = min(bp >> 3, lim); r.acc = 0; r.sacc = 0; r.nbits = 0; r.mark = false;
  jd_fill(r);
  const int drop = min((int)(bp & 7), r.nbits);
  jd_skip(r, drop);
}

__device__ __forceinline__ void jd_event(unsigned* status, uint32_t mcu) { atomicMin(status, mcu); }

// One lane's walk from `in` (its bp and st) until a code word starts at or beyond end_bit.  WRITE: the true path -- coefficients are
// stored from block B0 on, markers are counted from interval k0 on, and the first event ends the lane.
template <bool WRITE>
__device__ JdState jd_walk(const uint8_t* seg, const JdGeom& g, const Tables* tab, uint32_t in_bp, uint32_t in_st, uint32_t end_bit, uint32_t B0, uint32_t k0,
                           int16_t* coef, unsigned* status) {
  JdReader r;
  jd_open(r, seg, g.seg_bytes, in_bp);
  int blk = min((int)(in_st & 0xff), g.bpm - 1), z = min((int)(in_st >> 8), 63);
  uint32_t nblk = 0, nmark = 0, last_cross = kJdInfinite;
  for (;;) {
    jd_fill(r);
    if (r.mark && r.nbits < 8 && blk == 0 && z == 0) {
      // an MCU boundary before a marker, or the segment's end
      if (r.pos >= r.lim) {
        if (WRITE && (B0 + nblk != g.nblocks || k0 + nmark != g.nint - 1)) jd_event(status, (B0 + nblk) / g.bpm);
        JdState s = {g.seg_bytes * 8u, 0u, nblk, nmark};
        return s;
      }
      if (WRITE) {
        const uint32_t B = B0 + nblk, k = k0 + nmark;
        const uint32_t marker = r.pos + 1 < r.lim ? r.d[r.pos + 1] : 0u;
        if (k + 1 >= g.nint || B != (uint64_t)(k + 1) * g.restart * g.bpm || marker != 0xD0u + (k & 7u) || B == last_cross) {
          jd_event(status, B / g.bpm);
          JdState s = {g.seg_bytes * 8u, 0u, nblk, nmark};
          return s;
        }
        last_cross = B;
      }
      r.pos = min(r.pos + 2, r.lim); r.acc = 0; r.sacc = 0; r.nbits = 0; r.mark = false;
      ++nmark;
      continue;
    }
    const uint32_t cur = jd_bit(r);
    if (cur >= end_bit) {
      JdState s = {cur, (uint32_t)blk | ((uint32_t)z << 8), nblk, nmark};
      return s;
    }
    const uint32_t B = B0 + nblk;
    if (WRITE && B >= g.nblocks) {   // data beyond the last MCU
      jd_event(status, g.nmcu);
      JdState s = {g.seg_bytes * 8u, 0u, nblk, nmark};
      return s;
    }
    const int comp = g.ncomp == 3 ? max(0, blk - (g.bpm - 3)) : 0;
    const DTab& t = z == 0 ? tab->dc[comp] : tab->ac[comp];
    const uint32_t peek = (uint32_t)(r.acc >> 48);
    int len; uint32_t sym; bool bad = false;
    const uint32_t e = t.look[peek >> 8];
    if (e) { len = (int)(e >> 8); sym = e & 0xff; }
    else {
      len = 9;
      while (len <= 16 && (int32_t)(peek >> (16 - len)) > t.maxcode[len]) ++len;
      if (len > 16) { len = 16; sym = 0; bad = true; }   // no such code: sixteen bits, symbol 0 (never reported from a guessed walk)
      else sym = t.vals[((peek >> (16 - len)) + (uint32_t)t.valoff[len]) & 0xff];
    }
    const int s = (int)(sym & 15), run = (int)(sym >> 4);   // (a DC symbol is at most 15: the parser refuses any other table)
    int v = 0;
    if (s) {
      v = (int)((r.acc << len) >> (64 - s));
      if (v < (1 << (s - 1))) v = v - (1 << s) + 1;
    }
    jd_skip(r, len + s);
    bool event = bad;
    if (r.nbits < 0) {
      // the bits ran out inside an MCU: the walk goes on behind the marker, at an MCU's start
      if (WRITE) { jd_event(status, B / g.bpm); JdState st = {g.seg_bytes * 8u, 0u, nblk, nmark}; return st; }
      if (r.pos >= r.lim) { JdState st = {g.seg_bytes * 8u, 0u, nblk, nmark}; return st; }
      r.pos = min(r.pos + 2, r.lim); r.acc = 0; r.sacc = 0; r.nbits = 0; r.mark = false;
      ++nmark; blk = 0; z = 0;
      continue;
    }
    bool done = false;
    if (z == 0) {
      if (WRITE && !event) coef[(size_t)B * 64] = (int16_t)v;
      z = 1;
    } else if (s) {
      if (z + run > 63) { event = true; done = true; }
      else { z += run; if (WRITE && !event) coef[(size_t)B * 64 + z] = (int16_t)v; ++z; done = z >= 64; }
    } else if (run == 15) {
      if (z + 16 > 64) { event = true; done = true; }
      else { z += 16; done = z >= 64; }
    } else {
      done = true;
    }
    if (WRITE && event) { jd_event(status, B / g.bpm); JdState st = {g.seg_bytes * 8u, 0u, nblk, nmark}; return st; }
    if (done) { z = 0; blk = blk + 1 == g.bpm ? 0 : blk + 1; ++nblk; }
  }
}

__device__ __forceinline__ void jd_stage_tables(Tables* dst, const Tables* src) {
  const uint32_t* s = (const uint32_t*)src; uint32_t* d = (uint32_t*)dst;
  for (unsigned k = threadIdx.x; k < sizeof(Tables) / 4; k += kJdThreads) d[k] = s[k];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// words: [0] changed, [1] the most rounds any workgroup of this launch ran, [3] += lanes whose record changed after their first walk
__global__ __launch_bounds__(kJdThreads) void k_jpegd_sync(JpegdWork w, int first, const JdState* in, JdState* out) {
  __shared__ Tables s_tab;
  __shared__ JdState s_exit[kJdThreads];
  const JdGeom g = jd_geom(w);
  jd_stage_tables(&s_tab, (const Tables*)w.tables);
  const unsigned tid = threadIdx.x, i = blockIdx.x * kJdThreads + tid;
  const bool active = i < g.nsub;
  const uint32_t end_bit = i + 1 >= g.nsub ? kJdInfinite : (i + 1) * g.S * 8u;
  JdState rec = {0, 0, 0, 0}, before = {0, 0, 0, 0}, border = {0, 0, 0, 0};
  uint32_t last_bp = kJdInfinite, last_st = kJdInfinite;   // the entry state `rec` was walked from
  if (active && !first) {
    rec = before = in[i];
    if (i > 0) { const JdState p = in[i - 1]; if (tid == 0) border = p; else { last_bp = p.bp; last_st = p.st; } }
    else { last_bp = 0; last_st = 0; }
  }
  s_exit[tid] = rec;
  unsigned rounds = 0;
  bool moved = false;   // the record changed after the lane's first walk: its guess had not been true
  for (int round = 0; round <= kJdThreads; ++round) {
    __syncthreads();
    bool need = false; uint32_t e_bp = 0, e_st = 0;
    if (active) {
      if (first && round == 0) { e_bp = i * g.S * 8u; e_st = 0; need = true; }                   // the guess; true for subsequence 0
      else if (i == 0) need = false;
      else if (tid == 0) { e_bp = border.bp; e_st = border.st; need = !first && round == 0; }       // what the workgroup before left
      else { e_bp = s_exit[tid - 1].bp; e_st = s_exit[tid - 1].st; need = e_bp != last_bp || e_st != last_st; }
    }
    __syncthreads();
    int ch = 0;
    if (need) {
      const JdState x = jd_walk<false>(w.seg, g, &s_tab, e_bp, e_st, end_bit, 0, 0, nullptr, nullptr);
      last_bp = e_bp; last_st = e_st;
      if (x.bp != rec.bp || x.st != rec.st || x.nblk != rec.nblk || x.nmark != rec.nmark || (first && round == 0)) { rec = x; s_exit[tid] = x; ch = 1; moved = moved || !(first && round == 0); }
    }
    ++rounds;
    if (!__syncthreads_or(ch)) break;
  }
  if (active) {
    out[i] = rec;
    if (first || rec.bp != before.bp || rec.st != before.st || rec.nblk != before.nblk || rec.nmark != before.nmark) atomicOr(&w.words[0], 1u);
  }
  if (moved) atomicAdd(&w.words[3], 1u);
  if (tid == 0) atomicMax(&w.words[1], rounds);
}

// one workgroup: first[i] = (blocks, markers) before subsequence i
__global__ __launch_bounds__(1024) void k_jpegd_place(const JdState* st, uint32_t n, uint32_t* first) {
  __shared__ uint32_t s_b[1024], s_m[1024];
  const uint32_t t = threadIdx.x, per = (n + 1023) / 1024, lo = min(n, t * per), hi = min(n, lo + per);
  uint32_t b = 0, m = 0;
  for (uint32_t i = lo; i < hi; ++i) { b += st[i].nblk; m += st[i].nmark; }
  s_b[t] = b; s_m[t] = m;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint32_t ab = t >= d ? s_b[t - d] : 0, am = t >= d ? s_m[t - d] : 0;
    __syncthreads();
    s_b[t] += ab; s_m[t] += am;
    __syncthreads();
  }
  b = s_b[t] - b; m = s_m[t] - m;
  for (uint32_t i = lo; i < hi; ++i) { first[2 * i] = b; first[2 * i + 1] = m; b += st[i].nblk; m += st[i].nmark; }
}

// words[2]: the MCU of the first event of the true path (kJdNoEvent: none)
__global__ __launch_bounds__(kJdThreads) void k_jpegd_write(JpegdWork w, const JdState* st, const uint32_t* first) {
  __shared__ Tables s_tab;
  const JdGeom g = jd_geom(w);
  jd_stage_tables(&s_tab, (const Tables*)w.tables);
  __syncthreads();
  const unsigned i = blockIdx.x * kJdThreads + threadIdx.x;
  if (i >= g.nsub) return;
  const uint32_t end_bit = i + 1 >= g.nsub ? kJdInfinite : (i + 1) * g.S * 8u;
  const uint32_t bp = i ? st[i - 1].bp : 0, s = i ? st[i - 1].st : 0;
  jd_walk<true>(w.seg, g, &s_tab, bp, s, end_bit, first[2 * i], first[2 * i + 1], w.coef, &w.words[2]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// a workgroup per (interval, component): the component's DC differences of the interval, in MCU order, become values
constexpr unsigned kJdDcChunk = 2048;   // DC differences per workgroup: 8 per thread

// PASS 0: the sum of the chunk's differences -> sums[blockIdx.x].  PASS 1: the chunk's differences become values, on top of the sums of
// the chunks before it in the same (interval, component).  `chunks`: workgroups per (interval, component); one that lies beyond its
// interval's elements has nothing to do.  Unsigned arithmetic: the sums wrap as libjpeg's JCOEF does, whatever a hostile stream holds.
template <int PASS>
__global__ __launch_bounds__(256) void k_jpegd_dc(JpegdWork w, unsigned chunks, unsigned* sums) {
  __shared__ unsigned s_sum[256];
  const JdGeom g = jd_geom(w);
  const uint32_t chunk = blockIdx.x % chunks, seq = blockIdx.x / chunks;
  const uint32_t interval = seq / g.ncomp; const int comp = (int)(seq % g.ncomp);
  const uint32_t m0 = g.restart ? interval * g.restart : 0, m1 = g.restart ? min(g.nmcu, m0 + g.restart) : g.nmcu;
  const uint32_t per_mcu = comp == 0 ? (uint32_t)(g.bpm - (g.ncomp - 1)) : 1u, off = comp == 0 ? 0u : (uint32_t)(g.bpm - 3 + comp);
  const uint32_t L = (m1 - m0) * per_mcu, t = threadIdx.x, c0 = min(L, chunk * kJdDcChunk), c1 = min(L, c0 + kJdDcChunk);
  const uint32_t per = kJdDcChunk / 256, lo = min(c1, c0 + t * per), hi = min(c1, lo + per);
  int16_t* coef = w.coef;
  unsigned sum = 0;
  for (uint32_t e = lo; e < hi; ++e) sum += (unsigned)(int)coef[((size_t)(m0 + e / per_mcu) * g.bpm + off + e % per_mcu) * 64];
  s_sum[t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const unsigned a = t >= d ? s_sum[t - d] : 0;
    __syncthreads();
    s_sum[t] += a;
    __syncthreads();
  }
  if (PASS == 0) {
    if (t == 255) sums[blockIdx.x] = s_sum[255];
    return;
  }
  unsigned acc = s_sum[t] - sum;
  for (uint32_t q = 0; q < chunk; ++q) acc += sums[seq * chunks + q];
  for (uint32_t e = lo; e < hi; ++e) {
    int16_t* p = coef + ((size_t)(m0 + e / per_mcu) * g.bpm + off + e % per_mcu) * 64;
    acc += (unsigned)(int)*p; *p = (int16_t)acc;   // (int16 wrap-around, as libjpeg's JCOEF holds it)
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
static __device__ const uint8_t kJdZigOf[64] = {   // natural index -> zigzag index
    0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// one pass of jidctint over c[0..7]; unsigned arithmetic, so that a hostile stream wraps instead of overflowing
__device__ __forceinline__ void jd_idct8(const uint32_t* c, int shift, int* o) {
  uint32_t z2 = c[2], z3 = c[6];
  uint32_t z1 = (z2 + z3) * 4433u;
  uint32_t t2 = z1 + z3 * (uint32_t)-15137, t3 = z1 + z2 * 6270u;
  uint32_t t0 = (c[0] + c[4]) << 13, t1 = (c[0] - c[4]) << 13;
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = c[7]; t1 = c[5]; t2 = c[3]; t3 = c[1];
  z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2; uint32_t z4 = t1 + t3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  t0 *= 2446u; t1 *= 16819u; t2 *= 25172u; t3 *= 12299u;
  z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995; z3 = z3 * (uint32_t)-16069 + z5; z4 = z4 * (uint32_t)-3196 + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  const uint32_t rnd = 1u << (shift - 1);
  o[0] = (int32_t)(t10 + t3 + rnd) >> shift; o[7] = (int32_t)(t10 - t3 + rnd) >> shift;
  o[1] = (int32_t)(t11 + t2 + rnd) >> shift; o[6] = (int32_t)(t11 - t2 + rnd) >> shift;
  o[2] = (int32_t)(t12 + t1 + rnd) >> shift; o[5] = (int32_t)(t12 - t1 + rnd) >> shift;
  o[3] = (int32_t)(t13 + t0 + rnd) >> shift; o[4] = (int32_t)(t13 - t0 + rnd) >> shift;
}

constexpr int kJdIdctBlocks = 32;   // blocks per workgroup of 256: 8 lanes each
constexpr int kJdWsStride = 65;

__device__ __forceinline__ size_t jd_plane_bytes_y(const JdGeom& g) { return (size_t)g.mcu_cols * g.hs * 8 * g.mcu_rows * g.vs * 8; }
__device__ __forceinline__ size_t jd_plane_bytes_c(const JdGeom& g) { return (size_t)g.mcu_cols * 8 * g.mcu_rows * 8; }

__global__ __launch_bounds__(256) void k_jpegd_idct(JpegdWork w) {
  __shared__ int s_ws[kJdIdctBlocks * kJdWsStride];
  const JdGeom g = jd_geom(w);
  const Tables* tab = (const Tables*)w.tables;
  const unsigned lb = threadIdx.x >> 3, l = threadIdx.x & 7;
  const uint32_t b = blockIdx.x * kJdIdctBlocks + lb;
  const bool active = b < g.nblocks;
  const uint32_t m = active ? b / g.bpm : 0; const int j = active ? (int)(b % g.bpm) : 0;
  const int comp = g.ncomp == 3 ? max(0, j - (g.bpm - 3)) : 0;
  int* ws = s_ws + lb * kJdWsStride;
  if (active) {
    const int16_t* c = w.coef + (size_t)b * 64;
    const uint8_t* q = tab->quant[comp];
    uint32_t col[8]; int o[8];
    for (int r = 0; r < 8; ++r) { const int zz = kJdZigOf[r * 8 + l]; col[r] = (uint32_t)((int)c[zz] * (int)q[zz]); }
    jd_idct8(col, 11, o);
    for (int r = 0; r < 8; ++r) ws[r * 8 + l] = o[r];
  }
  __syncthreads();
  if (!active) return;
  uint32_t row[8]; int o[8];
  for (int k = 0; k < 8; ++k) row[k] = (uint32_t)ws[l * 8 + k];
  jd_idct8(row, 18, o);
  uint32_t lo = 0, hi = 0;
  for (int k = 0; k < 4; ++k) { lo |= (uint32_t)min(255, max(0, o[k] + 128)) << (8 * k); hi |= (uint32_t)min(255, max(0, o[k + 4] + 128)) << (8 * k); }
  const uint32_t mx = m % g.mcu_cols, my = m / g.mcu_cols;
  uint8_t* plane; size_t width, bx, by;
  if (comp == 0) { plane = w.planes; width = (size_t)g.mcu_cols * g.hs * 8; bx = (size_t)mx * g.hs + j % g.hs; by = (size_t)my * g.vs + j / g.hs; }
  else { plane = w.planes + jd_plane_bytes_y(g) + (comp - 1) * jd_plane_bytes_c(g); width = (size_t)g.mcu_cols * 8; bx = mx; by = my; }
  uint32_t* dst = (uint32_t*)(plane + (by * 8 + l) * width + bx * 8);
  dst[0] = lo; dst[1] = hi;
}

// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int jd_fix(double x) { return int(x * 65536 + 0.5); }

// one chroma sample at (x, y) of the image: libjpeg's triangle filter over the cw x ch real samples of `p` (rows `width` apart);
// at most two samples a row: plain replication, as libjpeg chooses there
__device__ __forceinline__ int jd_chroma(const uint8_t* p, size_t width, int cw, int ch, int hs, int vs, int x, int y) {
  if (hs == 1) return p[(size_t)y * width + x];
  const int cx = x >> 1;
  if (vs == 1) {
    const uint8_t* row = p + (size_t)y * width;
    if (cw <= 2) return row[cx];
    const int nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
    return (3 * row[cx] + row[nx] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int cy = y >> 1;
  if (cw <= 2) return p[(size_t)cy * width + cx];
  const int nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0), ny = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
  const uint8_t* r0 = p + (size_t)cy * width; const uint8_t* r1 = p + (size_t)ny * width;
  const int s = 3 * r0[cx] + r1[cx], sn = 3 * r0[nx] + r1[nx];
  return (3 * s + sn + ((x & 1) ? 7 : 8)) >> 4;
}

__global__ __launch_bounds__(256) void k_jpegd_pixels(JpegdWork w, uint32_t* bgra) {
  const JdGeom g = jd_geom(w);
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= g.cols * g.rows) return;
  const int x = (int)(idx % g.cols), y = (int)(idx / g.cols);
  const size_t yw = (size_t)g.mcu_cols * g.hs * 8, cwid = (size_t)g.mcu_cols * 8;
  const int Y = w.planes[(size_t)y * yw + x];
  int R = Y, G = Y, B = Y;
  if (g.ncomp == 3) {
    const uint8_t* pcb = w.planes + jd_plane_bytes_y(g); const uint8_t* pcr = pcb + jd_plane_bytes_c(g);
    const int cw = (int)((g.cols + g.hs - 1) / g.hs), ch = (int)((g.rows + g.vs - 1) / g.vs);
    const int cb = jd_chroma(pcb, cwid, cw, ch, g.hs, g.vs, x, y) - 128, cr = jd_chroma(pcr, cwid, cw, ch, g.hs, g.vs, x, y) - 128;
    R = Y + ((jd_fix(1.402) * cr + 32768) >> 16);
    B = Y + ((jd_fix(1.772) * cb + 32768) >> 16);
    G = Y + ((-jd_fix(0.34414) * cb - jd_fix(0.71414) * cr + 32768) >> 16);
  }
  // clamp first, then shift
  const uint32_t b8 = (uint32_t)min(255, max(0, B)), g8 = (uint32_t)min(255, max(0, G)), r8 = (uint32_t)min(255, max(0, R));
  bgra[idx] = b8 | (g8 << 8) | (r8 << 16) | 0xFF000000u;
}

}  // namespace

unsigned jpegd_dc_chunks(int ncomp, int hs, int vs, unsigned restart, unsigned nmcu) {
  const unsigned longest = (restart ? std::min(restart, nmcu) : nmcu) * (ncomp == 3 ? (unsigned)(hs * vs) : 1u);
  return std::max(1u, (longest + kJdDcChunk - 1) / kJdDcChunk);
}
void launch_jpegd_sync(hipStream_t st, const JpegdWork& w, int first, int from) {
  hipLaunchKernelGGL(k_jpegd_sync, dim3((w.nsub + kJdThreads - 1) / kJdThreads), dim3(kJdThreads), 0, st, w, first, (const JdState*)w.states[from], (JdState*)w.states[1 - from]);
}
void launch_jpegd_write(hipStream_t st, const JpegdWork& w, int from) {
  hipLaunchKernelGGL(k_jpegd_place, dim3(1), dim3(1024), 0, st, (const JdState*)w.states[from], w.nsub, (uint32_t*)w.first);
  hipLaunchKernelGGL(k_jpegd_write, dim3((w.nsub + kJdThreads - 1) / kJdThreads), dim3(kJdThreads), 0, st, w, (const JdState*)w.states[from], (const uint32_t*)w.first);
}
void launch_jpegd_pixels(hipStream_t st, const JpegdWork& w, uint8_t* bgra) {
  const uint32_t mcu_cols = (w.cols + 8 * w.hs - 1) / (8 * w.hs), mcu_rows = (w.rows + 8 * w.vs - 1) / (8 * w.vs), nmcu = mcu_cols * mcu_rows;
  const uint32_t nblocks = nmcu * (w.ncomp == 3 ? w.hs * w.vs + 2 : 1), nint = w.restart ? (nmcu + w.restart - 1) / w.restart : 1;
  const unsigned chunks = jpegd_dc_chunks(w.ncomp, w.hs, w.vs, w.restart, nmcu);
  if (chunks > 1) hipLaunchKernelGGL(k_jpegd_dc<0>, dim3(nint * w.ncomp * chunks), dim3(256), 0, st, w, chunks, w.dcsum);
  hipLaunchKernelGGL(k_jpegd_dc<1>, dim3(nint * w.ncomp * chunks), dim3(256), 0, st, w, chunks, w.dcsum);
  hipLaunchKernelGGL(k_jpegd_idct, dim3((nblocks + kJdIdctBlocks - 1) / kJdIdctBlocks), dim3(256), 0, st, w);
  if (bgra) hipLaunchKernelGGL(k_jpegd_pixels, dim3((w.cols * w.rows + 255) / 256), dim3(256), 0, st, w, (uint32_t*)bgra);
}

}  // namespace pf
