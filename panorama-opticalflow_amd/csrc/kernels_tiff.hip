// TIFF decoder on the device (gfx950): the strips of a file decode in parallel, one workgroup each (LZW, PackBits), then one workgroup
// per row undoes the predictor and stores BGRA.  The host (pf_api_tiff.inl, tiff_parse.hpp) parses the IFD and uploads the file's bytes
// and its strip tables.  Only workgroup-level primitives are used -- __syncthreads and integer atomics on LDS -- and no wave intrinsics,
// so this source also compiles as plain C++ and runs thread for thread on the host (tests/cpp/tiff_kernels_host.cpp).  A strip's output
// and status are a function of its bytes alone: no result depends on the order of workgroups.
//
// Bounds are the kernels' own: every read of the file is clamped to the strip's [offset, offset + count) and to the file, every write and
// every copy source to the strip's expected rows_in_strip * cols * samples bytes.  Every loop either consumes input or leaves.
#include <algorithm>

#include "pf_common.hpp"

namespace pf {
namespace {

constexpr int kStripThreads = 64;   // one workgroup per strip; also the number of LZW codes in a batch
constexpr int kLzwTable = 4096;
constexpr int kRowThreads = 256;

struct Strip {
  const uint8_t* src;   // the strip's compressed bytes
  uint32_t count;       // ... how many, clamped to the file
  uint32_t expect;      // bytes the strip decodes to
  uint8_t* out;         // its place in the samples plane
};
__device__ __forceinline__ Strip strip_of(const TiffWork& w, int s) {
  Strip r;
  const unsigned long long off = w.offsets[s];
  unsigned long long cnt = w.counts[s];
  if (off >= w.bytes) cnt = 0; else if (cnt > w.bytes - off) cnt = w.bytes - off;
  r.src = w.file + (off < w.bytes ? off : 0);
  r.count = (uint32_t)cnt;
  const unsigned long long row = (unsigned long long)w.cols * w.samples, first = (unsigned long long)s * w.rows_per_strip;
  const unsigned long long nrows = std::min<unsigned long long>(w.rows_per_strip, (unsigned long long)w.rows - first);
  r.expect = (uint32_t)std::min<unsigned long long>(nrows * row, 0x7fffffffull);
  r.out = w.plane + first * row;
  return r;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// LZW (compression 5), the TIFF flavour tools/image_io.hpp lzw_decode implements: MSB-first codes of 9..12 bits, Clear 256, EOI 257,
// early change, a full table keeps decoding at 12 bits, a missing leading Clear is tolerated.
//
// Code j after a Clear (j = 0: the first one; the strip's start counts as a Clear) is read while the table holds
// min(4096, 258 + max(0, j - 1)) entries, so its width and bit offset are closed functions of j (lzw_width, lzw_offset: the same
// functions as tiff_parse.hpp's).  A batch is 64 consecutive codes, one per thread.  The entry made while code i is processed is the
// previous code's string plus the first byte of code i's: contiguous bytes of the strip's own output, starting where the previous code
// was written.  The table therefore holds (position, length) per entry -- 4096 x (4 + 2) bytes of LDS; an entry is never longer than
// the number of entries -- and decoding a code is a copy from an earlier output position.
__device__ __forceinline__ uint32_t lzw_width(unsigned long long j) { return 9 + (j >= 254) + (j >= 766) + (j >= 1790); }
__device__ __forceinline__ unsigned long long lzw_offset(unsigned long long j) {
  return 9 * j + (j > 254 ? j - 254 : 0) + (j > 766 ? j - 766 : 0) + (j > 1790 ? j - 1790 : 0);
}
enum { kEndClear = 0, kEndEoi = 1, kEndCut = 2, kEndBad = 3, kEndBadFull = 4 };
constexpr unsigned kNoEnd = kStripThreads * 8;

// the code of the batch (b_pos[0..m) ascending) that covers output position q: the last i with b_pos[i] <= q
__device__ __forceinline__ int covering(const uint32_t* b_pos, int m, uint32_t q) {
  int lo = 0, hi = m;   // the answer is in [lo, hi)
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (b_pos[mid] <= q) lo = mid; else hi = mid; }
  return lo;
}

__global__ __launch_bounds__(kStripThreads) void k_tiff_lzw(TiffWork w) {
  __shared__ uint32_t tab_pos[kLzwTable];
  __shared__ uint16_t tab_len[kLzwTable];
  __shared__ uint32_t b_code[kStripThreads], b_len[kStripThreads], b_src[kStripThreads], b_pos[kStripThreads + 1];
  __shared__ uint32_t scan[2][kStripThreads];
  __shared__ unsigned s_end, s_unres;
  const int tid = threadIdx.x;
  for (int s = blockIdx.x; s < w.n_strips; s += gridDim.x) {
    const Strip st = strip_of(w, s);
    const unsigned long long nbits = 8ull * st.count;
    // the decoder's state, held identically by every thread (all of it derives from LDS values read behind a barrier)
    unsigned long long cbit = 0;   // bit offset of code 0 after the last Clear
    uint32_t j = 0;                // codes consumed since then
    uint32_t outpos = 0;           // bytes produced
    uint32_t old_pos = 0, old_len = 0;   // the previous code's string; old_len == 0: there is none (start, or just cleared)
    unsigned reason = 0;
    while (true) {
      // -- 1. extract 64 codes; the first Clear / EOI / cut / impossible code ends the batch (min-reduction in LDS)
      if (tid == 0) s_end = kNoEnd;
      __syncthreads();   // (B1) s_end reset; the previous batch's LDS arrays are free (every thread is past its reads)
      const unsigned long long jt = (unsigned long long)j + tid, bo = cbit + lzw_offset(jt);
      const uint32_t wd = lzw_width(jt);
      uint32_t code = 0;
      if (bo + wd > nbits) atomicMin(&s_end, unsigned(tid * 8 + kEndCut));
      else {
        const unsigned long long B = bo >> 3;   // B + 2 may pass the strip's last byte when the code ends inside byte B + 1
        const uint32_t v = (uint32_t(st.src[B]) << 16) | (B + 1 < st.count ? uint32_t(st.src[B + 1]) << 8 : 0u) | (B + 2 < st.count ? uint32_t(st.src[B + 2]) : 0u);
        code = (v >> (24 - (uint32_t)(bo & 7) - wd)) & ((1u << wd) - 1);
        const uint32_t next = jt == 0 ? 258u : (uint32_t)std::min<unsigned long long>(kLzwTable, 257 + jt);   // entries when this code is read
        if (code == 256) atomicMin(&s_end, unsigned(tid * 8 + kEndClear));
        else if (code == 257) atomicMin(&s_end, unsigned(tid * 8 + kEndEoi));
        else if (jt == 0 ? code >= 256 : (code > next || code >= (uint32_t)kLzwTable)) atomicMin(&s_end, unsigned(tid * 8 + kEndBad));
        else if (code == next && next == (uint32_t)kLzwTable) atomicMin(&s_end, unsigned(tid * 8 + kEndBadFull));
      }
      b_code[tid] = code;
      __syncthreads();   // (B2) s_end final
      const unsigned end = s_end;
      const int m = (int)std::min(end >> 3, (unsigned)kStripThreads);   // codes 0..m-1 are data codes
      // -- 2. lengths: 1 for a literal, a table read for an entry made before the batch, len(code k-1) + 1 for the entry code k of this
      //       batch makes (k <= tid; k == tid is KwKwK).  Resolved in rounds: a round resolves every code whose dependency is resolved.
      const int k = (int)code - 257 - (int)j;   // the batch code that makes entry `code` (for code >= 258)
      bool pending = false;
      uint32_t len = 0;
      if (tid < m) {
        if (code < 256) len = 1;
        else if (k < 0) len = tab_len[code];
        else if (k == 0) len = old_len + 1;
        else pending = true;   // depends on b_len[k - 1], k - 1 < tid
      }
      b_len[tid] = len;
      for (int round = 0; round < kStripThreads; ++round) {
        if (tid == 0) s_unres = 0;
        __syncthreads();   // (L1) the lengths written so far are visible; the counter is reset
        uint32_t got = 0;
        if (pending) { got = b_len[k - 1]; if (!got) atomicAdd(&s_unres, 1u); }
        __syncthreads();   // (L2) every read of this round is done before any write; the counter is final
        if (pending && got) { len = got + 1; b_len[tid] = len; pending = false; }
        const unsigned left = s_unres;
        __syncthreads();   // (L3) everyone has the counter before it is reset; this round's lengths are visible
        if (!left) break;
      }
      // -- 3. positions: exclusive prefix sum of the lengths (codes past m have length 0)
      scan[0][tid] = len;
      int cur = 0;
      for (int d = 1; d < kStripThreads; d <<= 1) {
        __syncthreads();   // (S) the previous step's sums are visible
        scan[cur ^ 1][tid] = scan[cur][tid] + (tid >= d ? scan[cur][tid - d] : 0u);
        cur ^= 1;
      }
      const uint32_t incl = scan[cur][tid];   // own element: no barrier needed
      b_pos[tid] = outpos + incl - len;
      if (tid == kStripThreads - 1) b_pos[kStripThreads] = outpos + incl;
      __syncthreads();   // (P1) positions visible
      // codes at or past the strip's expected bytes are never read (the serial decoder's loop condition)
      int m2 = 0;
      { int lo = 0, hi = m; while (lo < hi) { const int mid = (lo + hi) >> 1; if (b_pos[mid] < st.expect) lo = mid + 1; else hi = mid; } m2 = lo; }
      const uint32_t stop = std::min(b_pos[m2], st.expect);
      // -- 4. the batch's entries, and where each code's bytes come from
      if (tid < m2) {
        const uint32_t e = 257 + (uint32_t)std::min<unsigned long long>(jt, kLzwTable);   // the entry made while this code is processed
        if (jt >= 1 && e < (uint32_t)kLzwTable) { tab_pos[e] = tid ? b_pos[tid - 1] : old_pos; tab_len[e] = (uint16_t)((tid ? b_len[tid - 1] : old_len) + 1); }
        if (code >= 256) b_src[tid] = k < 0 ? tab_pos[code] : (k ? b_pos[k - 1] : old_pos);   // (k < 0: an entry below this batch's, not written here)
      }
      __syncthreads();   // (P2) sources visible; the table is complete for the next batch
      // -- 5. per output byte: find the covering code, chase the source while it falls inside this batch (each hop lands in an
      //       earlier code: at most 64 hops), end on a literal or on bytes an earlier batch stored (ordered behind (Q) below)
      for (uint32_t q = outpos + tid; q < stop; q += kStripThreads) {
        int i = covering(b_pos, m2, q);
        uint32_t x = q - b_pos[i], val = 0;
        for (int hop = 0; hop <= kStripThreads; ++hop) {
          const uint32_t c = b_code[i];
          if (c < 256) { val = c; break; }
          const uint32_t period = b_len[i] - (c == 257 + j + (uint32_t)i ? 1u : 0u);   // KwKwK: the string is its own first byte after one period
          if (x >= period) x -= period;
          const uint32_t sp = b_src[i] + x;
          if (sp < outpos) { val = st.out[sp]; break; }   // sp < outpos <= expect
          if (sp >= q || i == 0) break;                    // cannot happen for a table built above; never read ahead
          i = covering(b_pos, i, sp);
          x = sp - b_pos[i];
        }
        st.out[q] = (uint8_t)val;
      }
      // -- 6. advance the state
      if (m2 > 0) { old_pos = b_pos[m2 - 1]; old_len = b_len[m2 - 1]; }
      outpos = stop;
      j += (uint32_t)m2;
      __syncthreads();   // (Q) this batch's bytes are stored before any thread of the next batch reads them
      if (outpos >= st.expect) break;    // full: nothing further is read
      if (end == kNoEnd) continue;       // 64 data codes consumed
      const unsigned kind = end & 7;
      if (kind == kEndClear) { cbit += lzw_offset(j) + lzw_width(j); j = 0; old_len = 0; continue; }   // consumes the Clear's bits
      if (kind == kEndBad) reason = kTiffBadCode;
      if (kind == kEndBadFull) reason = kTiffBadTableFull;
      break;   // EOI, a cut code or an impossible one
    }
    if (tid == 0) w.status[s] = ((unsigned long long)reason << 32) | outpos;
    __syncthreads();   // the table and the batch arrays are free for the next strip
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// PackBits (compression 32773), the semantics of packbits_decode: header byte c >= 0 copies c + 1 literal bytes (as many as the strip
// still has), c in -127..-1 repeats the next byte 1 - c times, -128 does nothing; packets may run across a row end.  The header walk
// is serial: thread 0 walks up to 64 packets, the workgroup copies or fills them.
__global__ __launch_bounds__(kStripThreads) void k_tiff_packbits(TiffWork w) {
  __shared__ uint32_t p_src[kStripThreads], p_len[kStripThreads], p_dst[kStripThreads], p_fill[kStripThreads];
  __shared__ uint32_t s_n, s_stop;
  const int tid = threadIdx.x;
  for (int s = blockIdx.x; s < w.n_strips; s += gridDim.x) {
    const Strip st = strip_of(w, s);
    uint32_t i = 0, out = 0, reason = 0;   // the walk's state: thread 0's registers (the other threads never use theirs)
    while (true) {
      if (tid == 0) {
        uint32_t n = 0;
        bool cut = false;
        while (n < (uint32_t)kStripThreads && i < st.count && out < st.expect) {   // every turn consumes a header byte
          const int c = (int8_t)st.src[i++];
          if (c >= 0) {
            const uint32_t len = std::min<uint32_t>(uint32_t(c) + 1, st.count - i);
            p_src[n] = i; p_len[n] = len; p_dst[n] = out; p_fill[n] = 0; ++n;
            i += len; out += len;
            if (len < uint32_t(c) + 1) cut = true;
          } else if (c != -128) {
            if (i >= st.count) { cut = true; break; }
            p_src[n] = i; p_len[n] = uint32_t(1 - c); p_dst[n] = out; p_fill[n] = 1; ++n;
            i += 1; out += uint32_t(1 - c);
          }
        }
        s_n = n;
        if (cut && out < st.expect) reason = kTiffCutPacket;
        s_stop = (cut || i >= st.count || out >= st.expect) ? 1u : 0u;
      }
      __syncthreads();   // (K1) the packets are posted
      const uint32_t n = s_n;
      for (uint32_t p = 0; p < n; ++p) {
        const uint32_t len = p_len[p], dst = p_dst[p], src = p_src[p], fill = p_fill[p];
        for (uint32_t x = tid; x < len && dst + x < st.expect; x += kStripThreads) st.out[dst + x] = st.src[fill ? src : src + x];   // src + x < count by the walk
      }
      const uint32_t stop = s_stop;
      __syncthreads();   // (K2) everyone is done with the packets before thread 0 posts the next ones
      if (stop) break;
    }
    if (tid == 0) w.status[s] = ((unsigned long long)reason << 32) | std::min(out, st.expect);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Finish: one workgroup per row.  Predictor 2 is a per-channel inclusive prefix sum mod 256 along the row (byte addition is
// associative: any scan order gives the serial bytes); then RGB(A) -> BGRA, alpha 255 for RGB, stored as dwords.  For compression 1
// the samples come straight from the file, at whatever alignment the strip has.
__device__ __forceinline__ uint32_t add4(uint32_t a, uint32_t b) {   // four byte lanes, each mod 256
  return (((a & 0x00ff00ffu) + (b & 0x00ff00ffu)) & 0x00ff00ffu) | (((a & 0xff00ff00u) + (b & 0xff00ff00u)) & 0xff00ff00u);
}
// samples of pixel x as R | G << 8 | B << 16 | A << 24 (A = 0 for RGB); bytes at or past `avail` read as 0
__device__ __forceinline__ uint32_t load_px(const uint8_t* p, unsigned long long avail, int spp, long long x) {
  const unsigned long long o = (unsigned long long)x * spp;
  uint32_t v = 0;
  for (int ch = 0; ch < spp; ++ch) if (o + ch < avail) v |= uint32_t(p[o + ch]) << (8 * ch);
  return v;
}
__device__ __forceinline__ uint32_t to_bgra(uint32_t rgba, int spp) {
  return ((rgba >> 16) & 0xffu) | (rgba & 0xff00u) | ((rgba & 0xffu) << 16) | (spp == 4 ? (rgba & 0xff000000u) : 0xff000000u);
}

__global__ __launch_bounds__(kRowThreads) void k_tiff_finish(TiffWork w, int from_file, uint32_t* __restrict__ bgra) {
  __shared__ uint32_t sc[2][kRowThreads];
  const int tid = threadIdx.x;
  const unsigned long long row_bytes = (unsigned long long)w.cols * w.samples;
  for (int y = blockIdx.x; y < w.rows; y += gridDim.x) {
    const uint8_t* p;
    unsigned long long avail = row_bytes;
    if (from_file) {
      const int s = y / w.rows_per_strip;
      const unsigned long long off = w.offsets[s], cnt = w.counts[s], at = (unsigned long long)(y - s * w.rows_per_strip) * row_bytes;
      const unsigned long long lim = off >= w.bytes ? 0 : std::min<unsigned long long>(cnt, w.bytes - off);   // readable bytes of the strip
      avail = at >= lim ? 0 : std::min(row_bytes, lim - at);
      p = w.file + (avail ? off + at : 0);
    } else {
      p = w.plane + (unsigned long long)y * row_bytes;
    }
    uint32_t* dst = bgra + (size_t)y * w.cols;
    if (w.predictor != 2) {
      for (long long x = tid; x < w.cols; x += kRowThreads) dst[x] = to_bgra(load_px(p, avail, w.samples, x), w.samples);
      continue;
    }
    // each thread owns a run of consecutive pixels: its sum, an exclusive scan of the 256 sums, then the run again with the carry
    const long long chunk = ((long long)w.cols + kRowThreads - 1) / kRowThreads, x0 = std::min<long long>((long long)tid * chunk, w.cols), x1 = std::min<long long>(x0 + chunk, w.cols);
    uint32_t sum = 0;
    for (long long x = x0; x < x1; ++x) sum = add4(sum, load_px(p, avail, w.samples, x));
    sc[0][tid] = sum;
    int cur = 0;
    for (int d = 1; d < kRowThreads; d <<= 1) {
      __syncthreads();   // the previous step's sums are visible
      sc[cur ^ 1][tid] = tid >= d ? add4(sc[cur][tid], sc[cur][tid - d]) : sc[cur][tid];
      cur ^= 1;
    }
    __syncthreads();     // the inclusive sums are visible to the right-hand neighbour
    uint32_t run = tid ? sc[cur][tid - 1] : 0u;
    for (long long x = x0; x < x1; ++x) { run = add4(run, load_px(p, avail, w.samples, x)); dst[x] = to_bgra(run, w.samples); }
    __syncthreads();     // the scan buffers are free for the next row
  }
}

}  // namespace

void launch_tiff_lzw(hipStream_t st, const TiffWork& w) {
  hipLaunchKernelGGL(k_tiff_lzw, dim3((unsigned)std::min(w.n_strips, 1 << 20)), dim3(kStripThreads), 0, st, w);
}
void launch_tiff_packbits(hipStream_t st, const TiffWork& w) {
  hipLaunchKernelGGL(k_tiff_packbits, dim3((unsigned)std::min(w.n_strips, 1 << 20)), dim3(kStripThreads), 0, st, w);
}
void launch_tiff_finish(hipStream_t st, const TiffWork& w, bool from_file, uint8_t* bgra) {
  hipLaunchKernelGGL(k_tiff_finish, dim3((unsigned)std::min(w.rows, 1 << 20)), dim3(kRowThreads), 0, st, w, from_file ? 1 : 0, (uint32_t*)bgra);
}

}  // namespace pf
