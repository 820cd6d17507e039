// TIFF decoder on the device (gfx950): the strips of a file decode in parallel, one workgroup each (LZW, PackBits, deflate), then one workgroup
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
// Deflate (compression 8 / 32946): a strip is one zlib stream (RFC 1950 around RFC 1951).  The verdict is libz's own
// uncompress(dst, expect, strip): the strip is good when it delivers `expect` bytes with Z_OK or Z_BUF_ERROR.  So once the strip is
// full the walk goes on through whatever produces no byte (an end-of-block, block headers, empty stored blocks) and stops, accepted,
// at the first symbol that would produce one -- a length / distance pair is parsed and its symbols validated first -- or where the
// input runs out; the final end-of-block leads to the Adler-32.  The rest of a pair (or of a stored block) that the strip's end cuts
// is such a byte too: a match that fills the strip with length left over ends the walk there, accepted, and nothing behind it is read.
// Any error met on the way refuses the strip.
//
// A turn of the strip's loop: (1) the workgroup stages 2 KB of the strip's bytes from the walk's position into LDS; (2) thread 0
// walks: it parses the zlib header, block headers (a dynamic block's code lengths go to LDS) and up to 256 tokens -- a literal, a
// (length, distance) pair or a run of stored bytes, each with its output position -- and stops the turn when the tokens are full,
// they cover 4 KB, the staged bytes run low or a block needs its tables; (3) the workgroup copies the tokens: per output byte a binary
// search for the covering token, then a literal is its value, stored bytes come from the strip, and a match reads
// out[pos - dist + x mod dist], chasing the source while it falls inside this turn's tokens (each hop lands in an earlier token);
// every thread keeps the Adler-32's two sums of its own bytes; (4) if a block began, the workgroup builds its two decode tables.
// The walk's state is thread 0's registers; what the other threads need is posted in LDS words behind a barrier.
//
// Tables (inf_build): lengths are counted with LDS atomics; thread 0 checks the set as zlib's inflate_table does (over-subscribed:
// refused; incomplete: refused unless it is a single code of one bit; a distance set without any code is accepted and every distance
// symbol is then invalid) and derives the first canonical code and the first sorted slot per length; every symbol finds its rank among
// the symbols of its length, stores itself in the sorted list and, for codes of up to nine bits, fills its entries of a 512-entry
// primary table (symbol << 4 | length, indexed by the next nine stream bits).  Longer codes take the canonical walk over 10..15 bits.
constexpr int kInfTokens = 256;
constexpr uint32_t kInfBatchBytes = 4096;   // a turn's tokens cover about this much output: bounds the copy's chase through a run
constexpr int kInfInWords = 512;            // staged input per turn, in dwords
constexpr uint32_t kInfHeaderBytes = 600;   // a block header is at most 3 + 7 + 32 or 3 + 14 + 19 * 3 + 316 * (7 + 7) = 4498 bits
constexpr uint32_t kInfTokenBytes = 8;      // a token is at most 15 + 5 + 15 + 13 = 48 bits; the trailer is 7 + 32
constexpr uint32_t kAdlerBase = 65521;
enum { kInfLiteral = 0, kInfMatch = 1, kInfStored = 2 };                               // a token's kind: bits 30.. of t_len
enum { kInfNextWalk = 0, kInfNextFixed = 1, kInfNextDynamic = 2, kInfNextDone = 3 };   // what follows a turn's copy
enum { kInfZlibHeader = 0, kInfBlock = 1, kInfStoredData = 2, kInfCodes = 3, kInfTrailer = 4 };

// thread 0's view of the staged bytes: an LSB-first bit buffer over the LDS words; bits past the strip's end read as 0 and `avail`
// says how many are real
struct InfBits {
  const uint32_t* in;         // LDS: the strip's bytes [in_byte, in_byte + 4 * kInfInWords), zero past the strip
  unsigned long long in_byte, count, pos;   // pos: the bit position in the strip, never past 8 * count
  unsigned long long hold;
  uint32_t nb, widx;
  __device__ __forceinline__ uint32_t word(uint32_t i) const { return i < (uint32_t)kInfInWords ? in[i] : 0u; }
  __device__ __forceinline__ void seek(unsigned long long p) {
    pos = p;
    const unsigned long long rel = p - 8 * in_byte;
    widx = (uint32_t)std::min<unsigned long long>(rel >> 5, (unsigned long long)kInfInWords);
    const uint32_t sh = (uint32_t)(rel & 31);
    hold = (unsigned long long)(word(widx) >> sh); nb = 32 - sh; ++widx;
  }
  __device__ __forceinline__ void fill() { if (nb <= 32) { hold |= (unsigned long long)word(widx) << nb; ++widx; nb += 32; } }   // then nb >= 33
  __device__ __forceinline__ unsigned long long avail() const { return 8 * count - pos; }
  __device__ __forceinline__ uint32_t peek() const { return (uint32_t)hold; }
  __device__ __forceinline__ void drop(uint32_t n) { hold >>= n; nb -= n; pos += n; }
  __device__ __forceinline__ void align() { drop((8 - (uint32_t)(pos & 7)) & 7); }
  // the staged bytes hold `bytes` more from pos, or everything the strip has
  __device__ __forceinline__ bool room(uint32_t bytes) const { const unsigned long long hi = in_byte + 4ull * kInfInWords; return hi >= count || (pos >> 3) + bytes <= hi; }
};

// the symbol the next bits spell (peek: at least 15 buffered bits, zero-padded); false: no code matches (an incomplete or empty set)
__device__ __forceinline__ bool inf_decode(uint32_t peek, const uint16_t* tab, const unsigned* cnt, const uint16_t* first, const uint16_t* offs,
                                           const uint16_t* sorted, uint32_t* sym, uint32_t* len) {
  const uint32_t e = tab[peek & 511];
  if (e) { *sym = e >> 4; *len = e & 15; return true; }
  uint32_t code = __brev(peek) >> 23;   // the first nine bits, first bit on top: no code of up to nine bits is a prefix of them
  for (uint32_t l = 10; l <= 15; ++l) {
    code = (code << 1) | ((peek >> (l - 1)) & 1);
    const uint32_t d = code - first[l];
    if (d < cnt[l]) { *sym = sorted[offs[l] + d]; *len = l; return true; }
  }
  return false;
}

// lens[0..n) -> tab, cnt, first, offs, sorted; called by the whole workgroup.  s_bad (LDS) is set by thread 0 when zlib refuses the set.
__device__ __forceinline__ void inf_build(const uint8_t* lens, uint32_t n, uint16_t* tab, unsigned* cnt, uint16_t* first, uint16_t* offs, uint16_t* sorted, unsigned* s_bad) {
  const uint32_t tid = threadIdx.x;
  if (tid < 16) cnt[tid] = 0;
  for (uint32_t i = tid; i < 512; i += kStripThreads) tab[i] = 0;
  __syncthreads();   // (T1) counters and table cleared; the lengths are visible
  for (uint32_t sym = tid; sym < n; sym += kStripThreads) { const uint32_t l = lens[sym]; if (l) atomicAdd(&cnt[l], 1u); }
  __syncthreads();   // (T2) counts final
  if (tid == 0) {
    int left = 1, max = 0;
    bool bad = false;
    uint32_t code = 0, slot = 0;
    for (int l = 1; l <= 15; ++l) {
      const int c = (int)cnt[l];
      code <<= 1;
      first[l] = (uint16_t)code; offs[l] = (uint16_t)slot;   // (a refused set's values are never used)
      code += (uint32_t)c; slot += (uint32_t)c;
      if (c) max = l;
      if (!bad) { left = 2 * left - c; if (left < 0) bad = true; }
    }
    if (max && !bad && left > 0 && max != 1) bad = true;
    *s_bad = bad ? 1u : 0u;
  }
  __syncthreads();   // (T3) first codes, slots and the verdict visible
  if (*s_bad) return;
  for (uint32_t sym = tid; sym < n; sym += kStripThreads) {
    const uint32_t l = lens[sym];
    if (!l) continue;
    uint32_t rank = 0;
    for (uint32_t k = 0; k < sym; ++k) rank += lens[k] == l;
    sorted[offs[l] + rank] = (uint16_t)sym;   // offs[l] + rank < n
    if (l <= 9) {
      const uint32_t rev = __brev(first[l] + rank) >> (32 - l);   // the code as the stream carries it, first bit lowest; < 1 << l for an accepted set
      for (uint32_t k = rev & 511; k < 512; k += 1u << l) tab[k] = (uint16_t)(sym << 4 | l);
    }
  }
}

__global__ __launch_bounds__(kStripThreads) void k_tiff_inflate(TiffWork w) {
  __shared__ uint32_t s_in[kInfInWords];
  __shared__ uint32_t t_len[kInfTokens], t_arg[kInfTokens], t_pos[kInfTokens + 1];
  __shared__ uint16_t tab_lit[512], tab_dist[512], sorted_lit[288], sorted_dist[32], first_lit[16], first_dist[16], offs_lit[16], offs_dist[16];
  __shared__ unsigned cnt_lit[16], cnt_dist[16];
  __shared__ uint8_t s_lens[320], s_cl[128], s_cllen[19];
  __shared__ unsigned s_n, s_next, s_nlen, s_ndist, s_bad[2], s_sum[2];
  __shared__ unsigned long long s_in_byte;
  const int tid = threadIdx.x;
  for (int s = blockIdx.x; s < w.n_strips; s += gridDim.x) {
    const Strip st = strip_of(w, s);
    // the walk's state: thread 0's registers (the other threads never use theirs)
    unsigned long long pos = 0;
    uint32_t outpos = 0, mode = kInfZlibHeader, last = 0, stored_left = 0, reason = 0, want = 0;
    bool have_trailer = false, tables_bad = false;
    // held identically by every thread (read from LDS behind a barrier) / every thread's own
    unsigned long long in_byte = 0, sum_a = 0, sum_w = 0;
    while (true) {
      for (int i = tid; i < kInfInWords; i += kStripThreads) {
        const unsigned long long o = in_byte + 4ull * i;
        uint32_t v = 0;
        if (o + 4 <= st.count) __builtin_memcpy(&v, st.src + o, 4);
        else for (int k = 0; k < 4; ++k) if (o + k < st.count) v |= uint32_t(st.src[o + k]) << (8 * k);
        s_in[i] = v;
      }
      __syncthreads();   // (I1) the input is staged; the tables built after the previous turn are complete
      if (tid == 0) {
        const uint32_t out0 = outpos;
        uint32_t n = 0, next = kInfNextWalk;
        bool stop = false;   // the strip's walk ends: an error (reason), the input ran out, a byte past the full strip, the trailer
        InfBits b;
        b.in = s_in; b.in_byte = in_byte; b.count = st.count; b.seek(pos);
        while (!stop && next == kInfNextWalk && n < (uint32_t)kInfTokens && outpos - out0 < kInfBatchBytes) {   // every turn consumes input, stops or leaves
          if (mode == kInfZlibHeader) {
            b.fill();
            if (b.avail() < 16) { stop = true; continue; }
            const uint32_t cmf = b.peek() & 0xff, flg = (b.peek() >> 8) & 0xff;
            if (((cmf << 8) + flg) % 31 || (cmf & 15) != 8 || (cmf >> 4) > 7 || (flg & 0x20)) { reason = kTiffZlibHeader; stop = true; continue; }
            b.drop(16); mode = kInfBlock;
            continue;
          }
          if (mode == kInfBlock) {
            if (last) { b.align(); mode = kInfTrailer; continue; }
            if (!b.room(kInfHeaderBytes)) break;
            b.fill();
            if (b.avail() < 3) { stop = true; continue; }
            last = b.peek() & 1;
            const uint32_t type = (b.peek() >> 1) & 3;
            b.drop(3);
            if (type == 0) {
              b.align(); b.fill();
              if (b.avail() < 32) { stop = true; continue; }
              const uint32_t v = b.peek();
              if ((v & 0xffff) != ((v >> 16) ^ 0xffff)) { reason = kTiffBlockHeader; stop = true; continue; }
              stored_left = v & 0xffff;
              b.drop(32); mode = kInfStoredData;
            } else if (type == 1) {
              next = kInfNextFixed; mode = kInfCodes;
            } else if (type == 2) {
              b.fill();
              if (b.avail() < 14) { stop = true; continue; }
              const uint32_t nlen = (b.peek() & 31) + 257, ndist = ((b.peek() >> 5) & 31) + 1, ncode = ((b.peek() >> 10) & 15) + 4;
              b.drop(14);
              if (nlen > 286 || ndist > 30) { reason = kTiffCodeLengths; stop = true; continue; }
              // the code-length code: 19 lengths of three bits in the RFC's order, then its 128-entry table (symbol << 3 | length)
              for (uint32_t i = 0; i < 19; ++i) s_cllen[i] = 0;
              for (uint32_t i = 0; i < ncode && !stop; ++i) {
                b.fill();
                if (b.avail() < 3) { stop = true; break; }
                const uint32_t order = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? (19 - i) >> 1 : 6 + (i >> 1);   // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
                s_cllen[order] = (uint8_t)(b.peek() & 7);
                b.drop(3);
              }
              if (stop) continue;
              int left = 1;
              uint32_t code = 0, any = 0;
              for (uint32_t l = 1; l <= 7 && left >= 0; ++l) {
                left *= 2;
                for (uint32_t sym = 0; sym < 19 && left >= 0; ++sym) {
                  if (s_cllen[sym] != l) continue;
                  if (--left < 0) break;
                  const uint32_t rev = __brev(code) >> (32 - l);
                  for (uint32_t k = rev & 127; k < 128; k += 1u << l) s_cl[k] = (uint8_t)(sym << 3 | l);
                  ++code; any = 1;
                }
                code <<= 1;
              }
              if (!any) {   // zlib reads a length 0 per bit from the empty code and then misses the end-of-block code
                if (b.avail() < nlen + ndist) { stop = true; continue; }
                reason = kTiffCodeLengths; stop = true; continue;
              }
              if (left != 0) { reason = kTiffCodeLengths; stop = true; continue; }   // over-subscribed or incomplete
              uint32_t have = 0;
              while (have < nlen + ndist && !stop) {   // every turn consumes a code or stops
                b.fill();
                const uint32_t e = s_cl[b.peek() & 127], sym = e >> 3, l = e & 7;   // the code is complete: every entry is set
                if (l > b.avail()) { stop = true; break; }
                if (sym < 16) { b.drop(l); s_lens[have++] = (uint8_t)sym; continue; }
                const uint32_t xb = sym == 16 ? 2 : sym == 17 ? 3 : 7;
                if (l + xb > b.avail()) { stop = true; break; }
                b.drop(l);
                uint32_t val = 0;
                if (sym == 16) {
                  if (have == 0) { reason = kTiffCodeLengths; stop = true; break; }
                  val = s_lens[have - 1];
                }
                const uint32_t rep = (sym == 18 ? 11 : 3) + (b.peek() & ((1u << xb) - 1));
                b.drop(xb);
                if (have + rep > nlen + ndist) { reason = kTiffCodeLengths; stop = true; break; }
                for (uint32_t k = 0; k < rep; ++k) s_lens[have++] = (uint8_t)val;
              }
              if (stop) continue;
              if (s_lens[256] == 0) { reason = kTiffCodeLengths; stop = true; continue; }   // no end-of-block code
              s_nlen = nlen; s_ndist = ndist;
              next = kInfNextDynamic; mode = kInfCodes;
            } else {
              reason = kTiffBlockHeader; stop = true;
            }
            continue;
          }
          if (mode == kInfStoredData) {
            if (stored_left == 0) { mode = kInfBlock; continue; }
            const unsigned long long at = b.pos >> 3;   // byte-aligned here
            const uint32_t copy = (uint32_t)std::min<unsigned long long>(std::min<unsigned long long>(stored_left, st.count - at), st.expect - outpos);
            if (copy == 0) { stop = true; continue; }   // the strip is full, or the input ran out
            t_pos[n] = outpos; t_len[n] = copy | (uint32_t)kInfStored << 30; t_arg[n] = (uint32_t)at; ++n;
            outpos += copy; stored_left -= copy;
            b.seek(b.pos + 8ull * copy);
            if (!b.room(kInfTokenBytes)) break;
            continue;
          }
          if (mode == kInfTrailer) {
            if (!b.room(kInfTokenBytes)) break;
            b.fill();
            if (b.avail() >= 32) { const uint32_t v = b.peek(); want = (v << 24) | ((v & 0xff00) << 8) | ((v >> 8) & 0xff00) | (v >> 24); have_trailer = true; }
            stop = true;
            continue;
          }
          // kInfCodes: one literal/length symbol, and for a length the rest of its pair
          if (tables_bad) { reason = kTiffCodeLengths; stop = true; continue; }
          if (!b.room(kInfTokenBytes)) break;
          b.fill();
          uint32_t sym = 0, l = 0;
          if (!inf_decode(b.peek(), tab_lit, cnt_lit, first_lit, offs_lit, sorted_lit, &sym, &l)) {
            if (b.avail() >= 1) reason = kTiffInvalidSymbol;
            stop = true; continue;
          }
          if (l > b.avail()) { stop = true; continue; }
          b.drop(l);
          if (sym < 256) {
            if (outpos >= st.expect) { stop = true; continue; }   // a byte past the full strip: the over-long stream, accepted
            t_pos[n] = outpos; t_len[n] = 1u; t_arg[n] = sym; ++n;
            ++outpos;
            continue;
          }
          if (sym == 256) { mode = kInfBlock; continue; }
          if (sym > 285) { reason = kTiffInvalidSymbol; stop = true; continue; }
          uint32_t len = 258, xb = 0;
          if (sym < 265) len = sym - 254;
          else if (sym < 285) { xb = (sym - 261) >> 2; len = ((4 + ((sym - 265) & 3)) << xb) + 3; }
          b.fill();
          if (xb > b.avail()) { stop = true; continue; }
          len += b.peek() & ((1u << xb) - 1);
          b.drop(xb);
          b.fill();
          uint32_t dsym = 0;
          if (!inf_decode(b.peek(), tab_dist, cnt_dist, first_dist, offs_dist, sorted_dist, &dsym, &l)) {
            if (b.avail() >= 1) reason = kTiffInvalidSymbol;
            stop = true; continue;
          }
          if (l > b.avail()) { stop = true; continue; }
          b.drop(l);
          if (dsym > 29) { reason = kTiffInvalidSymbol; stop = true; continue; }
          uint32_t dist = dsym + 1;
          xb = 0;
          if (dsym >= 4) { xb = (dsym >> 1) - 1; dist = ((2 + (dsym & 1)) << xb) + 1; }
          b.fill();
          if (xb > b.avail()) { stop = true; continue; }
          dist += b.peek() & ((1u << xb) - 1);
          b.drop(xb);
          if (outpos >= st.expect) { stop = true; continue; }   // a validated pair past the full strip: accepted, not copied
          if (dist > outpos) { reason = kTiffFarBack; stop = true; continue; }   // a strip never refers to another strip
          const bool clipped = len > st.expect - outpos;   // the rest of the pair would be bytes past the full strip: zlib keeps the
          len = std::min(len, st.expect - outpos);         // remainder pending and reads nothing further -- accepted, like any such byte
          t_pos[n] = outpos; t_len[n] = len | (uint32_t)kInfMatch << 30; t_arg[n] = dist; ++n;
          outpos += len;
          if (clipped) stop = true;
        }
        pos = b.pos;
        t_pos[n] = outpos;
        s_n = n; s_next = stop ? (unsigned)kInfNextDone : next; s_in_byte = pos >> 3;
      }
      __syncthreads();   // (I2) the tokens, what follows them and the next staging position are posted
      const int n = (int)s_n;
      const unsigned next = s_next;
      const uint32_t out0 = t_pos[0], out1 = t_pos[n];   // out1 <= expect: the walk clips every token
      for (uint32_t q = out0 + tid; q < out1; q += kStripThreads) {
        int i = covering(t_pos, n, q);
        uint32_t at = q, val = 0;
        for (int hop = 0; hop <= kInfTokens; ++hop) {
          const uint32_t kind = t_len[i] >> 30, arg = t_arg[i], x = at - t_pos[i];
          if (kind == kInfLiteral) { val = arg; break; }
          if (kind == kInfStored) { val = st.src[arg + x]; break; }   // arg + x < count by the walk
          const uint32_t sp = t_pos[i] - arg + (x < arg ? x : x % arg);   // arg = the distance, 1 <= arg <= t_pos[i]: sp < t_pos[i]
          if (sp < out0) { val = st.out[sp]; break; }   // stored by an earlier turn, ordered behind (Q)
          if (i == 0) break;                            // cannot happen: sp >= out0 = t_pos[0] lies in an earlier token
          i = covering(t_pos, i, sp);
          at = sp;
        }
        st.out[q] = (uint8_t)val;
        sum_a += val; sum_w += (unsigned long long)q * val;
      }
      sum_w %= kAdlerBase;   // (a turn adds at most 2^18 bytes per thread, each below 2^39)
      in_byte = s_in_byte;
      __syncthreads();   // (Q) this turn's bytes are stored before the next turn's copies read them; the token arrays are free
      if (next == kInfNextDone) break;
      if (next != kInfNextWalk) {
        uint32_t nlen = 288, ndist = 32;
        if (next == kInfNextFixed) for (uint32_t i = tid; i < 320; i += kStripThreads) s_lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
        else { nlen = s_nlen; ndist = s_ndist; }
        inf_build(s_lens, nlen, tab_lit, cnt_lit, first_lit, offs_lit, sorted_lit, &s_bad[0]);
        inf_build(s_lens + nlen, ndist, tab_dist, cnt_dist, first_dist, offs_dist, sorted_dist, &s_bad[1]);
        if (tid == 0) tables_bad = s_bad[0] || s_bad[1];   // (thread 0 wrote both itself)
      }
    }
    // Adler-32 of the n bytes written: a = 1 + sum v, b = n + sum (n - q) v_q = n a - sum q v_q
    if (tid == 0) { s_sum[0] = 0; s_sum[1] = 0; }
    __syncthreads();   // (A1) the sums are reset
    atomicAdd(&s_sum[0], (unsigned)(sum_a % kAdlerBase)); atomicAdd(&s_sum[1], (unsigned)sum_w);
    __syncthreads();   // (A2) ... and final
    if (tid == 0) {
      const uint32_t a = (1 + s_sum[0]) % kAdlerBase, bsum = ((outpos % kAdlerBase) * a % kAdlerBase + kAdlerBase - s_sum[1] % kAdlerBase) % kAdlerBase;
      if (have_trailer && !reason && ((bsum << 16) | a) != want) reason = kTiffDataCheck;
      w.status[s] = ((unsigned long long)reason << 32) | outpos;
    }
    __syncthreads();   // the sums, the tables and the token arrays are free for the next strip
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
void launch_tiff_inflate(hipStream_t st, const TiffWork& w) {
  hipLaunchKernelGGL(k_tiff_inflate, dim3((unsigned)std::min(w.n_strips, 1 << 20)), dim3(kStripThreads), 0, st, w);
}
void launch_tiff_finish(hipStream_t st, const TiffWork& w, bool from_file, uint8_t* bgra) {
  hipLaunchKernelGGL(k_tiff_finish, dim3((unsigned)std::min(w.rows, 1 << 20)), dim3(kRowThreads), 0, st, w, from_file ? 1 : 0, (uint32_t*)bgra);
}

}  // namespace pf
