// PNG encoder on the device (gfx950): scanline filtering, deflate of independent segments, compaction.  The host (pf_api_png.inl,
// png_frame.hpp) only frames the stream.  Every kernel is a pure function of the image: no result depends on the order in which
// workgroups or atomics run (the LDS atomics below add integers or OR disjoint bit fields).
#include <algorithm>

#include "pf_common.hpp"
#include "png_frame.hpp"

namespace pf {
namespace {

constexpr int kSeg = (int)png_frame::kSegBytes;
constexpr int kSlot = (int)png_frame::kSegSlot;
constexpr int kThreads = 256;
constexpr int kChunk = 64;                  // stream positions per thread of the deflate workgroup: 256 * 64 >= kSeg
static_assert(kThreads * kChunk >= kSeg && kSeg % 4 == 0 && kSlot % 4 == 0, "segment geometry");

// ---------------------------------------------------------------------------------------------------------------------------------
// Filter pass.  One workgroup per row (grid-stride): the five PNG filters' sums of absolute residuals (residual bytes read as signed,
// libpng's heuristic), the smallest sum wins and the lowest type number breaks a tie; then the row is written with that filter.
// BGRA in, filter byte + RGBA out.  The filters work per channel at a distance of one pixel, so the channel swap commutes with them.
__device__ __forceinline__ unsigned absres(unsigned v) { v &= 0xff; return v < 128 ? v : 256 - v; }
__device__ __forceinline__ unsigned paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// residual of channel byte x under filter f (a = left, b = up, c = up-left)
__device__ __forceinline__ unsigned residual(int f, unsigned x, unsigned a, unsigned b, unsigned c) {
  switch (f) {
    case 0: return x;
    case 1: return (x - a) & 0xff;
    case 2: return (x - b) & 0xff;
    case 3: return (x - ((a + b) >> 1)) & 0xff;
    default: return (x - paeth((int)a, (int)b, (int)c)) & 0xff;
  }
}

__global__ __launch_bounds__(kThreads) void k_png_filter(const uint32_t* __restrict__ bgra, int cols, int rows, uint8_t* __restrict__ stream) {
  __shared__ unsigned long long red[5][kThreads];
  __shared__ int s_best;
  const int tid = threadIdx.x;
  for (int y = blockIdx.x; y < rows; y += gridDim.x) {
    const uint32_t* cur = bgra + size_t(y) * cols;
    const uint32_t* up = y ? cur - cols : nullptr;
    unsigned long long sum[5] = {0, 0, 0, 0, 0};
    for (int x = tid; x < cols; x += kThreads) {
      const uint32_t px = cur[x], pa = x ? cur[x - 1] : 0u, pb = up ? up[x] : 0u, pc = (up && x) ? up[x - 1] : 0u;
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        const unsigned v = (px >> (8 * ch)) & 0xff, a = (pa >> (8 * ch)) & 0xff, b = (pb >> (8 * ch)) & 0xff, c = (pc >> (8 * ch)) & 0xff;
#pragma unroll
        for (int f = 0; f < 5; ++f) sum[f] += absres(residual(f, v, a, b, c));
      }
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) red[f][tid] = sum[f];
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
      if (tid < s) {
#pragma unroll
        for (int f = 0; f < 5; ++f) red[f][tid] += red[f][tid + s];
      }
      __syncthreads();
    }
    if (tid == 0) {
      int best = 0;
      for (int f = 1; f < 5; ++f) if (red[f][0] < red[best][0]) best = f;
      s_best = best;
    }
    __syncthreads();
    const int f = s_best;
    uint8_t* out = stream + size_t(y) * (size_t(cols) * 4 + 1);
    if (tid == 0) out[0] = (uint8_t)f;
    for (int x = tid; x < cols; x += kThreads) {
      const uint32_t px = cur[x], pa = x ? cur[x - 1] : 0u, pb = up ? up[x] : 0u, pc = (up && x) ? up[x - 1] : 0u;
      unsigned r[4];
#pragma unroll
      for (int ch = 0; ch < 4; ++ch)
        r[ch] = residual(f, (px >> (8 * ch)) & 0xff, (pa >> (8 * ch)) & 0xff, (pb >> (8 * ch)) & 0xff, (pc >> (8 * ch)) & 0xff);
      uint8_t* o = out + 1 + size_t(x) * 4;
      o[0] = (uint8_t)r[2]; o[1] = (uint8_t)r[1]; o[2] = (uint8_t)r[0]; o[3] = (uint8_t)r[3];   // B G R A -> R G B A
    }
    __syncthreads();   // red / s_best are reused by the next row
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Deflate pass.  One workgroup per segment.
//
// Tokens.  Position j of the segment has class 4 if its byte equals the byte 4 back, else class 1 if it equals the byte 1 back, else 0
// (bytes before the segment start do not exist: no match reaches back across it).  A maximal run of positions of one non-zero class d,
// starting at a, is cut into pieces of 258 from a; a piece of 3 or more positions is one match (length = the piece, distance d), a
// shorter one is literals; class 0 is a literal.  This parse is a function of the bytes alone, so threads derive their own part of it:
// thread k owns positions [64 k, 64 k + 64), emits the tokens that START there, and finds how far the run of its first position reaches
// back from per-thread summaries (the count of equal classes at the end of each chunk).
//
// The segment's bytes sit in LDS with one dword of padding per 64 bytes, so that the threads' chunk walks (stride 68 bytes) spread over
// the banks.
__device__ __forceinline__ int ia(int p) { return p + ((p >> 6) << 2); }
constexpr int kInBytes = kSeg + (kSeg / 64 + 1) * 4;
constexpr int kOutWords = (kSeg + 16) / 4 + 2;
constexpr int kLitLen = 286, kClSyms = 19, kMaxSyms = 288;
constexpr int kLenSeq = kLitLen + 4;   // code lengths sent: 286 literal / length codes, 4 distance codes (lengths 1 0 0 1: distances 1 and 4)

__device__ __forceinline__ int tclass(const uint8_t* in, int j) {
  const uint8_t v = in[ia(j)];
  if (j >= 4 && in[ia(j - 4)] == v) return 4;
  if (j >= 1 && in[ia(j - 1)] == v) return 1;
  return 0;
}
// positions from j on (below n, at most cap) of class t
__device__ __forceinline__ int run_fwd(const uint8_t* in, int n, int j, int t, int cap) {
  int c = 0;
  while (c < cap && j + c < n && tclass(in, j + c) == t) ++c;
  return c;
}
// length symbol, number of extra bits and their value for a match length 3..258 (RFC 1951, 3.2.5)
__device__ __forceinline__ void len_code(int len, int& sym, int& nextra, int& extra) {
  if (len == 258) { sym = 285; nextra = 0; extra = 0; return; }
  const int l = len - 3;
  if (l < 8) { sym = 257 + l; nextra = 0; extra = 0; return; }
  const int e = 29 - __clz(l);   // floor(log2 l) - 2
  sym = 261 + 4 * e + ((l >> e) & 3); nextra = e; extra = l & ((1 << e) - 1);
}

// the tokens that start in [c0, min(c0 + 64, n)); `back` = positions before c0 that continue the class of c0 (0 for class 0)
template <class F>
__device__ __forceinline__ void walk_tokens(const uint8_t* in, int n, int c0, int back, F& f) {
  const int e = min(c0 + kChunk, n);
  int i = c0, run_t = 0, o_next = 0;
  if (i < e && back > 0) { run_t = tclass(in, i); o_next = back; }
  while (i < e) {
    const int t = tclass(in, i);
    if (t == 0) { f.lit(in[ia(i)]); run_t = 0; ++i; continue; }
    const int o = (t == run_t) ? o_next : 0;      // offset of i inside its run
    const int r = o % 258;                        // ... inside its piece
    const int cl = r + run_fwd(in, n, i, t, 258 - r);   // the piece's length
    if (cl >= 3) { if (r == 0) f.match(cl, t); i += cl - r; o_next = o + (cl - r); }
    else { f.lit(in[ia(i)]); ++i; o_next = o + 1; }
    run_t = t;
  }
}

struct HistF {
  unsigned* hist;
  __device__ __forceinline__ void lit(unsigned b) { atomicAdd(&hist[b], 1u); }
  __device__ __forceinline__ void match(int len, int) { int s, ne, ex; len_code(len, s, ne, ex); atomicAdd(&hist[s], 1u); }
};
struct CountF {
  const uint8_t* lens; unsigned bits;
  __device__ __forceinline__ void lit(unsigned b) { bits += lens[b]; }
  __device__ __forceinline__ void match(int len, int) { int s, ne, ex; len_code(len, s, ne, ex); bits += lens[s] + ne + 1; }
};
// n <= 32 bits of v at bit position pos of the little-endian word array (deflate packs from the least significant bit)
__device__ __forceinline__ void put_bits(unsigned* out, unsigned pos, unsigned v, int n) {
  const unsigned w = pos >> 5, sh = pos & 31;
  atomicOr(&out[w], v << sh);
  if (sh + n > 32) atomicOr(&out[w + 1], v >> (32 - sh));
}
struct EmitF {
  const uint8_t* lens; const unsigned* codes; unsigned* out; unsigned pos;
  __device__ __forceinline__ void lit(unsigned b) { put_bits(out, pos, codes[b], lens[b]); pos += lens[b]; }
  __device__ __forceinline__ void match(int len, int d) {
    int s, ne, ex; len_code(len, s, ne, ex);
    const int l = lens[s];
    // the length code, its extra bits, the distance code: 1 bit, 0 = distance 1 (symbol 0), 1 = distance 4 (symbol 3)
    const unsigned v = codes[s] | (unsigned)ex << l | (unsigned)(d == 4) << (l + ne);
    put_bits(out, pos, v, l + ne + 1); pos += l + ne + 1;
  }
};

// Length-limited canonical Huffman code of the n <= 288 symbols with freq > 0 (whole workgroup; every array in LDS).  Symbols ordered by
// (freq, index); the tree by the two-queue method; depths beyond maxbits folded back the way miniz does (move codes from the longest
// allowed length down until the Kraft sum is exact); the shortest codes go to the most frequent symbols.  A lone symbol gets a 1-bit code
// and so does one unused symbol, so that the code is complete (inflate refuses an incomplete literal or code-length code).
struct HuffScratch {
  unsigned w[2 * kMaxSyms];
  unsigned short parent[2 * kMaxSyms], depth[2 * kMaxSyms], sorted[kMaxSyms];
  unsigned count[16], next[16];
  unsigned used;
};
__device__ void build_code(const unsigned* freq, int n, int maxbits, uint8_t* lens, unsigned* codes, HuffScratch& hs) {
  const int tid = threadIdx.x;
  if (tid == 0) hs.used = 0;
  __syncthreads();
  for (int s = tid; s < n; s += kThreads) {
    lens[s] = 0; codes[s] = 0;
    const unsigned fs = freq[s];
    if (!fs) continue;
    int rank = 0;
    for (int q = 0; q < n; ++q) { const unsigned fq = freq[q]; rank += (fq != 0) && (fq < fs || (fq == fs && q < s)); }
    hs.sorted[rank] = (unsigned short)s;
    atomicAdd(&hs.used, 1u);
  }
  __syncthreads();
  if (tid == 0) {
    const int m = (int)hs.used;
    for (int i = 0; i < 16; ++i) hs.count[i] = 0;
    if (m == 1) {
      const int s = hs.sorted[0];
      lens[s] = 1; lens[s == 0 ? 1 : 0] = 1; hs.count[1] = 2;
    } else if (m >= 2) {
      for (int i = 0; i < m; ++i) hs.w[i] = freq[hs.sorted[i]];
      int lp = 0, ip = m, nx = m;
      for (int k = 0; k < m - 1; ++k) {
        unsigned sum = 0;
        for (int two = 0; two < 2; ++two) {
          const bool leaf = lp < m && (ip >= nx || hs.w[lp] <= hs.w[ip]);
          const int pick = leaf ? lp++ : ip++;
          sum += hs.w[pick]; hs.parent[pick] = (unsigned short)nx;
        }
        hs.w[nx++] = sum;
      }
      const int root = 2 * m - 2;
      hs.depth[root] = 0;
      for (int j = root - 1; j >= m; --j) hs.depth[j] = hs.depth[hs.parent[j]] + 1;
      for (int i = 0; i < m; ++i) { const int d = hs.depth[hs.parent[i]] + 1; hs.count[d < maxbits ? d : maxbits] += 1; }
      unsigned total = 0;
      for (int i = maxbits; i > 0; --i) total += hs.count[i] << (maxbits - i);
      while (total > (1u << maxbits)) {   // (a Huffman tree's Kraft sum is exact; folding depths back can only raise it)
        hs.count[maxbits] -= 1;
        for (int i = maxbits - 1; i > 0; --i) if (hs.count[i]) { hs.count[i] -= 1; hs.count[i + 1] += 2; break; }
        total -= 1;
      }
      int j = m;
      for (int l = 1; l <= maxbits; ++l) for (unsigned q = hs.count[l]; q > 0; --q) lens[hs.sorted[--j]] = (uint8_t)l;
    }
    unsigned code = 0;
    hs.next[0] = 0;
    for (int l = 1; l <= 15; ++l) { code = (code + (l > 1 ? hs.count[l - 1] : 0u)) << 1; hs.next[l] = code; }
  }
  __syncthreads();
  for (int s = tid; s < n; s += kThreads) {
    const int l = lens[s];
    if (!l) continue;
    unsigned idx = 0;
    for (int q = 0; q < s; ++q) idx += lens[q] == l;
    codes[s] = __brev(hs.next[l] + idx) >> (32 - l);   // Huffman codes go out most significant bit first
  }
  __syncthreads();
}

// serial bit writer of one thread (the block header)
struct BitW {
  unsigned* out; unsigned pos;
  __device__ __forceinline__ void put(unsigned v, int n) { put_bits(out, pos, v, n); pos += n; }
};

__global__ __launch_bounds__(kThreads) void k_png_deflate(const uint8_t* __restrict__ stream, unsigned long long total, uint8_t* __restrict__ slots,
                                                          unsigned* __restrict__ sizes, unsigned* __restrict__ adler) {
  __shared__ __attribute__((aligned(16))) uint8_t in[kInBytes];
  __shared__ unsigned outw[kOutWords];
  __shared__ unsigned hist[kMaxSyms], codes[kMaxSyms], cl_hist[kClSyms + 1], cl_codes[kClSyms + 1];
  __shared__ uint8_t lens[kMaxSyms], cl_lens[kClSyms + 1];
  __shared__ unsigned short cl_seq[kLenSeq];
  __shared__ HuffScratch hs;
  __shared__ unsigned long long red1[kThreads], red2[kThreads];
  __shared__ unsigned char s_tl[kThreads], s_tail[kThreads];
  __shared__ unsigned s_scan[kThreads + 1];
  __shared__ unsigned s_ncl, s_hdr_bits;

  const int tid = threadIdx.x;
  const size_t seg = blockIdx.x;
  const unsigned long long base = (unsigned long long)seg * kSeg;
  const int n = (int)min((unsigned long long)kSeg, total - base);
  const bool last = base + n == total;
  const uint8_t* src = stream + base;
  uint8_t* slot = slots + seg * kSlot;

  // ---- load (the stream buffer is padded to a multiple of 4 bytes), Adler-32 partial sums: a = 1 + sum b, b = n + sum (n - p) b[p] ----
  for (int i = tid; i < kMaxSyms; i += kThreads) hist[i] = 0;
  for (int i = tid; i < kOutWords; i += kThreads) outw[i] = 0;
  if (tid <= kClSyms) cl_hist[tid] = 0;
  unsigned long long a1 = 0, a2 = 0;
  for (int w = tid; w * 4 < n; w += kThreads) {
    const unsigned v = reinterpret_cast<const unsigned*>(src)[w];
    *reinterpret_cast<unsigned*>(&in[ia(w * 4)]) = v;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int p = w * 4 + k;
      if (p < n) { const unsigned b = (v >> (8 * k)) & 0xff; a1 += b; a2 += (unsigned long long)(n - p) * b; }
    }
  }
  red1[tid] = a1; red2[tid] = a2;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) { red1[tid] += red1[tid + s]; red2[tid] += red2[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    const unsigned a = (unsigned)((1 + red1[0]) % png_frame::kAdlerBase), b = (unsigned)((n + red2[0]) % png_frame::kAdlerBase);
    adler[seg] = b << 16 | a;
  }

  // ---- per-chunk summaries: class of the last position and how many positions at the chunk's end share it ----
  const int c0 = tid * kChunk;
  if (c0 + kChunk <= n) {
    const int tl = tclass(in, c0 + kChunk - 1);
    int tail = 1;
    while (tail < kChunk && tclass(in, c0 + kChunk - 1 - tail) == tl) ++tail;
    s_tl[tid] = (unsigned char)tl; s_tail[tid] = (unsigned char)tail;
  }
  __syncthreads();
  int back = 0;
  if (c0 < n) {
    const int tf = tclass(in, c0);
    if (tf != 0)
      for (int j = tid - 1; j >= 0; --j) {
        if (s_tl[j] != tf) break;
        back += s_tail[j];
        if (s_tail[j] < kChunk) break;
      }
  }

  // ---- histogram, the literal / length code ----
  { HistF f{hist}; walk_tokens(in, n, c0, back, f); }
  if (tid == 0) atomicAdd(&hist[256], 1u);   // end of block
  __syncthreads();
  build_code(hist, kLitLen, 15, lens, codes, hs);

  // ---- the code lengths as code-length symbols (RFC 1951, 3.2.7): 16 = repeat the previous 3-6 times, 17 / 18 = 3-10 / 11-138 zeros ----
  if (tid == 0) {
    unsigned nseq = 0;
    auto len_at = [&](int i) -> int { return i < kLitLen ? lens[i] : ((i == kLitLen || i == kLitLen + 3) ? 1 : 0); };
    auto emit = [&](unsigned sym, unsigned extra) { cl_seq[nseq++] = (unsigned short)(sym | extra << 8); cl_hist[sym] += 1; };
    for (int i = 0; i < kLenSeq;) {
      const int v = len_at(i);
      int run = 1;
      while (i + run < kLenSeq && len_at(i + run) == v) ++run;
      i += run;
      if (v == 0) {
        while (run >= 11) { const int k = run < 138 ? run : 138; emit(18, k - 11); run -= k; }
        if (run >= 3) { emit(17, run - 3); run = 0; }
        while (run-- > 0) emit(0, 0);
      } else {
        emit(v, 0); run -= 1;
        while (run >= 3) { const int k = run < 6 ? run : 6; emit(16, k - 3); run -= k; }
        while (run-- > 0) emit(v, 0);
      }
    }
    s_ncl = nseq;
  }
  __syncthreads();
  build_code(cl_hist, kClSyms, 7, cl_lens, cl_codes, hs);

  // ---- the dynamic block's header ----
  if (tid == 0) {
    BitW bw{outw, 0};
    bw.put(0, 1); bw.put(2, 2);                 // BFINAL = 0 (only the last segment's marker ends the stream), BTYPE = dynamic
    bw.put(kLitLen - 257, 5); bw.put(3, 5); bw.put(kClSyms - 4, 4);   // HLIT, HDIST (4 distance codes), HCLEN (all 19)
    const unsigned char order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < 19; ++i) bw.put(cl_lens[order[i]], 3);
    for (unsigned i = 0; i < s_ncl; ++i) {
      const unsigned sym = cl_seq[i] & 0xff, extra = cl_seq[i] >> 8;
      bw.put(cl_codes[sym], cl_lens[sym]);
      if (sym == 16) bw.put(extra, 2); else if (sym == 17) bw.put(extra, 3); else if (sym == 18) bw.put(extra, 7);
    }
    s_hdr_bits = bw.pos;
  }

  // ---- bits per thread, their prefix sum, coded or stored ----
  { CountF f{lens, 0}; walk_tokens(in, n, c0, back, f); s_scan[tid + 1] = f.bits; }
  __syncthreads();
  if (tid == 0) {
    unsigned acc = s_hdr_bits;
    for (int i = 0; i < kThreads; ++i) { const unsigned b = s_scan[i + 1]; s_scan[i] = acc; acc += b; }
    s_scan[kThreads] = acc;
  }
  __syncthreads();
  const unsigned eob_pos = s_scan[kThreads];
  const unsigned marker_bit = eob_pos + lens[256];                 // the sync marker's 3 header bits start here
  const unsigned marker_byte = (marker_bit + 3 + 7) >> 3;          // ... and its 00 00 FF FF here
  const unsigned coded_bytes = marker_byte + 4;
  const unsigned stored_bytes = (unsigned)n + (unsigned)png_frame::kSegOverhead;
  if (coded_bytes < stored_bytes) {
    { EmitF f{lens, codes, outw, s_scan[tid]}; walk_tokens(in, n, c0, back, f); }
    if (tid == 0) {
      put_bits(outw, eob_pos, codes[256], lens[256]);
      put_bits(outw, marker_bit, last ? 1u : 0u, 3);                // BFINAL, BTYPE = stored; the padding bits are zero already
    }
    __syncthreads();
    if (tid < 2) {   // LEN = 0, NLEN = 0xFFFF at a byte position: two bytes of ones
      const unsigned bytepos = marker_byte + 2 + tid;
      atomicOr(&outw[bytepos >> 2], 0xffu << (8 * (bytepos & 3)));
    }
    __syncthreads();
    unsigned* dst = reinterpret_cast<unsigned*>(slot);
    for (unsigned w = tid; w * 4 < coded_bytes; w += kThreads) dst[w] = outw[w];
    if (tid == 0) sizes[seg] = coded_bytes;
  } else {
    // one stored block (n <= 65535) and the marker
    if (tid == 0) {
      slot[0] = 0; slot[1] = (uint8_t)(n & 0xff); slot[2] = (uint8_t)(n >> 8); slot[3] = (uint8_t)(~n & 0xff); slot[4] = (uint8_t)((~n >> 8) & 0xff);
      uint8_t* m = slot + 5 + n;
      m[0] = last ? 1 : 0; m[1] = 0; m[2] = 0; m[3] = 0xff; m[4] = 0xff;
      sizes[seg] = stored_bytes;
    }
    for (int p = tid; p < n; p += kThreads) slot[5 + p] = in[ia(p)];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Compaction: exclusive prefix sum of the segment sizes (one workgroup; offs[nseg] = the stream's length), then one workgroup per
// segment moves its bytes to their place.
__global__ __launch_bounds__(1024) void k_png_scan(const unsigned* __restrict__ sizes, int nseg, unsigned long long* __restrict__ offs) {
  __shared__ unsigned long long part[1024];
  const int tid = threadIdx.x;
  const int per = (nseg + 1023) / 1024;
  const int lo = min(tid * per, nseg), hi = min(lo + per, nseg);
  unsigned long long s = 0;
  for (int i = lo; i < hi; ++i) s += sizes[i];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    unsigned long long acc = 0;
    for (int i = 0; i < 1024; ++i) { const unsigned long long v = part[i]; part[i] = acc; acc += v; }
    offs[nseg] = acc;
  }
  __syncthreads();
  unsigned long long acc = part[tid];
  for (int i = lo; i < hi; ++i) { offs[i] = acc; acc += sizes[i]; }
}

__global__ __launch_bounds__(kThreads) void k_png_gather(const uint8_t* __restrict__ slots, const unsigned* __restrict__ sizes,
                                                         const unsigned long long* __restrict__ offs, uint8_t* __restrict__ packed) {
  const size_t seg = blockIdx.x;
  const uint8_t* src = slots + seg * kSlot;
  uint8_t* dst = packed + offs[seg];
  const unsigned n = sizes[seg];
  for (unsigned p = threadIdx.x; p < n; p += kThreads) dst[p] = src[p];
}

}  // namespace

size_t png_stream_alloc_bytes(int cols, int rows) { return (png_frame::stream_bytes(cols, rows) + 3) & ~size_t(3); }

void launch_png_filter(hipStream_t st, const uint8_t* bgra, int cols, int rows, const PngWork& w) {
  hipLaunchKernelGGL(k_png_filter, dim3((unsigned)std::min(rows, 1 << 20)), dim3(kThreads), 0, st, (const uint32_t*)bgra, cols, rows, w.stream);
}
void launch_png_deflate(hipStream_t st, int cols, int rows, const PngWork& w) {
  const size_t total = png_frame::stream_bytes(cols, rows);
  hipLaunchKernelGGL(k_png_deflate, dim3((unsigned)png_frame::segments(total)), dim3(kThreads), 0, st, w.stream, (unsigned long long)total, w.slots, w.sizes, w.adler);
}
void launch_png_pack(hipStream_t st, int cols, int rows, const PngWork& w) {
  const int nseg = (int)png_frame::segments(png_frame::stream_bytes(cols, rows));
  hipLaunchKernelGGL(k_png_scan, dim3(1), dim3(1024), 0, st, w.sizes, nseg, w.offs);
  hipLaunchKernelGGL(k_png_gather, dim3((unsigned)nseg), dim3(kThreads), 0, st, w.slots, w.sizes, w.offs, w.packed);
}

}  // namespace pf
