// Baseline JPEG on the device: packed BGRA in HBM -> the entropy-coded segment of libjpeg's own file, byte for byte.
//   k_jpeg_blocks   reads the image once: colour transform, edge replication by clamped indices (no padded plane), 2x2 chroma
//                   downsampling, libjpeg's integer DCT (jfdctint), quantisation, zigzag; int16 coefficients in MCU order, the dummy
//                   luma blocks of 4:2:0 included (all AC zero, the DC of the block before them), so the coder treats every block alike
//   k_jpeg_size     one workgroup per restart interval runs the coder in LDS and keeps only the interval's byte count
//   k_jpeg_scan     exclusive prefix sum of those counts: every interval's place in the segment, and the segment's length
//   k_jpeg_write    the coder again, its bytes straight to their final place
// The coder: the interval's coefficients are staged in LDS; a thread per block forms the DC difference from the neighbour's stored DC
// and counts its bits; a workgroup prefix sum places the bit strings; they are merged into an LDS window of kWinBytes (atomicOr on
// big-endian words), window after window, so that no image can outgrow LDS; a byte-level scan per window does the 0xFF stuffing.
// Plain C++ throughout: the host-run test (tests/cpp/jpeg_kernels_host.cpp) compiles this file as it is.
#include <algorithm>

#include "pf_common.hpp"
#include "jpeg_frame.hpp"

namespace pf {
namespace {

using jpeg_frame::Tables;

// ---------------------------------------------------------------------------------------------------------------------------------
// k_jpeg_blocks: a workgroup takes a tile of 256 x 16 pixels (16 MCUs of 4:2:0) or 256 x 8 (32 MCUs of 4:4:4): 96 blocks either way
constexpr int kBlkThreads = 256;
constexpr int kTileBlocks = 96;
constexpr int kWsBlock = 73, kWsRow = 9;   // the DCT workspace's strides in dwords: odd, so that neither pass meets a bank twice

constexpr int fix(double x) { return int(x * 65536 + 0.5); }

__device__ __forceinline__ void ycc(uint32_t v, int& y, int& cb, int& cr) {
  const int b = v & 0xff, g = (v >> 8) & 0xff, r = (v >> 16) & 0xff;
  y = (fix(.299) * r + fix(.587) * g + fix(.114) * b + 32768) >> 16;
  cb = (-fix(.16874) * r - fix(.33126) * g + fix(.5) * b + (128 << 16) + 32767) >> 16;
  cr = (fix(.5) * r - fix(.41869) * g - fix(.08131) * b + (128 << 16) + 32767) >> 16;
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jfdctint over d[0..7]; FIRST: the row pass (results scaled up by 4), else the column pass (scaled back, and by 8 overall)
template <bool FIRST>
__device__ __forceinline__ void fdct8(const int* d, int* o) {
  constexpr int n = FIRST ? 11 : 15;
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  o[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
  o[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
  int z1 = (t12 + t13) * 4433;
  o[2] = descale(z1 + t13 * 6270, n);
  o[6] = descale(z1 - t12 * 15137, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
  z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
  o[7] = descale(u4 + z1 + z3, n);
  o[5] = descale(u5 + z2 + z4, n);
  o[3] = descale(u6 + z2 + z3, n);
  o[1] = descale(u7 + z1 + z4, n);
}

__global__ __launch_bounds__(kBlkThreads) void k_jpeg_blocks(const uint32_t* __restrict__ bgra, int cols, int rows, int sub, int mcu_cols, int tiles_x,
                                                             const Tables* __restrict__ tab, int16_t* __restrict__ coef) {
  __shared__ uint8_t samp[kTileBlocks * 64];           // samples, block after block
  __shared__ int ws[kTileBlocks * kWsBlock];           // the row pass's results
  __shared__ uint32_t outw[kTileBlocks * 32];          // quantised coefficients in zigzag order, two int16 to a word
  int16_t* const out = reinterpret_cast<int16_t*>(outw);
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % tiles_x, my = blockIdx.x / tiles_x;
  const int tile_mcus = sub ? 16 : 32, bpm = sub ? 6 : 3;
  const int nm = min(tile_mcus, mcu_cols - tile * tile_mcus);   // MCUs of this tile that exist
  const int px0 = tile * 256;
  const size_t W = (size_t)cols;

  // ---- samples ----
  if (sub) {
    const int crows = (rows + 1) >> 1;   // rows of the downsampled planes before their own padding
    for (int q = tid; q < 1024; q += kBlkThreads) {   // 2x2 quads of the tile
      const int qx = q & 127, qy = q >> 7, m = qx >> 3;
      if (m >= nm) continue;
      const int xa = min(px0 + 2 * qx, cols - 1), xb = min(px0 + 2 * qx + 1, cols - 1);
      const int yl0 = min(my * 16 + 2 * qy, rows - 1), yl1 = min(my * 16 + 2 * qy + 1, rows - 1);
      // chroma: the last column of the FULL plane is replicated before downsampling (xa, xb above), its last row to an even count
      // (yc1), and the last DOWNSAMPLED row below that (cy)
      const int cy = min(my * 8 + qy, crows - 1), yc0 = 2 * cy, yc1 = min(2 * cy + 1, rows - 1);
      uint32_t p[4] = {bgra[yl0 * W + xa], bgra[yl0 * W + xb], bgra[yl1 * W + xa], bgra[yl1 * W + xb]};
      int y[4], cb[4], cr[4];
      for (int i = 0; i < 4; ++i) ycc(p[i], y[i], cb[i], cr[i]);
      if (yc0 != yl0 || yc1 != yl1) {
        const uint32_t c[4] = {bgra[yc0 * W + xa], bgra[yc0 * W + xb], bgra[yc1 * W + xa], bgra[yc1 * W + xb]};
        int unused;
        for (int i = 0; i < 4; ++i) ycc(c[i], unused, cb[i], cr[i]);
      }
      for (int i = 0; i < 4; ++i) {
        const int lx = 2 * qx + (i & 1), ly = 2 * qy + (i >> 1);
        samp[(m * 6 + ((ly >> 3) << 1 | ((lx & 15) >> 3))) * 64 + (ly & 7) * 8 + (lx & 7)] = (uint8_t)y[i];
      }
      const int bias = 1 + (qx & 1), at = qy * 8 + (qx & 7);
      samp[(m * 6 + 4) * 64 + at] = (uint8_t)((cb[0] + cb[1] + cb[2] + cb[3] + bias) >> 2);
      samp[(m * 6 + 5) * 64 + at] = (uint8_t)((cr[0] + cr[1] + cr[2] + cr[3] + bias) >> 2);
    }
  } else {
    for (int q = tid; q < 2048; q += kBlkThreads) {
      const int lx = q & 255, ly = q >> 8, m = lx >> 3;
      if (m >= nm) continue;
      const int x = min(px0 + lx, cols - 1), yy = min(my * 8 + ly, rows - 1);
      int y, cb, cr;
      ycc(bgra[yy * W + x], y, cb, cr);
      const int at = m * 3 * 64 + ly * 8 + (lx & 7);
      samp[at] = (uint8_t)y; samp[at + 64] = (uint8_t)cb; samp[at + 128] = (uint8_t)cr;
    }
  }
  __syncthreads();   // B1: the samples are in LDS

  // ---- row pass: an item is a row of a block ----
  const int nblk = nm * bpm;
  for (int it = tid; it < nblk * 8; it += kBlkThreads) {
    const int blk = it >> 3, r = it & 7;
    int d[8], o[8];
    for (int k = 0; k < 8; ++k) d[k] = (int)samp[blk * 64 + r * 8 + k] - 128;
    fdct8<true>(d, o);
    for (int k = 0; k < 8; ++k) ws[blk * kWsBlock + r * kWsRow + k] = o[k];
  }
  __syncthreads();   // B2: every row is transformed

  // ---- column pass, quantisation, zigzag: an item is a column of a block ----
  const int bcols = (cols + 7) >> 3, brows = (rows + 7) >> 3;   // luma blocks that hold pixels
  for (int it = tid; it < nblk * 8; it += kBlkThreads) {
    const int blk = it >> 3, c = it & 7, m = blk / bpm, j = blk - m * bpm;
    const int cls = sub ? (j >= 4) : (j >= 1);
    const bool dummy = sub && j < 4 && (2 * (tile * 16 + m) + (j & 1) >= bcols || 2 * my + (j >> 1) >= brows);
    int d[8], o[8];
    for (int k = 0; k < 8; ++k) d[k] = ws[blk * kWsBlock + k * kWsRow + c];
    fdct8<false>(d, o);
    for (int k = 0; k < 8; ++k) {
      const int z = tab->unzig[k * 8 + c];
      const int qv = tab->qv[cls][z];
      const int a = o[k] < 0 ? -o[k] : o[k];
      const int v = (a + (qv >> 1)) / qv;   // round half away from zero
      out[blk * 64 + z] = dummy ? (int16_t)0 : (int16_t)(o[k] < 0 ? -v : v);
    }
  }
  __syncthreads();   // B3: every block's coefficients are in LDS
  // dummy luma blocks take the DC of the block before them in the MCU, in order: a thread per MCU, nothing shared between threads
  if (sub && tid < nm) {
    for (int j = 1; j < 4; ++j)
      if (2 * (tile * 16 + tid) + (j & 1) >= bcols || 2 * my + (j >> 1) >= brows) out[(tid * 6 + j) * 64] = out[(tid * 6 + j - 1) * 64];
  }
  __syncthreads();   // B4: ... and the dummies' DCs
  uint32_t* dst = reinterpret_cast<uint32_t*>(coef + ((size_t)my * mcu_cols + (size_t)tile * tile_mcus) * bpm * 64);
  for (int i = tid; i < nblk * 32; i += kBlkThreads) dst[i] = outw[i];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The entropy coder: one workgroup per restart interval
constexpr int kEntThreads = 192;
constexpr int kMaxIntBlocks = 2 * kEntThreads;    // blocks an interval may have (the product's intervals have kEntThreads)
constexpr int kWinBytes = 4096, kWinWords = kWinBytes / 4, kWinBits = kWinBytes * 8;
constexpr int kCoefStride = 33;   // dwords per block in LDS: 32 and one, so that the threads' blocks start in different banks
static_assert(jpeg_frame::kBlockBits <= kWinBits, "a block spans at most two windows");

// exclusive prefix sum of v over the workgroup's threads (Hillis-Steele on two LDS rows); total = the sum.  Every thread calls it.
__device__ unsigned wg_excl_scan(unsigned v, unsigned* buf /* [2 * kEntThreads] */, unsigned& total) {
  const int t = threadIdx.x;
  int cur = 0;
  buf[t] = v;
  __syncthreads();
  for (int off = 1; off < kEntThreads; off <<= 1) {
    const unsigned x = buf[cur * kEntThreads + t] + (t >= off ? buf[cur * kEntThreads + t - off] : 0u);
    buf[(cur ^ 1) * kEntThreads + t] = x;
    cur ^= 1;
    __syncthreads();
  }
  total = buf[cur * kEntThreads + kEntThreads - 1];
  const unsigned incl = buf[cur * kEntThreads + t];
  __syncthreads();   // buf may be written again
  return incl - v;
}

__device__ __forceinline__ int bit_length(int a) { return 32 - __clz(a); }   // a > 0

// the code words of one block, in order, to put(code, length); length <= 26 (a Huffman code and the value's bits as one word)
template <class Put>
__device__ __forceinline__ void code_block(const int16_t* __restrict__ c, int pred, const uint32_t* dc, const uint32_t* ac, Put put) {
  const int d = (int)c[0] - pred;
  {
    const int s = d ? bit_length(d < 0 ? -d : d) : 0;
    const uint32_t h = dc[s];
    put((h >> 5) << s | (unsigned)((d < 0 ? d - 1 : d) & ((1 << s) - 1)), (int)(h & 31) + s);
  }
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = c[k];
    if (v == 0) { ++run; continue; }
    for (; run >= 16; run -= 16) { const uint32_t h = ac[0xF0]; put(h >> 5, (int)(h & 31)); }   // ZRL
    const int s = bit_length(v < 0 ? -v : v);
    const uint32_t h = ac[run << 4 | s];
    put((h >> 5) << s | (unsigned)((v < 0 ? v - 1 : v) & ((1 << s) - 1)), (int)(h & 31) + s);
    run = 0;
  }
  if (run) { const uint32_t h = ac[0]; put(h >> 5, (int)(h & 31)); }   // EOB, unless coefficient 63 is not zero
}

// `len` bits of `code` at bit `rel` of the window (which may begin before the window or run past its end: those parts are left out)
__device__ __forceinline__ void put_bits(unsigned* win, int rel, unsigned code, int len) {
  const int w = rel >> 5, sh = rel & 31;   // (an arithmetic shift: floor, also below zero)
  const unsigned long long v = (unsigned long long)code << (64 - len - sh);
  const unsigned hi = (unsigned)(v >> 32), lo = (unsigned)v;
  if (w >= 0 && w < kWinWords && hi) atomicOr(&win[w], hi);
  if (w + 1 >= 0 && w + 1 < kWinWords && lo) atomicOr(&win[w + 1], lo);
}

template <bool WRITE>
__device__ __forceinline__ void jpeg_interval(const int16_t* __restrict__ coef, unsigned long long nmcu, int sub, int restart, const Tables* __restrict__ tab,
                                              unsigned* __restrict__ sizes, const unsigned long long* __restrict__ offs, uint8_t* __restrict__ packed) {
  __shared__ uint32_t s_dc[2][16], s_ac[2][256];
  __shared__ uint32_t s_coef[kEntThreads * kCoefStride];   // the coefficients of kEntThreads blocks ("a round"), two int16 to a word
  __shared__ unsigned s_bits[kMaxIntBlocks];   // a block's first bit
  __shared__ unsigned s_scan[2 * kEntThreads];
  __shared__ unsigned s_win[kWinWords];
  __shared__ uint8_t s_stuffed[WRITE ? 2 * kWinBytes : 4];
  const int tid = threadIdx.x;
  const unsigned long long iv = blockIdx.x, first = iv * (unsigned long long)restart;
  const int bpm = sub ? 6 : 3;
  const int nm = (int)min((unsigned long long)restart, nmcu - first), nblk = nm * bpm;
  const int16_t* const blocks = coef + first * bpm * 64;
  const bool last = first + nm == nmcu;

  for (int i = tid; i < 32; i += kEntThreads) s_dc[i >> 4][i & 15] = tab->dc[i >> 4][i & 15];
  for (int i = tid; i < 512; i += kEntThreads) s_ac[i >> 8][i & 255] = tab->ac[i >> 8][i & 255];
  __syncthreads();   // E1: the code tables are in LDS

  // the predictor of block b: the stored DC of the block of its component before it, zero in the interval's first MCU
  auto pred_of = [&](int b) -> int {
    const int m = b / bpm, j = b - m * bpm;
    const int back = sub ? (j == 0 ? 3 : j < 4 ? 1 : 6) : 3;
    const bool in_mcu = sub && j >= 1 && j < 4;
    return (in_mcu || m > 0) ? (int)blocks[(b - back) * 64] : 0;
  };
  auto cls_of = [&](int b) -> int { const int j = b % bpm; return sub ? (j >= 4) : (j >= 1); };
  // The coefficients come into LDS with coalesced loads, a round of kEntThreads blocks at a time (the product's intervals are one round:
  // staged once; a thread walking its block in global memory would pull a cache line per coefficient).  Every thread calls it; the
  // barriers around the copy are S1 (nobody still reads the round it replaces) and S2 (the round is in LDS).
  int staged = -1;
  auto stage = [&](int round) {
    if (staged == round) return;
    __syncthreads();   // S1
    const int nb = min(kEntThreads, nblk - round * kEntThreads);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(blocks + (size_t)round * kEntThreads * 64);
    for (int w = tid; w < nb * 32; w += kEntThreads) s_coef[(w >> 5) * kCoefStride + (w & 31)] = src[w];
    __syncthreads();   // S2
    staged = round;
  };
  const int16_t* const mine = reinterpret_cast<const int16_t*>(s_coef + tid * kCoefStride);   // this thread's block of the staged round

  // ---- every block's bit count ----
  unsigned cnt[2] = {0, 0};   // this thread's blocks are tid and tid + kEntThreads
  for (int i = 0; i * kEntThreads < nblk; ++i) {
    stage(i);
    const int b = tid + i * kEntThreads;
    if (b >= nblk) continue;
    unsigned n = 0;
    const int cls = cls_of(b);
    code_block(mine, pred_of(b), s_dc[cls], s_ac[cls], [&](unsigned, int len) { n += len; });
    cnt[i] = n;
  }
  // blocks are placed in order b = 0, 1, ...: a scan over the first kEntThreads blocks, then over the rest behind their total
  unsigned tot0, tot1;
  const unsigned e0 = wg_excl_scan(cnt[0], s_scan, tot0);
  const unsigned e1 = wg_excl_scan(cnt[1], s_scan, tot1) + tot0;
  if (tid < nblk) s_bits[tid] = e0;
  if (tid + kEntThreads < nblk) s_bits[tid + kEntThreads] = e1;
  const int total_bits = (int)(tot0 + tot1);
  const int pad = -total_bits & 7, nbytes = (total_bits + pad) >> 3;
  const unsigned long long at = WRITE ? offs[iv] : 0ull;
  unsigned outpos = 0;   // stuffed bytes before the current window (the same in every thread)

  for (int win0 = 0; win0 < nbytes; win0 += kWinBytes) {
    for (int i = tid; i < kWinWords; i += kEntThreads) s_win[i] = 0;
    __syncthreads();   // E2: the window is clear (and s_bits is written, the first time round)
    const int wbit0 = win0 * 8;
    for (int i = 0; i * kEntThreads < nblk; ++i) {
      stage(i);
      const int b = tid + i * kEntThreads;
      if (b >= nblk) continue;
      const int lo = (int)s_bits[b], hi = lo + (int)cnt[i];
      if (hi <= wbit0 || lo >= wbit0 + kWinBits) continue;
      int pos = lo - wbit0;
      const int cls = cls_of(b);
      code_block(mine, pred_of(b), s_dc[cls], s_ac[cls], [&](unsigned code, int len) { put_bits(s_win, pos, code, len); pos += len; });
    }
    if (tid == 0 && pad) put_bits(s_win, total_bits - wbit0, (1u << pad) - 1, pad);   // 1-bits up to the byte
    __syncthreads();   // E3: the window's bits are merged

    // ---- bytes: each thread a run of them; 0xFF takes a 0x00 behind it ----
    const int nb = min(kWinBytes, nbytes - win0), per = (nb + kEntThreads - 1) / kEntThreads;
    const int lo = min(tid * per, nb), hi = min(lo + per, nb);
    unsigned ff = 0;
    for (int i = lo; i < hi; ++i) ff += ((s_win[i >> 2] >> (24 - 8 * (i & 3))) & 0xff) == 0xff;
    unsigned ffs;
    const unsigned before = wg_excl_scan(ff, s_scan, ffs);
    if (WRITE) {
      unsigned j = lo + before;
      for (int i = lo; i < hi; ++i) {
        const uint8_t v = (uint8_t)(s_win[i >> 2] >> (24 - 8 * (i & 3)));
        s_stuffed[j++] = v;
        if (v == 0xff) s_stuffed[j++] = 0;
      }
      __syncthreads();   // E4: the window's stuffed bytes are in LDS
      uint8_t* dst = packed + at + outpos;
      for (unsigned k = tid; k < nb + ffs; k += kEntThreads) dst[k] = s_stuffed[k];
    }
    outpos += nb + ffs;
    __syncthreads();   // E5: the window and the stuffed bytes may be written again
  }
  if (tid == 0) {
    if (WRITE) {
      if (!last) { packed[at + outpos] = 0xFF; packed[at + outpos + 1] = (uint8_t)(0xD0 + (iv & 7)); }
    } else {
      sizes[iv] = outpos + (last ? 0 : 2);
    }
  }
}

__global__ __launch_bounds__(kEntThreads) void k_jpeg_size(const int16_t* __restrict__ coef, unsigned long long nmcu, int sub, int restart,
                                                           const Tables* __restrict__ tab, unsigned* __restrict__ sizes) {
  jpeg_interval<false>(coef, nmcu, sub, restart, tab, sizes, nullptr, nullptr);
}

__global__ __launch_bounds__(kEntThreads) void k_jpeg_write(const int16_t* __restrict__ coef, unsigned long long nmcu, int sub, int restart,
                                                            const Tables* __restrict__ tab, const unsigned long long* __restrict__ offs, uint8_t* __restrict__ packed) {
  jpeg_interval<true>(coef, nmcu, sub, restart, tab, nullptr, offs, packed);
}

// exclusive prefix sum of the intervals' sizes (one workgroup; offs[n] = the segment's length)
__global__ __launch_bounds__(1024) void k_jpeg_scan(const unsigned* __restrict__ sizes, int n, unsigned long long* __restrict__ offs) {
  __shared__ unsigned long long part[1024];
  const int tid = threadIdx.x;
  const int per = (n + 1023) / 1024;
  const int lo = min(tid * per, n), hi = min(lo + per, n);
  unsigned long long s = 0;
  for (int i = lo; i < hi; ++i) s += sizes[i];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    unsigned long long acc = 0;
    for (int i = 0; i < 1024; ++i) { const unsigned long long v = part[i]; part[i] = acc; acc += v; }
    offs[n] = acc;
  }
  __syncthreads();
  unsigned long long acc = part[tid];
  for (int i = lo; i < hi; ++i) { offs[i] = acc; acc += sizes[i]; }
}

}  // namespace

bool jpeg_restart_fits(int subsampling, int restart) { return restart >= 1 && restart <= 65535 && restart * (subsampling ? 6 : 3) <= kMaxIntBlocks; }

void launch_jpeg_blocks(hipStream_t st, const uint8_t* bgra, int cols, int rows, int subsampling, const JpegWork& w) {
  const int mc = (int)jpeg_frame::mcu_cols(cols, subsampling), mr = (int)jpeg_frame::mcu_cols(rows, subsampling);
  const int tile_mcus = subsampling ? 16 : 32, tiles_x = (mc + tile_mcus - 1) / tile_mcus;
  hipLaunchKernelGGL(k_jpeg_blocks, dim3((unsigned)tiles_x * (unsigned)mr), dim3(kBlkThreads), 0, st, (const uint32_t*)bgra, cols, rows, subsampling, mc, tiles_x,
                     (const Tables*)w.tables, w.coef);
}
void launch_jpeg_sizes(hipStream_t st, int cols, int rows, int subsampling, int restart, const JpegWork& w) {
  const unsigned long long nmcu = jpeg_frame::mcus(cols, rows, subsampling);
  const int n = (int)jpeg_frame::intervals(cols, rows, subsampling, restart);
  hipLaunchKernelGGL(k_jpeg_size, dim3((unsigned)n), dim3(kEntThreads), 0, st, (const int16_t*)w.coef, nmcu, subsampling, restart, (const Tables*)w.tables, w.sizes);
  hipLaunchKernelGGL(k_jpeg_scan, dim3(1), dim3(1024), 0, st, (const unsigned*)w.sizes, n, w.offs);
}
void launch_jpeg_write(hipStream_t st, int cols, int rows, int subsampling, int restart, const JpegWork& w, uint8_t* packed) {
  const unsigned long long nmcu = jpeg_frame::mcus(cols, rows, subsampling);
  const int n = (int)jpeg_frame::intervals(cols, rows, subsampling, restart);
  hipLaunchKernelGGL(k_jpeg_write, dim3((unsigned)n), dim3(kEntThreads), 0, st, (const int16_t*)w.coef, nmcu, subsampling, restart, (const Tables*)w.tables,
                     (const unsigned long long*)w.offs, packed);
}

}  // namespace pf
