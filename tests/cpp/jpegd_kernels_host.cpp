// The JPEG decoder's kernels (csrc/kernels_jpegd.hip) run on the host, thread for thread, under the address and undefined-behaviour
// sanitizers: every buffer has exactly the size the library gives it (the file: exactly its bytes), so a read past the segment, a
// coefficient past the last block, a state past the last subsequence or an index past an LDS array is caught here, without a GPU.
//   decode S [IN.jpg OUT.bin]... one file through the kernels as the library drives them; OUT.bin: 8 int32 (parsed, event MCU or -1,
//                                subsequences, rounds, launches, coefficient bytes, plane bytes, 0), then BGRA, coefficients, planes, states
//   variants S IN.pack OUT.txt   IN.pack: uint32 count, then per file uint32 length and its bytes.  One line per file: "P" (the parser
//                                refuses it), "R <mcu>" (the scan is refused: the MCU where decoding stopped) or "A <fnv1a of BGRA>"
// Built and run by tests/test_jpegd_kernels_host.py:  g++ -std=c++20 -fsanitize=address,undefined -Itests/cpp/hip_host_shim ... -pthread
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <string>

#include <hip/hip_runtime.h>

// what this kernel file uses beyond the shim's set
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline unsigned atomicMin(unsigned* p, unsigned v) {
  unsigned o = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
  return o;
}
inline unsigned atomicMax(unsigned* p, unsigned v) {
  unsigned o = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (v > o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
  return o;
}
inline std::atomic<int> host_shim_or{0};
inline int __syncthreads_or(int p) {
  if (p) host_shim_or.store(1);
  __syncthreads();
  const int r = host_shim_or.load();
  __syncthreads();
  if (threadIdx.x == 0) host_shim_or.store(0);
  __syncthreads();
  return r;
}

#include "../../panorama-opticalflow_amd/csrc/kernels_jpegd.hip"

using namespace pf;

static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

struct Result {
  bool parsed = false; unsigned event = 0xFFFFFFFFu; unsigned nsub = 0; int rounds = 0, launches = 0;
  std::vector<uint8_t> bgra, planes; std::vector<int16_t> coef; std::vector<JdState> states;
  std::string why;
};

// the library's jpegd_decode_group for one file, buffers at their exact sizes
static Result run(const std::vector<uint8_t>& file, unsigned S) {
  Result r;
  jpeg_parse::Info f;
  // (the parser reads a buffer of exactly the file's bytes: a copy, so that the sanitizer sees its end)
  std::vector<uint8_t> exact(file);
  if (!jpeg_parse::parse(exact.data(), exact.size(), &f, &r.why)) return r;
  r.parsed = true;
  const uint64_t seg = f.end - f.begin;
  const unsigned nsub = (unsigned)std::max<uint64_t>(1, (seg + S - 1) / S);
  r.nsub = nsub;
  std::vector<jpeg_parse::Tables> tab(1, f.tab);
  std::vector<JdState> st0(nsub), st1(nsub);
  std::vector<uint32_t> first(size_t(nsub) * 2);
  r.coef.assign(size_t(f.blocks()) * 64, 0);
  r.planes.assign(size_t(f.mcus()) * 64 * (f.ncomp == 3 ? f.hs * f.vs + 2 : 1), 0xEE);
  r.bgra.assign(size_t(f.cols) * f.rows * 4, 0xEE);
  std::vector<unsigned> words = {0, 0, 0xFFFFFFFFu, 0};
  JpegdWork w;
  w.seg = exact.data() + f.begin; w.seg_bytes = (unsigned)seg; w.S = S; w.nsub = nsub; w.ncomp = f.ncomp; w.hs = f.hs; w.vs = f.vs;
  w.restart = f.restart; w.cols = f.cols; w.rows = f.rows; w.tables = tab.data(); w.states[0] = st0.data(); w.states[1] = st1.data();
  w.words = words.data(); w.first = first.data(); w.coef = r.coef.data(); w.planes = r.planes.data();
  const unsigned groups = (nsub + kJdThreads - 1) / kJdThreads;
  int from = 0;
  for (;;) {
    words[0] = 0; words[1] = 0;
    host_shim_launch(k_jpegd_sync, groups, (unsigned)kJdThreads, w, r.launches == 0 ? 1 : 0, (const JdState*)w.states[from], (JdState*)w.states[1 - from]);
    from ^= 1; r.launches += 1; r.rounds += (int)words[1];
    if (!words[0]) break;
    if (r.launches > (int)groups + 1) { r.why = "the synchronisation did not settle"; r.parsed = false; return r; }
  }
  host_shim_launch(k_jpegd_place, 1u, 1024u, (const JdState*)w.states[from], nsub, first.data());
  host_shim_launch(k_jpegd_write, groups, (unsigned)kJdThreads, w, (const JdState*)w.states[from], (const uint32_t*)first.data());
  const unsigned nint = f.restart ? (unsigned)((f.mcus() + f.restart - 1) / f.restart) : 1u;
  const unsigned chunks = jpegd_dc_chunks(f.ncomp, f.hs, f.vs, f.restart, (unsigned)f.mcus());
  std::vector<unsigned> dcsum(size_t(nint) * f.ncomp * chunks);
  w.dcsum = dcsum.data();
  if (chunks > 1) host_shim_launch(k_jpegd_dc<0>, nint * (unsigned)f.ncomp * chunks, 256u, w, chunks, dcsum.data());
  host_shim_launch(k_jpegd_dc<1>, nint * (unsigned)f.ncomp * chunks, 256u, w, chunks, dcsum.data());
  host_shim_launch(k_jpegd_idct, (unsigned)((f.blocks() + kJdIdctBlocks - 1) / kJdIdctBlocks), 256u, w);
  host_shim_launch(k_jpegd_pixels, (unsigned)((size_t(f.cols) * f.rows + 255) / 256), 256u, w, (uint32_t*)r.bgra.data());
  r.event = words[2];
  r.states = from ? st1 : st0;
  return r;
}

static int decode(unsigned S, const char* in, const char* out) {
  const std::vector<uint8_t> file = read_file(in);
  const Result r = run(file, S);
  FILE* f = fopen(out, "wb");
  if (!f) { printf("cannot write %s\n", out); return 2; }
  const int head[8] = {r.parsed ? 1 : 0, r.event == 0xFFFFFFFFu ? -1 : (int)r.event, (int)r.nsub, r.rounds, r.launches, (int)(r.coef.size() * 2), (int)r.planes.size(), 0};
  fwrite(head, 4, 8, f);
  fwrite(r.bgra.data(), 1, r.bgra.size(), f); fwrite(r.coef.data(), 2, r.coef.size(), f); fwrite(r.planes.data(), 1, r.planes.size(), f);
  fwrite(r.states.data(), sizeof(JdState), r.states.size(), f);
  fclose(f);
  if (!r.parsed) printf("refused: %s\n", r.why.c_str());
  return 0;
}

static int variants(unsigned S, const char* in, const char* out) {
  const std::vector<uint8_t> pack = read_file(in);
  FILE* f = fopen(out, "w");
  if (!f || pack.size() < 4) { printf("cannot read %s or write %s\n", in, out); return 2; }
  uint32_t n; memcpy(&n, pack.data(), 4);
  size_t at = 4;
  for (uint32_t k = 0; k < n; ++k) {
    uint32_t len; memcpy(&len, pack.data() + at, 4); at += 4;
    const std::vector<uint8_t> file(pack.begin() + at, pack.begin() + at + len); at += len;
    const Result r = run(file, S);
    if (!r.parsed) fprintf(f, "P\n");
    else if (r.event != 0xFFFFFFFFu) fprintf(f, "R %u\n", r.event);
    else {
      uint64_t h = 1469598103934665603ull;
      for (uint8_t b : r.bgra) { h ^= b; h *= 1099511628211ull; }
      fprintf(f, "A %llu\n", (unsigned long long)h);
    }
  }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 5 && argc % 2 == 1 && !strcmp(argv[1], "decode")) { for (int i = 3; i < argc; i += 2) if (int e = decode((unsigned)atoi(argv[2]), argv[i], argv[i + 1])) return e; }
  else if (argc == 5 && !strcmp(argv[1], "variants")) { if (int e = variants((unsigned)atoi(argv[2]), argv[3], argv[4])) return e; }
  else { printf("usage: %s decode S [IN.jpg OUT.bin]... | variants S IN.pack OUT.txt\n", argv[0]); return 2; }
  printf("ok\n");
  return 0;
}
