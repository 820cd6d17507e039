// The PNG encoder's kernels (csrc/kernels_png.hip) run on the host, thread for thread, under the address and undefined-behaviour
// sanitizers: every buffer has exactly the size the library gives it, so an index past a segment, a slot or the stream is caught here,
// without a GPU.  Each file is then framed (csrc/png_frame.hpp), inflated with zlib, unfiltered and compared with the image.
// With arguments, groups of `IN.bgra cols rows OUT.png`: each raw BGRA file is encoded by the same kernels and the framed file written,
// for the byte comparison with the serial model (tests/png_model.py).  The one argument `scan`: k_png_scan alone, on size arrays of
// up to five elements per thread.  Without arguments: the shapes below, and build_code on frequency tables that reach both of its
// length limits.
// Built and run by tests/test_png_kernels_host.py:  g++ -std=c++20 -fsanitize=address,undefined -Itests/cpp/hip_host_shim ... -lz -pthread
#include <stdio.h>

#include <queue>
#include <string.h>
#include <zlib.h>

#include "../../panorama-opticalflow_amd/csrc/kernels_png.hip"

using namespace pf;

static int g_fail = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
  } while (0)

static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

// 0 noise, 1 a gentle gradient, 2 constant zero, 3 constant (7, 7, 7, 255), 4 alpha noise over a flat colour, 5 noise rows between flat rows
static std::vector<uint8_t> make_image(int cols, int rows, int kind, uint32_t seed) {
  std::vector<uint8_t> v(size_t(cols) * rows * 4);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x) {
      uint8_t* p = &v[(size_t(y) * cols + x) * 4];
      for (int ch = 0; ch < 4; ++ch) {
        const uint8_t noise = (uint8_t)rnd(seed);
        const uint8_t flat[4] = {40, 90, 90, 200};
        switch (kind) {
          case 0: p[ch] = noise; break;
          case 1: p[ch] = (uint8_t)(3 * y + 2 * x + 50 * ch); break;
          case 2: p[ch] = 0; break;
          case 3: p[ch] = ch == 3 ? 255 : 7; break;
          case 4: p[ch] = ch == 3 ? noise : flat[ch]; break;
          default: p[ch] = (y / 7) % 2 ? noise : flat[ch]; break;
        }
      }
    }
  return v;
}

static int ref_paeth(int a, int b, int c) {   // the check's own predictor, not the kernel's
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// the file of an image, by the kernels and the host framing the library uses; *stream_out = the filtered scanlines
static std::vector<uint8_t> encode_file(const std::vector<uint8_t>& img, int cols, int rows, std::vector<uint8_t>* stream_out, size_t* nseg_out) {
  const size_t stream = png_frame::stream_bytes(cols, rows), nseg = png_frame::segments(stream);
  std::vector<uint8_t> st(png_stream_alloc_bytes(cols, rows)), slots(nseg * png_frame::kSegSlot), packed(png_frame::deflate_bound(stream));
  std::vector<unsigned> sizes(nseg), adler(nseg);
  std::vector<unsigned long long> offs(nseg + 1);
  host_shim_launch(k_png_filter, (unsigned)std::min(rows, 3), 256u, (const uint32_t*)img.data(), cols, rows, st.data());
  host_shim_launch(k_png_deflate, (unsigned)nseg, 256u, (const uint8_t*)st.data(), (unsigned long long)stream, slots.data(), sizes.data(), adler.data());
  host_shim_launch(k_png_scan, 1u, 1024u, (const unsigned*)sizes.data(), (int)nseg, offs.data());
  host_shim_launch(k_png_gather, (unsigned)nseg, 256u, (const uint8_t*)slots.data(), (const unsigned*)sizes.data(), (const unsigned long long*)offs.data(), packed.data());
  const size_t dlen = offs[nseg];
  CHECK(dlen <= png_frame::deflate_bound(stream));
  if (dlen > png_frame::deflate_bound(stream)) return {};
  for (size_t s = 0; s < nseg; ++s) CHECK(sizes[s] <= std::min(png_frame::kSegBytes, stream - s * png_frame::kSegBytes) + png_frame::kSegOverhead);
  // the zlib stream as the library frames it
  const png_frame::Frame fr(cols, rows, dlen);
  std::vector<uint8_t> file(fr.file_size());
  fr.write_head(file.data());
  for (size_t d = 0; d < dlen;) { size_t run; const size_t at = fr.deflate_run(d, dlen - d, &run); memcpy(file.data() + at, packed.data() + d, run); d += run; }
  uint32_t ad = 1;
  for (size_t s = 0; s < nseg; ++s) ad = png_frame::adler32_combine(ad, adler[s], s + 1 < nseg ? png_frame::kSegBytes : stream - s * png_frame::kSegBytes);
  fr.write_tail(file.data(), ad);
  st.resize(stream);
  *stream_out = st; *nseg_out = nseg;
  return file;
}

static void encode_and_check(int cols, int rows, int kind) {
  const std::vector<uint8_t> img = make_image(cols, rows, kind, cols * 131 + rows * 7 + kind);
  std::vector<uint8_t> st;
  size_t nseg = 0;
  const std::vector<uint8_t> file = encode_file(img, cols, rows, &st, &nseg);
  if (file.empty()) return;
  const size_t stream = png_frame::stream_bytes(cols, rows);
  const png_frame::Frame fr(cols, rows, file.size() - png_frame::Frame(cols, rows, 0).file_size());
  CHECK(file.size() <= png_frame::bound(cols, rows));
  // inflate (zlib checks the Adler-32), unfilter, compare
  std::vector<uint8_t> raw(stream);
  uLongf rn = (uLongf)raw.size();
  const int zr = uncompress(raw.data(), &rn, file.data() + fr.file_offset(0), (uLong)fr.zlib_len());
  CHECK(zr == Z_OK && rn == stream);
  if (zr != Z_OK || rn != stream) { printf("  %dx%d kind %d: zlib says %d\n", cols, rows, kind, zr); return; }
  CHECK(memcmp(raw.data(), st.data(), stream) == 0);
  const size_t stride = size_t(cols) * 4;
  std::vector<uint8_t> prev(stride, 0), cur(stride);
  size_t bad = 0;
  for (int y = 0; y < rows; ++y) {
    const uint8_t* r = raw.data() + size_t(y) * (stride + 1);
    const int ft = r[0];
    CHECK(ft <= 4);
    for (size_t i = 0; i < stride; ++i) {
      const int a = i >= 4 ? cur[i - 4] : 0, b = prev[i], c = i >= 4 ? prev[i - 4] : 0;
      int v = r[1 + i];
      if (ft == 1) v += a; else if (ft == 2) v += b; else if (ft == 3) v += (a + b) >> 1; else if (ft == 4) v += ref_paeth(a, b, c);
      cur[i] = (uint8_t)v;
    }
    const uint8_t* src = &img[size_t(y) * stride];
    for (int x = 0; x < cols; ++x)
      bad += cur[4 * x] != src[4 * x + 2] || cur[4 * x + 1] != src[4 * x + 1] || cur[4 * x + 2] != src[4 * x] || cur[4 * x + 3] != src[4 * x + 3];
    prev.swap(cur);
  }
  CHECK(bad == 0);
  printf("  %dx%d kind %d: %zu segments, file %zu bytes (%.4f of raw)\n", cols, rows, kind, nseg, file.size(), double(file.size()) / double(img.size()));
}

// ---- build_code on given frequency tables ----
__global__ void k_test_build_code(const unsigned* freq, int n, int maxbits, uint8_t* lens, unsigned* codes) {
  __shared__ HuffScratch hs;
  build_code(freq, n, maxbits, lens, codes, hs);
}

// the check's own Huffman tree (a priority queue): the cost of an optimal prefix code and this tree's depth
static void plain_huffman(const std::vector<unsigned>& freq, unsigned long long* cost, int* depth) {
  typedef std::pair<unsigned long long, int> Node;   // weight, height
  std::priority_queue<Node, std::vector<Node>, std::greater<Node>> q;
  for (unsigned f : freq) if (f) q.push(Node(f, 0));
  *cost = 0; *depth = 0;
  while (q.size() > 1) {
    const Node a = q.top(); q.pop();
    const Node b = q.top(); q.pop();
    *cost += a.first + b.first;
    q.push(Node(a.first + b.first, std::max(a.second, b.second) + 1));
  }
  if (!q.empty()) *depth = q.top().second;
}

// returns whether the unrestricted tree was deeper than the limit
static bool check_code(const char* what, std::vector<unsigned> freq, int maxbits) {
  const int n = (int)freq.size();
  std::vector<uint8_t> lens(std::max(n, 2), 0xAB);
  std::vector<unsigned> codes(std::max(n, 2), 0xABABABABu);
  host_shim_launch(k_test_build_code, 1u, 256u, (const unsigned*)freq.data(), n, maxbits, lens.data(), codes.data());
  int used = 0, maxlen = 0, depth = 0;
  unsigned long long kraft = 0, cost = 0, best = 0;
  for (int s = 0; s < n; ++s) {
    used += freq[s] != 0;
    if (lens[s]) { CHECK(lens[s] <= maxbits); kraft += 1ull << (maxbits - std::min<int>(lens[s], maxbits)); maxlen = std::max<int>(maxlen, lens[s]); }
    cost += (unsigned long long)freq[s] * lens[s];
  }
  CHECK(kraft == 1ull << maxbits);                   // complete and not over-subscribed, the lone symbol's partner included
  CHECK(maxlen <= maxbits);
  if (used >= 2) {
    for (int s = 0; s < n; ++s) CHECK((lens[s] != 0) == (freq[s] != 0));
    // lengths do not grow along (freq, index)
    std::vector<int> order;
    for (int s = 0; s < n; ++s) if (freq[s]) order.push_back(s);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return freq[a] < freq[b]; });
    for (size_t i = 1; i < order.size(); ++i) CHECK(lens[order[i]] <= lens[order[i - 1]]);
    plain_huffman(freq, &best, &depth);
    if (depth <= maxbits) CHECK(cost == best); else CHECK(cost >= best);   // what fits costs what plain Huffman costs; a limited code no less
  } else if (used == 1) {
    int sym = 0, ones = 0;
    for (int s = 0; s < n; ++s) { if (freq[s]) sym = s; ones += lens[s] == 1; }
    CHECK(lens[sym] == 1 && ones == 2 && lens[sym == 0 ? 1 : 0] == 1);
  }
  // the codes fit their lengths, are distinct, and none is the start of another
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) {
      if (a == b || !lens[a] || !lens[b] || lens[a] > lens[b]) continue;
      CHECK((codes[b] & ((1u << lens[a]) - 1)) != codes[a]);   // sent from the least significant bit: a start is the low bits
    }
  for (int s = 0; s < n; ++s) if (lens[s]) CHECK(codes[s] >> lens[s] == 0);
  printf("  build_code %s, %d symbols of %d, limit %d: longest %d, plain tree %d deep, cost %llu (optimum %llu)\n", what, used, n, maxbits, maxlen, depth, cost, best);
  return depth > maxbits;
}

static void check_build_code() {
  int limited7 = 0, limited15 = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const int maxbits = pass ? 15 : 7, n = pass ? kLitLen : kClSyms;
    for (int k = pass ? 17 : 10; k <= (pass ? 30 : 19); ++k) {
      // Fibonacci counts 1, 1, 2, 3, ... on k symbols, the rarest at the highest index and the other way round, and spread over the table
      std::vector<unsigned> up(n, 0), down(n, 0), spread(n, 0);
      unsigned a = 1, b = 1;
      for (int i = 0; i < k; ++i) { up[i] = a; down[k - 1 - i] = a; spread[(i * 7) % n] = a; const unsigned c = a + b; a = b; b = c; }
      const bool l1 = check_code("fibonacci rising", up, maxbits), l2 = check_code("fibonacci falling", down, maxbits), l3 = check_code("fibonacci spread", spread, maxbits);
      CHECK(l1 == (k - 1 > maxbits) && l2 == l1 && l3 == l1);
      (pass ? limited15 : limited7) += l1 + l2 + l3;
    }
    check_code("all equal", std::vector<unsigned>(n, 5), maxbits);
    for (int s : {0, 1, n - 1}) { std::vector<unsigned> f(n, 0); f[s] = 9; check_code("one symbol", f, maxbits); }
    { std::vector<unsigned> f(n, 0); f[0] = 1; f[n - 1] = 1000; check_code("two symbols", f, maxbits); }
    { std::vector<unsigned> f(n, 0); f[3] = 4; f[4] = 4; check_code("two equal symbols", f, maxbits); }
  }
  CHECK(limited7 > 0 && limited15 > 0);
}

// k_png_scan on n sizes with values up to 2^32 - 1, buffers at their exact lengths, against a serial prefix sum: a thread sums
// ceil(n / 1024) of them (no image of a size the host can run has more than 1024 segments)
static void check_scan() {
  for (int n : {1, 1023, 1024, 1025, 2048, 2049, 5000}) {
    uint32_t seed = 99u + (uint32_t)n;
    std::vector<unsigned> sizes(n);
    for (int i = 0; i < n; ++i) sizes[i] = i % 5 == 0 ? 0xffffffffu : i % 7 == 0 ? 0u : rnd(seed) << 8 | (rnd(seed) & 0xff);
    std::vector<unsigned long long> offs(n + 1, 0xA5A5A5A5A5A5A5A5ull);
    host_shim_launch(k_png_scan, 1u, 1024u, (const unsigned*)sizes.data(), n, offs.data());
    unsigned long long acc = 0;
    int bad = 0;
    for (int i = 0; i < n; ++i) { bad += offs[i] != acc; acc += sizes[i]; }
    bad += offs[n] != acc;
    CHECK(bad == 0);
    printf("  k_png_scan n = %d (%d per thread): total %llu, %d of %d offsets differ\n", n, (n + 1023) / 1024, acc, bad, n + 1);
  }
}

static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

static int encode_files(int argc, char** argv) {
  if ((argc - 1) % 4) { printf("usage: %s [IN.bgra cols rows OUT.png]...\n", argv[0]); return 2; }
  for (int i = 1; i < argc; i += 4) {
    const int cols = atoi(argv[i + 1]), rows = atoi(argv[i + 2]);
    const std::vector<uint8_t> img = read_file(argv[i]);
    if (cols <= 0 || rows <= 0 || img.size() != size_t(cols) * rows * 4) { printf("%s is not %d x %d BGRA\n", argv[i], cols, rows); return 2; }
    std::vector<uint8_t> st;
    size_t nseg = 0;
    const std::vector<uint8_t> file = encode_file(img, cols, rows, &st, &nseg);
    FILE* f = fopen(argv[i + 3], "wb");
    if (!f || fwrite(file.data(), 1, file.size(), f) != file.size()) { printf("cannot write %s\n", argv[i + 3]); return 2; }
    fclose(f);
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "scan")) {
    check_scan();
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("ok\n");
    return 0;
  }
  if (argc > 1) return encode_files(argc, argv);
  // (a barrier of 256 host threads is slow: few rows, and only the shapes at which an index can go wrong)
  const int cases[][3] = {{1, 1, 0}, {1, 5, 1}, {7, 1, 1}, {65, 3, 0}, {65, 3, 1},   // no neighbours; a row around 256 bytes
                          {341, 12, 0}, {341, 12, 1}, {341, 13, 1},                     // rows of 1365 bytes: exactly one segment, and a row more
                          {1366, 9, 4}, {1366, 9, 5}};                                  // four segments; runs across thread chunks and segment ends
  for (const auto& cs : cases) encode_and_check(cs[0], cs[1], cs[2]);
  encode_and_check(4099, 3, 2);   // matches of 258 end to end, a run longer than a segment
  check_build_code();
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}
