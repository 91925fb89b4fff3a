// TEST INFRASTRUCTURE.  csrc/pcd_parse.hpp compiled for the CPU: the text -> fp32 arithmetic and the run-wise line machine exactly as
// the kernels of csrc/pcd_read.hip run them, compared HERE against the C library's strtof and against a plain sequential split
// (tests/test_pcd_read_cpu.py), plus a sequential strtof loop over a file's body as the baseline of tools/pcd_read_probe.py.
//   g++ -O2 -std=c++17 -shared -fPIC harness.cpp -o libpcdreademu.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DPCD_READ_HARNESS_MAIN harness.cpp -o pcd_read_harness && ./pcd_read_harness
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define __device__
#define __host__
#define LSR_HOST_EMU 1
#include "../../lidarslam_ros2_amd/csrc/pcd_parse.hpp"

using namespace lsr;

namespace {
bool is_nan_bits(uint32_t b) { return (b & 0x7f800000u) == 0x7f800000u && (b & 0x7fffffu); }

// the C library's answer for a whole token (NUL-terminated); a NaN is pinned to the quiet NaN of its sign
uint32_t strtof_bits(const char* text) {
  const float f = std::strtof(text, nullptr);
  uint32_t b;
  std::memcpy(&b, &f, 4);
  if (is_nan_bits(b)) b = (b & 0x80000000u) | 0x7fc00000u;
  return b;
}

struct Mismatch {
  long long count = 0, unresolved = 0;
  char text[64] = {0};
  uint32_t got = 0, want = 0;
};

void check_text(const char* text, uint32_t want, Mismatch* M) {
  uint32_t got = 0xdeadbeefu;
  const int st = pcd_parse_float(reinterpret_cast<const unsigned char*>(text), (int)std::strlen(text), &got);
  if (st == PCD_TOK_UNRESOLVED) M->unresolved++;
  if (st == PCD_TOK_OK && got == want) return;
  if (M->count++ == 0) {
    std::snprintf(M->text, sizeof(M->text), "%s", text);
    M->got = st == PCD_TOK_OK ? got : 0xdead0000u + (uint32_t)st;
    M->want = want;
  }
}

// "%.9g" must give the bits back, "%.8g" what strtof makes of that text
void check_bits(uint32_t bits, Mismatch* M) {
  float f;
  std::memcpy(&f, &bits, 4);
  char text[64];
  std::snprintf(text, sizeof(text), "%.9g", (double)f);
  check_text(text, is_nan_bits(bits) ? ((bits & 0x80000000u) | 0x7fc00000u) : bits, M);
  if (strtof_bits(text) != (is_nan_bits(bits) ? ((bits & 0x80000000u) | 0x7fc00000u) : bits)) M->count++;   // the premise itself
  std::snprintf(text, sizeof(text), "%.8g", (double)f);
  check_text(text, strtof_bits(text), M);
}

void report(const Mismatch& M, char* text64, uint32_t* got, uint32_t* want, long long* unresolved) {
  if (unresolved) *unresolved = M.unresolved;
  if (!M.count) return;
  if (text64) std::strcpy(text64, M.text);
  if (got) *got = M.got;
  if (want) *want = M.want;
}

// a plain sequential split: the offsets of the first non-blank byte of every line that has one
std::vector<size_t> plain_line_starts(const unsigned char* t, size_t n) {
  std::vector<size_t> out;
  size_t i = 0;
  while (i < n) {
    size_t e = i;
    while (e < n && t[e] != '\n') e++;
    size_t s = i;
    while (s < e && (t[s] == ' ' || t[s] == '\t' || t[s] == '\r')) s++;
    if (s < e) out.push_back(s);
    i = e + 1;
  }
  return out;
}

// the kernels' way: runs of `run` bytes, their summaries composed in order (the count), then every run walked with the entry state and
// the slot the composition gives it (the offsets)
bool runwise_matches(const unsigned char* t, size_t n, size_t run, const std::vector<size_t>& want) {
  const size_t nr = pcd_run_count(t, n, run);
  std::vector<PcdRun> prefix(nr + 1);
  prefix[0] = pcd_run_identity();
  size_t covered = 0;
  for (size_t g = 0; g < nr; g++) {
    size_t a, b;
    pcd_run_bounds(t, n, run, g, &a, &b);
    if (a != covered || b < a) return false;
    covered = b;
    prefix[g + 1] = pcd_run_compose(prefix[g], pcd_run_of(t, a, b));
  }
  if (covered != n || prefix[nr].c0 != want.size()) return false;
  std::vector<size_t> got(want.size(), (size_t)-1);
  for (size_t g = 0; g < nr; g++) {
    size_t a, b;
    pcd_run_bounds(t, n, run, g, &a, &b);
    size_t slot = prefix[g].c0;
    const uint32_t state = prefix[g].f & 1u;
    const uint32_t behind = pcd_run_index(t, a, b, state, [&](size_t i) {
      if (slot < got.size()) got[slot] = i;
      slot++;
    });
    if (behind != (prefix[g + 1].f & 1u) || slot != prefix[g + 1].c0) return false;
  }
  return got == want;
}
}  // namespace

extern "C" {

int emu_pcdr_parse(const char* text, int len, uint32_t* bits) { return pcd_parse_float(reinterpret_cast<const unsigned char*>(text), len, bits); }

// n NUL-terminated tokens back to back: status and bits from the parser, strtof's bits, whether strtof took the whole token
void emu_pcdr_batch(const char* blob, long long n, int* status, uint32_t* bits, uint32_t* want, int* whole) {
  const char* p = blob;
  for (long long i = 0; i < n; i++) {
    const size_t len = std::strlen(p);
    bits[i] = 0;
    status[i] = pcd_parse_float(reinterpret_cast<const unsigned char*>(p), (int)len, &bits[i]);
    char* end = nullptr;
    const float f = std::strtof(p, &end);
    std::memcpy(&want[i], &f, 4);
    if (is_nan_bits(want[i])) want[i] = (want[i] & 0x80000000u) | 0x7fc00000u;
    whole[i] = len > 0 && end == p + len;
    p += len + 1;
  }
}

// every exponent field x both signs x (the four fixed mantissas + n_stride mantissas k * stride mod 2^23)
long long emu_pcdr_sweep(uint32_t n_stride, uint32_t stride, char* text64, uint32_t* got, uint32_t* want, long long* n_checked,
                         long long* unresolved) {
  Mismatch M;
  long long checked = 0;
  const uint32_t fixed[4] = {0u, 1u, 0x400000u, 0x7fffffu};
  for (uint32_t sign = 0; sign < 2; sign++)
    for (uint32_t ex = 0; ex < 256; ex++) {
      const uint32_t hi = (sign << 31) | (ex << 23);
      for (uint32_t m : fixed) { check_bits(hi | m, &M); checked++; }
      uint32_t m = stride & 0x7fffffu;
      for (uint32_t k = 0; k < n_stride; k++) {
        check_bits(hi | m, &M);
        checked++;
        m = (m + stride) & 0x7fffffu;
      }
    }
  if (n_checked) *n_checked = checked;
  report(M, text64, got, want, unresolved);
  return M.count;
}

long long emu_pcdr_check_list(const uint32_t* bits, long long n, char* text64, uint32_t* got, uint32_t* want, long long* unresolved) {
  Mismatch M;
  for (long long i = 0; i < n; i++) check_bits(bits[i], &M);
  report(M, text64, got, want, unresolved);
  return M.count;
}

// n_texts random texts over {'\n', ' ', '\t', '\r', 'a'} of lengths 0 .. 300, each at every start misalignment 0 .. 15 and cut into runs
// of every length 1 .. 64: the run-wise logic against the plain split.  Returns the number of disagreements.
long long emu_pcdr_lines(int n_texts, uint32_t seed, long long* n_checked) {
  static const unsigned char alphabet[5] = {'\n', ' ', '\t', '\r', 'a'};
  uint64_t state = seed * 2654435761ull + 12345u;
  auto next = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
  long long bad = 0, checked = 0;
  alignas(16) static unsigned char buf[16 + 300 + 16];
  for (int t = 0; t < n_texts; t++) {
    const size_t n = t == 0 ? 0 : (t == 1 ? 300 : next() % 301u);
    std::vector<unsigned char> text(n);
    // a few texts are mostly letters, a few mostly newlines
    const uint32_t bias = next() % 4u;
    for (auto& c : text) c = (bias == 1 && next() % 2u) ? 'a' : ((bias == 2 && next() % 2u) ? '\n' : alphabet[next() % 5u]);
    for (size_t mis = 0; mis < 16; mis++) {
      std::memset(buf, 'a', sizeof(buf));   // what lies around the text must not be looked at: letters there would add lines
      if (n) std::memcpy(buf + mis, text.data(), n);
      const std::vector<size_t> want = plain_line_starts(buf + mis, n);
      for (size_t run = 1; run <= 64; run++) {
        if (!runwise_matches(buf + mis, n, run, want)) bad++;
        checked++;
      }
    }
  }
  if (n_checked) *n_checked = checked;
  return bad;
}

// The host way in: strtof over every token of the body of the .pcd file at `path`, one after the other.  Returns the number of tokens
// (-1: the file cannot be read or has no DATA line); *sum receives the sum of the values so that nothing is optimised away.
long long emu_host_strtof_loop(const char* path, double* sum) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return -1;
  std::string data;
  char chunk[1 << 16];
  size_t got;
  while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) data.append(chunk, got);
  std::fclose(f);
  const size_t at = data.find("\nDATA ");
  if (at == std::string::npos) return -1;
  const size_t body = data.find('\n', at + 1);
  if (body == std::string::npos) return -1;
  const char* p = data.c_str() + body + 1;
  long long n = 0;
  double s = 0;
  for (;;) {
    char* end = nullptr;
    const float v = std::strtof(p, &end);   // skips blanks and newlines in front of a token
    if (end == p) break;
    if (v == v) s += v;
    n++;
    p = end;
  }
  if (sum) *sum = s;
  return n;
}

}  // extern "C"

#ifdef PCD_READ_HARNESS_MAIN
// stand-alone form (for a sanitizer build on the host): a thinner sweep, the grammar's edges, the line machine; exit status 1 on any mismatch
int main() {
  char text[64] = {0};
  uint32_t got = 0, want = 0;
  long long n1 = 0, n2 = 0, unresolved = 0;
  const long long m1 = emu_pcdr_sweep(1u << 9, 7919u * 1009u, text, &got, &want, &n1, &unresolved);
  long long m3 = 0;
  const char* accept[] = {"+1", "1.", ".5", "1E5", "1e+05", "007", "-0", "INF", "Infinity", "NaN", "-nan", "3.4028236e38", "7e-46", "1e-400", "1e400",
                          "16777217", "33554434", "0.1000000000000000055511151231257827"};
  for (const char* a : accept) {
    Mismatch M;
    check_text(a, strtof_bits(a), &M);
    m3 += M.count;
  }
  const char* reject[] = {"0x10", "1.2.3", "1e", "1e+", "nan(1)", "1,5", "--1", "1f", ""};
  for (const char* r : reject) {
    uint32_t b;
    if (emu_pcdr_parse(r, (int)std::strlen(r), &b) != PCD_TOK_BAD) m3++;
  }
  const long long m2 = emu_pcdr_lines(40, 7u, &n2);
  std::printf("checked %lld values and %lld cuts, %lld mismatches, %lld unresolved\n", n1, n2, m1 + m2 + m3, unresolved);
  if (m1) std::printf("first: text '%s' got 0x%08x want 0x%08x\n", text, got, want);
  return (m1 + m2 + m3 || unresolved) ? 1 : 0;
}
#endif
