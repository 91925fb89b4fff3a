// TEST INFRASTRUCTURE.  csrc/pcd_format.hpp compiled for the CPU: the float -> "%.8g" formatter exactly as the kernels of
// csrc/pcd_text.hip run it, compared HERE against the C library's snprintf("%.8g", (double)f) (tests/test_pcd_ascii_cpu.py), plus a host
// restatement of the loop of PCL's ASCII writer as the baseline of tools/pcd_probe.py.
//   g++ -O2 -std=c++17 -shared -fPIC harness.cpp -o libpcdemu.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DPCD_HARNESS_MAIN harness.cpp -o pcd_harness && ./pcd_harness
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#define __device__
#define __host__
#define LSR_HOST_EMU 1
#include "../../lidarslam_ros2_amd/csrc/pcd_format.hpp"

using namespace lsr;

namespace {
// the C library's answer; every NaN is "nan" (the sign of a NaN is not printed)
int want_text(uint32_t bits, char* out) {
  if ((bits & 0x7f800000u) == 0x7f800000u && (bits & 0x7fffffu)) { std::memcpy(out, "nan", 4); return 3; }
  float f;
  std::memcpy(&f, &bits, 4);
  return std::snprintf(out, 32, "%.8g", (double)f);
}

struct Mismatch {
  long long count = 0;
  uint32_t bits = 0;
  char got[32] = {0}, want[32] = {0};
};

void check_one(uint32_t bits, Mismatch* M) {
  char guard[PCD_MAX_FIELD_BYTES + 2], want[32];
  std::memset(guard, 0x7f, sizeof(guard));
  const int n = pcd_format_float(bits, guard);
  const int nw = want_text(bits, want);
  const bool ok = n == nw && n <= PCD_MAX_FIELD_BYTES && std::memcmp(guard, want, (size_t)n) == 0 && guard[n] == 0x7f &&
                  pcd_float_length(bits) == n;
  if (ok) return;
  if (M->count++ == 0) {
    M->bits = bits;
    const int c = n < 0 ? 0 : (n > PCD_MAX_FIELD_BYTES ? PCD_MAX_FIELD_BYTES : n);
    std::memcpy(M->got, guard, (size_t)c);
    M->got[c] = 0;
    std::strcpy(M->want, want);
  }
}

void report(const Mismatch& M, uint32_t* first_bad, char* got32, char* want32) {
  if (!M.count) return;
  if (first_bad) *first_bad = M.bits;
  if (got32) std::strcpy(got32, M.got);
  if (want32) std::strcpy(want32, M.want);
}

void check_float(float f, Mismatch* M) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  check_one(b, M);
  check_one(b ^ 0x80000000u, M);
}
}  // namespace

extern "C" {

int emu_pcd_format(uint32_t bits, char* out) { return pcd_format_float(bits, out); }
int emu_pcd_length(uint32_t bits) { return pcd_float_length(bits); }

// every exponent field x both signs x (the four fixed mantissas + n_stride mantissas k * stride mod 2^23); returns the number of
// mismatches against snprintf and describes the first
long long emu_pcd_sweep(uint32_t n_stride, uint32_t stride, uint32_t* first_bad, char* got32, char* want32, long long* n_checked) {
  Mismatch M;
  long long checked = 0;
  const uint32_t fixed[4] = {0u, 1u, 0x400000u, 0x7fffffu};
  for (uint32_t sign = 0; sign < 2; sign++)
    for (uint32_t ex = 0; ex < 256; ex++) {
      const uint32_t hi = (sign << 31) | (ex << 23);
      for (uint32_t m : fixed) { check_one(hi | m, &M); checked++; }
      uint32_t m = stride & 0x7fffffu;
      for (uint32_t k = 0; k < n_stride; k++) {
        check_one(hi | m, &M);
        checked++;
        m = (m + stride) & 0x7fffffu;
      }
    }
  if (n_checked) *n_checked = checked;
  report(M, first_bad, got32, want32);
  return M.count;
}

// exact ties of the 8-digit rounding: j + 0.25 and j + 0.75 for j in [10^6, 10^6 + 4096), j + 0.125 * odd for j in [10^5, 10^5 + 512),
// and their negatives (all exact in fp32)
long long emu_pcd_ties(uint32_t* first_bad, char* got32, char* want32, long long* n_checked) {
  Mismatch M;
  long long checked = 0;
  for (int j = 1000000; j < 1000000 + 4096; j++) {
    check_float((float)j + 0.25f, &M);
    check_float((float)j + 0.75f, &M);
    checked += 4;
  }
  for (int j = 100000; j < 100000 + 512; j++)
    for (int odd = 1; odd < 8; odd += 2) {
      check_float((float)j + 0.125f * (float)odd, &M);
      checked += 2;
    }
  if (n_checked) *n_checked = checked;
  report(M, first_bad, got32, want32);
  return M.count;
}

// a list of bit patterns
long long emu_pcd_check_list(const uint32_t* bits, long long n, uint32_t* first_bad, char* got32, char* want32) {
  Mismatch M;
  for (long long i = 0; i < n; i++) check_one(bits[i], &M);
  report(M, first_bad, got32, want32);
  return M.count;
}

// The body loop of a host ASCII PCD writer as PCL runs it, restated: one ostringstream of precision 8 in the classic locale, one
// operator<< per field, the line trimmed of surrounding blanks, one write per line.  n_fields offsets into records of `step` bytes.
// Returns the bytes written (the header is the caller's), -1 when the file cannot be opened.
long long emu_host_writer_loop(const char* path, const unsigned char* records, long long n, int step, const int* offsets, int n_fields) {
  std::ofstream fs(path, std::ios::binary);
  if (!fs.is_open()) return -1;
  long long bytes = 0;
  std::ostringstream stream;
  stream.precision(8);
  stream.imbue(std::locale::classic());
  for (long long i = 0; i < n; i++) {
    for (int k = 0; k < n_fields; k++) {
      float v;
      std::memcpy(&v, records + i * step + offsets[k], 4);
      stream << v;
      if (k + 1 < n_fields) stream << " ";
    }
    std::string line = stream.str();
    const size_t a = line.find_first_not_of(" \t"), b = line.find_last_not_of(" \t");
    line = a == std::string::npos ? std::string() : line.substr(a, b - a + 1);
    stream.str("");
    fs << line << "\n";
    bytes += (long long)line.size() + 1;
  }
  fs.close();
  return fs.good() ? bytes : -1;
}

}  // extern "C"

#ifdef PCD_HARNESS_MAIN
// stand-alone form (for a sanitizer build on the host): a thinner sweep, the tie set, exit status 1 on any mismatch
int main() {
  uint32_t bad = 0;
  char got[32] = {0}, want[32] = {0};
  long long n1 = 0, n2 = 0;
  const long long m1 = emu_pcd_sweep(1u << 10, 7919u * 1009u, &bad, got, want, &n1);
  const long long m2 = emu_pcd_ties(&bad, got, want, &n2);
  std::printf("checked %lld + %lld values, %lld mismatches\n", n1, n2, m1 + m2);
  if (m1 + m2) std::printf("first: bits 0x%08x got '%s' want '%s'\n", bad, got, want);
  return m1 + m2 ? 1 : 0;
}
#endif
