// TEST AND TOOL INFRASTRUCTURE, never linked into the product: a stand-alone LZF codec for tools/pcd_compressed_timing.py and
// tests/test_pcd_lzf_cpu.py — a greedy encoder (one hash table of the last place three bytes were seen, matches extended as far as
// they go) that writes the token format restated in include/lidarslam_reg.h, and the literal byte-by-byte decoder that is the tool's
// one-thread host baseline.  Written from the format's description; the device path is csrc/pcd_lzf.hip.
//   g++ -O2 -std=c++17 -shared -fPIC tests/cpp/lzf_greedy.cpp -o tests/cpp/_build/liblzf_greedy.so
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

constexpr size_t MAX_LEN = 264, MAX_DIST = 8192;
constexpr int HASH_BITS = 16;

inline uint32_t hash3(const uint8_t* p) {
  const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  return (v * 2654435761u) >> (32 - HASH_BITS);
}

// literal runs of at most 32 bytes for in[a .. b)
inline bool put_literals(const uint8_t* in, size_t a, size_t b, uint8_t* out, size_t cap, size_t* o) {
  while (a < b) {
    const size_t k = b - a < 32 ? b - a : 32;
    if (*o + 1 + k > cap) return false;
    out[(*o)++] = (uint8_t)(k - 1);
    std::memcpy(out + *o, in + a, k);
    *o += k;
    a += k;
  }
  return true;
}

}  // namespace

extern "C" {

// the size of the worst case: everything literal
size_t lzfg_bound(size_t n) { return n + (n + 31) / 32; }

// in[0 .. n) -> an LZF stream in out[0 .. cap); returns its size, or -1 when cap is too small
long long lzfg_compress(const uint8_t* in, size_t n, uint8_t* out, size_t cap) {
  std::vector<int64_t> last((size_t)1 << HASH_BITS, -1);
  size_t i = 0, start = 0, o = 0;
  while (i + 3 <= n) {
    const uint32_t h = hash3(in + i);
    const int64_t p = last[h];
    last[h] = (int64_t)i;
    if (p >= 0 && i - (size_t)p <= MAX_DIST && in[p] == in[i] && in[p + 1] == in[i + 1] && in[p + 2] == in[i + 2]) {
      size_t len = 3;
      while (len < MAX_LEN && i + len < n && in[p + len] == in[i + len]) len++;
      if (!put_literals(in, start, i, out, cap, &o)) return -1;
      const size_t l = len - 2, d = i - (size_t)p - 1;
      if (o + 3 > cap) return -1;
      if (l < 7) {
        out[o++] = (uint8_t)((l << 5) | (d >> 8));
      } else {
        out[o++] = (uint8_t)((7u << 5) | (d >> 8));
        out[o++] = (uint8_t)(l - 7);
      }
      out[o++] = (uint8_t)(d & 255);
      i += len;
      start = i;
    } else {
      i++;
    }
  }
  if (!put_literals(in, start, n, out, cap, &o)) return -1;
  return (long long)o;
}

// The stream in[0 .. n) inflated into out[0 .. n_out), one byte at a time.  Returns n_out, or -1 - (offset of the bad token's control
// byte) for a token that passes the end of the stream, output past n_out or a reference to before the first output byte, or
// -1 - n for a stream that ends short.
long long lzfg_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t n_out) {
  size_t ip = 0, op = 0;
  while (ip < n) {
    const size_t at = ip;
    const unsigned c = in[ip++];
    if (c < 32) {
      const size_t k = c + 1;
      if (ip + k > n || op + k > n_out) return -1 - (long long)at;
      for (size_t j = 0; j < k; j++) out[op++] = in[ip++];
      continue;
    }
    size_t len = c >> 5;
    if (len == 7) {
      if (ip >= n) return -1 - (long long)at;
      len += in[ip++];
    }
    if (ip >= n) return -1 - (long long)at;
    const size_t dist = (((size_t)(c & 31) << 8) | in[ip++]) + 1;
    if (op + len + 2 > n_out || dist > op) return -1 - (long long)at;
    for (size_t j = 0; j < len + 2; j++, op++) out[op] = out[op - dist];
  }
  return op == n_out ? (long long)op : -1 - (long long)n;
}

}  // extern "C"
