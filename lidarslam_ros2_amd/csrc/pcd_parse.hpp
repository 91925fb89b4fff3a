// The counterpart of csrc/pcd_format.hpp: text -> fp32 and the line structure of an ASCII .pcd body, shared by the kernels of
// csrc/pcd_read.hip and, compiled for the host under LSR_HOST_EMU, by tools/pcd_read_host_emu (tests/test_pcd_read_cpu.py).  INTEGER
// arithmetic only: no floating-point operation decides a bit, so the host build and the device build agree by construction.
//   token       the decimal subset of what strtof accepts in the C locale, the WHOLE token:
//                 [+-]? (digits [. digits?] | . digits) ([eE] [+-]? digits)?     |     [+-]? (inf | infinity | nan), any letter case
//               everything else is refused (hex floats, nan(...), trailing characters, a comma, an empty exponent)
//   decimal     the first 19 significant digits as a 64-bit integer w, a decimal exponent q, and whether a non-zero digit was dropped
//               behind them; first digit at or above 10^39: inf, below 10^-46: zero (half the smallest denormal is 7.006e-46)
//   value       w * 10^q = w * 5^q * 2^q exactly, in eight 32-bit words: q >= 0 a product by 5^q (13 factors per 32-bit multiplier);
//               q < 0 the quotient of w << S by 5^-q (short divisions by 5^13, the remainders only say whether they are zero), S chosen
//               so that the quotient keeps at least 26 bits
//   rounding    24 bits (fewer in the denormal range: the last kept bit is 2^-149), a round bit, a sticky bit; nearest, ties to even —
//               glibc's strtof in the default rounding mode; overflow to inf, gradual underflow to 0, the sign of -0 kept
//   dropped     with digits dropped the value lies strictly between w and w + 1 (times 10^q): both ends are rounded, towards the
//               inside; if they agree that is the answer, otherwise the token is left UNRESOLVED — never guessed — and the host entry
//               asks the C library.  A token of at most 19 significant digits (so every "%.9g" or shorter text) drops nothing.
//   nan         nan, +nan -> 0x7fc00000, -nan -> 0xffc00000
// Line structure: a two-state machine over the body's bytes — 0 "only blanks since the last newline", 1 "inside a line" — whose
// transition over a run of bytes is a function on two states (2 bits) with, per entry state, the number of point lines starting in the
// run (a point line starts at its first byte that is neither blank nor newline).  Runs compose, so the body is cut among threads.
#pragma once
#ifndef LSR_HOST_EMU
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>
#include <stdint.h>

#ifdef LSR_HOST_EMU
#define PCD_UNROLL
#else
#define PCD_UNROLL _Pragma("unroll")
#endif

namespace lsr {

enum PcdTokenStatus : int { PCD_TOK_OK = 0, PCD_TOK_BAD = 1, PCD_TOK_UNRESOLVED = 2 };

struct PcdDecimal {
  uint64_t w;       // the first (at most 19) significant digits
  int q;            // value = w * 10^q (+ what was dropped)
  uint8_t neg;
  uint8_t kind;     // 0 number, 1 inf, 2 nan
  uint8_t dropped;  // a non-zero digit followed the 19 kept
};

__host__ __device__ inline bool pcd_is_blank(unsigned char c) { return c == ' ' || c == '\t' || c == '\r'; }
__host__ __device__ inline bool pcd_is_digit(unsigned char c) { return c >= '0' && c <= '9'; }

// s[0 .. n) against the lower-case word `word` of n letters, any letter case
__host__ __device__ inline bool pcd_word_is(const unsigned char* s, int n, const char* word, int word_len) {
  if (n != word_len) return false;
  for (int i = 0; i < n; i++)
    if ((s[i] | 0x20) != (unsigned char)word[i]) return false;
  return true;
}

// the grammar: false = not a number of the accepted subset
__host__ __device__ inline bool pcd_scan_token(const unsigned char* s, int n, PcdDecimal* D) {
  D->w = 0; D->q = 0; D->neg = 0; D->kind = 0; D->dropped = 0;
  int i = 0;
  if (n <= 0) return false;
  if (s[0] == '+' || s[0] == '-') { D->neg = s[0] == '-'; i = 1; }
  if (i >= n) return false;
  if (!pcd_is_digit(s[i]) && s[i] != '.') {
    if (pcd_word_is(s + i, n - i, "inf", 3) || pcd_word_is(s + i, n - i, "infinity", 8)) { D->kind = 1; return true; }
    if (pcd_word_is(s + i, n - i, "nan", 3)) { D->kind = 2; return true; }
    return false;
  }
  uint64_t w = 0;
  int nd = 0, q = 0;
  bool any = false, dropped = false;
  for (; i < n && pcd_is_digit(s[i]); i++) {
    const unsigned d = s[i] - '0';
    any = true;
    if (nd == 0 && d == 0) continue;   // leading zeros
    if (nd < 19) { w = w * 10 + d; nd++; } else { q++; dropped |= d != 0; }
  }
  if (i < n && s[i] == '.') {
    for (i++; i < n && pcd_is_digit(s[i]); i++) {
      const unsigned d = s[i] - '0';
      any = true;
      if (nd == 0 && d == 0) { q--; continue; }
      if (nd < 19) { w = w * 10 + d; nd++; q--; } else { dropped |= d != 0; }
    }
  }
  if (!any) return false;
  if (i < n && (s[i] | 0x20) == 'e') {
    i++;
    bool eneg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) { eneg = s[i] == '-'; i++; }
    if (i >= n || !pcd_is_digit(s[i])) return false;
    int e = 0;
    for (; i < n && pcd_is_digit(s[i]); i++)
      if (e < 100000) e = e * 10 + (s[i] - '0');
    q += eneg ? -e : e;
  }
  if (i != n) return false;
  D->w = w; D->q = q; D->dropped = dropped;
  return true;
}

constexpr int PCD_BIG_WORDS = 8;

__host__ __device__ inline void pcd_big_mul(uint32_t* W, uint32_t m) {
  uint64_t carry = 0;
PCD_UNROLL
  for (int i = 0; i < PCD_BIG_WORDS; i++) {
    const uint64_t cur = (uint64_t)W[i] * m + carry;
    W[i] = (uint32_t)cur;
    carry = cur >> 32;
  }
}

__host__ __device__ inline uint32_t pcd_big_div(uint32_t* W, uint32_t d) {
  uint64_t rem = 0;
PCD_UNROLL
  for (int i = PCD_BIG_WORDS - 1; i >= 0; i--) {
    const uint64_t cur = (rem << 32) | W[i];
    W[i] = (uint32_t)(cur / d);
    rem = cur % d;
  }
  return (uint32_t)rem;
}

__host__ __device__ inline uint32_t pcd_pow5_u32(int k) {   // k in [0, 13]
  uint32_t p = 1;
  for (int i = 0; i < k; i++) p *= 5u;
  return p;
}

// The fp32 (sign bit clear) nearest w * 10^q moved by `nudge` times an amount smaller than anything representable: 0 the value itself,
// +1 just above it, -1 just below it.  w >= 1, q in [-65, 38].
__host__ __device__ inline uint32_t pcd_round_decimal(uint64_t w, int q, int nudge) {
  uint32_t W[PCD_BIG_WORDS];
  bool rest = false;   // something non-zero lies below the integer in W
  int E;               // value = (W + rest) * 2^E
  if (q >= 0) {
    W[0] = (uint32_t)w; W[1] = (uint32_t)(w >> 32);
PCD_UNROLL
    for (int i = 2; i < PCD_BIG_WORDS; i++) W[i] = 0;
    int k = q;
    for (; k >= 13; k -= 13) pcd_big_mul(W, 1220703125u);   // 5^13
    if (k) pcd_big_mul(W, pcd_pow5_u32(k));
    E = q;                                                  // w * 5^38 < 2^153
  } else {
    int k = -q;
    const int S = (7 * k + 2) / 3 + 26;                     // 2^S >= 5^k * 2^26; S <= 178, w << S below 2^242
    const int s = S >> 5, b = S & 31;
    const uint64_t lo = w << b;
    const uint32_t p0 = (uint32_t)lo, p1 = (uint32_t)(lo >> 32), p2 = b ? (uint32_t)(w >> (64 - b)) : 0u;
PCD_UNROLL
    for (int i = 0; i < PCD_BIG_WORDS; i++) W[i] = i == s ? p0 : (i == s + 1 ? p1 : (i == s + 2 ? p2 : 0u));
    E = q - S;
    for (; k >= 13; k -= 13) rest |= pcd_big_div(W, 1220703125u) != 0;
    if (k) rest |= pcd_big_div(W, pcd_pow5_u32(k)) != 0;
  }
  if (nudge > 0) rest = true;
  if (nudge < 0 && !rest) {   // W - 1 and something above it (W >= 2: a product of w + 1 >= 2, or a quotient of at least 26 bits)
    bool borrow = true;
PCD_UNROLL
    for (int i = 0; i < PCD_BIG_WORDS; i++) {
      const uint32_t v = W[i];
      W[i] = borrow ? v - 1u : v;
      borrow = borrow && v == 0u;
    }
    rest = true;
  }
  int top = 0;
  uint32_t top_word = W[0];
PCD_UNROLL
  for (int i = 1; i < PCD_BIG_WORDS; i++)
    if (W[i]) { top = i; top_word = W[i]; }
  if (top_word == 0) return 0u;   // (not reached: w >= 1 gives W >= 1, and only w + 1 >= 2 is ever nudged down)
  const int L = 32 * top + (32 - __builtin_clz(top_word));
  int e2 = L - 1 + E;                                   // 2^e2 <= value < 2^(e2 + 1)
  const bool normal = e2 >= -126;
  const int p = normal ? 24 : e2 + 150;                 // bits kept
  if (p < 0) return 0u;                                 // below 2^-150: nearer to zero than to the smallest denormal
  const int shift = L - p;
  uint32_t mant;
  bool rnd = false, sticky = rest;
  if (shift <= 0) {
    mant = W[0] << -shift;                              // L <= 24: the integer is W[0], exact (a quotient always has shift >= 2)
  } else {
    const int at = shift - 1, wi = at >> 5, bo = at & 31;
    uint32_t a = 0, b1 = 0, c = 0;
    bool low = false;
PCD_UNROLL
    for (int i = 0; i < PCD_BIG_WORDS; i++) {
      if (i == wi) a = W[i];
      if (i == wi + 1) b1 = W[i];
      if (i == wi + 2) c = W[i];
      if (i < wi && W[i]) low = true;
    }
    const uint64_t lo64 = ((uint64_t)b1 << 32) | a;
    const uint64_t win = (lo64 >> bo) | (bo ? ((uint64_t)c << (64 - bo)) : 0ull);
    rnd = (win & 1ull) != 0;
    mant = (uint32_t)(win >> 1) & ((p >= 24) ? 0xffffffu : ((1u << p) - 1u));
    sticky = sticky || low || (bo && (a & ((1u << bo) - 1u)) != 0);
  }
  if (rnd && (sticky || (mant & 1u))) mant++;
  if (!normal) return mant;                             // mant <= 2^23: the largest denormal rounds up into the smallest normal
  if (mant == (1u << 24)) { mant >>= 1; e2++; }
  const int ef = e2 + 127;
  if (ef >= 255) return 0x7f800000u;
  return ((uint32_t)ef << 23) | (mant & 0x7fffffu);
}

__host__ __device__ inline int pcd_decimal_digits(uint64_t v) {
  int n = 1;
  uint64_t p = 10;
  while (n < 20 && v >= p) { p *= 10; n++; }
  return n;
}

// the bits of a scanned token; PCD_TOK_UNRESOLVED leaves *bits alone
__host__ __device__ inline int pcd_decimal_to_bits(const PcdDecimal& D, uint32_t* bits) {
  const uint32_t sign = (uint32_t)D.neg << 31;
  if (D.kind == 1) { *bits = sign | 0x7f800000u; return PCD_TOK_OK; }
  if (D.kind == 2) { *bits = sign | 0x7fc00000u; return PCD_TOK_OK; }
  if (D.w == 0) { *bits = sign; return PCD_TOK_OK; }   // nothing can follow a zero w: leading zeros are not kept
  // the first digit's decimal place; q beyond +-2000 cannot come back into range (w has at most 19 digits)
  const int q = D.q > 2000 ? 2000 : (D.q < -2000 ? -2000 : D.q);
  const int d = pcd_decimal_digits(D.w) + q;            // 10^(d - 1) <= value < 10^d
  if (d > 39) { *bits = sign | 0x7f800000u; return PCD_TOK_OK; }
  if (d < -46) { *bits = sign; return PCD_TOK_OK; }
  if (!D.dropped) { *bits = sign | pcd_round_decimal(D.w, q, 0); return PCD_TOK_OK; }
  const uint32_t lo = pcd_round_decimal(D.w, q, +1), hi = pcd_round_decimal(D.w + 1, q, -1);
  if (lo != hi) return PCD_TOK_UNRESOLVED;
  *bits = sign | lo;
  return PCD_TOK_OK;
}

__host__ __device__ inline int pcd_parse_float(const unsigned char* s, int n, uint32_t* bits) {
  PcdDecimal D;
  if (!pcd_scan_token(s, n, &D)) return PCD_TOK_BAD;
  return pcd_decimal_to_bits(D, bits);
}

// ---- the line machine ---------------------------------------------------------------------------------------------------------------
// What a run of bytes does: f bit s = the state behind the run when it is entered in state s; c[s] = point lines starting inside it.
struct PcdRun {
  uint32_t f, c0, c1;
};

__host__ __device__ inline PcdRun pcd_run_identity() { return PcdRun{2u, 0u, 0u}; }

// a, then b
__host__ __device__ inline PcdRun pcd_run_compose(const PcdRun& a, const PcdRun& b) {
  const uint32_t s0 = a.f & 1u, s1 = (a.f >> 1) & 1u;
  PcdRun r;
  r.f = ((b.f >> s0) & 1u) | (((b.f >> s1) & 1u) << 1);
  r.c0 = a.c0 + (s0 ? b.c1 : b.c0);
  r.c1 = a.c1 + (s1 ? b.c1 : b.c0);
  return r;
}

struct alignas(16) PcdChunk16 {
  uint32_t w[4];
};

// fn(byte, index) for every byte of text[a .. b) in order: single bytes up to a 16-byte boundary of the address, 16-byte loads, single
// bytes behind the last whole one.  Nothing outside [a, b) is read.
template <typename Fn>
__host__ __device__ inline void pcd_for_bytes(const unsigned char* text, size_t a, size_t b, Fn&& fn) {
  size_t i = a;
  for (; i < b && ((uintptr_t)(text + i) & 15u); i++) fn(text[i], i);
  for (; i + 16 <= b; i += 16) {
    const PcdChunk16 v = *reinterpret_cast<const PcdChunk16*>(text + i);
PCD_UNROLL
    for (int k = 0; k < 16; k++) fn((unsigned char)(v.w[k >> 2] >> (8 * (k & 3))), i + k);
  }
  for (; i < b; i++) fn(text[i], i);
}

// the run text[a .. b), both entry states walked side by side
__host__ __device__ inline PcdRun pcd_run_of(const unsigned char* text, size_t a, size_t b) {
  uint32_t s0 = 0, s1 = 1, c0 = 0, c1 = 0;
  pcd_for_bytes(text, a, b, [&](unsigned char c, size_t) {
    if (c == '\n') { s0 = 0; s1 = 0; }
    else if (!pcd_is_blank(c)) { c0 += s0 ^ 1u; c1 += s1 ^ 1u; s0 = 1; s1 = 1; }
  });
  return PcdRun{s0 | (s1 << 1), c0, c1};
}

// the same run entered in `state`: emit(index) at the first byte of every point line; returns the state behind the run
template <typename Emit>
__host__ __device__ inline uint32_t pcd_run_index(const unsigned char* text, size_t a, size_t b, uint32_t state, Emit&& emit) {
  pcd_for_bytes(text, a, b, [&](unsigned char c, size_t i) {
    if (c == '\n') state = 0;
    else if (!pcd_is_blank(c)) {
      if (!state) emit(i);
      state = 1;
    }
  });
  return state;
}

// Thread g's share of a text of n bytes cut into runs of `run` bytes counted from the 16-byte boundary at or below its first byte (so
// that with run a multiple of 16 every whole load of a run is aligned): [*a, *b), empty behind the end.
__host__ __device__ inline void pcd_run_bounds(const unsigned char* text, size_t n, size_t run, size_t g, size_t* a, size_t* b) {
  const size_t lead = (size_t)((uintptr_t)text & 15u);
  const size_t lo = g * run, hi = lo + run;   // positions counted from the boundary
  size_t x = lo > lead ? lo - lead : 0, y = hi > lead ? hi - lead : 0;
  if (x > n) x = n;
  if (y > n) y = n;
  *a = x;
  *b = y;
}

__host__ __device__ inline size_t pcd_run_count(const unsigned char* text, size_t n, size_t run) {
  return (n + (size_t)((uintptr_t)text & 15u) + run - 1) / run;
}

}  // namespace lsr
