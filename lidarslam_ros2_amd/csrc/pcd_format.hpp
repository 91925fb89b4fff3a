// One fp32 as text, the way pcl::PCDWriter::writeASCII prints a field at its default precision: operator<<(float) on a classic-locale
// stream of precision 8, i.e. C's "%.8g" of the float promoted to double (restated from knowledge of PCL and of the C
// library: unpinned) — shared by the kernels of csrc/pcd_text.hip and, compiled for the host under LSR_HOST_EMU, by tools/pcd_host_emu
// (tests/test_pcd_ascii_cpu.py).  INTEGER arithmetic only: no floating-point operation decides a digit, so contraction, fast-math and
// the device's rounding cannot matter, and the host build and the device build give the same bytes by construction.
//   value       |v| = m * 2^e exactly, m < 2^24 an integer, e in [-149, 104]
//   digits      the first significant decimal digits of that binary value, exact, with a sticky flag for everything behind them:
//               e in [0, 40]     m << e is one 64-bit integer
//               e in [-60, -1]   integer part m >> -e, fraction digits one at a time: F <- 10 F, digit = F >> -e      (64-bit; every
//                                magnitude a map holds down to 1e-11 comes through these two)
//               e > 40           m << e in four 32-bit words, divided by 10^9 into limbs
//               e < -60          the fraction in six 32-bit words, multiplied by 10^9 per limb of nine digits
//   rounding    to 8 significant digits on the integers: remainder against half the divisor, exact ties to the even digit
//   form        %g: trailing zeros removed and the point with them; d.ddddddde+XX when the decimal exponent is < -4 or >= 8
//   specials    0 / -0, inf / -inf, nan for every NaN whatever its sign
// The longest field is 14 bytes (-1.1754944e-38).
#pragma once
#ifndef LSR_HOST_EMU
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

namespace lsr {

constexpr int PCD_MAX_FIELD_BYTES = 14;

// what is left of a float once its digits are known: everything the length and the bytes depend on
struct PcdField {
  uint32_t q;      // the significant digits without trailing zeros (1 .. 99999999); specials: unused
  int16_t x10;     // decimal exponent of the first digit
  uint8_t ndig;    // number of digits in q (1 .. 8)
  uint8_t kind;    // bit 0: negative sign printed; bits 1-2: 0 finite non-zero, 1 zero, 2 inf, 3 nan
};

__host__ __device__ inline int pcd_count_digits_u64(uint64_t v) {
  int n = 1;
  uint64_t p = 10;
  while (n < 20 && v >= p) { p *= 10; n++; }
  return n;
}

__host__ __device__ inline uint64_t pcd_pow10_u64(int k) {   // k in [0, 19]
  uint64_t p = 1;
  for (int i = 0; i < k; i++) p *= 10;
  return p;
}

// acc holds the first nd significant digits (nd >= 1, acc < 2^64), sticky whether anything non-zero follows them; x10 the decimal
// exponent of acc's first digit.  Leaves the 8-digit rounding in F (trailing zeros removed).
__host__ __device__ inline void pcd_round8(uint64_t acc, int nd, bool sticky, int x10, PcdField* F) {
  uint64_t q;
  if (nd <= 8) {
    q = acc * pcd_pow10_u64(8 - nd);   // exact: nothing follows fewer than nine digits (the generators stop early only at a zero remainder)
  } else {
    const uint64_t div = pcd_pow10_u64(nd - 8), half = div / 2;
    q = acc / div;
    const uint64_t r = acc - q * div;
    if (r > half || (r == half && (sticky || (q & 1)))) q++;
    if (q == 100000000ull) { q = 10000000ull; x10++; }
  }
  uint32_t d = (uint32_t)q;
  int ndig = 8;
  while (d % 10u == 0) { d /= 10u; ndig--; }
  F->q = d;
  F->ndig = (uint8_t)ndig;
  F->x10 = (int16_t)x10;
}

__host__ __device__ inline PcdField pcd_decompose(uint32_t bits) {
  PcdField F;
  F.q = 0; F.x10 = 0; F.ndig = 1;
  const uint32_t neg = bits >> 31, ex = (bits >> 23) & 0xffu, man = bits & 0x7fffffu;
  if (ex == 0xffu) {
    F.kind = man ? (uint8_t)(3u << 1) : (uint8_t)((2u << 1) | neg);
    return F;
  }
  if (ex == 0 && man == 0) {
    F.kind = (uint8_t)((1u << 1) | neg);
    return F;
  }
  F.kind = (uint8_t)neg;
  const uint32_t m = ex ? (man | 0x800000u) : man;
  const int e = ex ? (int)ex - 150 : -149;
  if (e >= 0 && e <= 40) {
    const uint64_t N = (uint64_t)m << e;
    const int nd = pcd_count_digits_u64(N);
    pcd_round8(N, nd, false, nd - 1, &F);
  } else if (e < 0 && e >= -60) {
    const int f = -e;
    const uint64_t mask = ((uint64_t)1 << f) - 1;
    uint64_t acc = (uint64_t)m >> f, frac = (uint64_t)m & mask;   // f <= 60: the shift is defined, frac < 2^60 and 10 frac < 2^64
    int nd = acc ? pcd_count_digits_u64(acc) : 0;
    int x10 = nd - 1, lead = 0;
    while (nd < 9 && frac) {
      frac *= 10;
      const uint32_t dgt = (uint32_t)(frac >> f);
      frac &= mask;
      if (acc == 0 && dgt == 0) { lead++; continue; }
      if (acc == 0) x10 = -(lead + 1);
      acc = acc * 10 + dgt;
      nd++;
    }
    pcd_round8(acc, nd, frac != 0, x10, &F);
  } else if (e > 40) {
    // m << e below 2^128 in four words; limbs of nine decimal digits, least significant first (39 digits at most: five limbs)
    uint32_t w[4] = {0, 0, 0, 0};
    {
      const int s = e >> 5, b = e & 31;
      const uint64_t v = (uint64_t)m << b;
      for (int i = 0; i < 4; i++) {
        if (i == s) w[i] = (uint32_t)v;
        if (i == s + 1) w[i] = (uint32_t)(v >> 32);
      }
    }
    uint32_t limb[5] = {0, 0, 0, 0, 0};
    int nl = 0;
    for (int it = 0; it < 5; it++) {
      if ((w[0] | w[1] | w[2] | w[3]) == 0) break;
      uint64_t rem = 0;
      for (int i = 3; i >= 0; i--) {
        const uint64_t cur = (rem << 32) | w[i];
        w[i] = (uint32_t)(cur / 1000000000u);
        rem = cur % 1000000000u;
      }
      limb[it] = (uint32_t)rem;
      nl = it + 1;
    }
    // the two leading limbs carry 10 .. 18 digits (2^41 > 10^9: there are at least two); the rest only says whether it is zero
    uint32_t top = 0, next = 0;
    bool sticky = false;
    for (int i = 0; i < 5; i++) {
      if (i == nl - 1) top = limb[i];
      else if (i == nl - 2) next = limb[i];
      else if (i < nl - 2 && limb[i]) sticky = true;
    }
    const int dt = pcd_count_digits_u64(top);
    pcd_round8((uint64_t)top * 1000000000u + next, dt + 9, sticky, dt + 9 * (nl - 1) - 1, &F);
  } else {
    // e < -60: the value is a pure fraction m / 2^f, f in [61, 149]; frac < 2^f, 10^9 frac < 2^(f + 30) <= 2^179: six words
    const int f = -e, s = f >> 5, b = f & 31;
    uint32_t w[6] = {m, 0, 0, 0, 0, 0};
    uint64_t acc = 0;
    int nd = 0, lead = 0, x10 = 0, taken = 0;
    // at most 44 zeros lead (2^-149 = 1.4e-45): five empty limbs, then the two that are kept
    for (int it = 0; it < 8 && taken < 2; it++) {
      uint64_t carry = 0;
      for (int i = 0; i < 6; i++) {
        const uint64_t cur = (uint64_t)w[i] * 1000000000u + carry;
        w[i] = (uint32_t)cur;
        carry = cur >> 32;
      }
      // the limb: bits f .. f + 29 (s + 1 <= 5)
      uint32_t lo = 0, hi = 0;
      for (int i = 0; i < 6; i++) {
        if (i == s) lo = w[i];
        if (i == s + 1) hi = w[i];
      }
      const uint32_t l = (uint32_t)((((uint64_t)hi << 32) | lo) >> b);
      for (int i = 0; i < 6; i++) {
        if (i == s) w[i] &= (b ? ((1u << b) - 1u) : 0u);
        if (i > s) w[i] = 0;
      }
      if (taken == 0) {
        if (l == 0) { lead += 9; continue; }
        acc = l;
        nd = pcd_count_digits_u64(l);
        x10 = -(lead + (9 - nd) + 1);
        taken = 1;
      } else {
        acc = acc * 1000000000u + l;
        nd += 9;
        taken = 2;
      }
    }
    const bool sticky = (w[0] | w[1] | w[2] | w[3] | w[4] | w[5]) != 0;
    pcd_round8(acc, nd, sticky, x10, &F);
  }
  return F;
}

__host__ __device__ inline int pcd_field_length(const PcdField& F) {
  const int neg = F.kind & 1, cls = F.kind >> 1;
  if (cls == 1) return 1 + neg;
  if (cls == 2) return 3 + neg;
  if (cls == 3) return 3;
  const int x = F.x10, nd = F.ndig;
  if (x < -4 || x >= 8) return neg + nd + (nd > 1 ? 1 : 0) + 4;   // d[.ddd]e+XX: |x| <= 45, two exponent digits
  if (x >= 0) return neg + (nd <= x + 1 ? x + 1 : nd + 1);
  return neg + 2 + (-x - 1) + nd;                                   // 0.[zeros]ddd
}

// writes the text of F at out (no terminator) and returns its length, pcd_field_length(F)
__host__ __device__ inline int pcd_field_emit(const PcdField& F, char* out) {
  const int neg = F.kind & 1, cls = F.kind >> 1;
  int n = 0;
  if (cls == 3) { out[0] = 'n'; out[1] = 'a'; out[2] = 'n'; return 3; }
  if (neg) out[n++] = '-';
  if (cls == 1) { out[n++] = '0'; return n; }
  if (cls == 2) { out[n++] = 'i'; out[n++] = 'n'; out[n++] = 'f'; return n; }
  const int x = F.x10, nd = F.ndig;
  // digit i of q, most significant first, is written at out[n + pos(i)]: peel them off the low end
  uint32_t q = F.q;
  if (x < -4 || x >= 8) {
    for (int i = nd - 1; i >= 0; i--) {
      out[n + (i == 0 ? 0 : i + 1)] = (char)('0' + q % 10u);
      q /= 10u;
    }
    if (nd > 1) out[n + 1] = '.';
    n += nd + (nd > 1 ? 1 : 0);
    const int ax = x < 0 ? -x : x;
    out[n++] = 'e';
    out[n++] = x < 0 ? '-' : '+';
    out[n++] = (char)('0' + ax / 10);
    out[n++] = (char)('0' + ax % 10);
    return n;
  }
  if (x >= 0) {
    const int ni = x + 1;   // digits before the point
    if (nd <= ni) {
      for (int i = ni - 1; i >= nd; i--) out[n + i] = '0';
      for (int i = nd - 1; i >= 0; i--) { out[n + i] = (char)('0' + q % 10u); q /= 10u; }
      return n + ni;
    }
    for (int i = nd - 1; i >= 0; i--) {
      out[n + (i < ni ? i : i + 1)] = (char)('0' + q % 10u);
      q /= 10u;
    }
    out[n + ni] = '.';
    return n + nd + 1;
  }
  const int nz = -x - 1;
  out[n++] = '0';
  out[n++] = '.';
  for (int i = 0; i < nz; i++) out[n++] = '0';
  for (int i = nd - 1; i >= 0; i--) { out[n + i] = (char)('0' + q % 10u); q /= 10u; }
  return n + nd;
}

// the text of the float with these bits at out (at most PCD_MAX_FIELD_BYTES bytes, no terminator); returns its length
__host__ __device__ inline int pcd_format_float(uint32_t bits, char* out) {
  const PcdField F = pcd_decompose(bits);
  return pcd_field_emit(F, out);
}

__host__ __device__ inline int pcd_float_length(uint32_t bits) {
  const PcdField F = pcd_decompose(bits);
  return pcd_field_length(F);
}

}  // namespace lsr
