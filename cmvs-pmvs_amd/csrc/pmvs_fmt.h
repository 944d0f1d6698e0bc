// pmvs_fmt.h -- the writers' number formatting for host and device from one source: a decimal int32
// and fmt_g, the bytes of printf("%.{precision}g", (double)v) for a float v, which is what
// `ostream << float` emits at that precision (pmvs_write_ply / _patches at 17, _pset at 6).
// No libm, no printf; exact integer arithmetic throughout.
//
// fmt_g on a finite v = m * 2^e (m < 2^24):
//   e <  0   the scaled integer floor(m * 10^s / 2^-e), s = precision - 1 - floor(log10 2^b) for the
//            value's binary exponent b, has precision or precision + 1 digits; m * 5^s (s <= 61, below
//            2^166) lives in six 32-bit limbs and is shifted down by -e - s bits.  The bit below the cut
//            and the OR of the bits below that say how the dropped part compares with one half.
//   e >= 0   m << e (below 2^128) in the same limbs; while it exceeds 64 bits it is divided by 10, every
//            dropped digit folded into the same half / sticky pair.
// Then decimal digits are dropped until `precision` remain, the last step rounds half to even on the
// exact value, a carry to 10^precision moves the exponent, and the digits are laid out as %g does:
// fixed notation when -4 <= X < precision, d.ddde+XX otherwise, trailing zeros and a trailing '.' removed.
// The limbs are indexed by unrolled loops only (registers on the device, never scratch).
// Longest outputs: 23 bytes at precision 17 (-1.4012984643248171e-45), 12 at precision 6; the int32: 11.
#ifndef PMVS_FMT_H
#define PMVS_FMT_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PMVS_FMT_HD __host__ __device__ __forceinline__
#else
#define PMVS_FMT_HD inline
#endif

namespace pmvsfmt {

constexpr int kMaxFloatBytes = 23;  // at precision 17
constexpr int kMaxIntBytes = 11;    // -2147483648
constexpr int kLimbs = 6;

// Decimal int32.  WRITE = false: the length only (out is not touched).
template <bool WRITE>
PMVS_FMT_HD int fmt_i32_t(int32_t v, char* out) {
  const bool neg = v < 0;
  uint32_t u = neg ? 0u - (uint32_t)v : (uint32_t)v;
  int nd = 1;
  for (uint32_t t = u; t >= 10u; t /= 10u) ++nd;
  const int len = nd + (neg ? 1 : 0);
  if (WRITE) {
    if (neg) out[0] = '-';
    for (int i = len - 1; i >= (neg ? 1 : 0); --i) {
      out[i] = (char)('0' + u % 10u);
      u /= 10u;
    }
  }
  return len;
}
PMVS_FMT_HD int fmt_i32(int32_t v, char* out) { return fmt_i32_t<true>(v, out); }
PMVS_FMT_HD int fmt_i32_len(int32_t v) { return fmt_i32_t<false>(v, nullptr); }

// limbs *= c
PMVS_FMT_HD void limbs_mul(uint32_t (&L)[kLimbs], uint32_t c) {
  uint64_t carry = 0;
#pragma unroll
  for (int i = 0; i < kLimbs; ++i) {
    const uint64_t t = (uint64_t)L[i] * c + carry;
    L[i] = (uint32_t)t;
    carry = t >> 32;
  }
}

// limbs /= 10, returns the remainder
PMVS_FMT_HD uint32_t limbs_div10(uint32_t (&L)[kLimbs]) {
  uint32_t rem = 0;
#pragma unroll
  for (int i = kLimbs - 1; i >= 0; --i) {
    const uint64_t cur = ((uint64_t)rem << 32) | L[i];
    const uint64_t q = cur / 10u;
    L[i] = (uint32_t)q;
    rem = (uint32_t)(cur - q * 10u);
  }
  return rem;
}

// Dropping the decimal digit d in front of a tail that is described by (half, sticky): half = the tail
// is at least one half, sticky = it is not exactly 0 (half clear) or exactly one half (half set).
PMVS_FMT_HD void drop_digit(uint32_t d, bool& half, bool& sticky) {
  const bool tail = half || sticky;
  sticky = d == 5u ? tail : (d != 0u || tail);
  half = d >= 5u;
}

template <bool WRITE>
PMVS_FMT_HD int fmt_g_t(float v, int precision, char* out) {
  uint32_t bits;
  memcpy(&bits, &v, 4);
  const bool neg = (bits >> 31) != 0;
  const uint32_t ef = (bits >> 23) & 0xffu, frac = bits & 0x7fffffu;
  int len = 0;
  if (neg) {
    if (WRITE) out[0] = '-';
    len = 1;
  }
  if (ef == 0xffu) {
    if (WRITE) {
      const bool nan = frac != 0;
      out[len] = nan ? 'n' : 'i';
      out[len + 1] = nan ? 'a' : 'n';
      out[len + 2] = nan ? 'n' : 'f';
    }
    return len + 3;
  }
  if (ef == 0 && frac == 0) {
    if (WRITE) out[len] = '0';
    return len + 1;
  }
  const uint32_t m = ef ? (frac | 0x800000u) : frac;
  const int e = (ef ? (int)ef : 1) - 150;  // v = m * 2^e

  // Q * 10^-s with the dropped part in (half, sticky)
  uint64_t Q;
  int s;
  bool half = false, sticky = false;
  uint32_t L[kLimbs] = {m, 0, 0, 0, 0, 0};
  if (e < 0) {
    const int b = e + 31 - __builtin_clz(m);                                // 2^b <= v < 2^(b+1)
    const int x0 = b >= 0 ? (b * 78913) >> 18 : -((-b * 78913) >> 18) - 1;  // floor(log10 2^b), exact for |b| < 1651
    s = precision - 1 - x0;
    if (s < 0) s = 0;
    int left = s;
    for (; left >= 13; left -= 13) limbs_mul(L, 1220703125u);  // 5^13
    uint32_t p5 = 1;
    for (; left > 0; --left) p5 *= 5u;
    limbs_mul(L, p5);
    const int sh = -e - s;  // m * 10^s / 2^-e = (m * 5^s) >> sh
    if (sh <= 0) {
      Q = (((uint64_t)L[1] << 32) | L[0]) << (-sh);
    } else {
      int t = sh - 1;  // keep one bit below the cut
      for (; t >= 32; t -= 32) {
        sticky = sticky || L[0] != 0;
#pragma unroll
        for (int i = 0; i + 1 < kLimbs; ++i) L[i] = L[i + 1];
        L[kLimbs - 1] = 0;
      }
      uint64_t q2 = ((uint64_t)L[1] << 32) | L[0];
      if (t > 0) {
        sticky = sticky || (L[0] & ((1u << t) - 1u)) != 0;
        q2 = (q2 >> t) | ((uint64_t)L[2] << (64 - t));
      }
      half = (q2 & 1u) != 0;
      Q = q2 >> 1;
    }
  } else {
    s = 0;
    int t = e;
    for (; t >= 32; t -= 32) {
#pragma unroll
      for (int i = kLimbs - 1; i > 0; --i) L[i] = L[i - 1];
      L[0] = 0;
    }
    if (t > 0) {
#pragma unroll
      for (int i = kLimbs - 1; i > 0; --i) L[i] = (L[i] << t) | (L[i - 1] >> (32 - t));
      L[0] <<= t;
    }
    while ((L[2] | L[3] | L[4] | L[5]) != 0) {
      drop_digit(limbs_div10(L), half, sticky);
      --s;
    }
    Q = ((uint64_t)L[1] << 32) | L[0];
  }

  // to exactly `precision` digits
  uint64_t top = 1;  // 10^precision
  for (int i = 0; i < precision; ++i) top *= 10u;
  while (Q >= top) {
    const uint64_t q = Q / 10u;
    drop_digit((uint32_t)(Q - q * 10u), half, sticky);
    Q = q;
    --s;
  }
  if (half && (sticky || (Q & 1u))) {
    ++Q;
    if (Q == top) {
      Q = top / 10u;
      --s;
    }
  }
  while (Q < top / 10u) {  // an exact short value
    Q *= 10u;
    ++s;
  }
  const int X = precision - 1 - s;  // decimal exponent of the first digit

  // the digits, least significant first; nd = significant digits without the trailing zeros
  const bool sci = X < -4 || X >= precision;
  // digit i lies at lead + i, one further when i > point (behind the '.'): fixed with X >= 0 has the
  // point behind digit X, scientific behind digit 0, fixed with X < 0 starts with "0." and -X - 1 zeros
  const int lead = (!sci && X < 0) ? -X : 0;
  const int point = sci ? 0 : (X >= 0 ? X : -1);
  uint32_t lo = (uint32_t)(Q % 1000000000u), hi = (uint32_t)(Q / 1000000000u);
  int nd = 0;
  for (int i = precision - 1; i >= 0; --i) {
    uint32_t d;
    if (precision - 1 - i < 9) {
      d = lo % 10u;
      lo /= 10u;
    } else {
      d = hi % 10u;
      hi /= 10u;
    }
    if (nd == 0 && d != 0) nd = i + 1;
    if (WRITE && (nd != 0 || i <= point)) out[len + lead + i + (i > point ? 1 : 0)] = (char)('0' + d);
  }
  if (sci) {
    if (WRITE && nd > 1) out[len + 1] = '.';
    len += nd > 1 ? nd + 1 : 1;
    const int ax = X < 0 ? -X : X;  // at most 45: two digits
    if (WRITE) {
      out[len] = 'e';
      out[len + 1] = X < 0 ? '-' : '+';
      out[len + 2] = (char)('0' + ax / 10);
      out[len + 3] = (char)('0' + ax % 10);
    }
    return len + 4;
  }
  if (X >= 0) {
    if (WRITE && nd > X + 1) out[len + X + 1] = '.';
    return len + (nd > X + 1 ? nd + 1 : X + 1);
  }
  if (WRITE) {
    out[len] = '0';
    out[len + 1] = '.';
    for (int i = 0; i < -X - 1; ++i) out[len + 2 + i] = '0';
  }
  return len + lead + 1 + nd;
}

// The bytes of printf("%.{precision}g", (double)v) at out (no terminator); returns their number.
PMVS_FMT_HD int fmt_g(float v, int precision, char* out) { return fmt_g_t<true>(v, precision, out); }
PMVS_FMT_HD int fmt_g_len(float v, int precision) { return fmt_g_t<false>(v, precision, nullptr); }

}  // namespace pmvsfmt

#endif  // PMVS_FMT_H
