// acc_ops.h -- the accumulator identities and the pairwise combine of the AccKind slots, shared by the kernels (per-wave
// and per-block reductions, finalize_slot) and by the host's reduction of per-block records (host_final.h), which must
// reproduce the device's bits. No HIP dependency: it compiles in a plain C++ unit.
#pragma once
#include <stdint.h>

#include "device.h"

namespace phip {

PHIP_HD inline double acc_f64(uint64_t u) { return __builtin_bit_cast(double, u); }
PHIP_HD inline uint64_t acc_u64(double d) { return __builtin_bit_cast(uint64_t, d); }

#if !defined(__HIP_DEVICE_COMPILE__)
// The host's images of v_add_f64 / v_min_f64 / v_max_f64. The sum is the plain x86 one: an invalid sum (inf + -inf) is
// the negative quiet NaN 0xfff8000000000000 on both (measured: tests/test_gpu_host_final.py's specials case places the
// two infinities in different blocks; its nanmix case lets that NaN meet a stored 0x7ff8... NaN across blocks, again the
// same bits on both. NaNs of other payloads meeting across blocks are not covered). min / max order -0.0 below +0.0
// and return the other operand of a NaN (minNum / maxNum), which libm's fmin / fmax do not promise for the zeros.
inline double acc_host_add(double a, double b) {
#if defined(__clang__)
#pragma clang fp contract(off)  // (one rounding either way; never contracted into a neighbour after inlining)
#endif
  return a + b;
}
inline double acc_host_min(double a, double b) {
  if (a != a) return b;
  if (b != b) return a;
  if (a < b) return a;
  if (b < a) return b;
  return __builtin_signbit(a) ? a : b;  // equal: -0.0 before +0.0
}
inline double acc_host_max(double a, double b) {
  if (a != a) return b;
  if (b != b) return a;
  if (a > b) return a;
  if (b > a) return b;
  return __builtin_signbit(a) ? b : a;
}
#endif

PHIP_HD inline uint64_t acc_init(int kind) {
  if (kind == ACC_MIN_F64) return acc_u64(__builtin_huge_val());
  if (kind == ACC_MAX_F64) return acc_u64(-__builtin_huge_val());
  return 0;  // counts, int sums, f64 +0.0
}

PHIP_HD inline uint64_t acc_combine(int kind, uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (kind == ACC_SUM_F64) return acc_u64(acc_f64(a) + acc_f64(b));
  if (kind == ACC_MIN_F64) return acc_u64(fmin(acc_f64(a), acc_f64(b)));
  if (kind == ACC_MAX_F64) return acc_u64(fmax(acc_f64(a), acc_f64(b)));
#else
  if (kind == ACC_SUM_F64) return acc_u64(acc_host_add(acc_f64(a), acc_f64(b)));
  if (kind == ACC_MIN_F64) return acc_u64(acc_host_min(acc_f64(a), acc_f64(b)));
  if (kind == ACC_MAX_F64) return acc_u64(acc_host_max(acc_f64(a), acc_f64(b)));
#endif
  return a + b;
}

}  // namespace phip
