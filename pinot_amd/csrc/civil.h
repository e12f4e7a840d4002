// civil.h -- time transforms of one INT / LONG value (include/pinot_hip.h phip_time_transform): the civil calendar in
// 64-bit integer arithmetic, one function for the device (transform.hip dict_transform_kernel), the library's host
// checks and the stand-alone host test (tests/time_transform/civil_main.cpp), as codec.h is shared with load.hip.
//
//   out = scale(op(scale(v, in_mul, in_div)), out_mul, out_div)
//
// scale(x, m, d) = x * m, or Java's x / d (truncating toward zero; one of m, d is 1): java.util.concurrent.TimeUnit
// .convert without its saturation -- the caller proves with time_transform_fits that no product leaves int64.
// op works on epoch milliseconds (UTC): the identity (CONVERT), Joda's roundFloor to a unit (TRUNC: floors below 1970
// too) or an ISO-chronology field (FIELD). The calendar is the proleptic Gregorian one, from its definition: a cycle
// of 400 years holds 146097 days; counting years from March 1st puts the leap day at the end of its year, so within
// a cycle day-of-cycle -> year-of-cycle needs only the three leap rules (every 4th year = 1460 days, not every
// 100th = 36524 days, the 400th again = 146096 days), and months from March fall on the line (153 m + 2) / 5.
// ISO weeks start on Monday; a week belongs to the year of its Thursday. 1970-01-01 was a Thursday.
#ifndef PINOT_HIP_CIVIL_H_
#define PINOT_HIP_CIVIL_H_

#include <stdint.h>

#include <initializer_list>

#if defined(__HIPCC__) || defined(__HIP__)
#define PHIP_CIVIL_HD __host__ __device__
#else
#define PHIP_CIVIL_HD
#endif

namespace phip {

// phip_time_transform.function / .unit (PHIP_TT_*)
enum { kTtNone = 0, kTtConvert = 1, kTtTrunc = 2, kTtField = 3 };
enum { kTtSecond = 0, kTtMinute, kTtHour, kTtDay, kTtWeek, kTtMonth, kTtQuarter, kTtYear, kTtNumUnits };
enum {
  kTtfYear = 0, kTtfQuarter, kTtfMonth, kTtfWeek, kTtfDayOfYear, kTtfDayOfMonth, kTtfDayOfWeek, kTtfHour, kTtfMinute,
  kTtfSecond, kTtfMillisecond, kTtNumFields
};

struct TimeProgram {
  int32_t function, unit;
  int64_t in_mul, in_div, out_mul, out_div;
};

constexpr int64_t kMsPerDay = 86400000;

PHIP_CIVIL_HD inline int64_t tt_floor_div(int64_t a, int64_t b) {  // b > 0
  const int64_t q = a / b;
  return q - ((a % b) < 0 ? 1 : 0);
}

struct Civil {
  int64_t year;
  int32_t month, day;  // 1-based
};

PHIP_CIVIL_HD inline Civil civil_from_days(int64_t days) {
  const int64_t z = days + 719468;  // days since 0000-03-01
  const int64_t era = tt_floor_div(z, 146097);
  const int64_t doe = z - era * 146097;                                          // [0, 146096]
  const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;    // [0, 399]
  const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);                   // [0, 365], from March 1st
  const int64_t mp = (5 * doy + 2) / 153;                                        // [0, 11], from March
  Civil c;
  c.day = (int32_t)(doy - (153 * mp + 2) / 5 + 1);
  c.month = (int32_t)(mp < 10 ? mp + 3 : mp - 9);
  c.year = yoe + era * 400 + (c.month <= 2 ? 1 : 0);
  return c;
}

PHIP_CIVIL_HD inline int64_t days_from_civil(int64_t year, int32_t month, int32_t day) {
  const int64_t y = year - (month <= 2 ? 1 : 0);
  const int64_t era = tt_floor_div(y, 400);
  const int64_t yoe = y - era * 400;
  const int64_t doy = (153 * (int64_t)(month > 2 ? month - 3 : month + 9) + 2) / 5 + day - 1;
  return era * 146097 + yoe * 365 + yoe / 4 - yoe / 100 + doy - 719468;
}

// 0 = Monday ... 6 = Sunday
PHIP_CIVIL_HD inline int64_t iso_weekday0(int64_t days) { return days + 3 - 7 * tt_floor_div(days + 3, 7); }

PHIP_CIVIL_HD inline int64_t tt_trunc(int64_t ms, int32_t unit) {
  switch (unit) {
    case kTtSecond: return tt_floor_div(ms, 1000) * 1000;
    case kTtMinute: return tt_floor_div(ms, 60000) * 60000;
    case kTtHour: return tt_floor_div(ms, 3600000) * 3600000;
    default: break;
  }
  const int64_t days = tt_floor_div(ms, kMsPerDay);
  if (unit == kTtDay) return days * kMsPerDay;
  if (unit == kTtWeek) return (days - iso_weekday0(days)) * kMsPerDay;
  const Civil c = civil_from_days(days);
  const int32_t month = unit == kTtMonth ? c.month : unit == kTtQuarter ? (c.month - 1) / 3 * 3 + 1 : 1;
  return days_from_civil(c.year, month, 1) * kMsPerDay;
}

PHIP_CIVIL_HD inline int64_t tt_field(int64_t ms, int32_t field) {
  const int64_t days = tt_floor_div(ms, kMsPerDay);
  const int64_t rem = ms % kMsPerDay;  // (not ms - days * kMsPerDay: the product leaves int64 near INT64_MIN)
  const int64_t tod = rem < 0 ? rem + kMsPerDay : rem;
  switch (field) {
    case kTtfHour: return tod / 3600000;
    case kTtfMinute: return tod / 60000 % 60;
    case kTtfSecond: return tod / 1000 % 60;
    case kTtfMillisecond: return tod % 1000;
    case kTtfDayOfWeek: return iso_weekday0(days) + 1;
    case kTtfWeek: {
      const int64_t thursday = days - iso_weekday0(days) + 3;
      const Civil c = civil_from_days(thursday);
      return (thursday - days_from_civil(c.year, 1, 1)) / 7 + 1;
    }
    default: break;
  }
  const Civil c = civil_from_days(days);
  switch (field) {
    case kTtfYear: return c.year;
    case kTtfQuarter: return (c.month - 1) / 3 + 1;
    case kTtfMonth: return c.month;
    case kTtfDayOfMonth: return c.day;
    default: return days - days_from_civil(c.year, 1, 1) + 1;  // kTtfDayOfYear
  }
}

PHIP_CIVIL_HD inline int64_t time_transform(const TimeProgram &p, int64_t v) {
  int64_t x = p.in_div > 1 ? v / p.in_div : v * p.in_mul;
  if (p.function == kTtTrunc) x = tt_trunc(x, p.unit);
  else if (p.function == kTtField) x = tt_field(x, p.unit);
  return p.out_div > 1 ? x / p.out_div : x * p.out_mul;
}

// The program is well formed: a known function and unit, positive scales of which one per pair is 1, and no scale on
// the side of a FIELD or on the output side of a CONVERT.
inline bool time_program_valid(const TimeProgram &p) {
  if (p.in_mul < 1 || p.in_div < 1 || p.out_mul < 1 || p.out_div < 1) return false;
  if ((p.in_mul > 1 && p.in_div > 1) || (p.out_mul > 1 && p.out_div > 1)) return false;
  switch (p.function) {
    case kTtConvert: return p.unit == 0 && p.out_mul == 1 && p.out_div == 1;
    case kTtTrunc: return p.unit >= 0 && p.unit < kTtNumUnits;
    case kTtField: return p.unit >= 0 && p.unit < kTtNumFields && p.in_mul == 1 && p.in_div == 1 && p.out_mul == 1 && p.out_div == 1;
    default: return false;
  }
}

// No product of the program over values in [vmin, vmax] leaves int64 (a roundFloor moves a value down by less than
// 366 days before the output scale multiplies it).
inline bool time_transform_fits(const TimeProgram &p, int64_t vmin, int64_t vmax) {
  const __int128 lim = (__int128)INT64_MAX;
  for (int64_t v : {vmin, vmax}) {
    const __int128 x = (__int128)v * p.in_mul;
    if (x > lim || x < -lim - 1) return false;
    if (p.function == kTtTrunc) {
      const __int128 a = (x < 0 ? -x : x) / p.in_div + (__int128)366 * kMsPerDay;
      if (a * p.out_mul > lim) return false;
    }
  }
  return true;
}

}  // namespace phip

#endif  // PINOT_HIP_CIVIL_H_
