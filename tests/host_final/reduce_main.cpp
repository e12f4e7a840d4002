// Stand-alone check of the record mode's host side (pinot_amd/csrc/host_final.h), built by
// tests/test_host_final_reduce.py with -fsanitize=address,undefined and run as a fresh process.
//
//   reduce_main reduce           feeds the reducer record sets and checks accept / not-yet and the totals; prints
//                                "REDUCE OK" or the first difference and exits 1
//   reduce_main table L1,L2,...  prints the wave ranges and the block table for total_work 0..200, a few grids and both
//                                walks; the work-list entries are L1, L2, ... tiles long, cyclically (the test compares
//                                with its own brute force)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../pinot_amd/csrc/host_final.h"

using namespace phip;

static int g_fail = 0;
#define CHECK(c, ...)                    \
  do {                                   \
    if (!(c)) {                          \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);               \
      printf("\n");                      \
      g_fail++;                          \
    }                                    \
  } while (0)

static double f64(uint64_t u) { double d; memcpy(&d, &u, 8); return d; }
static uint64_t u64(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }

// A straight restatement of the device's order (aggregate.hip finalize_slot + dev_common.h wave_reduce_f64): 64 lanes,
// lane l combines blocks l, l + 64, ... from the identity, then every lane takes lane ^ offset as its second operand
// for offsets 32 .. 1, all lanes at once; lane 0 holds the result. Plain C arithmetic with IEEE minNum / maxNum.
static double op(int kind, double a, double b) {
  if (kind == ACC_SUM_F64) return a + b;
  if (a != a) return b;
  if (b != b) return a;
  if (a == b) return (kind == ACC_MIN_F64) == (bool)std::signbit(a) ? a : b;
  return kind == ACC_MIN_F64 ? (a < b ? a : b) : (a > b ? a : b);
}
static double restated(int kind, const std::vector<double> &v) {
  double lane[64], next[64];
  for (int l = 0; l < 64; l++) {
    lane[l] = kind == ACC_SUM_F64 ? 0.0 : (kind == ACC_MIN_F64 ? HUGE_VAL : -HUGE_VAL);
    for (size_t b = l; b < v.size(); b += 64) lane[l] = op(kind, lane[l], v[b]);
  }
  for (int o = 32; o > 0; o >>= 1) {
    for (int l = 0; l < 64; l++) next[l] = op(kind, lane[l], lane[l ^ o]);
    memcpy(lane, next, sizeof(lane));
  }
  return lane[0];
}
static bool same(double a, double b) { return u64(a) == u64(b); }  // bit for bit, NaN included

struct Set {
  RecPlan p;
  std::vector<int32_t> kinds, first, k, slot;
  std::vector<uint64_t> area;
  std::vector<std::vector<uint64_t>> acc;  // [a][block]
  std::vector<uint64_t> matched, scanned;
  std::vector<std::vector<uint64_t>> seg;  // [block][j]
};

static void write_block(Set &s, int b, uint32_t tag) {
  uint64_t *r = s.area.data() + (size_t)b * s.p.stride_words;
  r[0] = rec_word(tag, s.matched[b]);
  r[1] = rec_word(tag, s.scanned[b]);
  for (int a = 0; a < s.p.na; a++) {
    r[2 + 2 * a] = rec_word(tag, s.acc[a][b]);
    r[3 + 2 * a] = rec_word(tag, s.acc[a][b] >> 48);
  }
  for (int j = 0; j < s.k[b]; j++) r[2 + 2 * s.p.na + j] = rec_word(tag, s.seg[b][j]);
}

static Set make_set(int nblocks, std::vector<int32_t> kinds, int kmax, bool limit_k, std::mt19937_64 &rng) {
  Set s;
  s.kinds = kinds;
  const int na = (int)kinds.size();
  s.first.resize(nblocks);
  s.k.resize(nblocks);
  int e = 0;
  for (int b = 0; b < nblocks; b++) {  // neighbouring blocks share their boundary entry, some blocks touch none
    s.k[b] = limit_k ? kmax : (int)(rng() % (kmax + 1));
    s.first[b] = e;
    if (s.k[b] > 0) e += s.k[b] - 1;
  }
  s.slot.resize(e + 1);
  for (int i = 0; i <= e; i++) s.slot[i] = (i * 7) % (e + 1);  // (a permutation when gcd(7, e + 1) == 1; sums either way)
  int maxw = 0;
  for (int b = 0; b < nblocks; b++) maxw = std::max(maxw, rec_num_words(na, s.k[b]));
  CHECK(maxw <= kRecMaxWords, "test set too wide: %d words", maxw);
  s.p.nblocks = nblocks;
  s.p.na = na;
  s.p.stride_words = maxw <= 8 ? 8 : 16;
  s.area.assign((size_t)nblocks * s.p.stride_words, 0);
  s.acc.assign(na, std::vector<uint64_t>(nblocks));
  s.matched.resize(nblocks);
  s.scanned.resize(nblocks);
  s.seg.resize(nblocks);
  const double specials[] = {NAN, -0.0, 0.0, HUGE_VAL, -HUGE_VAL, 1e308, -1e308, 4.9e-324};
  for (int b = 0; b < nblocks; b++) {
    s.matched[b] = rng() & kRecFieldMask;
    s.scanned[b] = rng() % 1000003;
    for (int a = 0; a < na; a++) {
      if (kinds[a] == ACC_COUNT || kinds[a] == ACC_SUM_I64) {
        s.acc[a][b] = rng();  // (every bit of the two words in use, the sum wraps)
      } else {
        const uint64_t r = rng();
        double d = (double)(int64_t)(r >> 20) * 1e-3 - 1e9;
        if (r % 5 == 0) d = specials[(r >> 8) % 8];
        s.acc[a][b] = u64(d);
      }
    }
    s.seg[b].resize(s.k[b]);
    for (int j = 0; j < s.k[b]; j++) s.seg[b][j] = rng() % 2049;
  }
  return s;
}

static void bind(Set &s) {
  s.p.kinds = s.kinds.data();
  s.p.first = s.first.data();
  s.p.k = s.k.data();
  s.p.entry_slot = s.slot.data();
}

static void check_set(int nblocks, std::vector<int32_t> kinds, int kmax, bool limit_k, uint64_t seed) {
  std::mt19937_64 rng(seed);
  Set s = make_set(nblocks, kinds, kmax, limit_k, rng);
  bind(s);
  const uint32_t T = 40000 + (uint32_t)(seed % 100), Tp = T - 1;
  const int na = s.p.na;
  int cur = 0;
  CHECK(nblocks == 0 || !rec_accept(s.p, s.area.data(), T, &cur), "a zero-filled area was accepted");
  for (int b = 0; b < nblocks; b++) write_block(s, b, Tp);  // the previous execution's records
  cur = 0;
  CHECK(nblocks == 0 || (!rec_accept(s.p, s.area.data(), T, &cur) && cur == 0), "tag T-1 accepted as T");
  for (int b = 0; b < nblocks; b++) write_block(s, b, T);
  cur = 0;
  CHECK(rec_accept(s.p, s.area.data(), T, &cur) && cur == nblocks, "a full valid set was not accepted");
  if (nblocks > 0) {
    // one word still old / never written / an accumulator with a new low and an old high word, in a late block
    const int b = nblocks - 1 - (int)(seed % (uint64_t)std::min(nblocks, 3));
    uint64_t *r = s.area.data() + (size_t)b * s.p.stride_words;
    const int last = rec_num_words(na, s.k[b]) - 1;
    for (int variant = 0; variant < 3; variant++) {
      int w = last;
      uint32_t tag = Tp;
      if (variant == 1) tag = 0, w = 0;
      if (variant == 2) {
        if (na == 0) continue;
        w = 3 + 2 * (na - 1);  // the high word of the last accumulator
      }
      const uint64_t keep = r[w];
      r[w] = rec_word(tag, keep);
      cur = 0;
      CHECK(!rec_accept(s.p, s.area.data(), T, &cur), "variant %d: an incomplete record was accepted", variant);
      CHECK(cur == b, "variant %d: the cursor stopped at block %d, not %d", variant, cur, b);
      r[w] = keep;
      CHECK(rec_accept(s.p, s.area.data(), T, &cur) && cur == nblocks, "variant %d: not accepted once complete", variant);
    }
  }
  std::vector<uint64_t> out(std::max(na, 1)), segm(s.slot.size(), 0), want_seg(s.slot.size(), 0);
  uint64_t m = 0, sc = 0, wm = 0, ws = 0;
  std::vector<uint64_t> scratch(std::max(nblocks, 1));
  rec_reduce(s.p, s.area.data(), out.data(), &m, &sc, segm.data(), scratch.data());
  for (int b = 0; b < nblocks; b++) {
    wm += s.matched[b];
    ws += s.scanned[b];
    for (int j = 0; j < s.k[b]; j++) want_seg[s.slot[s.first[b] + j]] += s.seg[b][j];
  }
  CHECK(m == wm && sc == ws, "matched %llu / %llu scanned %llu / %llu", (unsigned long long)m, (unsigned long long)wm,
        (unsigned long long)sc, (unsigned long long)ws);
  CHECK(segm == want_seg, "per-segment counts differ");
  for (int a = 0; a < na; a++) {
    if (kinds[a] == ACC_COUNT || kinds[a] == ACC_SUM_I64) {
      uint64_t w = 0;
      for (int b = 0; b < nblocks; b++) w += s.acc[a][b];
      CHECK(out[a] == w, "slot %d: int64 total %llx, want %llx", a, (unsigned long long)out[a], (unsigned long long)w);
    } else {
      std::vector<double> v(nblocks);
      for (int b = 0; b < nblocks; b++) v[b] = f64(s.acc[a][b]);
      const double w = restated(kinds[a], v);
      CHECK(same(f64(out[a]), w), "slot %d kind %d: %a (%016llx), restated %a (%016llx), %d blocks", a, kinds[a],
            f64(out[a]), (unsigned long long)out[a], w, (unsigned long long)u64(w), nblocks);
    }
  }
}

static int run_reduce() {
  CHECK(rec_next_tag(65535) == 1 && rec_next_tag(0) == 1 && rec_next_tag(65534) == 65535 && rec_next_tag(7) == 8,
        "the tag counter must skip 0");
  CHECK(acc_combine(ACC_MIN_F64, u64(0.0), u64(-0.0)) == u64(-0.0) && acc_combine(ACC_MIN_F64, u64(-0.0), u64(0.0)) == u64(-0.0),
        "min orders -0.0 below +0.0");
  CHECK(acc_combine(ACC_MAX_F64, u64(0.0), u64(-0.0)) == u64(0.0) && acc_combine(ACC_MAX_F64, u64(-0.0), u64(0.0)) == u64(0.0),
        "max orders +0.0 above -0.0");
  const std::vector<int32_t> four = {ACC_SUM_I64, ACC_SUM_F64, ACC_MIN_F64, ACC_MAX_F64};
  uint64_t seed = 1;
  for (int nblocks : {1, 2, 8, 63, 64, 65, 130, 1280}) {
    check_set(nblocks, four, 6, false, seed++);            // 128-B records, K = 0 .. 6
    check_set(nblocks, four, 6, true, seed++);             // ... every block at the record's limit
    check_set(nblocks, {ACC_SUM_F64}, 4, false, seed++);   // 64-B records
    check_set(nblocks, {ACC_SUM_F64}, 12, true, seed++);   // one accumulator, K = 12: 16 words
    check_set(nblocks, {}, kRecSegSlots, true, seed++);    // a filter-only plan at K = 14
    check_set(nblocks, {}, 0, true, seed++);               // K = 0: two words
    check_set(nblocks, {ACC_COUNT, ACC_MAX_F64}, 2, false, seed++);
  }
  if (g_fail == 0) printf("REDUCE OK\n");
  return g_fail == 0 ? 0 : 1;
}

static int run_table(const char *arg) {
  std::vector<int> lens;
  for (const char *p = arg; *p;) {
    lens.push_back(atoi(p));
    while (*p && *p != ',') p++;
    if (*p == ',') p++;
  }
  const int grids0[] = {1, 3, 8, 20}, grids2[] = {8, 16, 40};
  for (int walk : {0, 2}) {
    for (int gi = 0; gi < (walk == 0 ? 4 : 3); gi++) {
      const int nblocks = walk == 0 ? grids0[gi] : grids2[gi];
      for (int total = 0; total <= 200; total++) {
        std::vector<int32_t> entry_begin;
        for (int t = 0, i = 0; t < total || entry_begin.empty(); t += lens[i % lens.size()], i++) entry_begin.push_back(t);
        const RecBlocks tb = rec_block_table(walk, total, nblocks, 4, entry_begin);
        printf("T %d %d %d\n", walk, nblocks, total);
        for (int b = 0; b < nblocks; b++) {
          printf("B %d %d %d %d %d", b, tb.begin[b], tb.end[b], tb.first[b], tb.k[b]);
          for (int w = 0; w < 4; w++) {
            const TileRange r = wave_tile_range(walk, total, nblocks, b, w, 4);
            printf(" %d %d", r.begin, r.end);
          }
          printf("\n");
        }
      }
    }
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 2 && !strcmp(argv[1], "reduce")) return run_reduce();
  if (argc >= 3 && !strcmp(argv[1], "table")) return run_table(argv[2]);
  fprintf(stderr, "usage: %s reduce | table L1,L2,...\n", argv[0]);
  return 2;
}
