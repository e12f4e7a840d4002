// Stand-alone check of the small fused scan's launch shape (pinot_amd/csrc/fused_shape.h), built by
// tests/test_fused_shape.py with -fsanitize=address,undefined and run as a fresh process.
//
//   shape_main sweep                                  every invariant over tile counts 1..8192, slots of 512 B..19 KB,
//                                                     1 and 256 CUs; prints "SHAPE OK <cases>" or the failures, exits 1
//   shape_main one TILES S0 R0 S1 R1 CUS [NBUF]       prints "mode blocks nbuf bpc T" of one input (slot / doc-ring
//                                                     bytes per mode; static LDS 448, 4 waves, 5 workgroups per CU)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../pinot_amd/csrc/fused_shape.h"

using namespace phip;

static int g_fail = 0;
#define CHECK(c, ...)                             \
  do {                                            \
    if (!(c)) {                                   \
      if (g_fail < 20) {                          \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                      \
        printf("\n");                             \
      }                                           \
      g_fail++;                                   \
    }                                             \
  } while (0)

static FusedShapeIn input(int64_t tiles, int s0, int r0, int s1, int r1, int cus, int nbuf) {
  FusedShapeIn in;
  memset(&in, 0, sizeof(in));
  in.tiles = tiles;
  in.slot[0] = s0;
  in.doc_ring[0] = r0;
  in.slot[1] = s1;
  in.doc_ring[1] = r1;
  in.static_lds = 448;
  in.waves = 4;
  in.cus = cus;
  in.wave_cap = 5;
  in.force_nbuf = nbuf;
  return in;
}

static int64_t lds_of(const FusedShapeIn &in, int mode, int nbuf) {
  return (int64_t)in.waves * nbuf * in.slot[mode] + in.doc_ring[mode] + in.static_lds;
}

// does T fit mode `mode` with some ring depth in [lo, hi]? (a restatement by brute force)
static bool fits(const FusedShapeIn &in, int mode, int64_t T, int lo, int hi) {
  const int64_t blocks = (in.tiles + in.waves * T - 1) / (in.waves * T);
  for (int nbuf = lo; nbuf <= hi; nbuf++) {
    const int64_t lds = lds_of(in, mode, nbuf);
    if (lds > 160 * 1024) continue;
    int64_t bpc = (160 * 1024) / lds;
    if (bpc > in.wave_cap) bpc = in.wave_cap;
    if (blocks <= in.cus * bpc) return true;
  }
  return false;
}

// the smallest T of one mode under the rule, by brute force from 1 upwards (T = 0: none)
static int64_t brute_T(const FusedShapeIn &in, int mode, int64_t stop) {
  if (in.slot[mode] <= 0) return 0;
  const bool two = lds_of(in, mode, 2) <= 160 * 1024;  // two slots per wave fit one workgroup
  for (int64_t T = 1; T <= stop; T++) {
    if (T == 1 && fits(in, mode, 1, 1, kShapeMaxRing)) return 1;
    if (T >= 2 && (two ? fits(in, mode, T, 2, kShapeMaxRing) : fits(in, mode, T, 1, 1))) return T;
  }
  return -1;  // beyond `stop`
}

static void check_one(const FusedShapeIn &in, int64_t *cases) {
  const FusedShape s = fused_small_shape(in);
  ++*cases;
  const bool any = (in.slot[0] > 0 && lds_of(in, 0, 1) <= 160 * 1024) || (in.slot[1] > 0 && lds_of(in, 1, 1) <= 160 * 1024);
  CHECK((s.mode >= 0) == any, "tiles %lld slots %d/%d cus %d: mode %d", (long long)in.tiles, in.slot[0], in.slot[1], in.cus, s.mode);
  if (s.mode < 0) return;
  const long long t = in.tiles;
#define CTX "tiles %lld slots %d/%d rings %d/%d cus %d -> mode %d blocks %d nbuf %d bpc %d T %lld", t, in.slot[0], in.slot[1], \
  in.doc_ring[0], in.doc_ring[1], in.cus, s.mode, s.blocks, s.nbuf, s.bpc, (long long)s.T
  CHECK(in.slot[s.mode] > 0, CTX);
  CHECK(s.T >= 1 && s.blocks >= 1 && s.nbuf >= 1 && s.nbuf <= kShapeMaxRing && s.bpc >= 1 && s.bpc <= in.wave_cap, CTX);
  // every tile has a wave: blocks * 4 * T >= tiles, and T is what that many blocks need
  CHECK((int64_t)s.blocks * in.waves * s.T >= in.tiles, CTX);
  CHECK(s.blocks == (in.tiles + in.waves * s.T - 1) / (in.waves * s.T), CTX);
  // the chosen LDS fits 160 KiB times the chosen workgroups per CU, and all blocks are resident at once
  CHECK(lds_of(in, s.mode, s.nbuf) * s.bpc <= 160 * 1024, CTX);
  CHECK(s.blocks <= (int64_t)in.cus * s.bpc, CTX);
  // ring depth: at least 2 under T >= 2 whenever two slots fit one workgroup at all (then the largest T, one
  // workgroup, fits with them); and the deepest that keeps the blocks resident: one slot more does not
  if (s.T >= 2) CHECK(s.nbuf >= 2 || lds_of(in, s.mode, 2) > 160 * 1024, CTX);
  if (s.nbuf < kShapeMaxRing) {
    const int64_t lds = lds_of(in, s.mode, s.nbuf + 1);
    int64_t bpc = lds > 160 * 1024 ? 0 : (160 * 1024) / lds;
    if (bpc > in.wave_cap) bpc = in.wave_cap;
    CHECK(s.blocks > in.cus * bpc, CTX);
  }
  // the smallest T of the mode, and the mode with the smaller T (mode 0 on a tie)
  const int64_t b0 = brute_T(in, 0, s.T), b1 = brute_T(in, 1, s.T);
  const int64_t mine = s.mode == 0 ? b0 : b1, other = s.mode == 0 ? b1 : b0;
  CHECK(mine == s.T, CTX);
  if (s.mode == 0) CHECK(other == 0 || other == -1 || other >= s.T, CTX);
  else CHECK(b0 == 0 || b0 == -1, CTX);  // (mode 0 found no T <= s.T)
#undef CTX
}

int main(int argc, char **argv) {
  if (argc >= 8 && !strcmp(argv[1], "one")) {
    const FusedShapeIn in = input(atoll(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]),
                                  argc > 8 ? atoi(argv[8]) : 0);
    const FusedShape s = fused_small_shape(in);
    printf("%d %d %d %d %lld\n", s.mode, s.blocks, s.nbuf, s.bpc, (long long)s.T);
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "sweep")) {
    const int slots[] = {512, 1040, 2624, 4096, 9856, 16384, 19456};
    int64_t cases = 0;
    for (int cus : {1, 256})
      for (int s0 : slots)
        for (int s1 : {0, 512, 2624, 9856, 19456})
          for (int64_t tiles = 1; tiles <= 8192; tiles += (tiles < 300 || tiles >= 8180 ? 1 : 7)) {
            if (s1 > s0) continue;  // (the deferred slot is the streamed one less the value columns)
            check_one(input(tiles, s0, 4096, s1, 8192, cus, 0), &cases);
          }
    // a forced depth is kept
    for (int nbuf = 1; nbuf <= 8; nbuf++)
      for (int64_t tiles : {1, 5, 40, 450, 3776}) {
        const FusedShapeIn in = input(tiles, 2624, 8192, 0, 0, 1, nbuf);
        const FusedShape s = fused_small_shape(in);
        cases++;
        CHECK(s.mode == 0 && s.nbuf == nbuf && (int64_t)s.blocks * 4 * s.T >= tiles && s.blocks <= s.bpc, "forced %d tiles %lld",
              nbuf, (long long)tiles);
      }
    if (g_fail) {
      printf("%d failures\n", g_fail);
      return 1;
    }
    printf("SHAPE OK %lld\n", (long long)cases);
    return 0;
  }
  fprintf(stderr, "usage: shape_main sweep | one TILES S0 R0 S1 R1 CUS [NBUF]\n");
  return 2;
}
