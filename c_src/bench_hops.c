/*
 * bench_hops.c — k neighbours' pending continuation messages at one replica: k
 * dgr_merkle_continue calls against ONE dgr_merkle_continue_batch (c_src/replica_merkle.c, the
 * calls deltagpu_nif.c makes).  X is a replica of `n` keys with a tree of depth `depth`; each of
 * KMAX neighbours differs from it on `permille` / 1000 of the keys (its own choice of keys).
 * Every neighbour's conversation with X is walked once in both orientations (the neighbour
 * prepares / X prepares, 8 levels per message, max_sync_size 200) and the messages X receives
 * are kept, per position of the conversation ("hop kind").  Then, per hop kind and k = 1, 2, 4,
 * 8, 16, 64: the k messages answered one by one and as one batch, alternating in one process;
 * the median of `rounds` rounds each, `repeats` times over -- the spread of the singles'
 * medians over the repeats is the noise a difference has to beat.  One JSON line per (hop
 * kind, k).  The batch's answers are compared with the singles' once, byte for byte.
 *     bench_hops N_KEYS DEPTH [ROUNDS [REPEATS [FRAC_PERMILLE [MAX_SYNC]]]]
 */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "replica.h"

#define DG(x)                                                                          \
  do {                                                                                 \
    int rc_ = (x);                                                                     \
    if (rc_ != DG_OK) {                                                                \
      fprintf(stderr, "FAIL %s:%d: %s -> %d (%s)\n", __FILE__, __LINE__, #x, rc_,        \
              dg_last_error());                                                        \
      exit(1);                                                                         \
    }                                                                                  \
  } while (0)

static double now_us(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return t.tv_sec * 1e6 + t.tv_nsec * 1e-3;
}

static int cmp_d(const void* a, const void* b) {
  const double x = *(const double*)a, y = *(const double*)b;
  return x < y ? -1 : x > y;
}

static int cmp_u64(const void* a, const void* b) {
  const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
  return x < y ? -1 : x > y;
}

static uint64_t mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ULL;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
  return x ^ (x >> 31);
}

#define KMAX DG_CONT_BATCH_MAX
#define MAX_KINDS 8 /* positions of a conversation at which X answers: 2 orientations x 4 */
#define MAX_TURNS 16

typedef struct {
  uint8_t* bin;
  uint64_t len;
} msg_t;

static msg_t g_msg[MAX_KINDS][KMAX];
static uint32_t g_level[MAX_KINDS];
static int g_kinds = 0;

static msg_t keep(const uint8_t* p, uint64_t len) {
  msg_t m = {malloc(len ? len : 1), len};
  if (len) memcpy(m.bin, p, len);
  return m;
}

static uint32_t level_of(const msg_t* m) {
  uint32_t l;
  memcpy(&l, m->bin, 4);
  return l;
}

/* one conversation between X and neighbour N (i), `first` preparing; X's incoming messages kept */
static void walk(dgr_state* X, dgr_state* N, int x_prepares, int i, uint32_t levels, uint64_t max_sync) {
  const uint8_t* out;
  uint64_t len;
  dgr_state* side[2] = {x_prepares ? N : X, x_prepares ? X : N}; /* who answers turn 0, 1 */
  DG(dgr_merkle_prepare(side[1], dgr_state_version(side[1]), levels, &out, &len));
  for (int turn = 0; turn < MAX_TURNS; turn++) {
    msg_t m = keep(out, len);
    dgr_state* S = side[turn % 2];
    if (S == X) {
      const int kind = (x_prepares ? MAX_KINDS / 2 : 0) + turn / 2;
      if (turn / 2 >= MAX_KINDS / 2) {
        fprintf(stderr, "a conversation of more turns than expected\n");
        exit(1);
      }
      g_msg[kind][i] = m;
    }
    int status;
    const uint64_t* k;
    uint64_t nk;
    DG(dgr_merkle_continue(S, dgr_state_version(S), m.bin, m.len, levels, max_sync, &status, &out, &len, &k, &nk));
    if (S != X) free(m.bin);
    if (status == 0) return;
  }
  fprintf(stderr, "too many turns\n");
  exit(1);
}

static double median(double* v, int n) {
  qsort(v, (size_t)n, sizeof(double), cmp_d);
  return v[n / 2];
}

int main(int argc, char** argv) {
  const uint64_t n = argc > 1 ? strtoull(argv[1], NULL, 10) : 12500000;
  const uint32_t depth = argc > 2 ? (uint32_t)atoi(argv[2]) : 22;
  const int rounds = argc > 3 ? atoi(argv[3]) : 20;
  const int repeats = argc > 4 ? atoi(argv[4]) : 3;
  const uint64_t permille = argc > 5 ? strtoull(argv[5], NULL, 10) : 10;
  const uint64_t max_sync = argc > 6 ? strtoull(argv[6], NULL, 10) : 200;
  const uint32_t levels = 8;
  uint64_t* key = malloc(n * 8);
  for (uint64_t i = 0; i < n; i++) key[i] = mix(i);
  qsort(key, n, 8, cmp_u64);
  uint64_t *val = malloc(n * 8), *cnt = malloc(n * 8), *valb = malloc(n * 8);
  int64_t* ts = malloc(n * 8);
  uint32_t* node = calloc(n, 4);
  for (uint64_t i = 0; i < n; i++) {
    val[i] = i;
    ts[i] = (int64_t)i;
    cnt[i] = i + 1;
  }
  dgr_engine* g;
  DG(dgr_engine_open(0, &g));
  DG(dgr_refresh_terms(g, NULL, 0, NULL, NULL, 0));
  uint32_t n0 = 0;
  uint64_t c0 = n;
  dg_context vv = {DG_CTX_VV, 0, &n0, &c0, 1, 1};
  dg_store rx = {key, val, ts, node, cnt, n, n};
  dgr_state* X;
  DG(dgr_state_load(g, &rx, &vv, &X));
  DG(dgr_merkle_build(X, dgr_state_version(X), depth));
  /* the neighbours, one resident at a time: their conversations leave X's incoming messages */
  for (int i = 0; i < KMAX; i++) {
    const uint64_t salt = 0x5555 + 0x10001ULL * (uint64_t)i;
    for (uint64_t r = 0; r < n; r++) valb[r] = (mix(r ^ salt) % 1000) < permille ? r + (UINT64_C(1) << 40) : r;
    dg_store rn = {key, valb, ts, node, cnt, n, n};
    dgr_state* N;
    DG(dgr_state_load(g, &rn, &vv, &N));
    DG(dgr_merkle_build(N, dgr_state_version(N), depth));
    walk(X, N, 0, i, levels, max_sync);
    walk(X, N, 1, i, levels, max_sync);
    DG(dgr_state_free(N));
  }
  /* the hop kinds every neighbour's conversation reached */
  int kinds[MAX_KINDS];
  for (int q = 0; q < MAX_KINDS; q++) {
    int all = 1;
    for (int i = 0; i < KMAX; i++) all &= g_msg[q][i].bin != NULL;
    if (!all) continue;
    g_level[q] = level_of(&g_msg[q][0]);
    kinds[g_kinds++] = q;
  }
  const int ks[] = {1, 2, 4, 8, 16, 64};
  const uint64_t ver = dgr_state_version(X);
  double* ts_single = calloc((size_t)rounds, sizeof(double));
  double* ts_batch = calloc((size_t)rounds, sizeof(double));
  const uint8_t* bins[KMAX];
  uint64_t lens[KMAX];
  dgr_cont_result res[KMAX];
  for (int qi = 0; qi < g_kinds; qi++) {
    const int q = kinds[qi];
    for (int i = 0; i < KMAX; i++) {
      bins[i] = g_msg[q][i].bin;
      lens[i] = g_msg[q][i].len;
    }
    /* once: the batch's answers are the singles' (copied: the single call reuses the buffers) */
    DG(dgr_merkle_continue_batch(X, ver, KMAX, bins, lens, levels, max_sync, res));
    uint64_t out_bytes = 0;
    msg_t copy[KMAX];
    for (int i = 0; i < KMAX; i++) {
      copy[i] = res[i].status == 1 ? keep(res[i].bin, res[i].len) : keep((const uint8_t*)res[i].keys, 8 * res[i].n_keys);
      out_bytes += copy[i].len;
    }
    for (int i = 0; i < KMAX; i++) {
      int status;
      const uint8_t* out;
      const uint64_t* k;
      uint64_t len, nk;
      DG(dgr_merkle_continue(X, ver, bins[i], lens[i], levels, max_sync, &status, &out, &len, &k, &nk));
      const int same = res[i].rc == DG_OK && status == res[i].status &&
                       (status == 1 ? len == copy[i].len && !memcmp(out, copy[i].bin, len)
                                    : 8 * nk == copy[i].len && !memcmp(k, copy[i].bin, 8 * nk));
      if (!same) {
        fprintf(stderr, "hop kind %d, message %d: the batch's answer differs from the single call's\n", q, i);
        return 1;
      }
      free(copy[i].bin);
    }
    for (unsigned a = 0; a < sizeof ks / sizeof ks[0]; a++) {
      const int k = ks[a];
      double ms[8], mb[8];
      for (int rep = 0; rep < repeats && rep < 8; rep++) {
        for (int it = -3; it < rounds; it++) {
          double t0 = now_us();
          for (int i = 0; i < k; i++) {
            int status;
            const uint8_t* out;
            const uint64_t* kk;
            uint64_t len, nk;
            DG(dgr_merkle_continue(X, ver, bins[i], lens[i], levels, max_sync, &status, &out, &len, &kk, &nk));
          }
          const double el_s = now_us() - t0;
          t0 = now_us();
          DG(dgr_merkle_continue_batch(X, ver, k, bins, lens, levels, max_sync, res));
          const double el_b = now_us() - t0;
          if (it >= 0) {
            ts_single[it] = el_s;
            ts_batch[it] = el_b;
          }
        }
        ms[rep] = median(ts_single, rounds);
        mb[rep] = median(ts_batch, rounds);
      }
      const int nr = repeats < 8 ? repeats : 8;
      double s_lo = ms[0], s_hi = ms[0], b_lo = mb[0], b_hi = mb[0];
      for (int rep = 1; rep < nr; rep++) {
        s_lo = ms[rep] < s_lo ? ms[rep] : s_lo;
        s_hi = ms[rep] > s_hi ? ms[rep] : s_hi;
        b_lo = mb[rep] < b_lo ? mb[rep] : b_lo;
        b_hi = mb[rep] > b_hi ? mb[rep] : b_hi;
      }
      printf("{\"n_keys\": %llu, \"depth\": %u, \"max_sync_size\": %llu, \"hop_kind\": %d, \"x_prepares\": %d, "
             "\"level_in\": %u, \"bytes_in\": %llu, \"bytes_out_64\": %llu, \"k\": %d, \"rounds\": %d, \"repeats\": %d, "
             "\"singles_us\": [%.2f, %.2f], \"batch_us\": [%.2f, %.2f], \"singles_spread_us\": %.2f, "
             "\"batch_wins\": %s}\n",
             (unsigned long long)n, depth, (unsigned long long)max_sync, q, q >= MAX_KINDS / 2, g_level[q],
             (unsigned long long)lens[0], (unsigned long long)out_bytes, k, rounds, nr, s_lo, s_hi, b_lo, b_hi,
             s_hi - s_lo, b_hi < s_lo - (s_hi - s_lo) ? "true" : "false");
      fflush(stdout);
    }
  }
  dgr_state_free(X);
  dgr_engine_close(g);
  return 0;
}
