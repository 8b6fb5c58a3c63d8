/*
 * bench_hop_take.c — the hop that ends a sync on its originator, with its rows: the two calls
 * (dgr_merkle_continue_batch, then dgr_take_batch on the keys it returned) against the ONE
 * dgr_merkle_continue_take_batch (c_src/replica_merkle.c, the calls deltagpu_nif.c makes).  X is a
 * replica of `n` keys with a tree of depth `depth`; each of `neigh` neighbours differs from it on
 * `permille` / 1000 of the keys.  X starts a sync with each (8 levels per message, max_sync_size
 * 200) and the leaf-form message it receives last is kept.  Then, for k = 1, 2, 8, 64 (up to
 * `neigh`): the k messages answered by the two calls and by the one, alternating in one process;
 * the median of `rounds` rounds each, `repeats` times over -- the spread of the two-call side's
 * medians is the noise a difference has to beat; at k = 1 also the single hop and dgr_take, the
 * lone hop's other route.  One JSON line per k.  Before timing, the one
 * call's answers are compared with the two calls' byte for byte: keys, and every hop's rows
 * against dgr_take of its keys.  DGR_TAKE_LONE=0 / 1 (replica_merkle.c) picks the lone hop's route.
 *     bench_hop_take N_KEYS DEPTH [ROUNDS [REPEATS [FRAC_PERMILLE [MAX_SYNC [NEIGH]]]]]
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
#define MAX_TURNS 16

typedef struct {
  uint8_t* bin;
  uint64_t len;
} msg_t;

static msg_t keep(const void* p, uint64_t len) {
  msg_t m = {malloc(len ? len : 1), len};
  if (len) memcpy(m.bin, p, len);
  return m;
}

/* X starts a sync with N; the leaf form X receives (the message it answers with keys) is returned */
static msg_t walk(dgr_state* X, dgr_state* N, uint32_t depth, uint32_t levels, uint64_t max_sync) {
  const uint8_t* out;
  uint64_t len;
  DG(dgr_merkle_prepare(X, dgr_state_version(X), levels, &out, &len));
  for (int turn = 0; turn < MAX_TURNS; turn++) {
    msg_t m = keep(out, len);
    dgr_state* S = turn % 2 ? X : N;
    int status;
    const uint64_t* k;
    uint64_t nk;
    DG(dgr_merkle_continue(S, dgr_state_version(S), m.bin, m.len, levels, max_sync, &status, &out, &len, &k, &nk));
    if (status == 0) {
      uint32_t level;
      memcpy(&level, m.bin, 4);
      if (S != X || level != depth + 1 || nk == 0) {
        fprintf(stderr, "the sync did not end on its originator with a leaf form and keys\n");
        exit(1);
      }
      return m;
    }
    free(m.bin);
  }
  fprintf(stderr, "too many turns\n");
  exit(1);
}

static double median(double* v, int n) {
  qsort(v, (size_t)n, sizeof(double), cmp_d);
  return v[n / 2];
}

static int same_rows(const dg_store* a, const dg_store* b) {
  return a->n == b->n && !memcmp(a->key, b->key, 8 * a->n) && !memcmp(a->val, b->val, 8 * a->n) &&
         !memcmp(a->ts, b->ts, 8 * a->n) && !memcmp(a->node, b->node, 4 * a->n) && !memcmp(a->cnt, b->cnt, 8 * a->n);
}

int main(int argc, char** argv) {
  const uint64_t n = argc > 1 ? strtoull(argv[1], NULL, 10) : 12500000;
  const uint32_t depth = argc > 2 ? (uint32_t)atoi(argv[2]) : 22;
  const int rounds = argc > 3 ? atoi(argv[3]) : 20;
  const int repeats = argc > 4 ? atoi(argv[4]) : 3;
  const uint64_t permille = argc > 5 ? strtoull(argv[5], NULL, 10) : 10;
  const uint64_t max_sync = argc > 6 ? strtoull(argv[6], NULL, 10) : 200;
  const int neigh = argc > 7 && atoi(argv[7]) >= 1 && atoi(argv[7]) <= KMAX ? atoi(argv[7]) : KMAX;
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
  msg_t msg[KMAX];
  for (int i = 0; i < neigh; i++) { /* the neighbours, one resident at a time */
    const uint64_t salt = 0x5555 + 0x10001ULL * (uint64_t)i;
    for (uint64_t r = 0; r < n; r++) valb[r] = (mix(r ^ salt) % 1000) < permille ? r + (UINT64_C(1) << 40) : r;
    dg_store rn = {key, valb, ts, node, cnt, n, n};
    dgr_state* N;
    DG(dgr_state_load(g, &rn, &vv, &N));
    DG(dgr_merkle_build(N, dgr_state_version(N), depth));
    msg[i] = walk(X, N, depth, levels, max_sync);
    DG(dgr_state_free(N));
  }
  const uint64_t ver = dgr_state_version(X);
  const uint8_t* bins[KMAX];
  uint64_t lens[KMAX], nks[KMAX];
  const uint64_t* keys[KMAX];
  uint8_t want[KMAX];
  dgr_cont_result res[KMAX];
  dgr_hop_rows taken[KMAX];
  dgr_taken tk;
  for (int i = 0; i < neigh; i++) {
    bins[i] = msg[i].bin;
    lens[i] = msg[i].len;
    want[i] = 1;
  }
  /* once: the one call's keys and rows are the two calls' (copied: the calls reuse the buffers) */
  DG(dgr_merkle_continue_take_batch(X, ver, neigh, bins, lens, want, levels, max_sync, res, taken));
  uint64_t keys_out = 0, rows_out = 0;
  msg_t ck[KMAX], cr[KMAX][5];
  uint64_t rn[KMAX];
  for (int i = 0; i < neigh; i++) {
    if (res[i].rc != DG_OK || res[i].status != 0 || !taken[i].offs) {
      fprintf(stderr, "message %d: no keys with rows\n", i);
      return 1;
    }
    ck[i] = keep(res[i].keys, 8 * res[i].n_keys);
    rn[i] = taken[i].rows.n;
    cr[i][0] = keep(taken[i].rows.key, 8 * rn[i]);
    cr[i][1] = keep(taken[i].rows.val, 8 * rn[i]);
    cr[i][2] = keep(taken[i].rows.ts, 8 * rn[i]);
    cr[i][3] = keep(taken[i].rows.node, 4 * rn[i]);
    cr[i][4] = keep(taken[i].rows.cnt, 8 * rn[i]);
    if (taken[i].offs[res[i].n_keys] != rn[i]) return 1;
    keys_out += res[i].n_keys;
    rows_out += rn[i];
  }
  DG(dgr_merkle_continue_batch(X, ver, neigh, bins, lens, levels, max_sync, res));
  for (int i = 0; i < neigh; i++)
    if (res[i].rc != DG_OK || res[i].status != 0 || 8 * res[i].n_keys != ck[i].len ||
        memcmp(res[i].keys, ck[i].bin, ck[i].len)) {
      fprintf(stderr, "message %d: the one call's keys differ from dgr_merkle_continue_batch's\n", i);
      return 1;
    }
  for (int i = 0; i < neigh; i++) {
    dg_store t1, mine = {(uint64_t*)cr[i][0].bin, (uint64_t*)cr[i][1].bin, (int64_t*)cr[i][2].bin,
                         (uint32_t*)cr[i][3].bin, (uint64_t*)cr[i][4].bin, rn[i], rn[i]};
    DG(dgr_take(X, ver, (const uint64_t*)ck[i].bin, ck[i].len / 8, &t1));
    if (!same_rows(&t1, &mine)) {
      fprintf(stderr, "message %d: the one call's rows differ from dgr_take's\n", i);
      return 1;
    }
  }
  const int ks[] = {1, 2, 8, 64};
  double* t_two = calloc((size_t)rounds, sizeof(double));
  double* t_one = calloc((size_t)rounds, sizeof(double));
  for (unsigned a = 0; a < sizeof ks / sizeof ks[0]; a++) {
    const int k = ks[a];
    if (k > neigh) break;
    double ms[8], mb[8];
    for (int rep = 0; rep < repeats && rep < 8; rep++) {
      for (int it = -3; it < rounds; it++) {
        double t0 = now_us();
        DG(dgr_merkle_continue_batch(X, ver, k, bins, lens, levels, max_sync, res));
        for (int i = 0; i < k; i++) {
          keys[i] = res[i].keys;
          nks[i] = res[i].n_keys;
        }
        DG(dgr_take_batch(X, ver, k, keys, nks, &tk));
        const double el_two = now_us() - t0;
        t0 = now_us();
        DG(dgr_merkle_continue_take_batch(X, ver, k, bins, lens, want, levels, max_sync, res, taken));
        const double el_one = now_us() - t0;
        if (it >= 0) {
          t_two[it] = el_two;
          t_one[it] = el_one;
        }
      }
      ms[rep] = median(t_two, rounds);
      mb[rep] = median(t_one, rounds);
    }
    double st_lo = 0, st_hi = 0; /* k = 1 only: the single hop and dgr_take, the lone hop's other route */
    for (int rep = 0; k == 1 && rep < repeats && rep < 8; rep++) {
      for (int it = -3; it < rounds; it++) {
        int status;
        const uint8_t* out;
        const uint64_t* kk;
        uint64_t len, nk;
        dg_store t1;
        const double t0 = now_us();
        DG(dgr_merkle_continue(X, ver, bins[0], lens[0], levels, max_sync, &status, &out, &len, &kk, &nk));
        DG(dgr_take(X, ver, kk, nk, &t1));
        if (it >= 0) t_two[it] = now_us() - t0;
      }
      const double md = median(t_two, rounds);
      st_lo = rep == 0 || md < st_lo ? md : st_lo;
      st_hi = rep == 0 || md > st_hi ? md : st_hi;
    }
    const int nr = repeats < 8 ? repeats : 8;
    double s_lo = ms[0], s_hi = ms[0], b_lo = mb[0], b_hi = mb[0];
    for (int rep = 1; rep < nr; rep++) {
      s_lo = ms[rep] < s_lo ? ms[rep] : s_lo;
      s_hi = ms[rep] > s_hi ? ms[rep] : s_hi;
      b_lo = mb[rep] < b_lo ? mb[rep] : b_lo;
      b_hi = mb[rep] > b_hi ? mb[rep] : b_hi;
    }
    const char* lone = getenv("DGR_TAKE_LONE");
    printf("{\"n_keys\": %llu, \"depth\": %u, \"max_sync_size\": %llu, \"neighbours\": %d, \"bytes_in\": %llu, "
           "\"keys_out_all\": %llu, \"rows_out_all\": %llu, \"take_lone\": \"%s\", \"k\": %d, \"rounds\": %d, "
           "\"repeats\": %d, \"two_calls_us\": [%.2f, %.2f], \"one_call_us\": [%.2f, %.2f], "
           "\"two_calls_spread_us\": %.2f, \"one_call_wins\": %s, \"single_hop_and_take_us\": [%.2f, %.2f]}\n",
           (unsigned long long)n, depth, (unsigned long long)max_sync, neigh, (unsigned long long)lens[0],
           (unsigned long long)keys_out, (unsigned long long)rows_out, lone ? lone : "default", k, rounds, nr, s_lo,
           s_hi, b_lo, b_hi, s_hi - s_lo, b_hi < s_lo - (s_hi - s_lo) ? "true" : "false", st_lo, st_hi);
    fflush(stdout);
  }
  dgr_state_free(X);
  dgr_engine_close(g);
  return 0;
}
