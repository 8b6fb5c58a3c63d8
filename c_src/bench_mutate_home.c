/*
 * bench_mutate_home.c — dgr_mutate_batch[_diffs]' two routes against each other (c_src/
 * replica_join.c): DGR_MUTATE_ROUTE=batch (the copy, dg_mutate_batch_async, the join) and =home
 * (dg_mutate_home on the packed message first), in ONE process, on TWO engines holding equal
 * states with a MerkleMap (bench_mutate.c's replica: n keys x -> x by node 0).
 *
 * Each of the `reps` rounds makes, for each of three legs in turn -- batch, home, batch again
 * -- the one-key ops `add` (a key the replica lacks), `update` and `remove`, then batches of 8,
 * 64 and 512 adds of keys it lacks (each followed by the same keys' removes, not timed), so
 * both states have n keys again after every leg.  The second batch leg measures the batch
 * route's own run-to-run spread: the home route is the faster one for a shape only where its
 * median is below BOTH batch legs' by more than those two differ.  Plain, then _diffs.
 *
 *   bench_mutate_home [n_keys=1000] [reps=300]
 *
 * prints one JSON line: the median microseconds per call, per shape and leg, and how often the
 * home route was tried, served and declined.
 */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "marshal.h"
#include "replica.h"

#define DG(x)                                                                                        \
  do {                                                                                               \
    int rc_ = (x);                                                                                   \
    if (rc_ != DG_OK) {                                                                              \
      fprintf(stderr, "FAIL %s:%d: %s -> %d (%s)\n", __FILE__, __LINE__, #x, rc_, dg_last_error()); \
      exit(1);                                                                                       \
    }                                                                                                \
  } while (0)
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                     \
    }                                                              \
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

static double median(double* v, int n) {
  qsort(v, (size_t)n, sizeof *v, cmp_d);
  return n ? v[n / 2] : 0.0;
}

static uint64_t key_int(int64_t k) {
  dgm_buf b = {0};
  dgm_enc_i64(&b, k);
  const uint64_t id = dgm_key_id(b.p, b.n);
  dgm_buf_free(&b);
  return id;
}

static uint64_t val_int(int64_t v) { return (uint64_t)v + (UINT64_C(1) << 62); }

typedef struct {
  uint64_t key, x;
} kx;

static int cmp_kx(const void* a, const void* b) {
  const uint64_t x = ((const kx*)a)->key, y = ((const kx*)b)->key;
  return x < y ? -1 : x > y;
}


enum { L_BATCH = 0, L_HOME, L_BATCH2, N_LEG };
enum { OP_ADD = 0, OP_UPDATE, OP_REMOVE, OP_ADDS8, OP_ADDS64, OP_ADDS512, N_OPS };
static const char* LEG_NAMES[N_LEG] = {"batch", "home", "batch_again"};
static const char* OP_NAMES[N_OPS] = {"add", "update", "remove", "adds8", "adds64", "adds512"};
static const int OP_M[N_OPS] = {1, 1, 1, 8, 64, 512};
#define MAXM 512

typedef struct {
  dgr_engine* g;
  dgr_state* s;
  uint64_t version;
} replica;

static void open_replica(replica* r, const char* route, const dg_store* hs, const dg_context* hc, uint32_t depth) {
  setenv("DGR_MUTATE_ROUTE", route, 1); /* read at engine open */
  DG(dgr_engine_open(0, &r->g));
  DG(dgr_state_load(r->g, hs, hc, &r->s));
  r->version = dgr_state_version(r->s);
  DG(dgr_refresh_terms(r->g, NULL, 0, NULL, NULL, 0));
  DG(dgr_merkle_build(r->s, r->version, depth));
}

/* one call of m ops through the replica's route; returns its microseconds */
static double call(replica* r, int diffs, uint64_t m, const uint8_t* kind, const uint64_t* k, const uint64_t* w,
                   const int64_t* at, uint64_t want_changed) {
  dgr_changed c;
  dgr_diffs d;
  const double t0 = now_us();
  if (diffs)
    DG(dgr_mutate_batch_diffs(r->s, r->version, 0, m, kind, k, w, at, &c, &d));
  else
    DG(dgr_mutate_batch(r->s, r->version, 0, m, kind, k, w, at, &c));
  const double dt = now_us() - t0;
  r->version = c.version;
  CHECK(c.n_changed == want_changed);
  if (diffs) CHECK(d.n == want_changed);
  return dt;
}

int main(int argc, char** argv) {
  const int64_t n = argc > 1 ? atoll(argv[1]) : 1000;
  const int reps = argc > 2 ? atoi(argv[2]) : 300;
  CHECK(n > 0 && reps > 0);
  /* the replica after n adds of x -> x */
  kx* v = malloc((size_t)n * sizeof *v);
  uint64_t* key = calloc((size_t)n, 8);
  uint64_t* val = calloc((size_t)n, 8);
  uint64_t* cnt = calloc((size_t)n, 8);
  int64_t* ts = calloc((size_t)n, 8);
  uint32_t* node = calloc((size_t)n, 4);
  for (int64_t x = 1; x <= n; x++) {
    v[x - 1].key = key_int(x);
    v[x - 1].x = (uint64_t)x;
  }
  qsort(v, (size_t)n, sizeof *v, cmp_kx);
  for (int64_t i = 0; i < n; i++) {
    key[i] = v[i].key;
    val[i] = val_int((int64_t)v[i].x);
    ts[i] = (int64_t)v[i].x;
    cnt[i] = v[i].x;
  }
  dg_store hs = {key, val, ts, node, cnt, (uint64_t)n, (uint64_t)n};
  uint32_t n0 = 0;
  uint64_t c0 = (uint64_t)n;
  dg_context hc = {DG_CTX_VV, 0, &n0, &c0, 1, 1};
  uint32_t depth = 8;
  while (depth < 28 && (UINT64_C(3) << depth) < (uint64_t)n) depth++;
  replica rep[2]; /* [0] route batch (both batch legs), [1] route home: equal states */
  open_replica(&rep[0], "batch", &hs, &hc, depth);
  open_replica(&rep[1], "home", &hs, &hc, depth);

  static uint8_t kind[MAXM];
  static uint64_t k[MAXM], w[MAXM];
  static int64_t at[MAXM];
  printf("{\"n_keys\": %lld, \"reps\": %d, \"unit\": \"us_per_call_median\"", (long long)n, reps);
  int64_t clock = n, fresh = n;
  for (int diffs = 0; diffs < 2; diffs++) {
    double* t[N_LEG][N_OPS];
    for (int a = 0; a < N_LEG; a++)
      for (int o = 0; o < N_OPS; o++) t[a][o] = malloc((size_t)reps * sizeof(double));
    const int warm = 20;
    for (int r = -warm; r < reps; r++) {
      for (int a = 0; a < N_LEG; a++) {
        replica* R = &rep[a == L_HOME];
        /* one key the replica lacks: add, update, remove */
        k[0] = key_int(++fresh);
        for (int o = OP_ADD; o <= OP_REMOVE; o++) {
          kind[0] = o != OP_REMOVE;
          w[0] = val_int(fresh + o);
          at[0] = ++clock;
          const double dt = call(R, diffs, 1, kind, k, w, at, 1);
          if (r >= 0) t[a][o][r] = dt;
        }
        /* m adds of keys it lacks as one batch (timed), then their removes (not timed) */
        for (int o = OP_ADDS8; o < N_OPS; o++) {
          const int m = OP_M[o];
          for (int i = 0; i < m; i++) {
            kind[i] = 1;
            k[i] = key_int(++fresh);
            w[i] = val_int(fresh);
            at[i] = ++clock;
          }
          const double dt = call(R, diffs, (uint64_t)m, kind, k, w, at, (uint64_t)m);
          if (r >= 0) t[a][o][r] = dt;
          memset(kind, 0, (size_t)m);
          call(R, diffs, (uint64_t)m, kind, k, w, at, (uint64_t)m);
        }
      }
    }
    printf(", \"%s\": {", diffs ? "diffs" : "plain");
    for (int o = 0; o < N_OPS; o++) {
      printf("%s\"%s\": {", o ? ", " : "", OP_NAMES[o]);
      for (int a = 0; a < N_LEG; a++) printf("%s\"%s\": %.2f", a ? ", " : "", LEG_NAMES[a], median(t[a][o], reps));
      printf("}");
    }
    printf("}");
  }
  uint64_t st[3];
  DG(dgr_mutate_route_stats(rep[1].g, st));
  printf(", \"home_route\": {\"tried\": %llu, \"served\": %llu, \"declined\": %llu}",
         (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2]);
  DG(dgr_mutate_route_stats(rep[0].g, st));
  CHECK(st[0] == 0);
  printf("}\n");
  for (int i = 0; i < 2; i++) {
    CHECK(dgr_state_rows(rep[i].s) == (uint64_t)n);
    dgr_state_free(rep[i].s);
    dgr_engine_close(rep[i].g);
  }
  return 0;
}
