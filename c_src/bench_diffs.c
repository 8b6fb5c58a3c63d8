/*
 * bench_diffs.c — what on_diffs costs per local mutation on a device-resident replica:
 * dgr_mutate_batch_diffs against dgr_mutate_batch (c_src/replica.c, the calls the NIF makes),
 * in ONE process on ONE state, alternating.
 *
 * The replica is bench_mutate.c's: n keys x -> x by node 0 with a MerkleMap of ~3 keys per
 * bucket.  Each of the `reps` rounds makes, for each of three variants in turn -- plain,
 * diffs, plain again -- the one-key ops `add` (a key the replica lacks), `update` (the same
 * key, a new value) and `remove` (the key goes), so the state has n keys again after every
 * round and every variant sees the same sequence of shapes.  The second plain leg measures the
 * run-to-run spread of the plain path itself, the yardstick for the diffs' cost.  The diffs
 * leg also checks what comes back (one changed key; NEW, OLD|NEW with different ids, OLD).
 *
 *   bench_diffs [n_keys=1000] [reps=300]
 *
 * prints one JSON line: the median microseconds per op and variant.
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

enum { V_PLAIN = 0, V_DIFFS, V_PLAIN2, N_VAR };
enum { OP_ADD = 0, OP_UPDATE, OP_REMOVE, N_OPS };
static const char* VAR_NAMES[N_VAR] = {"plain", "diffs", "plain_again"};
static const char* OP_NAMES[N_OPS] = {"add", "update", "remove"};

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
  dgr_engine* g;
  dgr_state* s;
  DG(dgr_engine_open(0, &g));
  dg_store hs = {key, val, ts, node, cnt, (uint64_t)n, (uint64_t)n};
  uint32_t n0 = 0;
  uint64_t c0 = (uint64_t)n;
  dg_context hc = {DG_CTX_VV, 0, &n0, &c0, 1, 1};
  DG(dgr_state_load(g, &hs, &hc, &s));
  uint64_t version = dgr_state_version(s);
  uint32_t depth = 8;
  while (depth < 28 && (UINT64_C(3) << depth) < (uint64_t)n) depth++;
  DG(dgr_refresh_terms(g, NULL, 0, NULL, NULL, 0));
  DG(dgr_merkle_build(s, version, depth));

  double* t[N_VAR][N_OPS];
  for (int a = 0; a < N_VAR; a++)
    for (int o = 0; o < N_OPS; o++) t[a][o] = malloc((size_t)reps * sizeof(double));
  int64_t clock = n, fresh = n;
  const int warm = 20;
  for (int r = -warm; r < reps; r++) {
    for (int a = 0; a < N_VAR; a++) {
      const uint64_t k = key_int(++fresh); /* a key the replica lacks */
      for (int o = 0; o < N_OPS; o++) {
        const uint8_t kind = o != OP_REMOVE;
        const uint64_t w = val_int(fresh + o);
        const int64_t at = ++clock;
        dgr_changed c;
        dgr_diffs d;
        const double t0 = now_us();
        if (a == V_DIFFS)
          DG(dgr_mutate_batch_diffs(s, version, 0, 1, &kind, &k, &w, &at, &c, &d));
        else
          DG(dgr_mutate_batch(s, version, 0, 1, &kind, &k, &w, &at, &c));
        const double dt = now_us() - t0;
        version = c.version;
        CHECK(c.n_changed == 1 && c.keys[0] == k);
        if (a == V_DIFFS) {
          CHECK(d.n == 1);
          if (o == OP_ADD) CHECK(d.flags[0] == DG_DIFF_NEW && d.new_val[0] == w && d.old_val[0] == 0);
          if (o == OP_UPDATE)
            CHECK(d.flags[0] == (DG_DIFF_OLD | DG_DIFF_NEW) && d.new_val[0] == w && d.old_val[0] == val_int(fresh));
          if (o == OP_REMOVE) CHECK(d.flags[0] == DG_DIFF_OLD && d.old_val[0] == val_int(fresh + 1) && d.new_val[0] == 0);
        }
        if (r >= 0) t[a][o][r] = dt;
      }
    }
  }
  CHECK(dgr_state_rows(s) == (uint64_t)n);
  printf("{\"n_keys\": %lld, \"reps\": %d, \"unit\": \"us_per_op_median\"", (long long)n, reps);
  for (int o = 0; o < N_OPS; o++) {
    printf(", \"%s\": {", OP_NAMES[o]);
    for (int a = 0; a < N_VAR; a++) printf("%s\"%s\": %.2f", a ? ", " : "", VAR_NAMES[a], median(t[a][o], reps));
    printf("}");
  }
  printf("}\n");
  dgr_state_free(s);
  dgr_engine_close(g);
  return 0;
}
