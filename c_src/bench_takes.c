/*
 * bench_takes.c — the fan-out half of a replica's mailbox: k pending {:get_diff, diff, keys} /
 * send_diff messages answered by k dgr_take calls against ONE dgr_take_batch (c_src/replica.c,
 * the calls the NIF makes), in ONE process on ONE state, alternating.
 *
 * The state holds n keys (hashed ids, one row each).  Two cases of k keysets of m keys:
 *   identical   every neighbour asks for the same m keys (after a burst of local mutations
 *               every Merkle conversation ends in the same keyset);
 *   shared80    the keysets share 80 % of their keys; the other 20 % are each keyset's own.
 * Each of the `reps` rounds times the k takes, then the batch; the batch leg also checks that
 * the ranges of keyset j's keys hold as many rows as its single take brought.  The bytes
 * brought home are counted from the sizes returned: 36 B per row, and 24 B per union key
 * (key, mask, offset) for the batch.  A third leg times the batch's host packing alone
 * (dgr_takes_pack: k sort-uniques, the same work the k takes do one by one), so the share of
 * the host sort in either figure can be read off.
 *
 *   bench_takes [n_keys=12500000] [m=125000] [k=8] [reps=20] [shuffle=0]
 *
 * shuffle = 0 gives the keysets in ascending id order, as a Merkle conversation names them
 * (dgr_take_batch copies such a keyset, dgr_take sorts it anyway); shuffle = 1 in random order
 * (both sort).
 *
 * prints one JSON line: the median microseconds of each leg and the bytes per case.
 */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

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

static int cmp_u64(const void* a, const void* b) {
  const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
  return x < y ? -1 : x > y;
}

static uint64_t mix(uint64_t x) { /* splitmix64: key ids are hashes */
  x += UINT64_C(0x9e3779b97f4a7c15);
  x = (x ^ (x >> 30)) * UINT64_C(0xbf58476d1ce4e5b9);
  x = (x ^ (x >> 27)) * UINT64_C(0x94d049bb133111eb);
  return x ^ (x >> 31);
}

#define MAXK 64
enum { C_IDENT = 0, C_SHARED, N_CASES };
static const char* CASE_NAMES[N_CASES] = {"identical", "shared80"};

int main(int argc, char** argv) {
  const int64_t n = argc > 1 ? atoll(argv[1]) : 12500000;
  const int64_t m = argc > 2 ? atoll(argv[2]) : 125000;
  const int k = argc > 3 ? atoi(argv[3]) : 8;
  const int reps = argc > 4 ? atoi(argv[4]) : 20;
  const int shuffle = argc > 5 ? atoi(argv[5]) : 0;
  CHECK(n > 0 && m > 0 && k > 0 && k <= MAXK && reps > 0 && (int64_t)(k + 1) * m <= n);
  uint64_t* key = malloc((size_t)n * 8);
  uint64_t* val = calloc((size_t)n, 8);
  uint64_t* cnt = calloc((size_t)n, 8);
  int64_t* ts = calloc((size_t)n, 8);
  uint32_t* node = calloc((size_t)n, 4);
  for (int64_t i = 0; i < n; i++) key[i] = mix((uint64_t)i);
  qsort(key, (size_t)n, 8, cmp_u64);
  for (int64_t i = 0; i < n; i++) {
    CHECK(i == 0 || key[i - 1] < key[i]);
    val[i] = (UINT64_C(1) << 62) + (uint64_t)i;
    ts[i] = i;
    cnt[i] = (uint64_t)i + 1;
  }
  dgr_engine* g;
  dgr_state* s;
  DG(dgr_engine_open(0, &g));
  dg_store hs = {key, val, ts, node, cnt, (uint64_t)n, (uint64_t)n};
  uint32_t n0 = 0;
  uint64_t c0 = (uint64_t)n;
  dg_context hc = {DG_CTX_VV, 0, &n0, &c0, 1, 1};
  DG(dgr_state_load(g, &hs, &hc, &s));
  const uint64_t version = dgr_state_version(s);

  /* the state's keys in k + 1 interleaved classes of n / (k + 1): class k is the shared core,
   * class j < k keyset j's own keys */
  const int64_t stride = n / m / (k + 1) * (k + 1);
  CHECK(stride >= k + 1);
  uint64_t* sets[N_CASES][MAXK];
  const uint64_t* views[N_CASES][MAXK];
  uint64_t nk[MAXK];
  const int64_t shared = m * 8 / 10;
  for (int j = 0; j < k; j++) {
    nk[j] = (uint64_t)m;
    sets[C_IDENT][j] = malloc((size_t)m * 8);
    sets[C_SHARED][j] = malloc((size_t)m * 8);
    for (int64_t i = 0; i < m; i++) {
      sets[C_IDENT][j][i] = key[i * stride + k];
      sets[C_SHARED][j][i] = key[i * stride + (i < shared ? k : j)];
    }
    for (int c = 0; shuffle && c < N_CASES; c++)
      for (int64_t i = m - 1; i > 0; i--) { /* Fisher-Yates on the hash of (case, set, i) */
        const int64_t o = (int64_t)(mix((uint64_t)(c * MAXK + j) << 32 | (uint64_t)i) % (uint64_t)(i + 1));
        const uint64_t x = sets[c][j][i];
        sets[c][j][i] = sets[c][j][o];
        sets[c][j][o] = x;
      }
    views[C_IDENT][j] = sets[C_IDENT][j];
    views[C_SHARED][j] = sets[C_SHARED][j];
  }

  double* t_take[N_CASES];
  double* t_batch[N_CASES];
  double* t_pack[N_CASES];
  uint64_t* pack_host = malloc((size_t)dgr_takes_words(k, nk) * 8 + 8);
  uint64_t* pack_dev = malloc((size_t)dgr_takes_words(k, nk) * 8 + 8); /* (only its addresses are used) */
  const uint64_t* pack_v[MAXK];
  uint64_t pack_n[MAXK];
  uint64_t bytes_take[N_CASES] = {0}, bytes_batch[N_CASES] = {0}, n_union[N_CASES] = {0};
  uint64_t rows_of_set[MAXK];
  for (int c = 0; c < N_CASES; c++) {
    t_take[c] = malloc((size_t)reps * sizeof(double));
    t_batch[c] = malloc((size_t)reps * sizeof(double));
    t_pack[c] = malloc((size_t)reps * sizeof(double));
  }
  const int warm = 3;
  for (int r = -warm; r < reps; r++) {
    for (int c = 0; c < N_CASES; c++) {
      uint64_t b = 0;
      double t0 = now_us();
      for (int j = 0; j < k; j++) {
        dg_store out;
        DG(dgr_take(s, version, views[c][j], nk[j], &out));
        rows_of_set[j] = out.n;
        b += out.n * 36;
      }
      const double dt_take = now_us() - t0;
      bytes_take[c] = b;
      dgr_taken tk;
      t0 = now_us();
      DG(dgr_take_batch(s, version, k, views[c], nk, &tk));
      const double dt_batch = now_us() - t0;
      CHECK(tk.offs[tk.n_keys] == tk.rows.n); /* the union's rows came home once */
      bytes_batch[c] = tk.rows.n * 36 + tk.n_keys * 24 + 8;
      n_union[c] = tk.n_keys;
      for (int j = 0; j < k; j++) {
        uint64_t rows = 0;
        for (uint64_t i = 0; i < tk.n_keys; i++)
          if (tk.masks[i] >> j & 1) rows += tk.offs[i + 1] - tk.offs[i];
        CHECK(rows == rows_of_set[j]);
      }
      t0 = now_us();
      dgr_takes_pack(pack_host, pack_dev, k, views[c], nk, pack_v, pack_n);
      const double dt_pack = now_us() - t0;
      if (r >= 0) {
        t_take[c][r] = dt_take;
        t_batch[c][r] = dt_batch;
        t_pack[c][r] = dt_pack;
      }
    }
  }
  CHECK(dgr_state_version(s) == version);
  printf("{\"n_keys\": %lld, \"keyset\": %lld, \"k\": %d, \"reps\": %d, \"shuffle\": %d, \"unit\": \"us_median\"", (long long)n,
         (long long)m, k, reps, shuffle);
  for (int c = 0; c < N_CASES; c++)
    printf(", \"%s\": {\"k_takes_us\": %.1f, \"take_batch_us\": %.1f, \"host_pack_us\": %.1f, \"union_keys\": %llu, \"k_takes_bytes\": %llu, "
           "\"take_batch_bytes\": %llu}",
           CASE_NAMES[c], median(t_take[c], reps), median(t_batch[c], reps), median(t_pack[c], reps),
           (unsigned long long)n_union[c],
           (unsigned long long)bytes_take[c], (unsigned long long)bytes_batch[c]);
  printf("}\n");
  dgr_state_free(s);
  dgr_engine_close(g);
  return 0;
}
