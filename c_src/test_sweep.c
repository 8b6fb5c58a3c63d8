/*
 * test_sweep.c — the universe's sweeps (marshal.c dgm_sweep_values / dgm_sweep_keys), host
 * only: no device, no libdeltagpu.
 *
 *   1. a flag array of the wrong length is refused (DG_E_INVAL) and nothing is dropped;
 *   2. keeps minus drops equals the live entries after every step (counting keep / drop ops:
 *      a term dropped twice or never would show here, and as a leak or a double free under
 *      the sanitizer build, `make _build/test_sweep_asan`);
 *   3. survivors keep ids, terms and hashes; dropped ids are unknown; a dropped term interned
 *      again lands between its neighbours;
 *   4. keys: the sorted table, the sweep, and every lookup after the map's rebuild;
 *   5. the sequence "intern 3000 values, sweep two thirds, intern 500 more": the ids are
 *      printed ("ID <index> <id>") and tests/test_marshal_sweep.py compares them with the
 *      Python Universe's for the same sequence (the same midpoint / stride choice).
 *
 * Value i of that sequence is the float x / 7 when i % 3 == 0, else the binary "s%08x" of x,
 * x = (i * 2654435761) mod 2^32.  Exit status 0 = pass.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "marshal.h"

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

enum { T_INT = 0, T_FLOAT = 1, T_BIN = 3 };
typedef struct {
  int kind;
  int64_t i;
  double f;
  char s[24];
} tterm;

static int cls(const tterm* t) { return t->kind <= T_FLOAT ? 0 : 10; }

static int tcmp(const void* pa, const void* pb, void* ud) {
  (void)ud;
  const tterm *a = (const tterm*)pa, *b = (const tterm*)pb;
  if (cls(a) != cls(b)) return cls(a) < cls(b) ? -1 : 1;
  if (cls(a) == 0) { /* map-key order: every integer before every float */
    if (a->kind != b->kind) return a->kind == T_INT ? -1 : 1;
    if (a->kind == T_INT) return a->i < b->i ? -1 : a->i > b->i;
    return a->f < b->f ? -1 : a->f > b->f;
  }
  return strcmp(a->s, b->s) < 0 ? -1 : strcmp(a->s, b->s) > 0 ? 1 : 0;
}

static int tenc(const void* p, dgm_buf* b, void* ud) {
  (void)ud;
  const tterm* t = (const tterm*)p;
  switch (t->kind) {
    case T_INT: return dgm_enc_i64(b, t->i);
    case T_FLOAT: return dgm_enc_float(b, t->f);
    default: return dgm_enc_binary(b, t->s, strlen(t->s));
  }
}

static long n_keep, n_drop;

static void* tkeep(const void* t, void* ud) {
  (void)ud;
  tterm* c = (tterm*)malloc(sizeof *c);
  memcpy(c, t, sizeof *c);
  n_keep++;
  return c;
}
static void tdrop(void* t, void* ud) {
  (void)ud;
  n_drop++;
  free(t);
}

static tterm seq_value(uint64_t i) {
  tterm t;
  memset(&t, 0, sizeof t);
  const uint64_t x = (i * 2654435761ull) & 0xFFFFFFFFull;
  if (i % 3 == 0) {
    t.kind = T_FLOAT;
    t.f = (double)x / 7.0;
  } else {
    t.kind = T_BIN;
    snprintf(t.s, sizeof t.s, "s%08x", (unsigned)x);
  }
  return t;
}

static tterm key_term_of(uint64_t i) {
  tterm t;
  memset(&t, 0, sizeof t);
  if (i % 2 == 0) {
    t.kind = T_INT;
    t.i = (int64_t)(i * 7919);
  } else {
    t.kind = T_BIN;
    snprintf(t.s, sizeof t.s, "k%llu", (unsigned long long)i);
  }
  return t;
}

static uint64_t value_id(dgm_universe* u, const tterm* t) {
  uint64_t id = 0;
  CHECK(dgm_value(u, t, &id, NULL) == DG_OK);
  return id;
}

/* the table (ascending ids) follows term order and holds no repeat */
static void check_table(const dgm_universe* u) {
  const uint64_t *ids, *hash;
  uint64_t n;
  dgm_value_hashes(u, &ids, &hash, &n);
  CHECK(n == dgm_value_count(u));
  for (uint64_t j = 0; j + 1 < n; j++) {
    CHECK(ids[j] < ids[j + 1]);
    CHECK(tcmp(dgm_value_term(u, ids[j]), dgm_value_term(u, ids[j + 1]), NULL) < 0);
  }
}

static uint64_t pos_of(const uint64_t* ids, uint64_t n, uint64_t id) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) / 2;
    if (ids[mid] < id)
      lo = mid + 1;
    else
      hi = mid;
  }
  CHECK(lo < n && ids[lo] == id);
  return lo;
}

enum { N1 = 3000, N2 = 500 };

static void test_values(void) {
  const dgm_term_ops ops = {tcmp, tenc, NULL, tkeep, tdrop, NULL};
  dgm_universe* u = dgm_universe_new(&ops);
  CHECK(u);
  for (uint64_t i = 0; i < N1; i++) {
    const tterm t = seq_value(i);
    value_id(u, &t);
  }
  CHECK(dgm_value_count(u) == N1);
  CHECK(n_keep - n_drop == N1);
  check_table(u);
  /* the ids now (a relabel may have moved early ones), the terms' hashes */
  static uint64_t id1[N1], h1[N1];
  const uint64_t *ids, *hash;
  uint64_t n;
  dgm_value_hashes(u, &ids, &hash, &n);
  for (uint64_t i = 0; i < N1; i++) {
    const tterm t = seq_value(i);
    id1[i] = value_id(u, &t);
    h1[i] = hash[pos_of(ids, n, id1[i])];
  }
  CHECK(dgm_value_count(u) == N1 && n_keep - n_drop == N1); /* looking up interned nothing */

  /* 1. a wrong length: refused, nothing dropped */
  static uint8_t used[N1 + 1];
  memset(used, 0, sizeof used);
  uint64_t dropped = 77;
  CHECK(dgm_sweep_values(u, used, N1 - 1, &dropped) == DG_E_INVAL && dropped == 0);
  CHECK(dgm_sweep_values(u, used, N1 + 1, &dropped) == DG_E_INVAL && dropped == 0);
  CHECK(dgm_sweep_values(u, NULL, N1, &dropped) == DG_E_INVAL);
  CHECK(dgm_value_count(u) == N1 && n_drop == 0);

  /* sweep two thirds: value i survives iff i % 3 == 1 */
  for (uint64_t i = 0; i < N1; i++) used[pos_of(ids, n, id1[i])] = i % 3 == 1;
  CHECK(dgm_sweep_values(u, used, N1, &dropped) == DG_OK);
  CHECK(dropped == N1 - N1 / 3 && dgm_value_count(u) == N1 / 3);
  CHECK(n_drop == (long)dropped && n_keep - n_drop == N1 / 3);
  check_table(u);
  dgm_value_hashes(u, &ids, &hash, &n);
  for (uint64_t i = 0; i < N1; i++) {
    const tterm t = seq_value(i);
    const tterm* got = (const tterm*)dgm_value_term(u, id1[i]);
    if (i % 3 == 1) {
      CHECK(got && tcmp(got, &t, NULL) == 0);
      CHECK(hash[pos_of(ids, n, id1[i])] == h1[i]);
    } else {
      CHECK(got == NULL);
    }
  }
  for (uint64_t i = 0; i < N1; i++)
    if (i % 3 == 1) {
      const tterm t = seq_value(i);
      CHECK(value_id(u, &t) == id1[i]); /* a survivor keeps its id */
    }
  CHECK(dgm_value_count(u) == N1 / 3);
  /* a second sweep with every flag set drops nothing */
  memset(used, 1, sizeof used);
  CHECK(dgm_sweep_values(u, used, N1 / 3, &dropped) == DG_OK && dropped == 0);
  /* an empty flag array on a table that is not empty is a mismatch */
  CHECK(dgm_sweep_values(u, used, 0, &dropped) == DG_E_INVAL);

  /* 500 more: new terms and dropped ones interned again, each between its neighbours */
  for (uint64_t i = 0; i < N2; i++) {
    const tterm t = seq_value(i % 2 ? N1 + i : 3 * i); /* 3 * i: dropped above (i % 3 == 0) */
    value_id(u, &t);
  }
  check_table(u);
  CHECK((uint64_t)(n_keep - n_drop) == dgm_value_count(u));
  for (uint64_t i = 0; i < N1 + N2; i++) {
    const tterm t = seq_value(i);
    const uint64_t before = dgm_value_count(u);
    int eq = 0;
    /* print only what the table holds: looked up through the sorted ids, not interned */
    dgm_value_hashes(u, &ids, &hash, &n);
    for (uint64_t lo = 0, hi = n; lo < hi;) {
      const uint64_t mid = (lo + hi) / 2;
      const int c = tcmp(dgm_value_term(u, ids[mid]), &t, NULL);
      if (c == 0) {
        printf("ID %llu %llu\n", (unsigned long long)i, (unsigned long long)ids[mid]);
        eq = 1;
        break;
      }
      if (c < 0)
        lo = mid + 1;
      else
        hi = mid;
    }
    (void)eq;
    CHECK(dgm_value_count(u) == before);
  }
  const long live = n_keep - n_drop;
  dgm_universe_free(u);
  CHECK(n_keep - n_drop == 0 && live > 0);
}

enum { NK = 1000 };

static void test_keys(void) {
  n_keep = n_drop = 0;
  const dgm_term_ops ops = {tcmp, tenc, NULL, tkeep, tdrop, NULL};
  dgm_universe* u = dgm_universe_new(&ops);
  CHECK(u);
  static uint64_t kid[NK];
  for (uint64_t i = 0; i < NK; i++) {
    const tterm t = key_term_of(i);
    CHECK(dgm_key(u, &t, &kid[i]) == DG_OK);
  }
  CHECK(dgm_key_count(u) == NK && n_keep == NK);
  const uint64_t* sorted;
  uint64_t n;
  CHECK(dgm_key_ids_sorted(u, &sorted, &n) == DG_OK && n == NK);
  for (uint64_t j = 0; j + 1 < n; j++) CHECK(sorted[j] < sorted[j + 1]);
  static uint8_t used[NK];
  uint64_t dropped = 5;
  memset(used, 1, sizeof used);
  CHECK(dgm_sweep_keys(u, sorted, used, NK - 1, &dropped) == DG_E_INVAL && dropped == 0);
  { /* a table that lacks one of the keys: refused, nothing dropped */
    static uint64_t wrong[NK];
    memcpy(wrong, sorted, sizeof wrong);
    wrong[NK - 1] += 1;
    memset(used, 0, sizeof used);
    CHECK(dgm_sweep_keys(u, wrong, used, NK, &dropped) == DG_E_INVAL);
    CHECK(dgm_key_count(u) == NK && n_drop == 0);
  }
  /* key i survives iff i % 4 != 0 */
  for (uint64_t i = 0; i < NK; i++) used[pos_of(sorted, n, kid[i])] = i % 4 != 0;
  CHECK(dgm_sweep_keys(u, sorted, used, NK, &dropped) == DG_OK);
  CHECK(dropped == NK / 4 && dgm_key_count(u) == NK - NK / 4);
  CHECK(n_drop == NK / 4 && (uint64_t)(n_keep - n_drop) == dgm_key_count(u));
  for (uint64_t i = 0; i < NK; i++) { /* every lookup goes through the rebuilt map */
    const tterm t = key_term_of(i);
    const tterm* got = (const tterm*)dgm_key_term(u, kid[i]);
    if (i % 4 != 0)
      CHECK(got && tcmp(got, &t, NULL) == 0);
    else
      CHECK(got == NULL);
  }
  for (uint64_t i = 0; i < NK; i++) { /* survivors are found, dropped keys interned afresh */
    const tterm t = key_term_of(i);
    uint64_t id = 0;
    CHECK(dgm_key(u, &t, &id) == DG_OK && id == kid[i]);
  }
  CHECK(dgm_key_count(u) == NK && (uint64_t)(n_keep - n_drop) == NK);
  CHECK(dgm_key_ids_sorted(u, &sorted, &n) == DG_OK && n == NK);
  for (uint64_t j = 0; j + 1 < n; j++) CHECK(sorted[j] < sorted[j + 1]);
  /* sweep everything, then an empty universe sweeps to nothing */
  memset(used, 0, sizeof used);
  CHECK(dgm_sweep_keys(u, sorted, used, NK, &dropped) == DG_OK && dropped == NK);
  CHECK(dgm_key_count(u) == 0 && n_keep - n_drop == 0);
  CHECK(dgm_key_ids_sorted(u, &sorted, &n) == DG_OK && n == 0);
  CHECK(dgm_sweep_keys(u, sorted, used, 0, &dropped) == DG_OK && dropped == 0);
  CHECK(dgm_sweep_values(u, used, 0, &dropped) == DG_OK && dropped == 0);
  const tterm t = key_term_of(3);
  uint64_t id = 0;
  CHECK(dgm_key(u, &t, &id) == DG_OK && id == kid[3]);
  dgm_universe_free(u);
  CHECK(n_keep - n_drop == 0);
}

int main(void) {
  test_values();
  test_keys();
  printf("test_sweep: ok\n");
  return 0;
}
