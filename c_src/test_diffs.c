/*
 * test_diffs.c — the term layer's half of on_diffs (marshal.c dgm_classify_diffs and
 * dgm_value_find), host only: no device, no libdeltagpu.
 *
 *   1. dgm_value_find: a term that was never interned is not found and is NOT interned by the
 *      lookup; an interned one gives dgm_value's id; a canonical integer its closed form; 1
 *      and 1.0 have different ids;
 *   2. dgm_classify_diffs over the full table of (old flag, new flag, old == new, old is nil,
 *      new is nil, nil never interned) against diffs_to_callback/3's case restated over
 *      optional values (causal_crdt.ex:368-374: Map.get gives nil for an absent key and for
 *      a nil value; {old, old} -> nothing, {_, nil} -> remove, else add).  Combinations that
 *      cannot occur are left out: equal values of which only one is nil, different values
 *      that are both nil, and a nil value when nil was never interned (no row can hold it);
 *      with nil never interned the nil id passed in is another value's, and must be ignored.
 *      Every row is printed ("ROW of nf old new hasnil nil kind") and
 *      tests/test_diffs_classify.py checks the Python helper behind nif.py against them.
 *
 * Exit status 0 = pass.  `make _build/test_diffs_asan` builds it with marshal.c under
 * AddressSanitizer and UBSan.
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

enum { T_INT = 0, T_FLOAT = 1, T_ATOM = 2, T_BIN = 3 };
typedef struct {
  int kind;
  int64_t i;
  double f;
  char s[24];
} tterm;

static int tcmp(const void* pa, const void* pb, void* ud) {
  (void)ud;
  const tterm *a = (const tterm*)pa, *b = (const tterm*)pb;
  if (a->kind != b->kind) return a->kind < b->kind ? -1 : 1; /* integers < floats < atoms < binaries */
  if (a->kind == T_INT) return a->i < b->i ? -1 : a->i > b->i;
  if (a->kind == T_FLOAT) return a->f < b->f ? -1 : a->f > b->f;
  return strcmp(a->s, b->s) < 0 ? -1 : strcmp(a->s, b->s) > 0 ? 1 : 0;
}

static int tenc(const void* p, dgm_buf* b, void* ud) {
  (void)ud;
  const tterm* t = (const tterm*)p;
  switch (t->kind) {
    case T_INT: return dgm_enc_i64(b, t->i);
    case T_FLOAT: return dgm_enc_float(b, t->f);
    case T_ATOM: return dgm_enc_atom(b, t->s, strlen(t->s));
    default: return dgm_enc_binary(b, t->s, strlen(t->s));
  }
}

static void* tkeep(const void* t, void* ud) {
  (void)ud;
  tterm* c = (tterm*)malloc(sizeof *c);
  memcpy(c, t, sizeof *c);
  return c;
}
static void tdrop(void* t, void* ud) {
  (void)ud;
  free(t);
}

static tterm mk(int kind, int64_t i, double f, const char* s) {
  tterm t;
  memset(&t, 0, sizeof t);
  t.kind = kind;
  t.i = i;
  t.f = f;
  if (s) snprintf(t.s, sizeof t.s, "%s", s);
  return t;
}

/* diffs_to_callback/3's case over optional values: has_* 0 is nil */
static uint8_t want_kind(int has_o, uint64_t o, int has_n, uint64_t n) {
  if (has_o == has_n && (!has_o || o == n)) return DGM_DIFF_NONE; /* {old, old} */
  if (!has_n) return DGM_DIFF_REMOVE;                             /* {_old, nil} */
  return DGM_DIFF_ADD;
}

int main(void) {
  const dgm_term_ops ops = {tcmp, tenc, NULL, tkeep, tdrop, NULL};
  dgm_universe* u = dgm_universe_new(&ops);
  CHECK(u);
  /* ---- 1. dgm_value_find */
  const tterm nil = mk(T_ATOM, 0, 0, "nil"), one = mk(T_INT, 1, 0, NULL), onef = mk(T_FLOAT, 0, 1.0, NULL);
  const tterm bin = mk(T_BIN, 0, 0, "v");
  uint64_t id = 77, nil_id = 0, a_id = 0, f_id = 0, i_id = 0;
  CHECK(dgm_value_find(u, &nil, &id) == 0 && id == 77);
  CHECK(dgm_value_count(u) == 0); /* the lookup interned nothing */
  CHECK(dgm_value_find(u, &one, &i_id) == 1 && i_id == (UINT64_C(1) << 62) + 1);
  CHECK(dgm_value(u, &bin, &a_id, NULL) == DG_OK);
  CHECK(dgm_value(u, &onef, &f_id, NULL) == DG_OK);
  CHECK(f_id != i_id); /* 1 and 1.0: different ids, as `{old, old}` does not match them */
  CHECK(dgm_value_find(u, &bin, &id) == 1 && id == a_id);
  CHECK(dgm_value_find(u, &onef, &id) == 1 && id == f_id);
  CHECK(dgm_value_find(u, &nil, &id) == 0);
  CHECK(dgm_value_count(u) == 2);
  CHECK(dgm_value(u, &nil, &nil_id, NULL) == DG_OK);
  CHECK(dgm_value_find(u, &nil, &id) == 1 && id == nil_id && dgm_value_count(u) == 3);
  CHECK(nil_id != a_id && nil_id != f_id);
  /* ---- 2. the table */
  uint64_t ov[64], nv[64];
  uint8_t fl[64], want[64], got[64];
  int hn[64];
  uint64_t nid[64];
  uint64_t n = 0;
  for (int hasnil = 0; hasnil < 2; hasnil++)
    for (int of = 0; of < 2; of++)
      for (int nf = 0; nf < 2; nf++)
        for (int eq = 0; eq < 2; eq++)
          for (int onil = 0; onil < 2; onil++)
            for (int nnil = 0; nnil < 2; nnil++) {
              if (eq && onil != nnil) continue;
              if (!eq && onil && nnil) continue;
              if (!hasnil && (onil || nnil)) continue;
              /* a value whose flag is clear is written as 0 (deltagpu.h) */
              const uint64_t o = !of ? 0 : (onil ? nil_id : a_id);
              const uint64_t w = !nf ? 0 : (nnil ? nil_id : (eq ? a_id : f_id));
              CHECK(n < 64);
              ov[n] = o;
              nv[n] = w;
              fl[n] = (uint8_t)((of ? DG_DIFF_OLD : 0) | (nf ? DG_DIFF_NEW : 0));
              hn[n] = hasnil;
              nid[n] = hasnil ? nil_id : a_id; /* never interned: the id passed is not nil's */
              want[n] = want_kind(of && !onil, o, nf && !nnil, w);
              n++;
            }
  CHECK(n == 28);
  for (uint64_t i = 0; i < n; i++) { /* one entry per call: has_nil varies by row */
    got[i] = 9;
    dgm_classify_diffs(ov + i, nv + i, fl + i, 1, hn[i], nid[i], got + i);
    printf("ROW %d %d %llu %llu %d %llu %d\n", (fl[i] & DG_DIFF_OLD) != 0, (fl[i] & DG_DIFF_NEW) != 0,
           (unsigned long long)ov[i], (unsigned long long)nv[i], hn[i], (unsigned long long)nid[i], got[i]);
    CHECK(got[i] == want[i]);
  }
  /* the rows with nil interned again as ONE call (n > 1, nothing written past n) */
  uint8_t many[65];
  memset(many, 9, sizeof many);
  uint64_t m = 0;
  for (uint64_t i = 0; i < n; i++)
    if (hn[i]) {
      ov[m] = ov[i], nv[m] = nv[i], fl[m] = fl[i], want[m] = want[i];
      m++;
    }
  dgm_classify_diffs(ov, nv, fl, m, 1, nil_id, many);
  for (uint64_t i = 0; i < m; i++) CHECK(many[i] == want[i]);
  CHECK(many[m] == 9);
  dgm_classify_diffs(ov, nv, fl, 0, 1, nil_id, many + m); /* n == 0: nothing */
  CHECK(many[m] == 9);
  /* every kind occurs */
  int seen[3] = {0, 0, 0};
  for (uint64_t i = 0; i < m; i++) seen[many[i]]++;
  CHECK(seen[DGM_DIFF_NONE] && seen[DGM_DIFF_ADD] && seen[DGM_DIFF_REMOVE]);
  dgm_universe_free(u);
  printf("test_diffs ok: %llu rows\n", (unsigned long long)n);
  return 0;
}
