/*
 * test_batch.c — the packed message of a batch of deltas (replica.h dgr_batch_words /
 * dgr_batch_pack) on the host: the offsets of every part, their 16-byte alignment, that no
 * two parts overlap and none leaves the message, the contents, and the keysets' sort-unique.
 * A plain executable with its own main; it calls host code only (no device is opened).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "replica.h"

static int g_fail = 0;
#define CHECK(c, ...)                         \
  do {                                        \
    if (!(c)) {                               \
      g_fail++;                               \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                    \
      printf("\n");                           \
    }                                         \
  } while (0)

#define MAXK 5
#define MAXN 70

typedef struct {
  const void* p;
  uint64_t bytes;
  const char* name;
} part;

static uint64_t even(uint64_t w) { return (w + 1) & ~UINT64_C(1); }

static void run(int k, const uint64_t* n_rows, const uint64_t* n_ctx, const uint64_t* n_keys) {
  static uint64_t key[MAXK][MAXN], val[MAXK][MAXN], cnt[MAXK][MAXN], ccnt[MAXK][MAXN], ks[MAXK][MAXN];
  static int64_t ts[MAXK][MAXN];
  static uint32_t node[MAXK][MAXN], cnode[MAXK][MAXN];
  dg_store deltas[MAXK];
  dg_context ctxs[MAXK];
  const uint64_t* keys[MAXK];
  for (int i = 0; i < k; i++) {
    for (uint64_t j = 0; j < n_rows[i]; j++) {
      key[i][j] = 1000 * (uint64_t)i + 7 * j + 1;
      val[i][j] = (UINT64_C(1) << 62) + j;
      ts[i][j] = (int64_t)j - 3;
      node[i][j] = (uint32_t)(i + 10 * j);
      cnt[i][j] = 100 + j;
    }
    for (uint64_t j = 0; j < n_ctx[i]; j++) {
      cnode[i][j] = (uint32_t)(50 + j);
      ccnt[i][j] = 9000 + 10 * (uint64_t)i + j;
    }
    /* descending, every third key twice: any order, duplicates allowed */
    for (uint64_t j = 0; j < n_keys[i]; j++) ks[i][j] = 5 * ((n_keys[i] - j) / 3 * 3) + (uint64_t)i;
    dg_store d = {key[i], val[i], ts[i], node[i], cnt[i], n_rows[i], n_rows[i]};
    dg_context c = {i % 2 ? DG_CTX_DOTS : DG_CTX_VV, 0, cnode[i], ccnt[i], n_ctx[i], n_ctx[i]};
    deltas[i] = d;
    ctxs[i] = c;
    keys[i] = n_keys[i] ? ks[i] : NULL;
  }
  const uint64_t words = dgr_batch_words(k, deltas, ctxs, n_keys);
  /* the message exactly as long as dgr_batch_words says (a write past it is a heap overrun) */
  uint64_t* host = (uint64_t*)malloc((words ? words : 1) * 8);
  uint64_t* dev = (uint64_t*)malloc((words ? words : 1) * 8); /* (stands for the device copy: only its addresses are used) */
  memset(host, 0xee, (words ? words : 1) * 8);
  dg_store rv[MAXK];
  dg_context cv[MAXK];
  const uint64_t* kv[MAXK];
  uint64_t nk[MAXK];
  const uint64_t got = dgr_batch_pack(host, dev, k, deltas, ctxs, keys, n_keys, rv, cv, kv, nk);
  CHECK(got == words, "packed %llu words, dgr_batch_words says %llu", (unsigned long long)got,
        (unsigned long long)words);
  part parts[MAXK * 8];
  int np = 0;
  uint64_t want = 0; /* the offsets, restated: 4 columns of even(n) words, node in even((n + 1) / 2) */
  for (int i = 0; i < k; i++) {
    const uint64_t n = n_rows[i], c = n_ctx[i], w = even(n), cw = even(c);
    CHECK(rv[i].n == n && rv[i].cap == n && cv[i].n == c && cv[i].kind == ctxs[i].kind, "delta %d: view sizes", i);
    CHECK(rv[i].key == dev + want && rv[i].val == dev + want + w && (uint64_t*)rv[i].ts == dev + want + 2 * w &&
              rv[i].cnt == dev + want + 3 * w && (uint64_t*)rv[i].node == dev + want + 4 * w,
          "delta %d: row columns not at word %llu", i, (unsigned long long)want);
    want += 4 * w + even((n + 1) / 2);
    CHECK(cv[i].cnt == dev + want && (uint64_t*)cv[i].node == dev + want + cw, "delta %d: context not at word %llu", i,
          (unsigned long long)want);
    want += cw + even((c + 1) / 2);
    CHECK(kv[i] == dev + want, "delta %d: keyset not at word %llu", i, (unsigned long long)want);
    want += even(n_keys[i]);
    part ps[8] = {{rv[i].key, n * 8, "key"},   {rv[i].val, n * 8, "val"},   {rv[i].ts, n * 8, "ts"},
                  {rv[i].cnt, n * 8, "cnt"},   {rv[i].node, n * 4, "node"}, {cv[i].cnt, c * 8, "ctx cnt"},
                  {cv[i].node, c * 4, "ctx node"}, {kv[i], nk[i] * 8, "keys"}};
    for (int q = 0; q < 8; q++) parts[np++] = ps[q];
    /* contents, read through the host side of each view */
#define HOST(p) ((const char*)host + ((const char*)(p) - (const char*)dev))
    CHECK(!n || (!memcmp(HOST(rv[i].key), key[i], n * 8) && !memcmp(HOST(rv[i].val), val[i], n * 8) &&
                 !memcmp(HOST(rv[i].ts), ts[i], n * 8) && !memcmp(HOST(rv[i].cnt), cnt[i], n * 8) &&
                 !memcmp(HOST(rv[i].node), node[i], n * 4)),
          "delta %d: rows differ", i);
    CHECK(!c || (!memcmp(HOST(cv[i].cnt), ccnt[i], c * 8) && !memcmp(HOST(cv[i].node), cnode[i], c * 4)),
          "delta %d: context differs", i);
    const uint64_t* hk = (const uint64_t*)HOST(kv[i]);
    uint64_t distinct = 0;
    for (uint64_t j = 0; j < n_keys[i]; j++) {
      int seen = 0;
      for (uint64_t l = 0; l < j; l++) seen |= ks[i][l] == ks[i][j];
      distinct += !seen;
      int found = 0;
      for (uint64_t l = 0; l < nk[i]; l++) found |= hk[l] == ks[i][j];
      CHECK(found, "delta %d: key %llu lost", i, (unsigned long long)ks[i][j]);
    }
    CHECK(nk[i] == distinct, "delta %d: %llu keys of %llu distinct", i, (unsigned long long)nk[i],
          (unsigned long long)distinct);
    for (uint64_t l = 1; l < nk[i]; l++) CHECK(hk[l - 1] < hk[l], "delta %d: keyset not ascending at %llu", i, (unsigned long long)l);
  }
  CHECK(want == words, "the parts end at word %llu of %llu", (unsigned long long)want, (unsigned long long)words);
  for (int a = 0; a < np; a++) {
    const uint64_t off = (uint64_t)((const char*)parts[a].p - (const char*)dev);
    CHECK(off % 16 == 0, "%s: byte offset %llu not 16-byte aligned", parts[a].name, (unsigned long long)off);
    CHECK(off + parts[a].bytes <= words * 8, "%s: ends at %llu of %llu bytes", parts[a].name,
          (unsigned long long)(off + parts[a].bytes), (unsigned long long)words * 8);
    for (int b = 0; b < a; b++) {
      const uint64_t o2 = (uint64_t)((const char*)parts[b].p - (const char*)dev);
      CHECK(!parts[a].bytes || !parts[b].bytes || off + parts[a].bytes <= o2 || o2 + parts[b].bytes <= off,
            "part %d (%s) overlaps part %d (%s)", a, parts[a].name, b, parts[b].name);
    }
  }
  free(host);
  free(dev);
}

int main(void) {
  const uint64_t sizes[] = {0, 1, 2, 3, 4, 5, 31, 32, 33, 64};
  const int ns = (int)(sizeof sizes / sizeof sizes[0]);
  long cases = 0;
  for (int a = 0; a < ns; a++)
    for (int b = 0; b < ns; b++)
      for (int c = 0; c < ns; c++) {
        /* three deltas whose sizes walk the list from different starts, then an empty one */
        const uint64_t nr[4] = {sizes[a], sizes[(a + b) % ns], sizes[(a + c) % ns], 0};
        const uint64_t nc[4] = {sizes[b], sizes[(b + c) % ns], sizes[a], 0};
        const uint64_t nk[4] = {sizes[c], sizes[a], sizes[(b + 1) % ns], 0};
        run(4, nr, nc, nk);
        cases++;
      }
  const uint64_t z[1] = {0};
  run(0, z, z, z);
  run(1, z, z, z);
  printf("batch packing: %ld cases, %d failures\n", cases + 2, g_fail);
  return g_fail ? 1 : 0;
}
