/*
 * test_mutate_pack.c — the packed message of a batch of ops (replica.h dgr_mutate_words /
 * dgr_mutate_pack) on the host: the ops stably sorted by key whatever their batch order, equal
 * keys keeping batch order, every add's rank the adds before it in the batch, a remove's value
 * and ts zero, the kinds as bytes behind the four columns, nothing written past the message;
 * at m = 0, 1, 512 and 513 (dg_mutate_home's limit and one more) and a few sizes between.
 * A plain executable with its own main; it calls host code only (no device is opened).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "replica.h"

static int g_fail = 0;
#define CHECK(c, ...)                             \
  do {                                            \
    if (!(c)) {                                   \
      if (g_fail++ < 20) {                        \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                      \
        printf("\n");                             \
      }                                           \
    }                                             \
  } while (0)

#define GUARD UINT64_C(0x5a5a5a5a5a5a5a5a)

/* m ops over n_keys distinct keys; order 0: keys descending in the batch, 1: ascending, 2: a
 * fixed scramble; every third op a remove */
static void run(uint64_t m, uint64_t n_keys, int order) {
  uint8_t* kind = (uint8_t*)malloc(m + 1);
  uint64_t* key = (uint64_t*)malloc((m + 1) * 8);
  uint64_t* val = (uint64_t*)malloc((m + 1) * 8);
  int64_t* ts = (int64_t*)malloc((m + 1) * 8);
  const uint64_t words = dgr_mutate_words(m);
  CHECK(words == 4 * m + (m + 7) / 8, "words %llu for m %llu", (unsigned long long)words, (unsigned long long)m);
  uint64_t* host = (uint64_t*)malloc((words + 2) * 8); /* exactly the message and two guard words */
  for (uint64_t i = 0; i < m; i++) {
    const uint64_t k = order == 0 ? (m - 1 - i) % n_keys : order == 1 ? i % n_keys : (i * 7919 + 13) % n_keys;
    key[i] = (k + 1) * UINT64_C(0x9e3779b97f4a7c15); /* (wraps: ids over the whole range) */
    kind[i] = i % 3 != 2 ? (uint8_t)(1 + i % 2) : 0; /* any nonzero byte is an add */
    val[i] = 1000 + i;
    ts[i] = (int64_t)i - 7; /* batch position, and signed */
  }
  host[words] = host[words + 1] = GUARD;
  if (words) memset(host, 0xee, words * 8);
  uint64_t n_adds = ~UINT64_C(0);
  CHECK(dgr_mutate_pack(host, m, kind, key, val, ts, &n_adds) == DG_OK, "pack failed");
  CHECK(host[words] == GUARD && host[words + 1] == GUARD, "written past %llu words", (unsigned long long)words);
  const uint64_t *hk = host, *hv = host + m, *hr = host + 3 * m;
  const int64_t* ht = (const int64_t*)(host + 2 * m);
  const uint8_t* hkind = (const uint8_t*)(host + 4 * m);
  uint64_t adds = 0;
  for (uint64_t i = 0; i < m; i++) adds += kind[i] != 0;
  CHECK(n_adds == adds, "n_adds %llu, %llu adds", (unsigned long long)n_adds, (unsigned long long)adds);
  uint8_t* seen = (uint8_t*)calloc(m + 1, 1);
  for (uint64_t j = 0; j < m; j++) {
    CHECK(hkind[j] <= 1, "kind byte %u", hkind[j]);
    if (j) CHECK(hk[j - 1] <= hk[j], "keys out of order at %llu", (unsigned long long)j);
    /* the op's batch position: an add carries it in val and ts; a remove is found by its rank and key */
    uint64_t i = m;
    if (hkind[j]) {
      i = hv[j] - 1000;
      CHECK(i < m && ht[j] == (int64_t)i - 7, "op %llu: val %llu ts %lld", (unsigned long long)j,
            (unsigned long long)hv[j], (long long)ht[j]);
    } else {
      CHECK(hv[j] == 0 && ht[j] == 0, "a remove with val %llu ts %lld", (unsigned long long)hv[j], (long long)ht[j]);
      for (uint64_t q = 0; q < m && i == m; q++)
        if (!kind[q] && !seen[q] && key[q] == hk[j]) i = q; /* (its key's removes in batch order) */
    }
    if (i >= m) {
      CHECK(0, "op %llu is no op of the batch", (unsigned long long)j);
      continue;
    }
    CHECK(!seen[i], "op %llu twice", (unsigned long long)i);
    seen[i] = 1;
    CHECK(key[i] == hk[j] && (kind[i] != 0) == hkind[j], "op %llu: key or kind", (unsigned long long)i);
    uint64_t before = 0;
    for (uint64_t q = 0; q < i; q++) before += kind[q] != 0;
    CHECK(hr[j] == before, "op %llu: rank %llu, %llu adds before it", (unsigned long long)i,
          (unsigned long long)hr[j], (unsigned long long)before);
    /* equal keys keep batch order: ranks never descend inside a key group, and an add's
     * position (its ts) ascends */
    if (j && hk[j - 1] == hk[j]) {
      CHECK(hr[j - 1] <= hr[j], "batch order lost inside a key at %llu", (unsigned long long)j);
      if (hkind[j] && hkind[j - 1]) CHECK(ht[j - 1] < ht[j], "two adds of a key out of batch order");
    }
  }
  for (uint64_t i = 0; i < m; i++) CHECK(seen[i], "op %llu missing", (unsigned long long)i);
  free(seen), free(host), free(kind), free(key), free(val), free(ts);
}

int main(void) {
  const uint64_t M[] = {0, 1, 2, 3, 7, 8, 9, 64, 300, 511, 512, 513};
  long cases = 0;
  for (unsigned a = 0; a < sizeof M / sizeof *M; a++)
    for (int order = 0; order < 3; order++) {
      const uint64_t m = M[a];
      const uint64_t NK[] = {1, 3, m / 2 + 1, m ? m : 1};
      for (unsigned b = 0; b < 4; b++) {
        run(m, NK[b], order);
        cases++;
      }
    }
  printf("%ld cases, %d failures\n", cases, g_fail);
  return g_fail ? 1 : 0;
}
