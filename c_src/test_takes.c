/*
 * test_takes.c — the packed message of a batch of keysets (replica.h dgr_takes_words /
 * dgr_takes_pack) on the host: every keyset sorted and unique at its documented 16-byte
 * aligned offset, the device views naming the same places, no keyset leaving the message or
 * overlapping another, and the word count the sizing function's.
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

#define MAXK 64
#define MAXN 70

static uint64_t even(uint64_t w) { return (w + 1) & ~UINT64_C(1); }

/* order 0: descending, every third key twice, the largest id among them (any order, duplicates
 * allowed: the sorted path); 1: ascending and unique already (the copied path); 2: ascending
 * but for one equal pair at the end (sorted again) */
static void run(int k, const uint64_t* n_keys, int order) {
  static uint64_t ks[MAXK][MAXN];
  const uint64_t* keys[MAXK];
  for (int i = 0; i < k; i++) {
    for (uint64_t j = 0; j < n_keys[i]; j++)
      ks[i][j] = order ? 7 * j + (uint64_t)i : 5 * ((n_keys[i] - j) / 3 * 3) + (uint64_t)i;
    if (!order && n_keys[i] > 4) ks[i][2] = UINT64_MAX;
    if (order == 1 && n_keys[i] > 1) ks[i][n_keys[i] - 1] = UINT64_MAX;
    if (order == 2 && n_keys[i] > 1) ks[i][n_keys[i] - 1] = ks[i][n_keys[i] - 2];
    keys[i] = n_keys[i] ? ks[i] : NULL;
  }
  const uint64_t words = dgr_takes_words(k, n_keys);
  /* the message exactly as long as dgr_takes_words says (a write past it is a heap overrun) */
  uint64_t* host = (uint64_t*)malloc((words ? words : 1) * 8);
  uint64_t* dev = (uint64_t*)malloc((words ? words : 1) * 8); /* (stands for the device copy: only its addresses are used) */
  memset(host, 0xee, (words ? words : 1) * 8);
  const uint64_t* kv[MAXK];
  uint64_t nk[MAXK];
  const uint64_t got = dgr_takes_pack(host, dev, k, keys, n_keys, kv, nk);
  CHECK(got == words, "packed %llu words, dgr_takes_words says %llu", (unsigned long long)got,
        (unsigned long long)words);
  uint64_t want = 0; /* the offsets, restated: keyset i behind the even word counts of those before */
  for (int i = 0; i < k; i++) {
    CHECK(kv[i] == dev + want, "keyset %d: not at word %llu", i, (unsigned long long)want);
    CHECK(want % 2 == 0, "keyset %d: word offset %llu not 16-byte aligned", i, (unsigned long long)want);
    CHECK(want + nk[i] <= words, "keyset %d: ends at word %llu of %llu", i, (unsigned long long)(want + nk[i]),
          (unsigned long long)words);
    const uint64_t* hk = host + (kv[i] - dev); /* the host side of the view */
    uint64_t distinct = 0;
    for (uint64_t j = 0; j < n_keys[i]; j++) {
      int seen = 0;
      for (uint64_t l = 0; l < j; l++) seen |= ks[i][l] == ks[i][j];
      distinct += !seen;
      int found = 0;
      for (uint64_t l = 0; l < nk[i]; l++) found |= hk[l] == ks[i][j];
      CHECK(found, "keyset %d: key %llu lost", i, (unsigned long long)ks[i][j]);
    }
    CHECK(nk[i] == distinct, "keyset %d: %llu keys of %llu distinct", i, (unsigned long long)nk[i],
          (unsigned long long)distinct);
    for (uint64_t l = 1; l < nk[i]; l++)
      CHECK(hk[l - 1] < hk[l], "keyset %d: not ascending at %llu", i, (unsigned long long)l);
    want += even(n_keys[i]); /* (the next keyset starts behind this one's room: no overlap) */
  }
  CHECK(want == words, "the keysets end at word %llu of %llu", (unsigned long long)want, (unsigned long long)words);
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
        /* three keysets whose sizes walk the list from different starts, then an empty one */
        const uint64_t nk[4] = {sizes[a], sizes[(a + b) % ns], sizes[(b + c) % ns], 0};
        run(4, nk, (a + b + c) % 3);
        cases++;
      }
  uint64_t many[MAXK];
  for (int i = 0; i < MAXK; i++) many[i] = sizes[i % ns];
  for (int order = 0; order < 3; order++) run(MAXK, many, order); /* the most keysets one call takes */
  const uint64_t z[2] = {0, 0};
  run(0, z, 0);
  run(1, z, 1);
  run(2, z, 0); /* only empty keysets: an empty message */
  printf("takes packing: %ld cases, %d failures\n", cases + 6, g_fail);
  return g_fail ? 1 : 0;
}
