/*
 * test_layout.c — the replica layer's host layouts (replica_pack.h): the return block's
 * regions as functions of (S, C) -- aligned, disjoint, inside the size function's figure, and
 * at the word offsets the kernels and the term layers know, restated here literally -- the
 * rows and context view constructors, the S that gives n bytes at the block's head, and the
 * continuation's byte frame.
 * A plain executable with its own main; it calls host code only (no device is opened).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "replica_pack.h"

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

typedef struct {
  const void* p;
  uint64_t bytes;
  const char* name;
} part;

#define LL(x) ((unsigned long long)(x))

/* every part 8-byte aligned and inside [b, b + words), no two overlapping */
static void check_parts(const uint64_t* b, uint64_t words, const part* ps, int np) {
  for (int i = 0; i < np; i++) {
    const uint64_t off = (uint64_t)((const char*)ps[i].p - (const char*)b);
    CHECK(off % 8 == 0, "%s: byte offset %llu not 8-byte aligned", ps[i].name, LL(off));
    CHECK(off + ps[i].bytes <= words * 8, "%s: ends at %llu of %llu bytes", ps[i].name, LL(off + ps[i].bytes),
          LL(words * 8));
    for (int j = 0; j < i; j++) {
      const uint64_t o2 = (uint64_t)((const char*)ps[j].p - (const char*)b);
      CHECK(off + ps[i].bytes <= o2 || o2 + ps[j].bytes <= off, "%s overlaps %s", ps[i].name, ps[j].name);
    }
  }
}

static void back_block(uint64_t S, uint64_t C) {
  const uint64_t words = rp_back_words(S, C);
  uint64_t* b = (uint64_t*)malloc(words * 8); /* only its addresses are used */
  const uint64_t* keys = rp_back_keys(b);
  const dg_store r = rp_back_rows(b, S);
  const dg_context c = rp_back_ctx(b, S, C);
  const dg_lww_diffs d = rp_back_diffs(b, S, C);
  CHECK(r.cap == S && r.n == 0 && c.cap == C && c.n == 0 && c.kind == DG_CTX_VV && d.cap == S,
        "S %llu C %llu: the views' n, cap or kind", LL(S), LL(C));
  const part ps[11] = {{keys, S * 8, "keys"},          {r.key, S * 8, "key"},         {r.val, S * 8, "val"},
                       {r.ts, S * 8, "ts"},            {r.cnt, S * 8, "cnt"},         {r.node, S * 4, "node"},
                       {c.cnt, C * 8, "ctx cnt"},      {c.node, C * 4, "ctx node"},   {d.old_val, S * 8, "diff old"},
                       {d.new_val, S * 8, "diff new"}, {d.flags, S, "diff flags"}};
  check_parts(b, words, ps, 11);
  /* today's offsets, restated: the kernels write them, nif.py and the NIF read views of them */
  CHECK(keys == b, "keys not at word 0");
  CHECK(r.key == b + S && r.val == b + 2 * S && r.ts == (int64_t*)(b + 3 * S) && r.cnt == b + 4 * S &&
            r.node == (uint32_t*)(b + 5 * S),
        "S %llu: row columns not at S, 2S, 3S, 4S, 5S", LL(S));
  CHECK(c.cnt == b + 6 * S && c.node == (uint32_t*)(b + 6 * S + C), "S %llu C %llu: context not at 6S, 6S + C",
        LL(S), LL(C));
  CHECK(d.old_val == b + 6 * S + 2 * C && d.new_val == b + 6 * S + 2 * C + S &&
            d.flags == (uint8_t*)(b + 6 * S + 2 * C + 2 * S),
        "S %llu C %llu: diffs not at 6S + 2C", LL(S), LL(C));
  free(b);
}

/* n rows and n context entries at `stride`: a distinct value through each field, read back
 * through the raw words in the column order key | val | ts | cnt | node, then cnt | node */
static void views(uint64_t n, uint64_t stride) {
  const uint64_t words = 5 * stride + 2 * stride;
  uint64_t* b = (uint64_t*)calloc(words + 1, 8);
  const dg_store r = rp_rows(b, stride, n, n + 1);
  const dg_context c = rp_ctx(b + 5 * stride, stride, DG_CTX_DOTS, n, n + 2);
  CHECK(r.n == n && r.cap == n + 1 && c.n == n && c.cap == n + 2 && c.kind == DG_CTX_DOTS && c.reserved == 0,
        "n %llu: the views' n, cap or kind", LL(n));
  const part ps[7] = {{r.key, n * 8, "key"},   {r.val, n * 8, "val"},     {r.ts, n * 8, "ts"},        {r.cnt, n * 8, "cnt"},
                      {r.node, n * 4, "node"}, {c.cnt, n * 8, "ctx cnt"}, {c.node, n * 4, "ctx node"}};
  check_parts(b, words, ps, 7);
  for (uint64_t i = 0; i < n; i++) {
    r.key[i] = 0x1000 + i;
    r.val[i] = 0x2000 + i;
    r.ts[i] = -(int64_t)(0x3000 + i);
    r.cnt[i] = 0x4000 + i;
    r.node[i] = (uint32_t)(0x5000 + i);
    c.cnt[i] = 0x6000 + i;
    c.node[i] = (uint32_t)(0x7000 + i);
  }
  const uint32_t* node = (const uint32_t*)(b + 4 * stride);
  const uint32_t* cnode = (const uint32_t*)(b + 6 * stride);
  for (uint64_t i = 0; i < n; i++) {
    CHECK(b[i] == 0x1000 + i && b[stride + i] == 0x2000 + i && (int64_t)b[2 * stride + i] == -(int64_t)(0x3000 + i) &&
              b[3 * stride + i] == 0x4000 + i && node[i] == 0x5000 + i,
          "n %llu stride %llu: row %llu not in the order key | val | ts | cnt | node", LL(n), LL(stride), LL(i));
    CHECK(b[5 * stride + i] == 0x6000 + i && cnode[i] == 0x7000 + i,
          "n %llu stride %llu: context entry %llu not in the order cnt | node", LL(n), LL(stride), LL(i));
  }
  free(b);
}

static void cont_frame(uint64_t n, uint64_t nb) {
  const uint64_t len = rp_cont_bytes(n, nb);
  CHECK(len == 20 + 16 * n + 8 * nb, "n %llu nb %llu: %llu bytes", LL(n), LL(nb), LL(len));
  uint8_t* bin = (uint8_t*)malloc(len + 8);
  memset(bin, 0xee, len + 8);
  uint8_t* data = rp_cont_write_head(bin, 7, n, nb);
  CHECK(data == bin + 20 && RP_CONT_HEAD == 20, "the data not behind the 20-byte header");
  uint32_t level = 0;
  uint64_t gn = 99, gnb = 99;
  CHECK(rp_cont_parse(bin, len, &level, &gn, &gnb) == DG_OK && level == 7 && gn == n && gnb == nb,
        "n %llu nb %llu: the header does not parse back", LL(n), LL(nb));
  /* a length off by one word either way, and an n larger than the length allows */
#define REJECTS(l, what) \
  CHECK(rp_cont_parse(bin, l, &level, &gn, &gnb) == DG_E_INVAL, "n %llu nb %llu: %s taken", LL(n), LL(nb), what)
  REJECTS(len + 8, "len + 8");
  if (n + nb) REJECTS(len - 8, "len - 8");
  rp_cont_write_head(bin, 7, (len - 20) / 16 + 1, nb);
  REJECTS(len, "n past the length");
  rp_cont_write_head(bin, 7, UINT64_MAX / 16 + 1 + n, nb); /* 16 n wraps round to today's len */
  REJECTS(len, "a wrapped n");
  CHECK(rp_cont_parse(bin, 19, &level, &gn, &gnb) == DG_E_INVAL, "a header of 19 bytes taken");
  /* the run behind a base: pos | hash | bucket, full */
  uint64_t* base = (uint64_t*)(void*)bin; /* (malloc's alignment) */
  const dg_merkle_cont c = rp_cont_at(base, 7, n, nb);
  CHECK(c.level == 7 && c.pos == base && c.hash == base + n && c.bucket == base + 2 * n && c.n == n && c.cap == n &&
            c.n_buckets == nb && c.cap_buckets == nb,
        "n %llu nb %llu: the continuation over a run", LL(n), LL(nb));
  free(bin);
}

int main(void) {
  long cases = 0;
  const uint64_t Ss[] = {64, 65, 127, 128, 1000}, Cs[] = {64, 65, 1023};
  for (int a = 0; a < 5; a++)
    for (int c = 0; c < 3; c++, cases++) back_block(Ss[a], Cs[c]);
  const uint64_t ns[] = {0, 1, 2, 5, 8, 33};
  for (int a = 0; a < 6; a++)
    for (uint64_t extra = 0; extra < 3; extra++, cases++) views(ns[a], ns[a] + extra);
  /* the head of the block (before the context region, which starts at the rows' cap S past
   * the keys' S words: 6 S words) holds n bytes, and S is (n + 47) / 48 as dgr_sweep had it */
  const uint64_t bytes[] = {0, 1, 47, 48, 49, 3071, 3072, 3073};
  for (int a = 0; a < 8; a++, cases++) {
    const uint64_t n = bytes[a], S = rp_back_s_for_bytes(n);
    uint64_t* b = (uint64_t*)malloc(rp_back_words(S, 64) * 8);
    const uint64_t head = (uint64_t)((const char*)rp_back_ctx(b, S, 64).cnt - (const char*)rp_back_keys(b));
    CHECK(head >= n, "%llu bytes: S %llu gives a head of %llu", LL(n), LL(S), LL(head));
    CHECK(S == (n + 47) / 48, "%llu bytes: S %llu, not %llu", LL(n), LL(S), LL((n + 47) / 48));
    free(b);
  }
  const uint64_t cn[] = {0, 1, 3};
  for (int a = 0; a < 3; a++)
    for (int c = 0; c < 3; c++, cases++) cont_frame(cn[a], cn[c]);
  printf("layouts: %ld cases, %d failures\n", cases, g_fail);
  return g_fail ? 1 : 0;
}
