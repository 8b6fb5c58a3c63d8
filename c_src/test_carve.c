/*
 * test_carve.c — the output carve of dgr_merkle_continue_batch (replica_pack.h
 * rp_cont_room_for / rp_cont_carve / rp_cont_room_out / rp_cont_room_keys): for k = 1 .. 64
 * hops at and around dg_merkle_continue_home's limits, every hop's pos, hash, bucket and keys
 * regions are 8-byte aligned, inside the block, disjoint from one another and from every other
 * hop's, and as large as the formulas a single hop is given -- restated here literally.  Every
 * word of every region is written with its hop's number and read back, so a region that left
 * the allocation or met another is a sanitizer report or a wrong word.
 * A plain executable with its own main; it calls host code only (no device is opened).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "replica_pack.h"

static int g_fail = 0, g_cases = 0;
#define CHECK(c, ...)                             \
  do {                                            \
    if (!(c)) {                                   \
      g_fail++;                                   \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                        \
      printf("\n");                               \
    }                                             \
  } while (0)
#define LL(x) ((unsigned long long)(x))

static uint64_t mn(uint64_t a, uint64_t b) { return a < b ? a : b; }
static uint64_t mx(uint64_t a, uint64_t b) { return a > b ? a : b; }

typedef struct {
  uint32_t level;
  uint64_t n;
} hop_in;

/* continue_small's formulas, as they stood before they were stated in replica_pack.h */
static void want_room(uint32_t level, uint64_t n, uint32_t depth, uint32_t levels, uint64_t max_sync, uint64_t rows_n,
                      uint64_t* C, uint64_t* CB, uint64_t* kcap) {
  *CB = mx(mn(n, max_sync), 1);
  if (level < depth) {
    const uint32_t k = levels < depth - level ? levels : depth - level;
    *C = mn(n << k, max_sync);
  } else {
    *C = mx(4 * mn(n, max_sync), 64);
  }
  *C = mx(*C, 1);
  *kcap = mx(mn(mn(max_sync, rows_n + n + 1), 65536), 1);
}

static void one_batch(int k, const hop_in* in, uint32_t depth, uint32_t levels, uint64_t max_sync, uint64_t rows_n) {
  rp_cont_room room[DG_CONT_BATCH_MAX];
  uint64_t off[DG_CONT_BATCH_MAX + 1];
  g_cases++;
  uint64_t sum = 0;
  for (int j = 0; j < k; j++) {
    room[j] = rp_cont_room_for(in[j].level, in[j].n, depth, levels, max_sync, rows_n);
    uint64_t C, CB, kcap;
    want_room(in[j].level, in[j].n, depth, levels, max_sync, rows_n, &C, &CB, &kcap);
    CHECK(room[j].C == C && room[j].CB == CB && room[j].kcap == kcap,
          "hop %d (level %u, n %llu): room %llu / %llu / %llu, want %llu / %llu / %llu", j, in[j].level, LL(in[j].n),
          LL(room[j].C), LL(room[j].CB), LL(room[j].kcap), LL(C), LL(CB), LL(kcap));
    sum += 2 * C + CB + kcap;
  }
  const uint64_t words = rp_cont_carve(k, room, off);
  CHECK(words == sum && off[k] == words, "k %d: %llu words, the rooms sum to %llu", k, LL(words), LL(sum));
  uint64_t* block = (uint64_t*)malloc(mx(words, 1) * 8); /* exactly the carve: a sanitizer sees one word more */
  if (!block) {
    CHECK(0, "malloc of %llu words", LL(words));
    return;
  }
  for (int j = 0; j < k; j++) {
    const dg_merkle_cont c = rp_cont_room_out(block, off[j], room[j]);
    uint64_t* keys = rp_cont_room_keys(block, off[j], room[j]);
    uint64_t* part[4] = {c.pos, c.hash, c.bucket, keys};
    const uint64_t len[4] = {room[j].C, room[j].C, room[j].CB, room[j].kcap};
    CHECK(c.cap == room[j].C && c.cap_buckets == room[j].CB && c.n == 0 && c.n_buckets == 0, "hop %d: capacities", j);
    for (int q = 0; q < 4; q++) {
      const uint64_t o = (uint64_t)((char*)part[q] - (char*)block);
      CHECK(o % 8 == 0, "hop %d part %d: byte offset %llu not 8-byte aligned", j, q, LL(o));
      CHECK(o / 8 >= off[j] && o / 8 + len[q] <= off[j + 1], "hop %d part %d: [%llu, %llu) outside [%llu, %llu)", j, q,
            LL(o / 8), LL(o / 8 + len[q]), LL(off[j]), LL(off[j + 1]));
      for (int p = 0; p < q; p++) {
        const uint64_t o2 = (uint64_t)((char*)part[p] - (char*)block) / 8;
        CHECK(o / 8 + len[q] <= o2 || o2 + len[p] <= o / 8, "hop %d: part %d overlaps part %d", j, q, p);
      }
      for (uint64_t i = 0; i < len[q]; i++) part[q][i] = ((uint64_t)j << 8) | (uint64_t)q;
    }
  }
  /* read back: every word holds the last writer's mark, and that is its own region's */
  for (int j = 0; j < k; j++) {
    const dg_merkle_cont c = rp_cont_room_out(block, off[j], room[j]);
    uint64_t* part[4] = {c.pos, c.hash, c.bucket, rp_cont_room_keys(block, off[j], room[j])};
    const uint64_t len[4] = {room[j].C, room[j].C, room[j].CB, room[j].kcap};
    for (int q = 0; q < 4; q++) {
      uint64_t bad = 0;
      for (uint64_t i = 0; i < len[q]; i++) bad += part[q][i] != (((uint64_t)j << 8) | (uint64_t)q);
      CHECK(bad == 0, "hop %d part %d: %llu words overwritten", j, q, LL(bad));
    }
  }
  free(block);
}

int main(void) {
  const uint32_t depth = 12;
  /* hops at the limits: the most entries, one entry, none; below, at and (leaf form) past the buckets */
  const hop_in kinds[] = {{3, 8},  {12, DG_CONT_HOME_ENTRIES}, {13, DG_CONT_HOME_ENTRIES}, {9, DG_CONT_HOME_ENTRIES},
                          {12, 1}, {13, 0},                    {0, 1},                     {11, 4095},
                          {8, 256}, {12, 513}};
  const int nkinds = (int)(sizeof kinds / sizeof kinds[0]);
  const uint64_t maxes[] = {UINT64_MAX, 200, 5, 1, 65536, 65537};
  const uint32_t lvls[] = {1, 3, 8, 12};
  const uint64_t rows[] = {0, 3000, 12500000};
  hop_in in[DG_CONT_BATCH_MAX];
  for (int k = 1; k <= DG_CONT_BATCH_MAX; k++)
    for (unsigned a = 0; a < sizeof maxes / sizeof maxes[0]; a++)
      for (unsigned b = 0; b < sizeof lvls / sizeof lvls[0]; b++) {
        /* every (max_sync, levels) at the ends of k, one pair per k between them */
        if (k > 2 && k < DG_CONT_BATCH_MAX - 1 && (a != (unsigned)k % 6 || b != (unsigned)k % 4)) continue;
        for (int j = 0; j < k; j++) in[j] = kinds[(j + k) % nkinds];
        one_batch(k, in, depth, lvls[b], maxes[a], rows[(a + b) % 3]);
      }
  /* 64 hops of the largest room a hop is given here (C = RP_CONT_SMALL_OUT) */
  for (int j = 0; j < DG_CONT_BATCH_MAX; j++) in[j] = (hop_in){4, DG_CONT_HOME_ENTRIES};
  one_batch(DG_CONT_BATCH_MAX, in, depth, 8, 65536, 12500000);
  printf("%d cases, %d failures\n", g_cases, g_fail);
  return g_fail != 0;
}
