/*
 * test_carve_take.c — the row rooms of dgr_merkle_continue_take_batch (replica_pack.h
 * rp_take_room_for / rp_take_carve / rp_take_room_rows / rp_take_room_offs) beside the output carve
 * of the batch (rp_cont_room_for / rp_cont_carve): for k = 1 .. 64 hops at dg_merkle_continue_home's
 * limits, max_sync of 1, 5, 200 and UINT64_MAX and a store of 0, a few and many rows, every hop's
 * five row columns and its offsets are 8-byte aligned, inside their block, disjoint from one another
 * and from every other hop's, and sized by the formulas -- restated here literally -- and the
 * existing regions (pos, hash, bucket, keys) are where they were.  Every word of every region is
 * written with its own tag and read back, so a region that left its allocation or met another is a
 * sanitizer report or a wrong word.
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

/* tag every byte of [p, p + bytes) of hop j's region r; 0 is "never written" */
static void fill(void* p, uint64_t bytes, int j, int r) { memset(p, 1 + (j * 8 + r) % 255, bytes); }
static int holds(const void* p, uint64_t bytes, int j, int r) {
  const unsigned char* b = (const unsigned char*)p;
  for (uint64_t i = 0; i < bytes; i++)
    if (b[i] != (unsigned char)(1 + (j * 8 + r) % 255)) return 0;
  return 1;
}

static void one_batch(int k, uint32_t level, uint64_t n, uint32_t depth, uint64_t max_sync, uint64_t rows_n) {
  rp_cont_room room[DG_CONT_BATCH_MAX];
  rp_take_room troom[DG_CONT_BATCH_MAX];
  uint64_t off[DG_CONT_BATCH_MAX + 1], toff[DG_CONT_BATCH_MAX + 1];
  g_cases++;
  uint64_t sum = 0;
  for (int j = 0; j < k; j++) {
    room[j] = rp_cont_room_for(level, n, depth, 8, max_sync, rows_n);
    troom[j] = rp_take_room_for(room[j].kcap, rows_n);
    const uint64_t R = mn(rows_n, 4 * mn(room[j].kcap, 4096) + 64);
    CHECK(troom[j].R == R && troom[j].kcap == room[j].kcap, "hop %d: R %llu want %llu", j, LL(troom[j].R), LL(R));
    CHECK(R <= 4 * 4096 + 64, "hop %d: R %llu over the ceiling", j, LL(R));
    sum += 4 * ((R + 1) & ~UINT64_C(1)) + (((R + 1) / 2 + 1) & ~UINT64_C(1)) + ((room[j].kcap + 2) & ~UINT64_C(1));
  }
  const uint64_t words = rp_cont_carve(k, room, off), twords = rp_take_carve(k, troom, toff);
  CHECK(twords == sum && toff[k] == twords, "k %d: %llu words, want %llu", k, LL(twords), LL(sum));
  uint64_t* block = (uint64_t*)calloc(words ? words : 1, 8); /* exact sizes: one word past is a report */
  uint64_t* tblock = (uint64_t*)calloc(twords ? twords : 1, 8);
  if (!block || !tblock) {
    CHECK(0, "out of memory");
    free(block);
    free(tblock);
    return;
  }
  for (int j = 0; j < k; j++) {
    const dg_merkle_cont c = rp_cont_room_out(block, off[j], room[j]);
    fill(c.pos, 8 * room[j].C, j, 0);
    fill(c.hash, 8 * room[j].C, j, 1);
    fill(c.bucket, 8 * room[j].CB, j, 2);
    fill(rp_cont_room_keys(block, off[j], room[j]), 8 * room[j].kcap, j, 3);
    const dg_store r = rp_take_room_rows(tblock, toff[j], troom[j]);
    uint64_t* o = rp_take_room_offs(tblock, toff[j], troom[j]);
    const uint64_t R = troom[j].R;
    CHECK(r.cap == R && r.n == 0, "hop %d: cap %llu", j, LL(r.cap));
    const void* ptr[6] = {r.key, r.val, r.ts, r.node, r.cnt, o};
    for (int q = 0; q < 6; q++) {
      CHECK(((uintptr_t)ptr[q] & 7) == 0, "hop %d region %d: not 8-byte aligned", j, q);
      CHECK((const uint64_t*)ptr[q] >= tblock + toff[j] && (const uint64_t*)ptr[q] <= tblock + toff[j + 1],
            "hop %d region %d: outside the hop's words", j, q);
    }
    fill(r.key, 8 * R, j, 0);
    fill(r.val, 8 * R, j, 1);
    fill(r.ts, 8 * R, j, 2);
    fill(r.node, 4 * R, j, 3);
    fill(r.cnt, 8 * R, j, 4);
    fill(o, 8 * (troom[j].kcap + 1), j, 5);
  }
  for (int j = 0; j < k; j++) { /* nothing written over by a later region */
    const dg_merkle_cont c = rp_cont_room_out(block, off[j], room[j]);
    CHECK(holds(c.pos, 8 * room[j].C, j, 0) && holds(c.hash, 8 * room[j].C, j, 1) &&
              holds(c.bucket, 8 * room[j].CB, j, 2) &&
              holds(rp_cont_room_keys(block, off[j], room[j]), 8 * room[j].kcap, j, 3),
          "hop %d: an existing region was written over", j);
    const dg_store r = rp_take_room_rows(tblock, toff[j], troom[j]);
    const uint64_t R = troom[j].R;
    CHECK(holds(r.key, 8 * R, j, 0) && holds(r.val, 8 * R, j, 1) && holds(r.ts, 8 * R, j, 2) &&
              holds(r.node, 4 * R, j, 3) && holds(r.cnt, 8 * R, j, 4) &&
              holds(rp_take_room_offs(tblock, toff[j], troom[j]), 8 * (troom[j].kcap + 1), j, 5),
          "hop %d: a row region was written over (k %d, max_sync %llu, rows %llu)", j, k, LL(max_sync), LL(rows_n));
  }
  free(block);
  free(tblock);
}

int main(void) {
  const uint64_t syncs[4] = {1, 5, 200, UINT64_MAX};
  const uint64_t stores[3] = {0, 7, 12500000};
  const uint32_t depth = 22;
  for (int a = 0; a < 4; a++)
    for (int b = 0; b < 3; b++) {
      for (int k = 1; k <= DG_CONT_BATCH_MAX; k++) /* leaf forms at the limits: 4096 pairs */
        one_batch(k, depth + 1, DG_CONT_HOME_ENTRIES, depth, syncs[a], stores[b]);
      one_batch(DG_CONT_BATCH_MAX, depth + 1, 1, depth, syncs[a], stores[b]);
      one_batch(DG_CONT_BATCH_MAX, depth, 200, depth, syncs[a], stores[b]); /* a node form: no rows asked */
    }
  printf("test_carve_take: %d cases, %d failures\n", g_cases, g_fail);
  return g_fail ? 1 : 0;
}
