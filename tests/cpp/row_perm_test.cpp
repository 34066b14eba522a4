// row_perm_test.cpp — properties of build_row_perm (trajopt_amd/csrc/tmx_row_perm.h) over every row count the fast path takes.
// Stand-alone (tests/test_row_perm.py builds it with -fsanitize=address,undefined); exit status 0 = every property held.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tmx_row_perm.h"

static const int NT = 256;  // TMX_QP_NT
static int failures = 0;

#define CHECK(cond, ...)                                                                                              \
  do                                                                                                                  \
  {                                                                                                                   \
    if (!(cond))                                                                                                      \
    {                                                                                                                 \
      if (++failures <= 20)                                                                                           \
      {                                                                                                               \
        std::fprintf(stderr, "FAILED %s: ", #cond);                                                                   \
        std::fprintf(stderr, __VA_ARGS__);                                                                            \
        std::fprintf(stderr, "\n");                                                                                   \
      }                                                                                                               \
      return;                                                                                                         \
    }                                                                                                                 \
  } while (0)

static uint64_t rng_state = 0;
static uint32_t rnd()  // splitmix64
{
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

static void check(const std::vector<int>& naux, const char* what)
{
  const int R = (int)naux.size();
  const std::vector<int> perm = build_row_perm(R, naux, NT);
  CHECK(perm.size() == 2 * (size_t)NT, "%s R %d: %zu entries", what, R, perm.size());
  // every row slot exactly once, every other entry -1
  std::vector<int> seen(R, 0);
  int placed = 0;
  for (int e : perm)
  {
    CHECK(e >= -1 && e < R, "%s R %d: entry %d", what, R, e);
    if (e >= 0)
    {
      ++seen[e];
      ++placed;
    }
  }
  CHECK(placed == R, "%s R %d: %d rows placed", what, R, placed);
  for (int r = 0; r < R; ++r)
    CHECK(seen[r] == 1, "%s R %d: row %d placed %d times", what, R, r, seen[r]);
  // second rows only on the last max(0, R - NT) threads, and only behind a first row
  const int two_first = NT - (R > NT ? R - NT : 0);
  for (int tid = 0; tid < NT; ++tid)
    if (perm[NT + tid] >= 0)
    {
      CHECK(tid >= two_first, "%s R %d: thread %d holds a second row", what, R, tid);
      CHECK(perm[tid] >= 0, "%s R %d: thread %d holds a second row and no first", what, R, tid);
    }
  // at most four chains per thread whenever the one-slack rows suffice: no thread carries two two-slack rows while a row with
  // fewer slacks sits on a single-row thread of a lower wave
  int top_double_heavy_wave = -1;
  for (int tid = 0; tid < NT; ++tid)
    if (perm[tid] >= 0 && perm[NT + tid] >= 0 && naux[perm[tid]] > 1 && naux[perm[NT + tid]] > 1)
      top_double_heavy_wave = tid / 64;
  for (int tid = 0; tid < NT; ++tid)
    if (perm[tid] >= 0 && perm[NT + tid] < 0 && naux[perm[tid]] <= 1)
      CHECK(tid / 64 >= top_double_heavy_wave, "%s R %d: one-slack row alone on thread %d below a thread with two two-slack rows (wave %d)",
            what, R, tid, top_double_heavy_wave);
}

int main()
{
  for (int R = 1; R <= 2 * NT; ++R)
  {
    std::vector<int> naux(R);
    // the three fixed shapes: one class only, then seeded vectors with entries in {0, 1, 2} of every mix
    for (int c = 0; c <= 2; ++c)
    {
      naux.assign(R, c);
      check(naux, "uniform");
    }
    const int n_random = (R <= NT || R >= 2 * NT - 8) ? 12 : 6;
    for (int s = 0; s < n_random; ++s)
    {
      rng_state = 0x1234567ull * (uint64_t)R + (uint64_t)s;
      const uint32_t heavy_pct = s == 0 ? 90 : (s == 1 ? 10 : rnd() % 101);  // s == 0: heavy-majority rows
      for (int r = 0; r < R; ++r)
        naux[r] = (rnd() % 100 < heavy_pct) ? 2 : (int)(rnd() % 2);
      check(naux, "random");
    }
    // two-slack rows last (config 1: the abs rows close the slot template) and first
    for (int r = 0; r < R; ++r)
      naux[r] = r >= R - R / 5 ? 2 : 1;
    check(naux, "heavy tail");
    for (int r = 0; r < R; ++r)
      naux[r] = r < R / 5 ? 2 : 1;
    check(naux, "heavy head");
  }
  if (failures)
    std::fprintf(stderr, "%d checks failed\n", failures);
  else
    std::printf("ok\n");
  return failures ? 1 : 0;
}
