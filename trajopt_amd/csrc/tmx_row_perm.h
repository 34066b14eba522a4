// tmx_row_perm.h — ROW -> THREAD assignment of the register-resident bursts (DevProblem::row_perm, tmx_part.h), built at upload.
// Pure planning code like wave_plan_build (tmx_wave_plan.h); needs the standard library only (tests/cpp/row_perm_test.cpp).
#pragma once
#include <algorithm>
#include <vector>

// With R > NT row slots the last R - NT threads carry two rows.  In slot order those threads got the LAST slots - for config 1 the 65
// abs rows (two slack variables each): one wave ran two rows x (row + two slacks) = six dependent chains per thread in phases A / C of
// every ADMM iteration while the other three ran two, and waited (tools/prof_loop.py: 2.0 k of the iteration's 4.7 k cycles).  Here the
// two-row threads (and the single-row threads of their waves) take one-slack rows, the two-slack rows go to single-row threads of
// the waves below, top down: at most four chains per thread anywhere.
// naux: slack count of every row slot, R <= 2 NT of them.  Returns perm[q * NT + tid] = the slot thread tid carries as its q-th row
// (-1: none); empty if the rows cannot be placed (slot order then).
static inline std::vector<int> build_row_perm(int R, const std::vector<int>& naux, int NT)
{
  std::vector<int> perm(2 * (size_t)NT, -1), cheap, heavy;
  for (int r = 0; r < R; ++r)
    (naux[r] > 1 ? heavy : cheap).push_back(r);
  const int extra = std::max(0, R - NT), two_first = NT - extra;
  const int prot_first = extra > 0 ? (two_first / 64) * 64 : NT;  // single-row threads [prot_first, two_first) share a wave with two-row threads
  std::vector<int> pool(cheap);
  pool.insert(pool.end(), heavy.begin(), heavy.end());  // (two-slack rows only if the one-slack rows run out)
  size_t take = 0;
  for (int q = 0; q < 2; ++q)
    for (int i = 0; i < extra; ++i)
      perm[(size_t)q * NT + two_first + i] = pool[take++];
  for (int tdx = prot_first; tdx < two_first && take < pool.size(); ++tdx)
    perm[tdx] = pool[take++];
  // the rest on the threads below: one-slack rows bottom up in slot order, two-slack rows top down (as few waves as possible run the
  // two-slot instantiation)
  const int n_free = std::min(prot_first, two_first);
  const size_t n_cheap_left = take < cheap.size() ? cheap.size() - take : 0, n_left = pool.size() - take, n_heavy_left = n_left - n_cheap_left;
  if ((int)n_left > n_free)  // (cannot happen: R - 2 extra - (two_first - prot_first) <= prot_first; kept as a guard)
    perm.clear();
  else
  {
    for (size_t i = 0; i < n_cheap_left; ++i)
      perm[i] = pool[take + i];
    for (size_t i = 0; i < n_heavy_left; ++i)
      perm[(size_t)n_free - n_heavy_left + i] = pool[take + n_cheap_left + i];
  }
  return perm;
}
