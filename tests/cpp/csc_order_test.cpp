// The host stage of the block-tridiagonal QP engine (trajopt_amd/csrc/tmx_csc_order.h) on patterns built here: the permutation is a
// permutation, and K = P + sigma I + A' diag(rho) A is block tridiagonal under the reported partition - by brute force over the
// pattern of K, formed independently of the header's adjacency lists.  Plain host code: also built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <set>
#include <utility>
#include <vector>

#include "tmx_csc_order.h"

typedef long long idx;
struct Pattern
{
  int n = 0, m = 0;
  std::vector<std::set<int>> pcol, acol;  // row indices per column (P: upper triangle)
  std::vector<idx> Pp, Pi, Ap, Ai;
  explicit Pattern(int n_, int m_) : n(n_), m(m_), pcol((size_t)n_), acol((size_t)n_) {}
  void P(int i, int j) { pcol[(size_t)std::max(i, j)].insert(std::min(i, j)); }
  void A(int r, int j) { acol[(size_t)j].insert(r); }
  void finish()
  {
    Pp.assign(1, 0);
    Ap.assign(1, 0);
    Pi.clear();
    Ai.clear();
    for (int j = 0; j < n; ++j)
    {
      Pi.insert(Pi.end(), pcol[(size_t)j].begin(), pcol[(size_t)j].end());
      Ai.insert(Ai.end(), acol[(size_t)j].begin(), acol[(size_t)j].end());
      Pp.push_back((idx)Pi.size());
      Ap.push_back((idx)Ai.size());
    }
  }
  // the same pattern with variable j renamed to map[j]
  Pattern renamed(const std::vector<int>& map) const
  {
    Pattern o(n, m);
    for (int j = 0; j < n; ++j)
    {
      for (int i : pcol[(size_t)j])
        o.P(map[(size_t)i], map[(size_t)j]);
      for (int r : acol[(size_t)j])
        o.A(r, map[(size_t)j]);
    }
    o.finish();
    return o;
  }
};

static int failures = 0;
#define CHECK(cond, ...)                                                                                              \
  do                                                                                                                  \
  {                                                                                                                   \
    if (!(cond))                                                                                                      \
    {                                                                                                                 \
      ++failures;                                                                                                     \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond);                                                      \
      std::printf(__VA_ARGS__);                                                                                       \
      std::printf("\n");                                                                                              \
    }                                                                                                                 \
  } while (0)

static CscPartition run(const char* name, const Pattern& p)
{
  const idx zero = 0;
  const CscPartition part = csc_partition(p.n, p.m, p.Pp.data(), p.Pi.empty() ? &zero : p.Pi.data(), p.Ap.data(), p.Ai.empty() ? &zero : p.Ai.data());
  std::printf("%-28s n %4d m %4d bandwidth %4d block %4d x %3d fits %d profitable %d placement %d\n", name, p.n, p.m, part.bandwidth, part.nb,
              part.n_blocks, (int)part.fits, (int)part.profitable, part.placement);
  if (part.perm.empty() && p.n > 0)
  {
    // refused from the rows of A alone, before any ordering: it must say so
    CHECK(!part.fits && !part.reason.empty(), "%s: no ordering and no reason", name);
    return part;
  }
  // a permutation, and pos its inverse
  CHECK((int)part.perm.size() == p.n && (int)part.pos.size() == p.n, "%s", name);
  std::vector<int> seen((size_t)p.n, 0);
  for (int k = 0; k < p.n; ++k)
  {
    const int v = part.perm[(size_t)k];
    CHECK(v >= 0 && v < p.n && !seen[(size_t)v], "%s: perm[%d] = %d", name, k, v);
    if (v >= 0 && v < p.n)
    {
      seen[(size_t)v] = 1;
      CHECK(part.pos[(size_t)v] == k, "%s: pos[perm[%d]]", name, k);
    }
  }
  CHECK(part.nb >= 1 && part.n_blocks * part.nb >= p.n && (part.n_blocks - 1) * part.nb < p.n, "%s: %d blocks of %d", name, part.n_blocks, part.nb);
  // brute force over K: (i, j) is an entry if P has it or a row of A touches both
  std::vector<std::vector<int>> rows((size_t)p.m);
  for (int j = 0; j < p.n; ++j)
    for (int r : p.acol[(size_t)j])
      rows[(size_t)r].push_back(j);
  auto entry = [&](int i, int j) {
    const int bi = part.pos[(size_t)i] / part.nb, bj = part.pos[(size_t)j] / part.nb;
    CHECK(std::abs(bi - bj) <= 1, "%s: entry (%d, %d) of K lies in block (%d, %d)", name, i, j, bi, bj);
    CHECK(std::abs(part.pos[(size_t)i] - part.pos[(size_t)j]) <= part.bandwidth, "%s: bandwidth", name);
  };
  for (int j = 0; j < p.n; ++j)
    for (int i : p.pcol[(size_t)j])
      entry(i, j);
  for (const auto& r : rows)
    for (int a : r)
      for (int b : r)
        entry(a, b);
  // deterministic: a second call gives the same ordering
  const CscPartition again = csc_partition(p.n, p.m, p.Pp.data(), p.Pi.empty() ? &zero : p.Pi.data(), p.Ap.data(), p.Ai.empty() ? &zero : p.Ai.data());
  CHECK(again.perm == part.perm && again.nb == part.nb, "%s: not deterministic", name);
  return part;
}

// T waypoints of D variables from variable first_var and row first_row on; P couples neighbouring waypoints densely; one row on
// every pair (t, t + 1) with a penalty variable of its own, the penalty variables appended after all waypoint variables of the chain
// (the reference layout); identity bound rows.  chain_n / chain_m: the variables and rows it takes.
static int chain_n(int T, int D) { return T * D + T - 1; }
static int chain_m(int T, int D) { return T - 1 + chain_n(T, D); }
static void add_chain(Pattern& p, int T, int D, int first_var, int first_row)
{
  const int nj = T * D, ns = T - 1, n = nj + ns;
  for (int t = 0; t < T; ++t)
    for (int a = 0; a < D; ++a)
      for (int b = 0; b < D; ++b)
      {
        p.P(first_var + t * D + a, first_var + t * D + b);
        if (t + 1 < T)
          p.P(first_var + t * D + a, first_var + (t + 1) * D + b);
      }
  for (int t = 0; t + 1 < T; ++t)
  {
    for (int a = 0; a < 2 * D; ++a)
      p.A(first_row + t, first_var + t * D + a);
    p.A(first_row + t, first_var + nj + t);
  }
  for (int v = 0; v < n; ++v)
    p.A(first_row + ns + v, first_var + v);
}

// csc_rows against the pattern: every entry once, rows in order, columns ascending within a row, rk the entry's CSC position
static void check_rows(const char* name, const Pattern& p)
{
  const idx zero = 0;
  std::vector<int> rp, rj, rk;
  rp.push_back(-7);  // (the function appends: what was there stays)
  csc_rows(p.m, p.n, p.Ap.data(), p.Ai.empty() ? &zero : p.Ai.data(), false, rp, rj, rk);
  CHECK((int)rp.size() == p.m + 2 && rp[0] == -7 && rp[1] == 0 && rp.back() == (int)p.Ai.size(), "%s: offsets of A", name);
  for (int r = 0; r < p.m; ++r)
    for (int e = rp[(size_t)r + 1]; e < rp[(size_t)r + 2]; ++e)
    {
      const int j = rj[(size_t)e], k = rk[(size_t)e];
      CHECK(k >= p.Ap[(size_t)j] && k < p.Ap[(size_t)j + 1] && p.Ai[(size_t)k] == r, "%s: A entry %d of row %d", name, e, r);
      CHECK(e == rp[(size_t)r + 1] || rj[(size_t)e - 1] < j, "%s: columns of row %d not ascending", name, r);
    }
  std::vector<int> pp, pj, pk;
  csc_rows(p.n, p.n, p.Pp.data(), p.Pi.empty() ? &zero : p.Pi.data(), true, pp, pj, pk);
  size_t strict = 0;
  for (int j = 0; j < p.n; ++j)
    strict += p.pcol[(size_t)j].size() - p.pcol[(size_t)j].count(j);
  CHECK(pp.back() == (int)strict && pj.size() == strict, "%s: strict upper triangle of P", name);
  for (int i = 0; i < p.n; ++i)
    for (int e = pp[(size_t)i]; e < pp[(size_t)i + 1]; ++e)
      CHECK(pj[(size_t)e] > i && p.Pi[(size_t)pk[(size_t)e]] == i, "%s: P entry %d of row %d", name, e, i);
}

int main()
{
  // 1. a chain of 6 blocks of 3 variables, 6 penalty variables appended (one of them on no pair row: bound row only)
  {
    Pattern p(24, 6 + 24);
    for (int t = 0; t < 6; ++t)
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
        {
          p.P(t * 3 + a, t * 3 + b);
          if (t < 5)
            p.P(t * 3 + a, (t + 1) * 3 + b);
        }
    for (int t = 0; t < 6; ++t)
    {
      for (int a = 0; a < 3; ++a)
      {
        p.A(t, t * 3 + a);
        if (t < 5)
          p.A(t, (t + 1) * 3 + a);
      }
      p.A(t, 18 + t);
    }
    for (int v = 0; v < 24; ++v)
      p.A(6 + v, v);
    p.finish();
    const CscPartition a = run("chain 6 x 3 + 6 penalties", p);
    CHECK(a.fits && a.nb <= 8 && a.n_blocks >= 3, "block size %d is not far below n = 24", a.nb);
    // 2. the same chain with its variables shuffled (a fixed linear-congruential shuffle)
    std::vector<int> map(24);
    std::iota(map.begin(), map.end(), 0);
    unsigned s = 12345u;
    for (int k = 23; k > 0; --k)
    {
      s = s * 1664525u + 1013904223u;
      std::swap(map[(size_t)k], map[(size_t)((s >> 8) % (unsigned)(k + 1))]);
    }
    const CscPartition b = run("the same, shuffled", p.renamed(map));
    CHECK(b.fits && b.nb <= 8, "shuffled: block size %d", b.nb);
  }
  // 3. two disconnected chains
  {
    const int n1 = chain_n(5, 3), m1 = chain_m(5, 3);
    Pattern p(n1 + chain_n(4, 2), m1 + chain_m(4, 2));
    add_chain(p, 5, 3, 0, 0);
    add_chain(p, 4, 2, n1, m1);
    p.finish();
    check_rows("two disconnected chains", p);
    const CscPartition a = run("two disconnected chains", p);
    CHECK(a.fits && a.nb <= 8, "block size %d", a.nb);
  }
  // 4. n = 1
  {
    Pattern p(1, 1);
    p.P(0, 0);
    p.A(0, 0);
    p.finish();
    const CscPartition a = run("n = 1", p);
    CHECK(a.fits && a.nb == 1 && a.n_blocks == 1 && !a.profitable, "n = 1");
  }
  // 5. m = 0 (a tridiagonal P alone), and P = 0 with isolated variables
  {
    Pattern p(9, 0);
    for (int j = 0; j < 9; ++j)
    {
      p.P(j, j);
      if (j)
        p.P(j - 1, j);
    }
    p.finish();
    const CscPartition a = run("m = 0", p);
    CHECK(a.fits && a.bandwidth == 1, "bandwidth %d", a.bandwidth);
    Pattern z(7, 0);
    z.finish();
    const CscPartition b = run("no entry at all", z);
    CHECK(b.fits && b.bandwidth == 0, "isolated variables");
  }
  // 6. a dense pattern has no chain: the partition is two half-bandwidth blocks (two blocks are always block tridiagonal; a single
  // block is what n = 1 gives), the cost model keeps the dense engine, and far above the cap it does not fit
  {
    Pattern p(30, 30);
    for (int i = 0; i < 30; ++i)
      for (int j = i; j < 30; ++j)
        p.P(i, j);
    for (int v = 0; v < 30; ++v)
      p.A(v, v);
    p.finish();
    const CscPartition a = run("dense 30", p);
    CHECK(a.fits && !a.profitable && a.n_blocks == 2 && a.nb == 15, "dense: %d blocks of %d, profitable %d", a.n_blocks, a.nb, (int)a.profitable);
    // dense rows of A above the dense engine's limit (n = 600, 200 full rows): every variable is coupled to every other after its first
    // row, the stage must stay small and fast, and AUTO keeps the dense engine
    Pattern rows(600, 200);
    for (int r = 0; r < 200; ++r)
      for (int j = 0; j < 600; ++j)
        rows.A(r, j);
    rows.finish();
    const CscPartition d = run("200 full rows, n = 600", rows);
    CHECK(d.fits && !d.profitable && d.n_blocks == 2 && d.nb == 300, "dense rows: %d blocks of %d", d.n_blocks, d.nb);
    check_rows("200 full rows, n = 600", rows);
    Pattern big(3 * TMX_CB_NB_MAX + 10, 1);
    for (int j = 0; j < big.n; ++j)
      big.A(0, j);
    big.finish();
    const CscPartition b = run("one full row of A", big);
    CHECK(!b.fits && !b.profitable && b.perm.empty() && !b.reason.empty(), "a full row above three blocks of the cap is refused before any ordering");
    Pattern mid(3 * TMX_CB_NB_MAX + 48, 0);
    for (int j = 1; j < mid.n; ++j)
      mid.P(0, j);   // a star: its centre borders every block, so three blocks at the most
    mid.finish();
    const CscPartition c = run("star of 1200", mid);
    CHECK(!c.fits && !c.reason.empty(), "star: block %d", c.nb);
  }
  // 7. an n the block size does not divide, incl. a last block of one variable
  {
    for (int n : { 13, 14, 16, 17 })
    {
      Pattern p(n, 0);
      for (int j = 0; j < n; ++j)
        for (int i = std::max(0, j - 4); i <= j; ++i)
          p.P(i, j);
      p.finish();
      const CscPartition a = run("band of 4", p);
      CHECK(a.fits && a.nb == 4, "n = %d: block %d", n, a.nb);
      if (n == 13 || n == 17)
        CHECK(n - (a.n_blocks - 1) * a.nb == 1, "n = %d: the last block should hold one variable", n);
    }
  }
  // 8. empty columns of A (variables no row touches) next to a chain
  {
    Pattern q(chain_n(6, 2) + 3, chain_m(6, 2));
    add_chain(q, 6, 2, 0, 0);
    q.P(chain_n(6, 2) + 1, chain_n(6, 2) + 1);
    q.finish();
    run("empty columns of A", q);
    check_rows("empty columns of A", q);
  }
  // 9. the AUTO rule's flop model at the headline shape (n = 572 in blocks of 32) and at its edges
  CHECK(csc_chain_profitable(572, 32, 18), "572 / 32 must be profitable");
  CHECK(!csc_chain_profitable(572, 286, 2), "two half blocks: the sweeps cost more than the dense mat-vec");
  CHECK(!csc_chain_profitable(10, 10, 1), "one block is never profitable");
  std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
