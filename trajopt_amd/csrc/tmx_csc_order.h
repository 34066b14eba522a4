// tmx_csc_order.h — host stage of the block-tridiagonal engine behind tmx_qp_solve_batched (tmx_csc_blocks.h): from the CSC
// arrays of one QP alone, the pattern of the reduced matrix K = P + sigma I + A' diag(rho) A, a symmetric ordering with a small
// profile (reverse Cuthill-McKee from a pseudo-peripheral node) and a partition of the ordered variables into uniform blocks
// under which K is block tridiagonal (the last block is padded by identity).  Pure C++: no HIP, no tmx type - a stand-alone
// host program can call it (tests/cpp/csc_order_test.cpp).
//
// Everything here is deterministic: ties are broken on the lowest index, components are handled one after the other in the
// order of their lowest variable, an isolated variable is a component of its own.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

// Block-size caps.  LDS tiles: the factor step of block k keeps S_{k-1}^-1 and the S_k it forms and
// inverts as two nb x nb fp64 tiles next to 1088 doubles of reduction scratch and pivot row / column:
// (1088 + 2 nb^2) * 8 B <= 160 KB gives nb <= 98; 96 is the multiple of 16 below it.  Larger blocks are worked on in the
// per-QP HBM workspace, where the three tiles of a factor step (S_{k-1}^-1, K_{k,k-1}, S_k) should stay in the 4 MB L2 of
// one XCD: 3 * 384^2 * 8 B = 3.4 MB.
#define TMX_CB_NB_LDS 96
#define TMX_CB_NB_MAX 384
#define TMX_CB_NB_MIN 4  // no chain of blocks smaller than this: every block costs the sweeps two barriers

enum
{
  TMX_CB_PLACE_NONE = 0,  // the QP does not fit the engine
  TMX_CB_PLACE_LDS = 1,   // tiles of the factor step in LDS, factors in the HBM workspace
  TMX_CB_PLACE_HBM = 2    // tiles and factors in the HBM workspace
};

struct CscPartition
{
  int n = 0;
  int nb = 0;        // block size
  int n_blocks = 0;  // n_blocks * nb >= n; the tail of the last block is padding
  int bandwidth = 0; // max |pos[i] - pos[j]| over the entries of K
  int placement = TMX_CB_PLACE_NONE;
  bool fits = false;        // nb <= TMX_CB_NB_MAX
  bool profitable = false;  // the cost model below prefers the chain to the dense engine
  std::string reason;       // why it does not fit
  std::vector<int> perm;    // perm[new] = old
  std::vector<int> pos;     // pos[old] = new
};

// Row-wise copy of a CSC pattern, APPENDED to rp / rj / rk: rp gets rows + 1 offsets that start at 0 for this matrix, rj the column
// and rk the index into the CSC value array of every entry - rows in order, within a row the entries in the order of the columns
// and of storage within a column.  skip_diagonal: P is given by its upper triangle; its copy holds the entries right of the diagonal.
template <class IDX>
static inline void csc_rows(int rows, int cols, const IDX* Cp, const IDX* Ci, bool skip_diagonal, std::vector<int>& rp, std::vector<int>& rj,
                            std::vector<int>& rk)
{
  std::vector<int> cnt((size_t)rows + 1, 0);
  for (int j = 0; j < cols; ++j)
    for (IDX p = Cp[j]; p < Cp[j + 1]; ++p)
      if (!(skip_diagonal && (int)Ci[p] == j))
        cnt[(size_t)Ci[p] + 1]++;
  for (int i = 0; i < rows; ++i)
    cnt[(size_t)i + 1] += cnt[(size_t)i];
  rp.insert(rp.end(), cnt.begin(), cnt.end());
  const size_t base = rj.size();
  rj.resize(base + (size_t)cnt[(size_t)rows]);
  rk.resize(base + (size_t)cnt[(size_t)rows]);
  for (int j = 0; j < cols; ++j)
    for (IDX p = Cp[j]; p < Cp[j + 1]; ++p)
      if (!(skip_diagonal && (int)Ci[p] == j))
      {
        const size_t at = base + (size_t)cnt[(size_t)Ci[p]]++;
        rj[at] = j;
        rk[at] = (int)p;
      }
}

// Adjacency lists of K without the diagonal, sorted.  The neighbours of a variable are collected per variable through a mark array
// (every distinct neighbour once: the memory is the size of the pattern of K, not of the sum of the squared row lengths), and the
// walk over a variable's rows ends once all other variables are its neighbours.  false (and `reason`) when the QP cannot fit: a
// variable and its neighbours lie in three consecutive blocks, so more than 3 TMX_CB_NB_MAX - 1 neighbours are too many.
template <class IDX>
static inline bool csc_pattern(int n, int m, const IDX* Pp, const IDX* Pi, const IDX* Ap, const IDX* Ai, std::vector<std::vector<int>>& adj,
                               std::string& reason)
{
  adj.assign((size_t)n, std::vector<int>());
  std::vector<int> rp, rj, rk;
  csc_rows(m, n, Ap, Ai, false, rp, rj, rk);
  // the strict upper triangle of P gives a neighbour to both of its variables
  for (int j = 0; j < n; ++j)
    for (IDX p = Pp[j]; p < Pp[j + 1]; ++p)
    {
      const int i = (int)Pi[p];
      if (i != j)
      {
        adj[(size_t)i].push_back(j);
        adj[(size_t)j].push_back(i);
      }
    }
  std::vector<int> mark((size_t)n, -1);
  for (int i = 0; i < n; ++i)
  {
    std::vector<int>& nbr = adj[(size_t)i];
    // (duplicate entries of P)
    std::sort(nbr.begin(), nbr.end());
    nbr.erase(std::unique(nbr.begin(), nbr.end()), nbr.end());
    mark[(size_t)i] = i;
    for (int j : nbr)
      mark[(size_t)j] = i;
    for (IDX p = Ap[i]; p < Ap[i + 1] && (int)nbr.size() < n - 1; ++p)
    {
      const int r = (int)Ai[p];
      for (int e = rp[(size_t)r]; e < rp[(size_t)r + 1]; ++e)
        if (mark[(size_t)rj[(size_t)e]] != i)
        {
          mark[(size_t)rj[(size_t)e]] = i;
          nbr.push_back(rj[(size_t)e]);
        }
    }
    if ((int)nbr.size() > 3 * TMX_CB_NB_MAX - 1)
    {
      reason = "variable " + std::to_string(i) + " is coupled to " + std::to_string(nbr.size()) + " others: more than three blocks of " +
               std::to_string(TMX_CB_NB_MAX) + " variables hold";
      return false;
    }
    std::sort(nbr.begin(), nbr.end());
  }
  return true;
}

// breadth-first levels from `root` within its component; returns the eccentricity, `last` = the nodes of the last level
static inline int csc_bfs_levels(const std::vector<std::vector<int>>& adj, int root, std::vector<int>& mark, int stamp, std::vector<int>& last)
{
  std::vector<int> cur(1, root), nxt;
  mark[(size_t)root] = stamp;
  int ecc = 0;
  for (;;)
  {
    nxt.clear();
    for (int v : cur)
      for (int w : adj[(size_t)v])
        if (mark[(size_t)w] != stamp)
        {
          mark[(size_t)w] = stamp;
          nxt.push_back(w);
        }
    if (nxt.empty())
      break;
    cur.swap(nxt);
    ++ecc;
  }
  last = cur;
  return ecc;
}

// reverse Cuthill-McKee: perm[new] = old
static inline void csc_rcm(const std::vector<std::vector<int>>& adj, std::vector<int>& perm)
{
  const int n = (int)adj.size();
  perm.clear();
  perm.reserve((size_t)n);
  std::vector<int> mark((size_t)n, 0), last;
  std::vector<char> done((size_t)n, 0);
  int stamp = 0;
  auto lower = [&](int a, int b) { return adj[(size_t)a].size() != adj[(size_t)b].size() ? adj[(size_t)a].size() < adj[(size_t)b].size() : a < b; };
  for (int s = 0; s < n; ++s)
  {
    if (done[(size_t)s])
      continue;
    // pseudo-peripheral node (George & Liu): walk to a lowest-degree node of the last level while the eccentricity grows
    int root = s, ecc = csc_bfs_levels(adj, root, mark, ++stamp, last);
    for (;;)
    {
      int cand = last[0];
      for (int v : last)
        if (lower(v, cand))
          cand = v;
      const int e2 = csc_bfs_levels(adj, cand, mark, ++stamp, last);
      if (e2 <= ecc)
        break;
      root = cand;
      ecc = e2;
    }
    // Cuthill-McKee from the root: neighbours in the order (degree, index)
    size_t head = perm.size();
    perm.push_back(root);
    done[(size_t)root] = 1;
    std::vector<int> nb;
    while (head < perm.size())
    {
      const int v = perm[head++];
      nb.clear();
      for (int w : adj[(size_t)v])
        if (!done[(size_t)w])
        {
          done[(size_t)w] = 1;
          nb.push_back(w);
        }
      std::sort(nb.begin(), nb.end(), lower);
      perm.insert(perm.end(), nb.begin(), nb.end());
    }
  }
  std::reverse(perm.begin(), perm.end());
}

// Cost model of the AUTO rule, in multiply-adds.  Chain: per block the multiplier K_{k,k-1} S_{k-1}^-1,
// the Schur update and the Gauss-Jordan inverse, nb^3 each; per solve a forward product with the multiplier and a backward
// one with the inverse and the next multiplier, 3 nb^2.  Dense engine: n^3 for the Gauss-Jordan inverse, n^2 per solve.
static inline bool csc_chain_profitable(int n, int nb, int n_blocks)
{
  const double N = (double)n, B = (double)nb, K = (double)n_blocks;
  return 3.0 * K * B * B * B < N * N * N && 3.0 * K * B * B < N * N;
}

// ordering + partition of one QP.  min_block > 0 replaces TMX_CB_NB_MIN (the tuning hook TMX_CB_BLOCK_MIN of the library).
template <class IDX>
static inline CscPartition csc_partition(int n, int m, const IDX* Pp, const IDX* Pi, const IDX* Ap, const IDX* Ai, int min_block = 0)
{
  CscPartition part;
  part.n = n;
  std::vector<std::vector<int>> adj;
  if (!csc_pattern(n, m, Pp, Pi, Ap, Ai, adj, part.reason))
    return part;
  csc_rcm(adj, part.perm);
  part.pos.assign((size_t)n, 0);
  for (int k = 0; k < n; ++k)
    part.pos[(size_t)part.perm[(size_t)k]] = k;
  int bw = 0;
  for (int i = 0; i < n; ++i)
    for (int j : adj[(size_t)i])
      bw = std::max(bw, std::abs(part.pos[(size_t)i] - part.pos[(size_t)j]));
  part.bandwidth = bw;
  // the smallest uniform block size under which every entry lies in a diagonal or a neighbouring block: s >= bw always
  // does, s < bw / 2 never
  auto tridiagonal = [&](int s) {
    for (int i = 0; i < n; ++i)
      for (int j : adj[(size_t)i])
        if (std::abs(part.pos[(size_t)i] / s - part.pos[(size_t)j] / s) > 1)
          return false;
    return true;
  };
  const int floor_nb = std::min(n, min_block > 0 ? min_block : TMX_CB_NB_MIN);
  int s = std::max(std::max(1, (bw + 1) / 2), floor_nb);
  while (s < bw && !tridiagonal(s))
    ++s;
  part.nb = s;
  part.n_blocks = (n + s - 1) / s;
  part.fits = s <= TMX_CB_NB_MAX;
  if (!part.fits)
    part.reason = "blocks of " + std::to_string(s) + " variables (half-bandwidth " + std::to_string(bw) + " after reverse Cuthill-McKee) exceed the cap of " +
                  std::to_string(TMX_CB_NB_MAX);
  part.placement = !part.fits ? TMX_CB_PLACE_NONE : (s <= TMX_CB_NB_LDS ? TMX_CB_PLACE_LDS : TMX_CB_PLACE_HBM);
  part.profitable = part.fits && csc_chain_profitable(n, part.nb, part.n_blocks);
  return part;
}
