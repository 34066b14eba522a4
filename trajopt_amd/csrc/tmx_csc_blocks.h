// tmx_csc_blocks.h — block-tridiagonal engine for QPs handed over in CSC form (tmx_qp_solve_batched, TMX_QP_ENGINE_BLOCKS / AUTO).
//
// The same OSQP v1.0.0 algorithm as qp_generic_block (tmx_generic.h), restated from oracle/osqp_restate.hpp with the same settings
// struct, for QPs whose reduced matrix K = P + sigma I + A' diag(rho) A becomes block tridiagonal under the symmetric ordering the
// host stage finds from the CSC arrays alone (tmx_csc_order.h): trajectory QPs in the reference layout, whatever built them.
// One workgroup per QP.  What differs from the dense engine:
//   * P x, A x, A' y come from the CSC arrays and row-wise copies of them (built on the host); P and A are never expanded;
//   * K lives in permuted block storage (nb x nb diagonal and sub-diagonal blocks), is assembled from the CSC arrays at every rho
//     update and factored as a block chain: S_0 = K_00, S_k = K_kk - K_{k,k-1} S_{k-1}^-1 K_{k-1,k}; kept are S_k^-1 (unpivoted
//     Gauss-Jordan on an SPD block, as gen_invert) and the multipliers M_k = K_{k,k-1} S_{k-1}^-1; a solve is a forward and a backward
//     sweep of block mat-vecs, followed by one step of iterative refinement against the sparse K (what TMX_DENSE_REFINE does there);
//   * the polish solves the reduced system P + delta I + Aact' Aact / delta on the same blocks and refines against the unperturbed
//     KKT residual ("fp64 carries the polish").
// HOUSE RULE: every output element has one owner thread and a fixed summation order; no sum's order follows the number of threads
// (cb_sum: 256 fixed partial sums, whatever the workgroup size).  The host build (one thread) and the SIMT emulation (256) therefore
// return the same bytes.
#pragma once
#include "tmx_generic.h"

#if TMX_IS_GCN
typedef __attribute__((address_space(3))) double cb_lds_d;
#else
typedef double cb_lds_d;
#endif

// TMX_CB_PROF=1 (a profiling build, tools/time_csc_blocks.py): thread 0 of every workgroup accumulates the 10 ns ticks spent in
// the assembly of K, its factorisation, the sweeps and the whole polish section; tmx_qp_solve_batched prints them to stderr
#ifndef TMX_CB_PROF
#define TMX_CB_PROF 0
#endif
#if TMX_CB_PROF
#define CB_T0() const long long cb_t0_ = tmx_wall_ticks()
#define CB_T1(k) cb_prof[(k) + (cb_in_polish ? 4 : 0)] += tmx_wall_ticks() - cb_t0_
#else
#define CB_T0() ((void)0)
#define CB_T1(k) ((void)0)
#endif

#define TMX_CB_LDS_FIXED 1088  // doubles in front of the tiles: 320 reduction scratch, 2 x 384 pivot row / column of the Gauss-Jordan

struct CbQp  // device view of one QP
{
  int n, m, nb, nblk;
  int place;                   // TMX_CB_PLACE_LDS / TMX_CB_PLACE_HBM
  int warm, slot;              // slot: index of the QP in the caller's batch (info record)
  long long oP, oA, oPp, oAp;  // as GenQp
  long long oPr, oPrp;         // row-wise copy of the strict upper triangle of P
  long long oAr, oArp;         // row-wise copy of A
  long long operm;             // perm / pos
  long long ov_n, ov_m, ows;
};
struct CbData
{
  GenData g;
  const int *Prp, *Prj, *Prk;  // row i of P above the diagonal: columns Prj[p], value index Prk[p] into the CSC values, p in Prp[i] .. Prp[i + 1]
  const int *Arp, *Arj, *Ark;  // row i of A likewise
  const int *perm, *pos;       // perm[new] = old, pos[old] = new
#if TMX_CB_PROF
  long long* prof;             // [slot][8]: assembly, factorisation, sweeps, (whole polish section) ; the same three inside the polish, total
#endif
};
TMX_HOSTDEVFN size_t cb_ws_doubles(int n, int m, int nb, int nblk, long long nnzP, long long nnzA)
{
  const size_t N = (size_t)n, M = (size_t)m, T = (size_t)nb * nb * nblk, NP = (size_t)nb * nblk;
  return (size_t)nnzP + (size_t)nnzA + 4 * T + 2 * NP + 16 * N + 19 * M + 64;  // (18 m-vectors + 2 m ints)
}

// fixed-order sum of f(0) .. f(count - 1): 256 strided partial sums, added in order - the same bits for every workgroup size
template <class F>
TMX_DEVFN double cb_sum(int count, F f, double* red, int tid, int NT)
{
  for (int k = tid; k < 256; k += NT)
  {
    double s = 0.0;
    for (int i = k; i < count; i += 256)
      s += f(i);
    red[k] = s;
  }
  TMX_SYNC();
  double s = 0.0;
  for (int k = 0; k < 256; ++k)
    s += red[k];
  TMX_SYNC();
  return s;
}

// in-place Gauss-Jordan inverse of the nb x nb tile S WITHOUT pivoting (gen_invert's arithmetic; the element walk carries its
// (row, column) instead of dividing); TP: typed LDS pointer or a plain one into the HBM workspace
template <class TP>
TMX_DEVFN void cb_invert(TP S, int nb, double* col, double* row, int tid, int NT)
{
  const int si = NT / nb, sj = NT % nb;
  for (int k = 0; k < nb; ++k)
  {
    for (int e = tid; e < nb; e += NT)
    {
      col[e] = S[e * nb + k];
      row[e] = S[k * nb + e];
    }
    TMX_SYNC();
    const double piv = 1.0 / row[k];
    int i = tid / nb, j = tid % nb;
    while (i < nb)
    {
      double v;
      if (i == k && j == k)
        v = piv;
      else if (i == k)
        v = row[j] * piv;
      else if (j == k)
        v = -col[i] * piv;
      else
        v = S[i * nb + j] - col[i] * row[j] * piv;
      S[i * nb + j] = v;
      i += si;
      j += sj;
      if (j >= nb)
      {
        j -= nb;
        ++i;
      }
    }
    TMX_SYNC();
  }
}

struct CbChain  // the factor storage of one QP
{
  double *Sv, *Kl, *Mb, *Mt;  // [nblk][nb][nb]: K_kk -> S_k^-1 ; K_{k,k-1} ; M_k ; M_k'
  int nb, nblk;
};

// factor the chain.  LDS = true: S_{k-1}^-1 and S_k are the two tiles t0 / t1 (ping-pong), S_k^-1 is copied to Sv; false: in place in Sv
template <bool LDS, class TP>
TMX_DEVFN void cb_factor(const CbChain& c, TP t0, TP t1, double* col, double* row, int tid, int NT)
{
  const int nb = c.nb, BB = nb * nb;
  const int si = NT / nb, sj = NT % nb;
  for (int k = 0; k < c.nblk; ++k)
  {
    double* Kd = c.Sv + (size_t)k * BB;
    const double* Kl = c.Kl + (size_t)k * BB;
    double *Mb = c.Mb + (size_t)k * BB, *Mt = c.Mt + (size_t)k * BB;
    TP prev, cur;
    if constexpr (LDS)
    {
      prev = (k & 1) ? t0 : t1;
      cur = (k & 1) ? t1 : t0;
    }
    else
    {
      prev = (TP)(c.Sv + (size_t)(k > 0 ? k - 1 : 0) * BB);
      cur = (TP)Kd;
    }
    if (k > 0)
    {
      // M_k = K_{k,k-1} S_{k-1}^-1
      int i = tid / nb, j = tid % nb;
      while (i < nb)
      {
        double s = 0.0;
        for (int q = 0; q < nb; ++q)
          s += Kl[i * nb + q] * prev[q * nb + j];
        Mb[i * nb + j] = s;
        Mt[j * nb + i] = s;
        i += si;
        j += sj;
        if (j >= nb)
        {
          j -= nb;
          ++i;
        }
      }
      TMX_SYNC();
    }
    if (LDS || k > 0)
    {
      // S_k = K_kk - M_k K_{k,k-1}'  (by symmetry entry (i, j) is taken as K_kk[i][j] - sum_q K_{k,k-1}[i][q] M_k[j][q])
      int i = tid / nb, j = tid % nb;
      while (i < nb)
      {
        double s = Kd[i * nb + j];
        if (k > 0)
        {
          double a = 0.0;
          for (int q = 0; q < nb; ++q)
            a += Kl[i * nb + q] * Mt[q * nb + j];
          s -= a;
        }
        cur[i * nb + j] = s;
        i += si;
        j += sj;
        if (j >= nb)
        {
          j -= nb;
          ++i;
        }
      }
      TMX_SYNC();
    }
    cb_invert(cur, nb, col, row, tid, NT);
    if (LDS)
    {
      for (int e = tid; e < BB; e += NT)
        Kd[e] = cur[e];
      TMX_SYNC();
    }
  }
}

// K xs = b for vectors in PERMUTED order: y (scratch) and b (overwritten by the solution), nb * nblk doubles each.
// When one thread walks a row, a block mat-vec of a sweep step is a dependent chain of loads with little in flight, and the sweeps
// were nine tenths of the kernel (profiles/csc_blocks_timing_row_walk.txt).  Every row's dot product is therefore cut into
// TMX_CB_PARTS FIXED column ranges, one work item each (their loads are in flight together), and the partial sums are added in the
// order of the ranges: the split is a constant of the code, not of the launch - the same bits for every workgroup size.
// part: 2 * TMX_CB_PARTS * nb doubles of LDS.
#define TMX_CB_PARTS 8
template <class LP>
TMX_DEVFN void cb_sweeps(const CbChain& c, double* b, double* y, LP part, int tid, int NT)
{
  const int nb = c.nb, BB = nb * nb, cw = (nb + TMX_CB_PARTS - 1) / TMX_CB_PARTS;
  const int i0 = tid % nb, p0 = tid / nb, si = NT % nb, sp = NT / nb;
  // forward: y_k = b_k - M_k y_{k-1}
  for (int k = 0; k < c.nblk; ++k)
  {
    if (k > 0)
    {
      const double *Mt = c.Mt + (size_t)k * BB, *yk = y + (k - 1) * nb;
      int i = i0, p = p0;
      while (p < TMX_CB_PARTS)
      {
        const int q0 = p * cw, q1 = (q0 + cw < nb) ? q0 + cw : nb;
        double a = 0.0;
        for (int q = q0; q < q1; ++q)
          a += Mt[q * nb + i] * yk[q];
        part[p * nb + i] = a;
        i += si;
        p += sp;
        if (i >= nb)
        {
          i -= nb;
          ++p;
        }
      }
      TMX_SYNC();
    }
    for (int i = tid; i < nb; i += NT)
    {
      double s = b[k * nb + i];
      if (k > 0)
      {
        double a = 0.0;
        for (int p = 0; p < TMX_CB_PARTS; ++p)
          a += part[p * nb + i];
        s -= a;
      }
      y[k * nb + i] = s;
    }
    TMX_SYNC();
  }
  // backward: x_k = S_k^-1 y_k - M_{k+1}' x_{k+1}   (S_k^-1 read by its transpose: the same matrix up to the rounding of the inverse)
  for (int k = c.nblk - 1; k >= 0; --k)
  {
    const bool next = k + 1 < c.nblk;
    const double *Sv = c.Sv + (size_t)k * BB, *Mn = c.Mb + (size_t)(k + 1) * BB, *yk = y + k * nb, *xn = b + (k + 1) * nb;
    int i = i0, p = p0;
    while (p < (next ? 2 : 1) * TMX_CB_PARTS)
    {
      const int pp = p < TMX_CB_PARTS ? p : p - TMX_CB_PARTS;
      const int q0 = pp * cw, q1 = (q0 + cw < nb) ? q0 + cw : nb;
      double a = 0.0;
      if (p < TMX_CB_PARTS)
        for (int q = q0; q < q1; ++q)
          a += Sv[q * nb + i] * yk[q];
      else
        for (int q = q0; q < q1; ++q)
          a += Mn[q * nb + i] * xn[q];
      part[p * nb + i] = a;
      i += si;
      p += sp;
      if (i >= nb)
      {
        i -= nb;
        ++p;
      }
    }
    TMX_SYNC();
    for (int r = tid; r < nb; r += NT)
    {
      double s = 0.0;
      for (int q = 0; q < TMX_CB_PARTS; ++q)
        s += part[q * nb + r];
      if (next)
      {
        double a = 0.0;
        for (int q = 0; q < TMX_CB_PARTS; ++q)
          a += part[(TMX_CB_PARTS + q) * nb + r];
        s -= a;
      }
      b[k * nb + r] = s;
    }
    TMX_SYNC();
  }
}

TMX_DEVFN void qp_csc_blocks_block(const CbQp& g, const CbData& dd, const tmx_osqp_settings& st, double* smem, int tid, int NT)
{
  const GenData& d = dd.g;
  const int n = g.n, m = g.m, nb = g.nb, nblk = g.nblk, npad = nb * nblk, BB = nb * nb;
  double* red = smem;
  double* gcol = smem + 320;
  double* grow = smem + 704;
  const long long *Pp = d.P_p + g.oPp, *Pi = d.P_i + g.oP, *Ap = d.A_p + g.oAp, *Ai = d.A_i + g.oA;
  const int *Prp = dd.Prp + g.oPrp, *Prj = dd.Prj + g.oPr, *Prk = dd.Prk + g.oPr;
  const int *Arp = dd.Arp + g.oArp, *Arj = dd.Arj + g.oAr, *Ark = dd.Ark + g.oAr;
  const int *perm = dd.perm + g.operm, *pos = dd.pos + g.operm;
  const long long nnzP = Pp[n], nnzA = Ap[n];
  double* w = d.ws + g.ows;
#define CTAKE(name, cnt)                                                                                              \
  double* name = w;                                                                                                   \
  w += (cnt)
  CTAKE(Pv, (size_t)nnzP);
  CTAKE(Av, (size_t)nnzA);
  CbChain ch;
  ch.nb = nb;
  ch.nblk = nblk;
  ch.Sv = w;
  w += (size_t)nblk * BB;
  ch.Kl = w;
  w += (size_t)nblk * BB;
  ch.Mb = w;
  w += (size_t)nblk * BB;
  ch.Mt = w;
  w += (size_t)nblk * BB;
  CTAKE(bp, npad);
  CTAKE(yp, npad);
  CTAKE(q, n);
  CTAKE(D, n);
  CTAKE(x, n);
  CTAKE(xprev, n);
  CTAKE(xt, n);
  CTAKE(dx, n);
  CTAKE(Px, n);
  CTAKE(Aty, n);
  CTAKE(tn, n);
  CTAKE(tn2, n);
  CTAKE(px, n);
  CTAKE(dres, n);
  CTAKE(pr1, n);
  CTAKE(pdx, n);
  CTAKE(kr, n);   // residual / correction of the refinement step
  CTAKE(kc, n);
  CTAKE(l, m);
  CTAKE(u, m);
  CTAKE(E, m);
  CTAKE(z, m);
  CTAKE(zprev, m);
  CTAKE(zt, m);
  CTAKE(y, m);
  CTAKE(dy, m);
  CTAKE(Ax, m);
  CTAKE(rho, m);
  CTAKE(tm, m);
  CTAKE(pz, m);
  CTAKE(py, m);
  CTAKE(pres, m);
  CTAKE(pw, m);   // row weights of the polish: 1 / delta on active rows, 0 elsewhere
  CTAKE(pb, m);   // the active bound
  CTAKE(pr2, m);
  CTAKE(km, m);   // A x of the refinement step
#undef CTAKE
  int* ctype = reinterpret_cast<int*>(w);  // m
  int* flag = ctype + m;                   // m
#if TMX_CB_PROF
  long long cb_prof[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
  bool cb_in_polish = false;
  const long long cb_start = tmx_wall_ticks();
#endif

  // ---- sparse products: one owner thread per output element, entries in storage order -----------------------------------------
  auto A_times = [&](const double* xx, double* out) {
    for (int i = tid; i < m; i += NT)
    {
      double s = 0.0;
      for (int p = Arp[i]; p < Arp[i + 1]; ++p)
        s += Av[Ark[p]] * xx[Arj[p]];
      out[i] = s;
    }
  };
  auto At_times = [&](const double* yy, double* out) {
    for (int j = tid; j < n; j += NT)
    {
      double s = 0.0;
      for (long long p = Ap[j]; p < Ap[j + 1]; ++p)
        s += Av[p] * yy[Ai[p]];
      out[j] = s;
    }
  };
  auto P_times = [&](const double* xx, double* out) {
    for (int j = tid; j < n; j += NT)
    {
      double s = 0.0;
      for (long long p = Pp[j]; p < Pp[j + 1]; ++p)  // column j of the upper triangle = row j left of and on the diagonal
        s += Pv[p] * xx[Pi[p]];
      for (int p = Prp[j]; p < Prp[j + 1]; ++p)      // row j right of the diagonal
        s += Pv[Prk[p]] * xx[Prj[p]];
      out[j] = s;
    }
  };
  auto P_colmax = [&](int j) -> double {
    double cn = 0.0;
    for (long long p = Pp[j]; p < Pp[j + 1]; ++p)
      cn = fmax(cn, fabs(Pv[p]));
    for (int p = Prp[j]; p < Prp[j + 1]; ++p)
      cn = fmax(cn, fabs(Pv[Prk[p]]));
    return cn;
  };

  // ---- load -------------------------------------------------------------------------------------------------------------------
  for (long long p = tid; p < nnzP; p += NT)
    Pv[p] = d.P_x[g.oP + p];
  for (long long p = tid; p < nnzA; p += NT)
    Av[p] = d.A_x[g.oA + p];
  for (int j = tid; j < n; j += NT)
  {
    q[j] = d.q[g.ov_n + j];
    D[j] = 1.0;
  }
  for (int i = tid; i < m; i += NT)
  {
    l[i] = d.l[g.ov_m + i];
    u[i] = d.u[g.ov_m + i];
    E[i] = 1.0;
    flag[i] = 0;
  }
  TMX_SYNC();

  // ---- Ruiz equilibration (scale_data) ------------------------------------------------------------------------------------------
  double c = 1.0;
  for (int it = 0; it < st.scaling; ++it)
  {
    for (int j = tid; j < n; j += NT)
    {
      double cn = P_colmax(j);
      for (long long p = Ap[j]; p < Ap[j + 1]; ++p)
        cn = fmax(cn, fabs(Av[p]));
      tn[j] = 1.0 / sqrt(limit_scaling(cn));
    }
    for (int i = tid; i < m; i += NT)
    {
      double rn = 0.0;
      for (int p = Arp[i]; p < Arp[i + 1]; ++p)
        rn = fmax(rn, fabs(Av[Ark[p]]));
      tm[i] = 1.0 / sqrt(limit_scaling(rn));
    }
    TMX_SYNC();
    for (int j = tid; j < n; j += NT)
    {
      for (long long p = Pp[j]; p < Pp[j + 1]; ++p)
        Pv[p] = tn[Pi[p]] * Pv[p] * tn[j];
      for (long long p = Ap[j]; p < Ap[j + 1]; ++p)
        Av[p] = tm[Ai[p]] * Av[p] * tn[j];
      q[j] *= tn[j];
      D[j] *= tn[j];
    }
    for (int i = tid; i < m; i += NT)
      E[i] *= tm[i];
    TMX_SYNC();
    // cost normalisation: mean column inf-norm of P, ||q||_inf
    double qmax = 0.0;
    for (int j = tid; j < n; j += NT)
    {
      tn2[j] = P_colmax(j);
      qmax = fmax(qmax, fabs(q[j]));
    }
    TMX_SYNC();
    qmax = gen_max(qmax, red, tid, NT);
    double csum = 0.0;
    for (int j = 0; j < n; ++j)  // every thread the same serial sum: the oracle's order on every build
      csum += tn2[j];
    double ct = (n > 0) ? csum / (double)n : 0.0;
    ct = fmax(ct, limit_scaling(qmax));
    ct = 1.0 / limit_scaling(ct);
    TMX_SYNC();
    for (long long p = tid; p < nnzP; p += NT)
      Pv[p] *= ct;
    for (int j = tid; j < n; j += NT)
      q[j] *= ct;
    c *= ct;
    TMX_SYNC();
  }
  const double cinv = 1.0 / c;
  for (int i = tid; i < m; i += NT)
  {
    l[i] *= E[i];
    u[i] *= E[i];
  }
  TMX_SYNC();
  double rho_s = fmin(fmax(st.rho, TMX_RHO_MIN), TMX_RHO_MAX);
  for (int i = tid; i < m; i += NT)
  {
    ctype[i] = constr_type(l[i], u[i]);
    rho[i] = rho_of_type(ctype[i], rho_s);
  }
  for (int e = tid; e < npad; e += NT)
    bp[e] = 0.0;  // (the padding of the last block stays zero in every solve)
  TMX_SYNC();

  // ---- K = P + sig I + A' diag(wts) A in block storage, and its chain factorisation ----------------------------------------------
  // The thread of permuted row I owns that row of K_kk and of K_{k,k-1}; an entry of the block above the diagonal belongs to the
  // row it mirrors.  Order of the additions into one entry: P, sig, then the rows of A in the storage order of column perm[I].
  auto factor = [&](const double* wts, double sig) {
    CB_T0();
    for (int I = tid; I < npad; I += NT)
    {
      const int k = I / nb, li = I - k * nb;
      double *Kd = ch.Sv + (size_t)k * BB + (size_t)li * nb, *Kl = ch.Kl + (size_t)k * BB + (size_t)li * nb;
      for (int e = 0; e < nb; ++e)
      {
        Kd[e] = 0.0;
        Kl[e] = 0.0;
      }
      if (I >= n)
      {
        Kd[li] = 1.0;
        continue;
      }
      const int i = perm[I];
      auto add = [&](int j, double v) {
        const int J = pos[j], kb = J / nb;
        if (kb == k)
          Kd[J - kb * nb] += v;
        else if (kb == k - 1)
          Kl[J - kb * nb] += v;
      };
      for (long long p = Pp[i]; p < Pp[i + 1]; ++p)
        add((int)Pi[p], Pv[p]);
      for (int p = Prp[i]; p < Prp[i + 1]; ++p)
        add(Prj[p], Pv[Prk[p]]);
      Kd[li] += sig;
      for (long long p = Ap[i]; p < Ap[i + 1]; ++p)
      {
        const int r = (int)Ai[p];
        if (wts[r] == 0.0)
          continue;
        const double wa = wts[r] * Av[p];
        for (int pp = Arp[r]; pp < Arp[r + 1]; ++pp)
          add(Arj[pp], wa * Av[Ark[pp]]);
      }
    }
    TMX_SYNC();
    CB_T1(0);
    {
      CB_T0();
      if (g.place == 1)
        cb_factor<true>(ch, (cb_lds_d*)(smem + TMX_CB_LDS_FIXED), (cb_lds_d*)(smem + TMX_CB_LDS_FIXED + BB), gcol, grow, tid, NT);
      else
        cb_factor<false>(ch, (double*)nullptr, (double*)nullptr, gcol, grow, tid, NT);
      CB_T1(1);
    }
  };
  // out = K^-1 rhs (vectors in the caller's variable order)
  auto chain_solve = [&](const double* rhs, double* out) {
    CB_T0();
    for (int j = tid; j < n; j += NT)
      bp[pos[j]] = rhs[j];
    TMX_SYNC();
    cb_sweeps(ch, bp, yp, (cb_lds_d*)(smem + TMX_CB_LDS_FIXED), tid, NT);  // (the tiles of the factor step are dead here)
    for (int j = tid; j < n; j += NT)
      out[j] = bp[pos[j]];
    TMX_SYNC();
    CB_T1(2);
  };
  // out = K^-1 rhs with one step of iterative refinement against the sparse K:  r = rhs - (P out + sig out + A' (wts . A out))
  auto kkt_solve = [&](const double* rhs, double* out, const double* wts, double sig) {
    chain_solve(rhs, out);
    A_times(out, km);
    TMX_SYNC();
    for (int i = tid; i < m; i += NT)
      km[i] = wts[i] * km[i];
    TMX_SYNC();
    At_times(km, kc);
    P_times(out, kr);
    TMX_SYNC();
    for (int j = tid; j < n; j += NT)
      kr[j] = rhs[j] - ((kr[j] + sig * out[j]) + kc[j]);
    TMX_SYNC();
    chain_solve(kr, kc);
    for (int j = tid; j < n; j += NT)
      out[j] += kc[j];
    TMX_SYNC();
  };
  factor(rho, st.sigma);

  // ---- iterates -------------------------------------------------------------------------------------------------------------------
  for (int j = tid; j < n; j += NT)
    x[j] = g.warm ? (1.0 / D[j]) * d.xw[g.ov_n + j] : 0.0;
  for (int i = tid; i < m; i += NT)
    y[i] = g.warm ? ((1.0 / E[i]) * d.yw[g.ov_m + i]) * c : 0.0;
  TMX_SYNC();
  if (g.warm)
    A_times(x, z);
  else
    for (int i = tid; i < m; i += NT)
      z[i] = 0.0;
  TMX_SYNC();

  QpInfo info;
  info.status = 11;
  info.iter = 0;
  info.rho_updates = 0;
  info.polish_status = 0;
  info.prim_res = info.dual_res = 0.0;
  double s_prim = 0, s_dual = 0, s_z = 0, s_ax = 0, s_q = 0, s_aty = 0, s_px = 0, u_z = 0, u_ax = 0, u_q = 0, u_aty = 0, u_px = 0;
  auto residuals = [&](const double* xx, const double* zz, const double* yy, double& prim, double& dual) {
    A_times(xx, Ax);
    P_times(xx, Px);
    At_times(yy, Aty);
    TMX_SYNC();
    double mx[12];
    for (int k = 0; k < 12; ++k)
      mx[k] = 0.0;
    for (int i = tid; i < m; i += NT)
    {
      const double rr = Ax[i] - zz[i], ei = 1.0 / E[i];
      pres[i] = rr;
      mx[0] = fmax(mx[0], fabs(ei * rr));
      mx[1] = fmax(mx[1], fabs(rr));
      mx[2] = fmax(mx[2], fabs(zz[i]));
      mx[3] = fmax(mx[3], fabs(Ax[i]));
      mx[4] = fmax(mx[4], fabs(ei * zz[i]));
      mx[5] = fmax(mx[5], fabs(ei * Ax[i]));
    }
    for (int j = tid; j < n; j += NT)
    {
      const double rr = (q[j] + Px[j]) + Aty[j], di = 1.0 / D[j];
      dres[j] = rr;
      mx[6] = fmax(mx[6], fabs(di * rr));
      mx[7] = fmax(mx[7], fabs(rr));
      mx[8] = fmax(mx[8], fabs(q[j]));
      mx[9] = fmax(mx[9], fabs(Aty[j]));
      mx[10] = fmax(mx[10], fabs(Px[j]));
      mx[11] = fmax(mx[11], fabs(di * q[j]));
    }
    double ua = 0.0, up = 0.0;
    for (int j = tid; j < n; j += NT)
    {
      ua = fmax(ua, fabs(Aty[j] / D[j]));
      up = fmax(up, fabs(Px[j] / D[j]));
    }
    for (int k = 0; k < 12; ++k)
      mx[k] = gen_max(mx[k], red, tid, NT);
    ua = gen_max(ua, red, tid, NT);
    up = gen_max(up, red, tid, NT);
    prim = (m == 0) ? 0.0 : mx[0];
    dual = cinv * mx[6];
    s_prim = mx[1];
    s_z = mx[2];
    s_ax = mx[3];
    u_z = mx[4];
    u_ax = mx[5];
    s_dual = mx[7];
    s_q = mx[8];
    s_aty = mx[9];
    s_px = mx[10];
    u_q = mx[11];
    u_aty = ua;
    u_px = up;
  };
  auto prim_infeasible = [&](double eps) -> bool {
    const double BIG = TMX_OSQP_INFTY * TMX_MIN_SCALING;
    double nd = 0.0;
    for (int i = tid; i < m; i += NT)
    {
      double v = dy[i];
      if (u[i] > BIG)
        v = (l[i] < -BIG) ? 0.0 : fmin(v, 0.0);
      else if (l[i] < -BIG)
        v = fmax(v, 0.0);
      dy[i] = v;
      nd = fmax(nd, fabs(E[i] * v));
    }
    TMX_SYNC();
    nd = gen_max(nd, red, tid, NT);
    const double lhs = cb_sum(m, [&](int i) { const double v = dy[i]; return (v > 0) ? u[i] * v : ((v < 0) ? l[i] * v : 0.0); }, red, tid, NT);
    if (nd > TMX_DIVISION_TOL && lhs < 0.0)
    {
      At_times(dy, tn);
      TMX_SYNC();
      double nrm = 0.0;
      for (int j = tid; j < n; j += NT)
        nrm = fmax(nrm, fabs(tn[j] / D[j]));
      nrm = gen_max(nrm, red, tid, NT);
      return nrm < eps * nd;
    }
    return false;
  };
  auto dual_infeasible = [&](double eps) -> bool {
    double nd = 0.0;
    for (int j = tid; j < n; j += NT)
      nd = fmax(nd, fabs(D[j] * dx[j]));
    nd = gen_max(nd, red, tid, NT);
    const double qdx = cb_sum(n, [&](int j) { return q[j] * dx[j]; }, red, tid, NT);
    if (nd > TMX_DIVISION_TOL && qdx < 0.0)
    {
      P_times(dx, tn);
      TMX_SYNC();
      double nrm = 0.0;
      for (int j = tid; j < n; j += NT)
        nrm = fmax(nrm, fabs(tn[j] / D[j]));
      nrm = gen_max(nrm, red, tid, NT);
      if (nrm < c * eps * nd)
      {
        A_times(dx, tm);
        TMX_SYNC();
        const double BIG = TMX_OSQP_INFTY * TMX_MIN_SCALING, thr = eps * nd;
        double bad = 0.0;
        for (int i = tid; i < m; i += NT)
        {
          const double a = tm[i] / E[i];
          if (((u[i] < BIG) && (a > thr)) || ((l[i] > -BIG) && (a < -thr)))
            bad = 1.0;
        }
        bad = gen_max(bad, red, tid, NT);
        return bad == 0.0;
      }
    }
    return false;
  };
  auto check_termination = [&](bool approximate) -> bool {
    double ea = st.eps_abs, er = st.eps_rel, epi = st.eps_prim_inf, edi = st.eps_dual_inf;
    if (info.prim_res > TMX_OSQP_INFTY || info.dual_res > TMX_OSQP_INFTY)
    {
      info.status = 9;
      return true;
    }
    if (approximate)
    {
      ea *= 10;
      er *= 10;
      epi *= 10;
      edi *= 10;
    }
    bool pok = false, dok = false, pinf = false, dinf = false;
    if (m == 0)
      pok = true;
    else if (info.prim_res < ea + er * fmax(u_z, u_ax))
      pok = true;
    else
      pinf = prim_infeasible(epi);
    if (info.dual_res < ea + er * (cinv * fmax(fmax(u_q, u_aty), u_px)))
      dok = true;
    else
      dinf = dual_infeasible(edi);
    if (pok && dok)
    {
      info.status = approximate ? 2 : 1;
      return true;
    }
    if (pinf)
    {
      info.status = approximate ? 4 : 3;
      return true;
    }
    if (dinf)
    {
      info.status = approximate ? 6 : 5;
      return true;
    }
    return false;
  };

  int iter = 0;
  bool can_check = false, terminated = false;
  for (iter = 1; iter <= st.max_iter; ++iter)
  {
    // x_prev <- x, z_prev <- z ; rhs = sigma x_prev - q + A'(rho z_prev - y)
    for (int j = tid; j < n; j += NT)
      xprev[j] = x[j];
    for (int i = tid; i < m; i += NT)
    {
      zprev[i] = z[i];
      tm[i] = rho[i] * z[i] - y[i];
    }
    TMX_SYNC();
    At_times(tm, tn);
    TMX_SYNC();
    for (int j = tid; j < n; j += NT)
      tn[j] = (st.sigma * xprev[j] - q[j]) + tn[j];
    TMX_SYNC();
    kkt_solve(tn, xt, rho, st.sigma);
    A_times(xt, zt);
    TMX_SYNC();
    for (int j = tid; j < n; j += NT)
    {
      x[j] = st.alpha * xt[j] + (1.0 - st.alpha) * xprev[j];
      dx[j] = x[j] - xprev[j];
    }
    for (int i = tid; i < m; i += NT)
    {
      const double zr = st.alpha * zt[i] + (1.0 - st.alpha) * zprev[i];
      const double zn = clampd(zr + (1.0 / rho[i]) * y[i], l[i], u[i]);
      dy[i] = rho[i] * (zr - zn);
      z[i] = zn;
      y[i] += dy[i];
    }
    TMX_SYNC();
    can_check = st.check_termination && (iter % st.check_termination == 0);
    const bool do_rho = st.adaptive_rho && st.adaptive_rho_interval && (iter % st.adaptive_rho_interval == 0);
    if (can_check || do_rho)
    {
      info.iter = iter;
      residuals(x, z, y, info.prim_res, info.dual_res);
    }
    if (can_check && check_termination(false))
    {
      terminated = true;
      break;
    }
    if (do_rho && m > 0)
    {
      const double prim = s_prim / (fmax(s_z, s_ax) + TMX_DIVISION_TOL);
      const double dual = s_dual / (fmax(fmax(s_q, s_aty), s_px) + TMX_DIVISION_TOL);
      const double est = fmin(fmax(rho_s * sqrt(prim / dual), TMX_RHO_MIN), TMX_RHO_MAX);
      if (est > rho_s * st.adaptive_rho_tolerance || est < rho_s / st.adaptive_rho_tolerance)
      {
        rho_s = fmin(fmax(est, TMX_RHO_MIN), TMX_RHO_MAX);
        info.rho_updates += 1;
        for (int i = tid; i < m; i += NT)
          rho[i] = rho_of_type(ctype[i], rho_s);
        TMX_SYNC();
        factor(rho, st.sigma);
      }
    }
  }
  const int exit_iter = terminated ? iter : iter - 1;
  if (!can_check)
  {
    info.iter = exit_iter;
    residuals(x, z, y, info.prim_res, info.dual_res);
    check_termination(false);
  }
  if (info.status == 11 && !check_termination(true))
    info.status = 7;

  // ---- polish ---------------------------------------------------------------------------------------------------------------------
  // OSQP solves [P + delta I, Aact'; Aact, -delta I] (dx; dy) = (r1; r2); eliminating dy = (Aact dx - r2) / delta leaves the reduced
  // system (P + delta I + Aact' Aact / delta) dx = r1 + Aact' r2 / delta on the blocks of K.  First solve with (r1; r2) = (-q; b),
  // then polish_refine_iter corrections against the residual of the UNPERTURBED system [P, Aact'; Aact, 0].
  if (st.polishing && info.status == 1)
  {
#if TMX_CB_PROF
    cb_in_polish = true;
    const long long cb_polish_start = tmx_wall_ticks();
#endif
    const double dinv = 1.0 / st.delta;
    for (int i = tid; i < m; i += NT)
    {
      flag[i] = (z[i] - l[i] < -y[i]) ? -1 : ((u[i] - z[i] < y[i]) ? 1 : 0);
      pw[i] = flag[i] != 0 ? dinv : 0.0;
      pb[i] = flag[i] < 0 ? l[i] : (flag[i] > 0 ? u[i] : 0.0);
      py[i] = 0.0;
    }
    for (int j = tid; j < n; j += NT)
      px[j] = 0.0;
    TMX_SYNC();
    factor(pw, st.delta);
    for (int pass = 0; pass <= st.polish_refine_iter; ++pass)
    {
      // (r1; r2): the right-hand side itself in the first pass, the unperturbed residual at (px, py) afterwards
      if (pass == 0)
      {
        for (int j = tid; j < n; j += NT)
          pr1[j] = -q[j];
        for (int i = tid; i < m; i += NT)
          pr2[i] = pb[i];
      }
      else
      {
        P_times(px, Px);
        At_times(py, Aty);
        A_times(px, Ax);
        TMX_SYNC();
        for (int j = tid; j < n; j += NT)
          pr1[j] = (-q[j] - Px[j]) - Aty[j];
        for (int i = tid; i < m; i += NT)
          pr2[i] = flag[i] != 0 ? pb[i] - Ax[i] : 0.0;
      }
      TMX_SYNC();
      for (int i = tid; i < m; i += NT)
        tm[i] = pw[i] * pr2[i];
      TMX_SYNC();
      At_times(tm, tn);
      TMX_SYNC();
      for (int j = tid; j < n; j += NT)
        tn[j] = pr1[j] + tn[j];
      TMX_SYNC();
      kkt_solve(tn, pdx, pw, st.delta);
      A_times(pdx, Ax);
      TMX_SYNC();
      for (int j = tid; j < n; j += NT)
        px[j] += pdx[j];
      for (int i = tid; i < m; i += NT)
        py[i] += pw[i] * (Ax[i] - pr2[i]);
      TMX_SYNC();
    }
    A_times(px, pz);
    TMX_SYNC();
    for (int i = tid; i < m; i += NT)
      pz[i] = clampd(pz[i], l[i], u[i]);
    TMX_SYNC();
    double pp = 0.0, pd = 0.0;
    residuals(px, pz, py, pp, pd);
    const bool ok = (pp < info.prim_res && pd < info.dual_res) || (pp < info.prim_res && info.dual_res < 1e-10) ||
                    (pd < info.dual_res && info.prim_res < 1e-10);
    if (ok)
    {
      info.polish_status = 1;
      info.prim_res = pp;
      info.dual_res = pd;
      for (int j = tid; j < n; j += NT)
        x[j] = px[j];
      for (int i = tid; i < m; i += NT)
      {
        z[i] = pz[i];
        y[i] = py[i];
      }
    }
    else
      info.polish_status = -1;
    TMX_SYNC();
#if TMX_CB_PROF
    cb_prof[3] = tmx_wall_ticks() - cb_polish_start;
#endif
  }

  // ---- store ----------------------------------------------------------------------------------------------------------------------
  const bool has_sol = !(info.status == 3 || info.status == 4 || info.status == 5 || info.status == 6 || info.status == 9);
  for (int j = tid; j < n; j += NT)
    d.x_out[g.ov_n + j] = has_sol ? D[j] * x[j] : NAN;
  for (int i = tid; i < m; i += NT)
  {
    d.y_out[g.ov_m + i] = has_sol ? (cinv * E[i]) * y[i] : NAN;
    if (d.flags_out)
      d.flags_out[g.ov_m + i] = flag[i];
  }
  if (tid == 0)
  {
    tmx_qp_info& o = d.info[g.slot];
    o.osqp_status = info.status;
    o.iter = (info.iter == 0) ? exit_iter : info.iter;
    o.rho_updates = info.rho_updates;
    o.polish_status = info.polish_status;
    o.rho_final = rho_s;
    o.prim_res = info.prim_res;
    o.dual_res = info.dual_res;
#if TMX_CB_PROF
    cb_prof[7] = tmx_wall_ticks() - cb_start;
    for (int k = 0; k < 8; ++k)
      dd.prof[(size_t)g.slot * 8 + k] = cb_prof[k];
#endif
  }
  TMX_SYNC();
}

TMX_KERNEL_LB(256) k_qp_csc_blocks(const CbQp* qps, CbData d, tmx_osqp_settings st)
{
  TMX_SMEM(smem);
  qp_csc_blocks_block(qps[blockIdx.x], d, st, smem, threadIdx.x, blockDim.x);
}
