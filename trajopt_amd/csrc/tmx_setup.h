// Ruiz equilibration (scale_data) of the dense fast path with the matrix in registers.
//
// The generic scaling of qp_solve_block (tmx_solve.h) keeps every entry in LDS, walks index lists through dependent loads, tests
// the features the fast-path predicate has excluded and crosses about ten workgroup barriers per pass.  Here the ownership is the
// register-resident burst's (admm_burst_core, tmx_part.h): a thread holds up to two constraint rows (DevProblem::row_perm) with their
// slack entries and running scalings, thread v < NX holds primary variable v with its objective entries, its own copy of the coupling
// po[v - D] and column v of A over the row list of its waypoint.  A pass is: maxima over the thread's own registers, the
// 1 / sqrt(limit_scaling(.)) of everything the thread owns, ONE exchange (D_v into tp with 8 slots per waypoint, E_r into hr grouped by
// waypoint at row_epos - the burst's buffers and index tables), one barrier, the scaling of both copies of an entry by the same
// expression on the same operands, and one block_reduce<2> for the cost normalisation.
//
// What keeps the bits (tests/test_fast_setup.py compares with the generic code through DevProblem::dbg_flags bit 1):
//  * a scaled entry is (E * a) * D, running products are X *= d once per pass, 1.0 / sqrt(x) is the IEEE square root and division
//  * maxima do not depend on the order; inactive rows hold exact zeros on this path (no compact lists) and write nothing
//  * the column-norm sum: thread tid contributes the value of variable tid to the tree of block_reduce, as the generic code does; the
//    maximum of |q| goes through the same call as a second value (every value sees its own tree)
//  * c_temp is formed by every thread from the two block-uniform results instead of by thread 0 with a broadcast: same operations
#pragma once
#include "tmx_qp.h"

#if TMX_IS_DEVICE
// Exclusive prefix over the workgroup (TMX_QP_NT threads, thread order) of a per-thread count below 8: inside the wave by ballots of
// the count's three bits, then the totals of the waves below through `scan` (one int per wave).  Integers - any order is exact.
// Starts with a barrier (the last readers of `scan` are past it) and ends after the one that publishes the wave totals.
TMX_DEVFN int block_excl_count8(int cnt, int* scan, int tid)
{
  const int lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  int off = 0, tot = 0;
  for (int bit = 0; bit < 3; ++bit)
  {
    const unsigned long long mk = __builtin_amdgcn_ballot_w64(((cnt >> bit) & 1) != 0);
    off += __builtin_popcountll(mk & below) << bit;
    tot += __builtin_popcountll(mk) << bit;
  }
  TMX_SYNC();
  if (lane == 0)
    scan[wave] = tot;
  TMX_SYNC();
  for (int u = 0; u < wave; ++u)
    off += scan[u];
  return off;
}

struct SetupRow
{
  int r, t, na, ao, epos;
  bool on;  // the thread holds this row and it is active
  double c[8], sa[2], bba[2], qa[2], Da[2], Eba[2], Er;
};

// rows_max <= TMX_SETUP_COL rows per waypoint, naux <= 2, R <= 2 NT, one thread per primary variable (DevProblem::setup_fast and the
// fast-path predicate); n = number of QP variables (dims[0]); returns the cost scaling c.  Leaves coef, sa, bba, qa, Er, Eba, Da, pd, po,
// bbp, qp, Dp, Ebp and the scaled bounds with their constraint types where the generic code leaves them.
TMX_DEVFN double ruiz_fast(const QpWs& w, const DevProblem* P, int n_pass, int n, int tid)
{
  constexpr int NT = TMX_QP_NT;
  const int D = w.D, T = w.T, NX = w.NX, R = w.R;
  // slots no thread writes (pad joints of tp, groups of inactive rows and pads of hr) are multiplied by exact zeros: keep them finite
  for (int e = tid; e < T * 8; e += NT)
    w.tp[e] = 0.0;
  for (int e = tid; e < R + T + TMX_SETUP_COL; e += NT)
    w.hr[e] = 0.0;
  SetupRow g[2];
  {
    const int* rperm = P->row_perm;
#pragma unroll
    for (int q = 0; q < 2; ++q)
    {
      SetupRow& s = g[q];
      const int slot = q * NT + tid;
      s.r = rperm ? rperm[slot] : (slot < R ? slot : -1);
      s.on = s.r >= 0 && s.r < R && w.act[s.r >= 0 && s.r < R ? s.r : 0] != 0;
      const int r = s.on ? s.r : 0;
      s.t = w.slot_t[r];
      s.na = s.on ? w.naux[r] : 0;
      s.ao = w.aoff[r];
      s.epos = w.row_epos[r];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        s.c[j] = (s.on && j < D) ? w.coef[r * D + j] : 0.0;
#pragma unroll
      for (int k = 0; k < 2; ++k)
      {
        const bool ok = k < s.na;
        s.sa[k] = ok ? w.sa[s.ao + k] : 0.0;
        s.qa[k] = ok ? w.qa[s.ao + k] : 0.0;
        s.bba[k] = ok ? w.bba[s.ao + k] : 0.0;
        s.Da[k] = 1.0;
        s.Eba[k] = 1.0;
      }
      s.Er = 1.0;
    }
  }
  const bool pv = tid < NX;
  const int v = pv ? tid : 0, vt = v / D, vj = v - vt * D;
  const bool has_prev = pv && vt > 0, has_next = pv && vt < T - 1;
  double pd = pv ? w.pd[v] : 0.0, po = pv ? w.po[v] : 0.0, pop = has_prev ? w.po[v - D] : 0.0;
  double bbp = pv ? w.bbp[v] : 0.0, qp = pv ? w.qp[v] : 0.0, Dp = 1.0, Ebp = 1.0;
  double cj[TMX_SETUP_COL];
  const int e0 = w.wp_pst[vt];
  {
    const int q0 = w.wp_start[vt], q1 = w.wp_start[vt + 1];
#pragma unroll
    for (int k = 0; k < TMX_SETUP_COL; ++k)
    {
      const bool ok = pv && q0 + k < q1;
      const int r = ok ? w.wp_list[q0 + k] : 0;
      cj[k] = ok ? w.coef[r * D + vj] : 0.0;
    }
  }
  double c_run = 1.0;
  TMX_SYNC();
  for (int it = 0; it < n_pass; ++it)
  {
    double dv = 0.0, ebp = 0.0;
    if (pv)
    {
      double cn = fabs(pd);
      if (has_prev)
        cn = fmax(cn, fabs(pop));
      if (has_next)
        cn = fmax(cn, fabs(po));
#pragma unroll
      for (int k = 0; k < TMX_SETUP_COL; ++k)
        cn = fmax(cn, fabs(cj[k]));
      cn = fmax(cn, fabs(bbp));
      dv = 1.0 / sqrt(limit_scaling(cn));
      ebp = 1.0 / sqrt(limit_scaling(fabs(bbp)));
      w.tp[vt * 8 + vj] = dv;
    }
    double er[2] = { 0.0, 0.0 }, da[2][2] = { { 0.0, 0.0 }, { 0.0, 0.0 } }, eba[2][2] = { { 0.0, 0.0 }, { 0.0, 0.0 } };
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (g[q].on)
      {
        SetupRow& s = g[q];
        double rn = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          rn = fmax(rn, fabs(s.c[j]));
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (k < s.na)
          {
            rn = fmax(rn, fabs(s.sa[k]));
            da[q][k] = 1.0 / sqrt(limit_scaling(fmax(fabs(s.sa[k]), fabs(s.bba[k]))));
            eba[q][k] = 1.0 / sqrt(limit_scaling(fabs(s.bba[k])));
          }
        er[q] = 1.0 / sqrt(limit_scaling(rn));
        w.hr[s.epos] = er[q];
      }
    TMX_SYNC();
    if (pv)
    {
      const double dn = has_next ? w.tp[(vt + 1) * 8 + vj] : 0.0, dl = has_prev ? w.tp[(vt - 1) * 8 + vj] : 0.0;
      pd = (dv * pd) * dv;
      if (has_next)
        po = (dv * po) * dn;
      if (has_prev)
        pop = (dl * pop) * dv;
      bbp = (ebp * bbp) * dv;
      qp *= dv;
      Dp *= dv;
      Ebp *= ebp;
#pragma unroll
      for (int k = 0; k < TMX_SETUP_COL; ++k)
        cj[k] = (w.hr[e0 + k] * cj[k]) * dv;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (g[q].on)
      {
        SetupRow& s = g[q];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          s.c[j] = (er[q] * s.c[j]) * w.tp[s.t * 8 + j];
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (k < s.na)
          {
            s.sa[k] = (er[q] * s.sa[k]) * da[q][k];
            s.bba[k] = (eba[q][k] * s.bba[k]) * da[q][k];
            s.qa[k] *= da[q][k];
            s.Da[k] *= da[q][k];
            s.Eba[k] *= eba[q][k];
          }
        s.Er *= er[q];
      }
    // cost normalisation: mean column inf-norm of P (aux columns are empty), ||q||_inf
    double nrm[2] = { 0.0, 0.0 };  // max |q|, sum of the column norms
    if (pv)
    {
      double cn = fabs(pd);
      if (has_prev)
        cn = fmax(cn, fabs(pop));
      if (has_next)
        cn = fmax(cn, fabs(po));
      nrm[1] = cn;
      nrm[0] = fabs(qp);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (g[q].on)
      {
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (k < g[q].na)
            nrm[0] = fmax(nrm[0], fabs(g[q].qa[k]));
      }
    {
      const bool issum[2] = { false, true };
      block_reduce<2>(nrm, issum, w.red, tid, NT);
    }
    double c_temp = nrm[1] / (double)n;
    c_temp = fmax(c_temp, limit_scaling(nrm[0]));
    c_temp = limit_scaling(c_temp);
    const double ct = 1.0 / c_temp;
    pd *= ct;
    po *= ct;
    pop *= ct;
    qp *= ct;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int k = 0; k < 2; ++k)
        g[q].qa[k] *= ct;
    c_run *= ct;
  }
  if (pv)
  {
    w.pd[v] = pd;
    w.po[v] = po;
    w.bbp[v] = bbp;
    w.qp[v] = qp;
    w.Dp[v] = Dp;
    w.Ebp[v] = Ebp;
    const double lb = w.lbp[v] * Ebp, ub = w.ubp[v] * Ebp;
    w.lbp[v] = lb;
    w.ubp[v] = ub;
    w.typ_bp[v] = constr_type(lb, ub);
  }
#pragma unroll
  for (int q = 0; q < 2; ++q)
    if (g[q].on)
    {
      const SetupRow& s = g[q];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < D)
          w.coef[s.r * D + j] = s.c[j];
#pragma unroll
      for (int k = 0; k < 2; ++k)
        if (k < s.na)
        {
          const int a = s.ao + k;
          w.sa[a] = s.sa[k];
          w.bba[a] = s.bba[k];
          w.qa[a] = s.qa[k];
          w.Da[a] = s.Da[k];
          w.Eba[a] = s.Eba[k];
          w.typ_ba[a] = constr_type(0.0, TMX_OSQP_INFTY * s.Eba[k]);
        }
      w.Er[s.r] = s.Er;
      const double lo = w.lor[s.r] * s.Er, hi = w.hir[s.r] * s.Er;
      w.lor[s.r] = lo;
      w.hir[s.r] = hi;
      w.typ_r[s.r] = constr_type(lo, hi);
    }
  TMX_SYNC();
  return c_run;
}
#endif
