// Polish (polish.c) of the dense fast path with the iterate in registers.
//
// The generic polish of qp_solve_block (tmx_solve.h) and kkt_solve(mode 1) (tmx_qp.h) walk TMX_ROWS sweeps and index lists through
// dependent loads and generic pointers, divide every variable index by D in every pass and form the pass-invariant parts of the aux
// elimination (dk, dmin, dmin / dk, den, dmin / den: IEEE divisions on operands that only depend on the active-set guess) twice per row
// in each of the four solves.  Here the ownership is the register-resident burst's (admm_burst_core, tmx_part.h) and ruiz_fast's
// (tmx_setup.h): a thread holds up to two constraint rows (DevProblem::row_perm) from the active-set guess to the final copy - their
// coefficients, slack entries, flags, the invariants above and the running dy_r / dx_a / dy_ba -, thread v < NX holds primary variable
// v with its objective entries, its flag, dx_p / dy_bp and column v of A over the row list of its waypoint.  LDS carries the exchanged
// vectors only, through address_space(3) pointers: the row values grouped by waypoint at row_epos (c_r of the elimination in hr, the
// running dy_r in the dead G region), the running dx_p with 8 slots per waypoint (G region), and the right-hand side / solution of the
// block chain in tp with the chain's own stride D.  A pass crosses four workgroup barriers.
//
// Called, not copied: kkt_factor(mode 1), kkt_invert (the one-wave chain factor), chain_diag_sweep.
//
// What keeps the bits (tests/test_fast_polish.py compares with the generic code through DevProblem::dbg_flags bit 2):
//  * every value comes from the expression of the generic code on the same operands; a division whose operands change from pass to pass
//    stays a division (num / den, (ta - sa nu) / dk, r2 / delta)
//  * the gather of kkt_solve adds s + h * c in wp_list order from 0.0 and SKIPS inactive rows (a select, not + h * 0.0: the partial sum may
//    be -0.0); the A'y sums of the refinement right-hand side and of the residuals keep at_rows' four partial sums over ALL slots of the
//    waypoint - the slots of inactive rows hold +0.0 in the grouped buffers (nothing writes them) against a +0.0 coefficient
//  * the two residuals the acceptance test reads are maxima: the order is free (block_reduce, as compute_residuals)
#pragma once
#include "tmx_qp.h"

// LDS doubles the fast polish lays over the G region: dx_p (8 per waypoint), dy_r grouped by waypoint (n_grouped = wp_pst[T] +
// TMX_SETUP_COL), the three flag arrays
TMX_HOSTDEVFN size_t polish_fast_doubles(int T, int NX, int R, int NA, int n_grouped)
{
  return (size_t)T * 8 + (size_t)n_grouped + ((size_t)R + NX + NA + 1) / 2 + 2;
}

#if TMX_IS_DEVICE
TMX_DEVFN void kkt_invert(const QpWs& w, bool partitioned, int tid, int NT, long long* pc, long long& tlast);  // tmx_solve.h

typedef __attribute__((address_space(3))) int tmx_lds_i;
#if defined(TMX_PROFILE) && defined(TMX_FINE)
// (-DTMX_PROFILE -DTMX_FINE=1: the slots of kkt_solve(mode 1)'s split - 13 row phase, 14 gather, 15 chain, 6 recovery; the rest stays in 7)
#define TMX_POLISH_TICK(slot)                                                                                         \
  do                                                                                                                  \
  {                                                                                                                   \
    if (TMX_FINE == 1)                                                                                                \
      TMX_TICK(slot);                                                                                                 \
  } while (0)
#else
#define TMX_POLISH_TICK(slot) ((void)0)
#endif

struct PolishRow
{
  int r, t, na, ao, epos, f, fa[2];
  bool on;  // the thread holds this row and it is active
  double c[8], sa[2], bba[2], qa[2];
  double r2, r2a[2];                          // the bound the flag selects (row; slack bounds)
  double dk[2], dmin, ratio[2], den, dmden;   // invariants of the aux elimination
  double ta[2], cr, dyr, dxa[2], dyba[2];
};

// Preconditions: the fast-path predicate of qp_solve_block, DevProblem::polish_fast, no long-horizon partition (w.WL == nullptr).
// In: the ADMM iterate in (xp, xa | zr, zbp, zba | yr, ybp, yba), info.prim_res / dual_res.  Out: info.polish_status and, when the polished
// point is accepted, the iterate and the two residuals replaced; flg_r / flg_bp / flg_ba hold the active-set guess.
TMX_DEVFN void polish_fast(const QpWs& w, const DevProblem* P, double delta, int n_refine, QpInfo& info, int tid, [[maybe_unused]] long long* pc,
                           [[maybe_unused]] long long& tlast)
{
  constexpr int NT = TMX_QP_NT;
  const int D = __builtin_amdgcn_readfirstlane(w.D), T = __builtin_amdgcn_readfirstlane(w.T), NX = __builtin_amdgcn_readfirstlane(w.NX),
            R = __builtin_amdgcn_readfirstlane(w.R), NA = __builtin_amdgcn_readfirstlane(P->NA);
#define TMX_LDS_PTR(p) ((tmx_lds_d*)(size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(p)))
  tmx_lds_d* const C = TMX_LDS_PTR(w.hr);  // c_r of the elimination, grouped by waypoint
  tmx_lds_d* const TP = TMX_LDS_PTR(w.tp); // right-hand side / solution of the chain (stride D)
  tmx_lds_d* const X = TMX_LDS_PTR(w.G);   // running dx_p, 8 slots per waypoint
#undef TMX_LDS_PTR
  const int ny = __builtin_amdgcn_readfirstlane(w.wp_pst[T]) + TMX_SETUP_COL;
  tmx_lds_d* const Y = X + T * 8;          // running dy_r, grouped by waypoint
  tmx_lds_i* const Fr = (tmx_lds_i*)(Y + ny);
  tmx_lds_i* const Fbp = Fr + R;
  tmx_lds_i* const Fba = Fbp + NX;
  QpWs wp = w;  // what kkt_factor / kkt_invert see: the flags of this polish
  wp.flg_r = reinterpret_cast<int*>(w.G + T * 8 + ny);
  wp.flg_bp = wp.flg_r + R;
  wp.flg_ba = wp.flg_bp + NX;
  // slots no thread writes: the pad joints of X, the groups of inactive rows and the pads of Y meet +0.0 coefficients (keep them +0.0),
  // inactive rows and their slacks keep flag 0 (the solution store hashes every flag)
  for (int e = tid; e < T * 8 + ny; e += NT)
    X[e] = 0.0;
  for (int e = tid; e < R; e += NT)
    Fr[e] = 0;
  for (int e = tid; e < NA; e += NT)
    Fba[e] = 0;
  // ---- the thread's rows and its primary variable, the active-set guess
  PolishRow g[2];
  {
    const int* rperm = P->row_perm;
#pragma unroll
    for (int q = 0; q < 2; ++q)
    {
      PolishRow& s = g[q];
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
      s.f = 0;
      if (s.on)
      {
        if (w.zr[r] - w.lor[r] < -w.yr[r])
          s.f = -1;
        else if (w.hir[r] - w.zr[r] < w.yr[r])
          s.f = 1;
      }
      s.r2 = (s.f < 0) ? w.lor[r] : w.hir[r];
#pragma unroll
      for (int k = 0; k < 2; ++k)
      {
        const bool ok = k < s.na;
        const int a = ok ? s.ao + k : 0;
        s.sa[k] = ok ? w.sa[a] : 0.0;
        s.qa[k] = ok ? w.qa[a] : 0.0;
        s.bba[k] = ok ? w.bba[a] : 0.0;
        s.fa[k] = 0;
        if (ok)
        {
          if (w.zba[a] - 0.0 < -w.yba[a])
            s.fa[k] = -1;
          else if (TMX_OSQP_INFTY * w.Eba[a] - w.zba[a] < w.yba[a])
            s.fa[k] = 1;
        }
        s.r2a[k] = (s.fa[k] < 0) ? 0.0 : TMX_OSQP_INFTY * w.Eba[a];
        s.ta[k] = s.dxa[k] = s.dyba[k] = 0.0;
      }
      s.cr = s.dyr = 0.0;
    }
  }
  const bool pv = tid < NX;
  const int v = pv ? tid : 0, vt = v / D, vj = v - vt * D;
  const bool has_prev = pv && vt > 0, has_next = pv && vt < T - 1;
  const double pd = w.pd[v], po = w.po[v], pop = has_prev ? w.po[v - D] : 0.0, bbp = w.bbp[v], qp = w.qp[v], lbp = w.lbp[v], ubp = w.ubp[v];
  int fbp = 0;
  if (w.zbp[v] - lbp < -w.ybp[v])
    fbp = -1;
  else if (ubp - w.zbp[v] < w.ybp[v])
    fbp = 1;
  const double r2bp = (fbp < 0) ? lbp : ubp;
  double dxp = 0.0, dybp = 0.0;
  // column v of A over the row list of its waypoint, which of those rows are active, the list's length
  double cj[TMX_SETUP_COL];
  unsigned amask = 0;
  const int e0 = w.wp_pst[vt];
  int nl = 0;
  {
    const int q0 = w.wp_start[vt], q1 = w.wp_start[vt + 1];
    nl = pv ? q1 - q0 : 0;
#pragma unroll
    for (int k = 0; k < TMX_SETUP_COL; ++k)
    {
      const bool ok = pv && q0 + k < q1;
      const int r = ok ? w.wp_list[q0 + k] : 0;
      cj[k] = ok ? w.coef[r * D + vj] : 0.0;
      amask |= (ok && w.act[r] != 0) ? (1u << k) : 0u;
    }
  }
  const int nl4 = nl & ~3;
  TMX_SYNC();
#pragma unroll
  for (int q = 0; q < 2; ++q)
    if (g[q].on)
    {
      Fr[g[q].r] = g[q].f;
#pragma unroll
      for (int k = 0; k < 2; ++k)
        if (k < g[q].na)
          Fba[g[q].ao + k] = g[q].fa[k];
    }
  if (pv)
    Fbp[v] = fbp;
  TMX_SYNC();
  kkt_factor(wp, P, 1, delta, delta, tid, NT);
  kkt_invert(wp, false, tid, NT, pc, tlast);
  TMX_SYNC();  // kkt_factor kept the effective row weights in hr
  for (int e = tid; e < ny; e += NT)
    C[e] = 0.0;
  // ---- invariants of the aux elimination (kkt_solve(mode 1): row phase and recovery of every solve)
#pragma unroll
  for (int q = 0; q < 2; ++q)
  {
    PolishRow& s = g[q];
    s.dk[0] = s.dk[1] = 1.0;
    s.dmin = 1.0;
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (k < s.na)
      {
        s.dk[k] = delta + (s.fa[k] != 0 ? 1.0 / delta : 0.0) * s.bba[k] * s.bba[k];
        s.dmin = (k == 0) ? s.dk[k] : fmin(s.dmin, s.dk[k]);
      }
    s.den = s.dmin * delta;
    s.ratio[0] = s.ratio[1] = 0.0;
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (k < s.na)
      {
        s.ratio[k] = s.dmin / s.dk[k];
        s.den += s.sa[k] * s.sa[k] * s.ratio[k];
      }
    s.dmden = s.dmin / s.den;
  }
  // (A'y)_v over the grouped dy_r: at_rows' four partial sums over all slots of the waypoint, the remainder into the first
  auto aty_rows = [&]() __attribute__((always_inline)) -> double {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int k = 0; k < TMX_SETUP_COL; ++k)
    {
      const double pr = cj[k] * Y[e0 + k];
      if (k < nl4)
      {
        if ((k & 3) == 0)
          s0 += pr;
        else if ((k & 3) == 1)
          s1 += pr;
        else if ((k & 3) == 2)
          s2 += pr;
        else
          s3 += pr;
      }
      else if (k < nl)
        s0 += pr;
    }
    return (s0 + s1) + (s2 + s3);
  };
  // (P x)_v at the running dx_p
  auto p_times_x = [&]() __attribute__((always_inline)) -> double {
    double s = pd * dxp;
    if (has_prev)
      s += pop * X[(vt - 1) * 8 + vj];
    if (has_next)
      s += po * X[(vt + 1) * 8 + vj];
    return s;
  };
  // a_r . dx_p + s_r . dx_a at the running iterate
  auto row_ax = [&](const PolishRow& s) __attribute__((always_inline)) -> double {
    double ax = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < D)
        ax += s.c[j] * X[s.t * 8 + j];
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (k < s.na)
        ax += s.sa[k] * s.dxa[k];
    return ax;
  };
  const bool chain_lds = tmx_in_lds(w.Sinv) && tmx_in_lds(w.tp) && tmx_in_lds(TMX_PC(w));
  TMX_SYNC();
  TMX_POLISH_TICK(7);
  // ---- the solve and its refinements; the polished iterate is (dxp, dxa | dyr, dybp, dyba)
  // (with fewer than three refinement passes, two passes against the REGULARISED system first: the generic polish, tmx_solve.h)
  const int n_reg = n_refine < 3 ? 2 : 0;
  for (int pass = 0; pass <= n_reg + n_refine; ++pass)
  {
    const bool reg = pass >= 1 && pass <= n_reg;
    // residual-form rhs: pass 0: r1 = -q, r2 = b ; pass > 0: r1 = -q - P x - Aact' y, r2 = b - Aact x
    double hrv[2] = { 0.0, 0.0 };
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (g[q].on)
      {
        PolishRow& s = g[q];
        if (s.f != 0)
        {
          double r2 = s.r2;
          if (pass > 0)
            r2 -= row_ax(s);
          if (reg)
            r2 += delta * s.dyr;
          hrv[q] = r2;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (k < s.na)
          {
            double r1 = -s.qa[k];
            double gb = 0.0;
            if (s.fa[k] != 0)
            {
              double r2 = s.r2a[k];
              if (pass > 0)
                r2 -= s.bba[k] * s.dxa[k];
              if (reg)
                r2 += delta * s.dyba[k];
              gb = r2 / delta;
            }
            if (pass > 0)
              r1 -= s.sa[k] * s.dyr + s.bba[k] * s.dyba[k];
            if (reg)
              r1 -= delta * s.dxa[k];
            s.ta[k] = r1 + s.bba[k] * gb;
          }
      }
    double rhs = 0.0;
    if (pv)
    {
      double r1 = -qp;
      double gb = 0.0;
      if (fbp != 0)
      {
        double r2 = r2bp;
        if (pass > 0)
          r2 -= bbp * dxp;
        if (reg)
          r2 += delta * dybp;
        gb = r2 / delta;
      }
      if (pass > 0)
        r1 -= p_times_x() + aty_rows() + bbp * dybp;
      if (reg)
        r1 -= delta * dxp;
      rhs = r1 + bbp * gb;
    }
    TMX_POLISH_TICK(7);
    // row phase: c_r = (r2 - sum s_k ta_k / d_k) / (delta + sum s_k^2 / d_k), numerator and denominator scaled by d_min
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (g[q].on)
      {
        PolishRow& s = g[q];
        double c = 0.0;
        if (s.f != 0)
        {
          double num = s.dmin * hrv[q];
#pragma unroll
          for (int k = 0; k < 2; ++k)
            if (k < s.na)
              num -= s.sa[k] * s.ta[k] * s.ratio[k];
          c = num / s.den;
        }
        s.cr = c;
        C[s.epos] = c;
      }
    TMX_SYNC();
    TMX_POLISH_TICK(13);
    // gather tp[v] += sum_r c_r coef[r][j] over the active rows of the waypoint, in list order
    if (pv)
    {
      double sg = 0.0;
#pragma unroll
      for (int k = 0; k < TMX_SETUP_COL; ++k)
      {
        const double h = C[e0 + k];
        sg = ((amask >> k) & 1u) ? sg + h * cj[k] : sg;
      }
      TP[v] = rhs + sg;
    }
    TMX_SYNC();
    TMX_POLISH_TICK(14);
    // block chain: one wave, the running vector in registers
    if (tid < 64)
    {
      if (chain_lds)
        chain_diag_sweep_d((tmx_dsw_clds*)w.Sinv, (tmx_dsw_clds*)TMX_PC(w), (tmx_dsw_lds*)w.tp, D, w.DS, w.DDS, T, tid);
      else
        chain_diag_sweep_d((const double*)w.Sinv, (const double*)TMX_PC(w), w.tp, D, w.DS, w.DDS, T, tid);
    }
    TMX_SYNC();
    TMX_POLISH_TICK(15);
    // recovery (nu_r, slack update) and the update of the polished iterate
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (g[q].on)
      {
        PolishRow& s = g[q];
        double dot = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (j < D)
            dot += s.c[j] * TP[s.t * D + j];
        double nu = 0.0;
        if (s.f != 0)
          nu = dot * s.dmden - s.cr;
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (k < s.na)
            s.ta[k] = (s.ta[k] - s.sa[k] * nu) / s.dk[k];
        s.cr = nu;
      }
    TMX_POLISH_TICK(6);
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (g[q].on)
      {
        PolishRow& s = g[q];
        const double dy = (s.f != 0) ? s.cr : 0.0;
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (k < s.na)
          {
            double dyb = 0.0;
            if (s.fa[k] != 0)
            {
              double r2 = s.r2a[k];
              if (pass > 0)
                r2 -= s.bba[k] * s.dxa[k];
              if (reg)
                r2 += delta * s.dyba[k];
              dyb = (s.bba[k] * s.ta[k] - r2) / delta;
            }
            if (pass == 0)
            {
              s.dxa[k] = s.ta[k];
              s.dyba[k] = dyb;
            }
            else
            {
              s.dxa[k] += s.ta[k];
              s.dyba[k] += dyb;
            }
          }
        if (pass == 0)
          s.dyr = dy;
        else
          s.dyr += dy;
        Y[s.epos] = s.dyr;
      }
    if (pv)
    {
      const double tpv = TP[v];
      double dyb = 0.0;
      if (fbp != 0)
      {
        double r2 = r2bp;
        if (pass > 0)
          r2 -= bbp * dxp;
        if (reg)
          r2 += delta * dybp;
        dyb = (bbp * tpv - r2) / delta;
      }
      if (pass == 0)
      {
        dxp = tpv;
        dybp = dyb;
      }
      else
      {
        dxp += tpv;
        dybp += dyb;
      }
      X[vt * 8 + vj] = dxp;
    }
    TMX_SYNC();
  }
  // ---- residuals at the polished point (z = clip(A x)): the two compute_residuals(., zmode = 1) hands to the acceptance test
  double m[2] = { 0.0, 0.0 };  // prim_res, dual_res / cinv
#pragma unroll
  for (int q = 0; q < 2; ++q)
    if (g[q].on)
    {
      const PolishRow& s = g[q];
      {
        const double ax = row_ax(s);
        const double z = clampd(ax, w.lor[s.r], w.hir[s.r]);
        const double einv = fast_rcp(w.Er[s.r]);
        m[0] = fmax(m[0], fabs(einv * (ax - z)));
      }
#pragma unroll
      for (int k = 0; k < 2; ++k)
        if (k < s.na)
        {
          const int a = s.ao + k;
          const double eba = w.Eba[a];
          const double ax = s.bba[k] * s.dxa[k];
          const double z = clampd(ax, 0.0, TMX_OSQP_INFTY * eba);
          const double einv = fast_rcp(eba);
          m[0] = fmax(m[0], fabs(einv * (ax - z)));
          const double aty = s.sa[k] * s.dyr + s.bba[k] * s.dyba[k];
          const double res = s.qa[k] + aty;
          const double dinv = fast_rcp(w.Da[a]);
          m[1] = fmax(m[1], fabs(dinv * res));
        }
    }
  if (pv)
  {
    const double ax = bbp * dxp;
    const double z = clampd(ax, lbp, ubp);
    const double einv = fast_rcp(w.Ebp[v]);
    m[0] = fmax(m[0], fabs(einv * (ax - z)));
    const double px = p_times_x();
    const double aty = aty_rows() + bbp * dybp;
    const double res = (qp + px) + aty;
    const double dinv = fast_rcp(w.Dp[v]);
    m[1] = fmax(m[1], fabs(dinv * res));
  }
  {
    const bool issum[2] = { false, false };
    block_reduce<2>(m, issum, w.red, tid, NT);
  }
  const double pprim = m[0], pdual = w.cinv * m[1];
  TMX_POLISH_TICK(7);
  const bool ok = (pprim < info.prim_res && pdual < info.dual_res) || (pprim < info.prim_res && info.dual_res < 1e-10) ||
                  (pdual < info.dual_res && info.prim_res < 1e-10);
  if (ok)
  {
    info.polish_status = 1;
    info.prim_res = pprim;
    info.dual_res = pdual;
    if (pv)
    {
      w.xp[v] = dxp;
      w.ybp[v] = dybp;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (g[q].on)
      {
        const PolishRow& s = g[q];
        w.yr[s.r] = s.dyr;
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (k < s.na)
          {
            w.xa[s.ao + k] = s.dxa[k];
            w.yba[s.ao + k] = s.dyba[k];
          }
      }
  }
  else
    info.polish_status = -1;
  for (int r = tid; r < R; r += NT)
    w.flg_r[r] = Fr[r];
  if (pv)
    w.flg_bp[v] = fbp;
  for (int a = tid; a < NA; a += NT)
    w.flg_ba[a] = Fba[a];
  TMX_SYNC();
}
#endif
