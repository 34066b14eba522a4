// ADMM factorisation of the dense fast path (kkt_factor(mode 0) + dpart_factor + admm_cache_weights of tmx_qp.h / tmx_part.h) with the
// interior inverses inside one wave.
//
// The generic dpart_factor puts matrix m of the P interior sub-matrices on threads m Gn .. m Gn + Gn - 1: matrices straddle waves, so
// every one of the Gn elimination steps of gj_rows ends in a WORKGROUP barrier, and the owner of row k + 1 forms the reciprocal of the
// next pivot (five dependent operations) behind its row update while three waves wait.  Here wave v holds the matrices
// v mpw .. v mpw + mpw - 1 (mpw = ceil(P / waves): two on each of the four waves for the 7 x 30 problem, 42 lanes), the pivot row
// travels through the same double-buffered LDS vector behind TMX_WAVE_SYNC - no s_barrier in the step loop - and the entry of the
// next pivot and its reciprocal are formed in front of the other FMAs of the row, so the reciprocal's chain runs under them.
// A wave builds the rows of its own matrices (no barrier between build and elimination); the Schur complement is dpart_factor's with
// address_space(3) pointers; the cached weights of the loop are formed in front of the build instead of behind a barrier of their own.
//
// What keeps the bits (tests/test_fast_factor.py compares with the generic code through DevProblem::dbg_flags bit 5):
//  * every entry of G sees gj_rows' operations on gj_rows' operands: fma(nmp, M[k][c], M[i][c]) with nmp = i == k ? piv - 1 : -m_ik piv,
//    m_ik from row k by the sign rule, the pivot column overwritten by piv / nmp, piv = fast_rcp of the updated M[k+1][k+1]; only the
//    thread that holds a row and the kind of barrier differ
//  * the cached weights are admm_cache_weights' expressions; the assembly of the diagonal blocks is the generic function, called
//  * the separator inverse pays its workgroup barrier once per three elimination steps (gj_sep_rows below; bit 6 of dbg_flags keeps
//    gj_rows, tests/test_factor_lookahead.py compares the three)
#pragma once
#include "tmx_qp.h"

// DevProblem::factor_fast beyond setup_fast: the dense nested dissection takes the problem, the matrices of a wave fit its 64 lanes and
// a row fits the widest register row of the elimination
TMX_HOSTDEVFN bool factor_fast_fits(int D, int T)
{
  if (!dpart_fits(D, T))
    return false;
  DPart p;
  dpart_make(T, p);
  const int nw = TMX_QP_NT >> 6, Gn = p.Lmax * D, mpw = (p.P + nw - 1) / nw;
  return mpw * Gn <= 64 && dpart_gstride(Gn) <= 34;
}

#if TMX_IS_DEVICE
#if defined(TMX_PROFILE) && defined(TMX_FINE)
// (-DTMX_PROFILE -DTMX_FINE=3: the cached weights in slot 6 - the build of G is part of slot 14 here - and the Schur build in slot 3)
#define TMX_FACTOR_TICK(slot)                                                                                         \
  do                                                                                                                  \
  {                                                                                                                   \
    if (TMX_FINE == 3)                                                                                                \
      TMX_TICK(slot);                                                                                                 \
  } while (0)
#else
#define TMX_FACTOR_TICK(slot) ((void)0)
#endif

// The P interior sub-matrices (Gn rows of stride Gs each, zero padded) built from the diagonal blocks in S and the couplings in po, and
// their Gauss-Jordan inversion in G, every matrix inside one wave: lane sub Gn + i of wave v builds row i of matrix v mpw + sub
// (dpart_factor, step 1: zero fill, the D entries of the diagonal block, the at most two coupling entries), reads its own row back into
// registers - no barrier between the two - and keeps it there.  buf: gj_rows' exchange vector, 2 P (Gs + 2) doubles.
// NK > 0: the number of steps (= Gn) as a compile-time constant - the loop unrolls, the pivot positions are literals and the entry of
// the next pivot with its reciprocal comes first in every step.  The caller's workgroup barriers stand before and behind.
template <int W, int NK>
TMX_DEVFN void gj_wave_rows(tmx_lds_d* G, tmx_lds_d* buf, const tmx_lds_d* S, const tmx_lds_d* po, int DS, int DDS, int Gn, int Gs, int P, int T, int D, int tid)
{
  constexpr int NW = TMX_QP_NT >> 6;
  const int lane = tid & 63, wv = tid >> 6;
  const int mpw = (P + NW - 1) / NW;
  if (!TMX_UNI_B(wv * mpw < P))  // (a wave without a matrix: nothing to exchange, no workgroup barrier inside)
    return;
  const int sub = tmx_fdiv(lane, 1.0f / (float)Gn), mm = wv * mpw + sub;
  const bool own = sub < mpw && mm < P;
  const int n = own ? dpart_len(T, P, mm) * D : 0;
  const int i = lane - sub * Gn;
  if (own)
  {
    tmx_lds_d* Gr = G + (mm * Gn + i) * Gs;
    for (int c = 0; c < Gs; ++c)
      Gr[c] = 0.0;
    if (i < n)
    {
      const int tb = tmx_fdiv(i, 1.0f / (float)D), j0 = i - tb * D, t = dpart_first(T, P, mm) + tb;
      const tmx_lds_d* Sr = S + t * DDS + j0 * DS;
      for (int j = 0; j < D; ++j)
        Gr[tb * D + j] = Sr[j];
      if (i + D < n)
        Gr[i + D] = po[t * D + j0];        // block column tb + 1, entry (j0, j0)
      if (tb > 0)
        Gr[i - D] = po[(t - 1) * D + j0];  // block column tb - 1
    }
  }
  const bool active = i < n;
  const int m = active ? mm : 0;
  const int bs = Gs + 2;  // row buffer + [pivot reciprocal, pad]
  tmx_lds_d* Mr = G + (m * Gn + (active ? i : 0)) * Gs;
  double val[W];  // (slots >= Gs hold what follows the row: never stored)
#pragma unroll
  for (int c = 0; c < W; c += 2)
  {
    const tmx_d2 t = *(const tmx_lds_d2*)(Mr + c);
    val[c] = active ? t.x : 0.0;
    val[c + 1] = active ? t.y : 0.0;
  }
  if (active && i == 0)
  {
    tmx_lds_d* rb = buf + m * bs;
#pragma unroll
    for (int c = 0; c < W; c += 2)
      if (c < Gs)
        *(tmx_lds_d2*)(rb + c) = tmx_d2{ val[c], val[c + 1] };
    rb[Gs] = fast_rcp(val[0]);
  }
  TMX_WAVE_SYNC();
  constexpr int unroll_steps = NK ? NK : 1;
#pragma unroll unroll_steps
  for (int k = 0; k < (NK ? NK : Gn); ++k)
  {
    const int par = k & 1;
    if (active && k < n)
    {
      const tmx_lds_d* rk = buf + (par * P + m) * bs;
      const double piv = rk[Gs];
      const double rki = rk[i];
      tmx_d2 mk[W / 2];
#pragma unroll
      for (int c = 0; c < W / 2; ++c)
        mk[c] = *((const tmx_lds_d2*)rk + c);
      const double mik = (i < k) ? -rki : rki;  // column k from row k by (anti)symmetry
      const bool prow = i == k;
      // (both arms formed by every lane and selected: as a branch the arms stood between the loads of the pivot row and their issue)
      double nmp_row = piv - 1.0, nmp_else = -mik * piv;
      pin(nmp_row, nmp_else);
      const double nmp = prow ? nmp_row : nmp_else;
      const double pcv = prow ? piv : nmp;  // value of the entry in the pivot column
      double rc = 0.0;
      if (NK)
      {
        // the updated M[i][k+1] (the same FMA as in the loop below) and its reciprocal first: the next pivot's, on the owner of row k + 1
        double mn = mk[0].x, vn = val[0];
#pragma unroll
        for (int c = 1; c < W; ++c)
        {
          mn = (c == k + 1) ? ((c & 1) ? mk[c >> 1].y : mk[c >> 1].x) : mn;
          vn = (c == k + 1) ? val[c] : vn;
        }
        rc = fast_rcp(__builtin_fma(nmp, mn, vn));
        pin(rc);  // (formed by every lane, here: left alone the compiler sinks the chain behind the row stores of the owner)
      }
#pragma unroll
      for (int c = 0; c < W / 2; ++c)
      {
        val[2 * c] = __builtin_fma(nmp, mk[c].x, val[2 * c]);
        val[2 * c + 1] = __builtin_fma(nmp, mk[c].y, val[2 * c + 1]);
      }
#pragma unroll
      for (int c = 0; c < W; ++c)
        val[c] = (c == k) ? pcv : val[c];
      if (i == k + 1)
      {
        tmx_lds_d* rb = buf + ((par ^ 1) * P + m) * bs;
        if (!NK)
        {
          double pvn = val[0];
#pragma unroll
          for (int c = 1; c < W; ++c)
            pvn = (c == k + 1) ? val[c] : pvn;
          rc = fast_rcp(pvn);
        }
#pragma unroll
        for (int c = 0; c < W; c += 2)
          if (c < Gs)
            *(tmx_lds_d2*)(rb + c) = tmx_d2{ val[c], val[c + 1] };
        rb[Gs] = rc;
      }
    }
    TMX_WAVE_SYNC();
  }
  if (active)
  {
#pragma unroll
    for (int c = 0; c < W; ++c)
      if (c < Gs && c < n)
        Mr[c] = val[c];
  }
}

// The separator inverse (gj_rows<W, true> on one matrix: lane = row, wave = column quarter of the row stride Zst) with ONE workgroup
// barrier and one LDS round trip per group of LA elimination steps.  The owners of rows k0 .. k0 + LA - 1 publish them as they stand
// before step k0, with the reciprocal of the pivot of step k0.  Every lane then carries PRIVATE copies of the published rows through
// the group: before it applies step k0 + s to its own row it advances the copies of the rows behind by that step - for row t > s the
// multiplier nm = -r_s[k0 + t] piv_s, fma(nm, r_s[c], r_t[c]) on the entries it needs (its own column segment, entry i, the entries
// k0 + u of the rows still to come), nm itself in the pivot column - and takes piv_t = fast_rcp(r_t[k0 + t]).  These are the IEEE
// operations of the owner of row t on the owner's operands, so a copy holds the bits the owner would have published, and every entry of
// the matrix still sees gj_rows' operations on gj_rows' operands.  The multipliers depend on 2 LA + LA (LA - 1) / 2 scalars only: they
// come first, the row FMAs follow with known multipliers.  The entry of the next group's first pivot and its reciprocal are formed in
// front of the row FMAs by every lane of the wave that holds its column (gj_wave_rows does the same with `rc`).
// buf: 2 LA (Zst + 2) doubles, two parities of LA row buffers of [row, pivot reciprocal, pad] (gj_sep_buf_doubles).
// NS steps of one group, NS <= LA (the last group may be short); kn = k0 + NS < ns: there is a next group to publish for
template <int W, int NS, int LA>
TMX_DEVFN void gj_sep_group(double (&val)[W], const tmx_lds_d* rin, tmx_lds_d* rout, int Zst, int wn, int j0, int i, int k0, bool more)
{
  const int bs = Zst + 2;
  const int kk0 = TMX_UNI_I(k0 - j0);  // position of the group's first pivot column in this wave's segment
  const int kkn = kk0 + NS;       // ... and of the next group's
  const int kcn = TMX_UNI_I(kkn < 0 ? 0 : (kkn >= W ? W - 1 : kkn));
  double piv[NS], ri[NS], rx[NS][NS], nmp[NS], pcv[NS], nm[NS][NS], e[NS];
  tmx_d2 rs[NS][W / 2];
  piv[0] = rin[Zst];
#pragma unroll
  for (int s = 0; s < NS; ++s)
  {
    ri[s] = rin[s * bs + i];
    e[s] = rin[s * bs + k0 + NS];  // (column k0 + NS <= ns < Zst)
#pragma unroll
    for (int u = s + (s ? 0 : 1); u < NS; ++u)
      rx[s][u] = rin[s * bs + k0 + u];
  }
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int c = 0; c < W / 2; ++c)
      rs[s][c] = *((const tmx_lds_d2*)(rin + s * bs + j0) + c);
  // the multipliers of the group: step k0 + s on the own row (nmp, pcv) and on the copies of the rows behind (nm[t][s])
#pragma unroll
  for (int s = 0; s < NS; ++s)
  {
    const int k = k0 + s;
    if (s > 0)
      piv[s] = fast_rcp(rx[s][s]);
    const double mik = (i < k) ? -ri[s] : ri[s];  // column k from row k by (anti)symmetry
    const bool prow = i == k;
    double nmp_row = piv[s] - 1.0, nmp_else = -mik * piv[s];
    nmp[s] = prow ? nmp_row : nmp_else;
    pcv[s] = prow ? piv[s] : nmp[s];  // value of the entry in the pivot column
#pragma unroll
    for (int t = s + 1; t < NS; ++t)
    {
      nm[t][s] = -rx[s][t] * piv[s];  // (row t > k: its column k is r_s[k0 + t] itself)
#pragma unroll
      for (int u = t; u < NS; ++u)
        rx[t][u] = __builtin_fma(nm[t][s], rx[s][u], rx[t][u]);
      const double adv = __builtin_fma(nm[t][s], ri[s], ri[t]);
      ri[t] = prow ? nm[t][s] : adv;  // (entry i is the pivot column on the lane of row k)
    }
  }
  // the next group's first pivot M[kn][kn] after the NS steps and its reciprocal, in front of the row FMAs
  const bool pw = more && kkn >= 0 && kkn < wn;  // (wave-uniform)
  double rcn = 0.0;
  if (pw)
  {
    double vn = val[kcn];
#pragma unroll
    for (int s = 0; s < NS; ++s)
    {
#pragma unroll
      for (int t = s + 1; t < NS; ++t)
        e[t] = __builtin_fma(nm[t][s], e[s], e[t]);
      vn = __builtin_fma(nmp[s], e[s], vn);
    }
    rcn = fast_rcp(vn);
    pin(rcn);
  }
  // the rows: step k0 + s on the copies of the rows behind, then on the own row
#pragma unroll
  for (int s = 0; s < NS; ++s)
  {
    const int kk = kk0 + s;
    // (the index is clamped before use and handed back as a scalar: gj_rows, round 6)
    const int kc = TMX_UNI_I(kk < 0 ? 0 : (kk >= W ? W - 1 : kk));
    const bool kin = kk >= 0 && kk < wn;
#pragma unroll
    for (int t = s + 1; t < NS; ++t)
    {
      double rt[W];
#pragma unroll
      for (int c = 0; c < W / 2; ++c)
      {
        rt[2 * c] = __builtin_fma(nm[t][s], rs[s][c].x, rs[t][c].x);
        rt[2 * c + 1] = __builtin_fma(nm[t][s], rs[s][c].y, rs[t][c].y);
      }
      const double keep = rt[kc];
      rt[kc] = kin ? nm[t][s] : keep;
#pragma unroll
      for (int c = 0; c < W / 2; ++c)
        rs[t][c] = tmx_d2{ rt[2 * c], rt[2 * c + 1] };
    }
#pragma unroll
    for (int c = 0; c < W / 2; ++c)
    {
      val[2 * c] = __builtin_fma(nmp[s], rs[s][c].x, val[2 * c]);
      val[2 * c + 1] = __builtin_fma(nmp[s], rs[s][c].y, val[2 * c + 1]);
    }
    const double keep = val[kc];
    val[kc] = kin ? pcv[s] : keep;
  }
  // the owners of the next group's rows publish them into the other parity
  const int kn = k0 + NS;
  if (i >= kn && i < kn + LA)
  {
    tmx_lds_d* rb = rout + (i - kn) * bs;
#pragma unroll
    for (int c = 0; c < W; c += 2)
      if (c < wn)
        *(tmx_lds_d2*)(rb + j0 + c) = tmx_d2{ val[c], val[c + 1] };
    if (pw && i == kn)
      rb[Zst] = rcn;
  }
}
TMX_HOSTDEVFN int gj_sep_buf_doubles(int Zst, int LA) { return 2 * LA * (Zst + 2); }
template <int W, int LA>
TMX_DEVFN void gj_sep_rows(tmx_lds_d* M, tmx_lds_d* buf, int Zst, int ns, int tid)
{
  static_assert(LA >= 1 && LA <= 3, "group size");
  const int wn = Zst >> 2, j0 = TMX_UNI_I(((tid >> 6) & 3) * wn);
  const bool active = (tid & 63) < ns && tid < 256;
  const int i = active ? (tid & 63) : 0;
  const int bs = Zst + 2;
  tmx_lds_d* Mr = M + i * Zst + j0;
  // (all W register slots are loaded and updated, slots >= wn hold what follows the segment and are never stored: gj_rows)
  double val[W];
#pragma unroll
  for (int c = 0; c < W; c += 2)
  {
    const tmx_d2 t = *(const tmx_lds_d2*)(Mr + c);
    val[c] = active ? t.x : 0.0;
    val[c + 1] = active ? t.y : 0.0;
  }
  if (active && i < LA)
  {
    tmx_lds_d* rb = buf + i * bs;
#pragma unroll
    for (int c = 0; c < W; c += 2)
      if (c < wn)
        *(tmx_lds_d2*)(rb + j0 + c) = tmx_d2{ val[c], val[c + 1] };
    if (i == 0 && j0 == 0)
      rb[Zst] = fast_rcp(val[0]);
  }
  TMX_SYNC();
  int k0 = 0, par = 0;
  for (; k0 + LA <= ns; k0 += LA, par ^= 1)
  {
    if (active)
      gj_sep_group<W, LA, LA>(val, buf + par * LA * bs, buf + (par ^ 1) * LA * bs, Zst, wn, j0, i, k0, k0 + LA < ns);
    TMX_SYNC();
  }
  if constexpr (LA > 1)
  {
    const int rem = ns - k0;  // (wave-uniform: the barriers stand in uniform control flow)
    if (rem == 1)
    {
      if (active)
        gj_sep_group<W, 1, LA>(val, buf + par * LA * bs, buf + (par ^ 1) * LA * bs, Zst, wn, j0, i, k0, false);
    }
    else if (LA > 2 && rem == 2)
    {
      if (active)
        gj_sep_group<W, (LA > 2 ? 2 : 1), LA>(val, buf + par * LA * bs, buf + (par ^ 1) * LA * bs, Zst, wn, j0, i, k0, false);
    }
  }
  if (active)
  {
#pragma unroll
    for (int c = 0; c < W; ++c)
      if (c < wn && j0 + c < ns)
        Mr[c] = val[c];
  }
  TMX_SYNC();
}

// Preconditions: the fast-path predicate of qp_solve_block and DevProblem::factor_fast; w.rho / w.sigma set.  In: the scaled problem.
// Out: G, Zs, fac, dinv (and hr, Sinv) as kkt_factor(mode 0) + kkt_invert(partitioned) + admm_cache_weights leave them.
TMX_DEVFN void factor_fast(const QpWs& w, const DevProblem* P, double delta, int tid, [[maybe_unused]] long long* pc, [[maybe_unused]] long long& tlast)
{
  constexpr int NT = TMX_QP_NT;
  kkt_factor(w, P, 0, w.sigma, delta, tid, NT);
  TMX_TICK(13);
  const int D = __builtin_amdgcn_readfirstlane(w.D), T = __builtin_amdgcn_readfirstlane(w.T), Gn = __builtin_amdgcn_readfirstlane(w.Gn),
            Gs = __builtin_amdgcn_readfirstlane(w.Gs), Zst = __builtin_amdgcn_readfirstlane(w.Zst);
  const int DS = w.DS, DDS = w.DDS;
#define TMX_LDS_PTR(p) ((tmx_lds_d*)(size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(p)))
  tmx_lds_d* const S = TMX_LDS_PTR(w.Sinv);
  tmx_lds_d* const G = TMX_LDS_PTR(w.G);
  tmx_lds_d* const Zs = TMX_LDS_PTR(w.Zs);
  tmx_lds_d* const po = TMX_LDS_PTR(w.po);
  tmx_lds_d* const sx = TMX_LDS_PTR(w.sx);
#undef TMX_LDS_PTR
  DPart p;
  dpart_make(T, p);
  const int ns = (p.P - 1) * D;
  const float rD = 1.0f / (float)D;
  // the cached weights of the ADMM loop (admm_cache_weights without its barrier: nothing reads fac / dinv before the loop, and the
  // barriers below stand in between)
  TMX_ROWS(w, r)
  {
    double f = 0.0;
    if (w.act[r])
    {
      const double rr = rho_of_type(w.typ_r[r], w.rho);
      double kappa = 0.0;
      for (int k = 0; k < w.naux[r]; ++k)
      {
        const int a = w.aoff[r] + k;
        const double di = 1.0 / (w.sigma + rho_of_type(w.typ_ba[a], w.rho) * w.bba[a] * w.bba[a]);
        w.dinv[a] = di;
        kappa += w.sa[a] * w.sa[a] * di;
      }
      f = rr / (1.0 + rr * kappa);
    }
    w.fac[r] = f;
  }
  TMX_FACTOR_TICK(6);
  // 1. + 2. the interior sub-matrices and their explicit inverses, every matrix inside one wave (scratch: the Zs region, not yet built)
  if (Gs <= 16)
    gj_wave_rows<16, 0>(G, Zs, S, po, DS, DDS, Gn, Gs, p.P, T, D, tid);
  else if (Gs <= 24 && Gn == 21)  // (three blocks of 7: BASELINE configuration 1)
    gj_wave_rows<24, 21>(G, Zs, S, po, DS, DDS, Gn, Gs, p.P, T, D, tid);
  else if (Gs <= 24)
    gj_wave_rows<24, 0>(G, Zs, S, po, DS, DDS, Gn, Gs, p.P, T, D, tid);
  else
    gj_wave_rows<34, 0>(G, Zs, S, po, DS, DDS, Gn, Gs, p.P, T, D, tid);
  TMX_SYNC();
  TMX_TICK(14);
  // 3. Schur complement on the separators: four threads per matrix row (dpart_factor, step 3)
  {
    const int zq = Zst >> 2;  // (Zst is a multiple of 8)
    for (int rq = tid; rq < 4 * ns; rq += NT)
    {
      const int rI = rq >> 2, q = rq & 3;
      const int kr = tmx_fdiv(rI, rD), i = rI - kr * D, kc = kr - 1 + q;
      tmx_lds_d* Zr = Zs + rI * Zst;
      const int c_lo = (kr - 1) * D, c_hi = (kr + 2) * D < ns ? (kr + 2) * D : ns;  // columns [c_lo, c_hi) belong to the three blocks
      for (int c = q * zq; c < (q + 1) * zq; ++c)
        if (c < c_lo || c >= c_hi)
          Zr[c] = 0.0;
      if (q < 3 && kc >= 0 && kc < p.P - 1)
      {
        const int sb = dpart_sep(T, p.P, kr);
        const tmx_lds_d* GL = G + kr * Gn * Gs;        // interior left of separator kr
        const tmx_lds_d* GR = G + (kr + 1) * Gn * Gs;  // interior right of it
        const int nL = dpart_len(T, p.P, kr) * D, nR = dpart_len(T, p.P, kr + 1) * D;
        const double cl_i = po[(sb - 1) * D + i], cr_i = po[sb * D + i];
        const int sc = dpart_sep(T, p.P, kc);
        for (int j = 0; j < D; ++j)
        {
          double val;
          if (q == 1)
            val = S[sb * DDS + i * DS + j] - cl_i * GL[(nL - D + i) * Gs + (nL - D + j)] * po[(sb - 1) * D + j] - cr_i * GR[i * Gs + j] * po[sb * D + j];
          else if (q == 2)
            val = -cr_i * GR[i * Gs + (nR - D + j)] * po[(sc - 1) * D + j];
          else
            val = -cl_i * GL[(nL - D + i) * Gs + j] * po[sc * D + j];
          Zr[kc * D + j] = val;
        }
      }
    }
  }
  TMX_SYNC();
  TMX_FACTOR_TICK(3);
  // 4. its dense inverse: lane = row, wave = column quarter, three elimination steps per barrier (gj_sep_rows; scratch: the separator
  //    exchange vectors w.sx, 6 x 64 doubles: room for three steps up to Zst = 56, the 7 x 30 problem's; a wider system keeps gj_rows).
  //    DevProblem::dbg_flags bit 6 keeps gj_rows, one step per barrier, on every problem: same bits
  constexpr int SEP_LA = 3;
  if (TMX_UNI_B(!(P->dbg_flags & 64) && gj_sep_buf_doubles(Zst, SEP_LA) <= 6 * 64))
  {
    if (Zst <= 32)
      gj_sep_rows<8, SEP_LA>(Zs, sx, Zst, ns, tid);
    else
      gj_sep_rows<16, SEP_LA>(Zs, sx, Zst, ns, tid);
  }
  else
  {
    const int i = tid & 63, seg = (tid >> 6) & 3;
    const bool active = i < ns && tid < 256;
    if (Zst <= 32)
      gj_rows<8, true>((double*)Zs, 0, Zst, 1, ns, active, 0, active ? i : 0, seg * (Zst >> 2), Zst >> 2, ns, w.sx);
    else
      gj_rows<16, true>((double*)Zs, 0, Zst, 1, ns, active, 0, active ? i : 0, seg * (Zst >> 2), Zst >> 2, ns, w.sx);
  }
  TMX_TICK(15);
}
#endif
