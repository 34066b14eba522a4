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
//  * the cached weights are admm_cache_weights' expressions; the assembly of the diagonal blocks and the separator inverse are the
//    generic functions, called
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
  // 4. its dense inverse: lane = row, wave = column quarter (gj_rows; scratch: the separator exchange vectors)
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
