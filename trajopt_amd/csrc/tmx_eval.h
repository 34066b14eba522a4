// The evaluation side of the specialised SQP step (tmx_step.h) on the problems DevProblem::eval_fast admits: work the generic code
// repeats although its inputs are the same.
//
// p_hash_column / tmx_build_p_hash_table: the two hashes of P (hashP and what the reference's memcmp compares, wsP) depend on
// upload-time constants only (p_colptr, the zero pattern of pd / po, nnzP) and on the number of QP variables n, yet qp_structure_fast
// summed their n + 1 + nnzP terms in every convexification.  The upload builds the pair for every n = NX .. n_max with the kernel's own
// per-column routine (one definition for host and device) and the structure pass adds the table entry instead.
//
// step_eval_fast: the exact evaluation at xnew (evaluate_terms) and the model values at the QP solution (sqp_model_values) of one
// trust-region evaluation as one function.
//  * sin / cos of every joint value once: thread (t, k) writes them to LDS, and one thread per waypoint walks the chain once and
//    stores the link frame of every joint.  The generic code runs a chain - D times tmx_sincos and 2 D frame products - per collision
//    slot and per cart-pose instance; here the slots read the frame of their link.  Same bits: the table holds tmx_sincos of the same
//    operand, the walk is fk_link_visit's left-to-right product, and the frame of link k is its value after joint k.
//  * the velocity sum once.  xnew[v] = xq[v] is an exact copy, and on these problems (trajopt_sco flavour, velocity kinds 0 and 1) the
//    terms (d * d) * coeff and their serial sum are the same expressions on the same operands in the same order at xnew and at xq:
//    the second sum has the first one's bits.  It runs on a thread of another wave than the one walking the chains.
//  * the per-slot model values (coef . xq, loads that do not depend on the kinematics) beside the trig table, and the per-owner
//    sums of the exact and of the model values in one phase, on threads of different waves.
// Four barriers, the final one included, where the two generic functions have seven.
//
// convexify_fast: the collision and cart-pose rows of a convexification from the same tables (described at the function).
//
// dbg_flags bit 4 keeps the generic code of all three on a qualifying problem (tests/test_fast_eval.py compares the two in one library).
#pragma once
#include "tmx_solve.h"

// contribution of column c <= n of the static upper-triangular P (the pattern of qp_structure: (c - D, c) if po != 0, (c, c) if
// pd != 0, empty penalty columns) to hashP / wsP of a QP with n variables
TMX_HOSTDEVFN void p_hash_column(const int* p_colptr, const double* pd, const double* po, int D, int NX, int nnzP, int n, int c,
                                 unsigned long long& hP, unsigned long long& wsP)
{
  const int pp_bytes = n + 1, pp_full = pp_bytes / 8, pp_rem = pp_bytes % 8;
  const int pi_full = nnzP / 8, pi_rem = nnzP % 8;
  auto p_term = [&](long long row, int run) {
    hP += tmx_hash_term(row, (uint64_t)run, 2);
    if (run < pi_full)
      wsP += tmx_hash_term(row, (uint64_t)run, 12);
    else if (run == pi_full && pi_rem > 0)
      wsP += tmx_hash_term((long long)((unsigned long long)row & ((1ULL << (8 * pi_rem)) - 1ULL)), (uint64_t)run, 12);
  };
  int run = (c <= NX) ? p_colptr[c] : nnzP;
  const long long val = run;
  hP += tmx_hash_term(val, (uint64_t)c, 1);
  if (c < pp_full)
    wsP += tmx_hash_term(val, (uint64_t)c, 11);
  else if (c == pp_full && pp_rem > 0)
    wsP += tmx_hash_term((long long)((unsigned long long)val & ((1ULL << (8 * pp_rem)) - 1ULL)), (uint64_t)c, 11);
  if (c < NX)
  {
    if (c >= D && po[c - D] != 0.0)
    {
      p_term(c - D, run);
      ++run;
    }
    if (pd[c] != 0.0)
      p_term(c, run);
  }
}

// DevProblem::p_hash: (hashP, wsP) of every n = NX .. n_max, two u64 per entry.  Host side of the upload.
static inline void tmx_build_p_hash_table(const int* p_colptr, const double* pd, const double* po, int D, int NX, int n_max, int nnzP,
                                          unsigned long long* tab)
{
  for (int n = NX; n <= n_max; ++n)
  {
    unsigned long long hP = 0ULL, wsP = 0ULL;
    for (int c = 0; c <= n; ++c)
      p_hash_column(p_colptr, pd, po, D, NX, nnzP, n, c, hP, wsP);
    tab[2 * (n - NX)] = hP;
    tab[2 * (n - NX) + 1] = wsP;
  }
}

// LDS doubles of step_eval_fast: the model values (where sqp_update_fast expects them), the per-slot values and keys of the exact and
// of the model side, velocity terms and sums, the trig table (2 NX) and the link frames (12 NX)
TMX_HOSTDEVFN size_t tmx_step_eval_doubles(int R, int NX, int n_vel, int n_costs, int n_cnts)
{
  return (size_t)n_costs + (size_t)n_cnts + 2 * ((size_t)R + (size_t)(R + 1) / 2) + (size_t)n_vel * NX + (size_t)n_vel + 14 * (size_t)NX;
}
// the slot kinds step_eval_fast evaluates
TMX_HOSTDEVFN bool tmx_step_eval_kind(int kind)
{
  return kind == SLOT_FIXED || kind == SLOT_CARTPOSE || kind == SLOT_JOINTPOS || kind == SLOT_JOINTPOS_INEQ || kind == SLOT_COLLISION;
}

#if TMX_IS_DEVICE
#define TMX_EVAL_LDS_PTR(p) ((tmx_lds_d*)(size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(p)))
// Results: Bt->new_cost_vals / new_cnt_viols of problem b as evaluate_terms<false> leaves them at xnew; with a solved QP also
// smem[0 .. n_costs) model costs, smem[n_costs .. n_costs + n_cnts) model violations as sqp_model_values<false> leaves them.  Ends
// with a barrier.  Preconditions (DevProblem::eval_fast and the caller): TMX_QP_NT threads, xnew = xq[0 .. NX) already copied.
TMX_DEVFN void step_eval_fast(const DevProblem* P, const DevBatch* Bt, int b, double* smem, int tid)
{
  constexpr int NT = TMX_QP_NT;
  const int D = P->D, NX = P->NX, R = P->R, T = P->T, nc = P->n_costs, nv = P->n_cnts, nvel = P->n_vel;
  const double* xv = Bt->xnew + (size_t)b * NX;
  const double* xq = Bt->xq + (size_t)b * P->n_max;
  double* cost_out = Bt->new_cost_vals + (size_t)b * nc;
  double* viol_out = Bt->new_cnt_viols + (size_t)b * nv;
  const bool solved = TMX_UNI_B(Bt->cvx[b] == TMX_CVX_SOLVED && Bt->phase[b] != PHASE_DONE);
  double* model_cost = smem;          // n_costs
  double* model_viol = smem + nc;     // n_cnts
  double* xval = model_viol + nv;     // R: exact per-slot values
  int* xkeys = reinterpret_cast<int*>(xval + R);
  double* mval = xval + R + (R + 1) / 2;  // R: model per-slot values
  int* mkeys = reinterpret_cast<int*>(mval + R);
  double* vterm = mval + R + (R + 1) / 2;  // n_vel x NX
  double* vsum = vterm + (size_t)nvel * NX;
  tmx_lds_d* const SN = TMX_EVAL_LDS_PTR(vsum + nvel);  // NX: sin of every joint value (revolute joints)
  tmx_lds_d* const CS = SN + NX;                   // NX: cos
  tmx_lds_d* const FR = CS + NX;                   // NX x 12: frame of link k at waypoint t, at (t D + k) 12
  // ---- phase 1: everything that needs no frame
  for (int v = tid; v < NX; v += NT)
    if (P->jtype[v % D] == 0)
    {
      double s, c;
      tmx_sincos(xv[v], &s, &c);
      SN[v] = s;
      CS[v] = c;
    }
  {
    const int* act = Bt->active + (size_t)b * R;
    const double* coef = Bt->coef + (size_t)b * R * D;
    const double* rhs = Bt->rhs + (size_t)b * R;
    QpWs wl;  // only for the layout of the per-problem scratch (aux_ref written by the QP kernel)
    qp_ws_carve(wl, smem, smem, Bt->qp_scratch + (size_t)b * Bt->qp_scratch_stride, D, T, R, P->NA, P->n_link, P->coef_far);
    const int* aux_ref = wl.aux_ref;
    for (int r = tid; r < R; r += NT)
    {
      const int kind = P->slot_kind[r];
      const int t = P->slot_t[r];
      // exact values of the joint-space slots (the expressions of evaluate_terms); collision and cart-pose slots follow in phase 3
      if (kind == SLOT_JOINTPOS_INEQ)
      {
        const double pos = xv[t * D + P->slot_sub[r]] - P->slot_aux1[r];
        const double e = (P->slot_sub2[r] == 0) ? (pos - P->slot_aux2[r]) * P->slot_scale[r] : ((pos * -1) + P->slot_aux2[r]) * P->slot_scale[r];
        xval[r] = (e > 0) ? e : 0.0;
      }
      else if (kind == SLOT_JOINTPOS)
      {
        const double d = xv[t * D + P->slot_sub[r]] - P->slot_aux1[r];
        xval[r] = fabs((d * d) * P->slot_scale[r]);
      }
      else if (kind == SLOT_FIXED)
        xval[r] = 0.0;
      xkeys[r] = (kind == SLOT_FIXED) ? -1 : (P->slot_iscnt[r] ? nc + P->slot_owner[r] : P->slot_owner[r]);
      if (solved)
      {
        // model value of the row at the QP solution (the expressions of sqp_model_values)
        double vr = 0.0;
        int key = -1;
        if (kind != SLOT_FIXED && act[r])
        {
          if (P->slot_iscnt[r])
          {
            double aff = 0.0;
            for (int j = 0; j < D; ++j)
              aff += coef[r * D + j] * xq[t * D + j];
            aff -= rhs[r];
            vr = P->slot_eq[r] ? fabs(aff) : ((aff > 0) ? aff : 0.0);
            key = nc + P->slot_owner[r];
          }
          else
          {
            double sacc = 0.0;
            for (int k = 0; k < P->slot_naux[r]; ++k)
              sacc += P->slot_objc[r] * xq[aux_ref[r] + k];
            vr = sacc;
            key = P->slot_owner[r];
          }
        }
        mval[r] = vr;
        mkeys[r] = key;
      }
    }
  }
  for (int v = 0; v < nvel; ++v)
  {
    const int pk = P->vel_kind[v];  // 0: difference of consecutive steps (JointVelEqCost), 1: position (JointPosEqCost)
    const int first = P->vel_first[v], len = P->vel_last[v] - first + vel_len_adj<false>(pk);
    for (int e = tid; e < D * len; e += NT)
    {
      const int j = e / len, i = first + e % len;
      const double dv = pk ? xv[i * D + j] : (xv[(i + 1) * D + j] - xv[i * D + j]);
      const double d = dv - P->vel_targets[v * TMX_MAX_DOF + j];
      vterm[(size_t)v * NX + e] = (d * d) * P->vel_coeffs[v * TMX_MAX_DOF + j];
    }
  }
  TMX_SYNC();
  // ---- phase 2: one chain per waypoint (fk_link_visit's product, every link frame kept); the velocity sums on another wave
  for (int t = tid; t < T; t += NT)
  {
    Tf3 F, O, M, U;
    tf_from12(P->base, F);
    for (int k = 0; k < D; ++k)
    {
      tf_from12(P->origin[k], O);
      tf_mul(F, O, U);
      const int type = P->jtype[k];
      double s = 0.0, c = 1.0;
      if (type == 0)
      {
        s = SN[t * D + k];
        c = CS[t * D + k];
      }
      tf_joint_motion_sc(P->axis[k], type, xv[t * D + k], s, c, M);
      tf_mul(U, M, F);
      tmx_lds_d* const o = FR + (size_t)(t * D + k) * 12;
#pragma unroll
      for (int i = 0; i < 9; ++i)
        o[i] = F.R[i];
#pragma unroll
      for (int i = 0; i < 3; ++i)
        o[9 + i] = F.t[i];
    }
  }
  for (int v = (tid + NT - 64) % NT; v < nvel; v += NT)
  {
    const int cnt = D * (P->vel_last[v] - P->vel_first[v] + vel_len_adj<false>(P->vel_kind[v]));
    double sacc = 0;
    for (int e = 0; e < cnt; ++e)
      sacc += vterm[(size_t)v * NX + e];
    vsum[v] = sacc;
  }
  TMX_SYNC();
  // ---- phase 3: collision slots and cart-pose instances from the frames
  auto frame_at = [&](int t, int k, Tf3& L) {
    tmx_lds_d* const o = FR + (size_t)(t * D + k) * 12;
#pragma unroll
    for (int i = 0; i < 9; ++i)
      L.R[i] = o[i];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      L.t[i] = o[9 + i];
  };
  for (int r = tid; r < R; r += NT)
    if (P->slot_kind[r] == SLOT_COLLISION)
    {
      const int s = P->slot_sub[r];
      Tf3 L;
      frame_at(P->slot_t[r], P->ls_link[s], L);
      double n[3], pw[3];
      const double dist = contact_distance_at<false>(P, L, s, P->slot_sub2[r], n, pw);
      const double margin = P->slot_aux1[r];
      double v = 0.0;
      if (!(dist > margin + P->slot_aux2[r]))
      {
        const double pv = margin - dist;
        v = ((pv > 0) ? pv : 0.0) * P->slot_objc[r];
      }
      xval[r] = v;
    }
  for (int c = tid; c < P->n_cp; c += NT)
  {
    Tf3 tgt, tinv, L, Tl, src;
    tf_from12(P->cp_target + 12 * c, tgt);
    tf_inv(tgt, tinv);
    frame_at(P->cp_t[c], D - 1, L);
    tf_from12(P->tool, Tl);
    tf_mul(L, Tl, src);
    double err[6], ax[3], ang;
    transform_error(tinv, src, err, ax, ang);
    const int s0 = P->cp_slot0[c];
    for (int i = 0; i < P->cp_nrows[c]; ++i)
    {
      const int ix = P->cp_idx[6 * c + i];
      const double e = (ix == 0) ? err[0] : (ix == 1) ? err[1] : (ix == 2) ? err[2] : (ix == 3) ? err[3] : (ix == 4) ? err[4] : err[5];
      const double cc = P->cp_coeff[6 * c + i];
      xval[s0 + i] = P->cp_iscnt[c] ? fabs(e * cc) : fabs(e) * cc;
    }
  }
  TMX_SYNC();
  // ---- phase 4: one thread per owner sums its slots in slot order - the exact values, and on another wave the model values
  for (int k = tid; k < nc + nv; k += NT)
  {
    double acc = 0.0;
    for (int r = P->own_lo[k]; r <= P->own_hi[k]; ++r)
      if (xkeys[r] == k)
        acc += xval[r];
    if (k < nc)
    {
      for (int v = 0; v < nvel; ++v)
        if (P->vel_cost[v] == k)
          acc += vsum[v];
      cost_out[k] = acc;
    }
    else
      viol_out[k - nc] = acc;
  }
  if (solved)
    for (int k = (tid + NT - 64) % NT; k < nc + nv; k += NT)
    {
      double acc = 0.0;
      for (int r = P->own_lo[k]; r <= P->own_hi[k]; ++r)
        if (mkeys[r] == k)
          acc += mval[r];
      if (k < nc)
      {
        for (int v = 0; v < nvel; ++v)
          if (P->vel_cost[v] == k)
            acc += vsum[v];
        model_cost[k] = acc;
      }
      else
        model_viol[k - nc] = acc;
    }
  TMX_SYNC();
}
#endif

// LDS doubles of convexify_fast: the records of convexify_terms (tmx_cvx_scratch_doubles), sin / cos of every joint value and of every
// perturbed one (4 NX), the frame before motion and the link frame of every joint (24 NX)
TMX_HOSTDEVFN size_t tmx_cvx_fast_doubles(int n_cp, int D, int NX) { return tmx_cvx_scratch_doubles(n_cp, D) + 28 * (size_t)NX; }

#if TMX_IS_DEVICE
// convexify_fast: convexify_terms<false> of a trajopt_sco problem whose dynamic rows are collision and cart-pose rows, from the
// tables of step_eval_fast plus two more: sin / cos of the perturbed values q + TMX_EPS_FD and the frames before motion U_k.  The
// generic code runs one chain per finite-difference item and two per collision slot (contact_distance, then the gradient pass), each
// with D tmx_sincos.  Here one thread per waypoint walks the chain once; a collision row reads the frame of its link and, for the
// gradient, the U_k of its joints; a finite-difference item keeps its full left-to-right product (the perturbed joint changes every
// frame behind it) and takes sin / cos from the tables.  Same `active` / `coef` / `rhs` bytes, the zeros of inactive rows included.
TMX_DEVFN void convexify_fast(const DevProblem* P, const double* xv, int* active, double* coef, double* rhs, double* scratch, int tid)
{
  constexpr int NT = TMX_QP_NT;
  const int D = P->D, NX = P->NX, T = P->T, n_cp = P->n_cp;
  double* rec = scratch;                             // [n_cp][D+1][7] : translation, rotation axis, angle
  double* errv = rec + (size_t)n_cp * (D + 1) * 7;   // [n_cp][6]
  double* Jm = errv + (size_t)n_cp * 6;              // [n_cp][6][D]
  tmx_lds_d* const SN = TMX_EVAL_LDS_PTR(scratch + tmx_cvx_scratch_doubles(n_cp, D));  // NX each: sin, cos, and of q + eps
  tmx_lds_d* const CS = SN + NX;
  tmx_lds_d* const SNP = CS + NX;
  tmx_lds_d* const CSP = SNP + NX;
  tmx_lds_d* const FU = CSP + NX;               // NX x 12: frame of joint k before motion at waypoint t, at (t D + k) 12
  tmx_lds_d* const FL = FU + (size_t)NX * 12;   // NX x 12: frame of link k
  auto frame_put = [&](tmx_lds_d* o, const Tf3& F) {
#pragma unroll
    for (int i = 0; i < 9; ++i)
      o[i] = F.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      o[9 + i] = F.t[i];
  };
  auto frame_get = [&](tmx_lds_d* o, Tf3& F) {
#pragma unroll
    for (int i = 0; i < 9; ++i)
      F.R[i] = o[i];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      F.t[i] = o[9 + i];
  };
  // ---- phase 1: the trig tables
  for (int v = tid; v < NX; v += NT)
    if (P->jtype[v % D] == 0)
    {
      double s, c;
      tmx_sincos(xv[v], &s, &c);
      SN[v] = s;
      CS[v] = c;
      if (n_cp > 0)
      {
        tmx_sincos(xv[v] + TMX_EPS_FD, &s, &c);
        SNP[v] = s;
        CSP[v] = c;
      }
    }
  TMX_SYNC();
  // ---- phase 2: one chain per waypoint, both frames of every joint kept; the finite-difference chains of the cart-pose instances
  for (int t = tid; t < T; t += NT)
  {
    Tf3 F, O, M, U;
    tf_from12(P->base, F);
    for (int k = 0; k < D; ++k)
    {
      tf_from12(P->origin[k], O);
      tf_mul(F, O, U);
      frame_put(FU + (size_t)(t * D + k) * 12, U);
      const int type = P->jtype[k];
      double s = 0.0, c = 1.0;
      if (type == 0)
      {
        s = SN[t * D + k];
        c = CS[t * D + k];
      }
      tf_joint_motion_sc(P->axis[k], type, xv[t * D + k], s, c, M);
      tf_mul(U, M, F);
      frame_put(FL + (size_t)(t * D + k) * 12, F);
    }
  }
  // (K1 of convexify_terms: one thread per (instance, perturbed joint | base pose), offset by a wave from the chain walkers)
  for (int item = (tid + NT - 64) % NT; item < n_cp * (D + 1); item += NT)
  {
    const int c = item / (D + 1), k = item % (D + 1);
    const int t = P->cp_t[c];
    const double* q = xv + t * D;
    Tf3 tgt, tinv, src, pp;
    tf_from12(P->cp_target + 12 * c, tgt);
    tf_inv(tgt, tinv);
    {
      // fk_tool_at over q with joint k perturbed (k == D: the unperturbed pose): fk_link_visit's product, sin / cos from the tables
      Tf3 F, O, M, U, Tl;
      tf_from12(P->base, F);
      for (int j = 0; j < D; ++j)
      {
        tf_from12(P->origin[j], O);
        tf_mul(F, O, U);
        const int type = P->jtype[j];
        double s = 0.0, cs = 1.0;
        if (type == 0)
        {
          s = (j == k) ? SNP[t * D + j] : SN[t * D + j];
          cs = (j == k) ? CSP[t * D + j] : CS[t * D + j];
        }
        tf_joint_motion_sc(P->axis[j], type, (j == k) ? q[j] + TMX_EPS_FD : q[j], s, cs, M);
        tf_mul(U, M, F);
      }
      tf_from12(P->tool, Tl);
      tf_mul(F, Tl, src);
    }
    tf_mul(tinv, src, pp);
    double ax[3], ang;
    if (k < D)
      rot_err_decomposed(pp.R, ax, ang);
    else
    {
      double err[6];
      transform_error(tinv, src, err, ax, ang);
      for (int r = 0; r < 6; ++r)
        errv[c * 6 + r] = err[r];
    }
    double* o = rec + (size_t)item * 7;
    for (int r = 0; r < 3; ++r)
    {
      o[r] = pp.t[r];
      o[3 + r] = ax[r];
    }
    o[6] = ang;
  }
  TMX_SYNC();
  // ---- phase 3: the finite-difference Jacobians; the collision rows from the frames
  for (int item = tid; item < n_cp * D; item += NT)
  {
    const int c = item / D, k = item % D;
    const double* o0 = rec + ((size_t)c * (D + 1) + D) * 7;  // base pose
    const double* o1 = rec + ((size_t)c * (D + 1) + k) * 7;
    const double a0 = o0[6], a1 = o1[6];
    // calcJacobianTransformErrorDiff(target, source, source_perturbed)
    double a1c = a1;
    if (a1 > M_PI_2 && a0 < -M_PI_2)
      a1c = a1 - 2.0 * M_PI;
    else if (a1 < -M_PI_2 && a0 > M_PI_2)
      a1c = a1 + 2.0 * M_PI;
    for (int i = 0; i < P->cp_nrows[c]; ++i)
    {
      const int r = P->cp_idx[6 * c + i];
      const double diff = (r < 3) ? o1[r] - o0[r] : o1[r] * a1c - o0[r] * a0;
      Jm[((size_t)c * 6 + i) * D + k] = diff / TMX_EPS_FD;
    }
  }
  for (int r = tid; r < P->R; r += NT)
  {
    if (P->slot_kind[r] != SLOT_COLLISION)
      continue;
    const int t = P->slot_t[r];
    const double* q = xv + t * D;
    const int s = P->slot_sub[r], o = P->slot_sub2[r];
    const int link = P->ls_link[s];
    double n[3], pw[3];
    Tf3 L;
    frame_get(FL + (size_t)(t * D + link) * 12, L);
    const double dist = contact_distance_at<false>(P, L, s, o, n, pw);
    const double margin = P->slot_aux1[r];
    if (dist > margin + P->slot_aux2[r])
    {
      active[r] = 0;
      for (int k = 0; k < D; ++k)
        coef[r * D + k] = 0.0;
      rhs[r] = 0.0;
      continue;
    }
    // gradient = -n' * J_trans(nearest point) over the joints up to the link, from their frames before motion; the raw gradient is
    // staged in the row's coefficient array (the statements of convexify_terms)
    double* grad = coef + (size_t)r * D;
    double gq = 0.0;
    for (int k = 0; k <= link; ++k)
    {
      Tf3 F;
      frame_get(FU + (size_t)(t * D + k) * 12, F);
      const double g = contact_grad_col(P, k, F, pw, n);
      grad[k] = g;
      gq += g * q[k];
    }
    for (int k = link + 1; k < D; ++k)
    {
      const double g = -1.0 * (n[0] * 0.0 + n[1] * 0.0 + n[2] * 0.0);
      grad[k] = g;
      gq += g * q[k];
    }
    // dist_expr = grad.x + (-(grad.q) + dist) ; viol = margin - dist_expr ; row: viol - hinge <= 0
    const double c_dist = (0.0 + (-gq)) + dist;
    const double viol_const = margin - c_dist;
    if (P->slot_iscnt[r])
    {
      const double cc = P->slot_scale[r];
      for (int k = 0; k < D; ++k)
        coef[r * D + k] = (-grad[k]) * cc;
      rhs[r] = -(viol_const * cc);
    }
    else
    {
      for (int k = 0; k < D; ++k)
        coef[r * D + k] = -grad[k];
      rhs[r] = -viol_const;
    }
    active[r] = 1;
  }
  TMX_SYNC();
  // ---- phase 4: the cart-pose rows (affFromValGrad: constant = y - J.x ; coeffs = J with |c| <= 1e-7 dropped ; exprScale)
  for (int item = tid; item < n_cp * 6; item += NT)
  {
    const int c = item / 6, i = item % 6;
    if (i >= P->cp_nrows[c])
      continue;
    const double* q = xv + P->cp_t[c] * D;
    const double* Jr = Jm + ((size_t)c * 6 + i) * D;
    const double y = errv[c * 6 + P->cp_idx[6 * c + i]];
    double dot = 0.0;
    for (int k = 0; k < D; ++k)
      dot += Jr[k] * q[k];
    const double cc = P->cp_coeff[6 * c + i];
    const int r = P->cp_slot0[c] + i;
    const double constant = (y - dot) * cc;
    for (int k = 0; k < D; ++k)
    {
      const double jv = Jr[k];
      coef[r * D + k] = (fabs(jv) > TMX_CLEANUP_TOL) ? jv * cc : 0.0;
    }
    rhs[r] = -constant;
    active[r] = 1;
  }
  TMX_SYNC();
}
#endif
