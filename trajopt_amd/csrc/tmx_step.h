// The SQP shell around the QP solve (sqp_step_block, tmx_kernels.h) for problems of the dense fast path: code that knows the problem
// class instead of the generic code of tmx_solve.h.
//
// qp_structure_fast: dims, the four hashes and row_ref / aux_ref of a convexification, as qp_structure<false> leaves them when it
// exports nothing.  The generic code forms its three exclusive prefix sums (rows, slack variables, column pointers) by every
// thread summing the entries of all its predecessors out of LDS - up to 255 dependent reads twice and n reads per column pointer - and
// walks the row list of a column twice through dependent loads (count, then hash).  Here
//  * the row and slack prefix counts come from wave ballots (block_excl_count8, tmx_setup.h: the routine of the QP setup)
//  * thread v < NX owns column v (the ownership of ruiz_fast): it reads the <= TMX_SETUP_COL coefficients of its column once, with
//    independent loads, into a non-zero mask and the reference row of every entry; the count and the hash terms come from the mask
//  * the column pointers over all n + 1 columns come from a wave scan per 256 columns plus the wave totals
// What keeps the bits: everything is an integer.  The hashes are wrap-around u64 sums of position-keyed terms (tmx_hash_term), so the
// order of the terms is free; positions, values and salts are the generic code's.
// Preconditions (DevProblem::step_fast, set at upload, and the caller): TMX_QP_NT threads, one waypoint per row, 1 <= R <= 2 NT,
// NX <= NT and a shape the dense partition takes (dpart_fits: the problems of the QP fast path), at most TMX_SETUP_COL rows per waypoint and two slack variables per row, n_max + 1 <= TMX_STEP_CP_PASSES * NT, no compact
// row lists, a static objective pattern without second / third differences.  dbg_flags bit 3 keeps the generic code on such a problem
// (tests/test_fast_step.py compares the two in one library).
#pragma once
#include "tmx_solve.h"
#include "tmx_eval.h"

#define TMX_STEP_CP_PASSES 6  // passes of NT columns of the column-pointer scan: NX + 2 R + 1 <= 256 + 1024 + 1

#if TMX_IS_DEVICE
TMX_DEVFN void qp_structure_fast(const DevProblem* P, const int* active, const double* coef, int* dims, unsigned long long* hashes,
                                 int* iscratch, int tid TMX_F5_PARAMS)
{
  constexpr int NT = TMX_QP_NT;
  const int D = P->D, NX = P->NX, R = P->R;
  // (the layout of qp_structure)
  int* colptr = iscratch;               // n_max + 1
  int* rowref = colptr + P->n_max + 1;  // R
  int* auxref = rowref + R;             // R
  int* lact = auxref + R;               // R
  int* lnaux = lact + R;                // R
  int* ccount = lnaux + R;              // n_max + 1
  int acc_off = 2 * (P->n_max + 1) + 4 * R;
  acc_off += (acc_off & 1);
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(iscratch + acc_off);  // 8 x u64
  int* scan = iscratch + acc_off + 16;                                                  // NT ints: wave totals of the scans ...
  int* nm = scan + TMX_STEP_CP_PASSES * (NT / 64);                                      // ... and behind them n and m
  for (int r = tid; r < R; r += NT)
  {
    lact[r] = active[r] ? 1 : 0;
    lnaux[r] = P->slot_naux[r];
  }
  for (int k = tid; k < 8; k += NT)
    acc[k] = 0ULL;
  TMX_SYNC();
  // exclusive prefix counts of the active rows and of their slack variables: one contiguous chunk of C <= 2 slots per thread
  {
    const int C = (R + NT - 1) / NT;
    const int r0 = tid * C < R ? tid * C : R, r1 = (tid + 1) * C < R ? (tid + 1) * C : R;
    int tot_r = 0;
    for (int pass = 0; pass < 2; ++pass)
    {
      int cnt = 0;
      for (int r = r0; r < r1; ++r)
        cnt += lact[r] ? (pass == 0 ? 1 : lnaux[r]) : 0;
      int off = block_excl_count8(cnt, scan, tid);
      for (int r = r0; r < r1; ++r)
      {
        if (pass == 0)
          rowref[r] = off;
        else
          auxref[r] = NX + off;
        off += lact[r] ? (pass == 0 ? 1 : lnaux[r]) : 0;
      }
      if (tid == NT - 1)
      {
        if (pass == 0)
          tot_r = off;
        else
        {
          dims[0] = NX + off;          // n
          dims[1] = tot_r + NX + off;  // m
          nm[0] = NX + off;
          nm[1] = tot_r + NX + off;
        }
      }
    }
  }
  TMX_SYNC();
  const int n = TMX_UNI_I(nm[0]), m = TMX_UNI_I(nm[1]), mg = m - n;
  // column v of A: non-zero mask over the row list of its waypoint, the reference row of every entry
  const bool pv = tid < NX;
  const int v = pv ? tid : 0, vt = v / D, vj = v - vt * D;
  unsigned mask = 0u;
  int rref[TMX_SETUP_COL];
  {
    const int q0 = P->wp_start[vt], q1 = P->wp_start[vt + 1];
#pragma unroll
    for (int k = 0; k < TMX_SETUP_COL; ++k)
    {
      const bool ok = pv && q0 + k < q1;
      const int r = ok ? P->wp_list[q0 + k] : 0;
      const double cv = ok ? coef[r * D + vj] : 0.0;
      rref[k] = rowref[r];
      mask |= (ok && lact[r] != 0 && cv != 0.0) ? (1u << k) : 0u;
    }
  }
  if (pv)
    ccount[v] = 1 + __builtin_popcount(mask);
  for (int r = tid; r < R; r += NT)
    if (lact[r])
      for (int k = 0; k < lnaux[r]; ++k)
        ccount[auxref[r] + k] = 2;
  TMX_SYNC();
  // column pointers: inclusive scan inside the wave, the totals of the waves (and passes) below through `scan`
  const int npass = (n + 1 + NT - 1) / NT;  // <= TMX_STEP_CP_PASSES, uniform
  const int lane = tid & 63, wave = tid >> 6;
  int cp[TMX_STEP_CP_PASSES];
#pragma unroll
  for (int p = 0; p < TMX_STEP_CP_PASSES; ++p)
  {
    cp[p] = 0;
    if (p < npass)
    {
      const int c = p * NT + tid;
      const int own = c < n ? ccount[c] : 0;
      int x = own;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1)
      {
        const int y = __shfl(x, lane >= d ? lane - d : lane, 64);
        x += lane >= d ? y : 0;
      }
      cp[p] = x - own;
      if (lane == 63)
        scan[p * (NT / 64) + wave] = x;
    }
  }
  TMX_SYNC();
  {
    int base = 0;
    for (int u = 0; u < wave; ++u)
      base += scan[u];
#pragma unroll
    for (int p = 0; p < TMX_STEP_CP_PASSES; ++p)
      if (p < npass)
      {
        cp[p] += base;
        const int c = p * NT + tid;
        if (c <= n)
          colptr[c] = cp[p];
        if (c == n)
        {
          dims[3] = cp[p];  // nnzA
          dims[2] = P->nnzP;
        }
        if (p + 1 < npass)
          for (int u = 0; u < NT / 64; ++u)
            base += scan[p * (NT / 64) + wave + u];
      }
  }
  TMX_SYNC();
  TMX_F5_TICK(15);
  const int nnzA = TMX_UNI_I(colptr[n]);
  // hashes of A: colptr (salt 3) + rowidx (salt 4); prefix hashes for the weak memcmp
  unsigned long long hA = 0ULL, wsA = 0ULL;
  const int cp_bytes = n + 1, cp_full = cp_bytes / 8, cp_rem = cp_bytes % 8;
  const int ri_bytes = nnzA, ri_full = ri_bytes / 8, ri_rem = ri_bytes % 8;
#pragma unroll
  for (int p = 0; p < TMX_STEP_CP_PASSES; ++p)
  {
    const int c = p * NT + tid;
    if (p < npass && c <= n)
    {
      const long long val = cp[p];
      hA += tmx_hash_term(val, (uint64_t)c, 3);
      if (c < cp_full)
        wsA += tmx_hash_term(val, (uint64_t)c, 13);
      else if (c == cp_full && cp_rem > 0)
        wsA += tmx_hash_term((long long)((unsigned long long)val & ((1ULL << (8 * cp_rem)) - 1ULL)), (uint64_t)c, 13);
    }
  }
  auto row_term = [&](long long ri, int pos) {
    hA += tmx_hash_term(ri, (uint64_t)pos, 4);
    if (pos < ri_full)
      wsA += tmx_hash_term(ri, (uint64_t)pos, 14);
    else if (pos == ri_full && ri_rem > 0)
      wsA += tmx_hash_term((long long)((unsigned long long)ri & ((1ULL << (8 * ri_rem)) - 1ULL)), (uint64_t)pos, 14);
  };
  if (pv)
  {
    // row indices of the primary column: its rows in list order, then the identity row of the variable bounds
    int pos = cp[0];
#pragma unroll
    for (int k = 0; k < TMX_SETUP_COL; ++k)
      if (mask & (1u << k))
      {
        row_term(rref[k], pos);
        ++pos;
      }
    row_term(mg + v, pos);
  }
  for (int r = tid; r < R; r += NT)
    if (lact[r])
      for (int k = 0; k < lnaux[r]; ++k)
      {
        const int col = auxref[r] + k;
        const int pos = colptr[col];
        row_term(rowref[r], pos);
        row_term(mg + col, pos + 1);
      }
  TMX_F5_TICK(6);
  // P: static pattern over the primary vars (upper triangle): (v-D, v) if po != 0 ; (v, v) if pd != 0; aux columns are empty.  Its
  // hashes depend on n alone: the upload-time table (DevProblem::p_hash, tmx_eval.h) on the problems that have one, else - and under
  // dbg_flags bit 4 - the sum over the columns
  const bool p_tab = TMX_UNI_B(P->eval_fast != 0 && !(P->dbg_flags & 16));
  if (!p_tab)
  {
    unsigned long long hP = 0ULL, wsP = 0ULL;
    for (int c = tid; c <= n; c += NT)
      p_hash_column(P->p_colptr, P->pd, P->po, D, NX, P->nnzP, n, c, hP, wsP);
    TMX_ATOMIC_ADD_U64(&acc[0], hP);
    TMX_ATOMIC_ADD_U64(&acc[2], wsP);
  }
  TMX_ATOMIC_ADD_U64(&acc[1], hA);
  TMX_ATOMIC_ADD_U64(&acc[3], wsA);
  TMX_SYNC();
  if (tid == 0)
  {
    const unsigned long long* e = P->p_hash + 2 * (size_t)(n - NX);  // (read with p_tab only)
    hashes[0] = p_tab ? e[0] : acc[0];
    hashes[1] = acc[1];
    hashes[2] = p_tab ? e[1] : acc[2];
    hashes[3] = acc[3];
  }
  TMX_SYNC();
}

// sqp_update_fast: sqp_update_block<false> with the decision fed from LDS.  The generic code runs sqp_decide on thread 0 against the
// arrays of the batch: about 7 (n_costs + n_cnts) loads and as many stores of the step log by one lane, through pointers the compiler
// must take to alias, while 255 threads wait at the barrier.  Here the workgroup copies the five vectors the decision reads (old /
// new costs and violations, merit coefficients) into the dead evaluation scratch behind the model values, thread 0 decides from the
// copies - the sums stay serial, in the reference's order, on the same values (sqp_decide_io) - and the workgroup writes the step log,
// one entry per thread.  The scalar bookkeeping and the merit inflation stay on thread 0, in their order.
// Room (DevProblem::step_fast): n_costs + 2 n_cnts + 1 doubles more than the model values need fit the scratch of evaluate_terms.
TMX_DEVFN void sqp_update_fast(const DevProblem* P, const DevBatch* Bt, int b, double* smem, int tid, bool have_model TMX_F5_PARAMS)
{
  constexpr int NT = TMX_QP_NT;
  const int NX = P->NX, nc = P->n_costs, nv = P->n_cnts;
  double* model_cost = smem;         // n_costs
  double* model_viol = smem + nc;    // n_cnts
  double* l_cost = model_viol + nv;  // the copies: 2 n_costs + 3 n_cnts, then the head record of the step log
  double* l_new_cost = l_cost + nc;
  double* l_viol = l_new_cost + nc;
  double* l_new_viol = l_viol + nv;
  double* l_merit = l_new_viol + nv;
  double* head = l_merit + nv;  // TMX_STEP_LOG_HEAD + 1
  double* cost_vals = Bt->cost_vals + (size_t)b * nc;
  double* cnt_viols = Bt->cnt_viols + (size_t)b * nv;
  const double* new_cost = Bt->new_cost_vals + (size_t)b * nc;
  const double* new_viol = Bt->new_cnt_viols + (size_t)b * nv;
  const double* merit = Bt->merit + (size_t)b * nv;
  const bool solved = Bt->cvx[b] == TMX_CVX_SOLVED && Bt->phase[b] != PHASE_DONE;
  // (have_model: step_eval_fast, tmx_eval.h, has left the model values with the exact evaluation)
  if (solved && !have_model)
    sqp_model_values<false>(P, Bt, b, Bt->xq + (size_t)b * P->n_max, smem, tid, NT);  // (ends with a barrier: its scratch is dead)
  TMX_F5_TICK(14);
  for (int k = tid; k < nc; k += NT)
  {
    l_cost[k] = cost_vals[k];
    l_new_cost[k] = new_cost[k];
  }
  for (int k = tid; k < nv; k += NT)
  {
    l_viol[k] = cnt_viols[k];
    l_new_viol[k] = new_viol[k];
    l_merit[k] = merit[k];
  }
  if (tid == 0)
    head[TMX_STEP_LOG_HEAD] = 0.0;
  TMX_SYNC();
  if (tid == 0)
  {
    Bt->accept_flag[b] = 0;
    const DecideIo io = { l_cost, l_viol, l_new_cost, l_new_viol, l_merit, head };
    sqp_decide_io(P, Bt, b, model_cost, model_viol, io);
  }
  TMX_SYNC();
  // BasicTrustRegionSQPResults of this evaluation -> Bt->step_log (the layout of step_log_write)
  const double logged = head[TMX_STEP_LOG_HEAD];
  if (logged != 0.0)
  {
    double* o = Bt->step_log + (size_t)b * Bt->step_log_stride;
    for (int k = tid; k < 10; k += NT)
      o[k] = head[k];
    if (logged == 2.0)
    {
      double* q = o + TMX_STEP_LOG_HEAD;
      for (int k = tid; k < nc; k += NT)
      {
        q[k] = l_cost[k];
        q[nc + k] = model_cost[k];
        q[2 * nc + k] = l_new_cost[k];
      }
      q += 3 * nc;
      for (int k = tid; k < nv; k += NT)
      {
        q[k] = l_viol[k];
        q[nv + k] = model_viol[k];
        q[2 * nv + k] = l_new_viol[k];
        q[3 * nv + k] = l_merit[k];
      }
    }
  }
  if (Bt->accept_flag[b])
  {
    double* x = Bt->x + (size_t)b * NX;
    const double* xn = Bt->xnew + (size_t)b * NX;
    for (int v = tid; v < NX; v += NT)
      x[v] = xn[v];
    for (int k = tid; k < nc; k += NT)
      cost_vals[k] = l_new_cost[k];
    for (int k = tid; k < nv; k += NT)
      cnt_viols[k] = l_new_viol[k];
  }
}

// As functions of their own, entered once per convexification / per step (as qp_ruiz_fast_nl / qp_polish_fast_nl): their registers do
// not join the allocation of the kernel's cold code.
#if TMX_ADMM_OUTLINED
__device__ __attribute__((noinline)) static void qp_structure_fast_nl(const DevProblem* P_in, const DevBatch* Bt_in, int b_in, unsigned lds_in)
{
  const DevProblem* P = tmx_uniform_ptr(P_in);
  const DevBatch* Bt = tmx_uniform_ptr(Bt_in);
  const int b = __builtin_amdgcn_readfirstlane(b_in);
  const int tid = threadIdx.x;
  double* smem = (double*)(tmx_lds_d*)(size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)lds_in);
  qp_structure_fast(P, Bt->active + (size_t)b * P->R, Bt->coef + (size_t)b * P->R * P->D, Bt->dims + 4 * b, Bt->hashes + 4 * b,
                    reinterpret_cast<int*>(smem), tid);
}
__device__ __attribute__((noinline)) static void sqp_update_fast_nl(const DevProblem* P_in, const DevBatch* Bt_in, int b_in, unsigned lds_in)
{
  const DevBatch* Bt = tmx_uniform_ptr(Bt_in);
  const int b = __builtin_amdgcn_readfirstlane(b_in);
  const DevProblem* P = tmx_uniform_ptr(query_problem(P_in, Bt, b));  // (multi-query batches: the exact evaluation reads goal targets)
  const int tid = threadIdx.x;
  double* smem = (double*)(tmx_lds_d*)(size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)lds_in);
  // on the problems of DevProblem::eval_fast the caller has skipped evaluate_terms: exact evaluation and model values as one pass
  // (tmx_eval.h) in front of the decision
  const bool merged = TMX_UNI_B(P->eval_fast != 0 && !(P->dbg_flags & 16));
  if (merged)
    step_eval_fast(P, Bt, b, smem, tid);
  sqp_update_fast(P, Bt, b, smem, tid, merged);
}
// the convexification of the problems of DevProblem::eval_fast (tmx_eval.h)
__device__ __attribute__((noinline)) static void convexify_fast_nl(const DevProblem* P_in, const DevBatch* Bt_in, int b_in, unsigned lds_in)
{
  const DevBatch* Bt = tmx_uniform_ptr(Bt_in);
  const int b = __builtin_amdgcn_readfirstlane(b_in);
  const DevProblem* P = tmx_uniform_ptr(query_problem(P_in, Bt, b));  // (multi-query batches: the cart-pose rows read goal targets)
  const int tid = threadIdx.x;
  double* smem = (double*)(tmx_lds_d*)(size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)lds_in);
  convexify_fast(P, Bt->x + (size_t)b * P->NX, Bt->active + (size_t)b * P->R, Bt->coef + (size_t)b * P->R * P->D, Bt->rhs + (size_t)b * P->R, smem, tid);
}
#endif
#endif
