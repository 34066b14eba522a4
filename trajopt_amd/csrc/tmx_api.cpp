// tmx_api.cpp — host side of libtrajopt_mi355x.so: the C-ABI of include/tmx.h.
// Lowers the problem description to the device term table / row-slot template, owns all device memory, and drives
// the batched SQP (convexify -> QP solve -> exact re-evaluation -> decisions) as a short chain of kernel launches per
// trust-region evaluation on one HIP stream; the host only reads back one "problems still running" counter.
#include <algorithm>
#include <cstddef>
#include <limits>
#include <string>
#include <vector>

#include "tmx_kernels.h"
#include "tmx_check.h"
#include "tmx_check_self.h"
#include "tmx_wave_kernels.h"
#include "tmx_wave_plan.h"
#include "tmx_row_perm.h"
#include "tmx_upload.h"
#include "tmx_csc_order.h"

#ifdef TMX_HOST_EMU
#include <chrono>
thread_local tmx_emu_idx tmx_emu_threadIdx, tmx_emu_blockIdx, tmx_emu_blockDim, tmx_emu_gridDim;
thread_local double* tmx_emu_smem = nullptr;
double tmx_emu_now_ms()
{
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
#else
#include <rccl/rccl.h>
#endif

#define HIPCHK(call)                                                                                                  \
  do                                                                                                                  \
  {                                                                                                                   \
    hipError_t e_ = (call);                                                                                           \
    if (e_ != hipSuccess)                                                                                             \
    {                                                                                                                 \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                                                   \
      return TMX_ERR_DEVICE;                                                                                          \
    }                                                                                                                 \
  } while (0)

struct tmx_ctx
{
  int device{ 0 };
  hipStream_t stream{ nullptr };
  std::string err;
  bool have_problem{ false };
  DevProblem hp{};        // host copy (device pointers inside)
  DevProblem* dp{ nullptr };
  DevBatch hb{};
  DevBatch* db{ nullptr };
  int Bcap{ 0 };
  std::vector<void*> prob_allocs, batch_allocs;
  long long* d_totals{ nullptr };
  size_t smem_qp{ 0 }, smem_small{ 0 }, smem_pool{ 0 }, ws_bytes{ 0 }, smem_chain{ 0 };
  int nt_qp{ 64 }, nt_small{ 64 };
  hipEvent_t ev0{ nullptr }, ev1{ nullptr };
  double ms_admm{ 0 }, ms_convexify{ 0 }, ms_evaluate{ 0 };
  long long launches_admm{ 0 };
  bool timing{ true };
  int pending{ 0 };  // a tmx_sqp_launch() not yet collected by tmx_sqp_wait()
  bool clock_started{ false };  // k_mark_start ran since the last tmx_batch_set_x0 (start of optimize(): sqp.max_time)
  long long pool_relaunches{ 0 };  // times tmx_sqp_wait had to restart the pool (expected: 0)
  int* h_tail{ nullptr };  // pinned, device-mapped word: 1 once the pool kernel of the pending launch has begun to retire workgroups
  bool dense{ false };      // DevProblem::qp_dense: Model::optimize() by k_qp_solve_dense
  bool band{ false };       // DevProblem::band: the pool driver launches k_sqp_pool_band
  size_t tt_scratch{ 0 };   // doubles the rank-one terms of TotalTime terms on the block chain add to the per-problem scratch (DevProblem::tt_place 2)
  bool tt_squared{ false }; // a TotalTime cost in its squared form (dense objective block over the time variables)
  bool hull{ false };       // DevProblem::n_ls_hull > 0: the term kernels are the *_hull instantiations (GJK / EPA contacts)
  bool piecewise{ false };  // DevProblem::st: the piecewise driver runs optimize() (host loop) - dense problems and row-only function terms
  bool ws_in_hbm{ false };  // QP workspace > 160 KB of LDS: k_*_hbm kernels, workspace carved in HBM (long horizons)
  int mode{ 2 };  // optimize() driver: 0 = one launch chain per step, 1 = k_sqp_fused, 2 = k_sqp_pool (default)
  bool wave{ false };      // DevProblem::wave_ok: optimize() and Model::optimize() run as a wave pair per problem (tmx_wave.h: k_sqp_wave / k_qp_solve_wave)
  size_t smem_wave{ 0 };
  int pool_wgs{ 0 };  // resident workgroups of the pool kernel (0 = CUs x workgroups-per-CU)
  void* nccl{ nullptr };
  bool nccl_owned{ false };
  double* d_pair{ nullptr };   // K7: [2] local (cost, index) + [2 * n_ranks] gathered pairs
  int pair_cap{ 0 };
  // result of the last tmx_argmin: owner rank of the winning pair (-1: no converged seed anywhere), its LOCAL problem index on the
  // owner (global index - the owner's global_offset; valid on the owner only), the rank count it was reduced over
  int best_owner{ -1 }, best_nranks{ 1 };
  long long best_local{ -1 }, best_global{ -1 };
  double* d_best{ nullptr };   // T * D + 1 doubles: the broadcast buffer of tmx_best_trajectory (trajectory, status word)
  size_t best_cap{ 0 };
  int max_rec{ 128 };
  // Multi-query batches (tmx_queries_set; DevBatch::q_prob / q_cp_target / q_aux1).  n_queries = 1: no table, null pointers.
  int n_queries{ 1 };
  std::vector<void*> query_allocs;
  DevProblem* d_qprob{ nullptr };
  double *d_qcp{ nullptr }, *d_qaux1{ nullptr };
  std::vector<double> own_cp, own_aux1;  // the description's own targets (Lowered::cp_target / aux1)
  std::vector<int> own_sub;              // Lowered::sub (the joint of a joint-position slot)
  std::vector<double> h_qcp, h_qaux1;    // host mirrors of the per-query tables
  // per term of the description: its kind and its ranges of cart-pose instances and row slots (Lowered::term_*)
  std::vector<int> term_kind, term_cp0, term_cp1, term_slot0, term_slot1;
  int n_dof{ 0 };
  // Bcap = 0 also says "no valid batch" (every entry point tests it): Balloc keeps the allocated capacity across an invalidation
  int Balloc{ 0 };
  // tmx_qp_solve_batched: the engine selector (tmx_qp_engine_set; a property of the context: tmx_problem_upload leaves it) and what
  // the last call used per QP (tmx_qp_engine_last)
  int qp_engine{ TMX_QP_ENGINE_DENSE };
  std::vector<int> qp_last_engine, qp_last_block, qp_last_nblocks, qp_last_place;
  // Self-collision side of the trajectory check (tmx_check_set_link_pairs): the link pairs in the caller's order, the primitive pairs
  // they expand to (host mirror and device table, 2 ints each), and the link of every primitive of the uploaded problem
  std::vector<int> check_link_pairs, check_prim_pairs, h_ls_link;
  int* d_check_pairs{ nullptr };
};

template <typename T>
static tmx_status upload(tmx_ctx* ctx, std::vector<void*>& pool, T** dst, const std::vector<T>& src)
{
  void* p = nullptr;
  const size_t bytes = std::max<size_t>(1, src.size()) * sizeof(T);
  HIPCHK(hipMalloc(&p, bytes));
  pool.push_back(p);
  if (!src.empty())
    HIPCHK(hipMemcpy(p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  *dst = static_cast<T*>(p);
  return TMX_OK;
}
template <typename T>
static tmx_status dalloc(tmx_ctx* ctx, std::vector<void*>& pool, T** dst, size_t count, bool zero = true)
{
  void* p = nullptr;
  const size_t bytes = std::max<size_t>(1, count) * sizeof(T);
  HIPCHK(hipMalloc(&p, bytes));
  // zero fill ordered on the context's stream (a null-stream hipMemset would wait for every blocking stream of the device,
  // i.e. for the other context's batch in flight)
  if (zero)
    HIPCHK(hipMemsetAsync(p, 0, bytes, ctx->stream));
  pool.push_back(p);
  *dst = static_cast<T*>(p);
  return TMX_OK;
}
// Entry points that modify or read the batch refuse while a tmx_sqp_launch() is pending: they would re-prepare, reallocate
// or read a batch that is still running (tmx_sqp_wait() collects it first).
#define TMX_REFUSE_WHILE_PENDING(ctx)                                                                                 \
  do                                                                                                                  \
  {                                                                                                                   \
    if ((ctx)->pending)                                                                                               \
    {                                                                                                                 \
      (ctx)->err = "a tmx_sqp_launch() is pending on this context: call tmx_sqp_wait() first";                        \
      return TMX_ERR_STATE;                                                                                           \
    }                                                                                                                 \
  } while (0)
static void free_pool(std::vector<void*>& pool)
{
  for (void* p : pool)
    (void)hipFree(p);
  pool.clear();
}

template <typename T>
static tmx_status d2h(tmx_ctx* ctx, T* dst, const T* src, size_t count)
{
  if (!dst)
    return TMX_OK;
  HIPCHK(hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyDeviceToHost, ctx->stream));
  return TMX_OK;
}

extern "C" {

void tmx_default_sqp_params(tmx_sqp_params* p)
{
  p->improve_ratio_threshold = 0.25;
  p->min_trust_box_size = 1e-4;
  p->min_approx_improve = 1e-4;
  p->min_approx_improve_frac = -1.7976931348623157e308;  // std::numeric_limits<double>::lowest()
  p->max_iter = 50;
  p->max_qp_solver_failures = 3;
  p->trust_shrink_ratio = 0.1;
  p->trust_expand_ratio = 1.5;
  p->cnt_tolerance = 1e-4;
  p->max_merit_coeff_increases = 5;
  p->merit_coeff_increase_ratio = 10;
  p->initial_merit_error_coeff = 10;
  p->inflate_constraints_individually = 1;
  p->pad_ = 0;
  p->trust_box_size = 1e-1;
  p->max_time = std::numeric_limits<double>::max();
}

void tmx_default_osqp_settings(tmx_osqp_settings* s)
{
  s->rho = 0.1;
  s->sigma = 1e-6;
  s->alpha = 1.6;
  s->eps_abs = 1e-4;
  s->eps_rel = 1e-6;
  s->eps_prim_inf = 1e-4;
  s->eps_dual_inf = 1e-4;
  s->adaptive_rho_tolerance = 5.0;
  s->delta = 1e-6;
  s->scaling = 10;
  s->adaptive_rho = 1;
  s->adaptive_rho_interval = 50;
  s->max_iter = 8192;
  s->polishing = 1;
  s->polish_refine_iter = 3;
  s->check_termination = 25;
  s->warm_starting = 1;
}

tmx_status tmx_create(int device, tmx_ctx** out)
{
  if (!out)
    return TMX_ERR_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return TMX_ERR_DEVICE;  // no HIP device: fail loudly, there is no CPU fallback
  if (device < 0 || device >= count)
    return TMX_ERR_INVALID;
  tmx_ctx* ctx = new tmx_ctx();
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&ctx->stream) != hipSuccess ||
      hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess)
  {
    delete ctx;
    return TMX_ERR_DEVICE;
  }
#ifdef TMX_HOST_EMU
  ctx->h_tail = new int(0);
#else
  {
    void* hp = nullptr;
    if (hipHostMalloc(&hp, sizeof(int), hipHostMallocMapped) != hipSuccess)
    {
      delete ctx;
      return TMX_ERR_DEVICE;
    }
    ctx->h_tail = static_cast<int*>(hp);
    *ctx->h_tail = 0;
  }
#endif
  void* p = nullptr;
  if (hipMalloc(&p, 4 * sizeof(long long)) != hipSuccess)
  {
    delete ctx;
    return TMX_ERR_DEVICE;
  }
  ctx->d_totals = static_cast<long long*>(p);
  *out = ctx;
  return TMX_OK;
}

void tmx_destroy(tmx_ctx* ctx)
{
  if (!ctx)
    return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  free_pool(ctx->prob_allocs);
  free_pool(ctx->batch_allocs);
  free_pool(ctx->query_allocs);
  if (ctx->dp)
    (void)hipFree(ctx->dp);
  if (ctx->db)
    (void)hipFree(ctx->db);
  if (ctx->d_totals)
    (void)hipFree(ctx->d_totals);
  if (ctx->d_pair)
    (void)hipFree(ctx->d_pair);
  if (ctx->d_best)
    (void)hipFree(ctx->d_best);
  if (ctx->d_check_pairs)
    (void)hipFree(ctx->d_check_pairs);
#ifdef TMX_HOST_EMU
  delete ctx->h_tail;
#else
  if (ctx->h_tail)
    (void)hipHostFree(ctx->h_tail);
#endif
#ifndef TMX_HOST_EMU
  if (ctx->nccl && ctx->nccl_owned)
    (void)ncclCommDestroy(static_cast<ncclComm_t>(ctx->nccl));
#endif
  (void)hipEventDestroy(ctx->ev0);
  (void)hipEventDestroy(ctx->ev1);
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char* tmx_last_error(const tmx_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// ---- tmx_problem_upload: the description -> DevProblem, in five stages (tmx_upload.h) ----

// the waypoint layout, the kinematic chain and the solver parameters
static void fill_basic_info(const tmx_problem_desc* d, const tmx_sqp_params* sqp, const tmx_osqp_settings* osqp, DevProblem& P)
{
  const int DK = d->n_dof, T = d->n_steps, D = DK + (d->use_time ? 1 : 0);
  std::memset(&P, 0, sizeof(P));
  P.D = D;
  P.DK = DK;
  P.use_time = d->use_time ? 1 : 0;
  P.T = T;
  P.NX = D * T;
  P.S = d->n_link_spheres;
  P.O = d->n_obstacles;
  for (int j = 0; j < DK; ++j)
  {
    P.jl[j] = d->joint_lower[j];
    P.ju[j] = d->joint_upper[j];
    std::memcpy(P.origin[j], d->joints[j].origin, sizeof(double) * 12);
    std::memcpy(P.axis[j], d->joints[j].axis, sizeof(double) * 3);
    P.jtype[j] = d->joints[j].type;
  }
  if (d->use_time)
  {
    // the time column as seen by the kinematic code: a prismatic joint with a zero axis behind the last link - no motion, a zero
    // Jacobian column; its variable bounds are the dt limits (TrajOptProb ctor, problem_description.cpp:583-588)
    P.jl[DK] = d->dt_lower_lim;
    P.ju[DK] = d->dt_upper_lim;
    const double ident[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    std::memcpy(P.origin[DK], ident, sizeof(ident));
    P.axis[DK][0] = P.axis[DK][1] = P.axis[DK][2] = 0.0;
    P.jtype[DK] = 1;
  }
  std::memcpy(P.base, d->base, sizeof(double) * 12);
  std::memcpy(P.tool, d->tool, sizeof(double) * 12);
  if (sqp)
    P.sqp = *sqp;
  else
    tmx_default_sqp_params(&P.sqp);
  if (osqp)
    P.osqp = *osqp;
  else
    tmx_default_osqp_settings(&P.osqp);
}

// Stage 1: validates the description and lowers the terms into the row-slot template, the static Hessian and the per-kind tables;
// then the waypoint grouping of the slots and the geometry tables.  No HIP call; writes the counts into P.
static tmx_status lower_terms(const tmx_problem_desc* d, DevProblem& P, Lowered& L, std::string& err)
{
  const int DK = P.DK, D = P.D, T = P.T;
  // ---- slot template in reference row order ----
  auto add_slot = [&](int k, int t, int s1, int s2, int own, int na, int isc, int eq, double oc, double sc, double a1, double a2) {
    L.kind.push_back(k);
    L.st.push_back(t);
    L.sub.push_back(s1);
    L.sub2.push_back(s2);
    L.owner.push_back(own);
    L.naux.push_back(na);
    L.iscnt.push_back(isc);
    L.iseq.push_back(eq);
    L.objc.push_back(oc);
    L.scale.push_back(sc);
    L.aux1.push_back(a1);
    L.aux2.push_back(a2);
    L.c2.push_back(-1);
    L.sub3.push_back(0);
    L.aux3.push_back(0.0);
  };
  // DiscreteCollisionEvaluator (evaluator_type 2) / CastCollisionEvaluator (3, 4): one term per SEGMENT (i, i+1)
  // (problem_description.cpp:1720-1761, :1779-1819); per (link sphere, obstacle) max_substates row slots in the order of the
  // flattened contact map (pair-major, sub-state ascending).  Cost and constraint forms share this construction.
  auto add_lvs_segments = [&](const tmx_term& tm) -> tmx_status {
#if !TMX_LINK_ROWS
    (void)tm;
    err = "rows on two consecutive waypoints (LVS / continuous collision) are not enabled in this build";
    return TMX_ERR_UNSUPPORTED;
#else
    if (!(tm.longest_valid_segment_length >= 0))
    {
      err = "collision: longest_valid_segment_length must be >= 0";  // :1634
      return TMX_ERR_INVALID;
    }
    const int kmax = tm.max_substates < 2 ? 2 : tm.max_substates;
    // every slot carries its term's sub-state capacity (bits 16.. of slot_sub3: it fixes the LinSpaced grid the slot's sub-state
    // index refers to), so terms with different max_substates coexist
    if (kmax > 0x7FFF)
    {
      err = "collision: max_substates too large";
      return TMX_ERR_UNSUPPORTED;
    }
    L.lvs_kmax = std::max(L.lvs_kmax, kmax);
    const bool cast = tm.evaluator_type != 2, is_cnt_c = tm.kind == TMX_TERM_COLLISION_CNT;
    for (int i = tm.first_step; i < tm.last_step; ++i)
    {
      const bool cur = std::find(tm.fixed_steps, tm.fixed_steps + tm.n_fixed_steps, i) != tm.fixed_steps + tm.n_fixed_steps;
      const bool nxt = std::find(tm.fixed_steps, tm.fixed_steps + tm.n_fixed_steps, i + 1) != tm.fixed_steps + tm.n_fixed_steps;
      const int fl = (cur ? 1 : 0) | ((!cur && nxt) ? 2 : 0) | (cast ? 4 : 0);
      const int own = is_cnt_c ? L.n_cnts++ : L.n_costs++;
      const int nsub = cast ? kmax - 1 : kmax;
      for (int sp = 0; sp < d->n_link_spheres; ++sp)
        for (int o = 0; o < d->n_obstacles; ++o)
          for (int q = 0; q < nsub; ++q)
          {
            add_slot(SLOT_COLLISION_LVS, i, sp, o, own, 1, is_cnt_c ? 1 : 0, 0, tm.coeff, is_cnt_c ? tm.coeff : 1.0, tm.margin, tm.buffer);
            L.c2.back() = L.R2++;
            L.sub3.back() = fl | (q << 3) | (kmax << 16);
            L.aux3.back() = tm.longest_valid_segment_length;
          }
    }
    return TMX_OK;
#endif
  };
  const int flavor = d->flavor;
  if (flavor != TMX_FLAVOR_SCO && flavor != TMX_FLAVOR_SQP)
  {
    err = "tmx_problem_desc.flavor must be TMX_FLAVOR_SCO or TMX_FLAVOR_SQP";
    return TMX_ERR_INVALID;
  }
  if (flavor == TMX_FLAVOR_SQP && (d->n_fixed_steps > 0 || d->n_fixed_dofs > 0))
  {
    err = "TMX_FLAVOR_SQP: fixed_steps / fixed_dofs are not part of the trajopt_sqp path (use JointPos constraint sets)";
    return TMX_ERR_UNSUPPORTED;
  }
#if !TMX_LINK_ROWS
  if (flavor == TMX_FLAVOR_SQP)
  {
    err = "TMX_FLAVOR_SQP needs a build with pair rows";
    return TMX_ERR_UNSUPPORTED;
  }
#endif
  if (flavor == TMX_FLAVOR_SQP && d->use_time)
  {
    err = "TMX_FLAVOR_SQP: time-parameterised problems are not part of the trajopt_sqp path (trajopt_ifopt has no such sets)";
    return TMX_ERR_UNSUPPORTED;
  }
  P.flavor = flavor;
  std::vector<int> fixed(d->fixed_steps, d->fixed_steps + d->n_fixed_steps);
  for (int t : fixed)
  {
    if (t < 0 || t >= T)
    {
      err = "fixed timestep out of range";
      return TMX_ERR_INVALID;
    }
    for (int j = 0; j < DK; ++j)  // (the joint columns only, problem_description.cpp:499-503)
      add_slot(SLOT_FIXED, t, j, 0, -1, 0, 0, 1, 0.0, 1.0, 0.0, 0.0);
  }
  // BasicInfo::fixed_dofs (problem_description.cpp:510-530): the joint keeps its initial value at every timestep that is not
  // already a fixed timestep
  for (int q = 0; q < d->n_fixed_dofs; ++q)
  {
    const int dof = d->fixed_dofs[q];
    if (dof < 0 || dof >= DK)
    {
      err = "DOF(aka Joint) indice is greater than the number of DOF available.";
      return TMX_ERR_INVALID;
    }
    for (int i = 0; i < T; ++i)
      if (std::find(fixed.begin(), fixed.end(), i) == fixed.end())
        add_slot(SLOT_FIXED, i, dof, 0, -1, 0, 0, 1, 0.0, 1.0, 0.0, 0.0);
  }
  for (std::vector<double>* v : { &L.pd, &L.po, &L.pq, &L.po2, &L.po3 })
    v->assign(P.NX, 0.0);
  // hatch order: all costs in list order, then the constraints; sco::OptProb keeps equality constraints in front of the
  // inequality constraints (modeling.cpp:234-241), which fixes both the row / aux order and the constraint numbering
  auto time_zero_tols = [](const tmx_term& tm, int nj) {
    bool z = true;
    for (int j = 0; j < nj; ++j)
      z = z && std::fabs(tm.upper_tols[j]) < 1e-5 && std::fabs(tm.lower_tols[j]) < 1e-5;  // trajopt_common::doubleEquals (vector_ops.hpp:17)
    return z;
  };
  L.term_cp0.assign((size_t)d->n_terms, 0);
  L.term_cp1.assign((size_t)d->n_terms, 0);
  L.term_slot0.assign((size_t)d->n_terms, 0);
  L.term_slot1.assign((size_t)d->n_terms, 0);
  for (int pass = 0; pass < 5; ++pass)
    for (int k = 0; k < d->n_terms; ++k)
    {
      const tmx_term& tm = d->terms[k];
      const bool is_ineq = tm.kind == TMX_TERM_JOINT_POS_INEQ_CNT || tm.kind == TMX_TERM_COLLISION_CNT || tm.kind == TMX_TERM_JOINT_VEL_INEQ_CNT ||
                           tm.kind == TMX_TERM_JOINT_ACC_INEQ_CNT || tm.kind == TMX_TERM_JOINT_JERK_INEQ_CNT ||
                           (tm.kind == TMX_TERM_FUNC_CNT && tm.cnt_type == 1) || (tm.kind == TMX_TERM_CART_VEL && tm.is_constraint) ||
                           (tm.kind == TMX_TERM_AVOID_SINGULARITY && tm.is_constraint) ||
                           (tm.kind == TMX_TERM_JOINT_VEL_TIME && tm.is_constraint && !time_zero_tols(tm, DK)) ||
                           (tm.kind == TMX_TERM_TOTAL_TIME && tm.is_constraint && !(std::fabs(tm.margin) < 1e-5));
      const bool is_cnt = is_ineq || (tm.kind == TMX_TERM_JOINT_POS_EQ_CNT) || (tm.kind == TMX_TERM_JOINT_VEL_EQ_CNT) ||
                          (tm.kind == TMX_TERM_JOINT_ACC_EQ_CNT) || (tm.kind == TMX_TERM_JOINT_JERK_EQ_CNT) || (tm.kind == TMX_TERM_FUNC_CNT) ||
                          (tm.kind == TMX_TERM_CART_POSE && tm.is_constraint) || (tm.kind == TMX_TERM_DYN_CART_POSE && tm.is_constraint) ||
                          ((tm.kind == TMX_TERM_JOINT_VEL_TIME || tm.kind == TMX_TERM_TOTAL_TIME) && tm.is_constraint);
      int want = !is_cnt ? 0 : (is_ineq ? 2 : 1);
      if (flavor == TMX_FLAVOR_SQP)
      {
        // TrajOptQPProblem::setup (trajopt_qp_problem.cpp:568-600): objective terms (squared), penalty constraints = hinge costs
        // (static, dynamic) then abs costs, merit constraints = static constraint sets then the dynamic ones
        switch (tm.kind)
        {
          case TMX_TERM_JOINT_VEL_COST:
          case TMX_TERM_JOINT_ACC_EQ_COST:
          case TMX_TERM_JOINT_JERK_EQ_COST:
            want = 0;
            break;
          case TMX_TERM_COLLISION_COST:
            want = 1;
            break;
          case TMX_TERM_JOINT_POS_EQ_COST:
            want = 2;
            break;
          case TMX_TERM_JOINT_POS_EQ_CNT:
            want = 3;
            break;
          case TMX_TERM_CART_POSE:  // trajopt_ifopt::CartPosConstraint as a (static) constraint set, round 5
            if (!tm.is_constraint)
            {
              err = "TMX_FLAVOR_SQP: cart_pose is lowered as a constraint set (CartPosConstraint) only";
              return TMX_ERR_UNSUPPORTED;
            }
            want = 3;
            break;
          case TMX_TERM_COLLISION_CNT:
            want = 4;
            break;
          default:
            err = "TMX_FLAVOR_SQP: this term kind is not lowered for the trajopt_sqp flavour (lowered: JointPosConstraint as constraint / "
                       "absolute cost, JointVel / JointAccel / JointJerk constraint sets as squared costs, CartPosConstraint as constraint, the "
                       "segment collision sets as hinge cost / constraint); not part of the trajopt_sqp path as built here";
            return TMX_ERR_UNSUPPORTED;
        }
        if ((tm.kind == TMX_TERM_COLLISION_COST || tm.kind == TMX_TERM_COLLISION_CNT) && tm.evaluator_type < 2)
        {
          err = "TMX_FLAVOR_SQP lowers the segment collision evaluators (evaluator_type 2..4) only";
          return TMX_ERR_UNSUPPORTED;
        }
      }
      if (pass != want)
        continue;
      if (tm.kind != TMX_TERM_TOTAL_TIME && (tm.first_step < 0 || tm.last_step >= T || tm.first_step > tm.last_step))
      {
        err = "term step range invalid";
        return TMX_ERR_INVALID;
      }
      if (tm.n_fixed_steps < 0 || (tm.n_fixed_steps > 0 && tm.fixed_steps == nullptr) ||
          (tm.n_fixed_steps > 0 && tm.kind != TMX_TERM_COLLISION_COST && tm.kind != TMX_TERM_COLLISION_CNT && tm.kind != TMX_TERM_FUNC_COST &&
           tm.kind != TMX_TERM_FUNC_CNT && tm.kind != TMX_TERM_FUNC_ERR_COST))
      {
        err = "tmx_term.fixed_steps: only collision and function terms carry fixed steps";
        return TMX_ERR_INVALID;
      }
      for (int q = 0; q < tm.n_fixed_steps; ++q)
        if (tm.fixed_steps[q] < tm.first_step || tm.fixed_steps[q] > tm.last_step)
        {
          err = "Fixed step is not between first step and last step";  // problem_description.cpp:1641-1649
          return TMX_ERR_INVALID;
        }
      // CartPose / DynamicCartPose with a tolerance band (CartPoseErrCalculator, kinematic_terms.cpp:206-247: toleranced unless the
      // vectors are empty or lower == upper): the band is applied to the six error rows before the row selection
      bool pose_tol = false;
      if (tm.kind == TMX_TERM_CART_POSE || tm.kind == TMX_TERM_DYN_CART_POSE)
        for (int i = 0; i < 6; ++i)
        {
          if (tm.lower_tols[i] > tm.upper_tols[i])
          {
            err = "CartPoseErrCalculator: Inverted tolerance band - lower > upper at one or more indices";  // kinematic_terms.cpp:47-54
            return TMX_ERR_INVALID;
          }
          pose_tol = pose_tol || std::fabs(tm.lower_tols[i] - tm.upper_tols[i]) > 1e-6;
        }
      const int kind_eff = (tm.kind == TMX_TERM_CART_POSE && pose_tol) ? TMX_TERM_DYN_CART_POSE : tm.kind;
      L.term_cp0[(size_t)k] = (int)L.cp_t.size();
      L.term_slot0[(size_t)k] = (int)L.kind.size();
      switch (kind_eff)
      {
        case TMX_TERM_JOINT_VEL_COST:
        {
          if (tm.last_step - 1 - tm.first_step < 0)
          {
            err = "JointVelEqCost, trajectory is too short!";  // trajectory_costs.cpp:269-270
            return TMX_ERR_INVALID;
          }
          L.vel_first.push_back(tm.first_step);
          L.vel_last.push_back(tm.last_step);
          L.vel_kind.push_back(0);
          L.vel_cost.push_back(L.n_costs++);
          for (int j = 0; j < TMX_MAX_DOF; ++j)
          {
            L.vel_coeffs.push_back(j < DK ? tm.coeffs[j] : 0.0);
            L.vel_targets.push_back(j < DK ? tm.targets[j] : 0.0);
          }
          if (flavor == TMX_FLAVOR_SQP)
          {
            // JointVelConstraint as a kSquared cost set: H = Bw' Bw with Bw = diag(sqrt(w)) B, B rows (-1 at x[i][j], +1 at
            // x[i+1][j]) accumulated over the rows in row order (AffExprs::square, expressions.cpp:43-112); the 1e-7 zeroing and
            // the factor 2 of OSQPEigenSolver::updateHessianMatrix are applied after all sets are summed (below)
            ++L.n_sq;
            for (int j = 0; j < DK; ++j)
              if (!(tm.coeffs[j] > 0))
              {
                err = "JointVelConstraint, coeff must be greater than zero.";  // joint_velocity_constraint.cpp:66
                return TMX_ERR_INVALID;
              }
            for (int i = tm.first_step; i <= tm.last_step - 1; ++i)
              for (int j = 0; j < DK; ++j)
              {
                const double sw = std::sqrt(tm.coeffs[j]);
                const double b0 = -1 * sw, b1 = 1 * sw;
                L.pd[i * D + j] += b0 * b0;
                L.po[i * D + j] += b0 * b1;
                L.pd[(i + 1) * D + j] += b1 * b1;
              }
            break;
          }
          // Hessian / linear term of sum_j c_j (x_{i+1,j} - x_{i,j} - targ_j)^2 exactly as exprSquare + exprToEigen build
          // them (expr_ops.cpp:55-84, solver_utils.cpp:49-109 with matrix_is_halved = true)
          for (int i = tm.first_step; i <= tm.last_step - 1; ++i)
            for (int j = 0; j < DK; ++j)
            {
              const double c = tm.coeffs[j];
              const double a0 = -1.0, a1 = 1.0, cst = 0.0 - tm.targets[j];
              const double q00 = (a0 * a0) * c, q01 = (2 * a0 * a1) * c, q11 = (a1 * a1) * c;
              if (q00 != 0.0)
                L.pd[i * D + j] += 2.0 * q00;
              if (q11 != 0.0)
                L.pd[(i + 1) * D + j] += 2.0 * q11;
              if (q01 != 0.0)
                L.po[i * D + j] += q01;
              const double l0 = (2 * cst * a0) * c, l1 = (2 * cst * a1) * c;
              if (l0 != 0.0)
                L.pq[i * D + j] += l0;
              if (l1 != 0.0)
                L.pq[(i + 1) * D + j] += l1;
            }
          break;
        }
        case TMX_TERM_JOINT_POS_EQ_CNT:
        {
          if (flavor == TMX_FLAVOR_SQP)
          {
            // one JointPosConstraint set per step (joint_position_constraint.cpp:36-75): unscaled identity rows with equality
            // bounds; the coefficient weighs the slack pair in the objective (trajopt_qp_problem.cpp:799-812)
            for (int i = tm.first_step; i <= tm.last_step; ++i)
            {
              const int own = L.n_cnts++;
              for (int j = 0; j < DK; ++j)
              {
                if (!(tm.coeffs[j] > 0))
                {
                  err = "JointPosConstraint, coeff must be greater than zero.";
                  return TMX_ERR_INVALID;
                }
                add_slot(SLOT_JOINTPOS, i, j, 0, own, 2, 1, 1, 0.0, tm.coeffs[j], tm.targets[j], 0.0);
              }
            }
            break;
          }
          const int own = L.n_cnts++;
          for (int i = tm.first_step; i <= tm.last_step; ++i)
            for (int j = 0; j < DK; ++j)
              add_slot(SLOT_JOINTPOS, i, j, 0, own, 2, 1, 1, 0.0, tm.coeffs[j], tm.targets[j], 0.0);
          break;
        }
        case TMX_TERM_JOINT_VEL_EQ_CNT:
        case TMX_TERM_JOINT_VEL_INEQ_COST:
        case TMX_TERM_JOINT_VEL_INEQ_CNT:
        {
#if !TMX_LINK_ROWS
          err = "rows on two consecutive waypoints (JointVel constraint / hinge forms) are not enabled in this build";
          return TMX_ERR_UNSUPPORTED;
#else
          if (tm.last_step - 1 - tm.first_step < 0)
          {
            err = "JointVel term, trajectory is too short!";  // trajectory_costs.cpp:320, :390, :444
            return TMX_ERR_INVALID;
          }
          // one row (EQ) or an upper and a lower row (INEQ) per step i in [first, last - 1] and joint j, in the order of the
          // reference's expr_vec_ (trajectory_costs.cpp:322-346, 392-400, 446-470): home coefficient on x[i][j], link on x[i+1][j]
          const bool is_cnt = tm.kind != TMX_TERM_JOINT_VEL_INEQ_COST;
          const int own = is_cnt ? L.n_cnts++ : L.n_costs++;
          for (int i = tm.first_step; i <= tm.last_step - 1; ++i)
            for (int j = 0; j < DK; ++j)
            {
              const double c = tm.coeffs[j];
              if (tm.kind == TMX_TERM_JOINT_VEL_EQ_CNT)
              {
                add_slot(SLOT_JOINTVEL, i, j, 0, own, 2, 1, 1, 0.0, c, tm.targets[j], 0.0);
                L.c2.back() = L.R2++;
              }
              else
              {
                add_slot(SLOT_JOINTVEL_INEQ, i, j, 0, own, 1, is_cnt ? 1 : 0, 0, is_cnt ? 0.0 : 1.0, c, tm.targets[j], tm.upper_tols[j]);
                L.c2.back() = L.R2++;
                add_slot(SLOT_JOINTVEL_INEQ, i, j, 1, own, 1, is_cnt ? 1 : 0, 0, is_cnt ? 0.0 : 1.0, c, tm.targets[j], tm.lower_tols[j]);
                L.c2.back() = L.R2++;
              }
            }
          break;
#endif
        }
        case TMX_TERM_FUNC_COST:
        case TMX_TERM_FUNC_CNT:
        case TMX_TERM_FUNC_ERR_COST:
        case TMX_TERM_AVOID_SINGULARITY:
        case TMX_TERM_DYN_CART_POSE:
        {
          // sco::CostFromFunc / sco::ConstraintFromErrFunc over a tmx_expr program of the waypoint's variables: one cost /
          // constraint per step (include/tmx.h).  The cost model is a dynamic quadratic: dense QP engine.
          // AvoidSingularity / DynamicCartPose: the same Cost / ConstraintFromErrFunc rows over a BUILT-IN kinematic function
          // with its own Jacobian (fx_nops < 0: -1 / -2, fx_op0 = link, parameters in the constants; tmx_terms.h).
          const bool pose = tm.kind == TMX_TERM_DYN_CART_POSE || tm.kind == TMX_TERM_CART_POSE;  // (a static target only with tolerances)
          const bool builtin = tm.kind == TMX_TERM_AVOID_SINGULARITY || pose;
          if (flavor == TMX_FLAVOR_SQP)
          {
            err = "TMX_FLAVOR_SQP: function terms are not part of the trajopt_sqp path";
            return TMX_ERR_UNSUPPORTED;
          }
          // (time-parameterised problems: user-defined functions see the joint columns of their waypoint, prob.GetVarRow(s, 0, n_dof) -
          //  round 5; the built-in kinematic functions likewise since round 6: the time column is a prismatic joint with a zero axis
          //  for the FK, a zero Jacobian column, and no column of the Jacobian AvoidSingularity decomposes - tmx_terms.h)
          if (!builtin && tmx_expr_check(tm.expr, DK) != 0)
          {
            err = "function term: malformed tmx_expr program (opcode, index, stack discipline or outputs)";
            return TMX_ERR_INVALID;
          }
          if (builtin && tm.kind != TMX_TERM_CART_POSE && (tm.link < 0 || tm.link >= DK))
          {
            err = "AvoidSingularity / DynamicCartPose: link is the index of a moving link, 0 .. n_dof - 1";
            return TMX_ERR_INVALID;
          }
          const bool is_cnt = builtin ? tm.is_constraint != 0 : tm.kind == TMX_TERM_FUNC_CNT;
          // AvoidSingularity: ABS cost / INEQ constraint (problem_description.cpp:1925-1934); DynamicCartPose: ABS cost / EQ
          // constraint (:808-816)
          const int cnt_type = tm.kind == TMX_TERM_AVOID_SINGULARITY ? 1 : (pose ? 0 : tm.cnt_type);
          const int penalty_type = builtin ? 1 : tm.penalty_type;
          double weights[TMX_EXPR_MAX_OUT];
          int n_out = builtin ? 0 : tm.expr->n_outputs;
          bool has_coeffs = builtin ? true : tm.has_coeffs != 0;
          for (int i = 0; i < TMX_EXPR_MAX_OUT; ++i)
            weights[i] = (!builtin && tm.has_coeffs && i < n_out) ? tm.coeffs[i] : 1.0;
          int pose_idx[6] = { 0, 0, 0, 0, 0, 0 };
          if (tm.kind == TMX_TERM_AVOID_SINGULARITY)
          {
            n_out = 1;
            weights[0] = tm.coeffs[0];
          }
          else if (pose)
            for (int i = 0; i < 6; ++i)  // rows with |coeff| <= 1e-5 are dropped (problem_description.cpp:756-775)
              if (std::fabs(tm.coeffs[i]) > 1e-5)
              {
                pose_idx[n_out] = i;
                weights[n_out++] = tm.coeffs[i];
              }
          if (tm.kind == TMX_TERM_FUNC_COST && n_out != 1)
          {
            err = "TMX_TERM_FUNC_COST: the program of a cost has one output";
            return TMX_ERR_INVALID;
          }
          if (is_cnt && cnt_type != 0 && cnt_type != 1)
          {
            err = "TMX_TERM_FUNC_CNT: cnt_type must be 0 (EQ) or 1 (INEQ)";
            return TMX_ERR_INVALID;
          }
          if (tm.kind == TMX_TERM_FUNC_ERR_COST && (penalty_type < 0 || penalty_type > 2))
          {
            err = "TMX_TERM_FUNC_ERR_COST: penalty_type must be 0 (SQUARED), 1 (ABS) or 2 (HINGE)";
            return TMX_ERR_INVALID;
          }
          // instance kind: 0 / 1 CostFromFunc (diagonal / full Hessian), 2 constraint rows, 3 squared error cost, 4 abs / hinge cost rows
          const int fk = tm.kind == TMX_TERM_FUNC_COST ? (tm.full_hessian ? 1 : 0) : (is_cnt ? 2 : (penalty_type == 0 ? 3 : 4));
          const bool quad = fk == 0 || fk == 1 || fk == 3;
          L.st_terms = true;
          if (quad)
            L.dyn_p = true;  // P changes with the iterate, but only inside the waypoint's diagonal block: QpWs::pb (row-only function terms leave the QP as it is)
          // the row weights (coeffs, 1 when absent) sit in front of the program's constants
          for (int i = 0; i < TMX_EXPR_MAX_OUT; ++i)
            L.fx_consts.push_back(weights[i]);
          int op0 = (int)L.fx_ops.size() / 2, n_ops = 0;
          const int c0 = (int)L.fx_consts.size();
          if (!builtin)
          {
            n_ops = tm.expr->n_ops;
            L.fx_ops.insert(L.fx_ops.end(), tm.expr->ops, tm.expr->ops + 2 * tm.expr->n_ops);
            L.fx_consts.insert(L.fx_consts.end(), tm.expr->consts, tm.expr->consts + tm.expr->n_consts);
          }
          else if (tm.kind == TMX_TERM_AVOID_SINGULARITY)
          {
            if (tm.subset_first < 0 || tm.subset_first > tm.link + 1)
            {
              err = "AvoidSingularity: subset_first is 0 (all joints) or 1 + the first joint of a subset that ends at `link`";
              return TMX_ERR_INVALID;
            }
            op0 = tm.link;
            n_ops = -1;
            L.fx_consts.push_back(tm.lambda);
            L.fx_consts.push_back((double)tm.subset_first);
          }
          else
          {
            op0 = tm.kind == TMX_TERM_CART_POSE ? -1 : tm.link;  // -1: the frame is world_T_target itself
            n_ops = -2;
            L.fx_consts.insert(L.fx_consts.end(), tm.target_pose, tm.target_pose + 12);  // link_T_target (world_T_target)
            for (int i = 0; i < 6; ++i)
              L.fx_consts.push_back((double)pose_idx[i]);
            L.fx_consts.push_back(pose_tol ? 1.0 : 0.0);
            L.fx_consts.insert(L.fx_consts.end(), tm.lower_tols, tm.lower_tols + 6);
            L.fx_consts.insert(L.fx_consts.end(), tm.upper_tols, tm.upper_tols + 6);
          }
          for (int t = tm.first_step; t <= tm.last_step; ++t)
          {
            if (!builtin && std::find(tm.fixed_steps, tm.fixed_steps + tm.n_fixed_steps, t) != tm.fixed_steps + tm.n_fixed_steps)
              continue;  // UserDefinedTermInfo::fixed_steps (problem_description.cpp:608, :645)
            const int inst = (int)L.fx_t.size();
            const int own = is_cnt ? L.n_cnts++ : L.n_costs++;
            L.fx_t.push_back(t);
            L.fx_kind.push_back(fk);
            L.fx_owner.push_back(own);
            L.fx_op0.push_back(op0);
            L.fx_nops.push_back(n_ops);
            L.fx_c0.push_back(c0);
            L.fx_nout.push_back(n_out);
            L.fx_slot0.push_back((int)L.kind.size());
            L.fx_ci.push_back(quad ? L.n_fx_cost++ : -1);
            if (!quad)
              for (int i = 0; i < n_out; ++i)
              {
                const double cc = has_coeffs ? weights[i] : 1.0;
                if (has_coeffs && cc == 0)
                  continue;  // modeling_utils.cpp:175-176, :258-259
                if (is_cnt)
                  add_slot(SLOT_FUNC, t, i, inst, own, cnt_type == 0 ? 2 : 1, 1, cnt_type == 0 ? 1 : 0, 0.0, cc, 0.0, 0.0);
                else  // ABS: exprScale(aff, weight); addAbs(aff, 1) -> two aux with objective 1; HINGE: one aux
                  add_slot(SLOT_FUNC, t, i, inst, own, penalty_type == 1 ? 2 : 1, 0, penalty_type == 1 ? 1 : 0, 1.0, cc, 0.0, 0.0);
              }
          }
          break;
        }
        case TMX_TERM_JOINT_ACC_EQ_COST:
        case TMX_TERM_JOINT_JERK_EQ_COST:
        {
          // JointAccEqCost / JointJerkEqCost (trajectory_costs.cpp:502-552, :756-809): sum_ij c_j (stencil . x[i..i+ord][j] - targ_j)^2
          // built once as a QuadExpr; Hessian / linear term exactly as exprSquare + exprToEigen build them (expr_ops.cpp:55-84,
          // solver_utils.cpp:49-109 with matrix_is_halved = true): diagonal 2 a_k^2 c, off-diagonal (2 a_k a_l) c, linear (2 cst a_k) c
          const int ord = tm.kind == TMX_TERM_JOINT_ACC_EQ_COST ? 2 : 3;
          if (!TMX_LINK_ROWS)
          {
            err = "rows on several waypoints (joint acceleration / jerk terms) are not enabled in this build";
            return TMX_ERR_UNSUPPORTED;
          }
          if (flavor == TMX_FLAVOR_SQP)
          {
            // trajopt_ifopt::JointAccelConstraint / JointJerkConstraint over the steps of the term as a kSquared cost set (round 5; the use
            // joint_acceleration_optimization_unit.cpp:110 / joint_jerk_optimization_unit.cpp:111 make of them): n rows per joint, the
            // last `ord` of them backward stencils (joint_acceleration_constraint.cpp:90-175, joint_jerk_constraint.cpp:90-180).
            // H = Bw' Bw with Bw = diag(sqrt(w)) B accumulated in row order (AffExprs::square, expressions.cpp:43-112), like the
            // JointVelConstraint set above; the 1e-7 zeroing and the factor 2 are applied after all sets are summed.
            const int n = tm.last_step - tm.first_step + 1;
            if (n < (ord == 2 ? 4 : 6))
            {
              err = ord == 2 ? "JointAccelConstraint requires a minimum of four position variables!"   // joint_acceleration_constraint.cpp:45-46
                                  : "JointJerkConstraint requires a minimum of six position variables!";    // joint_jerk_constraint.cpp:45-46
              return TMX_ERR_INVALID;
            }
            for (int j = 0; j < DK; ++j)
              if (!(tm.coeffs[j] > 0))
              {
                err = ord == 2 ? "JointAccelConstraint, coeff must be greater than zero." : "JointJerkConstraint, coeff must be greater than zero.";
                return TMX_ERR_INVALID;
              }
            ++L.n_sq;
            L.band = std::max(L.band, ord);
            L.st_terms = true;  // (the squared-set code of these kinds is instantiated in the piecewise kernels)
            L.vel_first.push_back(tm.first_step);
            L.vel_last.push_back(tm.last_step);
            L.vel_kind.push_back(ord + 2);  // 4: ifopt accel, 5: ifopt jerk (tmx_terms.h: vel_is_ifopt_kind)
            L.vel_cost.push_back(L.n_costs++);
            for (int j = 0; j < TMX_MAX_DOF; ++j)
            {
              L.vel_coeffs.push_back(j < DK ? tm.coeffs[j] : 0.0);
              L.vel_targets.push_back(j < DK ? tm.targets[j] : 0.0);
            }
            static const double E2[3] = { 1.0, -2.0, 1.0 }, E3[4] = { -1.0, 3.0, -3.0, 1.0 };
            const double* e = ord == 2 ? E2 : E3;
            for (int i = 0; i < n; ++i)
            {
              const int a0 = tm.first_step + ((i < n - ord) ? i : i - ord);
              for (int j = 0; j < DK; ++j)
              {
                const double sw = std::sqrt(tm.coeffs[j]);
                for (int k = 0; k <= ord; ++k)
                {
                  const double bk = e[k] * sw;
                  L.pd[(a0 + k) * D + j] += bk * bk;
                  for (int l = k + 1; l <= ord; ++l)
                  {
                    std::vector<double>& bnd = (l - k == 1) ? L.po : ((l - k == 2) ? L.po2 : L.po3);
                    bnd[(a0 + k) * D + j] += bk * (e[l] * sw);
                  }
                }
              }
            }
            break;
          }
          if (tm.last_step - ord - tm.first_step < 0)
          {
            err = ord == 2 ? "JointAccEqCost, trajectory is too short!" : "JointJerkEqCost, trajectory is too short!";  // :515, :768
            return TMX_ERR_INVALID;
          }
          L.band = std::max(L.band, ord);
          L.vel_first.push_back(tm.first_step);
          L.vel_last.push_back(tm.last_step);
          L.vel_kind.push_back(ord);
          L.vel_cost.push_back(L.n_costs++);
          for (int j = 0; j < TMX_MAX_DOF; ++j)
          {
            L.vel_coeffs.push_back(j < DK ? tm.coeffs[j] : 0.0);
            L.vel_targets.push_back(j < DK ? tm.targets[j] : 0.0);
          }
          static const double S2[3] = { 1.0, -2.0, 1.0 }, S3[4] = { -1.0, 3.0, -3.0, 1.0 };
          const double* a = ord == 2 ? S2 : S3;
          for (int i = tm.first_step; i <= tm.last_step - ord; ++i)
            for (int j = 0; j < DK; ++j)
            {
              const double c = tm.coeffs[j], cst = 0.0 - tm.targets[j];
              for (int k = 0; k <= ord; ++k)
              {
                const double qkk = (a[k] * a[k]) * c;
                if (qkk != 0.0)
                  L.pd[(i + k) * D + j] += 2.0 * qkk;
                const double lk = (2 * cst * a[k]) * c;
                if (lk != 0.0)
                  L.pq[(i + k) * D + j] += lk;
                for (int l = k + 1; l <= ord; ++l)
                {
                  const double qkl = (2 * a[k] * a[l]) * c;
                  if (qkl == 0.0)
                    continue;
                  std::vector<double>& bnd = (l - k == 1) ? L.po : ((l - k == 2) ? L.po2 : L.po3);
                  bnd[(i + k) * D + j] += qkl;
                }
              }
            }
          break;
        }
        case TMX_TERM_JOINT_ACC_EQ_CNT:
        case TMX_TERM_JOINT_ACC_INEQ_COST:
        case TMX_TERM_JOINT_ACC_INEQ_CNT:
        case TMX_TERM_JOINT_JERK_EQ_CNT:
        case TMX_TERM_JOINT_JERK_INEQ_COST:
        case TMX_TERM_JOINT_JERK_INEQ_CNT:
        {
#if !TMX_LINK_ROWS
          err = "rows on several waypoints (joint acceleration / jerk terms) are not enabled in this build";
          return TMX_ERR_UNSUPPORTED;
#else
          const bool acc = tm.kind == TMX_TERM_JOINT_ACC_EQ_CNT || tm.kind == TMX_TERM_JOINT_ACC_INEQ_COST || tm.kind == TMX_TERM_JOINT_ACC_INEQ_CNT;
          const int ord = acc ? 2 : 3;
          const bool is_eq = tm.kind == TMX_TERM_JOINT_ACC_EQ_CNT || tm.kind == TMX_TERM_JOINT_JERK_EQ_CNT;
          const bool is_cost = tm.kind == TMX_TERM_JOINT_ACC_INEQ_COST || tm.kind == TMX_TERM_JOINT_JERK_INEQ_COST;
          if (flavor == TMX_FLAVOR_SQP)
          {
            err = "TMX_FLAVOR_SQP: the ROW forms of the joint acceleration / jerk terms are not lowered for the trajopt_sqp flavour (their "
                       "squared cost sets are); not part of the trajopt_sqp path as built here";
            return TMX_ERR_UNSUPPORTED;
          }
          if (tm.last_step - ord - tm.first_step < 0)
          {
            err = acc ? "JointAcc term, trajectory is too short!" : "JointJerk term, trajectory is too short!";  // :575, :642, :699, ...
            return TMX_ERR_INVALID;
          }
          L.stencil_rows = true;  // (structured banded path or dense engine: decided below, when every term is known)
          L.max_row_order = std::max(L.max_row_order, ord);
          // rows in the order of the reference's expr_vec_ (:577-601, :644-652, :703-727 and the jerk twins): one row (EQ) or an
          // upper and a lower row (INEQ) per step i in [first, last - ord] and joint j over x[i .. i + ord][j]
          const int own = is_cost ? L.n_costs++ : L.n_cnts++;
          for (int i = tm.first_step; i <= tm.last_step - ord; ++i)
            for (int j = 0; j < DK; ++j)
            {
              const double c = tm.coeffs[j];
              if (is_eq)
              {
                add_slot(SLOT_JOINTVEL, i, j, 0, own, 2, 1, 1, 0.0, c, tm.targets[j], 0.0);
                L.c2.back() = L.R2++;
                L.sub3.back() = ord;
                ++L.n_stencil;
              }
              else
              {
                add_slot(SLOT_JOINTVEL_INEQ, i, j, 0, own, 1, is_cost ? 0 : 1, 0, is_cost ? 1.0 : 0.0, c, tm.targets[j], tm.upper_tols[j]);
                L.c2.back() = L.R2++;
                L.sub3.back() = ord;
                add_slot(SLOT_JOINTVEL_INEQ, i, j, 1, own, 1, is_cost ? 0 : 1, 0, is_cost ? 1.0 : 0.0, c, tm.targets[j], tm.lower_tols[j]);
                L.c2.back() = L.R2++;
                L.sub3.back() = ord;
                L.n_stencil += 2;
              }
            }
          break;
#endif
        }
        case TMX_TERM_JOINT_POS_EQ_COST:
        {
          if (flavor == TMX_FLAVOR_SQP)
          {
            // JointPosConstraint per step as a kAbsolute cost set: the same rows, slack pair weighted by the coefficient
            for (int i = tm.first_step; i <= tm.last_step; ++i)
            {
              const int own = L.n_costs++;
              for (int j = 0; j < DK; ++j)
              {
                if (!(tm.coeffs[j] > 0))
                {
                  err = "JointPosConstraint, coeff must be greater than zero.";
                  return TMX_ERR_INVALID;
                }
                add_slot(SLOT_JOINTPOS, i, j, 0, own, 2, 0, 1, tm.coeffs[j], tm.coeffs[j], tm.targets[j], 0.0);
              }
            }
            break;
          }
          // JointPosEqCost (trajectory_costs.cpp:28-65): squared cost on the joint positions; shares the device-side
          // machinery of the velocity cost (vel_kind 1: the term is x_ij - target_j instead of a difference of steps)
          L.vel_first.push_back(tm.first_step);
          L.vel_last.push_back(tm.last_step);
          L.vel_kind.push_back(1);
          L.vel_cost.push_back(L.n_costs++);
          for (int j = 0; j < TMX_MAX_DOF; ++j)
          {
            L.vel_coeffs.push_back(j < DK ? tm.coeffs[j] : 0.0);
            L.vel_targets.push_back(j < DK ? tm.targets[j] : 0.0);
          }
          // exprSquare(pos) * coeff with pos = 1*x - target  ->  Hessian 2*c on the diagonal, linear term 2*(0 - target)*c
          for (int i = tm.first_step; i <= tm.last_step; ++i)
            for (int j = 0; j < DK; ++j)
            {
              const double c = tm.coeffs[j];
              const double a1 = 1.0, cst = 0.0 - tm.targets[j];
              const double q11 = (a1 * a1) * c;
              if (q11 != 0.0)
                L.pd[i * D + j] += 2.0 * q11;
              const double l1 = (2 * cst * a1) * c;
              if (l1 != 0.0)
                L.pq[i * D + j] += l1;
            }
          break;
        }
        case TMX_TERM_JOINT_POS_INEQ_COST:
        {
          // JointPosIneqCost (trajectory_costs.cpp:67-137): the rows of the inequality constraint as hinge costs with
          // objective coefficient 1 (the per-joint coefficient already sits inside the affine expression)
          const int own = L.n_costs++;
          for (int i = tm.first_step; i <= tm.last_step; ++i)
            for (int j = 0; j < DK; ++j)
            {
              add_slot(SLOT_JOINTPOS_INEQ, i, j, 0, own, 1, 0, 0, 1.0, tm.coeffs[j], tm.targets[j], tm.upper_tols[j]);
              add_slot(SLOT_JOINTPOS_INEQ, i, j, 1, own, 1, 0, 0, 1.0, tm.coeffs[j], tm.targets[j], tm.lower_tols[j]);
            }
          break;
        }
        case TMX_TERM_JOINT_POS_INEQ_CNT:
        {
          // JointPosIneqConstraint (trajectory_costs.cpp:185-225): per step and joint an upper and a lower row, each an
          // inequality constraint -> hinge penalty (1 aux).  scale = coeff, aux1 = target, aux2 = tolerance
          const int own = L.n_cnts++;
          for (int i = tm.first_step; i <= tm.last_step; ++i)
            for (int j = 0; j < DK; ++j)
            {
              add_slot(SLOT_JOINTPOS_INEQ, i, j, 0, own, 1, 1, 0, 0.0, tm.coeffs[j], tm.targets[j], tm.upper_tols[j]);
              add_slot(SLOT_JOINTPOS_INEQ, i, j, 1, own, 1, 1, 0, 0.0, tm.coeffs[j], tm.targets[j], tm.lower_tols[j]);
            }
          break;
        }
        case TMX_TERM_CART_POSE:
        {
          for (int t = tm.first_step; t <= tm.last_step; ++t)
          {
            const int own = tm.is_constraint ? L.n_cnts++ : L.n_costs++;
            const int inst = static_cast<int>(L.cp_t.size());
            L.cp_t.push_back(t);
            L.cp_owner.push_back(own);
            L.cp_iscnt.push_back(tm.is_constraint ? 1 : 0);
            L.cp_slot0.push_back(static_cast<int>(L.kind.size()));
            int nr = 0;
            for (int i = 0; i < 6; ++i)
            {
              // problem_description.cpp:910-926; trajopt_ifopt::CartPosConstraint drops the rows whose coefficient is
              // almostEqualRelativeAndAbs(c, 0) (cartesian_position_constraint.cpp:95, :121)
              const bool keep = std::fabs(tm.coeffs[i]) > (flavor == TMX_FLAVOR_SQP ? 1e-6 : 1e-5);
              L.cp_idx.push_back(0);
              L.cp_coeff.push_back(0.0);
              if (keep)
              {
                L.cp_idx[inst * 6 + nr] = i;
                L.cp_coeff[inst * 6 + nr] = tm.coeffs[i];
                add_slot(SLOT_CARTPOSE, t, nr, i, own, 2, tm.is_constraint ? 1 : 0, 1, 1.0, tm.coeffs[i], 0.0, 0.0);
                ++nr;
              }
            }
            L.cp_nrows.push_back(nr);
            for (int q = 0; q < 12; ++q)
              L.cp_target.push_back(tm.target_pose[q]);
          }
          break;
        }
        case TMX_TERM_CART_VEL:
        {
#if !TMX_LINK_ROWS
          err = "rows on two consecutive waypoints (CartVel) are not enabled in this build";
          return TMX_ERR_UNSUPPORTED;
#else
          if (tm.last_step + 1 >= T)
          {
            err = "cart_vel: last_step + 1 must be a waypoint of the trajectory (the term couples steps i and i + 1)";
            return TMX_ERR_INVALID;
          }
          if (flavor == TMX_FLAVOR_SQP)
          {
            err = "TMX_FLAVOR_SQP: cart_vel is not part of the trajopt_sqp path";
            return TMX_ERR_UNSUPPORTED;
          }
          // CartVelTermInfo::hatch (problem_description.cpp:1011-1057): one cost / constraint per step i in [first, last] over
          // waypoints i and i + 1, six rows each
          for (int t = tm.first_step; t <= tm.last_step; ++t)
          {
            const int own = tm.is_constraint ? L.n_cnts++ : L.n_costs++;
            for (int i = 0; i < 6; ++i)
            {
              add_slot(SLOT_CARTVEL, t, i, 0, own, tm.is_constraint ? 1 : 2, tm.is_constraint ? 1 : 0, tm.is_constraint ? 0 : 1, 1.0, 1.0, tm.margin, 0.0);
              L.c2.back() = L.R2++;
            }
          }
          break;
#endif
        }
        case TMX_TERM_COLLISION_COST:
        {
          if (tm.evaluator_type < 0 || tm.evaluator_type > 4)
          {
            err = "collision evaluator_type must be <= 4";  // FAIL_IF_FALSE, problem_description.cpp:1637
            return TMX_ERR_INVALID;
          }
          if (tm.evaluator_type >= 2)
          {
            const tmx_status rc_lvs = add_lvs_segments(tm);
            if (rc_lvs != TMX_OK)
              return rc_lvs;
            break;
          }
          for (int i = tm.first_step; i <= tm.last_step; ++i)
          {
            if (std::find(tm.fixed_steps, tm.fixed_steps + tm.n_fixed_steps, i) != tm.fixed_steps + tm.n_fixed_steps)
              continue;  // the term's own fixed_steps, problem_description.cpp:1767
            const int own = L.n_costs++;
            for (int s = 0; s < d->n_link_spheres; ++s)
              for (int o = 0; o < d->n_obstacles; ++o)
                add_slot(SLOT_COLLISION, i, s, o, own, 1, 0, 0, tm.coeff, 1.0, tm.margin, tm.buffer);
          }
          break;
        }
        case TMX_TERM_COLLISION_CNT:
        {
          if (tm.evaluator_type < 0 || tm.evaluator_type > 4)
          {
            err = "collision evaluator_type must be <= 4";  // FAIL_IF_FALSE, problem_description.cpp:1637
            return TMX_ERR_INVALID;
          }
          if (tm.evaluator_type >= 2)
          {
            const tmx_status rc_lvs = add_lvs_segments(tm);
            if (rc_lvs != TMX_OK)
              return rc_lvs;
            break;
          }
          // CollisionConstraint per non-fixed step (problem_description.cpp:1821-1835): inequality rows, hinge penalty with
          // the merit coefficient; the collision coefficient scales the row itself (slot_scale)
          for (int i = tm.first_step; i <= tm.last_step; ++i)
          {
            if (std::find(tm.fixed_steps, tm.fixed_steps + tm.n_fixed_steps, i) != tm.fixed_steps + tm.n_fixed_steps)
              continue;  // :1827
            const int own = L.n_cnts++;
            for (int s = 0; s < d->n_link_spheres; ++s)
              for (int o = 0; o < d->n_obstacles; ++o)
                add_slot(SLOT_COLLISION, i, s, o, own, 1, 1, 0, tm.coeff, tm.coeff, tm.margin, tm.buffer);
          }
          break;
        }
        case TMX_TERM_JOINT_VEL_TIME:
        {
          // JointVelTermInfo::hatch with TT_USE_TIME (problem_description.cpp:1244-1325): per joint one TrajOptCostFromErrFunc /
          // TrajOptConstraintFromErrFunc over 2 (last - first) rows - the upper rows, then the lower rows - with the coefficient
          // coeffs[j] on every row (a zero coefficient drops the rows, modeling_utils.cpp:175-176, :258-259; the cost stays)
#if !TMX_LINK_ROWS
          err = "rows on two consecutive waypoints (time-parameterised joint velocities) are not enabled in this build";
          return TMX_ERR_UNSUPPORTED;
#else
          if (tm.last_step - tm.first_step < 1)
          {
            err = "joint_vel with use_time: the term needs two steps";
            return TMX_ERR_INVALID;
          }
          const bool zero = time_zero_tols(tm, DK);
          for (int j = 0; j < DK; ++j)
          {
            const int own = tm.is_constraint ? L.n_cnts++ : L.n_costs++;
            const double c = tm.coeffs[j];
            if (!tm.is_constraint && zero)
            {
              // sco::SQUARED: a dynamic quadratic model over (x[i][j], x[i+1][j], tau[i+1]) of every segment
              if (c != 0.0)
              {
                L.tv_owner.push_back(own);
                L.tv_joint.push_back(j);
                L.tv_first.push_back(tm.first_step);
                L.tv_last.push_back(tm.last_step);
                L.tv_coeff.push_back(c);
                L.tv_target.push_back(tm.targets[j]);
                L.tv_up.push_back(tm.upper_tols[j]);
                L.tv_lo.push_back(tm.lower_tols[j]);
                L.tv_terms = true;  // P changes with the iterate and couples a joint with the NEXT waypoint's time variable (engine: decided below)
              }
              continue;
            }
            if (c == 0.0)
              continue;
            for (int half = 0; half < 2; ++half)
              for (int i = tm.first_step; i < tm.last_step; ++i)
              {
                const double tol = half ? tm.lower_tols[j] : tm.upper_tols[j];
                if (tm.is_constraint)  // EQ -> abs penalty (2 aux), INEQ -> hinge (1 aux); objective = merit coefficient
                  add_slot(SLOT_JOINTVEL_TIME, i, j, half, own, zero ? 2 : 1, 1, zero ? 1 : 0, 0.0, c, tm.targets[j], tol);
                else                   // sco::HINGE: exprScale(aff, coeff); addHinge(aff, 1)
                  add_slot(SLOT_JOINTVEL_TIME, i, j, half, own, 1, 0, 0, 1.0, c, tm.targets[j], tol);
                L.c2.back() = L.R2++;
              }
          }
          L.st_terms = true;  // (rows only: the QP stays a block chain with pair rows - structured solvers, piecewise driver)
          break;
#endif
        }
        case TMX_TERM_TOTAL_TIME:
        {
          // TotalTimeTermInfo::hatch (problem_description.cpp:1852-1890): one cost / constraint over tau[1 .. T-1]
          if (T < 2)
          {
            err = "total_time: the problem needs two steps";
            return TMX_ERR_INVALID;
          }
          const bool zero = std::fabs(tm.margin) < 1e-5;
          const int own = tm.is_constraint ? L.n_cnts++ : L.n_costs++;
          const int form = tm.is_constraint ? (zero ? 2 : 3) : (zero ? 0 : 1);
          int slot = -1;
          if (form != 0 && tm.coeff != 0.0)
          {
            slot = (int)L.kind.size();
            if (form == 1)
              add_slot(SLOT_TOTAL_TIME, 1, (int)L.tt_owner.size(), 0, own, 1, 0, 0, 1.0, tm.coeff, 0.0, 0.0);
            else
              add_slot(SLOT_TOTAL_TIME, 1, (int)L.tt_owner.size(), 0, own, form == 2 ? 2 : 1, 1, form == 2 ? 1 : 0, 0.0, tm.coeff, 0.0, 0.0);
          }
          if (form == 0 && tm.coeff == 0.0)
            break;  // (no model, the value is zero: nothing to carry)
          L.tt_owner.push_back(own);
          L.tt_form.push_back(form);
          L.tt_slot.push_back(slot);
          L.tt_coeff.push_back(tm.coeff);
          L.tt_limit.push_back(tm.margin);
          L.st_terms = true;
          L.tt_terms = true;  // (dense engine or rank-one terms on the block chain: decided below, when every term is known)
          break;
        }
        default:
          err = "term kind not lowered by the device path";
          return TMX_ERR_UNSUPPORTED;
      }
      L.term_cp1[(size_t)k] = (int)L.cp_t.size();
      L.term_slot1[(size_t)k] = (int)L.kind.size();
    }
  if (flavor == TMX_FLAVOR_SQP)
    for (int v = 0; v < P.NX; ++v)
    {
      // "originally it pruned these but it changes sparsity so we now set to zero" (trajopt_qp_problem.cpp:938-942), then
      // OSQPEigenSolver::updateHessianMatrix: 2 H (osqp_eigen_solver.cpp:220-229).  A zeroed entry stays in the pattern
      // upstream; it does not contribute to any product here.
      L.pd[v] = 2.0 * ((std::fabs(L.pd[v]) < 1e-7) ? 0.0 : L.pd[v]);
      L.po[v] = 2.0 * ((std::fabs(L.po[v]) < 1e-7) ? 0.0 : L.po[v]);
      L.po2[v] = 2.0 * ((std::fabs(L.po2[v]) < 1e-7) ? 0.0 : L.po2[v]);   // (JointAccelConstraint / JointJerkConstraint squared sets)
      L.po3[v] = 2.0 * ((std::fabs(L.po3[v]) < 1e-7) ? 0.0 : L.po3[v]);
    }
  P.n_sq = L.n_sq;
  L.R = static_cast<int>(L.kind.size());
  P.R = L.R;
  P.n_costs = L.n_costs;
  P.n_cnts = L.n_cnts;
  P.n_cp = static_cast<int>(L.cp_t.size());
  P.n_vel = static_cast<int>(L.vel_first.size());
  L.aoff.assign(L.R, 0);
  for (int r = 0; r < L.R; ++r)
  {
    L.aoff[r] = L.NA;
    L.NA += L.naux[r];
  }
  P.NA = L.NA;
  P.n_max = P.NX + L.NA;
  P.m_max = L.R + P.NX + L.NA;
  int nnzP = 0;
  for (int v = 0; v < P.NX; ++v)
    nnzP += (L.pd[v] != 0.0) + (v < P.NX - D && L.po[v] != 0.0) + (v < P.NX - 2 * D && L.po2[v] != 0.0) + (v < P.NX - 3 * D && L.po3[v] != 0.0);
  P.nnzP = nnzP;
  // column c of upper-triangular P holds (c-3D, c) / (c-2D, c) if po3 / po2 are set there (jerk / acceleration costs), (c-D, c) if
  // po[c-D] != 0 and (c, c) if pd[c] != 0
  L.p_colptr.assign(P.NX + 1, 0);
  for (int c = 0; c < P.NX; ++c)
    L.p_colptr[c + 1] = L.p_colptr[c] + ((c >= 3 * D && L.po3[c - 3 * D] != 0.0) ? 1 : 0) + ((c >= 2 * D && L.po2[c - 2 * D] != 0.0) ? 1 : 0) +
                      ((c >= D && L.po[c - D] != 0.0) ? 1 : 0) + ((L.pd[c] != 0.0) ? 1 : 0);
  P.n_stencil = L.n_stencil;
  P.lvs_kmax = L.lvs_kmax;
  P.n_fx = (int)L.fx_t.size();
  P.n_fx_cost = L.n_fx_cost;
  P.n_tv = (int)L.tv_owner.size();
  P.n_tt = (int)L.tt_owner.size();
  // slots grouped by waypoint, ascending slot id inside a waypoint
  L.wp_start.assign(T + 1, 0);
  L.wp_list.assign(L.R, 0);
  for (int r = 0; r < L.R; ++r)
    L.wp_start[L.st[r] + 1]++;
  for (int t = 0; t < T; ++t)
    L.wp_start[t + 1] += L.wp_start[t];
  {
    std::vector<int> next(L.wp_start.begin(), L.wp_start.end() - 1);
    for (int r = 0; r < L.R; ++r)
      L.wp_list[next[L.st[r]]++] = r;
  }
  int n_ls_hull = 0;
  int n_ls_capsule = 0, n_ob_box = 0;
  for (int s = 0; s < d->n_link_spheres; ++s)
  {
    if (d->link_spheres[s].link < 0 || d->link_spheres[s].link >= D)
    {
      err = "link sphere attached to an invalid link";
      return TMX_ERR_INVALID;
    }
    L.ls_link.push_back(d->link_spheres[s].link);
    for (int q = 0; q < 3; ++q)
      L.ls_center.push_back(d->link_spheres[s].center[q]);
    L.ls_radius.push_back(d->link_spheres[s].radius);
    bool cap = false;
    for (int q = 0; q < 3; ++q)
    {
      const double a = d->link_sphere_axes ? d->link_sphere_axes[3 * s + q] : 0.0;
      L.ls_axis.push_back(a);
      cap = cap || a != 0.0;
    }
    n_ls_capsule += cap ? 1 : 0;
    const int hn = (d->link_hull && d->hull_vertices) ? d->link_hull[2 * s + 1] : 0;
    if (hn < 0 || (hn > 0 && (d->link_hull[2 * s] < 0 || d->link_hull[2 * s] + hn > d->n_hull_vertices)))
    {
      err = "link_hull: vertex range outside hull_vertices";
      return TMX_ERR_INVALID;
    }
    if (hn > 0 && cap)
    {
      err = "a link primitive is at most one of capsule (link_sphere_axes) and convex hull (link_hull)";
      return TMX_ERR_INVALID;
    }
    L.ls_hull.push_back(hn > 0 ? d->link_hull[2 * s] : 0);
    L.ls_hull.push_back(hn);
    n_ls_hull += hn > 0 ? 1 : 0;
  }
  P.n_ls_hull = n_ls_hull;
  if (n_ls_hull > 0)
    L.hullv.assign(d->hull_vertices, d->hull_vertices + (size_t)3 * d->n_hull_vertices);
  // Capsule links under a cast evaluator (evaluator_type 3 / 4): the swept volume of a capsule is not a capsule, but a capsule IS the
  // convex hull of its two cap centres rounded by its radius - such links become two-vertex hulls (every evaluator of the problem
  // then sees them through GJK / EPA; the oracle applies the same rule, oracle/trajprob.hpp constructProblem)
  {
    bool cast_term = false;
    for (int k = 0; k < d->n_terms; ++k)
      cast_term = cast_term || ((d->terms[k].kind == TMX_TERM_COLLISION_COST || d->terms[k].kind == TMX_TERM_COLLISION_CNT) && d->terms[k].evaluator_type >= 3);
    if (cast_term && n_ls_capsule > 0)
    {
      for (int sp = 0; sp < d->n_link_spheres; ++sp)
      {
        const double* a = &L.ls_axis[3 * (size_t)sp];
        if (a[0] == 0.0 && a[1] == 0.0 && a[2] == 0.0)
          continue;
        L.ls_hull[2 * (size_t)sp] = (int)(L.hullv.size() / 3);
        L.ls_hull[2 * (size_t)sp + 1] = 2;
        for (int q = 0; q < 3; ++q)
          L.hullv.push_back(L.ls_center[3 * (size_t)sp + q]);
        for (int q = 0; q < 3; ++q)
          L.hullv.push_back(L.ls_center[3 * (size_t)sp + q] + a[q]);
        L.ls_axis[3 * (size_t)sp] = L.ls_axis[3 * (size_t)sp + 1] = L.ls_axis[3 * (size_t)sp + 2] = 0.0;
        ++n_ls_hull;
        --n_ls_capsule;
      }
      P.n_ls_hull = n_ls_hull;
    }
  }
  P.n_ls_capsule = n_ls_capsule;
  for (int o = 0; o < d->n_obstacles; ++o)
  {
    for (int q = 0; q < 3; ++q)
      L.ob_center.push_back(d->obstacles[o].center[q]);
    L.ob_radius.push_back(d->obstacles[o].radius);
    for (int q = 0; q < 3; ++q)
      L.ob_axis.push_back(d->obstacle_axes ? d->obstacle_axes[3 * o + q] : 0.0);
    bool box = false;
    for (int q = 0; q < 12; ++q)
    {
      const double v = d->obstacle_boxes ? d->obstacle_boxes[12 * o + q] : 0.0;
      L.ob_box.push_back(v);
      box = box || (q < 3 && v > 0.0);
      if (q < 3 && v < 0.0)
      {
        err = "obstacle_boxes: negative half extent";
        return TMX_ERR_INVALID;
      }
    }
    if (box && d->obstacle_axes && (d->obstacle_axes[3 * o] != 0.0 || d->obstacle_axes[3 * o + 1] != 0.0 || d->obstacle_axes[3 * o + 2] != 0.0))
    {
      err = "an obstacle is a capsule (obstacle_axes) or a box (obstacle_boxes), not both";
      return TMX_ERR_INVALID;
    }
    const int nt = (d->obstacle_mesh && d->mesh_triangles) ? d->obstacle_mesh[2 * o + 1] : 0;
    if (nt < 0 || (nt > 0 && (d->obstacle_mesh[2 * o] < 0 || d->obstacle_mesh[2 * o] + nt > d->n_mesh_triangles)))
    {
      err = "obstacle_mesh: triangle range outside mesh_triangles";
      return TMX_ERR_INVALID;
    }
    if (nt > 0)
    {
      if (box || (d->obstacle_axes && (d->obstacle_axes[3 * o] != 0.0 || d->obstacle_axes[3 * o + 1] != 0.0 || d->obstacle_axes[3 * o + 2] != 0.0)))
      {
        err = "an obstacle is at most one of capsule (obstacle_axes), box (obstacle_boxes) and mesh (obstacle_mesh)";
        return TMX_ERR_INVALID;
      }
      double* rec = L.ob_box.data() + 12 * (size_t)o;
      rec[0] = -1.0;
      rec[1] = nt;
      rec[2] = 9.0 * d->obstacle_mesh[2 * o];
      box = true;  // (counted with the boxes: the same code path)
    }
    n_ob_box += box ? 1 : 0;
  }
  P.n_ob_box = n_ob_box;
  if (d->obstacle_mesh && d->mesh_triangles && d->n_mesh_triangles > 0)
    L.mesh.assign(d->mesh_triangles, d->mesh_triangles + (size_t)9 * d->n_mesh_triangles);
  return TMX_OK;
}

// Stage 2: the QP engine, from what the term loop established.  Pure.
static EngineChoice choose_engine(const Lowered& L, const DevProblem& P, const UploadHooks& hooks)
{
  EngineChoice E;
  bool qp_dense = L.qp_dense, st_terms = L.st_terms;
  int band = L.band, R2 = L.R2;
  std::string tv_why;  // what keeps squared velocity-with-time costs on the dense engine
  // TotalTime terms couple all time variables: one global row (HINGE / EQ / INEQ forms) or a dense objective block 2 c g g' over
  // tau[1 .. T-1] (SQUARED form).  Small problems keep the dense engine, bit for bit as before.  A problem over the dense engine's
  // size limit whose ONLY reason for that engine are these terms runs on the block chain instead: the terms become rank-one
  // corrections of the reduced KKT matrix (QpWs::ttn, tmx_qp.h), at any size.  TMX_TOTAL_TIME_CHAIN: "1" the chain at any size,
  // "0" never (the dense engine and its limit).  Problems that need the dense engine for another reason as well (squared
  // velocity-with-time costs, acceleration / jerk rows), banded objectives, function costs and more than TMX_TT_MAX terms stay there.
  if (L.tt_terms)
  {
    const bool able = TMX_LINK_ROWS && !qp_dense && !L.tv_terms && !L.stencil_rows && band == 0 && !L.dyn_p && (int)L.tt_owner.size() <= TMX_TT_MAX;
    const bool want = hooks.total_time_chain == '1' || (hooks.total_time_chain != '0' && P.n_max > hooks.dense_qp_max_n);
    E.tt_chain = able && want;
    if (!E.tt_chain)
      qp_dense = true;
  }
  // Squared JointVel-with-time costs (exprSquare of a x[t][j] + b x[t+1][j] + c tau[t+1] + k) put entries that change with the iterate
  // on (x[t][j], x[t+1][j]), inside block t+1 on (j, tau) and (tau, tau), and between the blocks on (x[t][j], tau[t+1]): P stays block
  // tridiagonal, its coupling blocks are a diagonal plus their last column.  Small problems keep the dense engine, bit for bit as
  // before.  A problem over the dense engine's size limit whose ONLY reason for that engine are these costs runs on the block chain
  // with dense coupling blocks - the pair rows' chain, which carries the costs alone, next to pair rows (velocity limits with time,
  // LVS / cast collision rows) and next to any other row term (QpWs::tvo, tmx_qp.h).  TMX_VEL_TIME_CHAIN: "1" the chain at any size,
  // "0" never (the dense engine and its limit).  Next to TotalTime terms, acceleration / jerk costs or rows, or function costs
  // (their D x D objective blocks live in the per-problem scratch, QpWs::pb, and take another ADMM loop) the dense engine stays.
  if (L.tv_terms)
  {
    const bool able = TMX_LINK_ROWS && !qp_dense && !L.tt_terms && !L.stencil_rows && band == 0 && !L.dyn_p;
    const bool want = hooks.vel_time_chain == '1' || (hooks.vel_time_chain != '0' && P.n_max > hooks.dense_qp_max_n);
    E.tv_chain = able && want;
    if (L.tt_terms)
      tv_why = " next to TotalTime terms";
    else if (band != 0 || L.stencil_rows)
      tv_why = " next to acceleration / jerk costs or rows";
    else if (L.dyn_p)
      tv_why = " next to function costs";
    else if (qp_dense || !TMX_LINK_ROWS)
      tv_why = " in a build without rows on two waypoints";
    else
      tv_why = " with TMX_VEL_TIME_CHAIN=0";
    if (!E.tv_chain)
      qp_dense = true;
    else
    {
      st_terms = true;  // (piecewise driver: the costs' linearisations and the QP kernels that carry them are the piecewise kernels')
      if (R2 == 0)
        R2 = 1;  // no pair row: one unused second-block slot, so that the workspace has the dense-coupling chain (Cd, Mf, Nb, yb)
    }
  }
  // Difference ROWS of order 2 / 3 touch one joint each: as long as every row on several waypoints is such a single-joint row (no
  // LVS / cast collision rows, no CartVel rows) all the blocks they add to the reduced KKT matrix are diagonal, and the problem runs
  // on the banded structured path at any size (band = max of the orders of costs and rows; DevProblem::band_rows).  Next to general
  // pair rows (dense coupling blocks) or to function costs (dynamic P) they keep the dense engine.
  std::string br_why;  // with TMX_BAND_ROW_PAIR_CHAIN=1: what keeps them on the dense engine next to general pair rows
  if (L.stencil_rows)
  {
    int other_pairs = 0;
    for (int r = 0; r < L.R; ++r)
      if (L.c2[r] >= 0 && !slot_is_diff(L.kind[r]))
        ++other_pairs;
    if (!qp_dense && other_pairs == 0 && P.D <= 255)
    {
      E.band_rows = true;
      st_terms = true;  // the term code of these rows is instantiated in the piecewise kernels (template flag ST)
      band = std::max(band, L.max_row_order);
    }
    else
    {
      // ... next to general pair rows the first coupling block of the reduced KKT matrix is dense (Cd: the pair rows' w_r coef_r c2_r'
      // plus, on its diagonal, the difference rows' first-coupling terms) and the far couplings stay diagonal (bk2 / bk3): the banded
      // factorisation with a dense first coupling of DevProblem::band_pairs, with the far entries of the rows in the ADMM loop of
      // band_rows - both flags.  OPT-IN, TMX_BAND_ROW_PAIR_CHAIN=1 (at any size); unset or "0" the dense engine and its limit, as
      // before.  Squared acceleration / jerk costs of the same problem ride along (po2 / po3 enter bk2 / bk3).  Next to function costs,
      // to time-parameterised terms or in the trajopt_sqp flavour the dense engine stays.
      const bool able = TMX_LINK_ROWS && !qp_dense && other_pairs > 0 && P.D <= 255 && !L.tt_terms && !L.tv_terms && !P.use_time && !L.dyn_p &&
                        P.flavor == TMX_FLAVOR_SCO;
      if (able && hooks.band_row_pair_chain == '1')
      {
        E.band_rows = true;
        E.band_pairs = true;
        st_terms = true;
        band = std::max(band, L.max_row_order);
      }
      else
      {
        if (hooks.band_row_pair_chain == '1')  // (the text of the refusal is the one of before unless the route was asked for)
        {
          if (L.dyn_p)
            br_why = "function costs";
          else if (L.tt_terms || L.tv_terms || P.use_time)
            br_why = "time-parameterised terms";
          else if (P.flavor != TMX_FLAVOR_SCO)
            br_why = "the trajopt_sqp flavour";
          else if (other_pairs == 0)
            br_why = "more than 255 variables per waypoint";
          else
            br_why = "a build without rows on two waypoints";
        }
        qp_dense = true;
      }
    }
  }
  // squared acceleration / jerk costs alone keep the structured solver (banded block factorisation of the generic path).  Together
  // with general pair rows (LVS / cast collision rows, CartVel rows: dense coupling blocks) small problems keep the dense engine, bit
  // for bit as before; a problem over that engine's size limit whose ONLY reason for it is this combination runs on the banded
  // factorisation with a dense first coupling block (DevProblem::band_pairs: K_{t+1,t} = Cd_t', the far couplings stay diagonal),
  // on the piecewise driver, whose QP kernels hold the pair-row + banded ADMM loop.  TMX_BAND_PAIR_CHAIN: "1" that route at any size,
  // "0" never (the dense engine and its limit).  Next to acceleration / jerk ROWS with general pair rows, to time-parameterised terms,
  // to function costs or in the trajopt_sqp flavour the dense engine stays.
  std::string bp_why;  // what keeps the combination on the dense engine
  if (band && !E.band_rows && (qp_dense || R2 > 0))
  {
    const bool able = TMX_LINK_ROWS && !qp_dense && !L.stencil_rows && R2 > 0 && !L.tt_terms && !L.tv_terms && !L.dyn_p && P.flavor == TMX_FLAVOR_SCO;
    const bool want = hooks.band_pair_chain == '1' || (hooks.band_pair_chain != '0' && P.n_max > hooks.dense_qp_max_n);
    E.band_pairs = able && want;
    if (L.dyn_p)
      bp_why = "function costs";
    else if (L.stencil_rows)
      bp_why = "acceleration / jerk rows";
    else if (L.tt_terms || L.tv_terms)
      bp_why = "time-parameterised terms";
    else if (P.flavor != TMX_FLAVOR_SCO)
      bp_why = "rows on two waypoints in the trajopt_sqp flavour";
    else if (qp_dense || !TMX_LINK_ROWS)
      bp_why = "rows on two waypoints in a build without them";
    else
      bp_why = "rows on two waypoints with TMX_BAND_PAIR_CHAIN=0";
    if (E.band_pairs)
      st_terms = true;  // (piecewise driver: its QP kernels carry the ROWSK + BANDK instantiations.  The lowering sets L.st_terms for these
                        //  costs in the trajopt_sqp flavour only; a trajopt_sco problem with squared costs alone runs on k_sqp_pool_band)
    else
    {
      qp_dense = true;
      band = 0;
    }
  }
  E.qp_dense = qp_dense;
  E.band = band;
  E.R2 = R2;
  // convex-hull links (and capsule links under a cast evaluator, which become hulls): their contact code (GJK / EPA) is instantiated
  // in the piecewise kernels only (template flag HULL)
  E.st = qp_dense || st_terms || P.n_ls_hull > 0;
  if (qp_dense)
  {
    // what put the problem on the dense engine (TotalTime terms alone do not above its size limit: they run on the block chain unless
    // one of the reasons below keeps them off it)
    std::string& why = E.dense_reasons;
    auto reason = [&why](const std::string& r) { why += (why.empty() ? "" : ", ") + r; };
    if (!L.tv_owner.empty())
      reason("squared joint-velocity costs with time" + tv_why);
    if (L.stencil_rows)
      reason("acceleration / jerk rows next to collision / CartVel rows on two waypoints or to time-parameterised terms" +
             (br_why.empty() ? std::string() : " (TMX_BAND_ROW_PAIR_CHAIN=1 does not apply: " + br_why + ")"));
    if (L.tt_terms && (int)L.tt_owner.size() > TMX_TT_MAX)
      reason("more than " + std::to_string(TMX_TT_MAX) + " TotalTime terms");
    else if (L.tt_terms && (band != 0 || L.dyn_p))
      reason("TotalTime terms next to acceleration / jerk costs or function costs");
    else if (L.tt_terms && L.tv_owner.empty() && !L.stencil_rows)
      reason("TotalTime terms with TMX_TOTAL_TIME_CHAIN=0 (or a build without rows on two waypoints)");
    // ("... next to rows on two waypoints or function costs": the wording of before for the cases of before; what the route of
    //  DevProblem::band_pairs leaves is named behind it)
    if (why.empty())
      reason("acceleration / jerk costs next to rows on two waypoints or function costs" + (bp_why.empty() ? std::string() : " (here: " + bp_why + ")"));
  }
  return E;
}

// the term / structure kernels' dynamic LDS (bytes)
static size_t small_smem_bytes(const Lowered& L, const DevProblem& P)
{
  const size_t small_ints = 2 * (size_t)(P.n_max + 1) + 4 * (size_t)L.R + 2 + 16 + 16 + 512;  // qp_structure: tables, hash accumulators, chunk totals
  const size_t small = std::max<size_t>((tmx_eval_scratch_doubles(L.R, P.D * P.T, (int)L.vel_first.size(), L.n_costs, L.n_cnts) + L.n_costs + L.n_cnts + 8) * sizeof(double),
                                        small_ints * sizeof(int) + 64);
  return std::max<size_t>(small, tmx_cvx_scratch_doubles(P.n_cp, P.D) * sizeof(double));
}

// Stage 3: where the QP workspace lives, which thread carries which row, the LDS budgets.  Pure; reads the engine fields of P.
static Placement place_workspace(const Lowered& L, const EngineChoice& E, const DevProblem& P, const UploadHooks& hooks)
{
  Placement pl;
  const int D = P.D, T = P.T, R = L.R, NA = L.NA, R2 = E.R2;
  // workspace placement: everything in LDS if it fits; else everything but the row coefficient arrays (they move to the HBM
  // scratch: config 4, 177 -> 125 KB); else the HBM-workspace kernels
  // TMX_FORCE_COEF_FAR - test hook: exercise the placement on small problems / the host build
  if (hooks.force_coef_far == '1' || (qp_smem_bytes(D, T, R, NA, R2, 0) > 160 * 1024 && qp_smem_bytes(D, T, R, NA, R2, 1) <= 160 * 1024))
    pl.coef_far = 1;
  // (round 4 also moved the rows of odd block sizes above 8 there, on the hypothesis that 16-byte flat accesses at 8-byte aligned LDS
  //  addresses fault; the hardware accepts them - tools/ubench/align_probe.hip, profiles/r05/r05a_align_probe.log - and the placement is gone)
  {
    // compact row lists (bit 1 of the flag word): problems whose row slots are mostly collision slots - thousands of slots, a
    // few hundred contacts at any time (config 3: 15.7 k slots, ~370 active rows).  Such problems never take the dense fast
    // path (R <= 512), which rebuilds its workspace descriptor without the lists.
    int n_coll = 0;
    for (int k : L.kind)
      n_coll += (k == SLOT_COLLISION || k == SLOT_COLLISION_LVS) ? 1 : 0;
    // TMX_FORCE_COMPACT - test hook: "1" on (any size > 512 is not required on the host build), "0" off
    // (pair-row problems never take the dense fast path, so the lists pay at any size: config 4 - 478 slots, ~195 active rows - 17 %)
    if (hooks.force_compact == '1' || (hooks.force_compact != '0' && (R >= 1024 || R2 > 0) && 2 * n_coll > R))
      pl.coef_far |= 2;
  }
  if (L.dyn_p && !E.qp_dense)
    pl.coef_far |= 4;  // dynamic objective blocks behind the far region of the per-problem scratch (qp_dynp_offset)
  // row -> thread assignment of the register-resident bursts (tmx_row_perm.h); TMX_ROW_PERM=0 keeps the slot order
  if (hooks.row_perm != '0' && R <= 2 * TMX_QP_NT && TMX_QP_NT == 256)
    pl.row_perm = build_row_perm(R, L.naux, TMX_QP_NT);
  {
    // constants of the QP setup (DevProblem::wp_pst / row_epos): the grouped e exchange of the register-resident burst keeps the rows of
    // waypoint t in wp_list order from the even offset wp_pst[t] on
    pl.pst.assign(T + 1, 0);
    pl.epos.assign(R, 0);
    int acc = 0, rows_max = 0, naux_max = 0;
    for (int t = 0; t <= T; ++t)
    {
      pl.pst[t] = acc;
      if (t == T)
        break;
      const int c = L.wp_start[t + 1] - L.wp_start[t];
      for (int u = L.wp_start[t]; u < L.wp_start[t + 1]; ++u)
        pl.epos[L.wp_list[u]] = acc + (u - L.wp_start[t]);
      acc += c + (c & 1);
      rows_max = std::max(rows_max, c);
    }
    for (int r = 0; r < R; ++r)
      naux_max = std::max(naux_max, L.naux[r]);
    pl.setup_fast = (rows_max <= TMX_SETUP_COL && naux_max <= 2 && R <= 2 * TMX_QP_NT) ? 1 : 0;
    // the register-resident polish (tmx_polish.h) lays its exchange buffers and flags over the G region of the dense fast path
    pl.polish_fast = 0;
    if (pl.setup_fast && dpart_fits(D, T) && R2 == 0)
    {
      DPart dp;
      dpart_make(T, dp);
      const size_t gn = (size_t)dp.Lmax * D, g_doubles = (size_t)dp.P * gn * dpart_gstride((int)gn);
      pl.polish_fast = polish_fast_doubles(T, D * T, R, NA, acc + TMX_SETUP_COL) <= g_doubles ? 1 : 0;
    }
    // the ADMM factorisation with the interior inverses inside one wave (tmx_factor.h)
    pl.factor_fast = (pl.setup_fast && R2 == 0 && factor_fast_fits(D, T)) ? 1 : 0;
    // the specialised SQP shell (tmx_step.h): one thread per primary column with its waypoint's rows in registers, column pointers by
    // TMX_STEP_CP_PASSES wave scans; the static objective pattern of the block-tridiagonal problems; no compact lists; trajopt_sco;
    // room for the decision's copies (2 n_costs + 3 n_cnts + the log head) in the scratch of evaluate_terms behind the model values
    const size_t eval_room = tmx_eval_scratch_doubles(R, D * T, (int)L.vel_first.size(), L.n_costs, L.n_cnts);
    pl.step_fast = (pl.setup_fast && dpart_fits(D, T) && R >= 1 && 2 * (size_t)L.n_costs + 3 * (size_t)L.n_cnts + TMX_STEP_LOG_HEAD + 1 <= eval_room && R2 == 0 && D * T <= TMX_QP_NT && P.n_max + 1 <= TMX_STEP_CP_PASSES * TMX_QP_NT && P.flavor == 0 &&
                    !P.st && !P.band && !P.band_rows && !E.qp_dense && !P.use_time && P.n_fx == 0 && P.n_stencil == 0 && P.n_tt == 0 && P.n_tv == 0 &&
                    !(pl.coef_far & 2))
                       ? 1
                       : 0;
    // the evaluation side of that step (tmx_eval.h): the slot kinds step_eval_fast evaluates, velocity kinds 0 and 1 (what step_fast
    // leaves: no stencil costs, trajopt_sco), and its tables fit the LDS of the QP workspace, dead at that point of the step; then the
    // hashes of P for every n = NX .. n_max
    bool kinds_ok = true;
    for (int k : L.kind)
      kinds_ok = kinds_ok && tmx_step_eval_kind(k);
    for (int k : L.vel_kind)
      kinds_ok = kinds_ok && (k == 0 || k == 1);
    const size_t qp_lds = qp_smem_bytes(D, T, R, NA, R2, pl.coef_far);
    pl.eval_fast = (pl.step_fast && kinds_ok && qp_lds <= 160 * 1024 &&
                    tmx_step_eval_doubles(R, D * T, (int)L.vel_first.size(), L.n_costs, L.n_cnts) * sizeof(double) <= qp_lds &&
                    tmx_cvx_fast_doubles((int)L.cp_t.size(), D, D * T) * sizeof(double) <= qp_lds)
                       ? 1
                       : 0;
    if (pl.eval_fast)
    {
      pl.p_hash.assign(2 * (size_t)(P.n_max - P.NX + 1), 0ULL);
      tmx_build_p_hash_table(L.p_colptr.data(), L.pd.data(), L.po.data(), D, P.NX, P.n_max, P.nnzP, pl.p_hash.data());
    }
  }
  pl.smem_small = small_smem_bytes(L, P);
#if TMX_IS_DEVICE
  {
    // a wave pair per problem (tmx_wave.h): block-tridiagonal QPs with diagonal couplings whose row-slot template fits the lane plan.
    // OPT-IN (TMX_WAVE=1): measured on MI355X (round 6, profiles/r06/) the wave-pair solver runs BASELINE config 1 at 101 k SQP it/s
    // against the 118 k of k_sqp_pool - its ADMM iteration costs 4.6 k cycles per problem per CU where the stated bar was < 3 k - so
    // the one-workgroup-per-CU kernels stay the default; DESIGN.md section 5
    std::vector<int> plan(TMX_WV_NT * TMX_WV_REC, 0);
    int gmax = 4, aux2 = 0, n3 = 0;
    if (hooks.wave == '1' && P.flavor == 0 && R2 == 0 && pl.coef_far == 0 && !E.qp_dense && !P.st && !P.band && !P.use_time && P.n_fx == 0 &&
        wave_plan_build(D, T, R, L.st.data(), L.naux.data(), plan.data(), &gmax, &aux2, &n3))
    {
      const size_t lds = std::max(pl.smem_small, wave_lds_doubles(D, T, R) * sizeof(double));
      if (lds <= 40 * 1024)  // four problems per CU
      {
        pl.plan.swap(plan);
        pl.wave_ok = 1;
        pl.wv_gmax = gmax;
        pl.wv_aux2 = aux2;
        pl.smem_wave = lds;
      }
    }
  }
#endif
  // LDS budgets
  pl.smem_qp = qp_smem_bytes(D, T, R, NA, R2, pl.coef_far);
  if (P.tt_chain > 0 || P.tv_chain)
  {
    // per-problem data of the rank-one terms (g, Z = K_chain^-1 g: read by every ADMM iteration) or the joint - time entries of
    // squared JointVel-with-time costs (read by every factorisation and every product with P): behind the QP workspace when it
    // stays in LDS with them, or lives in HBM anyway (long horizons); in the per-problem scratch when they alone would push an
    // LDS-resident workspace out
    const size_t tt_bytes = ((P.tv_chain ? qp_tv_doubles(D, T) : qp_tt_doubles(D, T, P.tt_chain)) + 2) * sizeof(double);
    // TMX_TT_PLACE - test hook: "2" = in the per-problem scratch whatever the sizes
    if (TMX_QP_COLD_IN_LDS && hooks.tt_place != '2' && (pl.smem_qp > 160 * 1024 || pl.smem_qp + tt_bytes <= 160 * 1024))
    {
      pl.tt_place = 1;
      pl.smem_qp += tt_bytes;
    }
    else
    {
      pl.tt_place = 2;
      pl.tt_scratch = tt_bytes / sizeof(double);
    }
  }
  return pl;
}

// Stage 4: every table to the device, in a fixed allocation order (tmx_ctx::prob_allocs), then DevProblem itself.
static tmx_status upload_tables(tmx_ctx* ctx, const Lowered& L, const Placement& pl, DevProblem& P)
{
  auto& pool = ctx->prob_allocs;
  tmx_status rc;
#define UP(field, vec)                                                                                                \
  if ((rc = upload(ctx, pool, &P.field, vec)) != TMX_OK)                                                              \
  return rc
  UP(slot_kind, L.kind);
  UP(slot_t, L.st);
  UP(slot_sub, L.sub);
  UP(slot_sub2, L.sub2);
  UP(slot_owner, L.owner);
  UP(slot_naux, L.naux);
  UP(slot_aoff, L.aoff);
  UP(slot_iscnt, L.iscnt);
  UP(slot_eq, L.iseq);
  UP(slot_objc, L.objc);
  UP(slot_scale, L.scale);
  UP(slot_aux1, L.aux1);
  UP(slot_aux2, L.aux2);
  UP(slot_c2, L.c2);
  UP(slot_sub3, L.sub3);
  UP(slot_aux3, L.aux3);
  {
    // slot range of every cost / constraint (key = cost index, or n_costs + constraint index)
    const int n_costs = L.n_costs, n_cnts = L.n_cnts;
    std::vector<int> lo((size_t)(n_costs + n_cnts), 1), hi((size_t)(n_costs + n_cnts), 0);
    std::vector<char> seen((size_t)(n_costs + n_cnts), 0);
    for (int r = 0; r < L.R; ++r)
    {
      if (L.kind[(size_t)r] == SLOT_FIXED)
        continue;
      const int k = L.iscnt[(size_t)r] ? n_costs + L.owner[(size_t)r] : L.owner[(size_t)r];
      if (k < 0 || k >= n_costs + n_cnts)
        continue;
      if (!seen[(size_t)k])
      {
        lo[(size_t)k] = r;
        seen[(size_t)k] = 1;
      }
      hi[(size_t)k] = r;
    }
    UP(own_lo, lo);
    UP(own_hi, hi);
  }
  UP(wp_start, L.wp_start);
  UP(wp_list, L.wp_list);
  UP(pd, L.pd);
  UP(po, L.po);
  UP(pq, L.pq);
  UP(ls_axis, L.ls_axis);
  UP(ls_hull, L.ls_hull);
  UP(hull, L.hullv);
  UP(ob_box, L.ob_box);
  UP(mesh, L.mesh);
  UP(po2, L.po2);
  UP(po3, L.po3);
  UP(fx_t, L.fx_t);
  UP(fx_kind, L.fx_kind);
  UP(fx_owner, L.fx_owner);
  UP(fx_op0, L.fx_op0);
  UP(fx_nops, L.fx_nops);
  UP(fx_c0, L.fx_c0);
  UP(fx_nout, L.fx_nout);
  UP(fx_slot0, L.fx_slot0);
  UP(fx_ci, L.fx_ci);
  UP(fx_ops, L.fx_ops);
  UP(fx_consts, L.fx_consts);
  UP(p_colptr, L.p_colptr);
  UP(vel_first, L.vel_first);
  UP(vel_last, L.vel_last);
  UP(vel_cost, L.vel_cost);
  UP(vel_kind, L.vel_kind);
  UP(vel_coeffs, L.vel_coeffs);
  UP(vel_targets, L.vel_targets);
  UP(cp_t, L.cp_t);
  UP(cp_owner, L.cp_owner);
  UP(cp_iscnt, L.cp_iscnt);
  UP(cp_nrows, L.cp_nrows);
  UP(cp_idx, L.cp_idx);
  UP(cp_slot0, L.cp_slot0);
  UP(cp_coeff, L.cp_coeff);
  UP(cp_target, L.cp_target);
  UP(ls_link, L.ls_link);
  UP(ls_center, L.ls_center);
  UP(ls_radius, L.ls_radius);
  UP(ob_center, L.ob_center);
  UP(ob_radius, L.ob_radius);
  UP(ob_axis, L.ob_axis);
  UP(tv_owner, L.tv_owner);
  UP(tv_joint, L.tv_joint);
  UP(tv_first, L.tv_first);
  UP(tv_last, L.tv_last);
  UP(tv_coeff, L.tv_coeff);
  UP(tv_target, L.tv_target);
  UP(tv_up, L.tv_up);
  UP(tv_lo, L.tv_lo);
  UP(tt_owner, L.tt_owner);
  UP(tt_form, L.tt_form);
  UP(tt_slot, L.tt_slot);
  UP(tt_coeff, L.tt_coeff);
  UP(tt_limit, L.tt_limit);
  // the placement: DevProblem::row_perm / wv_plan stay null without a permutation / a lane plan
  P.coef_far = pl.coef_far;
  P.setup_fast = pl.setup_fast;
  P.polish_fast = pl.polish_fast;
  P.step_fast = pl.step_fast;
  P.factor_fast = pl.factor_fast;
  P.eval_fast = pl.eval_fast;
  if (pl.eval_fast)
    UP(p_hash, pl.p_hash);
  P.tt_place = pl.tt_place;
  P.wave_ok = pl.wave_ok;
  P.wv_gmax = pl.wv_gmax;
  P.wv_aux2 = pl.wv_aux2;
  if (!pl.row_perm.empty())
    UP(row_perm, pl.row_perm);
  UP(wp_pst, pl.pst);
  UP(row_epos, pl.epos);
  if (pl.wave_ok)
    UP(wv_plan, pl.plan);
#undef UP
  if (!ctx->dp)
  {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, sizeof(DevProblem)));
    ctx->dp = static_cast<DevProblem*>(p);
  }
  HIPCHK(hipMemcpy(ctx->dp, &P, sizeof(DevProblem), hipMemcpyHostToDevice));
  return TMX_OK;
}

// Stage 5: the context's launch configuration - LDS budgets, the dense engine's size limit, kernel attributes, pool size.
static tmx_status configure_launch(tmx_ctx* ctx, const DevProblem& P, const Lowered& L, const EngineChoice& E, const Placement& pl, const UploadHooks& hooks)
{
  const int D = P.D, T = P.T, R = L.R, NA = L.NA, R2 = E.R2;
  ctx->smem_qp = pl.smem_qp;
  ctx->tt_scratch = pl.tt_scratch;
  if (pl.wave_ok)
    ctx->smem_wave = pl.smem_wave;
  if (hooks.verbose)
    std::fprintf(stderr, "[tmx] QP engine: %s; TotalTime terms %d, as rank-one terms on the block chain %d; squared velocity-with-time cost instances %d, "
                         "on the dense-coupling block chain %d (data of either %s)\n",
                 P.qp_dense ? "dense" : (P.st ? "structured, piecewise driver" : "structured"), P.n_tt, P.tt_chain, P.n_tv, P.tv_chain,
                 P.tt_place == 1 ? "behind the QP workspace" : (P.tt_place == 2 ? "in the per-problem scratch" : "-"));
  if (hooks.verbose)
    std::fprintf(stderr, "[tmx] problem: D %d (joints %d), T %d, row slots %d, aux %d, pair rows %d, workspace flags %d, band %d, dense %d, QP workspace %zu B, wave-pair solver %d (LDS %zu B, largest lane group %d, second slack in row slots 0x%x)\n", D, P.DK, T, R, NA, R2,
                 P.coef_far, P.band, (int)P.qp_dense, ctx->smem_qp, P.wave_ok, ctx->smem_wave, P.wv_gmax, P.wv_aux2);
  ctx->smem_small = pl.smem_small;
  ctx->dense = P.qp_dense != 0;
  ctx->piecewise = P.st != 0;
  ctx->band = P.band != 0;
  ctx->hull = P.n_ls_hull > 0;
  ctx->wave = P.wave_ok != 0;
  ctx->tt_squared = std::find(L.tt_form.begin(), L.tt_form.end(), 0) != L.tt_form.end();
  // The dense engine inverts n x n (every rho update) and (n + active rows)^2 (polish) matrices by Gauss-Jordan, one workgroup per
  // problem on an HBM-resident matrix: fine for the few-hundred-variable QPs of the reference's KATs, minutes per batch at the
  // size of BASELINE config 1 with smoothing costs (n = 572: a 64-seed batch did not finish in 800 s).  Refuse instead of hanging;
  // TMX_DENSE_QP_MAX_N lifts the limit for callers who accept the time.
  if (ctx->dense && P.n_max > hooks.dense_qp_max_n)
  {
    ctx->err = E.dense_reasons + ": the QP of this problem has too many variables for the dense engine to solve in practical time (limit 448 incl. "
               "penalty variables; TMX_DENSE_QP_MAX_N overrides); TotalTime terms alone (up to " + std::to_string(TMX_TT_MAX) + "), squared "
               "joint-velocity costs with time (alone, next to rows on two waypoints and to other row terms), function costs, "
               "smoothing costs, acceleration / jerk limits and function terms that are rows (constraints, ABS / HINGE costs, AvoidSingularity, "
               "DynamicCartPose) have no such limit";
    ctx->have_problem = false;
    return TMX_ERR_UNSUPPORTED;
  }
  if (ctx->dense)
    ctx->smem_small = std::max<size_t>(ctx->smem_small, 320 * sizeof(double));  // reduction scratch of qp_generic_block
#if defined(TMX_HOST_EMU) && !defined(TMX_EMU_SIMT)
  ctx->nt_qp = 1;
  ctx->nt_small = 1;
  ctx->smem_pool = std::max<size_t>(ctx->smem_qp, 64);
  ctx->pool_wgs = 8;
#else
  // long-horizon problems (config 2: T = 300): neither the QP workspace nor the term scratch fits the 160 KB of LDS;
  // every kernel then carves its scratch from a per-workgroup HBM slice (k_*_hbm for the QP / fused kernels)
  ctx->ws_in_hbm = ctx->smem_qp > 160 * 1024;
  ctx->ws_bytes = ctx->ws_in_hbm ? std::max({ ctx->smem_qp, ctx->smem_small, (size_t)(L.n_costs + L.n_cnts + 8) * sizeof(double) }) : 0;
  if (ctx->ws_in_hbm)
    ctx->smem_small = 64;
  ctx->smem_chain = 0;
  if (ctx->ws_in_hbm && qp_chain_lds_doubles(D, T, R2) * sizeof(double) <= 160 * 1024)
  {
    ctx->smem_chain = qp_chain_lds_doubles(D, T, R2) * sizeof(double);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_qp_solve_hbm), hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(ctx->smem_chain)));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sqp_fused_hbm), hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(ctx->smem_chain)));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sqp_fused_hbm_q), hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(ctx->smem_chain)));
  }
  // one problem per CU when the workspace is large: use 4 waves so the data-parallel phases go 4x wider
  ctx->nt_qp = TMX_QP_NT;
  ctx->nt_small = 64;
  if (!ctx->ws_in_hbm)
  {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_qp_solve), hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(ctx->smem_qp)));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sqp_fused), hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(ctx->smem_qp)));
  }
  ctx->smem_pool = ctx->ws_in_hbm ? 64 : std::max<size_t>(ctx->smem_qp, (2 * TMX_QP_NT + 8) * sizeof(int));
  if (!ctx->ws_in_hbm)
    HIPCHK(hipFuncSetAttribute(ctx->band ? reinterpret_cast<const void*>(k_sqp_pool_band) : reinterpret_cast<const void*>(k_sqp_pool),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(ctx->smem_pool)));
  if (ctx->smem_small > 64 * 1024)
  {
    // the term / structure kernels of a long-horizon problem need more than the default 64 KB of dynamic LDS
    const void* small_kernels[] = { reinterpret_cast<const void*>(k_prepare), reinterpret_cast<const void*>(k_evaluate),
                                    reinterpret_cast<const void*>(k_convexify), reinterpret_cast<const void*>(k_prepare_hull),
                                    reinterpret_cast<const void*>(k_evaluate_hull), reinterpret_cast<const void*>(k_convexify_hull), reinterpret_cast<const void*>(k_export_csc),
                                    reinterpret_cast<const void*>(k_sqp_update), reinterpret_cast<const void*>(k_qp_solve_dense),
                                    reinterpret_cast<const void*>(k_model_values) };
    for (const void* k : small_kernels)
      HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(ctx->smem_small)));
  }
  {
    // persistent pool size = what is resident at once: CUs x workgroups per CU (LDS- and register-limited)
    int cus = 256, per_cu = 1;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess)
      cus = prop.multiProcessorCount;
    const hipError_t occ = ctx->band ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_sqp_pool_band, TMX_QP_NT, ctx->smem_pool)
                                     : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_sqp_pool, TMX_QP_NT, ctx->smem_pool);
    if (occ != hipSuccess || per_cu < 1)
      per_cu = 1;
    per_cu = std::min(per_cu, TMX_QP_WGS_PER_CU);
    ctx->pool_wgs = cus * per_cu;
    if (const char* e = std::getenv("TMX_POOL_WGS"))  // tuning hook
      ctx->pool_wgs = std::max(1, std::atoi(e));
    if (const char* e = std::getenv("TMX_SQP_MODE"))  // tuning hook: 0 stepwise launches, 1 fused in-order, 2 pool
      ctx->mode = std::max(0, std::min(2, std::atoi(e)));
    if (hooks.verbose)
      std::fprintf(stderr, "[tmx] CUs %d, pool workgroups/CU %d, pool size %d, LDS %zu B\n", cus, per_cu, ctx->pool_wgs, ctx->smem_pool);
  }
#endif
  ctx->have_problem = true;
  return TMX_OK;
}

// no link pairs: the self-collision side of the check tests nothing
static void drop_check_pairs(tmx_ctx* ctx)
{
  if (ctx->d_check_pairs)
    (void)hipFree(ctx->d_check_pairs);
  ctx->d_check_pairs = nullptr;
  ctx->check_link_pairs.clear();
  ctx->check_prim_pairs.clear();
}

// back to one query: the per-query tables go and the next batch carries null pointers (ensure_batch)
static void drop_queries(tmx_ctx* ctx)
{
  free_pool(ctx->query_allocs);
  ctx->n_queries = 1;
  ctx->d_qprob = nullptr;
  ctx->d_qcp = ctx->d_qaux1 = nullptr;
  ctx->h_qcp.clear();
  ctx->h_qaux1.clear();
}

tmx_status tmx_problem_upload(tmx_ctx* ctx, const tmx_problem_desc* d, const tmx_sqp_params* sqp, const tmx_osqp_settings* osqp)
{
  if (!ctx || !d)
    return TMX_ERR_INVALID;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const UploadHooks hooks = UploadHooks::read();
  // DK joints; D variables per waypoint (time-parameterised problems carry the time variable 1 / dt behind the joints)
  const int DK = d->n_dof, T = d->n_steps;
  const int D = DK + (d->use_time ? 1 : 0);
  if (DK < 1 || D > TMX_MAX_DOF || T < 1)
  {
    ctx->err = "n_dof (+ 1 with use_time) must be in [1, TMX_MAX_DOF] and n_steps >= 1";
    return TMX_ERR_INVALID;
  }
  if (d->use_time && (d->dt_lower_lim <= 0 || d->dt_upper_lim < d->dt_lower_lim))
  {
    // ProblemConstructionInfo::readBasicInfo  problem_description.cpp:129-133
    ctx->err = "dt limits (Basic Info) invalid. The lower limit must be positive, and the minimum upper limit is equal to the lower limit.";
    return TMX_ERR_INVALID;
  }
  {
    // ConstructProblem  problem_description.cpp:415-452: a term that uses time <=> basic_info.use_time
    bool term_time = false;
    for (int k = 0; k < d->n_terms && d->terms; ++k)
      term_time = term_time || d->terms[k].kind == TMX_TERM_JOINT_VEL_TIME || d->terms[k].kind == TMX_TERM_TOTAL_TIME;
    if (term_time && !d->use_time)
    {
      ctx->err = "A term is using time and basic_info is not set correctly. Try basic_info.use_time = true";
      return TMX_ERR_INVALID;
    }
    // (the converse - "No terms use time and basic_info is not set correctly" - is a check on the TermInfo FLAGS in the reference: a
    //  joint_pos term listed with use_time switches the time column on without ever touching it, problem_description.cpp:1124-1125;
    //  the front ends make that check, the term table cannot)
  }
  if (d->n_fixed_steps < 0 || d->n_fixed_dofs < 0 || d->n_terms < 0 || d->n_link_spheres < 0 || d->n_obstacles < 0 ||
      (d->n_fixed_steps > 0 && !d->fixed_steps) || (d->n_fixed_dofs > 0 && !d->fixed_dofs) || (d->n_terms > 0 && !d->terms) ||
      (d->n_link_spheres > 0 && !d->link_spheres) || (d->n_obstacles > 0 && !d->obstacles))
  {
    ctx->err = "tmx_problem_desc: negative count or NULL array with a positive count";
    return TMX_ERR_INVALID;
  }
  free_pool(ctx->prob_allocs);
  free_pool(ctx->batch_allocs);
  ctx->Bcap = ctx->Balloc = 0;
  ctx->have_problem = false;
  drop_queries(ctx);  // a new problem has one query
  drop_check_pairs(ctx);  // ... and no link pairs
  ctx->h_ls_link.clear();
  DevProblem& P = ctx->hp;
  fill_basic_info(d, sqp, osqp, P);
  Lowered L;
  tmx_status rc;
  if ((rc = lower_terms(d, P, L, ctx->err)) != TMX_OK)
    return rc;
  // what tmx_queries_set / tmx_query_set_targets need of the lowering
  ctx->own_cp = L.cp_target;
  ctx->own_aux1 = L.aux1;
  ctx->own_sub = L.sub;
  ctx->term_cp0 = L.term_cp0;
  ctx->term_cp1 = L.term_cp1;
  ctx->term_slot0 = L.term_slot0;
  ctx->term_slot1 = L.term_slot1;
  ctx->term_kind.resize((size_t)d->n_terms);
  for (int k = 0; k < d->n_terms; ++k)
    ctx->term_kind[(size_t)k] = d->terms[k].kind;
  ctx->n_dof = DK;
  ctx->h_ls_link = L.ls_link;
  const EngineChoice E = choose_engine(L, P, hooks);
  P.band = E.band;
  P.band_rows = E.band_rows ? 1 : 0;
  P.qp_dense = E.qp_dense ? 1 : 0;
  P.st = E.st ? 1 : 0;
  P.tt_chain = E.tt_chain ? (int)L.tt_owner.size() : 0;
  P.tv_chain = E.tv_chain ? 1 : 0;
  P.band_pairs = E.band_pairs ? 1 : 0;
  P.n_link = E.R2;
  const Placement pl = place_workspace(L, E, P, hooks);
  if ((rc = upload_tables(ctx, L, pl, P)) != TMX_OK)
    return rc;
  return configure_launch(ctx, P, L, E, pl, hooks);
}

static tmx_status ensure_batch(tmx_ctx* ctx, int B)
{
  if (ctx->n_queries > 1 && B % ctx->n_queries != 0)
  {
    ctx->err = "tmx_batch_set_x0: the batch must hold the same number of seeds for each of the " + std::to_string(ctx->n_queries) +
               " queries (batch % n_queries == 0)";
    return TMX_ERR_INVALID;
  }
  const int spq = ctx->n_queries > 1 ? B / ctx->n_queries : 0;  // (one query: 0 and null tables)
  if (B <= ctx->Balloc)
  {
    // (stream-ordered and only when the batch size or the query tables change: a synchronous copy is a null-stream operation, which
    //  waits for every other blocking stream of the device - i.e. for the other context's batch still in flight)
    if (ctx->hb.B != B || ctx->hb.seeds_per_query != spq || ctx->hb.q_prob != ctx->d_qprob)
    {
      ctx->hb.B = B;
      ctx->hb.seeds_per_query = spq;
      ctx->hb.q_prob = ctx->d_qprob;
      ctx->hb.q_cp_target = ctx->d_qcp;
      ctx->hb.q_aux1 = ctx->d_qaux1;
      HIPCHK(hipMemcpyAsync(ctx->db, &ctx->hb, sizeof(DevBatch), hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));  // hb is host memory that the next call may modify
    }
    ctx->Bcap = ctx->Balloc;  // (valid again after an invalidation by tmx_queries_set / tmx_query_set_targets)
    return TMX_OK;
  }
  free_pool(ctx->batch_allocs);
  ctx->Bcap = ctx->Balloc = 0;
  const DevProblem& P = ctx->hp;
  DevBatch& H = ctx->hb;
  std::memset(&H, 0, sizeof(H));
  H.B = B;
  H.seeds_per_query = spq;
  H.q_prob = ctx->d_qprob;
  H.q_cp_target = ctx->d_qcp;
  H.q_aux1 = ctx->d_qaux1;
  H.max_rec = ctx->max_rec;
  auto& pool = ctx->batch_allocs;
  tmx_status rc;
  const size_t b = static_cast<size_t>(B);
#define AL(field, count)                                                                                              \
  if ((rc = dalloc(ctx, pool, &H.field, (count))) != TMX_OK)                                                          \
  return rc
  AL(x0, b * P.NX);
  AL(x, b * P.NX);
  AL(xnew, b * P.NX);
  AL(cost_vals, b * P.n_costs);
  AL(cnt_viols, b * P.n_cnts);
  AL(new_cost_vals, b * P.n_costs);
  AL(new_cnt_viols, b * P.n_cnts);
  AL(merit, b * P.n_cnts);
  AL(trust, b);
  AL(total_cost, b);
  AL(prev_rho, b);
  AL(phase, b);
  AL(iter, b);
  AL(merit_inc, b);
  AL(qp_fail, b);
  AL(status, b);
  AL(retval, b);
  AL(n_fe, b);
  AL(n_qp, b);
  AL(cvx, b);
  AL(prev_ok, b);
  AL(active, b * P.R);
  AL(coef, b * P.R * P.D);
  AL(coef2, b * P.n_link * P.D);
  AL(qdyn, b * P.NX);
  AL(rowc, b * P.R);
  AL(solver_init, b);
  AL(rhs, b * P.R);
  AL(dims, b * 4);
  AL(hashes, b * 4);
  AL(prev_dims, b * 4);
  AL(prev_ws, b * 2);
  AL(xq, b * P.n_max);
  AL(yq, b * P.m_max);
  AL(rec_last, b);
  AL(rec_log, b * ctx->max_rec);
  AL(rec_count, b);
  AL(admm_iters, b);
  AL(n_active, 1);
  AL(prof, b * 16);
  AL(sched_state, b);
  AL(sched_done, 1);
  H.step_log_stride = TMX_STEP_LOG_HEAD + 3 * P.n_costs + 4 * P.n_cnts;
  AL(step_log, b * (size_t)H.step_log_stride);
  AL(t_start, 1);
  AL(accept_flag, b);
  if (P.band)
  {
    H.band_stride = (long long)qp_band_doubles(P.D, P.T, P.band_rows ? P.n_link : 0);
    AL(band_ws, b * (size_t)H.band_stride);
  }
  if (P.qp_dense || P.n_fx_cost > 0)
  {
    // quadratic models of the function costs (rebuilt by every convexification): dense engine, or the dynamic objective blocks of the
    // structured solver (QpWs::pb)
    const size_t nfc = (size_t)std::max(1, P.n_fx_cost), dd = (size_t)P.D * P.D;
    AL(fx_H, b * nfc * dd);
    AL(fx_g, b * nfc * (size_t)P.D);
    AL(fx_c, b * nfc);
    AL(fx_W, b * nfc * 2 * dd);
  }
  if (P.qp_dense)
  {
    // dense engine: the QP in CSC form + dense workspace per problem (tmx_generic.h).  Capacity of A: every row slot with all the
    // entries its kind can have (a row on two waypoints: 2 D; a difference row of order 2 / 3 on one joint: 3 / 4 entries, which
    // exceeds 2 D on a one-joint chain), two entries per aux column, one identity entry per variable.
    size_t cap = (size_t)P.n_max + 2 * (size_t)P.NA;
    for (int r = 0; r < P.R; ++r)
      cap += (size_t)std::max(2 * P.D, 4);
    cap += (size_t)P.n_tt * P.T;  // global rows of the TotalTime terms
    if (P.n_max > 4096 || P.m_max > 16384)
    {
      ctx->err = "joint acceleration / jerk terms: the QP is too large for the dense engine (n <= 4096, m <= 16384)";
      return TMX_ERR_UNSUPPORTED;
    }
    H.dq_nnzA = (int)cap;
    // (+ the squared time-parameterised costs: per waypoint the joint diagonals and couplings, two columns of entries in the time
    //  column, its diagonal; a squared TotalTime cost couples all time variables)
    size_t nzp = (size_t)std::max(1, P.nnzP) + (size_t)P.n_fx_cost * P.D * (P.D + 1) / 2;
    if (P.n_tv > 0)
      nzp += (size_t)P.T * (4 * (size_t)P.D + 1);
    for (int k = 0; k < P.n_tt; ++k)
      if (ctx->tt_squared)
      {
        nzp += (size_t)P.T * (P.T + 1) / 2;
        break;
      }
    H.dq_nnzP = (int)nzp;
    AL(dq_Pp, b * (size_t)(P.n_max + 1));
    AL(dq_Pi, b * nzp);
    AL(dq_Px, b * nzp);
    AL(dq_Ap, b * (size_t)(P.n_max + 1));
    AL(dq_Ai, b * cap);
    AL(dq_Ax, b * cap);
    AL(dq_q, b * (size_t)P.n_max);
    AL(dq_l, b * (size_t)P.m_max);
    AL(dq_u, b * (size_t)P.m_max);
    AL(dq_x, b * (size_t)P.n_max);
    AL(dq_y, b * (size_t)P.m_max);
    AL(dq_xw, b * (size_t)P.n_max);
    AL(dq_yw, b * (size_t)P.m_max);
    AL(dq_flags, b * (size_t)P.m_max);
    AL(dq_info, b);
    H.dq_ws_stride = (long long)((gen_ws_doubles(P.n_max, P.m_max) + 1) & ~(size_t)1);
    if (b * (size_t)H.dq_ws_stride * sizeof(double) > ((size_t)200 << 30))
    {
      ctx->err = "joint acceleration / jerk terms: dense workspace of the batch exceeds 200 GiB (reduce the batch)";
      return TMX_ERR_UNSUPPORTED;
    }
    if ((rc = dalloc(ctx, pool, &H.dq_ws, b * (size_t)H.dq_ws_stride, /*zero=*/false)) != TMX_OK)
      return rc;
  }
  if (P.n_tv > 0)
    AL(tv_aff, b * (size_t)P.n_tv * P.T * TMX_TV_REC);
  if (P.n_tt > 0)
    AL(tt_aff, b * (size_t)P.n_tt * (P.T + 1));
  H.tail_flag = ctx->h_tail;  // pinned host memory is device-accessible at the same address (unified addressing)
  H.qp_scratch_stride = (long long)qp_scratch_doubles(P.D, P.T, P.R, P.NA, P.n_link, P.coef_far);
  if (ctx->tt_scratch > 0)  // rank-one terms of TotalTime terms behind everything else (qp_ws_attach_tt)
    H.qp_scratch_stride = (long long)(((qp_scratch_doubles(P.D, P.T, P.R, P.NA, P.n_link, P.coef_far) + 1) & ~(size_t)1) + ctx->tt_scratch);
  if (P.wave_ok)  // the one-wave solver keeps the cold part of the workspace behind the far part (wave_ws_carve)
    H.qp_scratch_stride = (long long)(((qp_far_doubles(P.D, P.T, P.R, P.NA, 0, P.coef_far) + 1) & ~(size_t)1) + qp_glb_doubles(P.D, P.T, P.R, P.NA, 0, P.coef_far) + 8);
  AL(qp_scratch, b * (size_t)H.qp_scratch_stride);
  H.ws_hbm_stride = ctx->ws_in_hbm ? (long long)((ctx->ws_bytes + 15) / 16 * 2) : 0;  // doubles, 16-byte aligned slices
  if (ctx->ws_in_hbm)  // stays nullptr otherwise: the kernels test the pointer
    AL(ws_hbm, b * (size_t)H.ws_hbm_stride);
  H.ws_chain_in_lds = ctx->smem_chain > 0 ? 1 : 0;
#undef AL
  if (!ctx->db)
  {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, sizeof(DevBatch)));
    ctx->db = static_cast<DevBatch*>(p);
  }
  HIPCHK(hipMemcpy(ctx->db, &H, sizeof(DevBatch), hipMemcpyHostToDevice));
  ctx->Bcap = ctx->Balloc = B;
  return TMX_OK;
}

static tmx_status prepare_batch(tmx_ctx* ctx)
{
  ctx->clock_started = false;  // Optimizer::initialize: the next run / launch starts optimize() and its clock
  if (ctx->hull)
    TMX_LAUNCH(k_prepare_hull, ctx->hb.B, ctx->nt_small, ctx->smem_small, ctx->stream, ctx->dp, ctx->db);
  else
    TMX_LAUNCH(k_prepare, ctx->hb.B, ctx->nt_small, ctx->smem_small, ctx->stream, ctx->dp, ctx->db);
  HIPCHK(hipGetLastError());
  return TMX_OK;
}

tmx_status tmx_batch_set_x0(tmx_ctx* ctx, const double* x0_host, int32_t batch)
{
  if (!ctx || !x0_host || batch < 1)
    return TMX_ERR_INVALID;
  if (!ctx->have_problem)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  tmx_status rc = ensure_batch(ctx, batch);
  if (rc != TMX_OK)
    return rc;
  HIPCHK(hipMemcpyAsync(ctx->hb.x0, x0_host, sizeof(double) * (size_t)batch * ctx->hp.NX, hipMemcpyHostToDevice, ctx->stream));
  return prepare_batch(ctx);
}

tmx_status tmx_batch_set_x0_device(tmx_ctx* ctx, const double* x0_dev, int32_t batch)
{
  if (!ctx || !x0_dev || batch < 1)
    return TMX_ERR_INVALID;
  if (!ctx->have_problem)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  tmx_status rc = ensure_batch(ctx, batch);
  if (rc != TMX_OK)
    return rc;
  HIPCHK(hipMemcpyAsync(ctx->hb.x0, x0_dev, sizeof(double) * (size_t)batch * ctx->hp.NX, hipMemcpyDeviceToDevice, ctx->stream));
  return prepare_batch(ctx);
}

static tmx_status read_totals(tmx_ctx* ctx, long long out[4])
{
  HIPCHK(hipMemsetAsync(ctx->d_totals, 0, 4 * sizeof(long long), ctx->stream));
  TMX_LAUNCH(k_count_active, 4, 256, 0, ctx->stream, ctx->db, ctx->d_totals);
  HIPCHK(hipMemcpyAsync(out, ctx->d_totals, 4 * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return TMX_OK;
}

#define TIMED(acc, launches, stmt)                                                                                    \
  do                                                                                                                  \
  {                                                                                                                   \
    if (ctx->timing)                                                                                                  \
      HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));                                                                  \
    stmt;                                                                                                             \
    if (ctx->timing)                                                                                                  \
    {                                                                                                                 \
      HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));                                                                  \
      HIPCHK(hipEventSynchronize(ctx->ev1));                                                                          \
      float ms_ = 0.f;                                                                                                \
      HIPCHK(hipEventElapsedTime(&ms_, ctx->ev0, ctx->ev1));                                                          \
      acc += ms_;                                                                                                     \
      launches;                                                                                                       \
    }                                                                                                                 \
  } while (0)

// Asynchronous half of tmx_sqp_run(ctx, 0, ...): enqueues the whole optimize() of the batch on the context's stream and
// returns.  Two contexts on one device (double-buffered batches) overlap the straggler tail of one batch - the kernel
// time of a batch is set by its longest chain of QP solves, and the persistent workgroups retire as soon as nothing is
// left for them - with the bulk of the next one.
static tmx_status sqp_run_piecewise(tmx_ctx* ctx, int32_t max_steps, int32_t* n_active_out);
tmx_status tmx_sqp_launch(tmx_ctx* ctx)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (!ctx->have_problem || ctx->Bcap == 0 || ctx->pending)
    return TMX_ERR_STATE;
  HIPCHK(hipSetDevice(ctx->device));
  const int B = ctx->hb.B;
  if (ctx->piecewise)
  {
    // the piecewise driver is a host loop: the whole optimize() runs here, tmx_sqp_wait() only collects it
    int32_t left = 0;
    const tmx_status rc = sqp_run_piecewise(ctx, 0, &left);
    if (rc != TMX_OK)
      return rc;
    ctx->pending = 2;
    return TMX_OK;
  }
  if (ctx->mode == 0)
    return TMX_ERR_UNSUPPORTED;  // the piecewise mode runs the loop on the host
  // only the pool kernel reports the start of its tail; the one-workgroup-per-problem kernels free CUs from their first
  // finished problem on, so for them the next batch may be enqueued at once
  *ctx->h_tail = (!ctx->ws_in_hbm && ctx->mode == 2) ? 0 : 1;  // (k_sqp_wave sets the word when its first problem finishes)
  if (!ctx->clock_started)
  {
    TMX_LAUNCH(k_mark_start, 1, 64, 0, ctx->stream, ctx->db);
    ctx->clock_started = true;
  }
  if (ctx->timing)
    HIPCHK(hipEventRecord(ctx->ev0, ctx->stream));
  if (ctx->ws_in_hbm && ctx->n_queries > 1)  // (the one-query kernel carries no multi-query code: sqp_step_block<.., MQ>)
    TMX_LAUNCH(k_sqp_fused_hbm_q, B, ctx->nt_qp > 1 ? TMX_HBM_NT : 1, ctx->smem_chain, ctx->stream, ctx->dp, ctx->db, 0);
  else if (ctx->ws_in_hbm)
    TMX_LAUNCH(k_sqp_fused_hbm, B, ctx->nt_qp > 1 ? TMX_HBM_NT : 1, ctx->smem_chain, ctx->stream, ctx->dp, ctx->db, 0);
#if TMX_IS_DEVICE
  else if (ctx->wave && ctx->mode == 2)
    TMX_LAUNCH(k_sqp_wave, B, TMX_WV_NT, ctx->smem_wave, ctx->stream, ctx->dp, ctx->db, 0);  // a wave pair per problem, all resident at B <= 4 x CUs
#endif
  else if (ctx->mode == 2)
  {
    const int G = std::min(B, ctx->pool_wgs);
    // the scheduler words follow the problem phases (bounded k_sqp_fused calls before this one do not maintain them)
    TMX_LAUNCH(k_pool_sync, 1, 256, 0, ctx->stream, ctx->db);
    if (ctx->band)  // (k_sqp_pool carries no code for banded objectives: qp_solve_block<.., BANDK>)
      TMX_LAUNCH(k_sqp_pool_band, G, ctx->nt_qp, ctx->smem_pool, ctx->stream, ctx->dp, ctx->db);
    else
      TMX_LAUNCH(k_sqp_pool, G, ctx->nt_qp, ctx->smem_pool, ctx->stream, ctx->dp, ctx->db);
  }
  else
    TMX_LAUNCH(k_sqp_fused, B, ctx->nt_qp, ctx->smem_qp, ctx->stream, ctx->dp, ctx->db, 0);
  HIPCHK(hipGetLastError());
  if (ctx->timing)
    HIPCHK(hipEventRecord(ctx->ev1, ctx->stream));
  ctx->pending = 1;
  return TMX_OK;
}

int32_t tmx_sqp_tail_started(const tmx_ctx* ctx)
{
  if (!ctx || !ctx->pending)
    return 1;
  return *static_cast<volatile int*>(ctx->h_tail) != 0 ? 1 : 0;
}

tmx_status tmx_sqp_wait(tmx_ctx* ctx, int32_t* n_active_out)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (!ctx->pending)
    return TMX_ERR_STATE;
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->pending == 2)  // piecewise problem (DevProblem::st): tmx_sqp_launch ran the loop
  {
    long long tot2[4] = { 0, 0, 0, 0 };
    const tmx_status rc2 = read_totals(ctx, tot2);
    if (rc2 != TMX_OK)
      return rc2;
    ctx->pending = 0;
    if (n_active_out)
      *n_active_out = static_cast<int32_t>(tot2[0]);
    return TMX_OK;
  }
  // (pending is cleared only once the launch has been collected: a device error leaves the context in the pending state)
  if (ctx->timing)
  {
    HIPCHK(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->ms_admm += ms;
    ctx->launches_admm++;
  }
  long long tot[4] = { 0, 0, 0, 0 };
  tmx_status rc = read_totals(ctx, tot);  // synchronises the stream
  if (rc != TMX_OK)
    return rc;
  // A run-to-completion launch must leave no problem unfinished.  The pool kernel retires workgroups that find nothing
  // ready; should the last workgroups ever leave with work undone, the scheduler words are rebuilt from the problem phases
  // (k_pool_sync) and the pool is started again - problems are independent, so the results do not depend on it.
  for (int again = 0; tot[0] > 0 && again < 4 && !ctx->ws_in_hbm && ctx->mode == 2 && !ctx->wave; ++again)
  {
    const int G = std::min(ctx->hb.B, ctx->pool_wgs);
    TMX_LAUNCH(k_pool_sync, 1, 256, 0, ctx->stream, ctx->db);
    if (ctx->band)
      TMX_LAUNCH(k_sqp_pool_band, G, ctx->nt_qp, ctx->smem_pool, ctx->stream, ctx->dp, ctx->db);
    else
      TMX_LAUNCH(k_sqp_pool, G, ctx->nt_qp, ctx->smem_pool, ctx->stream, ctx->dp, ctx->db);
    HIPCHK(hipGetLastError());
    ctx->pool_relaunches++;
    if ((rc = read_totals(ctx, tot)) != TMX_OK)
      return rc;
  }
  ctx->pending = 0;
  *ctx->h_tail = 1;
  if (n_active_out)
    *n_active_out = static_cast<int32_t>(tot[0]);
  if (tot[0] > 0)
  {
    ctx->err = "tmx_sqp_wait: the launch ended with unfinished problems (internal error)";
    return TMX_ERR_STATE;
  }
  return TMX_OK;
}

tmx_status tmx_sqp_run(tmx_ctx* ctx, int32_t max_steps, int32_t* n_active_out)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (!ctx->have_problem || ctx->Bcap == 0 || ctx->pending)
    return TMX_ERR_STATE;
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->piecewise)
    return sqp_run_piecewise(ctx, max_steps, n_active_out);
  const int B = ctx->hb.B;
  long long tot[4] = { B, 0, 0, 0 };
  if (ctx->mode != 0)
  {
    if (max_steps == 0)
    {
      tmx_status rc = tmx_sqp_launch(ctx);
      return rc != TMX_OK ? rc : tmx_sqp_wait(ctx, n_active_out);
    }
  }
  if (!ctx->clock_started)
  {
    TMX_LAUNCH(k_mark_start, 1, 64, 0, ctx->stream, ctx->db);
    ctx->clock_started = true;
  }
  if (ctx->mode != 0)
  {
    if (ctx->ws_in_hbm && ctx->n_queries > 1)
      TIMED(ctx->ms_admm, ctx->launches_admm++,
            TMX_LAUNCH(k_sqp_fused_hbm_q, B, ctx->nt_qp > 1 ? TMX_HBM_NT : 1, ctx->smem_chain, ctx->stream, ctx->dp, ctx->db, (int)max_steps));
    else if (ctx->ws_in_hbm)
      TIMED(ctx->ms_admm, ctx->launches_admm++,
            TMX_LAUNCH(k_sqp_fused_hbm, B, ctx->nt_qp > 1 ? TMX_HBM_NT : 1, ctx->smem_chain, ctx->stream, ctx->dp, ctx->db, (int)max_steps));
    else
      TIMED(ctx->ms_admm, ctx->launches_admm++,
            TMX_LAUNCH(k_sqp_fused, B, ctx->nt_qp, ctx->smem_qp, ctx->stream, ctx->dp, ctx->db, (int)max_steps));
    HIPCHK(hipGetLastError());
    tmx_status rc = read_totals(ctx, tot);
    if (rc != TMX_OK)
      return rc;
    if (n_active_out)
      *n_active_out = static_cast<int32_t>(tot[0]);
    return TMX_OK;
  }
  return sqp_run_piecewise(ctx, max_steps, n_active_out);
}

// optimize() as one launch chain per trust-region evaluation (k_convexify -> QP solve -> k_evaluate -> k_sqp_update), the loop on
// the host: driver mode 0, and the only driver of qp_dense problems (k_qp_solve_dense)
static tmx_status sqp_run_piecewise(tmx_ctx* ctx, int32_t max_steps, int32_t* n_active_out)
{
  const int B = ctx->hb.B;
  long long tot[4] = { B, 0, 0, 0 };
  int step = 0;
  if (!ctx->clock_started)
  {
    TMX_LAUNCH(k_mark_start, 1, 64, 0, ctx->stream, ctx->db);
    ctx->clock_started = true;
  }
  while (true)
  {
    tmx_status rc = read_totals(ctx, tot);
    if (rc != TMX_OK)
      return rc;
    if (tot[0] == 0 || (max_steps > 0 && step >= max_steps))
      break;
    // safety net: a run can never need more batched steps than the nested loop bounds of optimize() allow
    const long long cap = (long long)(ctx->hp.sqp.max_merit_coeff_increases + 1) * (ctx->hp.sqp.max_iter + 1) * 16;
    if (step > cap)
    {
      ctx->err = "tmx_sqp_run exceeded the iteration bound of BasicTrustRegionSQP (internal error)";
      return TMX_ERR_STATE;
    }
    TIMED(ctx->ms_convexify, (void)0,
          if (ctx->hull) TMX_LAUNCH(k_convexify_hull, B, ctx->nt_small, ctx->smem_small, ctx->stream, ctx->dp, ctx->db, 0);
          else TMX_LAUNCH(k_convexify, B, ctx->nt_small, ctx->smem_small, ctx->stream, ctx->dp, ctx->db, 0));
    if (ctx->dense)
      TIMED(ctx->ms_admm, ctx->launches_admm++,
            TMX_LAUNCH(k_qp_solve_dense, B, ctx->nt_qp > 1 ? 256 : 1, ctx->smem_small, ctx->stream, ctx->dp, ctx->db, 0));
    else if (ctx->ws_in_hbm)
      TIMED(ctx->ms_admm, ctx->launches_admm++, TMX_LAUNCH(k_qp_solve_hbm, B, ctx->nt_qp > 1 ? TMX_HBM_NT : 1, ctx->smem_chain, ctx->stream, ctx->dp, ctx->db, 0));
#if TMX_IS_DEVICE
    else if (ctx->wave)
      TIMED(ctx->ms_admm, ctx->launches_admm++, TMX_LAUNCH(k_qp_solve_wave, B, TMX_WV_NT, ctx->smem_wave, ctx->stream, ctx->dp, ctx->db, 0));
#endif
    else
      TIMED(ctx->ms_admm, ctx->launches_admm++,
            TMX_LAUNCH(k_qp_solve, B, ctx->nt_qp, ctx->smem_qp, ctx->stream, ctx->dp, ctx->db, 0));
    TIMED(ctx->ms_evaluate, (void)0,
          if (ctx->hull) TMX_LAUNCH(k_evaluate_hull, B, ctx->nt_small, ctx->smem_small, ctx->stream, ctx->dp, ctx->db, 1);
          else TMX_LAUNCH(k_evaluate, B, ctx->nt_small, ctx->smem_small, ctx->stream, ctx->dp, ctx->db, 1));
    // sqp_update_block carves the model values AND the per-slot / velocity-term scratch of evaluate_terms behind them
    TMX_LAUNCH(k_sqp_update, B, 64, ctx->smem_small, ctx->stream, ctx->dp, ctx->db);
    HIPCHK(hipGetLastError());
    ++step;
  }
  if (n_active_out)
    *n_active_out = static_cast<int32_t>(tot[0]);
  return TMX_OK;
}

tmx_status tmx_sqp_results(tmx_ctx* ctx, double* x, int32_t* status, double* total_cost, int32_t* n_func_evals, int32_t* n_qp_solves)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const size_t B = ctx->hb.B;
  tmx_status rc;
  if ((rc = d2h(ctx, x, ctx->hb.x, B * ctx->hp.NX)) != TMX_OK || (rc = d2h(ctx, status, ctx->hb.status, B)) != TMX_OK ||
      (rc = d2h(ctx, total_cost, ctx->hb.total_cost, B)) != TMX_OK || (rc = d2h(ctx, n_func_evals, ctx->hb.n_fe, B)) != TMX_OK ||
      (rc = d2h(ctx, n_qp_solves, ctx->hb.n_qp, B)) != TMX_OK)
    return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return TMX_OK;
}

tmx_status tmx_sqp_counters(tmx_ctx* ctx, int64_t* n_func_evals, int64_t* n_qp_solves, int64_t* n_admm_iters)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  long long tot[4];
  tmx_status rc = read_totals(ctx, tot);
  if (rc != TMX_OK)
    return rc;
  if (n_func_evals)
    *n_func_evals = tot[1];
  if (n_qp_solves)
    *n_qp_solves = tot[2];
  if (n_admm_iters)
    *n_admm_iters = tot[3];
  return TMX_OK;
}

tmx_status tmx_sqp_state(tmx_ctx* ctx, int32_t* sqp_iter, int32_t* merit_increases, double* trust_box_size, int32_t* done)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const size_t B = ctx->hb.B;
  tmx_status rc;
  std::vector<int> phase(done ? B : 0);
  if ((sqp_iter && (rc = d2h(ctx, sqp_iter, ctx->hb.iter, B)) != TMX_OK) ||
      (merit_increases && (rc = d2h(ctx, merit_increases, ctx->hb.merit_inc, B)) != TMX_OK) ||
      (trust_box_size && (rc = d2h(ctx, trust_box_size, ctx->hb.trust, B)) != TMX_OK) ||
      (done && (rc = d2h(ctx, phase.data(), ctx->hb.phase, B)) != TMX_OK))
    return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (done)
    for (size_t b = 0; b < B; ++b)
      done[b] = phase[b] == PHASE_DONE ? 1 : 0;
  return TMX_OK;
}

#if defined(TMX_PROFILE) && !defined(TMX_HOST_EMU)
// profile builds only: cycles of thread 0 in the three parts of the segmented chain sweeps (local sweeps, boundary vectors, spike
// correction) and the number of sweeps, summed over all workgroups since the library was loaded (tools/prof_phases.py)
extern "C" __attribute__((visibility("default"))) int tmx_debug_pspk(long long* out)
{
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pspk_prof), 8 * sizeof(long long)) == hipSuccess ? 0 : 1;
}
#endif
tmx_status tmx_sqp_stop(tmx_ctx* ctx, int32_t problem, int32_t status)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  if (problem < 0 || problem >= ctx->hb.B)
  {
    ctx->err = "tmx_sqp_stop: problem index outside the batch";
    return TMX_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(ctx->device));
  // (between launches: the next run step reads phase / status from HBM; k_pool_sync derives the scheduler state from the phase)
  const int done = PHASE_DONE, st = status;
  HIPCHK(hipMemcpyAsync(ctx->hb.phase + problem, &done, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->hb.status + problem, &st, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return TMX_OK;
}

tmx_status tmx_sqp_step_log(tmx_ctx* ctx, double* out, int32_t* stride_out)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  if (stride_out)
    *stride_out = ctx->hb.step_log_stride;
  tmx_status rc = d2h(ctx, out, ctx->hb.step_log, (size_t)ctx->hb.B * (size_t)ctx->hb.step_log_stride);
  if (rc != TMX_OK)
    return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return TMX_OK;
}

tmx_status tmx_model_values(tmx_ctx* ctx, const double* x_qp, double* model_cost_vals, double* model_cnt_viols)
{
  if (!ctx || !x_qp)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const size_t B = ctx->hb.B;
  // the three staging buffers are released on EVERY exit path (HIPCHK returns early on a device error)
  struct PoolGuard
  {
    std::vector<void*> pool;
    ~PoolGuard() { free_pool(pool); }
  } guard;
  double *d_x = nullptr, *d_c = nullptr, *d_v = nullptr;
  tmx_status rc;
  if ((rc = dalloc(ctx, guard.pool, &d_x, B * ctx->hp.n_max, false)) != TMX_OK || (rc = dalloc(ctx, guard.pool, &d_c, B * ctx->hp.n_costs)) != TMX_OK ||
      (rc = dalloc(ctx, guard.pool, &d_v, B * ctx->hp.n_cnts)) != TMX_OK)
    return rc;
  HIPCHK(hipMemcpyAsync(d_x, x_qp, sizeof(double) * B * ctx->hp.n_max, hipMemcpyHostToDevice, ctx->stream));
  TMX_LAUNCH(k_model_values, ctx->hb.B, ctx->nt_small, ctx->smem_small, ctx->stream, ctx->dp, ctx->db, d_x, d_c, d_v);
  HIPCHK(hipGetLastError());
  if ((rc = d2h(ctx, model_cost_vals, d_c, B * ctx->hp.n_costs)) == TMX_OK)
    rc = d2h(ctx, model_cnt_viols, d_v, B * ctx->hp.n_cnts);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return rc;
}

// The iterate alone: x of every problem is overwritten, NOTHING else changes - the convexification (active rows, coefficients,
// right-hand sides), the loop variables, the warm-start state and the records stay as they are (tmx_batch_set_x0 is
// Optimizer::initialize: it resets all of them).  trajopt_sqp::QPProblem::setVariables (qp_problem.h:44) is this operation:
// TrustRegionSQPSolver calls it with the QP's candidate before the exact evaluation and with the best point before it shrinks the
// box and re-exports the SAME convexification around it (trust_region_sqp_solver.cpp:262-371).
tmx_status tmx_sqp_set_x(tmx_ctx* ctx, const double* x_host)
{
  if (!ctx || !x_host)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(ctx->hb.x, x_host, sizeof(double) * (size_t)ctx->hb.B * ctx->hp.NX, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return TMX_OK;
}

tmx_status tmx_sqp_set_loop_vars(tmx_ctx* ctx, const double* trust_box_size, const double* merit_error_coeffs)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const size_t B = ctx->hb.B;
  if (trust_box_size)
    HIPCHK(hipMemcpyAsync(ctx->hb.trust, trust_box_size, sizeof(double) * B, hipMemcpyHostToDevice, ctx->stream));
  if (merit_error_coeffs && ctx->hp.n_cnts > 0)
    HIPCHK(hipMemcpyAsync(ctx->hb.merit, merit_error_coeffs, sizeof(double) * B * ctx->hp.n_cnts, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return TMX_OK;
}

tmx_status tmx_sqp_qp_records(tmx_ctx* ctx, tmx_qp_record* out, int32_t max_records, int32_t* counts)
{
  if (!ctx || max_records < 0)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const int B = ctx->hb.B;
  std::vector<tmx_qp_record> tmp((size_t)B * ctx->max_rec);
  std::vector<int> cnt(B);
  HIPCHK(hipMemcpy(tmp.data(), ctx->hb.rec_log, tmp.size() * sizeof(tmx_qp_record), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(cnt.data(), ctx->hb.rec_count, B * sizeof(int), hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b)
  {
    if (counts)
      counts[b] = cnt[b];
    if (out)
      for (int k = 0; k < std::min({ cnt[b], (int)max_records, ctx->max_rec }); ++k)
        out[(size_t)b * max_records + k] = tmp[(size_t)b * ctx->max_rec + k];
  }
  return TMX_OK;
}

tmx_status tmx_term_counts(tmx_ctx* ctx, int32_t* n_costs, int32_t* n_cnts, int32_t* n_row_slots)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (!ctx->have_problem)
    return TMX_ERR_STATE;
  if (n_costs)
    *n_costs = ctx->hp.n_costs;
  if (n_cnts)
    *n_cnts = ctx->hp.n_cnts;
  if (n_row_slots)
    *n_row_slots = ctx->hp.R;
  return TMX_OK;
}

tmx_status tmx_evaluate(tmx_ctx* ctx, double* cost_vals, double* cnt_viols)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const size_t B = ctx->hb.B;
  if (ctx->hull)
    TMX_LAUNCH(k_evaluate_hull, ctx->hb.B, ctx->nt_small, ctx->smem_small, ctx->stream, ctx->dp, ctx->db, 0);
  else
    TMX_LAUNCH(k_evaluate, ctx->hb.B, ctx->nt_small, ctx->smem_small, ctx->stream, ctx->dp, ctx->db, 0);
  HIPCHK(hipGetLastError());
  tmx_status rc;
  if ((rc = d2h(ctx, cost_vals, ctx->hb.cost_vals, B * ctx->hp.n_costs)) != TMX_OK ||
      (rc = d2h(ctx, cnt_viols, ctx->hb.cnt_viols, B * ctx->hp.n_cnts)) != TMX_OK)
    return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return TMX_OK;
}

tmx_status tmx_convexify(tmx_ctx* ctx, int32_t* active, double* coef, double* rhs)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const size_t B = ctx->hb.B;
  if (ctx->hull)
    TMX_LAUNCH(k_convexify_hull, ctx->hb.B, ctx->nt_small, ctx->smem_small, ctx->stream, ctx->dp, ctx->db, 1);
  else
    TMX_LAUNCH(k_convexify, ctx->hb.B, ctx->nt_small, ctx->smem_small, ctx->stream, ctx->dp, ctx->db, 1);
  HIPCHK(hipGetLastError());
  tmx_status rc;
  if ((rc = d2h(ctx, active, ctx->hb.active, B * ctx->hp.R)) != TMX_OK ||
      (rc = d2h(ctx, coef, ctx->hb.coef, B * ctx->hp.R * ctx->hp.D)) != TMX_OK ||
      (rc = d2h(ctx, rhs, ctx->hb.rhs, B * ctx->hp.R)) != TMX_OK)
    return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return TMX_OK;
}

tmx_status tmx_workspace_info(tmx_ctx* ctx, int32_t* in_hbm, int64_t* lds_bytes, int64_t* hbm_bytes_per_problem)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (!ctx->have_problem)
    return TMX_ERR_STATE;
  const DevProblem& P = ctx->hp;
  if (in_hbm)
    *in_hbm = ctx->ws_in_hbm ? 1 : 0;
  if (lds_bytes)
    *lds_bytes = static_cast<int64_t>(ctx->ws_in_hbm ? ctx->smem_chain : ctx->smem_pool);
  if (hbm_bytes_per_problem)
    *hbm_bytes_per_problem = static_cast<int64_t>(qp_scratch_doubles(P.D, P.T, P.R, P.NA, P.n_link, P.coef_far) * sizeof(double) + ctx->ws_bytes);
  return TMX_OK;
}

tmx_status tmx_qp_dims(tmx_ctx* ctx, int32_t* n_max, int32_t* m_max)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (!ctx->have_problem)
    return TMX_ERR_STATE;
  if (n_max)
    *n_max = ctx->hp.n_max;
  if (m_max)
    *m_max = ctx->hp.m_max;
  return TMX_OK;
}

tmx_status tmx_export_csc(tmx_ctx* ctx, int32_t problem, int32_t* n, int32_t* m, int32_t* nnzP, int32_t* nnzA, int64_t* P_p,
                          int64_t* P_i, double* P_x, double* q, int64_t* A_p, int64_t* A_i, double* A_x, double* l, double* u)
{
  if (!ctx || !n || !m || !nnzP || !nnzA)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  if (problem < 0 || problem >= ctx->hb.B)
    return TMX_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  const DevProblem& P = ctx->hp;
  // device scratch sized for the worst case
  const size_t nmax = P.n_max, mmax = P.m_max, nzA = (size_t)P.R * (std::max(2 * P.D, 4) + 2) + 2 * nmax + (size_t)P.n_tt * P.T,
               nzP = (size_t)P.nnzP + 1 + (size_t)P.n_fx_cost * P.D * (P.D + 1) / 2 + (P.n_tv > 0 ? (size_t)P.T * (4 * (size_t)P.D + 1) : 0) +
                     (ctx->tt_squared ? (size_t)P.T * (P.T + 1) / 2 : 0);
  std::vector<void*> pool;
  CscOut o{};
  int* d_dims = nullptr;
  unsigned long long* d_hash = nullptr;
  tmx_status rc;
#define AL2(ptr, type, count)                                                                                         \
  if ((rc = dalloc(ctx, pool, reinterpret_cast<type**>(&ptr), (count))) != TMX_OK)                                    \
  {                                                                                                                   \
    free_pool(pool);                                                                                                  \
    return rc;                                                                                                        \
  }
  AL2(o.P_p, long long, nmax + 1);
  AL2(o.P_i, long long, nzP);
  AL2(o.P_x, double, nzP);
  AL2(o.q, double, nmax);
  AL2(o.A_p, long long, nmax + 1);
  AL2(o.A_i, long long, nzA);
  AL2(o.A_x, double, nzA);
  AL2(o.l, double, mmax);
  AL2(o.u, double, mmax);
  AL2(d_dims, int, 4);
  AL2(d_hash, unsigned long long, 4);
#undef AL2
  TMX_LAUNCH(k_export_csc, 1, ctx->nt_small, ctx->smem_small, ctx->stream, ctx->dp, ctx->db, (int)problem, o, d_dims, d_hash);
  int dims[4];
  hipError_t e = hipMemcpy(dims, d_dims, sizeof(dims), hipMemcpyDeviceToHost);
  if (e != hipSuccess)
  {
    free_pool(pool);
    ctx->err = "export copy failed";
    return TMX_ERR_DEVICE;
  }
  *n = dims[0];
  *m = dims[1];
  *nnzP = dims[2];
  *nnzA = dims[3];
  auto cp = [&](void* dst, const void* src, size_t bytes) {
    if (dst)
      (void)hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
  };
  cp(P_p, o.P_p, sizeof(long long) * (dims[0] + 1));
  cp(P_i, o.P_i, sizeof(long long) * dims[2]);
  cp(P_x, o.P_x, sizeof(double) * dims[2]);
  cp(q, o.q, sizeof(double) * dims[0]);
  cp(A_p, o.A_p, sizeof(long long) * (dims[0] + 1));
  cp(A_i, o.A_i, sizeof(long long) * dims[3]);
  cp(A_x, o.A_x, sizeof(double) * dims[3]);
  cp(l, o.l, sizeof(double) * dims[1]);
  cp(u, o.u, sizeof(double) * dims[1]);
  free_pool(pool);
  return TMX_OK;
}

tmx_status tmx_qp_solve(tmx_ctx* ctx, double* x_qp, int32_t* cvx_status, tmx_qp_record* rec)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const size_t B = ctx->hb.B;
  if (ctx->dense)
    TIMED(ctx->ms_admm, ctx->launches_admm++,
          TMX_LAUNCH(k_qp_solve_dense, ctx->hb.B, ctx->nt_qp > 1 ? 256 : 1, ctx->smem_small, ctx->stream, ctx->dp, ctx->db, 1));
  else if (ctx->ws_in_hbm)
    TIMED(ctx->ms_admm, ctx->launches_admm++, TMX_LAUNCH(k_qp_solve_hbm, ctx->hb.B, ctx->nt_qp > 1 ? TMX_HBM_NT : 1, ctx->smem_chain, ctx->stream, ctx->dp, ctx->db, 1));
#if TMX_IS_DEVICE
  else if (ctx->wave)
    TIMED(ctx->ms_admm, ctx->launches_admm++, TMX_LAUNCH(k_qp_solve_wave, ctx->hb.B, TMX_WV_NT, ctx->smem_wave, ctx->stream, ctx->dp, ctx->db, 1));
#endif
  else
    TIMED(ctx->ms_admm, ctx->launches_admm++,
          TMX_LAUNCH(k_qp_solve, ctx->hb.B, ctx->nt_qp, ctx->smem_qp, ctx->stream, ctx->dp, ctx->db, 1));
  HIPCHK(hipGetLastError());
  tmx_status rc;
  if ((rc = d2h(ctx, x_qp, ctx->hb.xq, B * ctx->hp.n_max)) != TMX_OK || (rc = d2h(ctx, cvx_status, ctx->hb.cvx, B)) != TMX_OK ||
      (rc = d2h(ctx, rec, ctx->hb.rec_last, B)) != TMX_OK)
    return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return TMX_OK;
}

tmx_status tmx_qp_solve_batched(tmx_ctx* ctx, const tmx_qp_csc* qps, int32_t batch, const tmx_osqp_settings* settings, double* x,
                                double* y, int32_t* cvx_status, tmx_qp_info* info, int32_t* active_flags)
{
  if (!ctx || !qps || batch < 1 || !x || !y)
    return TMX_ERR_INVALID;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  tmx_osqp_settings st;
  if (settings)
    st = *settings;
  else
    tmx_default_osqp_settings(&st);
  // pack the batch: one contiguous host image per array kind, offsets per problem
  std::vector<GenQp> g((size_t)batch);
  std::vector<long long> Pp, Pi, Ap, Ai;
  std::vector<double> Px, Ax, q, l, u, xw, yw;
  long long ows = 0;
  // block-tridiagonal engine (tmx_csc_blocks.h): the QPs it takes, their row-wise copies of P and A and their orderings
  const int engine = ctx->qp_engine;
  const int dense_limit = engine == TMX_QP_ENGINE_AUTO ? UploadHooks::read().dense_qp_max_n : 0;
  std::vector<CbQp> cb;
  std::vector<int> cPrp, cPrj, cPrk, cArp, cArj, cArk, cperm, cpos;
  std::vector<int> last_engine((size_t)batch, TMX_QP_ENGINE_DENSE), last_block((size_t)batch, 0), last_nblocks((size_t)batch, 0), last_place((size_t)batch, 0);
  const char* cb_min_env = std::getenv("TMX_CB_BLOCK_MIN");  // tuning hook: smallest block size of the partition (default TMX_CB_NB_MIN)
  const int cb_min_block = cb_min_env ? std::max(1, std::atoi(cb_min_env)) : 0;
  CscPartition part;
  int part_of = -1;  // the QP `part` was computed for
  size_t cb_smem = 0;
  for (int b = 0; b < batch; ++b)
  {
    const tmx_qp_csc& Q = qps[b];
    if (Q.n < 1 || Q.m < 0 || !Q.P_p || !Q.q || !Q.A_p || (Q.m > 0 && (!Q.l || !Q.u)) || ((Q.x_warm == nullptr) != (Q.y_warm == nullptr)))
    {
      ctx->err = "tmx_qp_solve_batched: malformed tmx_qp_csc";
      return TMX_ERR_INVALID;
    }
    if (Q.n > 4096 || Q.m > 16384)
    {
      ctx->err = "tmx_qp_solve_batched: QP too large for the generic (dense) path";
      return TMX_ERR_UNSUPPORTED;
    }
    const long long nzP = Q.P_p[Q.n], nzA = Q.A_p[Q.n];
    if (nzP < 0 || nzA < 0 || (nzP > 0 && (!Q.P_i || !Q.P_x)) || (nzA > 0 && (!Q.A_i || !Q.A_x)))
    {
      ctx->err = "tmx_qp_solve_batched: malformed CSC arrays";
      return TMX_ERR_INVALID;
    }
    // what osqp_setup's validate_data rejects (OSQP_DATA_VALIDATION_ERROR): column pointers that do not start at 0 or decrease
    // (the kernel walks p = P_p[j] .. P_p[j+1] over device memory), row indices out of range, a P that is not upper
    // triangular (the kernel mirrors the strict upper triangle: a full symmetric P would be counted twice), l > u, NaN
    if (Q.P_p[0] != 0 || Q.A_p[0] != 0)
    {
      ctx->err = "tmx_qp_solve_batched: CSC column pointers must start at 0";
      return TMX_ERR_INVALID;
    }
    for (int j = 0; j < Q.n; ++j)
    {
      if (Q.P_p[j] > Q.P_p[j + 1] || Q.P_p[j + 1] > nzP || Q.A_p[j] > Q.A_p[j + 1] || Q.A_p[j + 1] > nzA)
      {
        ctx->err = "tmx_qp_solve_batched: CSC column pointers must be non-decreasing and end at nnz";
        return TMX_ERR_INVALID;
      }
      for (long long p = Q.P_p[j]; p < Q.P_p[j + 1]; ++p)
      {
        if (Q.P_i[p] < 0 || Q.P_i[p] >= Q.n)
        {
          ctx->err = "tmx_qp_solve_batched: P row index out of range";
          return TMX_ERR_INVALID;
        }
        if (Q.P_i[p] > j)
        {
          ctx->err = "tmx_qp_solve_batched: P must be given by its upper triangle (OSQP_DATA_VALIDATION_ERROR)";
          return TMX_ERR_INVALID;
        }
        if (std::isnan(Q.P_x[p]))
        {
          ctx->err = "tmx_qp_solve_batched: NaN in P";
          return TMX_ERR_INVALID;
        }
      }
      if (std::isnan(Q.q[j]))
      {
        ctx->err = "tmx_qp_solve_batched: NaN in q";
        return TMX_ERR_INVALID;
      }
    }
    for (long long p = 0; p < nzA; ++p)
      if (Q.A_i[p] < 0 || Q.A_i[p] >= Q.m || std::isnan(Q.A_x[p]))
      {
        ctx->err = "tmx_qp_solve_batched: A row index out of range (or NaN entry)";
        return TMX_ERR_INVALID;
      }
    for (int i = 0; i < Q.m; ++i)
      if (!(Q.l[i] <= Q.u[i]))  // also false for a NaN bound
      {
        ctx->err = "tmx_qp_solve_batched: lower bound above upper bound or NaN bound (OSQP_DATA_VALIDATION_ERROR)";
        return TMX_ERR_INVALID;
      }
    GenQp& gq = g[(size_t)b];
    gq.n = Q.n;
    gq.m = Q.m;
    gq.oP = (long long)Pi.size();
    gq.oA = (long long)Ai.size();
    gq.oPp = (long long)Pp.size();
    gq.oAp = (long long)Ap.size();
    gq.ov_n = (long long)q.size();
    gq.ov_m = (long long)l.size();
    gq.ows = ows;
    gq.warm = (Q.x_warm != nullptr && st.warm_starting) ? 1 : 0;
    bool blocks = false;
    if (engine != TMX_QP_ENGINE_DENSE && !(engine == TMX_QP_ENGINE_AUTO && Q.n <= dense_limit))
    {
      // ordering and partition from the pattern arrays; skipped when they equal those of the QP before
      bool same = part_of >= 0 && qps[part_of].n == Q.n && qps[part_of].m == Q.m;
      if (same)
      {
        const tmx_qp_csc& R = qps[part_of];
        same = std::equal(Q.P_p, Q.P_p + Q.n + 1, R.P_p) && std::equal(Q.A_p, Q.A_p + Q.n + 1, R.A_p) &&
               std::equal(Q.P_i, Q.P_i + nzP, R.P_i) && std::equal(Q.A_i, Q.A_i + nzA, R.A_i);
      }
      if (!same)
        part = csc_partition(Q.n, Q.m, Q.P_p, Q.P_i, Q.A_p, Q.A_i, cb_min_block);
      part_of = b;
      if (engine == TMX_QP_ENGINE_BLOCKS && !part.fits)
      {
        ctx->err = "tmx_qp_solve_batched: QP " + std::to_string(b) + " does not fit the block-tridiagonal engine: " + part.reason;
        return TMX_ERR_UNSUPPORTED;
      }
      blocks = part.fits && (engine == TMX_QP_ENGINE_BLOCKS || part.profitable);
    }
    if (blocks)
    {
      CbQp c{};
      c.n = Q.n;
      c.m = Q.m;
      c.nb = part.nb;
      c.nblk = part.n_blocks;
      c.place = part.placement;
      c.warm = gq.warm;
      c.slot = b;
      c.oP = gq.oP;
      c.oA = gq.oA;
      c.oPp = gq.oPp;
      c.oAp = gq.oAp;
      c.ov_n = gq.ov_n;
      c.ov_m = gq.ov_m;
      c.ows = ows;
      c.oPr = (long long)cPrj.size();
      c.oPrp = (long long)cPrp.size();
      c.oAr = (long long)cArj.size();
      c.oArp = (long long)cArp.size();
      c.operm = (long long)cperm.size();
      ows += (long long)((cb_ws_doubles(Q.n, Q.m, part.nb, part.n_blocks, nzP, nzA) + 1) & ~(size_t)1);
      csc_rows(Q.n, Q.n, Q.P_p, Q.P_i, /*skip_diagonal=*/true, cPrp, cPrj, cPrk);
      csc_rows(Q.m, Q.n, Q.A_p, Q.A_i, /*skip_diagonal=*/false, cArp, cArj, cArk);
      cperm.insert(cperm.end(), part.perm.begin(), part.perm.end());
      cpos.insert(cpos.end(), part.pos.begin(), part.pos.end());
      cb.push_back(c);
      last_engine[(size_t)b] = TMX_QP_ENGINE_BLOCKS;
      last_block[(size_t)b] = part.nb;
      last_nblocks[(size_t)b] = part.n_blocks;
      last_place[(size_t)b] = part.placement;
      // LDS: the fixed part, then the two tiles of a factor step (placement 1) or, in the same place, the partial sums of a sweep step
      cb_smem = std::max(cb_smem, (size_t)TMX_CB_LDS_FIXED + std::max(part.placement == TMX_CB_PLACE_LDS ? 2 * (size_t)part.nb * part.nb : (size_t)0,
                                                                       2 * (size_t)TMX_CB_PARTS * part.nb));
    }
    else
      ows += (long long)((gen_ws_doubles(Q.n, Q.m) + 1) & ~(size_t)1);
    Pp.insert(Pp.end(), Q.P_p, Q.P_p + Q.n + 1);
    Ap.insert(Ap.end(), Q.A_p, Q.A_p + Q.n + 1);
    Pi.insert(Pi.end(), Q.P_i, Q.P_i + nzP);
    Px.insert(Px.end(), Q.P_x, Q.P_x + nzP);
    Ai.insert(Ai.end(), Q.A_i, Q.A_i + nzA);
    Ax.insert(Ax.end(), Q.A_x, Q.A_x + nzA);
    q.insert(q.end(), Q.q, Q.q + Q.n);
    l.insert(l.end(), Q.l, Q.l + Q.m);
    u.insert(u.end(), Q.u, Q.u + Q.m);
    for (int j = 0; j < Q.n; ++j)
      xw.push_back(Q.x_warm ? Q.x_warm[j] : 0.0);
    for (int i = 0; i < Q.m; ++i)
      yw.push_back(Q.y_warm ? Q.y_warm[i] : 0.0);
  }
  if ((size_t)ows * sizeof(double) > ((size_t)16 << 30))
  {
    ctx->err = "tmx_qp_solve_batched: dense workspace of the batch exceeds 16 GiB";
    return TMX_ERR_UNSUPPORTED;
  }
  std::vector<void*> pool;
  GenData D{};
  GenQp* d_g = nullptr;
  tmx_status rc = TMX_OK;
  auto up = [&](auto** dst, const auto& vec) { return rc == TMX_OK ? (rc = upload(ctx, pool, dst, vec)) : rc; };
  long long *dPp = nullptr, *dPi = nullptr, *dAp = nullptr, *dAi = nullptr;
  double *dPx = nullptr, *dAx = nullptr, *dq = nullptr, *dl = nullptr, *du = nullptr, *dxw = nullptr, *dyw = nullptr;
  up(&d_g, g);
  up(&dPp, Pp);
  up(&dPi, Pi);
  up(&dAp, Ap);
  up(&dAi, Ai);
  up(&dPx, Px);
  up(&dAx, Ax);
  up(&dq, q);
  up(&dl, l);
  up(&du, u);
  up(&dxw, xw);
  up(&dyw, yw);
  int* d_flags = nullptr;
  if (rc == TMX_OK)
    rc = dalloc(ctx, pool, &D.x_out, q.size());
  if (rc == TMX_OK)
    rc = dalloc(ctx, pool, &D.y_out, l.size());
  if (rc == TMX_OK)
    rc = dalloc(ctx, pool, &d_flags, l.size());
  if (rc == TMX_OK)
    rc = dalloc(ctx, pool, &D.info, (size_t)batch);
  if (rc == TMX_OK)
    rc = dalloc(ctx, pool, &D.ws, (size_t)ows, /*zero=*/false);  // k_qp_generic zero-fills the dense P / A it builds itself
  if (rc != TMX_OK)
  {
    free_pool(pool);
    return rc;
  }
  D.P_p = dPp;
  D.P_i = dPi;
  D.A_p = dAp;
  D.A_i = dAi;
  D.P_x = dPx;
  D.A_x = dAx;
  D.q = dq;
  D.l = dl;
  D.u = du;
  D.xw = dxw;
  D.yw = dyw;
  D.flags_out = d_flags;
  std::vector<tmx_qp_info> hinfo((size_t)batch);
  std::vector<int> dslot;  // mixed batch: the caller's index of every QP of the dense launch, and that launch's info records
  tmx_qp_info* d_dinfo = nullptr;
  hipError_t e = hipSuccess;
#if TMX_CB_PROF
  int cb_prof_slots = 0;
  long long* cb_prof_dev = nullptr;
#endif
  if (cb.empty())
    TMX_LAUNCH(k_qp_generic, batch, ctx->nt_qp > 1 ? 256 : 1, 320 * sizeof(double), ctx->stream, d_g, D, st);
  else
  {
    // one launch per engine.  Both kernels write x, y and the flags at the QP's own offsets of the caller's order; the dense
    // kernel indexes its info records by workgroup, so its QPs get a compact list and their records are scattered below.
    std::vector<GenQp> gd;
    for (int b = 0; b < batch; ++b)
      if (last_engine[(size_t)b] == TMX_QP_ENGINE_DENSE)
      {
        gd.push_back(g[(size_t)b]);
        dslot.push_back(b);
      }
    CbData C{};
    CbQp* d_cb = nullptr;
    GenQp* d_gd = nullptr;
    int *dPrp = nullptr, *dPrj = nullptr, *dPrk = nullptr, *dArp = nullptr, *dArj = nullptr, *dArk = nullptr, *dperm = nullptr, *dpos = nullptr;
    up(&d_cb, cb);
    up(&dPrp, cPrp);
    up(&dPrj, cPrj);
    up(&dPrk, cPrk);
    up(&dArp, cArp);
    up(&dArj, cArj);
    up(&dArk, cArk);
    up(&dperm, cperm);
    up(&dpos, cpos);
    if (!gd.empty())
    {
      up(&d_gd, gd);
      if (rc == TMX_OK)
        rc = dalloc(ctx, pool, &d_dinfo, gd.size());
    }
    if (rc != TMX_OK)
    {
      free_pool(pool);
      return rc;
    }
    C.g = D;
    C.Prp = dPrp;
    C.Prj = dPrj;
    C.Prk = dPrk;
    C.Arp = dArp;
    C.Arj = dArj;
    C.Ark = dArk;
    C.perm = dperm;
    C.pos = dpos;
#if TMX_CB_PROF
    if ((rc = dalloc(ctx, pool, &C.prof, (size_t)batch * 8)) != TMX_OK)
    {
      free_pool(pool);
      return rc;
    }
    long long* const d_prof = C.prof;
    cb_prof_slots = batch;
    cb_prof_dev = d_prof;
#endif
#ifndef TMX_HOST_EMU
    if (cb_smem * sizeof(double) > 48 * 1024)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_qp_csc_blocks), hipFuncAttributeMaxDynamicSharedMemorySize,
                              static_cast<int>(cb_smem * sizeof(double)));
#endif
    if (e == hipSuccess)
      TMX_LAUNCH(k_qp_csc_blocks, (int)cb.size(), ctx->nt_qp > 1 ? 256 : 1, cb_smem * sizeof(double), ctx->stream, d_cb, C, st);
    if (e == hipSuccess && !gd.empty())
    {
      GenData Dd = D;
      Dd.info = d_dinfo;
      TMX_LAUNCH(k_qp_generic, (int)gd.size(), ctx->nt_qp > 1 ? 256 : 1, 320 * sizeof(double), ctx->stream, d_gd, Dd, st);
    }
  }
  if (e == hipSuccess)
    e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess)
    e = hipGetLastError();
  if (e == hipSuccess)
    e = hipMemcpy(x, D.x_out, sizeof(double) * q.size(), hipMemcpyDeviceToHost);
  if (e == hipSuccess && !l.empty())
    e = hipMemcpy(y, D.y_out, sizeof(double) * l.size(), hipMemcpyDeviceToHost);
  if (e == hipSuccess)
    e = hipMemcpy(hinfo.data(), D.info, sizeof(tmx_qp_info) * batch, hipMemcpyDeviceToHost);
#if TMX_CB_PROF
  if (e == hipSuccess && cb_prof_dev)
  {
    // profiling build: ticks of 10 ns per QP of the block-tridiagonal engine, to stderr
    std::vector<long long> hp((size_t)cb_prof_slots * 8);
    e = hipMemcpy(hp.data(), cb_prof_dev, sizeof(long long) * hp.size(), hipMemcpyDeviceToHost);
    for (int b = 0; b < cb_prof_slots; ++b)
      if (last_engine[(size_t)b] == TMX_QP_ENGINE_BLOCKS)
      {
        const long long* t = &hp[(size_t)b * 8];
        std::fprintf(stderr, "cb_prof qp %d admm_assembly %lld admm_factor %lld admm_sweeps %lld polish_total %lld polish_assembly %lld polish_factor %lld polish_sweeps %lld total %lld\n",
                     b, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
      }
  }
#endif
  if (e == hipSuccess && !dslot.empty())
  {
    std::vector<tmx_qp_info> dinfo(dslot.size());
    e = hipMemcpy(dinfo.data(), d_dinfo, sizeof(tmx_qp_info) * dslot.size(), hipMemcpyDeviceToHost);
    for (size_t k = 0; k < dslot.size(); ++k)
      hinfo[(size_t)dslot[k]] = dinfo[k];
  }
  if (e == hipSuccess && active_flags && !l.empty())
    e = hipMemcpy(active_flags, d_flags, sizeof(int) * l.size(), hipMemcpyDeviceToHost);
  free_pool(pool);
  if (e != hipSuccess)
  {
    ctx->err = std::string("tmx_qp_solve_batched: ") + hipGetErrorString(e);
    return TMX_ERR_DEVICE;
  }
  ctx->qp_last_engine = last_engine;
  ctx->qp_last_block = last_block;
  ctx->qp_last_nblocks = last_nblocks;
  ctx->qp_last_place = last_place;
  for (int b = 0; b < batch; ++b)
  {
    const int s = hinfo[(size_t)b].osqp_status;
    if (info)
      info[b] = hinfo[(size_t)b];
    if (cvx_status)  // OSQPModel::optimize, osqp_interface.cpp:565-614
      cvx_status[b] = (s == 1 || s == 2) ? TMX_CVX_SOLVED : ((s == 3 || s == 4 || s == 5 || s == 6) ? TMX_CVX_INFEASIBLE : TMX_CVX_FAILED);
  }
  return TMX_OK;
}

tmx_status tmx_qp_engine_set(tmx_ctx* ctx, int32_t engine)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  TMX_REFUSE_WHILE_PENDING(ctx);
  if (engine != TMX_QP_ENGINE_DENSE && engine != TMX_QP_ENGINE_AUTO && engine != TMX_QP_ENGINE_BLOCKS)
  {
    ctx->err = "tmx_qp_engine_set: engine must be TMX_QP_ENGINE_DENSE, _AUTO or _BLOCKS";
    return TMX_ERR_INVALID;
  }
  ctx->qp_engine = engine;
  return TMX_OK;
}

tmx_status tmx_qp_engine_last(tmx_ctx* ctx, int32_t batch, int32_t* engine_out, int32_t* block_out, int32_t* n_blocks_out, int32_t* placement_out)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  TMX_REFUSE_WHILE_PENDING(ctx);
  if (batch < 1 || (size_t)batch != ctx->qp_last_engine.size())
  {
    ctx->err = "tmx_qp_engine_last: batch differs from the last tmx_qp_solve_batched (" + std::to_string(ctx->qp_last_engine.size()) + " QPs)";
    return TMX_ERR_INVALID;
  }
  for (int b = 0; b < batch; ++b)
  {
    if (engine_out)
      engine_out[b] = ctx->qp_last_engine[(size_t)b];
    if (block_out)
      block_out[b] = ctx->qp_last_block[(size_t)b];
    if (n_blocks_out)
      n_blocks_out[b] = ctx->qp_last_nblocks[(size_t)b];
    if (placement_out)
      placement_out[b] = ctx->qp_last_place[(size_t)b];
  }
  return TMX_OK;
}

tmx_status tmx_qp_duals(tmx_ctx* ctx, double* y_qp)
{
  if (!ctx || !y_qp)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  tmx_status rc = d2h(ctx, y_qp, ctx->hb.yq, (size_t)ctx->hb.B * ctx->hp.m_max);
  if (rc != TMX_OK)
    return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return TMX_OK;
}

tmx_status tmx_qp_active_set(tmx_ctx* ctx, int32_t* flags)
{
  if (!ctx || !flags)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const size_t count = (size_t)ctx->hb.B * ctx->hp.m_max;
  std::vector<void*> pool;
  int* d_out = nullptr;
  tmx_status rc = dalloc(ctx, pool, &d_out, count);
  if (rc != TMX_OK)
    return rc;
  TMX_LAUNCH(k_export_active, ctx->hb.B, 256, 0, ctx->stream, ctx->dp, ctx->db, d_out);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpy(flags, d_out, sizeof(int) * count, hipMemcpyDeviceToHost);
  free_pool(pool);
  if (e != hipSuccess)
  {
    ctx->err = std::string("tmx_qp_active_set: ") + hipGetErrorString(e);
    return TMX_ERR_DEVICE;
  }
  return TMX_OK;
}

static tmx_status ensure_pairs(tmx_ctx* ctx, int n_ranks)
{
  if (ctx->d_pair && ctx->pair_cap >= n_ranks)
    return TMX_OK;
  if (ctx->d_pair)
    (void)hipFree(ctx->d_pair);
  ctx->d_pair = nullptr;
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, sizeof(double) * (2 + 2 * (size_t)n_ranks)));
  ctx->d_pair = static_cast<double*>(p);
  ctx->pair_cap = n_ranks;
  return TMX_OK;
}

tmx_status tmx_argmin(tmx_ctx* ctx, int64_t global_offset, int64_t* best_index, double* best_cost)
{
  if (!ctx || !best_index || !best_cost)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  int nranks = 1;
#ifndef TMX_HOST_EMU
  ncclComm_t comm = static_cast<ncclComm_t>(ctx->nccl);
  if (comm && ncclCommCount(comm, &nranks) != ncclSuccess)
    return TMX_ERR_NCCL;
#endif
  tmx_status rc = ensure_pairs(ctx, nranks);
  if (rc != TMX_OK)
    return rc;
  // local argmin on the device (one workgroup), then - with a communicator - the only collective on the path: an
  // all-gather of one (cost, index) pair per rank (16 bytes each) and an argmin over the n_ranks pairs
  const int conv = ctx->hp.flavor == TMX_FLAVOR_SQP ? (int)TMX_SQP_CONVERGED : (int)TMX_OPT_CONVERGED;
  const int nt = ctx->nt_qp > 1 ? 256 : 1;
  TMX_LAUNCH(k_argmin, 1, nt, (size_t)nt * 16, ctx->stream, ctx->db, conv, (long long)global_offset, ctx->d_pair);
  HIPCHK(hipGetLastError());
  std::vector<double> all(2 * (size_t)nranks);
#ifndef TMX_HOST_EMU
  if (comm)
  {
    if (ncclAllGather(ctx->d_pair, ctx->d_pair + 2, 2, ncclDouble, comm, ctx->stream) != ncclSuccess)
    {
      ctx->err = "ncclAllGather failed";
      return TMX_ERR_NCCL;
    }
    HIPCHK(hipMemcpyAsync(all.data(), ctx->d_pair + 2, sizeof(double) * 2 * nranks, hipMemcpyDeviceToHost, ctx->stream));
  }
  else
#endif
    HIPCHK(hipMemcpyAsync(all.data(), ctx->d_pair, sizeof(double) * 2, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  double bc = 1e300;
  long long bi = -1;
  int owner = -1;
  for (int r = 0; r < nranks; ++r)
    if (all[2 * r + 1] >= 0 && (all[2 * r] < bc || (all[2 * r] == bc && (bi < 0 || (long long)all[2 * r + 1] < bi))))
    {
      bc = all[2 * r];
      bi = static_cast<long long>(all[2 * r + 1]);
      owner = r;
    }
  *best_index = bi;
  *best_cost = bc;
  ctx->best_owner = owner;
  ctx->best_nranks = nranks;
  ctx->best_global = bi;
  ctx->best_local = bi >= 0 ? bi - (long long)global_offset : -1;  // meaningful on the owner rank only
  return TMX_OK;
}

// The optional last step of SURVEY.md section 8(e): the winning trajectory (T x D doubles, 1.7 KB for config 1) goes from its owner
// rank to every rank - one ncclBroadcast on the library's communicator, latency-bound; without a communicator (one rank) a copy.
tmx_status tmx_best_trajectory(tmx_ctx* ctx, double* x_out, int32_t* owner_rank)
{
  if (!ctx || !x_out)
    return TMX_ERR_INVALID;
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  if (owner_rank)
    *owner_rank = ctx->best_owner;
  if (ctx->best_owner < 0)
  {
    ctx->err = "tmx_best_trajectory: the last tmx_argmin found no converged seed on any rank (or tmx_argmin was not called)";
    return TMX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(ctx->device));
  const size_t NX = (size_t)ctx->hp.NX;
  if (ctx->best_cap < NX + 1)
  {
    if (ctx->d_best)
      (void)hipFree(ctx->d_best);
    ctx->d_best = nullptr;
    ctx->best_cap = 0;
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, sizeof(double) * (NX + 1)));
    HIPCHK(hipMemset(p, 0xFF, sizeof(double) * (NX + 1)));  // (a status word that was never written reads as not-valid)
    ctx->d_best = static_cast<double*>(p);
    ctx->best_cap = NX + 1;
  }
  int my_rank = 0;
#ifndef TMX_HOST_EMU
  ncclComm_t comm = static_cast<ncclComm_t>(ctx->nccl);
  if (comm && ncclCommUserRank(comm, &my_rank) != ncclSuccess)
    return TMX_ERR_NCCL;
#endif
  // The call is COLLECTIVE: every rank enters the broadcast whatever it finds locally.  The message is the trajectory plus ONE status
  // word behind it (0 = valid, 1 = the owner's winning index is not in its shard: global_offset of tmx_argmin inconsistent across
  // ranks) - an owner that cannot send the trajectory still takes part, so no rank is left blocked in ncclBroadcast, and every rank
  // reads the same verdict from the word, not from the payload.
  // (a device error on the owner before the broadcast is kept in owner_err and returned AFTER the collective, for the same reason)
  hipError_t owner_err = hipSuccess;
  if (my_rank == ctx->best_owner)
  {
    const bool owner_bad = ctx->best_local < 0 || ctx->best_local >= (long long)ctx->hb.B;
    const double word = owner_bad ? 1.0 : 0.0;
    owner_err = owner_bad ? hipMemsetAsync(ctx->d_best, 0, sizeof(double) * NX, ctx->stream) :
                            hipMemcpyAsync(ctx->d_best, ctx->hb.x + (size_t)ctx->best_local * NX, sizeof(double) * NX, hipMemcpyDeviceToDevice, ctx->stream);
    if (owner_err == hipSuccess)
      owner_err = hipMemcpyAsync(ctx->d_best + NX, &word, sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    const hipError_t se = hipStreamSynchronize(ctx->stream);  // (the staging word dies with this scope)
    if (owner_err == hipSuccess)
      owner_err = se;
  }
#ifndef TMX_HOST_EMU
  if (comm && ctx->best_nranks > 1 &&
      ncclBroadcast(ctx->d_best, ctx->d_best, NX + 1, ncclDouble, ctx->best_owner, comm, ctx->stream) != ncclSuccess)
  {
    ctx->err = "ncclBroadcast failed";
    return TMX_ERR_NCCL;
  }
#endif
  if (owner_err != hipSuccess)
  {
    ctx->err = std::string("tmx_best_trajectory: ") + hipGetErrorString(owner_err);
    return TMX_ERR_DEVICE;
  }
  double word_in = 1.0;
  HIPCHK(hipMemcpyAsync(x_out, ctx->d_best, sizeof(double) * NX, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(&word_in, ctx->d_best + NX, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (word_in != 0.0)
  {
    ctx->err = "tmx_best_trajectory: the winning index is not in the owner rank's shard (global_offset of tmx_argmin inconsistent across ranks)";
    return TMX_ERR_STATE;
  }
  return TMX_OK;
}

// ---- multi-query batches (include/tmx.h) ----

// the Q copies of the DevProblem: the uploaded one with cp_target / slot_aux1 pointing at the query's tables (DevBatch::q_prob)
static tmx_status sync_query_problems(tmx_ctx* ctx)
{
  if (ctx->n_queries <= 1 || !ctx->d_qprob)
    return TMX_OK;
  std::vector<DevProblem> qp((size_t)ctx->n_queries, ctx->hp);
  for (int q = 0; q < ctx->n_queries; ++q)
  {
    qp[(size_t)q].cp_target = ctx->d_qcp + (size_t)q * ctx->hp.n_cp * 12;
    qp[(size_t)q].slot_aux1 = ctx->d_qaux1 + (size_t)q * ctx->hp.R;
  }
  HIPCHK(hipMemcpy(ctx->d_qprob, qp.data(), qp.size() * sizeof(DevProblem), hipMemcpyHostToDevice));
  return TMX_OK;
}

// the current batch was prepared (first exact evaluation) with other targets: nothing runs or reads it until the next tmx_batch_set_x0*
static void invalidate_batch(tmx_ctx* ctx) { ctx->Bcap = 0; }

tmx_status tmx_queries_set(tmx_ctx* ctx, int32_t n_queries)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (n_queries < 1)
  {
    ctx->err = "tmx_queries_set: n_queries must be at least 1";
    return TMX_ERR_INVALID;
  }
  if (!ctx->have_problem)
  {
    ctx->err = "tmx_queries_set: no problem uploaded (call tmx_problem_upload first)";
    return TMX_ERR_STATE;
  }
  TMX_REFUSE_WHILE_PENDING(ctx);
  if (n_queries >= 2 && ctx->hp.flavor == TMX_FLAVOR_SQP)
  {
    ctx->err = "tmx_queries_set: multi-query batches are not lowered for TMX_FLAVOR_SQP problems (the trajopt_sqp term code reads the "
               "targets through code of its own)";
    return TMX_ERR_UNSUPPORTED;
  }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  invalidate_batch(ctx);
  drop_queries(ctx);
  if (n_queries == 1)
    return TMX_OK;
  const size_t Q = (size_t)n_queries, ncp = (size_t)ctx->hp.n_cp * 12, R = (size_t)ctx->hp.R;
  ctx->h_qcp.resize(Q * ncp);
  ctx->h_qaux1.resize(Q * R);
  for (size_t q = 0; q < Q; ++q)
  {
    std::copy(ctx->own_cp.begin(), ctx->own_cp.begin() + (std::ptrdiff_t)ncp, ctx->h_qcp.begin() + (std::ptrdiff_t)(q * ncp));
    std::copy(ctx->own_aux1.begin(), ctx->own_aux1.begin() + (std::ptrdiff_t)R, ctx->h_qaux1.begin() + (std::ptrdiff_t)(q * R));
  }
  tmx_status rc;
  if ((rc = upload(ctx, ctx->query_allocs, &ctx->d_qcp, ctx->h_qcp)) != TMX_OK || (rc = upload(ctx, ctx->query_allocs, &ctx->d_qaux1, ctx->h_qaux1)) != TMX_OK ||
      (rc = dalloc(ctx, ctx->query_allocs, &ctx->d_qprob, Q, false)) != TMX_OK)
  {
    drop_queries(ctx);
    return rc;
  }
  ctx->n_queries = n_queries;
  if ((rc = sync_query_problems(ctx)) != TMX_OK)
    drop_queries(ctx);
  return rc;
}

tmx_status tmx_query_set_targets(tmx_ctx* ctx, int32_t term, const double* targets, int32_t len)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (!ctx->have_problem)
  {
    ctx->err = "tmx_query_set_targets: no problem uploaded (call tmx_problem_upload first)";
    return TMX_ERR_STATE;
  }
  TMX_REFUSE_WHILE_PENDING(ctx);
  if (ctx->n_queries < 2)
  {
    ctx->err = "tmx_query_set_targets: the context has one query (call tmx_queries_set with n_queries >= 2 first)";
    return TMX_ERR_STATE;
  }
  if (!targets || term < 0 || term >= (int32_t)ctx->term_kind.size())
  {
    ctx->err = "tmx_query_set_targets: term index outside tmx_problem_desc::terms (or targets == NULL)";
    return TMX_ERR_INVALID;
  }
  const int kind = ctx->term_kind[(size_t)term];
  const int cp0 = ctx->term_cp0[(size_t)term], cp1 = ctx->term_cp1[(size_t)term];
  const int s0 = ctx->term_slot0[(size_t)term], s1 = ctx->term_slot1[(size_t)term];
  const bool pose = kind == TMX_TERM_CART_POSE;
  const bool jpos = kind == TMX_TERM_JOINT_POS_EQ_CNT || kind == TMX_TERM_JOINT_POS_INEQ_CNT || kind == TMX_TERM_JOINT_POS_INEQ_COST;
  if (pose && cp1 == cp0)
  {
    ctx->err = "tmx_query_set_targets: this cart_pose term was lowered as a function term (tolerance band): its target is a constant of "
               "the program table (fx_consts), not a per-query target";
    return TMX_ERR_UNSUPPORTED;
  }
  if (kind == TMX_TERM_JOINT_POS_EQ_COST)
  {
    ctx->err = "tmx_query_set_targets: the target of a squared joint_pos cost is baked into the static objective (pq), not a per-query target";
    return TMX_ERR_UNSUPPORTED;
  }
  if (!pose && !jpos)
  {
    ctx->err = "tmx_query_set_targets: this term kind carries no per-query target (accepted: cart_pose lowered into cart-pose instances, "
               "joint_pos equality / inequality constraints, joint_pos inequality cost)";
    return TMX_ERR_UNSUPPORTED;
  }
  const int want = pose ? 12 : ctx->n_dof;
  if (len != want)
  {
    ctx->err = "tmx_query_set_targets: len must be " + std::to_string(want) + " for this term (" + (pose ? "tmx_term::target_pose" : "tmx_term::targets, n_dof") + ")";
    return TMX_ERR_INVALID;
  }
  const size_t Q = (size_t)ctx->n_queries;
  for (size_t i = 0; i < Q * (size_t)len; ++i)
    if (!std::isfinite(targets[i]))
    {
      ctx->err = "tmx_query_set_targets: non-finite target value";
      return TMX_ERR_INVALID;
    }
  HIPCHK(hipSetDevice(ctx->device));
  invalidate_batch(ctx);
  const size_t ncp = (size_t)ctx->hp.n_cp * 12, R = (size_t)ctx->hp.R;
  if (pose)
  {
    for (size_t q = 0; q < Q; ++q)
      for (int c = cp0; c < cp1; ++c)  // (one instance per step of the term: the target applies to every step)
        std::copy(targets + q * 12, targets + q * 12 + 12, ctx->h_qcp.begin() + (std::ptrdiff_t)(q * ncp + (size_t)c * 12));
    HIPCHK(hipMemcpyAsync(ctx->d_qcp, ctx->h_qcp.data(), ctx->h_qcp.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  else
  {
    // the term's slots are SLOT_JOINTPOS / SLOT_JOINTPOS_INEQ rows: slot_sub = the joint
    for (size_t q = 0; q < Q; ++q)
      for (int r = s0; r < s1; ++r)
        ctx->h_qaux1[q * R + (size_t)r] = targets[q * (size_t)len + (size_t)ctx->own_sub[(size_t)r]];
    HIPCHK(hipMemcpyAsync(ctx->d_qaux1, ctx->h_qaux1.data(), ctx->h_qaux1.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return TMX_OK;
}

// the per-query reduction (k_argmin_queries); with x_out also the gather of the winning trajectories
static tmx_status argmin_queries(tmx_ctx* ctx, int64_t* best_index, double* best_cost, double* x_out, int32_t* found)
{
  if (ctx->Bcap == 0)
    return TMX_ERR_STATE;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  const int Q = ctx->n_queries, S = ctx->hb.B / Q, NX = ctx->hp.NX;
  struct PoolGuard
  {
    std::vector<void*> pool;
    ~PoolGuard() { free_pool(pool); }
  } guard;
  double *d_cost = nullptr, *d_x = nullptr;
  long long* d_idx = nullptr;
  tmx_status rc;
  if ((rc = dalloc(ctx, guard.pool, &d_cost, (size_t)Q, false)) != TMX_OK || (rc = dalloc(ctx, guard.pool, &d_idx, (size_t)Q, false)) != TMX_OK ||
      (x_out && (rc = dalloc(ctx, guard.pool, &d_x, (size_t)Q * NX, false)) != TMX_OK))
    return rc;
  const int conv = ctx->hp.flavor == TMX_FLAVOR_SQP ? (int)TMX_SQP_CONVERGED : (int)TMX_OPT_CONVERGED;
  [[maybe_unused]] const int nt = ctx->nt_qp > 1 ? 256 : 1;  // (the host build runs a workgroup as one thread)
  TMX_LAUNCH(k_argmin_queries, Q, nt, 16 * sizeof(double) + 18 * sizeof(int), ctx->stream, ctx->db, conv, S, NX, d_cost, d_idx, d_x);
  HIPCHK(hipGetLastError());
  std::vector<long long> idx((size_t)Q);
  std::vector<double> cost((size_t)Q);
  HIPCHK(hipMemcpyAsync(idx.data(), d_idx, sizeof(long long) * (size_t)Q, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(cost.data(), d_cost, sizeof(double) * (size_t)Q, hipMemcpyDeviceToHost, ctx->stream));
  if (x_out)
    HIPCHK(hipMemcpyAsync(x_out, d_x, sizeof(double) * (size_t)Q * NX, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (int q = 0; q < Q; ++q)
  {
    if (best_index)
      best_index[q] = idx[(size_t)q];
    if (best_cost)
      best_cost[q] = cost[(size_t)q];
    if (found)
      found[q] = idx[(size_t)q] >= 0 ? 1 : 0;
  }
  return TMX_OK;
}

tmx_status tmx_argmin_queries(tmx_ctx* ctx, int64_t* best_index, double* best_cost)
{
  if (!ctx || !best_index || !best_cost)
    return TMX_ERR_INVALID;
  return argmin_queries(ctx, best_index, best_cost, nullptr, nullptr);
}

tmx_status tmx_best_trajectories(tmx_ctx* ctx, double* x_out, int32_t* found)
{
  if (!ctx || !x_out)
    return TMX_ERR_INVALID;
  return argmin_queries(ctx, nullptr, nullptr, x_out, found);
}

void tmx_default_check_config(tmx_check_config* cfg)
{
  if (!cfg)
    return;
  cfg->evaluator_type = 4;  // LVS_CONTINUOUS
  cfg->max_substates = 32;
  cfg->margin = 0.0;
  cfg->longest_valid_segment_length = 0.05;
}

// launch geometry and LDS of k_check_trajectories for n trajectories under cfg (validated here): the tile is the largest number of
// items whose distance table and sub-state frames fit 64 KB of LDS (two workgroups and more per CU), at most the items of one step at
// cnt = max_substates - the count depends on the data, so the worst case sizes the tables
struct CheckPlan
{
  CheckArgs a;
  size_t smem;
  int nt;
};
// (items_per_substate < 0: the S x O pairs of the obstacle check; the self-collision check passes its primitive pairs)
static tmx_status check_plan(tmx_ctx* ctx, const tmx_check_config* cfg, int n, const char* who, CheckPlan& pl, long long items_per_substate = -1)
{
  const std::string w(who);
  if (!cfg)
  {
    ctx->err = w + ": cfg == NULL (tmx_default_check_config fills one)";
    return TMX_ERR_INVALID;
  }
  if (cfg->evaluator_type < 0 || cfg->evaluator_type > 4)
  {
    ctx->err = w + ": evaluator_type must be 0 .. 4 (0 / 1 DISCRETE, 2 LVS_DISCRETE, 3 CONTINUOUS, 4 LVS_CONTINUOUS)";
    return TMX_ERR_INVALID;
  }
  if (cfg->max_substates < 0 || cfg->max_substates > 0x7FFF)
  {
    ctx->err = w + ": max_substates must be 0 .. 32767 (0 = 2)";
    return TMX_ERR_INVALID;
  }
  if (!std::isfinite(cfg->margin) || !std::isfinite(cfg->longest_valid_segment_length))
  {
    ctx->err = w + ": non-finite margin or longest_valid_segment_length";
    return TMX_ERR_INVALID;
  }
  const int type = cfg->evaluator_type;
  if ((type == 2 || type == 4) && !(cfg->longest_valid_segment_length > 0.0))
  {
    ctx->err = w + ": longest_valid_segment_length must be > 0 for the LVS evaluators (types 2 and 4)";
    return TMX_ERR_INVALID;
  }
  if (type >= 3 && ctx->hp.n_ls_capsule > 0)
  {
    ctx->err = w + ": a cast check (evaluator_type 3 / 4) of capsule links: the swept volume of a capsule is not a capsule, and the "
                   "upload turns capsule links into two-vertex hulls only when the description has a cast collision term";
    return TMX_ERR_UNSUPPORTED;
  }
  const int DK = ctx->hp.DK, T = ctx->hp.T;
  const long long SO = items_per_substate < 0 ? (long long)ctx->hp.S * ctx->hp.O : items_per_substate;
  CheckArgs& a = pl.a;
  a.type = type;
  a.kmax = cfg->max_substates < 2 ? 2 : cfg->max_substates;
  a.margin = cfg->margin;
  a.lvs = cfg->longest_valid_segment_length;
  a.converged_only = 0;
  a.converged_code = ctx->hp.flavor == TMX_FLAVOR_SQP ? (int)TMX_SQP_CONVERGED : (int)TMX_OPT_CONVERGED;
  pl.nt = ctx->nt_qp > 1 ? 256 : 1;  // (the host build runs a workgroup as one thread)
  const long long nsub = type < 2 ? 1 : (type == 3 ? 1 : (type == 4 ? a.kmax - 1 : a.kmax));
  const long long step_items = std::max<long long>(1, nsub * SO);  // items of one step, worst case
  const long long so1 = std::max<long long>(1, SO);
  auto fits = [&](long long tile) { return check_lds_doubles(DK, (int)tile, (int)(tile / so1 + 3), pl.nt) * sizeof(double) <= 64 * 1024; };
  long long tile_max = (long long)((8192.0 - 2.0 * pl.nt - 2.0 - 36.0 * DK) / (12.0 * DK / (double)so1 + 1.0));
  tile_max = std::max<long long>(1, tile_max);
  while (tile_max > 1 && !fits(tile_max))
    --tile_max;
  long long tile = std::min(step_items, tile_max);
  // default: about 2048 workgroups in the grid, whole steps per workgroup
  long long chunks = std::max<long long>(1, std::min<long long>(T, (2048 + n - 1) / n));
  long long spc = (T + chunks - 1) / chunks;
  // TMX_CHECK_TILE=<items> (test hook, read at the call): a workgroup's LDS holds at most that many items - as many whole steps per
  // chunk as fit (at least one), and a tile smaller than a step when one step does not fit
  if (const char* e = std::getenv("TMX_CHECK_TILE"))
  {
    const long long want = std::max<long long>(1, std::atoll(e));
    tile = std::min(tile, want);
    spc = std::max<long long>(1, std::min<long long>(T, want / step_items));
  }
  chunks = (T + spc - 1) / spc;
  a.tile = (int)tile;
  a.fcap = (int)(tile / so1 + 3);
  a.spc = (int)spc;
  a.chunks = (int)chunks;
  pl.smem = check_lds_doubles(DK, a.tile, a.fcap, pl.nt) * sizeof(double);
  return TMX_OK;
}
static tmx_status check_launch(tmx_ctx* ctx, const CheckPlan& pl, const double* d_x, int n, double* d_min, double* d_pen, int* d_key)
{
  if (ctx->hull)
    TMX_LAUNCH(k_check_trajectories_hull, n * pl.a.chunks, pl.nt, pl.smem, ctx->stream, ctx->dp, ctx->db, d_x, pl.a, d_min, d_pen, d_key);
  else
    TMX_LAUNCH(k_check_trajectories, n * pl.a.chunks, pl.nt, pl.smem, ctx->stream, ctx->dp, ctx->db, d_x, pl.a, d_min, d_pen, d_key);
  HIPCHK(hipGetLastError());
  return TMX_OK;
}

tmx_status tmx_check_trajectories(tmx_ctx* ctx, const tmx_check_config* cfg, const double* x_host, int32_t n, double* min_distance,
                                  double* penetration, tmx_check_worst* worst)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (!ctx->have_problem)
  {
    ctx->err = "tmx_check_trajectories: no problem uploaded (call tmx_problem_upload first)";
    return TMX_ERR_STATE;
  }
  TMX_REFUSE_WHILE_PENDING(ctx);
  if (n < 1)
  {
    ctx->err = "tmx_check_trajectories: n must be >= 1";
    return TMX_ERR_INVALID;
  }
  CheckPlan pl;
  tmx_status rc;
  if ((rc = check_plan(ctx, cfg, n, "tmx_check_trajectories", pl)) != TMX_OK)
    return rc;
  const size_t T = (size_t)ctx->hp.T, NX = (size_t)ctx->hp.NX;
  if (!x_host)
  {
    if (ctx->Bcap == 0)
    {
      ctx->err = "tmx_check_trajectories: x_host == NULL checks the current iterates, but the context holds no batch (call tmx_batch_set_x0 first)";
      return TMX_ERR_STATE;
    }
    if (n != ctx->hb.B)
    {
      ctx->err = "tmx_check_trajectories: with x_host == NULL n must equal the batch (" + std::to_string(ctx->hb.B) + ")";
      return TMX_ERR_INVALID;
    }
  }
  else
    for (size_t i = 0; i < (size_t)n * NX; ++i)
      if (!std::isfinite(x_host[i]))
      {
        ctx->err = "tmx_check_trajectories: non-finite trajectory value";
        return TMX_ERR_INVALID;
      }
  HIPCHK(hipSetDevice(ctx->device));
  struct PoolGuard
  {
    std::vector<void*> pool;
    ~PoolGuard() { free_pool(pool); }
  } guard;
  double *d_x = nullptr, *d_min = nullptr, *d_pen = nullptr;
  int* d_key = nullptr;
  tmx_check_worst* d_worst = nullptr;
  if ((x_host && (rc = dalloc(ctx, guard.pool, &d_x, (size_t)n * NX, false)) != TMX_OK) ||
      (rc = dalloc(ctx, guard.pool, &d_min, (size_t)n * T, false)) != TMX_OK || (rc = dalloc(ctx, guard.pool, &d_pen, (size_t)n * T, false)) != TMX_OK ||
      (rc = dalloc(ctx, guard.pool, &d_key, (size_t)n * T * 3, false)) != TMX_OK ||
      (worst && (rc = dalloc(ctx, guard.pool, &d_worst, (size_t)n, false)) != TMX_OK))
    return rc;
  if (x_host)
    HIPCHK(hipMemcpyAsync(d_x, x_host, sizeof(double) * (size_t)n * NX, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = check_launch(ctx, pl, x_host ? d_x : ctx->hb.x, n, d_min, d_pen, d_key)) != TMX_OK)
    return rc;
  if (worst)
  {
    // the per-trajectory reduction over the per-step results (its own small launch: a trajectory may span several chunks)
    TMX_LAUNCH(k_check_worst, (n + pl.nt - 1) / pl.nt, pl.nt, 0, ctx->stream, (int)n, (int)T, d_min, d_key, d_worst);
    HIPCHK(hipGetLastError());
  }
  if ((rc = d2h(ctx, min_distance, d_min, (size_t)n * T)) != TMX_OK || (rc = d2h(ctx, penetration, d_pen, (size_t)n * T)) != TMX_OK ||
      (rc = d2h(ctx, worst, d_worst, (size_t)n)) != TMX_OK)
    return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return TMX_OK;
}

// ---- self-collision side of the check (tmx_check_self.h) ----
tmx_status tmx_check_set_link_pairs(tmx_ctx* ctx, const int32_t* link_pairs, int32_t n_pairs)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (!ctx->have_problem)
  {
    ctx->err = "tmx_check_set_link_pairs: no problem uploaded (call tmx_problem_upload first; an upload clears the pairs)";
    return TMX_ERR_STATE;
  }
  TMX_REFUSE_WHILE_PENDING(ctx);
  if (n_pairs < 0)
  {
    ctx->err = "tmx_check_set_link_pairs: n_pairs must be >= 0 (0 clears the pairs)";
    return TMX_ERR_INVALID;
  }
  if (!link_pairs)
    n_pairs = 0;
  const int DK = ctx->hp.DK;
  for (int k = 0; k < n_pairs; ++k)
  {
    const int a = link_pairs[2 * k], b = link_pairs[2 * k + 1];
    if (a < 0 || a >= DK || b < 0 || b >= DK)
    {
      ctx->err = "tmx_check_set_link_pairs: pair " + std::to_string(k) + " = (" + std::to_string(a) + ", " + std::to_string(b) +
                 "): a link index must be in 0 .. n_dof - 1 = " + std::to_string(DK - 1);
      return TMX_ERR_INVALID;
    }
    if (a == b)
    {
      ctx->err = "tmx_check_set_link_pairs: pair " + std::to_string(k) + " = (" + std::to_string(a) + ", " + std::to_string(b) +
                 "): a link is not tested against itself";
      return TMX_ERR_INVALID;
    }
    for (int j = 0; j < k; ++j)
      if ((link_pairs[2 * j] == a && link_pairs[2 * j + 1] == b) || (link_pairs[2 * j] == b && link_pairs[2 * j + 1] == a))
      {
        ctx->err = "tmx_check_set_link_pairs: pair " + std::to_string(k) + " = (" + std::to_string(a) + ", " + std::to_string(b) +
                   ") repeats pair " + std::to_string(j) + " (a pair is given once, in either order)";
        return TMX_ERR_INVALID;
      }
  }
  // primitive pairs: link pair, then sa, then sb, all ascending
  std::vector<int> prim;
  for (int k = 0; k < n_pairs; ++k)
    for (size_t sa = 0; sa < ctx->h_ls_link.size(); ++sa)
      if (ctx->h_ls_link[sa] == link_pairs[2 * k])
        for (size_t sb = 0; sb < ctx->h_ls_link.size(); ++sb)
          if (ctx->h_ls_link[sb] == link_pairs[2 * k + 1])
          {
            prim.push_back((int)sa);
            prim.push_back((int)sb);
          }
  HIPCHK(hipSetDevice(ctx->device));
  int* d_new = nullptr;
  if (!prim.empty())
  {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, prim.size() * sizeof(int)));
    d_new = static_cast<int*>(p);
    if (hipMemcpy(d_new, prim.data(), prim.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
    {
      (void)hipFree(d_new);
      ctx->err = "tmx_check_set_link_pairs: the copy of the primitive-pair table failed";
      return TMX_ERR_DEVICE;
    }
  }
  drop_check_pairs(ctx);
  ctx->d_check_pairs = d_new;
  ctx->check_link_pairs.assign(link_pairs, link_pairs + 2 * (size_t)n_pairs);
  ctx->check_prim_pairs = std::move(prim);
  return TMX_OK;
}

tmx_status tmx_check_link_pairs(tmx_ctx* ctx, int32_t* n_pairs, int32_t* n_primitive_pairs)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (n_pairs)
    *n_pairs = (int32_t)(ctx->check_link_pairs.size() / 2);
  if (n_primitive_pairs)
    *n_primitive_pairs = (int32_t)(ctx->check_prim_pairs.size() / 2);
  return TMX_OK;
}

static tmx_status check_self_launch(tmx_ctx* ctx, const CheckPlan& pl, const double* d_x, int n, double* d_min, double* d_pen, int* d_key)
{
  const int PP = (int)(ctx->check_prim_pairs.size() / 2);
  if (ctx->hull)
    TMX_LAUNCH(k_check_self_hull, n * pl.a.chunks, pl.nt, pl.smem, ctx->stream, ctx->dp, ctx->db, d_x, pl.a, ctx->d_check_pairs, PP, d_min, d_pen, d_key);
  else
    TMX_LAUNCH(k_check_self, n * pl.a.chunks, pl.nt, pl.smem, ctx->stream, ctx->dp, ctx->db, d_x, pl.a, ctx->d_check_pairs, PP, d_min, d_pen, d_key);
  HIPCHK(hipGetLastError());
  return TMX_OK;
}

tmx_status tmx_check_self_trajectories(tmx_ctx* ctx, const tmx_check_config* cfg, const double* x_host, int32_t n, double* min_distance,
                                       double* penetration, tmx_check_self_worst* worst)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (!ctx->have_problem)
  {
    ctx->err = "tmx_check_self_trajectories: no problem uploaded (call tmx_problem_upload first)";
    return TMX_ERR_STATE;
  }
  TMX_REFUSE_WHILE_PENDING(ctx);
  if (n < 1)
  {
    ctx->err = "tmx_check_self_trajectories: n must be >= 1";
    return TMX_ERR_INVALID;
  }
  CheckPlan pl;
  tmx_status rc;
  if ((rc = check_plan(ctx, cfg, n, "tmx_check_self_trajectories", pl, (long long)(ctx->check_prim_pairs.size() / 2))) != TMX_OK)
    return rc;
  const size_t T = (size_t)ctx->hp.T, NX = (size_t)ctx->hp.NX;
  if (!x_host)
  {
    if (ctx->Bcap == 0)
    {
      ctx->err = "tmx_check_self_trajectories: x_host == NULL checks the current iterates, but the context holds no batch (call tmx_batch_set_x0 first)";
      return TMX_ERR_STATE;
    }
    if (n != ctx->hb.B)
    {
      ctx->err = "tmx_check_self_trajectories: with x_host == NULL n must equal the batch (" + std::to_string(ctx->hb.B) + ")";
      return TMX_ERR_INVALID;
    }
  }
  else
    for (size_t i = 0; i < (size_t)n * NX; ++i)
      if (!std::isfinite(x_host[i]))
      {
        ctx->err = "tmx_check_self_trajectories: non-finite trajectory value";
        return TMX_ERR_INVALID;
      }
  HIPCHK(hipSetDevice(ctx->device));
  struct PoolGuard
  {
    std::vector<void*> pool;
    ~PoolGuard() { free_pool(pool); }
  } guard;
  double *d_x = nullptr, *d_min = nullptr, *d_pen = nullptr;
  int* d_key = nullptr;
  tmx_check_self_worst* d_worst = nullptr;
  if ((x_host && (rc = dalloc(ctx, guard.pool, &d_x, (size_t)n * NX, false)) != TMX_OK) ||
      (rc = dalloc(ctx, guard.pool, &d_min, (size_t)n * T, false)) != TMX_OK || (rc = dalloc(ctx, guard.pool, &d_pen, (size_t)n * T, false)) != TMX_OK ||
      (rc = dalloc(ctx, guard.pool, &d_key, (size_t)n * T * 2, false)) != TMX_OK ||
      (worst && (rc = dalloc(ctx, guard.pool, &d_worst, (size_t)n, false)) != TMX_OK))
    return rc;
  if (x_host)
    HIPCHK(hipMemcpyAsync(d_x, x_host, sizeof(double) * (size_t)n * NX, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = check_self_launch(ctx, pl, x_host ? d_x : ctx->hb.x, n, d_min, d_pen, d_key)) != TMX_OK)
    return rc;
  if (worst)
  {
    TMX_LAUNCH(k_check_self_worst, (n + pl.nt - 1) / pl.nt, pl.nt, 0, ctx->stream, (int)n, (int)T, d_min, d_key, ctx->d_check_pairs, d_worst);
    HIPCHK(hipGetLastError());
  }
  if ((rc = d2h(ctx, min_distance, d_min, (size_t)n * T)) != TMX_OK || (rc = d2h(ctx, penetration, d_pen, (size_t)n * T)) != TMX_OK ||
      (rc = d2h(ctx, worst, d_worst, (size_t)n)) != TMX_OK)
    return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return TMX_OK;
}

tmx_status tmx_best_trajectories_checked(tmx_ctx* ctx, const tmx_check_config* cfg, int64_t* best_index, double* best_cost,
                                         double* best_min_distance, double* x_out)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (!best_index || !best_cost)
  {
    ctx->err = "tmx_best_trajectories_checked: best_index and best_cost must not be NULL";
    return TMX_ERR_INVALID;
  }
  if (!ctx->have_problem || ctx->Bcap == 0)
  {
    ctx->err = "tmx_best_trajectories_checked: the context holds no batch (tmx_problem_upload, tmx_batch_set_x0, run first)";
    return TMX_ERR_STATE;
  }
  TMX_REFUSE_WHILE_PENDING(ctx);
  const int B = ctx->hb.B, Q = ctx->n_queries, S = B / Q, NX = ctx->hp.NX, T = ctx->hp.T;
  CheckPlan pl;
  tmx_status rc;
  if ((rc = check_plan(ctx, cfg, B, "tmx_best_trajectories_checked", pl)) != TMX_OK)
    return rc;
  pl.a.converged_only = 1;  // a workgroup of a seed that did not converge returns at once
  HIPCHK(hipSetDevice(ctx->device));
  struct PoolGuard
  {
    std::vector<void*> pool;
    ~PoolGuard() { free_pool(pool); }
  } guard;
  double *d_min = nullptr, *d_pen = nullptr, *d_cost = nullptr, *d_clear = nullptr, *d_x = nullptr;
  int* d_key = nullptr;
  long long* d_idx = nullptr;
  if ((rc = dalloc(ctx, guard.pool, &d_min, (size_t)B * T, false)) != TMX_OK || (rc = dalloc(ctx, guard.pool, &d_pen, (size_t)B * T, false)) != TMX_OK ||
      (rc = dalloc(ctx, guard.pool, &d_key, (size_t)B * T * 3, false)) != TMX_OK || (rc = dalloc(ctx, guard.pool, &d_cost, (size_t)Q, false)) != TMX_OK ||
      (rc = dalloc(ctx, guard.pool, &d_clear, (size_t)Q, false)) != TMX_OK || (rc = dalloc(ctx, guard.pool, &d_idx, (size_t)Q, false)) != TMX_OK ||
      (x_out && (rc = dalloc(ctx, guard.pool, &d_x, (size_t)Q * NX, false)) != TMX_OK))
    return rc;
  // one check launch (the per-step minima of the converged seeds stay on the device), one reduction launch, one copy
  if ((rc = check_launch(ctx, pl, ctx->hb.x, B, d_min, d_pen, d_key)) != TMX_OK)
    return rc;
  if (!ctx->check_prim_pairs.empty())
  {
    // link pairs are set: the self minima of the converged seeds, folded into the obstacle minima (a minimum does not round) - the
    // reduction below then sees "free of the obstacles and of itself" and the smaller clearance
    CheckPlan ps;
    if ((rc = check_plan(ctx, cfg, B, "tmx_best_trajectories_checked", ps, (long long)(ctx->check_prim_pairs.size() / 2))) != TMX_OK)
      return rc;
    ps.a.converged_only = 1;
    double *d_smin = nullptr, *d_spen = nullptr;
    int* d_skey = nullptr;
    if ((rc = dalloc(ctx, guard.pool, &d_smin, (size_t)B * T, false)) != TMX_OK || (rc = dalloc(ctx, guard.pool, &d_spen, (size_t)B * T, false)) != TMX_OK ||
        (rc = dalloc(ctx, guard.pool, &d_skey, (size_t)B * T * 2, false)) != TMX_OK)
      return rc;
    if ((rc = check_self_launch(ctx, ps, ctx->hb.x, B, d_smin, d_spen, d_skey)) != TMX_OK)
      return rc;
    TMX_LAUNCH(k_check_fold_min, (B * T + pl.nt - 1) / pl.nt, pl.nt, 0, ctx->stream, ctx->db, pl.a.converged_code, (int)B, (int)T, d_smin, d_min);
    HIPCHK(hipGetLastError());
  }
  TMX_LAUNCH(k_argmin_queries_checked, Q, pl.nt, 16 * sizeof(double) + 18 * sizeof(int), ctx->stream, ctx->db, pl.a.converged_code, S, NX, T,
             pl.a.margin, d_min, d_cost, d_idx, d_clear, d_x);
  HIPCHK(hipGetLastError());
  std::vector<long long> idx((size_t)Q);
  HIPCHK(hipMemcpyAsync(idx.data(), d_idx, sizeof(long long) * (size_t)Q, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(best_cost, d_cost, sizeof(double) * (size_t)Q, hipMemcpyDeviceToHost, ctx->stream));
  if (best_min_distance)
    HIPCHK(hipMemcpyAsync(best_min_distance, d_clear, sizeof(double) * (size_t)Q, hipMemcpyDeviceToHost, ctx->stream));
  if (x_out)
    HIPCHK(hipMemcpyAsync(x_out, d_x, sizeof(double) * (size_t)Q * NX, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (int q = 0; q < Q; ++q)
    best_index[q] = idx[(size_t)q];
  return TMX_OK;
}

tmx_status tmx_nccl_unique_id(uint8_t id[TMX_NCCL_UNIQUE_ID_BYTES])
{
  if (!id)
    return TMX_ERR_INVALID;
#ifdef TMX_HOST_EMU
  std::memset(id, 0, TMX_NCCL_UNIQUE_ID_BYTES);
  return TMX_OK;
#else
  static_assert(sizeof(ncclUniqueId) <= TMX_NCCL_UNIQUE_ID_BYTES, "ncclUniqueId larger than the ABI buffer");
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess)
    return TMX_ERR_NCCL;
  std::memset(id, 0, TMX_NCCL_UNIQUE_ID_BYTES);
  std::memcpy(id, &u, sizeof(u));
  return TMX_OK;
#endif
}

tmx_status tmx_nccl_init(tmx_ctx* ctx, const uint8_t id[TMX_NCCL_UNIQUE_ID_BYTES], int32_t n_ranks, int32_t rank)
{
  if (!ctx || !id || n_ranks < 1 || rank < 0 || rank >= n_ranks)
    return TMX_ERR_INVALID;
#ifdef TMX_HOST_EMU
  return TMX_OK;  // no collective in the host emulation (tests use gloo above the C-ABI)
#else
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->nccl && ctx->nccl_owned)
    (void)ncclCommDestroy(static_cast<ncclComm_t>(ctx->nccl));
  ctx->nccl = nullptr;
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  ncclComm_t comm = nullptr;
  if (ncclCommInitRank(&comm, n_ranks, u, rank) != ncclSuccess)
  {
    ctx->err = "ncclCommInitRank failed";
    return TMX_ERR_NCCL;
  }
  ctx->nccl = comm;
  ctx->nccl_owned = true;
  return TMX_OK;
#endif
}

tmx_status tmx_attach_nccl(tmx_ctx* ctx, void* nccl_comm)
{
  if (!ctx)
    return TMX_ERR_INVALID;
#ifndef TMX_HOST_EMU
  if (ctx->nccl && ctx->nccl_owned)
    (void)ncclCommDestroy(static_cast<ncclComm_t>(ctx->nccl));
#endif
  ctx->nccl = nccl_comm;
  ctx->nccl_owned = false;
  return TMX_OK;
}

tmx_status tmx_kernel_stats(tmx_ctx* ctx, double* admm_ms_total, int64_t* admm_launches, double* convexify_ms_total,
                            double* evaluate_ms_total)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  if (admm_ms_total)
    *admm_ms_total = ctx->ms_admm;
  if (admm_launches)
    *admm_launches = ctx->launches_admm;
  if (convexify_ms_total)
    *convexify_ms_total = ctx->ms_convexify;
  if (evaluate_ms_total)
    *evaluate_ms_total = ctx->ms_evaluate;
  return TMX_OK;
}

// debug/profiling hook (not part of include/tmx.h): per-phase shader-clock cycles of the last k_qp_solve, summed over problems
__attribute__((visibility("default"))) tmx_status tmx_debug_phase_cycles(tmx_ctx* ctx, long long* out16)
{
  if (!ctx || !out16 || ctx->Bcap == 0)
    return TMX_ERR_INVALID;
  std::vector<long long> h((size_t)ctx->hb.B * 16);
  HIPCHK(hipMemcpy(h.data(), ctx->hb.prof, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
  for (int k = 0; k < 16; ++k)
    out16[k] = 0;
  for (int b = 0; b < ctx->hb.B; ++b)
    for (int k = 0; k < 16; ++k)
      out16[k] += h[(size_t)b * 16 + k];
  return TMX_OK;
}

// debug hook (not in include/tmx.h): the device build of include/tmx_detmath.h on host arrays (parity test: the same
// bits as the oracle's build of the same header)
__attribute__((visibility("default"))) tmx_status tmx_debug_detmath(tmx_ctx* ctx, int op, int n, const double* a, const double* b, double* out)
{
  if (!ctx || !a || !b || !out || n < 1 || op < 0 || op > 2)
    return TMX_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  std::vector<void*> pool;
  double *da = nullptr, *db = nullptr, *dout = nullptr;
  tmx_status rc;
  if ((rc = dalloc(ctx, pool, &da, (size_t)n)) != TMX_OK || (rc = dalloc(ctx, pool, &db, (size_t)n)) != TMX_OK ||
      (rc = dalloc(ctx, pool, &dout, (size_t)n)) != TMX_OK)
  {
    free_pool(pool);
    return rc;
  }
  hipError_t e = hipMemcpy(da, a, sizeof(double) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(db, b, sizeof(double) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess)
  {
    TMX_LAUNCH(k_detmath, 64, 256, 0, ctx->stream, op, n, da, db, dout);
    e = hipStreamSynchronize(ctx->stream);
  }
  if (e == hipSuccess)
    e = hipMemcpy(out, dout, sizeof(double) * n, hipMemcpyDeviceToHost);
  free_pool(pool);
  if (e != hipSuccess)
  {
    ctx->err = std::string("tmx_debug_detmath: ") + hipGetErrorString(e);
    return TMX_ERR_DEVICE;
  }
  return TMX_OK;
}

// debug hook (not in include/tmx.h): per-problem ADMM iteration totals of the last run (load-balance analysis)
__attribute__((visibility("default"))) tmx_status tmx_debug_admm_iters(tmx_ctx* ctx, int64_t* out)
{
  if (!ctx || !out || ctx->hb.B <= 0)
    return TMX_ERR_INVALID;
  static_assert(sizeof(long long) == sizeof(int64_t), "");
  if (hipMemcpy(out, ctx->hb.admm_iters, sizeof(int64_t) * ctx->hb.B, hipMemcpyDeviceToHost) != hipSuccess)
    return TMX_ERR_DEVICE;
  return TMX_OK;
}

// debug hook (not in include/tmx.h): diagnostic switches of the uploaded problem (DevProblem::dbg_flags); bit 0 = scalar assembly of the
// diagonal KKT blocks instead of the MFMA one, bit 1 = generic QP setup, bit 2 = generic polish on the dense fast path, bit 3 = generic
// SQP shell around the QP solve (qp_structure) on a problem the specialised one can take, bit 4 = the hashes of P by the loop over its
// columns and the generic exact evaluation and model values on a problem of eval_fast, bit 5 = the generic ADMM factorisation on a
// problem of factor_fast, bit 6 = one elimination step per barrier in the separator inverse of factor_fast, bit 7 = no in-register
// filter in the epoch-resident ADMM burst: qp_check_nl at every check, on norms it forms itself
__attribute__((visibility("default"))) tmx_status tmx_debug_set_flags(tmx_ctx* ctx, int flags)
{
  if (!ctx || !ctx->have_problem || !ctx->dp)
    return TMX_ERR_INVALID;
  TMX_REFUSE_WHILE_PENDING(ctx);
  HIPCHK(hipSetDevice(ctx->device));
  ctx->hp.dbg_flags = flags;
  HIPCHK(hipMemcpy(reinterpret_cast<char*>(ctx->dp) + offsetof(DevProblem, dbg_flags), &flags, sizeof(int), hipMemcpyHostToDevice));
  return sync_query_problems(ctx);  // (the per-query copies of the DevProblem carry the switches too)
}

// debug hook (not in include/tmx.h): 1 when the uploaded problem qualifies for the register-resident QP setup of the dense fast path
// (DevProblem::setup_fast; the kernels add their own fast-path predicate), 0 when not, -1 without a problem
__attribute__((visibility("default"))) int tmx_debug_setup_fast(tmx_ctx* ctx)
{
  if (!ctx || !ctx->have_problem)
    return -1;
  return ctx->hp.setup_fast;
}

// debug hook (not in include/tmx.h): 1 when the uploaded problem qualifies for the register-resident polish of the dense fast path
// (DevProblem::polish_fast; the kernels add their own fast-path predicate), 0 when not, -1 without a problem
__attribute__((visibility("default"))) int tmx_debug_polish_fast(tmx_ctx* ctx)
{
  if (!ctx || !ctx->have_problem)
    return -1;
  return ctx->hp.polish_fast;
}

// debug hook (not in include/tmx.h): 1 when the uploaded problem qualifies for the ADMM factorisation with the interior inverses inside
// one wave (DevProblem::factor_fast; the kernels add their own fast-path predicate), 0 when not, -1 without a problem
__attribute__((visibility("default"))) int tmx_debug_factor_fast(tmx_ctx* ctx)
{
  if (!ctx || !ctx->have_problem)
    return -1;
  return ctx->hp.factor_fast;
}

// debug hook (not in include/tmx.h): the row lists of the uploaded problem by waypoint (DevProblem::wp_start, T + 1 entries) into out[0 .. cap);
// returns T + 1, or -1 without a problem or with too small a buffer (tests/test_burst_check.py: the list lengths mod 4 its shapes cover)
__attribute__((visibility("default"))) int tmx_debug_wp_start(tmx_ctx* ctx, int* out, int cap)
{
  if (!ctx || !ctx->have_problem || !ctx->hp.wp_start || !out || cap < ctx->hp.T + 1)
    return -1;
  if (hipSetDevice(ctx->device) != hipSuccess ||
      hipMemcpy(out, ctx->hp.wp_start, sizeof(int) * (size_t)(ctx->hp.T + 1), hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  return ctx->hp.T + 1;
}

// debug hook (not in include/tmx.h): 1 when the uploaded problem qualifies for the specialised SQP shell around the QP solve
// (DevProblem::step_fast; the kernels add the launch shape), 0 when not, -1 without a problem
__attribute__((visibility("default"))) int tmx_debug_step_fast(tmx_ctx* ctx)
{
  if (!ctx || !ctx->have_problem)
    return -1;
  return ctx->hp.step_fast;
}

// debug hook (not in include/tmx.h): 1 when the uploaded problem qualifies for the P-hash table and the merged evaluation of the
// specialised step (DevProblem::eval_fast; the kernels add the launch shape), 0 when not, -1 without a problem
__attribute__((visibility("default"))) int tmx_debug_eval_fast(tmx_ctx* ctx)
{
  if (!ctx || !ctx->have_problem)
    return -1;
  return ctx->hp.eval_fast;
}

// debug hooks (not in include/tmx.h): the engine the upload chose for the QP solves of the uploaded problem, -1 without a problem.
// DevProblem::wave_ok (the wave-pair solver, TMX_WAVE=1), qp_dense (the dense engine), tt_chain (the number of TotalTime terms carried
// as rank-one corrections of the block chain, 0 when not) and tv_chain (squared velocity-with-time costs on the dense-coupling chain)
__attribute__((visibility("default"))) int tmx_debug_wave_ok(tmx_ctx* ctx)
{
  if (!ctx || !ctx->have_problem)
    return -1;
  return ctx->hp.wave_ok;
}

__attribute__((visibility("default"))) int tmx_debug_qp_dense(tmx_ctx* ctx)
{
  if (!ctx || !ctx->have_problem)
    return -1;
  return ctx->hp.qp_dense;
}

__attribute__((visibility("default"))) int tmx_debug_tt_chain(tmx_ctx* ctx)
{
  if (!ctx || !ctx->have_problem)
    return -1;
  return ctx->hp.tt_chain;
}

__attribute__((visibility("default"))) int tmx_debug_tv_chain(tmx_ctx* ctx)
{
  if (!ctx || !ctx->have_problem)
    return -1;
  return ctx->hp.tv_chain;
}

// ... and band_pairs (squared acceleration / jerk costs next to general pair rows on the banded factorisation with a dense first coupling)
__attribute__((visibility("default"))) int tmx_debug_band_pairs(tmx_ctx* ctx)
{
  if (!ctx || !ctx->have_problem)
    return -1;
  return ctx->hp.band_pairs;
}

// ... and both band_rows and band_pairs (acceleration / jerk ROWS next to general pair rows on that factorisation, TMX_BAND_ROW_PAIR_CHAIN=1)
__attribute__((visibility("default"))) int tmx_debug_band_row_pairs(tmx_ctx* ctx)
{
  if (!ctx || !ctx->have_problem)
    return -1;
  return (ctx->hp.band_rows && ctx->hp.band_pairs) ? 1 : 0;
}

// debug hook (not in include/tmx.h): 1 = fused persistent optimize() kernel (default), 0 = one launch chain per step
__attribute__((visibility("default"))) tmx_status tmx_debug_set_fused(tmx_ctx* ctx, int mode)
{
  if (!ctx || mode < 0 || mode > 2)
    return TMX_ERR_INVALID;
  ctx->mode = mode;
  return TMX_OK;
}

tmx_status tmx_kernel_stats_reset(tmx_ctx* ctx)
{
  if (!ctx)
    return TMX_ERR_INVALID;
  ctx->ms_admm = ctx->ms_convexify = ctx->ms_evaluate = 0.0;
  ctx->launches_admm = 0;
  return TMX_OK;
}
}  // extern "C"
