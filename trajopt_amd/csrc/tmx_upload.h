// tmx_upload.h — what the stages of tmx_problem_upload (tmx_api.cpp) hand to each other.  Host only, included by tmx_api.cpp only.
//   lower_terms -> Lowered -> choose_engine -> EngineChoice -> place_workspace -> Placement -> upload_tables -> configure_launch
#pragma once
#include <cstddef>
#include <cstdlib>
#include <string>
#include <vector>

// The description lowered to the row-slot template, the static Hessian and the per-kind tables (lower_terms).
struct Lowered
{
  // slot template in reference row order
  std::vector<int> kind, st, sub, sub2, owner, naux, iscnt, iseq;
  std::vector<double> objc, scale, aux1, aux2;
  std::vector<int> c2, sub3;  // pair rows: index of the second coefficient block; LVS flags
  std::vector<double> aux3;
  std::vector<int> aoff;      // first penalty variable of every slot
  // static objective: diagonal, the bands at distance D / 2 D / 3 D, linear term; column pointers of upper-triangular P
  std::vector<double> pd, po, pq, po2, po3;
  std::vector<int> p_colptr;
  std::vector<int> fx_t, fx_kind, fx_owner, fx_op0, fx_nops, fx_c0, fx_nout, fx_slot0, fx_ci, fx_ops;  // function-term instances
  std::vector<double> fx_consts;
  std::vector<int> vel_first, vel_last, vel_cost, vel_kind, cp_t, cp_owner, cp_iscnt, cp_nrows, cp_idx, cp_slot0;
  std::vector<double> vel_coeffs, vel_targets, cp_coeff, cp_target;
  // time-parameterised terms
  std::vector<int> tv_owner, tv_joint, tv_first, tv_last, tt_owner, tt_form, tt_slot;
  std::vector<double> tv_coeff, tv_target, tv_up, tv_lo, tt_coeff, tt_limit;
  // geometry
  std::vector<int> ls_link, ls_hull;
  std::vector<double> ls_center, ls_radius, ob_center, ob_radius, ob_axis, ls_axis, ob_box, hullv, mesh;
  std::vector<int> wp_start, wp_list;  // slots grouped by waypoint, ascending slot id inside a waypoint
  // per term of the description (index into tmx_problem_desc::terms): the cart-pose instances [term_cp0, term_cp1) and the row
  // slots [term_slot0, term_slot1) it was lowered into (tmx_query_set_targets writes a query's targets there)
  std::vector<int> term_cp0, term_cp1, term_slot0, term_slot1;
  int R = 0, R2 = 0, NA = 0;           // row slots, second coefficient blocks (pair rows), penalty variables
  int n_costs = 0, n_cnts = 0;
  int n_sq = 0;
  int n_stencil = 0;      // rows of difference order 2 / 3
  int n_fx_cost = 0;
  int lvs_kmax = 2;
  int max_row_order = 0;
  // what the term loop establishes for the engine choice
  bool qp_dense = false;  // a term that needs the dense QP engine whatever else the problem holds (no term kind does today)
  bool tt_terms = false;  // TotalTime terms: dense engine, or - above its size limit - rank-one terms on the block chain
  bool tv_terms = false;  // squared JointVel-with-time costs: dense engine, or - above its size limit - joint - time entries on the dense-coupling block chain
  bool dyn_p = false;     // function COSTS (CostFromFunc / squared CostFromErrFunc): dynamic D x D objective blocks on the structured solver (round 5)
  bool stencil_rows = false;  // difference rows of order 2 / 3 (JointAcc / JointJerk Ineq costs, Eq / Ineq constraints)
  bool st_terms = false;  // function terms (any): the ST instantiations of the term code, piecewise driver
  int band = 0;           // acceleration (2) / jerk (3) squared costs: banded objective
};

// The QP engine of the problem (choose_engine): DevProblem::qp_dense / tt_chain / tv_chain / band_rows / band_pairs / st / band / n_link.
struct EngineChoice
{
  bool qp_dense = false, tt_chain = false, tv_chain = false, band_rows = false, st = false;
  bool band_pairs = false;  // squared acceleration / jerk costs next to general pair rows on the banded factorisation with a dense first coupling
                            // (together with band_rows: acceleration / jerk ROWS next to general pair rows, TMX_BAND_ROW_PAIR_CHAIN=1)
  int band = 0;
  int R2 = 0;  // Lowered::R2, or 1 for squared velocity-with-time costs on the chain without a pair row (an unused second-block slot)
  std::string dense_reasons;  // what put the problem on the dense engine, comma-joined (text of the refusal above its size limit)
};

// Test and tuning hooks of the upload.  The tests change them between uploads of one process: read at the start of every upload.
struct UploadHooks
{
  // first character of the variable ('\0': unset)
  char total_time_chain, vel_time_chain, band_pair_chain, band_row_pair_chain, force_coef_far, force_compact, row_perm, wave, tt_place;
  int dense_qp_max_n;  // size limit of the dense QP engine (QP variables incl. penalty variables); TMX_DENSE_QP_MAX_N lifts it for callers who accept the time
  bool verbose;
  static UploadHooks read()
  {
    auto first = [](const char* name) {
      const char* e = std::getenv(name);
      return e ? e[0] : '\0';
    };
    UploadHooks h;
    h.total_time_chain = first("TMX_TOTAL_TIME_CHAIN");
    h.vel_time_chain = first("TMX_VEL_TIME_CHAIN");
    h.band_pair_chain = first("TMX_BAND_PAIR_CHAIN");
    h.band_row_pair_chain = first("TMX_BAND_ROW_PAIR_CHAIN");
    h.force_coef_far = first("TMX_FORCE_COEF_FAR");
    h.force_compact = first("TMX_FORCE_COMPACT");
    h.row_perm = first("TMX_ROW_PERM");
    h.wave = first("TMX_WAVE");
    h.tt_place = first("TMX_TT_PLACE");
    const char* e = std::getenv("TMX_DENSE_QP_MAX_N");
    h.dense_qp_max_n = e ? std::max(1, std::atoi(e)) : 448;
    h.verbose = std::getenv("TMX_VERBOSE") != nullptr;
    return h;
  }
};

// Where the QP workspace lives and which thread carries which row (place_workspace).
struct Placement
{
  int coef_far = 0, setup_fast = 0, polish_fast = 0, step_fast = 0, eval_fast = 0, factor_fast = 0, tt_place = 0;  // DevProblem fields of the same names
  int wave_ok = 0, wv_gmax = 2, wv_aux2 = 0;
  // tables to upload: DevProblem::row_perm (empty: slot order), wp_pst, row_epos, wv_plan (with wave_ok only)
  std::vector<int> row_perm, pst, epos, plan;
  std::vector<unsigned long long> p_hash;  // DevProblem::p_hash (with eval_fast only)
  size_t smem_qp = 0, smem_small = 0, smem_wave = 0;  // LDS budgets (bytes)
  size_t tt_scratch = 0;                              // tmx_ctx::tt_scratch (doubles)
};
