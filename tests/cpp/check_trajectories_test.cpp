// Test program for the trajectory collision check of the C++ host layer (include/tmx_trajopt.hpp: CollisionCheckConfig,
// checkTrajectories, bestPerQuery(cfg)).  TEST CODE; built and driven by tests/test_cpp_check_trajectories.py.
// Reads one robot, the start state, the goals of the queries, one sphere obstacle, the check's settings and the seeds from a text file
// written by the Python test (hex floats), builds configuration 0 (joint-velocity cost + goal joint-position constraint, start fixed)
// at 6 waypoints next to the obstacle the way multi_query_test.cpp does, and prints
//   CHECK <trajectory> <free> <worst: step primitive obstacle substate min_distance> <min_distance x T> <penetration x T>
// for the seeds BEFORE optimize() (as the reference's tests check the initial trajectory) and, after optimize(),
//   BEST <query> <index in the batch> <found> <cost> <clearance> <trajectory ...>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <string>

#include "tmx_trajopt.hpp"

using namespace tmx;
using namespace tmx::trajopt;
using tmx::sco::BasicTrustRegionSQPBatchedHip;

static double rd(std::istream& f)
{
  std::string t;
  if (!(f >> t))
    throw std::runtime_error("unexpected end of input");
  return std::strtod(t.c_str(), nullptr);  // (C99 hex floats: operator>> does not parse those)
}

int main(int argc, char** argv)
{
  if (argc < 2)
    return 2;
  std::ifstream f(argv[1]);
  if (!f)
    return 2;
  auto rob = std::make_shared<JointGroup>();
  std::map<std::string, DblVec> vectors;
  std::string tok;
  while (f >> tok)
  {
    if (tok == "robot")
    {
      std::string name;
      int D = 0;
      f >> name >> D >> rob->tip_link;
      rob->joints.resize(static_cast<std::size_t>(D));
      rob->lower.resize(static_cast<std::size_t>(D));
      rob->upper.resize(static_cast<std::size_t>(D));
      for (int j = 0; j < D; ++j)
      {
        tmx_joint& jt = rob->joints[static_cast<std::size_t>(j)];
        jt = tmx_joint{};
        f >> jt.type;
        for (double& v : jt.origin)
          v = rd(f);
        for (double& v : jt.axis)
          v = rd(f);
        rob->lower[static_cast<std::size_t>(j)] = rd(f);
        rob->upper[static_cast<std::size_t>(j)] = rd(f);
        rob->joint_names.push_back("j" + std::to_string(j));
      }
      for (double& v : rob->base.m)
        v = rd(f);
      for (double& v : rob->tool.m)
        v = rd(f);
      int ns = 0;
      f >> ns;
      rob->link_spheres.resize(static_cast<std::size_t>(ns));
      for (auto& s : rob->link_spheres)
      {
        s = tmx_link_sphere{};
        f >> s.link;
        for (double& v : s.center)
          v = rd(f);
        s.radius = rd(f);
      }
    }
    else if (tok == "vector")
    {
      std::string name;
      std::size_t n = 0;
      f >> name >> n;
      DblVec v(n);
      for (double& x : v)
        x = rd(f);
      vectors[name] = v;
    }
    else
      return 2;
  }
  const int steps = 6, D = 7;
  const DblVec& start = vectors.at("start");
  const DblVec& goals = vectors.at("goals");  // n_queries x 7; query 0 = the problem's own goal
  const DblVec& flat = vectors.at("seeds");
  const DblVec& ob = vectors.at("obstacle");  // centre, radius
  const DblVec& cf = vectors.at("cfg");       // evaluator_type, max_substates, margin, longest_valid_segment_length
  const std::size_t nv = static_cast<std::size_t>(steps * D), Q = goals.size() / static_cast<std::size_t>(D);
  auto env = std::make_shared<Environment>();
  env->manipulators["right_arm"] = rob;
  env->state["right_arm"] = start;
  tmx_obstacle_sphere sphere{};
  sphere.center[0] = ob[0];
  sphere.center[1] = ob[1];
  sphere.center[2] = ob[2];
  sphere.radius = ob[3];
  env->obstacles.push_back(sphere);
  ProblemConstructionInfo pci(env);
  pci.basic_info.n_steps = steps;
  pci.basic_info.manip = "right_arm";
  pci.basic_info.fixed_timesteps = { 0 };
  pci.resolveKin();
  pci.init_info.type = InitInfo::JOINT_INTERPOLATED;
  pci.init_info.data = TrajArray(1, D);
  pci.init_info.data.data = DblVec(goals.begin(), goals.begin() + D);
  auto jv = std::make_shared<JointVelTermInfo>();
  jv->coeffs = DblVec(D, 1.0);
  jv->targets = DblVec(D, 0.0);
  jv->first_step = 0;
  jv->last_step = steps - 1;
  jv->name = "joint_vel";
  jv->term_type = TermType::TT_COST;
  pci.cost_infos.push_back(jv);
  auto jp = std::make_shared<JointPosTermInfo>();
  jp->coeffs = DblVec(D, 1.0);
  jp->targets = DblVec(goals.begin(), goals.begin() + D);
  jp->first_step = steps - 1;
  jp->last_step = steps - 1;
  jp->name = "joint_pos";
  jp->term_type = TermType::TT_CNT;
  pci.cnt_infos.push_back(jp);
  auto prob = ConstructProblem(pci);
  std::vector<DblVec> seeds;
  for (std::size_t o = 0; o + nv <= flat.size(); o += nv)
    seeds.emplace_back(flat.begin() + static_cast<std::ptrdiff_t>(o), flat.begin() + static_cast<std::ptrdiff_t>(o + nv));
  std::vector<DblVec> targets;
  for (std::size_t q = 0; q < Q; ++q)
    targets.emplace_back(goals.begin() + static_cast<std::ptrdiff_t>(q * D), goals.begin() + static_cast<std::ptrdiff_t>((q + 1) * D));
  tmx::sco::CollisionCheckConfig cfg;
  cfg.evaluator_type = static_cast<int>(cf[0]);
  cfg.max_substates = static_cast<int>(cf[1]);
  cfg.margin = cf[2];
  cfg.longest_valid_segment_length = cf[3];
  int fail = 0;
  try
  {
    // the defaults of the mirror are the library's
    tmx_check_config dflt;
    tmx_default_check_config(&dflt);
    const tmx_check_config mine = tmx::sco::CollisionCheckConfig().toTmx();
    fail += (dflt.evaluator_type != mine.evaluator_type) + (dflt.max_substates != mine.max_substates) + (dflt.margin != mine.margin) +
            (dflt.longest_valid_segment_length != mine.longest_valid_segment_length);
    BasicTrustRegionSQPBatchedHip opt(prob);
    const auto before = opt.checkTrajectories(cfg, seeds);
    if (before.min_distance.size() != seeds.size() || before.worst.size() != seeds.size())
      return 1;
    for (std::size_t b = 0; b < seeds.size(); ++b)
    {
      const tmx_check_worst& w = before.worst[b];
      std::printf("CHECK %zu %d %d %d %d %d %a", b, before.free[b] ? 1 : 0, w.step, w.primitive, w.obstacle, w.substate, w.min_distance);
      for (double v : before.min_distance[b])
        std::printf(" %a", v);
      for (double v : before.penetration[b])
        std::printf(" %a", v);
      std::printf("\n");
    }
    opt.setQueries(static_cast<int>(Q));
    opt.setQueryTargets(1, targets);  // term 1: the goal constraint (term 0 is the velocity cost)
    opt.initialize(seeds);
    opt.optimize();
    const auto best = opt.bestPerQuery(cfg);
    if (best.index.size() != Q || best.x.size() != Q || best.min_distance.size() != Q)
      return 1;
    // the current iterates (no trajectories given) are the batch results
    const auto after = opt.checkTrajectories(cfg);
    fail += after.min_distance.size() != seeds.size();
    for (std::size_t q = 0; q < Q; ++q)
    {
      std::printf("BEST %zu %lld %d %a %a", q, static_cast<long long>(best.index[q]), best.found[q] ? 1 : 0, best.total_cost[q], best.min_distance[q]);
      for (double v : best.x[q])
        std::printf(" %a", v);
      std::printf("\n");
      if (best.index[q] >= 0)
      {
        const std::size_t b = static_cast<std::size_t>(best.index[q]), S = seeds.size() / Q;
        fail += (b / S != q) + (best.x[q] != opt.batchResults()[b].x) + (best.total_cost[q] != opt.batchResults()[b].total_cost) + !after.free[b] +
                (after.worst[b].min_distance != best.min_distance[q]);
      }
    }
    // a refusal of the library arrives with its reason
    tmx::sco::CollisionCheckConfig bad = cfg;
    bad.evaluator_type = 7;
    bool thrown = false;
    try
    {
      opt.checkTrajectories(bad, seeds);
    }
    catch (const std::runtime_error& e)
    {
      thrown = std::string(e.what()).find("evaluator_type") != std::string::npos;
    }
    fail += thrown ? 0 : 1;
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
  if (fail)
    std::fprintf(stderr, "%d checks failed\n", fail);
  return fail ? 1 : 0;
}
