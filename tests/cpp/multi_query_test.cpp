// Test program for the multi-query operations of the C++ host layer (include/tmx_trajopt.hpp: setQueries, setQueryTargets,
// bestPerQuery).  TEST CODE; built and driven by tests/test_cpp_multi_query.py.
// Reads one robot, the start state, the goals of the queries and the seeds from a text file written by the Python test (hex floats),
// builds configuration 0 (joint-velocity cost + goal joint-position constraint, start fixed) at 6 waypoints the way host_api_test.cpp
// does, runs the seeds as `n_queries` queries that differ in the goal, and prints one line per query:
//   BEST <query> <index in the batch> <found> <cost> <trajectory ...>
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
  const std::size_t nv = static_cast<std::size_t>(steps * D), Q = goals.size() / static_cast<std::size_t>(D);
  auto env = std::make_shared<Environment>();
  env->manipulators["right_arm"] = rob;
  env->state["right_arm"] = start;
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
  int fail = 0;
  try
  {
    BasicTrustRegionSQPBatchedHip opt(prob);
    opt.setQueries(static_cast<int>(Q));
    opt.setQueryTargets(1, targets);  // term 1: the goal constraint (term 0 is the velocity cost)
    opt.initialize(seeds);
    opt.optimize();
    const auto& best = opt.bestPerQuery();
    if (best.index.size() != Q || best.x.size() != Q)
      return 1;
    for (std::size_t q = 0; q < Q; ++q)
    {
      std::printf("BEST %zu %lld %d %a", q, static_cast<long long>(best.index[q]), best.found[q] ? 1 : 0, best.total_cost[q]);
      for (double v : best.x[q])
        std::printf(" %a", v);
      std::printf("\n");
      // the winner is a seed of its own query, and the trajectory is that seed's
      if (best.index[q] >= 0)
      {
        const std::size_t b = static_cast<std::size_t>(best.index[q]), S = seeds.size() / Q;
        fail += (b / S != q) + (best.x[q] != opt.batchResults()[b].x) + (best.total_cost[q] != opt.batchResults()[b].total_cost);
      }
    }
    // a term without a per-query target is refused by the library, with its reason
    BasicTrustRegionSQPBatchedHip bad(prob);
    bad.setQueries(static_cast<int>(Q));
    bad.setQueryTargets(0, targets);
    bad.initialize(seeds);
    bool thrown = false;
    try
    {
      bad.optimize();
    }
    catch (const std::runtime_error& e)
    {
      thrown = std::string(e.what()).find("no per-query target") != std::string::npos;
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
