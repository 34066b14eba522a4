// Test program for the self-collision side of the trajectory check in the C++ host layer (include/tmx_trajopt.hpp:
// setSelfCollisionPairs, checkSelfTrajectories, bestPerQuery(cfg)).  TEST CODE; built and driven by tests/test_cpp_check_self.py.
// Reads one robot, the start state, the goal, the check's settings and the seeds from a text file written by the Python test (hex
// floats), builds configuration 0 (joint-velocity cost + goal joint-position constraint, start fixed) at 6 waypoints without an
// obstacle, names the moving links link0 .. link6, sets the pairs (link6, link2), (link4, link2) BY NAME before anything is uploaded and
// prints
//   SELF <trajectory> <free> <worst: step primitive_a primitive_b substate min_distance> <min_distance x T> <penetration x T>
// for the seeds before optimize(), AFTER ... the same for the iterates after optimize() (the class has uploaded the problem again in
// between: the pairs must have survived), and
//   BEST <index in the batch> <found> <cost> <clearance> <trajectory ...>
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
  const DblVec& goal = vectors.at("goal");
  const DblVec& flat = vectors.at("seeds");
  const DblVec& cf = vectors.at("cfg");  // evaluator_type, max_substates, margin, longest_valid_segment_length
  const std::size_t nv = static_cast<std::size_t>(steps * D);
  for (int k = 0; k < D; ++k)
    rob->link_names.push_back("link" + std::to_string(k));
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
  pci.init_info.data.data = goal;
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
  jp->targets = goal;
  jp->first_step = steps - 1;
  jp->last_step = steps - 1;
  jp->name = "joint_pos";
  jp->term_type = TermType::TT_CNT;
  pci.cnt_infos.push_back(jp);
  auto prob = ConstructProblem(pci);
  std::vector<DblVec> seeds;
  for (std::size_t o = 0; o + nv <= flat.size(); o += nv)
    seeds.emplace_back(flat.begin() + static_cast<std::ptrdiff_t>(o), flat.begin() + static_cast<std::ptrdiff_t>(o + nv));
  tmx::sco::CollisionCheckConfig cfg;
  cfg.evaluator_type = static_cast<int>(cf[0]);
  cfg.max_substates = static_cast<int>(cf[1]);
  cfg.margin = cf[2];
  cfg.longest_valid_segment_length = cf[3];
  auto print = [](const char* tag, const BasicTrustRegionSQPBatchedHip::SelfTrajectoryCheck& r) {
    for (std::size_t b = 0; b < r.worst.size(); ++b)
    {
      const tmx_check_self_worst& w = r.worst[b];
      std::printf("%s %zu %d %d %d %d %d %a", tag, b, r.free[b] ? 1 : 0, w.step, w.primitive_a, w.primitive_b, w.substate, w.min_distance);
      for (double v : r.min_distance[b])
        std::printf(" %a", v);
      for (double v : r.penetration[b])
        std::printf(" %a", v);
      std::printf("\n");
    }
  };
  int fail = 0;
  try
  {
    BasicTrustRegionSQPBatchedHip opt(prob);
    // an unknown link name throws and leaves the pairs alone
    bool thrown = false;
    try
    {
      opt.setSelfCollisionPairs(std::vector<std::pair<std::string, std::string>>{ { "link6", "no_such_link" } });
    }
    catch (const std::runtime_error& e)
    {
      thrown = std::string(e.what()).find("no_such_link") != std::string::npos;
    }
    fail += thrown ? 0 : 1;
    opt.setSelfCollisionPairs(std::vector<std::pair<std::string, std::string>>{ { "link6", "link2" }, { "link4", "link2" } });
    const auto before = opt.checkSelfTrajectories(cfg, seeds);  // (uploads the problem, then the pairs)
    fail += before.worst.size() != seeds.size();
    print("SELF", before);
    int32_t n_pairs = 0, n_prim = 0;
    fail += tmx_check_link_pairs(opt.context(), &n_pairs, &n_prim) != TMX_OK || n_pairs != 2;
    opt.initialize(seeds);
    opt.optimize();  // (uploads again)
    int32_t n_again = 0, n_prim_again = 0;
    fail += tmx_check_link_pairs(opt.context(), &n_again, &n_prim_again) != TMX_OK || n_again != 2 || n_prim_again != n_prim;
    const auto after = opt.checkSelfTrajectories(cfg);
    fail += after.worst.size() != seeds.size();
    print("AFTER", after);
    const auto best = opt.bestPerQuery(cfg);
    fail += best.index.size() != 1;
    std::printf("BEST %lld %d %a %a", static_cast<long long>(best.index[0]), best.found[0] ? 1 : 0, best.total_cost[0], best.min_distance[0]);
    for (double v : best.x[0])
      std::printf(" %a", v);
    std::printf("\n");
    if (best.index[0] >= 0)
      fail += !after.free[static_cast<std::size_t>(best.index[0])];
    // a refusal of the library arrives with its reason (the problem is uploaded: at once), and the pairs stay
    thrown = false;
    try
    {
      opt.setSelfCollisionPairs(std::vector<std::pair<int, int>>{ { 3, 3 } });
    }
    catch (const std::runtime_error& e)
    {
      thrown = std::string(e.what()).find("itself") != std::string::npos;
    }
    fail += thrown ? 0 : 1;
    fail += tmx_check_link_pairs(opt.context(), &n_again, nullptr) != TMX_OK || n_again != 2;
    // by index: the same pairs, the same bytes
    opt.setSelfCollisionPairs(std::vector<std::pair<int, int>>{ { 6, 2 }, { 4, 2 } });
    const auto by_index = opt.checkSelfTrajectories(cfg);
    fail += by_index.min_distance != after.min_distance || by_index.penetration != after.penetration;
    opt.setSelfCollisionPairs(std::vector<std::pair<int, int>>{});
    fail += tmx_check_link_pairs(opt.context(), &n_again, nullptr) != TMX_OK || n_again != 0;
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
