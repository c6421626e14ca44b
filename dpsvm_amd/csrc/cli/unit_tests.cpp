// Native unit tests (run by tests/test_native_unit.py; `--gpu` adds the
// device-side cases).  The reference had no tests at all.
#include <cmath>
#include <cstdio>
#include <functional>
#include <iostream>
#include <thread>
#include <unistd.h>

#include "dpsvm/comm.hpp"
#include "dpsvm/common.hpp"
#include "dpsvm/io.hpp"
#include "dpsvm/problem.hpp"
#include "dpsvm/solver.hpp"
#include "dpsvm/ws_plan.hpp"
#include "kernels/kernels.hpp"

using namespace dpsvm;

static int g_fail = 0, g_pass = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      ++g_fail;                                                             \
      fprintf(stderr, "  FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
    } else {                                                                \
      ++g_pass;                                                             \
    }                                                                       \
  } while (0)

static void test_keys() {
  // ordering of f with lowest-index tie-break
  float vals[] = {-3.5f, -1.f, -0.f, 0.f, 1e-30f, 2.f, 1e9f, -1e9f};
  for (float a : vals)
    for (float b : vals) {
      uint64_t ka = make_key(a, 7), kb = make_key(b, 3);
      if (a < b) EXPECT(ka < kb);
      if (a > b) EXPECT(ka > kb);
      if (a == b) EXPECT(kb < ka);  // same value -> lower index wins
      EXPECT(key_value(ka) == a);
      EXPECT(key_index(ka) == 7u);
    }
}

static void test_shards() {
  for (int64_t n : {1, 2, 10, 60000, 60001})
    for (int w : {1, 2, 3, 7, 8, 10}) {
      int64_t tot = 0, prev_end = 0, mx = 0, mn = n + 1;
      for (int r = 0; r < w; ++r) {
        Shard s = shard_of(n, r, w);
        EXPECT(s.offset == prev_end);
        prev_end = s.offset + s.size;
        tot += s.size;
        mx = std::max(mx, s.size);
        mn = std::min(mn, s.size);
      }
      EXPECT(tot == n);
      EXPECT(mx - mn <= 1);
    }
}

static void test_geometry() {
  // headline (60k rows): 512 rows x 118 workgroups on 1 GPU, 15 per rank on 8
  {
    const Geometry g1 = make_geometry(60000, dense_rows_min(60000, 1));
    EXPECT(g1.rows == 512 && g1.groups == 118);
    const int64_t nl8 = (60000 + 7) / 8;
    const Geometry g8 = make_geometry(nl8, dense_rows_min(nl8, 8));
    EXPECT(g8.rows == 512 && g8.groups == 15);
  }
  for (int64_t n : {2, 1000, 60000, 200000, 581012, 786432, 2000000})
    for (int w : {1, 2, 4, 8}) {
      const int64_t nl = (n + w - 1) / w;
      const Geometry d = make_geometry(nl, dense_rows_min(nl, w));
      EXPECT(d.rows % 256 == 0 && d.rows * d.groups >= nl);
      if (nl <= 256 * 3072) {  // the persistent dense engine's range
        EXPECT(d.groups <= 256);
        EXPECT(d.rows <= 3072);
        if (nl * w <= 256 * 3072) EXPECT(w * d.groups <= 256);  // one poll batch
      }
      const Geometry c = make_geometry(nl, 0);  // cache mode: ~one workgroup per CU
      EXPECT(c.rows % 256 == 0 && c.rows * c.groups >= nl && c.groups <= 256);
    }
}

static void test_io() {
  char tmpl[] = "/tmp/dpsvm_unitXXXXXX";
  char* dir = mkdtemp(tmpl);
  EXPECT(dir != nullptr);
  std::string base = dir;
  Dataset ds = make_synthetic(Synth::Blobs, 257, 5, 3);
  write_csv(base + "/a.csv", ds);
  Dataset rd = read_csv(base + "/a.csv", 0, 0);
  EXPECT(rd.n == 257 && rd.d == 5);
  bool same = true;
  for (size_t i = 0; i < ds.x.size(); ++i) same &= ds.x[i] == rd.x[i];
  for (size_t i = 0; i < ds.y.size(); ++i) same &= ds.y[i] == rd.y[i];
  EXPECT(same);
  Dataset part = read_csv_rows(base + "/a.csv", 100, 50, 5);
  EXPECT(part.n == 50 && part.x[0] == ds.x[100 * 5] && part.y[49] == ds.y[149]);
  // model round trip (both formats)
  std::vector<float> alpha(ds.n, 0.f);
  for (int64_t i = 0; i < ds.n; i += 3) alpha[i] = 0.5f + i;
  Model m = make_model(ds, alpha, -0.25f, 0.7f);
  write_model(base + "/m.txt", m);
  Model r = read_model(base + "/m.txt");
  EXPECT(r.has_b && r.b == -0.25f && r.gamma == 0.7f && r.nsv() == m.nsv() && r.d == 5);
  EXPECT(r.x == m.x && r.alpha == m.alpha && r.y == m.y);
  write_model(base + "/l.txt", m, 9, true);
  Model l = read_model(base + "/l.txt");
  EXPECT(!l.has_b && l.b == 0.f && l.nsv() == m.nsv() && l.x == m.x);
  // checkpoint round trip
  Checkpoint ck;
  ck.n = ds.n; ck.d = 5; ck.C = 2; ck.gamma = 0.5f; ck.eps = 1e-3f; ck.iter = 17;
  ck.b_hi = -1; ck.b_lo = 1; ck.alpha = alpha; ck.f = alpha;
  write_checkpoint(base + "/c.ck", ck);
  Checkpoint c2 = read_checkpoint(base + "/c.ck");
  EXPECT(c2.n == ck.n && c2.iter == 17 && c2.alpha == ck.alpha && c2.f == ck.f && c2.C == 2.f);
  // libsvm
  FILE* fp = fopen((base + "/s.txt").c_str(), "w");
  fprintf(fp, "+1 1:1 3:1\n-1 2:0.5 4:1\n");
  fclose(fp);
  Dataset sv = read_libsvm(base + "/s.txt", 4);
  EXPECT(sv.n == 2 && sv.x[0] == 1.f && sv.x[2] == 1.f && sv.x[5] == 0.5f && sv.x[7] == 1.f && sv.y[1] == -1.f);
  std::string cmd = "rm -rf " + base;
  EXPECT(system(cmd.c_str()) == 0);
}

static SolverParams small_params() {
  SolverParams p;
  p.C = 2.f;
  p.gamma = 0.5f;
  p.eps = 1e-3f;
  p.max_iter = 100000;
  return p;
}

static void test_cpu_solver_ranks() {
  Dataset ds = make_synthetic(Synth::Blobs, 600, 4, 11, 0, -1, 1.5f);
  SolverParams p = small_params();
  SolveResult r1 = solve_cpu(ds, p);
  EXPECT(r1.status == 1);
  EXPECT(r1.iters > 10);
  // KKT sanity: alphas within the box
  bool box = true;
  for (float a : r1.alpha) box &= (a >= 0.f && a <= p.C);
  EXPECT(box);
  for (int world : {2, 3}) {
    ThreadCommGroup g(world);
    std::vector<SolveResult> rs(world);
    std::vector<std::thread> ts;
    for (int r = 0; r < world; ++r)
      ts.emplace_back([&, r] {
        auto c = g.comm(r);
        rs[r] = solve_cpu(ds, p, c.get());
      });
    for (auto& t : ts) t.join();
    // identical decisions on every rank and identical to one rank
    for (int r = 0; r < world; ++r) {
      EXPECT(rs[r].iters == r1.iters);
      EXPECT(rs[r].alpha == r1.alpha);
      EXPECT(rs[r].b == r1.b);
    }
  }
  // clip=box keeps sum(alpha*y) == 0
  p.clip = ClipMode::Box;
  SolveResult rb = solve_cpu(ds, p);
  double s = 0;
  for (int64_t i = 0; i < ds.n; ++i) s += rb.alpha[i] * ds.y[i];
  EXPECT(std::fabs(s) < 1e-2);
  EXPECT(rb.status == 1);
  // accuracy on separable-ish blobs
  Model m = make_model(ds, r1.alpha, r1.b, p.gamma);
  auto dec = decision_cpu(m, ds.x.data(), ds.n, ds.d);
  EXPECT(accuracy_from_decision(dec, ds.y.data(), ds.n) > 0.8);
}

static void test_cpu_checkpoint_resume() {
  Dataset ds = make_synthetic(Synth::Blobs, 400, 3, 5, 0, -1, 1.0f);
  SolverParams p = small_params();
  SolveResult full = solve_cpu(ds, p);
  char path[] = "/tmp/dpsvm_ckXXXXXX";
  int fd = mkstemp(path);
  close(fd);
  SolverParams pc = p;
  pc.max_iter = full.iters / 2;
  pc.checkpoint_every = full.iters / 4;
  pc.checkpoint_path = path;
  solve_cpu(ds, pc);
  Checkpoint ck = read_checkpoint(path);
  EXPECT(ck.iter > 0 && ck.iter <= pc.max_iter);
  SolveResult res = solve_cpu(ds, p, nullptr, &ck);
  EXPECT(res.iters == full.iters);
  EXPECT(res.alpha == full.alpha);
  // resume without f: f recomputed from alpha (fp order differs -> close, not equal)
  ck.f.clear();
  SolveResult res2 = solve_cpu(ds, p, nullptr, &ck);
  EXPECT(res2.status == 1);
  EXPECT(std::fabs(res2.b - full.b) < 1e-2);
  unlink(path);
}

// launch::split_gram_path: the split Gram's launch plan (kernels.hpp), shape by shape
static void test_gram_path() {
  using launch::GramPath;
  auto path = [](int64_t M, int64_t N, int64_t ldo, int dp, bool sym, bool cold, int variant = 0) {
    return launch::split_gram_path(launch::GramShape{M, N, ldo, dp, sym, cold}, variant);
  };
  // the headline: persistent wide-wave, adaptive when cold
  EXPECT(path(60000, 60000, 60032, 784, true, false) == GramPath::W64Persist);
  EXPECT(path(60000, 60000, 60032, 784, true, true) == GramPath::Adaptive);
  // 4 k blocks a row: no wide-wave path
  EXPECT(path(60000, 60000, 60032, 128, true, false) == GramPath::Glds);
  EXPECT(path(60000, 60000, 60032, 128, true, true) == GramPath::Glds);
  // more than 2^32 elements: the persistent three-product kernel indexes the output in 32 bits
  EXPECT(path(66000, 66000, 66048, 784, true, false) == GramPath::W64Grid);
  EXPECT(path(66000, 66000, 66048, 784, true, true) == GramPath::Adaptive);
  // the packed epilogue's bound: a 256-row tile of ldo floats below 2^31 bytes
  const int64_t wide = (1ll << 21) - 128;
  EXPECT(path(256, wide, wide, 784, false, false) == GramPath::W64Grid);
  EXPECT(path(256, wide, wide, 784, false, true) == GramPath::Adaptive);
  EXPECT(path(256, 1ll << 21, 1ll << 21, 784, false, false) == GramPath::Glds);
  EXPECT(path(256, 1ll << 21, 1ll << 21, 784, false, true) == GramPath::Glds);
  // operand rows beyond 32 bits: the first M with (M + 512) x 25 x 8 >= 2^31
  const int64_t m32 = ((1ll << 31) + 199) / 200 - 512;
  EXPECT((m32 + 512) * 200 >= (1ll << 31) && (m32 + 511) * 200 < (1ll << 31));
  EXPECT(path(m32, 256, 256, 784, false, false) == GramPath::W64Grid);
  EXPECT(path(m32, 256, 256, 784, false, true) == GramPath::W64Grid);
  EXPECT(path(m32 - 1, 256, 256, 784, false, true) == GramPath::Adaptive);
  // tile tables hold 16-bit tile coordinates
  EXPECT(path(65535ll * 256, 256, 256, 160, false, true) == GramPath::Adaptive);
  EXPECT(path(65535ll * 256 + 1, 256, 256, 160, false, true) == GramPath::W64Grid);
  // forced variants (the tests' hook), and one the shape cannot take
  EXPECT(path(1000, 777, 896, 784, false, false, 1) == GramPath::Tile);
  EXPECT(path(1000, 777, 896, 784, false, false, 3) == GramPath::Glds);
  EXPECT(path(1000, 777, 896, 784, false, false, 11) == GramPath::W64Grid);
  EXPECT(path(1000, 777, 896, 784, false, false, 12) == GramPath::W64Persist);
  EXPECT(path(1000, 777, 896, 784, false, true, 11) == GramPath::W64Grid);
  EXPECT(path(1000, 777, 896, 784, false, true, 12) == GramPath::Adaptive);
  EXPECT(path(1000, 777, 896, 784, false, true, 3) == GramPath::Glds);
  EXPECT(path(1000, 777, 896, 100, false, false, 12) == GramPath::Glds);
  EXPECT(path(1000, 777, 896, 100, false, false, 11) == GramPath::Glds);
  EXPECT(path(1000, 777, 896, 100, false, false, 1) == GramPath::Tile);
}

// ws_round_plan / ws_round_shape (dpsvm/ws_plan.hpp): the working-set round's shape, case by case.
// Unless stated: 60,000 rows, ws_size 192, ws_blocks auto, one rank, 256 CUs, the peer exchange's self test passes.
static void test_ws_plan() {
  struct Case {
    const char* name;
    WsPlanFacts f;
    int blocks, q_max;
  };
  auto facts = [](auto&& edit) {
    WsPlanFacts f;
    f.n = 60000;
    f.dp = 784;
    f.uncoupled = true;
    f.ws_dense = true;
    f.cus = 256;
    edit(f);
    int32_t rpt = 0;
    launch::ws_geometry((f.n + f.world - 1) / f.world, f.world, &f.ws_G, &rpt);
    return f;
  };
  auto ranks = [](WsPlanFacts& f, int world, int share) {
    f.world = world;
    f.share = share;
  };
  auto cache = [](WsPlanFacts& f, int64_t L) {
    f.ws_dense = false;
    f.ws_cache = true;
    f.L = L;
  };
  const Case cases[] = {
      {"uncoupled dense", facts([](WsPlanFacts&) {}), 128, 48},
      {"coupled dense", facts([](WsPlanFacts& f) { f.uncoupled = false; }), 32, 96},
      {"uncoupled cache, L at the bound", facts([&](WsPlanFacts& f) { cache(f, 14336); }), 64, 48},
      {"uncoupled cache, L below it", facts([&](WsPlanFacts& f) { cache(f, 14335); }), 1, 192},
      {"below the auto row count", facts([](WsPlanFacts& f) { f.n = 49999; }), 1, 192},
      {"at the auto row count", facts([](WsPlanFacts& f) { f.n = 50000; }), 128, 48},
      {"ws_size 64, coupled", facts([](WsPlanFacts& f) { f.ws_size = 64, f.uncoupled = false; }), 32, 64},
      {"ws_size 32, uncoupled", facts([](WsPlanFacts& f) { f.ws_size = 32; }), 128, 32},
      {"ws_blocks 8", facts([](WsPlanFacts& f) { f.ws_blocks = 8; }), 8, 192},
      {"ws_blocks 4, odd ws_size", facts([](WsPlanFacts& f) { f.ws_blocks = 4, f.ws_size = 95; }), 1, 95},
      {"4 ranks on one device", facts([&](WsPlanFacts& f) { ranks(f, 4, 4); }), 64, 48},
      {"8 ranks on one device", facts([&](WsPlanFacts& f) { ranks(f, 8, 8); }), 32, 48},
      {"2 ranks, own devices", facts([&](WsPlanFacts& f) { ranks(f, 2, 1); }), 128, 48},
      {"8 ranks, own devices", facts([&](WsPlanFacts& f) { ranks(f, 8, 1); }), 128, 48},
      {"4 ranks on one device, forced collectives",
       facts([&](WsPlanFacts& f) { ranks(f, 4, 4), f.force_collectives = true, f.device_comm = true; }), 128, 48},
  };
  for (const Case& c : cases) {
    const WsRoundPlan p = ws_round_plan(c.f);
    const WsRoundShape s = ws_round_resolve(c.f, p, true, true);
    const bool ok = p.error.empty() && s.blocks == c.blocks && s.q_max == c.q_max;
    if (!ok) fprintf(stderr, "  ws_plan %s: %d x %d (want %d x %d) %s\n", c.name, s.blocks, s.q_max, c.blocks, c.q_max, p.error.c_str());
    EXPECT(ok);
  }
  {  // the headline's shape in full, and the coupled one
    WsPlanFacts f = cases[0].f;
    WsRoundShape s = ws_round_resolve(f, ws_round_plan(f), true, true);
    EXPECT(s.ncand == kWsCand && s.direct_sub == 1 && s.n_new == 48 && s.inner_max == 192 && s.note.empty());
    EXPECT(ws_round_plan(f).p1G == 59 && ws_round_plan(f).ks == 4);
    f = cases[1].f;
    s = ws_round_resolve(f, ws_round_plan(f), true, true);
    EXPECT(s.ncand == kWsCandStd && s.direct_sub == 0 && s.n_new == 96 && s.inner_max == 384);
    // exchange=peer at one rank (loopback): the solve gathers through the exchange
    f = cases[0].f;
    f.exchange = 2;
    EXPECT(ws_round_resolve(f, ws_round_plan(f), true, true).direct_sub == 0);
  }
  {  // refused: ws_blocks x ws_size beyond the union capacity
    const WsPlanFacts f = facts([](WsPlanFacts& f) { f.ws_blocks = 64; });
    EXPECT(ws_round_plan(f).error.find("the round's union capacity") != std::string::npos);
  }
  {  // ws_blocks asked for, one block run: the note
    const WsRoundShape s = ws_round_resolve(cases[9].f, ws_round_plan(cases[9].f), true, true);
    EXPECT(s.note.find("one block per round") != std::string::npos && s.n_new == 95 && s.inner_max == 380);
  }
  {  // ranks sharing a device: the halved union fits the wave slots, the self test decides the carrier
    const WsPlanFacts& f = cases[10].f;
    const WsRoundPlan p = ws_round_plan(f);
    EXPECT(p.xch_resident && p.xch_waves == 4 * (64 + 16 * 64) + 1024 && p.peer_multi && !p.collectives_multi);
    EXPECT(ws_round_resolve(f, p, true, false).blocks == 1);   // self test failed, host communicator
    EXPECT(ws_round_resolve(f, p, false, true).blocks == 1);   // a peer's cache is too small
    // 8 ranks of one block each do not fit a 40-CU device: collectives, with the reason
    WsPlanFacts g = facts([&](WsPlanFacts& f) { ranks(f, 8, 8), f.cus = 40, f.n = 3000; });
    const WsRoundPlan q = ws_round_plan(g);
    EXPECT(!q.xch_resident && !q.peer_one && q.note.find("8 ranks share a device") != std::string::npos);
  }
}

template <class F>
static std::string thrown(F&& call) {
  try {
    call();
  } catch (const std::exception& e) {
    return e.what();
  }
  return "";
}
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

static void test_problem() {
  using K = ProblemKind;
  auto params = [](int problem, float nu) {
    SolverParams p;
    p.problem = problem;
    p.one_class_nu = nu;
    return p;
  };
  EXPECT(resolve_problem(params(0, 0.f)) == K::Classify);
  EXPECT(resolve_problem(params(1, 0.f)) == K::Svr);
  EXPECT(resolve_problem(params(0, 0.2f)) == K::OneClass);
  EXPECT(has(thrown([&] { resolve_problem(params(1, 0.2f)); }), "one-class: problem must be 0"));
  EXPECT(has(thrown([&] { resolve_problem(params(2, 0.f)); }), "problem must be 0 (classification) or 1"));
  EXPECT(state_rows(K::Classify, 5) == 5 && state_rows(K::Svr, 5) == 10 && state_rows(K::OneClass, 5) == 5);

  const float y[4] = {2.5f, -1.f, 0.f, 1.f};
  std::vector<float> out;
  problem_labels(K::Classify, y, 4, out);
  EXPECT((out == std::vector<float>{1.f, -1.f, -1.f, 1.f}));
  problem_labels(K::Svr, y, 4, out);
  EXPECT((out == std::vector<float>{1.f, 1.f, 1.f, 1.f, -1.f, -1.f, -1.f, -1.f}));
  problem_labels(K::OneClass, y, 4, out);
  EXPECT((out == std::vector<float>{1.f, 1.f, 1.f, 1.f}));

  OneClassStart st = one_class_start(0.25f, 8);
  EXPECT(st.full == 2 && st.rest == 0.f && st.start_rows == 2);
  st = one_class_start(0.3f, 7);  // 0.3f * 7 = 2.100000083446502685546875 in double
  EXPECT(st.full == 2 && st.rest == 0.100000083446502685546875f && st.start_rows == 3);
  st = one_class_start(0.999f, 3);  // 0.999f * 3 = 2.997000038623809814453125
  EXPECT(st.full == 2 && st.rest == 0.997000038623809814453125f && st.start_rows == 3);
  st = one_class_start(0x1.fffffep-1f, (int64_t)1 << 24);  // (1 - 2^-24) 2^24 = 2^24 - 1: never past n
  EXPECT(st.full == ((int64_t)1 << 24) - 1 && st.rest == 0.f && st.start_rows == st.full);

  // check_problem: a valid parameter set of each kind passes on the device and on the CPU; every refused setting
  // throws on both where it applies, naming the kind and the setting
  const int64_t n = 8;
  const float z[8] = {0.f, 1.f, -2.f, 3.f, 0.5f, 0.f, 1.f, 2.f};
  float z_inf[8];
  std::copy(z, z + 8, z_inf);
  z_inf[5] = INFINITY;
  auto valid = [](K kind) {
    SolverParams p;
    p.clip = ClipMode::Box;
    p.solver = 2;
    p.ws_blocks = 1;
    if (kind == K::Svr) p.problem = 1, p.svr_epsilon = 0.1f, p.C = 10.f;
    if (kind == K::OneClass) p.one_class_nu = 0.2f, p.C = 1.f;
    return p;
  };
  auto site = [&](bool device) { return ProblemSite{n, 1, false, false, n, z, device}; };
  struct Refusal {
    const char* keyword;
    int kinds;     // 1 epsilon-SVR, 2 one-class, 3 both
    bool cpu;      // refused by solve_cpu too (else: an engine-level row)
    std::function<void(SolverParams&, ProblemSite&)> set;
  };
  const Refusal table[] = {
      {"box", 3, true, [](SolverParams& p, ProblemSite&) { p.clip = ClipMode::Independent; }},
      {"comm", 3, true, [](SolverParams&, ProblemSite& s) { s.world = 2; }},
      {"per-row C", 3, true, [](SolverParams&, ProblemSite& s) { s.row_C = true; }},
      {"resume", 3, true, [](SolverParams&, ProblemSite& s) { s.resume = true; }},
      {"checkpoints", 3, true, [](SolverParams& p, ProblemSite&) { p.checkpoint_every = 5; }},
      {"collectives", 3, false, [](SolverParams& p, ProblemSite&) { p.force_collectives = true; }},
      {"peer exchange", 3, false, [](SolverParams& p, ProblemSite&) { p.exchange = 2; }},
      {"solver", 3, false, [](SolverParams& p, ProblemSite&) { p.solver = 1; }},
      {"solver", 3, false, [](SolverParams& p, ProblemSite&) { p.solver = 0; }},
      {"solver", 3, false, [](SolverParams& p, ProblemSite&) { p.engines = 1; }},
      {"ws_blocks", 3, false, [](SolverParams& p, ProblemSite&) { p.ws_blocks = 8; }},
      {"ws_blocks", 3, false, [](SolverParams& p, ProblemSite&) { p.ws_blocks = 0; }},
      {"cache", 3, false, [](SolverParams& p, ProblemSite&) { p.force_cache = true; }},
      {"cache", 3, false, [](SolverParams& p, ProblemSite&) { p.cache_lines = 1000; }},
      {"cache", 3, false, [](SolverParams& p, ProblemSite&) { p.host_cache_lines = 10; }},
      {"cache", 3, false, [](SolverParams& p, ProblemSite&) { p.ws_recompute = 1; }},
      {"partitioned", 3, false, [](SolverParams& p, ProblemSite&) { p.x_mode = 2; }},
      {"partitioned", 3, false, [](SolverParams&, ProblemSite& s) { s.n_x_rows = 4; }},
      {"svr_epsilon", 1, true, [](SolverParams& p, ProblemSite&) { p.svr_epsilon = -1.f; }},
      {"svr_epsilon", 1, true, [](SolverParams& p, ProblemSite&) { p.svr_epsilon = NAN; }},
      {"31 bits", 1, true, [](SolverParams&, ProblemSite& s) { s.n = s.n_x_rows = (int64_t)1 << 30, s.targets = nullptr; }},
      {"finite", 1, true, [&](SolverParams&, ProblemSite& s) { s.targets = z_inf; }},
      {"(0, 1)", 2, true, [](SolverParams& p, ProblemSite&) { p.one_class_nu = 1.f; }},
      {"(0, 1)", 2, true, [](SolverParams& p, ProblemSite&) { p.one_class_nu = -0.1f; }},
      {"C must be 1", 2, true, [](SolverParams& p, ProblemSite&) { p.C = 2.f; }},
  };
  for (K kind : {K::Svr, K::OneClass})
    for (bool device : {true, false}) {
      EXPECT(thrown([&] { check_problem(kind, valid(kind), site(device)); }).empty());
      for (const Refusal& r : table) {
        if (!(r.kinds & (kind == K::Svr ? 1 : 2))) continue;
        SolverParams p = valid(kind);
        ProblemSite s = site(device);
        r.set(p, s);
        const std::string msg = thrown([&] { check_problem(kind, p, s); });
        if (device || r.cpu) {
          EXPECT(has(msg, problem_name(kind)) && has(msg, r.keyword));
          EXPECT(msg.find(problem_name(kind)) < msg.find(r.keyword));
        } else {
          EXPECT(msg.empty());  // an engine-level setting: nothing of the CPU solver's
        }
      }
    }
  {  // a classifier is refused nothing here, whatever the settings
    SolverParams p;
    p.clip = ClipMode::Independent, p.ws_blocks = 8, p.x_mode = 2, p.checkpoint_every = 5;
    EXPECT(thrown([&] { check_problem(K::Classify, p, ProblemSite{n, 4, true, true, 2, nullptr, true}); }).empty());
  }

  EXPECT(thrown([] { require_classifier(K::Classify, "platt_fit"); }).empty());
  for (K kind : {K::Svr, K::OneClass}) {
    const std::string msg = thrown([&] { require_classifier(kind, "platt_fit"); });
    EXPECT(has(msg, "platt_fit") && has(msg, problem_name(kind)));
  }
  EXPECT(std::string(problem_note(K::Classify)).empty());
  EXPECT(has(problem_note(K::Svr), "epsilon-SVR") && has(problem_note(K::OneClass), "one-class"));
}

static void test_gpu() {
  if (device_count() == 0) {
    printf("  (no GPU: device tests skipped)\n");
    return;
  }
  Dataset ds = make_synthetic(Synth::Blobs, 3000, 20, 9, 0, -1, 1.0f);
  SolverParams p = small_params();
  p.gamma = 0.05f;
  SolveResult rc = solve_cpu(ds, p);
  for (int mode = 0; mode < 3; ++mode) {
    SolverParams pg = p;
    pg.engines = 1;                       // the pair-at-a-time cache / partitioned engines (quarantined)
    if (mode == 1) pg.cache_lines = 64;   // LRU + speculation
    if (mode == 2) pg.x_mode = 2;         // partitioned records, LRU
    GpuSolver s(pg, nullptr, 0);
    s.setup(ds.x.data(), ds.n, ds.n, ds.d, ds.y.data());
    SolveResult rg = s.solve();
    EXPECT(rg.status == 1);
    int64_t nsv_c = 0, nsv_g = 0;
    for (int64_t i = 0; i < ds.n; ++i) { nsv_c += rc.alpha[i] > 0; nsv_g += rg.alpha[i] > 0; }
    printf("  gpu mode %d: iters %lld (cpu %lld)  nsv %lld (cpu %lld)  b %g (cpu %g)\n", mode,
           (long long)rg.iters, (long long)rc.iters, (long long)nsv_g, (long long)nsv_c, rg.b, rc.b);
    EXPECT(std::llabs(nsv_g - nsv_c) <= std::max<int64_t>(3, nsv_c / 50));
    EXPECT(std::fabs(rg.b - rc.b) < 2e-2);
    double acc = s.train_accuracy(rg);
    Model m = make_model(ds, rc.alpha, rc.b, p.gamma);
    double accc = accuracy_from_decision(decision_cpu(m, ds.x.data(), ds.n, ds.d), ds.y.data(), ds.n);
    EXPECT(std::fabs(acc - accc) < 0.02);
  }
}

int main(int argc, char** argv) {
  bool gpu = argc > 1 && std::string(argv[1]) == "--gpu";
  std::vector<std::pair<const char*, std::function<void()>>> tests = {
      {"keys", test_keys},
      {"shards", test_shards},
      {"io", test_io},
      {"cpu_solver_ranks", test_cpu_solver_ranks},
      {"cpu_checkpoint_resume", test_cpu_checkpoint_resume},
      {"gram_path", test_gram_path},
      {"ws_plan", test_ws_plan},
      {"problem", test_problem},
  };
  if (gpu) tests.push_back({"gpu", test_gpu});
  for (auto& [name, fn] : tests) {
    int before = g_fail;
    try {
      fn();
    } catch (const std::exception& e) {
      ++g_fail;
      fprintf(stderr, "  EXCEPTION in %s: %s\n", name, e.what());
    }
    printf("%-28s %s\n", name, g_fail == before ? "ok" : "FAILED");
  }
  printf("%d checks passed, %d failed\n", g_pass, g_fail);
  return g_fail ? 1 : 0;
}
