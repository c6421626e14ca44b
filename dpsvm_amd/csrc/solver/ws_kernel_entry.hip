// Kernel-level test entry points of the working-set engine (ws_*.hip): each
// runs ONE kernel (or the two f-update passes) on crafted device state and
// returns the state it leaves, so tests/test_ws_kernels_gpu.py can check the
// merge (sort, stop test, union, block assignment), the LDS pair loop and the
// line-search f update against float64 numpy models of the same rules —
// independently of the end-to-end solves (tests/test_ws_gpu.py), where one
// kernel's bug could hide behind another's.
//
//   ws_merge_multi_probe    ws_rank_merge: the multi-block merge (sort, stop test, union, block layout)
//   ws_solve_probe          ws_solve: the LDS pair loop, one or P blocks
//   ws_select_probe         ws_select: the f update and candidate lists (one pass; two passes with the line
//                           search; list slices; the wide pass 1)
//   ws_gather_probe         ws_gather, dense, one block: the one-block merge of ws_merge.hpp (lists folded
//                           four to a thread, stop codes, radix threshold, class order, dedup, previous-set
//                           retention) and the sub-Gram rows / aux gathered from a resident Gram
//   ws_subgram_split_probe  ws_subgram_split: the same merge, and the sub-Gram tiles computed from the split X
//                           rows — the resident split Gram's bits, zeros in the columns past q
//   ws_fupdate_split_probe  ws_fupdate_split: the recompute rounds' selection pass — f in the documented
//                           summation order over the split Gram's bits, the candidate lists, the stop states
//   ws_merge_cache_probe    ws_merge: the same merge through its third kernel, then the cache-mode line plan
//                           (hits keep their line, misses take victims after the CLOCK hand, pinned lines are
//                           skipped, the evicted rows lose their line, the hand moves); with lines,
//                           ws_gather_lines on the planned lines
//   ws_merge_multi_cache_probe  ws_rank_merge with WsArgs::cache: the multi-block merge and the line plan of its
//                           union; with lines, ws_gather_multi reading WsCtrl::line
//   ws_pack_rows_probe      ws_pack_rows: the misses' X rows packed for a partitioned X
//   ws_solve_direct_probe   ws_solve with WsArgs::direct_sub: the blocks' sub-Grams straight from the resident Gram
//                           (tests/test_ws_direct_kernels_gpu.py)
//   ws_shard_round_probe    one stage of a round once per rank of a sharded run (off / nl of shard_of, own control
//                           record, f shard and Gram panel), in the collectives or the peer-exchange form
//                           (tests/test_ws_shard_kernels_gpu.py)
// (tests/test_ws_kernels_gpu.py the first three, tests/test_ws_recompute_kernels_gpu.py the next three,
// tests/test_ws_cache_kernels_gpu.py the last three and kernel_entry.hip's rbf_rows_miss.)  A
// probe checks its arguments before it launches: a malformed call raises.
//
// Reference rules: the I-set classification and selection functors
// (svmTrain.cu:41-95, 400-467), the pair update and clipping
// (svmTrainMain.cpp:282-299), the f update (svmTrain.cu:98-137).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <functional>
#include <limits>

#include "probe_util.hpp"

namespace dpsvm {
namespace kernels {

using probe::Arena;
using probe::blank_ctrl;
using probe::EventTimer;
using probe::single_rank_args;
using probe::time_launches;
using probe::to_f32;

GramWsumProbe gram_rows_wsum_probe(const std::vector<float>& gram, int64_t L, int64_t ldg, int64_t n,
                                   const std::vector<int32_t>& lines, const std::vector<float>& coef,
                                   const std::vector<float>& base, int reps) {
  DPSVM_CHECK(n >= 1 && L >= 0 && ldg >= n && (int64_t)gram.size() == L * ldg,
              "gram_rows_wsum_probe: gram [L][ldg >= n], n >= 1");
  DPSVM_CHECK(lines.empty() || lines.size() == coef.size(), "gram_rows_wsum_probe: one coefficient per line");
  DPSVM_CHECK(base.empty() || (int64_t)base.size() == n, "gram_rows_wsum_probe: base of n entries (or none)");
  const int64_t m = (int64_t)coef.size();
  DPSVM_CHECK(!lines.empty() || m <= L, "gram_rows_wsum_probe: identity lines need m <= L");
  for (int32_t l : lines) DPSVM_CHECK(l >= 0 && l < L, "gram_rows_wsum_probe: line out of range");
  DPSVM_CHECK(reps >= 0, "gram_rows_wsum_probe: reps >= 0");
  Arena st;
  const float* dg = st.up(gram, gram.size());
  const int32_t* dl = lines.empty() ? nullptr : st.up(lines, lines.size());
  const float* dc = st.up(coef, coef.size());
  const float* db = base.empty() ? nullptr : st.up(base, base.size());
  const size_t n_out = (size_t)((n + 3) / 4 * 4) + kGramWsumProbePad;
  float* dout = st.up(std::vector<float>(n_out, kGramWsumProbeFill), n_out);
  double* part = st.alloc<double>((size_t)launch::gram_wsum_scratch_doubles(n));
  const auto wsum = [&] { launch::gram_rows_wsum(dg, L, ldg, n, dl, dc, m, db, dout, part, st.s); };
  GramWsumProbe r;
  r.slices = launch::gram_wsum_slices(n, m);
  r.us = to_f32(time_launches(st.s, reps, wsum));
  wsum();
  r.out = st.down(dout, n_out);
  return r;
}

GramDotProbe gram_rows_dot_probe(const std::vector<float>& Kt, int64_t nt, int64_t ld, int64_t n,
                                 const std::vector<float>& coef, int64_t ldc, int k, const std::vector<float>& b,
                                 int reps) {
  DPSVM_CHECK(nt >= 1 && n >= 1 && k >= 1 && ld >= n && ldc >= n, "gram_rows_dot_probe: nt, n, k >= 1, ld, ldc >= n");
  DPSVM_CHECK((int64_t)Kt.size() == nt * ld && (int64_t)coef.size() == (int64_t)k * ldc && (int64_t)b.size() == k,
              "gram_rows_dot_probe: Kt [nt][ld], coef [k][ldc], b [k]");
  DPSVM_CHECK(reps >= 0, "gram_rows_dot_probe: reps >= 0");
  Arena st;
  const float* dk = st.up(Kt, Kt.size());
  const float* dc = st.up(coef, coef.size());
  const float* db = st.up(b, b.size());
  const size_t n_out = (size_t)nt * k + 2 * kGramDotProbePad;
  float* dout = st.up(std::vector<float>(n_out, kGramDotProbeFill), n_out);
  const auto dot = [&] { launch::gram_rows_dot(dk, nt, ld, n, dc, ldc, k, db, dout + kGramDotProbePad, k, st.s); };
  GramDotProbe r;
  r.us = to_f32(time_launches(st.s, reps, dot));
  dot();
  r.out = st.down(dout, n_out);
  return r;
}

namespace {

// the cache-mode state a probe uploads: maps that are mutual inverses, every entry and the hand in range
void check_cache_maps(int64_t n, int64_t L, int hand, const std::vector<int32_t>& slot_of,
                      const std::vector<int32_t>& key_of) {
  DPSVM_CHECK(n >= 1 && n < ((int64_t)1 << 31) && L >= 1 && L < ((int64_t)1 << 31) && (int64_t)slot_of.size() == n &&
                  (int64_t)key_of.size() == L,
              "ws cache probe: slot_of of n rows, key_of of L lines");
  DPSVM_CHECK(hand >= 0 && hand < L, "ws cache probe: the hand must be a line");
  for (int64_t r = 0; r < n; ++r) {
    const int64_t l = slot_of[r];
    DPSVM_CHECK(l >= -1 && l < L, "ws cache probe: slot_of entry out of range");
    DPSVM_CHECK(l < 0 || key_of[l] == r, "ws cache probe: slot_of / key_of are not inverses");
  }
  for (int64_t l = 0; l < L; ++l) {
    const int64_t r = key_of[l];
    DPSVM_CHECK(r >= -1 && r < n, "ws cache probe: key_of entry out of range");
    DPSVM_CHECK(r < 0 || slot_of[r] == l, "ws cache probe: slot_of / key_of are not inverses");
  }
}

// the cache fields of a control record before the launch (kernel_probes.hpp)
void blank_cache_ctrl(WsCtrl& c, int hand) {
  c.hand = hand;
  c.n_miss = kWsProbeMiss;
  c.rows_computed = kWsProbeRowsComputed;
  c.row_hits = kWsProbeRowHits;
  for (int i = 0; i < kWsMaxAll; ++i) c.miss_row[i] = c.miss_line[i] = -1;
}

WsCacheState cache_state(Arena& st, const WsCtrl& o, const WsArgs& a, int64_t n) {
  WsCacheState r;
  r.n_miss = o.n_miss;
  r.hand = o.hand;
  r.rows_computed = o.rows_computed;
  r.row_hits = o.row_hits;
  r.miss_row.assign(o.miss_row, o.miss_row + kWsMaxAll);
  r.miss_line.assign(o.miss_line, o.miss_line + kWsMaxAll);
  r.slot_of = st.down(a.slot_of, (size_t)n);
  r.key_of = st.down(a.key_of, (size_t)a.L);
  return r;
}

void check_merge_multi(const std::vector<uint64_t>& cand, int G, int blocks, int q_max,
                       const std::vector<int32_t>& prev_union) {
  DPSVM_CHECK(G >= 1 && G <= kWsMaxGroups && (int64_t)cand.size() == (int64_t)G * 2 * kWsCand,
              "ws_merge_multi_probe: cand must be [G][2][kWsCand = 16] with G <= 256");
  DPSVM_CHECK(blocks >= 2 && blocks <= kWsMaxBlocks && q_max >= 2 && q_max <= kWsMax && q_max % 2 == 0,
              "ws_merge_multi_probe: 2 <= blocks <= 128, blocks x q_max <= 6144, even q_max <= 192");
  DPSVM_CHECK((int64_t)prev_union.size() <= (int64_t)blocks * q_max, "ws_merge_multi_probe: previous union too long");
}

// control record (round 1: it builds parity 1, the previous union sits in parity 0) and arguments of one
// multi-block merge
struct MergeMultiRound {
  std::unique_ptr<WsCtrl> c = blank_ctrl();
  WsArgs a = single_rank_args();
  MergeMultiRound(Arena& st, const std::vector<uint64_t>& cand, int G, int blocks, int p_act, int q_max, int n_new,
                  float eps, const std::vector<int32_t>& prev_union, int64_t iter, int64_t max_iter) {
    c->outer = 1;
    c->iter = iter;
    c->uq[0] = (int32_t)prev_union.size();
    for (size_t i = 0; i < prev_union.size(); ++i) c->uidx[0][i] = prev_union[i];
    c->p_act = p_act;
    for (int i = 0; i < kWsMaxAll; ++i) c->idx[1][i] = c->line[1][i] = -1;
    a.cand = a.cand_out = st.up(cand, cand.size());
    a.G = a.G_all = G;
    a.blocks = blocks;
    a.q_max = q_max;
    a.n_new = n_new;
    a.eps = eps;
    a.max_iter = max_iter;
    a.sorted = st.alloc<uint64_t>((size_t)2 * kWsMaxGroups * kWsCand);
  }
  static WsMergeProbe result(const WsCtrl& o, int blocks, int q_max) {
    WsMergeProbe r;
    r.done = o.done;
    r.b_hi = o.b_hi;
    r.b_lo = o.b_lo;
    r.p_round = o.p_round;
    if (o.done != kRunning) return r;
    r.uidx.assign(o.uidx[1], o.uidx[1] + o.uq[1]);
    r.qb.assign(o.qb[1], o.qb[1] + blocks);
    r.idx.assign((size_t)blocks * q_max, -1);
    for (int p = 0; p < blocks; ++p)
      for (int la = 0; la < o.qb[1][p]; ++la) r.idx[(size_t)p * q_max + la] = o.idx[1][p * q_max + la];
    return r;
  }
};

}  // namespace

WsMergeProbe ws_merge_multi_probe(const std::vector<uint64_t>& cand, int G, int blocks, int p_act, int q_max,
                                  int n_new, float eps, const std::vector<int32_t>& prev_union, int64_t iter,
                                  int64_t max_iter) {
  check_merge_multi(cand, G, blocks, q_max, prev_union);
  Arena st;
  MergeMultiRound m(st, cand, G, blocks, p_act, q_max, n_new, eps, prev_union, iter, max_iter);
  m.a.ctrl = st.up_one(*m.c);
  launch::ws_merge_multi(m.a, st.s);
  return MergeMultiRound::result(st.down(m.a.ctrl, 1)[0], blocks, q_max);
}

WsMergeMultiCacheProbe ws_merge_multi_cache_probe(const std::vector<uint64_t>& cand, int G, int blocks, int p_act,
                                                  int q_max, int n_new, float eps,
                                                  const std::vector<int32_t>& prev_union, int64_t iter,
                                                  int64_t max_iter, int64_t L, int hand,
                                                  const std::vector<int32_t>& slot_of,
                                                  const std::vector<int32_t>& key_of, const std::vector<float>& f,
                                                  const std::vector<float>& alpha, const std::vector<float>& y,
                                                  const float* lines, int64_t ldl) {
  check_merge_multi(cand, G, blocks, q_max, prev_union);
  const int64_t n = (int64_t)slot_of.size();
  check_cache_maps(n, L, hand, slot_of, key_of);
  DPSVM_CHECK(launch::ws_cache_multi_supported(L, blocks, q_max) && blocks * q_max <= kWsWindowMulti / 2,
              "ws_merge_multi_cache_probe: cache mode takes <= 4096 union rows and L >= 2 blocks q_max + 8192 lines");
  // the merge reads slot_of at every row it picks: any key of either side, any previous row
  for (uint64_t k : cand)
    DPSVM_CHECK(k == kKeyNone || (int64_t)key_index(k) < n, "ws_merge_multi_cache_probe: candidate row out of range");
  std::vector<char> seen((size_t)n, 0);
  for (int32_t r : prev_union) {
    DPSVM_CHECK(r >= 0 && r < n && !seen[r], "ws_merge_multi_cache_probe: previous-union rows: distinct, below n");
    seen[r] = 1;
  }
  DPSVM_CHECK(lines == nullptr || (ldl >= n && (int64_t)f.size() == n && (int64_t)alpha.size() == n &&
                                   (int64_t)y.size() == n),
              "ws_merge_multi_cache_probe: lines [L][ldl >= n] need f / alpha / y of n rows");
  Arena st;
  MergeMultiRound m(st, cand, G, blocks, p_act, q_max, n_new, eps, prev_union, iter, max_iter);
  blank_cache_ctrl(*m.c, hand);
  WsArgs& a = m.a;
  a.ctrl = st.up_one(*m.c);
  a.n = a.nl = n;
  a.cache = 1;
  a.L = (int32_t)L;
  a.slot_of = st.up(slot_of, (size_t)n);
  a.key_of = st.up(key_of, (size_t)L);
  launch::ws_merge_multi(a, st.s);
  const size_t nsub = (size_t)blocks * q_max * q_max, naux = (size_t)3 * blocks * kWsMax;
  if (lines != nullptr) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    float* sub = st.up(std::vector<float>(nsub + naux, nan), nsub + naux);
    a.subg = sub;
    a.aux = sub + nsub;
    a.aux_stride = blocks * kWsMax;
    a.gram = lines;
    a.ldg = ldl;
    a.f = st.up(f, (size_t)n);
    a.alpha = st.up(alpha, (size_t)n);
    a.y = st.up(y, (size_t)n);
    launch::ws_gather(a, st.s);  // blocks > 1: ws_gather_multi_kernel, lines from WsCtrl::line
  }
  const WsCtrl o = st.down(a.ctrl, 1)[0];
  WsMergeMultiCacheProbe r;
  r.merge = MergeMultiRound::result(o, blocks, q_max);
  r.cache = cache_state(st, o, a, n);
  if (lines != nullptr) {
    r.subg = st.down(a.subg, nsub);
    r.aux = st.down(a.aux, naux);
  }
  if (o.done != kRunning) return r;
  r.line.assign((size_t)blocks * q_max, -1);
  for (int p = 0; p < blocks; ++p)
    for (int la = 0; la < o.qb[1][p]; ++la) r.line[(size_t)p * q_max + la] = o.line[1][p * q_max + la];
  return r;
}

WsPackRowsProbe ws_pack_rows_probe(const std::vector<float>& x, int64_t nl, int dp, int64_t off,
                                   const std::vector<float>& xsq, const std::vector<int32_t>& miss_row, int n_miss,
                                   int q_max) {
  const int64_t n = (int64_t)xsq.size();
  DPSVM_CHECK(dp >= 16 && dp % 16 == 0 && nl >= 1 && off >= 0 && off + nl <= n && (int64_t)x.size() == nl * dp,
              "ws_pack_rows_probe: x [nl][dp], dp a multiple of 16, the shard [off, off + nl) inside xsq's n rows");
  DPSVM_CHECK(q_max >= 1 && q_max <= kWsMaxAll && n_miss >= 0 && n_miss <= q_max &&
                  (int64_t)miss_row.size() >= n_miss && (int64_t)miss_row.size() <= kWsMaxAll,
              "ws_pack_rows_probe: n_miss <= q_max <= 6144 rows, miss_row of at least n_miss entries");
  for (int i = 0; i < n_miss; ++i)
    DPSVM_CHECK(miss_row[i] >= 0 && miss_row[i] < n, "ws_pack_rows_probe: miss row out of range");
  Arena st;
  auto c = blank_ctrl();
  c->n_miss = n_miss;
  for (size_t i = 0; i < miss_row.size(); ++i) c->miss_row[i] = miss_row[i];
  const WsCtrl* dc = st.up_one(*c);
  const float* dx = st.up(x, x.size());
  const float* dsq = st.up(xsq, xsq.size());
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const size_t no = (size_t)q_max * dp;
  float* out = st.up(std::vector<float>(no + q_max, nan), no + q_max);
  launch::ws_pack_rows(dx, off, nl, dp, dsq, dc, q_max, out, out + no, st.s);
  WsPackRowsProbe r;
  r.out = st.down(out, no);
  r.out_sq = st.down(out + no, (size_t)q_max);
  return r;
}

namespace {

// the sub-problem's parameters in a launch's arguments
void set_solve_args(WsArgs& a, int blocks, int q_max, float C, int clip, float eps, float rel, float eps_floor,
                    float tau, int inner_max, int64_t max_iter, int wss) {
  a.blocks = blocks;
  a.q_max = q_max;
  a.inner_max = inner_max;
  a.rel_local = rel;
  a.eps_floor = eps_floor;
  a.C = C;
  a.eps = eps;
  a.tau = tau;
  a.clip = clip;
  a.max_iter = max_iter;
  a.wss = wss;
}

// what one ws_solve launch left in the control record (alpha: the caller's)
WsSolveProbe solve_result(const WsCtrl& o, int blocks, int q_max, int64_t iter0) {
  WsSolveProbe r;
  r.iter = o.iter;
  r.outer = o.outer;
  r.done = o.done;
  r.p_act = o.p_act;
  r.p1_round = o.p1_round;
  if (blocks == 1) {
    r.steps = {(int32_t)(o.iter - iter0)};
    r.nab = {o.n_apply};
    r.apply_idx.assign(o.apply_idx, o.apply_idx + o.n_apply);
    r.apply_coef.assign(o.apply_coef, o.apply_coef + o.n_apply);
  } else {
    for (int p = 0; p < blocks; ++p) {
      r.steps.push_back(o.inb[p]);
      r.nab.push_back(o.nab[p]);
      r.apply_idx.insert(r.apply_idx.end(), o.apply_idx + p * q_max, o.apply_idx + p * q_max + o.nab[p]);
      r.apply_coef.insert(r.apply_coef.end(), o.apply_coef + p * q_max, o.apply_coef + p * q_max + o.nab[p]);
    }
  }
  return r;
}

}  // namespace

WsSolveProbe ws_solve_probe(const std::vector<float>& K, const std::vector<float>& f, const std::vector<float>& alpha,
                            const std::vector<float>& y, const std::vector<int32_t>& qb, int q_max, int blocks,
                            int p_round, float C, int clip, float eps, float rel, float eps_floor, float tau,
                            float b_hi, float b_lo, int inner_max, int64_t iter0, int64_t max_iter, int wss,
                            const std::vector<float>& row_C, bool diag, int nu_cls) {
  DPSVM_CHECK(!diag || (blocks == 1 && clip == (int)ClipMode::Box),
              "ws_solve_probe: diag runs one block with box clipping");
  DPSVM_CHECK(nu_cls == 0 || ((nu_cls == 1 || nu_cls == -1) && blocks == 1 && clip == (int)ClipMode::Box &&
                              row_C.empty()),
              "ws_solve_probe: nu_cls is +1 / -1 and runs one block with box clipping and the scalar C");
  DPSVM_CHECK(blocks >= 1 && blocks <= kWsMaxBlocks && (int)qb.size() == blocks && q_max >= 2 && q_max <= kWsMax,
              "ws_solve_probe: 1 <= blocks <= 128, qb per block, q_max <= 192");
  DPSVM_CHECK((int64_t)blocks * q_max <= kWsMaxAll, "ws_solve_probe: blocks x q_max <= 6144 (the control record's rows)");
  const size_t nq = (size_t)blocks * q_max;
  DPSVM_CHECK(K.size() == nq * q_max && f.size() == nq && alpha.size() == nq && y.size() == nq,
              "ws_solve_probe: K [P][q_max][q_max], f / alpha / y [P][q_max]");
  for (int p = 0; p < blocks; ++p) DPSVM_CHECK(qb[p] >= 0 && qb[p] <= q_max, "ws_solve_probe: qb[p] <= q_max");
  DPSVM_CHECK(blocks > 1 || p_round == 1, "ws_solve_probe: one block means p_round 1");
  DPSVM_CHECK(row_C.empty() || row_C.size() == nq, "ws_solve_probe: row_C [P][q_max] or empty");
  Arena st;
  const int stride = blocks * kWsMax;
  std::vector<float> sub(nq * q_max + 3 * (size_t)stride, 0.f);
  std::copy(K.begin(), K.end(), sub.begin());
  float* aux = sub.data() + nq * q_max;
  for (int p = 0; p < blocks; ++p)
    for (int a = 0; a < qb[p]; ++a) {
      const size_t g = (size_t)p * q_max + a;
      aux[p * kWsMax + a] = f[g];
      aux[stride + p * kWsMax + a] = alpha[g];
      aux[2 * stride + p * kWsMax + a] = y[g];
    }
  auto c = blank_ctrl();
  c->iter = iter0;
  c->b_hi = b_hi;
  c->b_lo = b_lo;
  c->q[0] = qb[0];
  c->p_round = p_round;
  c->p_act = p_round;
  c->nu_cls = nu_cls;
  for (int p = 0; p < blocks; ++p) {
    c->qb[0][p] = qb[p];
    for (int a = 0; a < q_max; ++a) c->idx[0][p * q_max + a] = c->line[0][p * q_max + a] = p * q_max + a;
  }
  WsCtrl* dc = st.up_one(*c);
  float* dsub = st.up(sub, sub.size());
  WsArgs a = single_rank_args();
  a.subg = dsub;
  a.aux = dsub + nq * q_max;
  a.aux_stride = stride;
  a.alpha = st.up(alpha, nq);
  a.dalpha = st.alloc<float>(nq);
  set_solve_args(a, blocks, q_max, C, clip, eps, rel, eps_floor, tau, inner_max, max_iter, wss);
  if (!row_C.empty()) a.c_row = st.up(row_C, nq);  // row a of block p is global row p q_max + a
  a.diag = diag ? 1 : 0;
  a.nu_mode = nu_cls != 0 ? 1 : 0;
  a.ctrl = dc;
  launch::ws_solve(a, st.s);
  WsSolveProbe r = solve_result(st.down(dc, 1)[0], blocks, q_max, iter0);
  r.alpha = st.down(a.alpha, nq);
  return r;
}

WsSolveProbe ws_solve_direct_probe(const std::vector<float>& gram, int64_t n, int64_t ldg,
                                   const std::vector<float>& f, const std::vector<float>& alpha,
                                   const std::vector<float>& y, const std::vector<int32_t>& idx,
                                   const std::vector<int32_t>& qb, int q_max, int blocks, int p_round, float C,
                                   int clip, float eps, float rel, float eps_floor, float tau, float b_hi, float b_lo,
                                   int inner_max, int64_t iter0, int64_t max_iter, int wss,
                                   const std::vector<float>& row_C) {
  DPSVM_CHECK(blocks >= 1 && blocks <= kWsMaxBlocks && (int)qb.size() == blocks && q_max >= 2 && q_max <= 64,
              "ws_solve_direct_probe: 1 <= blocks <= 128, qb per block, 2 <= q_max <= 64");
  DPSVM_CHECK(n >= 1 && n < ((int64_t)1 << 31) && ldg >= n && (int64_t)gram.size() == n * ldg,
              "ws_solve_direct_probe: gram [n][ldg >= n]");
  DPSVM_CHECK((int64_t)f.size() == n && (int64_t)alpha.size() == n && (int64_t)y.size() == n,
              "ws_solve_direct_probe: f / alpha / y of n rows");
  DPSVM_CHECK(row_C.empty() || (int64_t)row_C.size() == n, "ws_solve_direct_probe: row_C of n rows or empty");
  DPSVM_CHECK((int64_t)blocks * q_max <= kWsMaxAll,
              "ws_solve_direct_probe: blocks x q_max <= 6144 (the control record's rows)");
  DPSVM_CHECK(idx.size() == (size_t)blocks * q_max, "ws_solve_direct_probe: idx [P][q_max]");
  DPSVM_CHECK(blocks > 1 || p_round == 1, "ws_solve_direct_probe: one block means p_round 1");
  std::vector<char> seen((size_t)n, 0);
  for (int p = 0; p < blocks; ++p) {
    DPSVM_CHECK(qb[p] >= 0 && qb[p] <= q_max, "ws_solve_direct_probe: qb[p] <= q_max");
    for (int k = 0; k < q_max; ++k) {
      const int64_t r = idx[(size_t)p * q_max + k];
      DPSVM_CHECK(r >= -1 && r < n && (k >= qb[p] || r >= 0), "ws_solve_direct_probe: row out of range");
      if (k < qb[p]) {  // two blocks committing one row's alpha would race
        DPSVM_CHECK(!seen[r], "ws_solve_direct_probe: a row listed twice in the blocks");
        seen[r] = 1;
      }
    }
  }
  Arena st;
  auto c = blank_ctrl();
  c->iter = iter0;
  c->b_hi = b_hi;
  c->b_lo = b_lo;
  c->q[0] = qb[0];
  c->p_round = c->p_act = p_round;
  for (int p = 0; p < blocks; ++p) c->qb[0][p] = qb[p];
  for (size_t i = 0; i < idx.size(); ++i) c->idx[0][i] = c->line[0][i] = idx[i];
  WsArgs a = single_rank_args(n);
  a.ctrl = st.up_one(*c);
  a.gram = st.up(gram, gram.size());
  a.ldg = ldg;
  a.f = st.up(f, (size_t)n);
  a.alpha = st.up(alpha, (size_t)n);
  a.y = st.up(y, (size_t)n);
  a.dalpha = st.alloc<float>((size_t)n);
  if (!row_C.empty()) a.c_row = st.up(row_C, (size_t)n);
  a.direct_sub = 1;  // subg / aux stay null: the branch must not read them
  a.aux_stride = blocks * kWsMax;
  set_solve_args(a, blocks, q_max, C, clip, eps, rel, eps_floor, tau, inner_max, max_iter, wss);
  launch::ws_solve(a, st.s);
  WsSolveProbe r = solve_result(st.down(a.ctrl, 1)[0], blocks, q_max, iter0);
  r.alpha = st.down(a.alpha, (size_t)n);
  return r;
}

WsSelectProbe ws_select_probe(const std::vector<float>& gram, int64_t L, int64_t ldg, const std::vector<float>& f,
                              const std::vector<float>& alpha, const std::vector<float>& y,
                              const std::vector<float>& dalpha, const std::vector<int32_t>& apply_line,
                              const std::vector<float>& apply_coef, const std::vector<int32_t>& nab, int blocks,
                              int p_round, int p_act, int q_max, float C, int64_t outer, int ks, int reps,
                              const std::vector<float>& row_C, int64_t fold, int done, int nu) {
  const int64_t n = (int64_t)f.size();
  DPSVM_CHECK(nu == 0 || (nu == 1 && blocks == 1 && row_C.empty()),
              "ws_select_probe: nu is 0 / 1 and runs one block with the scalar C");
  // fold > 0 (epsilon-SVR): n = 2 fold state rows on gram [L][ldg >= fold], geometry of the fold columns
  DPSVM_CHECK(fold == 0 || (n == 2 * fold && blocks == 1 && row_C.empty()),
              "ws_select_probe: fold needs 2 fold state rows, one block, scalar C");
  DPSVM_CHECK(done >= kRunning && done <= kCommFail, "ws_select_probe: done is a DoneCode");
  const int64_t ncol = fold > 0 ? fold : n;
  DPSVM_CHECK(n >= 1 && (int64_t)alpha.size() == n && (int64_t)y.size() == n && (int64_t)dalpha.size() == n,
              "ws_select_probe: f / alpha / y / dalpha of n rows");
  DPSVM_CHECK(ldg >= ncol && (int64_t)gram.size() == L * ldg, "ws_select_probe: gram [L][ldg >= n]");
  DPSVM_CHECK(blocks == 1 || (ldg % 4 == 0 && ldg >= (n + 3) / 4 * 4),
              "ws_select_probe: pass 1 loads 16 bytes a thread: ldg a multiple of 4 and >= round_up(n, 4)");
  DPSVM_CHECK(blocks >= 1 && blocks <= kWsMaxBlocks && (int)nab.size() == blocks && q_max >= 2 && q_max <= kWsMax,
              "ws_select_probe: nab per block, q_max <= 192");
  DPSVM_CHECK(apply_line.size() == apply_coef.size(), "ws_select_probe: apply lines / coefficients");
  DPSVM_CHECK(row_C.empty() || (int64_t)row_C.size() == n, "ws_select_probe: row_C of n rows or empty");
  int64_t tot = 0;
  for (int p = 0; p < blocks; ++p) {
    DPSVM_CHECK(nab[p] >= 0 && nab[p] <= q_max, "ws_select_probe: nab[p] <= q_max");
    tot += nab[p];
  }
  DPSVM_CHECK(tot == (int64_t)apply_line.size(), "ws_select_probe: sum(nab) apply rows");
  for (int32_t l : apply_line) DPSVM_CHECK(l >= 0 && l < L, "ws_select_probe: apply line out of range");
  int32_t G = 0, rpt = 0;
  launch::ws_geometry(ncol, 1, &G, &rpt);
  DPSVM_CHECK(rpt <= kWsMaxRPT, "ws_select_probe: too many rows");
  Arena st;
  auto c = blank_ctrl();
  c->outer = outer;
  c->done = done;
  c->n_apply = (int32_t)tot;
  c->p_round = p_round;
  c->p_act = p_act;
  int64_t at = 0;
  for (int p = 0; p < blocks; ++p) {
    c->nab[p] = nab[p];
    const int base = blocks == 1 ? 0 : p * q_max;
    for (int k = 0; k < nab[p]; ++k, ++at) {
      c->apply_line[base + k] = apply_line[at];
      c->apply_coef[base + k] = apply_coef[at];
      c->apply_idx[base + k] = apply_line[at];
    }
  }
  WsArgs a = single_rank_args(n);
  a.ctrl = st.up_one(*c);
  a.gram = st.up(gram, gram.size());
  a.ldg = ldg;
  a.f = st.up(f, (size_t)n);
  a.alpha = st.up(alpha, (size_t)n);
  a.y = st.up(y, (size_t)n);
  a.dalpha = st.up(dalpha, (size_t)n);
  a.ks = std::max(1, ks);
  a.p1G = blocks > 1 ? ws_pass1_v4_groups(n) : G;
  a.dfs = st.alloc<float>((size_t)n * a.ks);
  a.part = st.alloc<double>((size_t)2 * a.p1G * a.ks);
  a.cand = a.cand_out = st.alloc<uint64_t>((size_t)G * 2 * kWsCand);
  a.G = a.G_all = G;
  a.rpt = rpt;
  a.q_max = q_max;
  a.C = C;
  if (!row_C.empty()) a.c_row = st.up(row_C, (size_t)n);
  a.blocks = blocks;
  a.fold = fold;
  a.nu_mode = nu;
  WsSelectProbe r;
  // timing (bench/pass1_probe.py): pass 1 only reads the state, so it can repeat
  if (blocks > 1) r.pass1_us = to_f32(time_launches(st.s, reps, [&] { launch::ws_select_pass(a, 1, st.s); }));
  if (blocks == 1 && reps > 0) {
    // timing (bench/svr_probe.py): the one-pass kernel (plain or fold) repeated, rep i on the lines
    // apply_line[k] + (i mod (L / na)) na — a Gram of many times the list's lines keeps the rows out of the
    // caches from one launch to the next.  The launches update f: the state returned below includes them.
    const int64_t groups = std::max<int64_t>(1, tot > 0 ? L / tot : 1);
    int32_t* dline = (int32_t*)((char*)a.ctrl + offsetof(WsCtrl, apply_line));
    std::vector<int32_t> hl((size_t)tot);
    EventTimer timer(st.s);
    for (int i = 0; i <= reps; ++i) {  // the last pass restores the caller's lines
      const int64_t shift = i < reps ? (i % groups) * tot : 0;
      for (int64_t k = 0; k < tot; ++k) hl[k] = (int32_t)((apply_line[k] + shift) % L);
      if (tot > 0) HIP_CHECK(hipMemcpyAsync(dline, hl.data(), tot * 4, hipMemcpyHostToDevice, st.s));
      HIP_CHECK(hipStreamSynchronize(st.s));
      if (i < reps) r.select_us.push_back((float)timer.us([&] { launch::ws_select(a, st.s); }));
    }
  }
  launch::ws_select(a, st.s);  // blocks > 1: pass 1 then pass 2
  const WsCtrl o = st.down(a.ctrl, 1)[0];
  r.G = G;
  r.rpt = rpt;
  r.f = st.down(a.f, (size_t)n);
  r.alpha = st.down(a.alpha, (size_t)n);
  r.dalpha = st.down(a.dalpha, (size_t)n);
  r.dfs = st.down(a.dfs, (size_t)n);  // slice 0 (all of it at ks = 1)
  r.part = st.down(a.part, (size_t)2 * a.p1G * a.ks);
  r.p1G = a.p1G;
  r.cand = st.down(a.cand_out, (size_t)G * 2 * kWsCand);
  r.t = o.t_last;
  r.p_act = o.p_act;
  r.n_damped = o.n_damped;
  r.p1_round = o.p1_round;
  r.nonfinite = o.nonfinite;
  return r;
}

namespace {

// x [n][d] as the solver holds it: rows of pad_features(d) floats (zero
// padded), |x|^2 by row_sqnorm, the split GEMMs' operands by split_rows_f16
struct SplitX {
  int dp = 0;
  float* xsq = nullptr;
  void* xs = nullptr;
  int32_t* xsh = nullptr;
  SplitX(Arena& st, const std::vector<float>& x, int64_t n, int d) {
    dp = pad_features(d);
    const int64_t pr = launch::split_pad_rows(n);
    std::vector<float> xp((size_t)n * dp, 0.f);
    for (int64_t i = 0; i < n; ++i) std::copy(x.begin() + i * d, x.begin() + (i + 1) * d, xp.begin() + i * dp);
    const float* xd = st.up(xp, (size_t)pr * dp);
    xsq = st.alloc<float>((size_t)pr);
    launch::row_sqnorm(xd, n, dp, dp, xsq, st.s);
    const probe::SplitRows sr(st, xd, n, dp, dp);
    xs = sr.planes;
    xsh = sr.shift;
  }
};

void check_split_x(const std::vector<float>& x, int64_t n, int d) {
  DPSVM_CHECK(n >= 1 && n < ((int64_t)1 << 31) && d >= 1 && (int64_t)x.size() == n * d, "ws probe: x must be [n][d]");
  DPSVM_CHECK(pad_features(d) <= 64, "ws probe: the recompute kernels take dp <= 64");
}

// the crafted state of one one-block merge: every row the merge can pick must
// be a row of the problem (the kernels read f / alpha / y / Gram / X at it)
void check_merge_state(int64_t n, const std::vector<uint64_t>& cand, const std::vector<int32_t>& prev_set,
                       const std::vector<float>& f, const std::vector<float>& alpha, const std::vector<float>& y,
                       int q_max, int n_new, int nonfinite, int nu = 0) {
  DPSVM_CHECK(n >= 1 && n < ((int64_t)1 << 31) && (int64_t)f.size() == n && (int64_t)alpha.size() == n &&
                  (int64_t)y.size() == n,
              "ws merge probe: f / alpha / y of n rows");
  DPSVM_CHECK(q_max >= 2 && q_max <= kWsMax && n_new >= 1 && (nonfinite == 0 || nonfinite == 1),
              "ws merge probe: 2 <= q_max <= 192, n_new >= 1, nonfinite 0 / 1");
  const int64_t G = (int64_t)cand.size() / (2 * kWsCand);
  DPSVM_CHECK(G >= 1 && G <= (int64_t)kWsMaxGroups * kWsListsPerThread && (int64_t)cand.size() == G * 2 * kWsCand,
              "ws merge probe: cand must be [G][2][kWsCand = 16] with G <= 1024");
  DPSVM_CHECK((int64_t)prev_set.size() <= q_max, "ws merge probe: previous set longer than q_max");
  for (int32_t r : prev_set) DPSVM_CHECK(r >= 0 && r < n, "ws merge probe: previous-set row out of range");
  DPSVM_CHECK(nu == 0 || nu == 1, "ws merge probe: nu is 0 / 1");
  for (int64_t l = 0; l < 2 * G; ++l)
    for (int r = 0; r < (nu ? 2 : 1) * kWsCand1; ++r) {  // nu: class -'s keys behind class +'s
      const uint64_t k = cand[(size_t)l * kWsCand + r];
      DPSVM_CHECK(k == kKeyNone || (int64_t)key_index(k) < n, "ws merge probe: candidate row out of range");
    }
}

// control record and arguments of round `outer` of a one-block engine
struct MergeRound {
  WsCtrl* dc = nullptr;
  WsArgs a{};
  MergeRound(Arena& st, int64_t n, const std::vector<uint64_t>& cand, const std::vector<int32_t>& prev_set,
             const std::vector<float>& f, const std::vector<float>& alpha, const std::vector<float>& y, int q_max,
             int n_new, float eps, int64_t iter, int64_t max_iter, int nonfinite, int64_t outer,
             const std::function<void(WsCtrl&)>& more = nullptr) {  // further fields of the record before the upload
    auto c = blank_ctrl();
    const int par = (int)(outer & 1);
    c->outer = outer;
    c->iter = iter;
    c->nonfinite = nonfinite;
    c->n_apply = kWsProbeApply;
    c->q[par ^ 1] = (int32_t)prev_set.size();
    for (size_t i = 0; i < prev_set.size(); ++i) c->idx[par ^ 1][i] = prev_set[i];
    for (int i = 0; i < kWsMaxAll; ++i) c->idx[par][i] = -1;
    if (more) more(*c);
    dc = st.up_one(*c);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    float* sub = st.up(std::vector<float>((size_t)q_max * q_max + 3 * kWsMax, nan), (size_t)q_max * q_max + 3 * kWsMax);
    a = single_rank_args(n);
    a.ctrl = dc;
    a.cand = a.cand_out = st.up(cand, cand.size());
    a.G = a.G_all = (int32_t)(cand.size() / (2 * kWsCand));
    a.rpt = 1;
    a.f = st.up(f, (size_t)n);
    a.alpha = st.up(alpha, (size_t)n);
    a.y = st.up(y, (size_t)n);
    a.blocks = 1;
    a.q_max = q_max;
    a.n_new = n_new;
    a.eps = eps;
    a.max_iter = max_iter;
    a.subg = sub;
    a.aux = sub + (size_t)q_max * q_max;
    a.aux_stride = kWsMax;
  }
  WsGatherProbe result(Arena& st, int64_t outer) const {
    const WsCtrl o = st.down(dc, 1)[0];
    const int par = (int)(outer & 1);
    WsGatherProbe r;
    r.done = o.done;
    r.n_apply = o.n_apply;
    r.b_hi = o.b_hi;
    r.b_lo = o.b_lo;
    r.q = o.q[par];
    r.idx.assign(o.idx[par], o.idx[par] + std::max(0, std::min(r.q, (int)kWsMax)));
    r.line.assign(o.line[par], o.line[par] + std::max(0, std::min(r.q, (int)kWsMax)));
    r.subg = st.down(a.subg, (size_t)a.q_max * a.q_max);
    r.aux = st.down(a.aux, (size_t)3 * kWsMax);
    if (a.nu_mode) {
      r.nu_cls = o.nu_cls;
      r.nu_ext.assign(o.nu_ext, o.nu_ext + 4);
    }
    return r;
  }
};

}  // namespace

WsGatherProbe ws_gather_probe(const std::vector<float>& gram, int64_t n, int64_t ldg, const std::vector<uint64_t>& cand,
                              const std::vector<int32_t>& prev_set, const std::vector<float>& f,
                              const std::vector<float>& alpha, const std::vector<float>& y, int q_max, int n_new,
                              float eps, int64_t iter, int64_t max_iter, int nonfinite, int64_t outer, int64_t fold,
                              int nu) {
  check_merge_state(n, cand, prev_set, f, alpha, y, q_max, n_new, nonfinite, nu);
  // fold > 0 (epsilon-SVR): n = 2 fold state rows, gram [fold][ldg >= fold]
  DPSVM_CHECK(fold == 0 || n == 2 * fold, "ws_gather_probe: fold needs n = 2 fold state rows");
  const int64_t ng = fold > 0 ? fold : n;
  DPSVM_CHECK(ldg >= ng && (int64_t)gram.size() == ng * ldg && outer >= 0, "ws_gather_probe: gram [n][ldg >= n]");
  Arena st;
  MergeRound m(st, n, cand, prev_set, f, alpha, y, q_max, n_new, eps, iter, max_iter, nonfinite, outer);
  m.a.gram = st.up(gram, gram.size());
  m.a.ldg = ldg;
  m.a.fold = fold;
  m.a.nu_mode = nu;
  launch::ws_gather(m.a, st.s);  // dense, one block: ws_gather_kernel
  return m.result(st, outer);
}

WsGatherProbe ws_subgram_split_probe(const std::vector<float>& x, int64_t n, int d, const std::vector<uint64_t>& cand,
                                     const std::vector<int32_t>& prev_set, const std::vector<float>& f,
                                     const std::vector<float>& alpha, const std::vector<float>& y, float gamma,
                                     int q_max, int n_new, float eps, int64_t iter, int64_t max_iter, int nonfinite,
                                     int64_t outer) {
  check_split_x(x, n, d);
  check_merge_state(n, cand, prev_set, f, alpha, y, q_max, n_new, nonfinite);
  DPSVM_CHECK(outer >= 0, "ws_subgram_split_probe: outer >= 0");
  Arena st;
  SplitX sx(st, x, n, d);
  MergeRound m(st, n, cand, prev_set, f, alpha, y, q_max, n_new, eps, iter, max_iter, nonfinite, outer);
  DPSVM_CHECK(launch::ws_recompute_supported(m.a, sx.dp), "ws_subgram_split_probe: shape not supported");
  launch::ws_subgram_split(m.a, sx.xs, sx.xsh, sx.xsq, sx.dp, gamma, st.s);
  return m.result(st, outer);
}

WsMergeCacheProbe ws_merge_cache_probe(const std::vector<uint64_t>& cand, const std::vector<int32_t>& prev_set,
                                       const std::vector<float>& f, const std::vector<float>& alpha,
                                       const std::vector<float>& y, int q_max, int n_new, float eps, int64_t iter,
                                       int64_t max_iter, int nonfinite, int64_t outer, int done, int64_t L, int hand,
                                       const std::vector<int32_t>& slot_of, const std::vector<int32_t>& key_of,
                                       const float* lines, int64_t ldl) {
  const int64_t n = (int64_t)f.size();
  check_merge_state(n, cand, prev_set, f, alpha, y, q_max, n_new, nonfinite);
  check_cache_maps(n, L, hand, slot_of, key_of);
  DPSVM_CHECK(outer >= 0 && done >= kRunning && done <= kCommFail, "ws_merge_cache_probe: outer >= 0, done a DoneCode");
  DPSVM_CHECK(launch::ws_cache_supported(L, q_max), "ws_merge_cache_probe: L below ws_cache_min_lines(q_max)");
  DPSVM_CHECK(lines == nullptr || ldl >= n, "ws_merge_cache_probe: lines must be [L][ldl >= n]");
  Arena st;
  MergeRound m(st, n, cand, prev_set, f, alpha, y, q_max, n_new, eps, iter, max_iter, nonfinite, outer,
               [&](WsCtrl& c) {
                 c.done = done;
                 blank_cache_ctrl(c, hand);
               });
  WsArgs& a = m.a;
  a.cache = 1;
  a.L = (int32_t)L;
  a.slot_of = st.up(slot_of, (size_t)n);
  a.key_of = st.up(key_of, (size_t)L);
  launch::ws_merge(a, st.s);  // ws_merge_kernel: one workgroup
  if (lines != nullptr) {
    a.gram = lines;
    a.ldg = ldl;
    launch::ws_gather(a, st.s);  // cache, one block: ws_gather_lines_kernel
  }
  WsMergeCacheProbe r;
  r.round = m.result(st, outer);
  r.cache = cache_state(st, st.down(m.dc, 1)[0], a, n);
  return r;
}

WsFupdateProbe ws_fupdate_split_probe(const std::vector<float>& x, int64_t n, int d, const std::vector<float>& f,
                                      const std::vector<float>& alpha, const std::vector<float>& y,
                                      const std::vector<int32_t>& apply_idx, const std::vector<float>& apply_coef,
                                      float gamma, float C, int done) {
  check_split_x(x, n, d);
  DPSVM_CHECK((int64_t)f.size() == n && (int64_t)alpha.size() == n && (int64_t)y.size() == n,
              "ws_fupdate_split_probe: f / alpha / y of n rows");
  DPSVM_CHECK(apply_idx.size() == apply_coef.size() && apply_idx.size() <= (size_t)kWsMax,
              "ws_fupdate_split_probe: <= 192 apply rows, a coefficient each");
  for (int32_t r : apply_idx) DPSVM_CHECK(r >= 0 && r < n, "ws_fupdate_split_probe: apply row out of range");
  DPSVM_CHECK(done >= kRunning && done <= kCommFail, "ws_fupdate_split_probe: done is a DoneCode");
  int32_t G = 0, rpt = 0;
  launch::ws_geometry(n, 1, &G, &rpt);
  DPSVM_CHECK(rpt <= kWsMaxRPT, "ws_fupdate_split_probe: too many rows");
  Arena st;
  SplitX sx(st, x, n, d);
  auto c = blank_ctrl();
  c->outer = 1;
  c->done = done;
  c->n_apply = (int32_t)apply_idx.size();
  // past the list: what an earlier, longer round left there (the kernel pads the
  // list to a multiple of 32 rows and must give the padding a zero coefficient)
  for (int k = 0; k < kWsMax; ++k) c->apply_coef[k] = 3.f;
  for (size_t k = 0; k < apply_idx.size(); ++k) {
    c->apply_idx[k] = c->apply_line[k] = apply_idx[k];
    c->apply_coef[k] = apply_coef[k];
  }
  WsArgs a = single_rank_args(n);
  a.ctrl = st.up_one(*c);
  a.f = st.up(f, (size_t)n);
  a.alpha = st.up(alpha, (size_t)n);
  a.y = st.up(y, (size_t)n);
  const size_t nc = (size_t)G * 2 * kWsCand;
  a.cand = a.cand_out = st.up(std::vector<uint64_t>(nc, kWsProbeKey), nc);
  a.G = a.G_all = G;
  a.rpt = rpt;
  a.blocks = 1;
  a.q_max = kWsMax;
  a.C = C;
  DPSVM_CHECK(launch::ws_recompute_supported(a, sx.dp), "ws_fupdate_split_probe: shape not supported");
  launch::ws_fupdate_split(a, sx.xs, sx.xsh, sx.xsq, sx.dp, gamma, st.s);
  const WsCtrl o = st.down(a.ctrl, 1)[0];
  WsFupdateProbe r;
  r.f = st.down(a.f, (size_t)n);
  r.cand = st.down(a.cand_out, nc);
  r.nonfinite = o.nonfinite;
  r.rows_computed = o.rows_computed;
  r.G = G;
  r.rpt = rpt;
  return r;
}

namespace {

// every argument of a sharded stage that an address is computed from, before any HIP call
void check_shard_in(WsShardStage stage, const WsShardIn& in, int32_t G, int32_t rpt) {
  const int64_t n = in.n;
  const int W = in.world, P = in.blocks;
  const bool sel = stage == WsShardStage::Select, p1 = stage == WsShardStage::Pass1, p2 = stage == WsShardStage::Pass2;
  const bool g1 = stage == WsShardStage::Gather, gm = stage == WsShardStage::GatherMulti;
  const bool gl = stage == WsShardStage::GatherLines;
  DPSVM_CHECK(sel || p1 || p2 || g1 || gm || gl, "ws_shard_round_probe: stage is a WsShardStage");
  // 32 ranks: pass 1 pushes its partials from lanes 2 p, 2 p + 1 < 64
  DPSVM_CHECK(W >= 1 && W <= 32 && n >= W && n < ((int64_t)1 << 31),
              "ws_shard_round_probe: 1 <= world <= 32 ranks of at least one row each");
  DPSVM_CHECK(in.exchange == 0 || in.exchange == 1, "ws_shard_round_probe: exchange is 0 (collectives) or 1 (peer)");
  DPSVM_CHECK(in.exchange == 0 || (in.xtimeout_ticks >= 1 && in.xtimeout_ticks <= kWsProbeXTimeout),
              "ws_shard_round_probe: xtimeout_ticks in [1, 10^7] (0.1 s): a probe never waits longer");
  DPSVM_CHECK(rpt <= kWsMaxRPT && (int64_t)G * W <= (int64_t)kWsMaxGroups * kWsListsPerThread,
              "ws_shard_round_probe: too many rows");
  DPSVM_CHECK(in.L >= 1 && in.L < ((int64_t)1 << 31) && (int64_t)in.gram.size() == in.L * n,
              "ws_shard_round_probe: gram [L][n]");
  DPSVM_CHECK(in.ldg_extra >= 0 && in.ldg_extra % 4 == 0, "ws_shard_round_probe: ldg_extra a multiple of 4");
  DPSVM_CHECK((int64_t)in.f.size() == n && (int64_t)in.alpha.size() == n && (int64_t)in.y.size() == n &&
                  (int64_t)in.dalpha.size() == n,
              "ws_shard_round_probe: f / alpha / y / dalpha of n rows");
  DPSVM_CHECK(in.row_C.empty() || (int64_t)in.row_C.size() == n, "ws_shard_round_probe: row_C of n rows or empty");
  DPSVM_CHECK((sel || g1 || gl) ? P == 1 : (P >= 2 && P <= kWsMaxBlocks),
              "ws_shard_round_probe: Select / Gather / GatherLines run one block, Pass1 / Pass2 / GatherMulti 2 .. 128");
  DPSVM_CHECK(in.q_max >= 2 && in.q_max <= kWsMax && (int64_t)P * in.q_max <= kWsMaxAll,
              "ws_shard_round_probe: 2 <= q_max <= 192, blocks x q_max <= 6144");
  DPSVM_CHECK(in.cache == 0 || in.cache == 1, "ws_shard_round_probe: cache is 0 / 1");
  DPSVM_CHECK(gl ? in.cache == 1 : (gm || in.cache == 0),
              "ws_shard_round_probe: GatherLines is the cache form, only GatherMulti has both");
  DPSVM_CHECK(!(g1 || gm || gl) || in.cache == 1 || in.L == n, "ws_shard_round_probe: a dense gather reads gram [n][n]");
  DPSVM_CHECK(in.outer >= 0 && in.ks >= 1 && in.ks <= kWsMaxPass1Splits && in.ncand >= 0,
              "ws_shard_round_probe: outer >= 0, 1 <= ks <= 16, ncand >= 0");
  DPSVM_CHECK(in.p_round >= 1 && in.p_round <= P && in.p_act >= 1 && in.p_act <= P,
              "ws_shard_round_probe: p_round / p_act in [1, blocks]");
  if (sel || p1 || p2) {
    DPSVM_CHECK((int)in.nab.size() == P, "ws_shard_round_probe: nab per block");
    int64_t tot = 0;
    for (int p = 0; p < P; ++p) {
      DPSVM_CHECK(in.nab[p] >= 0 && in.nab[p] <= in.q_max, "ws_shard_round_probe: nab[p] <= q_max");
      tot += in.nab[p];
    }
    DPSVM_CHECK(tot == (int64_t)in.apply_idx.size() && tot == (int64_t)in.apply_line.size() &&
                    tot == (int64_t)in.apply_coef.size(),
                "ws_shard_round_probe: sum(nab) apply rows, lines and coefficients");
    for (int32_t l : in.apply_line) DPSVM_CHECK(l >= 0 && l < in.L, "ws_shard_round_probe: apply line out of range");
    for (int32_t i : in.apply_idx) DPSVM_CHECK(i >= 0 && i < n, "ws_shard_round_probe: apply row out of range");
  }
  if (p2) {
    const int64_t nl_max = (n + W - 1) / W;
    DPSVM_CHECK((int64_t)in.part.size() == (int64_t)2 * W * ws_pass1_v4_groups(nl_max) * in.ks,
                "ws_shard_round_probe: part [world p1G][ks][2]");
    DPSVM_CHECK((int64_t)in.dfs.size() == in.ks * n, "ws_shard_round_probe: dfs [ks][n]");
  }
  if (g1) {
    DPSVM_CHECK((int64_t)in.cand.size() == (int64_t)W * G * 2 * kWsCand,
                "ws_shard_round_probe: cand [world G][2][kWsCand = 16]");
    check_merge_state(n, in.cand, in.prev_set, in.f, in.alpha, in.y, in.q_max, in.n_new, 0);
  }
  if (gm || gl) {
    DPSVM_CHECK((int)in.qb.size() == P && in.idx.size() == (size_t)P * in.q_max && in.line.size() == in.idx.size(),
                "ws_shard_round_probe: qb per block, idx / line [blocks][q_max]");
    std::vector<char> seen((size_t)n, 0);
    for (int p = 0; p < P; ++p) {
      DPSVM_CHECK(in.qb[p] >= 0 && in.qb[p] <= in.q_max, "ws_shard_round_probe: qb[p] <= q_max");
      for (int k = 0; k < in.qb[p]; ++k) {
        const int64_t r = in.idx[(size_t)p * in.q_max + k], l = in.line[(size_t)p * in.q_max + k];
        DPSVM_CHECK(r >= 0 && r < n && l >= 0 && l < in.L, "ws_shard_round_probe: set row or line out of range");
        DPSVM_CHECK(!seen[r], "ws_shard_round_probe: a row listed twice in the set");
        seen[r] = 1;
      }
    }
  }
  if (in.exchange && (g1 || gm || gl))
    DPSVM_CHECK(in.inner_max >= 0 && (in.clip == 0 || in.clip == 1) && (in.wss == 1 || in.wss == 2),
                "ws_shard_round_probe: the peer form's solve: inner_max >= 0, clip 0 / 1, wss 1 / 2");
}

}  // namespace

WsShardProbe ws_shard_round_probe(WsShardStage stage, const WsShardIn& in) {
  const int64_t n = in.n;
  const int W = in.world, P = in.blocks, q_max = in.q_max;
  int32_t G = 0, rpt = 0;
  const int64_t nl_max = W >= 1 ? (n + W - 1) / W : n;
  launch::ws_geometry(nl_max, std::max(1, W), &G, &rpt);  // host arithmetic: as setup calls it
  check_shard_in(stage, in, G, rpt);
  const bool sel = stage == WsShardStage::Select, p1 = stage == WsShardStage::Pass1, p2 = stage == WsShardStage::Pass2;
  const bool g1 = stage == WsShardStage::Gather, gm = stage == WsShardStage::GatherMulti;
  const bool gather = !(sel || p1 || p2);
  const int par = (int)(in.outer & 1), ks = in.ks;
  const int p1G = P > 1 ? ws_pass1_v4_groups(nl_max) : G;
  const size_t ncand = (size_t)W * G * 2 * kWsCand, npart = (size_t)2 * W * p1G * ks;
  const size_t nsub = (size_t)P * q_max * q_max, naux = (size_t)3 * P * kWsMax;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  Arena st;
  WsShardProbe out;
  out.G = G;
  out.rpt = rpt;
  out.p1G = p1G;
  // the arguments every rank shares; the exchange region's layout from them
  WsArgs base = single_rank_args(n);
  base.world = W;
  base.G = G;
  base.rpt = rpt;
  base.G_all = G * W;
  base.ks = ks;
  base.p1G = p1G;
  base.ncand = in.ncand;
  base.n_new = in.n_new;
  base.cache = in.cache;
  base.L = (int32_t)in.L;
  base.aux_stride = P * kWsMax;
  set_solve_args(base, P, q_max, in.C, in.clip, in.eps, in.rel, in.eps_floor, in.tau, in.inner_max, in.max_iter,
                 in.wss);
  if (in.exchange) {
    out.xch_words = ws_xch_set_layout(base, q_max);
    std::vector<uint64_t*> bufs((size_t)W);
    bool uc = false;
    for (int r = 0; r < W; ++r) bufs[r] = st.alloc_receive<uint64_t>((size_t)out.xch_words, &uc);
    out.uncached = uc ? 1 : 0;
    base.xpeer = st.up(bufs, (size_t)W);
    base.xtimeout_ticks = in.xtimeout_ticks;
  }
  std::vector<WsArgs> args;
  int64_t tot = 0;
  for (int32_t v : in.nab) tot += v;
  for (int r = 0; r < W; ++r) {
    const Shard sh = shard_of(n, r, W);
    WsArgs a = base;
    a.nl = sh.size;
    a.off = sh.offset;
    a.rank = a.xrank = r;
    // the panel: columns [off, off + nl) of every line, NaN behind them
    a.ldg = (sh.size + 3) / 4 * 4 + in.ldg_extra;
    std::vector<float> panel((size_t)in.L * a.ldg, nan);
    for (int64_t l = 0; l < in.L; ++l)
      std::copy(in.gram.begin() + l * n + sh.offset, in.gram.begin() + l * n + sh.offset + sh.size,
                panel.begin() + l * a.ldg);
    a.gram = st.up(panel, panel.size());
    a.f = st.up(in.f.data() + sh.offset, (size_t)sh.size, (size_t)sh.size);
    a.alpha = st.up(in.alpha, (size_t)n);
    a.y = st.up(in.y, (size_t)n);
    a.dalpha = st.up(in.dalpha, (size_t)n);
    if (!in.row_C.empty()) a.c_row = st.up(in.row_C, (size_t)n);
    uint64_t* cand = g1 ? st.up(in.cand, ncand) : st.up(std::vector<uint64_t>(ncand, kWsProbeKey), ncand);
    a.cand = cand;
    a.cand_out = cand + (size_t)r * G * 2 * kWsCand;
    if (p2) {
      std::vector<float> d((size_t)ks * sh.size);
      for (int k = 0; k < ks; ++k)
        std::copy(in.dfs.begin() + k * n + sh.offset, in.dfs.begin() + k * n + sh.offset + sh.size,
                  d.begin() + k * sh.size);
      a.dfs = st.up(d, d.size());
      a.part = st.up(in.part, npart);
    } else {
      a.dfs = st.alloc<float>((size_t)ks * sh.size);
      a.part = st.up(std::vector<double>(npart, kWsProbePart), npart);
    }
    if (gather) {
      float* sub = st.up(std::vector<float>(nsub + naux, nan), nsub + naux);
      a.subg = sub;
      a.aux = sub + nsub;
    }
    auto c = blank_ctrl();
    c->outer = in.outer;
    c->iter = in.iter;
    c->p_round = in.p_round;
    c->p_act = in.p_act;
    c->b_hi = in.b_hi;
    c->b_lo = in.b_lo;
    if (!gather) {
      c->n_apply = (int32_t)tot;
      int64_t at = 0;
      for (int p = 0; p < P; ++p) {
        c->nab[p] = in.nab[p];
        const int b0 = P == 1 ? 0 : p * q_max;
        for (int k = 0; k < in.nab[p]; ++k, ++at) {
          c->apply_idx[b0 + k] = in.apply_idx[at];
          c->apply_line[b0 + k] = in.apply_line[at];
          c->apply_coef[b0 + k] = in.apply_coef[at];
        }
      }
    } else if (g1) {  // as ws_gather_probe: the merge builds parity par from the previous set in the other
      c->n_apply = kWsProbeApply;
      c->q[par ^ 1] = (int32_t)in.prev_set.size();
      for (size_t i = 0; i < in.prev_set.size(); ++i) c->idx[par ^ 1][i] = in.prev_set[i];
      for (int i = 0; i < kWsMaxAll; ++i) c->idx[par][i] = -1;
    } else {
      int32_t q = 0;
      for (int p = 0; p < P; ++p) {
        c->qb[par][p] = in.qb[p];
        q += in.qb[p];
      }
      c->q[par] = c->uq[par] = q;
      for (size_t i = 0; i < in.idx.size(); ++i) {
        c->idx[par][i] = in.idx[i];
        c->line[par][i] = in.line[i];
      }
    }
    a.ctrl = st.up_one(*c);
    args.push_back(a);
  }
  // every rank's producer, then (peer form) every rank's consumer: a slot is full before anything polls it
  for (const WsArgs& a : args) {
    if (sel) launch::ws_select(a, st.s);
    else if (p1 || p2) launch::ws_select_pass(a, p1 ? 1 : 2, st.s);
    else launch::ws_gather(a, st.s);
  }
  if (in.exchange)
    for (const WsArgs& a : args) {
      if (sel || p2) launch::ws_xcollect_cand(a, st.s);
      else if (p1) launch::ws_xcollect_part(a, st.s);
      else launch::ws_solve(a, st.s);
    }
  for (const WsArgs& a : args) {
    const WsCtrl o = st.down(a.ctrl, 1)[0];
    WsShardRank r;
    r.off = a.off;
    r.nl = a.nl;
    r.ldg = a.ldg;
    r.f = st.down(a.f, (size_t)a.nl);
    r.alpha = st.down(a.alpha, (size_t)n);
    r.dalpha = st.down(a.dalpha, (size_t)n);
    r.dfs = st.down(a.dfs, (size_t)ks * a.nl);
    r.part = st.down(a.part, npart);
    r.cand_out = st.down(a.cand_out, (size_t)G * 2 * kWsCand);
    r.cand = st.down(a.cand, ncand);
    r.t = o.t_last;
    r.b_hi = o.b_hi;
    r.b_lo = o.b_lo;
    r.p_act = o.p_act;
    r.n_damped = o.n_damped;
    r.nonfinite = o.nonfinite;
    r.done = o.done;
    r.n_apply = o.n_apply;
    r.p1_round = o.p1_round;
    r.iter = o.iter;
    r.outer = o.outer;
    if (gather) {
      r.q = o.q[par];
      if (g1) {
        const int q = std::max(0, std::min(r.q, (int)kWsMax));
        r.idx.assign(o.idx[par], o.idx[par] + q);
        r.line.assign(o.line[par], o.line[par] + q);
      }
      r.subg = st.down(a.subg, nsub);
      r.aux = st.down(a.aux, naux);
      if (in.exchange) {
        const WsSolveProbe s = solve_result(o, P, q_max, in.iter);
        r.steps = s.steps;
        r.apply_idx = s.apply_idx;
        r.apply_coef = s.apply_coef;
        r.nab = s.nab;
      }
    }
    out.ranks.push_back(std::move(r));
  }
  return out;
}

}  // namespace kernels
}  // namespace dpsvm
