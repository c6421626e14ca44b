// The shape of a working-set round, decided in one place: how many blocks of
// how many rows a round takes, what carries it between ranks, and the sizes
// that follow (candidate keys per list, pass-1 geometry, exchange region).
//
// Host-only and pure: no HIP call, no communicator, no environment, no static
// state — the same facts give the same plan on every rank, and on a CPU
// (cli/unit_tests.cpp ws_plan, tests/test_ws_plan.py).  gpu_setup.hip gathers
// the facts (agreeing what can differ per device), calls ws_round_plan, runs
// the two steps only a device can (the ranks' agreement on `multi_elig`, the
// peer exchange's self test) and hands their outcome to ws_round_shape.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>

#include "dpsvm/device_state.hpp"

namespace dpsvm {

// SolverParams::ws_size as the engines take it
inline int ws_clamp_q(int ws_size) { return std::max(2, std::min(ws_size, kWsMax)); }

// the wide pass 1 (ws_select.hip): column groups per rank, and list slices per
// group — about one workgroup per CU (the headline at one rank: 59 groups x 4
// slices; a rank of 8: 8 groups x 32 slices)
inline int ws_pass1_v4_groups(int64_t nl_max) {
  return (int)std::max<int64_t>(1, (nl_max + kWsPass1Cols - 1) / kWsPass1Cols);
}
inline int ws_pass1_v4_splits(int p1G) { return std::max(1, std::min(2 * kWsMaxPass1Splits, 256 / std::max(1, p1G))); }

// What setup knows before it plans the rounds (agreed across ranks, except L:
// the line count follows each device's free memory).
struct WsPlanFacts {
  int64_t n = 0;   // rows of the whole problem
  int world = 1;   // ranks sharding them
  int ws_size = kWsMax, ws_blocks = 0, ws_new = 0, ws_inner = 0;  // SolverParams
  int dp = 0;      // padded features
  bool uncoupled = false;  // mean off-diagonal K of the row sample < 1e-4: a round's blocks do not interact
  bool ws_dense = false;   // candidate: working-set rounds on the resident Gram
  bool ws_cache = false;   // candidate: ... on a kernel-row cache of L lines
  int64_t L = 0;
  int share = 1;   // most ranks on one device (rehearsals; 1 on distinct devices)
  int cus = 0;     // fewest compute units of any rank's device (world > 1)
  int exchange = 0;               // SolverParams::exchange: 0 auto, 1 allreduce, 2 peer
  bool force_collectives = false;
  bool device_comm = false;       // the communicator moves device memory
  int ws_G = 0;                   // selection workgroups per rank (launch::ws_geometry)
  bool replicated = true;         // X replicated (false: partitioned)
};

struct WsRoundPlan {
  int ws_q = 0;         // rows of a one-block round
  int want_blocks = 1;  // blocks and rows per block of the multi-block rounds, if they run
  int mb_q = 0;
  std::string error;    // not empty: the parameters are refused (setup throws it)
  bool cache_fits = false;  // ws-cache: L holds the one-block round's rows and the victim window
  bool multi_elig = false;  // this rank could run multi-block rounds (setup agrees it over the ranks)
  // ranks sharing a device: the wave slots their spinning consumers and one
  // rank's producers take, and whether the device has them
  int64_t xch_waves = 0;
  bool xch_resident = true;
  int p1G = 1, ks = 1;  // pass 1 of the multi-block rounds: column groups per rank, list slices
  // the peer exchange may carry the multi-block / the one-block rounds (then
  // setup requests a region of this many words and runs the self test)
  bool peer_multi = false, peer_one = false;
  int64_t xch_words_multi = 0, xch_words_one = 0;
  bool collectives_multi = false;  // the communicator's collectives may carry multi-block rounds
  std::string note;                // engine_note, when the peer exchange is refused for residency

  // multi-block rounds run: every rank eligible, and a carrier
  bool multi_ok(bool elig_all, bool multi_peer) const { return elig_all && (multi_peer || collectives_multi); }
};

// what the round kernels are given (WsArgs), once the carrier is known
struct WsRoundShape {
  int blocks = 1, q_max = 0, n_new = 0, inner_max = 0;
  int ncand = kWsCandStd, direct_sub = 0;
  std::string note;  // appended to engine_note: ws_blocks > 1 asked for, one block run
};

inline WsRoundPlan ws_round_plan(const WsPlanFacts& f) {
  WsRoundPlan p;
  const int ws_q = p.ws_q = ws_clamp_q(f.ws_size);
  const int64_t nl_max = (f.n + f.world - 1) / f.world;
  p.cache_fits = f.ws_cache && f.L >= ws_cache_min_lines(ws_q);
  // ws_blocks auto (0): multi-block rounds from kWsAutoBlocksRows rows on (the
  // round's fixed cost is amortised over P sub-problems; small problems need
  // few rounds).  The round's union: the rounds touch ~3.4 n rows in all
  // whatever the union (headline: 254 / 128 / 67 rounds at 768 / 1,536 / 3,072
  // rows), so a wider union divides the rounds' fixed cost (~50 us: selection,
  // rank, merge, launch gaps) — uncoupled ws-dense rounds take kWsMaxAll rows
  // (profiles/r5_union6144_ab.txt), everything else kWsAutoUnion (the cache
  // merge's line tables hold that many).  Where the kernel is numerically
  // diagonal at working-set scale (MNIST-shape at gamma 0.25: coupling 1.7e-9)
  // the blocks of a round do not interact, so blocks of 48 rows (one row per
  // solve lane: cheaper pair steps) beat 32 of 96; coupled data keeps 32
  // blocks (mnist-parity 0.0206 s with 32, 0.0422 s with 64: damped rounds;
  // profiles/r5_blocks_64_vs_32_ab.txt, r3_union3072_ab.txt).  Never more rows
  // per block than ws_size; the one-block rounds the adaptive count falls
  // back to keep ws_size rows.
  const int auto_union = f.uncoupled && f.ws_dense ? kWsMaxAll : kWsAutoUnion;
  const int auto_blocks = f.uncoupled ? auto_union / 48 : kWsAutoBlocks;
  const int auto_q = std::min(ws_q, auto_union / auto_blocks) & ~1;
  const bool blocks_auto = f.ws_blocks == 0;
  p.want_blocks = !blocks_auto ? f.ws_blocks
                               : (f.n >= kWsAutoBlocksRows ? std::min(auto_blocks, auto_union / auto_q) : 1);
  p.mb_q = blocks_auto ? auto_q : ws_q;
  // Residency of the ws peer exchange with ranks sharing a device.  No producer
  // ever waits: selection, gather and pass-1 workgroups push into every rank's
  // receive buffer and return.  The spinning consumers of one rank are the
  // collect kernels (<= 16 workgroups of 4 waves) and the solve (one workgroup
  // of 16 waves per block), so the share ranks' consumers plus one rank's
  // full-size producer kernel (1024 waves) must fit the device's wave slots (32
  // a CU) for every rank's producers to keep running — one-block and
  // multi-block rounds alike.
  auto waves = [&](int blocks) { return (int64_t)f.share * (64 + 16 * std::max(1, blocks)) + 1024; };
  const int64_t slots = (int64_t)f.cus * 32;
  // an auto union that would not fit: halve the block count until it does (4
  // ranks on one GPU: 64 blocks, 8 ranks: 32, over the peer exchange, rather
  // than one block per round over host collectives).  Distinct devices (share
  // 1) always fit 128 blocks.  Collectives (exchange=allreduce,
  // force_collectives) spin on nothing: the wide union stays.
  if (f.world > 1 && blocks_auto && p.want_blocks > 1 && f.exchange != 1 && !f.force_collectives)
    while (p.want_blocks > 8 && waves(p.want_blocks) > slots) p.want_blocks /= 2;
  // (only where working-set rounds can run: solver=smo or a small problem ignores ws_blocks)
  if ((f.ws_dense || f.ws_cache) && p.want_blocks > 1 && p.want_blocks * p.mb_q > kWsMaxAll) {
    p.error = "ws_blocks x ws_size must be <= " + std::to_string(kWsMaxAll) + " (the round's union capacity)";
    return p;
  }
  // multi-block rounds: the union merge reads <= kWsMaxGroups candidate lists
  // and deals rows to the blocks in pairs (an even q); ws-cache takes them when
  // its cache holds the union's lines twice over plus the victim window, for
  // unions of <= kWsAutoUnion rows
  const bool cache_multi = p.cache_fits && f.L >= ws_cache_multi_min_lines(p.want_blocks, p.mb_q);
  p.multi_elig = p.want_blocks > 1 && (f.ws_dense || cache_multi) && p.mb_q % 2 == 0 &&
                 (int64_t)f.ws_G * f.world <= kWsMaxGroups && (p.want_blocks * p.mb_q <= kWsAutoUnion || f.ws_dense);
  const bool rounds = f.ws_dense || p.cache_fits;
  if (f.world > 1) {
    p.xch_waves = waves(p.want_blocks);
    p.xch_resident = p.xch_waves <= slots;
    if (!p.xch_resident && f.exchange != 2 && rounds)
      p.note = "ws peer exchange refused: " + std::to_string(f.share) + " ranks share a device (" +
               std::to_string(p.xch_waves) + " spinning + producer waves > " + std::to_string(f.cus * 32) +
               " wave slots): collectives";
  }
  // what carries the rounds at world > 1: the in-kernel peer exchange
  // (candidate lists, the sub-Grams' owned entries and the line-search partials
  // pushed into every rank's receive buffer: no collective per round) or, when
  // that is unavailable, the communicator's collectives (three per round; a
  // device communicator, or exchange=allreduce).  exchange=peer at world 1:
  // loopback (tests).  Partitioned X in cache mode sums the miss rows by an
  // all-reduce: its multi-block rounds keep the collectives.
  p.peer_one = rounds && f.exchange != 1 && !f.force_collectives && (f.world > 1 || f.exchange == 2) &&
               (p.xch_resident || f.exchange == 2);
  p.peer_multi = p.peer_one && !(f.ws_cache && !f.replicated);
  p.collectives_multi = (f.world == 1 || f.device_comm || f.exchange == 1) && f.exchange != 2;
  // multi-block pass 1: the wide layout (1024-column groups, 16-B row loads:
  // headline round 227.5 -> 212.9 us, profiles/r5_pass1_wide_ab.txt)
  p.p1G = ws_pass1_v4_groups(nl_max);
  p.ks = ws_pass1_v4_splits(p.p1G);
  const int64_t G_all = (int64_t)f.ws_G * f.world;
  p.xch_words_multi = ws_xch_words_multi(G_all, (int64_t)p.p1G * f.world, p.ks, p.want_blocks, p.mb_q, ws_q);
  p.xch_words_one = ws_xch_words(G_all, ws_q);
  return p;
}

// multi_ok: WsRoundPlan::multi_ok of the agreed eligibility and the self
// test's outcome; xch: a peer exchange (or its loopback) carries the rounds
inline WsRoundShape ws_round_shape(const WsPlanFacts& f, const WsRoundPlan& p, bool multi_ok, bool xch) {
  WsRoundShape s;
  s.q_max = p.ws_q;
  // >= 2 new rows: the global maximal violating pair (up rank 0, low rank 0)
  // is always in the set, so every round makes progress
  // defaults measured on the MNIST-shape headline (profiles/r2_ws_param_sweep.txt)
  s.n_new = ws_new_auto(f.ws_new, p.ws_q, f.dp);
  if (p.want_blocks > 1) {
    if (multi_ok) {
      s.blocks = p.want_blocks;
      s.q_max = p.mb_q;
    } else if (f.ws_blocks > 1) {
      s.note = "ws_blocks > 1 needs an even ws_size, <= 256 candidate lists, the peer exchange or a "
               "device communicator, and (ws-cache) >= 2 P ws_size + 4096 lines: one block per round";
    }
  }
  s.inner_max = f.ws_inner > 0 ? f.ws_inner : 4 * s.q_max;
  // multi-block rounds replace the whole union each round by default (measured on the
  // headline at P = 8: 3/4 q new 0.0506 s, all new 0.0493 s; profiles/r2_ws_blocks_sweep.txt)
  if (s.blocks > 1 && f.ws_new <= 0) s.n_new = s.q_max;
  // keys per selection list: the union's half per side over the lists with
  // room to spare (8 cover 3,072-row unions: 1,880 a side on the headline's 235)
  s.ncand = s.blocks * s.q_max > kWsAutoUnion ? kWsCand : kWsCandStd;
  // blocks of <= 64 rows at world 1 on the resident Gram: the solve loads its
  // q x q block itself (96-row blocks measured slower that way: 9,216 loads a
  // workgroup, profiles/r4_direct_subgram_ab.txt)
  s.direct_sub = s.blocks > 1 && s.q_max <= 64 && f.world == 1 && f.ws_dense && !xch ? 1 : 0;
  return s;
}

// The whole decision for given outcomes of the two device steps (the tests'
// and the Python binding's view; setup runs the same calls around the real steps).
inline WsRoundShape ws_round_resolve(const WsPlanFacts& f, const WsRoundPlan& p, bool peers_eligible,
                                     bool selftest_ok) {
  const bool elig = p.multi_elig && (f.world == 1 || peers_eligible);  // world 1: nobody to ask
  const bool multi_peer = p.peer_multi && elig && selftest_ok;
  const bool multi_ok = p.multi_ok(elig, multi_peer);
  const bool xch = multi_peer || (p.peer_one && !multi_ok && selftest_ok);
  return ws_round_shape(f, p, multi_ok, xch);
}

}  // namespace dpsvm
