// The record space that the run limits (limits_host.inc), the submit limits (submit_host.inc) and the usage tables (usage_host.inc) all
// address: five tables back to back — user x qos, user_acct x partition, account x qos, account x partition, qos — then one "exists" array
// each for users, accounts and QoS.  One description of it (Space), one walk of the account chains, one range rule for a row's keys.
// No HIP in here: engine.hip includes it through the three *_check_host.inc, the CPU tests compile it with g++.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/crane_gpu/run_limits.h"

namespace cns_acct {

constexpr uint64_t kMaxRecords = 0xFFFFFFF0ull;   // record ids and the "no record" key stay a uint32

struct Verdict {   // what a *_check_host.inc of the three features answers
  int code = 0;   // CNS_OK, CNS_ERR_INVALID_ARG or CNS_ERR_UNSUPPORTED
  std::string msg;
  explicit operator bool() const { return code != 0; }
};
inline Verdict refuse(int code, std::string msg) {
  Verdict v;
  v.code = code; v.msg = std::move(msg);
  return v;
}

struct Space {
  uint64_t U = 0, UA = 0, A = 0, Q = 0, Pn = 0;
  uint64_t len[5] = {0, 0, 0, 0, 0};    // records of user_qos, user_part, acct_qos, acct_part, qos_usage
  uint64_t base[5] = {0, 0, 0, 0, 0};   // first record of each table
  uint64_t ent[3] = {0, 0, 0};          // first exists value of users, accounts, QoS (behind the records)
  uint64_t ent_len[3] = {0, 0, 0};      // U, A, Q
  uint64_t NR = 0, NE = 0;              // records, entities
};

// False when one table alone has more than kMaxRecords records.  Every count is below 2^32 and every table that passes at most
// kMaxRecords, so no sum in here can wrap.  Whether NR (+ NE) as a whole fits is the caller's rule.
inline bool make_space(uint32_t U, uint32_t UA, uint32_t A, uint32_t Q, uint32_t Pn, Space* out) {
  Space s;
  s.U = U; s.UA = UA; s.A = A; s.Q = Q; s.Pn = Pn;
  s.len[0] = s.U * s.Q; s.len[1] = s.UA * s.Pn; s.len[2] = s.A * s.Q; s.len[3] = s.A * s.Pn; s.len[4] = s.Q;
  for (int w = 0; w < 5; ++w)
    if (s.len[w] > kMaxRecords) return false;
  for (int w = 0; w < 5; ++w) { s.base[w] = s.NR; s.NR += s.len[w]; }
  s.ent_len[0] = s.U; s.ent_len[1] = s.A; s.ent_len[2] = s.Q;
  for (int w = 0; w < 3; ++w) { s.ent[w] = s.NR + s.NE; s.NE += s.ent_len[w]; }
  *out = s;
  return true;
}

// What a walk of the account chains found: nothing, or the first offending account and what is wrong with it.
struct ChainFinding {
  enum What { kOk, kParentRange, kNoEnd, kTooLong } what = kOk;
  uint64_t account = 0;   // kParentRange: the account whose parent is out of range; otherwise the account the chain starts at
  bool cut_short = false; // kNoEnd / kTooLong: found after CNS_LIM_MAX_CHAIN accounts without a level, not by the chain's counted length
  explicit operator bool() const { return what != kOk; }
};

// The rule of acct_parent: every parent CNS_LIM_NONE or below A, every chain ends, at most CNS_LIM_MAX_CHAIN accounts from an account to
// its root.  parents_first: all parents are ranged before any chain is walked (submit, usage); otherwise a parent is ranged when the walk
// of the accounts in ascending order reaches it (limits).  level: filled with every account's depth (root = 0) when nothing is found.
// Accounts that passed keep their level, so every account is walked once.
inline ChainFinding walk_chains(const uint32_t* parent, uint64_t A, bool parents_first, std::vector<uint32_t>* level) {
  ChainFinding f;
  if (parents_first)
    for (uint64_t a = 0; a < A; ++a)
      if (parent[a] != CNS_LIM_NONE && parent[a] >= A) { f.what = ChainFinding::kParentRange; f.account = a; return f; }
  std::vector<uint32_t> lv(A, CNS_LIM_NONE);
  for (uint64_t a = 0; a < A; ++a) {
    uint32_t chain[CNS_LIM_MAX_CHAIN];
    uint32_t n = 0, x = (uint32_t)a, from = (uint32_t)a;
    f.account = a;
    while (x != CNS_LIM_NONE) {
      if (x >= A) { f.what = ChainFinding::kParentRange; f.account = from; return f; }
      if (lv[x] != CNS_LIM_NONE) break;
      if (n == CNS_LIM_MAX_CHAIN) {   // too long already; whether it ends decides which of the two
        uint64_t more = 0;
        while (x != CNS_LIM_NONE && x < A && more <= A) { x = parent[x]; ++more; }
        f.what = more > A ? ChainFinding::kNoEnd : ChainFinding::kTooLong;
        f.cut_short = true;
        return f;
      }
      chain[n++] = from = x;
      x = parent[x];
    }
    uint32_t l = x == CNS_LIM_NONE ? 0 : lv[x] + 1;
    while (n) lv[chain[--n]] = l++;
    if (lv[a] >= CNS_LIM_MAX_CHAIN) { f.what = ChainFinding::kTooLong; return f; }
  }
  if (level) *level = std::move(lv);
  return {};
}

// The keys of one row against the five counts.  none_is_a_user_acct: CNS_LIM_NONE is accepted as user_acct (submit, usage).
inline bool keys_in_range(const Space& s, uint32_t user, uint32_t user_acct, uint32_t account, uint32_t qos, uint32_t partition,
                          bool none_is_a_user_acct) {
  return user < s.U && account < s.A && qos < s.Q && partition < s.Pn &&
         (user_acct < s.UA || (none_is_a_user_acct && user_acct == CNS_LIM_NONE));
}

}  // namespace cns_acct
