// slim_plan_check.cpp — drives SLIM's host-only planning (csrc/model_plan.cpp: slim_plan, the
// pair validation, the de-duplicated CSR and the geometry of the dense i8 operand; slim_check_ids
// and slim_check_lists, the validation of the scoring and ranking arguments) under
// AddressSanitizer + UndefinedBehaviorSanitizer.
// A stand-alone program: tests/test_slim_cpu.py compiles it with model_plan.cpp and status.cpp
// and runs it directly.  Every result is checked against a restatement with ordered sets; any
// sanitizer report aborts the run.
#include <stdio.h>

#include <random>
#include <set>
#include <utility>
#include <vector>

#include "../../include/bprmf.h"
#include "../../recommend-lib_amd/csrc/model_plan.h"

using namespace bprmf;

static int g_fail = 0, g_cases = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    ++g_cases;                                                      \
    if (!(c)) {                                                     \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                     \
    }                                                               \
  } while (0)

static void check_plan(std::mt19937_64& g, int64_t U, int64_t I, int64_t n) {
  std::vector<int32_t> u(n), it(n);
  std::set<std::pair<int32_t, int32_t>> want;
  for (int64_t k = 0; k < n; ++k) {
    u[k] = (int32_t)(g() % U);
    it[k] = (int32_t)(g() % I);
    if (k && g() % 4 == 0) u[k] = u[k - 1], it[k] = it[k - 1];  // duplicates collapse
    want.insert({u[k], it[k]});
  }
  SlimPlan p;
  const int rc = slim_plan(n ? u.data() : nullptr, n ? it.data() : nullptr, n, U, I, &p);
  CHECK(rc == 0);
  if (rc) return;
  CHECK((int64_t)p.indptr.size() == U + 1 && p.indptr[0] == 0);
  CHECK(p.indices.size() == want.size() && p.rows.size() == want.size());
  CHECK(p.indptr[U] == (int64_t)want.size());
  auto w = want.begin();  // (user, item) ascending = CSR order
  bool same = true;
  for (int64_t r = 0; r < U && same; ++r)
    for (int64_t q = p.indptr[r]; q < p.indptr[r + 1] && same; ++q, ++w)
      same = w != want.end() && w->first == r && w->second == p.indices[q] && p.rows[q] == r;
  CHECK(same && w == want.end());
  CHECK(p.p_pad >= I && p.p_pad % kSlimTile == 0 && p.p_pad - I < kSlimTile);
  CHECK(p.k_pad >= U && p.k_pad % kSlimTile == 0 && p.k_pad - U < kSlimTile);
  CHECK(p.operand_bytes == p.p_pad * p.k_pad);
  if (n) {  // one id out of range, at either end, in either column
    const int64_t k = (int64_t)(g() % n);
    const int32_t keep_u = u[k], keep_i = it[k];
    const int32_t bad_u[] = {-1, (int32_t)U}, bad_i[] = {-1, (int32_t)I};
    for (int b = 0; b < 2; ++b) {
      u[k] = bad_u[b];
      CHECK(slim_plan(u.data(), it.data(), n, U, I, &p) == BPRMF_E_RANGE && p.indptr.empty());
      u[k] = keep_u;
      it[k] = bad_i[b];
      CHECK(slim_plan(u.data(), it.data(), n, U, I, &p) == BPRMF_E_RANGE && p.indices.empty());
      it[k] = keep_i;
    }
  }
}

static void check_lists(std::mt19937_64& g, int64_t U, int64_t I, int64_t n_users) {
  std::vector<int32_t> users(n_users), items;
  std::vector<int64_t> off(n_users + 1, 0);
  off[0] = (int64_t)(g() % 3);
  items.resize(off[0], -7);  // before offsets[0]: never read
  for (int64_t r = 0; r < n_users; ++r) {
    users[r] = (int32_t)(g() % U);
    const int64_t len = (int64_t)(g() % 9);  // empty lists too
    for (int64_t q = 0; q < len; ++q) items.push_back((int32_t)(g() % I));
    off[r + 1] = (int64_t)items.size();
  }
  const int32_t* ip = items.empty() ? nullptr : items.data();
  CHECK(slim_check_lists(users.data(), off.data(), ip, n_users, U, I) == 0);
  {  // slim_score / slim_score_rows: n pairs, or n users with no items
    std::vector<int32_t> pi(n_users);
    for (auto& x : pi) x = (int32_t)(g() % I);
    const int32_t* up = n_users ? users.data() : nullptr;
    CHECK(slim_check_ids(up, n_users ? pi.data() : nullptr, n_users, U, I) == 0);
    CHECK(slim_check_ids(up, nullptr, n_users, U, I) == 0);
    if (n_users) {
      const int64_t r = (int64_t)(g() % n_users);
      const int32_t ku = users[r], ki = pi[r];
      for (int32_t bad : {(int32_t)-1, (int32_t)U}) {
        users[r] = bad;
        CHECK(slim_check_ids(users.data(), pi.data(), n_users, U, I) == BPRMF_E_RANGE);
        CHECK(slim_check_ids(users.data(), nullptr, n_users, U, I) == BPRMF_E_RANGE);
      }
      users[r] = ku;
      for (int32_t bad : {(int32_t)-1, (int32_t)I}) {
        pi[r] = bad;
        CHECK(slim_check_ids(users.data(), pi.data(), n_users, U, I) == BPRMF_E_RANGE);
        CHECK(slim_check_ids(users.data(), nullptr, n_users, U, I) == 0);
      }
      pi[r] = ki;
    }
  }
  if (!n_users) return;
  const int64_t r = (int64_t)(g() % n_users);
  const int32_t keep = users[r];
  users[r] = (int32_t)U;
  CHECK(slim_check_lists(users.data(), off.data(), ip, n_users, U, I) == BPRMF_E_RANGE);
  users[r] = -1;
  CHECK(slim_check_lists(users.data(), off.data(), ip, n_users, U, I) == BPRMF_E_RANGE);
  users[r] = keep;
  if (off[n_users] > off[0]) {
    const int64_t q = off[0] + (int64_t)(g() % (off[n_users] - off[0]));
    const int32_t ki = items[q];
    items[q] = (int32_t)I;
    CHECK(slim_check_lists(users.data(), off.data(), ip, n_users, U, I) == BPRMF_E_RANGE);
    items[q] = -1;
    CHECK(slim_check_lists(users.data(), off.data(), ip, n_users, U, I) == BPRMF_E_RANGE);
    items[q] = ki;
  }
  if (off[r + 1] > off[r]) {
    std::vector<int64_t> bad(off);
    std::swap(bad[r], bad[r + 1]);  // a decreasing step
    CHECK(slim_check_lists(users.data(), bad.data(), ip, n_users, U, I) == BPRMF_E_INVALID);
  }
  std::vector<int64_t> neg(off);
  neg[0] = -1;
  CHECK(slim_check_lists(users.data(), neg.data(), ip, n_users, U, I) == BPRMF_E_INVALID);
}

int main() {
  std::mt19937_64 g(20261019);
  const int64_t shapes[][3] = {{1, 1, 0},   {1, 1, 3},     {5, 3, 40},     {63, 31, 200},
                               {64, 64, 500}, {65, 129, 900}, {300, 7, 2500}, {7, 300, 2500}};
  for (const auto& s : shapes) check_plan(g, s[0], s[1], s[2]);
  SlimPlan p;
  CHECK(slim_plan(nullptr, nullptr, 0, 0, 0, &p) == 0 && p.indptr.size() == 1 && p.operand_bytes == 0);
  CHECK(slim_plan(nullptr, nullptr, 0, INT32_MAX, 4, &p) == BPRMF_E_UNSUPPORTED);
  CHECK(slim_plan(nullptr, nullptr, 0, 4, INT32_MAX, &p) == BPRMF_E_UNSUPPORTED);
  CHECK(slim_plan(nullptr, nullptr, 0, -1, 4, &p) == BPRMF_E_UNSUPPORTED);
  for (int64_t n : {0, 1, 2, 17, 100}) check_lists(g, 50, 33, n);
  if (g_fail) {
    fprintf(stderr, "slim_plan_check: %d of %d checks failed\n", g_fail, g_cases);
    return 1;
  }
  printf("slim_plan_check: ok (%d checks)\n", g_cases);
  return 0;
}
