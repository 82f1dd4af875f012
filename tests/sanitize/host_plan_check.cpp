// host_plan_check.cpp — drives the host-only planning logic of libbprmf_amd (csrc/host_plan.cpp:
// the shard's positive lists behind bprmf_set_train_ex, the sharded runner's geometry, exchange
// capacity and apply-plan sizes, the IPC blobs' device comparison; csrc/model_plan.cpp: the
// rating-SGD levels, SVD++ lists, WRMF's CSR sides and launch plans, Item2Vec's noise CDF, NCF's
// catch-up tables) under AddressSanitizer + UndefinedBehaviorSanitizer (tests/sanitize/Makefile;
// run by tests/test_sanitizers.py).
// Every result is checked against a direct restatement; any sanitizer report aborts the run.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../../include/bprmf.h"
#include "../../recommend-lib_amd/csrc/host_plan.h"
#include "../../recommend-lib_amd/csrc/model_plan.h"

using namespace bprmf;

static int g_fail = 0, g_cases = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    ++g_cases;                                                        \
    if (!(c)) {                                                       \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++g_fail;                                                       \
    }                                                                 \
  } while (0)

// the shard CSR, restated with ordered sets (train_mat as a dok of this shard's users)
static void check_csr(std::mt19937_64& g, int64_t U, int64_t I, int64_t nnz, int64_t n_ex, int W) {
  std::vector<int32_t> u(nnz), it(nnz), eu(n_ex), ei(n_ex);
  for (int64_t k = 0; k < nnz; ++k) {
    u[k] = (int32_t)(g() % U);
    it[k] = (int32_t)(g() % I);
    if (k && g() % 5 == 0) {  // duplicates of an earlier pair
      u[k] = u[k - 1];
      it[k] = it[k - 1];
    }
  }
  for (int64_t k = 0; k < n_ex; ++k) {
    eu[k] = (int32_t)(g() % U);
    ei[k] = (int32_t)(g() % I);
  }
  for (int R = 0; R < W; ++R) {
    const int64_t L = shard_rows(U, W, R);
    ShardCsr c;
    const int rc = build_shard_csr(nnz ? u.data() : nullptr, nnz ? it.data() : nullptr, nnz,
                                   n_ex ? eu.data() : nullptr, n_ex ? ei.data() : nullptr, n_ex, U, I,
                                   W, R, L, &c);
    CHECK(rc == 0);
    if (rc) continue;
    std::vector<int32_t> wu, wi;
    std::map<int64_t, std::set<int32_t>> dok;
    for (int64_t k = 0; k < nnz; ++k)
      if (u[k] % W == R) {
        wu.push_back(u[k]);
        wi.push_back(it[k]);
        dok[u[k] / W].insert(it[k]);
      }
    for (int64_t k = 0; k < n_ex; ++k)
      if (eu[k] % W == R) dok[eu[k] / W].insert(ei[k]);
    CHECK(c.pos_u == wu && c.pos_i == wi);
    CHECK((int64_t)c.indptr.size() == L + 1 && c.indptr[0] == 0);
    bool ok = true;
    for (int64_t lu = 0; lu < L && ok; ++lu) {
      const auto f = dok.find(lu);
      const size_t want = f == dok.end() ? 0 : f->second.size();
      ok = (size_t)(c.indptr[lu + 1] - c.indptr[lu]) == want;
      if (ok && want) ok = std::equal(f->second.begin(), f->second.end(), c.indices.begin() + c.indptr[lu]);
    }
    CHECK(ok);
    CHECK(c.indptr[L] == (int64_t)c.indices.size());
  }
}

// the device search (device_common.h kth_nonmember_tree), restated on the host
static int64_t tree_count(const int32_t* keys, int64_t n, int64_t k) {
  if (n <= 0) return 0;
  int L = 1;
  for (int64_t c = 16; c < n; c *= 16) ++L;
  int64_t node = 0;
  for (int l = L - 1;; --l) {
    int c = 0;
    for (int x = 0; x < 16; ++x) c += keys[node * 16 + x] <= k;
    if (l == 0) return node * 16 + c;
    if (c == 0) return 0;
    const int sh = 4 * (l + 1);
    keys += 16 * ((n + (1LL << sh) - 1) >> sh);
    node = node * 16 + (c - 1);
  }
}

static void check_tree(std::mt19937_64& g, int64_t U, int64_t I, int64_t maxdeg) {
  std::vector<int64_t> indptr(U + 1, 0);
  std::vector<int32_t> indices;
  for (int64_t u = 0; u < U; ++u) {
    const int64_t want = g() % 7 == 0 ? 0 : (int64_t)(g() % (maxdeg + 1));
    std::set<int32_t> s;
    while ((int64_t)s.size() < std::min(want, I)) s.insert((int32_t)(g() % I));
    indices.insert(indices.end(), s.begin(), s.end());
    indptr[u + 1] = (int64_t)indices.size();
  }
  SearchTree t;
  build_search_tree(indptr, indices, &t);
  CHECK((int64_t)t.soff.size() == U + 1 && t.soff[U] == (int64_t)t.keys.size());
  bool ok = true;
  for (int64_t u = 0; u < U && ok; ++u) {
    const int64_t n = indptr[u + 1] - indptr[u];
    ok = t.soff[u] % 16 == 0;
    const int32_t* a = indices.data() + indptr[u];
    for (int rep = 0; rep < 40 && ok; ++rep) {
      const int64_t k = rep < 4 ? rep : (int64_t)(g() % (uint64_t)std::max<int64_t>(1, I - n));
      int64_t m = 0;  // brute force: #{x : a[x] - x <= k}
      for (int64_t x = 0; x < n; ++x) m += a[x] - x <= k;
      ok = tree_count(t.keys.data() + t.soff[u], n, k) == m;
    }
  }
  CHECK(ok);
}

// train rows for the rating-SGD plans: mode 0 uniform, 1 every row on one user, 2 one item
static void draw_rows(std::mt19937_64& g, int64_t U, int64_t I, int64_t n, int mode,
                      std::vector<int32_t>* u, std::vector<int32_t>* it) {
  u->resize(n);
  it->resize(n);
  const int32_t fixed_u = (int32_t)(g() % U), fixed_i = (int32_t)(g() % I);
  for (int64_t s = 0; s < n; ++s) {
    (*u)[s] = mode == 1 ? fixed_u : (int32_t)(g() % U);
    (*it)[s] = mode == 2 ? fixed_i : (int32_t)(g() % I);
  }
}

// the dependency levels (mf_level_plan): the rating of sample s is s, so a slot names its sample
static void check_levels(std::mt19937_64& g, int64_t U, int64_t I, int64_t n, int mode) {
  std::vector<int32_t> u, it;
  draw_rows(g, U, I, n, mode, &u, &it);
  std::vector<double> r(n);
  for (int64_t s = 0; s < n; ++s) r[s] = (double)s;
  MfLevelPlan p;
  const int rc = mf_level_plan(u.data(), it.data(), r.data(), n, U, I, &p);
  CHECK(rc == 0);
  if (rc) return;
  const int64_t L = p.levels;
  CHECK((int64_t)p.su.size() == n && (int64_t)p.si.size() == n && (int64_t)p.sr.size() == n);
  CHECK((int64_t)p.loff.size() == L + 1 && p.loff[0] == 0 && p.loff[L] == n);
  if ((int64_t)p.sr.size() != n || (int64_t)p.loff.size() != L + 1) return;
  std::vector<int64_t> lvl(n, -1);  // level of each sample, read back through loff
  bool ok = true, kept = true;
  for (int64_t l = 0; l < L && ok; ++l) {
    ok = p.loff[l] < p.loff[l + 1];  // no empty level
    for (int64_t d = p.loff[l]; d < p.loff[l + 1] && ok; ++d) {
      const int64_t s = (int64_t)p.sr[d];
      ok = s >= 0 && s < n && lvl[s] < 0 && p.su[d] == u[s] && p.si[d] == it[s];
      if (ok) lvl[s] = l;
      if (d > p.loff[l] && p.sr[d - 1] >= p.sr[d]) kept = false;  // train order within a level
    }
  }
  CHECK(ok);
  CHECK(kept);
  if (!ok) return;
  bool before = true, tight = true;
  for (int64_t t = 0; t < n; ++t) {
    int64_t want = 0;  // 1 + max over the earlier samples sharing t's user or item
    for (int64_t s = 0; s < t; ++s)
      if (u[s] == u[t] || it[s] == it[t]) {
        before = before && lvl[s] < lvl[t];
        want = std::max(want, lvl[s] + 1);
      }
    tight = tight && lvl[t] == want;
  }
  CHECK(before);
  CHECK(tight);
  std::vector<int64_t> hist(L + 1, 0);
  for (int64_t s = 0; s < n; ++s) hist[lvl[s] + 1]++;
  for (int64_t l = 0; l < L; ++l) hist[l + 1] += hist[l];
  CHECK(std::equal(hist.begin(), hist.end(), p.loff.begin()));
}

// SVD++'s per-user lists (svdpp_plan); dup: the first user's list repeats an item on purpose
static void check_svdpp(std::mt19937_64& g, int64_t U, int64_t I, int64_t n, int mode, bool dup) {
  std::vector<int32_t> u, it;
  draw_rows(g, U, I, n, mode, &u, &it);
  if (dup && n >= 3) {
    u[n - 1] = u[0];
    it[n - 1] = it[0];
  }
  SvdppPlan p;
  const int rc = svdpp_plan(u.data(), it.data(), n, U, I, &p);
  CHECK(rc == 0);
  if (rc) return;
  CHECK((int64_t)p.uoff.size() == U + 1 && (int64_t)p.udup.size() == U);
  CHECK((int64_t)p.uitems.size() == n && (int64_t)p.uslot.size() == n);
  if ((int64_t)p.uoff.size() != U + 1 || (int64_t)p.uitems.size() != n || (int64_t)p.uslot.size() != n) return;
  bool lists = p.uoff[0] == 0, dups = true, slots = true;
  for (int64_t x = 0; x < U && lists; ++x) {
    std::vector<int32_t> want;  // x's items in train order
    for (int64_t s = 0; s < n; ++s)
      if (u[s] == x) want.push_back(it[s]);
    lists = p.uoff[x + 1] - p.uoff[x] == (int64_t)want.size() &&
            std::equal(want.begin(), want.end(), p.uitems.begin() + p.uoff[x]);
    if (!lists) break;
    bool repeats = false;
    for (size_t q = 0; q < want.size(); ++q) {
      const size_t first = std::find(want.begin(), want.end(), want[q]) - want.begin();
      repeats = repeats || first != q;
      slots = slots && p.uslot[p.uoff[x] + q] == (int32_t)first;
    }
    dups = dups && p.udup[x] == (repeats ? 1 : 0);
  }
  CHECK(lists);
  CHECK(dups);
  CHECK(slots);
  if (dup && n >= 3) CHECK(p.udup[u[0]] == 1);
}

// one WRMF side against its dense restatement D [rows][cols] (0 = absent), and its launch plan
static void check_wrmf_side(const WrmfSide& s, const std::vector<std::vector<double>>& D, int64_t rows,
                            int64_t cols, int32_t heavy) {
  CHECK(s.rows == rows && (int64_t)s.indptr.size() == rows + 1 && s.indptr[0] == 0);
  if ((int64_t)s.indptr.size() != rows + 1) return;
  bool csr = s.indices.size() == s.conf.size() && s.indptr[rows] == (int64_t)s.indices.size();
  for (int64_t r = 0; r < rows && csr; ++r) {
    int64_t x = s.indptr[r];
    for (int64_t c = 0; c < cols && csr; ++c)
      if (D[r][c] != 0.0) {
        csr = x < s.indptr[r + 1] && s.indices[x] == c && s.conf[x] == D[r][c];
        ++x;
      }
    csr = csr && x == s.indptr[r + 1];
  }
  CHECK(csr);
  if (!csr) return;
  auto nnz = [&](int64_t r) { return s.indptr[r + 1] - s.indptr[r]; };
  std::vector<int32_t> want;  // the light rows by decreasing nnz, ties by row id
  for (int64_t r = 0; r < rows; ++r)
    if (nnz(r) <= heavy) want.push_back((int32_t)r);
  std::sort(want.begin(), want.end(),
            [&](int32_t a, int32_t b) { return nnz(a) != nnz(b) ? nnz(a) > nnz(b) : a < b; });
  CHECK(s.order == want);
  CHECK(s.n_light == (int32_t)s.order.size() && s.n_heavy == (int32_t)s.hrow.size() &&
        s.n_parts == (int32_t)s.prow.size());
  CHECK((int64_t)s.order.size() + (int64_t)s.hrow.size() == rows);
  CHECK(s.hoff.size() == s.hrow.size() + 1 && s.hoff[0] == 0 && s.hoff.back() == (int64_t)s.prow.size());
  CHECK(s.pbeg.size() == s.prow.size() && s.pend.size() == s.prow.size());
  if (s.hoff.size() != s.hrow.size() + 1 || s.pbeg.size() != s.prow.size() || s.pend.size() != s.prow.size())
    return;
  std::set<int32_t> heavy_rows(s.hrow.begin(), s.hrow.end());
  bool exact = heavy_rows.size() == s.hrow.size(), tiles = true;
  for (size_t h = 0; h < s.hrow.size() && exact && tiles; ++h) {
    const int32_t r = s.hrow[h];
    exact = r >= 0 && r < rows && nnz(r) > heavy;
    if (!exact) break;
    int64_t at = s.indptr[r];  // the parts tile the row in order, `heavy` entries each but the last
    tiles = s.hoff[h] < s.hoff[h + 1] && s.hoff[h + 1] <= (int64_t)s.prow.size();
    for (int64_t q = s.hoff[h]; q < s.hoff[h + 1] && tiles; ++q) {
      const bool last = q + 1 == s.hoff[h + 1];
      tiles = s.prow[q] == r && s.pbeg[q] == at && s.pend[q] > at &&
              (last ? s.pend[q] == s.indptr[r + 1] && s.pend[q] - at <= heavy : s.pend[q] - at == heavy);
      at = s.pend[q];
    }
  }
  CHECK(exact);
  CHECK(tiles);
}

static void check_wrmf(std::mt19937_64& g, int64_t U, int64_t I, int fill_pct, int32_t heavy, int one_user) {
  std::vector<std::vector<double>> D(U, std::vector<double>(I, 0.0)), Dt(I, std::vector<double>(U, 0.0));
  std::vector<int64_t> indptr(U + 1, 0);
  std::vector<int32_t> indices;
  std::vector<double> conf;
  for (int64_t u = 0; u < U; ++u) {
    for (int64_t i = 0; i < I; ++i) {
      if (one_user >= 0 ? u != one_user : (int)(g() % 100) >= fill_pct) continue;
      const double c = g() % 4 == 0 ? 0.0 : 1.0 + (double)(g() % 1000) / 8.0;  // stored zeros are dropped
      indices.push_back((int32_t)i);
      conf.push_back(c);
      D[u][i] = Dt[i][u] = c;
    }
    indptr[u + 1] = (int64_t)indices.size();
  }
  WrmfCsrPlan p;
  const int rc = wrmf_csr_plan(indptr.data(), indices.data(), conf.data(), (int64_t)indices.size(), U, I,
                               heavy, &p);
  CHECK(rc == 0);
  if (rc) return;
  check_wrmf_side(p.side[0], D, U, I, heavy);
  check_wrmf_side(p.side[1], Dt, I, U, heavy);  // the exact transpose, rows ascending in a column
}

static void check_cdf(std::mt19937_64& g, int64_t V) {
  std::vector<double> w(V);
  for (int64_t x = 0; x < V; ++x) w[x] = g() % 3 == 0 ? 0.0 : (double)(g() % 100000) / 7.0;
  w[g() % V] = 5.0;  // not all zero
  std::vector<float> c;
  CHECK(sgns_noise_cdf(w.data(), V, &c) == 0);
  CHECK((int64_t)c.size() == V);
  if ((int64_t)c.size() != V) return;
  double tot = 0.0, acc = 0.0;
  for (int64_t x = 0; x < V; ++x) tot += std::pow(w[x], 0.75);
  bool sums = true, rises = true;
  for (int64_t x = 0; x < V; ++x) {
    acc += std::pow(w[x], 0.75) / tot;
    if (x + 1 < V) sums = sums && c[x] == (float)acc;
    if (x) rises = rises && c[x - 1] <= c[x];
  }
  CHECK(sums);
  CHECK(rises);
  CHECK(c[V - 1] == 2.0f);
}

// NCF's catch-up tables (ncf_catch_tables): the length and every entry from the formulas
static void check_catch(double lr, double b1, double b2, int terms) {
  std::vector<float> st, pw;
  CHECK(ncf_catch_tables(lr, b1, b2, terms, &st, &pw) == 0);
  const int64_t n = (int64_t)st.size() / 2, cap = 1 << 22;
  CHECK(st.size() % 2 == 0 && n >= 1 && n <= cap && (n & (n - 1)) == 0);
  // f32 cannot tell either bias correction from 1 once b^m <= 2^-26
  auto settled = [&](int64_t m) { return std::pow(b1, (double)m) <= 0x1p-26 && std::pow(b2, (double)m) <= 0x1p-26; };
  bool smallest = n == cap || settled(n);
  for (int64_t m = 1; m < n; m *= 2) smallest = smallest && !settled(m);
  CHECK(smallest);
  bool steps = true, powers = true;
  for (int64_t s = 1; s <= n && steps; ++s)
    steps = st[2 * (s - 1)] == (float)(lr / (1.0 - std::pow(b1, (double)s))) &&
            st[2 * (s - 1) + 1] == (float)(1.0 / std::sqrt(1.0 - std::pow(b2, (double)s)));
  CHECK(steps);
  CHECK((int64_t)pw.size() == 2 * (int64_t)terms);
  if ((int64_t)pw.size() != 2 * (int64_t)terms) return;
  for (int j = 1; j <= terms; ++j)
    powers = powers && pw[2 * (j - 1)] == (float)std::pow(b1, (double)j) &&
             pw[2 * (j - 1) + 1] == (float)std::pow(b2, 0.5 * j);
  CHECK(powers);
}

int main() {
  std::mt19937_64 g(20261017);
  // the sibling models' plans (model_plan.cpp): empty input, one user, one item, every row on one
  // user or one item, random small shapes
  check_levels(g, 1, 1, 0, 0);
  check_levels(g, 1, 7, 30, 0);
  check_levels(g, 7, 1, 30, 0);
  check_svdpp(g, 1, 1, 0, 0, false);
  check_svdpp(g, 1, 5, 40, 0, true);
  check_svdpp(g, 4, 6, 3, 0, true);
  for (int rep = 0; rep < 60; ++rep) {
    const int64_t U = 1 + (int64_t)(g() % 12), I = 1 + (int64_t)(g() % 12), n = (int64_t)(g() % 201);
    check_levels(g, U, I, n, rep % 3);
    check_svdpp(g, U, I, n, rep % 3, rep % 2 == 0);
  }
  {  // an id out of range, at either end of either column: refused, with nothing half-built
    const int32_t us[4][3] = {{0, 5, 1}, {0, -1, 1}, {0, 1, 2}, {0, 1, 2}};
    const int32_t is[4][3] = {{1, 1, 1}, {1, 1, 1}, {1, 4, 1}, {1, 1, -1}};
    const double r[3] = {1.0, 2.0, 3.0};
    for (int c = 0; c < 4; ++c) {
      MfLevelPlan p;
      CHECK(mf_level_plan(us[c], is[c], r, 3, 5, 4, &p) == BPRMF_E_RANGE);
      CHECK(p.su.empty() && p.si.empty() && p.sr.empty() && p.loff.empty() && p.levels == 0);
      SvdppPlan q;
      CHECK(svdpp_plan(us[c], is[c], 3, 5, 4, &q) == BPRMF_E_RANGE);
      CHECK(q.uoff.empty() && q.uitems.empty() && q.udup.empty() && q.uslot.empty());
    }
  }
  for (int32_t heavy : {1, 3, 1000}) {
    check_wrmf(g, 1, 1, 0, heavy, -1);   // no entry at all
    check_wrmf(g, 1, 9, 100, heavy, 0);  // one user
    check_wrmf(g, 8, 11, 100, heavy, 5); // every entry on one user
    for (int rep = 0; rep < 20; ++rep)
      check_wrmf(g, 1 + (int64_t)(g() % 12), 1 + (int64_t)(g() % 12), (int)(g() % 101), heavy, -1);
  }
  {  // wrmf_set_train's documented BPRMF_E_RANGE cases; 2 users, 4 items
    struct Bad {
      int64_t indptr[3];
      int32_t indices[3];
      int64_t nnz;
    };
    const Bad bad[] = {
        {{1, 2, 3}, {0, 1, 2}, 3},   // indptr does not start at 0
        {{0, 2, 2}, {0, 1, 2}, 3},   // ... or end at nnz
        {{0, 3, 2}, {0, 1, 2}, 2},   // a row running past nnz
        {{0, 2, 1}, {0, 1, 2}, 1},   // indptr decreases
        {{0, 2, 3}, {0, 4, 2}, 3},   // column past the end
        {{0, 2, 3}, {-1, 1, 2}, 3},  // negative column
        {{0, 2, 3}, {1, 1, 2}, 3},   // a repeated column
        {{0, 3, 3}, {0, 2, 1}, 3},   // columns not increasing
    };
    const double conf[3] = {1.0, 2.0, 3.0};
    for (const Bad& b : bad) {
      WrmfCsrPlan p;
      CHECK(wrmf_csr_plan(b.indptr, b.indices, conf, b.nnz, 2, 4, 3, &p) == BPRMF_E_RANGE);
      CHECK(p.side[0].indptr.empty() && p.side[1].indptr.empty() && p.side[0].hoff.empty());
    }
  }
  for (int64_t V : {2LL, 3LL, 12LL, 200LL}) check_cdf(g, V);
  {  // a negative weight, a NaN, all zeros
    std::vector<float> c(3, 1.f);
    const double neg[3] = {1.0, -0.5, 2.0}, nan_[3] = {1.0, std::nan(""), 2.0}, zero[3] = {0.0, 0.0, 0.0};
    CHECK(sgns_noise_cdf(neg, 3, &c) == BPRMF_E_INVALID && c.empty());
    CHECK(sgns_noise_cdf(nan_, 3, &c) == BPRMF_E_INVALID && c.empty());
    CHECK(sgns_noise_cdf(zero, 3, &c) == BPRMF_E_INVALID && c.empty());
  }
  // torch's default betas, no momentum at all, either one alone, and a beta2 whose bias correction
  // outlasts the cap of 2^22 steps (f32 values, as the ABI carries them)
  check_catch(1e-3f, 0.9f, 0.999f, 192);
  check_catch(1e-3f, 0.0, 0.0, 192);
  check_catch(0.5, 0.5f, 0.0, 5);
  check_catch(1e-3f, 0.0, 0.999f, 0);
  check_catch(1e-3f, 0.9f, 0.999999f, 192);
  {
    std::vector<float> st(2, 1.f), pw(2, 1.f);
    CHECK(ncf_catch_tables(1e-3, 1.0, 0.5, 4, &st, &pw) == BPRMF_E_INVALID && st.empty() && pw.empty());
    CHECK(ncf_catch_tables(1e-3, 0.5, -0.1, 4, &st, &pw) == BPRMF_E_INVALID && st.empty() && pw.empty());
    CHECK(ncf_catch_tables(1e-3, 0.5, 0.5, -1, &st, &pw) == BPRMF_E_INVALID && st.empty() && pw.empty());
  }
  // the sampler's search trees: empty users, one node, 2-4 levels (up to 16^3 + positives)
  check_tree(g, 50, 40, 16);
  check_tree(g, 200, 3000, 300);
  check_tree(g, 12, 100000, 70000);
  // shard CSR: empty input, small and skewed shapes, every world size up to one node's 16 ranks
  check_csr(g, 1, 1, 0, 0, 1);
  check_csr(g, 5, 3, 0, 4, 2);
  check_csr(g, 40, 48, 200, 0, 1);  // ncf_set_train's shape: one rank, no exclusions, duplicates
  for (int W : {1, 2, 3, 4, 7, 8, 16})
    for (int rep = 0; rep < 3; ++rep)
      check_csr(g, 1 + (int64_t)(g() % 300), 1 + (int64_t)(g() % 200), (int64_t)(g() % 5000),
                (int64_t)(g() % 300), W);
  {  // out-of-range ids and bad geometry are refused, with nothing half-built
    const int32_t u[2] = {0, 7}, it[2] = {1, 1};
    ShardCsr c;
    CHECK(build_shard_csr(u, it, 2, nullptr, nullptr, 0, 5, 4, 1, 0, 5, &c) == BPRMF_E_RANGE);
    const int32_t eu[1] = {1}, ei[1] = {9};
    CHECK(build_shard_csr(u, it, 1, eu, ei, 1, 5, 4, 1, 0, 5, &c) == BPRMF_E_RANGE);
    CHECK(build_shard_csr(u, it, 1, nullptr, nullptr, 0, 5, 4, 2, 0, 5, &c) == BPRMF_E_INVALID);
    CHECK(build_shard_csr(u, it, 1, nullptr, nullptr, 0, 5, 4, 2, 2, 2, &c) == BPRMF_E_INVALID);
    CHECK(build_shard_csr(nullptr, nullptr, 3, nullptr, nullptr, 0, 5, 4, 1, 0, 5, &c) == BPRMF_E_INVALID);
    CHECK(c.indptr.empty());
  }
  // shard rows partition every table
  for (int W = 1; W <= 16; ++W)
    for (int64_t T : {1LL, 2LL, 15LL, 16LL, 17LL, 26744LL, 100000000LL}) {
      int64_t s = 0;
      for (int R = 0; R < W; ++R) s += shard_rows(T, W, R);
      CHECK(s == T);
    }
  // runner geometry: ml-20m and C5 shapes at every world size, sizes without overflow
  for (int W = 1; W <= 16; ++W)
    for (int64_t I : {1LL, 7LL, 26744LL, 100000000LL})
      for (int64_t B : {1LL, 512LL, 4096LL, 8192LL}) {
        RunnerGeom rg;
        CHECK(runner_geom(B, I, W, 256, 256, &rg) == 0);
        const int64_t iloc = (I + W - 1) / W;
        CHECK(rg.S == (int)std::min<int64_t>(2 * B, iloc) && rg.S >= 1);
        CHECK((__int128)rg.row_elems == (__int128)W * rg.S * 256);
        CHECK((__int128)rg.id_elems == (__int128)W * 256 * rg.S);
        for (int cap : {0, 1, 63, 64, 65, rg.S})
          CHECK((__int128)aplan_words(256, W, cap) == (__int128)256 * W * (cap > 0 ? cap : 1) * (2 * W + 1));
      }
  {
    RunnerGeom rg;
    CHECK(runner_geom(0, 5, 1, 32, 1, &rg) == BPRMF_E_INVALID);
    CHECK(runner_geom(4, 5, 0, 32, 1, &rg) == BPRMF_E_INVALID);
  }
  // exchange capacity: in range it is raw (eager) or raw rounded up to 64, capped at S (graph)
  for (int S : {1, 63, 64, 65, 1000, 8192})
    for (int raw = -2; raw <= S + 2; ++raw) {
      const int e = exchange_capacity(raw, S, false), q = exchange_capacity(raw, S, true);
      if (raw < 0 || raw > S) {
        CHECK(e == -1 && q == -1);
      } else {
        CHECK(e == raw);
        CHECK(q >= raw && q <= S && (q == S || q % 64 == 0) && (raw > 0 || q == 0));
      }
    }
  // IPC blobs: ranks on one device are seen, ranks on distinct devices are not
  {
    const size_t bb = 512, off = 5 * 64, bus = 64;
    std::vector<uint8_t> blobs(8 * bb, 0);
    auto put = [&](int r, const char* id) { strncpy((char*)blobs.data() + r * bb + off, id, bus - 1); };
    for (int r = 0; r < 8; ++r) {
      char id[32];
      snprintf(id, sizeof id, "0000:%02x:00.0", 0x11 + r);
      put(r, id);
    }
    for (int r = 0; r < 8; ++r) CHECK(!ipc_shares_device(blobs.data(), 8, r, bb, off, bus));
    put(5, "0000:13:00.0");  // rank 5 on rank 2's GPU
    CHECK(ipc_shares_device(blobs.data(), 8, 2, bb, off, bus));
    CHECK(ipc_shares_device(blobs.data(), 8, 5, bb, off, bus));
    CHECK(!ipc_shares_device(blobs.data(), 8, 0, bb, off, bus));
    CHECK(!ipc_shares_device(blobs.data(), 1, 0, bb, off, bus));
    CHECK(!ipc_shares_device(blobs.data(), 8, 0, bb, bb - 8, bus));  // field past the blob
  }
  {  // the node barrier (node_barrier.cpp): one rank, a wrong world, then forked ranks
    char path[64];
    snprintf(path, sizeof path, "/tmp/bprmf_nb_check_%d", (int)getpid());
    void* b = nullptr;
    CHECK(bprmf_node_barrier_open(path, 1, 0, 1, &b) == 0);
    for (int k = 0; k < 1000; ++k) CHECK(bprmf_node_barrier_wait(b, 5.0) == 0);
    void* w = nullptr;
    CHECK(bprmf_node_barrier_open(path, 3, 1, 0, &w) == BPRMF_E_STATE && w == nullptr);
    CHECK(bprmf_node_barrier_close(b) == 0);
    const int W = 3, iters = 300;
    CHECK(bprmf_node_barrier_open(path, W, 0, 1, &b) == 0);
    for (int r = 1; r < W; ++r) {
      if (fork() == 0) {  // a rank: meets the others iters times, then exits with its status
        void* c = nullptr;
        int bad = bprmf_node_barrier_open(path, W, r, 0, &c) != 0;
        for (int k = 0; k < iters && !bad; ++k) bad = bprmf_node_barrier_wait(c, 30.0) != 0;
        bprmf_node_barrier_close(c);
        _exit(bad);
      }
    }
    bool ok = true;
    for (int k = 0; k < iters && ok; ++k) ok = bprmf_node_barrier_wait(b, 30.0) == 0;
    CHECK(ok);
    for (int r = 1; r < W; ++r) {
      int st = 0;
      wait(&st);
      CHECK(WIFEXITED(st) && WEXITSTATUS(st) == 0);
    }
    CHECK(bprmf_node_barrier_close(b) == 0);
    unlink(path);
  }
  printf("host_plan_check: %s, %d cases\n", g_fail ? "FAILED" : "ok", g_cases);
  return g_fail ? 1 : 0;
}
