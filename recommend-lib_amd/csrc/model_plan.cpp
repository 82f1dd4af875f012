// model_plan.cpp — host-only planning logic of the sibling model paths (model_plan.h).  No HIP:
// linked into libbprmf_amd.so and, with status.cpp, into the ASan + UBSan checker of
// tests/sanitize.
#include "model_plan.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <numeric>
#include <utility>

#include "../../include/bprmf.h"
#include "status.h"

namespace bprmf {

int mf_level_plan(const int32_t* users, const int32_t* items, const double* ratings, int64_t n,
                  int64_t user_num, int64_t item_num, MfLevelPlan* out) {
  *out = MfLevelPlan();
  const int64_t U = user_num, I = item_num;
  // dependency levels, in train-set order
  std::vector<int32_t> lu(U, -1), li(I, -1), lvl(n);
  int32_t L = 0;
  for (int64_t s = 0; s < n; ++s) {
    const int32_t u = users[s], i = items[s];
    if (u < 0 || u >= U || i < 0 || i >= I)
      return fail(BPRMF_E_RANGE, "train row %lld = (%d, %d) out of range", (long long)s, u, i);
    const int32_t l = std::max(lu[u], li[i]) + 1;
    lvl[s] = lu[u] = li[i] = l;
    L = std::max(L, l + 1);
  }
  // stable counting sort by level
  std::vector<int32_t> off(L + 1, 0);
  for (int64_t s = 0; s < n; ++s) off[lvl[s] + 1]++;
  for (int32_t l = 0; l < L; ++l) off[l + 1] += off[l];
  std::vector<int32_t> pos(off.begin(), off.end() - 1), su(n), si(n);
  std::vector<double> sr(n);
  for (int64_t s = 0; s < n; ++s) {
    const int32_t d = pos[lvl[s]]++;
    su[d] = users[s];
    si[d] = items[s];
    sr[d] = ratings[s];
  }
  out->su = std::move(su);
  out->si = std::move(si);
  out->sr = std::move(sr);
  out->loff = std::move(off);
  out->levels = L;
  return 0;
}

int svdpp_plan(const int32_t* users, const int32_t* items, int64_t n, int64_t user_num,
               int64_t item_num, SvdppPlan* out) {
  *out = SvdppPlan();
  const int64_t U = user_num, I = item_num;
  std::vector<int32_t> off(U + 1, 0), list(n), dup(U, 0);
  for (int64_t s = 0; s < n; ++s) {
    const int32_t u = users[s], i = items[s];
    if (u < 0 || u >= U || i < 0 || i >= I)
      return fail(BPRMF_E_RANGE, "train row %lld = (%d, %d) out of range", (long long)s, u, i);
    off[u + 1]++;
  }
  for (int64_t u = 0; u < U; ++u) off[u + 1] += off[u];
  std::vector<int32_t> pos(off.begin(), off.end() - 1);
  for (int64_t s = 0; s < n; ++s) list[pos[users[s]]++] = items[s];
  std::vector<int32_t> seen(I, -1), first(I, 0), slot(n);
  for (int64_t u = 0; u < U; ++u)
    for (int32_t q = off[u]; q < off[u + 1]; ++q) {
      const int32_t it = list[q];
      if (seen[it] == (int32_t)u) {
        dup[u] = 1;
      } else {
        seen[it] = (int32_t)u;
        first[it] = q - off[u];
      }
      slot[q] = first[it];
    }
  out->uoff = std::move(off);
  out->uitems = std::move(list);
  out->udup = std::move(dup);
  out->uslot = std::move(slot);
  return 0;
}

namespace {
// the launch plan of one side over its finished CSR arrays
int plan_side(WrmfSide& s, int32_t heavy) {
  const std::vector<int64_t>& indptr = s.indptr;
  std::vector<int32_t> by(s.rows);
  std::iota(by.begin(), by.end(), 0);
  std::stable_sort(by.begin(), by.end(), [&](int32_t a, int32_t b) {
    return indptr[a + 1] - indptr[a] > indptr[b + 1] - indptr[b];
  });
  s.hoff.assign(1, 0);
  for (int32_t r : by) {
    const int64_t b = indptr[r], e = indptr[r + 1];
    if (e - b <= heavy) {
      s.order.push_back(r);
      continue;
    }
    s.hrow.push_back(r);
    for (int64_t x = b; x < e; x += heavy) {
      s.prow.push_back(r);
      s.pbeg.push_back(x);
      s.pend.push_back(std::min<int64_t>(x + heavy, e));
    }
    s.hoff.push_back((int64_t)s.prow.size());
  }
  if (s.prow.size() >= (size_t)INT32_MAX) return fail(BPRMF_E_UNSUPPORTED, "too many heavy-row parts");
  s.n_light = (int32_t)s.order.size();
  s.n_heavy = (int32_t)s.hrow.size();
  s.n_parts = (int32_t)s.prow.size();
  return 0;
}
}  // namespace

int wrmf_csr_plan(const int64_t* indptr, const int32_t* indices, const double* conf, int64_t nnz,
                  int64_t user_num, int64_t item_num, int32_t heavy, WrmfCsrPlan* out) {
  *out = WrmfCsrPlan();
  const int64_t U = user_num, I = item_num;
  if (indptr[0] != 0 || indptr[U] != nnz) return fail(BPRMF_E_RANGE, "indptr must run from 0 to nnz");
  // validate, drop zero confidences (the reference's Pu != 0), count the columns
  std::vector<int64_t> up_(U + 1, 0), ip(I + 1, 0);
  std::vector<int32_t> ui;
  std::vector<double> uc;
  ui.reserve(nnz);
  uc.reserve(nnz);
  for (int64_t u = 0; u < U; ++u) {
    const int64_t b = indptr[u], e = indptr[u + 1];
    if (b > e || e > nnz) return fail(BPRMF_E_RANGE, "indptr decreases at row %lld", (long long)u);
    for (int64_t x = b; x < e; ++x) {
      const int32_t i = indices[x];
      if (i < 0 || i >= I) return fail(BPRMF_E_RANGE, "column %d of row %lld out of range", i, (long long)u);
      if (x > b && indices[x - 1] >= i)
        return fail(BPRMF_E_RANGE, "row %lld: column indices must be strictly increasing", (long long)u);
      if (conf[x] == 0.0) continue;
      ui.push_back(i);
      uc.push_back(conf[x]);
      ip[i + 1]++;
    }
    up_[u + 1] = (int64_t)ui.size();
  }
  for (int64_t i = 0; i < I; ++i) ip[i + 1] += ip[i];
  const int64_t kept = (int64_t)ui.size();
  std::vector<int32_t> ii(kept);
  std::vector<double> ic(kept);
  std::vector<int64_t> pos(ip.begin(), ip.end() - 1);
  for (int64_t u = 0; u < U; ++u)
    for (int64_t x = up_[u]; x < up_[u + 1]; ++x) {
      const int64_t q = pos[ui[x]]++;
      ii[q] = (int32_t)u;
      ic[q] = uc[x];
    }
  WrmfCsrPlan p;
  p.side[0].rows = U;
  p.side[0].indptr = std::move(up_);
  p.side[0].indices = std::move(ui);
  p.side[0].conf = std::move(uc);
  p.side[1].rows = I;
  p.side[1].indptr = std::move(ip);
  p.side[1].indices = std::move(ii);
  p.side[1].conf = std::move(ic);
  for (WrmfSide& s : p.side)
    if (int r = plan_side(s, heavy)) return r;
  *out = std::move(p);
  return 0;
}

int sgns_noise_cdf(const double* weights, int64_t vocab, std::vector<float>* cdf) {
  cdf->clear();
  const int64_t V = vocab;
  // SGNS.__init__: wf = weights^0.75, wf / wf.sum() (:77-80); its CDF for inverse sampling
  std::vector<double> wf(V);
  double tot = 0.0;
  for (int64_t x = 0; x < V; ++x) {
    if (!(weights[x] >= 0.0)) return fail(BPRMF_E_INVALID, "weights must be >= 0");
    wf[x] = std::pow(weights[x], 0.75);
    tot += wf[x];
  }
  if (!(tot > 0.0)) return fail(BPRMF_E_INVALID, "weights sum to 0");
  std::vector<float> c(V);
  double acc = 0.0;
  for (int64_t x = 0; x < V; ++x) {
    acc += wf[x] / tot;
    c[x] = (float)acc;
  }
  c[V - 1] = 2.0f;  // every u in [0, 1) lands
  *cdf = std::move(c);
  return 0;
}

static int slim_plan_build(const int32_t* users, const int32_t* items, int64_t n, int64_t user_num,
                           int64_t item_num, SlimPlan* out) {
  const int64_t U = user_num, I = item_num;
  if (U < 0 || I < 0 || n < 0 || U >= INT32_MAX - kSlimTile || I >= INT32_MAX - kSlimTile)
    return fail(BPRMF_E_UNSUPPORTED, "user_num and item_num must be in [0, 2^31 - %lld)",
                (long long)(kSlimTile + 1));
  // counting sort by user, then the items of every user sorted and made unique
  std::vector<int64_t> off(U + 1, 0);
  for (int64_t s = 0; s < n; ++s) {
    const int32_t u = users[s], i = items[s];
    if (u < 0 || u >= U || i < 0 || i >= I)
      return fail(BPRMF_E_RANGE, "train pair %lld = (%d, %d) out of range", (long long)s, u, i);
    off[u + 1]++;
  }
  for (int64_t u = 0; u < U; ++u) off[u + 1] += off[u];
  std::vector<int32_t> list(n);
  {
    std::vector<int64_t> pos(off.begin(), off.end() - 1);
    for (int64_t s = 0; s < n; ++s) list[pos[users[s]]++] = items[s];
  }
  std::vector<int64_t> indptr(U + 1, 0);
  std::vector<int32_t> indices, rows;
  indices.reserve(n);
  rows.reserve(n);
  for (int64_t u = 0; u < U; ++u) {
    auto b = list.begin() + off[u], e = list.begin() + off[u + 1];
    std::sort(b, e);
    e = std::unique(b, e);
    indices.insert(indices.end(), b, e);
    rows.insert(rows.end(), (size_t)(e - b), (int32_t)u);
    indptr[u + 1] = (int64_t)indices.size();
  }
  const int64_t p_pad = (I + kSlimTile - 1) / kSlimTile * kSlimTile;
  const int64_t k_pad = (U + kSlimTile - 1) / kSlimTile * kSlimTile;
  if (k_pad && p_pad > INT64_MAX / k_pad)
    return fail(BPRMF_E_UNSUPPORTED, "the dense operand's size overflows");
  out->indptr = std::move(indptr);
  out->indices = std::move(indices);
  out->rows = std::move(rows);
  out->p_pad = p_pad;
  out->k_pad = k_pad;
  out->operand_bytes = p_pad * k_pad;
  return 0;
}

int slim_plan(const int32_t* users, const int32_t* items, int64_t n, int64_t user_num,
              int64_t item_num, SlimPlan* out) {
  *out = SlimPlan();
  try {  // the vectors hold user_num + 1 and n entries: no exception may cross the C ABI
    return slim_plan_build(users, items, n, user_num, item_num, out);
  } catch (const std::bad_alloc&) {
    *out = SlimPlan();
    return fail(BPRMF_E_UNSUPPORTED, "out of host memory while planning %lld pairs of %lld users",
                (long long)n, (long long)user_num);
  }
}

int slim_check_ids(const int32_t* users, const int32_t* items, int64_t n, int64_t user_num,
                   int64_t item_num) {
  for (int64_t x = 0; x < n; ++x) {
    if (users[x] < 0 || users[x] >= user_num)
      return fail(BPRMF_E_RANGE, "user %lld = %d out of range", (long long)x, users[x]);
    if (items && (items[x] < 0 || items[x] >= item_num))
      return fail(BPRMF_E_RANGE, "pair %lld = (%d, %d) out of range", (long long)x, users[x], items[x]);
  }
  return 0;
}

int slim_check_lists(const int32_t* users, const int64_t* offsets, const int32_t* items,
                     int64_t n_users, int64_t user_num, int64_t item_num) {
  if (n_users <= 0) return 0;
  if (offsets[0] < 0) return fail(BPRMF_E_INVALID, "offsets must start at >= 0");
  for (int64_t r = 0; r < n_users; ++r) {
    if (users[r] < 0 || users[r] >= user_num)
      return fail(BPRMF_E_RANGE, "user %lld = %d out of range", (long long)r, users[r]);
    if (offsets[r + 1] < offsets[r]) return fail(BPRMF_E_INVALID, "offsets must not decrease");
  }
  for (int64_t q = offsets[0]; q < offsets[n_users]; ++q)
    if (items[q] < 0 || items[q] >= item_num)
      return fail(BPRMF_E_RANGE, "candidate %lld = %d out of range", (long long)q, items[q]);
  return 0;
}

int ncf_catch_tables(double lr, double b1, double b2, int terms, std::vector<float>* step,
                     std::vector<float>* pw) {
  step->clear();
  pw->clear();
  if (!(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0) || terms < 0)
    return fail(BPRMF_E_INVALID, "bad Adam hyper-parameters");
  int64_t n = 1;
  while (n < (1 << 22) && (std::pow(b1, (double)n) > 0x1p-26 || std::pow(b2, (double)n) > 0x1p-26)) n *= 2;
  std::vector<float> st(2 * (size_t)n), p(2 * (size_t)terms);
  for (int64_t s = 1; s <= n; ++s) {
    st[2 * (s - 1)] = (float)(lr / (1.0 - std::pow(b1, (double)s)));
    st[2 * (s - 1) + 1] = (float)(1.0 / std::sqrt(1.0 - std::pow(b2, (double)s)));
  }
  for (int j = 1; j <= terms; ++j) {
    p[2 * (j - 1)] = (float)std::pow(b1, (double)j);
    p[2 * (j - 1) + 1] = (float)std::pow(b2, 0.5 * j);
  }
  *step = std::move(st);
  *pw = std::move(p);
  return 0;
}

}  // namespace bprmf
