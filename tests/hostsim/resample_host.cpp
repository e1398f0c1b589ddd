// resample_host.cpp -- TEST-ONLY host build of the population resampling's per-element rules
// (csrc/bmpc_resample.h; bmpc_population_ancestors, bmpc_gather_egos).
//
// Two builds of this one file (tests/test_resample.py): a stand-alone program under the address and
// undefined-behaviour sanitizers -- main() below: the ancestor rule over batch sizes and weight
// families with its properties checked, and synthetic slabs gathered through a permutation, a
// broadcast and the rule's own arrangement, every child compared with a pre-call copy --, and a shared
// library whose `rs_*` symbols let the CPU tests hold the rule against bmpc/resample.py.  Never loaded
// by the belief-planning_amd package.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bmpc_resample.h"

using namespace bmpc;

// the kernel's passes, serially: prefix sums, children per slot, the packed scan, the arrangement
static void host_ancestors(int B, const uint64_t* k, uint64_t u53, int32_t* anc, int32_t* counts) {
  std::vector<uint64_t> C(B), P(B);
  uint64_t S = 0;
  for (int i = 0; i < B; ++i) C[i] = S += k[i];
  const u128 U0 = resample_offset(u53, S);
  uint64_t acc = 0;
  for (int i = 0; i < B; ++i) {
    const int n = resample_children_below(C[i], S, U0, B) - (i ? resample_children_below(C[i - 1], S, U0, B) : 0);
    if (counts) counts[i] = n;
    P[i] = acc += resample_pack(n);
  }
  for (int i = 0; i < B; ++i) anc[i] = resample_arrange(P.data(), B, i);
}

extern "C" {

// k [B] and the maximum of finite-or--inf log-weights; returns the count of NaN / +inf entries
int rs_quantise(int B, const double* logw, uint64_t* k, double* M_out) {
  double M = -INFINITY;
  int bad = 0;
  for (int i = 0; i < B; ++i) {
    bad += resample_bad_logw(logw[i]) ? 1 : 0;
    if (logw[i] > M && logw[i] < INFINITY) M = logw[i];
  }
  *M_out = M;
  for (int i = 0; i < B; ++i) k[i] = bad || !(M > -INFINITY) ? 0 : resample_quantise(logw[i], M);
  return bad;
}

uint64_t rs_u53(uint64_t seed, int64_t ego_base, uint32_t round) { return resample_u53(seed, (uint64_t)ego_base, round); }

void rs_ancestors(int B, const uint64_t* k, uint64_t u53, int32_t* anc, int32_t* counts) {
  host_ancestors(B, k, u53, anc, counts);
}

void rs_raw_ancestors(int B, const uint64_t* k, uint64_t u53, int32_t* raw) {
  std::vector<uint64_t> C(B);
  uint64_t S = 0;
  for (int i = 0; i < B; ++i) C[i] = S += k[i];
  const u128 U0 = resample_offset(u53, S);
  for (int j = 0; j < B; ++j) raw[j] = resample_raw_ancestor(C.data(), B, S, U0, j);
}

double rs_ess(int B, const uint64_t* k) {
  uint64_t S = 0;
  u128 Q = 0;
  for (int i = 0; i < B; ++i) S += k[i], Q += (u128)k[i] * k[i];
  return resample_ess(S, Q);
}

double rs_new_logw(double M, uint64_t S, int B) { return resample_new_logw(M, S, B); }

double rs_to_double(uint64_t hi, uint64_t lo) { return resample_to_double(((u128)hi << 64) | lo); }

}  // extern "C"

static int failures = 0;
#define CHECK(c)                             \
  do {                                       \
    if (!(c)) {                              \
      printf("line %d: %s\n", __LINE__, #c); \
      ++failures;                            \
    }                                        \
  } while (0)

// a small deterministic generator for the weight families (splitmix64)
static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint64_t next64() {
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static double uniform01() { return (double)(next64() >> 11) * (1.0 / 9007199254740992.0); }
static double gaussian() { return sqrt(-2.0 * log(1.0 - uniform01())) * cos(6.283185307179586 * uniform01()); }

static void check_rule(int B, const std::vector<double>& logw, uint64_t u53, bool equal) {
  std::vector<uint64_t> k(B);
  double M;
  CHECK(rs_quantise(B, logw.data(), k.data(), &M) == 0);
  std::vector<int32_t> anc(B), counts(B), raw(B), hist(B, 0);
  rs_ancestors(B, k.data(), u53, anc.data(), counts.data());
  rs_raw_ancestors(B, k.data(), u53, raw.data());
  u128 S = 0;
  for (int i = 0; i < B; ++i) S += k[i];
  long total = 0;
  for (int j = 0; j < B; ++j) {
    CHECK(raw[j] >= 0 && raw[j] < B);
    if (j) CHECK(raw[j] >= raw[j - 1]);
    hist[raw[j]]++;
  }
  std::vector<int32_t> surplus;
  for (int i = 0; i < B; ++i) {
    CHECK(counts[i] == hist[i]);
    total += counts[i];
    const u128 bk = (u128)B * k[i];
    CHECK((u128)counts[i] >= bk / S && (u128)counts[i] <= (bk + S - 1) / S);
    for (int r = 1; r < counts[i]; ++r) surplus.push_back(i);
  }
  CHECK(total == B);
  size_t next = 0;
  for (int i = 0; i < B; ++i) {
    if (counts[i] > 0) CHECK(anc[i] == i);
    else CHECK(next < surplus.size() && anc[i] == surplus[next++]);
    CHECK(counts[anc[i]] > 0);   // sources are never destinations
    if (equal) CHECK(anc[i] == i);
  }
  CHECK(next == surplus.size());
}

// synthetic egos: a "slab" of `stride` doubles with two spans that move, an int32 column and a
// 40-byte policy row; everything else must stay
static void check_gather(int B, const std::vector<int32_t>& a) {
  const size_t stride = 37, off1 = 3, len1 = 5, off2 = 20, len2 = 11, polw = sizeof(bmpc_policy) / 4;
  std::vector<double> ws(B * stride), J(B);
  std::vector<int32_t> st(B);
  std::vector<bmpc_policy> pol(B);
  for (size_t i = 0; i < ws.size(); ++i) ws[i] = 0.25 * (double)i + 1.0;
  for (int e = 0; e < B; ++e) {
    J[e] = 100.0 + e, st[e] = 7 * e - 3;
    pol[e].kind = e, pol[e].reserved = -e;
    for (int q = 0; q < 4; ++q) pol[e].p[q] = e + 0.125 * q;
  }
  const std::vector<double> ws0 = ws, J0 = J;
  const std::vector<int32_t> st0 = st;
  const std::vector<bmpc_policy> pol0 = pol;
  GatherList G = {};
  G.batch = B;
  CHECK(gather_add(G, ws.data(), 2 * stride, 2 * off1, 2 * len1));
  CHECK(gather_add(G, nullptr, 2, 0, 2));   // a skipped buffer
  CHECK(gather_add(G, J.data(), 2, 0, 2));
  CHECK(gather_add(G, st.data(), 1, 0, 1));
  CHECK(gather_add(G, pol.data(), polw, 0, polw));
  CHECK(gather_add(G, ws.data(), 2 * stride, 2 * off2, 2 * len2));
  CHECK(G.nseg == 5 && G.row_words == 2 * (len1 + len2) + 2 + 1 + polw);
  std::vector<uint32_t> stage((size_t)B * G.row_words);   // exactly its size: the sanitizer sees an overrun
  for (int lanes : {1, 3})
    for (int j = 0; j < B; ++j)
      for (int l = 0; l < lanes; ++l) gather_stage_ego(G, a.data(), stage.data(), j, l, lanes);
  for (int j = 0; j < B; ++j) gather_commit_ego(G, a.data(), stage.data(), j, 0, 1);
  for (int j = 0; j < B; ++j) {
    const int s = a[j] < 0 ? 0 : a[j] >= B ? B - 1 : a[j];
    CHECK(gather_source(a.data(), B, j) == s);
    for (size_t i = 0; i < stride; ++i) {
      const bool moves = (i >= off1 && i < off1 + len1) || (i >= off2 && i < off2 + len2);
      CHECK(ws[j * stride + i] == ws0[(moves ? s : j) * stride + i]);
    }
    CHECK(J[j] == J0[s] && st[j] == st0[s]);
    CHECK(memcmp(&pol[j], &pol0[s], sizeof(bmpc_policy)) == 0);
  }
}

int main() {
  // the conversion: exact below 2^53, ties to even, a sticky bit far below the rounding position
  CHECK(rs_to_double(0, 12345) == 12345.0);
  CHECK(rs_to_double(1, 0) == 18446744073709551616.0);
  CHECK(rs_to_double(1, 1) == 18446744073709551616.0);
  CHECK(rs_to_double(1, 1ull << 12) == 18446744073709551616.0 + 4096.0);
  CHECK(rs_to_double(1, 1ull << 11) == 18446744073709551616.0);                    // a tie: to even
  CHECK(rs_to_double(1, (1ull << 11) | 1) == 18446744073709551616.0 + 4096.0);      // above the tie
  CHECK(rs_to_double(1, 3ull << 11) == 18446744073709551616.0 + 8192.0);           // a tie: to even, up
  CHECK(rs_to_double(~0ull, ~0ull) == ldexp(1.0, 128));
  CHECK(rs_to_double(1ull << 63, 0) == ldexp(1.0, 127));
  // the rule over the issue's sizes, families and draws
  const uint64_t draws[] = {0, 1, (1ull << 53) - 1, next64() >> 11, next64() >> 11};
  for (int B : {1, 2, 3, 63, 64, 65, 257, 1000})
    for (int fam = 0; fam < 6; ++fam)
      for (uint64_t u53 : draws) {
        std::vector<double> lw(B);
        const double sd[] = {0, 1, 5, 30, 100, 1};
        for (int i = 0; i < B; ++i) lw[i] = fam == 0 ? -3.5 : sd[fam] * gaussian();
        if (fam == 5)
          for (int i = 0; i < B / 2; ++i) lw[(2 * i + 1) % B] = -INFINITY;
        check_rule(B, lw, u53, fam == 0);
      }
  // refusals of the quantiser
  {
    double M;
    uint64_t k[3];
    const double nan3[3] = {0.0, NAN, -1.0}, inf3[3] = {0.0, INFINITY, -1.0}, dead[3] = {-INFINITY, -INFINITY, -INFINITY};
    CHECK(rs_quantise(3, nan3, k, &M) == 1 && M == 0.0 && k[0] == 0);
    CHECK(rs_quantise(3, inf3, k, &M) == 1 && M == 0.0);
    CHECK(rs_quantise(3, dead, k, &M) == 0 && M == -INFINITY && k[0] == 0 && k[2] == 0);
  }
  // one dominant ego: every child comes from it
  {
    const int B = 65;
    std::vector<double> lw(B, -200.0);
    lw[17] = 0.0;
    std::vector<uint64_t> k(B);
    double M;
    rs_quantise(B, lw.data(), k.data(), &M);
    std::vector<int32_t> anc(B), counts(B);
    rs_ancestors(B, k.data(), 12345, anc.data(), counts.data());
    for (int i = 0; i < B; ++i) CHECK(anc[i] == 17 && counts[i] == (i == 17 ? B : 0));
    CHECK(fabs(rs_ess(B, k.data()) - 1.0) < 1e-12);
    CHECK(fabs(rs_new_logw(M, k[17], B) - (-log(65.0))) < 1e-14);
  }
  // the draw: purpose 1 is not the obstacle's draw
  CHECK(rs_u53(7, 3, 2) < (1ull << 53));
  CHECK((double)rs_u53(7, 3, 2) * (1.0 / 9007199254740992.0) != obstacle_uniform(7, 3, 2));
  CHECK((double)rs_u53(7, 3, 2) * (1.0 / 9007199254740992.0) == rng_draw(7, 3, 2, RNG_PURPOSE_RESAMPLE));
  // gathers: a permutation, a broadcast, out-of-range entries (clamped) and the rule's arrangement
  {
    const int B = 9;
    check_gather(B, {1, 2, 3, 4, 5, 6, 7, 8, 0});
    check_gather(B, {4, 4, 4, 4, 4, 4, 4, 4, 4});
    check_gather(B, {1, 0, 2, 2, 4, 4, 4, 8, 7});
    check_gather(B, {-5, 1, 2, 100, 4, 5, 6, 7, 3});
    std::vector<double> lw(B);
    for (int i = 0; i < B; ++i) lw[i] = 3.0 * gaussian();
    std::vector<uint64_t> k(B);
    double M;
    rs_quantise(B, lw.data(), k.data(), &M);
    std::vector<int32_t> anc(B);
    rs_ancestors(B, k.data(), 1ull << 52, anc.data(), nullptr);
    check_gather(B, anc);
  }
  // the span list of a synthetic robust transform plan: disjoint, inside the slab
  {
    Plan P = {};
    Layout L = {};
    P.U = 7, P.T = 8, P.n = 4, P.d = 2, P.bdim = 1, P.m = 3, P.nv = 50;
    P.desc.controller = BMPC_CTRL_ROBUST, P.desc.model = BMPC_MODEL_HIGHWAY_MERGE;
    L.uLin = 0, L.pprev = 16, L.misc = 24, L.xpred = 40, L.upred = 72, L.sol = 88, L.xbar = 144;
    L.xform = 200, L.xlin = 200 + ((XF_COUNT + 7) & ~7), L.stride = L.xlin + 32;
    EgoSpan sp[EGO_MAX_SPANS];
    const int n = ego_state_spans(P, L, sp);
    CHECK(n == 8);
    for (int a = 0; a < n; ++a) {
      CHECK(sp[a].off + sp[a].len <= L.stride);
      for (int b = a + 1; b < n; ++b) CHECK(sp[a].off + sp[a].len <= sp[b].off || sp[b].off + sp[b].len <= sp[a].off);
    }
    P.desc.controller = BMPC_CTRL_CVAR, P.desc.model = BMPC_MODEL_HIGHWAY;
    CHECK(ego_state_spans(P, L, sp) == 6);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
