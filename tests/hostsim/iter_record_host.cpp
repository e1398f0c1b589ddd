// iter_record_host.cpp -- the host build of the solver (hostsim.cpp and the two plan builders) as a
// program of its own: built with -fsanitize=address,undefined and run by
// tests/test_iter_record_host.py over one closed loop whose inputs the test recorded.  The file named
// by BMPC_ITER_RECORD_CASE holds: int32 egos, steps; the plan description; per step the egos * m policies
// (the scene step re-targets them), then x, z and xref (egos * n doubles each).  Prints one line per step, "status ... iters ...".
#include <stdio.h>

#include "bmpc_plan.cpp"
#include "bmpc_qpplan.cpp"
#include "hostsim.cpp"

namespace {
template <class T>
bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
}  // namespace

int main() {
  const char* path = getenv("BMPC_ITER_RECORD_CASE");
  FILE* f = path ? fopen(path, "rb") : nullptr;
  if (!f) return printf("FAILED: no case file\n"), 2;
  int32_t hdr[2];
  bmpc_plan_desc desc;
  if (!rd(f, hdr, 2) || !rd(f, &desc, 1)) return printf("FAILED: short header\n"), 2;
  const int egos = hdr[0], steps = hdr[1];
  std::vector<bmpc_policy> pol((size_t)egos * desc.m);
  void* h = nullptr;
  if (hs_create(&desc, egos, &h) != 0) return printf("FAILED: %s\n", hs_last_error()), 2;
  int32_t info[64] = {};
  hs_info(h, info);
  const size_t nin = (size_t)egos * desc.n;
  std::vector<double> x(nin), z(nin), xref(nin), J(egos);
  std::vector<double> up((size_t)egos * info[BMPC_INFO_U] * desc.d), xp((size_t)egos * info[BMPC_INFO_T] * desc.n);
  std::vector<int32_t> st(egos), it(egos);
  for (int s = 0; s < steps; ++s) {
    if (!rd(f, pol.data(), pol.size())) return printf("FAILED: short policies\n"), 2;
    hs_set_policies(h, pol.data());
    if (!rd(f, x.data(), nin) || !rd(f, z.data(), nin) || !rd(f, xref.data(), nin)) return printf("FAILED: short step\n"), 2;
    hs_solve(h, x.data(), z.data(), xref.data(), up.data(), xp.data(), nullptr, J.data(), st.data(), it.data());
    printf("status");
    for (int e = 0; e < egos; ++e) printf(" %d", st[e]);
    printf(" iters");
    for (int e = 0; e < egos; ++e) printf(" %d", it[e]);
    printf("\n");
  }
  fclose(f);
  hs_destroy(h);
  return 0;
}
