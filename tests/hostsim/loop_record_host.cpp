// loop_record_host.cpp -- the closed loops' row writer (csrc/bmpc_record.h) on the host, as a program
// of its own: built with -fsanitize=address,undefined and run by tests/test_loop_record.py.  It
// drives the writer the way the kernels do (64 lanes per ego, one call per lane) over a fake slab and
// checks the window, the guard margins around every column, the NULL optional columns and the offset
// arithmetic beyond 2^32.  Exit status 0 and "ok" on success; the first failure is printed.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "bmpc_record.h"

using namespace bmpc;

namespace {

constexpr double kSentinel = -7777.25;
constexpr int32_t kSentinelI = -77777;
constexpr size_t kGuard = 40;   // entries before and after every column

int failures = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (failures++ == 0) {                  \
        printf("FAILED %s: ", #cond);         \
        printf(__VA_ARGS__);                  \
        printf("\n");                         \
      }                                       \
    }                                         \
  } while (0)

// a column with guard margins, everything at the sentinel
template <class T>
struct Column {
  std::vector<T> buf;
  size_t len;
  T fill;
  Column(size_t n, T s) : buf(n + 2 * kGuard, s), len(n), fill(s) {}
  T* data() { return buf.data() + kGuard; }
  bool guards_intact() const {
    for (size_t i = 0; i < kGuard; ++i)
      if (buf[i] != fill || buf[kGuard + len + i] != fill) return false;
    return true;
  }
};

// the value ego e's step t puts into entry i of column c
double val(int c, int e, int t, int i) { return 1000.0 * c + 100.0 * e + 10.0 * t + 0.001 * i; }

enum { C_SCENE = 1, C_XREF, C_UPRED, C_J, C_XPRED, C_ZPRED, C_BW };

struct Case {
  int B, capacity, t_base, t_first, t_last;
  bool with_upred, with_xpred, with_zpred, with_bw;
};

void run(const Case& c) {
  const RecordDims D{4, 2, 7, 5, 3};   // n, d, T, U, nbranch - 1
  const size_t rows = (size_t)c.B * c.capacity;
  Column<double> scene(rows * BMPC_ENV_STRIDE, kSentinel), xref(rows * D.n, kSentinel), u(rows * D.d, kSentinel),
      J(rows, kSentinel), upred(rows * D.U * D.d, kSentinel), xpred(rows * D.T * D.n, kSentinel),
      zpred(rows * D.T * D.n, kSentinel), bw(rows * D.nbw, kSentinel);
  Column<int32_t> status(rows, kSentinelI), iters(rows, kSentinelI);
  bmpc_loop_record R{};
  R.capacity = c.capacity;
  R.t_base = c.t_base;
  R.scene = scene.data();
  R.xref = xref.data();
  R.u = u.data();
  R.J = J.data();
  R.status = status.data();
  R.iters = iters.data();
  R.upred = c.with_upred ? upred.data() : nullptr;
  R.xpred = c.with_xpred ? xpred.data() : nullptr;
  R.zpred = c.with_zpred ? zpred.data() : nullptr;
  R.branch_w = c.with_bw ? bw.data() : nullptr;

  // the fake slab of one ego and step: what the kernels hand the writer
  std::vector<double> s_scene(BMPC_ENV_STRIDE), s_xref(D.n), s_upred(D.U * D.d), s_xpred(D.T * D.n),
      s_zpred(D.T * D.n), s_bw(D.nbw);
  for (int t = c.t_first; t <= c.t_last; ++t)
    for (int e = 0; e < c.B; ++e) {
      for (size_t i = 0; i < s_scene.size(); ++i) s_scene[i] = val(C_SCENE, e, t, (int)i);
      for (size_t i = 0; i < s_xref.size(); ++i) s_xref[i] = val(C_XREF, e, t, (int)i);
      for (size_t i = 0; i < s_upred.size(); ++i) s_upred[i] = val(C_UPRED, e, t, (int)i);
      for (size_t i = 0; i < s_xpred.size(); ++i) s_xpred[i] = val(C_XPRED, e, t, (int)i);
      for (size_t i = 0; i < s_zpred.size(); ++i) s_zpred[i] = val(C_ZPRED, e, t, (int)i);
      for (size_t i = 0; i < s_bw.size(); ++i) s_bw[i] = val(C_BW, e, t, (int)i);
      const double Jv = val(C_J, e, t, 0);
      const int32_t st = 10 * e + t, it = 100 * e + t;
      const RecordSrc S{s_scene.data(), s_xref.data(), s_upred.data(), &Jv, &st, &it,
                        s_xpred.data(), s_zpred.data(), s_bw.data()};
      size_t r = 0;
      const bool in = record_row_of(R, t, &r);
      CHECK(in == (t >= c.t_base && t < c.t_base + c.capacity), "window of step %d", t);
      if (!in) continue;
      CHECK(r == (size_t)(t - c.t_base), "row of step %d is %zu", t, r);
      for (int lane = 0; lane < 64; ++lane) record_write_row(R, D, (size_t)e, r, lane, 64, S);
    }

  // every row holds its own step, or the sentinel when that step did not run
  for (int e = 0; e < c.B; ++e)
    for (int r = 0; r < c.capacity; ++r) {
      const int t = c.t_base + r;
      const bool ran = t >= c.t_first && t <= c.t_last;
      const size_t row = (size_t)e * c.capacity + r;
      auto want = [&](int col, int i) { return ran ? val(col, e, t, i) : kSentinel; };
      for (int i = 0; i < BMPC_ENV_STRIDE; ++i)
        CHECK(scene.data()[row * BMPC_ENV_STRIDE + i] == want(C_SCENE, i), "scene e %d r %d i %d", e, r, i);
      for (int i = 0; i < D.n; ++i) CHECK(xref.data()[row * D.n + i] == want(C_XREF, i), "xref e %d r %d", e, r);
      for (int i = 0; i < D.d; ++i) CHECK(u.data()[row * D.d + i] == want(C_UPRED, i), "u e %d r %d", e, r);
      CHECK(J.data()[row] == want(C_J, 0), "J e %d r %d", e, r);
      CHECK(status.data()[row] == (ran ? 10 * e + t : kSentinelI), "status e %d r %d", e, r);
      CHECK(iters.data()[row] == (ran ? 100 * e + t : kSentinelI), "iters e %d r %d", e, r);
      for (int i = 0; i < D.U * D.d; ++i)
        CHECK(upred.data()[row * D.U * D.d + i] == (c.with_upred ? want(C_UPRED, i) : kSentinel), "upred e %d r %d i %d",
              e, r, i);
      for (int i = 0; i < D.T * D.n; ++i) {
        CHECK(xpred.data()[row * D.T * D.n + i] == (c.with_xpred ? want(C_XPRED, i) : kSentinel), "xpred e %d r %d i %d",
              e, r, i);
        CHECK(zpred.data()[row * D.T * D.n + i] == (c.with_zpred ? want(C_ZPRED, i) : kSentinel), "zpred e %d r %d i %d",
              e, r, i);
      }
      for (int i = 0; i < D.nbw; ++i)
        CHECK(bw.data()[row * D.nbw + i] == (c.with_bw ? want(C_BW, i) : kSentinel), "branch_w e %d r %d", e, r);
    }
  CHECK(scene.guards_intact() && xref.guards_intact() && u.guards_intact() && J.guards_intact() &&
            status.guards_intact() && iters.guards_intact() && upred.guards_intact() && xpred.guards_intact() &&
            zpred.guards_intact() && bw.guards_intact(),
        "a guard margin was written (capacity %d, steps %d..%d)", c.capacity, c.t_first, c.t_last);
}

}  // namespace

int main() {
  // B = 3, capacity 3 from step 1, steps 0..4: rows hold steps 1..3, steps 0 and 4 write nothing
  run({3, 3, 1, 0, 4, true, true, true, true});
  // core columns only, and a mix: NULL optional columns are skipped
  run({3, 3, 1, 0, 4, false, false, false, false});
  run({3, 3, 1, 0, 4, false, true, false, true});
  // a loop that stops inside the window leaves the later rows alone
  run({3, 3, 1, 0, 2, true, true, true, true});
  // a detached recorder records nothing
  {
    bmpc_loop_record R{};
    size_t r = 99;
    CHECK(!record_row_of(R, 0, &r) && r == 99, "capacity 0 must not record");
  }
  // offsets beyond 2^32: the last row of ego 65,535 at capacity 4,096 in a column 1,480 wide
  {
    const unsigned long long want = (65535ULL * 4096ULL + 4095ULL) * 1480ULL;
    const size_t got = record_offset(65535, 4096, 4095, 1480);
    CHECK(sizeof(size_t) == 8 && want > (1ULL << 32) && (unsigned long long)got == want, "offset %zu, want %llu", got,
          want);
    CHECK(record_offset(65535, 4096, 0, 1480) == (size_t)(65535ULL * 4096ULL * 1480ULL), "row 0 of ego 65535");
    // the same from int arguments, as the kernels pass them
    const int e = 65535, cap = 4096, r = 4095, T = 370, n = 4;
    CHECK((unsigned long long)record_offset((size_t)e, (size_t)cap, (size_t)r, (size_t)(T * n)) == want,
          "offset from ints");
  }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
