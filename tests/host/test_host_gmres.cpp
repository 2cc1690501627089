// Host unit test of HostGmres (csrc/host_gmres.hpp), the dense part of a restart cycle of aggmg_fgmres_dev: random
// Hessenberg matrices column by column, every |g_{j+1}| and every y against a dense least-squares solve by Householder
// QR written here (long double).  No device, no HIP; built with -fsanitize=address,undefined by tests/test_fgmres_cpu.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../agglomerationmultigrid1d_amd/csrc/host_gmres.hpp"

static int g_fail = 0;
#define EXPECT(cond, ...)                      \
  do {                                         \
    if (!(cond)) {                             \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
      ++g_fail;                                \
    }                                          \
  } while (0)

static uint64_t g_state = 0x2545F4914F6CDD1Dull;
static double rnd() {   // splitmix64 -> (-1, 1)
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

// min_y || beta e_1 - H y ||_2 for the (k + 1) x k matrix H (row-major, leading dimension ld): Householder QR of
// [H | beta e_1]; returns the residual norm, y by back-substitution
static long double dense_lsq(const std::vector<double>& H, int ld, int k, double beta, std::vector<long double>& y) {
  const int m = k + 1;
  std::vector<long double> a((size_t)m * (k + 1));   // m x (k + 1), row-major
  for (int i = 0; i < m; ++i) {
    for (int j = 0; j < k; ++j) a[(size_t)i * (k + 1) + j] = H[(size_t)i * ld + j];
    a[(size_t)i * (k + 1) + k] = i == 0 ? beta : 0.0;
  }
  for (int j = 0; j < k; ++j) {
    long double nrm = 0;
    for (int i = j; i < m; ++i) nrm += a[(size_t)i * (k + 1) + j] * a[(size_t)i * (k + 1) + j];
    nrm = std::sqrt(nrm);
    if (nrm == 0) continue;
    std::vector<long double> v(m, 0.0L);
    const long double ajj = a[(size_t)j * (k + 1) + j];
    const long double al = ajj >= 0 ? -nrm : nrm;
    for (int i = j; i < m; ++i) v[i] = a[(size_t)i * (k + 1) + j];
    v[j] -= al;
    long double vv = 0;
    for (int i = j; i < m; ++i) vv += v[i] * v[i];
    if (vv == 0) continue;
    for (int c = j; c <= k; ++c) {
      long double dot = 0;
      for (int i = j; i < m; ++i) dot += v[i] * a[(size_t)i * (k + 1) + c];
      const long double f = 2 * dot / vv;
      for (int i = j; i < m; ++i) a[(size_t)i * (k + 1) + c] -= f * v[i];
    }
  }
  y.assign(k, 0.0L);
  for (int i = k - 1; i >= 0; --i) {
    long double t = a[(size_t)i * (k + 1) + k];
    for (int l = i + 1; l < k; ++l) t -= a[(size_t)i * (k + 1) + l] * y[l];
    y[i] = t / a[(size_t)i * (k + 1) + i];
  }
  return std::fabs(a[(size_t)k * (k + 1) + k]);
}

// one cycle of ncol columns; diag scales the sub-diagonal, zero_last makes the last sub-diagonal entry exactly 0
static void run_case(const char* name, int ncol, double beta, double sub_scale, bool zero_last) {
  const int ld = ncol;
  std::vector<double> H((size_t)(ncol + 1) * ld, 0.0);
  HostGmres ls;
  ls.start(beta);
  EXPECT(ls.size() == 0, "%s: size after start", name);
  double prev = beta;
  for (int j = 0; j < ncol; ++j) {
    double col[HostGmres::kMaxRestart + 1];
    for (int i = 0; i <= j; ++i) col[i] = rnd() + (i == j ? 2.0 : 0.0);   // a diagonal that keeps the matrix well away from singular
    col[j + 1] = (zero_last && j == ncol - 1) ? 0.0 : sub_scale * (0.05 + std::fabs(rnd()));
    for (int i = 0; i <= j + 1; ++i) H[(size_t)i * ld + j] = col[i];
    const double res = ls.push(col);
    EXPECT(ls.size() == j + 1, "%s: size after column %d", name, j);
    EXPECT(res <= prev * (1 + 1e-15), "%s: residual grew at column %d: %g > %g", name, j, res, prev);
    prev = res;
    std::vector<long double> yref;
    const long double ref = dense_lsq(H, ld, j + 1, beta, yref);
    EXPECT(std::fabs((long double)res - ref) <= 1e-12L * beta, "%s: column %d residual %g vs dense %Lg", name, j, res, ref);
    if (j == ncol - 1 || j % 7 == 0) {
      double y[HostGmres::kMaxRestart];
      ls.solve(y);
      long double ymax = 0;
      for (int i = 0; i <= j; ++i) ymax = std::fmax(ymax, std::fabs(yref[i]));
      for (int i = 0; i <= j; ++i)
        EXPECT(std::fabs((long double)y[i] - yref[i]) <= 1e-10L * ymax, "%s: column %d y[%d] %g vs dense %Lg", name, j, i, y[i],
               yref[i]);
    }
  }
  if (zero_last) EXPECT(prev == 0.0, "%s: a zero sub-diagonal entry ends with residual %g, not 0", name, prev);
}

int main() {
  run_case("one column", 1, 3.0, 1.0, false);
  run_case("five columns", 5, 1.0, 1.0, false);
  run_case("small sub-diagonal", 12, 7.5e-3, 1e-6, false);
  run_case("zero sub-diagonal (happy breakdown)", 6, 2.0, 1.0, true);
  run_case("zero sub-diagonal in the first column", 1, 2.0, 1.0, true);
  run_case("full cycle of 64", HostGmres::kMaxRestart, 1.0, 1.0, false);
  run_case("full cycle of 64, zero at the end", HostGmres::kMaxRestart, 4.0, 0.3, true);
  {   // a second cycle on the same object starts clean
    HostGmres ls;
    double col[3] = {1.0, 1.0, 0.0};
    ls.start(1.0);
    ls.push(col);
    ls.start(5.0);
    EXPECT(ls.size() == 0, "restart keeps columns");
    double c2[2] = {3.0, 4.0};
    const double res = ls.push(c2);   // min |5 e1 - (3, 4)' y|: y = 15 / 25, residual 5 * 4 / 5 = 4
    double y[1];
    ls.solve(y);
    EXPECT(std::fabs(res - 4.0) <= 1e-14 && std::fabs(y[0] - 0.6) <= 1e-15, "3-4-5 column: res %g y %g", res, y[0]);
  }
  if (g_fail) {
    std::printf("host_gmres FAILED: %d\n", g_fail);
    return 1;
  }
  std::printf("host_gmres OK\n");
  return 0;
}
