// HostGmres: the small dense part of one restart cycle of GMRES, on the host (no HIP: tests/host/test_host_gmres.cpp
// compiles it alone).  The solver (aggmg_fgmres_dev) hands it the Hessenberg matrix a column at a time; it keeps the
// matrix in triangular form by Givens rotations, so that after column j
//   |g_{j+1}| = min_y || beta e_1 - Hbar_j y ||_2        (Hbar_j: the (j + 2) x (j + 1) leading part)
// is known without solving, and y comes from one back-substitution when the cycle ends.  At most kMaxRestart columns:
// 65 x 64 doubles.
#pragma once
#include <cmath>

class HostGmres {
 public:
  static constexpr int kMaxRestart = 64;   // == AGGMG_FGMRES_MAX_RESTART

  // a new cycle: g = beta e_1, no columns
  void start(double beta) {
    k_ = 0;
    g_[0] = beta;
  }
  int size() const { return k_; }

  // column j = size() of the Hessenberg matrix: h[0 .. j] the projections, h[j + 1] the sub-diagonal entry (>= 0 from
  // a norm; 0: the Krylov space is exhausted).  Returns |g_{j+1}|, the residual norm of the least-squares problem with
  // this column in.  The caller adds no more than kMaxRestart columns to a cycle.
  double push(const double* h) {
    const int j = k_;
    double* r = r_[j];
    for (int i = 0; i <= j + 1; ++i) r[i] = h[i];
    for (int i = 0; i < j; ++i) {   // the rotations of the earlier columns
      const double a = r[i], b = r[i + 1];
      r[i] = c_[i] * a + s_[i] * b;
      r[i + 1] = c_[i] * b - s_[i] * a;
    }
    const double a = r[j], b = r[j + 1];
    const double d = std::hypot(a, b);
    if (d == 0.0) {   // a zero column below the rotations: nothing to rotate (the back-substitution will divide by 0)
      c_[j] = 1.0;
      s_[j] = 0.0;
    } else {
      c_[j] = a / d;
      s_[j] = b / d;
    }
    r[j] = d;
    r[j + 1] = 0.0;
    g_[j + 1] = -s_[j] * g_[j];
    g_[j] = c_[j] * g_[j];
    k_ = j + 1;
    return std::fabs(g_[k_]);
  }

  // y[0 .. size() - 1] = argmin || beta e_1 - Hbar y ||: back-substitution on the triangular factor
  void solve(double* y) const {
    for (int i = k_ - 1; i >= 0; --i) {
      double t = g_[i];
      for (int l = i + 1; l < k_; ++l) t -= r_[l][i] * y[l];
      y[i] = t / r_[i][i];
    }
  }

 private:
  int k_ = 0;
  double r_[kMaxRestart][kMaxRestart + 1];   // r_[column][row]: the rotated columns
  double c_[kMaxRestart], s_[kMaxRestart];
  double g_[kMaxRestart + 1];
};
