// Relative pose of every pair from its matches, on the device: five-point RANSAC (utils/metrics.py:79-109 estimate_pose,
// there OpenCV's findEssentialMat + recoverPose on the host, one pair at a time).  Float64 throughout; keypoints and
// intrinsics arrive as float32, as fm_epipolar_errors takes them.
//
//   k_pose_prep  : normalised coordinates q = ((x - cx) / fx, (y - cy) / fy) of every match, each image by its own K;
//                  the pairs' segments of the (sorted) match list by binary search; thr2 = (pixel_thr / f)^2 per pair.
//   k_pose_solve : one hypothesis per thread.  Sample: the first five distinct of eight hashed draws (splitmix64, the
//                  host reproduces it).  Solver: Nister's five-point method -
//                    the 5 x 9 constraint matrix of q1^T E q0 = 0, its null space X, Y, Z, W by Gauss-Jordan elimination,
//                    E = x X + y Y + z Z + W;  det E = 0 and (E E^T - tr(E E^T) / 2 I) E = 0 as ten cubics over 20
//                    monomials, built from polynomial products (1 x 1 -> 2, 2 x 1 -> 3);  Gauss-Jordan with partial
//                    pivoting in the order x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1;
//                    rows (x2z) - z (x2), (y2z) - z (y2), (xyz) - z (xy): a 3 x 3 matrix B(z) of polynomials of degree 3,
//                    3, 4 with B (x, y, 1)^T = 0, whose determinant is the degree-10 polynomial;
//                    its ten complex roots by Durand-Kerner (kPoseDkIters sweeps, no test of convergence); a root with
//                    |Im z| <= 1e-8 max(1, |z|) is real;  two Newton steps on det B(z);  (x, y, 1) from the cross product
//                    of two rows of B(z);  three Gauss-Newton steps of (x, y, z) on the ten constraints themselves, which
//                    frees a candidate from the conditioning of the eliminations;  a candidate is kept where
//                    || 2 E E^T E - tr(E E^T) E ||_F <= 1e-10 at || E ||_F = 1, in order of ascending z.
//                  A zero pivot, a non-finite value, no real root: the hypothesis has no candidate.  Each thread's 10 x 20
//                  matrix lives in LDS (element e of thread t at e * 64 + t: no bank conflict, row swaps index LDS and
//                  nothing indexed at run time sits in registers); 100 KB per workgroup of 64 threads.
//   k_pose_score : one wave per hypothesis, lanes over the pair's matches: inliers (squared Sampson distance < thr2) of
//                  every candidate, counted with ballots; the pair's winner by ONE 64-bit integer atomicMax on
//                  (count, ~hypothesis, ~slot): the largest count, then the lowest hypothesis, then the lowest slot.
//   k_pose_final : one workgroup per pair: the winner's inlier flags, the four decompositions (Ra, t), (Ra, -t), (Rb, t),
//                  (Rb, -t) by Horn's closed form, each counted by the inliers whose least-squares depths on both rays
//                  are positive; the first of the largest count wins.
// Every loop has a trip count fixed at compile time or by the arguments; the only atomics are integer.  The same inputs
// give the same bits whatever the scheduling.
#include "fm_debug.h"
#include "fm_internal.h"

#define FM_HD __host__ __device__ __forceinline__

namespace fm {

constexpr int kPoseCand = 10;               // candidates of a hypothesis (the degree of the polynomial)
constexpr int kPoseDraws = 8;               // hashed draws of a sample
constexpr int kPoseMaxSamples = 65536;      // hypotheses of a pair (16 bits of the winner's word)
constexpr int kPoseDkIters = 64;            // Durand-Kerner sweeps
constexpr int kPosePolish = 2;              // Newton steps on det B(z)
constexpr int kPoseRefine = 3;              // Gauss-Newton steps on the ten constraints
constexpr double kPoseGate = 1e-10;         // largest || 2 E E^T E - tr(E E^T) E ||_F of a candidate
constexpr double kPoseRealTol = 1e-8;
constexpr int kPoseMat = 200;               // doubles of a thread's 10 x 20 matrix
constexpr int kPoseSolveLds = 64 * kPoseMat * 8;
constexpr int kPoseMaxGrid = 1 << 20;
static_assert(kPoseSolveLds <= 160 * 1024, "one workgroup per CU");

// ---- monomials: key = 16 ex + 4 ey + ez (keys of a product add) ------------------------------------------------------
FM_HD constexpr int pose_key1(int i) { return i == 0 ? 16 : i == 1 ? 4 : i == 2 ? 1 : 0; }            // x y z 1
FM_HD constexpr int pose_mono2(int key) {                                  // x2 y2 z2 xy xz yz x y z 1
  switch (key) {
    case 32: return 0; case 8: return 1; case 2: return 2; case 20: return 3; case 17: return 4;
    case 5: return 5; case 16: return 6; case 4: return 7; case 1: return 8; default: return 9;
  }
}
FM_HD constexpr int pose_key2(int d) {
  constexpr int k[10] = {32, 8, 2, 20, 17, 5, 16, 4, 1, 0};
  return k[d];
}
FM_HD constexpr int pose_mono3(int key) {      // x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1
  switch (key) {
    case 48: return 0; case 12: return 1; case 36: return 2; case 24: return 3; case 33: return 4;
    case 32: return 5; case 9: return 6; case 8: return 7; case 21: return 8; case 20: return 9;
    case 18: return 10; case 17: return 11; case 16: return 12; case 6: return 13; case 5: return 14;
    case 4: return 15; case 3: return 16; case 2: return 17; case 1: return 18; default: return 19;
  }
}
// o += s a b: degree 1 x 1 -> 2, degree 2 x 1 -> 3
FM_HD void pose_mul11(double (&o)[10], const double (&a)[4], const double (&b)[4], double s = 1.0) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) o[pose_mono2(pose_key1(i) + pose_key1(j))] += s * a[i] * b[j];
}
FM_HD void pose_mul21(double (&o)[20], const double (&a)[10], const double (&b)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) o[pose_mono3(pose_key2(i) + pose_key1(j))] += a[i] * b[j];
}

// a thread's 10 x 20 matrix: element (r, c) at p[(20 r + c) stride]
struct PoseMat {
  double* p; int stride;
  FM_HD double& operator()(int r, int c) const { return p[(r * 20 + c) * stride]; }
  FM_HD double& at(int e) const { return p[e * stride]; }
};

// Gauss-Jordan with partial pivoting over the first R columns of the R x C matrix; a row above the pivot is brought to
// reduced form only from row KEEP on (the rows before are not read again).  false: a zero or non-finite pivot.
template <int R, int C, int KEEP>
FM_HD bool pose_gauss_jordan(const PoseMat& A) {
  for (int k = 0; k < R; ++k) {
    int p = k;
    double best = __builtin_fabs(A(k, k));
    for (int r = k + 1; r < R; ++r) {
      const double v = __builtin_fabs(A(r, k));
      if (v > best) { best = v; p = r; }
    }
    if (!(best > 0.0) || !__builtin_isfinite(best)) return false;
    if (p != k)
      for (int c = k; c < C; ++c) { const double t = A(k, c); A(k, c) = A(p, c); A(p, c) = t; }
    const double inv = 1.0 / A(k, k);
    for (int c = k; c < C; ++c) A(k, c) *= inv;
    for (int r = 0; r < R; ++r) {
      if (r == k || (r < k && r < KEEP)) continue;
      const double f = A(r, k);
      for (int c = k; c < C; ++c) A(r, c) -= f * A(k, c);
    }
  }
  return true;
}

FM_HD void pose_mm(const double (&a)[9], const double (&b)[9], double (&o)[9]) {          // o = a b
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
FM_HD void pose_mmt(const double (&a)[9], const double (&b)[9], double (&o)[9]) {         // o = a b^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1] + a[3 * i + 2] * b[3 * j + 2];
}
FM_HD void pose_mtm(const double (&a)[9], const double (&b)[9], double (&o)[9]) {         // o = a^T b
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o[3 * i + j] = a[i] * b[j] + a[3 + i] * b[3 + j] + a[6 + i] * b[6 + j];
}
// the cofactor matrix: row i = row (i + 1) x row (i + 2)
FM_HD void pose_cof(const double (&e)[9], double (&c)[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double* u = e + 3 * ((i + 1) % 3);
    const double* v = e + 3 * ((i + 2) % 3);
    c[3 * i] = u[1] * v[2] - u[2] * v[1];
    c[3 * i + 1] = u[2] * v[0] - u[0] * v[2];
    c[3 * i + 2] = u[0] * v[1] - u[1] * v[0];
  }
}
// f[0] = det E, f[1..9] = 2 E E^T E - tr(E E^T) E; also E E^T and its trace
FM_HD void pose_constraints(const double (&E)[9], double (&f)[10], double (&EEt)[9], double& tr) {
  pose_mmt(E, E, EEt);
  tr = EEt[0] + EEt[4] + EEt[8];
  double g[9];
  pose_mm(EEt, E, g);
#pragma unroll
  for (int e = 0; e < 9; ++e) f[1 + e] = 2.0 * g[e] - tr * E[e];
  f[0] = E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6]) + E[2] * (E[3] * E[7] - E[4] * E[6]);
}
FM_HD void pose_combine(const double (&N)[4][9], const double (&v)[3], double (&E)[9]) {
#pragma unroll
  for (int e = 0; e < 9; ++e) E[e] = v[0] * N[0][e] + v[1] * N[1][e] + v[2] * N[2][e] + N[3][e];
}
// one Gauss-Newton step of v = (x, y, z) on the ten constraints of E = x X + y Y + z Z + W
FM_HD void pose_gauss_newton(const double (&N)[4][9], double (&v)[3]) {
  double E[9], f[10], EEt[9], EtE[9], C[9], tr, J[10][3];
  pose_combine(N, v, E);
  pose_constraints(E, f, EEt, tr);
  pose_mtm(E, E, EtE);
  pose_cof(E, C);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double (&D)[9] = N[k];
    double t1[9], t2[9], t3[9], edt[9];
    pose_mm(D, EtE, t1);
    pose_mmt(E, D, edt);
    pose_mm(edt, E, t2);
    pose_mm(EEt, D, t3);
    double ed = 0.0, cd = 0.0;
#pragma unroll
    for (int e = 0; e < 9; ++e) { ed += E[e] * D[e]; cd += C[e] * D[e]; }
    J[0][k] = cd;
#pragma unroll
    for (int e = 0; e < 9; ++e) J[1 + e][k] = 2.0 * (t1[e] + t2[e] + t3[e]) - 2.0 * ed * E[e] - tr * D[e];
  }
  double A[9], g[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 10; ++i) s += J[i][k] * f[i];
    g[k] = -s;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      double a = 0.0;
#pragma unroll
      for (int i = 0; i < 10; ++i) a += J[i][k] * J[i][l];
      A[3 * k + l] = a;
    }
  }
  double Ac[9];
  pose_cof(A, Ac);
  const double det = A[0] * Ac[0] + A[1] * Ac[1] + A[2] * Ac[2];
#pragma unroll
  for (int j = 0; j < 3; ++j) v[j] += (Ac[j] * g[0] + Ac[3 + j] * g[1] + Ac[6 + j] * g[2]) / det;      // A^-1 = cof(A)^T / det
}

// B(z) [row][x y 1][ascending power of z] at z -> its determinant and the determinant's derivative
FM_HD void pose_bdet(const double (&B)[3][3][5], double z, double& f, double& df) {
  double v[3][3], d[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      double p = B[r][g][4], q = 0.0;
#pragma unroll
      for (int k = 3; k >= 0; --k) { q = q * z + p; p = p * z + B[r][g][k]; }
      v[r][g] = p; d[r][g] = q;
    }
  auto det3 = [](const double* a, const double* b, const double* c) {
    return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
  };
  f = det3(v[0], v[1], v[2]);
  df = det3(d[0], v[1], v[2]) + det3(v[0], d[1], v[2]) + det3(v[0], v[1], d[2]);
}

// o[0 .. NA + NB - 2] += s a b (ascending coefficients)
template <int NA, int NB>
FM_HD void pose_polymul(double* o, const double* a, const double* b, double s) {
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) o[i + j] += s * a[i] * b[j];
}

// The solver on one sample: q0[p], q1[p] = (x, y) of the five points -> the number of candidates; E_out [10][9], unit
// Frobenius norm, in order of ascending z.  A: the thread's matrix (kPoseMat doubles), scratch throughout.
FM_HD int pose_solve(const double (&q0)[5][2], const double (&q1)[5][2], const PoseMat& A, double* __restrict__ E_out) {
  // the 5 x 9 constraint matrix and its null space
#pragma unroll
  for (int p = 0; p < 5; ++p) {
    const double x0 = q0[p][0], y0 = q0[p][1], x1 = q1[p][0], y1 = q1[p][1];
    A(p, 0) = x1 * x0; A(p, 1) = x1 * y0; A(p, 2) = x1;
    A(p, 3) = y1 * x0; A(p, 4) = y1 * y0; A(p, 5) = y1;
    A(p, 6) = x0; A(p, 7) = y0; A(p, 8) = 1.0;
  }
  if (!pose_gauss_jordan<5, 9, 0>(A)) return 0;
  double N[4][9];                                   // X Y Z W, row-major E
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < 9; ++c) N[k][c] = c < 5 ? -A(c, 5 + k) : (c - 5 == k ? 1.0 : 0.0);
  {
    // entry (i, j) of E as a polynomial over (x, y, z, 1)
    double P[3][3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) P[i][j][k] = N[k][3 * i + j];
    // det E
    {
      double row[20];
#pragma unroll
      for (int c = 0; c < 20; ++c) row[c] = 0.0;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        double cf[10];
#pragma unroll
        for (int c = 0; c < 10; ++c) cf[c] = 0.0;
        pose_mul11(cf, P[1][j1], P[2][j2]);
        pose_mul11(cf, P[1][j2], P[2][j1], -1.0);
        pose_mul21(row, cf, P[0][j]);
      }
#pragma unroll
      for (int c = 0; c < 20; ++c) A(0, c) = row[c];
    }
    // L = E E^T - tr(E E^T) / 2 I, then L E
    double L[3][3][10];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j) {
#pragma unroll
        for (int c = 0; c < 10; ++c) L[i][j][c] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) pose_mul11(L[i][j], P[i][k], P[j][k]);
      }
#pragma unroll
    for (int c = 0; c < 10; ++c) {
      const double h = 0.5 * (L[0][0][c] + L[1][1][c] + L[2][2][c]);
      L[0][0][c] -= h; L[1][1][c] -= h; L[2][2][c] -= h;
      L[1][0][c] = L[0][1][c]; L[2][0][c] = L[0][2][c]; L[2][1][c] = L[1][2][c];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double row[20];
#pragma unroll
        for (int c = 0; c < 20; ++c) row[c] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) pose_mul21(row, L[i][k], P[k][j]);
#pragma unroll
        for (int c = 0; c < 20; ++c) A(1 + 3 * i + j, c) = row[c];
      }
  }
  if (!pose_gauss_jordan<10, 20, 4>(A)) return 0;
  // B(z): rows (x2z) - z (x2), (y2z) - z (y2), (xyz) - z (xy); columns: what multiplies x, y, 1
  double B[3][3][5];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const int n = g == 2 ? 4 : 3, c0 = 10 + 3 * g;          // the group's columns hold z^(n-1) .. z^0
#pragma unroll
      for (int k = 0; k < 5; ++k) B[r][g][k] = 0.0;
#pragma unroll
      for (int k = 0; k < n; ++k) {
        B[r][g][k] += A(4 + 2 * r, c0 + n - 1 - k);
        B[r][g][k + 1] -= A(5 + 2 * r, c0 + n - 1 - k);
      }
    }
  double det[11];
#pragma unroll
  for (int k = 0; k < 11; ++k) det[k] = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {                      // expansion along the column of 1: rows r1 < r2 are the others
    const int r1 = r == 0 ? 1 : 0, r2 = r == 2 ? 1 : 2;
    double m[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) m[k] = 0.0;
    pose_polymul<4, 4>(m, B[r1][0], B[r2][1], 1.0);
    pose_polymul<4, 4>(m, B[r1][1], B[r2][0], -1.0);
    pose_polymul<7, 5>(det, m, B[r][2], r == 1 ? -1.0 : 1.0);
  }
  double finite = 0.0;
#pragma unroll
  for (int k = 0; k < 11; ++k) finite += det[k] * 0.0;       // 0, or NaN where a coefficient is not finite
  if (!(finite == 0.0) || det[10] == 0.0) return 0;
  double c[10];
  {
    const double inv = 1.0 / det[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) c[k] = det[k] * inv;
  }
  // Durand-Kerner from ten points on a circle of the roots' scale
  double radius = 0.0;
#pragma unroll
  for (int k = 1; k <= 10; ++k) {
    const double v = pow(__builtin_fabs(c[10 - k]), 1.0 / k);
    radius = v > radius ? v : radius;
  }
  if (!__builtin_isfinite(radius)) return 0;
  // cos and sin of 2 pi k / 10 + 0.7
  const double ux[10] = {0.76484218728448850, 0.24010006119398122, -0.37635177945048860, -0.84904923320513690,
                         -0.99743805680154880, -0.76484218728448850, -0.24010006119398122, 0.37635177945048860,
                         0.84904923320513690, 0.99743805680154880};
  const double uy[10] = {0.64421768723769100, 0.97074817359100720, 0.92648582974545600, 0.52832079414908260,
                         -0.07164524509898605, -0.64421768723769100, -0.97074817359100720, -0.92648582974545600,
                         -0.52832079414908260, 0.07164524509898605};
  double zr[10], zi[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) { zr[i] = radius * ux[i]; zi[i] = radius * uy[i]; }
#pragma unroll 1
  for (int it = 0; it < kPoseDkIters; ++it) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      double pr = 1.0, pi = 0.0;
#pragma unroll
      for (int k = 9; k >= 0; --k) {
        const double t = pr * zr[i] - pi * zi[i] + c[k];
        pi = pr * zi[i] + pi * zr[i];
        pr = t;
      }
      double qr = 1.0, qi = 0.0;
#pragma unroll
      for (int j = 0; j < 10; ++j) {
        if (j == i) continue;
        const double dr = zr[i] - zr[j], di = zi[i] - zi[j];
        const double t = qr * dr - qi * di;
        qi = qr * di + qi * dr;
        qr = t;
      }
      const double s = 1.0 / (qr * qr + qi * qi);
      zr[i] -= (pr * qr + pi * qi) * s;
      zi[i] -= (pi * qr - pr * qi) * s;
    }
  }
  // the matrix is free from here on: [0, 10) real parts, [10, 20) imaginary parts, [20, 30) a candidate's z (+inf: none),
  // [30, 120) the candidates
#pragma unroll
  for (int i = 0; i < 10; ++i) { A.at(i) = zr[i]; A.at(10 + i) = zi[i]; }
  int count = 0;
#pragma unroll 1
  for (int i = 0; i < 10; ++i) {
    const double re = A.at(i), im = A.at(10 + i);
    const double mag = __builtin_sqrt(re * re + im * im);
    A.at(20 + i) = __builtin_inf();
    if (!(__builtin_fabs(im) <= kPoseRealTol * (mag > 1.0 ? mag : 1.0))) continue;
    double z = re;
#pragma unroll 1
    for (int s = 0; s < kPosePolish; ++s) {
      double f, df;
      pose_bdet(B, z, f, df);
      z -= f / df;
    }
    double bz[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        double p = B[r][g][4];
#pragma unroll
        for (int k = 3; k >= 0; --k) p = p * z + B[r][g][k];
        bz[r][g] = p;
      }
    // (x, y, 1) ~ the cross product of two rows: the pair (0,1), (0,2), (1,2) whose third component is largest
    double cx = 0.0, cy = 0.0, cz = 0.0;
#pragma unroll
    for (int pair = 0; pair < 3; ++pair) {
      const double* u = bz[pair == 2 ? 1 : 0];
      const double* w = bz[pair == 0 ? 1 : 2];
      const double x = u[1] * w[2] - u[2] * w[1], y = u[2] * w[0] - u[0] * w[2], zc = u[0] * w[1] - u[1] * w[0];
      if (pair == 0 || __builtin_fabs(zc) > __builtin_fabs(cz)) { cx = x; cy = y; cz = zc; }
    }
    double v[3] = {cx / cz, cy / cz, z};
#pragma unroll 1
    for (int s = 0; s < kPoseRefine; ++s) pose_gauss_newton(N, v);
    double E[9], f[10], EEt[9], tr;
    pose_combine(N, v, E);
    double n2 = 0.0;
#pragma unroll
    for (int e = 0; e < 9; ++e) n2 += E[e] * E[e];
    const double inv = 1.0 / __builtin_sqrt(n2);
#pragma unroll
    for (int e = 0; e < 9; ++e) E[e] *= inv;
    pose_constraints(E, f, EEt, tr);
    double res = 0.0;
#pragma unroll
    for (int e = 0; e < 9; ++e) res += f[1 + e] * f[1 + e];
    if (!(__builtin_sqrt(res) <= kPoseGate) || !__builtin_isfinite(v[2])) continue;       // (NaN fails the comparison)
    A.at(20 + i) = v[2];
#pragma unroll
    for (int e = 0; e < 9; ++e) A.at(30 + 9 * i + e) = E[e];
    ++count;
  }
  // in order of ascending z (equal z: in order of the root's index)
#pragma unroll 1
  for (int i = 0; i < 10; ++i) {
    const double z = A.at(20 + i);
    if (!(z < __builtin_inf())) continue;
    int rank = 0;
    for (int j = 0; j < 10; ++j) {
      const double w = A.at(20 + j);
      rank += (w < z || (w == z && j < i)) ? 1 : 0;
    }
    for (int e = 0; e < 9; ++e) E_out[9 * rank + e] = A.at(30 + 9 * i + e);
  }
  return count;
}

// ---- sampling ---------------------------------------------------------------------------------------------------------
constexpr uint64_t kGold = 0x9E3779B97F4A7C15ull, kMix1 = 0xBF58476D1CE4E5B9ull, kMix2 = 0x94D049BB133111EBull;
FM_HD uint64_t pose_splitmix64(uint64_t x) {
  uint64_t z = x + kGold;
  z = (z ^ (z >> 30)) * kMix1;
  z = (z ^ (z >> 27)) * kMix2;
  return z ^ (z >> 31);
}
FM_HD uint64_t pose_stream_key(uint64_t seed, uint64_t stream) {
  return pose_splitmix64(pose_splitmix64(seed) + stream * kMix1);
}
// the first five distinct of the eight draws of hypothesis h among m matches; false: fewer than five
FM_HD bool pose_sample(uint64_t key, int h, int m, int (&idx)[5]) {
  if (m < 5) return false;
  int got = 0;
#pragma unroll
  for (int k = 0; k < kPoseDraws; ++k) {
    const int d = (int)(pose_splitmix64((uint64_t)(8 * (int64_t)h + k) * kGold + key) % (uint64_t)m);
    bool fresh = got < 5;
#pragma unroll
    for (int j = 0; j < 5; ++j) fresh = fresh && !(j < got && idx[j] == d);
#pragma unroll
    for (int j = 0; j < 5; ++j)
      if (fresh && j == got) idx[j] = d;
    got += fresh ? 1 : 0;
  }
  return got == 5;
}

// squared Sampson distance of the match (x0, y0) <-> (x1, y1) to E
FM_HD double pose_sampson(const double (&E)[9], double x0, double y0, double x1, double y1) {
  const double a = E[0] * x0 + E[1] * y0 + E[2];
  const double b = E[3] * x0 + E[4] * y0 + E[5];
  const double c = E[6] * x0 + E[7] * y0 + E[8];
  const double f0 = E[0] * x1 + E[3] * y1 + E[6];
  const double f1 = E[1] * x1 + E[4] * y1 + E[7];
  const double num = x1 * a + y1 * b + c;
  return num * num / (a * a + b * b + f0 * f0 + f1 * f1);
}

// Workspace: seg [N + 1] first match of every pair | best [N] the winners' words | thr2 [N] | q [m_max][4] normalised
// (x0, y0, x1, y1) | ncand [N samples] | cand [N samples][10][9]
struct PoseWs {
  Region<int> seg; Region<unsigned long long> best; Region<double> thr2, q; Region<int> ncand; Region<double> cand;
  size_t total;
};
static PoseWs pose_layout(int N, int m_max, int samples) {
  PoseWs w;
  Carver c;
  const size_t H = (size_t)N * samples;
  c.take(w.seg, (size_t)N + 1);
  c.take(w.best, N);
  c.take(w.thr2, N);
  c.take(w.q, (size_t)m_max * 4);
  c.take(w.ncand, H);
  c.take(w.cand, H * kPoseCand * 9);
  w.total = c.pad();
  return w;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pose_prep(const float* __restrict__ k0, const float* __restrict__ k1, int kstride,
                                                   const int64_t* __restrict__ m_bids, const int32_t* __restrict__ d_count,
                                                   int m_max, int N, const float* __restrict__ K0, const float* __restrict__ K1,
                                                   double pixel_thr, int* __restrict__ seg, unsigned long long* __restrict__ best,
                                                   double* __restrict__ thr2, double* __restrict__ q,
                                                   unsigned char* __restrict__ inlier) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int M = d_count ? max(0, min(d_count[0], m_max)) : m_max;
  if (i < m_max) {
    inlier[i] = 0;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (i < M) {
      const int64_t b = m_bids[i];
      if (b >= 0 && b < N) {
        const float* a = K0 + b * 9;
        const float* c = K1 + b * 9;
        v[0] = ((double)k0[i * kstride] - (double)a[2]) / (double)a[0];
        v[1] = ((double)k0[i * kstride + 1] - (double)a[5]) / (double)a[4];
        v[2] = ((double)k1[i * kstride] - (double)c[2]) / (double)c[0];
        v[3] = ((double)k1[i * kstride + 1] - (double)c[5]) / (double)c[4];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) q[i * 4 + e] = v[e];
  }
  if (i <= N) {
    int lo = 0, hi = M;                              // the first row whose id is >= i (m_bids is non-decreasing)
    for (int s = 0; s < 32; ++s) {
      if (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (m_bids[mid] < i) lo = mid + 1; else hi = mid;
      }
    }
    seg[i] = lo;
    if (i < N) {
      best[i] = 0ull;
      const double f = ((double)K0[i * 9] + (double)K0[i * 9 + 4] + (double)K1[i * 9] + (double)K1[i * 9 + 4]) / 4.0;
      const double r = pixel_thr / f;
      thr2[i] = r * r;
    }
  }
}

// GIVEN: the samples are the caller's (fm_debug_pose_solve: q0g, q1g [S][5][2], N = 1, samples = S)
template <bool GIVEN>
__global__ __launch_bounds__(64) void k_pose_solve(const int* __restrict__ seg, const double* __restrict__ q, int N, int samples,
                                                   uint64_t seed, const double* __restrict__ q0g, const double* __restrict__ q1g,
                                                   double* __restrict__ cand, int* __restrict__ ncand) {
  extern __shared__ __attribute__((aligned(16))) double pose_lds[];
  const PoseMat A = {pose_lds + threadIdx.x, 64};
  const int chunks = (samples + 63) / 64;
  const long items = (long)N * chunks;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const int b = (int)(item / chunks);
    const int h = (int)(item - (long)b * chunks) * 64 + (int)threadIdx.x;
    if (h >= samples) continue;
    const size_t g = (size_t)b * samples + h;
    double s0[5][2], s1[5][2];
    bool live = true;
    if (GIVEN) {
#pragma unroll
      for (int p = 0; p < 5; ++p) {
        s0[p][0] = q0g[g * 10 + 2 * p]; s0[p][1] = q0g[g * 10 + 2 * p + 1];
        s1[p][0] = q1g[g * 10 + 2 * p]; s1[p][1] = q1g[g * 10 + 2 * p + 1];
      }
    } else {
      const int first = seg[b], m = seg[b + 1] - first;
      int idx[5] = {0, 0, 0, 0, 0};
      live = pose_sample(pose_stream_key(seed, (uint64_t)b), h, m, idx);
#pragma unroll
      for (int p = 0; p < 5; ++p) {
        const double* r = q + (size_t)(first + (live ? idx[p] : 0)) * 4;
        s0[p][0] = live ? r[0] : 0.0; s0[p][1] = live ? r[1] : 0.0;
        s1[p][0] = live ? r[2] : 0.0; s1[p][1] = live ? r[3] : 0.0;
      }
    }
    ncand[g] = live ? pose_solve(s0, s1, A, cand + g * (kPoseCand * 9)) : 0;
  }
}

FM_HD unsigned long long pose_word(int count, int h, int slot) {
  return ((unsigned long long)(unsigned)count << 32) | ((unsigned long long)(kPoseMaxSamples - 1 - h) << 4) |
         (unsigned long long)(15 - slot);
}

__global__ __launch_bounds__(256) void k_pose_score(const int* __restrict__ seg, const double* __restrict__ q,
                                                    const double* __restrict__ thr2, int N, int samples,
                                                    const double* __restrict__ cand, const int* __restrict__ ncand,
                                                    unsigned long long* __restrict__ best) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long items = (long)N * samples;
  for (long g = (long)blockIdx.x * 4 + wave; g < items; g += (long)gridDim.x * 4) {
    const int nc = ncand[g];
    if (nc <= 0) continue;
    const int b = (int)(g / samples), h = (int)(g - (long)b * samples);
    const int first = seg[b], m = seg[b + 1] - first;
    const double t2 = thr2[b];
    unsigned long long word = 0ull;
    for (int s = 0; s < nc; ++s) {
      double E[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) E[e] = cand[(size_t)g * (kPoseCand * 9) + 9 * s + e];
      int count = 0;
      for (int i0 = 0; i0 < m; i0 += 64) {
        const int i = i0 + lane;
        bool in = false;
        if (i < m) {
          const double* r = q + (size_t)(first + i) * 4;
          in = pose_sampson(E, r[0], r[1], r[2], r[3]) < t2;
        }
        count += __popcll(__ballot(in));
      }
      const unsigned long long w = pose_word(count, h, s);
      word = w > word ? w : word;
    }
    if (lane == 0) atomicMax(&best[b], word);
  }
}

// least-squares depths l0, l1 of l1 q1 = l0 R q0 + t, both positive
FM_HD bool pose_in_front(const double (&R)[9], const double (&t)[3], double x0, double y0, double x1, double y1) {
  const double a0 = R[0] * x0 + R[1] * y0 + R[2], a1 = R[3] * x0 + R[4] * y0 + R[5], a2 = R[6] * x0 + R[7] * y0 + R[8];
  const double aa = a0 * a0 + a1 * a1 + a2 * a2, bb = x1 * x1 + y1 * y1 + 1.0, ab = a0 * x1 + a1 * y1 + a2;
  const double at = a0 * t[0] + a1 * t[1] + a2 * t[2], bt = x1 * t[0] + y1 * t[1] + t[2];
  const double det = aa * bb - ab * ab;
  return det > 0.0 && ab * bt - bb * at > 0.0 && aa * bt - ab * at > 0.0;
}

// E (unit norm) -> Ra, Rb and t (unit length) of its decompositions (Ra, t), (Ra, -t), (Rb, t), (Rb, -t): Horn's closed
// form, t t^T = tr(E E^T) / 2 I - E E^T read off its largest diagonal entry (the first of equals), Ra / Rb =
// (cof(E) -/+ [t]x E) / t.t (cof(E) = t t^T R), each taken to the nearest rotation by three steps R <- R (3 I - R^T R) / 2
FM_HD void pose_decompose(const double (&E)[9], double (&Ra)[9], double (&Rb)[9], double (&t)[3]) {
  double EEt[9], C[9];
  pose_mmt(E, E, EEt);
  const double half = 0.5 * (EEt[0] + EEt[4] + EEt[8]);
  double tt[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) tt[e] = (e % 4 == 0 ? half : 0.0) - EEt[e];
  int i = 0;
  double top = tt[0];
  if (tt[4] > top) { i = 1; top = tt[4]; }
  if (tt[8] > top) { i = 2; top = tt[8]; }
  const double inv = 1.0 / __builtin_sqrt(top);
#pragma unroll
  for (int e = 0; e < 3; ++e) t[e] = (i == 0 ? tt[e] : i == 1 ? tt[3 + e] : tt[6 + e]) * inv;
  pose_cof(E, C);
  const double tx[9] = {0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0};
  double txE[9];
  pose_mm(tx, E, txE);
  const double n2 = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Ra[3 * r + c] = (C[3 * r + c] - txE[3 * r + c]) / n2;
      Rb[3 * r + c] = (C[3 * r + c] + txE[3 * r + c]) / n2;
    }
#pragma unroll 1
  for (int s = 0; s < 3; ++s) {
    double g[9], o[9];
    pose_mtm(Ra, Ra, g);
#pragma unroll
    for (int e = 0; e < 9; ++e) g[e] = (e % 4 == 0 ? 1.5 : 0.0) - 0.5 * g[e];
    pose_mm(Ra, g, o);
#pragma unroll
    for (int e = 0; e < 9; ++e) Ra[e] = o[e];
    pose_mtm(Rb, Rb, g);
#pragma unroll
    for (int e = 0; e < 9; ++e) g[e] = (e % 4 == 0 ? 1.5 : 0.0) - 0.5 * g[e];
    pose_mm(Rb, g, o);
#pragma unroll
    for (int e = 0; e < 9; ++e) Rb[e] = o[e];
  }
  const double tn = 1.0 / __builtin_sqrt(n2);
#pragma unroll
  for (int e = 0; e < 3; ++e) t[e] *= tn;
}

__global__ __launch_bounds__(256) void k_pose_final(const int* __restrict__ seg, const double* __restrict__ q,
                                                    const double* __restrict__ thr2, int N, int samples,
                                                    const double* __restrict__ cand, const unsigned long long* __restrict__ best,
                                                    double* __restrict__ R_out, double* __restrict__ t_out,
                                                    double* __restrict__ E_out, unsigned char* __restrict__ inlier,
                                                    int32_t* __restrict__ per_pair) {
  __shared__ int votes[5];                           // the four decompositions, the inliers
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < 5) votes[tid] = 0;
  __syncthreads();
  const int first = seg[b], m = seg[b + 1] - first;
  const unsigned long long word = best[b];
  const bool valid = m >= 5 && word != 0ull;
  double E[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Ra[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Rb[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1},
         t[3] = {0, 0, 0};
  if (valid) {
    const int h = kPoseMaxSamples - 1 - (int)((word >> 4) & 0xFFFF), slot = 15 - (int)(word & 15);
    const double* src = cand + ((size_t)b * samples + h) * (kPoseCand * 9) + 9 * slot;
#pragma unroll
    for (int e = 0; e < 9; ++e) E[e] = src[e];
    pose_decompose(E, Ra, Rb, t);
    const double tm[3] = {-t[0], -t[1], -t[2]};
    const double t2 = thr2[b];
    int n[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < m; i += 256) {
      const double* r = q + (size_t)(first + i) * 4;
      const bool in = pose_sampson(E, r[0], r[1], r[2], r[3]) < t2;
      inlier[first + i] = in ? 1 : 0;
      if (in) {
        n[4] += 1;
        n[0] += pose_in_front(Ra, t, r[0], r[1], r[2], r[3]) ? 1 : 0;
        n[1] += pose_in_front(Ra, tm, r[0], r[1], r[2], r[3]) ? 1 : 0;
        n[2] += pose_in_front(Rb, t, r[0], r[1], r[2], r[3]) ? 1 : 0;
        n[3] += pose_in_front(Rb, tm, r[0], r[1], r[2], r[3]) ? 1 : 0;
      }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (n[k]) atomicAdd(&votes[k], n[k]);
  }
  __syncthreads();
  if (tid != 0) return;
  int pick = 0;
  for (int k = 1; k < 4; ++k)
    if (votes[k] > votes[pick]) pick = k;
  const bool ok = valid && votes[pick] > 0;
  const double sign = (pick & 1) ? -1.0 : 1.0;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    R_out[(size_t)b * 9 + e] = ok ? (pick < 2 ? Ra[e] : Rb[e]) : (e % 4 == 0 ? 1.0 : 0.0);
    E_out[(size_t)b * 9 + e] = E[e];
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) t_out[(size_t)b * 3 + e] = ok ? sign * t[e] : 0.0;
  per_pair[b * 4] = m;
  per_pair[b * 4 + 1] = votes[4];
  per_pair[b * 4 + 2] = votes[pick];
  per_pair[b * 4 + 3] = ok ? 1 : 0;
}

// ---- host -----------------------------------------------------------------------------------------------------------------
static bool pose_sizes_ok(int N, int m_max, int samples) { return N > 0 && m_max >= 0 && samples > 0; }
static bool pose_route(int m_max, int samples) { return samples <= kPoseMaxSamples && (long)m_max < (1L << 31) / 8; }

struct PoseCall {
  const float *mkpts0, *mkpts1; int kpt_stride; const int64_t* m_bids; const int32_t* d_count; int m_max, N;
  const float *K0, *K1; float pixel_thr; int samples; uint64_t seed; void* workspace; size_t workspace_bytes;
  double *R_out, *t_out, *E_out; unsigned char* inlier; int32_t* per_pair; void* stream;
};

// the ONLY copy of fm_estimate_pose's argument checks, in the header's order
static int pose_status(const PoseCall& c) {
  if (!c.mkpts0 || !c.mkpts1 || !c.m_bids || !c.K0 || !c.K1 || !c.R_out || !c.t_out || !c.E_out || !c.inlier || !c.per_pair)
    return FM_E_NULL;
  if (!pose_sizes_ok(c.N, c.m_max, c.samples) || c.kpt_stride < 2) return FM_E_SHAPE;
  if (!(c.pixel_thr > 0.0f) || !__builtin_isfinite(c.pixel_thr) || !pose_route(c.m_max, c.samples)) return FM_E_UNSUPPORTED;
  if (!c.workspace || !workspace_ok(c.workspace, c.workspace_bytes, pose_layout(c.N, c.m_max, c.samples).total))
    return FM_E_WORKSPACE;
  return FM_OK;
}

static int pose_grid(long items) { return (int)(items < kPoseMaxGrid ? items : kPoseMaxGrid); }

template <bool GIVEN>
static hipError_t pose_launch_solve(const int* seg, const double* q, int N, int samples, uint64_t seed, const double* q0g,
                                    const double* q1g, double* cand, int* ncand, hipStream_t st) {
  static unsigned long long lds_set = 0;
  const hipError_t e = ensure_dynamic_lds(k_pose_solve<GIVEN>, kPoseSolveLds, &lds_set);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_pose_solve<GIVEN>, dim3(pose_grid((long)N * ((samples + 63) / 64))), dim3(64), kPoseSolveLds, st, seg, q,
                     N, samples, seed, q0g, q1g, cand, ncand);
  return hipGetLastError();
}

}  // namespace fm

using namespace fm;

extern "C" size_t fm_pose_workspace_bytes(int N, int m_max, int samples) {
  if (!pose_sizes_ok(N, m_max, samples) || !pose_route(m_max, samples)) return 0;
  return pose_layout(N, m_max, samples).total;
}

extern "C" int fm_estimate_pose(const float* mkpts0, const float* mkpts1, int kpt_stride, const int64_t* m_bids,
                                const int32_t* d_count, int m_max, int N, const float* K0, const float* K1, float pixel_thr,
                                int samples, uint64_t seed, void* workspace, size_t workspace_bytes, double* R_out,
                                double* t_out, double* E_out, unsigned char* inlier, int32_t* per_pair, void* stream) {
  const PoseCall c = {mkpts0, mkpts1, kpt_stride, m_bids, d_count, m_max, N, K0, K1, pixel_thr, samples, seed, workspace,
                      workspace_bytes, R_out, t_out, E_out, inlier, per_pair, stream};
  const int status = pose_status(c);
  if (status != FM_OK || m_max == 0) return status;
  const PoseWs w = pose_layout(N, m_max, samples);
  hipStream_t st = (hipStream_t)stream;
  int* seg = w.seg.in(workspace);
  unsigned long long* best = w.best.in(workspace);
  double* thr2 = w.thr2.in(workspace);
  double* q = w.q.in(workspace);
  int* ncand = w.ncand.in(workspace);
  double* cand = w.cand.in(workspace);
  const long prep = (long)m_max > (long)N + 1 ? (long)m_max : (long)N + 1;
  hipLaunchKernelGGL(k_pose_prep, dim3((unsigned)((prep + 255) / 256)), dim3(256), 0, st, mkpts0, mkpts1, kpt_stride, m_bids,
                     d_count, m_max, N, K0, K1, (double)pixel_thr, seg, best, thr2, q, inlier);
  const hipError_t e = pose_launch_solve<false>(seg, q, N, samples, seed, nullptr, nullptr, cand, ncand, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_pose_score, dim3(pose_grid(((long)N * samples + 3) / 4)), dim3(256), 0, st, (const int*)seg,
                     (const double*)q, (const double*)thr2, N, samples, (const double*)cand, (const int*)ncand, best);
  hipLaunchKernelGGL(k_pose_final, dim3(N), dim3(256), 0, st, (const int*)seg, (const double*)q, (const double*)thr2, N, samples,
                     (const double*)cand, (const unsigned long long*)best, R_out, t_out, E_out, inlier, per_pair);
  return (int)hipGetLastError();
}

extern "C" int fm_debug_pose_solve(const double* q0, const double* q1, int S, double* E_out, int32_t* count_out, void* stream) {
  if (!q0 || !q1 || !E_out || !count_out) return FM_E_NULL;
  if (S <= 0) return FM_E_SHAPE;
  return (int)pose_launch_solve<true>(nullptr, nullptr, 1, S, 0, q0, q1, E_out, count_out, (hipStream_t)stream);
}
