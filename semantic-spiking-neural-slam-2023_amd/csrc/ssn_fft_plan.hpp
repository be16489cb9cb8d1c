// ssn_fft_plan.hpp - the host-side plan of the LDS transforms: which route a length takes, its tables, its launch geometry.
// One definition for k_dft (Sim::plan_dft, launch_dft) and the binder (ssn_bind.hip).  Plain C++17, no HIP, nothing of the simulator:
// csrc/fft_plan_dump.cpp prints it on a CPU (tests/test_fft_plan.py).  `cfloat` has the layout of float2 (asserted where uploaded).
// One workgroup transforms a length d with everything in LDS:
//   * smooth d (prime factors <= 32): mixed-radix Stockham passes (dft_stockham), one pass and one workgroup barrier per radix;
//   * any other d (97, 1801, 2049 = 3 * 683): Bluestein's chirp-z form, a circular convolution of smooth length M >= 2d - 1 - in
//     place on one array when every pass of M is an in-register one (2, 4, 8; dft_bluestein_inplace), else out of place;
//   * on request the four-step transform on the matrix cores (dft4_fft): L = N1 * N2, two dense DFTs around a twiddle product.
// No route (the caller keeps the matrix, or refuses) when nothing fits MAX_POINTS.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

namespace ssn {
namespace fft {
struct cfloat { float x, y; };
constexpr int MAX_POINTS = 6400;                                    // points of the longest transform (32-bit index products: p j fn < L * 32)
constexpr int MAX_RADICES = 12;                                     // DftArgs::radix, BindArgs::radix
constexpr size_t STOCKHAM_POINT_BYTES = 3 * sizeof(cfloat);         // two arrays of L complex points and the twiddle table
constexpr size_t FOUR_STEP_POINT_BYTES = 4 * sizeof(float);         // planar re / im, in and out
constexpr int MAX_LDS_BYTES = MAX_POINTS * (int)STOCKHAM_POINT_BYTES;      // 153.6 KB: what the kernels are allowed once (set_max_dynamic_lds_once)
constexpr double PI = 3.14159265358979323846;

inline bool in_register(int r) { return r == 8 || r == 4 || r == 2; }      // dft_pass_small / dft_pass_inplace
// radices (<= 32 each) of a smooth length, largest first; empty when L has a prime factor > 32
inline std::vector<int> smooth_radices(int L) {
  std::vector<int> primes;
  int rest = L, twos = 0;
  while (rest % 2 == 0) { ++twos; rest /= 2; }
  for (int p = 3; p <= 32 && rest > 1; ++p)
    while (rest % p == 0) { primes.push_back(p); rest /= p; }
  if (rest != 1) return {};
  std::vector<int> rad;
  // factors of two run as in-register butterflies: eights, with a remainder of 2^1 as one radix-2 pass and of 2^4 as two fours
  while (twos >= 3 && twos != 4) { rad.push_back(8); twos -= 3; }
  while (twos >= 2) { rad.push_back(4); twos -= 2; }
  if (twos) rad.push_back(2);
  for (size_t i = 0; i < primes.size();) {           // greedy merge of ascending odd primes while the product stays <= 16
    int r = primes[i++];
    while (i < primes.size() && r * primes[i] <= 16) r *= primes[i++];
    rad.push_back(r);
  }
  std::sort(rad.rbegin(), rad.rend());
  return rad;
}
// relative cost of the passes: a generic radix-r pass does r complex multiply-adds per point out of LDS, an in-register one
// reads and writes each point once; < 0: no passes
inline double stockham_cost(int L) {
  const std::vector<int> rad = smooth_radices(L);
  if (rad.empty() || rad.size() > (size_t)MAX_RADICES) return -1.0;
  double c = 0.0;
  for (int r : rad) c += in_register(r) ? 1.0 : 0.25 * r + 0.5;
  return c * L;
}
// cost of a four-step split in MFMA instructions (16 x 16 x 4, two per k step: real and imaginary rows / columns)
inline long long dft4_cost(int N1, int N2, bool complex_in) {
  const long long P1 = (N1 + 15) / 16, C1 = (N2 + 15) / 16, N1p = (N1 + 3) / 4 * 4, N2p = (N2 + 3) / 4 * 4;
  return P1 * C1 * ((complex_in ? 2 : 1) * N1p / 4) * 2 + P1 * C1 * (2 * N2p / 4) * 2;
}
// best (N1, N2) with N1 * N2 = L, both <= 192 (the step-3 matrix is (2 N2)^2 floats); {0, 0} if L has no such divisor pair
inline std::pair<int, int> dft4_split(int L, bool complex_in) {
  std::pair<int, int> best{0, 0};
  long long bc = -1;
  for (int n1 = 1; n1 <= L; ++n1) {
    if (L % n1) continue;
    const int n2 = L / n1;
    if (n2 > 192 || n1 > 192) continue;
    const long long c = dft4_cost(n1, n2, complex_in);
    if (bc < 0 || c < bc) { bc = c; best = {n1, n2}; }
  }
  return best;
}
// position of frequency k after the in-place decimation-in-frequency passes with radices rad[0], rad[1], ...
inline int dif_position(int k, int M, const std::vector<int>& rad) {
  int pos = 0, len = M;
  for (int r : rad) { len /= r; pos += (k % r) * len; k /= r; }
  return pos;
}

// ---- routes ----
struct Route {
  int d = 0, L = 0;            // length asked for; length of the transforms run (M, or d; 0: no route)
  int M = 0, inplace = 0;      // M > 0: Bluestein's convolution length; inplace: both of its transforms on one array
  int N1 = 0, N2 = 0;          // > 0: the four-step split of L (no radices then)
  std::vector<int> radix;      // the Stockham passes of L
  explicit operator bool() const { return L > 0; }
};
// Stockham passes: a smooth d directly, any other through the cheapest smooth M in [2d - 1, min(MAX_POINTS, 2 (2d - 1))] (a power
// of two where one fits: four radix-8 passes at 4096); in place when every pass of M is an in-register one and the caller allows it
inline Route plan_stockham(int d, bool allow_inplace) {
  Route r;
  if (d < 1 || d > MAX_POINTS) return r;
  std::vector<int> rad = smooth_radices(d);
  int M = 0;
  if (rad.empty()) {
    double best = -1.0;
    for (int c = 2 * d - 1; c <= MAX_POINTS && c <= 2 * (2 * d - 1); ++c) {
      const double cost = stockham_cost(c);
      if (cost > 0.0 && (best < 0.0 || cost < best)) { best = cost; M = c; }
    }
    if (best < 0.0) return r;
    rad = smooth_radices(M);
  }
  if (rad.empty() || rad.size() > (size_t)MAX_RADICES) return r;
  bool small_only = M > 0 && allow_inplace;
  for (int q : rad) small_only = small_only && in_register(q);
  r.d = d; r.M = M; r.L = M > 0 ? M : d; r.inplace = small_only ? 1 : 0; r.radix = rad;
  return r;
}
// Four-step: the best divisor pair of d; a length without one (a prime above 192, or 2 x such a prime ...) through Bluestein's
// convolution of the cheapest splittable M in [2d - 1, 2d - 1 + 12 %] (its input is complex whatever d's was)
inline Route plan_four_step(int d, bool complex_in) {
  Route r;
  if (d < 1 || d > MAX_POINTS) return r;
  std::pair<int, int> sp = dft4_split(d, complex_in);
  int M = 0;
  if (!sp.first) {
    long long bc = -1;
    for (int c = 2 * d - 1; c <= MAX_POINTS && c <= (2 * d - 1) + (2 * d - 1) / 8; ++c) {
      const std::pair<int, int> s2 = dft4_split(c, true);
      if (!s2.first) continue;
      const long long cost = dft4_cost(s2.first, s2.second, true);
      if (bc < 0 || cost < bc) { bc = cost; M = c; sp = s2; }
    }
  }
  if (!sp.first) return r;
  r.d = d; r.M = M; r.L = M > 0 ? M : d; r.N1 = sp.first; r.N2 = sp.second;
  return r;
}

// ---- tables ----
inline std::vector<cfloat> twiddles(int L) {      // exp(-2 pi i k / L), k = 0 .. L - 1
  std::vector<cfloat> h((size_t)L);
  for (int k = 0; k < L; ++k) {
    const double ang = -2.0 * PI * (double)k / (double)L;
    h[(size_t)k] = cfloat{(float)std::cos(ang), (float)std::sin(ang)};
  }
  return h;
}
// phase of the chirp w_n = exp(-i pi n^2 / d), reduced exactly (n^2 mod 2d)
inline double chirp_angle(int n, int d) { return -PI * (double)(((long long)n * n) % (2LL * d)) / (double)d; }
inline std::vector<cfloat> chirp(int d) {
  std::vector<cfloat> w((size_t)d);
  for (int n = 0; n < d; ++n) w[(size_t)n] = cfloat{(float)std::cos(chirp_angle(n, d)), (float)std::sin(chirp_angle(n, d))};
  return w;
}
// FFT_M of the conjugate chirp wrapped over M (b_n = b_{M-n} = conj w_n, n < d), divided by M; with `inplace_radices` entry k
// moves to dif_position(k): the in-place engine multiplies in digit-reversed order.  A plain O(M d) float64 DFT, once per
// length at build time, summed over ascending n (the table's bits depend on that order).
inline std::vector<cfloat> chirp_spectrum(int d, int M, const std::vector<int>* inplace_radices = nullptr) {
  std::vector<double> br((size_t)M, 0.0), bi((size_t)M, 0.0), cs((size_t)M), sn((size_t)M);
  std::vector<int> nz;                                  // the 2d - 1 non-zero entries of b, ascending
  for (int n = 0; n < d; ++n) {
    const double ang = chirp_angle(n, d);
    br[(size_t)n] = std::cos(ang); bi[(size_t)n] = -std::sin(ang);
    nz.push_back(n);
    if (n) { br[(size_t)(M - n)] = std::cos(ang); bi[(size_t)(M - n)] = -std::sin(ang); nz.push_back(M - n); }
  }
  std::sort(nz.begin(), nz.end());
  for (int k = 0; k < M; ++k) { cs[(size_t)k] = std::cos(-2.0 * PI * k / M); sn[(size_t)k] = std::sin(-2.0 * PI * k / M); }
  std::vector<cfloat> fb((size_t)M);
  for (int k = 0; k < M; ++k) {
    double sr = 0.0, si = 0.0;
    for (int n : nz) {
      const size_t q = (size_t)(((long long)k * n) % M);
      sr += br[(size_t)n] * cs[q] - bi[(size_t)n] * sn[q];
      si += br[(size_t)n] * sn[q] + bi[(size_t)n] * cs[q];
    }
    fb[(size_t)(inplace_radices ? dif_position(k, M, *inplace_radices) : k)] = cfloat{(float)(sr / M), (float)(si / M)};
  }
  return fb;
}
// A dense DFT of N points as the operand of the four-step engine's MFMA products, in lane order:
// [ceil(N / 16) tile pairs p][part: re | im outputs][k steps ks][64 lanes l], output k1 = 16 p + (l & 15), K index
// k = 4 ks + (l >> 4) over Np = N rounded up to 4 real inputs n = k, then Np imaginary ones n = k - Np; zero outside N.
// With th = 2 pi k1 n / N (F = cos - i sin):  re out = cos xr + sin xi,  im out = -sin xr + cos xi.
// Step 1 takes it as the A operand with N = N1 (row tiles), step 3 as the B operand with N = N2 (column tiles).
inline std::vector<float> dft4_matrix(int N) {
  const int P = (N + 15) / 16, Np = (N + 3) / 4 * 4, KS = 2 * Np / 4;
  std::vector<float> g((size_t)P * 2 * KS * 64, 0.0f);
  for (int p = 0; p < P; ++p)
    for (int part = 0; part < 2; ++part)
      for (int ks = 0; ks < KS; ++ks)
        for (int l = 0; l < 64; ++l) {
          const int k1 = 16 * p + (l & 15), k = 4 * ks + (l >> 4);
          const int n = k < Np ? k : k - Np;
          if (k1 >= N || n >= N) continue;
          const double th = 2.0 * PI * (double)(((long long)k1 * n) % N) / (double)N;
          const double v = part == 0 ? (k < Np ? std::cos(th) : std::sin(th)) : (k < Np ? -std::sin(th) : std::cos(th));
          g[(((size_t)p * 2 + part) * KS + ks) * 64 + l] = (float)v;
        }
  return g;
}

// ---- launch geometry (L: the longest transform of a launch) ----
inline int wave_round(int threads, int lo) { return std::min(1024, std::max(lo, (threads + 63) / 64 * 64)); }
inline int threads(int L, bool inplace, int N1, int N2) {
  if (N1 > 0) return wave_round(((N1 + 15) / 16) * ((N2 + 15) / 16) * 64, 256);      // four-step: one wave per tile task of the larger step (at most 16 waves)
  if (inplace) return wave_round(L / 8, 64);                                           // one radix-8 group per thread and pass
  return wave_round((L + 3) / 4, 64);                                                  // four output points per thread (dft_stockham)
}
inline size_t lds_bytes(int L, bool inplace, int N1, const int* radix, int nr) {      // of one transform
  if (N1 > 0) return (size_t)L * FOUR_STEP_POINT_BYTES;
  if (!inplace) return (size_t)L * STOCKHAM_POINT_BYTES;
  int rmin = 8;                                         // in place: L + L / 8 points (padded) + L / (smallest radix) twiddles
  for (int q = 0; q < nr; ++q) rmin = std::min(rmin, radix[q]);
  return (size_t)(L + L / 8 + L / rmin) * sizeof(cfloat);
}
inline int threads(const Route& r) { return threads(r.L, r.inplace != 0, r.N1, r.N2); }
inline size_t lds_bytes(const Route& r) { return lds_bytes(r.L, r.inplace != 0, r.N1, r.radix.data(), (int)r.radix.size()); }
}  // namespace fft
}  // namespace ssn
