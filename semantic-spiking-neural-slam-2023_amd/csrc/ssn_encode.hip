// ssn_encode.hip - SSP encoding of points behind ssn_encoder_* (include/ssn.h) and the table of ssn_decoder_create_from_points.
//
// Not on the step path and independent of ssn_sim, like ssn_decoder.  With (K, M, w) of SSPSpace.refine_tables() and th = x @ M.T,
//   encode(x)[c] = sum_{k<K} w_k ( cos th_k cos(2 pi k c / d) - sin th_k sin(2 pi k c / d) )
// (half spectrum with w = 1/d, 2/d, ... for a conjugate-symmetric phase matrix, all d bins with w = 1/d otherwise), so the SSPs of
// N points are P = [cos th_0, sin th_0, cos th_1, ...] (N x 2K) times a fixed table B (d x 2K) transposed, DESIGN.md 3.14.
//
//   k_encode_phase     one thread per (point, bin): th_k a float64 fma chain in axis order over the point converted to float64, a
//                      float64 sincos with full range reduction - in BOTH dtypes, because an f32 phase is off by eps |th| and |th|
//                      reaches a thousand radians - and only (cos, sin) rounded to the encoder's dtype, into P (row-major, 2K
//                      padded to Kp = 32 ceil(2K / 32), padding zero).
//   product, f32       ssn::launch_gemm_nt<float> with one split against B (d x Kp): every entry the k-ordered fmaf chain over Kp.
//   k_encode_product   f64 (parity mode, and what decoder tables are made with): 64 x 64 entries per 256-thread workgroup, 4 x 4
//                      per thread, K in slabs of 16 through LDS (so B is read from memory once per 64 points, not per point);
//                      every entry one fma chain in k order.  Its output type may be float: the float64 entry rounded once.
//   k_encode_widen     f32 entries to the doubles the host-output call returns.
//
// Regions.  The SSP of an axis-aligned box - its integral, its mean, or the sum over a linspace mesh of n_a points
// per axis (slam_map_new.py:412-416) - is encode(centre)'s bin k times a real amplitude A_k(box), so a region is the same product on
// P = [A cos th, A sin th]:
//   integral  A_k = prod_a L_a sinc(y_a),  y_a = M_ka L_a / 2           mean  the same without the L_a
//   mesh      A_k = prod_a sin(n_a y_a) / sin(y_a),  y_a = M_ka L_a / (2 (n_a - 1))
//   k_encode_phase_box one thread per (box, bin): a box row is lo_0, hi_0, lo_1, hi_1, ...; th_k the same fma chain on
//                      c_a = 0.5 (lo_a + hi_a), the amplitude and the sincos float64 in both dtypes, (A cos th, A sin th) rounded
//                      once.  The removable singularities are selected away in float64, never branched on:
//                        sinc(y)      |y| < 2^-10: 1 - y^2/6 + y^4/120, which leaves y^6/5040 < 2^-72; else sin(y) / y.  Bin 0 has
//                                     M_0 = 0, so every box takes the series there.
//                        mesh ratio   y = q pi + r with q = rint(y / pi) and pi in two parts (|r| <= pi/2, the reduction exact to
//                                     |q| 2^-107), sin(n y) / sin(y) = (-1)^(q (n - 1)) sin(n r) / sin(r).  |r| < 2^-26: sin(r) = r to
//                                     r^2/6 < 2^-54 relative, and the ratio is n sinc(n r) with the sinc above (at r = 0: +-n); else
//                                     sin(n r) / sin(r).
//                      A box with hi_a < lo_a raises a flag word (a plain store of 1 by every thread that sees one).
//   k_encode_rownorm   one wave per row: sum x^2 in float64, lane l over the columns l, l + 64, ... in order, then a fixed xor butterfly
//                      (every lane ends with the same bits); the row divided in place by max(norm, 1e-8) - SSPSpace.normalize's
//                      rule - in float64 and rounded once.  Only for a normalised result that stays on the device.
// The box path stages 2 dim doubles per row and sizes its own chunks from that; the point path's sizes are untouched.
//
// B is made on the host in float64 at creation, the angle reduced exactly ((k c) mod d), and converted once.  Scratch (fixed at
// creation, default 64 MB): per point dim doubles of staging, Kp values of P, d values of the result and, in f32, d doubles of
// the widened result.  Points are cut into chunks that fit; an entry never depends on the chunk it is in, and there are no
// atomics, so the bits are the same for any scratch size, for host and device points and from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>
#include "../../include/ssn.h"
#include "ssn_launch.hpp"      // launch_gemm_nt<float>, instantiated by ssn_f32.hip
#include "ssn_encode.hpp"
#include "ssn_service.hpp"

using namespace ssn::svc;      // fail, SVC_HIP, DevGuard, Lane, elapsed, stage_rows, check_rows

namespace {

constexpr int ROWS = 64;             // points per product tile: chunks are whole tiles
constexpr int KPAD = 32;             // 2K is padded to a multiple of this
constexpr int BK = 16;               // slab of the f64 product

template <typename TI, typename T>
__global__ __launch_bounds__(256) void k_encode_phase(const TI* __restrict__ pts, long long ld, int n, int dim, int K, int Kp,
                                                      const double* __restrict__ M, T* __restrict__ P) {
  const int half = Kp >> 1;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long row = i / half;
  if (row >= n) return;
  const int k = (int)(i - row * half);
  T cs_t = T(0), sn_t = T(0);
  if (k < K) {
    const TI* __restrict__ x = pts + (size_t)row * ld;
    const double* __restrict__ m = M + (size_t)k * dim;
    double th = m[0] * (double)x[0];
    for (int a = 1; a < dim; ++a) th = fma(m[a], (double)x[a], th);
    double sn, cs;
    sincos(th, &sn, &cs);
    cs_t = (T)cs;
    sn_t = (T)sn;
  }
  T* __restrict__ p = P + (size_t)row * Kp + 2 * k;
  p[0] = cs_t;
  p[1] = sn_t;
}

enum { BOX_INTEGRAL = 0, BOX_MEAN = 1, BOX_MESH = 2 };

__device__ __forceinline__ double sinc_guarded(double y) {
  const bool small = fabs(y) < 0x1p-10;
  const double y2 = y * y;
  const double series = fma(y2, fma(y2, 1.0 / 120.0, -1.0 / 6.0), 1.0);
  const double ratio = sin(y) / (small ? 1.0 : y);
  return small ? series : ratio;
}

// sin(n y) / sin(y) for an integer n >= 2 held in nd
__device__ __forceinline__ double dirichlet_guarded(double y, double nd, bool n_even) {
  constexpr double PI_HI = 0x1.921fb54442d18p+1, PI_LO = 0x1.1a62633145c07p-53, INV_PI = 0x1.45f306dc9c883p-2;
  const double q = rint(y * INV_PI);
  const double r = fma(-q, PI_LO, fma(-q, PI_HI, y));
  const bool small = fabs(r) < 0x1p-26;
  const double nr = nd * r;
  const double near = nd * sinc_guarded(nr);
  const double away = sin(nr) / sin(small ? 1.0 : r);
  const double v = small ? near : away;
  const bool q_odd = fmod(fabs(q), 2.0) == 1.0;
  return (q_odd && n_even) ? -v : v;
}

// tab: per axis (n_a, 0.5 / (n_a - 1)) for the mesh; unused otherwise
template <typename TI, typename T>
__global__ __launch_bounds__(256) void k_encode_phase_box(const TI* __restrict__ boxes, long long ld, int n, int dim, int K, int Kp,
                                                          const double* __restrict__ M, int mode, const double* __restrict__ tab,
                                                          int* __restrict__ flag, T* __restrict__ P) {
  const int half = Kp >> 1;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long row = i / half;
  if (row >= n) return;
  const int k = (int)(i - row * half);
  T cs_t = T(0), sn_t = T(0);
  if (k < K) {
    const TI* __restrict__ b = boxes + (size_t)row * ld;
    const double* __restrict__ m = M + (size_t)k * dim;
    double th = 0.0, amp = 1.0;
    bool bad = false;
    for (int a = 0; a < dim; ++a) {
      const double lo = (double)b[2 * a], hi = (double)b[2 * a + 1];
      const double c = 0.5 * (lo + hi), L = hi - lo;
      bad |= hi < lo;
      th = a == 0 ? m[0] * c : fma(m[a], c, th);
      const double mL = m[a] * L;
      double f;
      if (mode == BOX_MESH) {
        const double nd = tab[2 * a];
        f = dirichlet_guarded(mL * tab[2 * a + 1], nd, fmod(nd, 2.0) == 0.0);
      } else {
        f = sinc_guarded(0.5 * mL);
        if (mode == BOX_INTEGRAL) f *= L;
      }
      amp *= f;
    }
    if (bad) *flag = 1;
    double sn, cs;
    sincos(th, &sn, &cs);
    cs_t = (T)(amp * cs);
    sn_t = (T)(amp * sn);
  }
  T* __restrict__ p = P + (size_t)row * Kp + 2 * k;
  p[0] = cs_t;
  p[1] = sn_t;
}

template <typename T>
__global__ __launch_bounds__(256) void k_encode_rownorm(T* __restrict__ X, long long ld, int n, int d) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;      // a whole wave at a time
  T* __restrict__ x = X + (size_t)row * ld;
  double s = 0.0;
  for (int c = lane; c < d; c += 64) {
    const double v = (double)x[c];
    s = fma(v, v, s);
  }
  for (int w = 32; w >= 1; w >>= 1) s += __shfl_xor(s, w, 64);
  const double nrm = fmax(sqrt(s), 1e-8);
  for (int c = lane; c < d; c += 64) x[c] = (T)((double)x[c] / nrm);
}

template <typename TO>
__global__ __launch_bounds__(256) void k_encode_product(const double* __restrict__ P, const double* __restrict__ B, int Kp, int n, int d,
                                                        TO* __restrict__ C, long long ldc) {
  __shared__ double Ps[ROWS][BK + 1];
  __shared__ double Bs[ROWS][BK + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int r0 = blockIdx.y * ROWS, c0 = blockIdx.x * ROWS;
  const int lr = tid >> 4, lc = tid & 15;      // this thread stages rows lr + 16 i, column lc of a slab
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  for (int k0 = 0; k0 < Kp; k0 += BK) {      // Kp is a multiple of 32: every slab is whole
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + lr + 16 * i, c = c0 + lr + 16 * i;
      Ps[lr + 16 * i][lc] = r < n ? P[(size_t)r * Kp + k0 + lc] : 0.0;
      Bs[lr + 16 * i][lc] = c < d ? B[(size_t)c * Kp + k0 + lc] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < BK; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = Ps[ty + 16 * i][kk]; b[i] = Bs[tx + 16 * i][kk]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + ty + 16 * i;
    if (r >= n) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + tx + 16 * j;
      if (c < d) C[(size_t)r * ldc + c] = (TO)acc[i][j];
    }
  }
}

__global__ __launch_bounds__(256) void k_encode_widen(const float* __restrict__ src, double* __restrict__ dst, long long count) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < count) dst[i] = (double)src[i];
}

}  // namespace

struct ssn_encoder : Lane {
  int dtype = 0;
  int64_t d = 0, K = 0, Kp = 0, dim = 0;
  size_t esz = 4;
  double* M = nullptr;             // (K x dim)
  void* B = nullptr;               // (d x Kp) in the encoder's dtype
  double phase_ms = 0.0, product_ms = 0.0;      // of the last encode call

  int64_t row_bytes() const { return dim * 8 + Kp * (int64_t)esz + d * (int64_t)esz + (esz == 4 ? d * 8 : 0); }
  int64_t min_scratch() const { return ROWS * row_bytes(); }
  // rows per chunk: whole tiles that fit, bounded so that the 32-bit sizes of the kernels hold
  int64_t chunk_rows() const {
    int64_t tiles = std::max<int64_t>(1, scratch_bytes / (ROWS * row_bytes()));
    const int64_t widest = std::max(Kp, d);
    tiles = std::min<int64_t>(tiles, std::max<int64_t>(1, ((int64_t)1 << 30) / (ROWS * widest)));
    return std::min<int64_t>(tiles, 1 << 15) * ROWS;
  }
  // the box path: 2 dim doubles of staging per row in place of dim
  double* box_tab = nullptr;       // per axis (n_a, 0.5 / (n_a - 1)), then the flag word of k_encode_phase_box; made by the first box call
  int64_t box_row_bytes() const { return row_bytes() + dim * 8; }
  int64_t box_min_scratch() const { return ROWS * box_row_bytes(); }
  int64_t box_chunk_rows() const {
    int64_t tiles = std::max<int64_t>(1, scratch_bytes / (ROWS * box_row_bytes()));
    const int64_t widest = std::max(Kp, d);
    tiles = std::min<int64_t>(tiles, std::max<int64_t>(1, ((int64_t)1 << 30) / (ROWS * widest)));
    return std::min<int64_t>(tiles, 1 << 15) * ROWS;
  }

  ~ssn_encoder() {
    DevGuard g(device);
    for (void* p : {(void*)M, B, (void*)box_tab}) if (p) (void)hipFree(p);
  }
};

namespace {

struct Areas {      // the regions of the scratch area for a chunk capacity of `rows` input rows of `width` values
  char* stage; double* wide; void* P; void* out;
  Areas(const ssn_encoder* e, int64_t rows, int64_t width) {
    char* p = e->scratch;
    stage = p; p += (size_t)rows * width * 8;
    wide = (double*)p; if (e->esz == 4) p += (size_t)rows * e->d * 8;
    P = p; p += (size_t)rows * e->Kp * e->esz;
    out = p;
  }
};

template <typename T>
int upload_tables(ssn_encoder* e, const double* M, const double* w) {
  const int64_t d = e->d, K = e->K, Kp = e->Kp;
  std::vector<double> cs((size_t)d), sn((size_t)d);      // cos, sin of 2 pi r / d
  for (int64_t r = 0; r < d; ++r) {
    const double a = 2.0 * M_PI * (double)r / (double)d;
    cs[r] = std::cos(a);
    sn[r] = std::sin(a);
  }
  SVC_HIP(hipMalloc((void**)&e->M, (size_t)K * e->dim * 8));
  SVC_HIP(hipMemcpy(e->M, M, (size_t)K * e->dim * 8, hipMemcpyHostToDevice));
  SVC_HIP(hipMalloc(&e->B, (size_t)d * Kp * sizeof(T)));
  const int64_t per = std::max<int64_t>(1, (int64_t)(8 << 20) / Kp);
  std::vector<T> stage((size_t)std::min(per, d) * Kp, T(0));
  for (int64_t c0 = 0; c0 < d; c0 += per) {
    const int64_t nc = std::min(per, d - c0);
    for (int64_t c = 0; c < nc; ++c) {
      T* o = stage.data() + (size_t)c * Kp;
      for (int64_t k = 0; k < K; ++k) {
        const int64_t r = (k * (c0 + c)) % d;
        o[2 * k] = (T)(w[k] * cs[r]);
        o[2 * k + 1] = (T)(-(w[k] * sn[r]));
      }
    }
    SVC_HIP(hipMemcpy((T*)e->B + (size_t)c0 * Kp, stage.data(), (size_t)nc * Kp * sizeof(T), hipMemcpyHostToDevice));
  }
  return SSN_OK;
}

template <typename TI, typename T>
hipError_t launch_phase(ssn_encoder* e, const TI* pts, int64_t ld, int n, T* P) {
  const long long total = (long long)n * (e->Kp / 2);
  hipLaunchKernelGGL((k_encode_phase<TI, T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream, pts, (long long)ld, n, (int)e->dim, (int)e->K,
                     (int)e->Kp, (const double*)e->M, P);
  return hipGetLastError();
}

template <typename TI, typename T>
hipError_t launch_phase_box(ssn_encoder* e, int mode, const TI* boxes, int64_t ld, int n, T* P) {
  const long long total = (long long)n * (e->Kp / 2);
  hipLaunchKernelGGL((k_encode_phase_box<TI, T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream, boxes, (long long)ld, n, (int)e->dim,
                     (int)e->K, (int)e->Kp, (const double*)e->M, mode, (const double*)e->box_tab, (int*)(e->box_tab + 2 * e->dim), P);
  return hipGetLastError();
}

// The phase launcher of a call: the rows of a chunk (dtype in_dtype, leading dimension ld, on the device by then) into P of the encoder's dtype.
struct PointPhase {
  static constexpr int per_dim = 1;      // values per row and axis
  hipError_t operator()(ssn_encoder* e, const void* rows, int in_dtype, int64_t ld, int n, void* P) const {
    if (e->dtype == SSN_F32)
      return in_dtype == SSN_F32 ? launch_phase<float, float>(e, (const float*)rows, ld, n, (float*)P) : launch_phase<double, float>(e, (const double*)rows, ld, n, (float*)P);
    return in_dtype == SSN_F32 ? launch_phase<float, double>(e, (const float*)rows, ld, n, (double*)P) : launch_phase<double, double>(e, (const double*)rows, ld, n, (double*)P);
  }
};

struct BoxPhase {
  static constexpr int per_dim = 2;
  int mode;
  hipError_t operator()(ssn_encoder* e, const void* rows, int in_dtype, int64_t ld, int n, void* P) const {
    if (e->dtype == SSN_F32)
      return in_dtype == SSN_F32 ? launch_phase_box<float, float>(e, mode, (const float*)rows, ld, n, (float*)P)
                                 : launch_phase_box<double, float>(e, mode, (const double*)rows, ld, n, (float*)P);
    return in_dtype == SSN_F32 ? launch_phase_box<float, double>(e, mode, (const float*)rows, ld, n, (double*)P)
                               : launch_phase_box<double, double>(e, mode, (const double*)rows, ld, n, (double*)P);
  }
};

template <typename T>
hipError_t launch_rownorm(ssn_encoder* e, T* X, int64_t ld, int n) {
  hipLaunchKernelGGL((k_encode_rownorm<T>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, e->stream, X, (long long)ld, n, (int)e->d);
  return hipGetLastError();
}

template <typename TO>
hipError_t launch_product64(ssn_encoder* e, const double* P, int n, TO* C, int64_t ldc) {
  hipLaunchKernelGGL((k_encode_product<TO>), dim3((unsigned)((e->d + ROWS - 1) / ROWS), (unsigned)((n + ROWS - 1) / ROWS)), dim3(256), 0, e->stream, P,
                     (const double*)e->B, (int)e->Kp, n, (int)e->d, C, (long long)ldc);
  return hipGetLastError();
}

// Rows (points, or boxes with phase.per_dim == 2): host (on_device == 0) or device rows of pts_dtype with leading dimension pts_ld, `cap`
// of them per chunk, through the phase launcher `phase`.  Output: host doubles (dense), or a device buffer of out_dtype with leading
// dimension out_ld, its rows scaled to unit length with `normalize`.
template <typename Phase>
int encode(ssn_encoder* e, const Phase& phase, int64_t cap, const void* pts, int on_device, int pts_dtype, int64_t pts_ld, int64_t n, double* host_out,
           void* dev_out, int out_dtype, int64_t out_ld, bool normalize = false) {
  DevGuard g(e->device);
  const int64_t width = e->dim * Phase::per_dim;
  const Areas a(e, cap, width);
  const size_t isz = pts_dtype == SSN_F32 ? 4 : 8, osz = out_dtype == SSN_F32 ? 4 : 8;
  const bool f32 = e->dtype == SSN_F32;
  e->phase_ms = e->product_ms = 0.0;
  e->launches = 0;
  for (int64_t r0 = 0; r0 < n; r0 += cap) {
    const int m = (int)std::min(cap, n - r0);
    const void* src = (const char*)pts + (size_t)r0 * pts_ld * isz;
    int64_t ld = pts_ld;
    if (!on_device) {
      if (const int rc = stage_rows(e->stream, a.stage, src, pts_ld, width, isz, m)) return rc;
      src = a.stage;
      ld = width;
    }
    SVC_HIP(hipEventRecord(e->ev[0], e->stream));
    SVC_HIP(phase(e, src, pts_dtype, ld, m, a.P));
    SVC_HIP(hipEventRecord(e->ev[1], e->stream));
    e->launches += 2;
    if (f32) {
      float* C = host_out ? (float*)a.out : (float*)dev_out + (size_t)r0 * out_ld;
      const int ldc = host_out ? (int)e->d : (int)out_ld;
      SVC_HIP(ssn::launch_gemm_nt<float>(e->stream, (const float*)a.P, (int)e->Kp, (const float*)e->B, (int)e->Kp, C, ldc, m, (int)e->d, (int)e->Kp, 1));
      if (host_out) {
        const long long count = (long long)m * e->d;
        hipLaunchKernelGGL(k_encode_widen, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, e->stream, (const float*)a.out, a.wide, count);
        SVC_HIP(hipGetLastError());
        e->launches += 1;
      }
    } else if (host_out) {
      SVC_HIP(launch_product64<double>(e, (const double*)a.P, m, (double*)a.out, e->d));
    } else if (osz == 8) {
      SVC_HIP(launch_product64<double>(e, (const double*)a.P, m, (double*)dev_out + (size_t)r0 * out_ld, out_ld));
    } else {
      SVC_HIP(launch_product64<float>(e, (const double*)a.P, m, (float*)dev_out + (size_t)r0 * out_ld, out_ld));
    }
    if (normalize) {
      if (osz == 4) SVC_HIP(launch_rownorm<float>(e, (float*)dev_out + (size_t)r0 * out_ld, out_ld, m));
      else SVC_HIP(launch_rownorm<double>(e, (double*)dev_out + (size_t)r0 * out_ld, out_ld, m));
      e->launches += 1;
    }
    SVC_HIP(hipEventRecord(e->ev[2], e->stream));
    if (host_out)
      SVC_HIP(hipMemcpyAsync(host_out + (size_t)r0 * e->d, f32 ? (const void*)a.wide : (const void*)a.out, (size_t)m * e->d * 8, hipMemcpyDeviceToHost, e->stream));
    SVC_HIP(hipStreamSynchronize(e->stream));      // the next chunk reuses the scratch area
    if (const int rc = elapsed(e->ev[0], e->ev[1], &e->phase_ms)) return rc;
    if (const int rc = elapsed(e->ev[1], e->ev[2], &e->product_ms)) return rc;
  }
  return SSN_OK;
}

// The amplitude mode of a box call from (samples, mean); named errors for what the two exclude.
int box_mode(const ssn_encoder* e, const char* who, const int32_t* samples, int32_t mean, int* mode) {
  if (samples && mean) return fail(SSN_EINVAL, "%s: mean given together with samples (the mean of a mesh is its sum over the number of points)", who);
  if (samples)
    for (int64_t a = 0; a < e->dim; ++a)
      if (samples[a] < 2) return fail(SSN_EINVAL, "%s: samples[%lld] = %d below 2 (a linspace mesh has both ends)", who, (long long)a, samples[a]);
  *mode = samples ? BOX_MESH : mean ? BOX_MEAN : BOX_INTEGRAL;
  return SSN_OK;
}

template <typename TI>
int64_t first_inverted(const TI* boxes, int64_t ld, int64_t n, int64_t dim) {
  for (int64_t i = 0; i < n; ++i)
    for (int64_t a = 0; a < dim; ++a)
      if (boxes[i * ld + 2 * a + 1] < boxes[i * ld + 2 * a]) return i;
  return -1;
}

int encode_boxes(ssn_encoder* e, const char* who, int mode, const int32_t* samples, const void* boxes, int on_device, int dtype, int64_t ld, int64_t n,
                 double* host_out, void* dev_out, int64_t out_ld, bool normalize) {
  if (e->scratch_bytes < e->box_min_scratch())
    return fail(SSN_EINVAL, "%s: scratch_bytes %lld too small for one %d-box tile of d %lld, K %lld (%lld bytes)", who, (long long)e->scratch_bytes, ROWS,
                (long long)e->d, (long long)e->K, (long long)e->box_min_scratch());
  if (!on_device) {
    const int64_t bad = dtype == SSN_F32 ? first_inverted((const float*)boxes, ld, n, e->dim) : first_inverted((const double*)boxes, ld, n, e->dim);
    if (bad >= 0) return fail(SSN_EINVAL, "%s: box %lld has hi < lo on an axis", who, (long long)bad);
  }
  DevGuard g(e->device);
  const size_t tab_bytes = (size_t)(2 * e->dim + 1) * 8;      // the table and, in its last word, the flag
  if (!e->box_tab) SVC_HIP(hipMalloc((void**)&e->box_tab, tab_bytes));
  std::vector<double> tab((size_t)(2 * e->dim + 1), 0.0);
  for (int64_t a = 0; a < e->dim && samples; ++a) {
    tab[2 * a] = (double)samples[a];
    tab[2 * a + 1] = 0.5 / (double)(samples[a] - 1);
  }
  SVC_HIP(hipMemcpy(e->box_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice));
  const int rc = encode(e, BoxPhase{mode}, e->box_chunk_rows(), boxes, on_device, dtype, ld, n, host_out, dev_out, e->dtype, out_ld, normalize);
  if (rc != SSN_OK) return rc;
  int flag = 0;
  SVC_HIP(hipMemcpy(&flag, e->box_tab + 2 * e->dim, sizeof flag, hipMemcpyDeviceToHost));
  if (flag) return fail(SSN_EINVAL, "%s: a box has hi < lo on an axis", who);
  return SSN_OK;
}

}  // namespace

namespace ssn {

int encoder_encode_into(ssn_encoder* enc, const double* points, int64_t n, void* out_dev, int32_t out_dtype, int64_t out_ld) {
  if (!enc || !points || !out_dev || n <= 0) return fail(SSN_EINVAL, "encoder_encode_into: null or empty argument");
  if (out_ld < enc->d) return fail(SSN_EINVAL, "encoder_encode_into: leading dimension %lld below the width %lld", (long long)out_ld, (long long)enc->d);
  if (enc->dtype == SSN_F32 && out_dtype != SSN_F32) return fail(SSN_EINVAL, "encoder_encode_into: an f32 encoder writes f32 only");
  return encode(enc, PointPhase(), enc->chunk_rows(), points, 0, SSN_F64, enc->dim, n, nullptr, out_dev, out_dtype, out_ld);
}

}  // namespace ssn

extern "C" {

int ssn_encoder_create(int32_t dtype, int32_t device, int64_t d, int64_t K, int32_t dim, const double* M, const double* w, int64_t scratch_bytes,
                       ssn_encoder** out) {
  if (!out) return fail(SSN_EINVAL, "ssn_encoder_create: null handle");
  *out = nullptr;
  if (!M || !w) return fail(SSN_EINVAL, "ssn_encoder_create: null argument");
  if (dtype != SSN_F32 && dtype != SSN_F64) return fail(SSN_EINVAL, "ssn_encoder_create: unknown dtype %d", dtype);
  if (dim < 1) return fail(SSN_EINVAL, "ssn_encoder_create: dim %d below 1", dim);
  if (d < 1 || d > (1 << 20)) return fail(SSN_EINVAL, "ssn_encoder_create: d %lld outside 1 .. 2^20", (long long)d);
  if (K < 1 || K > d) return fail(SSN_EINVAL, "ssn_encoder_create: K %lld outside 1 .. d = %lld", (long long)K, (long long)d);
  std::unique_ptr<ssn_encoder> e(new ssn_encoder);
  e->dtype = dtype;
  e->esz = dtype == SSN_F32 ? 4 : 8;
  e->d = d;
  e->K = K;
  e->dim = dim;
  e->Kp = (2 * K + KPAD - 1) / KPAD * KPAD;
  if (const int rc = e->open("ssn_encoder_create", device, scratch_bytes, e->min_scratch(), "%d-point tile of d %lld, K %lld", ROWS, (long long)d, (long long)K))
    return rc;
  DevGuard g(device);
  const int rc = dtype == SSN_F32 ? upload_tables<float>(e.get(), M, w) : upload_tables<double>(e.get(), M, w);
  if (rc != SSN_OK) return rc;
  *out = e.release();
  return SSN_OK;
}

void ssn_encoder_destroy(ssn_encoder* enc) { delete enc; }

int ssn_encoder_encode(ssn_encoder* enc, const double* points, int64_t n, double* out) {
  if (!enc) return fail(SSN_EINVAL, "ssn_encoder_encode: null encoder");
  if (n < 0) return fail(SSN_EINVAL, "ssn_encoder_encode: negative n");
  if (n == 0) return SSN_OK;
  if (!points || !out) return fail(SSN_EINVAL, "ssn_encoder_encode: null argument");
  return encode(enc, PointPhase(), enc->chunk_rows(), points, 0, SSN_F64, enc->dim, n, out, nullptr, SSN_F64, enc->d);
}

int ssn_encoder_encode_device(ssn_encoder* enc, const void* points, int32_t points_on_device, int32_t points_dtype, int64_t points_ld, int64_t n,
                              void* out_dev, int64_t out_ld) {
  if (!enc) return fail(SSN_EINVAL, "ssn_encoder_encode_device: null encoder");
  if (n < 0) return fail(SSN_EINVAL, "ssn_encoder_encode_device: negative n");
  if (const int rc = check_rows("ssn_encoder_encode_device", "points", points_dtype, points_ld, enc->dim, " of the points", "dim")) return rc;
  if (out_ld < enc->d) return fail(SSN_EINVAL, "ssn_encoder_encode_device: leading dimension %lld of the output below the width %lld", (long long)out_ld, (long long)enc->d);
  if (out_ld > INT32_MAX) return fail(SSN_EINVAL, "ssn_encoder_encode_device: leading dimension %lld of the output above 2^31 - 1", (long long)out_ld);
  if (n == 0) return SSN_OK;
  if (!points || !out_dev) return fail(SSN_EINVAL, "ssn_encoder_encode_device: null argument");
  return encode(enc, PointPhase(), enc->chunk_rows(), points, points_on_device != 0, points_dtype, points_ld, n, nullptr, out_dev, enc->dtype, out_ld);
}

int ssn_encoder_encode_boxes(ssn_encoder* enc, const double* boxes, int64_t n, const int32_t* samples, int32_t mean, double* out) {
  const char* who = "ssn_encoder_encode_boxes";
  if (!enc) return fail(SSN_EINVAL, "%s: null encoder", who);
  if (n < 0) return fail(SSN_EINVAL, "%s: negative n", who);
  int mode = 0;
  if (const int rc = box_mode(enc, who, samples, mean, &mode)) return rc;
  if (n == 0) return SSN_OK;
  if (!boxes || !out) return fail(SSN_EINVAL, "%s: null argument", who);
  return encode_boxes(enc, who, mode, samples, boxes, 0, SSN_F64, 2 * enc->dim, n, out, nullptr, enc->d, false);
}

int ssn_encoder_encode_boxes_device(ssn_encoder* enc, const void* boxes, int32_t boxes_on_device, int32_t boxes_dtype, int64_t boxes_ld, int64_t n,
                                    const int32_t* samples, int32_t mean, int32_t normalize, void* out_dev, int64_t out_ld) {
  const char* who = "ssn_encoder_encode_boxes_device";
  if (!enc) return fail(SSN_EINVAL, "%s: null encoder", who);
  if (n < 0) return fail(SSN_EINVAL, "%s: negative n", who);
  if (const int rc = check_rows(who, "boxes", boxes_dtype, boxes_ld, 2 * enc->dim, " of the boxes", "2 dim =")) return rc;
  if (out_ld < enc->d) return fail(SSN_EINVAL, "%s: leading dimension %lld of the output below the width %lld", who, (long long)out_ld, (long long)enc->d);
  if (out_ld > INT32_MAX) return fail(SSN_EINVAL, "%s: leading dimension %lld of the output above 2^31 - 1", who, (long long)out_ld);
  int mode = 0;
  if (const int rc = box_mode(enc, who, samples, mean, &mode)) return rc;
  if (n == 0) return SSN_OK;
  if (!boxes || !out_dev) return fail(SSN_EINVAL, "%s: null argument", who);
  return encode_boxes(enc, who, mode, samples, boxes, boxes_on_device != 0, boxes_dtype, boxes_ld, n, nullptr, out_dev, out_ld, normalize != 0);
}

int ssn_encoder_get_info(ssn_encoder* enc, int64_t n, ssn_encoder_info* out) {
  if (!enc || !out || n < 0) return fail(SSN_EINVAL, "ssn_encoder_get_info: null argument");
  const int64_t cap = enc->chunk_rows();
  out->row_chunk = cap;
  out->n_chunks = (n + cap - 1) / cap;
  out->tile = ROWS;
  out->scratch_bytes = enc->scratch_bytes;
  out->min_scratch_bytes = enc->min_scratch();
  out->padded_2k = enc->Kp;
  out->last_launches = enc->launches;
  out->last_kernel_ms = enc->phase_ms + enc->product_ms;
  out->last_phase_ms = enc->phase_ms;
  out->last_product_ms = enc->product_ms;
  return SSN_OK;
}

}  // extern "C"
