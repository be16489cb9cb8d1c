// ssn_bind.hip - binding (circular convolution) of rows behind ssn_binder_* (include/ssn.h): SSPSpace.bind / SPSpace.bind,
// ifft(fft(a) * fft(b)).real per row pair, with the operands' inversion, the row pairing and the normalisation of the landmark vector
// queries (slam_map_new.py:453-485) in the same launch.  DESIGN.md 3.17.
//
// Not on the step path and independent of ssn_sim, like the decoder and the encoder.  A binder depends on d and the dtype only.
//
//   k_bind_rows    f32: one workgroup per output row, the whole convolution in LDS (24 B per point of the transform length L:
//                  two arrays of L complex points and the twiddle table, as dft_body lays them out).
//                    load      x_i = (a_i, b_i); an inverted operand is read at (d - i) mod d (an index, no conjugation).
//                    balance   Sa = sum a_i^2, Sb = sum b_i^2 in float64: lane l of EVERY wave sums i = l, l + 64, ... in order,
//                              then a fixed xor butterfly - the same bits in every lane of every wave for any workgroup size.
//                              Sa == 0 or Sb == 0: the output row is zero, exactly.  Otherwise q = ilogb(Sa / Sb),
//                              e = floor((q + 1) / 2), s = 2^e: |a| / (s |b|) lies in [1 / sqrt 2, sqrt 2).  z = a + i s b.
//                    forward   Z = FFT_d(z) (dft_chirpz: dft_stockham, through the chirp-z form when d is not smooth).
//                    separate  A_k = (Z_k + conj Z_{d-k}) / 2, s B_k = (Z_k - conj Z_{d-k}) / 2i, conj(A_k s B_k) for all d bins
//                              into the other array; bin 0, and bin d / 2 of an even d, are Re Z * Im Z: real.
//                    back      FFT_d of that: its real part is d s c_j.  Times 1 / d, then 2^-e (exact).
//                    normalise (flag) the row over max(sqrt(sum c_j^2), floor): the sum in float64 in the order of `balance`
//                              over the row parked in LDS, the quotient float64, rounded once.
//   k_bind_direct  f64 (the parity mode): one workgroup per row, a and b in LDS as doubles (16 B per point), entry j the fma chain
//                  over i = 0 .. d - 1 of a_i b_{(j - i) mod d}, started from 0.  No transform.  The same normalisation.
//
// Pairing: output row r takes operand row r / (n / count), count in {1, n, a divisor of n}.  Operands are f32 or f64, on the host
// (staged through the scratch area, chunk by chunk) or on the binder's device (read in place with their own row stride).
// Scratch (fixed at creation, default 64 MB): per row of a chunk d doubles for each staged operand and d doubles of host output.
// An entry never depends on the chunk its row is in, and there are no atomics, so the bits are the same for any scratch size, for
// host and device operands of the same values and from run to run.
// The route of a width - direct, or out-of-place Bluestein -, its tables, its workgroup and its LDS bytes are the planner's
// (ssn_fft_plan.hpp: plan_stockham with in-place forbidden), shared with k_dft.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>
#include "../../include/ssn.h"
#include "ssn_launch.hpp"
#include "ssn_fft_plan.hpp"
#include "ssn_kernels.hpp"      // dft_chirpz, cmulf
#include "ssn_service.hpp"

using namespace ssn::svc;      // fail, SVC_HIP, DevGuard, Lane, elapsed, stage_rows, check_rows

namespace {

namespace fft = ssn::fft;
static_assert(sizeof(fft::cfloat) == sizeof(float2), "the planner's tables are uploaded as float2");
constexpr int BIND_MAX_L = fft::MAX_POINTS;      // points of the longest transform: 153.6 KB of LDS
constexpr int BIND_MAX_D64 = 10000;        // f64: 16 B of LDS per point
enum { BIND_INVERT_A = 1, BIND_INVERT_B = 2, BIND_NORMALIZE = 4 };

struct BindArgs {
  const void* a; const void* b; void* out;
  long long a_ld, b_ld, out_ld;            // elements
  long long a_div, b_div;                  // output row r pairs operand row r / div
  long long a_row0, b_row0;                // first operand row behind the pointer (a staged chunk)
  long long row0;                          // output row of workgroup 0; `out` points at it
  int a64, b64, out64;                     // element types: 1 double, 0 float
  int d, L, M, nr;
  int radix[fft::MAX_RADICES];
  int flags;
  double norm_floor;
  const float2* tw;                        // exp(-2 pi i k / L)
  const float2* chirp;                     // M > 0: exp(-i pi n^2 / d)
  const float2* fb;                        // M > 0: FFT_M of the wrapped conjugate chirp over M
};

__device__ __forceinline__ float ld_f32(const void* p, int is64, int i) {
  return is64 ? (float)((const double*)p)[i] : ((const float*)p)[i];
}
__device__ __forceinline__ double ld_f64(const void* p, int is64, int i) {
  return is64 ? ((const double*)p)[i] : (double)((const float*)p)[i];
}
__device__ __forceinline__ const void* operand_row(const void* base, int is64, long long row, long long ld) {
  return (const char*)base + (size_t)row * (size_t)ld * (is64 ? 8 : 4);
}
__device__ __forceinline__ double wave_sum(double s) {
  for (int w = 32; w >= 1; w >>= 1) s += __shfl_xor(s, w, 64);
  return s;
}

__global__ __launch_bounds__(1024) void k_bind_rows(const BindArgs g) {
  extern __shared__ __align__(16) unsigned char ssn_bind_smem[];
  const int d = g.d, L = g.L, tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
  float2* x = reinterpret_cast<float2*>(ssn_bind_smem);
  float2* y = x + L;
  float2* tw = y + L;
  const long long r = g.row0 + blockIdx.x;
  const void* ap = operand_row(g.a, g.a64, r / g.a_div - g.a_row0, g.a_ld);
  const void* bp = operand_row(g.b, g.b64, r / g.b_div - g.b_row0, g.b_ld);
  char* op = (char*)g.out + (size_t)blockIdx.x * (size_t)g.out_ld * (g.out64 ? 8 : 4);
  const bool inv_a = g.flags & BIND_INVERT_A, inv_b = g.flags & BIND_INVERT_B;
  for (int i = tid; i < L; i += nthr) {
    tw[i] = g.tw[i];
    float2 v = make_float2(0.0f, 0.0f);
    if (i < d) {
      const int m = i ? d - i : 0;
      v = make_float2(ld_f32(ap, g.a64, inv_a ? m : i), ld_f32(bp, g.b64, inv_b ? m : i));
    }
    x[i] = v;
  }
  __syncthreads();
  double sa = 0.0, sb = 0.0;
  for (int i = lane; i < d; i += 64) {
    const float2 v = x[i];
    sa = fma((double)v.x, (double)v.x, sa);
    sb = fma((double)v.y, (double)v.y, sb);
  }
  sa = wave_sum(sa);
  sb = wave_sum(sb);
  if (sa == 0.0 || sb == 0.0) {      // (the same bits in every wave: the whole workgroup leaves)
    for (int j = tid; j < d; j += nthr) {
      if (g.out64) ((double*)op)[j] = 0.0; else ((float*)op)[j] = 0.0f;
    }
    return;
  }
  const int t = ilogb(sa / sb) + 1;
  const int e = min(100, max(-100, (t - (t & 1)) / 2));
  const float s = ldexpf(1.0f, e);
  __syncthreads();                   // every wave has read x
  for (int i = tid; i < d; i += nthr) {
    float2 v = x[i];
    v.y *= s;
    if (g.M > 0) v = ssn::cmulf(v, g.chirp[i]);
    x[i] = v;
  }
  __syncthreads();
  ssn::dft_chirpz(x, y, tw, L, g, d, tid, nthr);
  for (int k = tid; k < L; k += nthr) {
    float2 c = make_float2(0.0f, 0.0f);
    if (k < d) {
      const float2 zk = x[k];
      if (k == 0 || 2 * k == d) {
        c = make_float2(zk.x * zk.y, 0.0f);
      } else {
        const float2 zm = x[d - k];
        const float ar = zk.x + zm.x, ai = zk.y - zm.y, br = zk.y + zm.y, bi = zm.x - zk.x;      // 2 A_k, 2 s B_k
        c = make_float2(0.25f * fmaf(ar, br, -(ai * bi)), -0.25f * fmaf(ar, bi, ai * br));
      }
      if (g.M > 0) c = ssn::cmulf(c, g.chirp[k]);
    }
    y[k] = c;
  }
  __syncthreads();
  { float2* t2 = x; x = y; y = t2; }
  ssn::dft_chirpz(x, y, tw, L, g, d, tid, nthr);
  const float inv_d = 1.0f / (float)d;
  if (!(g.flags & BIND_NORMALIZE)) {
    for (int j = tid; j < d; j += nthr) {
      const float v = ldexpf(x[j].x * inv_d, -e);
      if (g.out64) ((double*)op)[j] = (double)v; else ((float*)op)[j] = v;
    }
    return;
  }
  float* row = reinterpret_cast<float*>(y);
  for (int j = tid; j < d; j += nthr) row[j] = ldexpf(x[j].x * inv_d, -e);
  __syncthreads();
  double ss = 0.0;
  for (int j = lane; j < d; j += 64) {
    const double v = (double)row[j];
    ss = fma(v, v, ss);
  }
  const double nrm = fmax(sqrt(wave_sum(ss)), g.norm_floor);
  for (int j = tid; j < d; j += nthr) {
    const float v = (float)((double)row[j] / nrm);
    if (g.out64) ((double*)op)[j] = (double)v; else ((float*)op)[j] = v;
  }
}

template <int NU>      // entries of a row per thread: ceil(d / threads)
__global__ __launch_bounds__(1024) void k_bind_direct(const BindArgs g) {
  extern __shared__ __align__(16) unsigned char ssn_bind_smem[];
  const int d = g.d, tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
  double* a = reinterpret_cast<double*>(ssn_bind_smem);
  double* b = a + d;
  const long long r = g.row0 + blockIdx.x;
  const void* ap = operand_row(g.a, g.a64, r / g.a_div - g.a_row0, g.a_ld);
  const void* bp = operand_row(g.b, g.b64, r / g.b_div - g.b_row0, g.b_ld);
  double* op = (double*)g.out + (size_t)blockIdx.x * (size_t)g.out_ld;
  const bool inv_a = g.flags & BIND_INVERT_A, inv_b = g.flags & BIND_INVERT_B;
  for (int i = tid; i < d; i += nthr) {
    const int m = i ? d - i : 0;
    a[i] = ld_f64(ap, g.a64, inv_a ? m : i);
    b[i] = ld_f64(bp, g.b64, inv_b ? m : i);
  }
  __syncthreads();
  double c[NU];
  int idx[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    c[u] = 0.0;
    const int j = tid + u * nthr;
    idx[u] = j < d ? j : 0;            // (an entry past the row runs the chain on entry 0 and is never stored)
  }
  for (int i = 0; i < d; ++i) {
    const double ai = a[i];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      c[u] = fma(ai, b[idx[u]], c[u]);
      idx[u] = idx[u] ? idx[u] - 1 : d - 1;
    }
  }
  if (!(g.flags & BIND_NORMALIZE)) {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int j = tid + u * nthr;
      if (j < d) op[j] = c[u];
    }
    return;
  }
  __syncthreads();                     // every chain has read a
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int j = tid + u * nthr;
    if (j < d) a[j] = c[u];
  }
  __syncthreads();
  double ss = 0.0;
  for (int j = lane; j < d; j += 64) ss = fma(a[j], a[j], ss);
  const double nrm = fmax(sqrt(wave_sum(ss)), g.norm_floor);
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int j = tid + u * nthr;
    if (j < d) op[j] = c[u] / nrm;
  }
}

}  // namespace

struct ssn_binder : Lane {
  int dtype = 0;
  int64_t d = 0;
  int M = 0, L = 0, threads = 0;
  int64_t lds_bytes = 0;
  std::vector<int> radix;
  float2* tw = nullptr;
  float2* chirp = nullptr;
  float2* fb = nullptr;
  double kernel_ms = 0.0;      // of the last call

  int64_t row_bytes() const { return 3 * d * 8; }      // two staged operands and the host output, doubles
  int64_t min_scratch() const { return row_bytes(); }
  int64_t chunk_rows() const { return std::min<int64_t>(std::max<int64_t>(1, scratch_bytes / row_bytes()), (int64_t)1 << 30); }

  ~ssn_binder() {
    DevGuard g(device);
    for (float2* p : {tw, chirp, fb}) if (p) (void)hipFree(p);
  }
};

namespace {

int upload(float2** dst, const std::vector<fft::cfloat>& h) {
  SVC_HIP(hipMalloc((void**)dst, h.size() * sizeof(float2)));
  SVC_HIP(hipMemcpy(*dst, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice));
  return SSN_OK;
}

hipError_t launch_bind(ssn_binder* bd, const BindArgs& g, int rows) {
  static std::atomic<uint64_t> configured32{0};
  if (bd->dtype == SSN_F32) {
    if (hipError_t e = ssn::set_max_dynamic_lds_once(reinterpret_cast<const void*>(&k_bind_rows), fft::MAX_LDS_BYTES, configured32); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bind_rows, dim3((unsigned)rows), dim3((unsigned)bd->threads), (size_t)bd->lds_bytes, bd->stream, g);
  } else {
    switch ((int)((bd->d + bd->threads - 1) / bd->threads)) {
#define BIND_DIRECT_CASE(NU)                                                                                                                      \
      case NU: {                                                                                                                                  \
        static std::atomic<uint64_t> configured64{0};                                                                                             \
        if (hipError_t e = ssn::set_max_dynamic_lds_once(reinterpret_cast<const void*>(&k_bind_direct<NU>), BIND_MAX_D64 * 16, configured64);    \
            e != hipSuccess) return e;                                                                                                            \
        hipLaunchKernelGGL((k_bind_direct<NU>), dim3((unsigned)rows), dim3((unsigned)bd->threads), (size_t)bd->lds_bytes, bd->stream, g);        \
        break;                                                                                                                                    \
      }
      BIND_DIRECT_CASE(1) BIND_DIRECT_CASE(2) BIND_DIRECT_CASE(3) BIND_DIRECT_CASE(4) BIND_DIRECT_CASE(5)
      BIND_DIRECT_CASE(6) BIND_DIRECT_CASE(7) BIND_DIRECT_CASE(8) BIND_DIRECT_CASE(9) BIND_DIRECT_CASE(10)
#undef BIND_DIRECT_CASE
      default: return hipErrorInvalidValue;
    }
  }
  return hipGetLastError();
}

struct Operand { const void* p; int on_device, dtype; int64_t ld, count; };

// n / count when `count` pairs with n output rows (1, n, or a divisor of n); 0 otherwise
int64_t pairing(int64_t n, int64_t count) { return count >= 1 && count <= n && n % count == 0 ? n / count : 0; }

int bind(ssn_binder* bd, const char* who, const Operand& a, const Operand& b, int64_t n, int32_t flags, double norm_floor, double* host_out, void* dev_out,
         int64_t out_ld) {
  const int64_t d = bd->d, a_div = pairing(n, a.count), b_div = pairing(n, b.count);
  if (!a_div) return fail(SSN_EINVAL, "%s: %lld rows of a pair with %lld output rows neither as 1, n nor a divisor of n", who, (long long)a.count, (long long)n);
  if (!b_div) return fail(SSN_EINVAL, "%s: %lld rows of b pair with %lld output rows neither as 1, n nor a divisor of n", who, (long long)b.count, (long long)n);
  DevGuard guard(bd->device);
  const int64_t cap = bd->chunk_rows();
  const bool staged = !a.on_device || !b.on_device || host_out;
  char* stage_a = bd->scratch;
  char* stage_b = stage_a + (size_t)cap * d * 8;
  double* stage_out = (double*)(stage_b + (size_t)cap * d * 8);
  const size_t osz = bd->dtype == SSN_F32 ? 4 : 8;
  BindArgs g{};
  g.a_div = a_div; g.b_div = b_div;
  g.a64 = a.dtype == SSN_F64; g.b64 = b.dtype == SSN_F64;
  g.d = (int)d; g.L = bd->L; g.M = bd->M; g.nr = (int)bd->radix.size();
  for (size_t i = 0; i < bd->radix.size(); ++i) g.radix[i] = bd->radix[i];
  g.flags = flags; g.norm_floor = norm_floor;
  g.tw = bd->tw; g.chirp = bd->chirp; g.fb = bd->fb;
  bd->kernel_ms = 0.0;
  bd->launches = 0;
  if (!staged) SVC_HIP(hipEventRecord(bd->ev[0], bd->stream));
  for (int64_t r0 = 0; r0 < n; r0 += cap) {
    const int64_t m = std::min(cap, n - r0);
    const Operand* ops[2] = {&a, &b};
    char* stages[2] = {stage_a, stage_b};
    const int64_t divs[2] = {a_div, b_div};
    const void* ptr[2]; int64_t ld[2], first_row[2];
    for (int o = 0; o < 2; ++o) {
      ptr[o] = ops[o]->p; ld[o] = ops[o]->ld; first_row[o] = 0;
      if (ops[o]->on_device) continue;
      const size_t esz = ops[o]->dtype == SSN_F64 ? 8 : 4;
      const int64_t first = r0 / divs[o], count = (r0 + m - 1) / divs[o] - first + 1;      // count <= m <= cap
      if (const int rc = stage_rows(bd->stream, stages[o], (const char*)ops[o]->p + (size_t)first * ops[o]->ld * esz, ops[o]->ld, d, esz, count)) return rc;
      ptr[o] = stages[o]; ld[o] = d; first_row[o] = first;
    }
    g.a = ptr[0]; g.a_ld = ld[0]; g.a_row0 = first_row[0];
    g.b = ptr[1]; g.b_ld = ld[1]; g.b_row0 = first_row[1];
    g.row0 = r0;
    if (host_out) { g.out = stage_out; g.out_ld = d; g.out64 = 1; }
    else { g.out = (char*)dev_out + (size_t)r0 * out_ld * osz; g.out_ld = out_ld; g.out64 = osz == 8; }
    if (staged) SVC_HIP(hipEventRecord(bd->ev[0], bd->stream));
    SVC_HIP(launch_bind(bd, g, (int)m));
    bd->launches += 1;
    if (!staged) continue;
    SVC_HIP(hipEventRecord(bd->ev[1], bd->stream));
    if (host_out) SVC_HIP(hipMemcpyAsync(host_out + (size_t)r0 * d, stage_out, (size_t)m * d * 8, hipMemcpyDeviceToHost, bd->stream));
    SVC_HIP(hipStreamSynchronize(bd->stream));      // the next chunk reuses the scratch area
    if (const int rc = elapsed(bd->ev[0], bd->ev[1], &bd->kernel_ms)) return rc;
  }
  if (!staged) {
    SVC_HIP(hipEventRecord(bd->ev[1], bd->stream));
    SVC_HIP(hipStreamSynchronize(bd->stream));
    if (const int rc = elapsed(bd->ev[0], bd->ev[1], &bd->kernel_ms)) return rc;
  }
  return SSN_OK;
}

}  // namespace

extern "C" {

int ssn_binder_create(int32_t dtype, int32_t device, int64_t d, int64_t scratch_bytes, ssn_binder** out) {
  if (!out) return fail(SSN_EINVAL, "ssn_binder_create: null handle");
  *out = nullptr;
  if (dtype != SSN_F32 && dtype != SSN_F64) return fail(SSN_EINVAL, "ssn_binder_create: unknown dtype %d", dtype);
  if (d < 2) return fail(SSN_EINVAL, "ssn_binder_create: d %lld below 2", (long long)d);
  std::unique_ptr<ssn_binder> b(new ssn_binder);
  b->dtype = dtype;
  b->d = d;
  if (dtype == SSN_F32) {
    const fft::Route route = d <= BIND_MAX_L ? fft::plan_stockham((int)d, false) : fft::Route{};
    if (!route)
      return fail(SSN_EUNSUPPORTED, "ssn_binder_create: SSN_EUNSUPPORTED: no f32 route for d %lld: a smooth d (prime factors <= 32) up to %d is transformed directly, "
                  "any other through a smooth M >= 2 d - 1 = %lld, and M <= %d points fit in LDS (the f64 binder takes d <= %d)", (long long)d, BIND_MAX_L,
                  (long long)(2 * d - 1), BIND_MAX_L, BIND_MAX_D64);
    b->M = route.M; b->L = route.L; b->radix = route.radix;
    b->threads = fft::threads(route);
    b->lds_bytes = (int64_t)fft::lds_bytes(route);
  } else {
    if (d > BIND_MAX_D64)
      return fail(SSN_EUNSUPPORTED, "ssn_binder_create: SSN_EUNSUPPORTED: d %lld above %d, what the f64 binder holds in LDS (16 B per point)", (long long)d, BIND_MAX_D64);
    b->L = (int)d;
    b->threads = std::min(1024, std::max(64, ((int)d + 63) / 64 * 64));
    b->lds_bytes = d * 16;
  }
  if (const int rc = b->open("ssn_binder_create", device, scratch_bytes, b->min_scratch(), "row of d %lld", (long long)d)) return rc;
  DevGuard g(device);
  if (dtype == SSN_F32) {
    if (const int rc = upload(&b->tw, fft::twiddles(b->L))) return rc;
    if (b->M > 0) {
      if (const int rc = upload(&b->chirp, fft::chirp((int)d))) return rc;
      if (const int rc = upload(&b->fb, fft::chirp_spectrum((int)d, b->M))) return rc;
    }
  }
  *out = b.release();
  return SSN_OK;
}

void ssn_binder_destroy(ssn_binder* binder) { delete binder; }

int ssn_binder_bind(ssn_binder* binder, const double* a, int64_t a_n, const double* b, int64_t b_n, int64_t n, int32_t flags, double norm_floor, double* out) {
  const char* who = "ssn_binder_bind";
  if (!binder) return fail(SSN_EINVAL, "%s: null binder", who);
  if (n < 0) return fail(SSN_EINVAL, "%s: negative n", who);
  if (flags & ~7) return fail(SSN_EINVAL, "%s: unknown flags %d", who, flags);
  if (n == 0) return SSN_OK;
  if (!a || !b || !out) return fail(SSN_EINVAL, "%s: null argument", who);
  return bind(binder, who, Operand{a, 0, SSN_F64, binder->d, a_n}, Operand{b, 0, SSN_F64, binder->d, b_n}, n, flags, norm_floor, out, nullptr, binder->d);
}

int ssn_binder_bind_device(ssn_binder* binder, const void* a, int32_t a_on_device, int32_t a_dtype, int64_t a_ld, int64_t a_n, const void* b,
                           int32_t b_on_device, int32_t b_dtype, int64_t b_ld, int64_t b_n, int64_t n, int32_t flags, double norm_floor, void* out_dev,
                           int64_t out_ld) {
  const char* who = "ssn_binder_bind_device";
  if (!binder) return fail(SSN_EINVAL, "%s: null binder", who);
  if (n < 0) return fail(SSN_EINVAL, "%s: negative n", who);
  if (flags & ~7) return fail(SSN_EINVAL, "%s: unknown flags %d", who, flags);
  if (const int rc = check_rows(who, "a", a_dtype, a_ld, binder->d, " of a")) return rc;
  if (const int rc = check_rows(who, "b", b_dtype, b_ld, binder->d, " of b")) return rc;
  if (out_ld < binder->d) return fail(SSN_EINVAL, "%s: leading dimension %lld of the output below the width %lld", who, (long long)out_ld, (long long)binder->d);
  if (n == 0) return SSN_OK;
  if (!a || !b || !out_dev) return fail(SSN_EINVAL, "%s: null argument", who);
  return bind(binder, who, Operand{a, a_on_device != 0, a_dtype, a_ld, a_n}, Operand{b, b_on_device != 0, b_dtype, b_ld, b_n}, n, flags, norm_floor, nullptr,
              out_dev, out_ld);
}

int ssn_binder_get_info(ssn_binder* binder, int64_t n, ssn_binder_info* out) {
  if (!binder || !out || n < 0) return fail(SSN_EINVAL, "ssn_binder_get_info: null argument");
  const int64_t cap = binder->chunk_rows();
  out->row_chunk = cap;
  out->n_chunks = (n + cap - 1) / cap;
  out->scratch_bytes = binder->scratch_bytes;
  out->min_scratch_bytes = binder->min_scratch();
  out->d = binder->d;
  out->transform_length = binder->L;
  out->bluestein_m = binder->M;
  out->n_radices = (int64_t)binder->radix.size();
  for (int i = 0; i < 12; ++i) out->radices[i] = i < (int)binder->radix.size() ? binder->radix[i] : 0;
  out->threads = binder->threads;
  out->lds_bytes = binder->lds_bytes;
  out->last_launches = binder->launches;
  out->last_kernel_ms = binder->kernel_ms;
  return SSN_OK;
}

}  // extern "C"
