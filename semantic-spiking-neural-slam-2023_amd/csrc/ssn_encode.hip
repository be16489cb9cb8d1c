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

using namespace ssn::svc;      // fail, SVC_HIP, DevGuard, check_device

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

struct ssn_encoder {
  int dtype = 0, device = 0;
  int64_t d = 0, K = 0, Kp = 0, dim = 0, scratch_bytes = 0;
  size_t esz = 4;
  double* M = nullptr;             // (K x dim)
  void* B = nullptr;               // (d x Kp) in the encoder's dtype
  char* scratch = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
  double phase_ms = 0.0, product_ms = 0.0;      // of the last encode call
  int64_t launches = 0;

  int64_t row_bytes() const { return dim * 8 + Kp * (int64_t)esz + d * (int64_t)esz + (esz == 4 ? d * 8 : 0); }
  int64_t min_scratch() const { return ROWS * row_bytes(); }
  // rows per chunk: whole tiles that fit, bounded so that the 32-bit sizes of the kernels hold
  int64_t chunk_rows() const {
    int64_t tiles = std::max<int64_t>(1, scratch_bytes / (ROWS * row_bytes()));
    const int64_t widest = std::max(Kp, d);
    tiles = std::min<int64_t>(tiles, std::max<int64_t>(1, ((int64_t)1 << 30) / (ROWS * widest)));
    return std::min<int64_t>(tiles, 1 << 15) * ROWS;
  }

  ~ssn_encoder() {
    DevGuard g(device);
    for (hipEvent_t e : {e0, e1, e2}) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    if (M) (void)hipFree(M);
    if (B) (void)hipFree(B);
    if (scratch) (void)hipFree(scratch);
  }
};

namespace {

struct Areas {      // the regions of the scratch area for a chunk capacity of `rows` points
  char* stage; double* wide; void* P; void* out;
  Areas(const ssn_encoder* e, int64_t rows) {
    char* p = e->scratch;
    stage = p; p += (size_t)rows * e->dim * 8;
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

template <typename T>
hipError_t phase_for(ssn_encoder* e, const void* pts, int pts_dtype, int64_t ld, int n, T* P) {
  return pts_dtype == SSN_F32 ? launch_phase<float, T>(e, (const float*)pts, ld, n, P) : launch_phase<double, T>(e, (const double*)pts, ld, n, P);
}

template <typename TO>
hipError_t launch_product64(ssn_encoder* e, const double* P, int n, TO* C, int64_t ldc) {
  hipLaunchKernelGGL((k_encode_product<TO>), dim3((unsigned)((e->d + ROWS - 1) / ROWS), (unsigned)((n + ROWS - 1) / ROWS)), dim3(256), 0, e->stream, P,
                     (const double*)e->B, (int)e->Kp, n, (int)e->d, C, (long long)ldc);
  return hipGetLastError();
}

// Points: host (on_device == 0) or device rows of pts_dtype with leading dimension pts_ld.  Output: host doubles (dense), or a device
// buffer of out_dtype with leading dimension out_ld.
int encode(ssn_encoder* e, const void* pts, int on_device, int pts_dtype, int64_t pts_ld, int64_t n, double* host_out, void* dev_out, int out_dtype,
           int64_t out_ld) {
  DevGuard g(e->device);
  const int64_t cap = e->chunk_rows();
  const Areas a(e, cap);
  const size_t isz = pts_dtype == SSN_F32 ? 4 : 8, osz = out_dtype == SSN_F32 ? 4 : 8;
  const bool f32 = e->dtype == SSN_F32;
  e->phase_ms = e->product_ms = 0.0;
  e->launches = 0;
  for (int64_t r0 = 0; r0 < n; r0 += cap) {
    const int m = (int)std::min(cap, n - r0);
    const void* src = (const char*)pts + (size_t)r0 * pts_ld * isz;
    int64_t ld = pts_ld;
    if (!on_device) {
      if (pts_ld == e->dim) SVC_HIP(hipMemcpyAsync(a.stage, src, (size_t)m * e->dim * isz, hipMemcpyHostToDevice, e->stream));
      else SVC_HIP(hipMemcpy2DAsync(a.stage, (size_t)e->dim * isz, src, (size_t)pts_ld * isz, (size_t)e->dim * isz, (size_t)m, hipMemcpyHostToDevice, e->stream));
      src = a.stage;
      ld = e->dim;
    }
    SVC_HIP(hipEventRecord(e->e0, e->stream));
    if (f32) SVC_HIP(phase_for<float>(e, src, pts_dtype, ld, m, (float*)a.P));
    else SVC_HIP(phase_for<double>(e, src, pts_dtype, ld, m, (double*)a.P));
    SVC_HIP(hipEventRecord(e->e1, e->stream));
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
    SVC_HIP(hipEventRecord(e->e2, e->stream));
    if (host_out)
      SVC_HIP(hipMemcpyAsync(host_out + (size_t)r0 * e->d, f32 ? (const void*)a.wide : (const void*)a.out, (size_t)m * e->d * 8, hipMemcpyDeviceToHost, e->stream));
    SVC_HIP(hipStreamSynchronize(e->stream));      // the next chunk reuses the scratch area
    float ms = 0.0f;
    SVC_HIP(hipEventElapsedTime(&ms, e->e0, e->e1));
    e->phase_ms += ms;
    SVC_HIP(hipEventElapsedTime(&ms, e->e1, e->e2));
    e->product_ms += ms;
  }
  return SSN_OK;
}

}  // namespace

namespace ssn {

int encoder_encode_into(ssn_encoder* enc, const double* points, int64_t n, void* out_dev, int32_t out_dtype, int64_t out_ld) {
  if (!enc || !points || !out_dev || n <= 0) return fail(SSN_EINVAL, "encoder_encode_into: null or empty argument");
  if (out_ld < enc->d) return fail(SSN_EINVAL, "encoder_encode_into: leading dimension %lld below the width %lld", (long long)out_ld, (long long)enc->d);
  if (enc->dtype == SSN_F32 && out_dtype != SSN_F32) return fail(SSN_EINVAL, "encoder_encode_into: an f32 encoder writes f32 only");
  return encode(enc, points, 0, SSN_F64, enc->dim, n, nullptr, out_dev, out_dtype, out_ld);
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
  if (scratch_bytes < 0) return fail(SSN_EINVAL, "ssn_encoder_create: negative scratch_bytes");
  std::unique_ptr<ssn_encoder> e(new ssn_encoder);
  e->dtype = dtype;
  e->device = device;
  e->esz = dtype == SSN_F32 ? 4 : 8;
  e->d = d;
  e->K = K;
  e->dim = dim;
  e->Kp = (2 * K + KPAD - 1) / KPAD * KPAD;
  e->scratch_bytes = scratch_bytes ? scratch_bytes : std::max<int64_t>((int64_t)64 << 20, e->min_scratch());
  if (e->scratch_bytes < e->min_scratch())
    return fail(SSN_EINVAL, "ssn_encoder_create: scratch_bytes %lld too small for one %d-point tile of d %lld, K %lld (%lld bytes)", (long long)scratch_bytes,
                ROWS, (long long)d, (long long)K, (long long)e->min_scratch());
  if (const int rc = check_device("ssn_encoder_create", device)) return rc;
  DevGuard g(device);
  SVC_HIP(hipStreamCreate(&e->stream));
  SVC_HIP(hipEventCreate(&e->e0));
  SVC_HIP(hipEventCreate(&e->e1));
  SVC_HIP(hipEventCreate(&e->e2));
  SVC_HIP(hipMalloc((void**)&e->scratch, (size_t)e->scratch_bytes));
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
  return encode(enc, points, 0, SSN_F64, enc->dim, n, out, nullptr, SSN_F64, enc->d);
}

int ssn_encoder_encode_device(ssn_encoder* enc, const void* points, int32_t points_on_device, int32_t points_dtype, int64_t points_ld, int64_t n,
                              void* out_dev, int64_t out_ld) {
  if (!enc) return fail(SSN_EINVAL, "ssn_encoder_encode_device: null encoder");
  if (n < 0) return fail(SSN_EINVAL, "ssn_encoder_encode_device: negative n");
  if (points_dtype != SSN_F32 && points_dtype != SSN_F64) return fail(SSN_EINVAL, "ssn_encoder_encode_device: unknown points_dtype %d", points_dtype);
  if (points_ld < enc->dim)
    return fail(SSN_EINVAL, "ssn_encoder_encode_device: leading dimension %lld of the points below dim %lld", (long long)points_ld, (long long)enc->dim);
  if (out_ld < enc->d) return fail(SSN_EINVAL, "ssn_encoder_encode_device: leading dimension %lld of the output below the width %lld", (long long)out_ld, (long long)enc->d);
  if (out_ld > INT32_MAX) return fail(SSN_EINVAL, "ssn_encoder_encode_device: leading dimension %lld of the output above 2^31 - 1", (long long)out_ld);
  if (n == 0) return SSN_OK;
  if (!points || !out_dev) return fail(SSN_EINVAL, "ssn_encoder_encode_device: null argument");
  return encode(enc, points, points_on_device != 0, points_dtype, points_ld, n, nullptr, out_dev, enc->dtype, out_ld);
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
