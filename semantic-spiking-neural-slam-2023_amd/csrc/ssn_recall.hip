// ssn_recall.hip - recall of a learned associative memory on the device, behind ssn_recall_* (include/ssn.h).
//
// Not on the step path and never in the step graph: it runs on the simulator's own stream between two ssn_run_steps calls and
// reads the two matrices the learning rules update where they lie - E, the scaled encoders k_voja moves (row-major [n][ld]), and
// W, the decoders k_pes moves (row-major [d_val][ld], or neuron-major [n][ldt] where the plan made them spike-sparse).  For L key
// rows V (reference experiments/slam_map_new.py:342-347, run_slam_map_gif.py:323-329; harness.map_recall_learned is the host
// definition):
//   J[l][m] = s[m] (V[l] . E[m]) + bias[m]      a[l][m] = rate(J[l][m])      q[l][r] = sum_m W[r][m] a[l][m]
//
// f32 (v_mfma_f32_32x32x2_f32; 256 threads = 2 x 2 waves, one 32 x 32 accumulator per wave, k in slabs of 32 through LDS with the
// next slab prefetched into registers, as k_decode_tiles):
//   k_recall_act      64 keys x 64 neurons per workgroup over the whole key width; scale, bias and the rate function in the
//                     epilogue, so J is never stored.  Every J is one k-ordered chain.  The activities go to an L x n matrix in HBM
//                     (2.6 MB at L = 50, n = 10 150, against 41 MB of E), zero for neurons >= n.  E is guarded by row < n and
//                     column < d_key: what the padding of a row holds is never multiplied.  E is read once for L <= 64.
//   k_recall_partial  64 keys x 64 outputs per workgroup over ONE chunk of 256 neurons: a k-ordered chain from zero, written as
//                     the chunk's partial sum with plain stores.  <false> reads W row-major, <true> neuron-major; both guard
//                     row < d_val and neuron < n.  W is read once for L <= 64.
//   k_recall_finish   one thread per output: the chunk partials added in ascending chunk order.  When the scratch area holds
//                     fewer partials than there are chunks the chunks go in passes and the running sum carries on from pass to
//                     pass - the same additions in the same order, so the result does not depend on the scratch size.  No atomics.
// f64 (parity mode): k_recall_act_ordered / k_recall_dec_ordered, one thread per output, plain ordered sums.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>
#include "../../include/ssn.h"
#include "ssn_recall.hpp"
#include "ssn_service.hpp"

using namespace ssn::svc;      // fail, SVC_HIP, DevGuard, check_device

namespace {

constexpr int TL = 64;        // key rows of a tile
constexpr int TN = 64;        // neurons (k_recall_act) or outputs (k_recall_partial) of a tile
constexpr int BK = 32;        // slab of the inner dimension
constexpr int LD = BK + 1;
constexpr int CH = 256;       // neurons per partial sum of the decoder product
constexpr int RPT = TL * BK / 256;      // slab elements per thread and operand

typedef float acc_t __attribute__((ext_vector_type(16)));
__device__ __forceinline__ int acc_row(int v, int lane) { return (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5); }

struct RateParams { int neuron; double tau_rc, tau_ref, amplitude; };

__device__ __forceinline__ float rate_of(float J, int neuron, float tau_rc, float tau_ref, float amp) {
  if (neuron == SSN_RELU) return amp * fmaxf(J, 0.0f);
  return J > 1.0f ? amp / (tau_ref + tau_rc * log1pf(1.0f / (J - 1.0f))) : 0.0f;
}
__device__ __forceinline__ double rate_of(double J, int neuron, double tau_rc, double tau_ref, double amp) {
  if (neuron == SSN_RELU) return amp * fmax(J, 0.0);
  return J > 1.0 ? amp / (tau_ref + tau_rc * log1p(1.0 / (J - 1.0))) : 0.0;
}

__global__ __launch_bounds__(256) void k_recall_act(const float* __restrict__ keys, int Kp, const float* __restrict__ E, long long ldE, int n, int d_key,
                                                    const float* __restrict__ scale, const float* __restrict__ bias, int neuron, float tau_rc, float tau_ref,
                                                    float amp, float* __restrict__ act, long long n_ld) {
  __shared__ float Vs[TL][LD];
  __shared__ float Es[TN][LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wl = wave >> 1, wn = wave & 1, mn = lane & 31, lk = lane >> 5;
  const int m0 = blockIdx.x * TN, l0 = blockIdx.y * TL;
  const int lr = tid / BK, lc = tid % BK;
  float rv[RPT], re[RPT];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int row = lr + (256 / BK) * i;
      rv[i] = keys[(size_t)(l0 + row) * Kp + k0 + lc];      // (padded to whole tiles with zeros: no guard)
      const int m = m0 + row, k = k0 + lc;
      re[i] = (m < n && k < d_key) ? E[(size_t)m * ldE + k] : 0.0f;
    }
  };
  acc_t acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
  const float* vp = &Vs[wl * 32 + mn][lk];
  const float* ep = &Es[wn * 32 + mn][lk];
  fetch(0);
  for (int k0 = 0; k0 < Kp; k0 += BK) {
#pragma unroll
    for (int i = 0; i < RPT; ++i) { Vs[lr + (256 / BK) * i][lc] = rv[i]; Es[lr + (256 / BK) * i][lc] = re[i]; }
    __syncthreads();
    if (k0 + BK < Kp) fetch(k0 + BK);
#pragma unroll 4
    for (int kk = 0; kk < BK; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[kk], ep[kk], acc, 0, 0, 0);
    __syncthreads();
  }
  const int m = m0 + wn * 32 + mn;      // < n_ld: the grid covers n_ld / TN tiles
  const bool live = m < n;
  const float s = live ? scale[m] : 0.0f, b = live ? bias[m] : 0.0f;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int l = l0 + wl * 32 + acc_row(v, lane);
    const float J = fmaf(s, acc[v], b);
    act[(size_t)l * n_ld + m] = live ? rate_of(J, neuron, tau_rc, tau_ref, amp) : 0.0f;
  }
}

template <bool TR>
__global__ __launch_bounds__(256) void k_recall_partial(const float* __restrict__ act, long long n_ld, const float* __restrict__ W, long long ldw, int n, int d_val,
                                                        int chunk0, float* __restrict__ part, int dvp, int Lp) {
  __shared__ float As[TL][LD];
  __shared__ float Ws[TN][LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wl = wave >> 1, wn = wave & 1, mn = lane & 31, lk = lane >> 5;
  const int r0 = blockIdx.x * TN, l0 = blockIdx.z * TL;
  const int mbeg = (chunk0 + (int)blockIdx.y) * CH;      // mbeg + CH <= n_ld
  const int lr = tid / BK, lc = tid % BK;
  const int tr_r = tid & 63, tr_k = tid >> 6;      // neuron-major W: 64 consecutive outputs of one neuron per wave
  float ra[RPT], rw[RPT];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int row = lr + (256 / BK) * i;
      ra[i] = act[(size_t)(l0 + row) * n_ld + mbeg + k0 + lc];      // (zero for neurons >= n and allocated up to n_ld: no guard)
      if (TR) {
        const int r = r0 + tr_r, m = mbeg + k0 + tr_k + 4 * i;
        rw[i] = (r < d_val && m < n) ? W[(size_t)m * ldw + r] : 0.0f;
      } else {
        const int r = r0 + row, m = mbeg + k0 + lc;
        rw[i] = (r < d_val && m < n) ? W[(size_t)r * ldw + m] : 0.0f;
      }
    }
  };
  acc_t acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
  const float* ap = &As[wl * 32 + mn][lk];
  const float* wp = &Ws[wn * 32 + mn][lk];
  fetch(0);
  for (int k0 = 0; k0 < CH; k0 += BK) {
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      As[lr + (256 / BK) * i][lc] = ra[i];
      if (TR) Ws[tr_r][tr_k + 4 * i] = rw[i];
      else Ws[lr + (256 / BK) * i][lc] = rw[i];
    }
    __syncthreads();
    if (k0 + BK < CH) fetch(k0 + BK);
#pragma unroll 4
    for (int kk = 0; kk < BK; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], wp[kk], acc, 0, 0, 0);
    __syncthreads();
  }
  float* p = part + (size_t)blockIdx.y * Lp * dvp;
  const int r = r0 + wn * 32 + mn;      // < dvp
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int l = l0 + wl * 32 + acc_row(v, lane);      // < Lp
    p[(size_t)l * dvp + r] = acc[v];
  }
}

__global__ __launch_bounds__(256) void k_recall_finish(const float* __restrict__ part, int n_slots, long long slot_elems, int dvp, int L, int d_val, int first,
                                                       float* __restrict__ qacc, double* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)L * d_val) return;
  const int l = (int)(idx / d_val), r = (int)(idx % d_val);
  const size_t at = (size_t)l * dvp + r;
  float acc = first ? 0.0f : qacc[at];
  for (int s = 0; s < n_slots; ++s) acc += part[(size_t)s * slot_elems + at];
  qacc[at] = acc;
  out[idx] = (double)acc;
}

// parity mode: one thread per activity / per output, the sums in index order
__global__ __launch_bounds__(256) void k_recall_act_ordered(const double* __restrict__ keys, int Kp, const double* __restrict__ E, long long ldE, int n, int d_key,
                                                            const double* __restrict__ scale, const double* __restrict__ bias, int neuron, double tau_rc,
                                                            double tau_ref, double amp, double* __restrict__ act, long long n_ld) {
  const int m = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
  if (m >= n) return;
  const double* __restrict__ v = keys + (size_t)l * Kp;
  const double* __restrict__ e = E + (size_t)m * ldE;
  double dot = 0.0;
  for (int k = 0; k < d_key; ++k) dot += v[k] * e[k];
  act[(size_t)l * n_ld + m] = rate_of(scale[m] * dot + bias[m], neuron, tau_rc, tau_ref, amp);
}

__global__ __launch_bounds__(256) void k_recall_dec_ordered(const double* __restrict__ act, long long n_ld, const double* __restrict__ W, long long ldw, int tr, int n,
                                                            int d_val, double* __restrict__ out) {
  const int r = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
  if (r >= d_val) return;
  const double* __restrict__ a = act + (size_t)l * n_ld;
  double acc = 0.0;
  if (tr) for (int m = 0; m < n; ++m) acc += W[(size_t)m * ldw + r] * a[m];
  else for (int m = 0; m < n; ++m) acc += W[(size_t)r * ldw + m] * a[m];
  out[(size_t)l * d_val + r] = acc;
}

}  // namespace

namespace {

int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

}  // namespace

struct ssn_recall {
  ssn_sim* sim = nullptr;
  int enc_buffer = 0, dec_buffer = 0, dtype = 0, device = 0;
  size_t esz = 4;
  int64_t n = 0, d_key = 0, d_val = 0, L = 0;
  int64_t Kp = 0, Lp = 0, n_ld = 0, dvp = 0, n_chunks = 0, scratch_bytes = 0;
  RateParams rp{};
  void *scale = nullptr, *bias = nullptr;      // n values each, the simulator's dtype
  void *keys = nullptr, *act = nullptr;        // [Lp][Kp], [Lp][n_ld]
  float *part = nullptr, *qacc = nullptr;      // f32: chunk partials (the scratch area), running sums [Lp][dvp]
  double* out = nullptr;                       // [L][d_val]
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double kernel_ms = 0.0;
  int64_t launches = 0;
  int last_transposed = 0;
  bool scratch_default = false;                // scratch_bytes == 0 at creation: the area follows the number of keys

  int64_t partial_bytes() const { return Lp * dvp * 4; }
  int64_t chunks_per_pass() const { return std::max<int64_t>(1, std::min(n_chunks, scratch_bytes / std::max<int64_t>(1, partial_bytes()))); }

  void drop_keys() {
    for (void* p : {keys, act, (void*)qacc, (void*)out}) if (p) (void)hipFree(p);
    keys = act = nullptr; qacc = nullptr; out = nullptr;
    L = Lp = 0;
  }
  ~ssn_recall() {
    DevGuard g(device);
    drop_keys();
    for (void* p : {scale, bias, (void*)part}) if (p) (void)hipFree(p);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

namespace {

template <typename T>
int upload_vec(void** dst, const double* src, int64_t count) {
  std::vector<T> h((size_t)count);
  for (int64_t i = 0; i < count; ++i) h[(size_t)i] = (T)src[i];
  SVC_HIP(hipMalloc(dst, (size_t)count * sizeof(T)));
  SVC_HIP(hipMemcpy(*dst, h.data(), (size_t)count * sizeof(T), hipMemcpyHostToDevice));
  return SSN_OK;
}

template <typename T>
int set_keys(ssn_recall* rc, const double* keys, int64_t L) {
  const int64_t Lp = round_up(L, TL);
  if (sizeof(T) == 4 && rc->scratch_default) {      // all partial sums, up to 64 MB; one at the least
    const int64_t one = Lp * rc->dvp * 4, want = std::max(one, std::min<int64_t>(one * rc->n_chunks, (int64_t)64 << 20));
    if (want != rc->scratch_bytes || !rc->part) {
      if (rc->part) (void)hipFree(rc->part);
      rc->part = nullptr;
      rc->scratch_bytes = 0;
      SVC_HIP(hipMalloc((void**)&rc->part, (size_t)want));
      rc->scratch_bytes = want;
    }
  }
  if (sizeof(T) == 4 && Lp * rc->dvp * 4 > rc->scratch_bytes)
    return fail(SSN_EINVAL, "ssn_recall: the scratch area of %lld bytes does not hold one partial sum of %lld key rows (%lld bytes)", (long long)rc->scratch_bytes,
                (long long)L, (long long)(Lp * rc->dvp * 4));
  if (Lp != rc->Lp) {
    rc->drop_keys();
    SVC_HIP(hipMalloc(&rc->keys, (size_t)(Lp * rc->Kp) * sizeof(T)));
    SVC_HIP(hipMalloc(&rc->act, (size_t)(Lp * rc->n_ld) * sizeof(T)));
    SVC_HIP(hipMemset(rc->act, 0, (size_t)(Lp * rc->n_ld) * sizeof(T)));
    if (sizeof(T) == 4) SVC_HIP(hipMalloc((void**)&rc->qacc, (size_t)(Lp * rc->dvp) * 4));
    rc->Lp = Lp;
  } else if (rc->out) {
    (void)hipFree(rc->out);
    rc->out = nullptr;
  }
  SVC_HIP(hipMalloc((void**)&rc->out, (size_t)(L * rc->d_val) * 8));
  std::vector<T> h((size_t)(Lp * rc->Kp), T(0));
  for (int64_t l = 0; l < L; ++l)
    for (int64_t k = 0; k < rc->d_key; ++k) h[(size_t)(l * rc->Kp + k)] = (T)keys[l * rc->d_key + k];
  SVC_HIP(hipMemcpy(rc->keys, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  rc->L = L;
  return SSN_OK;
}

// the two matrices as the simulator holds them now; their shapes were checked at creation and cannot change
int views(ssn_recall* rc, ssn::BufView* e, ssn::BufView* w) {
  int st = ssn::sim_buffer_view(rc->sim, rc->enc_buffer, e);
  if (st != SSN_OK) return st;
  st = ssn::sim_buffer_view(rc->sim, rc->dec_buffer, w);
  if (st != SSN_OK) return st;
  if (e->transposed || e->rows != rc->n || e->cols != rc->d_key)
    return fail(SSN_EINVAL, "ssn_recall: buffer %d is not a row-major %lld x %lld encoder matrix (%lld x %lld%s)", rc->enc_buffer, (long long)rc->n,
                (long long)rc->d_key, (long long)e->rows, (long long)e->cols, e->transposed ? ", neuron-major" : "");
  if (w->rows != rc->d_val || w->cols != rc->n)
    return fail(SSN_EINVAL, "ssn_recall: buffer %d is not a %lld x %lld decoder matrix (%lld x %lld)", rc->dec_buffer, (long long)rc->d_val, (long long)rc->n,
                (long long)w->rows, (long long)w->cols);
  if (e->dtype != rc->dtype || w->dtype != rc->dtype) return fail(SSN_EINVAL, "ssn_recall: the simulator's dtype changed");
  return SSN_OK;
}

int run_f32(ssn_recall* rc, const ssn::BufView& e, const ssn::BufView& w, hipStream_t st) {
  const RateParams& rp = rc->rp;
  hipLaunchKernelGGL(k_recall_act, dim3((unsigned)(rc->n_ld / TN), (unsigned)(rc->Lp / TL)), dim3(256), 0, st, (const float*)rc->keys, (int)rc->Kp,
                     (const float*)e.d, (long long)e.ld, (int)rc->n, (int)rc->d_key, (const float*)rc->scale, (const float*)rc->bias, rp.neuron,
                     (float)rp.tau_rc, (float)rp.tau_ref, (float)rp.amplitude, (float*)rc->act, (long long)rc->n_ld);
  SVC_HIP(hipGetLastError());
  rc->launches = 1;
  const int64_t cpp = rc->chunks_per_pass();
  const long long ldw = w.transposed ? w.ldt : w.ld;
  for (int64_t c0 = 0; c0 < rc->n_chunks; c0 += cpp) {
    const int nc = (int)std::min(cpp, rc->n_chunks - c0);
    const dim3 grid((unsigned)(rc->dvp / TN), (unsigned)nc, (unsigned)(rc->Lp / TL));
    if (w.transposed)
      hipLaunchKernelGGL(k_recall_partial<true>, grid, dim3(256), 0, st, (const float*)rc->act, (long long)rc->n_ld, (const float*)w.d, ldw, (int)rc->n,
                         (int)rc->d_val, (int)c0, rc->part, (int)rc->dvp, (int)rc->Lp);
    else
      hipLaunchKernelGGL(k_recall_partial<false>, grid, dim3(256), 0, st, (const float*)rc->act, (long long)rc->n_ld, (const float*)w.d, ldw, (int)rc->n,
                         (int)rc->d_val, (int)c0, rc->part, (int)rc->dvp, (int)rc->Lp);
    SVC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_recall_finish, dim3((unsigned)((rc->L * rc->d_val + 255) / 256)), dim3(256), 0, st, (const float*)rc->part, nc,
                       (long long)(rc->Lp * rc->dvp), (int)rc->dvp, (int)rc->L, (int)rc->d_val, c0 == 0 ? 1 : 0, rc->qacc, rc->out);
    SVC_HIP(hipGetLastError());
    rc->launches += 2;
  }
  return SSN_OK;
}

int run_f64(ssn_recall* rc, const ssn::BufView& e, const ssn::BufView& w, hipStream_t st) {
  const RateParams& rp = rc->rp;
  hipLaunchKernelGGL(k_recall_act_ordered, dim3((unsigned)((rc->n + 255) / 256), (unsigned)rc->L), dim3(256), 0, st, (const double*)rc->keys, (int)rc->Kp,
                     (const double*)e.d, (long long)e.ld, (int)rc->n, (int)rc->d_key, (const double*)rc->scale, (const double*)rc->bias, rp.neuron, rp.tau_rc,
                     rp.tau_ref, rp.amplitude, (double*)rc->act, (long long)rc->n_ld);
  SVC_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_recall_dec_ordered, dim3((unsigned)((rc->d_val + 255) / 256), (unsigned)rc->L), dim3(256), 0, st, (const double*)rc->act,
                     (long long)rc->n_ld, (const double*)w.d, (long long)(w.transposed ? w.ldt : w.ld), w.transposed, (int)rc->n, (int)rc->d_val, rc->out);
  SVC_HIP(hipGetLastError());
  rc->launches = 2;
  return SSN_OK;
}

}  // namespace

extern "C" {

int ssn_recall_create(ssn_sim* sim, int32_t enc_buffer, int32_t dec_buffer, int64_t n, int64_t d_key, int64_t d_val, const double* scale,
                      const double* bias, int32_t neuron, double tau_rc, double tau_ref, double amplitude, const double* keys, int64_t n_keys,
                      int64_t scratch_bytes, ssn_recall** out) {
  if (!out) return fail(SSN_EINVAL, "ssn_recall_create: null handle");
  *out = nullptr;
  if (!scale || !bias || !keys) return fail(SSN_EINVAL, "ssn_recall_create: null argument");
  if (n_keys <= 0 || n_keys > 65536 * (int64_t)TL / 2) return fail(SSN_EINVAL, "ssn_recall_create: %lld key rows outside 1 .. 2^21", (long long)n_keys);
  if (n <= 0 || n > (1 << 24) || d_key <= 0 || d_key > (1 << 20) || d_val <= 0 || d_val > (1 << 20))
    return fail(SSN_EINVAL, "ssn_recall_create: shape n = %lld, d_key = %lld, d_val = %lld outside 1 .. 2^24, 2^20, 2^20", (long long)n, (long long)d_key,
                (long long)d_val);
  if (neuron != SSN_LIF && neuron != SSN_LIFRATE && neuron != SSN_RELU) return fail(SSN_EINVAL, "ssn_recall_create: unknown neuron type %d", neuron);
  if (scratch_bytes < 0) return fail(SSN_EINVAL, "ssn_recall_create: negative scratch_bytes");
  if (const int rc = check_device(nullptr, 0)) return rc;      // the device is the simulator's: only the count is tested, and before `sim`
  if (!sim) return fail(SSN_EINVAL, "ssn_recall_create: null simulator");
  std::unique_ptr<ssn_recall> rc(new ssn_recall);
  rc->sim = sim;
  rc->enc_buffer = enc_buffer; rc->dec_buffer = dec_buffer;
  rc->n = n; rc->d_key = d_key; rc->d_val = d_val;
  rc->rp = RateParams{neuron, tau_rc, tau_ref, amplitude};
  ssn::BufView e, w;
  int st = ssn::sim_buffer_view(sim, enc_buffer, &e);
  if (st != SSN_OK) return st;
  rc->dtype = e.dtype; rc->device = e.device;
  rc->esz = e.dtype == SSN_F32 ? 4 : 8;
  st = views(rc.get(), &e, &w);
  if (st != SSN_OK) return st;
  rc->Kp = round_up(d_key, BK);
  rc->n_ld = round_up(n, CH);
  rc->dvp = round_up(d_val, TN);
  rc->n_chunks = rc->n_ld / CH;
  DevGuard g(rc->device);
  SVC_HIP(hipEventCreate(&rc->e0));
  SVC_HIP(hipEventCreate(&rc->e1));
  st = rc->dtype == SSN_F32 ? upload_vec<float>(&rc->scale, scale, n) : upload_vec<double>(&rc->scale, scale, n);
  if (st == SSN_OK) st = rc->dtype == SSN_F32 ? upload_vec<float>(&rc->bias, bias, n) : upload_vec<double>(&rc->bias, bias, n);
  if (st != SSN_OK) return st;
  rc->scratch_default = scratch_bytes == 0;
  if (rc->dtype == SSN_F32 && !rc->scratch_default) {
    const int64_t one = round_up(n_keys, TL) * rc->dvp * 4;
    if (scratch_bytes < one)
      return fail(SSN_EINVAL, "ssn_recall_create: scratch_bytes %lld too small for one partial sum of %lld key rows (%lld bytes)", (long long)scratch_bytes,
                  (long long)n_keys, (long long)one);
    SVC_HIP(hipMalloc((void**)&rc->part, (size_t)scratch_bytes));
    rc->scratch_bytes = scratch_bytes;
  }
  st = rc->dtype == SSN_F32 ? set_keys<float>(rc.get(), keys, n_keys) : set_keys<double>(rc.get(), keys, n_keys);
  if (st != SSN_OK) return st;
  *out = rc.release();
  return SSN_OK;
}

void ssn_recall_destroy(ssn_recall* rc) { delete rc; }

int ssn_recall_set_keys(ssn_recall* rc, const double* keys, int64_t n_keys) {
  if (!rc) return fail(SSN_EINVAL, "ssn_recall_set_keys: null handle");
  if (!keys) return fail(SSN_EINVAL, "ssn_recall_set_keys: null argument");
  if (n_keys <= 0 || n_keys > 65536 * (int64_t)TL / 2) return fail(SSN_EINVAL, "ssn_recall_set_keys: %lld key rows outside 1 .. 2^21", (long long)n_keys);
  DevGuard g(rc->device);
  return rc->dtype == SSN_F32 ? set_keys<float>(rc, keys, n_keys) : set_keys<double>(rc, keys, n_keys);
}

int ssn_recall_run(ssn_recall* rc, double* dst) {
  if (!rc) return fail(SSN_EINVAL, "ssn_recall_run: null handle");
  if (!dst) return fail(SSN_EINVAL, "ssn_recall_run: null argument");
  if (!rc->L) return fail(SSN_EINVAL, "ssn_recall_run: no keys");
  ssn::BufView e, w;
  int st = views(rc, &e, &w);
  if (st != SSN_OK) return st;
  DevGuard g(rc->device);
  hipStream_t s = e.stream;
  SVC_HIP(hipEventRecord(rc->e0, s));
  st = rc->dtype == SSN_F32 ? run_f32(rc, e, w, s) : run_f64(rc, e, w, s);
  if (st != SSN_OK) return st;
  SVC_HIP(hipEventRecord(rc->e1, s));
  SVC_HIP(hipMemcpyAsync(dst, rc->out, (size_t)(rc->L * rc->d_val) * 8, hipMemcpyDeviceToHost, s));
  SVC_HIP(hipStreamSynchronize(s));
  float ms = 0.0f;
  SVC_HIP(hipEventElapsedTime(&ms, rc->e0, rc->e1));
  rc->kernel_ms = ms;
  rc->last_transposed = w.transposed;
  return SSN_OK;
}

int ssn_recall_get_info(ssn_recall* rc, ssn_recall_info* out) {
  if (!rc || !out) return fail(SSN_EINVAL, "ssn_recall_get_info: null argument");
  out->n = rc->n; out->d_key = rc->d_key; out->d_val = rc->d_val; out->n_keys = rc->L;
  out->padded_keys = rc->Lp;
  out->chunk = CH;
  out->n_chunks = rc->n_chunks;
  out->chunks_per_pass = rc->dtype == SSN_F32 ? rc->chunks_per_pass() : rc->n_chunks;
  out->scratch_bytes = rc->scratch_bytes;
  out->min_scratch_bytes = rc->dtype == SSN_F32 ? rc->partial_bytes() : 0;
  ssn::BufView w;
  out->dec_neuron_major = ssn::sim_buffer_view(rc->sim, rc->dec_buffer, &w) == SSN_OK ? w.transposed : rc->last_transposed;
  out->last_launches = rc->launches;
  out->last_kernel_ms = rc->kernel_ms;
  return SSN_OK;
}

}  // extern "C"
